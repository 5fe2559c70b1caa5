"""The CPU restatement of rt_rebuild_accel (tests/accel_build_checker.cpp) builds sound, well-formed, reproducible trees on every scene of the rebuild tests, and they
stay sound under the restated refit.  No GPU: this pins the algorithm the device builder is held to word for word (tests/test_gpu_accel_build.py)."""
import numpy as np
import pytest

import accel_build
import refit


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return accel_build.build(tmp_path_factory.mktemp("accel_build"))


@pytest.fixture(scope="module")
def trees(lib):
    """name -> (scene, desc, host tree, restated device tree), built once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            sc, desc, host, _, _ = accel_build.host_tree(lib, name)
            cache[name] = (sc, desc, host, accel_build.rebuilt(lib, desc, host))
        return cache[name]
    return get


@pytest.mark.parametrize("name", accel_build.SCENES)
def test_restated_tree_is_sound_and_well_formed(lib, trees, name):
    _, desc, host, t = trees(name)
    assert t is not None
    assert t.moved.all()                                   # every record is held to its padded full box
    assert t.check() == (0, "")
    assert accel_build.structure(lib, t) == (0, "")
    assert t.depth <= accel_build.STACK_MAX and t.num_recs == host.ref.shape[0]
    # the pad is a fresh build's for the same scene
    fresh = refit.Tree.built(lib, desc)
    assert np.float32(t.tri_pad) == np.float32(fresh.tri_pad) == np.float32(t.tree_pad)
    # the records are the host build's, by globalId
    a, b = t.records(), fresh.records()
    by_id = np.zeros(t.num_recs, np.int64)
    by_id[b["globalId"]] = np.arange(len(b))               # (any reference of a split triangle: they carry the same words)
    for field in ("v0", "e1", "e2", "flags", "alphaIdx", "omm"):
        assert np.array_equal(a[field].view(np.uint32), b[field][by_id[a["globalId"]]].view(np.uint32)), field


@pytest.mark.parametrize("name", accel_build.SCENES)
def test_two_runs_give_the_same_words(lib, trees, name):
    _, desc, host, t = trees(name)
    u = accel_build.rebuilt(lib, desc, host)
    assert np.array_equal(t.nodes, u.nodes) and np.array_equal(t.recs, u.recs) and t.depth == u.depth


def test_shapes_of_the_tiny_trees(lib, trees):
    shape = {name: (trees(name)[3].num_nodes, trees(name)[3].depth) for name in accel_build.TINY}
    assert shape["one"] == (1, 1) and shape["two"] == (1, 1) and shape["four"] == (1, 1)
    assert shape["row25"][0] > 1 and shape["row25"][1] > 1 and shape["grid"][0] > 1 and shape["same30"][0] > 1
    four = trees("four")[3].nodes.reshape(-1, refit.NODE)[0, 24:32]
    assert (four != 0).sum() >= 2                          # more than one leaf slot
    # equal keys: the sorted order is globalId's, and a leaf slot is a run of consecutive sorted positions — so the records of every leaf slot are consecutive ascending
    # globalIds, and the slots of the whole tree partition 0..29 into such runs
    t = trees("same30")[3]
    gid, nodes, runs = t.records()["globalId"], t.nodes.reshape(-1, refit.NODE), []
    for n in nodes:
        tri_base = int(n[20:24].copy().view("<u4")[0])
        for s in range(8):
            m = int(n[24 + s])
            if m and not (int(n[15]) >> s) & 1:
                run = gid[tri_base + (m & 31):tri_base + (m & 31) + bin(m >> 5).count("1")].tolist()
                assert run == list(range(run[0], run[0] + len(run))), run
                runs.append(run)
    assert sorted(g for run in runs for g in run) == list(range(30)) and len(runs) >= 10


@pytest.mark.parametrize("name", accel_build.SCENES)
def test_refit_after_a_rebuild_keeps_the_tree_sound(lib, trees, name):
    sc, desc, host, t0 = trees(name)
    t = refit.Tree(lib, desc, t0.nodes, t0.recs, t0.inst, t0.tree_pad)
    t.moved[:] = 1
    ext = refit.scene_extent(t)
    home = refit.instances_of(desc)["objectToWorld"]
    ids = [0] if desc.numInstances == 1 else [min(3, desc.numInstances - 1), desc.numInstances - 1]
    cur = home.copy()
    for kind in refit.MOVES:
        inst = refit.instances_of(desc)
        inst["objectToWorld"] = cur
        desc2 = type(desc).from_buffer_copy(desc)
        desc2.instances = inst.ctypes.data
        xf = np.stack([refit.move_matrix(kind, desc2, i, ext, home) for i in ids])
        assert t.refit(ids, xf) == 0, kind
        cur[ids] = xf
        assert t.check() == (0, ""), kind
        assert accel_build.structure(lib, t, t0.depth) == (0, ""), kind
        assert int(t.stats[2]) == t0.depth


def test_a_tree_deeper_than_the_limit_is_refused(lib, trees):
    _, desc, host, t = trees("street")
    assert t.depth > 2
    assert accel_build.rebuilt(lib, desc, host, max_levels=t.depth - 1) is None
    assert accel_build.rebuilt(lib, desc, host, max_levels=t.depth) is not None
    assert accel_build.structure(lib, t, stack_max=t.depth - 1)[0] == 1

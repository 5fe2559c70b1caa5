"""rt_update_instances without a GPU: the CPU restatement of the refit (tests/refit_checker.cpp) on trees the builder itself made.  After every class of move the
refitted tree is sound (check_tree) and every leaf record equals, word for word, the record a fresh build of the moved scene produces; updates that move nothing
change nothing; check_tree reports one-word corruptions.  tests/test_gpu_refit.py holds the HIP kernels to this restatement word for word."""
import ctypes as C
import re
import os
import numpy as np
import pytest

from helpers import ROOT, abi
import refit

NAMES = ("rt_update_instances", "rt_update_lights", "rt_get_refit_stats", "rt_accel_readback")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refit.build(tmp_path_factory.mktemp("refit"))


@pytest.fixture(scope="module", params=["cornell", "street"])
def scene(request):
    return request.param, (refit.cornell() if request.param == "cornell" else refit.street())


def moved_ids(name, desc):
    """the instances the tests move: in the street scene one of each kind (shared prim mesh, emissive, alpha-tested, mirrored)"""
    if name == "cornell":
        return [3, 5]          # the short box and the light
    d = refit.describe(desc)
    return sorted({int(d[k][0]) for k in ("shared", "emissive", "alpha", "mirrored")})


def fresh_records(lib, sc):
    t = refit.Tree.built(lib, sc.desc())
    r = t.records()
    by_id = {}
    for k in np.argsort(r["globalId"], kind="stable"):
        by_id.setdefault(int(r["globalId"][k]), r[k])
    return t, by_id


def test_header_and_python_mirror():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert "RT_ACCEL_NODES = 0, RT_ACCEL_TRIS = 1, RT_ACCEL_INSTANCES = 2" in src
    assert 'static_assert(sizeof(rt_refit_stats) == 32, "rt_refit_stats");' in src
    assert C.sizeof(abi.RefitStats) == 32
    from restir_amd import renderer
    assert set(NAMES) <= set(renderer.ABI_SYMBOLS)
    for m in ("update_instances", "update_lights", "refit_stats", "accel_readback"):
        assert hasattr(renderer.Renderer, m)


def test_street_scene_has_what_the_tests_need(lib):
    sc = refit.street()
    desc = sc.desc()
    t = refit.Tree.built(lib, desc)
    d = refit.describe(desc)
    for k in ("shared", "emissive", "alpha", "mirrored"):
        assert len(d[k]) >= 1, k
    assert len(d["shared"]) >= 2
    assert 1000 < t.triangles < 10000
    assert t.num_recs > t.triangles and t.splits > 0      # the default build took spatial splits
    assert len(t.levels()[0]) >= 4 and t.depth >= 4
    assert t.check() == (0, "")


def test_moves_keep_the_tree_sound_and_the_records_equal_a_fresh_build(lib, scene):
    name, sc = scene
    sc = refit.cornell() if name == "cornell" else refit.street()    # (moved below: a scene of its own)
    desc = sc.desc()
    t = refit.Tree.built(lib, desc)
    ext = refit.scene_extent(t)
    ids = moved_ids(name, desc)
    home = refit.instances_of(desc)["objectToWorld"]
    base_pad = t.tri_pad
    seen_full = seen_shrink = False
    for kind in refit.MOVES:
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        pad_before = t.tri_pad
        assert t.refit(ids, xf) == 0
        sc.updateInstances(ids, xf)
        bad, msg = t.check()
        assert bad == 0, (kind, msg)
        assert t.stats[0] > 0 and t.stats[1] > 0
        seen_full |= bool(t.stats[3])
        seen_shrink |= t.tri_pad < pad_before
        assert t.tree_pad >= t.tri_pad
        if kind == "far":
            assert t.stats[3] == 1 and t.tri_pad > base_pad and t.stats[1] == t.num_nodes
        # against a fresh build of the moved scene: the pad, every record by globalId, the instance rows
        f, by_id = fresh_records(lib, sc)
        assert np.float32(f.tri_pad).tobytes() == np.float32(t.tri_pad).tobytes(), kind
        assert f.inst.tobytes() == t.inst.tobytes(), kind
        r = t.records()
        want = np.array([by_id[int(g)] for g in r["globalId"]], dtype=refit.REC_DT)
        for field in ("v0", "e1", "e2", "flags"):
            assert np.array_equal(r[field].view(np.uint32), want[field].view(np.uint32)), (kind, field)
        if kind == "mirror":
            flipped = np.isin(t.ref[r["globalId"], 0], ids)
            assert (r["flags"][flipped] & refit.TRI_FLIP).any()
    assert seen_full and seen_shrink


def test_empty_and_identity_updates(lib, scene):
    name, sc = scene
    desc = sc.desc()
    t = refit.Tree.built(lib, desc)
    nodes0, recs0, inst0 = t.nodes.copy(), t.recs.copy(), t.inst.copy()
    assert t.refit([], np.zeros((0, 12), np.float32)) == 0
    assert t.nodes.tobytes() == nodes0.tobytes() and t.recs.tobytes() == recs0.tobytes() and t.inst.tobytes() == inst0.tobytes()
    assert list(t.stats[:2]) == [0, 0]
    # identity update of ALL instances: the records keep their bytes, the tree stays sound
    inst = refit.instances_of(desc)
    assert t.refit(np.arange(len(inst)), inst["objectToWorld"]) == 0
    assert t.recs.tobytes() == recs0.tobytes() and t.inst.tobytes() == inst0.tobytes()
    assert t.check()[0] == 0
    # one instance: only the ancestor chains of its leaf records may change
    t2 = refit.Tree.built(lib, desc)
    i = moved_ids(name, desc)[0]
    assert t2.refit([i], inst["objectToWorld"][i:i + 1]) == 0
    _, parent = t2.levels()
    chain = np.zeros(t2.num_nodes, bool)
    for n in np.unique(t2.rec_node()[t2.ref[t2.records()["globalId"], 0] == i]):
        while n >= 0 and not chain[n]:
            chain[n] = True
            n = parent[n]
    a, b = t2.nodes.reshape(-1, refit.NODE), nodes0.reshape(-1, refit.NODE)
    assert (a[~chain] == b[~chain]).all()
    assert (~chain).any() and t2.stats[1] == chain.sum()
    assert t2.check()[0] == 0


def test_refused_calls_change_nothing(lib):
    sc = refit.cornell()   # (the description points into the scene: keep it alive)
    desc = sc.desc()
    t = refit.Tree.built(lib, desc)
    before = (t.nodes.tobytes(), t.recs.tobytes(), t.inst.tobytes())
    ok = refit.instances_of(desc)["objectToWorld"][1]
    nan = ok.copy(); nan[5] = np.nan
    singular = ok.copy(); singular[0:3] = 0
    for ids, xf in (([99], [ok]), ([1, 1], [ok, ok]), ([1], [nan]), ([1], [singular])):
        assert t.refit(ids, np.stack(xf)) == -1
        assert (t.nodes.tobytes(), t.recs.tobytes(), t.inst.tobytes()) == before


def test_check_tree_reports_one_word_corruptions(lib):
    sc = refit.street()
    desc = sc.desc()
    t = refit.Tree.built(lib, desc)
    assert t.check()[0] == 0
    r = t.records()
    single = np.bincount(r["globalId"], minlength=t.triangles)[r["globalId"]] == 1
    n = t.nodes.reshape(-1, refit.NODE)
    # a leaf slot whose triangles all have one reference: the builder's box of it is the union of their padded boxes, covered with the smallest bytes
    node = slot = rec = None
    for k in range(t.num_nodes):
        base = int(n[k, 20:24].copy().view("<u4")[0])
        for s in range(8):
            m = int(n[k, 24 + s])
            if m and not (int(n[k, 15]) >> s) & 1 and single[base + (m & 31):base + (m & 31) + bin(m >> 5).count("1")].all():
                node, slot, rec = k, s, base + (m & 31)
                break
        if node is not None:
            break
    assert node is not None
    saved = t.nodes.copy()
    # (a) a qhi lowered by one, on every axis
    for axis in range(3):
        t.nodes[:] = saved
        n[node, 56 + 8 * axis + slot] -= 1
        assert t.check()[0] > 0, axis
    t.nodes[:] = saved
    # (b) a v0 moved beyond the pad
    saved_r = t.recs.copy()
    r["v0"][rec, 0] -= np.float32(1000 * t.tri_pad + 1.0)
    assert t.check()[0] > 0
    t.recs[:] = saved_r
    # (c) a triBase off by one: a record is reached twice / never
    n[node, 20:24] = (n[node, 20:24].copy().view("<u4") + 1).view(np.uint8)
    assert t.check()[0] > 0
    t.nodes[:] = saved
    assert t.check()[0] == 0

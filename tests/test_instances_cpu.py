"""rt_set_instances without a GPU: the sequential restatement of the expansion (tests/instances_checker.cpp) gives, for every table of the GPU tests, the triRef and
the per-globalId flags of buildBvh8's flatten step for the same description; every refusal has its verdict; the checker runs clean under the sanitizers in a
program of its own.  Exact comparisons only."""
import os
import subprocess
import numpy as np
import pytest

from helpers import ROOT
import instances
import refit


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return instances.build(tmp_path_factory.mktemp("instances"))


@pytest.mark.parametrize("name", instances.TABLES)
def test_expansion_equals_the_builders_flatten(lib, name):
    sc, steps = instances.tables(name)
    desc = sc.desc()
    base = instances.mesh_alpha_base(lib, desc)
    tris_of = refit.prim_meshes_of(desc)["indexCount"] // 3
    assert list(base) == [int(tris_of[:m].sum()) for m in range(len(tris_of))]
    cur = refit.instances_of(desc)
    for label, table in steps:
        assert instances.verdict(lib, instances.desc_with(desc, cur), table) == (instances.OK, 0), label
        prefix, ref, rec = instances.expand(lib, desc, table)
        new = instances.desc_with(desc, table)
        bref, bflags = instances.flatten(lib, new)
        n = int(tris_of[table["primMesh"]].sum())
        assert len(ref) == len(bref) == n and int(prefix[-1]) == n, label
        assert np.array_equal(ref, bref) and np.array_equal(ref, refit.tri_ref(new)), label
        assert np.array_equal(rec[:, 0], np.arange(n, dtype=np.uint32)), label
        assert np.array_equal(rec[:, 1], bflags & ~np.uint32(instances.TRI_FLIP)), label
        # TRI_FLIP is k_refit_tris' to write, from bit 31 of the prefix words: the builder's handedness
        assert np.array_equal((prefix[ref[:, 0]] & instances.FLIP_BIT) != 0, (bflags & instances.TRI_FLIP) != 0), label
        det = np.array([np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for m in table["objectToWorld"]])
        assert np.array_equal((prefix[:-1] & instances.FLIP_BIT) != 0, det < 0), label
        assert np.array_equal(prefix & ~np.uint32(instances.FLIP_BIT), np.concatenate([[0], np.cumsum(tris_of[table["primMesh"]])]).astype(np.uint32)), label
        # alphaIdx: a function of (prim mesh, triangle) for a triangle that is alpha-tested, 0 for an opaque one
        opaque = (table["flags"][ref[:, 0]] & instances.FORCE_OPAQUE) != 0
        assert np.array_equal(rec[:, 2], np.where(opaque, 0, base[table["primMesh"][ref[:, 0]]] + ref[:, 1] + 1).astype(np.uint32)), label
        cur = table


def test_the_tables_exercise_what_they_are_for(lib):
    """mirrored, non-opaque and opaque instances of one mesh, instances without triangles: present in the tables, or the tests above show nothing"""
    sc, steps = instances.tables("cornell")
    dets = [np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for m in steps[0][1]["objectToWorld"]]
    assert min(dets) < 0 and len(steps[1][1]) == len(steps[0][1]) - 1
    sc, steps = instances.tables("street")
    t = steps[-1][1]
    leaf = t["primMesh"][(t["flags"] & instances.FORCE_OPAQUE) == 0][0]
    assert sorted(set((t["flags"][t["primMesh"] == leaf] & instances.FORCE_OPAQUE).tolist())) == [0, 1]
    sc, steps = instances.tables("street_lazy")
    leafs = [set(t["primMesh"][(t["flags"] & instances.FORCE_OPAQUE) == 0].tolist()) for _, t in steps]
    assert len(leafs[0]) == 2 and len(leafs[1]) == 1 and len(leafs[2]) == 1 and leafs[3] == leafs[0]
    sc, steps = instances.tables("empty_mesh")
    prefix, _, _ = instances.expand(lib, sc.desc(), steps[0][1])
    assert (np.diff(prefix & ~np.uint32(instances.FLIP_BIT)) == 0).sum() == 4


@pytest.mark.parametrize("name", instances.REFUSALS)
def test_every_refusal_has_its_verdict(lib, name):
    sc, cases = instances.refusals(name)
    desc = sc.desc()
    assert instances.verdict(lib, desc, refit.instances_of(desc)) == (instances.OK, 0)      # the table the scene has is accepted
    for label, table, code, offender in cases:
        got = instances.verdict(lib, desc, table)
        assert got[0] == code, (label, got)
        if code in instances.PER_INSTANCE:
            assert got[1] == offender, (label, got)
    if name == "cornell":
        assert sorted({c for _, _, c, _ in cases}) == [instances.NULL, instances.NO_INSTANCES, instances.PRIM_MESH, instances.NON_FINITE, instances.SINGULAR,
                                                       instances.NO_INVERSE, instances.EMITTER_CHANGED, instances.EMITTER_ADDED]


def test_an_instance_a_binding_names_is_held_in_place(lib, tmp_path):
    import lights
    sc, desc, src, bound, box, moved = instances.bound_box_scene(lights.build(tmp_path))
    assert box in bound and box not in refit.describe(desc)["emissive"]
    assert instances.verdict(lib, desc, moved) == (instances.OK, 0)                                   # without a binding the box may move
    assert instances.verdict(lib, desc, moved, bound=bound) == (instances.EMITTER_CHANGED, box)
    assert instances.verdict(lib, desc, np.delete(moved, box), bound=bound) == (instances.EMITTER_CHANGED, box)
    assert instances.verdict(lib, desc, refit.instances_of(desc), bound=bound) == (instances.OK, 0)


@pytest.mark.parametrize("name", instances.TABLES)
def test_the_ray_seeds_are_informative(name):
    """the counts tests/test_gpu_instances.py asserts on the GPU's hits hold for the chosen seeds: the oracle's ray code traces the same rays on the CPU"""
    from oracle.binding import Oracle
    import test_gpu_refit as seq
    sc, steps = instances.tables(name)
    desc0 = sc.desc()
    cur = refit.instances_of(desc0)
    for label, table in steps:
        desc = instances.desc_with(desc0, table)
        ids, added = instances.aim_ids(cur, table)
        o = Oracle(0)
        o.upload_scene(desc)
        leaves = instances.alpha_added(cur, table)
        hits, aimed, alpha = instances.informative(desc, o.trace_closest(seq.make_rays(desc, ids, instances.RAYS, instances.RAY_SEED[name])), ids, leaves)
        assert hits > 400 and aimed > 20, (label, hits, aimed)
        if name == "street" and leaves:
            assert alpha >= 20, (label, alpha)
        cur = table


def test_checker_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "instances_san")
    srcs = [os.path.join(ROOT, "tests", "instances_san_main.cpp"), instances.SRC, refit.BUILDER]
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-w", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + srcs + ["-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout

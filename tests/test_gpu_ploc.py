"""The PLOC builder of the device rebuild on the GPU (rt_set_rebuild_options): the device tree equals the CPU restatement (tests/ploc_checker.cpp) word
for word at every radius, rays and frames on it equal those of a host-built tree / of the oracle bit for bit, rt_update_instances and rt_set_instances work on and
under it, switching builders changes nothing but the tree, refused options and a refused build change nothing.  No tolerance anywhere: results are a function of the
triangle set, never of the tree.  Scenes, rays and the 8-frame Cornell sequence are those of tests/test_gpu_refit.py and tests/test_gpu_accel_build.py."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
import accel_build
import instances
import optin
import ploc
import refit
import test_gpu_accel_build as tab
import test_gpu_instances as tgi
import test_gpu_refit as seq

pytestmark = pytest.mark.gpu

SAME = {"nodes": 0, "records": 0, "instances": 0}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ploc.build(tmp_path_factory.mktemp("ploc_gpu"))


def options(r):
    o = r.rebuild_options()
    return [o.builder, o.radius, o.maxIterations, o.reserved]


def moved_context(lib, name):
    """(renderer that holds the host-built tree of the moved scene, description of the moved scene, that tree as a refit.Tree for the checker)"""
    sc, ids, xf = ploc.make(name)
    desc = sc.desc()
    host = refit.Tree.built(lib, desc)
    r = seq.renderer(desc)
    if len(ids):
        assert host.refit(ids, xf) == 0
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
        desc = sc.desc()
    return sc, r, desc, tab.host_tree_of(lib, r, desc, host)


def check_against(r, t, desc, label):
    st, acc = r.rebuild_stats(), r.accel_stats()
    diff = tab.words(r, t, desc.numInstances)
    print(label, diff, "nodes", st.nodes, "levels", st.levels, "iterations", st.iterations, "ms", round(st.ms, 3))
    assert diff == SAME, label
    assert [st.triangles, st.nodes, st.levels, st.maxDepth, st.iterations] == [t.num_recs, t.num_nodes, t.depth, t.depth, getattr(t, "iterations", 0)], label
    assert np.float32(st.triPad) == np.float32(t.tri_pad), label
    assert [acc["nodes"], acc["triangles"], acc["references"], acc["max_depth"], acc["spatial_splits"]] == [t.num_nodes, t.num_recs, t.num_recs, t.depth, 0], label


# ---- 1. word-for-word agreement with the checker ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 0, 64])      # 0: the default radius
@pytest.mark.parametrize("name", ploc.SCENES)
def test_device_tree_equals_the_checker_word_for_word(lib, name, radius):
    _, r, desc, host = moved_context(lib, name)
    in_force = radius or ploc.DEFAULT_RADIUS
    t = ploc.rebuilt(lib, desc, host, radius=in_force)
    assert not isinstance(t, int), t
    r.set_rebuild_options(abi.REBUILD_PLOC, radius)
    assert options(r) == [abi.REBUILD_PLOC, in_force, ploc.DEFAULT_MAX_ITERATIONS, 0]
    for run in range(2):
        r.rebuild_accel()
        check_against(r, t, desc, (name, radius, run))
        assert options(r) == [abi.REBUILD_PLOC, in_force, ploc.DEFAULT_MAX_ITERATIONS, 0]
    r.destroy()


# ---- 2. rays: the PLOC-built context against a fresh context that uploaded and host-built the same moved scene -----------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street"])
def test_rays_equal_a_host_build(name):
    sc = seq.make(name)
    desc = sc.desc()
    r = seq.renderer(desc)
    r.set_rebuild_options(abi.REBUILD_PLOC)
    ids = seq.moved_ids(name, desc)
    home = refit.instances_of(desc)["objectToWorld"]
    ext = max(np.abs(refit.world_bounds(desc, i)).max() for i in range(desc.numInstances))
    for kind in ("rotate", "mirror", "far", "back", "scale"):
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
    r.rebuild_accel()
    assert r.rebuild_stats().iterations > 0
    desc = sc.desc()
    fresh = seq.renderer(desc)
    rays = seq.make_rays(desc, ids, 4096, 11)
    a = tgi.same_rays(r, fresh, rays)
    hit = a.view(np.uint32)[:, 1] != 0xffffffff
    moved_hits = np.isin(refit.tri_ref(desc)[a.view(np.uint32)[:, 1][hit], 0], ids).sum()
    print(name, "rays that hit:", int(hit.sum()), "of them on moved instances:", int(moved_hits))
    assert hit.sum() > 400 and moved_hits > 20
    r.destroy(); fresh.destroy()


# ---- 3. frames: the Cornell sequence with a PLOC rebuild before every frame, or a rebuild on even and a refit on odd frames -----------------------------------
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 2])
@pytest.mark.parametrize("alternate", [False, True])
def test_frames_equal_the_oracle(overlap, traversal, alternate):
    W, H = seq.SIZES[1]
    want = seq.Sequence.oracle_frames(W, H)
    s = seq.Sequence(W, H)
    r = seq.renderer(s.sc.desc(), W, H, overlap, traversal)
    r.set_rebuild_options(abi.REBUILD_PLOC)
    bad = {}
    for f in range(seq.FRAMES):
        ids, xf, desc, cam = s.step(f)
        r.update_instances(ids, xf)
        if not alternate or f % 2 == 0:
            r.rebuild_accel()
            assert r.rebuild_stats().iterations > 0
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
        for b in frame_buffers(f):
            d = optin.words(r.readback(b), want[f][b])
            if d:
                bad[(f, abi.BUFFER_NAMES[b])] = d
    r.destroy()
    assert bad == {}


# ---- 4. rt_update_instances on the PLOC tree ------------------------------------------------------------------------------------------------------------------
def test_update_after_a_ploc_rebuild_equals_the_checker(lib):
    sc = seq.make("street")
    desc = sc.desc()
    r = seq.renderer(desc)
    t = ploc.rebuilt(lib, desc, tab.host_tree_of(lib, r, desc, refit.Tree.built(lib, desc)))
    r.set_rebuild_options(abi.REBUILD_PLOC)
    r.rebuild_accel()
    levels = r.rebuild_stats().levels
    assert tab.words(r, t, desc.numInstances) == SAME
    ids = seq.moved_ids("street", desc)
    home = refit.instances_of(desc)["objectToWorld"]
    ext = refit.scene_extent(t)
    for kind in refit.MOVES:
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        assert t.refit(ids, xf) == 0
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
        st = r.refit_stats()
        assert tab.words(r, t, desc.numInstances) == SAME, kind
        assert t.check() == (0, ""), kind
        assert [st.instances, st.leafRecords, st.nodes, st.levels, st.fullRefit] == [len(ids)] + [int(x) for x in t.stats], kind
        assert st.levels == levels
    r.destroy()


# ---- 5. rt_set_instances under PLOC ---------------------------------------------------------------------------------------------------------------------------
def test_set_instances_builds_with_ploc(lib):
    sc, steps = instances.tables("street")
    desc0 = sc.desc()
    label, table = steps[0]
    desc = instances.desc_with(desc0, table)
    r = seq.renderer(desc0)
    r.set_rebuild_options(abi.REBUILD_PLOC, 8)
    r.set_instances(table)
    assert r.instances_stats().reallocated == 1
    fresh = seq.renderer(desc)
    t = ploc.rebuilt(lib, desc, tab.host_tree_of(lib, fresh, desc, refit.Tree.built(lib, desc)), radius=8)
    assert tgi.diff_tree(r, t, len(table)) == SAME, label
    rs = r.rebuild_stats()
    assert [rs.triangles, rs.nodes, rs.levels, rs.iterations] == [t.num_recs, t.num_nodes, t.depth, t.iterations] and t.iterations > 0
    r.set_instances(table)      # again: the same tree, nothing allocated
    assert tgi.diff_tree(r, t, len(table)) == SAME and r.instances_stats().reallocated == 0
    ids, _ = instances.aim_ids(refit.instances_of(desc0), table)
    tgi.same_rays(r, fresh, seq.make_rays(desc, ids, instances.RAYS, instances.RAY_SEED["street"]))
    r.destroy(); fresh.destroy()


# ---- 6. switching -----------------------------------------------------------------------------------------------------------------------------------------------
def test_switching_builders_on_one_context(lib):
    _, r, desc, host = moved_context(lib, "street")
    lb, pl = ploc.rebuilt(lib, desc, host, builder=ploc.LBVH), ploc.rebuilt(lib, desc, host)
    assert options(r) == [abi.REBUILD_LBVH, ploc.DEFAULT_RADIUS, ploc.DEFAULT_MAX_ITERATIONS, 0]      # the defaults
    seen = []
    for builder, t in ((abi.REBUILD_LBVH, lb), (abi.REBUILD_PLOC, pl), (abi.REBUILD_LBVH, lb), (abi.REBUILD_PLOC, pl)):
        r.set_rebuild_options(builder)
        r.rebuild_accel()
        check_against(r, t, desc, builder)
        seen.append([r.accel_readback(w, desc.numInstances).copy() for w in range(3)])
    assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[2])) and all(np.array_equal(a, b) for a, b in zip(seen[1], seen[3]))
    assert not np.array_equal(seen[0][0], seen[1][0])      # (the two builders do give different trees here)
    # the options survive a host build; rt_set_instances tells what it allocates: the first table the working buffers, the first PLOC build on them PLOC's, then —
    # LBVH, PLOC again — nothing: switching back freed nothing that the later PLOC build had to allocate again
    assert refit.hip_build_accel(r) == 0
    assert options(r) == [abi.REBUILD_PLOC, ploc.DEFAULT_RADIUS, ploc.DEFAULT_MAX_ITERATIONS, 0]
    table = refit.instances_of(desc)
    realloc = []
    for builder in (abi.REBUILD_LBVH, abi.REBUILD_PLOC, abi.REBUILD_LBVH, abi.REBUILD_PLOC, abi.REBUILD_PLOC):
        r.set_rebuild_options(builder)
        r.set_instances(table)
        realloc.append(r.instances_stats().reallocated)
        assert (r.rebuild_stats().iterations > 0) == (builder == abi.REBUILD_PLOC)
    assert realloc == [1, 1, 0, 0, 0]
    r.destroy()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_options_change_nothing():
    from restir_amd.renderer import Renderer, hip_lib
    r = Renderer().setup(0)      # valid right after rt_create
    r.set_rebuild_options(abi.REBUILD_PLOC, 24, 100)
    want = [abi.REBUILD_PLOC, 24, 100, 0]
    assert options(r) == want
    for bad in ((2, 0, 0, 0), (-1, 0, 0, 0), (abi.REBUILD_PLOC, 65, 0, 0), (abi.REBUILD_PLOC, -1, 0, 0), (abi.REBUILD_PLOC, 16, -1, 0), (abi.REBUILD_LBVH, 0, 0, 1)):
        o = abi.RebuildOptions(*bad)
        assert hip_lib().rt_set_rebuild_options(r._h, C.byref(o)) == abi.ERR_INVALID_ARG, bad
        assert b"rt_set_rebuild_options" in hip_lib().rt_last_error(r._h), bad
        assert options(r) == want, bad
    assert hip_lib().rt_set_rebuild_options(r._h, None) == abi.ERR_INVALID_ARG and hip_lib().rt_get_rebuild_options(r._h, None) == abi.ERR_INVALID_ARG
    # ... and they survive a scene upload with its host build, and a resize
    sc = refit.cornell()
    r.load_scene(sc.desc())
    r.update(32, 24)
    assert options(r) == want
    r.destroy()


def test_a_build_over_the_iteration_cap_is_refused_and_the_tree_stays(lib):
    from restir_amd.renderer import hip_lib
    _, r, desc, host = moved_context(lib, "nested40")
    t = ploc.rebuilt(lib, desc, host, radius=1)
    assert t.iterations == 39
    assert ploc.rebuilt(lib, desc, host, radius=1, max_iterations=2) == ploc.REFUSED_ITERATIONS
    before = [r.accel_readback(w, desc.numInstances).copy() for w in range(3)]
    r.set_rebuild_options(abi.REBUILD_PLOC, 1, 2)
    assert hip_lib().rt_rebuild_accel(r._h) == abi.ERR_INVALID_ARG
    assert b"PLOC did not reach one cluster within maxIterations" in hip_lib().rt_last_error(r._h)
    assert all(np.array_equal(a, r.accel_readback(w, desc.numInstances)) for w, a in enumerate(before))
    fresh = seq.renderer(desc)
    tgi.same_rays(r, fresh, seq.make_rays(desc, [0], 1024, 3))
    # exactly enough iterations are not refused
    r.set_rebuild_options(abi.REBUILD_PLOC, 1, 39)
    r.rebuild_accel()
    check_against(r, t, desc, "nested40 at the cap")
    tgi.same_rays(r, fresh, seq.make_rays(desc, [0], 1024, 3))
    r.destroy(); fresh.destroy()


def test_set_instances_over_the_iteration_cap_is_refused_and_the_tree_stays(lib):
    """The same refusal through rt_set_instances, which shares the build with rt_rebuild_accel but has buffers of its own to put back: as the first call on a context
    (the buffers it allocated for the table go again), and after a table that succeeded under LBVH (the table fits: the shared working buffers describe the context's
    table again).  Either way the context is as before the call, and a rebuild with exactly enough iterations gives the checker's tree."""
    from restir_amd.renderer import hip_lib
    for branch in ("fresh pool", "put back"):
        _, r, desc, host = moved_context(lib, "nested40")
        t = ploc.rebuilt(lib, desc, host, radius=1)
        assert t.iterations == 39
        table = refit.instances_of(desc)
        rows = np.ascontiguousarray(table).view(np.uint8).reshape(-1)
        if branch == "put back":
            r.set_instances(table)
            assert r.instances_stats().reallocated == 1 and r.rebuild_stats().iterations == 0
        before = [r.accel_readback(w, desc.numInstances).copy() for w in range(3)]
        r.set_rebuild_options(abi.REBUILD_PLOC, 1, 2)
        assert hip_lib().rt_set_instances(r._h, len(table), rows.ctypes.data) == abi.ERR_INVALID_ARG, branch
        assert b"PLOC did not reach one cluster within maxIterations" in hip_lib().rt_last_error(r._h), branch
        assert all(np.array_equal(a, r.accel_readback(w, desc.numInstances)) for w, a in enumerate(before)), branch
        fresh = seq.renderer(desc)
        tgi.same_rays(r, fresh, seq.make_rays(desc, [0], 1024, 3))
        r.set_rebuild_options(abi.REBUILD_PLOC, 1, 39)
        r.rebuild_accel()
        check_against(r, t, desc, "nested40 at the cap, after the refused table: " + branch)
        tgi.same_rays(r, fresh, seq.make_rays(desc, [0], 1024, 3))
        r.destroy(); fresh.destroy()

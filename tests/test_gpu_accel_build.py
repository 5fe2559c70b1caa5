"""rt_rebuild_accel on the GPU: the device-built tree equals the CPU restatement (tests/accel_build_checker.cpp) word for word, rays and frames on it equal those of a
host-built tree / of the oracle bit for bit, rt_update_instances works on it, the opt-in passes keep their histories across it.  No tolerance anywhere: results are a
function of the triangle set, never of the tree.  The scenes, the ray generator and the 8-frame Cornell sequence are those of tests/test_gpu_refit.py."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
import accel_build
import optin
import refit
import test_gpu_refit as seq

pytestmark = pytest.mark.gpu

FRAMES = seq.FRAMES
SIZES = seq.SIZES


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return accel_build.build(tmp_path_factory.mktemp("accel_build"))


def host_tree_of(lib, r, desc, cpu_host):
    """the context's host-built tree as a refit.Tree: the leaf records are read back, because alphaIdx and the opacity micro-maps are made by rt_build_accel and not by
    the builder the checker links; the instance rows are the CPU's (builder + restated refit), so the comparison of the rows stays one of device against CPU"""
    return refit.Tree(lib, desc, r.accel_readback(abi.ACCEL_NODES), r.accel_readback(abi.ACCEL_TRIS), cpu_host.inst, 0.0)


def words(r, t, n_inst):
    return {"nodes": optin.words(r.accel_readback(abi.ACCEL_NODES), t.nodes), "records": optin.words(r.accel_readback(abi.ACCEL_TRIS), t.recs),
            "instances": optin.words(r.accel_readback(abi.ACCEL_INSTANCES, n_inst), t.inst)}


# ---- word-for-word agreement with the checker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", accel_build.SCENES)
def test_device_tree_equals_the_checker_word_for_word(lib, name):
    sc, ids, xf = accel_build.make(name)
    desc = sc.desc()
    host = refit.Tree.built(lib, desc)
    r = seq.renderer(desc)
    if len(ids):
        assert host.refit(ids, xf) == 0
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
        desc = sc.desc()
    t = accel_build.rebuilt(lib, desc, host_tree_of(lib, r, desc, host))
    for run in range(2):
        r.rebuild_accel()
        st, acc = r.rebuild_stats(), r.accel_stats()
        diff = words(r, t, desc.numInstances)
        print(name, run, diff, "nodes", st.nodes, "levels", st.levels, "ms", round(st.ms, 3), "sort", round(st.sortMs, 3))
        assert diff == {"nodes": 0, "records": 0, "instances": 0}
        assert [st.triangles, st.nodes, st.levels, st.maxDepth] == [t.num_recs, t.num_nodes, t.depth, t.depth]
        assert np.float32(st.triPad) == np.float32(t.tri_pad)
        assert [acc["nodes"], acc["triangles"], acc["references"], acc["max_depth"], acc["spatial_splits"]] == [t.num_nodes, t.num_recs, t.num_recs, t.depth, 0]
    r.destroy()


# ---- rays: the device-built context against a fresh context that uploaded and host-built the same moved scene ------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street"])
def test_rays_equal_a_host_build(name):
    sc = seq.make(name)
    desc = sc.desc()
    r = seq.renderer(desc)
    ids = seq.moved_ids(name, desc)
    home = refit.instances_of(desc)["objectToWorld"]
    ext = max(np.abs(refit.world_bounds(desc, i)).max() for i in range(desc.numInstances))
    for kind in ("rotate", "mirror", "far", "back", "scale"):
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
    r.rebuild_accel()
    desc = sc.desc()
    fresh = seq.renderer(desc)
    rays = seq.make_rays(desc, ids, 4096, 11)
    for mode in (abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY):
        r.set_traversal(mode); fresh.set_traversal(mode)
        a, b = r.trace_closest(rays), fresh.trace_closest(rays)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
        assert np.array_equal(r.trace_any(rays), fresh.trace_any(rays)), mode
    hit = a.view(np.uint32)[:, 1] != 0xffffffff
    moved_hits = np.isin(refit.tri_ref(desc)[a.view(np.uint32)[:, 1][hit], 0], ids).sum()
    print(name, "rays that hit:", int(hit.sum()), "of them on moved instances:", int(moved_hits))
    assert hit.sum() > 400 and moved_hits > 20
    # the records by globalId against the host build's
    dev, built = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT), fresh.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    by_id = {int(g): k for k, g in enumerate(built["globalId"])}
    pick = np.array([by_id[int(g)] for g in dev["globalId"]])
    assert sorted(dev["globalId"].tolist()) == list(range(len(refit.tri_ref(desc))))
    for field in ("v0", "e1", "e2", "flags", "omm"):
        assert np.array_equal(dev[field].view(np.uint32), built[field][pick].view(np.uint32)), field
    r.destroy(); fresh.destroy()


# ---- frames: the Cornell sequence with a rebuild before every frame, or a rebuild on even and a refit on odd frames -----------------------------------------
def run_case(W, H, overlap, traversal, alternate, far=False, frames=FRAMES):
    want = seq.Sequence.oracle_frames(W, H, far, frames)
    s = seq.Sequence(W, H, far)
    r = seq.renderer(s.sc.desc(), W, H, overlap, traversal)
    bad, pads = {}, []
    for f in range(frames):
        ids, xf, desc, cam = s.step(f)
        r.update_instances(ids, xf)
        if not alternate or f % 2 == 0:
            r.rebuild_accel()
            pads.append(float(r.rebuild_stats().triPad))
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
        for b in frame_buffers(f):
            d = optin.words(r.readback(b), want[f][b])
            if d:
                bad[(f, abi.BUFFER_NAMES[b])] = d
    return r, s, bad, pads


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 2])
@pytest.mark.parametrize("alternate", [False, True])
def test_frames_equal_the_oracle(W, H, overlap, traversal, alternate):
    r, s, bad, _ = run_case(W, H, overlap, traversal, alternate)
    r.destroy()
    assert bad == {}


@pytest.mark.parametrize("alternate", [False, True])
def test_frames_with_a_pad_that_grows_and_shrinks_across_rebuilds(alternate):
    W, H = SIZES[0]
    r, s, bad, pads = run_case(W, H, 2, None, alternate, far=True)
    r.destroy()
    assert bad == {}
    if not alternate:       # the box leaves the room at frames 4-5
        assert pads[4] > pads[3] and pads[5] > pads[3] and pads[6] < pads[5]


# ---- rt_update_instances on the device-built tree ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street"])
def test_update_after_rebuild_equals_the_checker(lib, name):
    sc = seq.make(name)
    desc = sc.desc()
    host = refit.Tree.built(lib, desc)
    r = seq.renderer(desc)
    t = accel_build.rebuilt(lib, desc, host_tree_of(lib, r, desc, host))
    r.rebuild_accel()
    levels = r.rebuild_stats().levels
    assert words(r, t, desc.numInstances) == {"nodes": 0, "records": 0, "instances": 0}
    ids = seq.moved_ids(name, desc)
    home = refit.instances_of(desc)["objectToWorld"]
    ext = refit.scene_extent(t)
    for kind in refit.MOVES:
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        assert t.refit(ids, xf) == 0
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
        st = r.refit_stats()
        assert words(r, t, desc.numInstances) == {"nodes": 0, "records": 0, "instances": 0}, kind
        assert t.check() == (0, ""), kind
        assert [st.instances, st.leafRecords, st.nodes, st.levels, st.fullRefit] == [len(ids)] + [int(x) for x in t.stats], kind
        assert st.levels == levels
    r.destroy()


# ---- one case each with an opt-in pass on, a rebuild before every frame -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["svgf", "gi_spatial", "taa"])
def test_rebuilds_with_an_opt_in_pass(tmp_path, which):
    import gi_spatial
    W, H = SIZES[1]
    kw = {"svgf": dict(den=abi.Denoiser(mode=abi.DENOISER_SVGF)), "gi_spatial": dict(gis=abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY)), "taa": dict(t=abi.Taa(mode=abi.TAA_ON))}[which]
    rig = optin.Rig(tmp_path, abi.PROC_CORNELL, 1.0, None, W, H, overlap=2, **kw)
    home = refit.instances_of(rig.sc.desc())["objectToWorld"]
    for f in range(5):
        ids, xf = seq.plan(f, home)
        rig.sc.updateInstances(ids, xf)
        desc = rig.sc.desc()
        rig.r.update_instances(ids, xf)
        rig.r.rebuild_accel()
        rig.r.update_lights(desc)
        rig.o.upload_scene(desc)
        rig.kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp_path), desc)
        rig.desc = desc
        rig.frame(f)
        assert rig.diff(f) == {}, f
    n = rig.history_lengths()
    if which != "gi_spatial":
        assert set(n) == ({"svgf_direct", "svgf_indirect"} if which == "svgf" else {"taa"}), sorted(n)     # the pass ran and its history is what is measured
        assert all(v.max() >= 3 for v in n.values()), {k: v.max() for k, v in n.items()}     # the histories were carried across the rebuilds, not dropped
    rig.destroy()


# ---- state and refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_a_host_build():
    from restir_amd.renderer import Renderer, hip_lib
    sc = refit.cornell()
    desc = sc.desc()
    r0 = Renderer().setup(0)
    assert hip_lib().rt_rebuild_accel(r0._h) == abi.ERR_NO_SCENE
    assert hip_lib().rt_upload_scene(r0._h, C.byref(desc)) == 0
    assert hip_lib().rt_rebuild_accel(r0._h) == abi.ERR_NO_ACCEL
    r0.destroy()


def test_reference_sums_restart_priorities_stay_and_a_later_host_build_matches():
    W, H = SIZES[0]
    want = seq.Sequence.oracle_frames(W, H)
    s = seq.Sequence(W, H)
    r = seq.renderer(s.sc.desc(), W, H, 2)
    for f in range(4):      # past the probe frames: the context has decided
        ids, xf, desc, cam = s.step(f)
        r.update_instances(ids, xf)
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
    r.sync()
    before = r.stream_priorities()
    assert before["decided"]
    r.reference_render(s.st, 2)
    assert r.reference_samples() == 2
    r.rebuild_accel()
    assert r.reference_samples() == 0
    assert r.stream_priorities() == before
    for f in (4, 5):        # frame 4 on the device-built tree, frame 5 after a later host build of the moved scene
        ids, xf, desc, cam = s.step(f)
        r.update_instances(ids, xf)
        if f == 5:
            assert refit.hip_build_accel(r) == 0
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
        assert {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), want[f][b]) for b in frame_buffers(f) if optin.words(r.readback(b), want[f][b])} == {}, f
    r.destroy()

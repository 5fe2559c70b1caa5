"""rt_update_instances on the GPU: the refitted device tree equals the CPU restatement (tests/refit_checker.cpp) word for word, rays and frames equal those of a fresh
build / of the oracle rendering the moved scene bit for bit, refused calls change nothing.  No tolerance anywhere: results are a function of the triangle set, never of
the tree."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, host, frame_buffers
from oracle.binding import Oracle
import optin
import refit

pytestmark = pytest.mark.gpu

FRAMES = 8
SIZES = ((64, 48), (67, 45))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refit.build(tmp_path_factory.mktemp("refit"))


def renderer(desc, W=None, H=None, overlap=None, traversal=None):
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0)
    if overlap is not None:
        r.set_overlap(overlap)
    r.load_scene(desc)
    if W:
        r.update(W, H)
    if traversal is not None:
        r.set_traversal(traversal)
    return r


def device_tree(lib, r, desc):
    """the device tree as a refit.Tree (the checker then refits what the GPU refits); after an update, which tells the pad of the tree's boxes"""
    st = r.refit_stats()
    return refit.Tree(lib, desc, r.accel_readback(abi.ACCEL_NODES), r.accel_readback(abi.ACCEL_TRIS), r.accel_readback(abi.ACCEL_INSTANCES, desc.numInstances),
                      st.treePad)


def same_tree(r, t, desc):
    return {"nodes": optin.words(r.accel_readback(abi.ACCEL_NODES), t.nodes), "records": optin.words(r.accel_readback(abi.ACCEL_TRIS), t.recs),
            "instances": optin.words(r.accel_readback(abi.ACCEL_INSTANCES, desc.numInstances), t.inst)}


def moved_ids(name, desc):
    if name == "cornell":
        return [3, 5]
    d = refit.describe(desc)
    return sorted({int(d[k][0]) for k in ("shared", "emissive", "alpha", "mirrored")})


def make(name):
    return refit.cornell() if name == "cornell" else refit.street()


# ---- word-for-word agreement with the checker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street"])
def test_device_tree_equals_the_checker_word_for_word(lib, name):
    sc = make(name)
    desc = sc.desc()
    r = renderer(desc)
    ids = moved_ids(name, desc)
    home = refit.instances_of(desc)["objectToWorld"]
    # the first update moves nothing: it tells the build's pad, and must change no word
    before = [r.accel_readback(w, desc.numInstances) for w in range(3)]
    r.update_instances([], np.zeros((0, 12), np.float32))
    assert all(np.array_equal(a, r.accel_readback(w, desc.numInstances)) for w, a in enumerate(before))
    t = device_tree(lib, r, desc)
    assert t.check() == (0, "")
    ext = refit.scene_extent(t)
    fulls = 0
    for kind in refit.MOVES:
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        assert t.refit(ids, xf) == 0
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
        st = r.refit_stats()
        diff = same_tree(r, t, desc)
        print(name, kind, diff, "records", st.leafRecords, "nodes", st.nodes, "levels", st.levels, "full", st.fullRefit, "ms", round(st.ms, 3))
        assert diff == {"nodes": 0, "records": 0, "instances": 0}, kind
        assert t.check() == (0, ""), kind
        assert [st.instances, st.leafRecords, st.nodes, st.levels, st.fullRefit] == [len(ids)] + [int(x) for x in t.stats], kind
        assert np.float32(st.triPad) == np.float32(t.tri_pad) and np.float32(st.treePad) == np.float32(t.tree_pad)
        fulls += st.fullRefit
    assert fulls >= 1
    r.destroy()


# ---- rays: the updated context against a fresh context that uploaded and built the moved scene ----------------------------------------------------------------
make_rays = refit.make_rays      # (lives in tests/refit.py: the CPU tests aim the same rays without importing this module)


@pytest.mark.parametrize("name", ["cornell", "street"])
def test_rays_equal_a_fresh_build(name):
    sc = make(name)
    desc = sc.desc()
    r = renderer(desc)
    ids = moved_ids(name, desc)
    home = refit.instances_of(desc)["objectToWorld"]
    ext = max(np.abs(refit.world_bounds(desc, i)).max() for i in range(desc.numInstances))
    for kind in ("rotate", "mirror", "far", "back", "scale"):
        desc = sc.desc()
        xf = np.stack([refit.move_matrix(kind, desc, i, ext, home) for i in ids])
        r.update_instances(ids, xf)
        sc.updateInstances(ids, xf)
    desc = sc.desc()
    fresh = renderer(desc)
    rays = make_rays(desc, ids, 4096, 11)
    hits = 0
    for mode in (abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY):
        r.set_traversal(mode); fresh.set_traversal(mode)
        a, b = r.trace_closest(rays), fresh.trace_closest(rays)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
        assert np.array_equal(r.trace_any(rays), fresh.trace_any(rays)), mode
        hits = int((a.view(np.uint32)[:, 1] != 0xffffffff).sum())
    moved_hits = np.isin(refit.tri_ref(desc)[a.view(np.uint32)[:, 1][a.view(np.uint32)[:, 1] != 0xffffffff], 0], ids).sum()
    print(name, "rays that hit:", hits, "of them on moved instances:", int(moved_hits))
    assert hits > 400 and moved_hits > 20
    # ... and a later rebuild gives the records of the refitted tree (by globalId) and the same hits
    rec_refit = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    assert refit.hip_build_accel(r) == 0
    rec_built = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    by_id = {int(g): k for k, g in enumerate(rec_built["globalId"])}
    pick = np.array([by_id[int(g)] for g in rec_refit["globalId"]])
    for field in ("v0", "e1", "e2", "flags", "omm"):
        assert np.array_equal(rec_refit[field].view(np.uint32), rec_built[field][pick].view(np.uint32)), field
    assert np.array_equal(r.trace_closest(rays).view(np.uint32), b.view(np.uint32))
    r.destroy(); fresh.destroy()


# ---- frames: an 8-frame sequence in which two instances move every frame (one of them the emitter), orbiting camera, against the oracle ------------------
def plan(f, home, far=False):
    """the moves before frame f of the Cornell sequence: the short box (3) slides and turns, the light (5) slides under the ceiling"""
    box = refit.compose(refit.translation([0.03 * f, 0.0, -0.02 * f]), refit.compose(refit.rotation_y(0.1 * f, (0.33, 0.3, 0.35)), home[3]))
    light = refit.compose(refit.translation([0.04 * f - 0.1, 0.0, 0.02 * f]), home[5])
    if far and f in (4, 5):     # the box leaves the room: the pad grows at frame 4 and shrinks again at frame 6
        box = refit.compose(refit.translation([9.0, 1.0, -7.0]), box)
    return [3, 5], np.stack([box, light])


class Sequence:
    """the scene, the oracle and the per-frame cameras; the oracle's frames are rendered once per size and shared by the cases"""
    cache = {}

    def __init__(self, W, H, far=False):
        self.W, self.H, self.far = W, H, far
        self.sc = refit.cornell()
        self.home = refit.instances_of(self.sc.desc())["objectToWorld"]
        self.st = host.default_state(W, H, self.sc, None)
        self.st.environmentProb = 0.0
        self.pose = self.sc.cameraPose()

    def step(self, f):
        """move the scene for frame f and return (ids, xf, desc, camera)"""
        ids, xf = plan(f, self.home, self.far)
        self.sc.updateInstances(ids, xf)
        eye, center, up, fov = self.pose
        a = 0.06 * f
        d = np.asarray(eye, np.float64) - center
        e = center + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        self.st.time = 1000 + f
        return ids, xf, self.sc.desc(), self.sc.getCamera()

    @classmethod
    def oracle_frames(cls, W, H, far=False, frames=FRAMES):
        key = (W, H, far, frames)
        if key not in cls.cache:
            s = cls(W, H, far)
            o = Oracle(0)
            o.upload_scene(s.sc.desc())
            o.resize(W, H)
            out = []
            for f in range(frames):
                _, _, desc, cam = s.step(f)
                o.upload_scene(desc)          # (the oracle keeps its frame buffers across a scene upload: the history carries over)
                o.set_camera(cam)
                o.render_frame(s.st, f)
                out.append({b: o.readback(b).copy() for b in frame_buffers(f)})
            cls.cache[key] = out
        return cls.cache[key]


def run_case(W, H, overlap, traversal, far=False, frames=FRAMES, after=None):
    want = Sequence.oracle_frames(W, H, far, frames)
    s = Sequence(W, H, far)
    r = renderer(s.sc.desc(), W, H, overlap, traversal)
    bad, fulls = {}, []
    for f in range(frames):
        ids, xf, desc, cam = s.step(f)
        r.update_instances(ids, xf)
        r.update_lights(desc)
        fulls.append(int(r.refit_stats().fullRefit))
        r.set_camera(cam)
        r.run(s.st, f)
        if after:
            after(r, s, f)
        for b in frame_buffers(f):
            d = optin.words(r.readback(b), want[f][b])
            if d:
                bad[(f, abi.BUFFER_NAMES[b])] = d
    return r, s, bad, fulls


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
def test_frames_equal_the_oracle_rendering_the_moved_scene(W, H, overlap, traversal):
    r, s, bad, _ = run_case(W, H, overlap, traversal)
    r.destroy()
    assert bad == {}
    # the sequence is not a still: the moved surfaces and the moved light change the frames
    want = Sequence.oracle_frames(W, H)
    assert optin.words(want[2][abi.BUF_GBUFFER0], want[4][abi.BUF_GBUFFER0]) > 0


def test_pad_growth_mid_sequence_and_a_later_rebuild():
    W, H = SIZES[0]
    r, s, bad, fulls = run_case(W, H, 2, None, far=True)
    assert bad == {}
    # the box leaves the room at frame 4 (the pad grows: a full refit), drifts on at frame 5 and is back at frame 6: a smaller pad refits nothing in full
    assert fulls[:4] == [0, 0, 0, 0] and fulls[4] == 1 and fulls[6:] == [0, 0]
    # rt_build_accel after the updates: the next frames are the refitted tree's, which are the oracle's
    want = Sequence.oracle_frames(W, H, True, FRAMES + 2)
    s2 = Sequence(W, H, True)
    for f in range(FRAMES):
        s2.step(f)
    assert refit.hip_build_accel(r) == 0
    for f in range(FRAMES, FRAMES + 2):
        ids, xf, desc, cam = s2.step(f)
        r.update_instances(ids, xf)     # (on the rebuilt tree: the update's maps are derived again)
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s2.st, f)
        # (rt_build_accel leaves the frame buffers alone: the history carries over like the oracle's)
        assert {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), want[f][b]) for b in frame_buffers(f) if optin.words(r.readback(b), want[f][b])} == {}, f
    r.destroy()


# ---- one case each with an opt-in pass on, against its checker ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["svgf", "gi_spatial", "taa"])
def test_moves_with_an_opt_in_pass(tmp_path, which):
    import gi_spatial
    W, H = SIZES[1]
    kw = {"svgf": dict(den=abi.Denoiser(mode=abi.DENOISER_SVGF)), "gi_spatial": dict(gis=abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY)), "taa": dict(t=abi.Taa(mode=abi.TAA_ON))}[which]
    rig = optin.Rig(tmp_path, abi.PROC_CORNELL, 1.0, None, W, H, overlap=2, **kw)
    home = refit.instances_of(rig.sc.desc())["objectToWorld"]
    for f in range(5):
        ids, xf = plan(f, home)
        rig.sc.updateInstances(ids, xf)
        desc = rig.sc.desc()
        rig.r.update_instances(ids, xf)
        rig.r.update_lights(desc)
        rig.o.upload_scene(desc)
        rig.kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp_path), desc)
        rig.desc = desc
        rig.frame(f)
        assert rig.diff(f) == {}, f
    n = rig.history_lengths()
    if which != "gi_spatial":
        assert all(v.max() >= 3 for v in n.values()), {k: v.max() for k, v in n.items()}     # the histories were carried across the updates, not dropped
    rig.destroy()


# ---- state ----------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_mode_restarts_and_the_priority_decision_stays():
    W, H = SIZES[0]
    s = Sequence(W, H)
    r = renderer(s.sc.desc(), W, H, 2)
    for f in range(4):      # past the probe frames: the context has decided
        ids, xf, desc, cam = s.step(f)
        r.set_camera(cam)
        r.run(s.st, f)
    r.sync()
    before = r.stream_priorities()
    assert before["decided"]
    r.reference_render(s.st, 2)
    assert r.reference_samples() == 2
    ids, xf, desc, cam = s.step(4)
    r.update_instances(ids, xf)
    assert r.reference_samples() == 0
    r.reference_render(s.st, 1)
    r.update_lights(desc)
    assert r.reference_samples() == 0
    assert r.stream_priorities() == before
    r.destroy()


def test_refused_calls_change_nothing_and_the_next_frame_matches():
    from restir_amd.renderer import Renderer, RtError, hip_lib
    W, H = SIZES[0]
    want = Sequence.oracle_frames(W, H)
    s = Sequence(W, H)
    desc0 = s.sc.desc()
    # before rt_build_accel
    r0 = Renderer().setup(0)
    ok = refit.instances_of(desc0)["objectToWorld"][3:4]
    ids1 = np.array([3], np.uint32)
    assert hip_lib().rt_update_instances(r0._h, 1, ids1.ctypes.data, ok.ctypes.data) == abi.ERR_NO_SCENE
    assert hip_lib().rt_upload_scene(r0._h, C.byref(desc0)) == 0
    assert hip_lib().rt_update_instances(r0._h, 1, ids1.ctypes.data, ok.ctypes.data) == abi.ERR_NO_ACCEL
    r0.destroy()
    r = renderer(desc0, W, H, 2)
    for f in range(2):
        ids, xf, desc, cam = s.step(f)
        r.update_instances(ids, xf)
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
    state = [r.accel_readback(w, desc.numInstances).copy() for w in range(3)]
    stats = bytes(r.refit_stats())
    nan = ok.copy(); nan[0, 7] = np.nan
    inf = ok.copy(); inf[0, 0] = np.inf
    singular = ok.copy(); singular[0, 4:7] = singular[0, 0:3]
    for bad_ids, xf in (([desc.numInstances], ok), ([3, 3], np.concatenate([ok, ok])), ([3], nan), ([3], inf), ([3], singular), ([2, 3], np.concatenate([ok, nan]))):
        with pytest.raises(RtError):
            r.update_instances(bad_ids, xf)
        assert all(np.array_equal(a, r.accel_readback(w, desc.numInstances)) for w, a in enumerate(state)), bad_ids
        assert bytes(r.refit_stats()) == stats
    # a wrong light count
    info = abi.LightBufInfo.from_buffer_copy(desc.lightInfo)
    info.trigLightSize -= 1
    assert hip_lib().rt_update_lights(r._h, desc.trigLights, info.trigLightSize, desc.puncLights, 0, C.byref(info)) == abi.ERR_INVALID_ARG
    assert hip_lib().rt_update_lights(r._h, desc.trigLights, desc.lightInfo.trigLightSize, desc.puncLights, 0, C.byref(info)) == abi.ERR_INVALID_ARG
    # the next frame of the sequence still matches the oracle
    ids, xf, desc, cam = s.step(2)
    r.update_instances(ids, xf)
    r.update_lights(desc)
    r.set_camera(cam)
    r.run(s.st, 2)
    assert {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), want[2][b]) for b in frame_buffers(2) if optin.words(r.readback(b), want[2][b])} == {}
    r.destroy()

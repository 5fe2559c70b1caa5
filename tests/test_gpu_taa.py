"""Temporal anti-aliasing on the MI355X (rt_set_taa, csrc/taa.hip) against the oracle rendered with rt_taa_jitter_camera's camera and the CPU restatement of the
resolve (tests/taa_checker.cpp), word for word: every frame buffer of the existing parity tests, the resolved images and n, on three scenes and every schedule,
with SVGF and with GI spatial reuse; a static camera's motion vectors; the tonemapped frame; every invalidation rule; the error paths; mode off allocating
and changing nothing; the reference mode unaffected."""
import ctypes as C
import numpy as np
import pytest
from helpers import abi, host, make_scene, frame_buffers
from oracle.binding import Oracle
import taa
import svgf
import gi_spatial

pytestmark = pytest.mark.gpu

# name, kind, scale, env, W, H
SCENES = [
    ("cornell", abi.PROC_CORNELL, 1.0, None, 64, 48),
    ("sponza-env", abi.PROC_SPONZA, 0.01, (64, 32), 64, 48),
    ("bistro-ext-alpha", abi.PROC_BISTRO_EXT, 0.01, (64, 32), 64, 40),
]
N = 5


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return taa.build(tmp_path_factory.mktemp("taa"))


def _diff(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)
    return int((a != b).sum())


class Setup:
    def __init__(self, lib, scene, overlap=0, t=None, denoise=1, oracle=True, den=None, gis=None, set_taa=True):
        from restir_amd.renderer import Renderer
        name, kind, scale, env_size, W, H = scene
        self.sc, self.env = make_scene(kind, scale, 1, env_size)
        self.W, self.H = W, H
        self.st = host.default_state(W, H, self.sc, self.env)
        if self.env is None:
            self.st.environmentProb = 0.0
        self.st.denoise = denoise
        self.desc = self.sc.desc(self.env)
        self.t = t if t is not None else abi.Taa(mode=abi.TAA_ON)
        self.r = Renderer().setup(0)
        self.r.set_overlap(overlap)
        self.r.load_scene(self.desc)
        self.r.update(W, H)
        if den is not None:
            self.r.set_denoiser(den)
        if gis is not None:
            self.r.set_gi_spatial(gis)
        if set_taa:
            self.r.set_taa(self.t)
        self.o = self.k = None
        if oracle:
            self.o = Oracle(0)
            self.o.upload_scene(self.desc)
            self.o.resize(W, H)
            self.k = taa.TaaChecker(lib, W, H, self.t)
        self.pose = self.sc.cameraPose()

    def camera(self, f, move=0.0, orbit=0.0):
        eye, center, up, fov = self.pose
        eye = np.array(eye, dtype=np.float64)
        if orbit:
            c = np.array(center, dtype=np.float64)
            v = eye - c
            a = orbit * f
            v = np.array([v[0] * np.cos(a) - v[2] * np.sin(a), v[1], v[0] * np.sin(a) + v[2] * np.cos(a)])
            eye = c + v
        eye = eye + move * f * np.array([1.0, 0.25, -0.75])
        self.sc.setCamera(eye.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        return self.sc.getCamera()

    def gpu_frame(self, f, cam):
        self.st.time = 1000 + f
        self.r.set_camera(cam)
        self.r.run(self.st, f)

    def oracle_frame(self, f, cam):
        self.st.time = 1000 + f
        return taa.oracle_frame(self.o, self.k, self.st, cam, f, self.t.jitterPhases)


def _check_resolved(s, f):
    bad = {}
    cur = f & 1
    for which, want in ((abi.TAA_DIRECT, s.k.D[cur]), (abi.TAA_INDIRECT, s.k.I[cur]), (abi.TAA_HISTORY_LENGTH, s.k.N[cur])):
        d = _diff(s.r.taa_readback(which), want)
        if d:
            bad[f"taa{which}"] = d
    return bad


@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_frames_match_the_oracle_with_the_jittered_camera(lib, scene, overlap):
    s = Setup(lib, scene, overlap)
    for f in range(N):
        cam = s.camera(f, move=0.01)
        s.gpu_frame(f, cam)
        s.oracle_frame(f, cam)
        bad = {}
        for b in frame_buffers(f):
            d = _diff(s.r.readback(b), s.o.readback(b))
            if d:
                bad[abi.BUFFER_NAMES[b]] = d
        bad.update(_check_resolved(s, f))
        assert not bad, f"frame {f}: {bad}"
    assert (s.k.N[(N - 1) & 1] > 1).any()


@pytest.mark.parametrize("camera", ["static", "orbit"])
def test_resolve_over_many_frames_with_a_reset(lib, camera):
    s = Setup(lib, SCENES[1], 2, abi.Taa(mode=abi.TAA_ON, jitterPhases=16, alpha=0.1, clipGamma=1.0))
    nmax = 0
    for f in range(10):
        if f == 5:
            s.r.taa_reset()
            s.k.reset()
        cam = s.camera(f, orbit=0.01 if camera == "orbit" else 0.0)
        s.gpu_frame(f, cam)
        s.oracle_frame(f, cam)
        bad = _check_resolved(s, f)
        assert not bad, f"frame {f}: {bad}"
        n = s.k.N[f & 1]
        if f == 5:
            assert (n == 1).all()
        nmax = max(nmax, int(n.max()))
    assert nmax >= 5


@pytest.mark.parametrize("which", ["svgf", "gi_spatial"])
def test_with_svgf_and_with_gi_spatial_reuse(lib, tmp_path_factory, which):
    den = abi.Denoiser(mode=abi.DENOISER_SVGF) if which == "svgf" else None
    gis = abi.GiSpatial(mode=abi.GI_SPATIAL_ON, samples=5, radius=6) if which == "gi_spatial" else None
    s = Setup(lib, SCENES[1], 2, den=den, gis=gis)
    k2 = svgf.SvgfChecker(svgf.build(tmp_path_factory.mktemp("svgf")), s.W, s.H, den) if den is not None else None
    kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp_path_factory.mktemp("gis")), s.desc) if gis is not None else None
    for f in range(N):
        cam = s.camera(f, move=0.01)
        s.gpu_frame(f, cam)
        s.st.time = 1000 + f
        jc = taa.jitter_camera(cam, f, s.t.jitterPhases, s.W, s.H)
        s.o.set_camera(jc)
        if kg is not None:
            gi_spatial.oracle_frame(s.o, kg, s.st, jc, f, gis)
        else:
            svgf.oracle_frame(s.o, k2, s.st, jc, f)
        cur = f & 1
        s.k.frame(jc, f, s.o.readback(abi.BUF_GBUFFER0 + cur), s.o.readback(abi.BUF_GBUFFER0 + 1 - cur), s.o.readback(abi.BUF_DIRECT_RESULT0 + cur),
                  s.o.readback(abi.BUF_INDIRECT_RESULT0 + cur))
        bad = {}
        for b in (abi.BUF_GBUFFER0 + cur, abi.BUF_MOTION, abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESV0 + cur):
            d = _diff(s.r.readback(b), s.o.readback(b))
            if d:
                bad[abi.BUFFER_NAMES[b]] = d
        bad.update(_check_resolved(s, f))
        assert not bad, f"frame {f}: {bad}"


def _surface(r, f, W, H):
    g = r.readback(abi.BUF_GBUFFER0 + (f & 1)).view(np.uint32).reshape(H, W, 4)
    return (g[..., 3] & np.uint32(0xFF000000)) != 0xFF000000


def test_static_camera_motion_and_the_tonemapped_frame(lib):
    s = Setup(lib, SCENES[0], 2)
    off = Setup(lib, SCENES[0], 2, abi.Taa(), oracle=False)
    W, H = s.W, s.H
    for f in range(4):
        cam = s.camera(f)
        s.gpu_frame(f, cam)
        off.gpu_frame(f, cam)
        s.oracle_frame(f, cam)
        both = _surface(s.r, f, W, H) & _surface(off.r, f, W, H)
        ma = s.r.readback(abi.BUF_MOTION).view(np.int16).reshape(H, W, 2)
        mb = off.r.readback(abi.BUF_MOTION).view(np.int16).reshape(H, W, 2)
        assert both.mean() > 0.5 and np.array_equal(ma[both], mb[both]), f
    # rt_tonemap of a resolved frame == the oracle's tonemap over the resolved images
    f = 3
    tm = abi.Tonemapper()
    s.r.tonemap(tm, 0, f)
    cur = f & 1
    s.o.upload_history(abi.BUF_DIRECT_RESULT0 + cur, s.k.D[cur])
    s.o.upload_history(abi.BUF_INDIRECT_RESULT0 + cur, s.k.I[cur])
    s.o.tonemap(tm, 0, f)
    assert _diff(s.r.readback(abi.BUF_LDR), s.o.readback(abi.BUF_LDR)) == 0
    # a frame that was not resolved (debugging_mode != 0) is tonemapped from the plain result images
    s.st.debugging_mode = 4   # RT_DBG_NORMAL
    s.r.set_camera(s.camera(4)); s.st.time = 1004
    s.r.run(s.st, 4)
    s.r.tonemap(tm, 0, 4)
    o2 = Oracle(0); o2.upload_scene(s.desc); o2.resize(W, H)
    for b in (abi.BUF_DIRECT_RESULT0, abi.BUF_INDIRECT_RESULT0):
        o2.upload_history(b, s.r.readback(b))
    o2.tonemap(tm, 0, 4)
    assert _diff(s.r.readback(abi.BUF_LDR), o2.readback(abi.BUF_LDR)) == 0


def _n_after(s, f, cam=None):
    s.gpu_frame(f, cam if cam is not None else s.camera(f))
    n = s.r.taa_readback(abi.TAA_HISTORY_LENGTH)
    return n[_surface(s.r, f, s.W, s.H)]


@pytest.mark.parametrize("overlap", [0, 2])
def test_invalidation_rules(lib, overlap):
    s = Setup(lib, SCENES[1], overlap, oracle=False)
    f = 0
    for f in range(3):
        _n_after(s, f)
    assert (_n_after(s, 3) > 1).mean() > 0.5
    f = 4
    rules = [("reset", lambda: s.r.taa_reset()),
             ("set_taa", lambda: s.r.set_taa(abi.Taa(mode=abi.TAA_ON, alpha=0.15))),
             ("upload_scene", lambda: s.r.load_scene(s.desc)),
             ("debug frame", lambda: (setattr(s.st, "debugging_mode", 4), s.gpu_frame(100, s.camera(0)), setattr(s.st, "debugging_mode", 0))),
             ("taa off frame", lambda: (s.r.set_taa(abi.Taa()), s.gpu_frame(100, s.camera(0)), s.r.set_taa(abi.Taa(mode=abi.TAA_ON, alpha=0.15)))),
             ("parity", None),
             ("resize", lambda: s.r.update(s.W, s.H))]
    for name, action in rules:
        for _ in range(2):
            _n_after(s, f); f += 1
        assert (_n_after(s, f) > 1).any(), name
        f += 1
        if action is None:
            f += 1   # skip a frame: the parity does not follow
        else:
            action()
        n = _n_after(s, f)
        f += 1
        assert (n == 1).all(), (name, float((n != 1).mean()))


def test_error_paths(lib):
    s = Setup(lib, SCENES[0], 0, abi.Taa(), oracle=False)
    from restir_amd import renderer
    L = renderer.hip_lib()
    h = s.r._h
    good = s.r.get_taa()
    assert bytes(good) == bytes(abi.Taa())
    nan, inf = float("nan"), float("inf")
    base = dict(mode=abi.TAA_ON, jitterPhases=8, alpha=0.1, clipGamma=1.0)
    for bad in (dict(mode=2), dict(mode=-1), dict(jitterPhases=-1), dict(jitterPhases=17), dict(alpha=0.0), dict(alpha=1.01), dict(alpha=nan),
                dict(clipGamma=0.0), dict(clipGamma=-1.0), dict(clipGamma=inf), dict(clipGamma=nan)):
        t = abi.Taa(**dict(base, **bad))
        assert L.rt_set_taa(h, C.byref(t)) == abi.ERR_INVALID_ARG, bad
        assert bytes(s.r.get_taa()) == bytes(good), bad
    for i in range(4):
        t = abi.Taa(**base)
        t.reserved[i] = 1
        assert L.rt_set_taa(h, C.byref(t)) == abi.ERR_INVALID_ARG and bytes(s.r.get_taa()) == bytes(good)
    assert L.rt_set_taa(h, None) == abi.ERR_INVALID_ARG
    for ok in (dict(jitterPhases=0), dict(jitterPhases=16), dict(alpha=1.0), dict(clipGamma=1e-3)):
        t = abi.Taa(**dict(base, **ok))
        assert L.rt_set_taa(h, C.byref(t)) == 0 and bytes(s.r.get_taa()) == bytes(t), ok
    s.r.set_taa(abi.Taa(**base))
    W, H = s.W, s.H
    buf = np.zeros((H, W, 4), np.float32)
    assert L.rt_taa_readback(h, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET        # before the first resolved frame
    s.st.time = 1000
    s.r.set_camera(s.camera(0))
    assert L.rt_run_stage(h, C.byref(s.st), 0, abi.STAGE_DIRECT, 0, 0, 0) == abi.ERR_INVALID_ARG
    assert b"TAA" in L.rt_last_error(h)
    s.gpu_frame(0, s.camera(0))
    assert L.rt_taa_readback(h, 0, buf.ctypes.data, buf.nbytes) == 0
    for which, wrong in ((0, buf.nbytes - 4), (2, buf.nbytes), (1, 0)):
        assert L.rt_taa_readback(h, which, buf.ctypes.data, wrong) == abi.ERR_INVALID_ARG
    assert L.rt_taa_readback(h, 3, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG
    assert L.rt_taa_readback(h, 0, None, buf.nbytes) == abi.ERR_INVALID_ARG
    s.r.update(W, H)
    assert L.rt_taa_readback(h, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET        # after rt_resize
    s.r.set_taa(abi.Taa())
    assert L.rt_run_stage(h, C.byref(s.st), 0, abi.STAGE_DIRECT, 0, 0, 0) == 0


def test_mode_off_allocates_and_changes_nothing(lib):
    a = Setup(lib, SCENES[2], 2, abi.Taa(), oracle=False)
    b = Setup(lib, SCENES[2], 2, abi.Taa(mode=abi.TAA_OFF, jitterPhases=3, alpha=0.5), oracle=False)
    c = Setup(lib, SCENES[2], 2, oracle=False, set_taa=False)   # never calls rt_set_taa
    for f in range(N):
        cam = a.camera(f, move=0.01)
        for s in (a, b, c):
            s.gpu_frame(f, cam)
    for b_ in frame_buffers(N - 1):
        assert _diff(a.r.readback(b_), c.r.readback(b_)) == 0 and _diff(b.r.readback(b_), c.r.readback(b_)) == 0, abi.BUFFER_NAMES[b_]
    from restir_amd import renderer
    buf = np.zeros((a.H, a.W, 4), np.float32)
    assert renderer.hip_lib().rt_taa_readback(a.r._h, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET   # nothing was allocated or resolved
    tm = abi.Tonemapper()
    a.r.tonemap(tm, 0, N - 1); c.r.tonemap(tm, 0, N - 1)
    assert _diff(a.r.readback(abi.BUF_LDR), c.r.readback(abi.BUF_LDR)) == 0


def test_reference_mode_is_unaffected(lib):
    on = Setup(lib, SCENES[1], 2, oracle=False)
    off = Setup(lib, SCENES[1], 2, abi.Taa(), oracle=False)
    for s in (on, off):
        for f in range(3):
            s.gpu_frame(f, s.camera(0))
        s.r.reference_render(s.st, 4)
    for comp in (abi.REF_DIRECT, abi.REF_INDIRECT, abi.REF_SUM):
        assert _diff(on.r.reference_readback(comp), off.r.reference_readback(comp)) == 0

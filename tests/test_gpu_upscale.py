"""Temporal upsampling on the MI355X (rt_set_upscale, csrc/upscale.hip) against the oracle rendered at the render size with rt_upscale_jitter_camera's camera
and the CPU restatement of the resolve (tests/upscale_checker.cpp), word for word: every frame buffer, the resolved images and n at the output size — integer,
ragged non-integer, unit and limit ratios, below one tile in a child process — under every schedule, with SVGF and with GI spatial reuse; the tonemapped
output-size frame; every invalidation rule; every refusal; mode off allocating and changing nothing; the reference mode unaffected."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import abi, host, make_scene, frame_buffers
from oracle.binding import Oracle
import upscale
import svgf
import gi_spatial

pytestmark = pytest.mark.gpu

SPONZA = (abi.PROC_SPONZA, 0.01, (64, 32))
CORNELL = (abi.PROC_CORNELL, 1.0, None)
# render W, H -> output Wo, Ho
SIZES = [
    (24, 16, 48, 32),   # ratio 2: dyadic sample geometry, 6 x 4 output tiles
    (37, 27, 56, 41),   # ragged at both sizes, non-integer ratios that differ per axis (1.51, 1.52)
    (16, 16, 16, 16),   # ratio 1: the pass degenerates to TAA's geometry
    (8, 8, 32, 32),     # ratio 4, the limit: one render tile feeds 16 output tiles
]
TINY = (1, 1, 3, 2)     # below one tile at both sizes (child process)
FRAMES = 12             # six static, six orbiting
RESET_AT = 9


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return upscale.build(tmp_path_factory.mktemp("upscale"))


def _diff(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.size == b.size, (a.size, b.size)
    return int((a != b).sum())


def _ups(size, **kw):
    return abi.Upscale(**dict(dict(mode=abi.UPSCALE_TEMPORAL, outWidth=size[2], outHeight=size[3]), **kw))


class Setup:
    def __init__(self, lib, size, overlap=0, u=None, scene=SPONZA, oracle=True, den=None, gis=None, set_upscale=True):
        from restir_amd.renderer import Renderer
        kind, scale, env_size = scene
        W, H = size[:2]
        self.sc, self.env = make_scene(kind, scale, 1, env_size)
        self.W, self.H, self.size = W, H, size
        self.st = host.default_state(W, H, self.sc, self.env)
        if self.env is None:
            self.st.environmentProb = 0.0
        self.desc = self.sc.desc(self.env)
        self.u = u if u is not None else _ups(size)
        self.r = Renderer().setup(0)
        self.r.set_overlap(overlap)
        self.r.load_scene(self.desc)
        self.r.update(W, H)
        if den is not None:
            self.r.set_denoiser(den)
        if gis is not None:
            self.r.set_gi_spatial(gis)
        if set_upscale:
            self.r.set_upscale(self.u)
        self.o = self.k = None
        if oracle:
            self.o = Oracle(0)
            self.o.upload_scene(self.desc)
            self.o.resize(W, H)
            self.k = upscale.UpscaleChecker(lib, W, H, self.u)
        self.pose = self.sc.cameraPose()

    def destroy(self):
        self.r.destroy()

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

    def oracle_frame(self, f, cam, render=None):
        self.st.time = 1000 + f
        return upscale.oracle_frame(self.o, self.k, self.st, cam, f, render)


def _check_resolved(s, f):
    bad = {}
    cur = f & 1
    for which, want in ((abi.UPSCALE_DIRECT, s.k.D[cur]), (abi.UPSCALE_INDIRECT, s.k.I[cur]), (abi.UPSCALE_HISTORY_LENGTH, s.k.N[cur])):
        d = _diff(s.r.upscale_readback(which), want)
        if d:
            bad[f"upscale{which}"] = d
    return bad


def _check_tonemap(s, f):
    """rt_upscale_tonemap of frame f == the oracle's post pass over the resolved images in an oracle sized Wo x Ho"""
    Wo, Ho = s.size[2:]
    tm = abi.Tonemapper()
    s.r.upscale_tonemap(tm, f)
    o2 = Oracle(0); o2.upload_scene(s.desc); o2.resize(Wo, Ho)
    cur = f & 1
    o2.upload_history(abi.BUF_DIRECT_RESULT0 + cur, s.k.D[cur])
    o2.upload_history(abi.BUF_INDIRECT_RESULT0 + cur, s.k.I[cur])
    o2.tonemap(tm, 0, f)
    return _diff(s.r.upscale_readback(abi.UPSCALE_LDR), o2.readback(abi.BUF_LDR))


def run_case(lib, size, overlap, scene=SPONZA, frames=FRAMES, live=True):
    """six frames of a static camera, then an orbit, one reset on the way: every frame buffer against the oracle with the jittered camera, the resolved images and
    n against the checker, after every frame; then the tonemapped output-size frame"""
    s = Setup(lib, size, overlap, scene=scene)
    try:
        nmax = 0
        for f in range(frames):
            if f == RESET_AT:
                s.r.upscale_reset()
                s.k.reset()
            cam = s.camera(f, orbit=0.01 * (f - 5) if f >= 6 else 0.0)
            s.gpu_frame(f, cam)
            s.oracle_frame(f, cam)
            bad = {}
            for b in frame_buffers(f):
                d = _diff(s.r.readback(b), s.o.readback(b))
                if d:
                    bad[abi.BUFFER_NAMES[b]] = d
            bad.update(_check_resolved(s, f))
            assert not bad, f"{size} overlap {overlap} frame {f}: {bad}"
            n = s.k.N[f & 1]
            if f == RESET_AT:
                assert (n == 1).all()
            nmax = max(nmax, int(n.max()))
        assert not live or nmax >= 5, nmax
        assert _check_tonemap(s, frames - 1) == 0
    finally:
        s.destroy()


@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda v: "%dx%d-%dx%d" % v)
def test_frames_resolve_and_tonemap_match_under_every_schedule(lib, size, overlap):
    run_case(lib, size, overlap)


def tiny_child():
    upscale.load(os.environ["RESTIR_UPSCALE_CHK"])
    for overlap in (0, 2):
        run_case(upscale._lib, TINY, overlap, scene=CORNELL, live=False)
    print("tiny ok", flush=True)
    return 0


def test_below_one_tile(lib):
    """1 x 1 -> 3 x 2 in a child process of its own, with its own time limit, serial and with frames in flight"""
    env = dict(os.environ, RESTIR_UPSCALE_CHK=upscale.lib_path)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tiny"], env=env, cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "tiny ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("which", ["svgf", "gi_spatial"])
def test_with_svgf_and_with_gi_spatial_reuse(lib, tmp_path_factory, which):
    den = abi.Denoiser(mode=abi.DENOISER_SVGF) if which == "svgf" else None
    gis = abi.GiSpatial(mode=abi.GI_SPATIAL_ON, samples=5, radius=6) if which == "gi_spatial" else None
    s = Setup(lib, SIZES[1], 2, den=den, gis=gis)
    try:
        k2 = svgf.SvgfChecker(svgf.build(tmp_path_factory.mktemp("svgf")), s.W, s.H, den) if den is not None else None
        kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp_path_factory.mktemp("gis")), s.desc) if gis is not None else None
        if kg is not None:
            render = lambda o, st, jc, f: gi_spatial.oracle_frame(o, kg, st, jc, f, gis)   # noqa: E731
        else:
            render = lambda o, st, jc, f: svgf.oracle_frame(o, k2, st, jc, f)   # noqa: E731
        for f in range(5):
            cam = s.camera(f, move=0.01)
            s.gpu_frame(f, cam)
            s.oracle_frame(f, cam, render)
            cur = f & 1
            bad = {}
            for b in (abi.BUF_GBUFFER0 + cur, abi.BUF_MOTION, abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESV0 + cur):
                d = _diff(s.r.readback(b), s.o.readback(b))
                if d:
                    bad[abi.BUFFER_NAMES[b]] = d
            bad.update(_check_resolved(s, f))
            assert not bad, f"frame {f}: {bad}"
        assert (s.k.N[0] > 1).any()
    finally:
        s.destroy()


def _n_after(s, f, cam=None):
    s.gpu_frame(f, cam if cam is not None else s.camera(0))
    return s.r.upscale_readback(abi.UPSCALE_HISTORY_LENGTH)


@pytest.mark.parametrize("overlap", [0, 2])
def test_invalidation_rules(lib, overlap):
    size = SIZES[0]
    s = Setup(lib, size, overlap, oracle=False)
    try:
        for f in range(3):
            _n_after(s, f)
        assert (_n_after(s, 3) > 1).any()
        f = 4
        on = _ups(size, alpha=0.15)
        rules = [("reset", lambda: s.r.upscale_reset()),
                 ("set_upscale", lambda: s.r.set_upscale(on)),
                 ("output size", lambda: (s.r.set_upscale(_ups((24, 16, 40, 30))), s.r.set_upscale(on))),
                 ("upload_scene", lambda: s.r.load_scene(s.desc)),
                 ("debug frame", lambda: (setattr(s.st, "debugging_mode", 4), s.gpu_frame(100, s.camera(0)), setattr(s.st, "debugging_mode", 0))),
                 ("upscale off frame", lambda: (s.r.set_upscale(abi.Upscale()), s.gpu_frame(100, s.camera(0)), s.r.set_upscale(on))),
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
    finally:
        s.destroy()


def test_refusals_and_error_paths(lib):
    size = SIZES[0]
    W, H, Wo, Ho = size
    s = Setup(lib, size, 0, abi.Upscale(), oracle=False)
    try:
        from restir_amd import renderer
        L = renderer.hip_lib()
        h = s.r._h
        err = lambda: L.rt_last_error(h)   # noqa: E731
        good = s.r.get_upscale()
        assert bytes(good) == bytes(abi.Upscale())
        nan, inf = float("nan"), float("inf")
        base = dict(mode=abi.UPSCALE_TEMPORAL, outWidth=Wo, outHeight=Ho, jitterPhases=16, alpha=0.1, clipGamma=1.0)
        # bad field values, the ratio limits among them (a target exists): refused, the settings in use stay
        for bad in (dict(mode=2), dict(mode=-1), dict(jitterPhases=-1), dict(jitterPhases=65), dict(alpha=0.0), dict(alpha=1.01), dict(alpha=nan),
                    dict(clipGamma=0.0), dict(clipGamma=-1.0), dict(clipGamma=inf), dict(clipGamma=nan), dict(outWidth=0), dict(outHeight=0), dict(outWidth=-1),
                    dict(outWidth=W - 1), dict(outHeight=H - 1), dict(outWidth=4 * W + 1), dict(outHeight=4 * H + 1)):
            u = abi.Upscale(**dict(base, **bad))
            assert L.rt_set_upscale(h, C.byref(u)) == abi.ERR_INVALID_ARG, bad
            assert b"rt_set_upscale" in err(), bad
            assert bytes(s.r.get_upscale()) == bytes(good), bad
        for i in range(2):
            u = abi.Upscale(**base)
            u.reserved[i] = 1
            assert L.rt_set_upscale(h, C.byref(u)) == abi.ERR_INVALID_ARG and bytes(s.r.get_upscale()) == bytes(good)
        assert L.rt_set_upscale(h, None) == abi.ERR_INVALID_ARG
        for ok in (dict(jitterPhases=0), dict(jitterPhases=64), dict(alpha=1.0), dict(clipGamma=1e-3), dict(outWidth=W, outHeight=H),
                   dict(outWidth=4 * W, outHeight=4 * H), dict(outWidth=W + 1, outHeight=4 * H)):
            u = abi.Upscale(**dict(base, **ok))
            assert L.rt_set_upscale(h, C.byref(u)) == 0 and bytes(s.r.get_upscale()) == bytes(u), ok
        s.r.set_upscale(abi.Upscale())
        # turning upsampling on while TAA is on
        s.r.set_taa(abi.Taa(mode=abi.TAA_ON))
        u = abi.Upscale(**base)
        assert L.rt_set_upscale(h, C.byref(u)) == abi.ERR_INVALID_ARG and b"TAA" in err()
        assert bytes(s.r.get_upscale()) == bytes(abi.Upscale())
        s.r.set_taa(abi.Taa())
        # rt_set_taa(ON) while upsampling is on; switching TAA's other fields with mode OFF stays possible
        s.r.set_upscale(u)
        t = abi.Taa(mode=abi.TAA_ON)
        assert L.rt_set_taa(h, C.byref(t)) == abi.ERR_INVALID_ARG and b"rt_set_upscale" in err()
        assert bytes(s.r.get_taa()) == bytes(abi.Taa())
        s.r.set_taa(abi.Taa(jitterPhases=4))
        # readbacks and the tonemap before the first resolved frame
        buf = np.zeros((Ho, Wo, 4), np.float32)
        tm = abi.Tonemapper()
        assert L.rt_upscale_readback(h, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
        assert L.rt_upscale_tonemap(h, C.byref(tm), 0) == abi.ERR_NO_TARGET
        # rt_run_stage while the mode is on
        s.st.time = 1000
        s.r.set_camera(s.camera(0))
        assert L.rt_run_stage(h, C.byref(s.st), 0, abi.STAGE_DIRECT, 0, 0, 0) == abi.ERR_INVALID_ARG
        assert b"upsampling" in err()
        s.gpu_frame(0, s.camera(0))
        assert L.rt_upscale_readback(h, 0, buf.ctypes.data, buf.nbytes) == 0
        assert L.rt_upscale_readback(h, 3, buf.ctypes.data, Wo * Ho * 4) == abi.ERR_NO_TARGET     # LDR before rt_upscale_tonemap
        assert L.rt_upscale_tonemap(h, C.byref(tm), 1) == abi.ERR_NO_TARGET                       # a frame that was not resolved
        assert L.rt_upscale_tonemap(h, None, 0) == abi.ERR_INVALID_ARG
        assert L.rt_upscale_tonemap(h, C.byref(tm), 0) == 0
        assert L.rt_upscale_readback(h, 3, buf.ctypes.data, Wo * Ho * 4) == 0
        for which, wrong in ((0, buf.nbytes - 4), (2, buf.nbytes), (1, 0), (3, buf.nbytes)):
            assert L.rt_upscale_readback(h, which, buf.ctypes.data, wrong) == abi.ERR_INVALID_ARG
        assert L.rt_upscale_readback(h, 4, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG
        assert L.rt_upscale_readback(h, -1, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG
        assert L.rt_upscale_readback(h, 0, None, buf.nbytes) == abi.ERR_INVALID_ARG
        # an rt_resize after which the render size no longer satisfies the ratio limits: the next frame is refused, the settings stay
        for w2, h2 in ((Wo + 1, H), (W, Ho + 8), (Wo // 4 - 1, H)):
            s.r.update(w2, h2)
            s.st.size.x, s.st.size.y = w2, h2
            assert L.rt_upscale_readback(h, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET    # after rt_resize
            s.r.set_camera(s.camera(0))
            assert L.rt_render_frame(h, C.byref(s.st), 0) == abi.ERR_INVALID_ARG and b"rt_resize" in err(), (w2, h2)
            assert bytes(s.r.get_upscale()) == bytes(u)
        s.r.update(W, H)
        s.st.size.x, s.st.size.y = W, H
        s.gpu_frame(0, s.camera(0))
        s.r.set_upscale(abi.Upscale())
        assert L.rt_run_stage(h, C.byref(s.st), 0, abi.STAGE_DIRECT, 0, 0, 0) == 0
    finally:
        s.destroy()


def test_mode_off_allocates_and_changes_nothing(lib):
    size = SIZES[1]
    a = Setup(lib, size, 2, abi.Upscale(), scene=(abi.PROC_BISTRO_EXT, 0.01, (64, 32)), oracle=False)
    b = Setup(lib, size, 2, abi.Upscale(mode=abi.UPSCALE_OFF, outWidth=999, outHeight=3, jitterPhases=3, alpha=0.5), scene=(abi.PROC_BISTRO_EXT, 0.01, (64, 32)),
              oracle=False)
    c = Setup(lib, size, 2, scene=(abi.PROC_BISTRO_EXT, 0.01, (64, 32)), oracle=False, set_upscale=False)   # never calls rt_set_upscale
    try:
        for f in range(5):
            cam = a.camera(f, move=0.01)
            for s in (a, b, c):
                s.gpu_frame(f, cam)
        for b_ in frame_buffers(4):
            assert _diff(a.r.readback(b_), c.r.readback(b_)) == 0 and _diff(b.r.readback(b_), c.r.readback(b_)) == 0, abi.BUFFER_NAMES[b_]
        from restir_amd import renderer
        L = renderer.hip_lib()
        buf = np.zeros((size[3], size[2], 4), np.float32)
        tm = abi.Tonemapper()
        for s in (a, b, c):   # nothing was allocated or resolved
            assert L.rt_upscale_readback(s.r._h, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
            assert L.rt_upscale_tonemap(s.r._h, C.byref(tm), 4) == abi.ERR_NO_TARGET
        a.r.tonemap(tm, 0, 4); c.r.tonemap(tm, 0, 4)
        assert _diff(a.r.readback(abi.BUF_LDR), c.r.readback(abi.BUF_LDR)) == 0
    finally:
        for s in (a, b, c):
            s.destroy()


def test_reference_mode_and_rt_tonemap_are_unaffected(lib):
    size = SIZES[0]
    on = Setup(lib, size, 2, oracle=False)
    off = Setup(lib, size, 2, abi.Upscale(), oracle=False)
    try:
        for s in (on, off):
            for f in range(3):
                s.gpu_frame(f, s.camera(0))
            s.r.reference_render(s.st, 4)
        for comp in (abi.REF_DIRECT, abi.REF_INDIRECT, abi.REF_SUM):
            assert _diff(on.r.reference_readback(comp), off.r.reference_readback(comp)) == 0
        # rt_tonemap keeps reading the render-size result images with the mode on
        tm = abi.Tonemapper()
        on.r.tonemap(tm, 0, 2)
        o2 = Oracle(0); o2.upload_scene(on.desc); o2.resize(on.W, on.H)
        for b in (abi.BUF_DIRECT_RESULT0, abi.BUF_INDIRECT_RESULT0):
            o2.upload_history(b, on.r.readback(b))
        o2.tonemap(tm, 0, 2)
        assert _diff(on.r.readback(abi.BUF_LDR), o2.readback(abi.BUF_LDR)) == 0
    finally:
        on.destroy(); off.destroy()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--tiny":
        sys.exit(tiny_child())

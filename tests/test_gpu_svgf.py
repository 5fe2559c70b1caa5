"""The SVGF denoiser on the MI355X (rt_set_denoiser RT_DENOISER_SVGF, csrc/svgf.hip) against its CPU restatement (tests/svgf_checker.cpp) word for word:
both result images, the filtered indirect image and the four history buffers, on three scenes, through a moving camera with one cut, in every schedule;
the history reset rules; no trace of the mode in a context that switched back to the A-Trous chain; the error paths."""
import ctypes as C
import numpy as np
import pytest
from helpers import abi, host, make_scene, frame_buffers
from oracle.binding import Oracle
import svgf

pytestmark = pytest.mark.gpu

# name, kind, scale, env, W, H
SCENES = [
    ("cornell", abi.PROC_CORNELL, 1.0, None, 64, 64),
    ("sponza-env", abi.PROC_SPONZA, 0.01, (64, 32), 64, 48),
    ("bistro-ext-alpha", abi.PROC_BISTRO_EXT, 0.01, (64, 32), 64, 40),   # alpha-masked foliage
]
N = 8
CUT = 4   # the camera turns round before this frame: most of the history is rejected
HISTORY = (abi.SVGF_DIRECT_COLOR, abi.SVGF_INDIRECT_COLOR, abi.SVGF_DIRECT_MOMENTS, abi.SVGF_INDIRECT_MOMENTS)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return svgf.build(tmp_path_factory.mktemp("svgf"))


class Setup:
    def __init__(self, lib, kind, scale, env_size, W, H, overlap=0, den=None):
        from restir_amd.renderer import Renderer
        self.lib = lib
        self.sc, self.env = make_scene(kind, scale, 1, env_size)
        self.W, self.H = W, H
        self.st = host.default_state(W, H, self.sc, self.env)
        self.desc = self.sc.desc(self.env)
        self.den = den if den is not None else abi.Denoiser(mode=abi.DENOISER_SVGF)
        self.r = Renderer().setup(0)
        self.r.set_overlap(overlap)
        self.r.load_scene(self.desc)
        self.r.update(W, H)
        self.r.set_denoiser(self.den)
        self.o = Oracle(0)
        self.o.upload_scene(self.desc)
        self.o.resize(W, H)
        self.k = svgf.SvgfChecker(lib, W, H, self.den)
        self.pose = self.sc.cameraPose()

    def camera(self, f):
        eye, center, up, fov = self.pose
        if f >= CUT:   # the cut: the view from the opposite side (what it sees was not visible before), then moving again
            eye = center - (eye - center)
        eye = eye + np.array([0.02 * f, 0.005 * f, -0.015 * f], dtype=np.float32)
        self.sc.setCamera(eye, center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        return self.sc.getCamera()

    def frame(self, f, gpu=True, cpu=True):
        self.st.time = 1000 + f
        cam = self.camera(f)
        if gpu:
            self.r.set_camera(cam)
            self.r.run(self.st, f)
        if cpu:
            self.o.set_camera(cam)
            svgf.oracle_frame(self.o, self.k, self.st, cam, f)

    def compare(self, f):
        cur = f & 1
        bad = {}
        for b in (abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESULT0 + cur, abi.BUF_DENOISE_IND_B):
            x, y = self.r.readback(b).view(np.uint32), self.o.readback(b).view(np.uint32)
            if (x != y).any():
                bad[abi.BUFFER_NAMES[b]] = int((x != y).sum())
        for w in HISTORY:
            x, y = self.r.denoiser_readback(w).view(np.uint32), self.k.history(w).view(np.uint32)
            if (x != y).any():
                bad["history%d" % w] = int((x != y).sum())
        assert not bad, f"frame {f}: {bad}"


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("name,kind,scale,env_size,W,H", SCENES, ids=[s[0] for s in SCENES])
def test_bit_exact_every_frame(lib, name, kind, scale, env_size, W, H, overlap):
    s = Setup(lib, kind, scale, env_size, W, H, overlap)
    mean_n = []
    for f in range(N):
        s.frame(f)
        s.compare(f)
        n = s.r.denoiser_readback(abi.SVGF_DIRECT_COLOR)[..., 3]
        mean_n.append(float(n[n > 0].mean()))
    assert mean_n[CUT - 1] > 2.0 and mean_n[CUT] < mean_n[CUT - 1] - 0.5, mean_n   # history accepted, then partly rejected at the cut
    assert n.max() >= 4


@pytest.mark.parametrize("overlap", [2, 3])
@pytest.mark.parametrize("name,kind,scale,env_size,W,H", SCENES, ids=[s[0] for s in SCENES])
def test_bit_exact_frames_in_flight(lib, name, kind, scale, env_size, W, H, overlap):
    """frames submitted back to back (no sync in between); compared after the last one"""
    s = Setup(lib, kind, scale, env_size, W, H, overlap)
    for f in range(N):
        s.frame(f, cpu=False)
    for f in range(N):
        s.frame(f, gpu=False)
    s.compare(N - 1)


def _fresh_history(s, f):
    """frame f's history has n == 1 on every valid pixel and matches the checker"""
    s.frame(f)
    s.compare(f)
    for w, shape in ((abi.SVGF_DIRECT_COLOR, (s.H, s.W)), (abi.SVGF_INDIRECT_COLOR, (s.H // 2, s.W // 2))):
        n = s.r.denoiser_readback(w)[..., 3]
        assert n.shape == shape
        assert set(np.unique(n).tolist()) <= {0.0, 1.0} and (n == 1).sum() > n.size // 4, (w, np.unique(n))


def test_reset_rules(lib):
    name, kind, scale, env_size, W, H = SCENES[1]
    s = Setup(lib, kind, scale, env_size, W, H, overlap=1)
    f = 0

    def warm():
        nonlocal f
        for _ in range(3):
            s.frame(f); f += 1
        assert s.r.denoiser_readback(abi.SVGF_DIRECT_COLOR)[..., 3].max() >= 3

    # rt_denoiser_reset
    warm(); s.r.denoiser_reset(); s.k.reset(); _fresh_history(s, f); f += 1
    # a parameter change
    warm()
    s.den = abi.Denoiser(mode=abi.DENOISER_SVGF, alphaColor=0.3, phiLumIndirect=6.0)
    s.r.set_denoiser(s.den); s.k.set(s.den); _fresh_history(s, f); f += 1
    # a frame with denoise == 0 (the A-Trous-free frame composes the noisy indirect image)
    warm()
    s.st.denoise = 0
    s.frame(f); f += 1
    s.st.denoise = 1
    _fresh_history(s, f); f += 1
    # rt_build_accel
    warm()
    assert renderer_lib().rt_build_accel(s.r._h) == 0
    s.k.reset(); _fresh_history(s, f); f += 1
    # rt_upload_scene (+ rt_build_accel)
    warm()
    s.r.load_scene(s.desc); s.o.upload_scene(s.desc); s.k.reset(); _fresh_history(s, f); f += 1
    # rt_resize: a new size, nothing allocated until the next SVGF frame
    warm()
    W2, H2 = 48, 32
    s.r.update(W2, H2); s.o.resize(W2, H2)
    assert renderer_lib().rt_denoiser_readback(s.r._h, 0, C.c_void_p(0), C.c_size_t(0)) == -1   # (dst NULL)
    buf = np.zeros((H2, W2, 4), dtype=np.float32)
    assert renderer_lib().rt_denoiser_readback(s.r._h, 0, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == abi.ERR_NO_TARGET
    s.W, s.H = W2, H2
    s.st = host.default_state(W2, H2, s.sc, s.env)
    s.k = svgf.SvgfChecker(lib, W2, H2, s.den)
    _fresh_history(s, f)


def renderer_lib():
    from restir_amd import renderer
    return renderer.hip_lib()


def test_no_trace_in_default_mode(lib):
    """A context that rendered SVGF frames and switched back to the A-Trous chain computes what a fresh context computes, and a context that never
    used SVGF holds no history"""
    name, kind, scale, env_size, W, H = SCENES[1]
    a = Setup(lib, kind, scale, env_size, W, H, overlap=2)
    b = Setup(lib, kind, scale, env_size, W, H, overlap=2, den=abi.Denoiser())
    buf = np.zeros((H, W, 4), dtype=np.float32)
    for s in (a, b):   # nothing allocated before the first SVGF frame
        assert renderer_lib().rt_denoiser_readback(s.r._h, 0, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == abi.ERR_NO_TARGET
    for f in range(3):
        a.frame(f, cpu=False); b.frame(f, cpu=False)
    a.r.set_denoiser(abi.Denoiser())
    for f in range(3, 6):
        a.frame(f, cpu=False); b.frame(f, cpu=False)
    bufs = frame_buffers(5) + [abi.BUF_DIRECT_RESULT0, abi.BUF_INDIRECT_RESULT0, abi.BUF_GBUFFER0]
    for buf_id in bufs:
        x, y = a.r.readback(buf_id).view(np.uint32), b.r.readback(buf_id).view(np.uint32)
        assert np.array_equal(x, y), abi.BUFFER_NAMES[buf_id]
    assert renderer_lib().rt_denoiser_readback(b.r._h, 0, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == abi.ERR_NO_TARGET


def test_error_paths(lib):
    name, kind, scale, env_size, W, H = SCENES[0]
    s = Setup(lib, kind, scale, env_size, W, H, overlap=0)
    L = renderer_lib()
    h = s.r._h
    good = s.r.get_denoiser()
    assert bytes(good) == bytes(s.den)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=2), dict(mode=-1), dict(alphaColor=0.0), dict(alphaColor=1.5), dict(alphaColor=nan), dict(alphaMoments=0.0), dict(alphaMoments=-0.1),
                dict(historyCap=0), dict(phiLumDirect=0.0), dict(phiLumDirect=inf), dict(phiLumIndirect=-1.0), dict(phiLumIndirect=nan)):
        d = abi.Denoiser(**dict(dict(mode=abi.DENOISER_SVGF, alphaColor=0.5, alphaMoments=0.5, historyCap=8, phiLumDirect=2.0, phiLumIndirect=2.0), **bad))
        assert L.rt_set_denoiser(h, C.byref(d)) == -1, bad
        assert bytes(s.r.get_denoiser()) == bytes(good), bad
    d = abi.Denoiser(mode=abi.DENOISER_SVGF)
    d.reserved[1] = 1
    assert L.rt_set_denoiser(h, C.byref(d)) == -1 and bytes(s.r.get_denoiser()) == bytes(good)
    assert L.rt_set_denoiser(h, None) == -1
    # the denoise stages are the A-Trous chain: rejected in SVGF mode, the other stages run
    s.st.time = 1000
    s.r.set_camera(s.camera(0))
    s.r.run_stage(s.st, 0, abi.STAGE_DIRECT)
    for stage in (abi.STAGE_DENOISE_DIRECT, abi.STAGE_DENOISE_INDIRECT):
        assert L.rt_run_stage(h, C.byref(s.st), 0, stage, 0, 0, 0) == -1
        assert b"SVGF" in L.rt_last_error(h)
    s.r.set_denoiser(abi.Denoiser())
    for stage, levels in ((abi.STAGE_DENOISE_DIRECT, 4), (abi.STAGE_DENOISE_INDIRECT, 5)):
        for lv in range(levels):
            assert L.rt_run_stage(h, C.byref(s.st), 0, stage, lv, 0, 0) == 0
    buf = np.zeros(4, dtype=np.float32)
    for which in (-1, 4):
        assert L.rt_denoiser_readback(h, which, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == -1

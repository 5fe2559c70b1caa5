"""ReSTIR GI spatial reuse on the MI355X (rt_set_gi_spatial, csrc/gi_spatial.hip) against its CPU restatement (tests/gi_spatial_checker.cpp) word for word:
the pass's reservoirs, RT_BUF_DENOISE_IND_A and both result images, on four scenes, modes 1 and 2, every schedule, through a moving camera; with both
denoisers; the invariants (mode 0 = never set, samples = 0 = mode off, the temporal reservoir chain and the ray counters untouched); the error paths."""
import ctypes as C
import numpy as np
import pytest
from helpers import abi, host, make_scene
from oracle.binding import Oracle
import gi_spatial
import svgf

pytestmark = pytest.mark.gpu

SKY = dict(in_use=1, haze=0.5, sun_disk_scale=3.0, physically_scaled_sun=0, multiplier=0.02)
# name, kind, scale, env, W, H, sun & sky
SCENES = [
    ("cornell", abi.PROC_CORNELL, 1.0, None, 64, 64, None),
    ("sponza-env", abi.PROC_SPONZA, 0.01, (64, 32), 64, 48, None),
    ("bistro-ext-alpha", abi.PROC_BISTRO_EXT, 0.01, (64, 32), 64, 40, None),   # alpha-masked foliage: visibility rays through cut-outs
    ("sponza-sky", abi.PROC_SPONZA, 0.01, (64, 32), 48, 48, SKY),             # procedural sun & sky
]
N = 6
RESV_BYTES = 76


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return gi_spatial.build(tmp_path_factory.mktemp("gi_spatial"))


@pytest.fixture(scope="module")
def svgf_lib(tmp_path_factory):
    return svgf.build(tmp_path_factory.mktemp("svgf"))


def renderer_lib():
    from restir_amd import renderer
    return renderer.hip_lib()


class Setup:
    def __init__(self, lib, kind, scale, env_size, W, H, sky=None, overlap=0, gis=None, denoise=0, den=None, oracle=True):
        from restir_amd.renderer import Renderer
        self.sc, self.env = make_scene(kind, scale, 1, env_size)
        self.W, self.H = W, H
        self.st = host.default_state(W, H, self.sc, self.env)
        if self.env is None:
            self.st.environmentProb = 0.0
        self.st.denoise = denoise
        self.desc = self.sc.desc(self.env)
        self.gis = gis
        self.r = Renderer().setup(0)
        self.r.set_overlap(overlap)
        self.r.load_scene(self.desc)
        self.r.update(W, H)
        if sky:
            self.r.set_sun_and_sky(abi.SunAndSky(**sky))
        if gis is not None:
            self.r.set_gi_spatial(gis)
        if den is not None:
            self.r.set_denoiser(den)
        self.o = self.k = None
        if oracle:
            self.o = Oracle(0)
            self.o.upload_scene(self.desc)
            self.o.resize(W, H)
            if sky:
                self.o.set_sun_and_sky(abi.SunAndSky(**sky))
            self.k = gi_spatial.GiSpatialChecker(lib, self.desc)
        self.pose = self.sc.cameraPose()

    def camera(self, f):
        eye, center, up, fov = self.pose
        self.sc.setCamera(eye + np.array([0.02 * f, 0.005 * f, -0.015 * f], dtype=np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        return self.sc.getCamera()

    def gpu_frame(self, f):
        self.st.time = 1000 + f
        cam = self.camera(f)
        self.r.set_camera(cam)
        self.r.run(self.st, f)
        return cam

    def oracle_frame(self, f, svgf_checker=None):
        self.st.time = 1000 + f
        cam = self.camera(f)
        self.o.set_camera(cam)
        return gi_spatial.oracle_frame(self.o, self.k, self.st, cam, f, self.gis, svgf_checker)


def _ind_a(buf, W, H):
    return np.ascontiguousarray(buf).view(np.float32)[:W * H * 4].reshape(H, W, 4)


def _diff(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)
    return int((a != b).sum())


def _compare_frame(s, f):
    """after frame f on both sides: the pass's reservoirs, IND_A (denoise == 0) and both result images against the oracle + checker"""
    cur = f & 1
    bad = {}
    for b in (abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESV0 + cur, abi.BUF_GBUFFER0 + cur):
        d = _diff(s.r.readback(b), s.o.readback(b))
        if d:
            bad[abi.BUFFER_NAMES[b]] = d
    return bad


@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", [abi.GI_SPATIAL_ON, abi.GI_SPATIAL_VISIBILITY])
@pytest.mark.parametrize("name,kind,scale,env_size,W,H,sky", SCENES, ids=[s[0] for s in SCENES])
def test_bit_exact_denoise_off(lib, name, kind, scale, env_size, W, H, sky, mode, overlap):
    gis = abi.GiSpatial(mode=mode, samples=6, radius=6)
    s = Setup(lib, kind, scale, env_size, W, H, sky, overlap, gis, denoise=0)
    taps_total = 0
    for f in range(N):
        s.gpu_frame(f)
        want_resv, want_img = s.oracle_frame(f)
        bad = _compare_frame(s, f)
        got_resv = s.r.gi_spatial_readback()
        if _diff(got_resv, want_resv):
            bad["gi_spatial_resv"] = _diff(got_resv, want_resv)
        got_a = _ind_a(s.r.readback(abi.BUF_DENOISE_IND_A), W, H)[:H // 2, :W // 2]
        if _diff(got_a, want_img[:H // 2, :W // 2]):
            bad["denoise_ind_a"] = _diff(got_a, want_img[:H // 2, :W // 2])
        # the checker on the GPU's own readbacks: the GPU's noisy IND_A is gone (the pass rewrote it), so the oracle's stands in at the pixels the pass keeps
        cur = f & 1
        out, img, taps = s.k.run(s.st, s.camera(f), gis, s.r.readback(abi.BUF_GBUFFER0 + cur), s.r.readback(abi.BUF_INDIRECT_RESV0 + cur),
                                 s.o.readback(abi.BUF_DENOISE_IND_A))
        if _diff(out, got_resv):
            bad["own_resv"] = _diff(out, got_resv)
        if _diff(img[:H // 2, :W // 2], got_a):
            bad["own_ind_a"] = _diff(img[:H // 2, :W // 2], got_a)
        taps_total += int(taps.sum())
        assert not bad, f"frame {f}: {bad}"
    assert taps_total > 0


@pytest.mark.parametrize("denoiser", ["atrous", "svgf"])
@pytest.mark.parametrize("overlap", [0, 2])
def test_bit_exact_with_denoising(lib, svgf_lib, denoiser, overlap):
    name, kind, scale, env_size, W, H, sky = SCENES[1]
    gis = abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY, samples=5, radius=8)
    den = abi.Denoiser(mode=abi.DENOISER_SVGF if denoiser == "svgf" else abi.DENOISER_ATROUS)
    s = Setup(lib, kind, scale, env_size, W, H, sky, overlap, gis, denoise=1, den=den)
    k2 = svgf.SvgfChecker(svgf_lib, W, H, den) if denoiser == "svgf" else None
    for f in range(N):
        s.gpu_frame(f)
        want_resv, _ = s.oracle_frame(f, k2)
        bad = _compare_frame(s, f)
        got_resv = s.r.gi_spatial_readback()
        if _diff(got_resv, want_resv):
            bad["gi_spatial_resv"] = _diff(got_resv, want_resv)
        assert not bad, f"frame {f}: {bad}"


def _run(s, n):
    for f in range(n):
        s.gpu_frame(f)
    return {b: s.r.readback(b).copy() for b in (abi.BUF_DIRECT_RESULT0 + ((n - 1) & 1), abi.BUF_INDIRECT_RESULT0 + ((n - 1) & 1),
                                                abi.BUF_INDIRECT_RESV0, abi.BUF_INDIRECT_RESV1, abi.BUF_DENOISE_IND_A)}


@pytest.mark.parametrize("overlap", [0, 2])
def test_invariants(lib, overlap):
    name, kind, scale, env_size, W, H, sky = SCENES[2]
    mk = lambda gis, denoise=0: Setup(lib, kind, scale, env_size, W, H, sky, overlap, gis, denoise=denoise, oracle=False)  # noqa: E731
    base = mk(None)
    base.r.set_counting(True)
    ref = _run(base, N)
    c_ref = base.r.counters()
    # mode 0 set explicitly == never set
    m0 = _run(mk(abi.GiSpatial(mode=abi.GI_SPATIAL_OFF, samples=7, radius=3)), N)
    for b in ref:
        assert _diff(m0[b], ref[b]) == 0, abi.BUFFER_NAMES[b]
    # samples = 0: the mode-off images, bit for bit
    for mode in (abi.GI_SPATIAL_ON, abi.GI_SPATIAL_VISIBILITY):
        z = _run(mk(abi.GiSpatial(mode=mode, samples=0)), N)
        for b in ref:
            assert _diff(z[b], ref[b]) == 0, (mode, abi.BUFFER_NAMES[b])
    # the mode on: the temporal reservoir chain and the ray counters do not change, the indirect image does
    on = mk(abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY))
    on.r.set_counting(True)
    got = _run(on, N)
    c_on = on.r.counters()
    for b in (abi.BUF_INDIRECT_RESV0, abi.BUF_INDIRECT_RESV1):
        assert _diff(got[b], ref[b]) == 0, abi.BUFFER_NAMES[b]
    assert _diff(got[abi.BUF_DENOISE_IND_A], ref[abi.BUF_DENOISE_IND_A]) > 0
    for fld in ("closestHitRays", "anyHitRays", "nodesVisited", "trisTested", "hitsShaded", "risCandidates"):
        assert getattr(c_on, fld) == getattr(c_ref, fld), fld
    # with denoising too: mode 0 after the mode was on == a context that never set it
    a = mk(abi.GiSpatial(mode=abi.GI_SPATIAL_ON), denoise=1)
    b = mk(None, denoise=1)
    for f in range(3):
        a.gpu_frame(f); b.gpu_frame(f)
    a.r.set_gi_spatial(abi.GiSpatial())
    for f in range(3, N):
        a.gpu_frame(f); b.gpu_frame(f)
    for buf in (abi.BUF_DIRECT_RESULT0 + ((N - 1) & 1), abi.BUF_INDIRECT_RESULT0 + ((N - 1) & 1), abi.BUF_INDIRECT_RESV0, abi.BUF_INDIRECT_RESV1):
        assert _diff(a.r.readback(buf), b.r.readback(buf)) == 0, abi.BUFFER_NAMES[buf]


def test_error_paths(lib):
    name, kind, scale, env_size, W, H, sky = SCENES[0]
    s = Setup(lib, kind, scale, env_size, W, H, sky, 0, None, oracle=False)
    L = renderer_lib()
    h = s.r._h
    good = s.r.get_gi_spatial()
    assert bytes(good) == bytes(abi.GiSpatial())
    nan, inf = float("nan"), float("inf")
    base = dict(mode=abi.GI_SPATIAL_ON, samples=4, radius=10, normalThreshold=0.9, depthThreshold=0.1, jacobianMax=10.0)
    for bad in (dict(mode=3), dict(mode=-1), dict(samples=-1), dict(samples=17), dict(radius=0), dict(radius=65), dict(normalThreshold=1.01),
                dict(normalThreshold=-1.5), dict(normalThreshold=nan), dict(depthThreshold=0.0), dict(depthThreshold=-0.1), dict(depthThreshold=inf),
                dict(depthThreshold=nan), dict(jacobianMax=0.99), dict(jacobianMax=inf), dict(jacobianMax=nan)):
        g = abi.GiSpatial(**dict(base, **bad))
        assert L.rt_set_gi_spatial(h, C.byref(g)) == abi.ERR_INVALID_ARG, bad
        assert bytes(s.r.get_gi_spatial()) == bytes(good), bad
    for i in range(2):
        g = abi.GiSpatial(**base)
        g.reserved[i] = 1
        assert L.rt_set_gi_spatial(h, C.byref(g)) == abi.ERR_INVALID_ARG and bytes(s.r.get_gi_spatial()) == bytes(good)
    assert L.rt_set_gi_spatial(h, None) == abi.ERR_INVALID_ARG
    # the edges of every range are accepted
    for ok in (dict(samples=0), dict(samples=16), dict(radius=1), dict(radius=64), dict(normalThreshold=-1.0), dict(normalThreshold=1.0), dict(jacobianMax=1.0)):
        g = abi.GiSpatial(**dict(base, **ok))
        assert L.rt_set_gi_spatial(h, C.byref(g)) == 0, ok
        assert bytes(s.r.get_gi_spatial()) == bytes(g)
    s.r.set_gi_spatial(abi.GiSpatial(**base))
    # readback before the first frame with the mode on
    nbytes = (W // 2) * (H // 2) * RESV_BYTES
    buf = np.zeros(nbytes, dtype=np.uint8)
    assert L.rt_gi_spatial_readback(h, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
    # rt_run_stage(RT_STAGE_INDIRECT) with the mode on; the other stages run
    s.st.time = 1000
    s.r.set_camera(s.camera(0))
    s.r.run_stage(s.st, 0, abi.STAGE_DIRECT)
    assert L.rt_run_stage(h, C.byref(s.st), 0, abi.STAGE_INDIRECT, 0, 0, 0) == abi.ERR_INVALID_ARG
    assert b"GI spatial" in L.rt_last_error(h)
    s.gpu_frame(0)
    assert L.rt_gi_spatial_readback(h, buf.ctypes.data, buf.nbytes) == 0
    for wrong in (nbytes - 1, nbytes + RESV_BYTES, 0):
        assert L.rt_gi_spatial_readback(h, buf.ctypes.data, wrong) == abi.ERR_INVALID_ARG, wrong
    assert L.rt_gi_spatial_readback(h, None, nbytes) == abi.ERR_INVALID_ARG
    # after rt_resize: nothing until the next frame with the mode on
    s.r.update(48, 32)
    assert L.rt_gi_spatial_readback(h, buf.ctypes.data, (24 * 16) * RESV_BYTES) == abi.ERR_NO_TARGET
    # mode off: rt_run_stage(RT_STAGE_INDIRECT) runs again
    s.r.set_gi_spatial(abi.GiSpatial())
    s.W, s.H = 48, 32
    s.st = host.default_state(48, 32, s.sc, s.env)
    s.st.environmentProb = 0.0
    s.st.time = 1001
    s.r.set_camera(s.camera(1))
    s.r.run_stage(s.st, 1, abi.STAGE_DIRECT)
    assert L.rt_run_stage(h, C.byref(s.st), 1, abi.STAGE_INDIRECT, 0, 0, 0) == 0

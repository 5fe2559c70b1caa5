"""Reference mode on the MI355X (rt_reference_*, ABI 2.4): the progressive ground-truth path tracer of csrc/reference.hip against its CPU restatement
(tests/refpt_checker.cpp over the oracle's shading library) word for word; split invariance; the reset rules; non-interference with the real-time frame;
exact emitter / miss pixels; the tonemap pass over the means; the error paths."""
import ctypes as C
import numpy as np
import pytest
from helpers import abi, host, make_scene, frame_buffers
import refpt
from refpt import deterministic_pixels

pytestmark = pytest.mark.gpu

SKY = dict(in_use=1, haze=0.5, sun_disk_scale=3.0, physically_scaled_sun=0, multiplier=0.02)
# name, kind, scale, env, W, H, sun & sky
SCENES = [
    ("cornell", abi.PROC_CORNELL, 1.0, None, 64, 64, None),
    ("sponza-env", abi.PROC_SPONZA, 0.01, (64, 32), 64, 48, None),
    ("bistro-ext-alpha", abi.PROC_BISTRO_EXT, 0.01, (64, 32), 64, 40, None),   # alpha-masked foliage: the stochastic alpha test keyed on (seed, triangle)
    ("sponza-sky", abi.PROC_SPONZA, 0.01, (64, 32), 48, 48, SKY),             # procedural sun & sky: reference_sky.hip
]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refpt.build(tmp_path_factory.mktemp("refpt"))


class Setup:
    def __init__(self, lib, kind, scale, env_size, W, H, sky=None, checker=True):
        from restir_amd.renderer import Renderer
        self.sc, self.env = make_scene(kind, scale, 1, env_size)
        self.W, self.H = W, H
        self.st = host.default_state(W, H, self.sc, self.env)
        if self.env is None:
            self.st.environmentProb = 0.0
        self.desc = self.sc.desc(self.env)
        self.sky = abi.SunAndSky(**sky) if sky else None
        self.r = Renderer().setup(0)
        self.r.load_scene(self.desc)
        self.r.update(W, H)
        self.k = refpt.RefChecker(lib, self.desc) if checker else None
        if self.k:
            self.k.resize(W, H)
        if self.sky:
            self.r.set_sun_and_sky(self.sky)
            if self.k:
                self.k.set_sun_and_sky(self.sky)
        self.sc.updateCamera(W, H)
        self.cam = self.sc.getCamera()
        self.r.set_camera(self.cam)
        if self.k:
            self.k.set_camera(self.cam)

    def gpu(self):
        return [self.r.reference_readback(c) for c in range(3)]

    def cpu(self):
        return [self.k.readback(c) for c in range(3)]


def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def mismatch(a, b):
    return [int((x.view(np.uint32) != y.view(np.uint32)).sum()) for x, y in zip(a, b)]


@pytest.mark.parametrize("name,kind,scale,env_size,W,H,sky", SCENES, ids=[s[0] for s in SCENES])
def test_reference_bit_exact_against_cpu_checker(lib, name, kind, scale, env_size, W, H, sky):
    s = Setup(lib, kind, scale, env_size, W, H, sky)
    for max_depth in (1, 4):
        for mis in (0, 1):
            st = abi.RtxState.from_buffer_copy(s.st)
            st.maxDepth, st.MIS = max_depth, mis
            for n in (1, 3, 4):
                s.r.reference_render(st, n)
            s.k.reset()
            s.k.render(st, 8)
            assert s.r.reference_samples() == 8 and s.k.samples() == 8
            g, c = s.gpu(), s.cpu()
            assert same(g, c), f"maxDepth {max_depth} MIS {mis}: mismatching words (direct, indirect, sum) {mismatch(g, c)}"
            assert np.isfinite(g[2]).all() and g[2][..., :3].max() > 0
            if max_depth == 1:
                assert not g[1][..., :3].any()                       # maxDepth 1: the direct stage's integrand alone
            else:
                assert g[1][..., :3].max() > 0


def test_reference_split_invariant_under_every_traversal_mode(lib):
    s = Setup(lib, abi.PROC_BISTRO_EXT, 0.01, (64, 32), 64, 40, checker=False)
    want = None
    for mode in (abi.TRAVERSAL_AUTO, abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY):
        s.r.set_traversal(mode)
        for split in ([1] * 8, [8], [3, 5]):
            s.r.reference_reset()
            for n in split:
                s.r.reference_render(s.st, n)
            assert s.r.reference_samples() == 8
            got = s.gpu()
            if want is None:
                want = got
            assert same(got, want), (mode, split, mismatch(got, want))


def test_reference_reset_rules(lib):
    s = Setup(lib, abi.PROC_SPONZA, 0.01, (64, 32), 48, 32)
    st = abi.RtxState.from_buffer_copy(s.st)
    s.k.render(st, 4)
    four = s.cpu()
    # inputs outside the integral keep accumulating
    s.r.reference_render(st, 2)
    st2 = abi.RtxState.from_buffer_copy(st)
    st2.time += 17; st2.frame += 5; st2.denoise = 1 - st2.denoise; st2.fireflyClampThreshold *= 0.5; st2.ReSTIRState = abi.RESTIR_NONE; st2.accumulate = 1
    s.r.set_camera(s.cam)                                            # the same camera again
    s.r.reference_render(st2, 2)
    assert s.r.reference_samples() == 4 and same(s.gpu(), four)

    def fresh_after(change_gpu, change_cpu, st_new=st, samples=3):
        s.r.reference_render(st, 2)                                      # something accumulated under the old inputs
        change_gpu()
        s.r.reference_render(st_new, samples)
        change_cpu()
        s.k.reset(); s.k.render(st_new, samples)
        assert s.r.reference_samples() == samples
        assert same(s.gpu(), s.cpu())

    # the camera (viewInverse / projInverse): rt_set_camera resets at once
    eye, center, up, fov = s.sc.cameraPose()
    s.sc.setCamera(eye + np.array([0.05, 0.02, -0.03], dtype=np.float32), center, up, fov)
    s.sc.updateCamera(s.W, s.H)
    cam2 = s.sc.getCamera()
    s.r.reference_render(st, 1)
    s.r.set_camera(cam2)
    assert s.r.reference_samples() == 0
    s.r.set_camera(s.cam)
    fresh_after(lambda: s.r.set_camera(cam2), lambda: s.k.set_camera(cam2))
    # the history matrices alone do not reset
    cam3 = abi.SceneCamera.from_buffer_copy(cam2)
    cam3.lastView.m[12] += 1.0; cam3.lastProjView.m[0] *= 1.5; cam3.lastPosition.x += 0.25
    s.r.set_camera(cam3)
    assert s.r.reference_samples() == 3
    # maxDepth / MIS / hdrMultiplier / environmentProb
    for field, value in (("maxDepth", 2), ("MIS", 0), ("hdrMultiplier", 0.5), ("environmentProb", 0.6)):
        st_new = abi.RtxState.from_buffer_copy(st)
        assert getattr(st_new, field) != value, field
        setattr(st_new, field, value)
        fresh_after(lambda: None, lambda: None, st_new)
    # sun & sky, the scene, the size
    fresh_after(lambda: s.r.set_sun_and_sky(abi.SunAndSky(in_use=0)), lambda: s.k.set_sun_and_sky(abi.SunAndSky(in_use=0)))
    fresh_after(lambda: s.r.load_scene(s.desc), lambda: None)
    s.r.reference_render(st, 2)
    s.r.update(32, 24)
    assert s.r.reference_samples() == 0
    st_small = abi.RtxState.from_buffer_copy(st); st_small.size.x, st_small.size.y = 32, 24
    s.r.reference_render(st_small, 2)
    s.k.resize(32, 24); s.k.render(st_small, 2)
    assert same(s.gpu(), s.cpu())
    # rt_reference_reset
    s.r.reference_reset()
    assert s.r.reference_samples() == 0
    s.r.reference_render(st_small, 1)
    s.k.reset(); s.k.render(st_small, 1)
    assert s.r.reference_samples() == 1 and same(s.gpu(), s.cpu())


def test_reference_does_not_disturb_the_realtime_frames():
    """6 frames under the default frames-in-flight schedule, with and without reference calls between them: every frame buffer and the counters are
    identical, and the frames still equal the oracle"""
    from restir_amd.renderer import Renderer
    from oracle.binding import Oracle
    W, H = 96, 64
    sc, env = make_scene(abi.PROC_BISTRO_EXT, 0.01, 1, (64, 32))
    st = host.default_state(W, H, sc, env)
    desc = sc.desc(env)
    plain, mixed = Renderer().setup(0), Renderer().setup(0)
    for r in (plain, mixed):
        r.load_scene(desc); r.update(W, H); r.set_counting(True)
    o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    st_ref = abi.RtxState.from_buffer_copy(st); st_ref.maxDepth = 3
    eye, center, up, fov = sc.cameraPose()
    for f in range(6):
        st.time = 1000 + f
        sc.setCamera(eye + np.array([0.03 * f, 0.0, -0.02 * f], dtype=np.float32), center, up, fov)
        sc.updateCamera(W, H)
        cam = sc.getCamera()
        for r in (plain, mixed):
            r.set_camera(cam)
        o.set_camera(cam)
        mixed.reference_render(st_ref, 1 + (f % 2))
        plain.run(st, f); mixed.run(st, f); o.render_frame(st, f)
        mixed.reference_render(st_ref, 2)                            # queued behind the frame in flight
        if f % 2:
            assert mixed.reference_samples() > 0
            mixed.reference_readback(abi.REF_SUM)
        for buf in frame_buffers(f):
            a, b, c = plain.readback(buf), mixed.readback(buf), o.readback(buf)
            assert np.array_equal(a, b), f"frame {f}: {abi.BUFFER_NAMES[buf]} differs with reference calls interleaved"
            assert np.array_equal(b, c), f"frame {f}: {abi.BUFFER_NAMES[buf]} differs from the oracle"
    ca, cb = plain.counters(), mixed.counters()
    for field in ("closestHitRays", "anyHitRays", "nodesVisited", "trisTested", "hitsShaded", "risCandidates", "framesTimed", "laneRounds", "laneLiveRounds"):
        assert getattr(ca, field) == getattr(cb, field), field
    assert ca.closestHitRays > 0
    assert plain.stream_priorities()["decided"] == mixed.stream_priorities()["decided"]
    plain.destroy(); mixed.destroy()


@pytest.mark.parametrize("name,kind,scale,env_size,W,H,sky", SCENES, ids=[s[0] for s in SCENES])
def test_reference_emitter_and_miss_pixels_exact(lib, name, kind, scale, env_size, W, H, sky):
    s = Setup(lib, kind, scale, env_size, W, H, sky, checker=False)
    s.r.reference_render(s.st, 5)
    d, i, t = s.gpu()
    miss, emit, want = deterministic_pixels(s.desc, s.st, s.cam, W, H, s.sky)
    assert (miss | emit).sum() > 0
    if env_size is not None:
        assert miss.sum() > 0
    m = miss | emit
    assert np.array_equal(d[m][:, :3].view(np.uint32), want[m][:, :3].view(np.uint32))
    assert (i[m][:, :3] == 0).all()
    assert np.array_equal(t[m][:, :3].view(np.uint32), want[m][:, :3].view(np.uint32))


@pytest.mark.parametrize("auto_exposure", [0, 1, 3])
def test_reference_tonemap_equals_oracle_post_pass(lib, auto_exposure):
    from oracle.binding import Oracle
    s = Setup(lib, abi.PROC_SPONZA, 0.01, (64, 32), 64, 48, checker=False)
    s.r.reference_render(s.st, 4)
    d, i = s.r.reference_readback(abi.REF_DIRECT), s.r.reference_readback(abi.REF_INDIRECT)
    o = Oracle(0); o.upload_scene(s.desc); o.resize(s.W, s.H)
    o.upload_history(abi.BUF_DIRECT_RESULT0, d)
    o.upload_history(abi.BUF_INDIRECT_RESULT0, i)
    tm = abi.Tonemapper(autoExposure=auto_exposure, vignette=0.2, saturation=1.1)
    o.tonemap(tm, 0, 0)
    s.r.reference_tonemap(tm)
    a, b = s.r.readback(abi.BUF_LDR), o.readback(abi.BUF_LDR)
    assert np.array_equal(a, b), f"{int((a.view(np.uint32) != b.view(np.uint32)).sum())} LDR pixels differ"
    assert a.view(np.uint32).any()


def test_reference_error_paths():
    from restir_amd.renderer import Renderer, RtError, hip_lib
    L = hip_lib()
    sc, env = make_scene(abi.PROC_CORNELL, 1.0, 1, None)
    W, H = 32, 32
    st = host.default_state(W, H, sc, None)
    desc = sc.desc(None)
    r = Renderer().setup(0)
    buf = np.zeros((H, W, 4), dtype=np.float32)

    def code(rc, text=None):
        if text is not None:
            assert text in L.rt_last_error(r._h).decode(), L.rt_last_error(r._h)
        return rc

    assert code(L.rt_reference_render(r._h, C.byref(st), 1)) == -4                                      # RT_ERR_NO_SCENE
    assert L.rt_upload_scene(r._h, C.byref(desc)) == 0
    assert code(L.rt_reference_render(r._h, C.byref(st), 1)) == -5                                      # RT_ERR_NO_ACCEL
    assert L.rt_build_accel(r._h) == 0
    assert code(L.rt_reference_render(r._h, C.byref(st), 1)) == -6                                      # RT_ERR_NO_TARGET (no rt_resize)
    assert code(L.rt_reference_readback(r._h, 0, buf.ctypes.data, buf.nbytes)) == -6
    assert code(L.rt_reference_tonemap(r._h, C.byref(abi.Tonemapper()))) == -6
    r.update(W, H)
    sc.updateCamera(W, H)
    r.set_camera(sc.getCamera())
    bad = abi.RtxState.from_buffer_copy(st); bad.size.x = W + 8
    assert code(L.rt_reference_render(r._h, C.byref(bad), 1)) == -6                                     # state size != rt_resize
    assert code(L.rt_reference_render(r._h, C.byref(st), -1), "samples") == -1                          # RT_ERR_INVALID_ARG
    dbg = abi.RtxState.from_buffer_copy(st); dbg.debugging_mode = 3
    assert code(L.rt_reference_render(r._h, C.byref(dbg), 1), "debugging_mode") == -1
    assert L.rt_reference_render(None, C.byref(st), 1) == -1 and L.rt_reference_render(r._h, None, 1) == -1
    assert code(L.rt_reference_readback(r._h, 3, buf.ctypes.data, buf.nbytes), "component") == -1
    assert code(L.rt_reference_readback(r._h, -1, buf.ctypes.data, buf.nbytes), "component") == -1
    assert code(L.rt_reference_readback(r._h, 0, buf.ctypes.data, buf.nbytes - 16), "size") == -1
    assert L.rt_reference_readback(r._h, 0, None, buf.nbytes) == -1 and L.rt_reference_tonemap(r._h, None) == -1
    # nothing accumulated yet: the mean of no samples is 0 (a = 1); 0 samples is a valid call
    assert L.rt_reference_render(r._h, C.byref(st), 0) == 0 and r.reference_samples() == 0
    z = r.reference_readback(abi.REF_SUM)
    assert z.shape == (H, W, 4) and z.dtype == np.float32 and not z[..., :3].any() and (z[..., 3] == 1).all()
    with pytest.raises(RtError):
        r.reference_render(dbg, 1)
    r.reference_render(st, 2)
    assert r.reference_samples() == 2 and r.reference_readback(abi.REF_SUM)[..., :3].max() > 0
    r.destroy()

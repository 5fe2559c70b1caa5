"""Temporal anti-aliasing (rt_set_taa) without a GPU: include/rt_abi.h declares the entry points and rt_taa, the product library exports them with the error
convention, rt_taa_jitter_camera (a pure host function) jitters exactly as DESIGN.md §16 states, the jitter leaves the oracle's motion vectors of a static
camera unchanged, and the CPU checker (tests/taa_checker.cpp, which the GPU tests hold the kernel to word for word) agrees with an independent float64 numpy
statement of the resolve on real oracle frames through a camera move, plus hand-built cases."""
import ctypes as C
import os
import re
from fractions import Fraction
import numpy as np
import pytest
from helpers import ROOT, abi, host, make_scene
from oracle.binding import Oracle
from test_denoise_model import INVALID, _geometry, _mat
import taa

NAMES = ("rt_set_taa", "rt_get_taa", "rt_taa_reset", "rt_taa_readback", "rt_taa_jitter_camera")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return taa.build(tmp_path_factory.mktemp("taa"))


def _hip():
    from restir_amd import renderer
    return renderer.hip_lib()


def test_header_declares_the_taa_entry_points():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES[:4]:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert re.search(r"\bint rt_taa_jitter_camera\(const rt_scene_camera\* in", src)
    assert "RT_TAA_OFF = 0" in src and "RT_TAA_ON = 1" in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert C.sizeof(abi.Taa) == 32


def test_library_exports_the_taa_entry_points():
    from restir_amd import renderer
    L = _hip()
    for n in NAMES:
        assert hasattr(L, n) and n in renderer.ABI_SYMBOLS
    t = abi.Taa()
    buf = np.zeros(4, dtype=np.float32)
    assert L.rt_set_taa(None, C.byref(t)) == -1
    assert L.rt_get_taa(None, C.byref(t)) == -1
    assert L.rt_taa_reset(None) == -1
    assert L.rt_taa_readback(None, 0, buf.ctypes.data, buf.nbytes) == -1
    cam = abi.SceneCamera()
    out = abi.SceneCamera()
    for bad in ((None, 0, 8, 4, 4, C.byref(out)), (C.byref(cam), 0, 8, 4, 4, None), (C.byref(cam), 0, 17, 4, 4, C.byref(out)),
                (C.byref(cam), 0, -1, 4, 4, C.byref(out)), (C.byref(cam), 0, 8, 0, 4, C.byref(out)), (C.byref(cam), 0, 8, 4, 0, C.byref(out))):
        assert L.rt_taa_jitter_camera(*bad) == abi.ERR_INVALID_ARG


def _radical_inverse(k, b):
    r, f = Fraction(0), Fraction(1, b)
    while k:
        r += f * (k % b)
        k //= b
        f /= b
    return r


def _camera(W=64, H=48):
    sc, _ = make_scene(abi.PROC_SPONZA, 0.01, 1, None)
    sc.updateCamera(W, H)
    sc.updateCamera(W, H)
    return sc.getCamera()


def test_jitter_camera_halton_offsets_and_untouched_fields():
    W, H = 64, 48
    cam = _camera(W, H)
    raw = bytes(cam)
    pi = np.array(list(cam.projInverse.m), dtype=np.float32)
    seen = set()
    for phases in range(1, 17):
        for frames in range(-3, 2 * phases + 3):
            k = frames % phases + 1
            dx = np.float32(float(_radical_inverse(k, 2)) - 0.5)
            dy = np.float32(float(_radical_inverse(k, 3)) - 0.5)
            assert abs(dx) < 0.5 and abs(dy) < 0.5 and max(abs(dx), abs(dy)) <= 0.46875
            ox = np.float32(np.float32(2.0) * dx) / np.float32(W)
            oy = np.float32(np.float32(2.0) * dy) / np.float32(H)
            want = pi.copy()
            for r in range(4):
                want[12 + r] = np.float32(np.float32(pi[12 + r] + np.float32(pi[r] * ox)) + np.float32(pi[4 + r] * oy))
            out = taa.jitter_camera(cam, frames, phases, W, H)
            got = np.array(list(out.projInverse.m), dtype=np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (phases, frames)
            # only the translation column of projInverse changes
            ob = bytes(out)
            off = abi.SceneCamera.projInverse.offset
            assert ob[:off + 48] == raw[:off + 48] and ob[off + 64:] == raw[off + 64:]
            seen.add((float(dx), float(dy)))
    assert len(seen) == 16
    # the first values of the Halton (2, 3) sequence
    out = taa.jitter_camera(cam, 0, 8, W, H)
    assert bytes(out) != raw
    for frames, (hx, hy) in enumerate([(0.5, 1 / 3), (0.25, 2 / 3), (0.75, 1 / 9), (0.125, 4 / 9)]):
        assert float(_radical_inverse(frames + 1, 2)) == hx and abs(float(_radical_inverse(frames + 1, 3)) - hy) < 1e-15
    # jitterPhases = 0: the input bits
    for frames in (0, 5, -7):
        assert bytes(taa.jitter_camera(cam, frames, 0, W, H)) == raw


def _surface(o, f, W, H):
    g = o.readback(abi.BUF_GBUFFER0 + (f & 1)).view(np.uint32).reshape(H, W, 4)
    return (g[..., 3] & np.uint32(INVALID)) != INVALID


@pytest.mark.parametrize("kind,scale,env", [(abi.PROC_CORNELL, 1.0, None), (abi.PROC_SPONZA, 0.01, (64, 32)), (abi.PROC_BISTRO_EXT, 0.01, (64, 32))],
                         ids=["cornell", "sponza", "bistro"])
def test_static_camera_motion_ignores_the_jitter(kind, scale, env):
    W, H = 48, 32
    sc, e = make_scene(kind, scale, 1, env)
    st = host.default_state(W, H, sc, e)
    if e is None:
        st.environmentProb = 0.0
    desc = sc.desc(e)
    a, b = Oracle(0), Oracle(0)
    for o in (a, b):
        o.upload_scene(desc)
        o.resize(W, H)
    for f in range(3):
        st.time = 1000 + f
        sc.updateCamera(W, H)
        cam = sc.getCamera()
        a.set_camera(cam)
        b.set_camera(taa.jitter_camera(cam, f, 16, W, H))
        a.run_stage(st, f, abi.STAGE_DIRECT)
        b.run_stage(st, f, abi.STAGE_DIRECT)
        # wherever both rays hit a surface (a jittered ray at a silhouette may miss, and the stage stores no motion for a miss)
        both = _surface(a, f, W, H) & _surface(b, f, W, H)
        assert both.mean() > 0.3
        ma = a.readback(abi.BUF_MOTION).view(np.int16).reshape(H, W, 2)
        mb = b.readback(abi.BUF_MOTION).view(np.int16).reshape(H, W, 2)
        assert np.array_equal(ma[both], mb[both]), (f, int((ma[both] != mb[both]).sum()))
    # ... while the frame itself does change
    assert not np.array_equal(a.readback(abi.BUF_GBUFFER0), b.readback(abi.BUF_GBUFFER0)) or \
        not np.array_equal(a.readback(abi.BUF_DIRECT_RESULT0), b.readback(abi.BUF_DIRECT_RESULT0))


# ---- float64 model of one resolve -------------------------------------------------------------------------------------------------------------------------
def _ycocg(c):
    return np.stack([0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2], 0.5 * c[..., 0] - 0.5 * c[..., 2],
                     -0.25 * c[..., 0] + 0.5 * c[..., 1] - 0.25 * c[..., 2]], -1)


def _rgb(v):
    return np.stack([v[..., 0] + v[..., 1] - v[..., 2], v[..., 0] + v[..., 2], v[..., 0] - v[..., 1] - v[..., 2]], -1)


def _cr(t):
    return [t * (-0.5 + t * (1 - 0.5 * t)), 1 + t * t * (-2.5 + 1.5 * t), t * (0.5 + t * (2 - 1.5 * t)), t * t * (-0.5 + 0.5 * t)]


def model_resolve(cam, taa_s, hist_ok, g, gl, cd, ci, pD, pI, pN):
    """returns (D, I, n, consistent, borderline) in float64; borderline marks pixels whose consistency decision is within rounding of a threshold"""
    H, W = g.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    nrm, pos, mat = _geometry(g, cam, xx, yy, (W, H))
    valid = mat != INVALID
    lpv = _mat(cam.lastProjView)
    with np.errstate(invalid="ignore", over="ignore"):
        clip = np.concatenate([pos, np.ones((H, W, 1))], -1) @ lpv.T
        s = np.stack([(clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * W, (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * H], -1)
    s = np.where(np.isfinite(s) & valid[..., None], s, -1.0)   # (sky pixels: no history, their s never reaches an image index)
    q = np.floor(s)
    inb = (q[..., 0] >= 0) & (q[..., 1] >= 0) & (q[..., 0] < W) & (q[..., 1] < H)
    qx, qy = np.clip(q[..., 0], 0, W - 1).astype(int), np.clip(q[..., 1], 0, H - 1).astype(int)
    pn, _, pmat = _geometry(gl, cam, qx, qy, (W, H))
    pdepth = gl[qy, qx, 0].view(np.float32).astype(np.float64)
    lp = np.array([cam.lastPosition.x, cam.lastPosition.y, cam.lastPosition.z])
    reproj = np.linalg.norm(lp - pos, axis=-1)
    ndot = (nrm * pn).sum(-1)
    cons = hist_ok & valid & inb & (pmat == mat) & (ndot > 0.9) & (reproj < pdepth * 1.05)
    frac = s - np.round(s)
    border = valid & hist_ok & ((np.abs(frac) < 1e-3).any(-1) | (np.abs(ndot - 0.9) < 1e-4) | (np.abs(reproj - pdepth * 1.05) < 1e-4 * pdepth))
    n = np.where(cons, np.minimum(pN[qy, qx] + 1, 1024), 1)
    a = np.maximum(np.float64(np.float32(taa_s.alpha)), 1.0 / n)[..., None]
    t = s - 0.5
    b = np.floor(t)
    wx, wy = _cr(t[..., 0] - b[..., 0]), _cr(t[..., 1] - b[..., 1])
    outs = []
    for cur, prev in ((cd, pD), (ci, pI)):
        c = cur[..., :3]
        h = np.zeros((H, W, 3))
        for j in range(4):
            ty = np.clip(b[..., 1].astype(int) - 1 + j, 0, H - 1)
            for i in range(4):
                tx = np.clip(b[..., 0].astype(int) - 1 + i, 0, W - 1)
                h += prev[ty, tx, :3] * (wx[i] * wy[j])[..., None]
        v = _ycocg(c)
        s1, s2, cnt = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 1))
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                ok = ((xx + i >= 0) & (xx + i < W) & (yy + j >= 0) & (yy + j < H))[..., None]
                vq = v[np.clip(yy + j, 0, H - 1), np.clip(xx + i, 0, W - 1)]
                s1 += np.where(ok, vq, 0.0); s2 += np.where(ok, vq * vq, 0.0); cnt += ok
        mu = s1 / cnt
        sigma = np.sqrt(np.maximum(s2 / cnt - mu * mu, 0.0))
        d = _ycocg(h) - mu
        e = sigma * np.float64(np.float32(taa_s.clipGamma))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.abs(d) > e, np.abs(d) / e, 1.0)
        tt = np.maximum(ratio.max(-1, keepdims=True), 1.0)
        hc = _rgb(np.where(np.isinf(tt), mu, mu + d / tt))
        out = np.concatenate([hc * (1 - a) + c * a, np.ones((H, W, 1))], -1)
        out = np.where(cons[..., None], out, np.concatenate([c, np.ones((H, W, 1))], -1))
        out = np.where(valid[..., None], out, cur)
        outs.append(out)
    return outs[0], outs[1], np.where(valid, n, 1), cons, border


def check_model(lib, W, H, border_pixels=None):
    """the checker against model_resolve over five frames of a moving camera at W x H; returns what the frames exercised.  The cap on the pixels left out as
    borderline is 5 % of the image, or `border_pixels` (an absolute count, for images of a few pixels: tests/test_optin_shapes_cpu.py)"""
    sc, env = make_scene(abi.PROC_SPONZA, 0.01, 1, (64, 32))
    st = host.default_state(W, H, sc, env)
    o = Oracle(0); o.upload_scene(sc.desc(env)); o.resize(W, H)
    t = abi.Taa(mode=abi.TAA_ON, alpha=0.2, clipGamma=1.25)
    k = taa.TaaChecker(lib, W, H, t)
    eye, center, up, fov = sc.cameraPose()
    accepted = rejected = clipped = 0
    for f in range(5):   # a camera move at every frame: the history follows the reprojection; frames 1.. accept most pixels
        st.time = 300 + f
        sc.setCamera(eye + np.array([0.01 * f, 0.0, -0.01 * f], dtype=np.float32), center, up, fov)
        sc.updateCamera(W, H)
        prev = [x.copy() for x in (k.D[(f + 1) & 1], k.I[(f + 1) & 1], k.N[(f + 1) & 1])]
        hist_ok = k.valid and k.last == ((f + 1) & 1)
        jc, d, i, n = taa.oracle_frame(o, k, st, sc.getCamera(), f, t.jitterPhases)
        cur = f & 1
        g = o.readback(abi.BUF_GBUFFER0 + cur).view(np.uint32).reshape(H, W, 4)
        gl = o.readback(abi.BUF_GBUFFER0 + 1 - cur).view(np.uint32).reshape(H, W, 4)
        cd = o.readback(abi.BUF_DIRECT_RESULT0 + cur).view(np.float32).reshape(H, W, 4).astype(np.float64)
        ci = o.readback(abi.BUF_INDIRECT_RESULT0 + cur).view(np.float32).reshape(H, W, 4).astype(np.float64)
        mD, mI, mn, cons, border = model_resolve(jc, t, hist_ok, g, gl, cd, ci, *[p.astype(np.float64) for p in prev])
        ok = ~border
        if border_pixels is None:
            assert border.mean() < 0.05, f
        else:
            assert border.sum() <= border_pixels, (f, int(border.sum()))
        assert np.array_equal(k.consistent[ok], cons[ok]), (f, int((k.consistent[ok] != cons[ok]).sum()))
        assert np.array_equal(n[ok], mn[ok].astype(np.float32)), f
        for got, want, what in ((d, mD, "direct"), (i, mI, "indirect")):
            scale = np.abs(want[..., :3]).max()
            err = np.abs(got[ok] - want[ok]) - (2e-4 * np.abs(want[ok]) + 1e-5 * scale + 1e-7)
            assert (err <= 0).all(), (what, f, float(err.max()))
        if f > 0:
            accepted += int((n > 1).sum()); rejected += int((n == 1).sum())
            box = np.abs(d[..., :3] - cd[..., :3]).sum(-1) > 0
            clipped += int(box.sum())
    return dict(accepted=accepted, rejected=rejected, clipped=clipped, peak=float(d[..., :3].max()))


def test_checker_matches_an_independent_model(lib):
    W, H = 48, 32
    got = check_model(lib, W, H)
    assert got["accepted"] > W * H and got["rejected"] > 0 and got["clipped"] > 0
    assert got["peak"] > 0


def _flat_frame(W, H, hash_=0x01000000, depth=1.0):
    g = np.zeros((H, W, 4), np.uint32)
    g[..., 0] = np.float32(depth).view(np.uint32)
    g[..., 3] = hash_
    return g


def test_hand_cases(lib):
    # Catmull-Rom weights sum to 1 (to rounding) and interpolate at the integer positions
    w = np.zeros(4, np.float32)
    for fr in np.linspace(0, 1, 33, dtype=np.float32)[:-1]:
        lib.taa_catmull_rom(C.c_float(fr), w.ctypes.data)
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6, fr
    lib.taa_catmull_rom(C.c_float(0.0), w.ctypes.data)
    assert list(w) == [0.0, 1.0, 0.0, 0.0]
    # YCoCg round trip
    rgb = np.array([0.3, 0.6, 0.1], np.float32)
    v, back = np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib.taa_ycocg(rgb.ctypes.data, v.ctypes.data, 0)
    lib.taa_ycocg(v.ctypes.data, back.ctypes.data, 1)
    assert np.allclose(back, rgb, atol=1e-7)
    # the clip: inside the box untouched (bit for bit), outside onto the box surface along the segment towards mu
    mu, sig = np.array([0.5, 0.1, -0.1], np.float32), np.array([0.1, 0.05, 0.02], np.float32)
    out = np.zeros(3, np.float32)
    inside = np.array([0.55, 0.12, -0.11], np.float32)
    lib.taa_clip(inside.ctypes.data, mu.ctypes.data, sig.ctypes.data, C.c_float(1.0), out.ctypes.data)
    assert np.array_equal(out.view(np.uint32), inside.view(np.uint32))
    outside = np.array([0.9, 0.1, -0.1], np.float32)
    for gamma in (1.0, 2.0):
        lib.taa_clip(outside.ctypes.data, mu.ctypes.data, sig.ctypes.data, C.c_float(gamma), out.ctypes.data)
        d = (out - mu).astype(np.float64) / (gamma * sig)
        assert abs(np.abs(d).max() - 1.0) < 1e-5, gamma                    # on the surface
        dir0 = (outside - mu) / np.linalg.norm(outside - mu)
        dir1 = (out - mu) / np.linalg.norm(out - mu)
        assert np.allclose(dir0, dir1, atol=1e-6)                          # along the segment, not a per-channel clamp
    # a static frame pair: accumulation, alpha = 1, disocclusion
    W, H = 16, 12
    cam = _camera(W, H)
    g = _flat_frame(W, H)
    lastg = g.copy()
    rng = np.random.default_rng(3)
    cur = rng.uniform(0.1, 1.0, (H, W, 4)).astype(np.float32)
    for alpha in (1.0, 0.1):
        k = taa.TaaChecker(lib, W, H, abi.Taa(mode=abi.TAA_ON, alpha=alpha))
        d0, _, n0 = k.frame(cam, 0, g, lastg, cur, cur)
        assert (n0 == 1).all() and np.array_equal(d0[..., :3], cur[..., :3])
        k.frame(cam, 1, g, lastg, cur * 0.5, cur * 0.5)
        assert k.consistent.all() and (k.N[1] == 2).all()   # a static camera over a flat surface: every pixel keeps its history
        if alpha == 1.0:
            assert np.array_equal(k.D[1][..., :3], (cur * 0.5)[..., :3])
    # a different material hash in the previous G-buffer: no history anywhere (disocclusion resets n)
    k = taa.TaaChecker(lib, W, H)
    k.frame(cam, 0, g, lastg, cur, cur)
    _, _, n1 = k.frame(cam, 1, g, _flat_frame(W, H, 0x02000000), cur, cur)
    assert (n1 == 1).all()
    # invalid material: pass through with n = 1
    bad = _flat_frame(W, H, INVALID)
    d2, i2, n2 = k.frame(cam, 2, bad, g, cur, cur * 2)
    assert np.array_equal(d2, cur) and np.array_equal(i2, cur * 2) and (n2 == 1).all()

"""Temporal upsampling (rt_set_upscale) without a GPU: include/rt_abi.h declares the entry points and rt_upscale, the product library exports them with the error
convention, rt_upscale_jitter_camera (a pure host function) shares rt_taa_jitter_camera's arithmetic and returns the offset it applied, and the CPU checker
(tests/upscale_checker.cpp, which the GPU tests hold the kernel to word for word) agrees with an independent float64 numpy statement of the resolve on real
oracle frames through a camera move, plus hand-built cases and the property that justifies the feature: accumulating jittered low-resolution frames gets closer
to the image at the output resolution than interpolating one frame does."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from helpers import ROOT, abi, host, make_scene
from oracle.binding import Oracle
from test_denoise_model import INVALID, _geometry, _mat
from test_taa_cpu import _camera, _cr, _flat_frame, _radical_inverse, _rgb, _ycocg
import taa
import upscale

NAMES = ("rt_set_upscale", "rt_get_upscale", "rt_upscale_reset", "rt_upscale_readback", "rt_upscale_tonemap", "rt_upscale_jitter_camera")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return upscale.build(tmp_path_factory.mktemp("upscale"))


def _hip():
    from restir_amd import renderer
    return renderer.hip_lib()


def test_header_declares_the_upscale_entry_points():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES[:5]:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert re.search(r"\bint rt_upscale_jitter_camera\(const rt_scene_camera\* in", src)
    assert "RT_UPSCALE_OFF = 0" in src and "RT_UPSCALE_TEMPORAL = 1" in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert C.sizeof(abi.Upscale) == 32
    u = abi.Upscale()
    assert (u.mode, u.outWidth, u.outHeight, u.jitterPhases, u.reserved[0], u.reserved[1]) == (0, 0, 0, 16, 0, 0)
    assert u.alpha == np.float32(0.1) and u.clipGamma == 1.0


def test_library_exports_the_upscale_entry_points():
    from restir_amd import renderer
    L = _hip()
    for n in NAMES:
        assert hasattr(L, n) and n in renderer.ABI_SYMBOLS
    u = abi.Upscale()
    tm = abi.Tonemapper()
    buf = np.zeros(4, dtype=np.float32)
    assert L.rt_set_upscale(None, C.byref(u)) == -1
    assert L.rt_get_upscale(None, C.byref(u)) == -1
    assert L.rt_upscale_reset(None) == -1
    assert L.rt_upscale_readback(None, 0, buf.ctypes.data, buf.nbytes) == -1
    assert L.rt_upscale_tonemap(None, C.byref(tm), 0) == -1
    cam, out = abi.SceneCamera(), abi.SceneCamera()
    for bad in ((None, 0, 8, 4, 4, C.byref(out), None), (C.byref(cam), 0, 8, 4, 4, None, None), (C.byref(cam), 0, 65, 4, 4, C.byref(out), None),
                (C.byref(cam), 0, -1, 4, 4, C.byref(out), None), (C.byref(cam), 0, 8, 0, 4, C.byref(out), None), (C.byref(cam), 0, 8, 4, 0, C.byref(out), None)):
        assert L.rt_upscale_jitter_camera(*bad) == abi.ERR_INVALID_ARG
    assert L.rt_upscale_jitter_camera(C.byref(cam), 3, 64, 4, 4, C.byref(out), None) == 0   # delta may be NULL
    # rt_taa_jitter_camera keeps its range
    assert L.rt_taa_jitter_camera(C.byref(cam), 0, 17, 4, 4, C.byref(out)) == abi.ERR_INVALID_ARG


def test_jitter_camera_shares_taa_arithmetic_and_returns_the_offset():
    W, H = 37, 27
    cam = _camera(W, H)
    raw = bytes(cam)
    pi = np.array(list(cam.projInverse.m), dtype=np.float32)
    for phases in range(1, 65):
        for frames in list(range(-2, phases + 2)) if phases <= 16 else (-1, 0, 1, phases // 2, phases - 1, phases, phases + 1):
            out, delta = upscale.jitter_camera(cam, frames, phases, W, H)
            if phases <= 16:   # the camera bits are rt_taa_jitter_camera's
                assert bytes(out) == bytes(taa.jitter_camera(cam, frames, phases, W, H)), (phases, frames)
            k = frames % phases + 1
            dx = np.float32(float(_radical_inverse(k, 2)) - 0.5)
            dy = np.float32(float(_radical_inverse(k, 3)) - 0.5)
            assert delta.dtype == np.float32 and delta[0] == dx and delta[1] == dy, (phases, frames)
            assert abs(float(delta[0])) < 0.5 and abs(float(delta[1])) < 0.5
            # the returned delta reproduces the projInverse translation column bit for bit
            ox = np.float32(np.float32(2.0) * delta[0]) / np.float32(W)
            oy = np.float32(np.float32(2.0) * delta[1]) / np.float32(H)
            want = pi.copy()
            for r in range(4):
                want[12 + r] = np.float32(np.float32(pi[12 + r] + np.float32(pi[r] * ox)) + np.float32(pi[4 + r] * oy))
            got = np.array(list(out.projInverse.m), dtype=np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (phases, frames)
            ob = bytes(out)
            off = abi.SceneCamera.projInverse.offset
            assert ob[:off + 48] == raw[:off + 48] and ob[off + 64:] == raw[off + 64:]
    # 0 phases: the input bits and a zero offset
    for frames in (0, 5, -7):
        out, delta = upscale.jitter_camera(cam, frames, 0, W, H)
        assert bytes(out) == raw and delta[0] == 0 and delta[1] == 0


# ---- float64 model of one resolve -------------------------------------------------------------------------------------------------------------------------
def model_resolve(cam, delta, u_s, hist_ok, g, gl, cd, ci, pD, pI, pN):
    """returns (D, I, n, consistent, borderline) in float64 at the output size; borderline marks pixels whose nearest-sample choice, consistency decision or
    history pixel is within rounding of a floor boundary or a threshold"""
    H, W = g.shape[:2]
    Ho, Wo = pN.shape
    oy, ox = np.mgrid[0:Ho, 0:Wo]
    rho = np.array([W / Wo, H / Ho])
    d = np.array([float(delta[0]), float(delta[1])])
    u = np.stack([(ox + 0.5) * rho[0], (oy + 0.5) * rho[1]], -1)
    t = u - d
    near_p = np.abs(t - np.round(t))
    inside = (t > 0) & (t < np.array([W, H]))   # (a floor boundary outside the image is clamped away)
    border = (((near_p > 0) & (near_p < 1e-4)) & inside).any(-1)   # (an exact integer is exact in fp32 too: dyadic ratios with dyadic offsets)
    p = np.clip(np.floor(t), 0, [W - 1, H - 1]).astype(int)
    px, py = p[..., 0], p[..., 1]
    e = u - (p + 0.5 + d)
    nrm, pos, mat = _geometry(g, cam, px, py, (W, H))
    valid = mat != INVALID
    lpv = _mat(cam.lastProjView)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        clip = np.concatenate([pos, np.ones((Ho, Wo, 1))], -1) @ lpv.T
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
    so = (s + e) / rho
    ho = np.floor(so)
    inbo = (ho[..., 0] >= 0) & (ho[..., 1] >= 0) & (ho[..., 0] < Wo) & (ho[..., 1] < Ho)
    hx, hy = np.clip(ho[..., 0], 0, Wo - 1).astype(int), np.clip(ho[..., 1], 0, Ho - 1).astype(int)
    cons = hist_ok & valid & inb & inbo & (pmat == mat) & (ndot > 0.9) & (reproj < pdepth * 1.05)
    border |= valid & hist_ok & ((np.abs(s - np.round(s)) < 1e-3).any(-1) | (np.abs(so - np.round(so)) < 1e-3).any(-1) | (np.abs(ndot - 0.9) < 1e-4) |
                                 (np.abs(reproj - pdepth * 1.05) < 1e-4 * pdepth))
    n = np.where(cons, np.minimum(pN[hy, hx] + 1, 1024), 1)
    kappa = np.maximum(0, 1 - np.abs(e[..., 0]) / rho[0]) * np.maximum(0, 1 - np.abs(e[..., 1]) / rho[1])
    a = np.maximum(np.float64(np.float32(u_s.alpha)) * kappa, 1.0 / n)[..., None]
    tt = so - 0.5
    b = np.floor(tt)
    wx, wy = _cr(tt[..., 0] - b[..., 0]), _cr(tt[..., 1] - b[..., 1])
    yy, xx = np.mgrid[0:H, 0:W]
    outs = []
    for cur, prev in ((cd, pD), (ci, pI)):
        c = cur[py, px, :3]
        h = np.zeros((Ho, Wo, 3))
        for j in range(4):
            ty = np.clip(b[..., 1].astype(int) - 1 + j, 0, Ho - 1)
            for i in range(4):
                tx = np.clip(b[..., 0].astype(int) - 1 + i, 0, Wo - 1)
                h += prev[ty, tx, :3] * (wx[i] * wy[j])[..., None]
        v = _ycocg(cur[..., :3])
        s1, s2, cnt = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 1))
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                ok = ((xx + i >= 0) & (xx + i < W) & (yy + j >= 0) & (yy + j < H))[..., None]
                vq = v[np.clip(yy + j, 0, H - 1), np.clip(xx + i, 0, W - 1)]
                s1 += np.where(ok, vq, 0.0); s2 += np.where(ok, vq * vq, 0.0); cnt += ok
        mu_r = s1 / cnt
        sigma_r = np.sqrt(np.maximum(s2 / cnt - mu_r * mu_r, 0.0))
        mu, sigma = mu_r[py, px], sigma_r[py, px]   # the render-size box of p
        dd = _ycocg(h) - mu
        ee = sigma * np.float64(np.float32(u_s.clipGamma))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.abs(dd) > ee, np.abs(dd) / ee, 1.0)
        tq = np.maximum(ratio.max(-1, keepdims=True), 1.0)
        with np.errstate(invalid="ignore"):
            hc = _rgb(np.where(np.isinf(tq), mu, mu + dd / tq))
        out = np.concatenate([hc * (1 - a) + c * a, np.ones((Ho, Wo, 1))], -1)
        out = np.where(cons[..., None], out, np.concatenate([c, np.ones((Ho, Wo, 1))], -1))
        out = np.where(valid[..., None], out, cur[py, px])
        outs.append(out)
    return outs[0], outs[1], np.where(valid, n, 1), cons, border


def check_model(lib, W, H, Wo, Ho):
    """the checker against model_resolve over five frames of a moving camera, W x H -> Wo x Ho; returns what the frames exercised"""
    sc, env = make_scene(abi.PROC_SPONZA, 0.01, 1, (64, 32))
    st = host.default_state(W, H, sc, env)
    o = Oracle(0); o.upload_scene(sc.desc(env)); o.resize(W, H)
    u = abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=Wo, outHeight=Ho, alpha=0.2, clipGamma=1.25)
    k = upscale.UpscaleChecker(lib, W, H, u)
    eye, center, up, fov = sc.cameraPose()
    accepted = rejected = clipped = 0
    worst = 0.0
    for f in range(5):   # a camera move at every frame: the history follows the reprojection; frames 1.. accept most pixels
        st.time = 300 + f
        sc.setCamera(eye + np.array([0.01 * f, 0.0, -0.01 * f], dtype=np.float32), center, up, fov)
        sc.updateCamera(W, H)
        prev = [x.copy() for x in (k.D[(f + 1) & 1], k.I[(f + 1) & 1], k.N[(f + 1) & 1])]
        hist_ok = k.valid and k.last == ((f + 1) & 1)
        jc, delta, d, i, n = upscale.oracle_frame(o, k, st, sc.getCamera(), f)
        cur = f & 1
        g = o.readback(abi.BUF_GBUFFER0 + cur).view(np.uint32).reshape(H, W, 4)
        gl = o.readback(abi.BUF_GBUFFER0 + 1 - cur).view(np.uint32).reshape(H, W, 4)
        cd = o.readback(abi.BUF_DIRECT_RESULT0 + cur).view(np.float32).reshape(H, W, 4).astype(np.float64)
        ci = o.readback(abi.BUF_INDIRECT_RESULT0 + cur).view(np.float32).reshape(H, W, 4).astype(np.float64)
        mD, mI, mn, cons, border = model_resolve(jc, delta, u, hist_ok, g, gl, cd, ci, *[p.astype(np.float64) for p in prev])
        ok = ~border
        worst = max(worst, float(border.mean()))
        assert border.mean() < 0.05, (f, float(border.mean()))
        assert np.array_equal(k.consistent[ok], cons[ok]), (f, int((k.consistent[ok] != cons[ok]).sum()))
        assert np.array_equal(n[ok], mn[ok].astype(np.float32)), f
        for got, want, what in ((d, mD, "direct"), (i, mI, "indirect")):
            scale = np.abs(want[..., :3]).max()
            err = np.abs(got[ok] - want[ok]) - (2e-4 * np.abs(want[ok]) + 1e-5 * scale + 1e-7)
            assert (err <= 0).all(), (what, f, float(err.max()))
        if f > 0:
            accepted += int((n > 1).sum()); rejected += int((n == 1).sum())
            near = cd[np.clip(np.floor(((np.mgrid[0:Ho, 0:Wo][0] + 0.5) * H / Ho) - float(delta[1])), 0, H - 1).astype(int),
                      np.clip(np.floor(((np.mgrid[0:Ho, 0:Wo][1] + 0.5) * W / Wo) - float(delta[0])), 0, W - 1).astype(int)]
            clipped += int((np.abs(d[..., :3] - near[..., :3]).sum(-1) > 0).sum())
    return dict(accepted=accepted, rejected=rejected, clipped=clipped, peak=float(d[..., :3].max()), border=worst)


@pytest.mark.parametrize("W,H,Wo,Ho", [(37, 27, 56, 41), (24, 16, 48, 32)], ids=["37x27-56x41", "24x16-48x32"])
def test_checker_matches_an_independent_model(lib, W, H, Wo, Ho):
    """Observed share of pixels left out as borderline (the largest of the five frames): 37x27 -> 56x41: 0.17 %; 24x16 -> 48x32: 0.26 % (cap: 5 %)."""
    got = check_model(lib, W, H, Wo, Ho)
    print(f"borderline share {W}x{H} -> {Wo}x{Ho}: {got['border']:.4f}")
    assert got["accepted"] > Wo * Ho and got["rejected"] > 0 and got["clipped"] > 0
    assert got["peak"] > 0


def _static_setup(W, H):
    cam = _camera(W, H)
    g = _flat_frame(W, H)
    return cam, g, g.copy()


def test_hand_cases(lib, tmp_path_factory):
    rng = np.random.default_rng(5)
    # ratio 1 with 0 phases runs, and is TAA's resolve bit for bit (e = 0, kappa = 1, sO = sR)
    W, H = 16, 12
    cam, g, lastg = _static_setup(W, H)
    tl = taa.build(tmp_path_factory.mktemp("taa"))
    u1 = abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=W, outHeight=H, jitterPhases=0, alpha=0.1, clipGamma=1.0)
    k = upscale.UpscaleChecker(lib, W, H, u1)
    kt = taa.TaaChecker(tl, W, H, abi.Taa(mode=abi.TAA_ON, jitterPhases=0, alpha=0.1, clipGamma=1.0))
    for f in range(4):
        cur = rng.uniform(0.1, 1.0, (H, W, 4)).astype(np.float32)
        jc, delta = upscale.jitter_camera(cam, f, 0, W, H)
        got = k.frame(jc, delta, f, g, lastg, cur, cur * 0.5)
        want = kt.frame(jc, f, g, lastg, cur, cur * 0.5)
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
        if f:
            assert k.consistent.all() and (k.kappa == 1).all() and (got[2] == f + 1).all()
    # alpha = 1 with kappa = 1 returns c
    k = upscale.UpscaleChecker(lib, W, H, abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=W, outHeight=H, jitterPhases=0, alpha=1.0))
    c0, c1 = rng.uniform(0.1, 1.0, (H, W, 4)).astype(np.float32), rng.uniform(0.1, 1.0, (H, W, 4)).astype(np.float32)
    k.frame(cam, (0, 0), 0, g, lastg, c0, c0)
    d1, i1, n1 = k.frame(cam, (0, 0), 1, g, lastg, c1, c1 * 2)
    assert k.consistent.all() and (n1 == 2).all()
    assert np.array_equal(d1[..., :3], c1[..., :3]) and np.array_equal(i1[..., :3], (c1 * 2)[..., :3]) and (d1[..., 3] == 1).all()
    # a constant-colour input returns that colour, within rounding of the Catmull-Rom weight sum, at a ragged non-integer ratio under the jitter
    W, H, Wo, Ho = 13, 9, 20, 23
    cam, g, lastg = _static_setup(W, H)
    k = upscale.UpscaleChecker(lib, W, H, abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=Wo, outHeight=Ho, jitterPhases=16))
    colour = np.array([0.7, 0.3, 0.1, 1.0], np.float32)
    const = np.broadcast_to(colour, (H, W, 4)).copy()
    for f in range(6):
        jc, delta = upscale.jitter_camera(cam, f, 16, W, H)
        d, i, n = k.frame(jc, delta, f, g, lastg, const, const * 3)
        assert np.abs(d[..., :3] - colour[:3]).max() < 4e-6 and np.abs(i[..., :3] - 3 * colour[:3]).max() < 12e-6, f
    assert k.consistent.all() and (n == 6).all()
    # disocclusion (another material hash in the previous G-buffer) gives c of the nearest sample and n = 1
    jc, delta = upscale.jitter_camera(cam, 6, 16, W, H)
    cur = rng.uniform(0.1, 1.0, (H, W, 4)).astype(np.float32)
    d, i, n = k.frame(jc, delta, 6, g, _flat_frame(W, H, 0x02000000), cur, cur)
    oy, ox = np.mgrid[0:Ho, 0:Wo]
    f32 = np.float32   # (the sample geometry in the pass's own precision)
    px = np.clip(np.floor((ox.astype(f32) + f32(0.5)) * (f32(W) / f32(Wo)) - delta[0]), 0, W - 1).astype(int)
    py = np.clip(np.floor((oy.astype(f32) + f32(0.5)) * (f32(H) / f32(Ho)) - delta[1]), 0, H - 1).astype(int)
    assert (n == 1).all() and not k.consistent.any()
    assert np.array_equal(d[..., :3], cur[py, px, :3]) and (d[..., 3] == 1).all()
    # invalid material: the nearest sample passes through with all four channels and n = 1
    d, i, n = k.frame(jc, delta, 7, _flat_frame(W, H, INVALID), g, cur, cur * 2)
    assert np.array_equal(d, cur[py, px]) and np.array_equal(i, (cur * 2)[py, px]) and (n == 1).all()
    # kappa = 0 keeps the clipped history: 8 x 8 -> 32 x 32 without jitter puts the samples 1.5 output pixels from the outer columns of every 4 x 4 block.
    # There the current sample enters only through the 1 / n floor of the blend factor, whatever alpha is.
    W, H, Wo, Ho = 8, 8, 32, 32
    cam, g, lastg = _static_setup(W, H)
    hist = rng.uniform(0.1, 1.0, (Ho, Wo, 4)).astype(np.float32)
    cur = rng.uniform(0.1, 1.0, (H, W, 4)).astype(np.float32)
    outs = []
    for alpha in (1.0, 0.01):
        k = upscale.UpscaleChecker(lib, W, H, abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=Wo, outHeight=Ho, jitterPhases=0, alpha=alpha, clipGamma=1e6))
        k.D[0][:], k.I[0][:], k.N[0][:] = hist, hist, 1023.0
        k.valid, k.last = True, 0
        outs.append(k.frame(cam, (0, 0), 1, g, lastg, cur, cur))
        assert k.consistent.all() and (outs[-1][2] == 1024).all()
        zero = k.kappa == 0
    edge = (np.arange(Wo) % 4 == 0) | (np.arange(Wo) % 4 == 3)
    assert np.array_equal(zero, edge[None, :] | edge[:, None])
    assert np.array_equal(outs[0][0][zero], outs[1][0][zero]) and not np.array_equal(outs[0][0][~zero], outs[1][0][~zero])
    # (a static camera reprojects an output pixel onto itself up to the rounding of the camera matrices: the Catmull-Rom sample is the history texel to ~1e-4)
    assert np.abs(outs[0][0][zero][:, :3] - hist[zero][:, :3]).max() < 1.0 / 1024 + 2e-3


def _analytic(x, y):
    """a smooth image over render-pixel coordinates of a 16 x 16 frame, with detail near the render grid's Nyquist limit"""
    return 0.5 + 0.25 * np.sin(2.4 * x + 0.3) * np.cos(1.9 * y - 0.2) + 0.15 * np.sin(0.35 * x * y / 4.0 + 0.8)


def _bilinear(img, Wo, Ho):
    H, W = img.shape
    oy, ox = np.mgrid[0:Ho, 0:Wo]
    x = np.clip((ox + 0.5) * W / Wo - 0.5, 0, W - 1); y = np.clip((oy + 0.5) * H / Ho - 0.5, 0, H - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - x0, y - y0
    return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


def upsampling_property(lib):
    """(RMSE of the resolved image, RMSE of a bilinear upsample of one unjittered frame) against the analytic image at the output centres: static camera,
    hand-made valid G-buffer, 16 x 16 -> 32 x 32, 32 phases, 64 frames, no clipping"""
    W = H = 16
    Wo = Ho = 32
    cam, g, lastg = _static_setup(W, H)
    k = upscale.UpscaleChecker(lib, W, H, abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=Wo, outHeight=Ho, jitterPhases=32, alpha=0.1, clipGamma=1e6))
    py, px = np.mgrid[0:H, 0:W]
    for f in range(64):
        jc, delta = upscale.jitter_camera(cam, f, 32, W, H)
        v = _analytic(px + 0.5 + float(delta[0]), py + 0.5 + float(delta[1])).astype(np.float32)
        cur = np.stack([v, v, v, np.ones_like(v)], -1)
        d, _, n = k.frame(jc, delta, f, g, lastg, cur, cur)
    assert k.consistent.all() and (n == 64).all()
    oy, ox = np.mgrid[0:Ho, 0:Wo]
    truth = _analytic((ox + 0.5) * W / Wo, (oy + 0.5) * H / Ho)
    one = _analytic(px + 0.5, py + 0.5)
    rmse = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))   # noqa: E731
    return rmse(d[..., 0].astype(np.float64)), rmse(_bilinear(one, Wo, Ho))


def test_accumulation_adds_information(lib):
    """The property that justifies the feature.  Measured: RMSE 0.0394 resolved against 0.0792 for the bilinear upsample."""
    up, bi = upsampling_property(lib)
    print(f"RMSE against the analytic image at 32 x 32: resolved {up:.5f}, bilinear upsample of one 16 x 16 frame {bi:.5f}")
    assert up < bi, (up, bi)


def test_checker_under_the_sanitizers(tmp_path):
    """the checker under AddressSanitizer + UndefinedBehaviorSanitizer in a program of its own (tests/upscale_san_main.cpp): exactly sized buffers, reprojections
    in the image, on its borders, far outside and NaN, at every size of the GPU tests"""
    import subprocess
    exe = str(tmp_path / "upscale_san")
    srcs = [os.path.join(ROOT, "tests", "upscale_san_main.cpp"), upscale.SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp")]
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-w"]
    cxx = os.environ.get("CXX", "g++")
    objs = [str(tmp_path / (os.path.basename(src) + ".o")) for src in srcs]
    jobs = [subprocess.Popen([cxx] + flags + ["-c", src, "-o", obj]) for src, obj in zip(srcs, objs)]      # one compiler per file, side by side
    assert all(j.wait() == 0 for j in jobs)
    subprocess.check_call([cxx] + flags + objs + ["-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout

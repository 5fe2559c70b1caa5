"""The SVGF denoiser (rt_set_denoiser RT_DENOISER_SVGF) without a GPU: include/rt_abi.h declares the four entry points and rt_denoiser, the product library
exports them with the error convention, and the CPU checker (tests/svgf_checker.cpp, which the GPU tests hold the kernels to word for word) agrees with an
independent float64 numpy statement of the algorithm of DESIGN.md §14 on real noisy oracle frames of a small textured scene, through a camera move
(history accepted and rejected) and past n = 4 (variance from the temporal moments).  Tolerance as tests/test_denoise_model.py: 2e-4 relative + 1e-6 absolute."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from helpers import ROOT, abi, host, make_scene
from oracle.binding import Oracle
from test_denoise_model import GAUSS, INVALID, _geometry
import svgf

NAMES = ("rt_set_denoiser", "rt_get_denoiser", "rt_denoiser_reset", "rt_denoiser_readback")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return svgf.build(tmp_path_factory.mktemp("svgf"))


def test_header_declares_the_denoiser_entry_points():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert "RT_DENOISER_ATROUS = 0" in src and "RT_DENOISER_SVGF = 1" in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert C.sizeof(abi.Denoiser) == 32
    # the status codes abi.py mirrors (the error-path tests compare against them)
    body = re.search(r"typedef enum \{([^{}]*)\} rt_status;", src).group(1)
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"RT_(\w+) = (-?\d+)", body)}
    assert codes and all(getattr(abi, name) == v for name, v in codes.items()), codes


def test_library_exports_the_denoiser_entry_points():
    from restir_amd import renderer
    L = C.CDLL(renderer.HIP_LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n) and n in renderer.ABI_SYMBOLS
    d = abi.Denoiser()
    buf = np.zeros(4, dtype=np.float32)
    assert L.rt_set_denoiser(None, C.byref(d)) == -1
    assert L.rt_get_denoiser(None, C.byref(d)) == -1
    assert L.rt_denoiser_reset(None) == -1
    assert L.rt_denoiser_readback(None, 0, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == -1


def _lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _shift(a, dx, dy):
    """a[y + dy, x + dx] with clamped indices, and the in-grid mask"""
    h, w = a.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    qx, qy = xx + dx, yy + dy
    ok = (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
    return a[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)], ok


class Model:
    """float64 numpy statement of one component's chain; vectorised over the image (one shifted array per tap)"""

    def __init__(self, den, ind):
        self.den, self.ind = den, ind
        self.C = self.n = self.m = None

    def frame(self, st, cam, hist_ok, g, g_last, motion, noisy):
        ind, den = self.ind, self.den
        H, W = g.shape[:2]
        bx, by = (W // 2, H // 2) if ind else (W, H)
        f = 2 if ind else 1
        yy, xx = np.mgrid[0:by, 0:bx]
        nrm, pos, mat = _geometry(g, cam, xx * f, yy * f, (bx, by))
        valid = mat != INVALID
        c = noisy[:by, :bx, :3].astype(np.float64)
        sig_n = st.sigNormalIndirect if ind else st.sigNormalDirect
        sig_d = st.sigDepthIndirect if ind else st.sigDepthDirect
        phi = den.phiLumIndirect if ind else den.phiLumDirect
        # (a) temporal accumulation
        mv = motion[yy * f, xx * f].astype(np.int64)
        qx, qy = (mv[..., 0] >> 1, mv[..., 1] >> 1) if ind else (mv[..., 0], mv[..., 1])
        inb = (qx >= 0) & (qy >= 0) & (qx < bx) & (qy < by)
        cqx, cqy = np.clip(qx, 0, bx - 1), np.clip(qy, 0, by - 1)
        pn, _, pmat = _geometry(g_last, cam, cqx * f, cqy * f, (bx, by))
        pdepth = g_last[cqy * f, cqx * f, 0].view(np.float32).astype(np.float64)
        last_pos = np.array([cam.lastPosition.x, cam.lastPosition.y, cam.lastPosition.z], dtype=np.float64)
        reproj = np.linalg.norm(last_pos - pos, axis=-1)
        cons = inb & (pmat == mat) & ((nrm * pn).sum(-1) > 0.9) & (reproj < pdepth * 1.05) & valid
        if not hist_ok or self.C is None:
            cons &= False
            pC, pn_, pm = np.zeros((by, bx, 3)), np.zeros((by, bx)), np.zeros((by, bx, 2))
        else:
            pC, pn_, pm = self.C[cqy, cqx], self.n[cqy, cqx], self.m[cqy, cqx]
        n = np.where(cons, np.minimum(pn_ + 1, den.historyCap), 1)
        a = np.maximum(np.float32(den.alphaColor), 1.0 / n)[..., None]
        am = np.maximum(np.float32(den.alphaMoments), 1.0 / n)
        pC = np.where(cons[..., None], pC, 0.0)
        pm = np.where(cons[..., None], pm, 0.0)
        l = _lum(c)
        C_ = pC * (1 - a) + c * a
        m = np.stack([pm[..., 0] * (1 - am) + l * am, pm[..., 1] * (1 - am) + l * l * am], -1)
        C_[~valid] = 0.0; m[~valid] = 0.0
        n = np.where(valid, n, 0)
        # (b) variance
        s = np.zeros((by, bx, 2)); sw = np.zeros((by, bx))
        for j in range(-3, 4):
            for i in range(-3, 4):
                nq, ok = _shift(nrm, i, j)
                pq, _ = _shift(pos, i, j)
                mq, _ = _shift(mat, i, j)
                mmq, _ = _shift(m, i, j)
                ok &= mq == mat
                w = np.minimum(1.0, np.exp(-((nrm - nq) ** 2).sum(-1) / sig_n)) * (np.exp(-((pos - pq) ** 2).sum(-1) / sig_d) + 1e-2)
                w = np.where(ok, w, 0.0)
                s += mmq * w[..., None]; sw += w
        sp = s / np.maximum(sw, 1e-300)[..., None]
        var = np.where(n >= 4, m[..., 1] - m[..., 0] ** 2, sp[..., 1] - sp[..., 0] ** 2)
        var = np.where(valid, np.maximum(var, 0.0), 0.0)
        cur = np.concatenate([np.where(valid[..., None], C_, 0.0), var[..., None]], -1)
        # (c) the levels
        levels = 5 if ind else 4
        for level in range(levels):
            step = 1 << level
            gv = np.zeros((by, bx))
            for j in range(-1, 2):
                for i in range(-1, 2):
                    vq, ok = _shift(cur[..., 3], i, j)
                    k = 0.25 if (i == 0 and j == 0) else (0.125 if (i == 0 or j == 0) else 0.0625)
                    gv += np.where(ok, k * vq, 0.0)
            denom = phi * np.sqrt(gv) + 1e-10
            lp = _lum(cur[..., :3])
            tot, tv, tw = np.zeros((by, bx, 3)), np.zeros((by, bx)), np.zeros((by, bx))
            for j in range(-2, 3):
                for i in range(-2, 3):
                    cq, ok = _shift(cur, i * step, j * step)
                    nq, _ = _shift(nrm, i * step, j * step)
                    pq, _ = _shift(pos, i * step, j * step)
                    mq, _ = _shift(mat, i * step, j * step)
                    ok &= mq == mat
                    w = np.exp(-np.abs(lp - _lum(cq[..., :3])) / denom) * np.minimum(1.0, np.exp(-((nrm - nq) ** 2).sum(-1) / sig_n)) * \
                        (np.exp(-((pos - pq) ** 2).sum(-1) / sig_d) + 1e-2) * GAUSS[i + 2][j + 2]
                    w = np.where(ok, w, 0.0)
                    tot += cq[..., :3] * w[..., None]; tv += w * w * cq[..., 3]; tw += w
            zero = tw < 1e-5
            res = np.where(zero[..., None], 0.0, tot / np.maximum(tw, 1e-300)[..., None])
            v = np.where(zero, 0.0, tv / np.maximum(tw * tw, 1e-300))
            bad = np.isnan(res).any(-1) | (res < 0).any(-1) | (res > 1e8).any(-1) | ~valid
            res[bad] = 0.0; v[bad] = 0.0
            if level == 0:
                C_ = res.copy()
            cur = np.concatenate([res, v[..., None]], -1)
        self.C, self.n, self.m = C_, n, m
        return cur[..., :3] / (1.01 - cur[..., :3])


def _close(got, want, what):
    err = np.abs(got - want) - (2e-4 * np.abs(want) + 1e-6)
    assert (err <= 0).all(), (what, float(err.max()), np.unravel_index(err.argmax(), err.shape))


def check_model(lib, W, H):
    """the checker against `Model` over five frames of a moving camera at W x H; returns what the frames exercised"""
    sc, env = make_scene(abi.PROC_SPONZA, 0.01, 1, (64, 32))
    st = host.default_state(W, H, sc, env)
    o = Oracle(0); o.upload_scene(sc.desc(env)); o.resize(W, H)
    den = abi.Denoiser(mode=abi.DENOISER_SVGF)
    k = svgf.SvgfChecker(lib, W, H, den)
    models = [Model(den, False), Model(den, True)]
    eye, center, up, fov = sc.cameraPose()
    accepted = rejected = 0
    for f in range(5):   # a camera move at every frame: history follows the motion vectors; frames 1.. accept most pixels, 4 reaches n >= 4
        st.time = 300 + f
        sc.setCamera(eye + np.array([0.01 * f, 0.0, -0.01 * f], dtype=np.float32), center, up, fov)
        sc.updateCamera(W, H)
        cam = sc.getCamera(); o.set_camera(cam)
        ins, out_d, out_i = svgf.oracle_frame(o, k, st, cam, f)
        g = ins["this_g"].view(np.uint32).reshape(H, W, 4)
        gl = ins["last_g"].view(np.uint32).reshape(H, W, 4)
        mv = ins["motion"].view(np.int16).reshape(H, W, 2)
        nd = ins["noisy_dir"].view(np.float32).reshape(H, W, 4)
        ni = ins["noisy_ind"].view(np.float32).reshape(H, W, 4)
        want_d = models[0].frame(st, cam, f > 0, g, gl, mv, nd)
        want_i = models[1].frame(st, cam, f > 0, g, gl, mv, ni)
        _close(out_d[..., :3], want_d, f"direct frame {f}")
        _close(out_i[:H // 2, :W // 2, :3], want_i, f"indirect frame {f}")
        for which, mdl in ((abi.SVGF_DIRECT_COLOR, models[0]), (abi.SVGF_INDIRECT_COLOR, models[1])):
            h = k.history(which)
            assert np.array_equal(h[..., 3], mdl.n.astype(np.float32)), (f, which)
            _close(h[..., :3], mdl.C, f"history {which} frame {f}")
        for which, mdl in ((abi.SVGF_DIRECT_MOMENTS, models[0]), (abi.SVGF_INDIRECT_MOMENTS, models[1])):
            _close(k.history(which), mdl.m, f"moments {which} frame {f}")
        n = models[0].n
        if f > 0:
            accepted += int((n > 1).sum()); rejected += int((n == 1).sum())
    return dict(accepted=accepted, rejected=rejected, long_history=int((models[0].n >= 4).sum()), long_history_indirect=int((models[1].n >= 4).sum()),
                peak_direct=float(out_d[..., :3].max()), peak_indirect=float(out_i[:H // 2, :W // 2, :3].max()) if (W // 2) * (H // 2) else 0.0)


def test_checker_matches_an_independent_model(lib):
    W, H = 48, 32
    got = check_model(lib, W, H)
    assert got["accepted"] > 0 and got["rejected"] > 0
    assert got["long_history"] > W * H // 4       # the temporal-variance branch is exercised
    assert got["peak_direct"] > 0 and got["peak_indirect"] > 0

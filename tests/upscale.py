"""ctypes driver of tests/upscale_checker.cpp: the CPU restatement of the temporal upsampling resolve (rt_set_upscale, csrc/upscale.hip).
Built once per test session (the first caller's directory) with the flags of tests/taa.py.  `UpscaleChecker` keeps the history the way the context does (two
parities at the output size, validity, the reset rules); `oracle_frame` renders one frame through the oracle at the render size with the jittered camera
(rt_upscale_jitter_camera) and resolves it."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi
import taa

SRC = os.path.join(ROOT, "tests", "upscale_checker.cpp")
FLAGS = taa.FLAGS
_lib = None
lib_path = None   # where build() put the library (child processes load() it instead of compiling again)


def build(out_dir):
    """compile the checker + oracle/orc_scene.cpp into out_dir/libupschk.so (once per process) and load it"""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "libupschk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp"), "-o", so])
    return load(so)


def load(so):
    """load a library build() compiled (once per process)"""
    global _lib, lib_path
    if _lib is not None:
        return _lib
    L = C.CDLL(so)
    L.upscale_resolve.argtypes = [C.c_int] * 4 + [C.c_void_p] + [C.c_float] * 4 + [C.c_int] + [C.c_void_p] * 12
    _lib, lib_path = L, so
    return L


def jitter_camera(cam, frames, phases, W, H):
    """(jittered camera, delta) of rt_upscale_jitter_camera at the render size W x H"""
    from restir_amd.renderer import Renderer
    return Renderer.upscale_jitter_camera(cam, frames, phases, W, H)


def _f32(a, shape):
    return np.ascontiguousarray(np.ascontiguousarray(a).view(np.float32).reshape(-1)[:int(np.prod(shape))].reshape(shape))


class UpscaleChecker:
    """the resolve with the context's history rules: frame f reads the history of parity f-1 if it is valid and was written by the frame before"""

    def __init__(self, lib, W, H, ups):
        self.L, self.W, self.H = lib, W, H
        self.ups = ups
        self._alloc()
        self.consistent = self.kappa = None

    def _alloc(self):
        Wo, Ho = self.ups.outWidth, self.ups.outHeight
        self.Wo, self.Ho = Wo, Ho
        self.D = [np.zeros((Ho, Wo, 4), np.float32) for _ in range(2)]
        self.I = [np.zeros((Ho, Wo, 4), np.float32) for _ in range(2)]
        self.N = [np.zeros((Ho, Wo), np.float32) for _ in range(2)]
        self.valid, self.last = False, -1

    def set(self, ups):
        if bytes(ups) != bytes(self.ups):
            self.valid = False
        resized = (ups.outWidth, ups.outHeight) != (self.Wo, self.Ho)
        self.ups = ups
        if resized:
            self._alloc()

    def reset(self):
        self.valid = False

    def skip(self):
        """a frame without the pass (mode off, debugging_mode != 0)"""
        self.valid = False

    def frame(self, cam, delta, frames, this_g, last_g, cur_d, cur_i):
        """cam, delta: the jittered camera of the frame and its offset; arrays in the rt_readback layouts at the render size.  Returns (direct, indirect, n) of
        parity frames & 1 at the output size."""
        W, H, Wo, Ho = self.W, self.H, self.Wo, self.Ho
        ok = self.valid and self.last == ((frames + 1) & 1)
        cur, prev = frames & 1, (frames + 1) & 1
        g = np.ascontiguousarray(this_g).view(np.uint32).reshape(-1)[:W * H * 4].copy()
        gl = np.ascontiguousarray(last_g).view(np.uint32).reshape(-1)[:W * H * 4].copy()
        cd, ci = _f32(cur_d, (H, W, 4)), _f32(cur_i, (H, W, 4))
        oD, oI, oN = np.zeros((Ho, Wo, 4), np.float32), np.zeros((Ho, Wo, 4), np.float32), np.zeros((Ho, Wo), np.float32)
        cons, kappa = np.zeros((Ho, Wo), np.uint8), np.zeros((Ho, Wo), np.float32)
        rc = self.L.upscale_resolve(W, H, Wo, Ho, C.byref(cam), float(delta[0]), float(delta[1]), self.ups.alpha, self.ups.clipGamma, 1 if ok else 0,
                                    g.ctypes.data, gl.ctypes.data, cd.ctypes.data, ci.ctypes.data, self.D[prev].ctypes.data, self.I[prev].ctypes.data,
                                    self.N[prev].ctypes.data, oD.ctypes.data, oI.ctypes.data, oN.ctypes.data, cons.ctypes.data, kappa.ctypes.data)
        assert rc == 0
        self.D[cur], self.I[cur], self.N[cur] = oD, oI, oN
        self.valid, self.last = True, cur
        self.consistent, self.kappa = cons.astype(bool), kappa
        return oD, oI, oN


def oracle_frame(o, k, state, cam, frames, render=None):
    """one frame of the oracle `o` (sized to the render size) with the jittered camera of `cam`, resolved by the checker `k`; `render(o, state, jc, frames)`
    replaces the oracle's plain render_frame (SVGF, GI spatial reuse).  Returns (jittered camera, delta, resolved direct, indirect, n)"""
    jc, delta = jitter_camera(cam, frames, k.ups.jitterPhases, state.size.x, state.size.y)
    o.set_camera(jc)
    if render is None:
        o.render_frame(state, frames)
    else:
        render(o, state, jc, frames)
    cur = frames & 1
    d, i, n = k.frame(jc, delta, frames, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_GBUFFER0 + (1 - cur)),
                      o.readback(abi.BUF_DIRECT_RESULT0 + cur), o.readback(abi.BUF_INDIRECT_RESULT0 + cur))
    return jc, delta, d, i, n

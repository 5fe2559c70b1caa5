"""ctypes driver of tests/taa_checker.cpp: the CPU restatement of the temporal anti-aliasing resolve (rt_set_taa, csrc/taa.hip).
Built once per test session (the first caller's directory) with the flags of oracle/Makefile.  `TaaChecker` keeps the history the way the context does (two
parities, validity, the reset rules); `oracle_frame` renders one frame through the oracle with the jittered camera (rt_taa_jitter_camera) and resolves it."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "taa_checker.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared"]
_lib = None
lib_path = None   # where build() put the library (tests/optin.py hands it to child processes, which load() it instead of compiling again)


def build(out_dir):
    """compile the checker + oracle/orc_scene.cpp into out_dir/libtaachk.so (once per process) and load it"""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "libtaachk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp"), "-o", so])
    return load(so)


def load(so):
    """load a library build() compiled (once per process)"""
    global _lib, lib_path
    if _lib is not None:
        return _lib
    L = C.CDLL(so)
    L.taa_resolve.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 11
    L.taa_catmull_rom.argtypes = [C.c_float, C.c_void_p]
    L.taa_clip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    L.taa_ycocg.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    _lib, lib_path = L, so
    return L


def jitter_camera(cam, frames, phases, W, H):
    from restir_amd.renderer import Renderer
    return Renderer.taa_jitter_camera(cam, frames, phases, W, H)


def _f32(a, shape):
    return np.ascontiguousarray(np.ascontiguousarray(a).view(np.float32).reshape(-1)[:int(np.prod(shape))].reshape(shape))


class TaaChecker:
    """the resolve with the context's history rules: frame f reads the history of parity f-1 if it is valid and was written by the frame before"""

    def __init__(self, lib, W, H, taa=None):
        self.L, self.W, self.H = lib, W, H
        self.taa = taa if taa is not None else abi.Taa(mode=abi.TAA_ON)
        self.D = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
        self.I = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
        self.N = [np.zeros((H, W), np.float32) for _ in range(2)]
        self.valid, self.last = False, -1
        self.consistent = None

    def set(self, taa):
        if bytes(taa) != bytes(self.taa):
            self.valid = False
        self.taa = taa

    def reset(self):
        self.valid = False

    def skip(self):
        """a frame without the pass (TAA off, debugging_mode != 0)"""
        self.valid = False

    def frame(self, cam, frames, this_g, last_g, cur_d, cur_i):
        """cam: the jittered camera of the frame; arrays in the rt_readback layouts.  Returns (direct, indirect, n) of parity frames & 1."""
        W, H = self.W, self.H
        ok = self.valid and self.last == ((frames + 1) & 1)
        cur, prev = frames & 1, (frames + 1) & 1
        g = np.ascontiguousarray(this_g).view(np.uint32).reshape(-1)[:W * H * 4].copy()
        gl = np.ascontiguousarray(last_g).view(np.uint32).reshape(-1)[:W * H * 4].copy()
        cd, ci = _f32(cur_d, (H, W, 4)), _f32(cur_i, (H, W, 4))
        oD, oI, oN = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
        cons = np.zeros((H, W), np.uint8)
        rc = self.L.taa_resolve(W, H, C.byref(cam), self.taa.alpha, self.taa.clipGamma, 1 if ok else 0, g.ctypes.data, gl.ctypes.data, cd.ctypes.data,
                                ci.ctypes.data, self.D[prev].ctypes.data, self.I[prev].ctypes.data, self.N[prev].ctypes.data, oD.ctypes.data, oI.ctypes.data,
                                oN.ctypes.data, cons.ctypes.data)
        assert rc == 0
        self.D[cur], self.I[cur], self.N[cur] = oD, oI, oN
        self.valid, self.last = True, cur
        self.consistent = cons.astype(bool)
        return oD, oI, oN


def oracle_frame(o, k, state, cam, frames, jitter_phases):
    """one frame of the oracle `o` with the jittered camera of `cam` (render_frame: every stage), resolved by the checker `k`; returns (jittered camera, resolved
    direct, indirect, n)"""
    jc = jitter_camera(cam, frames, jitter_phases, state.size.x, state.size.y)
    o.set_camera(jc)
    o.render_frame(state, frames)
    cur = frames & 1
    d, i, n = k.frame(jc, frames, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_GBUFFER0 + (1 - cur)), o.readback(abi.BUF_DIRECT_RESULT0 + cur),
                      o.readback(abi.BUF_INDIRECT_RESULT0 + cur))
    return jc, d, i, n

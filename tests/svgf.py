"""ctypes driver of tests/svgf_checker.cpp: the CPU restatement of the SVGF denoiser (rt_set_denoiser RT_DENOISER_SVGF, csrc/svgf.hip).
Built once per test session (the first caller's directory) with the flags of oracle/Makefile.  `oracle_frame` runs one frame through the oracle with the
checker in place of the A-Trous chains: the oracle's DIRECT and INDIRECT stages make the noisy inputs, the checker filters them, the filtered images go back
into the oracle (upload_history) for its COMPOSE stage."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "svgf_checker.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared"]
_lib = None
lib_path = None   # where build() put the library (tests/optin.py hands it to child processes, which load() it instead of compiling again)


def build(out_dir):
    """compile the checker + oracle/orc_scene.cpp into out_dir/libsvgfchk.so (once per process) and load it"""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "libsvgfchk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp"), "-o", so])
    return load(so)


def load(so):
    """load a library build() compiled (once per process)"""
    global _lib, lib_path
    if _lib is not None:
        return _lib
    L = C.CDLL(so)
    L.svgf_create.restype = C.c_void_p
    L.svgf_create.argtypes = [C.c_int, C.c_int]
    L.svgf_destroy.argtypes = [C.c_void_p]
    L.svgf_set.argtypes = [C.c_void_p, C.c_void_p]
    L.svgf_reset.argtypes = [C.c_void_p]
    L.svgf_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    L.svgf_history.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    _lib, lib_path = L, so
    return L


class SvgfChecker:
    def __init__(self, lib, W, H, den=None):
        self.L = lib
        self.size = (W, H)
        self.h = lib.svgf_create(W, H)
        self.set(den if den is not None else abi.Denoiser(mode=abi.DENOISER_SVGF))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.svgf_destroy(self.h)
            self.h = None

    def set(self, den): self.L.svgf_set(self.h, C.byref(den))
    def reset(self): self.L.svgf_reset(self.h)

    def frame(self, state, cam, frames, this_g, last_g, motion, noisy_dir, noisy_ind):
        """arrays in the boundary layouts (rt_readback); returns the filtered direct image and the filtered indirect image (RT_BUF_DENOISE_IND_B layout)"""
        W, H = self.size
        ins = [np.ascontiguousarray(a) for a in (this_g, last_g, motion, noisy_dir, noisy_ind)]
        out_d = np.zeros((H, W, 4), dtype=np.float32)
        out_i = np.zeros((H, W, 4), dtype=np.float32)
        rc = self.L.svgf_frame(self.h, C.byref(state), C.byref(cam), int(frames), *[a.ctypes.data for a in ins], out_d.ctypes.data, out_i.ctypes.data)
        assert rc == 0, rc
        return out_d, out_i

    def history(self, which):
        """like Renderer.denoiser_readback"""
        W, H = self.size
        w, h = (W // 2, H // 2) if which & 1 else (W, H)
        out = np.empty((h, w, 4 if which < 2 else 2), dtype=np.float32)
        self.L.svgf_history(self.h, int(which), out.ctypes.data)
        return out


def oracle_frame(o, k, state, cam, frames):
    """one frame of the oracle `o` (camera already set) with the checker `k` as its denoiser; returns the noisy inputs it filtered"""
    o.run_stage(state, frames, abi.STAGE_DIRECT)
    o.run_stage(state, frames, abi.STAGE_INDIRECT)
    cur = frames & 1
    ins = dict(this_g=o.readback(abi.BUF_GBUFFER0 + cur), last_g=o.readback(abi.BUF_GBUFFER0 + (1 - cur)), motion=o.readback(abi.BUF_MOTION),
               noisy_dir=o.readback(abi.BUF_DIRECT_RESULT0 + cur), noisy_ind=o.readback(abi.BUF_DENOISE_IND_A))
    out_d, out_i = k.frame(state, cam, frames, **ins)
    if state.denoise > 0:
        o.upload_history(abi.BUF_DIRECT_RESULT0 + cur, out_d)
        o.upload_history(abi.BUF_DENOISE_IND_B, out_i)
    o.run_stage(state, frames, abi.STAGE_COMPOSE)
    return ins, out_d, out_i

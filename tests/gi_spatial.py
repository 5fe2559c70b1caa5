"""ctypes driver of tests/gi_spatial_checker.cpp: the CPU restatement of the ReSTIR GI spatial reuse pass (rt_set_gi_spatial, csrc/gi_spatial.hip).
Built once per test session (the first caller's directory) with the flags of oracle/Makefile.  `oracle_frame` runs one frame through the oracle with the
checker inserted after its INDIRECT stage: the checker resamples the oracle's reservoirs and rewrites its noisy indirect image (upload_history) before the
oracle's filters and COMPOSE stage, the way tests/svgf.py inserts the SVGF checker."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "gi_spatial_checker.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared"]
RESV_BYTES = 76
_lib = None
lib_path = None   # where build() put the library (tests/optin.py hands it to child processes, which load() it instead of compiling again)


def build(out_dir):
    """compile the checker + oracle/orc_scene.cpp into out_dir/libgischk.so (once per process) and load it"""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "libgischk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp"), "-o", so])
    return load(so)


def load(so):
    """load a library build() compiled (once per process)"""
    global _lib, lib_path
    if _lib is not None:
        return _lib
    L = C.CDLL(so)
    L.gis_create.restype = C.c_void_p
    L.gis_create.argtypes = [C.c_void_p]
    L.gis_destroy.argtypes = [C.c_void_p]
    L.gis_jacobian.restype = C.c_float
    L.gis_jacobian.argtypes = [C.c_void_p] * 4 + [C.c_float, C.POINTER(C.c_int)]
    L.gis_run.argtypes = [C.c_void_p] * 9
    _lib, lib_path = L, so
    return L


def jacobian(lib, xr, xn, xs, ns, jacobian_max=10.0):
    """(J, accepted) of one tap; sky samples give J = 1"""
    arrs = [np.ascontiguousarray(v, dtype=np.float32) for v in (xr, xn, xs, ns)]
    ok = C.c_int()
    J = lib.gis_jacobian(*[a.ctypes.data for a in arrs], C.c_float(jacobian_max), C.byref(ok))
    return float(J), bool(ok.value)


class GiSpatialChecker:
    def __init__(self, lib, desc):
        self.L = lib
        self._desc = desc   # keeps the arrays the descriptor points at alive until the upload copied them
        self.h = lib.gis_create(C.byref(desc))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.gis_destroy(self.h)
            self.h = None

    def run(self, state, cam, settings, this_g, resv, ind_a):
        """this_g / resv / ind_a in the rt_readback layouts (any dtype); returns (the pass's reservoirs as bytes, IND_A as float32 (H, W, 4), accepted taps per
        half-res pixel)"""
        W, H = state.size.x, state.size.y
        g = np.ascontiguousarray(this_g).view(np.uint8).reshape(-1)
        rv = np.ascontiguousarray(resv).view(np.uint8).reshape(-1)[:(W // 2) * (H // 2) * RESV_BYTES].copy()
        out = np.zeros((W // 2) * (H // 2) * RESV_BYTES, dtype=np.uint8)
        img = np.ascontiguousarray(ind_a).view(np.float32).reshape(-1)[:W * H * 4].copy().reshape(H, W, 4)
        taps = np.zeros((H // 2, W // 2), dtype=np.int32)
        rc = self.L.gis_run(self.h, C.byref(state), C.byref(cam), C.byref(settings), g.ctypes.data, rv.ctypes.data, out.ctypes.data, img.ctypes.data,
                            taps.ctypes.data)
        assert rc == 0, rc
        return out, img, taps


def oracle_frame(o, k, state, cam, frames, settings, svgf_checker=None):
    """one frame of the oracle `o` (camera already set) with the GI spatial checker `k` after its INDIRECT stage and, when given, the SVGF checker as its
    denoiser; returns the checker's reservoirs and IND_A"""
    import svgf
    o.run_stage(state, frames, abi.STAGE_DIRECT)
    o.run_stage(state, frames, abi.STAGE_INDIRECT)
    cur = frames & 1
    out, img, _ = k.run(state, cam, settings, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_INDIRECT_RESV0 + cur), o.readback(abi.BUF_DENOISE_IND_A))
    o.upload_history(abi.BUF_DENOISE_IND_A, img)
    if svgf_checker is not None:
        ins = dict(this_g=o.readback(abi.BUF_GBUFFER0 + cur), last_g=o.readback(abi.BUF_GBUFFER0 + (1 - cur)), motion=o.readback(abi.BUF_MOTION),
                   noisy_dir=o.readback(abi.BUF_DIRECT_RESULT0 + cur), noisy_ind=o.readback(abi.BUF_DENOISE_IND_A))
        out_d, out_i = svgf_checker.frame(state, cam, frames, **ins)
        if state.denoise > 0:
            o.upload_history(abi.BUF_DIRECT_RESULT0 + cur, out_d)
            o.upload_history(abi.BUF_DENOISE_IND_B, out_i)
    elif state.denoise > 0:
        for i in range(4):
            o.run_stage(state, frames, abi.STAGE_DENOISE_DIRECT, i)
        for i in range(5):
            o.run_stage(state, frames, abi.STAGE_DENOISE_INDIRECT, i)
    o.run_stage(state, frames, abi.STAGE_COMPOSE)
    return out, img

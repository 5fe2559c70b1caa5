"""ctypes driver of tests/refpt_checker.cpp: the CPU restatement of the reference mode (rt_reference_render) over the oracle's shading library.
Built once per test session (the first caller's directory) with the flags of oracle/Makefile."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "refpt_checker.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared"]
THREADS = 8
_lib = None


def build(out_dir):
    """compile the checker + oracle/orc_scene.cpp into out_dir/librefpt.so (once per process) and load it"""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "librefpt.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp"), "-o", so])
    L = C.CDLL(so)
    L.refpt_create.restype = C.c_void_p
    L.refpt_create.argtypes = [C.c_void_p]
    L.refpt_destroy.argtypes = [C.c_void_p]
    L.refpt_set_camera.argtypes = [C.c_void_p, C.c_void_p]
    L.refpt_set_sun_and_sky.argtypes = [C.c_void_p, C.c_void_p]
    L.refpt_resize.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.refpt_reset.argtypes = [C.c_void_p]
    L.refpt_samples.argtypes = [C.c_void_p]
    L.refpt_samples.restype = C.c_uint32
    L.refpt_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.refpt_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.refpt_rays.argtypes = [C.c_void_p]
    L.refpt_rays.restype = C.c_uint64
    _lib = L
    return L


class RefChecker:
    def __init__(self, lib, desc):
        self.L = lib
        self._desc = desc   # keeps the arrays the descriptor points at alive until the upload copied them
        self.h = lib.refpt_create(C.byref(desc))
        self.size = (0, 0)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.refpt_destroy(self.h)
            self.h = None

    def set_camera(self, cam): self.L.refpt_set_camera(self.h, C.byref(cam))
    def set_sun_and_sky(self, ss): self.L.refpt_set_sun_and_sky(self.h, C.byref(ss))
    def reset(self): self.L.refpt_reset(self.h)
    def samples(self): return int(self.L.refpt_samples(self.h))
    def rays(self): return int(self.L.refpt_rays(self.h))   # ray queries of the last render()

    def resize(self, w, h):
        self.L.refpt_resize(self.h, w, h)
        self.size = (w, h)

    def render(self, state, samples, threads=THREADS):
        rc = self.L.refpt_render(self.h, C.byref(state), int(samples), int(threads))
        assert rc == 0, rc

    def readback(self, component):
        W, H = self.size
        out = np.empty((H, W, 4), dtype=np.float32)
        assert self.L.refpt_readback(self.h, int(component), out.ctypes.data) == 0
        return out


def emissive_hashes(desc):
    """G-buffer material hashes (hash8bit, common.glsl:141-143) of the untextured emitters — dropping hashes a non-emitter shares"""
    raw = np.ctypeslib.as_array(C.cast(desc.materials, C.POINTER(C.c_uint8)), shape=(desc.numMaterials * 80,)).reshape(-1, 80)
    emis = raw[:, 36:48].copy().view(np.float32).reshape(-1, 3)
    etex = raw[:, 32:36].copy().view(np.int32).reshape(-1)
    h = [(((m ^ (m >> 8)) << 24) & 0xffffffff) for m in range(desc.numMaterials)]
    emitter = [(etex[m] == -1 and float(emis[m].sum()) > 1e-3) for m in range(desc.numMaterials)]
    return {h[m] for m in range(desc.numMaterials) if emitter[m]} - {h[m] for m in range(desc.numMaterials) if not emitter[m]}


def deterministic_pixels(desc, st, cam, W, H, sun_and_sky=None):
    """masks of the pixels whose primary ray misses / hits an emitter, and the oracle's direct-stage colour there (EnvRadiance / emission,
    clampRadiance with the clamp out of the way): what every reference sample of such a pixel must produce"""
    from oracle.binding import Oracle
    o = Oracle(0)
    o.upload_scene(desc)
    o.resize(W, H)
    if sun_and_sky is not None:
        o.set_sun_and_sky(sun_and_sky)
    o.set_camera(cam)
    s = abi.RtxState.from_buffer_copy(st)
    s.fireflyClampThreshold = 3.0e38
    o.run_stage(s, 0, abi.STAGE_DIRECT)
    g = o.readback(abi.BUF_GBUFFER0).view(np.uint32).reshape(H, W, 4)
    miss = g[..., 0].view(np.float32) >= 1e28 * 0.8
    emit = np.isin(g[..., 3] & 0xff000000, list(emissive_hashes(desc))) & ~miss
    want = o.readback(abi.BUF_DIRECT_RESULT0).view(np.float32).reshape(H, W, 4)
    return miss, emit, want

"""ctypes driver of tests/env_accel_checker.cpp (the CPU restatement of the environment's importance table, include/rt_abi.h "The environment") and
the maps the environment tests share, all generated from seeds: the smallest at which the build can still go wrong.  The checker is compiled once per process with
g++ (no GPU)."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np

from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "env_accel_checker.cpp")
FLAGS = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-Wall"]
_lib = None

# name -> what the map is there for (the order is the order of the parametrised tests)
MAPS = {
    "1x1": "one texel: the only large, no search has anything to find",
    "2x1": "one small, one large",
    "5x3": "odd sizes, three rows of different area",
    "64x1_equal": "all texels equal in one row: every texel is large, there are no smalls",
    "16x8_random": "about a quarter of the texels are large",
    "37x19_sun": "one texel at 1e3 and its neighbour at a third: two larges, a long run of smalls per large",
    "64x32_lower_black": "the lower half black: W = 0, those smalls have q = 0",
    "64x32_ramp": "a monotone ramp: consecutive larges exhaust in cascade",
    "257x129_sun": "33 153 ragged texels: several scan tiles, a tile boundary in the middle of a row",
    "8x4_black": "all black: M = 0, the identity table",
    "16x8_nan_negative": "a NaN texel and a negative texel: importance 0",
}
REFUSED = "16x8_inf"      # one +inf texel: the whole map is refused
ALL = list(MAPS) + [REFUSED]


@functools.lru_cache(maxsize=None)
def make(name):
    """(h, w, 4) float32, alpha 1; read-only (shared among the tests)"""
    w, h = (int(v) for v in name.split("_")[0].split("x"))
    rng = np.random.default_rng(1000 + ALL.index(name))
    a = np.ones((h, w, 4), np.float32)
    a[..., :3] = rng.uniform(0.05, 1.0, (h, w, 3)).astype(np.float32)
    kind = name.split("_", 1)[1] if "_" in name else ""
    if kind == "equal":
        a[..., :3] = np.float32([0.25, 0.75, 0.5])
    elif kind == "random":      # a heavy tail, so that roughly a quarter of the texels lie above the mean
        a[..., :3] = (rng.uniform(0.0, 1.0, (h, w, 1)) ** 4 * 8 + 0.01).astype(np.float32) * a[..., :3]
    elif kind == "sun":
        a[..., :3] *= np.float32(0.5)
        y, x = h // 2, w // 2
        a[y, x, :3] = np.float32(1e3)
        a[y, x + 1, :3] = np.float32(1e3) / np.float32(3)
    elif kind == "lower_black":
        a[h // 2:, :, :3] = 0
    elif kind == "ramp":
        a[..., :3] = ((np.arange(h * w, dtype=np.float32) + 1) / np.float32(h * w)).reshape(h, w, 1)
    elif kind == "black":
        a[..., :3] = 0
    elif kind == "nan_negative":
        a[2, 3, 0] = np.nan      # (in r: std::max(r, ...) then IS the NaN; a NaN in g or b is skipped by the comparison order)
        a[6, 1, 2] = np.nan
        a[5, 9, :3] = np.float32([-1.0, -0.5, -2.0])
    elif kind == "inf":
        a[3, 7, 2] = np.inf
    a.setflags(write=False)
    return a


def build(out_dir):
    global _lib
    if _lib is None:
        so = os.path.join(str(out_dir), "libenvchk.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, "-o", so])
        L = C.CDLL(so)
        L.evc_accel.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.evc_weights.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.evc_importance.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


_checked = {}


def check(lib, name):
    """the checker on a named map, computed once per process: (table, integral, average, numSmall), or None for a refused map"""
    if name not in _checked:
        a = make(name)
        h, w = a.shape[:2]
        out = np.zeros(w * h, abi.IMPT_SAMP_DT)
        integral, average, small = C.c_float(), C.c_float(), C.c_uint32()
        rc = lib.evc_accel(w, h, a.ctypes.data, out.ctypes.data, C.byref(integral), C.byref(average), C.byref(small))
        out.setflags(write=False)
        _checked[name] = None if rc else (out, integral.value, average.value, int(small.value))
    return _checked[name]


def weights(lib, a):
    """(W uint64 per texel, T): the quantised distribution the table must reproduce"""
    h, w = a.shape[:2]
    W, T = np.zeros(w * h, np.uint64), C.c_uint64()
    assert lib.evc_weights(w, h, a.ctypes.data, W.ctypes.data, C.byref(T)) == 0
    return W, int(T.value)


def importance(lib, a):
    h, w = a.shape[:2]
    out = np.zeros((h, w), np.float32)
    lib.evc_importance(w, h, a.ctypes.data, out.ctypes.data)
    return out


def implied_probabilities(table):
    """p_i = (q_i + sum over k with alias_k = i of (1 - q_k)) / n, in float64"""
    q = table["q"].astype(np.float64)
    return (q + np.bincount(table["alias"], weights=1.0 - q, minlength=len(table))) / len(table)


def words(table):
    return np.ascontiguousarray(table).view(np.uint32)


def f32_words(x):
    return np.float32(x).view(np.uint32)

"""ctypes driver of tests/light_derive_checker.cpp (the CPU restatement of the derived triangle-light records of the emitter mode, include/rt_abi.h "Emitters") and
the instance tables the CPU and the GPU tests share: not a test.  The checker is compiled once per process with g++ (no GPU)."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi
import instances
import lights
import refit

SRC = os.path.join(ROOT, "tests", "light_derive_checker.cpp")
_lib = None


def build(out_dir):
    global _lib
    if _lib is None:
        so = os.path.join(str(out_dir), "liblightderivechk.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + lights.FLAGS + [SRC, "-o", so])
        L = C.CDLL(so)
        L.ldc_derive.restype = C.c_int64
        L.ldc_derive.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class LightInfo(C.Structure):  # rt_light_buf_info
    _fields_ = [("puncLightSize", C.c_uint32), ("trigLightSize", C.c_uint32), ("trigSampProb", C.c_float), ("pad", C.c_int32)]


def info_of(desc):
    return LightInfo.from_buffer_copy(desc.lightInfo)


def prob_bits(info):
    return np.float32(info.trigSampProb).view(np.uint32)


def derive(lib, desc, table, meshes, rows, punc_weight, info):
    """(records, sources, derived lightInfo, emitting instances) of the checker for `table` as the instance table of `desc`; info: the lightInfo before.  An int
    instead: the first instance whose emissive prim mesh has no template"""
    t = instances.rows(table)
    m = np.ascontiguousarray(meshes, dtype=abi.EMITTER_MESH_DT)
    r = np.ascontiguousarray(rows, dtype=abi.EMITTER_ROW_DT)
    keep = r if r.size else np.zeros(1, abi.EMITTER_ROW_DT)
    out = LightInfo.from_buffer_copy(info)
    args = (C.addressof(desc), t.ctypes.data, len(t), m.ctypes.data, m.size, keep.ctypes.data, C.c_float(punc_weight))
    n = lib.ldc_derive(*args, None, None, None, None)
    if n < 0:
        return -1 - n
    rec, src = np.zeros(max(n, 1), lights.TRIG_DT), np.zeros(max(n, 1), lights.SOURCE_DT)
    em = C.c_uint32(0)
    assert lib.ldc_derive(*args, rec.ctypes.data, src.ctypes.data, C.byref(out), C.byref(em)) == n
    return rec[:n], src[:n], out, em.value


def bus_bytes(records, emitting):
    """the light bytes an rt_set_instances moves host -> device in the emitter mode (the formula of include/rt_abi.h "Emitters")"""
    return records * 16 + (2 * emitting + 1) * 4


def sequence(desc):
    """[(label, table)]: the successive instance tables of the emitter tests for a scene with at least one emissive and two plain instances.  Copies of emitters
    are placed with mirrored and non-uniformly scaled matrices (refit.move_matrix)"""
    base = refit.instances_of(desc)
    em = [int(i) for i in refit.describe(desc)["emissive"]]
    plain = [i for i in range(len(base)) if i not in em]
    assert em and len(plain) >= 2
    extent = float(max(np.abs(np.concatenate(refit.world_bounds(desc, i))).max() for i in range(desc.numInstances)))
    emissive_meshes = set(int(base["primMesh"][i]) for i in em)

    def copy(i, kind, shift):
        return instances.placed(desc, i, kind, extent, shift)

    def emitters_of(t):
        return [k for k in range(len(t)) if int(t["primMesh"][k]) in emissive_meshes]

    steps = []
    t = np.concatenate([base, copy(em[0], "mirror", (0.05 * extent, 0.0, 0.02 * extent))])
    steps.append(("an emitter added at the end", t))
    t = np.concatenate([copy(em[-1], "scale", (-0.04 * extent, 0.01 * extent, 0.0)), t])
    steps.append(("an emitter added at index 0", t))
    e = emitters_of(t)
    s = t.copy()
    s[[e[0], e[-1]]] = t[[e[-1], e[0]]]
    steps.append(("two emitters swapped", s))
    t = np.delete(s, emitters_of(s)[0])
    steps.append(("the first emitter removed", t))
    t = np.delete(t, emitters_of(t)[-1])
    steps.append(("the last emitter removed", t))
    two = np.concatenate([t, copy(em[0], "rotate", (0.0, 0.03 * extent, -0.05 * extent))])
    steps.append(("one emissive mesh with two instances", two))
    mixed = []
    for k in range(4):      # emitter, plain, emitter, plain ... with the table's remaining rows behind them
        mixed += [copy(em[k % len(em)], ("mirror", "scale", "translate", "rotate")[k], (0.02 * extent * k, 0.01 * extent, -0.03 * extent * k)), base[plain[k % len(plain)]:plain[k % len(plain)] + 1]]
    steps.append(("emitters interleaved with plain instances", np.concatenate(mixed + [base[plain]])))
    steps.append(("no emitter", base[plain]))
    steps.append(("back to the scene's table", base))
    return steps

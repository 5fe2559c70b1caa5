"""ctypes driver of tests/morph_checker.cpp (the CPU restatement of rt_update_morphs' arithmetic) and the targets and weights the morph tests share.
The checker is compiled once per process with g++ (no GPU).  Morph-then-skin is the checker's rows fed to skin.pose."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi
import skin

SRC = os.path.join(ROOT, "tests", "morph_checker.cpp")
FLAGS = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-Wall"]
_lib = None
VERTEX_DT, SET_DT, DELTA_DT = abi.VERTEX_DT, abi.MORPH_SET_DT, abi.MORPH_DELTA_DT


def build(out_dir):
    global _lib
    if _lib is None:
        so = os.path.join(str(out_dir), "libmorphchk.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, "-o", so])
        L = C.CDLL(so)
        L.mpc_morph.restype = C.c_uint32
        L.mpc_morph.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mpc_encode.restype = C.c_uint32
        L.mpc_encode.argtypes = [C.c_float] * 3
        _lib = L
    return _lib


def planes_per_target(planes):
    return 1 + (planes & 1) + ((planes >> 1) & 1)


def morph(lib, rest, deltas, target_count, planes, weights):
    """(morphed rows, non-finite positions, active targets): the checker on one mesh's rest rows, the set's delta rows (target-major) and its weights"""
    rest = np.ascontiguousarray(rest, dtype=VERTEX_DT)
    d = np.ascontiguousarray(deltas, dtype=DELTA_DT)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    assert w.size == target_count and d.size == target_count * planes_per_target(planes) * rest.size
    out = np.zeros_like(rest)
    active = C.c_uint32(0)
    bad = lib.mpc_morph(rest.ctypes.data, rest.size, d.ctypes.data, target_count, planes, w.ctypes.data, out.ctypes.data, C.byref(active))
    return out, int(bad), int(active.value)


def random_deltas(rest_count, target_count, planes, seed, scale=0.1):
    """target-major delta rows: small position deltas, direction deltas large enough to turn a normal; the pad column holds a NaN pattern (it is not read as a value)"""
    rng = np.random.default_rng(seed)
    d = np.zeros(target_count * planes_per_target(planes) * rest_count, DELTA_DT)
    rows = d["d"].reshape(target_count, planes_per_target(planes), rest_count, 3)
    rows[:, 0] = rng.uniform(-scale, scale, (target_count, rest_count, 3)).astype(np.float32)
    rows[:, 1:] = rng.uniform(-0.8, 0.8, rows[:, 1:].shape).astype(np.float32)
    d["pad"] = np.float32(np.nan)
    return d


class MorphedMesh:
    """one morphed prim mesh of a scene description: rest rows, delta rows, and the checker's morph of them"""

    def __init__(self, lib, desc, mesh, target_count, planes, seed=0, deltas=None, scale=0.1):
        self.lib, self.mesh, self.target_count, self.planes = lib, mesh, target_count, planes
        self.first, self.count = skin.mesh_range(desc, mesh)
        self.rest = skin.vertices_of(desc)[self.first:self.first + self.count]
        self.deltas = random_deltas(self.count, target_count, planes, seed, scale) if deltas is None else np.ascontiguousarray(deltas, dtype=DELTA_DT)

    def morphed(self, weights):
        rows, bad, _ = morph(self.lib, self.rest, self.deltas, self.target_count, self.planes, weights)
        assert bad == 0
        return rows

    def active(self, weights):
        return int((np.asarray(weights, np.float32) != 0).sum())


def sets_table(meshes):
    """(abi.MORPH_SET_DT records, concatenated delta rows) for a list of MorphedMesh"""
    st = np.zeros(len(meshes), SET_DT)
    first = 0
    for k, m in enumerate(meshes):
        st[k] = (m.mesh, m.target_count, first, m.planes)
        first += m.deltas.size
    return st, (np.concatenate([m.deltas for m in meshes]) if meshes else np.zeros(0, DELTA_DT))


def position_deltas(target_positions):
    """delta rows of a set without direction planes from a list of (V x 3) per-target position deltas"""
    t = np.asarray(target_positions, np.float32)
    d = np.zeros(t.shape[0] * t.shape[1], DELTA_DT)
    d["d"] = t.reshape(-1, 3)
    return d

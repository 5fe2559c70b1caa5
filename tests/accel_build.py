"""ctypes driver of tests/accel_build_checker.cpp (the CPU restatement of rt_rebuild_accel and the structural check of a tree), the tiny scenes and the scene list the
rebuild tests share.  The checker is compiled once per process together with tests/refit_checker.cpp and csrc/bvh8_builder.cpp (g++, no GPU): the restated builder
gets its boxes from the restated refit, as the device builder gets its boxes from the refit kernel."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi
import refit

SRC = os.path.join(ROOT, "tests", "accel_build_checker.cpp")
STACK_MAX = 64      # csrc/stages.h
_lib = None


def build(out_dir):
    global _lib
    if _lib is not None:
        return _lib
    ref = refit.build(out_dir)
    so = os.path.join(str(out_dir), "libaccelbuildchk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + refit.FLAGS + [SRC, refit.SRC, refit.BUILDER, "-o", so])
    L = C.CDLL(so)
    for name in ("rfc_build", "rfc_free", "rfc_counts", "rfc_pad", "rfc_copy", "rfc_refit", "rfc_check_tree"):   # the refit checker's entry points, compiled alongside
        getattr(L, name).argtypes = getattr(ref, name).argtypes
        getattr(L, name).restype = getattr(ref, name).restype
    L.abc_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.abc_check_structure.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_int]
    _lib = L
    return L


def table_of(host_tree):
    """per globalId the host build's record (all references of a triangle carry the same position-independent words)"""
    rec = host_tree.records()
    out = np.zeros(host_tree.ref.shape[0], refit.REC_DT)
    out[rec["globalId"]] = rec
    return out


def rebuilt(L, desc, host_tree, max_levels=STACK_MAX):
    """the restated device build of `desc` (instance rows and per-triangle table from `host_tree`, a host-built refit.Tree that followed the scene's moves) as a
    refit.Tree with .levels_built / .depth; None when the builder refuses (deeper than max_levels)"""
    n = host_tree.ref.shape[0]
    table = table_of(host_tree)
    nodes, recs, counts = np.zeros(max(n, 1) * refit.NODE, np.uint8), np.zeros(n * refit.REC, np.uint8), np.zeros(2, np.uint32)
    ref = np.ascontiguousarray(host_tree.ref)
    rc = L.abc_build(C.addressof(desc), host_tree.inst.ctypes.data, host_tree.inst.size // refit.INST, ref.ctypes.data, table.ctypes.data, n, max_levels,
                     nodes.ctypes.data, recs.ctypes.data, counts.ctypes.data)
    if rc == 1:
        return None
    assert rc == 0, rc
    t = refit.Tree(L, desc, nodes[:int(counts[0]) * refit.NODE], recs, host_tree.inst, 0.0)
    assert t.refit([], np.zeros((0, 12), np.float32)) == 0      # the boxes: the restated refit in its full mode (the pad "grows" from 0)
    assert t.stats[3] == 1 and int(t.stats[1]) == int(counts[0])
    t.depth = t.levels_built = int(counts[1])
    return t


def structure(L, t, depth=None, stack_max=STACK_MAX):
    msg = C.create_string_buffer(256)
    bad = L.abc_check_structure(t.nodes.ctypes.data, t.num_nodes, t.recs.ctypes.data, t.num_recs, t.ref.shape[0], t.depth if depth is None else depth, stack_max, msg, 256)
    return bad, msg.value.decode()


# ---- tiny scenes from numpy arrays --------------------------------------------------------------------------------------------------------------------------
class TinyScene:
    """one prim mesh, one opaque instance (identity), one material, no lights: the triangles given as (n, 3, 3) positions"""

    def __init__(self, tris):
        tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
        n = tris.shape[0]
        self.vertices = np.zeros((3 * n, 8), np.float32)      # rt_vertex, 32 B
        self.vertices[:, :3] = tris.reshape(-1, 3)
        self.indices = np.arange(3 * n, dtype=np.uint32)
        self.prim = np.array([[0, 3 * n, 0, 3 * n, 0]], np.uint32)
        self.inst = np.zeros(1, refit.INSTANCE_DT)
        self.inst["objectToWorld"][0] = np.eye(4, dtype=np.float32)[:3].reshape(12)
        self.inst["flags"][0] = 1 | 2                             # force opaque, no culling
        mat = np.zeros(20, np.float32)                            # rt_material, 80 B
        mat[0:4] = 1.0
        mat.view(np.int32)[[4, 7, 8, 12, 15]] = -1                # no textures
        mat[5], mat[6], mat[16] = 0.0, 1.0, 1.5
        self.mat = mat
        d = abi.SceneDesc()
        d.numPrimMeshes, d.primMeshes = 1, self.prim.ctypes.data
        d.numVertices, d.vertices = 3 * n, self.vertices.ctypes.data
        d.numIndices, d.indices = 3 * n, self.indices.ctypes.data
        d.numInstances, d.instances = 1, self.inst.ctypes.data
        d.numMaterials, d.materials = 1, self.mat.ctypes.data
        self._desc = d

    def desc(self):
        return self._desc


def _tri(p, s=0.3):
    p = np.asarray(p, np.float32)
    return [p, p + np.float32([s, 0, 0]), p + np.float32([0, s, 0.1 * s])]


def tiny(name):
    rng = np.random.default_rng(5)
    if name == "one":
        return TinyScene([_tri([0, 0, 0])])
    if name == "two":
        return TinyScene([_tri([0, 0, 0]), _tri([1, 0.5, -0.25])])
    if name == "four":          # more than one leaf slot
        return TinyScene([_tri(3 * rng.random(3)) for _ in range(4)])
    if name == "row25":         # more than one node can hold
        return TinyScene([_tri([0.4 * k, 0.01 * (k % 3), 0.0]) for k in range(25)])
    if name == "grid":          # a flat quad grid: zero extent on y
        out = []
        for i in range(5):
            for j in range(4):
                a, b, c, d = ([i, 0, j], [i + 1, 0, j], [i + 1, 0, j + 1], [i, 0, j + 1])
                out += [[a, b, c], [a, c, d]]
        return TinyScene(out)
    if name == "same30":        # 30 triangles around one centre: every key equal, the order is globalId's
        out = []
        for k in range(30):
            h = np.float32(2.0 ** -(k % 6)) * np.float32([1, 1, 1])     # symmetric about the centre: the box centre is exactly (1, 2, 3) for every one
            c = np.float32([1, 2, 3])
            out.append([c - h, c + h * np.float32([1, -1, 1]), c + h])
        return TinyScene(out)
    raise ValueError(name)


TINY = ("one", "two", "four", "row25", "grid", "same30")
SCENES = ("cornell", "street") + TINY + ("street_dup",)


def make(name):
    """(scene object with .desc(), ids, transforms) — the moves applied before the rebuild (street_dup: one instance moved exactly onto another of the same prim mesh)"""
    none = ([], np.zeros((0, 12), np.float32))
    if name == "cornell":
        return (refit.cornell(),) + none
    if name == "street":
        return (refit.street(),) + none
    if name == "street_dup":
        sc = refit.street()
        inst = refit.instances_of(sc.desc())
        pm = inst["primMesh"]
        for i in range(len(pm)):
            twins = np.nonzero(pm == pm[i])[0]
            if len(twins) > 1 and i == twins[0]:
                return sc, [int(twins[1])], inst["objectToWorld"][i:i + 1].copy()
        raise AssertionError("no two instances share a prim mesh")
    return (tiny(name),) + none


def host_tree(L, name):
    """(scene, desc of the moved scene, the host-built refit.Tree carried through the moves)"""
    sc, ids, xf = make(name)
    t = refit.Tree.built(L, sc.desc())
    if len(ids):
        assert t.refit(ids, xf) == 0
        sc.updateInstances(ids, xf)
    return sc, sc.desc(), t, ids, xf

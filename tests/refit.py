"""ctypes driver of tests/refit_checker.cpp (the CPU restatement of rt_update_instances and the tree check) and the scenes / moves the refit tests share.
The checker is compiled once per process together with csrc/bvh8_builder.cpp (g++, no GPU), so the CPU tests refit the builder's own trees."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi, host

SRC = os.path.join(ROOT, "tests", "refit_checker.cpp")
BUILDER = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc", "bvh8_builder.cpp")
FLAGS = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared", "-w", "-D__HIP_PLATFORM_AMD__",
         "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")]
_lib = None

NODE, REC, INST = 80, 64, 112
REC_DT = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("globalId", "<u4"), ("flags", "<u4"), ("alphaIdx", "<u4"), ("omm", "<u4", 4)])
INSTANCE_DT = np.dtype([("objectToWorld", "<f4", 12), ("primMesh", "<u4"), ("flags", "<u4")])   # rt_instance, 56 B
TRI_FLIP = 4


def build(out_dir):
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "librefitchk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, BUILDER, "-o", so])
    L = C.CDLL(so)
    L.rfc_build.restype = C.c_void_p
    L.rfc_build.argtypes = [C.c_void_p, C.c_int]
    L.rfc_free.argtypes = [C.c_void_p]
    L.rfc_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.rfc_pad.restype = C.c_float
    L.rfc_pad.argtypes = [C.c_void_p]
    L.rfc_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.rfc_refit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    L.rfc_check_tree.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_char_p, C.c_int]
    _lib = L
    return L


# ---- scene descriptions as numpy
def instances_of(desc):
    """a copy of the instance table"""
    return np.frombuffer((C.c_char * (desc.numInstances * 56)).from_address(desc.instances), dtype=INSTANCE_DT).copy()


def prim_meshes_of(desc):
    return np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.dtype([("vertexOffset", "<u4"), ("vertexCount", "<u4"), ("firstIndex", "<u4"),
                                                                                                               ("indexCount", "<u4"), ("materialIndex", "<i4")])).copy()


def tri_ref(desc):
    """globalId -> (instance, primitive): the running index over (instance, triangle) pairs (csrc/bvh8.h TriRef), from the scene description alone"""
    inst, pm = instances_of(desc), prim_meshes_of(desc)
    out = []
    for i, m in enumerate(inst["primMesh"]):
        n = int(pm["indexCount"][m]) // 3
        out.append(np.stack([np.full(n, i, np.uint32), np.arange(n, dtype=np.uint32)], axis=1))
    return np.ascontiguousarray(np.concatenate(out)) if out else np.zeros((0, 2), np.uint32)


def world_bounds(desc, i):
    """(lo, hi) of instance i in world space (float64; for aiming rays, not for comparisons)"""
    inst, pm = instances_of(desc), prim_meshes_of(desc)
    m = pm[inst["primMesh"][i]]
    v = np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=np.float32).reshape(-1, 8)[:, :3]
    p = v[int(m["vertexOffset"]):int(m["vertexOffset"]) + int(m["vertexCount"])].astype(np.float64)
    M = inst["objectToWorld"][i].reshape(3, 4).astype(np.float64)
    w = p @ M[:, :3].T + M[:, 3]
    return w.min(axis=0), w.max(axis=0)


# ---- rays for the comparisons of an edited context with a fresh one
def make_rays(desc, ids, n, seed):
    """n rays (origin, direction, tmax, a random word) over the scene, half of them through the boxes of the instances `ids`"""
    rng = np.random.default_rng(seed)
    inst = instances_of(desc)
    lo = np.min([world_bounds(desc, i)[0] for i in range(len(inst))], axis=0)
    hi = np.max([world_bounds(desc, i)[1] for i in range(len(inst))], axis=0)
    c, rad = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    target = lo + rng.random((n, 3)) * (hi - lo)
    for k in range(n // 2):      # half of the rays through the moved instances' new boxes
        a, b = world_bounds(desc, ids[k % len(ids)])
        target[k] = a + rng.random(3) * (b - a)
    d = rng.normal(size=(n, 3))
    origin = c + 1.5 * rad * d / np.linalg.norm(d, axis=1, keepdims=True)
    inside = rng.random(n) < 0.25
    origin[inside] = lo + rng.random((int(inside.sum()), 3)) * (hi - lo)
    dirs = target - origin
    dist = np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6] = origin, dirs / dist
    rays[:, 6] = (dist[:, 0] * rng.uniform(0.3, 2.0, n)).astype(np.float32)
    rays[:, 7] = rng.integers(0, 2 ** 32, n, dtype=np.uint32).view(np.float32)
    return rays


# ---- moves: 3 x 4 row-major matrices applied in world space on top of an instance's matrix
def compose(a, b):
    """a . b for two 3 x 4 affine matrices (12 floats each), rounded to float32"""
    A, B = np.eye(4), np.eye(4)
    A[:3] = np.asarray(a, np.float64).reshape(3, 4)
    B[:3] = np.asarray(b, np.float64).reshape(3, 4)
    return (A @ B)[:3].reshape(12).astype(np.float32)


def translation(t):
    m = np.eye(4)[:3]
    m[:, 3] = t
    return m.reshape(12)


def rotation_y(angle, about=(0, 0, 0)):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0]], np.float64)
    return compose(translation(about), compose(R.reshape(12), translation(-np.asarray(about, np.float64))))


def scaling(f, about=(0, 0, 0)):
    S = np.zeros((3, 4))
    S[0, 0], S[1, 1], S[2, 2] = f
    return compose(translation(about), compose(S.reshape(12), translation(-np.asarray(about, np.float64))))


MOVES = ("translate", "rotate", "scale", "mirror", "far", "back")


def move_matrix(kind, desc, i, extent, home=None):
    """the new objectToWorld of instance i for one of the transform classes of the tests; `extent` = the scene's largest |coordinate|, `home` = the matrices the
    scene was built with (where "back" returns to)"""
    cur = instances_of(desc)["objectToWorld"][i]
    lo, hi = world_bounds(desc, i)
    c = 0.5 * (lo + hi)
    if kind == "translate":
        return compose(translation(0.13 * (hi - lo) + 0.01 * extent), cur)
    if kind == "rotate":
        return compose(rotation_y(0.7, c), cur)
    if kind == "scale":
        return compose(scaling((1.3, 0.6, 0.9), c), cur)
    if kind == "mirror":
        return compose(scaling((-1.0, 1.0, 1.0), c), cur)
    if kind == "far":      # far outside the old extent: the pad grows
        return compose(translation(np.array([3.0, 0.5, -2.0]) * extent), cur)
    if kind == "back":     # ... and back inside: the pad shrinks
        return compose(translation(np.array([0.02, 0.01, 0.03]) * extent), cur if home is None else home[i])
    raise ValueError(kind)


class Tree:
    """nodes / leaf records / instance rows as byte arrays + the two pads; refit() and check() run the checker on them"""

    def __init__(self, lib, desc, nodes, recs, inst, tree_pad):
        self.L, self.desc = lib, desc
        self.nodes, self.recs, self.inst = (np.ascontiguousarray(np.asarray(a).view(np.uint8).reshape(-1)).copy() for a in (nodes, recs, inst))
        self.ref = tri_ref(desc)
        self.tree_pad = self.tri_pad = float(np.float32(tree_pad))
        self.moved = np.zeros(desc.numInstances, np.uint8)   # instances refitted since the build (all of them after a full refit)
        self.stats = None

    @classmethod
    def built(cls, lib, desc, threads=4):
        h = lib.rfc_build(C.byref(desc), threads)
        assert h
        cnt = np.zeros(8, np.uint64)
        lib.rfc_counts(h, cnt.ctypes.data)
        arrs = [np.zeros(int(cnt[k]) * sz, np.uint8) for k, sz in ((0, NODE), (1, REC), (3, INST))]
        for which, a in enumerate(arrs):
            lib.rfc_copy(h, which, a.ctypes.data)
        t = cls(lib, desc, arrs[0], arrs[1], arrs[2], lib.rfc_pad(h))
        t.depth, t.splits, t.triangles = int(cnt[4]), int(cnt[5]), int(cnt[2])
        lib.rfc_free(h)
        return t

    @property
    def num_nodes(self): return self.nodes.size // NODE
    @property
    def num_recs(self): return self.recs.size // REC
    def records(self): return self.recs.view(REC_DT)

    def refit(self, ids, xf):
        """rfc_refit in place; returns 0 / -1 (refused, nothing changed)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        xf = np.ascontiguousarray(xf, dtype=np.float32).reshape(-1)
        tp, pad, stats = C.c_float(self.tree_pad), C.c_float(0), np.zeros(4, np.uint32)
        rc = self.L.rfc_refit(self.nodes.ctypes.data, self.num_nodes, self.recs.ctypes.data, self.num_recs, self.ref.ctypes.data, self.ref.shape[0], self.inst.ctypes.data,
                              self.inst.size // INST, C.addressof(self.desc), ids.ctypes.data, xf.ctypes.data, ids.size, C.byref(tp), C.byref(pad), stats.ctypes.data)
        if rc == 0:
            self.tree_pad, self.tri_pad, self.stats = tp.value, pad.value, stats
            self.moved[ids] = 1
            if stats[3]:
                self.moved[:] = 1
        return rc

    def check(self, pad=None):
        """(violations, first message) of rfc_check_tree with the hit rule's pad"""
        msg = C.create_string_buffer(256)
        bad = self.L.rfc_check_tree(self.nodes.ctypes.data, self.num_nodes, self.recs.ctypes.data, self.num_recs, self.ref.ctypes.data, self.ref.shape[0],
                                    self.moved.ctypes.data, self.tri_pad if pad is None else pad, msg, 256)
        return bad, msg.value.decode()

    def levels(self):
        """[(first node, count)] per level, root first, and the parent of every node"""
        n = self.nodes.reshape(-1, NODE)
        imask, child_base = n[:, 15], n[:, 16:20].copy().view("<u4")[:, 0]
        parent = np.full(self.num_nodes, -1, np.int64)
        out, first, count = [], 0, 1
        while count:
            out.append((first, count))
            nxt = 0
            for k in range(first, first + count):
                c = bin(int(imask[k])).count("1")
                parent[int(child_base[k]):int(child_base[k]) + c] = k
                nxt += c
            first, count = first + count, nxt
        return out, parent

    def rec_node(self):
        """leaf record -> node that holds it"""
        n = self.nodes.reshape(-1, NODE)
        out = np.full(self.num_recs, -1, np.int64)
        tri_base = n[:, 20:24].copy().view("<u4")[:, 0]
        for k in range(self.num_nodes):
            for s in range(8):
                m = int(n[k, 24 + s])
                if m and not (int(n[k, 15]) >> s) & 1:
                    out[int(tri_base[k]) + (m & 31):int(tri_base[k]) + (m & 31) + bin(m >> 5).count("1")] = k
        return out


def hip_build_accel(r):
    """rt_build_accel on a Renderer's context (builds the context's own copy of the scene: the moved one after updates)"""
    from restir_amd.renderer import hip_lib
    return hip_lib().rt_build_accel(r._h)


def scene_extent(tree):
    r = tree.records()
    v = np.concatenate([r["v0"], r["v0"] + r["e1"], r["v0"] + r["e2"]])
    return float(np.abs(v).max())


# ---- the two scenes
def cornell():
    sc = host.Scene().makeProcedural(abi.PROC_CORNELL)
    return sc


def street(scale=0.004, seed=3):
    """the exterior street scene at a few thousand triangles: instanced trees with alpha-tested leaves, emissive lamps, mirrored props, long thin triangles"""
    return host.Scene().makeProcedural(abi.PROC_BISTRO_EXT, scale, seed)


def describe(desc):
    """which instances share a prim mesh / are emissive / alpha-tested / mirrored"""
    inst, pm = instances_of(desc), prim_meshes_of(desc)
    mats = np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.float32).reshape(-1, 20)
    emis = mats[:, 9:12]   # rt_material::emissiveFactor
    lum = 0.2126 * emis[:, 0] + 0.7152 * emis[:, 1] + 0.0722 * emis[:, 2]
    uses = np.bincount(inst["primMesh"], minlength=len(pm))
    det = np.array([np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for m in inst["objectToWorld"]])
    return {"shared": np.nonzero(uses[inst["primMesh"]] > 1)[0], "emissive": np.nonzero(lum[np.maximum(pm["materialIndex"][inst["primMesh"]], 0)] > 1e-2)[0],
            "alpha": np.nonzero((inst["flags"] & 1) == 0)[0], "mirrored": np.nonzero(det < 0)[0]}

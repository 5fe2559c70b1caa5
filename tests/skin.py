"""ctypes driver of tests/skin_checker.cpp (the CPU restatement of rt_update_skins' arithmetic) and the meshes, influences and poses the skinning tests share.
The checker is compiled once per process with g++ (no GPU)."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi
import refit

SRC = os.path.join(ROOT, "tests", "skin_checker.cpp")
FLAGS = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-Wall"]
_lib = None
VERTEX_DT, INFLUENCE_DT, SKIN_DT = abi.VERTEX_DT, abi.SKIN_INFLUENCE_DT, abi.SKIN_DT
IDENTITY = np.eye(4, dtype=np.float64)[:3].reshape(12)


def build(out_dir):
    global _lib
    if _lib is None:
        so = os.path.join(str(out_dir), "libskinchk.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, "-o", so])
        L = C.CDLL(so)
        L.skc_skin.restype = C.c_uint32
        L.skc_skin.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skc_decode.argtypes = [C.c_uint32, C.c_void_p]
        L.skc_encode.restype = C.c_uint32
        L.skc_encode.argtypes = [C.c_float] * 3
        _lib = L
    return _lib


def pose(lib, rest, influences, joints):
    """(posed rows, number of non-finite positions): the checker on one mesh's rest rows, influence rows and joint matrices (n x 12)"""
    rest = np.ascontiguousarray(rest, dtype=VERTEX_DT)
    inf = np.ascontiguousarray(influences, dtype=INFLUENCE_DT)
    j = np.ascontiguousarray(joints, dtype=np.float32).reshape(-1, 12)
    assert inf.size == rest.size and (inf["joint"] < len(j)).all()
    out = np.zeros_like(rest)
    bad = lib.skc_skin(rest.ctypes.data, rest.size, inf.ctypes.data, j.ctypes.data, out.ctypes.data)
    return out, int(bad)


def decode(lib, packed):
    out = np.zeros((len(packed), 3), np.float32)
    for k, p in enumerate(packed):
        lib.skc_decode(int(p), out[k].ctypes.data)
    return out


# ---- scene descriptions
def vertices_of(desc):
    return np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=VERTEX_DT).copy()


def with_vertices(desc, verts):
    """a copy of the description that reads `verts` (kept alive by the copy)"""
    d = abi.SceneDesc.from_buffer_copy(desc)
    v = np.ascontiguousarray(verts, dtype=VERTEX_DT)
    assert v.size == desc.numVertices
    d.vertices = v.ctypes.data
    d._keep = v
    return d


def mesh_range(desc, m):
    pm = refit.prim_meshes_of(desc)[m]
    return int(pm["vertexOffset"]), int(pm["vertexCount"])


def instances_of_mesh(desc, m):
    return np.nonzero(refit.instances_of(desc)["primMesh"] == m)[0].astype(np.uint32)


class Patches:
    """several prim meshes of n_k triangles each (a strip of small triangles along +y, real packed normals / tangents / colours), one opaque instance per mesh
    side by side along x; `extra` = per mesh a vertex at that position that no index references"""

    def __init__(self, lib, counts, extra=None, mirror_instance_of=None):
        rng = np.random.default_rng(17)
        verts, idx, prim = [], [], []
        for k, n in enumerate(counts):
            v = np.zeros(3 * n + (1 if extra is not None else 0), VERTEX_DT)
            t = np.arange(n, dtype=np.float32)
            base = np.stack([0.05 * (t % 3), 0.04 * t, 0.03 * (t % 2)], axis=1)
            for c, off in enumerate(([0, 0, 0], [0.3, 0, 0.02], [0, 0.3, 0.05])):
                v["position"][c:3 * n:3] = base + np.float32(off)
            d = rng.normal(size=(v.size, 3)).astype(np.float32)
            v["normal"] = [lib.skc_encode(*x) for x in d]
            d = rng.normal(size=(v.size, 3)).astype(np.float32)
            v["tangent"] = [lib.skc_encode(*x) for x in d]
            v["texcoord"] = rng.random((v.size, 2)).astype(np.float32)
            v["color"] = rng.integers(0, 2 ** 32, v.size, dtype=np.uint32)
            v["normal"][0] = 0xffffffff      # the codec's sentinel stays
            if extra is not None:
                v["position"][3 * n] = extra
            prim.append([sum(len(x) for x in verts), v.size, sum(len(x) for x in idx), 3 * n, 0])
            verts.append(v)
            idx.append(np.arange(3 * n, dtype=np.uint32))
        self.vertices, self.indices = np.concatenate(verts), np.concatenate(idx)
        self.prim = np.array(prim, np.uint32)
        meshes = list(range(len(counts))) + ([mirror_instance_of] if mirror_instance_of is not None else [])
        self.inst = np.zeros(len(meshes), refit.INSTANCE_DT)
        for i, m in enumerate(meshes):
            M = np.eye(4)[:3]
            M[:, 3] = [1.2 * i, 0, 0]
            if i >= len(counts):
                M[0, 0] = -1.0
            self.inst["objectToWorld"][i] = M.reshape(12)
            self.inst["primMesh"][i] = m
            self.inst["flags"][i] = 1 | 2
        mat = np.zeros(20, np.float32)
        mat[0:4] = 1.0
        mat.view(np.int32)[[4, 7, 8, 12, 15]] = -1
        mat[5], mat[6], mat[16] = 0.0, 1.0, 1.5
        self.mat = mat
        d = abi.SceneDesc()
        d.numPrimMeshes, d.primMeshes = len(counts), self.prim.ctypes.data
        d.numVertices, d.vertices = self.vertices.size, self.vertices.ctypes.data
        d.numIndices, d.indices = self.indices.size, self.indices.ctypes.data
        d.numInstances, d.instances = len(meshes), self.inst.ctypes.data
        d.numMaterials, d.materials = 1, self.mat.ctypes.data
        self._desc = d

    def desc(self):
        return self._desc


def deformed_mesh(name, desc):
    """the prim mesh the tests deform: Cornell's tall box; the street scene's instanced tree mesh (shared, with a mirrored instance where the scene has one)"""
    inst = refit.instances_of(desc)
    if name == "cornell":
        return int(inst["primMesh"][4])
    d = refit.describe(desc)
    shared = set(int(m) for m in inst["primMesh"][d["shared"]])
    both = [int(inst["primMesh"][i]) for i in d["mirrored"] if int(inst["primMesh"][i]) in shared]
    pm = refit.prim_meshes_of(desc)
    return max(both or shared, key=lambda m: int(pm["indexCount"][m]))


def alpha_mesh(desc):
    """the largest prim mesh of an alpha-tested instance (the street scene's leaves)"""
    inst, pm = refit.instances_of(desc), refit.prim_meshes_of(desc)
    return max((int(inst["primMesh"][i]) for i in refit.describe(desc)["alpha"]), key=lambda m: int(pm["vertexCount"][m]))


# ---- influences and poses
def influences_by_height(rest, joint_count, seed=0):
    """joint k owns the k-th slab of the mesh's y range; a vertex blends the two slabs around it.  Every fourth row carries its whole weight in slot 3, every
    seventh has a zero-weight row entry pointing at another joint (zero weights are not skipped)"""
    rng = np.random.default_rng(seed)
    y = rest["position"][:, 1].astype(np.float64)
    lo, hi = (y.min(), y.max()) if y.size else (0.0, 1.0)
    u = (y - lo) / max(hi - lo, 1e-9) * (joint_count - 1)
    j0 = np.minimum(np.floor(u).astype(np.int64), joint_count - 1)
    j1 = np.minimum(j0 + 1, joint_count - 1)
    f = (u - j0).astype(np.float32)
    inf = np.zeros(rest.size, INFLUENCE_DT)
    inf["joint"][:, 0], inf["joint"][:, 1] = j0, j1
    inf["weight"][:, 0], inf["weight"][:, 1] = np.float32(1) - f, f
    inf["joint"][:, 2] = rng.integers(0, joint_count, rest.size)
    whole = np.arange(rest.size) % 4 == 3
    inf["joint"][whole, 3] = j0[whole]
    inf["weight"][whole] = [0, 0, 0, 1]
    return inf


def affine(R=np.eye(3), t=(0, 0, 0), about=(0, 0, 0)):
    """x -> R (x - about) + about + t as 12 floats"""
    R, t, about = np.asarray(R, np.float64), np.asarray(t, np.float64), np.asarray(about, np.float64)
    M = np.zeros((3, 4))
    M[:, :3] = R
    M[:, 3] = about + t - R @ about
    return M.reshape(12).astype(np.float32)


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


POSES = ("bend", "twist", "mirror", "far", "back")


def pose_matrices(kind, joint_count, centre, extent):
    """joint matrices (joint_count x 12) of one of the poses of the tests: joint 0 stays, the others turn / lean more the higher they sit"""
    out = []
    for k in range(joint_count):
        s = k / max(joint_count - 1, 1) if joint_count > 1 else 1.0
        if kind == "bend":
            out.append(affine(rot("z", 0.5 * s), (0.03 * s * extent, 0, 0), centre))
        elif kind == "twist":
            out.append(affine(rot("y", 1.1 * s) @ np.diag([1.0, 1.0 + 0.2 * s, 1.0]), (0, 0, 0.02 * s * extent), centre))
        elif kind == "mirror":      # the last joint mirrors: its vertices' normals turn with the cofactors and the sign of the determinant
            out.append(affine(np.diag([-1.0, 1.0, 1.0]) if k == joint_count - 1 else rot("y", 0.3 * s), (0, 0.01 * extent, 0), centre))
        elif kind == "far":         # far outside the scene: the pad grows
            out.append(affine(rot("x", 0.2 * s), np.array([3.0, 0.5, -2.0]) * extent, centre))
        elif kind == "back":
            out.append(affine(rot("x", 0.05 * s), np.array([0.02, 0.01, 0.03]) * extent, centre))
        else:
            raise ValueError(kind)
    return np.stack(out)


class SkinnedMesh:
    """one skinned prim mesh of a scene description: rest rows, influences, and the checker's pose of it"""

    def __init__(self, lib, desc, mesh, joint_count, seed=0):
        self.lib, self.mesh, self.joint_count = lib, mesh, joint_count
        self.first, self.count = mesh_range(desc, mesh)
        self.rest = vertices_of(desc)[self.first:self.first + self.count]
        self.influences = influences_by_height(self.rest, joint_count, seed)
        p = self.rest["position"].astype(np.float64)
        self.centre = 0.5 * (p.min(axis=0) + p.max(axis=0)) if self.count else np.zeros(3)

    def posed(self, joints):
        rows, bad = pose(self.lib, self.rest, self.influences, joints)
        assert bad == 0
        return rows

    def matrices(self, kind, extent):
        return pose_matrices(kind, self.joint_count, self.centre, extent)


def skins_table(meshes):
    """(abi.SKIN_DT records, concatenated influences) for a list of SkinnedMesh"""
    sk = np.zeros(len(meshes), SKIN_DT)
    first = 0
    for k, m in enumerate(meshes):
        sk[k] = (m.mesh, 0, m.joint_count, first)
        first += m.count
    return sk, (np.concatenate([m.influences for m in meshes]) if meshes else np.zeros(0, INFLUENCE_DT))

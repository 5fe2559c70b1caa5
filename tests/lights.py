"""ctypes driver of tests/light_checker.cpp (the CPU restatement of the light-record rewrite of rt_set_light_sources) and the scene the light-source tests share: not a
test.  The checker is compiled once per process with g++ (no GPU)."""
import ctypes as C
import json
import os
import subprocess
import numpy as np

from helpers import ROOT, abi, host
import refit
import skin

SRC = os.path.join(ROOT, "tests", "light_checker.cpp")
FLAGS = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-Wall"]
_lib = None
TRIG_DT, SOURCE_DT = abi.TRIG_LIGHT_DT, abi.LIGHT_SOURCE_DT
POS = slice(8, 44)      # the bytes of a record that move: v0 v1 v2


def build(out_dir):
    global _lib
    if _lib is None:
        so = os.path.join(str(out_dir), "liblightchk.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, "-o", so])
        L = C.CDLL(so)
        L.lgc_validate.restype = C.c_uint32
        L.lgc_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.lgc_rewrite.restype = C.c_uint32
        L.lgc_rewrite.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def records_of(desc):
    """a copy of the triangle-light records of a scene description"""
    n = desc.lightInfo.trigLightSize if desc.trigLights else 0
    return np.frombuffer((C.c_char * (n * 96)).from_address(desc.trigLights), dtype=TRIG_DT).copy() if n else np.zeros(0, TRIG_DT)


def rewrite(lib, desc, sources, records, dirty=None):
    """(records rewritten by the checker for the geometry of `desc`, count): dirty = instance ids, or None for every record"""
    src = np.ascontiguousarray(sources, dtype=SOURCE_DT)
    out = np.ascontiguousarray(records, dtype=TRIG_DT).copy()
    assert src.size == out.size
    assert lib.lgc_validate(desc.primMeshes, desc.instances, desc.numInstances, src.ctypes.data, src.size, out.ctypes.data) == 0
    mask = None
    if dirty is not None:
        mask = np.zeros(max(desc.numInstances, 1), np.uint8)
        mask[np.asarray(dirty, np.int64)] = 1
    n = lib.lgc_rewrite(desc.primMeshes, desc.vertices, desc.indices, desc.instances, src.ctypes.data, src.size, mask.ctypes.data if mask is not None else None, out.ctypes.data)
    return out, int(n)


def raw(records):
    """records as (n, 96) bytes"""
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 96)


def with_lights(desc, records):
    """a copy of the description that reads `records` as its triangle lights (kept alive by the copy)"""
    d = abi.SceneDesc.from_buffer_copy(desc)
    r = np.ascontiguousarray(records, dtype=TRIG_DT)
    assert r.size == desc.lightInfo.trigLightSize
    d.trigLights = r.ctypes.data
    d._keep = r
    return d


def permuted(records, sources, perm):
    """records and sources listed in the order perm (new[k] = old[perm[k]]); the alias entries follow their records"""
    perm = np.asarray(perm, np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    rec = records[perm].copy()
    rec["impSamp"]["alias"] = inv[rec["impSamp"]["alias"]]
    return rec, sources[perm].copy()


def interleave(n):
    """a fixed order of 0..n-1 that puts neighbours far apart: a stride of about 0.38 n through the list (the first such stride coprime with n)"""
    import math
    s = max(1, int(0.382 * n))
    while math.gcd(s, n) != 1:
        s += 1
    return np.array([(s * k) % n for k in range(n)], np.int64)


class Emitters:
    """emissive strip meshes (skin.Patches' strips: n small triangles along +y) of `counts` triangles each behind `plain` instances of a one-triangle plain mesh,
    one emissive instance per mesh and a mirrored second instance of mesh `mirror_of`; written as glTF and read by host.Scene, so that the scene's own
    createTrigLightBuffer, updateInstances and updateVertices give the expected records.  Instance ids: 0 .. plain-1 plain, then the emitters in mesh order, then
    the mirrored one"""

    def __init__(self, tmp, counts, plain, mirror_of):
        rng = np.random.default_rng(23)
        blob, views, accessors, meshes = b"", [], [], []

        def add(a, target, typ, comp):
            nonlocal blob
            a = np.ascontiguousarray(a)
            views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": a.nbytes, "target": target})
            acc = {"bufferView": len(views) - 1, "componentType": comp, "count": len(a), "type": typ}
            if typ == "VEC3":
                acc["min"], acc["max"] = a.min(axis=0).tolist(), a.max(axis=0).tolist()
            accessors.append(acc)
            blob += a.tobytes()
            return len(accessors) - 1

        for k, n in enumerate([1] + list(counts)):      # mesh 0: the plain triangle
            t = np.arange(n, dtype=np.float32)
            base = np.stack([0.05 * (t % 3), 0.04 * t, 0.03 * (t % 2)], axis=1).astype(np.float32)
            pos = np.zeros((3 * n, 3), np.float32)
            for c, off in enumerate(([0, 0, 0], [0.3, 0, 0.02], [0, 0.3, 0.05])):
                pos[c::3] = base + np.float32(off)
            uv = rng.random((3 * n, 2)).astype(np.float32)
            idx = np.arange(3 * n, dtype=np.uint32)
            meshes.append({"primitives": [{"attributes": {"POSITION": add(pos, 34962, "VEC3", 5126), "TEXCOORD_0": add(uv, 34962, "VEC2", 5126)},
                                           "indices": add(idx, 34963, "SCALAR", 5125), "material": 0 if k == 0 else 1, "mode": 4}]})
        nodes = []
        of_mesh = [0] * plain + list(range(1, len(counts) + 1)) + [1 + mirror_of]
        for i, m in enumerate(of_mesh):
            M = np.eye(4)
            M[:3, 3] = [0.7 * (i % 9), 0.0, -0.9 * (i // 9)]
            if i == len(of_mesh) - 1:
                M[0, 0] = -1.0
            nodes.append({"mesh": m, "matrix": M.T.reshape(16).tolist()})      # column-major
        doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": list(range(len(nodes)))}], "nodes": nodes, "meshes": meshes,
               "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.7, 0.7, 1.0]}},
                             {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0]}, "emissiveFactor": [1.0, 0.8, 0.6]}],
               "buffers": [{"uri": "emitters.bin", "byteLength": len(blob)}], "bufferViews": views, "accessors": accessors}
        path = os.path.join(str(tmp), "emitters.gltf")
        with open(os.path.join(str(tmp), "emitters.bin"), "wb") as f:
            f.write(blob)
        with open(path, "w") as f:
            json.dump(doc, f)
        self.sc = host.Scene()
        assert self.sc.load(path)
        self.plain, self.counts = plain, list(counts)
        self.emitter = {m: plain + m for m in range(len(counts))}      # emissive mesh number (0-based among the emitters) -> its first instance
        self.mirrored = len(of_mesh) - 1
        desc = self.sc.desc()
        inst = refit.instances_of(desc)
        assert desc.numInstances == len(of_mesh) and desc.numPrimMeshes == len(counts) + 1
        assert [int(refit.prim_meshes_of(desc)["indexCount"][m]) // 3 for m in inst["primMesh"]] == [([1] + list(counts))[m] for m in of_mesh]
        assert desc.lightInfo.trigLightSize == sum(counts) + counts[mirror_of]

    def prim_mesh(self, m):
        """the prim mesh of emissive mesh m"""
        return int(refit.instances_of(self.sc.desc())["primMesh"][self.emitter[m]])


def positions_moved(desc, mesh, delta):
    """the rows of one prim mesh with every position displaced by a per-vertex amount derived from `delta` (texcoords keep their bits)"""
    first, count = skin.mesh_range(desc, mesh)
    rows = skin.vertices_of(desc)[first:first + count].copy()
    k = np.arange(count, dtype=np.float32)[:, None]
    rows["position"] += (np.float32(delta) * (np.float32(1) + np.float32(0.01) * k)).astype(np.float32)
    return rows

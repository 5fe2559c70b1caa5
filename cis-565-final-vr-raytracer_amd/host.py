"""Python face of the host side (host/scene.hpp, host/hdr_sampling.hpp): scene + environment preparation.

Mirrors the reference call order SampleExample::loadScene / loadEnvironmentHdr / updateUniformBuffer
(src/sample_example.cpp:82-106, 164-173) without Vulkan.
"""
import ctypes as C
import os
import numpy as np
from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.environ.get("RESTIR_HOST_LIB") or os.path.join(_HERE, "host", "librestir_host.so")   # env override: the sanitizer build (tests/test_ingest_fuzz.py)
_lib = None

def host_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} missing: run __graft_entry__.build() first")
        L = C.CDLL(HOST_LIB_PATH)
        L.rth_scene_create.restype = C.c_void_p
        L.rth_env_create.restype = C.c_void_p
        L.rth_env_integral.restype = C.c_float
        L.rth_env_average.restype = C.c_float
        L.rth_scene_light_sources.restype = C.c_uint32
        for name, args in {
            "rth_scene_destroy": [C.c_void_p], "rth_scene_load": [C.c_void_p, C.c_char_p],
            "rth_scene_make_procedural": [C.c_void_p, C.c_int, C.c_float, C.c_uint32], "rth_scene_save_gltf": [C.c_void_p, C.c_char_p], "rth_decode_jpeg": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
            "rth_decode_png": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t], "rth_write_png": [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int],
            "rth_scene_set_camera": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float],
            "rth_scene_get_camera_pose": [C.c_void_p, C.c_void_p], "rth_scene_update_camera": [C.c_void_p, C.c_int, C.c_int],
            "rth_scene_get_camera": [C.c_void_p, C.c_void_p], "rth_scene_light_weights": [C.c_void_p, C.c_void_p, C.c_void_p],
            "rth_scene_update_instances": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32],
            "rth_scene_set_instances": [C.c_void_p, C.c_void_p, C.c_uint32],
            "rth_scene_update_vertices": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
            "rth_scene_set_materials": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32],
            "rth_scene_set_texture": [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_size_t],
            "rth_scene_light_sources": [C.c_void_p, C.c_void_p, C.c_uint32],
            "rth_scene_emitter_meshes": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
            "rth_scene_stats": [C.c_void_p, C.c_void_p], "rth_scene_desc": [C.c_void_p, C.c_void_p, C.c_void_p],
            "rth_env_destroy": [C.c_void_p], "rth_env_load": [C.c_void_p, C.c_char_p], "rth_env_set": [C.c_void_p, C.c_void_p, C.c_int, C.c_int],
            "rth_env_adopt": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float], "rth_env_importance": [C.c_void_p, C.c_void_p],
            "rth_env_make_sky": [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint32], "rth_env_integral": [C.c_void_p], "rth_env_average": [C.c_void_p],
            "rth_env_width": [C.c_void_p], "rth_env_height": [C.c_void_p], "rth_env_get_accel": [C.c_void_p, C.c_void_p],
            "rth_default_state": [C.c_void_p], "rth_alias_table": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
        }.items():
            getattr(L, name).argtypes = args
        _lib = L
    return _lib


class HdrSampling:
    """hdr_sampling.hpp:38-66 (data products only)."""
    def __init__(self):
        self._h = host_lib().rth_env_create()
    def __del__(self):
        if getattr(self, "_h", None) and host_lib is not None:      # (module globals are gone at interpreter shutdown)
            host_lib().rth_env_destroy(self._h); self._h = None
    def loadEnvironment(self, path):
        return host_lib().rth_env_load(self._h, path.encode()) == 0
    def setEnvironment(self, rgba, renderer=None):
        """(h, w, 4) float32 texels.  With a renderer.Renderer: HdrSampling::setEnvironment over a context — the call forwards to rt_set_environment, the table is
        built on the GPU, and getIntegral() / getAverage() / accel() afterwards are the device's (include/rt_abi.h "The environment")"""
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        if renderer is None:
            host_lib().rth_env_set(self._h, a.ctypes.data, a.shape[1], a.shape[0])
            return
        renderer.set_environment(a)
        st, table = renderer.environment_stats(), renderer.environment_readback(abi.ENV_ACCEL)
        host_lib().rth_env_adopt(self._h, a.ctypes.data, a.shape[1], a.shape[0], table.ctypes.data, st.integral, st.average)
    def importance(self):
        """the importances createEnvironmentAccel builds its table from, (h, w) float32"""
        w, h = self.size
        out = np.zeros((h, w), dtype=np.float32)
        host_lib().rth_env_importance(self._h, out.ctypes.data)
        return out
    def makeSyntheticSky(self, w, h, sun_peak=5e4, seed=7):
        host_lib().rth_env_make_sky(self._h, w, h, sun_peak, seed)
    def getIntegral(self): return host_lib().rth_env_integral(self._h)
    def getAverage(self): return host_lib().rth_env_average(self._h)
    @property
    def size(self): return host_lib().rth_env_width(self._h), host_lib().rth_env_height(self._h)
    def accel(self):
        w, h = self.size
        a = np.zeros(w * h, dtype=abi.IMPT_SAMP_DT)
        host_lib().rth_env_get_accel(self._h, a.ctypes.data)
        return a


class Scene:
    """scene.hpp:59-80: setup / load / updateCamera / getCamera / getStat + light weights."""
    STAT_NAMES = ["triangles", "instancedTriangles", "vertices", "primMeshes", "nodes", "materials", "textures", "puncLights", "trigLights"]
    def __init__(self):
        self._h = host_lib().rth_scene_create()
    def __del__(self):
        if getattr(self, "_h", None) and host_lib is not None:
            host_lib().rth_scene_destroy(self._h); self._h = None
    def load(self, filename):
        return host_lib().rth_scene_load(self._h, filename.encode()) == 0
    def saveGltf(self, filename):
        """Write the loaded scene as a self-contained .gltf (host/gltf_loader.cpp writer; exchange/test utility)."""
        return host_lib().rth_scene_save_gltf(self._h, filename.encode()) == 0
    def makeProcedural(self, kind, scale=1.0, seed=1):
        if host_lib().rth_scene_make_procedural(self._h, kind, scale, seed) != 0:
            raise RuntimeError("procedural scene generation failed")
        return self
    def setCamera(self, eye, center, up=(0, 1, 0), fov=45.0):
        e, c, u = (np.asarray(v, dtype=np.float32) for v in (eye, center, up))
        host_lib().rth_scene_set_camera(self._h, e.ctypes.data, c.ctypes.data, u.ctypes.data, fov)
    def cameraPose(self):
        out = np.zeros(10, dtype=np.float32)
        host_lib().rth_scene_get_camera_pose(self._h, out.ctypes.data)
        return out[0:3].copy(), out[3:6].copy(), out[6:9].copy(), float(out[9])
    def updateCamera(self, width, height):
        host_lib().rth_scene_update_camera(self._h, width, height)
    def getCamera(self):
        cam = abi.SceneCamera()
        host_lib().rth_scene_get_camera(self._h, C.byref(cam))
        return cam
    def getStat(self):
        out = np.zeros(9, dtype=np.uint64)
        host_lib().rth_scene_stats(self._h, out.ctypes.data)
        return dict(zip(self.STAT_NAMES, (int(v) for v in out)))
    @property
    def lightWeights(self):
        p, t = C.c_float(), C.c_float()
        host_lib().rth_scene_light_weights(self._h, C.byref(p), C.byref(t))
        return p.value, t.value
    def updateInstances(self, ids, transforms):
        """Scene::updateInstances: move drawable nodes (transforms: (n, 12) float32, 3 x 4 row-major) and recompute the triangle-light records; desc() afterwards
        describes the moved scene"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        xf = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        assert xf.shape[0] == ids.size
        if host_lib().rth_scene_update_instances(self._h, ids.ctypes.data, xf.ctypes.data, ids.size) != 0:
            raise ValueError("Scene.updateInstances: instance id out of range")
    def setInstances(self, inst_array):
        """Scene::setInstances: replace the instance list (abi.INSTANCE_DT records or n x 56 bytes); the nodes, the triangle-light records and the statistics follow;
        desc() afterwards describes the new scene"""
        rows = np.ascontiguousarray(inst_array).view(np.uint8).reshape(-1)
        if rows.size % 56 or host_lib().rth_scene_set_instances(self._h, rows.ctypes.data, rows.size // 56) != 0:
            raise ValueError("Scene.setInstances: an empty table, a row that is not 56 bytes, or a prim mesh out of range")
    def updateVertices(self, prim_mesh, first, rows):
        """Scene::updateVertices: rows (abi.VERTEX_DT records or n x 32 bytes) replace vertices [first, first + n) of one prim mesh; the triangle-light records are
        recomputed; desc() afterwards describes the deformed scene"""
        rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        assert rows.size % 32 == 0
        if host_lib().rth_scene_update_vertices(self._h, int(prim_mesh), int(first), rows.size // 32, rows.ctypes.data) != 0:
            raise ValueError("Scene.updateVertices: prim mesh or vertex range out of bounds")
    def setMaterials(self, ids, rows):
        """Scene::setMaterials: rows (abi.MATERIAL_DT records or n x 80 bytes) replace the material rows `ids`; the triangle-light records follow a changed
        emission; desc() afterwards describes the edited scene (Renderer.update_materials takes the same arguments)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        if rows.size != 80 * ids.size or host_lib().rth_scene_set_materials(self._h, ids.ctypes.data, rows.ctypes.data, ids.size) != 0:
            raise ValueError("Scene.setMaterials: an id out of range, a row that is not 80 bytes, or a row that moves a material across the light rule")
    def setTexture(self, texture, x, y, bgra):
        """Scene::setTexture: bgra (h, w, 4) uint8 replaces the texels at (x, y) of one texture (Renderer.update_texture takes the same arguments)"""
        a = np.ascontiguousarray(bgra, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4 or host_lib().rth_scene_set_texture(self._h, int(texture), int(x), int(y), a.shape[1], a.shape[0], a.ctypes.data, 4 * a.shape[1]) != 0:
            raise ValueError("Scene.setTexture: (h, w, 4) texels inside the texture")
    def lightSources(self):
        """Scene::lightSources: the (instance, triangle) every triangle-light record came from, in record order (abi.LIGHT_SOURCE_DT rows): what
        Renderer.set_light_sources takes"""
        n = host_lib().rth_scene_light_sources(self._h, None, 0)
        out = np.zeros(n, dtype=abi.LIGHT_SOURCE_DT)
        if n:
            host_lib().rth_scene_light_sources(self._h, out.ctypes.data, n)
        return out
    def emitterMeshes(self):
        """Scene::emitterMeshes: (abi.EMITTER_MESH_DT entries, abi.EMITTER_ROW_DT rows), the templates Renderer.set_emitter_meshes takes (with lightWeights[0])"""
        nm, nr = C.c_uint32(0), C.c_uint32(0)
        if host_lib().rth_scene_emitter_meshes(self._h, None, 0, C.byref(nm), None, 0, C.byref(nr)) != 0:
            raise RuntimeError("Scene.emitterMeshes failed")
        meshes, rows = np.zeros(nm.value, dtype=abi.EMITTER_MESH_DT), np.zeros(nr.value, dtype=abi.EMITTER_ROW_DT)
        host_lib().rth_scene_emitter_meshes(self._h, meshes.ctypes.data, nm.value, C.byref(nm), rows.ctypes.data, nr.value, C.byref(nr))
        return meshes, rows
    def desc(self, env=None):
        d = abi.SceneDesc()
        host_lib().rth_scene_desc(self._h, env._h if env is not None else None, C.byref(d))
        return d


def scene_digest(desc):
    """SHA-256 (first 16 hex digits) of everything rt_upload_scene reads from a scene description — prim meshes (20 B), vertices (32 B), indices, instances (56 B),
    materials (80 B), every texture's size / sampler and texels, punctual (80 B) and triangle (96 B) lights, light info — per part and over all of them.  Two scenes with
    the same digest upload the same bytes: the same frames follow (bench.py --via-gltf: the procedural scene against itself written to glTF and read back by Scene::load)."""
    import hashlib

    def raw(ptr, nbytes):
        return bytes((C.c_char * nbytes).from_address(ptr)) if ptr and nbytes else b""
    parts = {"primMeshes": raw(desc.primMeshes, desc.numPrimMeshes * 20), "vertices": raw(desc.vertices, desc.numVertices * 32), "indices": raw(desc.indices, desc.numIndices * 4),
             "instances": raw(desc.instances, desc.numInstances * 56), "materials": raw(desc.materials, desc.numMaterials * 80),
             "puncLights": raw(desc.puncLights, desc.lightInfo.puncLightSize * 80), "trigLights": raw(desc.trigLights, desc.lightInfo.trigLightSize * 96),
             "lightInfo": bytes(desc.lightInfo)}
    h = hashlib.sha256()
    n = int(desc.numTextures)
    if desc.textures and n:
        t = np.frombuffer((C.c_char * (n * 32)).from_address(desc.textures), dtype=np.dtype([("ptr", "<u8"), ("w", "<i4"), ("h", "<i4"), ("rest", "<i4", 4)]))
        for k in range(n):
            h.update(t[k]["w"].tobytes() + t[k]["h"].tobytes() + t[k]["rest"][:3].tobytes())
            h.update(raw(int(t[k]["ptr"]), int(t[k]["w"]) * int(t[k]["h"]) * 4))
    out = {k: hashlib.sha256(v).hexdigest()[:16] for k, v in parts.items()}
    out["textures"] = h.hexdigest()[:16]
    out["all"] = hashlib.sha256("".join(out[k] for k in sorted(out)).encode()).hexdigest()[:16]
    return out


def default_state(width, height, scene=None, env=None, time=1000):
    """RtxState as SampleExample fills it: defaults (sample_example.hpp:154-184) + the derived constants of
    sample_example.cpp:87 (lightLuminIntegInv) and :104-105 (fireflyClampThreshold, envMapLuminIntegInv)."""
    st = abi.RtxState()
    host_lib().rth_default_state(C.byref(st))
    st.size.x, st.size.y = width, height
    st.time = time
    if scene is not None:
        p, t = scene.lightWeights
        st.lightLuminIntegInv = 1.0 / (p + t) if (p + t) > 0 else float("inf")
    if env is not None:
        st.fireflyClampThreshold = env.getIntegral() * 4.0
        st.envMapLuminIntegInv = 1.0 / env.getIntegral()
    return st


def decode_jpeg(data):
    """host/jpeg_decoder.cpp on a bytes object -> (H, W, 4) uint8 BGRA array, or None when the stream is not supported."""
    buf = np.frombuffer(data, dtype=np.uint8)
    w, h = C.c_int(), C.c_int()
    out = np.empty(64 << 20, dtype=np.uint8)
    rc = host_lib().rth_decode_jpeg(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), out.ctypes.data, out.size)
    if rc != 0:
        return None
    return out[: w.value * h.value * 4].reshape(h.value, w.value, 4).copy()


def write_png(path, rgba, keep_alpha=False):
    """host/png_writer.cpp: (H, W, 4) uint8 array, R first (the layout of BUF_LDR) -> 8-bit PNG file."""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = a.shape[:2]
    if host_lib().rth_write_png(path.encode(), a.ctypes.data, w, h, 1 if keep_alpha else 0) != 0:
        raise IOError(f"cannot write {path}")


def decode_png(data):
    """host/gltf_loader.cpp's PNG reader on a bytes object -> (H, W, 4) uint8 BGRA array, or None."""
    buf = np.frombuffer(data, dtype=np.uint8)
    w, h = C.c_int(), C.c_int()
    out = np.empty(64 << 20, dtype=np.uint8)
    if host_lib().rth_decode_png(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), out.ctypes.data, out.size) != 0:
        return None
    return out[: w.value * h.value * 4].reshape(h.value, w.value, 4).copy()

"""Renderer: the reference's stage dispatcher (src/renderer.hpp:49-61) over the C-ABI of csrc/librestir_hip.so.

setup / create / run / update / destroy keep the reference's names and order; the Vulkan handle parameters are gone.
There is no CPU path: if the HIP library or a GPU is missing every entry point raises.
"""
import ctypes as C
import os
import numpy as np
from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("RESTIR_HIP_LIB") or os.path.join(_HERE, "csrc", "librestir_hip.so")  # env override: A/B builds
_lib = None
PRIO_FILTER_SHARE = 0.30   # the threshold of rt_render_frame's stream-priority rule (csrc/rt_api.cpp PRIO_FILTER_SHARE; profiles/r06_prio_rule.txt) — for reports and tests

# every symbol include/rt_abi.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = ["rt_create", "rt_destroy", "rt_set_stream", "rt_upload_scene", "rt_build_accel", "rt_resize", "rt_set_camera",
               "rt_render_frame", "rt_run_stage", "rt_readback", "rt_upload_history", "rt_buffer_bytes", "rt_device_ptr",
               "rt_set_counting", "rt_get_counters", "rt_sync", "rt_last_error", "rt_abi_version", "rt_set_traversal", "rt_set_history_rows", "rt_history_miss", "rt_set_overlap", "rt_tonemap", "rt_set_sun_and_sky", "rt_pick", "rt_trace_rays", "rt_history_miss_stage", "rt_rotate_buffers", "rt_select_frame", "rt_measure_valu_peak", "rt_set_stream_priorities", "rt_get_stream_priorities", "rt_get_streams", "rt_get_stream_layout",
               "rt_reference_render", "rt_reference_reset", "rt_reference_samples", "rt_reference_readback", "rt_reference_tonemap",
               "rt_set_denoiser", "rt_get_denoiser", "rt_denoiser_reset", "rt_denoiser_readback",
               "rt_set_gi_spatial", "rt_get_gi_spatial", "rt_gi_spatial_readback",
               "rt_set_taa", "rt_get_taa", "rt_taa_reset", "rt_taa_readback", "rt_taa_jitter_camera",
               "rt_set_upscale", "rt_get_upscale", "rt_upscale_reset", "rt_upscale_readback", "rt_upscale_tonemap", "rt_upscale_jitter_camera",
               "rt_update_instances", "rt_update_lights", "rt_get_refit_stats", "rt_accel_readback", "rt_rebuild_accel", "rt_get_rebuild_stats", "rt_set_rebuild_options", "rt_get_rebuild_options",
               "rt_set_instances", "rt_get_instances_stats",
               "rt_set_object_motion", "rt_object_motion_camera", "rt_object_motion_readback", "rt_vertex_motion_readback",
               "rt_update_vertices", "rt_set_skins", "rt_update_skins", "rt_vertices_readback", "rt_get_deform_stats",
               "rt_set_light_sources", "rt_lights_readback", "rt_get_light_stats", "rt_set_emitter_meshes", "rt_get_emitter_stats",
               "rt_set_morph_targets", "rt_update_morphs", "rt_get_morph_stats",
               "rt_update_materials", "rt_update_texture", "rt_get_material_stats", "rt_opacity_map",
               "rt_set_environment", "rt_environment_readback", "rt_get_environment_stats", "rt_env_accel", "rt_env_importance", "rt_get_primary_replay_stats", "rt_primary_replay_readback",
               "rt_mgpu_create", "rt_mgpu_destroy", "rt_mgpu_upload_scene", "rt_mgpu_resize", "rt_mgpu_set_camera", "rt_mgpu_render_frame", "rt_mgpu_readback",
               "rt_mgpu_sync", "rt_mgpu_set_balance", "rt_mgpu_set_serialize", "rt_mgpu_set_pipeline", "rt_mgpu_set_gather", "rt_mgpu_set_solo", "rt_mgpu_set_bands", "rt_mgpu_get_stats", "rt_mgpu_get_link_stats", "rt_mgpu_get_stream_layout", "rt_mgpu_last_error", "rt_mgpu_plan_bands"]


def hip_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise RuntimeError(f"{HIP_LIB_PATH} is missing — build it with __graft_entry__.build(); this package has no fallback path")
        # PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).  If torch
        # is loaded first, librestir_hip.so binds to that one runtime and streams / device pointers can be shared with
        # torch.distributed (RCCL).  Loaded the other way round the process ends up with two HIP runtimes and torch then
        # reports "No HIP GPUs are available".  So: when torch is installed, load it first.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(HIP_LIB_PATH)
        L.rt_last_error.restype = C.c_char_p
        L.rt_last_error.argtypes = [C.c_void_p]
        L.rt_buffer_bytes.restype = C.c_size_t
        L.rt_buffer_bytes.argtypes = [C.c_void_p, C.c_int]
        L.rt_abi_version.restype = C.c_uint32
        L.rt_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        for n in ["rt_destroy", "rt_build_accel", "rt_sync"]:
            getattr(L, n).argtypes = [C.c_void_p]
        L.rt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_upload_scene.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_resize.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rt_set_camera.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_render_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rt_run_stage.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5
        L.rt_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.rt_upload_history.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.rt_device_ptr.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.rt_set_counting.argtypes = [C.c_void_p, C.c_int]
        L.rt_set_traversal.argtypes = [C.c_void_p, C.c_int]
        L.rt_set_overlap.argtypes = [C.c_void_p, C.c_int]
        L.rt_tonemap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.rt_set_sun_and_sky.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_history_miss_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rt_rotate_buffers.argtypes = [C.c_void_p, C.c_int]
        L.rt_select_frame.argtypes = [C.c_void_p, C.c_int]
        L.rt_trace_rays.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.rt_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
        L.rt_set_history_rows.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rt_history_miss.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.rt_get_counters.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_measure_valu_peak.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.rt_mgpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]
        for n in ["rt_mgpu_destroy", "rt_mgpu_sync"]:
            getattr(L, n).argtypes = [C.c_void_p]
        L.rt_mgpu_upload_scene.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_mgpu_resize.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rt_mgpu_set_camera.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_mgpu_render_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rt_mgpu_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.rt_mgpu_set_balance.argtypes = [C.c_void_p, C.c_int]
        L.rt_mgpu_set_serialize.argtypes = [C.c_void_p, C.c_int]
        L.rt_mgpu_set_pipeline.argtypes = [C.c_void_p, C.c_int]
        L.rt_mgpu_set_gather.argtypes = [C.c_void_p, C.c_int]
        L.rt_mgpu_set_solo.argtypes = [C.c_void_p, C.c_int]
        L.rt_mgpu_set_bands.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_mgpu_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_mgpu_last_error.argtypes = [C.c_void_p]; L.rt_mgpu_last_error.restype = C.c_char_p
        L.rt_mgpu_plan_bands.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rt_set_stream_priorities.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rt_get_stream_priorities.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_get_streams"):   # (absent from the library round 5 shipped, which scripts/ab_libs2.sh loads through RESTIR_HIP_LIB for same-box A/Bs)
            L.rt_get_streams.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
            L.rt_get_stream_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int * 3)]
            L.rt_mgpu_get_stream_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_reference_render"):   # ABI 2.4 (absent from older A/B libraries loaded through RESTIR_HIP_LIB)
            L.rt_reference_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.rt_reference_reset.argtypes = [C.c_void_p]
            L.rt_reference_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            L.rt_reference_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            L.rt_reference_tonemap.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_denoiser"):   # the denoiser selection (absent from older A/B libraries loaded through RESTIR_HIP_LIB)
            L.rt_set_denoiser.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_get_denoiser.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_denoiser_reset.argtypes = [C.c_void_p]
            L.rt_denoiser_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        if hasattr(L, "rt_set_gi_spatial"):   # the GI spatial reuse (absent from older A/B libraries loaded through RESTIR_HIP_LIB)
            L.rt_set_gi_spatial.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_get_gi_spatial.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_gi_spatial_readback.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        if hasattr(L, "rt_set_taa"):   # temporal anti-aliasing (absent from older A/B libraries loaded through RESTIR_HIP_LIB)
            L.rt_set_taa.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_get_taa.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_taa_reset.argtypes = [C.c_void_p]
            L.rt_taa_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            L.rt_taa_jitter_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        if hasattr(L, "rt_set_upscale"):   # temporal upsampling (absent from older A/B libraries loaded through RESTIR_HIP_LIB)
            L.rt_set_upscale.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_get_upscale.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_upscale_reset.argtypes = [C.c_void_p]
            L.rt_upscale_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            L.rt_upscale_tonemap.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.rt_upscale_jitter_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_update_instances"):   # moving instances (absent from older A/B libraries loaded through RESTIR_HIP_LIB)
            L.rt_update_instances.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.rt_update_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
            L.rt_get_refit_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_accel_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        if hasattr(L, "rt_rebuild_accel"):   # rebuilding on the device (absent from older A/B libraries)
            L.rt_rebuild_accel.argtypes = [C.c_void_p]
            L.rt_get_rebuild_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_rebuild_options"):   # the PLOC builder of the device rebuild (absent from older A/B libraries)
            L.rt_set_rebuild_options.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_get_rebuild_options.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_instances"):   # adding and removing instances (absent from older A/B libraries)
            L.rt_set_instances.argtypes = abi.SET_INSTANCES_ARGTYPES
            L.rt_get_instances_stats.argtypes = abi.GET_INSTANCES_STATS_ARGTYPES
        if hasattr(L, "rt_set_object_motion"):   # object motion vectors (absent from older A/B libraries)
            L.rt_set_object_motion.argtypes = [C.c_void_p, C.c_int]
            L.rt_object_motion_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.rt_object_motion_readback.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        if hasattr(L, "rt_vertex_motion_readback"):   # per-vertex motion vectors (absent from older A/B libraries)
            L.rt_vertex_motion_readback.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        if hasattr(L, "rt_update_vertices"):   # deforming meshes (absent from older A/B libraries)
            L.rt_update_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
            L.rt_set_skins.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
            L.rt_update_skins.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.rt_vertices_readback.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
            L.rt_get_deform_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_light_sources"):   # light sources (absent from older A/B libraries)
            L.rt_set_light_sources.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            L.rt_lights_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            L.rt_get_light_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_emitter_meshes"):   # emitters (absent from older A/B libraries)
            L.rt_set_emitter_meshes.argtypes = abi.SET_EMITTER_MESHES_ARGTYPES
            L.rt_get_emitter_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_morph_targets"):   # morph targets (absent from older A/B libraries)
            L.rt_set_morph_targets.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
            L.rt_update_morphs.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.rt_get_morph_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_update_materials"):   # editing materials and textures (absent from older A/B libraries)
            L.rt_update_materials.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.rt_update_texture.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_size_t]
            L.rt_get_material_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_opacity_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_set_environment"):   # the environment (absent from older A/B libraries)
            L.rt_set_environment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            L.rt_environment_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            L.rt_get_environment_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_env_accel.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.rt_env_importance.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_get_primary_replay_stats"):   # settled primary visibility (absent from older A/B libraries)
            L.rt_get_primary_replay_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_primary_replay_readback.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rt_accel_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.rt_accel_quality.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib = L
    return _lib


class RtError(RuntimeError):
    pass


class _DevArray:
    """Zero-copy view of a ctx-owned HBM buffer for torch.as_tensor / RCCL (via __cuda_array_interface__)."""
    def __init__(self, ptr, nbytes, owner):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}
        self._owner = owner


class Renderer:
    def __init__(self):
        self._h = None
        self.size = (0, 0)

    # Renderer::setup (renderer.cpp:62-73)
    def setup(self, device=0):
        h = C.c_void_p()
        rc = hip_lib().rt_create(C.byref(h), device)
        if rc != 0:
            raise RtError(f"rt_create failed ({rc}): {hip_lib().rt_last_error(None).decode()}")
        self._h = h
        return self

    def _chk(self, rc, what):
        if rc != 0:
            raise RtError(f"{what} failed ({rc}): {hip_lib().rt_last_error(self._h).decode()}")

    # Renderer::destroy (renderer.cpp:75-91)
    def destroy(self):
        if self._h:
            hip_lib().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # AccelStructure::create + the upload half of Scene::load / HdrSampling::loadEnvironment
    def load_scene(self, desc):
        self._chk(hip_lib().rt_upload_scene(self._h, C.byref(desc)), "rt_upload_scene")
        self._chk(hip_lib().rt_build_accel(self._h), "rt_build_accel")

    # Renderer::create (renderer.cpp:97-148) / Renderer::update (renderer.cpp:209-225)
    def create(self, width, height, scene=None, env=None):
        if scene is not None:
            self.load_scene(scene.desc(env))
        self.update(width, height)
        return self

    def update(self, width, height):
        self._chk(hip_lib().rt_resize(self._h, width, height), "rt_resize")
        self.size = (width, height)

    def set_camera(self, cam):
        self._chk(hip_lib().rt_set_camera(self._h, C.byref(cam)), "rt_set_camera")
        self.camera = type(cam).from_buffer_copy(cam)   # the camera the next launches will use (hosts that defer work re-set it)

    def set_stream(self, stream_ptr):
        self._chk(hip_lib().rt_set_stream(self._h, stream_ptr), "rt_set_stream")

    # Renderer::run (renderer.cpp:154-206)
    def run(self, state, frames):
        self._chk(hip_lib().rt_render_frame(self._h, C.byref(state), frames), "rt_render_frame")

    def run_stage(self, state, frames, stage, level=0, row_begin=0, row_end=0):
        self._chk(hip_lib().rt_run_stage(self._h, C.byref(state), frames, stage, level, row_begin, row_end), "rt_run_stage")

    def sync(self):
        self._chk(hip_lib().rt_sync(self._h), "rt_sync")

    def buffer_bytes(self, buf):
        return hip_lib().rt_buffer_bytes(self._h, buf)

    def readback(self, buf):
        out = np.empty(self.buffer_bytes(buf), dtype=np.uint8)
        self._chk(hip_lib().rt_readback(self._h, buf, out.ctypes.data, out.nbytes), "rt_readback")
        return out

    def upload_history(self, buf, data):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self._chk(hip_lib().rt_upload_history(self._h, buf, a.ctypes.data, a.nbytes), "rt_upload_history")

    def device_array(self, buf):
        p, n, pitch = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._chk(hip_lib().rt_device_ptr(self._h, buf, C.byref(p), C.byref(n), C.byref(pitch)), "rt_device_ptr")
        return _DevArray(p.value, n.value, self), pitch.value

    def set_traversal(self, mode):
        """abi.TRAVERSAL_AUTO (per launch, by its size) / TRAVERSAL_THROUGHPUT / TRAVERSAL_LATENCY: which build of the traced kernels runs; same bits."""
        self._chk(hip_lib().rt_set_traversal(self._h, int(mode)), "rt_set_traversal")

    def tonemap(self, tm=None, debugging_mode=0, frames=0):
        """RenderOutput::run (render_output.cpp:224-237): post.frag over the result images of `frames` -> BUF_LDR (RGBA8)."""
        tm = tm if tm is not None else abi.Tonemapper()
        self._chk(hip_lib().rt_tonemap(self._h, C.byref(tm), debugging_mode, frames), "rt_tonemap")

    def pick(self, view_inv, proj_inv, x, y):
        """SampleExample::screenPicking (sample_example.cpp:456-497): x, y = normalised window position; returns abi.PickResult."""
        out = abi.PickResult()
        self._chk(hip_lib().rt_pick(self._h, C.byref(view_inv), C.byref(proj_inv), x, y, C.byref(out)), "rt_pick")
        return out

    def trace_closest(self, rays):
        """rays: (n, 8) float32 (origin, direction, tmax, seed bits) -> (n, 4) float32: t, triangle index bits, u, v  (the oracle's trace_closest format)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        out = np.zeros((rays.shape[0], 4), dtype=np.float32)
        self._chk(hip_lib().rt_trace_rays(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data, 0), "rt_trace_rays")
        return out

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        out = np.zeros((rays.shape[0], 4), dtype=np.float32)
        self._chk(hip_lib().rt_trace_rays(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data, 1), "rt_trace_rays")
        return (out[:, 0] > 0.5).astype(np.int32)

    def set_sun_and_sky(self, ss):
        """updateUniformBuffer's SunAndSky upload (sample_example.cpp:172); ss.in_use = 1 switches the environment to the procedural sky."""
        self._chk(hip_lib().rt_set_sun_and_sky(self._h, C.byref(ss)), "rt_set_sun_and_sky")

    def select_frame(self, frames):
        """RT_BUF_DENOISE_IND_A exists once per frame parity: name the one of `frames` for the next device_array / readback."""
        self._chk(hip_lib().rt_select_frame(self._h, int(frames)), "rt_select_frame")

    def set_overlap(self, mode):
        """0 = serial launches, 1 = direct A-Trous beside the indirect stage, 2 = 1 + frames in flight (default), 3 = 2 with a third frame in flight."""
        self._chk(hip_lib().rt_set_overlap(self._h, int(mode)), "rt_set_overlap")

    def history_miss_stage(self, stage):
        m = C.c_int()
        self._chk(hip_lib().rt_history_miss_stage(self._h, stage, C.byref(m)), "rt_history_miss_stage")
        return bool(m.value)

    def rotate_buffers(self, frames):
        self._chk(hip_lib().rt_rotate_buffers(self._h, frames), "rt_rotate_buffers")

    def set_history_rows(self, row0, row1):
        self._chk(hip_lib().rt_set_history_rows(self._h, row0, row1), "rt_set_history_rows")

    def history_miss(self):
        m = C.c_int()
        self._chk(hip_lib().rt_history_miss(self._h, C.byref(m)), "rt_history_miss")
        return bool(m.value)

    def set_counting(self, enable):
        self._chk(hip_lib().rt_set_counting(self._h, 1 if enable else 0), "rt_set_counting")

    def counters(self):
        c = abi.Counters()
        self._chk(hip_lib().rt_get_counters(self._h, C.byref(c)), "rt_get_counters")
        return c

    def measure_valu_peak(self, variant=0, waves_per_simd=8):
        """wave-level VALU instructions per second of a chain-free loop on this device (csrc/microbench.hip)"""
        v = C.c_double()
        self._chk(hip_lib().rt_measure_valu_peak(self._h, variant, waves_per_simd, C.byref(v)), "rt_measure_valu_peak")
        return v.value

    def set_stream_priorities(self, indirect_level, filter_level):
        """levels -1 / 0 / +1 of the indirect-stage stream and the filter stream of the frames-in-flight schedule (same bits under every setting)"""
        self._chk(hip_lib().rt_set_stream_priorities(self._h, int(indirect_level), int(filter_level)), "rt_set_stream_priorities")

    def stream_priorities(self):
        """{"chosen": [indirect, filter], "filter_share": filters / (direct + indirect) of the last probe frame or None, "decided": bool} (rt_get_stream_priorities)"""
        a, b, sh, d = C.c_int(), C.c_int(), C.c_float(), C.c_int()
        self._chk(hip_lib().rt_get_stream_priorities(self._h, C.byref(a), C.byref(b), C.byref(sh), C.byref(d)), "rt_get_stream_priorities")
        return {"chosen": [a.value, b.value], "filter_share": (round(sh.value, 4) if sh.value >= 0 else None), "decided": bool(d.value)}

    def streams(self):
        """{"main", "ind", "side"}: the context's three hipStream_t handles of the frames-in-flight schedule (rt_get_streams; created on first call — filter stream, then
        indirect stream — with the current levels).  A host that issues the stages itself runs on these (restir_amd/tiled.py) instead of on streams of its own."""
        m, i, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(hip_lib().rt_get_streams(self._h, C.byref(m), C.byref(i), C.byref(f)), "rt_get_streams")
        return {"main": m.value, "ind": i.value, "side": f.value}

    def stream_layout(self):
        """{"library_streams_created": n, "creation_index": {"main": i, "ind": j, "side": k}} (rt_get_stream_layout; -1 = not created)"""
        n, idx = C.c_int(), (C.c_int * 3)()
        self._chk(hip_lib().rt_get_stream_layout(self._h, C.byref(n), C.byref(idx)), "rt_get_stream_layout")
        return {"library_streams_created": n.value, "creation_index": {"main": idx[0], "ind": idx[1], "side": idx[2]}}

    # ---- reference mode (ABI 2.4): the progressive ground-truth path tracer (include/rt_abi.h)
    def reference_render(self, state, samples):
        """add `samples` samples per pixel to the reference sums (n resets where an input of the integral changed: see rt_abi.h)"""
        self._chk(hip_lib().rt_reference_render(self._h, C.byref(state), int(samples)), "rt_reference_render")

    def reference_reset(self):
        self._chk(hip_lib().rt_reference_reset(self._h), "rt_reference_reset")

    def reference_samples(self):
        n = C.c_uint32()
        self._chk(hip_lib().rt_reference_samples(self._h, C.byref(n)), "rt_reference_samples")
        return n.value

    def reference_readback(self, component=abi.REF_SUM):
        """(H, W, 4) float32 mean of abi.REF_DIRECT / REF_INDIRECT / REF_SUM, a = 1"""
        W, H = self.size
        out = np.empty((H, W, 4), dtype=np.float32)
        self._chk(hip_lib().rt_reference_readback(self._h, int(component), out.ctypes.data, out.nbytes), "rt_reference_readback")
        return out

    def reference_tonemap(self, tm=None):
        """post.frag over the two reference means -> BUF_LDR (RGBA8)"""
        tm = tm if tm is not None else abi.Tonemapper()
        self._chk(hip_lib().rt_reference_tonemap(self._h, C.byref(tm)), "rt_reference_tonemap")

    # ---- denoiser selection: A-Trous (default) or SVGF (include/rt_abi.h)
    def set_denoiser(self, d=None, **kw):
        """rt_set_denoiser with an abi.Denoiser, or the library defaults overridden by keywords (set_denoiser(mode=abi.DENOISER_SVGF))"""
        d = d if d is not None else abi.Denoiser(**kw)
        self._chk(hip_lib().rt_set_denoiser(self._h, C.byref(d)), "rt_set_denoiser")

    def get_denoiser(self):
        d = abi.Denoiser()
        self._chk(hip_lib().rt_get_denoiser(self._h, C.byref(d)), "rt_get_denoiser")
        return d

    def denoiser_reset(self):
        self._chk(hip_lib().rt_denoiser_reset(self._h), "rt_denoiser_reset")

    def denoiser_readback(self, which):
        """the SVGF history the last SVGF frame wrote: abi.SVGF_DIRECT_COLOR / _INDIRECT_COLOR -> (h, w, 4) float32 (colour, n);
        abi.SVGF_DIRECT_MOMENTS / _INDIRECT_MOMENTS -> (h, w, 2) float32 (m1, m2); the indirect ones at half resolution"""
        W, H = self.size
        w, h = (W // 2, H // 2) if which in (abi.SVGF_INDIRECT_COLOR, abi.SVGF_INDIRECT_MOMENTS) else (W, H)
        out = np.empty((h, w, 4 if which in (abi.SVGF_DIRECT_COLOR, abi.SVGF_INDIRECT_COLOR) else 2), dtype=np.float32)
        self._chk(hip_lib().rt_denoiser_readback(self._h, int(which), out.ctypes.data, out.nbytes), "rt_denoiser_readback")
        return out

    # ---- ReSTIR GI spatial reuse (include/rt_abi.h)
    def set_gi_spatial(self, s=None, **kw):
        """rt_set_gi_spatial with an abi.GiSpatial, or the library defaults overridden by keywords (set_gi_spatial(mode=abi.GI_SPATIAL_ON))"""
        s = s if s is not None else abi.GiSpatial(**kw)
        self._chk(hip_lib().rt_set_gi_spatial(self._h, C.byref(s)), "rt_set_gi_spatial")

    def get_gi_spatial(self):
        s = abi.GiSpatial()
        self._chk(hip_lib().rt_get_gi_spatial(self._h, C.byref(s)), "rt_get_gi_spatial")
        return s

    def gi_spatial_readback(self):
        """the spatially resampled reservoirs of the last frame rendered with the mode on: rt_indirect_reservoir records as raw bytes,
        (W/2) * (H/2) * 76 (the layout of rt_readback(RT_BUF_INDIRECT_RESV0))"""
        W, H = self.size
        out = np.empty((W // 2) * (H // 2) * 76, dtype=np.uint8)
        self._chk(hip_lib().rt_gi_spatial_readback(self._h, out.ctypes.data, out.nbytes), "rt_gi_spatial_readback")
        return out

    # ---- temporal anti-aliasing (include/rt_abi.h)
    def set_taa(self, t=None, **kw):
        """rt_set_taa with an abi.Taa, or the library defaults overridden by keywords (set_taa(mode=abi.TAA_ON))"""
        t = t if t is not None else abi.Taa(**kw)
        self._chk(hip_lib().rt_set_taa(self._h, C.byref(t)), "rt_set_taa")

    def get_taa(self):
        t = abi.Taa()
        self._chk(hip_lib().rt_get_taa(self._h, C.byref(t)), "rt_get_taa")
        return t

    def taa_reset(self):
        self._chk(hip_lib().rt_taa_reset(self._h), "rt_taa_reset")

    def taa_readback(self, which):
        """the last resolved frame: abi.TAA_DIRECT / TAA_INDIRECT -> (H, W, 4) float32; abi.TAA_HISTORY_LENGTH -> (H, W) float32 n"""
        W, H = self.size
        out = np.empty((H, W, 4) if which in (abi.TAA_DIRECT, abi.TAA_INDIRECT) else (H, W), dtype=np.float32)
        self._chk(hip_lib().rt_taa_readback(self._h, int(which), out.ctypes.data, out.nbytes), "rt_taa_readback")
        return out

    @staticmethod
    def taa_jitter_camera(cam, frames, jitter_phases, width, height):
        """rt_taa_jitter_camera (no context, no GPU): the camera the context renders frame `frames` with when TAA is on"""
        out = abi.SceneCamera()
        rc = hip_lib().rt_taa_jitter_camera(C.byref(cam), int(frames), int(jitter_phases), int(width), int(height), C.byref(out))
        if rc != 0:
            raise RtError(f"rt_taa_jitter_camera failed ({rc})")
        return out

    # ---- temporal upsampling (include/rt_abi.h "Temporal upsampling")
    def set_upscale(self, u=None, **kw):
        """rt_set_upscale with an abi.Upscale, or the library defaults overridden by keywords (set_upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=.., outHeight=..))"""
        u = u if u is not None else abi.Upscale(**kw)
        self._chk(hip_lib().rt_set_upscale(self._h, C.byref(u)), "rt_set_upscale")

    def get_upscale(self):
        u = abi.Upscale()
        self._chk(hip_lib().rt_get_upscale(self._h, C.byref(u)), "rt_get_upscale")
        return u

    def upscale_reset(self):
        self._chk(hip_lib().rt_upscale_reset(self._h), "rt_upscale_reset")

    def upscale_readback(self, which):
        """the last resolved frame at the output size: abi.UPSCALE_DIRECT / UPSCALE_INDIRECT -> (Ho, Wo, 4) float32; UPSCALE_HISTORY_LENGTH -> (Ho, Wo) float32 n;
        UPSCALE_LDR -> (Ho, Wo, 4) uint8, what upscale_tonemap last wrote"""
        u = self.get_upscale()
        Wo, Ho = u.outWidth, u.outHeight
        if which == abi.UPSCALE_LDR:
            out = np.empty((Ho, Wo, 4), dtype=np.uint8)
        else:
            out = np.empty((Ho, Wo, 4) if which in (abi.UPSCALE_DIRECT, abi.UPSCALE_INDIRECT) else (Ho, Wo), dtype=np.float32)
        self._chk(hip_lib().rt_upscale_readback(self._h, int(which), out.ctypes.data, out.nbytes), "rt_upscale_readback")
        return out

    def upscale_tonemap(self, tm, frames):
        """rt_upscale_tonemap: the post pass over the resolved images of frame `frames` at the output size (read it with upscale_readback(abi.UPSCALE_LDR))"""
        self._chk(hip_lib().rt_upscale_tonemap(self._h, C.byref(tm), int(frames)), "rt_upscale_tonemap")

    @staticmethod
    def upscale_jitter_camera(cam, frames, jitter_phases, width, height):
        """rt_upscale_jitter_camera (no context, no GPU): (the camera the context renders frame `frames` with at the render size width x height when temporal
        upsampling is on, the jitter offset (dx, dy) in render pixels as float32)"""
        out = abi.SceneCamera()
        delta = (C.c_float * 2)()
        rc = hip_lib().rt_upscale_jitter_camera(C.byref(cam), int(frames), int(jitter_phases), int(width), int(height), C.byref(out), delta)
        if rc != 0:
            raise RtError(f"rt_upscale_jitter_camera failed ({rc})")
        return out, np.array([delta[0], delta[1]], dtype=np.float32)

    # ---- moving instances (include/rt_abi.h "Moving instances")
    def update_instances(self, ids, transforms):
        """rt_update_instances: ids (n,) and transforms (n, 12) float32, 3 x 4 row-major like rt_instance::objectToWorld.  Rewrites the moved instances' leaf records
        and refits the BVH8 above them on the GPU; drains the frames in flight"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        xf = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1)
        if xf.size != 12 * ids.size:
            raise ValueError("update_instances: 12 floats per id")
        self._chk(hip_lib().rt_update_instances(self._h, ids.size, ids.ctypes.data, xf.ctypes.data), "rt_update_instances")

    def update_lights(self, desc):
        """rt_update_lights with the light records of a scene description (Scene.updateInstances recomputes them for moved emitters)"""
        nt = desc.lightInfo.trigLightSize if desc.trigLights else 0
        npu = desc.lightInfo.puncLightSize if desc.puncLights else 0
        self._chk(hip_lib().rt_update_lights(self._h, desc.trigLights, nt, desc.puncLights, npu, C.byref(desc.lightInfo)), "rt_update_lights")

    def refit_stats(self):
        s = abi.RefitStats()
        self._chk(hip_lib().rt_get_refit_stats(self._h, C.byref(s)), "rt_get_refit_stats")
        return s

    # ---- rebuilding on the device (include/rt_abi.h "Rebuilding on the device")
    def rebuild_accel(self):
        """rt_rebuild_accel: a new BVH8 topology built on the GPU from the scene as it is after the update_instances calls so far; drains the frames in flight"""
        self._chk(hip_lib().rt_rebuild_accel(self._h), "rt_rebuild_accel")

    def rebuild_stats(self):
        s = abi.RebuildStats()
        self._chk(hip_lib().rt_get_rebuild_stats(self._h, C.byref(s)), "rt_get_rebuild_stats")
        return s

    def set_rebuild_options(self, builder=abi.REBUILD_LBVH, radius=0, max_iterations=0):
        """rt_set_rebuild_options: the builder of every later device build (rebuild_accel, set_instances) — abi.REBUILD_LBVH or abi.REBUILD_PLOC with its search
        radius (1..64) and iteration cap; 0 = the default.  Builds nothing (include/rt_abi.h "The PLOC builder")"""
        o = abi.RebuildOptions(int(builder), int(radius), int(max_iterations), 0)
        self._chk(hip_lib().rt_set_rebuild_options(self._h, C.byref(o)), "rt_set_rebuild_options")

    def rebuild_options(self):
        """rt_get_rebuild_options: the values in force, defaults filled in"""
        o = abi.RebuildOptions()
        self._chk(hip_lib().rt_get_rebuild_options(self._h, C.byref(o)), "rt_get_rebuild_options")
        return o

    # ---- adding and removing instances (include/rt_abi.h "Adding and removing instances")
    def set_instances(self, inst_array):
        """rt_set_instances: inst_array = abi.INSTANCE_DT records (or n x 56 bytes), the whole new instance table.  Expands it into the device builder's input and
        builds a new tree on the GPU; drains the frames in flight.  Emissive instances must stay in place (include/rt_abi.h, the emitter rule)"""
        rows = np.ascontiguousarray(inst_array).view(np.uint8).reshape(-1)
        if rows.size % 56:
            raise ValueError("set_instances: 56 bytes per instance")
        self._chk(hip_lib().rt_set_instances(self._h, rows.size // 56, rows.ctypes.data), "rt_set_instances")

    def instances_stats(self):
        s = abi.InstancesStats()
        self._chk(hip_lib().rt_get_instances_stats(self._h, C.byref(s)), "rt_get_instances_stats")
        return s

    # ---- deforming meshes (include/rt_abi.h "Deforming meshes")
    def update_vertices(self, prim_mesh, first_vertex, rows):
        """rt_update_vertices: rows = abi.VERTEX_DT records (or n x 32 bytes) that replace rows [first_vertex, first_vertex + n) of one prim mesh; every instance of
        the mesh is refitted on the GPU; drains the frames in flight"""
        rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        if rows.size % 32:
            raise ValueError("update_vertices: 32 bytes per row")
        self._chk(hip_lib().rt_update_vertices(self._h, int(prim_mesh), int(first_vertex), rows.size // 32, rows.ctypes.data), "rt_update_vertices")

    def set_skins(self, skins, influences):
        """rt_set_skins: skins = abi.SKIN_DT records (one per skinned prim mesh), influences = abi.SKIN_INFLUENCE_DT records; captures the rest pose.  Empty: removes the skins"""
        sk = np.ascontiguousarray(skins, dtype=abi.SKIN_DT).reshape(-1)
        inf = np.ascontiguousarray(influences, dtype=abi.SKIN_INFLUENCE_DT).reshape(-1)
        self._chk(hip_lib().rt_set_skins(self._h, sk.size, sk.ctypes.data, inf.size, inf.ctypes.data), "rt_set_skins")

    def update_skins(self, skin_ids, joint_matrices):
        """rt_update_skins: re-poses the listed skins on the GPU; joint_matrices = per listed skin jointCount x 12 floats (3 x 4 row-major), concatenated"""
        ids = np.ascontiguousarray(skin_ids, dtype=np.uint32).reshape(-1)
        m = np.ascontiguousarray(joint_matrices, dtype=np.float32).reshape(-1)
        self._chk(hip_lib().rt_update_skins(self._h, ids.size, ids.ctypes.data, m.ctypes.data), "rt_update_skins")

    def vertices_readback(self, first_vertex, count):
        """the device vertex array as it is now: abi.VERTEX_DT records"""
        out = np.zeros(int(count), dtype=abi.VERTEX_DT)
        self._chk(hip_lib().rt_vertices_readback(self._h, int(first_vertex), int(count), out.ctypes.data), "rt_vertices_readback")
        return out

    def deform_stats(self):
        s = abi.DeformStats()
        self._chk(hip_lib().rt_get_deform_stats(self._h, C.byref(s)), "rt_get_deform_stats")
        return s

    # ---- morph targets (include/rt_abi.h "Morph targets")
    def set_morph_targets(self, sets, deltas):
        """rt_set_morph_targets: sets = abi.MORPH_SET_DT records (one per morphed prim mesh), deltas = abi.MORPH_DELTA_DT rows (or n x 3 / n x 4 floats), target-major:
        per target the position plane, then the normal plane, then the tangent plane, vertexCount rows each.  Skins first.  Empty: removes the sets"""
        st = np.ascontiguousarray(sets, dtype=abi.MORPH_SET_DT).reshape(-1)
        d = np.asarray(deltas)
        if d.dtype != abi.MORPH_DELTA_DT:
            f = np.asarray(d, dtype=np.float32).reshape(-1, d.shape[-1] if d.ndim > 1 else 4)
            d = np.zeros(len(f), abi.MORPH_DELTA_DT)
            d["d"] = f[:, :3]
        d = np.ascontiguousarray(d).reshape(-1)
        self._chk(hip_lib().rt_set_morph_targets(self._h, st.size, st.ctypes.data, d.size, d.ctypes.data), "rt_set_morph_targets")

    def update_morphs(self, set_ids, weights):
        """rt_update_morphs: stores the weights (per listed set targetCount floats, concatenated) and re-poses the listed meshes from their rest pose on the GPU;
        a mesh that also has a skin is skinned with the matrices of its last update_skins"""
        ids = np.ascontiguousarray(set_ids, dtype=np.uint32).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        self._chk(hip_lib().rt_update_morphs(self._h, ids.size, ids.ctypes.data, w.ctypes.data), "rt_update_morphs")

    def morph_stats(self):
        s = abi.MorphStats()
        self._chk(hip_lib().rt_get_morph_stats(self._h, C.byref(s)), "rt_get_morph_stats")
        return s

    # ---- editing materials and textures (include/rt_abi.h "Editing materials and textures")
    def update_materials(self, ids, rows):
        """rt_update_materials: rows = abi.MATERIAL_DT records (or n x 80 bytes) that replace the material rows `ids`; the alpha records and opacity micro-maps of
        the triangles whose alpha parameters or base colour texture changed are re-derived on the GPU; drains the frames in flight"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        if rows.size != 80 * ids.size:
            raise ValueError("update_materials: 80 bytes per id")
        self._chk(hip_lib().rt_update_materials(self._h, ids.size, ids.ctypes.data, rows.ctypes.data), "rt_update_materials")

    def update_texture(self, texture, x, y, bgra, row_pitch=None):
        """rt_update_texture: bgra = (h, w, 4) uint8 texels that replace the rectangle at (x, y) of one texture.  row_pitch (bytes): the texels are handed over in
        a staging buffer whose rows are that far apart (the padding is filled with 0xA5 and never read); a pitch below 4 w is passed on for the library to refuse"""
        a = np.ascontiguousarray(bgra, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("update_texture: (h, w, 4) uint8 texels")
        h, w = a.shape[0], a.shape[1]
        pitch = 4 * w if row_pitch is None else int(row_pitch)
        if pitch != 4 * w:   # a padded copy with the rows `pitch` bytes apart: what a host with a wider staging buffer hands over
            if pitch < 4 * w:
                self._chk(hip_lib().rt_update_texture(self._h, int(texture), int(x), int(y), w, h, a.ctypes.data, pitch), "rt_update_texture")
                return
            buf = np.full((h, pitch), 0xA5, dtype=np.uint8)
            buf[:, :4 * w] = a.reshape(h, 4 * w)
            a = buf
        self._chk(hip_lib().rt_update_texture(self._h, int(texture), int(x), int(y), w, h, a.ctypes.data, pitch), "rt_update_texture")

    def material_stats(self):
        s = abi.MaterialStats()
        self._chk(hip_lib().rt_get_material_stats(self._h, C.byref(s)), "rt_get_material_stats")
        return s

    @staticmethod
    def opacity_map(uv, base_alpha, cutoff, alpha_mode, bgra=None, wrap_s=10497, wrap_t=10497, filter=9729):
        """rt_opacity_map (no context, no GPU): the four micro-map words of one triangle — uv = 6 floats (uv0 uv1 uv2), bgra = (h, w, 4) uint8 or None"""
        d = abi.OpacityMapDesc()
        d.uv[:] = [float(v) for v in np.asarray(uv, dtype=np.float32).reshape(6)]
        d.baseAlpha, d.cutoff, d.alphaMode, d.wrapS, d.wrapT, d.filter = float(base_alpha), float(cutoff), int(alpha_mode), int(wrap_s), int(wrap_t), int(filter)
        tex = None
        if bgra is not None:
            tex = np.ascontiguousarray(bgra, dtype=np.uint8)
            d.h, d.w = tex.shape[0], tex.shape[1]
        out = (C.c_uint32 * 4)()
        rc = hip_lib().rt_opacity_map(C.byref(d), tex.ctypes.data if tex is not None else None, out)
        if rc != 0:
            raise RtError(f"rt_opacity_map failed ({rc})")
        return np.array(list(out), dtype=np.uint32)

    # ---- the environment (include/rt_abi.h "The environment")
    def set_environment(self, rgba, accel=None):
        """rt_set_environment: rgba = (h, w, 4) float32 texels (None: the 1 x 1 black map); accel = abi.IMPT_SAMP_DT rows to copy, or None: the table is built on
        the GPU by the rule of csrc/env_accel.h.  Afterwards environment_stats().integral is what rt_state.envMapLuminIntegInv is the inverse of."""
        if rgba is None:
            self._chk(hip_lib().rt_set_environment(self._h, 0, 0, None, None), "rt_set_environment")
            return
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("set_environment: (h, w, 4) float32 texels")
        t = None
        if accel is not None:
            t = np.ascontiguousarray(accel).view(np.uint8).reshape(-1)
            if t.size != 16 * a.shape[0] * a.shape[1]:
                raise ValueError("set_environment: 16 bytes of table per texel")
        self._chk(hip_lib().rt_set_environment(self._h, a.shape[1], a.shape[0], a.ctypes.data, t.ctypes.data if t is not None else None), "rt_set_environment")

    def environment_stats(self):
        s = abi.EnvironmentStats()
        self._chk(hip_lib().rt_get_environment_stats(self._h, C.byref(s)), "rt_get_environment_stats")
        return s

    def environment_readback(self, which):
        """rt_environment_readback: abi.ENV_TEXELS -> (h, w, 4) float32, abi.ENV_ACCEL -> w h abi.IMPT_SAMP_DT rows, of the environment in use"""
        st = self.environment_stats()
        out = np.empty(st.width * st.height * 16, dtype=np.uint8)
        self._chk(hip_lib().rt_environment_readback(self._h, int(which), out.ctypes.data, out.nbytes), "rt_environment_readback")
        return out.view(np.float32).reshape(st.height, st.width, 4) if which == abi.ENV_TEXELS else out.view(abi.IMPT_SAMP_DT)

    @staticmethod
    def env_accel(rgba):
        """rt_env_accel (no context, no GPU): (abi.IMPT_SAMP_DT rows, integral, average) of (h, w, 4) float32 texels, by the rule of csrc/env_accel.h"""
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        out = np.zeros(a.shape[0] * a.shape[1], dtype=abi.IMPT_SAMP_DT)
        integral, average = C.c_float(), C.c_float()
        rc = hip_lib().rt_env_accel(a.shape[1], a.shape[0], a.ctypes.data, out.ctypes.data, C.byref(integral), C.byref(average))
        if rc != 0:
            raise RtError(f"rt_env_accel failed ({rc})")
        return out, integral.value, average.value

    @staticmethod
    def env_importance(rgba):
        """rt_env_importance (no context, no GPU): step 1 of the rule, (h, w) float32"""
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        out = np.zeros(a.shape[:2], dtype=np.float32)
        rc = hip_lib().rt_env_importance(a.shape[1], a.shape[0], a.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise RtError(f"rt_env_importance failed ({rc})")
        return out

    def primary_replay_stats(self):
        """rt_get_primary_replay_stats: state, K, the pixel classes of the recording in force and the launches recorded / replayed"""
        s = abi.PrimaryReplayStats()
        self._chk(hip_lib().rt_get_primary_replay_stats(self._h, C.byref(s)), "rt_get_primary_replay_stats")
        return s

    def primary_replay_readback(self, width, height):
        """rt_primary_replay_readback: the count plane of the recording in force, (height, width) uint32 — listed candidates per pixel, 0xffffffff = overflow"""
        out = np.empty((height, width), dtype=np.uint32)
        self._chk(hip_lib().rt_primary_replay_readback(self._h, out.ctypes.data, out.nbytes), "rt_primary_replay_readback")
        return out

    # ---- light sources (include/rt_abi.h "Light sources")
    def set_light_sources(self, sources):
        """rt_set_light_sources: sources = abi.LIGHT_SOURCE_DT records, one per uploaded triangle-light record (host.Scene.lightSources()); the update calls then
        rewrite the records of the instances they refit on the GPU.  Empty: removes the binding"""
        src = np.ascontiguousarray(sources, dtype=abi.LIGHT_SOURCE_DT).reshape(-1)
        self._chk(hip_lib().rt_set_light_sources(self._h, src.size, src.ctypes.data), "rt_set_light_sources")

    def lights_readback(self, which=abi.LIGHTS_TRIG, count=None):
        """the device light array as it is now: abi.TRIG_LIGHT_DT (96 B) or abi.PUNC_LIGHT_DT (80 B) records; count defaults to the bound record count"""
        if count is None:
            count = self.light_stats().bound
        out = np.zeros(int(count), dtype=abi.TRIG_LIGHT_DT if which == abi.LIGHTS_TRIG else abi.PUNC_LIGHT_DT)
        self._chk(hip_lib().rt_lights_readback(self._h, int(which), out.ctypes.data, out.nbytes), "rt_lights_readback")
        return out

    def light_stats(self):
        s = abi.LightStats()
        self._chk(hip_lib().rt_get_light_stats(self._h, C.byref(s)), "rt_get_light_stats")
        return s

    # ---- emitters (include/rt_abi.h "Emitters")
    def set_emitter_meshes(self, meshes=None, rows=None, punc_light_weight=0.0):
        """rt_set_emitter_meshes: meshes / rows = abi.EMITTER_MESH_DT / abi.EMITTER_ROW_DT records (host.Scene.emitterMeshes()), punc_light_weight = the scene's
        punctual weight (host.Scene.lightWeights[0]).  Switches the emitter mode on: set_instances then derives the triangle-light records of the new table on the
        GPU, so emissive instances may be added and removed.  No meshes: switches it off"""
        m = np.zeros(0, abi.EMITTER_MESH_DT) if meshes is None else np.ascontiguousarray(meshes, dtype=abi.EMITTER_MESH_DT).reshape(-1)
        r = np.zeros(0, abi.EMITTER_ROW_DT) if rows is None else np.ascontiguousarray(rows, dtype=abi.EMITTER_ROW_DT).reshape(-1)
        self._chk(hip_lib().rt_set_emitter_meshes(self._h, m.size, m.ctypes.data if m.size else None, r.size, r.ctypes.data if r.size else None,
                                                  C.c_float(punc_light_weight)), "rt_set_emitter_meshes")

    def emitter_stats(self):
        s = abi.EmitterStats()
        self._chk(hip_lib().rt_get_emitter_stats(self._h, C.byref(s)), "rt_get_emitter_stats")
        return s

    # ---- object motion vectors (include/rt_abi.h "Object motion vectors")
    def set_object_motion(self, mode):
        """rt_set_object_motion: abi.OBJECT_MOTION_OFF (default) / OBJECT_MOTION_ON / OBJECT_MOTION_VERTEX (per-vertex motion vectors)"""
        self._chk(hip_lib().rt_set_object_motion(self._h, int(mode)), "rt_set_object_motion")

    def object_motion_readback(self):
        """the instance image of the last frame rendered with the mode on: (H, W) uint32, 0xffffffff where the primary ray missed"""
        nbytes = self.buffer_bytes(abi.BUF_MOTION)   # 4 B per full-resolution pixel
        out = np.empty(nbytes // 4, dtype=np.uint32)
        self._chk(hip_lib().rt_object_motion_readback(self._h, out.ctypes.data, out.nbytes), "rt_object_motion_readback")
        return out

    def vertex_motion_readback(self):
        """the delta image of the last frame rendered with OBJECT_MOTION_VERTEX: (W * H, 4) float32, x_prev - position in .xyz, zero at a miss and where nothing moved"""
        n = self.buffer_bytes(abi.BUF_MOTION) // 4
        out = np.empty((n, 4), dtype=np.float32)
        self._chk(hip_lib().rt_vertex_motion_readback(self._h, out.ctypes.data, out.nbytes), "rt_vertex_motion_readback")
        return out

    @staticmethod
    def object_motion_camera(cam, prev, cur):
        """rt_object_motion_camera (no context, no GPU): the per-instance previous camera for an instance that moved from objectToWorld `prev` to `cur` (12 floats each)"""
        p = np.ascontiguousarray(prev, dtype=np.float32).reshape(12)
        c = np.ascontiguousarray(cur, dtype=np.float32).reshape(12)
        out = abi.SceneCamera()
        rc = hip_lib().rt_object_motion_camera(C.byref(cam), p.ctypes.data, c.ctypes.data, C.byref(out))
        if rc != 0:
            raise RtError(f"rt_object_motion_camera failed ({rc})")
        return out

    def accel_readback(self, which, num_instances=None):
        """the device tree as raw bytes: abi.ACCEL_NODES (80 B per node), ACCEL_TRIS (64 B per leaf record), ACCEL_INSTANCES (112 B per instance; pass num_instances),
        ACCEL_ALPHA (64 B per alpha record, view as abi.ALPHA_REC_DT; num_instances is then the record count, or None: 1 + the largest alphaIdx of the leaf records)"""
        st = self.accel_stats()
        if which == abi.ACCEL_ALPHA and num_instances is None:
            tris = self.accel_readback(abi.ACCEL_TRIS).view(np.uint32).reshape(-1, 16)
            num_instances = int(tris[:, 11].max()) + 1 if len(tris) else 1
        count = {abi.ACCEL_NODES: st["nodes"], abi.ACCEL_TRIS: st["references"], abi.ACCEL_INSTANCES: num_instances, abi.ACCEL_ALPHA: num_instances}[which]
        out = np.empty(int(count) * abi.ACCEL_RECORD_BYTES[which], dtype=np.uint8)
        self._chk(hip_lib().rt_accel_readback(self._h, int(which), out.ctypes.data, out.nbytes), "rt_accel_readback")
        return out

    def accel_stats(self):
        n, t, d = C.c_uint64(), C.c_uint64(), C.c_int()
        self._chk(hip_lib().rt_accel_stats(self._h, C.byref(n), C.byref(t), C.byref(d)), "rt_accel_stats")
        refs, sp, sn, stt = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double()
        self._chk(hip_lib().rt_accel_quality(self._h, C.byref(refs), C.byref(sp), C.byref(sn), C.byref(stt)), "rt_accel_quality")
        return {"nodes": n.value, "triangles": t.value, "max_depth": d.value, "references": refs.value, "spatial_splits": sp.value,
                "sah_node_steps": round(sn.value, 3), "sah_tri_steps": round(stt.value, 3)}


class MgpuStats(C.Structure):  # rt_mgpu_stats
    _fields_ = [("numRanks", C.c_int32), ("frames", C.c_uint32), ("historyFallbacks", C.c_uint32), ("pad", C.c_uint32), ("haloBytes", C.c_uint64),
                ("bandBegin", C.c_int32 * 16), ("bandEnd", C.c_int32 * 16), ("tracedMs", C.c_float * 16), ("filterMs", C.c_float * 16), ("haloBytesKind", C.c_uint64 * 6), ("haloBytesRankKind", (C.c_uint64 * 6) * 16)]


class MgpuLinkStats(C.Structure):  # rt_mgpu_link_stats (ABI 2.1)
    _fields_ = [("numRanks", C.c_int32), ("devices", C.c_int32 * 16), ("peerAccess", (C.c_uint8 * 16) * 16), ("pullMs", (C.c_float * 4) * 16), ("pullBytes", (C.c_uint64 * 4) * 16)]


LINK_GROUPS = ("history", "history_indirect", "filter_direct", "filter_indirect")


class MultiGpuRenderer:
    """rt_mgpu_*: one process drives N devices (csrc/mgpu.cpp) — the Renderer interface over the native row-tiled frame."""
    def __init__(self):
        self._h = None
        self.size = (0, 0)

    def setup(self, devices):
        devices = list(devices)
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = hip_lib().rt_mgpu_create(C.byref(h), len(devices), arr)
        if rc != 0:
            raise RtError(f"rt_mgpu_create failed ({rc}): {hip_lib().rt_last_error(None).decode()}")
        self._h, self.world = h, len(devices)
        return self

    def _chk(self, rc, what):
        if rc != 0:
            raise RtError(f"{what} failed ({rc}): {hip_lib().rt_mgpu_last_error(self._h).decode()}")

    def destroy(self):
        if self._h:
            hip_lib().rt_mgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def load_scene(self, desc): self._chk(hip_lib().rt_mgpu_upload_scene(self._h, C.byref(desc)), "rt_mgpu_upload_scene")
    def update(self, width, height):
        self._chk(hip_lib().rt_mgpu_resize(self._h, width, height), "rt_mgpu_resize")
        self.size = (width, height)
    def set_camera(self, cam): self._chk(hip_lib().rt_mgpu_set_camera(self._h, C.byref(cam)), "rt_mgpu_set_camera")
    def run(self, state, frames): self._chk(hip_lib().rt_mgpu_render_frame(self._h, C.byref(state), frames), "rt_mgpu_render_frame")
    def sync(self): self._chk(hip_lib().rt_mgpu_sync(self._h), "rt_mgpu_sync")
    def set_balance(self, on): self._chk(hip_lib().rt_mgpu_set_balance(self._h, int(on)), "rt_mgpu_set_balance")   # True / 1: cost weighted, False / 0: equal, 2: freeze
    def set_serialize(self, on): self._chk(hip_lib().rt_mgpu_set_serialize(self._h, 1 if on else 0), "rt_mgpu_set_serialize")
    def set_pipeline(self, on): self._chk(hip_lib().rt_mgpu_set_pipeline(self._h, 1 if on else 0), "rt_mgpu_set_pipeline")
    def set_gather(self, on): self._chk(hip_lib().rt_mgpu_set_gather(self._h, 1 if on else 0), "rt_mgpu_set_gather")
    def set_solo(self, rank): self._chk(hip_lib().rt_mgpu_set_solo(self._h, int(rank)), "rt_mgpu_set_solo")
    def set_bands(self, bands):
        arr = (C.c_int * len(bands))(*[int(b) for b in bands])
        self._chk(hip_lib().rt_mgpu_set_bands(self._h, arr), "rt_mgpu_set_bands")
    @staticmethod
    def plan_bands(height, ranks, stripe_cost, prev=None, max_move=-1):
        cost = (C.c_float * len(stripe_cost))(*[float(x) for x in stripe_cost])
        pb = (C.c_int * (ranks + 1))(*prev) if prev is not None else None
        out = (C.c_int * (ranks + 1))()
        rc = hip_lib().rt_mgpu_plan_bands(height, ranks, cost, pb, max_move, out)
        if rc != 0:
            raise RtError(f"rt_mgpu_plan_bands failed ({rc})")
        return list(out)
    def stats(self):
        s = MgpuStats()
        self._chk(hip_lib().rt_mgpu_get_stats(self._h, C.byref(s)), "rt_mgpu_get_stats")
        return s
    def stream_layout(self):
        """per rank: creation index of its main / indirect / filter stream in the process (-1 = not created yet), + the levels (rt_mgpu_get_stream_layout)"""
        n = self.world
        created, idx, lv = C.c_int(), (C.c_int * (3 * n))(), (C.c_int * 3)()
        self._chk(hip_lib().rt_mgpu_get_stream_layout(self._h, C.byref(created), idx, lv), "rt_mgpu_get_stream_layout")
        return {"library_streams_created": created.value, "levels_main_ind_side": [lv[0], lv[1], lv[2]],
                "creation_index": [{"main": idx[3 * r], "ind": idx[3 * r + 1], "side": idx[3 * r + 2]} for r in range(n)]}
    def link_stats(self):
        s = MgpuLinkStats()
        self._chk(hip_lib().rt_mgpu_get_link_stats(self._h, C.byref(s)), "rt_mgpu_get_link_stats")
        return s
    def readback(self, buf):
        W, H = self.size
        half = buf in (abi.BUF_INDIRECT_RESV0, abi.BUF_INDIRECT_RESV0 + 1, abi.BUF_INDIRECT_RESV0 + 2)
        elem = {abi.BUF_MOTION: 4, abi.BUF_LIGHT_ID0: 4, abi.BUF_LIGHT_ID0 + 1: 4, abi.BUF_LDR: 4, abi.BUF_DIRECT_RESV0: 36, abi.BUF_DIRECT_RESV0 + 1: 36,
                abi.BUF_DIRECT_RESV0 + 2: 36, abi.BUF_INDIRECT_RESV0: 76, abi.BUF_INDIRECT_RESV0 + 1: 76, abi.BUF_INDIRECT_RESV0 + 2: 76}.get(buf, 16)
        n = ((W // 2) * (H // 2) if half else W * H) * elem
        out = np.empty(n, dtype=np.uint8)
        self._chk(hip_lib().rt_mgpu_readback(self._h, buf, out.ctypes.data, out.nbytes), "rt_mgpu_readback")
        return out

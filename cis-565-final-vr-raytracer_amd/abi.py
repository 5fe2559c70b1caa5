"""ctypes mirrors of include/rt_abi.h (the data contract of shaders/host_device.h:153-333)."""
import ctypes as C
import numpy as np

class Vec2(C.Structure): _fields_ = [("x", C.c_float), ("y", C.c_float)]
class Vec3(C.Structure): _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]
class Vec4(C.Structure): _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]
class IVec2(C.Structure): _fields_ = [("x", C.c_int32), ("y", C.c_int32)]
class Mat4(C.Structure): _fields_ = [("m", C.c_float * 16)]

class SceneCamera(C.Structure):  # host_device.h:153-165
    _fields_ = [("viewInverse", Mat4), ("projInverse", Mat4), ("projView", Mat4), ("lastView", Mat4),
                ("lastProjView", Mat4), ("lastPosition", Vec3), ("nbLights", C.c_int32)]

class RtxState(C.Structure):  # host_device.h:207-238
    _fields_ = [("frame", C.c_int32), ("maxDepth", C.c_int32), ("modulate", C.c_int32), ("fireflyClampThreshold", C.c_float),
                ("hdrMultiplier", C.c_float), ("debugging_mode", C.c_int32), ("environmentProb", C.c_float), ("time", C.c_uint32),
                ("ReSTIRState", C.c_int32), ("RISSampleNum", C.c_int32), ("reservoirClamp", C.c_int32), ("accumulate", C.c_int32),
                ("size", IVec2), ("envMapLuminIntegInv", C.c_float), ("lightLuminIntegInv", C.c_float), ("MIS", C.c_int32),
                ("sigLuminDirect", C.c_float), ("sigNormalDirect", C.c_float), ("sigDepthDirect", C.c_float), ("denoise", C.c_int32),
                ("sigLuminIndirect", C.c_float), ("sigNormalIndirect", C.c_float), ("sigDepthIndirect", C.c_float), ("denoiseLevel", C.c_int32)]

class ImptSamp(C.Structure): _fields_ = [("alias", C.c_int32), ("q", C.c_float), ("pdf", C.c_float), ("aliasPdf", C.c_float)]
class LightBufInfo(C.Structure): _fields_ = [("puncLightSize", C.c_uint32), ("trigLightSize", C.c_uint32), ("trigSampProb", C.c_float), ("pad", C.c_int32)]

class SceneDesc(C.Structure):  # rt_scene_desc
    _fields_ = [("numPrimMeshes", C.c_uint32), ("primMeshes", C.c_void_p),
                ("numVertices", C.c_uint64), ("vertices", C.c_void_p),
                ("numIndices", C.c_uint64), ("indices", C.c_void_p),
                ("numInstances", C.c_uint32), ("instances", C.c_void_p),
                ("numMaterials", C.c_uint32), ("materials", C.c_void_p),
                ("numTextures", C.c_uint32), ("textures", C.c_void_p),
                ("puncLights", C.c_void_p), ("trigLights", C.c_void_p), ("lightInfo", LightBufInfo),
                ("envWidth", C.c_int32), ("envHeight", C.c_int32), ("envRgba32f", C.c_void_p), ("envAccel", C.c_void_p)]

class Tonemapper(C.Structure):  # rt_tonemapper (host_device.h:336-351); defaults = RenderOutput::m_tm (render_output.hpp:44-55)
    _fields_ = [("brightness", C.c_float), ("contrast", C.c_float), ("saturation", C.c_float), ("vignette", C.c_float), ("avgLum", C.c_float), ("zoom", C.c_float),
                ("renderingRatio", C.c_float * 2), ("autoExposure", C.c_int32), ("Ywhite", C.c_float), ("key", C.c_float), ("pad", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        self.brightness = self.contrast = self.saturation = 1.0; self.vignette = 0.0; self.avgLum = 1.0; self.zoom = 1.0
        self.renderingRatio[0] = self.renderingRatio[1] = 1.0; self.autoExposure = 0; self.Ywhite = 0.5; self.key = 0.5
        for k, v in kw.items():
            setattr(self, k, v)

assert C.sizeof(Tonemapper) == 48

class SunAndSky(C.Structure):  # rt_sun_and_sky (host_device.h:353-377); defaults = SampleExample::m_sunAndSky (sample_example.hpp:186-203)
    _fields_ = [("rgb_unit_conversion", C.c_float * 3), ("multiplier", C.c_float), ("haze", C.c_float), ("redblueshift", C.c_float), ("saturation", C.c_float),
                ("horizon_height", C.c_float), ("ground_color", C.c_float * 3), ("horizon_blur", C.c_float), ("night_color", C.c_float * 3),
                ("sun_disk_intensity", C.c_float), ("sun_direction", C.c_float * 3), ("sun_disk_scale", C.c_float), ("sun_glow_intensity", C.c_float),
                ("y_is_up", C.c_int32), ("physically_scaled_sun", C.c_int32), ("in_use", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        self.rgb_unit_conversion[:] = [1, 1, 1]; self.multiplier = 0.0000101320; self.haze = 0.0; self.redblueshift = 0.0; self.saturation = 1.0
        self.horizon_height = 0.0; self.ground_color[:] = [0.4, 0.4, 0.4]; self.horizon_blur = 0.1; self.night_color[:] = [0.0, 0.0, 0.01]
        self.sun_disk_intensity = 0.8; self.sun_direction[:] = [0.0, 0.78, 0.62]; self.sun_disk_scale = 5.0; self.sun_glow_intensity = 1.0
        self.y_is_up = 1; self.physically_scaled_sun = 1; self.in_use = 0
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                getattr(self, k)[:] = v
            else:
                setattr(self, k, v)

assert C.sizeof(SunAndSky) == 96

class PickResult(C.Structure):  # rt_pick_result == nvvk::RayPickerKHR::PickResult
    _fields_ = [("worldRayOrigin", C.c_float * 4), ("worldRayDirection", C.c_float * 4), ("hitT", C.c_float), ("primitiveID", C.c_int32), ("instanceID", C.c_int32),
                ("instanceCustomIndex", C.c_int32), ("baryCoord", C.c_float * 3)]
RT_STAGE_COUNT = 7
TRAVERSAL_AUTO, TRAVERSAL_THROUGHPUT, TRAVERSAL_LATENCY = 0, 1, 2   # rt_set_traversal
class Counters(C.Structure):  # rt_counters
    _fields_ = [("closestHitRays", C.c_uint64), ("anyHitRays", C.c_uint64), ("nodesVisited", C.c_uint64), ("trisTested", C.c_uint64),
                ("hitsShaded", C.c_uint64), ("risCandidates", C.c_uint64), ("stageMs", C.c_float * RT_STAGE_COUNT), ("frameMs", C.c_float), ("framesTimed", C.c_uint32),
                ("laneRounds", C.c_uint64), ("laneLiveRounds", C.c_uint64)]

assert C.sizeof(SceneCamera) == 336 and C.sizeof(RtxState) == 100

# rt_buffer_id
(BUF_GBUFFER0, BUF_GBUFFER1, BUF_MOTION, BUF_DIRECT_RESV0, BUF_DIRECT_RESV1, BUF_DIRECT_RESV_TEMP, BUF_INDIRECT_RESV0,
 BUF_INDIRECT_RESV1, BUF_INDIRECT_RESV_TEMP, BUF_DENOISE_DIR_A, BUF_DENOISE_DIR_B, BUF_DENOISE_IND_A, BUF_DENOISE_IND_B,
 BUF_DIRECT_RESULT0, BUF_DIRECT_RESULT1, BUF_INDIRECT_RESULT0, BUF_INDIRECT_RESULT1, BUF_LIGHT_ID0, BUF_LIGHT_ID1, BUF_LDR, BUF_COUNT) = range(21)
BUFFER_NAMES = ["gbuffer0", "gbuffer1", "motion", "direct_resv0", "direct_resv1", "direct_resv_temp", "indirect_resv0", "indirect_resv1",
                "indirect_resv_temp", "denoise_dir_a", "denoise_dir_b", "denoise_ind_a", "denoise_ind_b", "direct_result0", "direct_result1",
                "indirect_result0", "indirect_result1", "light_id0", "light_id1", "ldr"]
# rt_reference_readback components
REF_DIRECT, REF_INDIRECT, REF_SUM = range(3)
# rt_status (include/rt_abi.h)
(OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NO_SCENE, ERR_NO_ACCEL, ERR_NO_TARGET, ERR_OOM) = (0, -1, -2, -3, -4, -5, -6, -7)
# rt_set_denoiser (include/rt_abi.h "Denoiser selection"); rt_denoiser_readback ids
DENOISER_ATROUS, DENOISER_SVGF = range(2)
SVGF_DIRECT_COLOR, SVGF_INDIRECT_COLOR, SVGF_DIRECT_MOMENTS, SVGF_INDIRECT_MOMENTS = range(4)


class Denoiser(C.Structure):  # rt_denoiser, 32 B; defaults = the library's
    _fields_ = [("mode", C.c_int32), ("alphaColor", C.c_float), ("alphaMoments", C.c_float), ("historyCap", C.c_int32),
                ("phiLumDirect", C.c_float), ("phiLumIndirect", C.c_float), ("reserved", C.c_int32 * 2)]

    def __init__(self, **kw):
        d = dict(mode=DENOISER_ATROUS, alphaColor=0.2, alphaMoments=0.2, historyCap=32, phiLumDirect=4.0, phiLumIndirect=4.0)
        d.update(kw)
        super().__init__(**d)
# rt_set_gi_spatial (include/rt_abi.h "ReSTIR GI spatial reuse")
GI_SPATIAL_OFF, GI_SPATIAL_ON, GI_SPATIAL_VISIBILITY = range(3)


class GiSpatial(C.Structure):  # rt_gi_spatial, 32 B; defaults = the library's
    _fields_ = [("mode", C.c_int32), ("samples", C.c_int32), ("radius", C.c_int32), ("normalThreshold", C.c_float),
                ("depthThreshold", C.c_float), ("jacobianMax", C.c_float), ("reserved", C.c_int32 * 2)]

    def __init__(self, **kw):
        d = dict(mode=GI_SPATIAL_OFF, samples=4, radius=10, normalThreshold=0.9, depthThreshold=0.1, jacobianMax=10.0)
        d.update(kw)
        super().__init__(**d)
# rt_set_taa (include/rt_abi.h "Temporal anti-aliasing"); rt_taa_readback ids
TAA_OFF, TAA_ON = range(2)
TAA_DIRECT, TAA_INDIRECT, TAA_HISTORY_LENGTH = range(3)


class Taa(C.Structure):  # rt_taa, 32 B; defaults = the library's
    _fields_ = [("mode", C.c_int32), ("jitterPhases", C.c_int32), ("alpha", C.c_float), ("clipGamma", C.c_float), ("reserved", C.c_int32 * 4)]

    def __init__(self, **kw):
        d = dict(mode=TAA_OFF, jitterPhases=8, alpha=0.1, clipGamma=1.0)
        d.update(kw)
        super().__init__(**d)
# rt_set_upscale (include/rt_abi.h "Temporal upsampling"); rt_upscale_readback ids
UPSCALE_OFF, UPSCALE_TEMPORAL = range(2)
UPSCALE_DIRECT, UPSCALE_INDIRECT, UPSCALE_HISTORY_LENGTH, UPSCALE_LDR = range(4)


class Upscale(C.Structure):  # rt_upscale, 32 B; defaults = the library's
    _fields_ = [("mode", C.c_int32), ("outWidth", C.c_int32), ("outHeight", C.c_int32), ("jitterPhases", C.c_int32), ("alpha", C.c_float),
                ("clipGamma", C.c_float), ("reserved", C.c_int32 * 2)]

    def __init__(self, **kw):
        d = dict(mode=UPSCALE_OFF, outWidth=0, outHeight=0, jitterPhases=16, alpha=0.1, clipGamma=1.0)
        d.update(kw)
        super().__init__(**d)
# rt_stage_id
(STAGE_DIRECT, STAGE_INDIRECT, STAGE_DENOISE_DIRECT, STAGE_DENOISE_INDIRECT, STAGE_COMPOSE, STAGE_DIRECT_GEN, STAGE_DIRECT_REUSE) = range(7)
# rt_restir_state
RESTIR_NONE, RESTIR_RIS, RESTIR_SPATIAL, RESTIR_TEMPORAL, RESTIR_SPATIOTEMPORAL = range(5)
# ProcScene (host/scene.hpp)
PROC_CORNELL, PROC_HELMET, PROC_SPONZA, PROC_BISTRO_EXT, PROC_BISTRO_INT, PROC_BISTRO_EXT_REAL, PROC_SPONZA_1K = range(7)
# rt_accel_readback ids; record sizes of the device tree (csrc/bvh8.h, csrc/dev_scene.h)
ACCEL_NODES, ACCEL_TRIS, ACCEL_INSTANCES, ACCEL_ALPHA = range(4)
ACCEL_RECORD_BYTES = (80, 64, 112, 64)
# rt_accel_readback(ACCEL_ALPHA): the alpha records (csrc/bvh8.h AlphaRec) with the texel address replaced by the texture's index, all ones for none
ALPHA_REC_DT = np.dtype([("uv", "<f4", 6), ("baseAlpha", "<f4"), ("cutoff", "<f4"), ("texture", "<u8"), ("w", "<i4"), ("h", "<i4"), ("wrapS", "<i4"),
                         ("wrapT", "<i4"), ("filter", "<i4"), ("alphaMode", "<i4")])
# rt_material (80 B) as a numpy row
MATERIAL_DT = np.dtype([("pbrBaseColorFactor", "<f4", 4), ("pbrBaseColorTexture", "<i4"), ("pbrMetallicFactor", "<f4"), ("pbrRoughnessFactor", "<f4"),
                        ("pbrMetallicRoughnessTexture", "<i4"), ("emissiveTexture", "<i4"), ("emissiveFactor", "<f4", 3), ("normalTexture", "<i4"),
                        ("normalTextureScale", "<f4"), ("transmissionFactor", "<f4"), ("transmissionTexture", "<i4"), ("ior", "<f4"), ("alphaMode", "<i4"),
                        ("alphaCutoff", "<f4"), ("pad", "<i4")])


class OpacityMapDesc(C.Structure):  # rt_opacity_map_desc, 64 B
    _fields_ = [("uv", C.c_float * 6), ("baseAlpha", C.c_float), ("cutoff", C.c_float), ("alphaMode", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("wrapS", C.c_int32), ("wrapT", C.c_int32), ("filter", C.c_int32), ("reserved", C.c_uint32 * 2)]


class MaterialStats(C.Structure):  # rt_material_stats, 32 B
    _fields_ = [("materialsWritten", C.c_uint32), ("dirtyMaterials", C.c_uint32), ("alphaRecords", C.c_uint32), ("leafRecords", C.c_uint32),
                ("texelsScanned", C.c_uint64), ("bytesUploaded", C.c_uint32), ("ms", C.c_float)]


assert ALPHA_REC_DT.itemsize == 64 and MATERIAL_DT.itemsize == 80 and C.sizeof(OpacityMapDesc) == 64 and C.sizeof(MaterialStats) == 32
# rt_environment_readback ids; rt_impt_samp (16 B) as a numpy row
ENV_TEXELS, ENV_ACCEL = range(2)
IMPT_SAMP_DT = np.dtype([("alias", "<i4"), ("q", "<f4"), ("pdf", "<f4"), ("aliasPdf", "<f4")])
ENV_MAX_TEXELS = 1 << 23   # the device build's (and rt_env_accel's) limit


class EnvironmentStats(C.Structure):  # rt_environment_stats, 40 B
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("integral", C.c_float), ("average", C.c_float), ("numSmall", C.c_uint32), ("numLarge", C.c_uint32),
                ("builtOnDevice", C.c_uint32), ("ms", C.c_float), ("deviceBytes", C.c_uint64)]


assert IMPT_SAMP_DT.itemsize == 16 and C.sizeof(EnvironmentStats) == 40
OBJECT_MOTION_OFF, OBJECT_MOTION_ON, OBJECT_MOTION_VERTEX = 0, 1, 3   # rt_set_object_motion (VERTEX: per-vertex motion vectors; 2 is not a mode)


class RebuildStats(C.Structure):  # rt_rebuild_stats, 32 B
    _fields_ = [("triangles", C.c_uint32), ("nodes", C.c_uint32), ("levels", C.c_uint32), ("maxDepth", C.c_uint32), ("ms", C.c_float), ("sortMs", C.c_float),
                ("triPad", C.c_float), ("iterations", C.c_uint32)]


REBUILD_LBVH, REBUILD_PLOC = 0, 1   # rt_rebuild_options.builder


class RebuildOptions(C.Structure):  # rt_rebuild_options, 16 B
    _fields_ = [("builder", C.c_int32), ("radius", C.c_int32), ("maxIterations", C.c_int32), ("reserved", C.c_int32)]


class InstancesStats(C.Structure):  # rt_instances_stats, 32 B
    _fields_ = [("instances", C.c_uint32), ("triangles", C.c_uint32), ("added", C.c_uint32), ("removed", C.c_uint32), ("bytesUploaded", C.c_uint32),
                ("reallocated", C.c_uint32), ("expandMs", C.c_float), ("ms", C.c_float)]


INSTANCE_DT = np.dtype([("objectToWorld", "<f4", 12), ("primMesh", "<u4"), ("flags", "<u4")])   # rt_instance, 56 B
# int rt_set_instances(rt_ctx*, uint32_t numInstances, const rt_instance*); int rt_get_instances_stats(rt_ctx*, rt_instances_stats*)
SET_INSTANCES_ARGTYPES = [C.c_void_p, C.c_uint32, C.c_void_p]
GET_INSTANCES_STATS_ARGTYPES = [C.c_void_p, C.c_void_p]


class DeformStats(C.Structure):  # rt_deform_stats, 32 B
    _fields_ = [("meshes", C.c_uint32), ("vertices", C.c_uint32), ("instances", C.c_uint32), ("vertexBytesCopied", C.c_uint32), ("skinMs", C.c_float), ("ms", C.c_float),
                ("reserved", C.c_uint32 * 2)]


# rt_skin (16 B) and rt_skin_influence (24 B) as numpy rows; rt_vertex (32 B)
SKIN_DT = np.dtype([("primMesh", "<u4"), ("firstJoint", "<u4"), ("jointCount", "<u4"), ("firstInfluence", "<u4")])
SKIN_INFLUENCE_DT = np.dtype([("joint", "<u2", 4), ("weight", "<f4", 4)])
VERTEX_DT = np.dtype([("position", "<f4", 3), ("normal", "<u4"), ("texcoord", "<f4", 2), ("tangent", "<u4"), ("color", "<u4")])


# rt_set_morph_targets / rt_update_morphs: rt_morph_set (16 B) and rt_morph_delta (16 B) as numpy rows
MORPH_NORMALS, MORPH_TANGENTS = 1, 2
MORPH_SET_DT = np.dtype([("primMesh", "<u4"), ("targetCount", "<u4"), ("firstDelta", "<u4"), ("planes", "<u4")])
MORPH_DELTA_DT = np.dtype([("d", "<f4", 3), ("pad", "<f4")])


class MorphStats(C.Structure):  # rt_morph_stats, 32 B
    _fields_ = [("sets", C.c_uint32), ("vertices", C.c_uint32), ("targetsApplied", C.c_uint32), ("instances", C.c_uint32), ("morphMs", C.c_float), ("ms", C.c_float),
                ("reserved", C.c_uint32 * 2)]


assert MORPH_SET_DT.itemsize == 16 and MORPH_DELTA_DT.itemsize == 16 and C.sizeof(MorphStats) == 32


class PrimaryReplayStats(C.Structure):  # rt_primary_replay_stats, 32 B
    _fields_ = [("state", C.c_uint32), ("K", C.c_uint32), ("pixelsSettled", C.c_uint32), ("pixelsListed", C.c_uint32), ("pixelsOverflow", C.c_uint32),
                ("launchesRecorded", C.c_uint32), ("launchesReplayed", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(PrimaryReplayStats) == 32


class LightStats(C.Structure):  # rt_light_stats, 32 B
    _fields_ = [("bound", C.c_uint32), ("rewritten", C.c_uint32), ("lightBytesCopied", C.c_uint32), ("ms", C.c_float), ("reserved", C.c_uint32 * 4)]


# rt_set_light_sources / rt_lights_readback: rt_light_source (8 B), rt_trig_light (96 B) and rt_punc_light (80 B) as numpy rows
LIGHTS_TRIG, LIGHTS_PUNC = range(2)
LIGHT_SOURCE_DT = np.dtype([("instance", "<u4"), ("triangle", "<u4")])
_IMPT_SAMP_DT = np.dtype([("alias", "<i4"), ("q", "<f4"), ("pdf", "<f4"), ("aliasPdf", "<f4")])
TRIG_LIGHT_DT = np.dtype([("matIndex", "<u4"), ("transformIndex", "<u4"), ("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3),
                          ("uv0", "<f4", 2), ("uv1", "<f4", 2), ("uv2", "<f4", 2), ("impSamp", _IMPT_SAMP_DT), ("pad", "<f4", 3)])
PUNC_LIGHT_DT = np.dtype([("type", "<i4"), ("direction", "<f4", 3), ("intensity", "<f4"), ("color", "<f4", 3), ("position", "<f4", 3), ("range", "<f4"),
                          ("outerConeCos", "<f4"), ("innerConeCos", "<f4"), ("padding", "<f4", 2), ("impSamp", _IMPT_SAMP_DT)])
assert LIGHT_SOURCE_DT.itemsize == 8 and TRIG_LIGHT_DT.itemsize == 96 and PUNC_LIGHT_DT.itemsize == 80 and C.sizeof(LightStats) == 32


class EmitterStats(C.Structure):  # rt_emitter_stats, 32 B
    _fields_ = [("enabled", C.c_uint32), ("records", C.c_uint32), ("emittingInstances", C.c_uint32), ("bytesUploaded", C.c_uint32), ("reallocated", C.c_uint32),
                ("expandMs", C.c_float), ("reserved", C.c_uint32 * 2)]


# rt_set_emitter_meshes (include/rt_abi.h "Emitters"): rt_emitter_mesh (16 B) and rt_emitter_row (32 B) as numpy rows
EMITTER_MESH_DT = np.dtype([("primMesh", "<u4"), ("firstRow", "<u4"), ("rowCount", "<u4"), ("reserved", "<u4")])
EMITTER_ROW_DT = np.dtype([("triangle", "<u4"), ("uv", "<f4", 6), ("pad", "<u4")])
# int rt_set_emitter_meshes(rt_ctx*, uint32_t numMeshes, const rt_emitter_mesh*, uint32_t numRows, const rt_emitter_row*, float puncLightWeight)
SET_EMITTER_MESHES_ARGTYPES = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float]
assert EMITTER_MESH_DT.itemsize == 16 and EMITTER_ROW_DT.itemsize == 32 and C.sizeof(EmitterStats) == 32


class RefitStats(C.Structure):  # rt_refit_stats, 32 B
    _fields_ = [("instances", C.c_uint32), ("leafRecords", C.c_uint32), ("nodes", C.c_uint32), ("levels", C.c_uint32), ("fullRefit", C.c_uint32),
                ("ms", C.c_float), ("triPad", C.c_float), ("treePad", C.c_float)]

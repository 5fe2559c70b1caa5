/*
 * rt_abi.h — data contract + C-ABI of librestir_hip.so (MI355X / gfx950 ReSTIR DI+GI frame path).
 *
 * This header is the drop-in boundary for the per-frame hot path of
 * IwakuraRein/CIS-565-Final-VR-Raytracer.  It replaces two reference interfaces:
 *
 *   (1) the host<->shader data contract   shaders/host_device.h:153-333
 *       (RtxState push constant, SceneCamera UBO, VertexAttributes, GltfShadeMaterial,
 *        reservoirs, light records, ImptSampData).  Every POD below has the same field
 *        order and the same byte size as the reference struct it cites (GLSL `scalar`
 *        block layout == tightly packed C), checked by static_assert at the bottom.
 *
 *   (2) the Vulkan plumbing inside Renderer / Scene / AccelStructure / HdrSampling
 *       (src/renderer.cpp:97-237, src/scene.cpp:57-125, src/accelstruct.cpp:55-162,
 *        src/hdr_sampling.cpp:56-99): buffer creation + vkCmdDispatch sequences become
 *       the extern "C" calls at the bottom.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  All calls return 0 on success or a
 * negative rt_status; the message is available from rt_last_error().  Nothing throws.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Small POD vector types (nvmath::vecNf stand-ins; column-major mat4 like nvmath::mat4f)
 * ---------------------------------------------------------------------------------------------- */
typedef struct { float x, y; } rt_vec2;
typedef struct { float x, y, z; } rt_vec3;
typedef struct { float x, y, z, w; } rt_vec4;
typedef struct { int32_t x, y; } rt_ivec2;
typedef struct { float m[16]; } rt_mat4; /* column-major: m[c*4+r] */

/* ------------------------------------------------------------------------------------------------
 * host_device.h mirrors
 * ---------------------------------------------------------------------------------------------- */

/* host_device.h:128-139 */
enum rt_debug_mode {
  RT_DBG_NONE = 0, RT_DBG_DIRECT_STAGE = 1, RT_DBG_INDIRECT_STAGE = 2, RT_DBG_BASECOLOR = 3, RT_DBG_NORMAL = 4,
  RT_DBG_DEPTH = 5, RT_DBG_METALLIC = 6, RT_DBG_EMISSIVE = 7, RT_DBG_ROUGHNESS = 8, RT_DBG_TEXCOORD = 9
};

/* host_device.h:142-148 */
enum rt_restir_state { RT_RESTIR_NONE = 0, RT_RESTIR_RIS = 1, RT_RESTIR_SPATIAL = 2, RT_RESTIR_TEMPORAL = 3, RT_RESTIR_SPATIOTEMPORAL = 4 };

#define RT_ALPHA_OPAQUE 0 /* host_device.h:179-181 */
#define RT_ALPHA_MASK 1
#define RT_ALPHA_BLEND 2
#define RT_MAX_IOR_MINUS_ONE 3.0f /* host_device.h:182 */
#define RT_INFINITY 1e28f         /* globals.glsl:35 */
#define RT_INVALID_MAT_ID 0xff000000u /* globals.glsl:106 */

/* host_device.h:153-165 — 336 B */
typedef struct {
  rt_mat4 viewInverse;
  rt_mat4 projInverse;
  rt_mat4 projView;
  rt_mat4 lastView;
  rt_mat4 lastProjView;
  rt_vec3 lastPosition;
  int32_t nbLights;
} rt_scene_camera;

/* host_device.h:167-174 — 32 B; packed by scene.cpp:236-258 */
typedef struct {
  rt_vec3 position;
  uint32_t normal;   /* oct-compressed (compress.glsl:111-139) */
  rt_vec2 texcoord;  /* LSB of .y = tangent handedness */
  uint32_t tangent;  /* oct-compressed */
  uint32_t color;    /* unorm8 x4 */
} rt_vertex;

/* host_device.h:183-204 — 80 B */
typedef struct {
  rt_vec4 pbrBaseColorFactor;
  int32_t pbrBaseColorTexture;
  float pbrMetallicFactor;
  float pbrRoughnessFactor;
  int32_t pbrMetallicRoughnessTexture;
  int32_t emissiveTexture;
  rt_vec3 emissiveFactor;
  int32_t normalTexture;
  float normalTextureScale;
  float transmissionFactor;
  int32_t transmissionTexture;
  float ior;
  int32_t alphaMode;
  float alphaCutoff;
  int32_t pad;
} rt_material;

/* host_device.h:207-238 — 100 B push constant, passed by value to every stage */
typedef struct {
  int32_t frame;
  int32_t maxDepth;
  int32_t modulate;
  float fireflyClampThreshold;
  float hdrMultiplier;
  int32_t debugging_mode;
  float environmentProb;
  uint32_t time; /* RNG seed input; wall-clock ms in the reference (sample_example.cpp:402), explicit here */
  int32_t ReSTIRState;
  int32_t RISSampleNum;
  int32_t reservoirClamp;
  int32_t accumulate;
  rt_ivec2 size;
  float envMapLuminIntegInv;
  float lightLuminIntegInv;
  int32_t MIS;
  float sigLuminDirect;
  float sigNormalDirect;
  float sigDepthDirect;
  int32_t denoise;
  float sigLuminIndirect;
  float sigNormalIndirect;
  float sigDepthIndirect;
  int32_t denoiseLevel;
} rt_state;

/* host_device.h:260-264 — 28 B */
typedef struct { rt_vec3 Li; rt_vec3 wi; float dist; } rt_light_sample;
/* host_device.h:266-271 — 64 B */
typedef struct { rt_vec3 L; rt_vec3 xv, nv; rt_vec3 xs, ns; float pHat; } rt_gi_sample;
/* host_device.h:273-277 — 36 B */
typedef struct { rt_light_sample lightSample; uint32_t num; float weight; } rt_direct_reservoir;
/* host_device.h:279-284 — 76 B */
typedef struct { rt_gi_sample giSample; uint32_t num; float weight; float bigW; } rt_indirect_reservoir;

/* host_device.h:287-293 — 16 B */
typedef struct { int32_t alias; float q; float pdf; float aliasPdf; } rt_impt_samp;

/* host_device.h:295-312 — 80 B */
typedef struct {
  int32_t type; rt_vec3 direction;
  float intensity; rt_vec3 color;
  rt_vec3 position; float range;
  float outerConeCos; float innerConeCos; rt_vec2 padding;
  rt_impt_samp impSamp;
} rt_punc_light;

/* host_device.h:314-325 — 96 B */
typedef struct {
  uint32_t matIndex; uint32_t transformIndex;
  rt_vec3 v0, v1, v2;
  rt_vec2 uv0, uv1, uv2;
  rt_impt_samp impSamp;
  rt_vec3 pad;
} rt_trig_light;

/* host_device.h:336-351 — 48 B; push constant of post.frag together with debugging_mode (render_output.hpp:40-43) */
typedef struct {
  float brightness, contrast, saturation, vignette;
  float avgLum, zoom; rt_vec2 renderingRatio;
  int32_t autoExposure; float Ywhite, key; int32_t pad;
} rt_tonemapper;

/* host_device.h:353-377 — 96 B; the uniform block `_sunAndSky` (layouts.glsl:53), defaults sample_example.hpp:186-203 */
typedef struct {
  rt_vec3 rgb_unit_conversion; float multiplier;
  float haze, redblueshift, saturation, horizon_height;
  rt_vec3 ground_color; float horizon_blur;
  rt_vec3 night_color; float sun_disk_intensity;
  rt_vec3 sun_direction; float sun_disk_scale;
  float sun_glow_intensity; int32_t y_is_up; int32_t physically_scaled_sun; int32_t in_use;
} rt_sun_and_sky;

/* host_device.h:327-333 — 16 B */
typedef struct { uint32_t puncLightSize; uint32_t trigLightSize; float trigSampProb; int32_t pad; } rt_light_buf_info;

/* ------------------------------------------------------------------------------------------------
 * Scene description handed to rt_upload_scene.  The reference hands the same content to Vulkan as
 * one vertex + one index VkBuffer per glTF primitive mesh (scene.cpp:209-289), an InstanceData table
 * with buffer device addresses (host_device.h:242-247, scene.cpp:179-195), one TLAS instance per node
 * (accelstruct.cpp:132-162), a material SSBO, a texture array, light SSBOs and the env texture + alias
 * table (hdr_sampling.cpp:56-99).  Device addresses become offsets into two shared arrays.
 * All arrays are copied by rt_upload_scene; the caller keeps ownership.
 * ---------------------------------------------------------------------------------------------- */

/* one per glTF primitive mesh == one reference BLAS + one InstanceData row (index = instanceCustomIndex) */
typedef struct {
  uint32_t vertexOffset; /* into rt_scene_desc.vertices */
  uint32_t vertexCount;
  uint32_t firstIndex;   /* into rt_scene_desc.indices; indices are relative to vertexOffset */
  uint32_t indexCount;   /* multiple of 3 */
  int32_t materialIndex;
} rt_prim_mesh;

/* accelstruct.cpp:145-149 */
#define RT_INST_FORCE_OPAQUE 1u /* VK_GEOMETRY_INSTANCE_FORCE_OPAQUE_BIT_KHR */
#define RT_INST_CULL_DISABLE 2u /* VK_GEOMETRY_INSTANCE_TRIANGLE_FACING_CULL_DISABLE_BIT_KHR */

/* one per drawable glTF node == one reference TLAS instance */
typedef struct {
  float objectToWorld[12]; /* 3 rows x 4 cols, row-major (VkTransformMatrixKHR, accelstruct.cpp:152) */
  uint32_t primMesh;       /* instanceCustomIndex */
  uint32_t flags;          /* RT_INST_* */
} rt_instance;

/* glTF sampler enums kept as glTF integers (scene.cpp:513-548) */
#define RT_WRAP_REPEAT 10497
#define RT_WRAP_CLAMP 33071
#define RT_WRAP_MIRROR 33648
#define RT_FILTER_NEAREST 9728
#define RT_FILTER_LINEAR 9729

/* VK_FORMAT_B8G8R8A8_UNORM texels, LOD 0 only (scene.cpp:559, 598 — mip generation is commented out) */
typedef struct {
  const uint8_t* bgra8;
  int32_t width, height;
  int32_t wrapS, wrapT; /* RT_WRAP_* */
  int32_t magFilter;    /* RT_FILTER_*; compute shaders sample LOD 0 => mag filter applies */
  int32_t pad;
} rt_texture;

typedef struct {
  uint32_t numPrimMeshes;  const rt_prim_mesh* primMeshes;
  uint64_t numVertices;    const rt_vertex* vertices;
  uint64_t numIndices;     const uint32_t* indices;
  uint32_t numInstances;   const rt_instance* instances;
  uint32_t numMaterials;   const rt_material* materials;
  uint32_t numTextures;    const rt_texture* textures;
  const rt_punc_light* puncLights;  /* lightInfo.puncLightSize entries (may be NULL when 0) */
  const rt_trig_light* trigLights;  /* lightInfo.trigLightSize entries (may be NULL when 0) */
  rt_light_buf_info lightInfo;
  int32_t envWidth, envHeight;      /* RGBA32F lat-long map, U repeat / V clamp, bilinear (hdr_sampling.cpp:69-77) */
  const float* envRgba32f;          /* envWidth*envHeight*4 floats; NULL => 1x1 black */
  const rt_impt_samp* envAccel;     /* envWidth*envHeight entries (hdr_sampling.cpp:181-242); NULL when no env */
} rt_scene_desc;

/* ------------------------------------------------------------------------------------------------
 * Screen-space buffers owned by the context (renderer.cpp:227-302, render_output.cpp:82-148).
 * Reference element layouts are kept at the boundary (readback/upload use them verbatim).
 * ---------------------------------------------------------------------------------------------- */
typedef enum {
  RT_BUF_GBUFFER0 = 0,        /* RGBA32UI 16 B/px (renderer.hpp:88)              */
  RT_BUF_GBUFFER1 = 1,
  RT_BUF_MOTION = 2,          /* RG16_SINT 4 B/px (renderer.hpp:94)               */
  RT_BUF_DIRECT_RESV0 = 3,    /* rt_direct_reservoir 36 B/px (renderer.cpp:229)   */
  RT_BUF_DIRECT_RESV1 = 4,
  RT_BUF_DIRECT_RESV_TEMP = 5,
  RT_BUF_INDIRECT_RESV0 = 6,  /* rt_indirect_reservoir 76 B/half-px               */
  RT_BUF_INDIRECT_RESV1 = 7,
  RT_BUF_INDIRECT_RESV_TEMP = 8,
  RT_BUF_DENOISE_DIR_A = 9,   /* RGBA32F 16 B/px (renderer.cpp:267-285)           */
  RT_BUF_DENOISE_DIR_B = 10,
  RT_BUF_DENOISE_IND_A = 11,  /* RGBA32F, allocated full-res, top-left quarter used */
  RT_BUF_DENOISE_IND_B = 12,
  RT_BUF_DIRECT_RESULT0 = 13, /* RGBA32F 16 B/px (render_output.cpp:104-133)      */
  RT_BUF_DIRECT_RESULT1 = 14,
  RT_BUF_INDIRECT_RESULT0 = 15,
  RT_BUF_INDIRECT_RESULT1 = 16,
  RT_BUF_LIGHT_ID0 = 17,      /* u32/px, ping-pong like the reservoirs: id of the light sample held by the direct
                                 reservoir (0x80000000|env texel, 0x40000000|triangle light, 0x20000000|punctual light,
                                 0xffffffff none).  Added for the "reservoir sample indices bit-exact" check of
                                 BASELINE.json; the reference stores the sample itself, not an index. */
  RT_BUF_LIGHT_ID1 = 18,
  RT_BUF_LDR = 19,            /* RGBA8 UNORM 4 B/px (R in the low byte): output of rt_tonemap = the swapchain image post.frag draws */
  RT_BUF_COUNT = 20
} rt_buffer_id;

/* per-frame stage selector for rt_run_stage — the dispatch list of renderer.cpp:163-205 */
typedef enum {
  RT_STAGE_DIRECT = 0,           /* direct_stage.comp  (live); rt_run_stage level 1 / 2: only the first / second half of the spatial-reuse modes (see rt_run_stage) */
  RT_STAGE_INDIRECT = 1,         /* indirect_stage.comp, half resolution         */
  RT_STAGE_DENOISE_DIRECT = 2,   /* denoise_direct.comp, level 0..3              */
  RT_STAGE_DENOISE_INDIRECT = 3, /* denoise_indirect.comp, level 0..4            */
  RT_STAGE_COMPOSE = 4,          /* compose.comp                                 */
  RT_STAGE_DIRECT_GEN = 5,       /* direct_gen.comp   (compiled, not dispatched: renderer.cpp:166-168) */
  RT_STAGE_DIRECT_REUSE = 6,     /* direct_reuse.comp (compiled, not dispatched: renderer.cpp:170-171) */
  RT_STAGE_COUNT = 7
} rt_stage_id;

typedef struct {
  uint64_t closestHitRays;   /* ClosestHit() invocations (traceray_rq.glsl:108)  */
  uint64_t anyHitRays;       /* AnyHit() invocations (traceray_rq.glsl:153)      */
  uint64_t nodesVisited;     /* BVH8 nodes fetched (80 B each)                   */
  uint64_t trisTested;       /* triangle records fetched (48 B + 8 B each)       */
  uint64_t hitsShaded;       /* GetState() invocations (108 B gather + 80 B material) */
  uint64_t risCandidates;    /* SampleDirectLightNoVisibility() invocations      */
  /* HIP-event timings on the ctx stream, ACCUMULATED over the rt_render_frame calls since the last rt_set_counting()
   * (which resets them); denoise entries sum their 4 / 5 levels. Divide by framesTimed for per-frame averages. */
  float stageMs[RT_STAGE_COUNT];
  float frameMs;
  uint32_t framesTimed;
  /* SIMD efficiency of the traversal loops (counting mode): summed over lanes, the scheduling rounds a lane sat through while
   * its wave was traversing (laneRounds) and the rounds in which it still had a ray to advance (laneLiveRounds).
   * (nodesVisited + trisTested) / laneLiveRounds = share of live lanes the majority vote lets step;
   * laneLiveRounds / laneRounds = share of lanes that are not just waiting for the slowest ray of their wave. */
  uint64_t laneRounds, laneLiveRounds;
} rt_counters;

typedef enum {
  RT_OK = 0,
  RT_ERR_INVALID_ARG = -1,
  RT_ERR_NO_DEVICE = -2,
  RT_ERR_HIP = -3,
  RT_ERR_NO_SCENE = -4,
  RT_ERR_NO_ACCEL = -5,
  RT_ERR_NO_TARGET = -6,
  RT_ERR_OOM = -7
} rt_status;

typedef struct rt_ctx rt_ctx;

/* Renderer::setup (renderer.cpp:62-73): bind to HIP device `device`, create the stream + events. */
int rt_create(rt_ctx** out, int device);
/* Renderer::destroy + Scene::destroy + AccelStructure::destroy (renderer.cpp:75-91). */
int rt_destroy(rt_ctx* ctx);
/* Run every later launch on a caller-owned hipStream_t (NULL = ctx-owned stream). Lets the caller
 * order RCCL halo exchanges with the stages without host syncs. */
int rt_set_stream(rt_ctx* ctx, void* hipStream);
/* Scene::load's buffer uploads (scene.cpp:94-112) + HdrSampling::loadEnvironment upload (hdr_sampling.cpp:79-95).
 * Every value the kernels use as an array index (vertex indices, material / texture ids, light material ids, alias-table
 * entries) is range-checked here: RT_ERR_INVALID_ARG instead of a device fault.  (The reference trusts nvh::GltfScene.) */
int rt_upload_scene(rt_ctx* ctx, const rt_scene_desc* scene);
/* AccelStructure::create (accelstruct.cpp:55-65): host-built flat BVH8 over world-space triangles. */
int rt_build_accel(rt_ctx* ctx);
/* Renderer::create / Renderer::update (renderer.cpp:97-148, 209-225): (re)allocate all screen-space buffers, zeroed. */
int rt_resize(rt_ctx* ctx, int width, int height);
/* Scene::updateCamera's vkCmdUpdateBuffer (scene.cpp:777-811). */
int rt_set_camera(rt_ctx* ctx, const rt_scene_camera* cam);
/* Renderer::run (renderer.cpp:154-206): the 12 dispatches of one frame. `frames` selects the ping-pong
 * side exactly like m_descSet[(frames+1)%2] (renderer.cpp:157, 346-356): this = [frames&1], last = [(frames+1)&1]. */
int rt_render_frame(rt_ctx* ctx, const rt_state* state, int frames);
/* One dispatch of the list above, restricted to pixel rows [rowBegin,rowEnd) of the stage's own grid
 * (full-res rows for direct/denoise_direct/compose, half-res rows for indirect/denoise_indirect).
 * rowEnd <= 0 means "all rows".  Used for row-tiled multi-GPU frames.
 * `level`: the a-trous level for the two denoise stages.  For RT_STAGE_DIRECT with ReSTIRState eSpatial / eSpatiotemporal it selects
 * the half of the stage: 0 = both, 1 = everything up to cacheTempReservoir (direct_stage.comp:224-235), 2 = the neighbour merges and
 * the shading (:236-262) — a row-tiled host runs 1, exchanges the neighbouring rows of RT_BUF_DIRECT_RESV_TEMP, then runs 2. */
int rt_run_stage(rt_ctx* ctx, const rt_state* state, int frames, int stage, int level, int rowBegin, int rowEnd);
/* Copy a screen-space buffer to / from host memory in the reference element layout. Synchronous. */
int rt_readback(rt_ctx* ctx, int buffer, void* dst, size_t bytes);
int rt_upload_history(rt_ctx* ctx, int buffer, const void* src, size_t bytes);
/* Size in bytes of a buffer's boundary layout at the current resolution. */
size_t rt_buffer_bytes(rt_ctx* ctx, int buffer);
/* Raw device pointer of a buffer's device-side storage, its ALLOCATED byte size and the bytes per row of the stage
 * grid, for RCCL exchanges by the caller.  Device-side layout == boundary layout; every allocation carries 128 rows
 * (64 for the half-resolution reservoirs) of slack behind the image so equal-height row bands of up to 8 ranks can be
 * all-gathered in place. */
int rt_device_ptr(rt_ctx* ctx, int buffer, void** ptr, size_t* bytes, size_t* rowPitch);
/* Enable (1) / disable (0) traversal + gather counting for subsequent frames (adds atomics to the kernels), and reset
 * every counter and accumulated timing. */
int rt_set_counting(rt_ctx* ctx, int enable);
int rt_get_counters(rt_ctx* ctx, rt_counters* out);
/* Row-tiled multi-GPU: declare which rows [row0,row1) of the LAST-frame buffers (G-buffer, reservoirs, light ids; full-res
 * rows, the half-res reservoirs use row/2) hold valid data on this GPU — its own band plus the halo rows received from its
 * neighbours.  Temporal reuse that reprojects inside the image but outside this range sets a flag instead of silently
 * reading stale rows; rt_history_miss() returns and clears the flag (synchronises the ctx stream) so the caller can
 * gather the full history and redo the frame.  Default: every row is valid. */
int rt_set_history_rows(rt_ctx* ctx, int row0, int row1);
int rt_history_miss(rt_ctx* ctx, int* missed);
/* The same flag per stage kind, for hosts that keep the direct stage of frame f+1 in flight beside the indirect stage of
 * frame f on different streams: RT_STAGE_DIRECT* launches raise flag 0, RT_STAGE_INDIRECT launches raise flag 1;
 * this call waits for the ctx stream only, then reads and clears the flag of `stage`.  (rt_history_miss = both flags.) */
int rt_history_miss_stage(rt_ctx* ctx, int stage, int* missed);
/* Stage-wise submission with frames in flight (what rt_render_frame does internally in overlap mode 2): before submitting the
 * stages of frame `frames`, swap RT_BUF_GBUFFER0 + (frames & 1) and RT_BUF_MOTION with their spare buffers so that this
 * frame's direct stage does not overwrite the G-buffer / motion vectors that the previous frame's indirect stage, possibly
 * still running on another stream, reads.  Calling it a second time with the same `frames` undoes the swap.
 * Invalidates rt_device_ptr results for those three buffers. */
int rt_rotate_buffers(rt_ctx* ctx, int frames);
/* RT_BUF_DENOISE_IND_A (the noisy indirect colour: indirect stage -> its five filter levels) exists once per frame parity, so that the indirect stage of frame
 * f+1 does not wait for the filters of frame f.  The id names the buffer of the frame most recently passed to rt_render_frame / rt_run_stage / this call:
 * a host that touches the buffer itself (rt_device_ptr for a halo exchange) of a frame other than the last one it launched selects that frame first. */
int rt_select_frame(rt_ctx* ctx, int frames);
/* RenderOutput::run (render_output.cpp:224-237) + post.frag:103-175 as a compute pass: reads the two result images of
 * frame `frames` (RT_BUF_DIRECT_RESULT0/INDIRECT_RESULT0 + (frames & 1)), applies auto-exposure (tonemapping by the image
 * mean, post.frag:133-153), the Uncharted-2 tone curve (tonemapping.glsl:48-66), dithering (post.frag:50-55), contrast /
 * brightness / saturation / vignette (post.frag:163-171) or the debug views (post.frag:106-118) and writes RT_BUF_LDR.
 * Differences from the fragment shader, all documented in DESIGN.md: the image mean replaces the driver-generated mip
 * pyramid's top level; tm.zoom samples the nearest texel.  The "local" auto-exposure bit (autoExposure & 2, toneLocalExposure,
 * post.frag:70-101) samples mip levels 0..7 of the two result images: the pyramid is built level by level with the linear-blit
 * formula of RenderOutput::genMipmap (render_output.cpp:243-254; 2x2 box for even sizes) and sampled bilinearly at the fragment;
 * the variable the reference leaves uninitialised in the default view (`v2 ==` at post.frag:91) is 0. */
int rt_tonemap(rt_ctx* ctx, const rt_tonemapper* tm, int debugging_mode, int frames);
/* The ray query on its own, for tests and tools: n rays (8 floats each: origin xyz, direction xyz, tmax, the bits of the ray's seed — the seed only enters
 * the stochastic alpha test) through ClosestHit (anyHit = 0: out = 4 floats per ray, t | bits of the flattened triangle index (0xffffffff: miss) | u | v;
 * tmax is ignored, the range is (0, 1e28)) or AnyHit (anyHit = 1: out[4 i] = 1 if anything accepts inside (0, tmax), else 0) of traceray_rq.glsl:108-185,
 * with the traversal the stage kernels use.  Host arrays in, host arrays out. */
int rt_trace_rays(rt_ctx* ctx, int n, const float* rays, float* out, int anyHit);
/* Which build of the ray-traced kernels (direct_stage / direct_gen / indirect_stage) a launch gets.  There are two, with identical
 * results: THROUGHPUT (majority-vote traversal rounds, 4-5 waves per SIMD — a full frame is bound by instruction issue) and LATENCY
 * (every ray advances every round, node fetches overlapped with the triangle work, register budget of 2 waves per SIMD — a row band
 * of a multi-GPU frame or a small image is bound by the dependent memory accesses of its slowest wave).  AUTO (default) picks per
 * launch from its size.  ABI 2.0: replaces the pipeline switch of ABI 1.0, whose second (queue-based) kernel organisation was removed. */
enum { RT_TRAVERSAL_AUTO = 0, RT_TRAVERSAL_THROUGHPUT = 1, RT_TRAVERSAL_LATENCY = 2 };
int rt_set_traversal(rt_ctx* ctx, int mode);
/* SampleExample::screenPicking (sample_example.cpp:456-497): nvvk::RayPickerKHR — one camera ray through the normalised
 * window position (pickX, pickY in [0,1]) built like raySpawn (origin = modelViewInv * (0,0,0,1), direction = modelViewInv *
 * normalize(perspectiveInv * (2*pick-1, 1, 1))), traced with the path's ClosestHit rules.  The result mirrors
 * nvvk::RayPickerKHR::PickResult; instanceID == -1 => nothing hit. */
typedef struct {
  rt_vec4 worldRayOrigin, worldRayDirection;
  float hitT; int32_t primitiveID; int32_t instanceID; int32_t instanceCustomIndex;
  rt_vec3 baryCoord;
} rt_pick_result;
int rt_pick(rt_ctx* ctx, const rt_mat4* modelViewInv, const rt_mat4* perspectiveInv, float pickX, float pickY, rt_pick_result* out);
/* SampleExample::updateUniformBuffer's vkCmdUpdateBuffer(m_sunAndSkyBuffer, ...) (sample_example.cpp:172): the procedural
 * sun & sky environment.  With in_use == 1 EnvRadiance / EnvSample / EnvEval (pathtrace.glsl:40-72, env_sampling.glsl:105-135)
 * evaluate sun_and_sky() (sun_and_sky.glsl:453-601) instead of the HDR map.  Default: in_use = 0. */
int rt_set_sun_and_sky(rt_ctx* ctx, const rt_sun_and_sky* ss);
/* Stream-level concurrency of rt_render_frame (results are identical in every mode):
 *   0 = every launch of Renderer::run's list (renderer.cpp:163-205) in order on the ctx stream;
 *   1 = the direct A-Trous chain runs beside the indirect stage on an internal stream and joins before compose;
 *   2 = (default) 1 + frames in flight: the call returns after enqueueing and the next frame's direct stage runs beside
 *       this frame's indirect stage and filters (internally triple-buffered G-buffer, double-buffered motion vectors).
 *       Throughput mode of a renderer that keeps submitting; one frame's latency is higher than in mode 1.
 *   3 = 2 with a third frame in flight (four G-buffers, three motion buffers, three direct images): direct(f) waits for frame f-3 instead of f-2, which takes
 *       the filter chain of frame f-2 off the path to direct(f).  Measured, not the default (profiles/r06_three_frames_ab.txt).
 * rt_sync / rt_readback / rt_get_counters wait for everything in flight.  In modes 2 and 3, rt_device_ptr results for the
 * G-buffers and the motion buffer (mode 3: and the direct result images) are invalidated by rt_render_frame (rt_run_stage never rotates buffers).
 * Also settable with RESTIR_OVERLAP=0|1|2|3 before rt_create. */
int rt_set_overlap(rt_ctx* ctx, int mode);
/* Priorities of the indirect-stage stream and the filter stream of mode 2 (levels: -1 low, 0 normal, +1 high).  The reference submits its dispatches to ONE queue
 * (src/renderer.cpp:154-206) and has no such choice; here three streams share the chip and the fastest setting depends on the workload
 * (profiles/r05_prio_by_config_ab.txt).  Unset (no call, no RESTIR_PRIO), the context decides on its first three mode-2 frames ("probe frames": every stage alone on
 * the main stream, timed): the filter stream becomes high next to the indirect stream when filters / (direct + indirect) of the LAST probe frame — warm caches, warm
 * history — is >= 0.30 (profiles/r06_prio_rule.txt); the two streams are created afterwards.  rt_resize, a new scene / tree and a denoise toggle re-open that decision (round 6; round 5 decided once,
 * on the cold first frame).  An explicit call is best made before the first frame: a stream created after others exist may share a hardware queue with them; it
 * stands for the context's lifetime.  Results are identical under every setting.  Drains the context. */
int rt_set_stream_priorities(rt_ctx* ctx, int indirectLevel, int filterLevel);
/* The levels in use; filterShare = the last probe frame's filters / (direct + indirect) (-1: not measured: no frame yet, or the levels were given); decided = 0 while a
 * context that decides for itself is still probing.  Any pointer may be NULL. */
int rt_get_stream_priorities(rt_ctx* ctx, int* indirectLevel, int* filterLevel, float* filterShare, int* decided);
/* The context's three streams of the frames-in-flight schedule (hipStream_t; owned by the context), for a host that issues the stages itself through rt_run_stage +
 * rt_set_stream (restir_amd/tiled.py wraps them in torch.cuda.ExternalStream; csrc/mgpu.cpp uses them per rank).  The reference has ONE queue (src/renderer.cpp:154-206);
 * here a host that brought its own streams (torch's pool of 32, created after RCCL's) ran on a stream layout the schedule was never measured on.  Creates the filter,
 * then the indirect stream with the current levels if they do not exist (only when one of the two is asked for: with both NULL nothing is created); call before anything
 * else in the process creates streams.  Any pointer may be NULL. */
int rt_get_streams(rt_ctx* ctx, void** mainStream, void** indirectStream, void** filterStream);
/* created = HIP streams this library has created in the process so far; index[0..2] = creation index of this context's main / indirect / filter stream (-1: none yet). */
int rt_get_stream_layout(rt_ctx* ctx, int* created, int index[3]);
/* ------------------------------------------------------------------------------------------------------------------
 * Multi-GPU context (csrc/mgpu.cpp): the row-tiled frame of BASELINE.json / SURVEY.md §8(e) for a host that owns all the
 * GPUs of the node from ONE process — "multi-GPU ctx internally drives 8 streams" (§8b threading row).  One worker thread,
 * one rt_ctx and one HIP stream per device; halos and history rows move with hipMemcpyPeerAsync over xGMI; band heights
 * are cost weighted from the ranks' measured stage times.  Call order == the single-GPU context's:
 *     rt_mgpu_create -> rt_mgpu_upload_scene (upload + BVH8 build on every device) -> rt_mgpu_resize
 *     per frame: rt_mgpu_set_camera, rt_mgpu_render_frame
 *     rt_mgpu_readback assembles a buffer of the last frame from the ranks that own its rows (same layout as rt_readback).
 * Frames in flight (default, rt_mgpu_set_pipeline): rt_mgpu_render_frame QUEUES the frame (at most two ahead) and returns; every rank runs the three-stream
 * schedule of rt_render_frame and every cross-rank dependency is a HIP event another rank's stream waits for — no host barrier per frame.  Frames must be
 * consecutive (`frames` + 1 per call); rt_mgpu_sync / rt_mgpu_readback / rt_mgpu_get_stats finish what is in flight first.  With rt_mgpu_set_pipeline(0),
 * in the spatial-reuse modes and under rt_mgpu_set_serialize the call returns when the frame is complete on every device (barrier schedule).
 * Every output is bit-identical to the single-GPU frame, in every ReSTIRState (the spatial-reuse modes run the direct stage in two
 * halves around an exchange of the cached reservoirs' boundary rows).  `devices` may name the same device more than once (used by the
 * tests on a one-GPU machine).  The caller's thread discipline is the reference's: one thread issues the calls.
 * (One-process-per-GPU hosts use restir_amd/tiled.py over torch.distributed / RCCL instead.)
 * ---------------------------------------------------------------------------------------------------------------- */
#define RT_MGPU_MAX_RANKS 16
typedef struct rt_mgpu rt_mgpu;
typedef struct {
  int32_t numRanks;
  uint32_t frames;                               /* frames rendered since creation */
  uint32_t historyFallbacks;                     /* frames whose temporal reuse left band + halo (full history pulled, stages re-run) */
  uint32_t pad;
  uint64_t haloBytes;                            /* bytes pulled from peers during the last frame, all ranks */
  int32_t bandBegin[RT_MGPU_MAX_RANKS], bandEnd[RT_MGPU_MAX_RANKS]; /* full-res row range of every rank in the last frame */
  float tracedMs[RT_MGPU_MAX_RANKS];             /* direct + indirect stage of the last frame, HIP events on the rank's stream */
  float filterMs[RT_MGPU_MAX_RANKS];             /* 4 + 5 A-Trous passes + compose */
  uint64_t haloBytesKind[6];                     /* haloBytes by purpose: history rows | filter halos | spatial-reuse rows | rows that changed owner | display gather | fallback pulls */
  uint64_t haloBytesRankKind[RT_MGPU_MAX_RANKS][6]; /* the same per rank (bytes that rank pulled for its latest complete frame) */
} rt_mgpu_stats;
int rt_mgpu_create(rt_mgpu** out, int numRanks, const int* devices /* NULL: devices 0..numRanks-1 */);
int rt_mgpu_destroy(rt_mgpu* m);
int rt_mgpu_upload_scene(rt_mgpu* m, const rt_scene_desc* scene);
int rt_mgpu_resize(rt_mgpu* m, int width, int height);
int rt_mgpu_set_camera(rt_mgpu* m, const rt_scene_camera* cam);
int rt_mgpu_render_frame(rt_mgpu* m, const rt_state* state, int frames);
int rt_mgpu_readback(rt_mgpu* m, int buffer, void* dst, size_t bytes);
int rt_mgpu_sync(rt_mgpu* m);
int rt_mgpu_set_balance(rt_mgpu* m, int mode);    /* 1 (default): cost-weighted band heights; 0: equal heights; 2: freeze the current partition */
int rt_mgpu_set_bands(rt_mgpu* m, const int* bands /* numRanks + 1 row boundaries, multiples of 16, 0 .. height */);   /* explicit partition; freezes it */
int rt_mgpu_set_serialize(rt_mgpu* m, int on);    /* measurement aid when several ranks share ONE device: ranks take turns on the GPU */
int rt_mgpu_set_pipeline(rt_mgpu* m, int on);     /* 1 (default): frames in flight per rank, event-ordered pulls; 0: barrier schedule */
int rt_mgpu_set_gather(rt_mgpu* m, int on);       /* 1 (default): rank 0 pulls the result bands every frame (display rank); 0: results stay with their owners */
int rt_mgpu_set_solo(rt_mgpu* m, int rank);       /* measurement aid: only `rank` renders (its pulls read the idle ranks' stale rows): the PERIOD of one rank on a GPU to itself; -1 = off */
int rt_mgpu_get_stats(rt_mgpu* m, rt_mgpu_stats* out);
/* Link statistics of the latest complete frame of the frames-in-flight schedule (ABI 2.1): every rank's four pull groups — 0 history rows (main stream),
 * 1 indirect-reservoir history (indirect stream), 2 direct filter halo, 3 indirect filter halo (filter stream) — timed with HIP events on the stream that
 * carried them, and their bytes; the device of every rank; peerAccess[puller][owner] = 1 when the puller's device has direct peer access to the owner's
 * (xGMI on an MI355X node; 0 = staged by the runtime).  This is the measured point bench.py's xgmi_model stands in for on a one-GPU box.
 * pullBytes / pullMs of a group are a pair of ONE frame (a frame whose events cannot be read yet leaves the previous pair standing); the barrier schedule
 * (rt_mgpu_set_pipeline(0), serialize, spatial modes) does not bracket its pulls: zeros. */
typedef struct {
  int32_t numRanks;
  int32_t devices[RT_MGPU_MAX_RANKS];
  uint8_t peerAccess[RT_MGPU_MAX_RANKS][RT_MGPU_MAX_RANKS];
  float pullMs[RT_MGPU_MAX_RANKS][4];
  uint64_t pullBytes[RT_MGPU_MAX_RANKS][4];
} rt_mgpu_link_stats;
int rt_mgpu_get_link_stats(rt_mgpu* m, rt_mgpu_link_stats* out);
/* rt_get_stream_layout of every rank's context: created = streams the library has created in the process; index[3 * rank + {0, 1, 2}] = creation index of that rank's
 * main / indirect / filter stream (-1: not created yet — a rank's two extra streams are created on its first frame in flight); levels[3] = their priority levels. */
int rt_mgpu_get_stream_layout(rt_mgpu* m, int* created, int* index, int levels[3]);
/* The partition rule on its own (pure host arithmetic): boundaries (numRanks + 1 rows, multiples of 16) that equalise the summed cost of the
 * 16-row stripes; with prevBands a boundary moves at most maxMoveStripes stripes (< 0: unlimited); every rank keeps >= one stripe. */
int rt_mgpu_plan_bands(int height, int numRanks, const float* stripeCost, const int* prevBands, int maxMoveStripes, int* outBands);
const char* rt_mgpu_last_error(rt_mgpu* m);

/* Measured VALU issue ceiling of the device the ctx lives on (csrc/microbench.hip): wave-level VALU instructions per second of a
 * chain-free loop.  variant 0 = the instruction mix of the traced kernels, 1 = v_fma_f32 only; wavesPerSimd in 1..8.
 * bench.py prices `roofline.valu` against this measurement instead of an assumed cycles-per-instruction figure.
 * (Introspection like rt_get_counters; no counterpart in the reference.) */
int rt_measure_valu_peak(rt_ctx* ctx, int variant, int wavesPerSimd, double* waveInstPerSec);
/* ------------------------------------------------------------------------------------------------------------------
 * Reference mode (ABI 2.4): a progressive, unbiased, deterministic path tracer over the same scene, camera, traversal and shading code
 * as the frame — the converged image the real-time estimator approximates (the reference's RtxState.accumulate / frame slot,
 * host_device.h:209,222, whose accumulating shader body it never wired).  Per sample of pixel (x, y) it estimates, in fp32:
 *   primary ray = raySpawn (pathtrace.glsl:260-270), no extra jitter;  miss: direct = EnvRadiance;  emitter hit: direct = emission, the path ends;
 *   vertex 1: direct = emission + one SampleDirectLight sample with its shadow ray, weight 1, BSDF with the material's real albedo;
 *   vertices 2..maxDepth: pathTraceIndirect's integrand (indirect_stage.comp:129-226) into indirect — NEE with the power heuristic when MIS > 0, BSDF-sampled
 *   env and emitter hits at depth > 1 with their MIS weight — with every path multi-bounce, throughput starting at 1 and the real albedo at vertex 1.
 * No firefly clamp, no HDR->LDR encoding, no reservoirs, no denoiser: fireflyClampThreshold, modulate, ReSTIRState, RISSampleNum, reservoirClamp,
 * denoise*, sig*, frame, time and accumulate are ignored; debugging_mode != 0 is RT_ERR_INVALID_ARG.  
 * Determinism: sample s (0-based since the last reset) of pixel (x, y) of a W-wide image is seeded with
 *     seed = tea(W * y + x, tea(s, 0x52454631))          (tea = random.glsl:34-48)
 * and nothing else, so the result does not depend on how samples are split over calls, on rt_set_traversal or on frames in flight.  Each sample's
 * radiance is added, in sample order, to per-pixel fp64 sums (direct rgb, indirect rgb: 48 B/px, allocated by the first rt_reference_render and
 * freed by rt_resize / rt_destroy); a mean is float(sum / n) in IEEE double, one rounding.
 * The sums reset (n -> 0) when an input of the integral changes: rt_resize, rt_upload_scene, rt_build_accel, rt_set_sun_and_sky, a camera whose
 * viewInverse or projInverse differs (rt_set_camera; the history matrices do not count), and a call whose maxDepth, hdrMultiplier, environmentProb or
 * MIS differ from the previous call's.  Nothing else resets them.
 * The calls join the frames in flight and run on the context's main stream; they read and write no frame buffer (rt_reference_tonemap writes
 * RT_BUF_LDR only), leave rt_get_counters, the stream-priority decision and the buffer rotation alone, and do not change what rt_render_frame computes.
 * One launch adds one sample to a band of at most 2^20 pixels.  The multi-GPU context has no reference mode. */
/* adds `samples` (>= 0) samples to every pixel.  RT_ERR_NO_SCENE / NO_ACCEL / NO_TARGET like rt_render_frame (state->size must match rt_resize). */
int rt_reference_render(rt_ctx* ctx, const rt_state* state, int samples);
/* n -> 0 */
int rt_reference_reset(rt_ctx* ctx);
/* samples accumulated since the last reset */
int rt_reference_samples(rt_ctx* ctx, uint32_t* n);
/* the mean of component 0 (direct), 1 (indirect) or 2 (direct + indirect: float((sumDirect + sumIndirect) / n)) as RGBA32F, a = 1; bytes = W * H * 16.
 * With n == 0 every pixel is (0, 0, 0, 1).  Synchronous. */
int rt_reference_readback(rt_ctx* ctx, int component, float* dst, size_t bytes);
/* rt_tonemap's pass (post.frag, default view) over the direct and indirect means in place of the frame's two result images -> RT_BUF_LDR. */
int rt_reference_tonemap(rt_ctx* ctx, const rt_tonemapper* tm);
/* ------------------------------------------------------------------------------------------------------------------
 * Denoiser selection (added within ABI 2.4, no version bump): the filter that turns the two noisy, demodulated, LDR-encoded colour images of a frame
 * (HDRToLDR(clampRadiance(x)): the direct image and the half-resolution indirect image) into the images compose reads.
 *   RT_DENOISER_ATROUS (default)  the reference's edge-aware A-Trous chain (denoise_direct.comp / denoise_indirect.comp), fixed luminance sigma sigLumin*.
 *   RT_DENOISER_SVGF              variance-guided spatiotemporal filter, per component, in the same signal domain:
 *     (a) temporal accumulation: previous pixel q = motion(p) (direct) / motion(2p) >> 1 (indirect); q is consistent when it lies in the image, the previous
 *         G-buffer at q (2q for indirect) has the same material hash, dot(n, n_prev) > 0.9 and |cam.lastPosition - position| < depth_prev * 1.05 (the temporal
 *         test of the direct stage).  n = consistent ? min(n_prev + 1, historyCap) : 1; a = max(alphaColor, 1/n), am = max(alphaMoments, 1/n);
 *         C = mix(C_prev, c, a), m1 = mix(m1_prev, l, am), m2 = mix(m2_prev, l^2, am) with l = luminance(c).  Pixels without a valid material get what the
 *         A-Trous chain writes there and cleared history.
 *     (b) variance: n >= 4: max(0, m2 - m1^2); else the same over a 7x7 neighbourhood of moments weighted by the normal and depth terms, same material only.
 *     (c) 4 (direct) / 5 (indirect) A-Trous levels, step 2^level, the 5x5 kGauss weights, the A-Trous normal and depth terms, luminance term
 *         exp(-|l_p - l_q| / (phiLum * sqrt(g3x3(var)_p) + 1e-10)); colour = sum(w c) / sum(w), variance = sum(w^2 var) / sum(w)^2; the filtered colour of
 *         level 0 becomes the colour history; the last level applies LDRToHDR (direct -> RT_BUF_DIRECT_RESULT, indirect -> RT_BUF_DENOISE_IND_B).
 *   History (colour + n, moments; per component) is double-buffered by frame parity, allocated by the first frame rendered in SVGF mode and freed by rt_resize /
 *   rt_destroy.  It is invalid (every valid pixel restarts at n = 1) after rt_resize, rt_upload_scene, rt_build_accel, an rt_set_denoiser that changes anything,
 *   a frame rendered with denoise == 0, rt_denoiser_reset, and a frame whose parity does not follow the previous SVGF frame's.
 *   rt_run_stage of RT_STAGE_DENOISE_DIRECT / _INDIRECT on a context in SVGF mode is RT_ERR_INVALID_ARG (row-tiled hosts keep the A-Trous chain).
 *   Timings accumulate under the RT_STAGE_DENOISE_* entries of rt_counters.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_DENOISER_ATROUS = 0 /* default: the reference's filter */, RT_DENOISER_SVGF = 1 };
typedef struct {
  int32_t mode;          /* RT_DENOISER_* */
  float alphaColor;      /* (0, 1]: colour history blend factor floor */
  float alphaMoments;    /* (0, 1]: moments history blend factor floor */
  int32_t historyCap;    /* >= 1: longest history n counts */
  float phiLumDirect;    /* > 0, finite: luminance edge-stopping scale of the direct filter */
  float phiLumIndirect;  /* > 0, finite: ... of the indirect filter */
  int32_t reserved[2];   /* must be 0 */
} rt_denoiser;           /* 32 B; defaults: ATROUS, 0.2, 0.2, 32, 4.0, 4.0 */
/* validates every field (bad values: RT_ERR_INVALID_ARG, the settings in use stay); a change of mode re-opens the stream-priority decision like a denoise toggle */
int rt_set_denoiser(rt_ctx* ctx, const rt_denoiser* d);
int rt_get_denoiser(rt_ctx* ctx, rt_denoiser* out);
/* the next SVGF frame starts without history */
int rt_denoiser_reset(rt_ctx* ctx);
/* the history the last SVGF frame wrote: which = 0 direct colour + n (RGBA32F, W * H * 16 B), 1 indirect colour + n (RGBA32F, (W/2) * (H/2) * 16 B),
 * 2 direct moments (m1, m2 as 2 x f32, W * H * 8 B), 3 indirect moments ((W/2) * (H/2) * 8 B).  RT_ERR_NO_TARGET before the first SVGF frame.  Synchronous. */
int rt_denoiser_readback(rt_ctx* ctx, int which, void* dst, size_t bytes);
/* ------------------------------------------------------------------------------------------------------------------
 * ReSTIR GI spatial reuse (added within ABI 2.4, no version bump): one pass per frame after the indirect stage, at half resolution, that
 * resamples each pixel's indirect reservoir with up to `samples` neighbours (biased variant: no 1/Z correction).  It reads this frame's G-buffer (at 2p) and the
 * indirect reservoirs as the indirect stage wrote them (after temporal reuse), and writes its own reservoir buffer and RT_BUF_DENOISE_IND_A.  Per pixel p:
 *   receiver   the indirect stage's decode: ray = raySpawn(p, indSize), state from the G-buffer at 2p, position moved 2e-2 along ffnormal -> x_r, n_r = ffnormal,
 *              wo = -ray.direction, albedo 1.  No surface: IND_A stays as the stage wrote it (0), the pass writes a zero reservoir.
 *   seed       tea(indW * y + x, tea(time, 0x47495350)), a stream of its own; visibility rays draw alpha tests from it as every ray does.
 *   start      r_s = the pixel's reservoir r_p, unchanged (sample, stored xv / nv, weight, num).
 *   taps       k = 0 .. samples - 1: u1, u2, rr drawn in that order, always.  o = (floor(u1 (2R+1)) - R, floor(u2 (2R+1)) - R); skipped when o = (0, 0) or
 *              q = p + o lies outside the half-resolution image.  Rejected unless q has a surface, the same material hash, dot(n_p, n_q) >= normalThreshold
 *              and |d_q - d_p| <= depthThreshold * d_p (G-buffer normals and depths), r_q has num > 0, a valid weight and a valid sample, and the sample lies
 *              in the receiver's hemisphere, dot(n_r, x_s - x_r) > 0 (sky samples: -n_s in place of x_s - x_r).
 *              Jacobian, v_r = x_r - x_s, v_n = x_n - x_s (x_n = r_q's stored xv):
 *                J = (|dot(n_s, v_r)| / sqrt(|v_r|^2)) * |v_n|^2 / ((|dot(n_s, v_n)| / sqrt(|v_n|^2)) * |v_r|^2), left to right, no contraction;
 *              a sky sample (any |x_s| component >= 1e20) has J = 1.  Rejected when J is not finite, J > jacobianMax or J < 1 / jacobianMax.
 *              RT_GI_SPATIAL_VISIBILITY: an any-hit ray from x_r towards normalize(x_s - x_r) with tmax = length(x_s - x_r) - 2e-2 (rejected when tmax <= 0),
 *              for a sky sample along -n_s with tmax = RT_INFINITY; occluded taps are rejected.
 *              merge: w = W_q * J (pHat = luminance(L) is the same at every receiver); r_s.weight += w; r_s.num += r_q.num; if rr * r_s.weight < w the sample
 *              becomes r_s's with xv = x_r, nv = n_r.  A rejected tap adds nothing.
 *   output     r_s, unclamped (nothing feeds it back), to the pass's buffer; the indirect stage's shading of r_s (BSDF at the stored xv / nv,
 *              bigW = weight / (luminance(L) * num), clampRadiance, HDRToLDR, clampRadiance) -> RT_BUF_DENOISE_IND_A, the image the filters (or compose with
 *              denoise == 0) read.
 *   samples = 0 reproduces the mode-off IND_A bit for bit; the pass never writes RT_BUF_INDIRECT_RESV0 / 1; nothing carries over between frames.
 *   The pass runs on the indirect stage's stream right after it in every schedule and every debugging_mode, and is timed under RT_STAGE_INDIRECT; it does not
 *   feed the ray counters.  Its reservoir buffer is allocated by the first frame rendered with the mode on and freed by rt_resize / rt_destroy.
 *   rt_run_stage(RT_STAGE_INDIRECT) on a context with the mode on is RT_ERR_INVALID_ARG (row-tiled hosts and the reference mode do not use the pass).
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_GI_SPATIAL_OFF = 0 /* default */, RT_GI_SPATIAL_ON = 1, RT_GI_SPATIAL_VISIBILITY = 2 };
typedef struct {
  int32_t mode;            /* RT_GI_SPATIAL_* ; default OFF */
  int32_t samples;         /* 0..16 neighbour taps per half-res pixel; default 4 (0 = the pass runs and merges nothing) */
  int32_t radius;          /* 1..64, half-resolution pixels; default 10 */
  float   normalThreshold; /* [-1, 1]: dot(n_p, n_q) >= it; default 0.9 */
  float   depthThreshold;  /* > 0, finite: |d_q - d_p| <= it * d_p; default 0.1 */
  float   jacobianMax;     /* >= 1, finite: taps with J > it or J < 1/it are rejected; default 10 */
  int32_t reserved[2];     /* must be 0 */
} rt_gi_spatial;           /* 32 B */
/* validates every field (bad values: RT_ERR_INVALID_ARG, the settings in use stay); a change of mode re-opens the stream-priority decision */
int rt_set_gi_spatial(rt_ctx* ctx, const rt_gi_spatial* s);
int rt_get_gi_spatial(rt_ctx* ctx, rt_gi_spatial* out);
/* the spatially resampled reservoirs of the last frame rendered with the mode on: rt_indirect_reservoir, (W/2) * (H/2) * 76 B; synchronous;
 * RT_ERR_NO_TARGET before the first such frame since rt_resize */
int rt_gi_spatial_readback(rt_ctx* ctx, void* dst, size_t bytes);
/* ------------------------------------------------------------------------------------------------------------------
 * Temporal anti-aliasing (added within ABI 2.4, no version bump): sub-pixel camera jitter plus one resolve pass per frame after compose.
 * Jitter (host side; the traced kernels are unchanged): a frame with debugging_mode == 0 is rendered with rt_taa_jitter_camera(&cam, frames, jitterPhases,
 * W, H) in place of the camera rt_set_camera stored (debug-view frames are neither jittered nor resolved):
 *   k = (frames mod jitterPhases) + 1 (frames < 0 taken modulo like a non-negative number); delta = (h2(k) - 0.5, h3(k) - 0.5) pixels, h2 / h3 the base-2 /
 *   base-3 radical inverses evaluated in IEEE double, each component rounded once to float (|delta| <= 0.469 per component for jitterPhases <= 16);
 *   ox = (2 * delta.x) / W, oy = (2 * delta.y) / H in fp32; the projInverse translation column becomes, per row r (fp32, no contraction, this order):
 *       m[12 + r] = (m[12 + r] + m[0 + r] * ox) + m[4 + r] * oy
 *   so that projInverse · (x, y, z, 1) becomes projInverse · (x + ox, y + oy, z, 1).  Every other field is copied bit for bit; jitterPhases = 0 returns the
 *   input bits.  projView, lastProjView, lastView and lastPosition stay unjittered, so motion vectors do not carry the jitter.  The context jitters the copy of
 *   the camera each frame's launches receive; rt_set_camera's stored camera, rt_pick and rt_reference_* never see the jitter.
 * Resolve (csrc/taa.hip), per full-resolution pixel p of frame f, for the two components D = RT_BUF_DIRECT_RESULT and I = RT_BUF_INDIRECT_RESULT after compose:
 *   no valid material in G(f) at p: D and I pass through unchanged, n = 1.
 *   x = cameraPosDenoise(jittered camera, p, G-buffer distance) (denoise_common.glsl:27-40); s = (ndc(lastProjView · (x, 1)).xy · 0.5 + 0.5) · (W, H);
 *   q = floor(s).  The history is consistent when the previous history is valid, q lies in the image and G(f-1) at q has the same material hash,
 *   dot(n, n_prev) > 0.9 and |lastPosition - x| < depth_prev · 1.05 (the direct stage's temporal test).  Inconsistent: out = (c.rgb, 1), n = 1.
 *   Consistent: n = min(n_prev(q) + 1, 1024); h = the 4 x 4 Catmull-Rom sample of the previous resolved image around s - 0.5 (taps clamped to the image,
 *   weights w0 = t(-0.5 + t(1 - 0.5t)), w1 = 1 + t²(-2.5 + 1.5t), w2 = t(0.5 + t(2 - 1.5t)), w3 = t²(-0.5 + 0.5t)); in YCoCg (Y = (r/4 + g/2) + b/4,
 *   Co = r/2 - b/2, Cg = (-r/4 + g/2) - b/4) mu and sigma = sqrt(max(0, E[v²] - mu²)) of c over the in-image 3 x 3 neighbourhood; d = h - mu, e = clipGamma ·
 *   sigma, t = max(1, max over channels with |d| > e of |d| / e), h = mu + d / t (a clip along the segment towards mu, not a per-channel clamp), back to RGB;
 *   a = max(alpha, 1/n); out = (h (1 - a) + c a, 1).  The outputs and n form the history of parity f.
 * History: two RGBA32F images + one f32 n per parity (W * H * 36 B each), allocated by the first frame rendered with the mode on and freed by rt_resize /
 * rt_destroy.  It is invalid after rt_resize, rt_upload_scene, rt_build_accel, an rt_set_taa that changes anything, rt_taa_reset, a frame with
 * debugging_mode != 0 (which skips the pass) and a frame whose parity does not follow the previous resolved frame's.
 * Schedule: the pass runs right after compose on compose's stream in every schedule and is timed under RT_STAGE_COMPOSE (rt_counters keeps its layout).
 * rt_tonemap(frames) reads the resolved images when frame `frames` was resolved, the plain result images otherwise.  The frame buffers (G-buffers, reservoirs,
 * result images, ...) are what the frame computes with the jittered camera; the pass writes only its history.  rt_run_stage on a context with the mode on is
 * RT_ERR_INVALID_ARG (the row-tiled hosts have no TAA); the reference mode ignores it.  A change of mode re-opens the stream-priority decision.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_TAA_OFF = 0 /* default */, RT_TAA_ON = 1 };
typedef struct {
  int32_t mode;          /* RT_TAA_*; default OFF */
  int32_t jitterPhases;  /* 0..16; default 8.  0 = no jitter (temporal accumulation only, for A/B) */
  float   alpha;         /* (0, 1]: blend-factor floor; default 0.1 */
  float   clipGamma;     /* > 0, finite: width of the colour box in standard deviations; default 1.0 */
  int32_t reserved[4];   /* must be 0 */
} rt_taa;                /* 32 B */
/* validates every field (bad values: RT_ERR_INVALID_ARG, the settings in use stay) */
int rt_set_taa(rt_ctx* ctx, const rt_taa* t);
int rt_get_taa(rt_ctx* ctx, rt_taa* out);
/* the next resolved frame starts without history */
int rt_taa_reset(rt_ctx* ctx);
/* the last resolved frame: which = 0 direct, 1 indirect (RGBA32F, W * H * 16 B), 2 history length n (f32, W * H * 4 B).  Synchronous.
 * RT_ERR_NO_TARGET before the first resolved frame since rt_resize. */
int rt_taa_readback(rt_ctx* ctx, int which, void* dst, size_t bytes);
/* pure function, no context, callable without a GPU: the camera the context renders frame `frames` with (jitterPhases 0..16, width, height >= 1) */
int rt_taa_jitter_camera(const rt_scene_camera* in, int frames, int jitterPhases, int width, int height, rt_scene_camera* out);
/* ------------------------------------------------------------------------------------------------------------------
 * Temporal upsampling (added within ABI 2.4, no version bump): render at the size rt_resize set (the render size W x H) with the jittered
 * camera, resolve after compose into a history at the output size Wo x Ho (W <= Wo <= 4 W, H <= Ho <= 4 H; the two ratios may differ and need not be
 * integers), read the displayable frame at the output size.  Tracing fewer pixels is what it buys: the traced stages cost in proportion to W * H.
 * Jitter: a frame with debugging_mode == 0 is rendered with rt_upscale_jitter_camera(&cam, frames, jitterPhases, W, H, ., delta) in place of the camera
 *   rt_set_camera stored: the arithmetic of rt_taa_jitter_camera (one implementation), 0..64 phases; for jitterPhases <= 16 the camera bits are
 *   rt_taa_jitter_camera's.  delta = (h2(k) - 0.5, h3(k) - 0.5), k = (frames mod jitterPhases) + 1, is the offset in render pixels (|delta| < 0.5 per
 *   component; (0, 0) for jitterPhases = 0): under the jitter render pixel p is sampled at render-pixel position p + 0.5 + delta.
 * Resolve (csrc/upscale.hip), per output pixel o of frame f, fp32, IEEE divisions and square roots, no contraction, for the two components
 * D = RT_BUF_DIRECT_RESULT and I = RT_BUF_INDIRECT_RESULT after compose (c = that image at render pixel p):
 *   rho = (float(W) / float(Wo), float(H) / float(Ho)); u = (float(o) + 0.5) * rho; p = int(min(max(floor(u - delta), 0), float((W, H) - 1)));
 *   e = u - ((float(p) + 0.5) + delta): from this frame's nearest sample to the output pixel's centre, in render pixels.
 *   No valid material in G(f) at p: D and I of p pass through unchanged (all four channels), n = 1.
 *   Reprojection as in TAA, at the render size: x = cameraPosDenoise(jittered camera, p, G-buffer distance, (W, H)); sR = (ndc(lastProjView · (x, 1)).xy ·
 *   0.5 + 0.5) · (W, H); q = floor(sR).  sO = (sR + e) / rho is the history position of o.  The history is consistent when the previous history is
 *   valid, q lies in the render image, G(f-1) at q has the same material hash, dot(n, n_prev) > 0.9 and |lastPosition - x| < depth_prev · 1.05 (the direct
 *   stage's temporal test), and floor(sO) lies in the output image.  Inconsistent: out = (c.rgb, 1), n = 1 (nearest-sample upsampling).
 *   Consistent: n = min(n_prev(floor(sO)) + 1, 1024); h = the 4 x 4 Catmull-Rom sample of the previous resolved image (Wo x Ho, taps clamped, TAA's
 *   weights and order) around sO - 0.5; h is clipped in YCoCg onto mu ± clipGamma · sigma of c over the in-image 3 x 3 RENDER-size neighbourhood of p with
 *   TAA's clip along the segment; kappa = max(0, 1 - |e.x| / rho.x) * max(0, 1 - |e.y| / rho.y) (a sample on the output centre counts fully, one a whole
 *   output pixel away not at all: that pixel keeps its clipped history this frame); a = max(alpha * kappa, 1 / float(n)); out = (h (1 - a) + c a, 1).
 *   The outputs and n form the history of parity f.
 * History: two RGBA32F images + one f32 n per parity (Wo * Ho * 36 B each), allocated by the first resolved frame together with what rt_upscale_tonemap
 *   needs at the output size (an RGBA8 target, row sums, means, mip pyramids); freed by rt_resize, rt_destroy and an rt_set_upscale that changes the output
 *   size.  It is invalid after rt_resize, rt_upload_scene, rt_build_accel, an rt_set_upscale that changes anything, rt_upscale_reset, a frame with
 *   debugging_mode != 0 (neither jittered nor resolved) and a frame whose parity does not follow the previous resolved frame's.  Mode off allocates nothing
 *   and launches nothing.
 * Schedule: the pass runs right after compose on compose's stream in every schedule (with frames in flight before the frame's completion event is
 *   recorded) and is timed under RT_STAGE_COMPOSE.  It writes only its history: the frame buffers are what the frame computes at W x H with the jittered
 *   camera, and rt_tonemap / RT_BUF_LDR keep showing the render-size result images.  Settled primary visibility is off while the mode is on.
 * Refusals (RT_ERR_INVALID_ARG, rt_last_error names the reason, the settings in use stay): bad field values; turning the mode on while TAA is on, and
 *   rt_set_taa(RT_TAA_ON) while it is on (one jitter, one resolve); rt_run_stage while it is on; an rt_render_frame whose render size no longer satisfies
 *   the ratio limits after an rt_resize (rt_set_upscale checks them when a target exists).  The row-tiled hosts and rt_mgpu_* have no upsampling; the
 *   reference mode ignores it.  A change of mode re-opens the stream-priority decision.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_UPSCALE_OFF = 0 /* default */, RT_UPSCALE_TEMPORAL = 1 };
typedef struct {
  int32_t mode;                  /* RT_UPSCALE_*; default OFF */
  int32_t outWidth, outHeight;   /* W <= outWidth <= 4 W, H <= outHeight <= 4 H (checked with mode TEMPORAL; ignored, but >= 0, with mode OFF); default 0 */
  int32_t jitterPhases;          /* 0..64; default 16.  0 = no jitter (for A/B) */
  float   alpha;                 /* (0, 1]: weight of a sample that lies on the output pixel's centre; default 0.1 */
  float   clipGamma;             /* > 0, finite: width of the colour box in standard deviations; default 1.0 */
  int32_t reserved[2];           /* must be 0 */
} rt_upscale;                    /* 32 B */
/* validates every field (bad values: RT_ERR_INVALID_ARG, the settings in use stay) */
int rt_set_upscale(rt_ctx* ctx, const rt_upscale* u);
int rt_get_upscale(rt_ctx* ctx, rt_upscale* out);
/* the next resolved frame starts without history */
int rt_upscale_reset(rt_ctx* ctx);
/* the last resolved frame at the output size: which = 0 direct, 1 indirect (RGBA32F, Wo * Ho * 16 B), 2 history length n (f32, Wo * Ho * 4 B), 3 the
 * RGBA8 image rt_upscale_tonemap last wrote (Wo * Ho * 4 B).  Synchronous.  RT_ERR_NO_TARGET before the first resolved frame since the history was freed. */
int rt_upscale_readback(rt_ctx* ctx, int which, void* dst, size_t bytes);
/* rt_tonemap's post pass (debugging_mode 0) over the resolved images of frame `frames` at Wo x Ho, into the output-size RGBA8 target.  RT_ERR_NO_TARGET
 * when frame `frames` is not the resolved frame its parity's history holds. */
int rt_upscale_tonemap(rt_ctx* ctx, const rt_tonemapper* tm, int frames);
/* pure function, no context, callable without a GPU: the camera the context renders frame `frames` with (jitterPhases 0..64, width, height >= 1: the RENDER
 * size) and, when delta is not NULL, the offset in render pixels */
int rt_upscale_jitter_camera(const rt_scene_camera* in, int frames, int jitterPhases, int width, int height, rt_scene_camera* out, float delta[2]);
/* ------------------------------------------------------------------------------------------------------------------
 * Moving instances (added within ABI 2.4, no version bump; csrc/refit.hip).  The reference changes an instance's objectToWorld and rebuilds its TLAS per frame
 * (src/accelstruct.cpp:132-162).  Here every (instance, triangle) pair is a world-space leaf record of one flat BVH8, so a move rewrites the leaf records of the
 * moved instances and refits the node boxes above them on the GPU; the tree keeps its topology (no rebuild, no re-derived alpha records or micro-maps, no upload
 * of the scene).  Results are a function of the triangle set only, never of the tree, so frames and ray queries after an update are bit for bit
 * those of a context that uploaded and built the moved scene; what a refitted tree loses against a fresh one is speed (profiles/refit_timing.txt).
 *
 * rt_update_instances(ctx, count, instanceIds, objectToWorld): objectToWorld = count x 12 floats, the layout of rt_instance::objectToWorld.
 *   Valid after rt_build_accel (RT_ERR_NO_SCENE / RT_ERR_NO_ACCEL otherwise).  An id out of range, a duplicate id, a non-finite matrix entry or a determinant that is
 *   zero or not finite refuses the WHOLE call with RT_ERR_INVALID_ARG and changes nothing.  count == 0 is a valid call that moves nothing.
 *   It overwrites objectToWorld in the context's copy of the scene (a later rt_build_accel builds the moved scene); the device instance rows (objectToWorld and its
 *   inverse, the builder's own expression, so the bits equal a fresh build's); v0 / e1 / e2 and the TRI_FLIP bit of EVERY leaf record of those instances (spatial-split
 *   duplicates included; globalId, alphaIdx, the micro-map and the other flags stay); the boxes of every node above such a record; and the hit rule's pad
 *   2e-5 * max(1e-3, largest |world coordinate| over all triangles), which equals a fresh build's value.  A leaf slot whose triangles did not move keeps its box (its
 *   bytes where the node's grid of that axis did not change); a node with no moved record below it keeps all 80 bytes.  When the pad grows beyond the one the
 *   tree's boxes were computed with, every leaf box is recomputed with the new pad (rt_refit_stats::fullRefit); a smaller pad leaves the boxes as they are.
 *   It resets the reference-mode sums (n -> 0) like rt_build_accel.  It leaves the SVGF and TAA histories alone: their consistency tests (material hash, normal,
 *   depth) reject a surface that changed under a pixel, and motion vectors stay camera-only as in the reference.  It does not re-open the stream-priority decision
 *   and frees nothing.
 *   Ordering: v1 drains the pipeline — the call joins the frames in flight, runs its kernels on the context's main stream and returns after they completed.
 *   Scope: the single-GPU context only.  rt_mgpu_* contexts and the row-tiled hosts (restir_amd/tiled.py) have no update path: they upload the moved scene.
 * rt_update_lights: overwrites the device light arrays in place, for a host that moved an emissive instance (its Scene recomputes the triangle-light records; without
 *   this call a moved emitter keeps lighting from its old place, unless rt_set_light_sources has bound the records to their triangles).  numTrig / numPunc and info's sizes must equal the uploaded counts, and the records pass the index
 *   checks of rt_upload_scene, else RT_ERR_INVALID_ARG and nothing changes.  info->trigSampProb replaces the uploaded one.  Resets the reference-mode sums; drains the pipeline.
 * rt_get_refit_stats: what the last rt_update_instances did.
 * rt_accel_readback: the device tree as it is now, for tests and diagnostics: RT_ACCEL_NODES (80 B per node, rt_accel_stats' node count), RT_ACCEL_TRIS (64 B per
 *   leaf record, rt_accel_quality's reference count), RT_ACCEL_INSTANCES (112 B per instance: objectToWorld, worldToObject, primMesh, flags, 8 B of padding).
 *   `bytes` must be the exact size.  Synchronous.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t instances;     /* instances moved by the call */
  uint32_t leafRecords;   /* leaf records rewritten */
  uint32_t nodes;         /* nodes refitted */
  uint32_t levels;        /* levels of the tree (one launch each) */
  uint32_t fullRefit;     /* 1: the pad grew and every leaf box was recomputed */
  float    ms;            /* HIP-event time of the call's kernels and copies on the main stream */
  float    triPad;        /* the hit rule's pad after the call */
  float    treePad;       /* the pad the tree's boxes are computed with (>= triPad) */
} rt_refit_stats;         /* 32 B */
enum { RT_ACCEL_NODES = 0, RT_ACCEL_TRIS = 1, RT_ACCEL_INSTANCES = 2, RT_ACCEL_ALPHA = 3 /* "Editing materials and textures" below */ };
int rt_update_instances(rt_ctx* ctx, uint32_t count, const uint32_t* instanceIds, const float* objectToWorld);
int rt_update_lights(rt_ctx* ctx, const rt_trig_light* trigLights, uint32_t numTrig, const rt_punc_light* puncLights, uint32_t numPunc, const rt_light_buf_info* info);
int rt_get_refit_stats(rt_ctx* ctx, rt_refit_stats* out);
int rt_accel_readback(rt_ctx* ctx, int which, void* dst, size_t bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Rebuilding on the device (added within ABI 2.4, no version bump; csrc/accel_build.hip).  A refitted tree keeps the topology of the scene it was
 * built for and traces slower the further the instances move (profiles/refit_timing.txt); rt_build_accel is the host builder and pauses a large scene for more than a
 * second.  rt_rebuild_accel builds a NEW topology on the GPU from the scene as it is after all rt_update_instances calls so far: Morton order of the triangle box
 * centres (63-bit keys), a binary radix tree over the sorted keys, a top-down collapse to 8-wide nodes, and the refit kernel's boxes.  No spatial splits and no SAH:
 * one leaf record per (instance, triangle) pair.  Results are a function of the triangle set only: frames and ray queries on the device-built tree are
 * bit for bit those of the host-built tree; the two differ in speed (profiles/accel_build_timing.txt).  The build is deterministic: the same scene gives the same words.
 * rt_set_rebuild_options ("The PLOC builder" below) selects another builder for the binary tree, whose trees trace faster and take longer to build.
 *
 * rt_rebuild_accel(ctx): valid after rt_build_accel (RT_ERR_NO_SCENE / RT_ERR_NO_ACCEL otherwise) — the host build stays the way a scene gets its first tree, and it
 *   is the source of what does not depend on position (globalId, TRI_OPAQUE / TRI_NOCULL, alphaIdx, the opacity micro-map), kept per triangle on the device.
 *   Ordering: like rt_update_instances v1 it joins the frames in flight, runs on the context's main stream and returns after its kernels completed.
 *   It leaves the frame buffers, the SVGF / TAA histories and the stream-priority decision alone, and resets the reference-mode sums (n -> 0).
 *   Afterwards rt_accel_stats, rt_accel_quality's reference count (= the triangle count; the SAH expectations read 0) and rt_accel_readback describe the new tree,
 *   the hit rule's pad and the pad of the tree's boxes are both 2e-5 * max(1e-3, largest |world coordinate|), and rt_update_instances works on the new tree.  A
 *   later rt_build_accel builds the host tree of the moved scene, as before.
 *   Buffers: working buffers and two trees (the build never writes the tree the context uses; they swap on success) are allocated by the first rebuild after a host
 *   build, about 0.7 KB per triangle, and kept; a repeated rebuild allocates and frees nothing unless the tree's depth crosses a multiple of 4 (the traversal stack).
 *   Failure: a wide tree deeper than the traversal stack (64 levels) gives RT_ERR_INVALID_ARG, an allocation that fails RT_ERR_OOM, a HIP error or an internal
 *   invariant of the builder that did not hold RT_ERR_HIP (rt_last_error names it); the previous tree stays in place and usable.
 *   Scope: the single-GPU context only.  rt_mgpu_* contexts and the row-tiled hosts (restir_amd/tiled.py) have no rebuild path: they upload the moved scene.
 * rt_get_rebuild_stats: what the last rt_rebuild_accel did.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t triangles;     /* leaf records = (instance, triangle) pairs */
  uint32_t nodes;         /* wide nodes */
  uint32_t levels;        /* levels of the wide tree (one collapse launch each) */
  uint32_t maxDepth;      /* rt_accel_stats' depth of the new tree (= levels) */
  float    ms;            /* HIP-event time of the call's kernels and copies on the main stream */
  float    sortMs;        /* of which the radix sort */
  float    triPad;        /* the hit rule's pad = the pad of the tree's boxes after the call */
  uint32_t iterations;    /* PLOC: merge iterations of the build; 0 for LBVH */
} rt_rebuild_stats;       /* 32 B */
int rt_rebuild_accel(rt_ctx* ctx);                       /* LBVH (or PLOC, below) -> BVH8 on the GPU from the context's current scene */
int rt_get_rebuild_stats(rt_ctx* ctx, rt_rebuild_stats* out);
/* ------------------------------------------------------------------------------------------------------------------
 * The PLOC builder (added within ABI 2.4, no version bump; csrc/accel_build.hip).  The device build's binary hierarchy is by default an LBVH: cheap to
 * build, slow to trace.  rt_set_rebuild_options selects PLOC instead (parallel locally-ordered clustering, Meister & Bittner 2018): the sorted triangles start as
 * one cluster each; in every iteration a cluster looks `radius` positions to each side along the Morton order for the neighbour whose union box has the smallest
 * surface area, and two clusters that chose each other merge into one node.  The area of the merged box is what a SAH build minimises, so the tree is tighter.
 * Records, keys, sort, the collapse to 8-wide nodes, the slot rule, the leaf size (<= 3) and the boxes are the LBVH path's: one quantiser, one layout.  The build is
 * deterministic (ties go to the lower positions; tests/ploc_checker.cpp restates it word for word) and results do not depend on the tree; the
 * trees differ in speed and in build time (profiles/ploc_timing.txt).
 *
 * rt_set_rebuild_options(ctx, options): valid any time after rt_create; the options survive rt_upload_scene, rt_build_accel and rt_resize.  It governs every later
 *   device build — rt_rebuild_accel and the build inside rt_set_instances — and itself builds nothing and drops nothing.
 *   Values: builder RT_REBUILD_LBVH (the default) or RT_REBUILD_PLOC; radius 1..64, 0 = the default (16); maxIterations > 0, 0 = the default (512); reserved 0.
 *   Anything else gives RT_ERR_INVALID_ARG and leaves the options as they were.  radius and maxIterations are kept, and ignored, under RT_REBUILD_LBVH.
 *   Buffers: PLOC's clusters (two copies: an iteration reads one and writes the other) and neighbour links, 76 B per triangle of the working buffers' capacity, are
 *   allocated by the first PLOC build into the pool of the rebuild's working buffers and dropped with it (a host build, a new scene, an rt_set_instances that
 *   outgrows the capacity); switching back to LBVH frees nothing, a repeated PLOC build allocates nothing.  An rt_set_instances that allocates them reports
 *   rt_instances_stats.reallocated = 1.
 *   Cost: one read-back of the cluster count per iteration (rt_rebuild_stats.iterations), and about 2 x radius candidate boxes per cluster per iteration.
 *   Failure: a build that has not reached one cluster after maxIterations iterations is refused like a tree deeper than the stack — RT_ERR_INVALID_ARG,
 *   rt_last_error "... PLOC did not reach one cluster within maxIterations merge iterations", the previous tree in place and usable.  (Every iteration merges at
 *   least one pair, so n - 1 iterations always suffice for n triangles; nested boxes come close to needing them.)  An iteration that merges nothing is a broken
 *   invariant: RT_ERR_HIP.
 *   Scope: the single-GPU context only, like rt_rebuild_accel.
 * rt_get_rebuild_options: the values in force, defaults filled in.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_REBUILD_LBVH = 0, RT_REBUILD_PLOC = 1 };
typedef struct {
  int32_t builder;        /* RT_REBUILD_*; default RT_REBUILD_LBVH */
  int32_t radius;         /* PLOC search radius in cluster positions, 1..64; 0 = the default radius */
  int32_t maxIterations;  /* PLOC: refuse the build after this many merge iterations; 0 = the default cap (512) */
  int32_t reserved;       /* must be 0 */
} rt_rebuild_options;     /* 16 B */
int rt_set_rebuild_options(rt_ctx* ctx, const rt_rebuild_options* options);
int rt_get_rebuild_options(rt_ctx* ctx, rt_rebuild_options* out);   /* the values in force, defaults filled in */
/* ------------------------------------------------------------------------------------------------------------------
 * Adding and removing instances (added within ABI 2.4, no version bump; csrc/instances.hip).  rt_update_instances moves instances, the deform
 * calls bend meshes, rt_rebuild_accel gives a new topology; what none of them can do is change WHICH objects exist.  rt_set_instances replaces the whole instance
 * table without a new scene: prim meshes, vertices (as they are on the device now, skins and morphs applied), indices, materials, textures, lights and environment
 * stay as uploaded.  What a leaf record holds besides its position is a function of (prim mesh, triangle, instance flags) only; it is kept per prim mesh on the
 * device (the templates: one alpha record and one opacity micro-map per triangle, made the first time a mesh has an instance without RT_INST_FORCE_OPAQUE) and
 * expanded per (instance, triangle) pair by a kernel; positions, TRI_FLIP and the tree come from rt_rebuild_accel's pipeline.  Frames, rays and the tree are bit
 * for bit those of rt_upload_scene + rt_build_accel + rt_rebuild_accel of the new description (leaf records differ in alphaIdx only, whose numbering is per mesh).
 *
 * rt_set_instances(ctx, numInstances, instances): valid after rt_build_accel (RT_ERR_NO_SCENE / RT_ERR_NO_ACCEL otherwise), on a host-built or device-built tree.
 *   Afterwards the context is in the state rt_rebuild_accel leaves: the tree is a device-built tree over the new set (an LBVH, or PLOC's when rt_set_rebuild_options selected it; no spatial splits: it traces slower
 *   than a host-built one until a later rt_build_accel, which builds the new scene because the context's copy of the table is replaced); rt_update_instances,
 *   rt_update_vertices, rt_update_skins, rt_update_morphs and rt_rebuild_accel work on it; rt_accel_stats and rt_accel_readback describe it.
 *   Refusals (RT_ERR_INVALID_ARG, nothing changes, rt_last_error names the first offender): a NULL table; numInstances == 0; a total triangle count of 0 or above
 *   2^31 - 1 (bit 31 of the record index is used by the call); a prim mesh out of range; a matrix rt_update_instances would refuse (a non-finite entry, a
 *   determinant that is zero or not finite, no finite inverse); the emitter rule.  rt_upload_scene refuses no instance flag bits, and neither does this call.
 *   The emitter rule: triangle-light records, the alias table and the light-source binding name instances by index.  In a scene with triangle lights, every
 *   index i below the old count whose old instance has an emissive prim mesh (the scene's light rule, as rt_set_skins applies it: luminance of the material's
 *   emissiveFactor > 1e-2), or that a light-source binding names, must hold the same rt_instance in the new table, all bytes of primMesh, flags and objectToWorld equal, and no other new instance may use
 *   an emissive prim mesh.  A host puts its emitters first and moves them with rt_update_instances.  A scene without triangle lights is not affected.
 *   Ordering: like rt_rebuild_accel it joins the frames in flight, runs on the context's main stream and returns after its kernels completed.  It leaves the frame
 *   buffers, the SVGF / TAA histories and the stream-priority decision alone and resets the reference-mode sums (n -> 0).  It also drops the settled primary
 *   visibility (as rt_build_accel does), resets the primary seed plane, and makes every instance's previous matrix its current one: object and vertex motion see
 *   no motion across the call, and a surface that appeared restarts through the G-buffer tests.  No other per-pixel plane holds an instance or record index across
 *   frames.  Skins, morph sets (with their weights) and the light-source binding are kept.
 *   Buffers: the rebuild's working buffers and two trees, two record tables, two triRef arrays and two instance-row arrays (a call writes the ones the context
 *   does not use; they swap on success) are allocated by the first call after a host build, with 1/8 slack over the triangle and the instance count, and again by a
 *   call whose counts exceed that capacity (reallocated = 1 in both cases; the old buffers are freed after the new tree is in place).  A call that fits allocates
 *   and frees nothing unless the tree's depth crosses a multiple of 4 (the traversal stack), or the table outgrows the deform calls' per-instance job table.
 *   Bus traffic: a call that makes no template moves numInstances * 112 + (numInstances + 1) * 4 + 24 bytes host -> device: the instance rows, the prefix words
 *   (first record of every instance; bit 31: the matrix mirrors) and the 24-byte seed of the build's centre bounds.  The first call also uploads one word per prim
 *   mesh, and a call that makes templates 80 bytes per triangle of the meshes concerned.
 *   Failure: an allocation that fails (RT_ERR_OOM), a tree deeper than the traversal stack (RT_ERR_INVALID_ARG), a HIP error or a builder invariant (RT_ERR_HIP)
 *   leave the previous instance table, tree, record table and refit state in place and usable.
 *   Not done: rt_mgpu_* contexts and the row-tiled hosts (they upload the new scene); new prim meshes or
 *   triangles (emissive instances added, removed or re-indexed: the emitter mode, "Emitters" below); event-ordered instead of drained updates; SAH / spatial splits on the device (DESIGN.md §19's frame cost applies until a host build).
 * rt_get_instances_stats: what the last rt_set_instances that succeeded did.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t instances;        /* instances after the call */
  uint32_t triangles;        /* leaf records = (instance, triangle) pairs after the call */
  uint32_t added, removed;   /* new count - common prefix length with the old table; old count - that length (diagnostic only) */
  uint32_t bytesUploaded;    /* bytes the call moved host -> device */
  uint32_t reallocated;      /* 1: the device buffers were too small for the new counts (or absent: first call after a host build; PLOC's on its first build) and were allocated */
  float    expandMs;         /* HIP-event time of the record-expansion kernels */
  float    ms;               /* HIP-event time of the whole call on the main stream (expansion + device build) */
} rt_instances_stats;        /* 32 B */
int rt_set_instances(rt_ctx* ctx, uint32_t numInstances, const rt_instance* instances);
int rt_get_instances_stats(rt_ctx* ctx, rt_instances_stats* out);
/* ------------------------------------------------------------------------------------------------------------------
 * Object motion vectors (added within ABI 2.4, no version bump; the RT_OM builds of csrc/stages.hip).  rt_update_instances moves a surface, but the
 * reference's temporal lookup reprojects a hit with the camera's lastProjView and measures reprojDepth from the camera's lastPosition only, so on a moved surface
 * it lands on whatever was at that world position one frame earlier: the history is rejected (the prop stays noisy) or, on a large one-material object, taken
 * from the wrong surface point.  With the mode on, for a pixel that sees instance i the frame behaves as if the previous camera had been a per-instance camera:
 *   P = the instance's objectToWorld when the previous frame was rendered, C = its current one, M = P · inverse(C) (a current world point -> where that material
 *   point was); lastProjView_i = lastProjView · M; lastPosition_i = C · (inverse(P) · lastPosition), so that |lastPosition_i - x| = |lastPosition - M x| for rigid motion.
 * Every kernel expression stays what it is; createMotionIndex reads lastProjView_i, and reprojDepth of the direct and the indirect temporal lookup lastPosition_i.
 * The normal test, the material hash, the column 0-1 exclusion and every quirk of DESIGN.md §6 are untouched — so a rotation of more than acos(0.9) = 25.8 degrees
 * per frame (indirect: acos(0.5)) rejects the history, and a reused reservoir's light sample / GI sample points are one frame stale (ReSTIR's own lag).
 *
 * rt_object_motion_camera(cam, prev, cur, out): pure function, no context, callable without a GPU.  out = *cam with lastProjView and lastPosition replaced.
 *   fp32, no contraction (include/rt_detmath.h), this order: Pi = inverseAffine(prev), Ci = inverseAffine(cur) (the BVH builder's expression);
 *   M[r][c] = (P[r][0] Ci[0][c] + P[r][1] Ci[1][c]) + P[r][2] Ci[2][c], and for c = 3 then + P[r][3];
 *   lastProjView_i[r][c] = (L[r][0] M[0][c] + L[r][1] M[1][c]) + L[r][2] M[2][c], and for c = 3 then + L[r][3]   (L = cam->lastProjView; M's fourth row is 0 0 0 1);
 *   q = (Pi[r][0] x + Pi[r][1] y + Pi[r][2] z) + Pi[r][3] of lastPosition, lastPosition_i = the same expression with cur applied to q.
 *   prev == cur bit for bit returns *cam bit for bit (copied, not computed); so does a prev or cur that is not finite, or whose determinant is zero or not
 *   finite, or whose inverse is not finite.  RT_ERR_INVALID_ARG only for a NULL pointer.
 * rt_set_object_motion(ctx, mode): RT_OBJECT_MOTION_OFF (default) / _ON / _VERTEX ("Per-vertex motion vectors" below).  A call that changes nothing does nothing; a change invalidates no history and does
 *   not re-open the stream-priority decision.  The context keeps, per instance, the objectToWorld of the last frame rt_render_frame rendered (whether the mode is
 *   on or off): rt_update_instances records it once, so several updates between two frames keep the rendered frame's matrix; issuing a frame's direct stage makes
 *   every previous matrix the current one.  rt_build_accel and rt_rebuild_accel keep this state; rt_upload_scene and rt_resize clear it.  An instance is IN
 *   MOTION for a frame when its two matrices differ in any bit.
 *   Frames (rt_render_frame) with the mode on run the direct and the indirect stage from the object-motion builds, which store the instance image (below).  When
 *   at least one instance is in motion, the table {lastProjView_i, lastPosition_i} of all instances (rt_object_motion_camera per moved instance, the camera's
 *   values copied for the others; 80 B per instance) is uploaded on the direct stage's stream ahead of it; when none is, no table exists and every pixel reads the
 *   camera's values, so the frame equals the mode-off frame word for word — as do the pixels of a static instance in any frame.
 *   There is no counting form of these builds: with rt_set_counting on, a frame with an instance in motion is RT_ERR_INVALID_ARG (the message names the
 *   combination), and a frame with none runs the counting kernels, which do not write the instance image.
 *   rt_run_stage (and so restir_amd/tiled.py) and rt_mgpu_* contexts ignore the mode in this version: they run the default kernels with the camera's values and do
 *   not advance the motion state.  The SVGF and TAA passes are unchanged: SVGF reads RT_BUF_MOTION, so it reprojects to the object-motion position and keeps its
 *   camera-only depth test (it may reject, it cannot accept a wrong surface); TAA reprojects from its own camera.
 * rt_object_motion_readback(ctx, dst, bytes): the instance image of the last frame rendered with the mode on (in motion or not; counting frames excepted):
 *   uint32 per full-resolution pixel (W * H * 4 B, `bytes` must be exact, else RT_ERR_INVALID_ARG), the index of the instance the primary ray hit, 0xffffffff
 *   where it missed.  RT_ERR_NO_TARGET before the first such frame since rt_resize.  Synchronous.  The image has the lifetime of RT_BUF_MOTION (written by the
 *   direct stage, read by the indirect stage of the same frame at 2p) and is rotated with it by the frames-in-flight schedules and rt_rotate_buffers; it is
 *   allocated by rt_resize once the mode has been switched on (or by the call that first switches it on).
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_OBJECT_MOTION_OFF = 0 /* default */, RT_OBJECT_MOTION_ON = 1, RT_OBJECT_MOTION_VERTEX = 3 /* per-vertex motion vectors, below; 2 is not a mode: RT_ERR_INVALID_ARG */ };
int rt_set_object_motion(rt_ctx* ctx, int mode);
int rt_object_motion_camera(const rt_scene_camera* cam, const float prevObjectToWorld[12], const float curObjectToWorld[12], rt_scene_camera* out);
int rt_object_motion_readback(rt_ctx* ctx, void* dst, size_t bytes);
/* ------------------------------------------------------------------------------------------------------------------
 * Per-vertex motion vectors (added within ABI 2.4, no version bump; the RT_VM builds of csrc/stages.hip, csrc/vmotion.hip): a third mode (value 3; 2 is not a mode and stays RT_ERR_INVALID_ARG) of
 * rt_set_object_motion.  The per-instance camera of mode 1 cannot express a deformation (rt_update_vertices, rt_update_skins, rt_update_morphs): a bent surface
 * has no single matrix.  Mode RT_OBJECT_MOTION_VERTEX runs both temporal lookups with the PREVIOUS WORLD POSITION OF THE MATERIAL POINT under the pixel, from the
 * previous frame's vertices and the previous frame's objectToWorld; it covers rigid instance motion too, with no matrix inverse.  Modes 0 and 1 keep their
 * meaning and their kernels.  For a full-resolution pixel p whose primary ray hits triangle (i0, i1, i2) of prim mesh m in instance i, bary = ((1 - u) - v, u, v):
 *   q_k    = the position vertex i_k had at the last frame rt_render_frame rendered, when m was deformed since that frame by rt_update_vertices, rt_update_skins
 *            or rt_update_morphs; else its live position.
 *   P      = the objectToWorld instance i had at that frame when it was moved since (rt_update_instances; the state mode 1 keeps); else its current matrix.
 *   x_prev = xformPoint(P, (q0 * bary.x + q1 * bary.y) + q2 * bary.z), every component of the interpolation in that order and
 *            xformPoint(P, q)[r] = ((P[4r] * q.x + P[4r+1] * q.y) + P[4r+2] * q.z) + P[4r+3]: fp32, no contraction (include/rt_detmath.h) — the expression of
 *            state.position with the previous data.  Computed only when i is in motion or m was deformed; otherwise x_prev = state.position, copied.
 *   d(p)   = x_prev - state.position, component by component; 0 at a miss.
 *   direct stage:   motionIdx = createMotionIndex(x_prev) with the camera's own lastProjView; reprojDepth = length(lastPosition - x_prev).
 *   indirect stage at half-resolution pixel q: reprojDepth = length(lastPosition - (primState.position + d(2q))); the motion index is read from RT_BUF_MOTION
 *            at 2q as before, and primState.position keeps its reconstruction from the half-resolution ray.
 *   Everything else is untouched: the normal tests, the material hash, the column 0-1 exclusion, every quirk of DESIGN.md §6.  A bend of more than acos(0.9)
 *   per frame still rejects the direct history (previous normals are not kept), and a reused sample is one frame stale.
 * When no instance is in motion and no mesh was deformed since the last rendered frame no table exists, every pixel takes the camera's values and the frame
 * equals the mode-off frame word for word; so do the pixels of static, undeformed instances in any frame.
 * Context: once the mode has been switched on the context keeps one 16-byte row per scene vertex (the previous-position plane).  The first deforming call for a
 * mesh after a rendered frame copies the mesh's live positions there ahead of its commit, whether the mode is on or off; later calls before the next frame do
 * not (the rendered frame's positions stay, as the matrices of mode 1 do); issuing a frame's direct stage makes every mesh undeformed.  rt_build_accel and
 * rt_rebuild_accel keep the state; rt_upload_scene and rt_resize clear it; switching the mode invalidates no history.  A frame with something in motion or
 * deformed uploads one 64-byte row per instance {P, flags (bit 0 moved, bit 1 mesh deformed)} ahead of the direct stage.  Counting, rt_run_stage,
 * restir_amd/tiled.py, rt_mgpu_*, SVGF and TAA: as mode 1 (a frame with something in motion or deformed under rt_set_counting is RT_ERR_INVALID_ARG).
 * Frames of this mode also write the instance image, so rt_object_motion_readback keeps its contract.
 * rt_vertex_motion_readback(ctx, dst, bytes): the delta image of the last frame rendered with this mode: float4 (d.xyz, 0) per full-resolution pixel, W * H * 16 B,
 *   `bytes` must be exact (else RT_ERR_INVALID_ARG).  RT_ERR_NO_TARGET before the first such frame since rt_resize.  Synchronous.  The image has the lifetime of
 *   the instance image: three copies rotated with RT_BUF_MOTION, allocated by rt_resize once this mode has been on (or by the call that first switches it on).
 * ---------------------------------------------------------------------------------------------------------------- */
int rt_vertex_motion_readback(rt_ctx* ctx, void* dst, size_t bytes);
/* ------------------------------------------------------------------------------------------------------------------
 * Deforming meshes (added within ABI 2.4, no version bump; csrc/deform.hip).  rt_update_instances moves rigid instances; these calls change the
 * VERTICES of a prim mesh on the device — rows supplied by the host (rt_update_vertices: cloth, anything the host computes; morph targets have a device path of their own, "Morph targets" below) or posed on the GPU from
 * a rest pose and a few joint matrices (rt_set_skins once, rt_update_skins per frame) — then rewrite the leaf records of every instance of that mesh and refit the
 * BVH8 above them with the kernels of rt_update_instances.  No upload of the scene, no rebuild, no re-derived alpha records or micro-maps.  Results are a function of
 * the triangle set only: frames and ray queries afterwards are bit for bit those of a context that uploaded and built the deformed scene.
 * EVERY instance of a prim mesh deforms with it: characters that move independently need a prim mesh each.
 *
 * rt_update_vertices(ctx, primMesh, firstVertex, count, rows): replaces rows [firstVertex, firstVertex + count) of one prim mesh (indices relative to the mesh).
 *   Valid after rt_build_accel (RT_ERR_NO_SCENE / RT_ERR_NO_ACCEL otherwise).  A prim mesh out of range, a range outside the mesh, a non-finite position, a texcoord
 *   whose bits differ from the uploaded row (the alpha records and opacity micro-maps were derived from it, and the tangent's handedness bit lives there) or a mesh
 *   that has a skin refuses the WHOLE call with RT_ERR_INVALID_ARG and changes nothing.  Position, normal, tangent and colour may change.  count == 0 is a valid call
 *   that changes no vertex.  The rows also replace the context's copy of the scene (a later rt_build_accel builds the deformed scene).
 *   Emitters: the triangle-light records hold world positions; a host that deforms an emissive mesh recomputes them and calls rt_update_lights, or binds the
 *   records to their triangles once (rt_set_light_sources, "Light sources" below): the call then rewrites them on the device.
 * rt_set_skins(ctx, numSkins, skins, numInfluences, influences): valid after rt_upload_scene.  Replaces all skins (numSkins == 0 removes them).  Skin k poses prim
 *   mesh skins[k].primMesh with jointCount matrices; its vertex v has the influence row influences[firstInfluence + v] (vertexCount rows).  The call captures the rest
 *   pose — the context's current rows of those meshes — into a device buffer of its own and allocates a staging range of the same size for the posed rows.
 *   RT_ERR_INVALID_ARG, nothing changed, for: a prim mesh out of range or listed twice; jointCount == 0 or > 65536; an influence range that lies outside the array
 *   (it is vertexCount rows long); a joint index >= jointCount; a non-finite weight; a mesh whose material is emissive by the scene's light rule (luminance of
 *   emissiveFactor > 1e-2) while no light-source binding is set: its triangle-light records hold world positions the host could no longer supply.  With
 *   rt_set_light_sources the context rewrites those records itself and the mesh is accepted; without it host-deformed emitters go through rt_update_vertices +
 *   rt_update_lights.  rt_upload_scene drops the skins; rt_build_accel and rt_rebuild_accel keep them.
 * rt_update_skins(ctx, count, skinIds, jointMatrices): re-poses the listed skins from the rest pose on the GPU.  jointMatrices = for every listed skin, in the
 *   order listed, jointCount x 12 floats (3 x 4 row-major, the layout of rt_instance::objectToWorld), concatenated.  Valid after rt_build_accel.  No skins set, an id
 *   out of range or listed twice, a non-finite matrix entry, or a pose that yields a non-finite position refuses the WHOLE call with RT_ERR_INVALID_ARG: the kernel
 *   writes the staging range and counts such positions, and the staged rows are copied to the live vertex array only when the count is zero.
 *   The arithmetic, fp32, no contraction (include/rt_detmath.h), for a vertex with rest row (p, normal, texcoord, tangent, colour) and influence (j_k, w_k), k = 0..3:
 *     B[e] = ((w0 M[j0][e] + w1 M[j1][e]) + w2 M[j2][e]) + w3 M[j3][e] for each of the 12 entries e; a zero weight is not skipped;
 *     position' = ((B[r][0] x + B[r][1] y) + B[r][2] z) + B[r][3] per row r (xformPointRaw);
 *     with a b c / d e f / g h i the rows of B's 3 x 3 part, the cofactors  c00 = e i - f h, c01 = f g - d i, c02 = d h - e g, c10 = c h - b i, c11 = a i - c g,
 *     c12 = b g - a h, c20 = b f - c e, c21 = c d - a f, c22 = a e - b d, det = (a c00 + b c01) + c c02, s = -1 when det < 0, else +1, n = decompress_unit_vec(normal),
 *     m[r] = s ((c[r][0] n.x + c[r][1] n.y) + c[r][2] n.z)   (the inverse transpose without its division, turned outwards again under a mirroring blend);
 *     u[r] = (B[r][0] t.x + B[r][1] t.y) + B[r][2] t.z with t = decompress_unit_vec(tangent);
 *     for v = m or u: d = (v.x v.x + v.y v.y) + v.z v.z, q = 1 / sqrt(d), packed' = compress_unit_vec(v q) — but the rest row's packed value is kept when d is not
 *     > 0, d is infinite or q is infinite, and a packed value of 0xffffffff (the codec's sentinel) stays as it is.  texcoord (with the handedness bit) and colour are copied.
 * All three: like rt_update_instances v1 they join the frames in flight, run on the context's main stream and return after their kernels completed; they reset the
 *   reference-mode sums (n -> 0); they leave the SVGF / TAA histories, the object-motion state and the stream-priority decision alone (a deformation is not instance
 *   motion: an instance's previous matrix stays its current one, and the histories' G-buffer tests reject a surface that changed under a pixel); they free nothing.
 *   rt_update_vertices and rt_update_skins refit like rt_update_instances — v0 / e1 / e2 and TRI_FLIP of every leaf record of every instance of the deformed meshes,
 *   the boxes above them, the hit rule's pad (which equals a fresh build's: a reduction over the INDEXED vertices, so a vertex no triangle references does not
 *   move it), a full refit when the pad grows — and rt_get_refit_stats afterwards describes that refit (instances = the instances refitted).
 *   Host copy: rt_update_skins moves no vertex across the bus; the context's own copy of a skinned mesh is refreshed from the device by the calls that read it
 *   (rt_build_accel, rt_rebuild_accel's first use, rt_update_instances of an instance of that mesh, rt_set_skins).
 *   Scope: the single-GPU context only.  rt_mgpu_* contexts and the row-tiled hosts (restir_amd/tiled.py) have no deformation path: they upload the deformed scene.
 * rt_vertices_readback(ctx, firstVertex, count, dst): rows [firstVertex, firstVertex + count) of the device vertex array (indices into rt_scene_desc::vertices) as
 *   they are now, for tests and diagnostics.  Valid after rt_upload_scene; a range outside the array is RT_ERR_INVALID_ARG.  Synchronous.
 * rt_get_deform_stats: what the last rt_update_vertices / rt_update_skins that succeeded did.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t primMesh, firstJoint, jointCount, firstInfluence; } rt_skin;   /* one per skinned prim mesh; firstJoint is the host's own bookkeeping (its joint palette) and is not read */
typedef struct { uint16_t joint[4]; float weight[4]; } rt_skin_influence;                /* 24 B per vertex; joint < the skin's jointCount */
typedef struct {
  uint32_t meshes;            /* prim meshes deformed by the call */
  uint32_t vertices;          /* vertices written */
  uint32_t instances;         /* instances refitted */
  uint32_t vertexBytesCopied; /* vertex bytes the call moved between host and device, either way (0 for rt_update_skins) */
  float    skinMs;            /* HIP-event time of the skinning kernel and the commit copy (0 for rt_update_vertices) */
  float    ms;                /* HIP-event time of the whole call on the main stream */
  uint32_t reserved[2];
} rt_deform_stats;            /* 32 B */
int rt_update_vertices(rt_ctx* ctx, uint32_t primMesh, uint32_t firstVertex, uint32_t count, const rt_vertex* rows);
int rt_set_skins(rt_ctx* ctx, uint32_t numSkins, const rt_skin* skins, uint64_t numInfluences, const rt_skin_influence* influences);
int rt_update_skins(rt_ctx* ctx, uint32_t count, const uint32_t* skinIds, const float* jointMatrices);
int rt_vertices_readback(rt_ctx* ctx, uint64_t firstVertex, uint64_t count, rt_vertex* dst);
int rt_get_deform_stats(rt_ctx* ctx, rt_deform_stats* out);
/* ------------------------------------------------------------------------------------------------------------------
 * Light sources (added within ABI 2.4, no version bump; csrc/light_records.hip).  A triangle-light record (rt_trig_light) holds WORLD positions
 * v0 v1 v2, and the context does not know which triangle a record came from: rt_update_instances on an emissive instance moves the surface and leaves its light
 * where it was until the host recomputes every record and calls rt_update_lights, and rt_set_skins refuses an emissive mesh.  A BINDING tells the context the
 * source of every record; the update calls then rewrite the records of the instances they refit on the GPU, in the same refit tail, with no bus traffic.
 * Only the 36 bytes v0 v1 v2 of a record depend on the matrix or the positions: the light pick is weighted by luminance(emissiveFactor), not by area, so impSamp
 * (the alias table) and lightInfo.trigSampProb never change under motion or deformation, and texcoords keep their bits under rt_update_vertices and skinning.
 *
 * rt_set_light_sources(ctx, numTrig, sources): sources[k] = {instance, triangle}: trigLights[k] is triangle `triangle` (position in the index list / 3, relative
 *   to the prim mesh) of instance `instance`.  Valid after rt_upload_scene (RT_ERR_NO_SCENE otherwise), before or after rt_build_accel.  numTrig == 0 removes the
 *   binding.  Otherwise RT_ERR_INVALID_ARG, nothing changed, for: numTrig != the uploaded trigLightSize; NULL sources; an instance index out of range; a
 *   triangle >= indexCount / 3 of the instance's prim mesh; a record whose matIndex differs from that prim mesh's materialIndex; and a binding that does not
 *   describe the records: the call evaluates the update kernel for ALL records into a scratch array and compares v0 v1 v2 with the device records bit for bit, and
 *   the message names the first record that differs.  So switching the binding on never changes a bit of a consistent scene; a host whose records went stale (it
 *   moved an emitter without rt_update_lights) calls rt_update_lights first.  Records may be listed in any order, the records of one instance need not be
 *   contiguous, and two records may name the same triangle.  Removing the binding while a skin on an emissive mesh exists is RT_ERR_INVALID_ARG.
 *   Drains the pipeline; does not reset the reference-mode sums (no byte of the scene changes).
 * With a binding set, rt_update_instances, rt_update_vertices and rt_update_skins rewrite v0 v1 v2 of every bound record whose instance they refit:
 *   v_k = ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3] per row r of the instance's objectToWorld (xformPointRaw; fp32, no contraction) with (x, y, z) the
 *   position of vertex indices[firstIndex + 3 triangle + k] + vertexOffset — the expression of the leaf records and of the host Scene's createTrigLightBuffer.
 *   matIndex, transformIndex, uv0..uv2, impSamp and pad keep their bytes; records of other instances keep all 96 bytes; trigSampProb is untouched.  The kernel runs
 *   on the main stream after the instance rows and the vertex commit are in place; a refused update (a pose with a non-finite position included) writes no record.
 *   rt_set_skins accepts an emissive mesh while a binding is set (without one it refuses as before).  rt_update_lights still works and leaves the binding in
 *   place; punctual lights stay the host's business.  rt_build_accel and rt_rebuild_accel keep the binding, rt_upload_scene drops it (as it drops skins),
 *   rt_resize does not touch it.  Without a binding no call launches the kernel: the default path is unchanged.
 *   A reused reservoir's light sample is one frame stale on a moving emitter: ReSTIR's own lag.
 *   Scope: the single-GPU context only.  rt_mgpu_* contexts, rt_run_stage hosts and restir_amd/tiled.py are unchanged: they upload the moved scene.
 * rt_lights_readback(ctx, which, dst, bytes): the device light arrays as they are now: RT_LIGHTS_TRIG (96 B per record) or RT_LIGHTS_PUNC (80 B per record).
 *   Valid after rt_upload_scene; `bytes` must be the exact size (RT_ERR_INVALID_ARG otherwise).  Synchronous.
 * rt_get_light_stats: the binding, and what the last update call did to the light records (rt_update_lights: rewritten = 0, lightBytesCopied = the bytes uploaded).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t instance, triangle; } rt_light_source;   /* 8 B */
typedef struct {
  uint32_t bound;            /* records that have a source (0: no binding) */
  uint32_t rewritten;        /* records whose v0 v1 v2 the last update call rewrote */
  uint32_t lightBytesCopied; /* light bytes the last update call moved across the bus (0 on the device path) */
  float    ms;               /* HIP-event time of the light kernel in that call */
  uint32_t reserved[4];
} rt_light_stats;            /* 32 B */
enum { RT_LIGHTS_TRIG = 0, RT_LIGHTS_PUNC = 1 };
int rt_set_light_sources(rt_ctx* ctx, uint32_t numTrig, const rt_light_source* sources);
int rt_lights_readback(rt_ctx* ctx, int which, void* dst, size_t bytes);
int rt_get_light_stats(rt_ctx* ctx, rt_light_stats* out);
/* ------------------------------------------------------------------------------------------------------------------
 * Emitters (added within ABI 2.4, no version bump; csrc/light_derive.hip).  rt_set_instances refuses an emissive instance that is added, removed or
 * re-indexed (the emitter rule above), because the number of triangle-light records is fixed by rt_upload_scene: a lamp can be switched on only by a new scene.
 * In the EMITTER MODE (opt-in, default off) the context DERIVES the triangle-light records from the instance table, so rt_set_instances may add and remove
 * emitters.  With the mode off every call behaves exactly as without this section, the emitter rule and its messages included.
 * Why the host hands over templates: a record's uv0..uv2 are the RAW texcoords of its vertices, while the device vertex rows carry the tangent's handedness in the
 * LSB of texcoord.y; the raw bit is not on the device.  So the host hands the raw texcoords over once per emissive prim mesh: the TEMPLATE of the mesh, a list of
 * rows {triangle, uv0, uv1, uv2}, in the sense of the alpha templates of rt_set_instances.
 *
 * The derived list of an instance table: walk the instances in index order; for every instance whose prim mesh has a template, emit the template's rows in
 *   template order.  (The host Scene's createTrigLightBuffer order when the template lists the triangles ascending; the host owns the loop bound of that function.)
 *   The record of (instance i, row r): matIndex = the prim mesh's materialIndex; transformIndex = 0xffffffff; v_k = xformPointRaw(objectToWorld_i,
 *   position[indices[firstIndex + 3 r.triangle + k] + vertexOffset]), the expression of "Light sources" above (fp32, no contraction); uv0 uv1 uv2 = r.uv; pad = 0;
 *   impSamp from the alias table of the list.  The binding entry of the record is {i, r.triangle}.
 *   Alias table: made on the CPU inside the library (Vose's construction is sequential and its weights do not depend on geometry): the weight of a record is
 *   luminance(emissiveFactor) of its material, `total` is the fp32 sum of the weights in record order, the table is the host Scene's construction
 *   (host/alias_table.hpp, the same code), impSamp = {failId, prob, w / total, w[failId] / total}.  lightInfo.trigLightSize = the length of the list;
 *   lightInfo.trigSampProb = total / (total + puncLightWeight) when the list or the punctual lights are not empty, and keeps its value otherwise.
 *
 * rt_set_emitter_meshes(ctx, numMeshes, meshes, numRows, rows, puncLightWeight), numMeshes > 0: switches the mode on (or replaces the templates while it is on).
 *   meshes[m] = {primMesh, firstRow, rowCount, reserved}: the template of primMesh is rows[firstRow .. firstRow + rowCount); puncLightWeight: the summed weight of
 *   the punctual lights (the host Scene's m_puncLightWeight; 0 without punctual lights).  Valid after rt_build_accel (RT_ERR_NO_SCENE / RT_ERR_NO_ACCEL otherwise).
 *   The call derives ALL records of the CURRENT instance table into scratch memory with the kernel every later call uses and compares all 96 bytes of every
 *   record, the count and trigSampProb with the device's: a difference refuses the call and rt_last_error names the first differing record.  So switching the mode
 *   on never changes a bit of a consistent scene; a host whose records went stale calls rt_update_lights first.  On success the derived (instance, triangle) list
 *   becomes the light-source binding (rt_get_light_stats.bound = the count; a binding set before is replaced): rt_update_instances, rt_update_vertices,
 *   rt_update_skins and rt_update_morphs move the records of emitters, spawned ones included, through the refit tail of "Light sources".
 *   Refusals (RT_ERR_INVALID_ARG, nothing changed): NULL meshes, or NULL rows with numRows > 0; a prim mesh out of range or listed twice; a prim mesh that is not
 *   emissive by the scene's light rule (luminance of its material's emissiveFactor > 1e-2) or that has no material; an emissive prim mesh that has an instance
 *   but no template; a row range outside rows; a row whose triangle is >= indexCount / 3 of its mesh; a non-finite uv; a non-finite or negative
 *   puncLightWeight; derived records that differ from the device's.
 * rt_set_emitter_meshes(ctx, 0, NULL, 0, NULL, any): switches the mode off.  Records, binding and lightInfo stay as they are; the emitter rule applies again.
 * rt_set_instances while the mode is on: the emitter rule is replaced by "every emissive prim mesh the new table uses has a template" (RT_ERR_INVALID_ARG, the
 *   message names the first instance without one).  The call derives the records, the binding, the alias table and lightInfo of the new table; a list of zero
 *   records is valid, and so is going from zero records back to some.  Records and binding are written to spare buffers by k_light_expand on the main stream,
 *   after the new instance rows are in place, and swapped together with lightInfo and the tree on success: every failure of rt_set_instances leaves the previous
 *   lights in place.  There are two sets of light buffers; the one a call writes is allocated with 1/8 slack over its record and emitting-instance counts when it
 *   is absent or too small (rt_emitter_stats.reallocated = 1).
 *   Bus traffic beyond rt_set_instances' own: records * 16 + (2 * emittingInstances + 1) * 4 bytes: the alias entries, one prefix word per emitting instance plus
 *   one, and one instance id per emitting instance.  No vertex, texcoord or position crosses the bus.
 * Other calls while the mode is on: rt_set_light_sources is refused (RT_ERR_INVALID_ARG: the binding is derived).  rt_update_lights works with the CURRENT counts
 *   (the next rt_set_instances derives the records anew; a changed punctual weight is handed over by rt_set_emitter_meshes).  rt_set_skins and rt_set_morph_targets
 *   accept an emissive mesh, as with a binding.  rt_upload_scene drops the mode and the templates; rt_build_accel, rt_rebuild_accel and rt_resize keep them.  The
 *   reference-mode sums reset as rt_set_instances resets them.  Direct-light reservoirs hold Li / wi / dist of their sample, not a light index, so no history plane
 *   names a record: a lamp that was removed fades through ReSTIR's own lag, one frame with the temporal pass.
 *   Scope: the single-GPU context only.  rt_mgpu_* contexts, rt_run_stage hosts and restir_amd/tiled.py are unchanged.  Punctual lights stay the host's business.
 * rt_get_emitter_stats: the mode, and what the last rt_set_emitter_meshes / rt_set_instances that succeeded with the mode on did to the lights.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t primMesh, firstRow, rowCount, reserved; } rt_emitter_mesh;   /* 16 B */
typedef struct { uint32_t triangle; float uv[6]; uint32_t pad; } rt_emitter_row;       /* 32 B: uv0 uv1 uv2 */
typedef struct {
  uint32_t enabled;            /* 1: the emitter mode is on */
  uint32_t records;            /* triangle-light records after the call */
  uint32_t emittingInstances;  /* instances of the table whose prim mesh has a template */
  uint32_t bytesUploaded;      /* light bytes the call moved host -> device (switching on: the templates, 32 B per row + 4 B per prim mesh, and the formula above) */
  uint32_t reallocated;        /* 1: the light buffers the call wrote were absent or too small and were allocated */
  float    expandMs;           /* HIP-event time of k_light_expand in that call */
  uint32_t reserved[2];
} rt_emitter_stats;            /* 32 B */
int rt_set_emitter_meshes(rt_ctx* ctx, uint32_t numMeshes, const rt_emitter_mesh* meshes, uint32_t numRows, const rt_emitter_row* rows, float puncLightWeight);
int rt_get_emitter_stats(rt_ctx* ctx, rt_emitter_stats* out);
/* ------------------------------------------------------------------------------------------------------------------
 * Morph targets (added within ABI 2.4, no version bump; csrc/morph.hip).  glTF's second deformation mechanism (blend shapes: faces, correctives,
 * cloth presets) on the GPU: a prim mesh has a SET of targets, a target is a plane of position deltas (plus, optionally, a plane of normal deltas and one of
 * tangent deltas), and a pose is one weight per target.  rt_set_morph_targets uploads the deltas once; rt_update_morphs takes weights, re-poses the meshes from
 * their rest pose on the device and refits like rt_update_skins.  A mesh may be morphed AND skinned (a character): morph, then skin.
 *
 * Delta layout, target-major: with P = 1 + (planes & RT_MORPH_NORMALS ? 1 : 0) + (planes & RT_MORPH_TANGENTS ? 1 : 0) and V = the prim mesh's vertexCount, target
 *   t of set k occupies rows [firstDelta + t P V, firstDelta + (t + 1) P V) of `deltas`: the position plane (V rows, row v belongs to vertex v), then the normal
 *   plane if present, then the tangent plane if present.  A row is 16 bytes; `pad` is not read as a value.
 * rt_set_morph_targets(ctx, numSets, sets, numDeltas, deltas): valid after rt_upload_scene (RT_ERR_NO_SCENE otherwise).  Replaces all sets (numSets == 0 removes
 *   them); every set starts with all weights zero.  RT_ERR_INVALID_ARG, nothing changed, for: a prim mesh out of range or listed twice; targetCount == 0 or
 *   > 4096; unknown `planes` bits; a delta range (targetCount P V rows from firstDelta) outside the array; a non-finite d[]; a mesh whose material is emissive by
 *   the scene's light rule while no light-source binding is set (the rule and the message of rt_set_skins).
 *   Rest pose: a mesh that has a skin uses the skin's rest pose and staging range; for any other mesh the call captures the context's current rows, as
 *   rt_set_skins does, into a pool of its own with a staging range of the same size.  Order: skins first.  rt_set_skins while any morph set exists is
 *   RT_ERR_INVALID_ARG (remove the sets, set the skins, set the sets again).  rt_update_vertices on a mesh that has a morph set is RT_ERR_INVALID_ARG, as it is for
 *   a skin.  rt_set_light_sources(numTrig == 0) while a morph set on an emissive mesh exists is RT_ERR_INVALID_ARG, like a skin.  rt_upload_scene drops the sets;
 *   rt_build_accel, rt_rebuild_accel and rt_resize keep them (and their weights).
 * rt_update_morphs(ctx, count, setIds, weights): weights = for every listed set, in the order listed, targetCount floats, concatenated.  Valid after
 *   rt_build_accel.  RT_ERR_INVALID_ARG for: no sets; an id out of range or listed twice; a non-finite weight; a set whose mesh has a skin that no successful
 *   rt_update_skins has listed yet ("pose the skin first"); a pose that yields a non-finite position (the staged-then-commit rule and the counter of
 *   rt_update_skins).  A refused call leaves the stored weights, the vertices, the tree, the light records and the stats as they were.  Otherwise the call stores
 *   the weights in the context and re-poses every listed mesh from its rest pose.
 *   Morph then skin: when the mesh also has a skin, the morphed rows are the skin's input, with the joint matrices of the last successful rt_update_skins that
 *   listed that skin (the context keeps them per skin).  Conversely rt_update_skins on a mesh that has a morph set applies the stored weights first; with all
 *   stored weights zero (or -0) it runs exactly the path it runs without morph sets and produces the same bits.
 *   The arithmetic, fp32, no contraction, in the order written, for a vertex with rest row (p, normal, texcoord, tangent, colour): the ACTIVE targets of a set are
 *   those whose weight is not zero (w != 0.0f, so -0 is inactive), in ascending target index a < b < ...; inactive targets are skipped, not multiplied by zero
 *   (-0 + 0 d would differ), and the kernel never sees them: the host builds the active list.
 *     p' = (((p + w_a dP_a) + w_b dP_b) + ...) per component, each product rounded before its add;
 *     with the normal plane and normal != 0xffffffff: n = decompress_unit_vec(normal), m = ((n + w_a dN_a) + ...), then the rule of rt_update_skins:
 *     d = (m.x m.x + m.y m.y) + m.z m.z, q = 1 / sqrt(d), packed' = compress_unit_vec(m q), but the rest value is kept when d is not > 0, d is infinite or q is
 *     infinite.  Without the plane, with the sentinel, or when the set has NO active target the packed value is copied: no decode / encode round trip.
 *     The tangent follows the same rules with its plane.  texcoord (with the handedness bit) and colour are copied.
 *   A set with no active target yields the rest row bit for bit.
 *   Everything else — joining the frames in flight, the reference-mode reset, the histories, the object-motion state, the refit, the pad, the light records
 *   (with a binding) and the host-copy refresh — follows the "All three:" paragraph of "Deforming meshes".  No vertex crosses the bus: rt_get_deform_stats
 *   afterwards describes the call like an rt_update_skins (vertexBytesCopied = 0; skinMs = the morph kernel, the skinning kernel and the commit copy).
 *   Scope: the single-GPU context only, like skins.
 * rt_get_morph_stats: what the last rt_update_morphs that succeeded did.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t primMesh, targetCount, firstDelta, planes; } rt_morph_set;   /* 16 B; planes: bit 0 = normal deltas, bit 1 = tangent deltas */
typedef struct { float d[3]; float pad; } rt_morph_delta;                              /* 16 B; pad is not read as a value */
typedef struct {
  uint32_t sets;             /* sets the call listed */
  uint32_t vertices;         /* vertices posed */
  uint32_t targetsApplied;   /* active targets (weight != 0) over the listed sets */
  uint32_t instances;        /* instances refitted */
  float    morphMs;          /* HIP-event time of the morph kernel */
  float    ms;               /* HIP-event time of the whole call on the main stream */
  uint32_t reserved[2];
} rt_morph_stats;            /* 32 B */
enum { RT_MORPH_NORMALS = 1, RT_MORPH_TANGENTS = 2 };
int rt_set_morph_targets(rt_ctx* ctx, uint32_t numSets, const rt_morph_set* sets, uint64_t numDeltas, const rt_morph_delta* deltas);
int rt_update_morphs(rt_ctx* ctx, uint32_t count, const uint32_t* setIds, const float* weights);
int rt_get_morph_stats(rt_ctx* ctx, rt_morph_stats* out);
/* ------------------------------------------------------------------------------------------------------------------
 * Editing materials and textures (added within ABI 2.4, no version bump; csrc/materials.hip, csrc/opacity_map.h).  The plain fields of a material
 * row are an 80-byte copy; what a new scene was needed for is the state DERIVED from a material's alpha parameters (pbrBaseColorFactor.w, alphaCutoff, alphaMode,
 * pbrBaseColorTexture) and from the alpha channel of its base colour texture: one 64-byte alpha record per triangle that takes the alpha test, its copy in the
 * latency build's per-record array, and one 8x8 opacity micro-map per such triangle (in the leaf records, in the device builder's table and in the templates of
 * rt_set_instances).  The two calls below re-derive that state on the GPU for the triangles of the DIRTY materials, and for nothing else: a material is dirty when
 * one of the four fields above changed bitwise, or when an alpha byte of its base colour texture changed.  If no material is dirty no kernel is launched.
 * After either call the device material rows, the context's copy of them, the alpha records, the per-record copies, every affected micro-map and the templates
 * hold the words that rt_upload_scene + rt_build_accel of the edited description would give (after rt_set_instances: in the per-mesh alphaIdx numbering of that
 * section; a template of a mesh that has no alpha-tested instance in the current table is dropped and made again from the edited tables when a table needs it).
 * The micro-map rule is stated once, in csrc/opacity_map.h; rt_opacity_map evaluates it on the host.  Two clarifications of the rule came with that header: a cell
 * with a non-finite corner texcoord, or a corner beyond 2^31 - 4096 texels in magnitude, is "unknown" (state 0), where the scan used to convert the value to an
 * integer that cannot hold it.
 *
 * rt_update_materials(ctx, count, materialIds, materials): materials[k] replaces row materialIds[k].  Valid after rt_upload_scene (RT_ERR_NO_SCENE otherwise);
 *   before rt_build_accel it is a row copy into the context's and the device's tables.  The whole call is checked before anything changes; it joins the frames in
 *   flight, as rt_update_instances does.  RT_ERR_INVALID_ARG, nothing changed, rt_last_error names the first offender: NULL arrays with count > 0; an id out of
 *   range; an id listed twice; a row that fails the checks rt_upload_scene applies to a material row (a texture id outside the scene's textures); a row that moves
 *   the material across the scene's light rule (luminance of emissiveFactor > 1e-2) in either direction: the emissive meshes are fixed by the scene, as for
 *   rt_set_skins; while the emitter mode is on, a row that changes the luminance of emissiveFactor of an emissive material (the derived alias table would go
 *   stale; a stated scope limit).  With the emitter mode off, light records stay the host's business, as at upload: a host that changed an emission follows with
 *   rt_update_lights.  A HIP error after the checks (RT_ERR_HIP) may leave the call partly applied, as for the other update calls: upload the scene again.
 * rt_update_texture(ctx, texture, x, y, w, h, bgra, rowPitchBytes): replaces the w x h texels at (x, y) of one texture, same size, same sampler; row r of the
 *   rectangle starts at bgra + r rowPitchBytes.  RT_ERR_INVALID_ARG, nothing changed: a texture outside the scene's textures; an empty rectangle or one that
 *   leaves the texture; rowPitchBytes < 4 w; NULL data.  Updates the device texels, the context's alpha plane and the plane's hash.  When an alpha byte inside the
 *   rectangle differs, every material whose pbrBaseColorTexture is this texture is dirty; a texture used only as an emissive, normal or roughness texture, or an
 *   edit that leaves every alpha byte as it was, launches nothing.
 * Both: settled primary visibility is dropped; the reference-mode sums reset; NO history is invalidated: the material hash of the G-buffer and
 *   ReSTIR's own lag apply, as for rt_update_lights.  The next rt_build_accel sees the edit in its cache key: a cached host build of the old scene is not reused.
 *   Every other call that edits a loaded scene commutes with the edits, in either order and any interleaving: rt_update_instances, rt_rebuild_accel (under either
 *   builder of rt_set_rebuild_options), rt_build_accel, rt_set_instances (with and without the emitter mode), rt_update_vertices, rt_update_skins, rt_update_morphs,
 *   rt_set_skins / rt_set_morph_targets (an edit may name the material of a mesh that has a skin or a morph set), rt_set_light_sources and rt_update_lights —
 *   the state afterwards is that of rt_upload_scene + rt_build_accel of the description with all of them applied (tests/test_gpu_scene_edits.py).
 *   Scope: the single-GPU context only; rt_mgpu_* contexts, rt_run_stage hosts and restir_amd/tiled.py are unchanged.  Not covered: texture resizes, sampler changes, the emitter mode's re-derivation.
 * rt_get_material_stats: what the last of the two calls that succeeded did.
 * rt_opacity_map(desc, bgra, omm): no context, no GPU.  The four micro-map words of one triangle: uv = uv0 uv1 uv2, bgra = the w x h BGRA8 texels of the base
 *   colour texture or NULL for none (w, h and the wrap modes are then not read).  RT_ERR_INVALID_ARG for NULL desc / omm or a texture with w <= 0 or h <= 0.
 * rt_accel_readback(RT_ACCEL_ALPHA): the alpha records, 64 B each (record 0 is the all-zero record of opaque triangles; the count is 1 + the alpha-tested
 *   triangles of a host tree, 1 + the triangles of all prim meshes once rt_set_instances has run); the 8 bytes of the texel address are replaced by the texture's
 *   index as uint64, all ones for none, so that two contexts compare equal.  `bytes` may also be a smaller multiple of 64: the first bytes / 64 records.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
  float uv[6];
  float baseAlpha, cutoff;
  int32_t alphaMode, w, h, wrapS, wrapT, filter;
  uint32_t reserved[2];
} rt_opacity_map_desc;         /* 64 B */
typedef struct {
  uint32_t materialsWritten;   /* rows the call copied (rt_update_texture: 0) */
  uint32_t dirtyMaterials;     /* materials whose alpha records had to be re-derived */
  uint32_t alphaRecords;       /* alpha records rebuilt (one micro-map each) */
  uint32_t leafRecords;        /* leaf records rewritten */
  uint64_t texelsScanned;      /* texels the build kernel read */
  uint32_t bytesUploaded;      /* host -> device: material rows or texels, plus the dirty words */
  float    ms;                 /* HIP-event time of the device work (copies and kernels) */
} rt_material_stats;           /* 32 B */
int rt_update_materials(rt_ctx* ctx, uint32_t count, const uint32_t* materialIds, const rt_material* materials);
int rt_update_texture(rt_ctx* ctx, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* bgra, size_t rowPitchBytes);
int rt_get_material_stats(rt_ctx* ctx, rt_material_stats* out);
int rt_opacity_map(const rt_opacity_map_desc* d, const uint8_t* bgra, uint32_t omm[4]);
/* ------------------------------------------------------------------------------------------------------------------
 * The environment (added within ABI 2.4, no version bump; csrc/env_accel.hip, csrc/env_accel.h).  The RGBA32F lat-long map and its importance table
 * (one rt_impt_samp {alias, q, pdf, aliasPdf} per texel) used to enter through rt_upload_scene alone.  rt_set_environment replaces both without a new scene, and
 * with accel == NULL it builds the table on the GPU by the rule csrc/env_accel.h states once for host and device: importance = row area x max(r, g, b) in fp32
 * (NaN and negative texels count 0), quantised against the maximum to integers below 2^40, so that every sum is an integer sum and the table is the same bits
 * whatever adds them up, in whatever order; an exact alias table from two 128-bit prefix sums (deficits of the below-average texels, excesses of the others, both
 * in index order) and two binary searches, q a multiple of 2^-24 taken between two rounded marks of those sums, so that the probability of every texel is within
 * 2^-24 / n of its share whatever the number of texels that alias to it; pdf = max(r, g, b) / integral.  rt_env_accel is the same rule on the host, word for word.  The table is NOT
 * HdrSampling::createEnvironmentAccel's (a float sum and a sequential sweep whose result depends on the order); both are proper alias tables of the same
 * importances, and a context given either renders what the oracle renders from that table.
 *
 * rt_set_environment(ctx, width, height, rgba32f, accel): valid after rt_upload_scene (RT_ERR_NO_SCENE otherwise).  width == 0, height == 0 or rgba32f == NULL:
 *   the 1 x 1 black map of rt_upload_scene (accel is then not read).  accel != NULL: the table is checked as rt_upload_scene checks it (every alias inside the
 *   table), then map and table are copied.  accel == NULL: the table is built on the device; width x height <= 2^23 (the rule's integer range).  The size may
 *   differ from the current map's.  RT_ERR_INVALID_ARG, nothing changed, rt_last_error says why: a negative size; more than 2^23 texels with accel == NULL; an
 *   alias outside the table; a texel with +inf in r, g or b, or finite texels whose importance or luminance overflows fp32 to +inf (found on the host for the
 *   copy path, by the first kernel on the device path: the build runs in a staging pair of buffers, which replaces the pair in use only when the device's flag is
 *   clear, as rt_update_skins stages its rows).  The context keeps two pairs (map + table) and builds into the one not in use, each sized by the largest map it has
 *   held, plus the build's work arrays (28 B per texel): repeated calls at one size allocate nothing.  rt_upload_scene frees them.
 *   Every accepted call joins the frames in flight, runs on the main stream and returns after its copies and kernels have completed; resets the reference-mode
 *   sums; drops settled primary visibility (miss pixels carry the environment's radiance in the G-buffer).  It does not touch sun & sky: while rt_sun_and_sky
 *   .in_use == 1 the map is stored and not seen.  Reservoirs and the SVGF / TAA / upsampling histories are left alone, as by the other edits; so are the tree and
 *   the stream-priority decision.  The caller sets rt_state.envMapLuminIntegInv = 1 / integral (rt_get_environment_stats, or its own HdrSampling::getIntegral()
 *   on the copy path), exactly as after rt_upload_scene.  A HIP error after the checks (RT_ERR_HIP) leaves the environment in use as it was.
 * rt_environment_readback(ctx, which, dst, bytes): RT_ENV_TEXELS (16 B per texel) or RT_ENV_ACCEL (16 B per texel) of the environment in use; bytes must be
 *   width x height x 16.  Drains the context.
 * rt_get_environment_stats: the environment in use and what the last accepted rt_set_environment did.  integral, average, numSmall and numLarge are the device
 *   build's (0 after a copy-path call or before any call: the caller's HdrSampling knows its own).
 * rt_env_accel(width, height, rgba32f, out, integral, average): no context, no GPU; the rule on the host.  RT_ERR_INVALID_ARG for NULL rgba32f / out, a size
 *   below 1, more than 2^23 texels, or a texel that refuses the map (out is then untouched).  integral / average may be NULL.  rt_env_importance: step 1 of the
 *   rule alone, width x height floats (the same refusals).  Scope: the single-GPU context; rt_mgpu_* contexts and restir_amd/tiled.py upload a table of
 *   rt_env_accel's through their scene description.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { RT_ENV_TEXELS = 0, RT_ENV_ACCEL = 1 };
typedef struct {
  int32_t  width, height;      /* the environment in use */
  float    integral;           /* sum of the importances (what HdrSampling::getIntegral() is to its own table) */
  float    average;            /* mean luminance of the texels */
  uint32_t numSmall, numLarge; /* texels below / not below the average importance */
  uint32_t builtOnDevice;      /* 1: the table in use was built by the device */
  float    ms;                 /* HIP-event time of the device work of the last accepted call (copies and kernels) */
  uint64_t deviceBytes;        /* device memory the context holds for rt_set_environment (both pairs + work arrays) */
} rt_environment_stats;        /* 40 B */
int rt_set_environment(rt_ctx* ctx, int width, int height, const float* rgba32f, const rt_impt_samp* accel);
int rt_environment_readback(rt_ctx* ctx, int which, void* dst, size_t bytes);
int rt_get_environment_stats(rt_ctx* ctx, rt_environment_stats* out);
int rt_env_accel(int width, int height, const float* rgba32f, rt_impt_samp* out, float* integral, float* average);
int rt_env_importance(int width, int height, const float* rgba32f, float* out);
/* ---- Settled primary visibility -------------------------------------------------------------------------------------------------------
 * While the launch camera (viewInverse, projInverse, size: bitwise) and the scene stay what they were, full-frame direct launches of the throughput build stop
 * tracing the primary ray: the third launch at a camera (RESTIR_VIS_REST_FRAMES at-rest launches, default and minimum 2) also RECORDS per pixel the leaf record of
 * the closest deterministic accept and up to K (RESTIR_VIS_K, default RT_VIS_K_DEFAULT, at most 64) stochastic candidates in front of it; later launches REPLAY:
 * they re-test those records with the frame's seed.  Frames are bit for bit what tracing gives.  A pixel with more than K such candidates keeps tracing.  A camera
 * change, rt_resize, rt_upload_scene, rt_build_accel, rt_rebuild_accel, every rt_update_* / rt_set_skins / rt_set_morph_targets call, rt_set_stream, a row-band or
 * latency-build launch, TAA, temporal upsampling or an object-motion mode on drop the state; the rt_mgpu_* hosts never record; RESTIR_PRIMARY_REPLAY=0 switches it off.  The three
 * planes, (2 + K) x 4 B per pixel, are allocated by the first recording and freed by rt_resize / rt_destroy.
 * rt_get_primary_replay_stats: state (0 none, 1 valid), K, and in state 1 the pixel classes of the recording in force (this drains the context); launches since
 * rt_create.  A replayed query counts as a query in rt_counters.closestHitRays. */
#define RT_VIS_K_DEFAULT 32
typedef struct {
  uint32_t state;             /* 0: none, 1: valid (the next at-rest launch replays) */
  uint32_t K;                 /* list entries per pixel */
  uint32_t pixelsSettled;     /* no stochastic candidate in front of the deterministic hit: one record test per frame */
  uint32_t pixelsListed;      /* 1..K listed candidates */
  uint32_t pixelsOverflow;    /* more than K: the pixel keeps tracing */
  uint32_t launchesRecorded, launchesReplayed;
  uint32_t reserved;
} rt_primary_replay_stats;    /* 32 B */
int rt_get_primary_replay_stats(rt_ctx* ctx, rt_primary_replay_stats* out);
/* the count plane of the recording in force: W x H uint32, listed candidates per pixel (0..K), 0xffffffff = more than K (diagnostics: the histogram that chose
 * RT_VIS_K_DEFAULT, scripts/primary_replay_probe.py); RT_ERR_INVALID_ARG in state 0.  Drains the context. */
int rt_primary_replay_readback(rt_ctx* ctx, void* dst, size_t bytes);
/* Wait for all work on the ctx stream. */
int rt_sync(rt_ctx* ctx);
/* Last error message of this ctx (or of rt_create when ctx == NULL). Never NULL. */
const char* rt_last_error(rt_ctx* ctx);
/* ABI version: (major<<16)|minor.  2.4: + object motion vectors (rt_set_object_motion, rt_object_motion_camera, rt_object_motion_readback; additions), + moving instances (rt_update_instances, rt_update_lights, rt_get_refit_stats, rt_accel_readback; additions that change no existing call, so the version stays 2.4 like the three opt-in passes before them), + temporal anti-aliasing (rt_set_taa, rt_get_taa, rt_taa_reset, rt_taa_readback, rt_taa_jitter_camera), + temporal upsampling (rt_set_upscale, rt_get_upscale, rt_upscale_reset, rt_upscale_readback, rt_upscale_tonemap, rt_upscale_jitter_camera), + the GI spatial reuse (rt_set_gi_spatial, rt_get_gi_spatial, rt_gi_spatial_readback) and the denoiser selection
 * (rt_set_denoiser, rt_get_denoiser, rt_denoiser_reset, rt_denoiser_readback; opt-in additions that change no existing call, so the version stays 2.4), + rt_reference_render, rt_reference_reset, rt_reference_samples, rt_reference_readback, rt_reference_tonemap.  2.3 (round 6): + rt_get_streams, rt_get_stream_layout, rt_mgpu_get_stream_layout; the priority rule probes three frames and re-opens on resize / scene / denoise.  2.2 (round 5): + rt_set_stream_priorities, rt_get_stream_priorities.  2.1 (round 4): + rt_mgpu_get_link_stats.  2.0 (round 3): rt_set_pipeline -> rt_set_traversal; RT_STAGE_DIRECT levels 1 / 2 are rejected outside the
 * spatial modes; 1.1 would have been round 2's additions (rt_mgpu_*, rt_measure_valu_peak, the `level` halves of RT_STAGE_DIRECT). */
#define RT_ABI_VERSION_MAJOR 2u
#define RT_ABI_VERSION_MINOR 4u
uint32_t rt_abi_version(void);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(rt_scene_camera) == 336, "SceneCamera host_device.h:153-165");
static_assert(sizeof(rt_vertex) == 32, "VertexAttributes host_device.h:167-174");
static_assert(sizeof(rt_material) == 80, "GltfShadeMaterial host_device.h:183-204");
static_assert(sizeof(rt_state) == 100, "RtxState host_device.h:207-238");
static_assert(sizeof(rt_direct_reservoir) == 36, "DirectReservoir host_device.h:273-277");
static_assert(sizeof(rt_indirect_reservoir) == 76, "IndirectReservoir host_device.h:279-284");
static_assert(sizeof(rt_impt_samp) == 16, "ImptSampData host_device.h:287-293");
static_assert(sizeof(rt_punc_light) == 80, "PuncLight host_device.h:295-312");
static_assert(sizeof(rt_trig_light) == 96, "TrigLight host_device.h:314-325");
static_assert(sizeof(rt_light_buf_info) == 16, "LightBufInfo host_device.h:327-333");
static_assert(sizeof(rt_tonemapper) == 48, "Tonemapper host_device.h:336-351");
static_assert(sizeof(rt_sun_and_sky) == 96, "SunAndSky host_device.h:353-377");
static_assert(sizeof(rt_denoiser) == 32, "rt_denoiser");
static_assert(sizeof(rt_gi_spatial) == 32, "rt_gi_spatial");
static_assert(sizeof(rt_taa) == 32, "rt_taa");
static_assert(sizeof(rt_upscale) == 32, "rt_upscale");
static_assert(sizeof(rt_refit_stats) == 32, "rt_refit_stats");
static_assert(sizeof(rt_deform_stats) == 32, "rt_deform_stats");
static_assert(sizeof(rt_skin_influence) == 24, "rt_skin_influence");
static_assert(sizeof(rt_light_source) == 8, "rt_light_source");
static_assert(sizeof(rt_light_stats) == 32, "rt_light_stats");
static_assert(sizeof(rt_emitter_mesh) == 16 && sizeof(rt_emitter_row) == 32 && sizeof(rt_emitter_stats) == 32, "rt_emitter_mesh / _row / _stats");
static_assert(sizeof(rt_morph_set) == 16, "rt_morph_set");
static_assert(sizeof(rt_morph_delta) == 16, "rt_morph_delta");
static_assert(sizeof(rt_morph_stats) == 32, "rt_morph_stats");
static_assert(sizeof(rt_primary_replay_stats) == 32, "rt_primary_replay_stats");
static_assert(sizeof(rt_opacity_map_desc) == 64 && sizeof(rt_material_stats) == 32, "rt_opacity_map_desc / rt_material_stats");
static_assert(sizeof(rt_environment_stats) == 40, "rt_environment_stats");
#endif

#endif /* RT_ABI_H */

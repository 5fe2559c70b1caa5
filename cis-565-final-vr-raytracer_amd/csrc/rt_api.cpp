// rt_api.cpp — the C-ABI of include/rt_abi.h over HIP: context, HBM residency, stage launches, readback.
// Stands where the reference has Renderer / Scene / AccelStructure / HdrSampling talking to Vulkan
// (src/renderer.cpp:62-302, src/scene.cpp:453-508, src/accelstruct.cpp:55-65, src/hdr_sampling.cpp:79-95).
#include <hip/hip_runtime.h>
#include <array>
#include <atomic>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <map>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../include/rt_abi.h"
#include "../../include/rt_cpus.h"
#include "bvh8_builder.h"
#include "stages.h"
#include "primary_replay.h"
#include "parity_history.h"
#include "reference.h"
#include "svgf.h"
#include "gi_spatial.h"
#include "taa.h"
#include "upscale.h"
#include "refit.h"
#include "accel_build.h"
#include "instances.h"
#include "deform.h"
#include "morph.h"
#include "light_records.h"
#include "light_derive.h"
#include "opacity_map.h"
#include "materials.h"
#include "env_accel.h"
#include "../host/alias_table.hpp"
#include "dev_math.h"

using namespace rt;

struct rt_ctx {
  int device = 0;
  hipStream_t ownStream = nullptr, stream = nullptr;
  hipStream_t sideStream = nullptr;           // direct A-Trous runs here, concurrently with the indirect stage
  hipStream_t indStream = nullptr;            // overlap 2: the indirect stage of frame f runs here, next to direct(f+1) on `stream`
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  // overlap 2 (frames in flight): ring of per-frame dependency events — direct done / indirect done / frame done
  hipEvent_t evD[4] = {}, evI[4] = {}, evDone[4] = {};
  uint64_t seq = 0;          // frames submitted through the pipelined path since the last join
  bool inFlight = false;     // work may be pending on indStream / sideStream
  // One stream per (role, level), created on first use and kept until rt_destroy: a stream takes a hardware queue of its priority class round-robin at creation, so a
  // context that destroyed and re-created its streams while trying settings ended with its filter stream on the main stream's queue (the 5th normal-priority stream of
  // the process lands on the 1st one's queue): 3.38 -> 3.71 ms per frame, found by two back-to-back bench lines in round 5.
  hipStream_t indStreams[3] = {nullptr, nullptr, nullptr}, sideStreams[3] = {nullptr, nullptr, nullptr};   // index = level + 1
  int prio[3] = {0, 1, 0};   // priority level of the main / indirect / filter stream (-1 low, 0 normal, +1 high): prioSpec() at rt_create, rt_set_stream_priorities, the rule
  bool prioFromEnv = false;  // RESTIR_PRIO was set (A/B scripts stay in control)
  bool prioExplicit = false; // rt_set_stream_priorities was called: the rule stays out of it, also after rt_resize / a new scene
  bool prioDecided = false;  // the levels are final (environment, rt_set_stream_priorities, or the rule applied to the probe frames' stage times)
  float filterShare = -1.f;  // filters / (direct + indirect) of the LAST probe frame, stages run alone (the rule's input); -1: not measured
  int probeFrames = 0;       // probe frames rendered so far for the pending decision (PRIO_PROBE_FRAMES of them: warm caches, warm history)
  int denoiseSeen = -1;      // RtxState.denoise of the frames the decision was taken on: a toggle re-opens it (without the filters the share is compose alone)
  int mainIdx = -1, indIdx[3] = {-1, -1, -1}, sideIdx[3] = {-1, -1, -1};   // creation index (process-wide, g_streamsCreated) of every stream above: rt_get_stream_layout
  void* dSky = nullptr;      // SkyPre (csrc/sky.h), valid while sunAndSky.in_use == 1
  void* dPick = nullptr;     // rt_pick_result written by k_pick
  rt_sun_and_sky sunAndSky{};
  // The ring of frames in flight: per rotated kind, the buffers that wait beside the live one (ringLive), next one first.  Overlap 2 swaps the live G-buffer and
  // motion buffer with their first spare (third G-buffer / second motion buffer, rotated per pipelined frame); overlap 3 (three frames in flight) shifts through
  // both spares and also rotates the noisy / filtered direct image, which has one spare — direct(f) then only waits for frame f-3 (rt_render_frame).  The
  // instance and delta images of rt_set_object_motion rotate with the motion buffer.
  enum Ring { RING_G, RING_MOTION, RING_DIRECT, RING_INST, RING_DELTA, RING_KINDS };
  void* spare[RING_KINDS][2] = {};
  // The noisy indirect colour (RT_BUF_DENOISE_IND_A: written by the indirect stage, read and rewritten by its five filter levels) exists twice, by frame parity:
  // indirect(f+1) must not wait for the filters of frame f (round 3: that wait made a rank's period indirect + filters instead of max(direct, indirect)).
  // The boundary id names the buffer of the frame most recently passed to rt_render_frame / rt_run_stage / rt_select_frame.
  void* indA[2] = {nullptr, nullptr};
  int overlap = 2;           // 0 = one stream; 1 = direct A-Trous beside the indirect stage; 2 = 1 + consecutive frames overlap; 3 = 2 with a third frame in flight
  std::string err;
  // host copy of the scene (rt_build_accel runs after rt_upload_scene returns; the caller keeps ownership of its arrays)
  std::vector<rt_prim_mesh> primMeshes; std::vector<rt_vertex> vertices; std::vector<uint32_t> indices; std::vector<rt_instance> instances;
  std::vector<rt_material> materials; std::vector<DevTexture> devTextures;
  std::vector<std::vector<uint8_t>> hostAlpha;  // alpha channel of every texture (opacity micro-map build)
  std::vector<std::array<uint64_t, 2>> alphaHash;   // ... and its hash (rt_build_accel's cache key)
  // device allocations of the scene
  std::vector<void*> sceneAllocs, accelAllocs, ovfAllocs;
  DevScene ds{};
  bool haveScene = false, haveAccel = false;
  int maxDepth = 0; size_t numNodes = 0, numTris = 0, numRefs = 0, spatialSplits = 0;
  double sahNodeSteps = 0, sahTriSteps = 0;
  // screen-space buffers
  int W = 0, H = 0;
  void* bufs[RT_BUF_COUNT] = {};
  size_t bufBytes[RT_BUF_COUNT] = {};   // logical bytes (W x H elements): readback / upload size
  size_t bufAlloc[RT_BUF_COUNT] = {};   // allocated bytes: + RT_PAD_ROWS rows so equal-height row bands can be all-gathered in place
  rt_scene_camera cam{};
  // internal per-frame scratch (DevFrame)
  std::vector<void*> scratchAllocs;
  DevFrame scratch{};
  int histRow0 = 0, histRow1 = 1 << 30;  // rt_set_history_rows
  int traversal = RT_TRAVERSAL_AUTO;     // rt_set_traversal: which build of the traced kernels a launch gets
  bool counting = false;
  unsigned long long* dCounters = nullptr;
  // Settled primary visibility (primary_replay.h).  `replay` is all the trust there is: the planes of `vis` (allocated by the first recording, freed by
  // rt_resize / rt_destroy) are read only by a launch for which primaryReplayStep said REPLAY.
  rt::PrimaryReplayState replay;
  rt::DevVis vis{};
  bool replayOff = false;      // a rank context of an rt_mgpu_* host: never records
  bool visAllocFailed = false; // the planes did not fit once: this target size keeps tracing
  uint32_t replayRecorded = 0, replayReplayed = 0;   // launches, since rt_create
  // timing: per frame one event set; event 0 = frame start, event k = end of launch k.  Sets are harvested lazily.
  static constexpr int MAX_EV = 24, MAX_SETS = 1024;
  struct EvSet { hipEvent_t ev[MAX_EV]; int stage[MAX_EV]; int prev[MAX_EV]; int count; int last; };
  std::vector<EvSet> evSets;
  size_t evUsed = 0;
  double accStage[RT_STAGE_COUNT] = {}; double accFrame = 0; uint32_t accFrames = 0;
  // rt_reference_* (progressive ground-truth path tracer, csrc/reference.hip): allocated by the first rt_reference_render, freed by rt_resize / rt_destroy
  double* refAcc = nullptr;    // W x H x 6 fp64 sums (direct rgb, indirect rgb)
  float4* refMean = nullptr;   // W x H x 2 RGBA32F: the means rt_reference_readback / rt_reference_tonemap read
  uint32_t refN = 0;           // samples in refAcc; 0 = the sums are stale and are cleared by the next rt_reference_render
  bool refKeyValid = false;    // the RtxState inputs of the integral the sums were taken with (the others reset refN where they change)
  int32_t refMaxDepth = 0, refMIS = 0; float refHdrMultiplier = 0.f, refEnvironmentProb = 0.f;
  // The history of a temporal pass: its planes by frame parity (up to four per parity) and, next to them, the host state that says what they are worth.
  // Frame f reads parity f-1 and writes parity f; when it may is parity_history.h's rule.
  struct History { void* plane[2][4] = {}; rt::ParityHistory state; };
  // rt_set_denoiser (csrc/svgf.hip).  SVGF history: [frame parity][direct colour + n, indirect colour + n, direct moments, indirect moments], allocated by the
  // first frame rendered in SVGF mode, freed by rt_resize / rt_destroy.
  rt_denoiser den{RT_DENOISER_ATROUS, 0.2f, 0.2f, 32, 4.0f, 4.0f, {0, 0}};
  History histSvgf;
  // rt_set_gi_spatial (csrc/gi_spatial.hip).  The pass's reservoirs, allocated by the first frame rendered with the mode on, freed by rt_resize / rt_destroy.
  rt_gi_spatial gis{RT_GI_SPATIAL_OFF, 4, 10, 0.9f, 0.1f, 10.0f, {0, 0}};
  void* gisResv = nullptr;
  bool gisWritten = false;   // a frame with the mode on has been enqueued since gisResv was allocated
  // rt_set_taa (csrc/taa.hip).  History: [frame parity][direct, indirect, n], allocated by the first frame rendered with the mode on, freed by rt_resize /
  // rt_destroy.
  rt_taa taa{RT_TAA_OFF, 8, 0.1f, 1.0f, {0, 0, 0, 0}};
  History histTaa;
  // rt_set_upscale (csrc/upscale.hip).  History at the output size: [frame parity][direct, indirect, n], allocated by the first resolved frame
  // together with the output-size RGBA8 target and the tonemap's scratch (row sums, means, mip pyramids), freed by rt_resize / rt_destroy / an rt_set_upscale
  // that changes the output size.
  rt_upscale ups{RT_UPSCALE_OFF, 0, 0, 16, 0.1f, 1.0f, {0, 0}};
  History histUps;
  int upsW = 0, upsH = 0;    // the output size histUps was allocated for
  void* upsLdr = nullptr; double* upsRowSums = nullptr; float* upsMean = nullptr; float4* upsMipD = nullptr; float4* upsMipI = nullptr;
  bool upsLdrWritten = false;
  // rt_update_instances (csrc/refit.hip).  Made by the first update after a build from the device tree (ensureRefitState) and dropped with the tree: the record -> node
  // map, the contiguous node range of every level, per instance its largest |world coordinate| (the pad is a reduction over instances) and its handedness.
  // The device arrays live in accelAllocs.
  struct Refit {
    bool ready = false;
    std::vector<DevInstance> inst;               // host copy of the device instance rows
    std::vector<float> instMax;                  // largest |world coordinate| of every instance's triangles
    std::vector<uint8_t> flip;                   // 1: the instance's current matrix mirrors (det < 0): the TRI_FLIP bit k_refit_tris gives its records
    std::vector<std::pair<uint32_t, uint32_t>> levels;   // (first node, count), root level first
    uint32_t* dDirty = nullptr; uint32_t* dFlip = nullptr; uint32_t* dRecNode = nullptr; uint32_t* dNodeDirty = nullptr; uint32_t* dCounters = nullptr;
    float treePad = 0.f;                         // the pad the tree's boxes were last computed with
    rt_refit_stats stats{};
  } refit;
  hipEvent_t evRefit[2] = {nullptr, nullptr};    // timing of the last update (created by the first one)
  // rt_rebuild_accel (csrc/accel_build.hip).  Working buffers and two trees (the build writes the one the frames do not read; they swap after a build that succeeded),
  // allocated by the first rebuild after a host build and dropped with the host tree; `table` holds what the host build derived per triangle.
  struct Rebuild {
    AccelBuildWork work;
    AccelBuildSet set[2];
    int cur = -1;                                // the set the context's tree lives in (-1: the host build's arrays)
    bool ready = false;
    rt_rebuild_stats stats{};
    // rt_set_instances: what a new instance table is expanded into, twice (a call writes the ones the context does not use; they swap after a build that succeeded);
    // work.table is table[icur].  Sized with slack (triCap / instCap) by the first call after a host build and by a call whose counts do not fit.
    bool instReady = false;
    int icur = 0;
    uint32_t triCap = 0, instCap = 0;
    Tri48* table[2] = {nullptr, nullptr}; TriRef* triRef[2] = {nullptr, nullptr}; DevInstance* inst[2] = {nullptr, nullptr};
    uint32_t* prefix = nullptr;                  // instCap + 1 words (instances.h)
    uint32_t* dDirty = nullptr; uint32_t* dFlip = nullptr; uint32_t* dCounters = nullptr;   // the refit state's device words at instance capacity
  } rebuild;
  std::vector<void*> rebuildAllocs;
  // rt_set_rebuild_options: the values in force (defaults filled in).  They belong to the context, not to the buffers above: a new scene or host build keeps them.
  rt_rebuild_options rebuildOpt{RT_REBUILD_LBVH, ACCEL_PLOC_RADIUS_DEFAULT, ACCEL_PLOC_ITERATIONS_DEFAULT, 0};
  hipEvent_t evRebuild[4] = {nullptr, nullptr, nullptr, nullptr};   // start, sort begin, sort end, end
  // rt_set_instances (csrc/instances.hip).  The templates: per triangle of every prim mesh one AlphaRec and one opacity micro-map at
  // alphaIdx = meshAlphaBase[mesh] + triangle + 1, filled per mesh by the first table in which the mesh has an instance without RT_INST_FORCE_OPAQUE (meshMade).
  // They live in instAllocs from the first call until rt_upload_scene; once a call has succeeded they are the context's alpha records (DevScene::alphaRec).
  struct InstTemplates {
    std::vector<uint32_t> meshAlphaBase;
    std::vector<uint8_t> meshMade;
    AlphaRec* dAlpha = nullptr; uint4* dOmm = nullptr; uint32_t* dMeshAlphaBase = nullptr;
    size_t numAlpha = 0;                         // records of dAlpha / dOmm: 1 + the triangles of all prim meshes
    rt_instances_stats stats{};
  } inst;
  std::vector<void*> instAllocs;
  hipEvent_t evInst[2] = {nullptr, nullptr};     // around the expansion kernels
  // rt_update_vertices / rt_set_skins / rt_update_skins (csrc/deform.hip).  The skins' device buffers (rest pose, staging range, influences, the
  // per-call job and matrix tables) live in skinAllocs: replaced by rt_set_skins, dropped by rt_upload_scene.  The per-instance job table and the result words of
  // k_inst_coord_max live in deformAllocs, made by the first deforming call after an upload.  `stale[k]`: the device rows of skin k's mesh are newer than c->vertices.
  struct Deform {
    std::vector<rt_skin> skins;
    std::vector<uint32_t> restFirst;             // per skin: first row of its mesh in dRest / dStaged
    std::vector<int32_t> skinOfMesh;             // per prim mesh: its skin, or -1 (empty: no skins)
    std::vector<uint8_t> stale;
    rt_vertex* dRest = nullptr; rt_vertex* dStaged = nullptr; rt_skin_influence* dInfluences = nullptr;
    float* dJoints = nullptr; SkinJob* dSkinJobs = nullptr;
    CoordJob* dCoordJobs = nullptr; uint32_t* dOut = nullptr;   // dOut[0]: non-finite staged positions; dOut[1 + j]: coordinate maximum of job j
    size_t coordCap = 0;                         // instances dCoordJobs / dOut were sized for (rt_set_instances drops them when the table outgrows it)
    rt_deform_stats stats{};
  } deform;
  std::vector<void*> skinAllocs, deformAllocs;
  hipEvent_t evDeform[2] = {nullptr, nullptr};   // start / end of the skinning kernel and its commit copy
  // rt_set_morph_targets / rt_update_morphs (csrc/morph.hip).  The deltas, the rest pose and staging range of the morph-only meshes (a mesh with a
  // skin uses the skin's), and the per-call job and active-target tables live in morphAllocs: replaced by rt_set_morph_targets, dropped by rt_upload_scene.
  // weights[k]: the stored weights of set k; stale[k]: the device rows of a morph-only set's mesh are newer than c->vertices (a skinned mesh marks its skin).
  // skinMats[s]: the joint matrices of the last successful rt_update_skins that listed skin s (empty: never posed); kept with the skins, used by morph-then-skin.
  struct Morph {
    std::vector<rt_morph_set> sets;
    std::vector<int32_t> setOfMesh;              // per prim mesh: its set, or -1 (empty: no sets)
    std::vector<uint32_t> restFirst;             // per set: first row of its mesh in dRest / dStaged (morph-only meshes; unused where the mesh has a skin)
    std::vector<std::vector<float>> weights;
    std::vector<uint8_t> stale;
    rt_vertex* dRest = nullptr; rt_vertex* dStaged = nullptr; rt_morph_delta* dDeltas = nullptr;
    MorphJob* dJobs = nullptr; MorphActive* dActive = nullptr;
    rt_morph_stats stats{};
  } morph;
  std::vector<std::vector<float>> skinMats;
  std::vector<void*> morphAllocs;
  hipEvent_t evMorph[2] = {nullptr, nullptr};    // start / end of the morph kernel
  // rt_set_light_sources (csrc/light_records.hip).  The binding (one source per triangle-light record), the scratch records of the bind-time check
  // and the counter live in lightAllocs: replaced by rt_set_light_sources, dropped by rt_upload_scene.  The context keeps no host copy of the light records.
  struct Lights {
    uint32_t bound = 0;                          // records that have a source (0: no binding)
    std::vector<uint8_t> instances;              // per instance at binding time: 1 = a source names it (rt_set_instances keeps those in place)
    rt_light_source* dSources = nullptr;
    uint32_t* dCounter = nullptr;
    rt_light_stats stats{};
  } lights;
  std::vector<void*> lightAllocs;
  hipEvent_t evLights[2] = {nullptr, nullptr};   // start / end of the light kernel of the last update (created by the first binding)
  // rt_set_emitter_meshes (csrc/light_derive.hip).  The templates (rows of all meshes, first row per prim mesh) live in emitAllocs: replaced by
  // rt_set_emitter_meshes, dropped by rt_upload_scene.  set[]: the light buffers rt_set_instances derives into, each in a pool of its own; cur: the set the
  // context's records and binding live in (-1: the uploaded array and the binding of the switch-on, in sceneAllocs / lightAllocs).
  struct Emit {
    bool on = false;
    std::vector<int64_t> meshFirstRow;           // per prim mesh: first template row, or -1 (no template)
    std::vector<uint32_t> meshRows;              // per prim mesh: rows of its template
    float puncWeight = 0.f;
    rt_emitter_row* dRows = nullptr; uint32_t* dMeshFirstRow = nullptr;
    struct Set {
      rt_trig_light* rec = nullptr; rt_light_source* src = nullptr; rt_impt_samp* alias = nullptr; uint32_t* prefix = nullptr; uint32_t* ids = nullptr;
      uint32_t recCap = 0, emitCap = 0;
      std::vector<void*> pool;
    } set[2];
    int cur = -1;
    rt_emitter_stats stats{};
  } emit;
  std::vector<void*> emitAllocs;
  hipEvent_t evEmit[2] = {nullptr, nullptr};     // around k_light_expand
  // rt_update_materials / rt_update_texture (csrc/materials.hip).  The device words of the re-derivation live in matAllocs, sized by the first call
  // that needs them and again when the alpha records outgrow them; dropped by rt_upload_scene.  numTextures: the textures the scene uploaded (devTextures has one
  // white texel more when there were none); hostNumAlpha: the alpha records of the host tree (DevScene::alphaRec after rt_build_accel); the templates count theirs.
  struct Materials {
    uint32_t* dDirty = nullptr; uint32_t* dOwner = nullptr; uint32_t* dOwners = nullptr; uint32_t* dCounters = nullptr; uint4* dOmm = nullptr;
    size_t alphaCap = 0, dirtyWords = 0;
    rt_material_stats stats{};
  } mat;
  std::vector<void*> matAllocs;
  hipEvent_t evMat[2] = {nullptr, nullptr};      // around the device work of the last edit
  uint32_t numTextures = 0;
  size_t hostNumAlpha = 0;
  // rt_set_environment (csrc/env_accel.hip).  Two pairs of (map, table): a call fills the pair that DevScene does not name and DevScene takes it
  // only when the call is accepted.  live = -1: DevScene names the scene's own pair (sceneAllocs, rt_upload_scene).  A pair grows to the largest map it has held;
  // the work arrays of the device build (row areas, W, prefixes, ranks, tile sums, counters) likewise.  rt_upload_scene frees everything.
  struct Env {
    struct Pair { float* texels = nullptr; rt_impt_samp* accel = nullptr; size_t cap = 0; } pair[2];
    int live = -1;
    float* dArea = nullptr; size_t areaCap = 0;
    uint64_t* dW = nullptr; EnvU128* dP = nullptr; uint32_t* dIdx = nullptr; EnvBlockSum* dBlockSums = nullptr; uint32_t* dCounters = nullptr;
    size_t workCap = 0;
    rt_environment_stats stats{};
  } env;
  hipEvent_t evEnv[2] = {nullptr, nullptr};      // around the device work of the last accepted call
  // rt_set_object_motion (the RT_OM builds of csrc/stages.hip).  omPrev[i] is instance i's objectToWorld at the last rendered frame where omMoved[i]
  // is set (rt_update_instances records it once per frame; every other instance's previous matrix is its current one); a rendered frame clears the flags.
  int objMotion = RT_OBJECT_MOTION_OFF;
  std::vector<std::array<float, 12>> omPrev;
  std::vector<uint8_t> omMoved;
  bool omPending = false;    // some omMoved flag is set
  // the instance image (lifetime of RT_BUF_MOTION: rotated with it) and the per-instance camera table (rewritten only by frames with motion, which follow the
  // drain of rt_update_instances, so one copy serves the frames in flight); allocated once the mode has been switched on
  void* omInst = nullptr;    // (its ring partners: spare[RING_INST])
  bool omInstValid = false;  // a frame has written omInst since rt_resize
  void* omTable = nullptr; size_t omTableRows = 0;
  std::vector<OmCamera> omHost;
  // per-vertex motion vectors (mode RT_OBJECT_MOTION_VERTEX; the RT_VM builds of csrc/stages.hip, csrc/vmotion.hip).  Everything below exists once
  // the mode has been switched on (vmEver).  vmPlane: one float4 per scene vertex; the first deforming call for a mesh after a rendered frame copies the mesh's
  // live positions into it ahead of its commit and sets vmDeformed[mesh] (whether the mode is on or off, like omPrev); a rendered frame clears the flags.
  // vmDelta: the delta image, lifetime and rotation of omInst.  vmTable: the per-instance rows, rewritten only by frames that follow a draining update.
  bool vmEver = false;
  void* vmPlane = nullptr;
  std::vector<uint8_t> vmDeformed;
  bool vmPending = false;    // some vmDeformed flag is set
  void* vmDelta = nullptr;   // (its ring partners: spare[RING_DELTA])
  bool vmDeltaValid = false; // a vertex-mode frame has written vmDelta since rt_resize
  void* vmTable = nullptr; size_t vmTableRows = 0;
  std::vector<VmRow> vmHost;
};

static void harvestTimings(rt_ctx* c)
{
  for(size_t s = 0; s < c->evUsed; s++) {
    rt_ctx::EvSet& E = c->evSets[s];
    for(int k = 1; k < E.count; k++) {
      float ms = 0.f;
      if(E.stage[k] >= 0 && hipEventElapsedTime(&ms, E.ev[E.prev[k]], E.ev[k]) == hipSuccess) c->accStage[E.stage[k]] += ms;
    }
    float ms = 0.f;
    if(E.count > 1 && hipEventElapsedTime(&ms, E.ev[0], E.ev[E.last]) == hipSuccess) { c->accFrame += ms; c->accFrames++; }
  }
  c->evUsed = 0;
}

// Wait (host) for everything this context has submitted.
static hipError_t syncAll(rt_ctx* c)
{
  hipError_t e = hipStreamSynchronize(c->stream);
  if(e == hipSuccess && c->indStream) e = hipStreamSynchronize(c->indStream);
  if(e == hipSuccess && c->sideStream) e = hipStreamSynchronize(c->sideStream);
  c->inFlight = false; c->seq = 0;
  return e;
}
// Make `stream` (device side) wait for the frames in flight on the internal streams: needed before work that is submitted
// to `stream` alone (rt_run_stage, the non-pipelined rt_render_frame) may touch the frame buffers.
static hipError_t joinInFlight(rt_ctx* c)
{
  if(!c->inFlight) return hipSuccess;
  const int r = int((c->seq - 1) & 3);
  hipError_t e = hipStreamWaitEvent(c->stream, c->evI[r], 0);
  if(e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->evDone[r], 0);
  c->inFlight = false; c->seq = 0;
  return e;
}

// What runs a launch: the filter chains and compose exist once (csrc/filters.hip); every other stage comes from one of the builds of stages.hip (STAGE_BUILDS in
// build.py).  Which one is stage_select.h's rule; this file holds what the rule is fed with and the table from its answer to a function.
// The traced kernels exist twice: the throughput build (one ray per lane, majority-vote rounds, 4-5 waves per
// SIMD: full frames are bound by instruction issue) and the latency build (RT_LAT: eight lanes per ray, a workgroup of eight waves per tile:
// a row band of a multi-GPU frame or a small image is bound by the dependent steps of its slowest rays, and the latency build shortens the step).
// RT_TRAVERSAL_AUTO decides by the number of 8x8 tiles of the launch; the thresholds are where the two builds measured equal on the benchmark scene
// (profiles/r03_band_chunk_ab.txt, profiles/r03_lat_wide_ab.txt):
//   launches that run alone (rt_set_overlap 0/1; the barrier schedule of rt_mgpu): direct stage up to 2000 tiles (64 rows of 1080p), indirect stage up to
//     2000 half-res tiles (256 rows of 1080p) — round 4, with gang mode in the latency build (round 3: 1440 / 1536; profiles/r04_band_thresholds.txt, profiles/r04_gang_ab.txt);
//   launches that share the CUs with the kernels of another frame (rt_set_overlap 2; frames in flight in rt_mgpu): 512 / 640 — eight lanes per ray buy a
//     short chain with 2-4x the lane-cycles, which a co-running kernel would have used.
// The counting build is a throughput build.  Bit-identical either way.  RESTIR_LAT_TILES / RESTIR_LAT_TILES_IND override both cases (experiments).
static int envInt(const char* name) { const char* e = getenv(name); return e ? atoi(e) : -1; }
static rt::LatencyTiles latencyTiles(bool shared)
{
  static const int alone = envInt("RESTIR_LAT_TILES"), sh = envInt("RESTIR_LAT_TILES_SHARED");
  static const int aloneInd = envInt("RESTIR_LAT_TILES_IND"), shInd = envInt("RESTIR_LAT_TILES_IND_SHARED");
  if(!shared) return {alone >= 0 ? alone : 2000, aloneInd >= 0 ? aloneInd : 2000};
  return {sh >= 0 ? sh : (alone >= 0 ? alone : 512), shInd >= 0 ? shInd : (aloneInd >= 0 ? aloneInd : 640)};
}
typedef hipError_t (*StageLauncher)(hipStream_t, const DevScene&, const DevFrame&, const rt::StageExtra&, const rt_state&, const rt_scene_camera&, int, int, int, int);
static hipError_t filterLauncher(hipStream_t stream, const DevScene&, const DevFrame& F, const rt::StageExtra&, const rt_state& st, const rt_scene_camera& cam, int stage,
                                 int level, int r0, int r1)
{ return rt::launchFilterStage(stream, F, st, cam, stage, level, r0, r1); }
static const StageLauncher g_stageLaunchers[rt::STAGE_BUILD_COUNT] = {   // by rt::StageBuild
#define RT_STAGE_LAUNCHER(ns) rt::ns::launchStage,
  RT_STAGE_BUILDS(RT_STAGE_LAUNCHER)
#undef RT_STAGE_LAUNCHER
  filterLauncher};

// ---- settled primary visibility (primary_replay.h) -------------------------------------------------------------------------------------------------
// RESTIR_PRIMARY_REPLAY=0 switches it off, RESTIR_VIS_K sets the list length per pixel (1..64), RESTIR_VIS_REST_FRAMES the at-rest launches ahead of a recording (>= 2);
// each is read once per process.
static bool replayEnabled() { static const int v = envInt("RESTIR_PRIMARY_REPLAY"); return v != 0; }
static uint32_t visListLength() { static const int v = envInt("RESTIR_VIS_K"); return uint32_t(v <= 0 ? RT_VIS_K_DEFAULT : std::min(v, 64)); }
static int visRestFrames() { static const int v = envInt("RESTIR_VIS_REST_FRAMES"); return v < 2 ? 2 : v; }
static void freeVis(rt_ctx* c)
{
  for(uint32_t** p : {&c->vis.det, &c->vis.count, &c->vis.list}) { if(*p) (void)hipFree(*p); *p = nullptr; }
  c->vis.K = 0;
  c->visAllocFailed = false;
  rt::primaryReplayInvalidate(c->replay);
}
// whatever can change what a primary ray hits, or the order of the leaf records, calls this (the list is in DESIGN.md §25)
static void dropPrimaryReplay(rt_ctx* c) { rt::primaryReplayInvalidate(c->replay); }
// One direct launch passes through the rule.  Returns what it does; for RECORD / REPLAY `V` is the kernel argument.  A recording whose planes cannot be allocated
// is a normal launch, and the target size stops asking.
static rt::PrimaryReplayAction primaryReplayLaunch(rt_ctx* c, const rt_state& st, const rt_scene_camera& cam, bool fullFrame, bool eligible, rt::DevVis& V)
{
  rt::PrimaryReplayLaunch l{};
  l.view = rt::primaryReplayViewOf(cam, st.size.x, st.size.y);
  l.fullFrame = fullFrame;
  l.eligible = eligible && replayEnabled() && !c->replayOff && !c->visAllocFailed && c->ds.numTris > 0;
  rt::PrimaryReplayAction a = rt::primaryReplayStep(c->replay, l, visRestFrames());
  if(a == rt::PRIMARY_REPLAY_RECORD && !c->vis.det) {
    const size_t n = size_t(c->W) * size_t(c->H);
    const uint32_t K = visListLength();
    bool ok = hipMalloc(reinterpret_cast<void**>(&c->vis.det), n * 4) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&c->vis.count), n * 4) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&c->vis.list), n * 4 * K) == hipSuccess;
    if(!ok) { (void)hipGetLastError(); freeVis(c); c->visAllocFailed = true; return rt::PRIMARY_REPLAY_NORMAL; }
    c->vis.K = K;
  }
  V = c->vis;
  V.record = a == rt::PRIMARY_REPLAY_RECORD ? 1u : 0u;
  return a;
}
// after a RECORD / REPLAY launch was issued (or failed to be)
static void primaryReplayIssued(rt_ctx* c, rt::PrimaryReplayAction a, bool ok)
{
  if(!ok) { dropPrimaryReplay(c); return; }
  if(a == rt::PRIMARY_REPLAY_RECORD) c->replayRecorded++;
  if(a == rt::PRIMARY_REPLAY_REPLAY) c->replayReplayed++;
}

// One launch of a stage on `strm`, for rt_render_frame and rt_run_stage alike.  A direct launch that spawns primary rays (level 2 is the rayless half) passes through
// the replay rule, eligible when it would be a throughput launch of a context without TAA, without temporal upsampling and without a motion-vector mode; stage_select.h names the build; a
// RECORD / REPLAY launch reports back to the rule.  `motion`: the motion-vector form of the frame's traced stages, whose argument `X` then holds.
static hipError_t launchStageOn(rt_ctx* c, hipStream_t strm, const DevFrame& F, rt::StageExtra X, rt::StageMotion motion, const rt_state& st, const rt_scene_camera& cam,
                                int stage, int level, int rowBegin, int rowEnd)
{
  const bool lat = rt::latencyBuild(c->counting, c->traversal, stage, st.size.x, st.size.y, rowBegin, rowEnd, latencyTiles(c->overlap >= 2));
  rt::DevVis V{};
  rt::PrimaryReplayAction act = rt::PRIMARY_REPLAY_NORMAL;
  if(stage == RT_STAGE_DIRECT && level != 2) {
    const bool fullFrame = rowBegin == 0 && (rowEnd <= 0 || rowEnd >= c->H);
    act = primaryReplayLaunch(c, st, cam, fullFrame, c->taa.mode == RT_TAA_OFF && c->ups.mode == RT_UPSCALE_OFF && c->objMotion == RT_OBJECT_MOTION_OFF && !lat, V);
  }
  X.vis = &V;
  const hipError_t e = g_stageLaunchers[rt::stageBuild(c->ds.sky, c->counting, lat, stage, motion, act)](strm, c->ds, F, X, st, cam, stage, level, rowBegin, rowEnd);
  if(act != rt::PRIMARY_REPLAY_NORMAL) primaryReplayIssued(c, act, e == hipSuccess);
  return e;
}

// ---- host side of rt_build_accel, cached by scene content (buildHostAccel below) ---------------------------------------------------------------------
struct HostAccel {
  uint64_t key0 = 0, key1 = 0;      // content hash of everything the build reads
  BuildOutput bo;
  std::vector<AlphaRec> alpha;      // bgra left null: patched per device from alphaTex
  std::vector<int32_t> alphaTex;    // texture index of every alpha record, -1 = none
};
static std::mutex g_accelMutex;
static std::shared_ptr<const HostAccel> g_accelCache;   // the most recent build; dropped with the last context
static std::atomic<int> g_liveCtx{0};

static thread_local std::string g_createErr;

// the one rule for a HIP call that failed: the context's error names who failed and why, the code tells out-of-memory from the rest
static int hipFail(rt_ctx* c, const char* who, hipError_t e)
{
  c->err = std::string(who) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP;
}

#define RT_HIP(ctx, call)                                                                                                   \
  do {                                                                                                                      \
    hipError_t e_ = (call);                                                                                                 \
    if(e_ != hipSuccess) return hipFail((ctx), #call, e_);                                                                  \
  } while(0)

// creates the events of the array that do not exist yet; stops at the first error
template <size_t N> static hipError_t ensureEvents(hipEvent_t (&ev)[N])
{
  for(hipEvent_t& e : ev)
    if(!e) { const hipError_t he = hipEventCreate(&e); if(he != hipSuccess) return he; }
  return hipSuccess;
}

// ---- opacity micro-map ---------------------------------------------------------------------------------------------
// The rule (cell footprint, cell state) is csrc/opacity_map.h's; here is the host's serial scan over an alpha plane (rt_upload_scene's hostAlpha).
static void buildOpacityMap(const AlphaRec& a, const std::vector<uint8_t>* alpha, uint32_t omm[4])
{
  const float uv[6] = {a.uv0x, a.uv0y, a.uv1x, a.uv1y, a.uv2x, a.uv2y};
  ommBuildSerial(uv, a.baseAlpha, a.cutoff, a.alphaMode, a.w, a.h, a.wrapS, a.wrapT, alpha ? alpha->data() : nullptr, 1, omm);
}

static int fail(rt_ctx* c, int code, const char* msg) { c->err = msg; return code; }
// what rt_upload_scene and rt_update_materials ask of a material row in a scene of nTex textures: why it is refused, or nullptr
static const char* checkMaterialRow(const rt_material& m, int32_t nTex)
{
  const int32_t ids[5] = {m.pbrBaseColorTexture, m.pbrMetallicRoughnessTexture, m.emissiveTexture, m.normalTexture, m.transmissionTexture};
  for(int32_t id : ids)
    if(id < -1 || id >= nTex) return "material references a missing texture";
  return nullptr;
}
// a device buffer of at least 256 bytes with every byte set to `fill` (on the null stream: the caller synchronises the device before its streams touch it)
static hipError_t mallocFilled(void** p, size_t bytes, int fill)
{
  bytes = std::max<size_t>(bytes, 256);
  const hipError_t e = hipMalloc(p, bytes);
  if(e != hipSuccess) { *p = nullptr; return e; }
  return hipMemset(*p, fill, bytes);
}
// the planes of a temporal pass's history (the caller has drained the context)
static void freeHistory(rt_ctx::History& h)
{
  for(auto& par : h.plane) for(void*& p : par) { if(p) (void)hipFree(p); p = nullptr; }
  h.state.reset();
}
// Both parities of the history of `pass`, one plane per entry of `bytes` (rt_render_frame's first frame with the pass on; the caller has drained the context).
// Zeroed: nothing reads a plane before a frame wrote it.  All or nothing.
static int allocHistory(rt_ctx* c, rt_ctx::History& h, std::initializer_list<size_t> bytes, const char* pass)
{
  bool ok = true;
  for(auto& par : h.plane) {
    void** p = par;
    for(size_t b : bytes) ok = ok && mallocFilled(p++, b, 0) == hipSuccess;
  }
  if(!ok) { freeHistory(h); c->err = std::string("rt_render_frame: hipMalloc of the ") + pass + " history failed"; return RT_ERR_OOM; }
  RT_HIP(c, hipDeviceSynchronize());
  h.state.reset();
  return RT_OK;
}
// The arguments of the resolve of frame `frames` that TAA and temporal upsampling share (TaaArgs / UpscaleArgs): the frame's images and G-buffers, the
// history planes [direct, indirect, n] the pass reads and writes, and the pass's settings.
template <class Args, class Settings> static Args resolveArgs(const rt_ctx* c, const rt_ctx::History& h, const Settings& s, const DevFrame& F, int frames, bool histValid)
{
  Args A{};
  void* const* cur = h.plane[rt::frameParity(frames)]; void* const* prev = h.plane[rt::otherParity(frames)];
  A.thisG = F.thisG; A.lastG = F.lastG;
  A.curD = F.thisDirectResult; A.curI = F.thisIndirectResult;
  A.prevD = static_cast<const float4*>(prev[0]); A.prevI = static_cast<const float4*>(prev[1]); A.prevN = static_cast<const float*>(prev[2]);
  A.outD = static_cast<float4*>(cur[0]); A.outI = static_cast<float4*>(cur[1]); A.outN = static_cast<float*>(cur[2]);
  A.W = c->W; A.H = c->H;
  A.histValid = histValid ? 1 : 0;
  A.alpha = s.alpha; A.clipGamma = s.clipGamma;
  return A;
}
// the tail of the *_readback calls, after their own argument checks: drain the context, then copy `bytes` bytes of device memory to the host
static int readbackDrained(rt_ctx* c, const void* src, void* dst, size_t bytes)
{
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  if(bytes) RT_HIP(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}
// a new scene or a new tree: the next frame of every temporal pass starts without history
static void invalidateHistories(rt_ctx* c) { for(rt_ctx::History* h : {&c->histSvgf, &c->histTaa, &c->histUps}) h->state.invalidate(); }
// The ring of frames in flight (rt_ctx::spare).  The live buffer of a kind for frame `frames`: the boundary ids keep their meaning across rotations.
static void*& ringLive(rt_ctx* c, int kind, int frames)
{
  switch(kind) {
    case rt_ctx::RING_G: return c->bufs[RT_BUF_GBUFFER0 + rt::frameParity(frames)];
    case rt_ctx::RING_MOTION: return c->bufs[RT_BUF_MOTION];
    case rt_ctx::RING_DIRECT: return c->bufs[RT_BUF_DIRECT_RESULT0 + rt::frameParity(frames)];
    case rt_ctx::RING_INST: return c->omInst;
    default: return c->vmDelta;
  }
}
// three frames in flight: rt_set_overlap 3, and rt_resize made every buffer the deeper ring needs
static bool ringDeep(const rt_ctx* c) { return c->overlap >= 3 && c->spare[rt_ctx::RING_G][1] && c->spare[rt_ctx::RING_MOTION][1] && c->spare[rt_ctx::RING_DIRECT][0]; }
// one kind moves on by a frame: the two-deep swap with the first spare, or the three-deep shift (the next spare becomes live, the live buffer waits longest)
static void rotate(void*& live, void* spare[2], bool deep)
{
  if(deep) { void* t = live; live = spare[0]; spare[0] = spare[1]; spare[1] = t; }
  else std::swap(live, spare[0]);
}
// Every kind that exists moves on by a frame.  The direct image rotates only at three frames in flight, where its two parities and its one spare make the three.
static void rotateRing(rt_ctx* c, int frames, bool deep)
{
  for(int kind = 0; kind < rt_ctx::RING_KINDS; kind++) {
    void*& live = ringLive(c, kind, frames);
    if(live && (kind != rt_ctx::RING_DIRECT || deep)) rotate(live, c->spare[kind], deep && kind != rt_ctx::RING_DIRECT);
  }
}
static void freeSpares(rt_ctx* c, std::initializer_list<int> kinds)
{
  for(int kind : kinds) for(void*& p : c->spare[kind]) { if(p) (void)hipFree(p); p = nullptr; }
}
// the GI spatial reservoirs (the caller has drained the context)
static void freeGiSpatial(rt_ctx* c)
{
  if(c->gisResv) (void)hipFree(c->gisResv);
  c->gisResv = nullptr; c->gisWritten = false;
}
// the instance images of rt_set_object_motion, and the motion state: what moved before the buffers were dropped is not in motion for the next frame
// (the caller has drained the context)
static void freeObjectMotion(rt_ctx* c)
{
  for(void** p : {&c->omInst, &c->vmDelta}) if(*p) { (void)hipFree(*p); *p = nullptr; }
  freeSpares(c, {rt_ctx::RING_INST, rt_ctx::RING_DELTA});
  c->omInstValid = c->vmDeltaValid = false;
  c->omPrev.clear(); c->omMoved.clear(); c->omPending = false;
  std::fill(c->vmDeformed.begin(), c->vmDeformed.end(), uint8_t(0)); c->vmPending = false;   // (the plane is sized by the scene: it stays)
}
// The previous-position plane of per-vertex motion vectors: one float4 per vertex of the uploaded scene, zeroed (a row is read only after a capture wrote it).
// Made by the call that first switches the mode on and again by every rt_upload_scene after it (callers have drained the context).
static int allocVertexMotionPlane(rt_ctx* c)
{
  if(c->vmPlane || !c->haveScene) return RT_OK;
  const size_t bytes = std::max<size_t>(c->vertices.size() * sizeof(float4), 256);
  RT_HIP(c, hipMalloc(&c->vmPlane, bytes));
  RT_HIP(c, hipMemset(c->vmPlane, 0, bytes));
  RT_HIP(c, hipDeviceSynchronize());
  c->vmDeformed.assign(c->primMeshes.size(), 0); c->vmPending = false;
  return RT_OK;
}
// What a deforming call does for prim mesh `mesh` before it changes the live rows (on stream s, which the change follows): the first one after a rendered frame
// copies the mesh's live positions into the plane; later ones before the next frame keep the rendered frame's positions, as omPrev keeps its matrices.
static int capturePrevPositions(rt_ctx* c, hipStream_t s, uint32_t mesh)
{
  if(!c->vmPlane || mesh >= c->vmDeformed.size() || c->vmDeformed[mesh]) return RT_OK;
  const rt_prim_mesh& pm = c->primMeshes[mesh];
  RT_HIP(c, launchCapturePositions(s, c->ds.vertices, static_cast<float4*>(c->vmPlane), pm.vertexOffset, pm.vertexCount));
  c->vmDeformed[mesh] = 1; c->vmPending = true;
  return RT_OK;
}
// the upsampling history and what rt_upscale_tonemap needs at the output size (the caller has drained the context)
static void freeUpscaleHistory(rt_ctx* c)
{
  freeHistory(c->histUps);
  for(void* p : {c->upsLdr, static_cast<void*>(c->upsRowSums), static_cast<void*>(c->upsMean), static_cast<void*>(c->upsMipD), static_cast<void*>(c->upsMipI)}) if(p) (void)hipFree(p);
  c->upsLdr = nullptr; c->upsRowSums = nullptr; c->upsMean = nullptr; c->upsMipD = c->upsMipI = nullptr;
  c->upsW = c->upsH = 0; c->upsLdrWritten = false;
}

// Stream priorities of the frames-in-flight schedule.  RESTIR_PRIO = 0..3 (rounds 2-4: 0 none, 1 indirect + filter streams high, 2 indirect stream high — the
// default —, 3 filter stream high) or three characters over {-, 0, +} for the main (direct stage) / indirect / filter stream: "+00" = main stream high, "0+-" =
// indirect high and filters low.  level: -1 low, 0 normal, +1 high.
static void prioSpec(int level[3])   // (read at every rt_create: a host may change RESTIR_PRIO between contexts)
{
  level[0] = 0; level[1] = 1; level[2] = 0;
  const char* e = getenv("RESTIR_PRIO");
  if(e && strlen(e) == 3 && strspn(e, "-0+") == 3) { for(int i = 0; i < 3; i++) level[i] = e[i] == '+' ? 1 : (e[i] == '-' ? -1 : 0); }
  else if(e) { const int m = atoi(e); level[0] = 0; level[1] = (m == 1 || m == 2) ? 1 : 0; level[2] = (m == 1 || m == 3) ? 1 : 0; }
}
static std::atomic<int> g_streamsCreated{0};   // HIP streams this library has created in the process so far (a stream's worth depends on its place in that order)
static hipError_t createStreamLevel(hipStream_t* s, int level)
{
  int plo = 0, phi = 0;
  (void)hipDeviceGetStreamPriorityRange(&plo, &phi);
  hipError_t e;
  if(level < 0 && phi < plo) e = hipStreamCreateWithPriority(s, hipStreamNonBlocking, plo);   // (numerically larger = lower priority)
  else e = (level > 0 && phi < plo) ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, phi) : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  if(e == hipSuccess) g_streamsCreated.fetch_add(1);
  return e;
}

template <class T> static int upload(rt_ctx* c, std::vector<void*>& pool, const T* src, size_t count, const T** out)
{
  void* d = nullptr;
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  RT_HIP(c, hipMalloc(&d, bytes));
  pool.push_back(d);
  if(count && src) RT_HIP(c, hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
  else RT_HIP(c, hipMemset(d, 0, bytes));
  *out = static_cast<const T*>(d);
  return RT_OK;
}
// a zero-filled device array the library itself writes later (upload is for scene data, which stays const)
template <class T> static int allocZeroed(rt_ctx* c, std::vector<void*>& pool, size_t count, T** out)
{
  const T* const noSource = nullptr;   // upload clears the array instead of copying
  const T* p = nullptr;
  const int rc = upload(c, pool, noSource, count, &p);
  *out = const_cast<T*>(p);
  return rc;
}
static void freePool(std::vector<void*>& pool) { for(void* p : pool) (void)hipFree(p); pool.clear(); }
// what rt_set_environment allocated (the caller has drained the context and no longer lets c->ds name a pair); the statistics go with it
static void freeEnvironment(rt_ctx* c)
{
  rt_ctx::Env& E = c->env;
  for(auto& p : E.pair) { if(p.texels) (void)hipFree(p.texels); if(p.accel) (void)hipFree(p.accel); }
  for(void* p : {static_cast<void*>(E.dArea), static_cast<void*>(E.dW), static_cast<void*>(E.dP), static_cast<void*>(E.dIdx), static_cast<void*>(E.dBlockSums),
                 static_cast<void*>(E.dCounters)})
    if(p) (void)hipFree(p);
  E = rt_ctx::Env{};
}
// the emitter mode leaves the context: templates and derived light buffers go (the caller has drained the context and replaces what c->ds.trigLights names)
static void dropEmitters(rt_ctx* c)
{
  freePool(c->emitAllocs);
  for(auto& S : c->emit.set) freePool(S.pool);
  c->emit = rt_ctx::Emit{};
}
// RESTIR_BVH_TIMING=1: where the seconds of rt_upload_scene / rt_build_accel go (stderr)
struct LoadTimer {
  const bool on = getenv("RESTIR_BVH_TIMING") && atoi(getenv("RESTIR_BVH_TIMING")) != 0;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what) { if(!on) return; const auto n = std::chrono::steady_clock::now(); fprintf(stderr, "[scene load] %-34s %.3f s\n", what, std::chrono::duration<double>(n - t).count()); t = n; }
};
static int ensureStackOverflow(rt_ctx* c);
static int syncHostVertices(rt_ctx* c, int mesh = -1);
static size_t numAlphaRecords(const rt_ctx* c);
static int allocObjectMotion(rt_ctx* c);
static void reopenPriorityDecision(rt_ctx* c);
static void hashBytes(const void* p, size_t n, uint64_t& h0, uint64_t& h1);
static int stackLdsEnv() { static const int v = getenv("RESTIR_STACK_LDS") ? std::max(2, atoi(getenv("RESTIR_STACK_LDS"))) : 0; return v; }
static int stackLdsMin() { return stackLdsEnv() ? stackLdsEnv() : 6; }   // the shortest LDS stack any schedule uses: sizes the overflow areas

static size_t elemBytes(int id)
{
  switch(id) {
    case RT_BUF_GBUFFER0: case RT_BUF_GBUFFER1: return 16;
    case RT_BUF_MOTION: return 4;
    case RT_BUF_DIRECT_RESV0: case RT_BUF_DIRECT_RESV1: case RT_BUF_DIRECT_RESV_TEMP: return sizeof(rt_direct_reservoir);
    case RT_BUF_INDIRECT_RESV0: case RT_BUF_INDIRECT_RESV1: case RT_BUF_INDIRECT_RESV_TEMP: return sizeof(rt_indirect_reservoir);
    case RT_BUF_LIGHT_ID0: case RT_BUF_LIGHT_ID1: case RT_BUF_LDR: return 4;
    default: return 16;
  }
}
#ifndef RT_WAVEPROF
#define RT_WAVEPROF 0
#endif
static constexpr size_t WAVEPROF_RECORDS = 1 << 17;   // measurement builds: one record per workgroup of a traced launch
static constexpr int RT_PAD_ROWS = 128;  // full-res rows of slack behind every buffer (64 for half-res buffers)
static bool halfRes(int id) { return id == RT_BUF_INDIRECT_RESV0 || id == RT_BUF_INDIRECT_RESV1 || id == RT_BUF_INDIRECT_RESV_TEMP; }

extern "C" {

uint32_t rt_abi_version(void) { return (RT_ABI_VERSION_MAJOR << 16) | RT_ABI_VERSION_MINOR; }

const char* rt_last_error(rt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_createErr.c_str(); }

}  // extern "C"
// rt_create with explicit stream levels (main / indirect / filter; nullptr = RESTIR_PRIO or the defaults): csrc/mgpu.cpp gives every rank's context the levels of its
// schedule so that the rank's streams are the CONTEXT's streams, created in the order the single-GPU schedule was tuned for (round 6) — not part of the C ABI.
int rtCreateWithLevels(rt_ctx** out, int device, const int* levels);
extern "C" {
int rt_create(rt_ctx** out, int device) { return rtCreateWithLevels(out, device, nullptr); }
}
int rtCreateWithLevels(rt_ctx** out, int device, const int* levels)
{
  if(!out) { g_createErr = "rt_create: out is NULL"; return RT_ERR_INVALID_ARG; }
  *out = nullptr;
  int n = 0;
  if(hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_createErr = "rt_create: no HIP device (this library has no CPU path)"; return RT_ERR_NO_DEVICE; }
  if(device < 0 || device >= n) { g_createErr = "rt_create: device index out of range"; return RT_ERR_INVALID_ARG; }
  if(hipSetDevice(device) != hipSuccess) { g_createErr = "rt_create: hipSetDevice failed"; return RT_ERR_HIP; }
  rt_ctx* c = new(std::nothrow) rt_ctx();
  if(!c) { g_createErr = "rt_create: out of host memory"; return RT_ERR_OOM; }
  g_liveCtx.fetch_add(1);   // counted from here on: every exit below goes through rt_destroy, which un-counts it
  c->device = device;
  {
    prioSpec(c->prio); c->prioFromEnv = getenv("RESTIR_PRIO") != nullptr; c->prioDecided = c->prioFromEnv;
    if(levels) { for(int i = 0; i < 3; i++) c->prio[i] = std::max(-1, std::min(1, levels[i])); c->prioDecided = c->prioExplicit = true; }
    c->replayOff = levels != nullptr;   // the rt_mgpu_* hosts render row bands and exchange history between devices: their contexts never record primary visibility
    bool ok = createStreamLevel(&c->ownStream, c->prio[0]) == hipSuccess;
    if(!ok) { g_createErr = "rt_create: hipStreamCreate failed"; rt_destroy(c); return RT_ERR_HIP; }
    c->mainIdx = g_streamsCreated.load() - 1;
    c->stream = c->ownStream;
    for(int i = 0; i < 4; i++) {
      ok = ok && hipEventCreateWithFlags(&c->evD[i], hipEventDisableTiming) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&c->evI[i], hipEventDisableTiming) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&c->evDone[i], hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming) == hipSuccess;
    if(!ok) { g_createErr = "rt_create: creating the internal events failed"; rt_destroy(c); return RT_ERR_HIP; }
  }
  if(const char* e = getenv("RESTIR_OVERLAP")) c->overlap = atoi(e);
  if(hipMalloc(reinterpret_cast<void**>(&c->dCounters), 8 * sizeof(unsigned long long)) != hipSuccess) { g_createErr = "rt_create: hipMalloc failed"; rt_destroy(c); return RT_ERR_OOM; }
  (void)hipMemset(c->dCounters, 0, 8 * sizeof(unsigned long long));
  *out = c;
  return RT_OK;
}

extern "C" {

int rt_destroy(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->device);
  (void)syncAll(c);
  freePool(c->sceneAllocs); freePool(c->accelAllocs); freePool(c->scratchAllocs); freePool(c->ovfAllocs); freePool(c->rebuildAllocs);
  freePool(c->skinAllocs); freePool(c->deformAllocs); freePool(c->lightAllocs); freePool(c->morphAllocs); freePool(c->instAllocs);
  dropEmitters(c);
  for(int i = 0; i < RT_BUF_COUNT; i++) if(c->bufs[i]) (void)hipFree(c->bufs[i]);
  freeSpares(c, {rt_ctx::RING_G, rt_ctx::RING_MOTION, rt_ctx::RING_DIRECT, rt_ctx::RING_INST, rt_ctx::RING_DELTA});
  for(void* p : {c->omInst, c->omTable, c->vmPlane, c->vmDelta, c->vmTable}) if(p) (void)hipFree(p);
  for(void* p : c->indA) if(p && p != c->bufs[RT_BUF_DENOISE_IND_A]) (void)hipFree(p);
  for(hipStream_t& q : c->indStreams) { if(q) (void)hipStreamDestroy(q); q = nullptr; }
  for(hipStream_t& q : c->sideStreams) { if(q) (void)hipStreamDestroy(q); q = nullptr; }
  c->indStream = c->sideStream = nullptr;   // (the per-level arrays own the streams)
  for(int i = 0; i < 4; i++) { if(c->evD[i]) (void)hipEventDestroy(c->evD[i]); if(c->evI[i]) (void)hipEventDestroy(c->evI[i]); if(c->evDone[i]) (void)hipEventDestroy(c->evDone[i]); }
  if(c->dCounters) (void)hipFree(c->dCounters);
  freeVis(c);
  if(c->dSky) (void)hipFree(c->dSky);
  if(c->dPick) (void)hipFree(c->dPick);
  if(c->refAcc) (void)hipFree(c->refAcc);
  if(c->refMean) (void)hipFree(c->refMean);
  freeHistory(c->histSvgf);
  freeGiSpatial(c);
  freeHistory(c->histTaa);
  freeUpscaleHistory(c);
  for(auto& E : c->evSets) for(int i = 0; i < rt_ctx::MAX_EV; i++) (void)hipEventDestroy(E.ev[i]);
  if(c->ownStream) (void)hipStreamDestroy(c->ownStream);
  if(c->evFork) (void)hipEventDestroy(c->evFork);
  if(c->evJoin) (void)hipEventDestroy(c->evJoin);
  for(hipEvent_t e : c->evRefit) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evDeform) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evMorph) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evLights) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evRebuild) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evInst) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evEmit) if(e) (void)hipEventDestroy(e);
  for(hipEvent_t e : c->evMat) if(e) (void)hipEventDestroy(e);
  freePool(c->matAllocs);
  for(hipEvent_t e : c->evEnv) if(e) (void)hipEventDestroy(e);
  freeEnvironment(c);
  delete c;
  if(g_liveCtx.fetch_sub(1) == 1) { std::lock_guard<std::mutex> one(g_accelMutex); g_accelCache.reset(); }   // the last context takes the cached host build with it
  return RT_OK;
}

int rt_set_stream(rt_ctx* c, void* s)
{
  if(!c) return RT_ERR_INVALID_ARG;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  c->stream = s ? static_cast<hipStream_t>(s) : c->ownStream;
  return RT_OK;
}

int rt_sync(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  return RT_OK;
}

// The seed plane of the direct stage (DevFrame::seedIn / seedOut) holds indices into the tree's leaf records: whatever changes their order or count — a new
// scene, a host build, a device rebuild — and rt_resize empty it, on the context's stream (the direct stages run there), so that two contexts that issue
// the same calls trace the same steps and report the same counters.  The refit paths (rt_update_instances / _vertices / _skins) keep record indices: the
// plane stays warm across them.  Nothing but speed depends on its contents (traverse.h traceRaySeeded).
static int resetSeedPlane(rt_ctx* c)
{
  if(!c->scratch.seedOut || c->W <= 0) return RT_OK;
  RT_HIP(c, hipMemsetAsync(c->scratch.seedOut, 0xff, size_t(c->W) * size_t(c->H) * sizeof(uint32_t), c->stream));
  return RT_OK;
}

int rt_upload_scene(rt_ctx* c, const rt_scene_desc* d)
{
  if(!c) return RT_ERR_INVALID_ARG;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  if(!d || !d->primMeshes || !d->vertices || !d->indices || !d->instances || !d->materials || d->numMaterials == 0)
    return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: missing geometry/material arrays");
  for(uint32_t i = 0; i < d->numInstances; i++)
    if(d->instances[i].primMesh >= d->numPrimMeshes) return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: instance references a missing prim mesh");
  for(uint32_t i = 0; i < d->numPrimMeshes; i++) {
    const rt_prim_mesh& pm = d->primMeshes[i];
    if(uint64_t(pm.firstIndex) + pm.indexCount > d->numIndices || uint64_t(pm.vertexOffset) + pm.vertexCount > d->numVertices || pm.indexCount % 3 != 0)
      return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: prim mesh range out of bounds");
    if(pm.materialIndex >= int32_t(d->numMaterials)) return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: material index out of range");
    for(uint32_t k = 0; k < pm.indexCount; k++)
      if(d->indices[pm.firstIndex + k] >= pm.vertexCount) return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: vertex index beyond the prim mesh's vertex range");
  }
  // everything the kernels use as an array index is checked here: a bad id must come back as an error, not as a GPU fault
  const int32_t nTex = d->textures ? int32_t(d->numTextures) : 0;
  for(uint32_t i = 0; i < d->numMaterials; i++)
    if(const char* why = checkMaterialRow(d->materials[i], nTex)) return fail(c, RT_ERR_INVALID_ARG, (std::string("rt_upload_scene: ") + why).c_str());
  if(d->trigLights)
    for(uint32_t i = 0; i < d->lightInfo.trigLightSize; i++)
      if(d->trigLights[i].matIndex >= d->numMaterials || d->trigLights[i].impSamp.alias < 0 || uint32_t(d->trigLights[i].impSamp.alias) >= d->lightInfo.trigLightSize)
        return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: triangle light with a bad material or alias index");
  if(d->puncLights)
    for(uint32_t i = 0; i < d->lightInfo.puncLightSize; i++)
      if(d->puncLights[i].impSamp.alias < 0 || uint32_t(d->puncLights[i].impSamp.alias) >= d->lightInfo.puncLightSize)
        return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: punctual light with a bad alias index");
  if(d->envRgba32f && d->envAccel && d->envWidth > 0 && d->envHeight > 0) {
    const int64_t n = int64_t(d->envWidth) * d->envHeight;
    for(int64_t i = 0; i < n; i++)
      if(d->envAccel[i].alias < 0 || d->envAccel[i].alias >= n) return fail(c, RT_ERR_INVALID_ARG, "rt_upload_scene: environment alias table entry out of range");
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  LoadTimer lt;
  freePool(c->sceneAllocs); freePool(c->accelAllocs); freePool(c->rebuildAllocs);
  freePool(c->skinAllocs); freePool(c->deformAllocs);   // a new scene has no skins
  freePool(c->morphAllocs);   // ... and no morph sets
  c->morph = rt_ctx::Morph{}; c->skinMats.clear();
  freePool(c->lightAllocs);   // ... and no light-source binding
  c->lights = rt_ctx::Lights{};
  dropEmitters(c);            // ... and no emitter mode
  freePool(c->instAllocs);    // ... and no instance templates
  c->inst = rt_ctx::InstTemplates{};
  freePool(c->matAllocs);     // ... and the material edits' device words are sized again
  c->mat = rt_ctx::Materials{};
  c->numTextures = uint32_t(nTex); c->hostNumAlpha = 0;
  freeEnvironment(c);         // ... and the environment is the scene's own again
  c->deform = rt_ctx::Deform{};
  c->refit = rt_ctx::Refit{};
  c->rebuild = rt_ctx::Rebuild{};
  c->haveScene = c->haveAccel = false;
  c->refN = 0;   // a new scene: the reference sums start again
  invalidateHistories(c);
  c->omPrev.clear(); c->omMoved.clear(); c->omPending = false;   // object motion: nothing of the new scene has moved
  if(c->vmPlane) { (void)hipFree(c->vmPlane); c->vmPlane = nullptr; }   // ... or has been deformed; the plane is made again for the new vertex array below
  c->vmDeformed.clear(); c->vmPending = false;
  c->ds = DevScene{};
  c->ds.sky = (c->sunAndSky.in_use == 1) ? static_cast<const SkyPre*>(c->dSky) : nullptr;
  c->primMeshes.assign(d->primMeshes, d->primMeshes + d->numPrimMeshes);
  c->vertices.assign(d->vertices, d->vertices + d->numVertices);
  c->indices.assign(d->indices, d->indices + d->numIndices);
  c->instances.assign(d->instances, d->instances + d->numInstances);
  c->materials.assign(d->materials, d->materials + d->numMaterials);

  int rc;
  if((rc = upload(c, c->sceneAllocs, d->primMeshes, d->numPrimMeshes, &c->ds.primMeshes))) return rc;
  if((rc = upload(c, c->sceneAllocs, d->vertices, size_t(d->numVertices), &c->ds.vertices))) return rc;
  if((rc = upload(c, c->sceneAllocs, d->indices, size_t(d->numIndices), &c->ds.indices))) return rc;
  if((rc = upload(c, c->sceneAllocs, d->materials, d->numMaterials, &c->ds.materials))) return rc;
  if((rc = upload(c, c->sceneAllocs, d->puncLights, d->puncLights ? d->lightInfo.puncLightSize : 0, &c->ds.puncLights))) return rc;
  if((rc = upload(c, c->sceneAllocs, d->trigLights, d->trigLights ? d->lightInfo.trigLightSize : 0, &c->ds.trigLights))) return rc;
  c->ds.lightInfo = d->lightInfo;
  if(!d->puncLights) c->ds.lightInfo.puncLightSize = 0;
  if(!d->trigLights) c->ds.lightInfo.trigLightSize = 0;
  // textures (BGRA8, LOD 0)
  lt.lap("geometry copies + uploads");
  c->hostAlpha.clear();
  std::vector<const uint8_t*> alphaSrc;
  std::vector<DevTexture> texs(std::max<uint32_t>(d->numTextures, 1));
  static const uint8_t white[4] = {255, 255, 255, 255};
  for(uint32_t i = 0; i < uint32_t(texs.size()); i++) {
    rt_texture t{white, 1, 1, RT_WRAP_REPEAT, RT_WRAP_REPEAT, RT_FILTER_LINEAR, 0};
    if(i < d->numTextures && d->textures && d->textures[i].bgra8 && d->textures[i].width > 0 && d->textures[i].height > 0) t = d->textures[i];
    const uint8_t* dp = nullptr;
    if((rc = upload(c, c->sceneAllocs, t.bgra8, size_t(t.width) * t.height * 4, &dp))) return rc;
    texs[i] = DevTexture{dp, t.width, t.height, t.wrapS, t.wrapT, t.magFilter, 0};
    c->hostAlpha.emplace_back(size_t(t.width) * t.height);
    alphaSrc.push_back(t.bgra8);
  }
  lt.lap("texture uploads");
  {  // the alpha planes (opacity micro-map build) and their hashes (rt_build_accel's cache key), one task per texture on the host's cores: 0.87 G byte-strided
     // copies + a hash of them took 1.1 s of the headline scene's load on one core (round 6)
    c->alphaHash.assign(c->hostAlpha.size(), {0ull, 0ull});
    std::atomic<size_t> next{0};
    auto work = [&] {
      for(;;) {
        const size_t i = next.fetch_add(1);
        if(i >= c->hostAlpha.size()) return;
        std::vector<uint8_t>& a = c->hostAlpha[i];
        const uint8_t* src = alphaSrc[i];
        for(size_t k = 0; k < a.size(); k++) a[k] = src[k * 4 + 3];
        uint64_t h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull;
        hashBytes(a.data(), a.size(), h0, h1);
        c->alphaHash[i] = {h0, h1};
      }
    };
    const size_t nt = std::min<size_t>(c->hostAlpha.size(), size_t(rt_cpu_budget()));
    std::vector<std::thread> pool;
    for(size_t k = 1; k < nt; k++) pool.emplace_back(work);
    work();
    for(auto& th : pool) th.join();
  }
  lt.lap("alpha planes + hashes");
  if((rc = upload(c, c->sceneAllocs, texs.data(), texs.size(), &c->ds.textures))) return rc;
  c->devTextures = texs;
  // environment
  if(d->envRgba32f && d->envWidth > 0 && d->envHeight > 0) {
    const size_t n = size_t(d->envWidth) * d->envHeight;
    if((rc = upload(c, c->sceneAllocs, d->envRgba32f, n * 4, &c->ds.env))) return rc;
    if(d->envAccel) { if((rc = upload(c, c->sceneAllocs, d->envAccel, n, &c->ds.envAccel))) return rc; }
    else {
      std::vector<rt_impt_samp> a(n, rt_impt_samp{0, 1.0f, 0.0f, 0.0f});
      if((rc = upload(c, c->sceneAllocs, a.data(), n, &c->ds.envAccel))) return rc;
    }
    c->ds.envW = d->envWidth; c->ds.envH = d->envHeight;
  } else {
    const float black[4] = {0, 0, 0, 0};
    const rt_impt_samp one{0, 1.0f, 0.0f, 0.0f};
    if((rc = upload(c, c->sceneAllocs, black, 4, &c->ds.env))) return rc;
    if((rc = upload(c, c->sceneAllocs, &one, 1, &c->ds.envAccel))) return rc;
    c->ds.envW = c->ds.envH = 1;
  }
  RT_HIP(c, hipDeviceSynchronize());
  c->haveScene = true;
  reopenPriorityDecision(c);   // (the context is drained: syncAll above / hipDeviceSynchronize below)
  if(c->vmEver && (rc = allocVertexMotionPlane(c))) return rc;
  return resetSeedPlane(c);
}


static void hashBytes(const void* p, size_t n, uint64_t& h0, uint64_t& h1)
{
  const unsigned char* b = static_cast<const unsigned char*>(p);
  size_t i = 0;
  for(; i + 8 <= n; i += 8) {
    uint64_t w; memcpy(&w, b + i, 8);
    h0 = (h0 ^ w) * 0x9E3779B97F4A7C15ull; h0 ^= h0 >> 29;
    h1 = (h1 + w) * 0xC2B2AE3D27D4EB4Full; h1 ^= h1 >> 31;
  }
  uint64_t w = 0; memcpy(&w, b + i, n - i); w |= uint64_t(n) << 56;
  h0 = (h0 ^ w) * 0x9E3779B97F4A7C15ull; h0 ^= h0 >> 29;
  h1 = (h1 + w) * 0xC2B2AE3D27D4EB4Full; h1 ^= h1 >> 31;
}
#define RT_HASH_VEC(v) do { const uint64_t n_ = (v).size(); hashBytes(&n_, 8, h0, h1); if(n_) hashBytes((v).data(), n_ * sizeof((v)[0]), h0, h1); } while(0)
static void sceneKey(const rt_ctx* c, uint64_t& h0, uint64_t& h1)
{
  h0 = 0x243F6A8885A308D3ull; h1 = 0x13198A2E03707344ull;
  RT_HASH_VEC(c->primMeshes); RT_HASH_VEC(c->vertices); RT_HASH_VEC(c->indices); RT_HASH_VEC(c->instances); RT_HASH_VEC(c->materials);
  for(size_t i = 0; i < c->devTextures.size(); i++) {
    const DevTexture& t = c->devTextures[i];
    const int meta[5] = {t.w, t.h, t.wrapS, t.wrapT, t.filter};
    hashBytes(meta, sizeof(meta), h0, h1);
    if(i < c->alphaHash.size()) { const uint64_t n_ = c->hostAlpha[i].size(); hashBytes(&n_, 8, h0, h1); hashBytes(c->alphaHash[i].data(), 16, h0, h1); }   // (hashed per texture at upload, in parallel)
  }
  // the builder's settings are part of what is cached: a host that changes RESTIR_BVH_* between two contexts of one process gets the tree it asked for, not the first
  // one's (advisor finding of round 5)
  for(const char* name : {"RESTIR_BVH_SPLIT", "RESTIR_BVH_SPLIT_BUDGET", "RESTIR_BVH_SPLIT_ALPHA", "RESTIR_BVH_SPLIT_WORK", "RESTIR_BVH_ROTATE", "RESTIR_BVH_ROTATE_GG",
                           "RESTIR_BVH_REINSERT", "RESTIR_BVH_PAR_MIN", "RESTIR_BVH_SEQ_MAX"}) {
    const char* v = getenv(name);
    hashBytes(name, strlen(name), h0, h1);
    if(v) hashBytes(v, strlen(v) + 1, h0, h1);
  }
}
#undef RT_HASH_VEC
// What HitTest needs for triangle `prim` of prim mesh `pm`, from the mesh's texcoords and material alone (never from an instance): the alpha record (without the
// texture address, which is per device: `tex` names the texture, -1 for none) and the opacity micro-map, cached per distinct (texture, uv triple, alpha parameters).
// rt_build_accel makes them per non-opaque leaf record, rt_set_instances per triangle of a prim mesh.
// (a hash map since round 6: 2 M lookups with 48-byte keys in a std::map were a second of the headline scene's load)
struct OmmKeyHash { size_t operator()(const std::array<uint32_t, 12>& k) const { uint64_t h = 1469598103934665603ull; for(uint32_t w : k) { h ^= w; h *= 1099511628211ull; } return size_t(h ^ (h >> 29)); } };
typedef std::unordered_map<std::array<uint32_t, 12>, std::array<uint32_t, 4>, OmmKeyHash> OmmCache;
static void alphaTemplate(const rt_ctx* c, const rt_prim_mesh& pm, uint32_t prim, OmmCache& ommCache, AlphaRec& a, int32_t& tex, std::array<uint32_t, 4>& omm)
{
  const rt_material& m = c->materials[size_t(pm.materialIndex > 0 ? pm.materialIndex : 0)];
  const uint32_t* ix = &c->indices[pm.firstIndex + 3 * prim];
  a = AlphaRec{};
  tex = -1;
  const rt_vec2 t0 = c->vertices[pm.vertexOffset + ix[0]].texcoord, t1 = c->vertices[pm.vertexOffset + ix[1]].texcoord, t2 = c->vertices[pm.vertexOffset + ix[2]].texcoord;
  a.uv0x = t0.x; a.uv0y = t0.y; a.uv1x = t1.x; a.uv1y = t1.y; a.uv2x = t2.x; a.uv2y = t2.y;
  a.baseAlpha = m.pbrBaseColorFactor.w; a.cutoff = m.alphaCutoff; a.alphaMode = m.alphaMode;
  if(m.pbrBaseColorTexture > -1 && size_t(m.pbrBaseColorTexture) < c->devTextures.size()) {
    const DevTexture& t = c->devTextures[size_t(m.pbrBaseColorTexture)];
    tex = m.pbrBaseColorTexture; a.w = t.w; a.h = t.h; a.wrapS = t.wrapS; a.wrapT = t.wrapT; a.filter = t.filter;
  }
  std::array<uint32_t, 12> key{};
  memcpy(key.data(), &a.uv0x, 8 * sizeof(float));
  key[8] = uint32_t(m.pbrBaseColorTexture); key[9] = uint32_t(a.alphaMode); key[10] = uint32_t(a.wrapS) ^ (uint32_t(a.wrapT) << 16); key[11] = uint32_t(a.filter);
  auto it = ommCache.find(key);
  if(it == ommCache.end()) {
    std::array<uint32_t, 4> o{};
    const std::vector<uint8_t>* al = (tex >= 0 && size_t(tex) < c->hostAlpha.size()) ? &c->hostAlpha[size_t(m.pbrBaseColorTexture)] : nullptr;
    buildOpacityMap(a, al, o.data());
    it = ommCache.emplace(key, o).first;
  }
  omm = it->second;
}

static int buildHostAccel(rt_ctx* c, HostAccel& out)
{
  LoadTimer lt;
  rt_scene_desc d{};
  d.numPrimMeshes = uint32_t(c->primMeshes.size()); d.primMeshes = c->primMeshes.data();
  d.numVertices = c->vertices.size(); d.vertices = c->vertices.data();
  d.numIndices = c->indices.size(); d.indices = c->indices.data();
  d.numInstances = uint32_t(c->instances.size()); d.instances = c->instances.data();
  BuildOutput& bo = out.bo;
  int threads = rt_cpu_budget();   // (the cgroup quota, not the machine: include/rt_cpus.h)
  if(!buildBvh8(d, bo, threads > 0 ? threads : 1)) return fail(c, RT_ERR_INVALID_ARG, "rt_build_accel: BVH8 build failed");
  if(bo.maxDepth > STACK_MAX) {
    // rotations and spatial splits can deepen a tree: before giving up, the tree of rounds 1-4 (object splits only), which would have built (advisor finding of round 5)
    bo = BuildOutput{};
    if(!buildBvh8(d, bo, threads > 0 ? threads : 1, true)) return fail(c, RT_ERR_INVALID_ARG, "rt_build_accel: BVH8 build failed");
  }
  if(bo.maxDepth > STACK_MAX) return fail(c, RT_ERR_INVALID_ARG, "rt_build_accel: BVH8 deeper than the traversal stack");
  lt.lap("buildBvh8");
  // alpha records for the triangles that go through HitTest (instances without FORCE_OPAQUE)
  std::vector<AlphaRec>& alpha = out.alpha; alpha.assign(1, AlphaRec{});
  std::vector<int32_t>& alphaTex = out.alphaTex; alphaTex.assign(1, -1);
  OmmCache ommCache;
  ommCache.reserve(1 << 16);
  std::vector<uint32_t> alphaOf;   // by globalId: the record of a triangle that has several references (spatial splits) is made once
  if(bo.tris.size() > bo.triRef.size()) alphaOf.assign(bo.triRef.size(), 0u);
  std::vector<std::array<uint32_t, 4>> ommOf;
  for(Tri48& T : bo.tris) {
    if(T.flags & TRI_OPAQUE) continue;
    if(!alphaOf.empty() && alphaOf[T.globalId]) { T.alphaIdx = alphaOf[T.globalId]; memcpy(T.omm, ommOf[T.alphaIdx].data(), sizeof(T.omm)); continue; }
    const TriRef ref = bo.triRef[T.globalId];
    AlphaRec a{};
    int32_t tex = -1;
    std::array<uint32_t, 4> omm{};
    alphaTemplate(c, c->primMeshes[c->instances[ref.inst].primMesh], ref.prim, ommCache, a, tex, omm);
    T.alphaIdx = uint32_t(alpha.size());
    alpha.push_back(a); alphaTex.push_back(tex);
    memcpy(T.omm, omm.data(), sizeof(T.omm));
    if(!alphaOf.empty()) { alphaOf[T.globalId] = T.alphaIdx; ommOf.resize(alpha.size()); ommOf[T.alphaIdx] = omm; }
  }
  lt.lap("alpha records + micro-maps");
  return RT_OK;
}

int rt_build_accel(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_build_accel: no scene uploaded");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  { const int rc = syncHostVertices(c); if(rc) return rc; }   // the build and its cache key read the context's copy: skinned meshes are current on the device only
  freePool(c->accelAllocs); freePool(c->rebuildAllocs);
  c->refit = rt_ctx::Refit{};
  c->rebuild = rt_ctx::Rebuild{};
  c->haveAccel = false;
  c->refN = 0;
  invalidateHistories(c);
  // Host products (BVH8, alpha records, opacity micro-maps): built once per distinct scene in this process and shared by every context that uploads
  // the same scene — the N ranks of an rt_mgpu context, or an application's contexts on several devices (1.4-1.6 s per build at 2.8 M triangles).
  std::shared_ptr<const HostAccel> ha;
  LoadTimer lt;
  {
    std::lock_guard<std::mutex> one(g_accelMutex);   // also: one multi-threaded host build at a time
    uint64_t k0, k1;
    sceneKey(c, k0, k1);
    lt.lap("scene key");
    if(g_accelCache && g_accelCache->key0 == k0 && g_accelCache->key1 == k1) ha = g_accelCache;
    else {
      auto fresh = std::make_shared<HostAccel>();
      fresh->key0 = k0; fresh->key1 = k1;
      const int rc = buildHostAccel(c, *fresh);
      if(rc) return rc;
      ha = fresh; g_accelCache = ha;
    }
  }
  lt.lap("host products (build or cache)");
  const BuildOutput& bo = ha->bo;
  int rc;
  {
    std::vector<AlphaRec> alpha = ha->alpha;   // texture addresses are per device
    for(size_t i = 0; i < alpha.size(); i++) if(ha->alphaTex[i] >= 0) alpha[i].bgra = c->devTextures[size_t(ha->alphaTex[i])].bgra;
    if((rc = upload(c, c->accelAllocs, alpha.data(), alpha.size(), &c->ds.alphaRec))) return rc;
    c->hostNumAlpha = alpha.size();
    // the latency build's copy, addressable without the triangle record (one dependent access less per alpha candidate); 64 B per triangle
    std::vector<AlphaRec> byTri(bo.tris.size(), AlphaRec{});
    for(size_t i = 0; i < bo.tris.size(); i++) if(!(bo.tris[i].flags & TRI_OPAQUE)) byTri[i] = alpha[bo.tris[i].alphaIdx];
    if((rc = upload(c, c->accelAllocs, byTri.data(), byTri.size(), &c->ds.alphaByTri))) return rc;
  }
  if((rc = upload(c, c->accelAllocs, bo.nodes.data(), bo.nodes.size(), &c->ds.nodes))) return rc;
  if((rc = upload(c, c->accelAllocs, bo.tris.data(), bo.tris.size(), &c->ds.tris))) return rc;
  if((rc = upload(c, c->accelAllocs, bo.triRef.data(), bo.triRef.size(), &c->ds.triRef))) return rc;
  if((rc = upload(c, c->accelAllocs, bo.instances.data(), bo.instances.size(), &c->ds.instances))) return rc;
  c->ds.numNodes = uint32_t(bo.nodes.size()); c->ds.numTris = uint32_t(bo.tris.size());
  // traversal stack: what a ray of this tree can need.  How much of it each lane keeps in LDS is a per-launch choice (stackLdsEntries below): with frames
  // in flight 6 entries = 3 KB per wave (measured, profiles/r02_short_stack_ab.txt), deeper entries in a per-thread area in HBM (ensureStackOverflow);
  // serial schedules have the LDS to themselves and keep the whole stack there.  RESTIR_STACK_LDS=<n> forces n entries in every schedule.
  c->ds.stackTotal = std::max(8, ((bo.maxDepth + 1 + 3) / 4) * 4);
  c->ds.stackEntries = c->ds.stackTotal;   // the launchers shorten it per launch (DevFrame::stackLds)
  c->ds.triPad = bo.pad;
  { const char* e = getenv("RESTIR_COOP"); c->ds.coopLive = e ? std::max(0, std::min(64, atoi(e))) : 4; }
  { const char* e = getenv("RESTIR_WIDE_TAIL"); c->ds.wideTail = e ? std::max(0, std::min(8, atoi(e))) : 8; }   // throughput build: the last rays of a dry ray pool, eight lanes per ray (traverse.h wideTail)
  { const char* e = getenv("RESTIR_GANG"); c->ds.gangMax = e ? std::max(0, std::min(7, atoi(e))) : 4; }   // latency build: gang mode for the last rays of a wave (traverse.h)
  c->numNodes = bo.nodes.size(); c->numTris = bo.triRef.size(); c->maxDepth = bo.maxDepth;
  c->numRefs = bo.tris.size(); c->spatialSplits = size_t(bo.spatialSplits); c->sahNodeSteps = bo.sahNodeSteps; c->sahTriSteps = bo.sahTriSteps;
  RT_HIP(c, hipDeviceSynchronize());
  lt.lap("uploads (tree, alpha records)");
  c->haveAccel = true;
  reopenPriorityDecision(c);
  if((rc = resetSeedPlane(c))) return rc;
  return ensureStackOverflow(c);
}

int rt_resize(rt_ctx* c, int w, int h)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(w <= 0 || h <= 0 || w > 32767 || h > 32767) return fail(c, RT_ERR_INVALID_ARG, "rt_resize: size must be in 1..32767 (RG16_SINT motion vectors)");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  reopenPriorityDecision(c);
  for(void*& p : c->indA) { if(p && p != c->bufs[RT_BUF_DENOISE_IND_A]) (void)hipFree(p); p = nullptr; }
  for(int i = 0; i < RT_BUF_COUNT; i++) { if(c->bufs[i]) (void)hipFree(c->bufs[i]); c->bufs[i] = nullptr; c->bufBytes[i] = 0; }
  freeSpares(c, {rt_ctx::RING_G, rt_ctx::RING_MOTION, rt_ctx::RING_DIRECT});   // (freeObjectMotion: the other two kinds)
  c->W = c->H = 0;
  for(void* p : {static_cast<void*>(c->refAcc), static_cast<void*>(c->refMean)}) if(p) (void)hipFree(p);
  c->refAcc = nullptr; c->refMean = nullptr; c->refN = 0;
  freeHistory(c->histSvgf);
  freeGiSpatial(c);
  freeHistory(c->histTaa);
  freeUpscaleHistory(c);
  freeObjectMotion(c);
  freeVis(c);
  const size_t n = size_t(w) * h, nh = size_t(w / 2) * (h / 2);
  for(int i = 0; i < RT_BUF_COUNT; i++) {
    const size_t bytes = (halfRes(i) ? nh : n) * elemBytes(i);
    const size_t alloc = bytes + (halfRes(i) ? size_t(w / 2) * (RT_PAD_ROWS / 2) : size_t(w) * RT_PAD_ROWS) * elemBytes(i) + 16;
    RT_HIP(c, hipMalloc(&c->bufs[i], alloc));
    RT_HIP(c, hipMemset(c->bufs[i], (i == RT_BUF_LIGHT_ID0 || i == RT_BUF_LIGHT_ID1) ? 0xff : 0, alloc));
    c->bufBytes[i] = bytes; c->bufAlloc[i] = alloc;
    if(i == RT_BUF_DENOISE_IND_A) {  // the second parity of the noisy indirect colour
      c->indA[0] = c->bufs[i];
      RT_HIP(c, hipMalloc(&c->indA[1], alloc));
      RT_HIP(c, hipMemset(c->indA[1], 0, alloc));
    }
    // rotation partners for frames in flight (rt_render_frame, overlap 2): two of the G-buffer and of the motion buffer, and one of the direct image (overlap 3:
    // the direct image of frame f-3 is the one direct(f) overwrites)
    const int kind = i == RT_BUF_GBUFFER0 ? rt_ctx::RING_G : (i == RT_BUF_MOTION ? rt_ctx::RING_MOTION : (i == RT_BUF_DIRECT_RESULT0 ? rt_ctx::RING_DIRECT : -1));
    for(int s = 0; kind >= 0 && s < (kind == rt_ctx::RING_DIRECT ? 1 : 2); s++) RT_HIP(c, mallocFilled(&c->spare[kind][s], alloc, 0));
  }
  // internal scratch
  freePool(c->scratchAllocs);
  c->scratch = DevFrame{};
  auto alloc = [&](size_t bytes, void** out) -> int {
    RT_HIP(c, hipMalloc(out, std::max<size_t>(bytes, 256)));
    c->scratchAllocs.push_back(*out);
    RT_HIP(c, hipMemset(*out, 0, std::max<size_t>(bytes, 256)));
    return RT_OK;
  };
  DevFrame& X = c->scratch;
  int rc;
#define RT_SCRATCH(field, count, T) if((rc = alloc(size_t(count) * sizeof(T), reinterpret_cast<void**>(&X.field)))) return rc
  RT_SCRATCH(surf, n, SurfRec); RT_SCRATCH(status, n, uint32_t); RT_SCRATCH(qcount, 256, uint32_t);
  RT_SCRATCH(geomN, n, float4); RT_SCRATCH(geomP, n, float4); RT_SCRATCH(geomNh, nh, float4); RT_SCRATCH(geomPh, nh, float4);
  RT_SCRATCH(postRowSums, size_t(h) * 6, double); RT_SCRATCH(postMean, 8, float);
  RT_SCRATCH(postMipD, n + 64, float4); RT_SCRATCH(postMipI, n + 64, float4);   // levels 1..7 (n/3 texels; up to n for one-pixel-wide images)
  RT_SCRATCH(tileOrder, (size_t(w / 2 + 7) / 8) * (size_t(h / 2 + 7) / 8 + 16 * 2) + 64 + 4096, uint32_t);   // 8 per-XCD lists: tiles + one chunk of slack each
  RT_SCRATCH(seedOut, n, uint32_t); X.seedIn = X.seedOut;   // the direct stage's seed plane: read and written in place (dev_scene.h)
#if RT_WAVEPROF
  RT_SCRATCH(waveProf, WAVEPROF_RECORDS * 16, uint32_t);
#endif
#undef RT_SCRATCH
  RT_HIP(c, hipDeviceSynchronize());  // memsets above ran on the null stream; the ctx stream does not wait for it implicitly
  c->W = w; c->H = h;
  if((rc = resetSeedPlane(c))) return rc;
  if((c->objMotion != RT_OBJECT_MOTION_OFF || c->vmEver) && (rc = allocObjectMotion(c))) return rc;
  return ensureStackOverflow(c);
}

// Overflow part of the traversal stacks (DevScene::stackOvf): (stackTotal - stackEntries) entries for every thread of the largest traced launch of
// this frame size, one area per stage kind.  Only schedules that shorten the LDS stack touch them (frames in flight, RESTIR_STACK_LDS), so they are
// allocated when such a schedule is selected and (re)sized when the tree or the frame size changes; a serial ctx (every rt_mgpu rank of the barrier
// schedule) holds none.  Callers have drained the ctx.
static int ensureStackOverflow(rt_ctx* c)
{
  freePool(c->ovfAllocs);
  c->ds.stackOvf = c->ds.stackOvfInd = nullptr; c->ds.stackOvfThreads = 0;
  if(!(stackLdsEnv() || c->overlap >= 2)) return RT_OK;
  if(!c->haveAccel || c->W <= 0 || c->ds.stackTotal <= stackLdsMin()) return RT_OK;
  const size_t tilesX = size_t(c->W + 7) / 8, tilesY = size_t(c->H + 7) / 8;
  const size_t blocks = std::max<size_t>(16384, tilesX * tilesY + 8 * tilesX + 1024);   // >= any traced grid: tileGrid() of the full frame; 4 waves per half-res tile
  const size_t bytes = blocks * 64 * size_t(c->ds.stackTotal - stackLdsMin()) * sizeof(uint2);
  void* p[2] = {nullptr, nullptr};
  for(int i = 0; i < 2; i++) { RT_HIP(c, hipMalloc(&p[i], bytes)); c->ovfAllocs.push_back(p[i]); }
  c->ds.stackOvf = static_cast<uint2*>(p[0]); c->ds.stackOvfInd = static_cast<uint2*>(p[1]);
  c->ds.stackOvfThreads = uint32_t(blocks * 64);
  return RT_OK;
}

int rt_set_camera(rt_ctx* c, const rt_scene_camera* cam)
{
  if(!c || !cam) return RT_ERR_INVALID_ARG;
  // the reference sums belong to one view: a new viewInverse / projInverse resets them (the history matrices move every frame and do not)
  if(std::memcmp(&c->cam.viewInverse, &cam->viewInverse, sizeof(rt_mat4)) != 0 || std::memcmp(&c->cam.projInverse, &cam->projInverse, sizeof(rt_mat4)) != 0) c->refN = 0;
  c->cam = *cam;
  return RT_OK;
}

static void selectFrame(rt_ctx* c, int frames) { if(c->indA[0]) c->bufs[RT_BUF_DENOISE_IND_A] = c->indA[frames & 1]; }

// The two extra streams of rt_render_frame's overlapped schedules, created on first use: a host that drives the stages itself (rt_run_stage on its own streams:
// rt_mgpu, tiled.py) never needs them, and every stream of a process takes one of the device's few hardware queues (4 by default) out of the rotation.
// Stream priorities of the frames-in-flight schedule: prioSpec() above (RESTIR_PRIO).  Default: indirect stream high (measured 2 % faster than indirect + filter
// streams high on the lite config 4, round 2).
static hipError_t ensureOverlapStreams(rt_ctx* c)
{
  if(c->sideStream && c->indStream) return hipSuccess;
  hipError_t e = hipSuccess;
  hipStream_t& side = c->sideStreams[c->prio[2] + 1];
  hipStream_t& ind = c->indStreams[c->prio[1] + 1];
  if(!side) { e = createStreamLevel(&side, c->prio[2]); if(e == hipSuccess) c->sideIdx[c->prio[2] + 1] = g_streamsCreated.load() - 1; }
  if(e == hipSuccess && !ind) { e = createStreamLevel(&ind, c->prio[1]); if(e == hipSuccess) c->indIdx[c->prio[1] + 1] = g_streamsCreated.load() - 1; }
  c->sideStream = side; c->indStream = ind;
  return e;
}

// The rule of rt_render_frame's probe frames (see there).  RESTIR_PRIO_PROBE = number of probe frames (default 3; 1 = round 5's first-frame decision).
static constexpr float PRIO_FILTER_SHARE = 0.30f;   // (restir_amd/renderer.py mirrors it for reports)
static int prioProbeFrames() { static const int n = getenv("RESTIR_PRIO_PROBE") ? std::max(1, atoi(getenv("RESTIR_PRIO_PROBE"))) : 3; return n; }
// what the decision was taken on has changed (target size, scene, tree, denoise toggle): the next frames probe again.  The streams of the old levels stay alive, idle
// (one per role and level, never destroyed: see rt_ctx::indStreams); the caller has drained the context.
static void reopenPriorityDecision(rt_ctx* c)
{
  if(c->prioExplicit || c->prioFromEnv) return;
  c->prioDecided = false; c->filterShare = -1.f; c->probeFrames = 0; c->denoiseSeen = -1;
  c->prio[1] = 1; c->prio[2] = 0;
  c->indStream = c->sideStream = nullptr;
}

// the arguments of one SVGF chain of frame `frames` (ind: the half-resolution indirect component)
static SvgfArgs svgfArgs(const rt_ctx* c, const DevFrame& F, const rt_state& st, int frames, bool ind, bool histValid)
{
  SvgfArgs A{};
  const int k = ind ? 1 : 0;
  void* const* cur = c->histSvgf.plane[rt::frameParity(frames)]; void* const* prev = c->histSvgf.plane[rt::otherParity(frames)];
  A.thisG = F.thisG; A.lastG = F.lastG; A.motion = F.motion;
  A.noisy = ind ? F.denoiseIndA : F.thisDirectResult;
  // the A-Trous temporaries: direct DirA <-> DirB; indirect thisIndirectResult (scratch, as in the A-Trous chain) <-> the noisy buffer, read by then
  A.bufA = ind ? F.thisIndirectResult : F.denoiseDirA;
  A.bufB = ind ? F.denoiseIndA : F.denoiseDirB;
  A.out = ind ? F.denoiseIndB : F.thisDirectResult;
  A.geomN = ind ? F.geomNh : F.geomN; A.geomP = ind ? F.geomPh : F.geomP;
  A.prevC = static_cast<const float4*>(prev[k]); A.prevM = static_cast<const float2*>(prev[2 + k]);
  A.histC = static_cast<float4*>(cur[k]); A.histM = static_cast<float2*>(cur[2 + k]);
  A.W = c->W; A.H = c->H;
  A.bx = ind ? c->W / 2 : c->W; A.by = ind ? c->H / 2 : c->H;
  A.histValid = histValid ? 1 : 0;
  A.cap = c->den.historyCap;
  A.alphaC = c->den.alphaColor; A.alphaM = c->den.alphaMoments;
  A.phiLum = ind ? c->den.phiLumIndirect : c->den.phiLumDirect;
  A.sigN = ind ? st.sigNormalIndirect : st.sigNormalDirect;
  A.sigD = ind ? st.sigDepthIndirect : st.sigDepthDirect;
  return A;
}

// The GI spatial reservoirs (rt_render_frame's first frame with the mode on; the caller has drained the context)
static int allocGiSpatial(rt_ctx* c)
{
  const size_t bytes = std::max<size_t>(size_t(c->W / 2) * (c->H / 2) * sizeof(rt_indirect_reservoir), 256);
  if(hipMalloc(&c->gisResv, bytes) != hipSuccess) { c->gisResv = nullptr; return fail(c, RT_ERR_OOM, "rt_render_frame: hipMalloc of the GI spatial reservoirs failed"); }
  RT_HIP(c, hipMemset(c->gisResv, 0, bytes));
  RT_HIP(c, hipDeviceSynchronize());
  c->gisWritten = false;
  return RT_OK;
}

// the arguments of a frame's GI spatial pass
static GiSpatialArgs giSpatialArgs(const rt_ctx* c, const DevFrame& F)
{
  GiSpatialArgs A{};
  A.thisG = F.thisG; A.resv = F.thisIndirectResv;
  A.out = static_cast<rt_indirect_reservoir*>(c->gisResv);
  A.indA = F.denoiseIndA;
  A.W = c->W; A.H = c->H;
  A.mode = c->gis.mode; A.samples = c->gis.samples; A.radius = c->gis.radius;
  A.normalThreshold = c->gis.normalThreshold; A.depthThreshold = c->gis.depthThreshold; A.jacobianMax = c->gis.jacobianMax;
  return A;
}

// The instance images of rt_set_object_motion (callers have drained the context); they start as "miss everywhere"
static int allocObjectMotion(rt_ctx* c)
{
  const size_t n = size_t(c->W) * c->H;
  for(void** p : {&c->omInst, &c->spare[rt_ctx::RING_INST][0], &c->spare[rt_ctx::RING_INST][1]}) if(!*p) RT_HIP(c, mallocFilled(p, n * sizeof(uint32_t), 0xff));
  if(c->vmEver)   // the delta images of per-vertex motion vectors: zero = "nothing moved"
    for(void** p : {&c->vmDelta, &c->spare[rt_ctx::RING_DELTA][0], &c->spare[rt_ctx::RING_DELTA][1]}) if(!*p) RT_HIP(c, mallocFilled(p, n * sizeof(float4), 0));
  RT_HIP(c, hipDeviceSynchronize());
  return RT_OK;
}

// A per-instance device table of a motion-vector mode grows to `rows` rows: its readers are drained first, and the frame that asked rewrites every row.
static int growTable(rt_ctx* c, void** table, size_t* have, size_t rows, size_t rowBytes)
{
  if(*have >= rows) return RT_OK;
  RT_HIP(c, syncAll(c));
  if(*table) { (void)hipFree(*table); *table = nullptr; *have = 0; }
  RT_HIP(c, hipMalloc(table, rows * rowBytes));
  *have = rows;
  return RT_OK;
}

// The upsampling history at the output size with the RGBA8 target and the tonemap's scratch (rt_render_frame's first frame with the mode on; the caller has
// drained the context).  All or nothing; the history comes last, and its device synchronisation covers the rest.
static int allocUpscaleHistory(rt_ctx* c)
{
  const int wo = c->ups.outWidth, ho = c->ups.outHeight;
  const size_t n = size_t(wo) * ho;
  auto get = [](auto** p, size_t bytes) { return mallocFilled(reinterpret_cast<void**>(p), bytes, 0) == hipSuccess; };
  const bool ok = get(&c->upsLdr, n * 4) && get(&c->upsRowSums, size_t(ho) * 6 * sizeof(double)) && get(&c->upsMean, 8 * sizeof(float)) &&
                  get(&c->upsMipD, (n + 64) * sizeof(float4)) && get(&c->upsMipI, (n + 64) * sizeof(float4));   // (sized as rt_resize sizes the render-size ones)
  const int rc = ok ? allocHistory(c, c->histUps, {n * sizeof(float4), n * sizeof(float4), n * sizeof(float)}, "upsampling")
                    : fail(c, RT_ERR_OOM, "rt_render_frame: hipMalloc of the upsampling history failed");
  if(rc) { freeUpscaleHistory(c); return rc; }
  c->upsW = wo; c->upsH = ho; c->upsLdrWritten = false;
  return RT_OK;
}
// the ratio limits of rt_set_upscale for a render size
static bool upscaleRatioOk(int w, int h, int wo, int ho) { return wo >= w && ho >= h && int64_t(wo) <= 4 * int64_t(w) && int64_t(ho) <= 4 * int64_t(h); }

static DevFrame makeFrame(rt_ctx* c, int frames)
{
  selectFrame(c, frames);
  const int cur = rt::frameParity(frames), last = rt::otherParity(frames);  // m_descSet[(frames+1)%2]: this = [!i] (renderer.cpp:157, 346-356)
  DevFrame F{};
  F.stackLds = stackLdsEnv() ? stackLdsEnv() : (c->overlap >= 2 ? 6 : 0);
  F.thisG = static_cast<uint4*>(c->bufs[RT_BUF_GBUFFER0 + cur]); F.lastG = static_cast<const uint4*>(c->bufs[RT_BUF_GBUFFER0 + last]);
  F.motion = static_cast<short2*>(c->bufs[RT_BUF_MOTION]);
  F.thisDirectResv = static_cast<rt_direct_reservoir*>(c->bufs[RT_BUF_DIRECT_RESV0 + cur]);
  F.lastDirectResv = static_cast<const rt_direct_reservoir*>(c->bufs[RT_BUF_DIRECT_RESV0 + last]);
  F.thisIndirectResv = static_cast<rt_indirect_reservoir*>(c->bufs[RT_BUF_INDIRECT_RESV0 + cur]);
  F.lastIndirectResv = static_cast<const rt_indirect_reservoir*>(c->bufs[RT_BUF_INDIRECT_RESV0 + last]);
  F.tempDirectResv = static_cast<rt_direct_reservoir*>(c->bufs[RT_BUF_DIRECT_RESV_TEMP]);
  F.thisLightId = static_cast<uint32_t*>(c->bufs[RT_BUF_LIGHT_ID0 + cur]); F.lastLightId = static_cast<const uint32_t*>(c->bufs[RT_BUF_LIGHT_ID0 + last]);
  F.thisDirectResult = static_cast<float4*>(c->bufs[RT_BUF_DIRECT_RESULT0 + cur]);
  F.thisIndirectResult = static_cast<float4*>(c->bufs[RT_BUF_INDIRECT_RESULT0 + cur]);
  F.denoiseDirA = static_cast<float4*>(c->bufs[RT_BUF_DENOISE_DIR_A]); F.denoiseDirB = static_cast<float4*>(c->bufs[RT_BUF_DENOISE_DIR_B]);
  F.denoiseIndA = static_cast<float4*>(c->bufs[RT_BUF_DENOISE_IND_A]); F.denoiseIndB = static_cast<float4*>(c->bufs[RT_BUF_DENOISE_IND_B]);
  F.counters = c->counting ? c->dCounters : nullptr;
  F.W = c->W; F.H = c->H;
  const DevFrame& X = c->scratch;
  F.surf = X.surf; F.status = X.status; F.qcount = X.qcount; F.waveProf = X.waveProf;
  F.seedIn = X.seedIn; F.seedOut = X.seedOut;
  F.histRow0 = c->histRow0; F.histRow1 = c->histRow1; F.histMiss = X.qcount + 250;
  F.geomN = X.geomN; F.geomP = X.geomP; F.geomNh = X.geomNh; F.geomPh = X.geomPh; F.tileOrder = X.tileOrder; F.postRowSums = X.postRowSums; F.postMean = X.postMean;
  return F;
}

static int checkReady(rt_ctx* c, const rt_state* st)
{
  if(!c || !st) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "no scene uploaded");
  if(!c->haveAccel) return fail(c, RT_ERR_NO_ACCEL, "rt_build_accel has not been called");
  if(c->W == 0 || st->size.x != c->W || st->size.y != c->H) return fail(c, RT_ERR_NO_TARGET, "RtxState.size does not match rt_resize");
  return RT_OK;
}

int rt_run_stage(rt_ctx* c, const rt_state* st, int frames, int stage, int level, int rowBegin, int rowEnd)
{
  int rc = checkReady(c, st);
  if(rc) return rc;
  if(stage < 0 || stage >= RT_STAGE_COUNT) return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: unknown stage");
  if(c->den.mode == RT_DENOISER_SVGF && (stage == RT_STAGE_DENOISE_DIRECT || stage == RT_STAGE_DENOISE_INDIRECT))
    return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: the denoise stages are the A-Trous chain; this context is in SVGF mode (rt_set_denoiser), which only rt_render_frame runs");
  if(c->gis.mode != RT_GI_SPATIAL_OFF && stage == RT_STAGE_INDIRECT)
    return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: this context has GI spatial reuse on (rt_set_gi_spatial), whose pass after the indirect stage only rt_render_frame runs");
  if(c->taa.mode != RT_TAA_OFF)
    return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: this context has TAA on (rt_set_taa), whose jittered camera and resolve pass only rt_render_frame runs");
  if(c->ups.mode != RT_UPSCALE_OFF)
    return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: this context has temporal upsampling on (rt_set_upscale), whose jittered camera and resolve pass only rt_render_frame runs");
  if(rowBegin < 0 || (rowBegin & 7)) return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: rowBegin must be a non-negative multiple of 8");
  {  // levels: the filter chains have 4 / 5, the direct stage its two halves in the spatial modes, every other stage only level 0
    const bool spatial = st->ReSTIRState == RT_RESTIR_SPATIAL || st->ReSTIRState == RT_RESTIR_SPATIOTEMPORAL;
    const int maxLevel = stage == RT_STAGE_DENOISE_DIRECT ? 3 : (stage == RT_STAGE_DENOISE_INDIRECT ? 4 : ((stage == RT_STAGE_DIRECT && spatial) ? 2 : 0));
    if(level < 0 || level > maxLevel)
      return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: level out of range for this stage (RT_STAGE_DIRECT levels 1 / 2 exist in the spatial modes only)");
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, joinInFlight(c));
  DevFrame F = makeFrame(c, frames);
  if(stage == RT_STAGE_INDIRECT) F.histMiss = c->scratch.qcount + 251;  // per-stage-kind flag (rt_history_miss_stage)
  // (stage kinds share no scratch: a caller may spread them over several streams, tiled.PipelinedTiledFrame does)
  // (never a motion-vector build, whatever rt_set_object_motion says: the motion state belongs to rt_render_frame's frames)
  const hipError_t e = launchStageOn(c, c->stream, F, rt::StageExtra{}, rt::STAGE_MOTION_NONE, *st, c->cam, stage, level, rowBegin, rowEnd);
  if(e == hipErrorInvalidValue) return fail(c, RT_ERR_INVALID_ARG, "rt_run_stage: level out of range for this stage (RT_STAGE_DIRECT levels 1 / 2 exist in the spatial modes only)");
  if(e == hipErrorInvalidConfiguration) return fail(c, RT_ERR_HIP, "rt_run_stage: the traversal-stack overflow area is missing or too small for this launch (internal sizing error)");
  RT_HIP(c, e);
  return RT_OK;
}

int rt_render_frame(rt_ctx* c, const rt_state* st, int frames)
{
  int rc = checkReady(c, st);
  if(rc) return rc;
  if(c->ups.mode != RT_UPSCALE_OFF && !upscaleRatioOk(c->W, c->H, c->ups.outWidth, c->ups.outHeight))
    return fail(c, RT_ERR_INVALID_ARG, "rt_render_frame: temporal upsampling is on (rt_set_upscale) and the render size rt_resize set no longer satisfies W <= outWidth <= 4 W, H <= outHeight <= 4 H");
  RT_HIP(c, hipSetDevice(c->device));
  if(c->evUsed == rt_ctx::MAX_SETS) { RT_HIP(c, syncAll(c)); harvestTimings(c); }
  if(c->evUsed == c->evSets.size()) {
    rt_ctx::EvSet E{};
    for(int i = 0; i < rt_ctx::MAX_EV; i++) RT_HIP(c, hipEventCreate(&E.ev[i]));
    c->evSets.push_back(E);
  }
  // The first PRIO_PROBE_FRAMES frames of a frames-in-flight context ("probe frames") run every stage alone on the main stream and are timed; the LAST of them — warm
  // caches, warm history, the steady state's ray lengths — decides the priorities of the two other streams BEFORE they are created (below): filter stream high as
  // well when the filter chain is a sizeable part of the frame's work.  Round 5 decided on frame 0 alone (cold history; threshold 0.14 with the real scene 10 % from
  // the edge).  Warm shares and the setting that is fastest (profiles/r06_prio_rule.txt, every cell a fresh process): real exterior scene 0.16 -> (1,0); the same scene
  // seen from above across the street 0.26 -> (1,0) by 5 %; lite 0.24 -> (1,1) by 1.6 %; interior 4K 0.41, 15 degrees off axis 0.43, config 3 0.53 -> (1,1) by 6-9 %.
  // No threshold gets lite and the elevated view both right; 0.30 errs towards the indirect stream alone, which costs 1.6 % where it is wrong (0.20 cost 4.9 %).  A camera
  // that starts at the expensive pose and moves off it (bench.py --moving-camera) is judged on its first three frames and keeps (1,0): 2.9 % slower than (1,1) once the
  // view has become cheap — a host that knows its workload says so (rt_set_stream_priorities).  The decision has to precede the streams: a stream's place in the process's
  // creation order changes what the schedule gets out of it (a setting introduced after another one's streams exist ran 15-45 % slower than in a fresh process,
  // profiles/r05_prio_by_config_ab.txt), so settings cannot be compared in place — and cannot be switched later for free either.  A new target size, a new scene / tree
  // or a denoise toggle re-opens the decision (reopenPriorityDecision); an explicit rt_set_stream_priorities / RESTIR_PRIO closes it for good.
  if(c->prioDecided && !c->prioExplicit && !c->prioFromEnv && c->denoiseSeen >= 0 && (st->denoise > 0) != (c->denoiseSeen > 0)) { RT_HIP(c, syncAll(c)); reopenPriorityDecision(c); }
  // SVGF (rt_set_denoiser) replaces both A-Trous chains at their place in every schedule; its history is allocated by the first frame that needs it
  const bool svgf = c->den.mode == RT_DENOISER_SVGF && st->denoise > 0;
  const size_t nPix = size_t(c->W) * c->H, nHalf = size_t(c->W / 2) * (c->H / 2);
  if(svgf && !c->histSvgf.plane[0][0]) {
    RT_HIP(c, syncAll(c));
    if((rc = allocHistory(c, c->histSvgf, {nPix * sizeof(float4), nHalf * sizeof(float4), nPix * sizeof(float2), nHalf * sizeof(float2)}, "SVGF"))) return rc;
  }
  // GI spatial reuse (rt_set_gi_spatial): a pass right after the indirect stage on its stream in every schedule; its reservoirs are allocated by the first frame that needs them
  const bool gis = c->gis.mode != RT_GI_SPATIAL_OFF;
  if(gis && !c->gisResv) { RT_HIP(c, syncAll(c)); if((rc = allocGiSpatial(c))) return rc; }
  // TAA (rt_set_taa): frames with debugging_mode == 0 are rendered with the jittered camera and resolved by a pass right after compose on its stream in every
  // schedule; its history is allocated by the first frame that needs it
  const bool taa = c->taa.mode == RT_TAA_ON && st->debugging_mode == 0;
  if(taa && !c->histTaa.plane[0][0]) {
    RT_HIP(c, syncAll(c));
    if((rc = allocHistory(c, c->histTaa, {nPix * sizeof(float4), nPix * sizeof(float4), nPix * sizeof(float)}, "TAA"))) return rc;
  }
  rt_scene_camera cam = c->cam;   // the camera of this frame's launches (c->cam stays what rt_set_camera stored)
  if(taa) (void)rt_taa_jitter_camera(&c->cam, frames, c->taa.jitterPhases, c->W, c->H, &cam);
  // Temporal upsampling (rt_set_upscale; never together with TAA): the same, with its own jitter phases and a resolve into a history at the output size
  const bool ups = c->ups.mode == RT_UPSCALE_TEMPORAL && st->debugging_mode == 0;
  if(ups && (!c->histUps.plane[0][0] || c->upsW != c->ups.outWidth || c->upsH != c->ups.outHeight)) {
    RT_HIP(c, syncAll(c));
    freeUpscaleHistory(c);
    if((rc = allocUpscaleHistory(c))) return rc;
  }
  float upsDelta[2] = {0.0f, 0.0f};
  if(ups) (void)rt_upscale_jitter_camera(&c->cam, frames, c->ups.jitterPhases, c->W, c->H, &cam, upsDelta);
  // Object motion vectors (rt_set_object_motion): the direct and the indirect stage come from the RT_OM builds, which write / read the instance image; when an
  // instance is in motion they also read the per-instance camera table, filled here and uploaded ahead of the direct stage on its stream (below)
  const bool om = c->objMotion == RT_OBJECT_MOTION_ON && !c->counting && c->omInst;
  bool omMotion = false;
  if(c->objMotion == RT_OBJECT_MOTION_ON) {
    const size_t nInst = c->instances.size();
    if(c->omPending) for(size_t i = 0; i < nInst && !omMotion; i++) omMotion = c->omMoved[i] && std::memcmp(c->omPrev[i].data(), c->instances[i].objectToWorld, 48) != 0;
    if(omMotion && c->counting)
      return fail(c, RT_ERR_INVALID_ARG, "rt_render_frame: instances are in motion with object motion vectors on (rt_set_object_motion) and counting on (rt_set_counting): the counting build has no object-motion form");
    if(omMotion) {
      if((rc = growTable(c, &c->omTable, &c->omTableRows, nInst, sizeof(OmCamera)))) return rc;
      c->omHost.resize(nInst);
      for(size_t i = 0; i < nInst; i++) {
        rt_scene_camera ci = cam;
        if(c->omMoved[i]) (void)rt_object_motion_camera(&cam, c->omPrev[i].data(), c->instances[i].objectToWorld, &ci);
        c->omHost[i].lastProjView = ci.lastProjView; c->omHost[i].lastPosition = ci.lastPosition; c->omHost[i].pad = 0.f;
      }
    }
  }
  // Per-vertex motion vectors (mode RT_OBJECT_MOTION_VERTEX): the two stages come from the RT_VM builds, which write the instance image and the delta image; when
  // an instance is in motion or its mesh was deformed since the last rendered frame they also read the per-instance rows {previous objectToWorld, flags}, filled
  // here and uploaded like the camera table, and the previous-position plane the deforming calls filled.
  const bool vm = c->objMotion == RT_OBJECT_MOTION_VERTEX && !c->counting && c->omInst && c->vmDelta;
  bool vmMotion = false;
  if(c->objMotion == RT_OBJECT_MOTION_VERTEX) {
    const size_t nInst = c->instances.size();
    const bool moves = c->omPending && c->omMoved.size() == nInst, bends = c->vmPending && c->vmPlane;
    auto flagsOf = [&](size_t i) -> uint32_t {
      uint32_t f = 0;
      if(moves && c->omMoved[i] && std::memcmp(c->omPrev[i].data(), c->instances[i].objectToWorld, 48) != 0) f |= VM_MOVED;
      if(bends && c->vmDeformed[c->instances[i].primMesh]) f |= VM_DEFORMED;
      return f;
    };
    if(moves || bends) for(size_t i = 0; i < nInst && !vmMotion; i++) vmMotion = flagsOf(i) != 0u;
    if(vmMotion && c->counting)
      return fail(c, RT_ERR_INVALID_ARG, "rt_render_frame: instances are in motion or meshes deformed with per-vertex motion vectors on (rt_set_object_motion) and counting on (rt_set_counting): the counting build has no motion-vector form");
    if(vmMotion) {
      if((rc = growTable(c, &c->vmTable, &c->vmTableRows, nInst, sizeof(VmRow)))) return rc;
      c->vmHost.resize(nInst);
      for(size_t i = 0; i < nInst; i++) {
        VmRow& r = c->vmHost[i];
        r.flags = flagsOf(i); r.pad[0] = r.pad[1] = r.pad[2] = 0u;
        memcpy(r.P, (r.flags & VM_MOVED) ? c->omPrev[i].data() : c->instances[i].objectToWorld, 48);
      }
    }
  }
  const bool haveRing = c->spare[rt_ctx::RING_G][0] && c->spare[rt_ctx::RING_MOTION][0];
  const bool decide = c->overlap >= 2 && !c->prioDecided && haveRing;
  if(decide) { RT_HIP(c, syncAll(c)); harvestTimings(c); }
  const double tracedBefore = c->accStage[RT_STAGE_DIRECT] + c->accStage[RT_STAGE_INDIRECT];
  const double filterBefore = c->accStage[RT_STAGE_DENOISE_DIRECT] + c->accStage[RT_STAGE_DENOISE_INDIRECT] + c->accStage[RT_STAGE_COMPOSE];
  rt_ctx::EvSet& E = c->evSets[c->evUsed];
  if(c->overlap >= 1 && !decide) RT_HIP(c, ensureOverlapStreams(c));
  const bool pipelined = !decide && c->overlap >= 2 && c->sideStream && c->indStream && haveRing;
  const bool deep = ringDeep(c);
  if(pipelined) {
    // Rotate the G-buffer (3 physical buffers) and the motion buffer (2): direct(f+1) must not overwrite what indirect(f)
    // still reads (its own G-buffer + motion, and G(f-1) for temporal reprojection).  The boundary ids keep their meaning:
    // RT_BUF_GBUFFER0 + (frames & 1) / RT_BUF_MOTION are this frame's buffers once the call returns.
    // Mode 3 (three frames in flight): one more buffer of each kind, taken oldest first, and the direct image (noisy, filtered in place, composed) three deep —
    // direct(f) then overwrites G(f-4), motion(f-3) and the direct image of f-3 and has nothing to wait for in frame f-2 (below).
    rotateRing(c, frames, deep);
  } else {
    RT_HIP(c, joinInFlight(c));
  }
  const DevFrame F = makeFrame(c, frames);
  const DevObjMotion OM{static_cast<uint32_t*>(c->omInst), omMotion ? static_cast<const OmCamera*>(c->omTable) : nullptr, uint32_t(c->instances.size()), 0u};
  const DevVtxMotion VM{static_cast<uint32_t*>(c->omInst), static_cast<float4*>(c->vmDelta), vmMotion ? static_cast<const VmRow*>(c->vmTable) : nullptr,
                        static_cast<const float4*>(c->vmPlane), uint32_t(c->instances.size()), 0u};
  int k = 0, lastMain = 0, lastSide = 0, lastInd = 0;
  auto record = [&](hipStream_t strm, int stage) -> int {   // end-of-launch timestamp, timed against the previous one of the stream
    const hipError_t e = hipEventRecord(E.ev[k], strm);
    if(e != hipSuccess) { c->err = std::string("hipEventRecord: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    int& last = (strm == c->stream) ? lastMain : (strm == c->indStream ? lastInd : lastSide);
    E.stage[k] = stage; E.prev[k] = last; last = k; k++;
    return RT_OK;
  };
  auto launched = [&](hipStream_t strm, int stage, const char* launcher, hipError_t e) -> int {   // what follows every launch: its error, or its timestamp
    if(e != hipSuccess) { c->err = std::string(launcher) + ": " + hipGetErrorString(e); return RT_ERR_HIP; }
    return record(strm, stage);
  };
  auto run = [&](hipStream_t strm, int stage, int level) -> int {
    return launched(strm, stage, "launchStage", launchStageOn(c, strm, F, rt::StageExtra{&OM, &VM, nullptr},
                                                              om ? rt::STAGE_MOTION_OBJECT : (vm ? rt::STAGE_MOTION_VERTEX : rt::STAGE_MOTION_NONE), *st, cam, stage, level, 0, 0));
  };
  // the direct stage, after the per-instance camera table when instances are in motion: the copy is ordered before the direct stage on its stream, and the
  // indirect stage follows the direct stage in every schedule (stream order, evD).  The table's previous reader is a frame before the last rt_update_instances,
  // which drained the context.  The host rows (omHost, pageable) are rewritten only by such a frame too, and hipMemcpyAsync from pageable memory has staged
  // them by the time it returns.  An update that no longer drains (event-ordered, DESIGN.md §20 "Not done") needs a table and pinned rows per frame in flight.
  // Once the stage is issued the frame has been rendered as far as the motion state goes: every previous matrix becomes the current one.
  auto direct = [&](hipStream_t strm) -> int {
    if(om && omMotion) RT_HIP(c, hipMemcpyAsync(c->omTable, c->omHost.data(), c->omHost.size() * sizeof(OmCamera), hipMemcpyHostToDevice, strm));
    if(vm && vmMotion) RT_HIP(c, hipMemcpyAsync(c->vmTable, c->vmHost.data(), c->vmHost.size() * sizeof(VmRow), hipMemcpyHostToDevice, strm));
    const int r = run(strm, RT_STAGE_DIRECT, 0);   // (through the replay rule: launchStageOn)
    if(r == RT_OK) {
      if(om) c->omInstValid = true;
      if(vm) c->omInstValid = c->vmDeltaValid = true;
      if(c->vmPending) { std::fill(c->vmDeformed.begin(), c->vmDeformed.end(), uint8_t(0)); c->vmPending = false; }   // every mesh is undeformed for the next frame
      if(c->omPending) { std::fill(c->omMoved.begin(), c->omMoved.end(), uint8_t(0)); c->omPending = false; }
    }
    return r;
  };
  // The history a temporal pass of this frame reads is the one its pass of the previous frame wrote, if nothing invalidated it since (parity_history.h).  Every
  // history sees every frame begin, whether or not its pass runs; the history of this frame's parity becomes valid once the pass is enqueued (svgfEnqueued for the
  // two SVGF chains, compose for the resolves); until then, and on every error return, it is not.
  const bool svgfRead = c->histSvgf.state.begin(frames), taaRead = c->histTaa.state.begin(frames), upsRead = c->histUps.state.begin(frames);
  SvgfArgs svgfA[2] = {};
  if(svgf) for(int ind = 0; ind < 2; ind++) svgfA[ind] = svgfArgs(c, F, *st, frames, ind != 0, svgfRead);
  auto svgfEnqueued = [&]() { if(svgf) c->histSvgf.state.commit(frames); };
  // one component's filter chain: the 4 / 5 A-Trous levels, or the SVGF steps; timed under the stage's RT_STAGE_DENOISE_* entry
  auto filters = [&](hipStream_t strm, bool ind) -> int {
    const int stage = ind ? RT_STAGE_DENOISE_INDIRECT : RT_STAGE_DENOISE_DIRECT;
    int r;
    if(!svgf) {
      for(int i = 0; i < (ind ? 5 : 4); i++) if((r = run(strm, stage, i))) return r;
      return RT_OK;
    }
    for(int s = 0; s < svgfSteps(ind); s++) if((r = launched(strm, stage, "launchSvgfStep", launchSvgfStep(strm, svgfA[ind ? 1 : 0], cam, ind, s)))) return r;
    return RT_OK;
  };
  // the indirect stage, then the GI spatial pass when the mode is on; both timed under RT_STAGE_INDIRECT
  auto indirect = [&](hipStream_t strm) -> int {
    int r;
    if((r = run(strm, RT_STAGE_INDIRECT, 0))) return r;
    if(!gis) return RT_OK;
    const hipError_t e = launchGiSpatial(strm, c->ds, *st, cam, giSpatialArgs(c, F));
    if(e == hipSuccess) c->gisWritten = true;
    return launched(strm, RT_STAGE_INDIRECT, "launchGiSpatial", e);
  };
  TaaArgs taaA{};
  if(taa) taaA = resolveArgs<TaaArgs>(c, c->histTaa, c->taa, F, frames, taaRead);
  UpscaleArgs upsA{};
  if(ups) {   // the same at the output size, with the frame's jitter offset in render pixels
    upsA = resolveArgs<UpscaleArgs>(c, c->histUps, c->ups, F, frames, upsRead);
    upsA.Wo = c->upsW; upsA.Ho = c->upsH; upsA.dx = upsDelta[0]; upsA.dy = upsDelta[1];
  }
  // compose, then the upsampling or the TAA resolve when one runs (never both); all timed under RT_STAGE_COMPOSE
  auto compose = [&](hipStream_t strm) -> int {
    int r;
    if((r = run(strm, RT_STAGE_COMPOSE, 0)) || !(ups || taa)) return r;
    if((r = ups ? launched(strm, RT_STAGE_COMPOSE, "launchUpscaleResolve", launchUpscaleResolve(strm, upsA, cam))
                : launched(strm, RT_STAGE_COMPOSE, "launchTaaResolve", launchTaaResolve(strm, taaA, cam)))) return r;
    (ups ? c->histUps : c->histTaa).state.commit(frames);
    return RT_OK;
  };
  auto mark = [&](hipStream_t strm, int& last) -> hipError_t {  // start-of-chain timestamp on a stream (after its waits)
    hipError_t e = hipEventRecord(E.ev[k], strm);
    E.stage[k] = -1; E.prev[k] = k; last = k; k++;
    return e;
  };

  if(pipelined) {
    // Frames in flight.  Three in-order streams:
    //   stream    : direct(f)                                      -> evD
    //   indStream : wait evD; indirect(f)                          -> evI
    //   sideStream: wait evD; direct A-Trous x4; wait evI; indirect A-Trous x5; compose -> evDone
    // so that direct(f+1), submitted by the next call, runs beside indirect(f) and the filters of frame f: the long
    // tail of multi-bounce tiles no longer leaves the chip idle, and the bandwidth-bound filters hide behind traversal.
    // Buffer reuse across frames is ordered explicitly:
    //   direct(f) overwrites G(f-3) [read by indirect(f-2)], motion(f-2) [indirect(f-2)] and the result image of f-2 [compose(f-2)];
    //   indirect(f) overwrites the noisy-indirect buffer of its parity, which the indirect A-Trous of f-2 read (two buffers: no wait for f-1's filters).
    // Mode 3: with the deeper rotation above the same three hazards are those of frame f-3.  Mode 2's wait closes a loop direct(f-2) -> filters(f-2) -> direct(f):
    // two periods cannot be shorter than a direct stage plus the whole filter chain of one frame, and in flight that chain is stretched to the length of a frame.
    // SVGF (rt_set_denoiser) adds reads across frames, all covered by the same waits:
    //   its history is double-buffered by parity: the chains of f read parity f-1 and write parity f, and every filter chain runs in order on sideStream, so
    //   the chains of f-1 have finished writing before those of f read, and those of f-2 before those of f overwrite;
    //   its temporal pass reads G(f-1) (lastG) and motion(f): direct(f+1) writes the G-buffer that held G(f-2) and the motion buffer of f-1, and the first
    //   writer of G(f-1) / motion(f) is direct(f+2) (mode 3: f+3), which waits for evDone(f) (s >= depth above);
    //   mode 3's three-deep direct image: the direct chain reads and rewrites the image of f only, which direct(f+3) overwrites after evDone(f).
    // GI spatial reuse (rt_set_gi_spatial) runs on indStream right after indirect(f), before evI is recorded, so stream order covers it:
    //   it reads G(f) and the indirect reservoirs of f and rewrites IND_A of f; indirect(f+2), the next writer of that reservoir parity and of that IND_A,
    //   runs after it on the same stream; the filters and compose of f, which read IND_A, wait on evI.  Its own reservoir buffer is rewritten by the pass of
    //   f+1, again on indStream; rt_gi_spatial_readback drains the context first.
    // TAA (rt_set_taa) resolves f on sideStream right after compose(f), before evDone(f) is recorded:
    //   it reads the result images of f (written by compose on the same stream), G(f) and G(f-1) (lastG).  The first writer of G(f-1) is direct(f+2) (mode 3:
    //   f+3), which waits for evDone(f) (s >= depth above); G(f) is next written by direct(f+3) / f+4, after evDone(f+1); mode 3's three-deep direct image of f
    //   is overwritten by direct(f+3) after evDone(f), the indirect image of f by compose(f+2) on sideStream;
    //   its history is double-buffered by parity: the pass of f reads parity f-1 (written by the pass of f-1, earlier on sideStream) and the parity it writes
    //   is rewritten only by the pass of f+2, again on sideStream; rt_tonemap and rt_taa_readback join the frames in flight first.
    // Temporal upsampling (rt_set_upscale) takes TAA's place on sideStream, after compose(f) and before evDone(f), and reads exactly what TAA reads — the result
    //   images of f, G(f), G(f-1) — so the three writers above are ordered behind it by the same waits; its history at the output size is double-buffered by
    //   parity and written and read on sideStream only; rt_upscale_tonemap and rt_upscale_readback join the frames in flight first.
    const uint64_t s = c->seq;
    const int r = int(s & 3);
    const uint64_t depth = deep ? 3u : 2u;
    if(s >= depth) {
      RT_HIP(c, hipStreamWaitEvent(c->stream, c->evI[(s - depth) & 3], 0));
      RT_HIP(c, hipStreamWaitEvent(c->stream, c->evDone[(s - depth) & 3], 0));
    }
    RT_HIP(c, mark(c->stream, lastMain));
    if((rc = direct(c->stream))) return rc;
    RT_HIP(c, hipEventRecord(c->evD[r], c->stream));

    RT_HIP(c, hipStreamWaitEvent(c->indStream, c->evD[r], 0));
    if(s >= 2) RT_HIP(c, hipStreamWaitEvent(c->indStream, c->evDone[(s - 2) & 3], 0));   // the noisy-indirect buffer of this parity: filtered for f-2
    RT_HIP(c, mark(c->indStream, lastInd));
    if((rc = indirect(c->indStream))) return rc;
    RT_HIP(c, hipEventRecord(c->evI[r], c->indStream));

    RT_HIP(c, hipStreamWaitEvent(c->sideStream, c->evD[r], 0));
    RT_HIP(c, mark(c->sideStream, lastSide));
    if(st->denoise > 0 && (rc = filters(c->sideStream, false))) return rc;
    RT_HIP(c, hipStreamWaitEvent(c->sideStream, c->evI[r], 0));
    RT_HIP(c, mark(c->sideStream, lastSide));
    if(st->denoise > 0 && (rc = filters(c->sideStream, true))) return rc;
    if((rc = compose(c->sideStream))) return rc;
    RT_HIP(c, hipEventRecord(c->evDone[r], c->sideStream));
    svgfEnqueued();
    c->seq = s + 1; c->inFlight = true;
    E.count = k; E.last = lastSide;
    c->evUsed++;
    return RT_OK;
  }

  RT_HIP(c, mark(c->stream, lastMain));
  // Renderer::run, renderer.cpp:163-205.  The direct A-Trous chain only depends on the direct stage and the indirect stage
  // + its A-Trous chain only on the G-buffer, so the two chains run on two streams and join before compose: the direct
  // filter (ALU bound, full occupancy) fills the CUs that the indirect stage's long tail of multi-bounce tiles leaves idle.
  const bool fork = !decide && c->overlap && st->denoise > 0 && c->sideStream;
  if((rc = direct(c->stream))) return rc;
  if(fork) {
    RT_HIP(c, hipEventRecord(c->evFork, c->stream));
    RT_HIP(c, hipStreamWaitEvent(c->sideStream, c->evFork, 0));
    RT_HIP(c, mark(c->sideStream, lastSide));
    if((rc = filters(c->sideStream, false))) return rc;
    RT_HIP(c, hipEventRecord(c->evJoin, c->sideStream));
  }
  if((rc = indirect(c->stream))) return rc;
  if(st->denoise > 0) {
    if(!fork && (rc = filters(c->stream, false))) return rc;
    if((rc = filters(c->stream, true))) return rc;
  }
  if(fork) RT_HIP(c, hipStreamWaitEvent(c->stream, c->evJoin, 0));
  if((rc = compose(c->stream))) return rc;
  svgfEnqueued();
  E.count = k; E.last = lastMain;
  c->evUsed++;
  if(decide) {
    RT_HIP(c, syncAll(c));
    harvestTimings(c);
    const double traced = (c->accStage[RT_STAGE_DIRECT] + c->accStage[RT_STAGE_INDIRECT]) - tracedBefore;
    const double filt = (c->accStage[RT_STAGE_DENOISE_DIRECT] + c->accStage[RT_STAGE_DENOISE_INDIRECT] + c->accStage[RT_STAGE_COMPOSE]) - filterBefore;
    c->filterShare = traced > 0.0 ? float(filt / traced) : -1.f;
    c->denoiseSeen = st->denoise > 0 ? 1 : 0;
    if(++c->probeFrames >= prioProbeFrames()) {
      c->prio[1] = 1; c->prio[2] = (c->filterShare >= PRIO_FILTER_SHARE) ? 1 : 0;
      c->prioDecided = true;
      c->indStream = c->sideStream = nullptr;   // (created with these levels by the next frame: filter stream first, then the indirect stream)
    }
  }
  return RT_OK;
}

size_t rt_buffer_bytes(rt_ctx* c, int buffer) { return (c && buffer >= 0 && buffer < RT_BUF_COUNT) ? c->bufBytes[buffer] : 0; }

int rt_readback(rt_ctx* c, int buffer, void* dst, size_t bytes)
{
  if(!c || !dst || buffer < 0 || buffer >= RT_BUF_COUNT) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_readback: rt_resize has not been called");
  if(bytes != c->bufBytes[buffer]) return fail(c, RT_ERR_INVALID_ARG, "rt_readback: size mismatch (see rt_buffer_bytes)");
  return readbackDrained(c, c->bufs[buffer], dst, bytes);
}

int rt_upload_history(rt_ctx* c, int buffer, const void* src, size_t bytes)
{
  if(!c || !src || buffer < 0 || buffer >= RT_BUF_COUNT) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_upload_history: rt_resize has not been called");
  if(bytes != c->bufBytes[buffer]) return fail(c, RT_ERR_INVALID_ARG, "rt_upload_history: size mismatch (see rt_buffer_bytes)");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  RT_HIP(c, hipMemcpy(c->bufs[buffer], src, bytes, hipMemcpyHostToDevice));
  if(buffer == RT_BUF_DENOISE_IND_A)   // both parities: the caller's next stage may name either frame
    for(void* p : c->indA) if(p && p != c->bufs[buffer]) RT_HIP(c, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
  RT_HIP(c, hipDeviceSynchronize());
  return RT_OK;
}

int rt_device_ptr(rt_ctx* c, int buffer, void** ptr, size_t* bytes, size_t* rowPitch)
{
  if(!c || buffer < 0 || buffer >= RT_BUF_COUNT || !ptr) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_device_ptr: rt_resize has not been called");
  *ptr = c->bufs[buffer];
  if(bytes) *bytes = c->bufAlloc[buffer];
  if(rowPitch) *rowPitch = size_t(halfRes(buffer) ? c->W / 2 : c->W) * elemBytes(buffer);
  return RT_OK;
}

int rt_set_counting(rt_ctx* c, int enable)
{
  if(!c) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  RT_HIP(c, hipMemset(c->dCounters, 0, 8 * sizeof(unsigned long long)));
  RT_HIP(c, hipDeviceSynchronize());
  harvestTimings(c);
  for(double& v : c->accStage) v = 0;
  c->accFrame = 0; c->accFrames = 0;
  c->counting = enable != 0;
  return RT_OK;
}

int rt_get_counters(rt_ctx* c, rt_counters* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  unsigned long long h[8];
  RT_HIP(c, hipMemcpy(h, c->dCounters, sizeof(h), hipMemcpyDeviceToHost));
  out->closestHitRays = h[0]; out->anyHitRays = h[1]; out->nodesVisited = h[2]; out->trisTested = h[3]; out->hitsShaded = h[4]; out->risCandidates = h[5]; out->laneRounds = h[6]; out->laneLiveRounds = h[7];
  harvestTimings(c);
  for(int i = 0; i < RT_STAGE_COUNT; i++) out->stageMs[i] = float(c->accStage[i]);
  out->frameMs = float(c->accFrame);
  out->framesTimed = c->accFrames;
  return RT_OK;
}

int rt_set_history_rows(rt_ctx* c, int row0, int row1)
{
  if(!c || row0 < 0 || row1 < row0) return RT_ERR_INVALID_ARG;
  c->histRow0 = row0; c->histRow1 = row1;
  return RT_OK;
}

int rt_history_miss(rt_ctx* c, int* missed)
{
  if(!c || !missed) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_history_miss: rt_resize has not been called");
  RT_HIP(c, hipSetDevice(c->device));
  uint32_t v[2] = {0, 0};
  RT_HIP(c, syncAll(c));
  RT_HIP(c, hipMemcpyAsync(v, c->scratch.qcount + 250, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  RT_HIP(c, hipMemsetAsync(c->scratch.qcount + 250, 0, sizeof(v), c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  *missed = (v[0] | v[1]) ? 1 : 0;
  return RT_OK;
}

int rt_history_miss_stage(rt_ctx* c, int stage, int* missed)
{
  if(!c || !missed || stage < 0 || stage >= RT_STAGE_COUNT) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_history_miss_stage: rt_resize has not been called");
  RT_HIP(c, hipSetDevice(c->device));
  uint32_t* flag = c->scratch.qcount + 250 + (stage == RT_STAGE_INDIRECT ? 1 : 0);
  uint32_t v = 0;
  RT_HIP(c, hipMemcpyAsync(&v, flag, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  RT_HIP(c, hipMemsetAsync(flag, 0, sizeof(v), c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));  // the ctx stream only: other streams of the host keep running
  *missed = v ? 1 : 0;
  return RT_OK;
}

int rt_select_frame(rt_ctx* c, int frames)
{
  if(!c) return RT_ERR_INVALID_ARG;
  selectFrame(c, frames);
  return RT_OK;
}

int rt_rotate_buffers(rt_ctx* c, int frames)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(c->W == 0 || !c->spare[rt_ctx::RING_G][0] || !c->spare[rt_ctx::RING_MOTION][0]) return fail(c, RT_ERR_NO_TARGET, "rt_rotate_buffers: rt_resize has not been called");
  rotateRing(c, frames, false);
  return RT_OK;
}

int rt_get_primary_replay_stats(rt_ctx* c, rt_primary_replay_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof *out);
  out->state = uint32_t(c->replay.state);
  out->K = c->vis.K ? c->vis.K : visListLength();
  out->launchesRecorded = c->replayRecorded; out->launchesReplayed = c->replayReplayed;
  if(c->replay.state == rt::PRIMARY_REPLAY_VALID && c->vis.count && c->W > 0) {   // the pixel classes of the recording in force
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    std::vector<uint32_t> cnt(size_t(c->W) * size_t(c->H));
    RT_HIP(c, hipMemcpy(cnt.data(), c->vis.count, cnt.size() * 4, hipMemcpyDeviceToHost));
    for(uint32_t v : cnt) { if(v == rt::VIS_OVERFLOW) out->pixelsOverflow++; else if(v == 0u) out->pixelsSettled++; else out->pixelsListed++; }
  }
  return RT_OK;
}

int rt_primary_replay_readback(rt_ctx* c, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(c->replay.state != rt::PRIMARY_REPLAY_VALID || !c->vis.count) return fail(c, RT_ERR_INVALID_ARG, "rt_primary_replay_readback: no recording in force");
  if(bytes != size_t(c->W) * size_t(c->H) * 4) return fail(c, RT_ERR_INVALID_ARG, "rt_primary_replay_readback: size mismatch (W x H x 4 bytes)");
  return readbackDrained(c, c->vis.count, dst, bytes);
}

int rt_set_traversal(rt_ctx* c, int mode)
{
  if(!c || mode < RT_TRAVERSAL_AUTO || mode > RT_TRAVERSAL_LATENCY) return RT_ERR_INVALID_ARG;
  c->traversal = mode;
  return RT_OK;
}

int rt_pick(rt_ctx* c, const rt_mat4* modelViewInv, const rt_mat4* perspectiveInv, float pickX, float pickY, rt_pick_result* out)
{
  if(!c || !modelViewInv || !perspectiveInv || !out) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "no scene uploaded");
  if(!c->haveAccel) return fail(c, RT_ERR_NO_ACCEL, "rt_build_accel has not been called");
  RT_HIP(c, hipSetDevice(c->device));
  if(!c->dPick) RT_HIP(c, hipMalloc(&c->dPick, sizeof(rt_pick_result)));
  rt_pick_result* d = static_cast<rt_pick_result*>(c->dPick);
  RT_HIP(c, launchPick(c->stream, c->ds, *modelViewInv, *perspectiveInv, pickX, pickY, d));
  RT_HIP(c, hipMemcpyAsync(out, d, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_trace_rays(rt_ctx* c, int n, const float* rays, float* out, int anyHit)
{
  if(!c || n < 0 || (n > 0 && (!rays || !out))) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "no scene uploaded");
  if(!c->haveAccel) return fail(c, RT_ERR_NO_ACCEL, "rt_build_accel has not been called");
  if(n == 0) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  float4* dr = nullptr; float4* dout = nullptr;
  RT_HIP(c, hipMalloc(reinterpret_cast<void**>(&dr), size_t(n) * 32));
  if(hipMalloc(reinterpret_cast<void**>(&dout), size_t(n) * 16) != hipSuccess) { (void)hipFree(dr); return fail(c, RT_ERR_OOM, "rt_trace_rays: hipMalloc failed"); }
  hipError_t e = hipMemcpyAsync(dr, rays, size_t(n) * 32, hipMemcpyHostToDevice, c->stream);
  if(e == hipSuccess) e = launchTraceRays(c->stream, c->ds, n, dr, dout, anyHit);
  if(e == hipSuccess) e = hipMemcpyAsync(out, dout, size_t(n) * 16, hipMemcpyDeviceToHost, c->stream);
  if(e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(dr); (void)hipFree(dout);
  RT_HIP(c, e);
  return RT_OK;
}

int rt_set_sun_and_sky(rt_ctx* c, const rt_sun_and_sky* ss)
{
  if(!c || !ss) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  c->sunAndSky = *ss;
  if(ss->in_use == 1) {
    if(!c->dSky) RT_HIP(c, hipMalloc(&c->dSky, 512));
    RT_HIP(c, launchSkyPrepare(c->stream, *ss, static_cast<SkyPre*>(c->dSky)));
    RT_HIP(c, hipStreamSynchronize(c->stream));
  }
  c->ds.sky = (ss->in_use == 1) ? static_cast<const SkyPre*>(c->dSky) : nullptr;
  c->refN = 0;
  return RT_OK;
}

int rt_tonemap(rt_ctx* c, const rt_tonemapper* tm, int debugging_mode, int frames)
{
  if(!c || !tm) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_tonemap: rt_resize has not been called");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, joinInFlight(c));  // the result images of `frames` are complete once compose (side stream) is done
  const int cur = rt::frameParity(frames);
  // the resolved images when frame `frames` was resolved (rt_set_taa), the plain result images otherwise
  void* const* hist = c->histTaa.plane[cur];
  const bool resolved = hist[0] && c->histTaa.state.holds(frames);
  const float4* dImg = static_cast<const float4*>(resolved ? hist[0] : c->bufs[RT_BUF_DIRECT_RESULT0 + cur]);
  const float4* iImg = static_cast<const float4*>(resolved ? hist[1] : c->bufs[RT_BUF_INDIRECT_RESULT0 + cur]);
  RT_HIP(c, launchTonemap(c->stream, dImg, iImg,
                          c->scratch.postRowSums, c->scratch.postMean, *tm, debugging_mode, c->W, c->H, static_cast<uint32_t*>(c->bufs[RT_BUF_LDR]),
                          c->scratch.postMipD, c->scratch.postMipI));
  return RT_OK;
}

// ---- rt_reference_*: the progressive ground-truth path tracer (csrc/reference.hip).  Main stream only, after the frames in flight; it reads the scene, the
// camera and the RtxState it is given and touches no frame buffer, counter, stream decision or rotation of the real-time path.
static int ensureReferenceBuffers(rt_ctx* c)
{
  if(c->refAcc) return RT_OK;
  const size_t n = size_t(c->W) * size_t(c->H);
  RT_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->refAcc), n * REF_ACC_DOUBLES * sizeof(double)));
  if(hipMalloc(reinterpret_cast<void**>(&c->refMean), n * 2 * sizeof(float4)) != hipSuccess) {
    (void)hipFree(c->refAcc); c->refAcc = nullptr;
    return fail(c, RT_ERR_OOM, "rt_reference_render: hipMalloc of the reference accumulators failed");
  }
  c->refN = 0;
  return RT_OK;
}

int rt_reference_render(rt_ctx* c, const rt_state* st, int samples)
{
  int rc = checkReady(c, st);
  if(rc) return rc;
  if(samples < 0) return fail(c, RT_ERR_INVALID_ARG, "rt_reference_render: samples must be >= 0");
  if(st->debugging_mode != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_reference_render: debugging_mode must be 0 (the reference mode has no debug views)");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, joinInFlight(c));
  if((rc = ensureReferenceBuffers(c))) return rc;
  // the RtxState inputs of the integral; the other inputs (size, scene, tree, sun & sky, view) reset refN where they change
  const bool same = c->refKeyValid && st->maxDepth == c->refMaxDepth && st->MIS == c->refMIS &&
                    std::memcmp(&st->hdrMultiplier, &c->refHdrMultiplier, sizeof(float)) == 0 && std::memcmp(&st->environmentProb, &c->refEnvironmentProb, sizeof(float)) == 0;
  if(!same) c->refN = 0;
  c->refKeyValid = true; c->refMaxDepth = st->maxDepth; c->refMIS = st->MIS; c->refHdrMultiplier = st->hdrMultiplier; c->refEnvironmentProb = st->environmentProb;
  if(samples == 0) return RT_OK;
  if(uint64_t(c->refN) + uint64_t(samples) > 0xffffffffull) return fail(c, RT_ERR_INVALID_ARG, "rt_reference_render: more than 2^32 - 1 samples");
  if(c->refN == 0) RT_HIP(c, hipMemsetAsync(c->refAcc, 0, size_t(c->W) * size_t(c->H) * REF_ACC_DOUBLES * sizeof(double), c->stream));
  const auto launch = c->ds.sky ? rt::ref_sky::launchReference : rt::ref_base::launchReference;
  const int band = std::max(8, (REF_BAND_PIXELS / c->W) & ~7);   // rows per launch: no launch longer than a frame's stages on the largest scenes
  for(int s = 0; s < samples; s++)
    for(int r0 = 0; r0 < c->H; r0 += band) RT_HIP(c, launch(c->stream, c->ds, *st, c->cam, c->refAcc, c->refN + uint32_t(s), r0, std::min(c->H, r0 + band)));
  c->refN += uint32_t(samples);
  return RT_OK;
}

int rt_reference_reset(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  c->refN = 0;
  return RT_OK;
}

int rt_reference_samples(rt_ctx* c, uint32_t* n)
{
  if(!c || !n) return RT_ERR_INVALID_ARG;
  *n = c->refN;
  return RT_OK;
}

int rt_reference_readback(rt_ctx* c, int component, float* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(component < 0 || component > 2) return fail(c, RT_ERR_INVALID_ARG, "rt_reference_readback: component must be 0 (direct), 1 (indirect) or 2 (sum)");
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_reference_readback: rt_resize has not been called");
  const size_t n = size_t(c->W) * size_t(c->H);
  if(bytes != n * sizeof(float4)) return fail(c, RT_ERR_INVALID_ARG, "rt_reference_readback: size mismatch (W * H * 16 bytes, RGBA32F)");
  if(c->refN == 0 || !c->refAcc) {   // nothing accumulated: the mean of no samples is 0
    for(size_t i = 0; i < n; i++) { dst[4 * i] = dst[4 * i + 1] = dst[4 * i + 2] = 0.f; dst[4 * i + 3] = 1.f; }
    return RT_OK;
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, joinInFlight(c));
  RT_HIP(c, launchReferenceMean(c->stream, c->refAcc, c->refN, component, n, c->refMean));
  RT_HIP(c, hipMemcpyAsync(dst, c->refMean, bytes, hipMemcpyDeviceToHost, c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_reference_tonemap(rt_ctx* c, const rt_tonemapper* tm)
{
  if(!c || !tm) return RT_ERR_INVALID_ARG;
  if(c->W == 0) return fail(c, RT_ERR_NO_TARGET, "rt_reference_tonemap: rt_resize has not been called");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, joinInFlight(c));
  int rc;
  if((rc = ensureReferenceBuffers(c))) return rc;
  const size_t n = size_t(c->W) * size_t(c->H);
  RT_HIP(c, launchReferenceMean(c->stream, c->refAcc, c->refN, 0, n, c->refMean));
  RT_HIP(c, launchReferenceMean(c->stream, c->refAcc, c->refN, 1, n, c->refMean + n));
  // post.frag over the two means in place of the two result images (rt_tonemap's pass, default view)
  RT_HIP(c, launchTonemap(c->stream, c->refMean, c->refMean + n, c->scratch.postRowSums, c->scratch.postMean, *tm, 0, c->W, c->H, static_cast<uint32_t*>(c->bufs[RT_BUF_LDR]),
                          c->scratch.postMipD, c->scratch.postMipI));
  return RT_OK;
}

// ---- rt_set_denoiser: A-Trous (default) or SVGF (csrc/svgf.hip); the settings are host state read when a frame is enqueued
int rt_set_denoiser(rt_ctx* c, const rt_denoiser* d)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!d) return fail(c, RT_ERR_INVALID_ARG, "rt_set_denoiser: NULL settings");
  if(d->mode != RT_DENOISER_ATROUS && d->mode != RT_DENOISER_SVGF) return fail(c, RT_ERR_INVALID_ARG, "rt_set_denoiser: mode must be RT_DENOISER_ATROUS or RT_DENOISER_SVGF");
  if(!(d->alphaColor > 0.0f && d->alphaColor <= 1.0f) || !(d->alphaMoments > 0.0f && d->alphaMoments <= 1.0f))
    return fail(c, RT_ERR_INVALID_ARG, "rt_set_denoiser: alphaColor and alphaMoments must lie in (0, 1]");
  if(d->historyCap < 1) return fail(c, RT_ERR_INVALID_ARG, "rt_set_denoiser: historyCap must be >= 1");
  if(!(d->phiLumDirect > 0.0f && std::isfinite(d->phiLumDirect)) || !(d->phiLumIndirect > 0.0f && std::isfinite(d->phiLumIndirect)))
    return fail(c, RT_ERR_INVALID_ARG, "rt_set_denoiser: phiLumDirect and phiLumIndirect must be positive and finite");
  if(d->reserved[0] != 0 || d->reserved[1] != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_denoiser: reserved fields must be 0");
  if(std::memcmp(&c->den, d, sizeof(rt_denoiser)) == 0) return RT_OK;
  if(d->mode != c->den.mode) {   // the filter share the stream priorities were decided on has changed, like a denoise toggle
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    reopenPriorityDecision(c);
  }
  c->den = *d;
  c->histSvgf.state.invalidate();
  return RT_OK;
}

int rt_get_denoiser(rt_ctx* c, rt_denoiser* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->den;
  return RT_OK;
}

int rt_denoiser_reset(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  c->histSvgf.state.invalidate();
  return RT_OK;
}

int rt_denoiser_readback(rt_ctx* c, int which, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(which < 0 || which > 3) return fail(c, RT_ERR_INVALID_ARG, "rt_denoiser_readback: which must be 0 (direct colour + n), 1 (indirect colour + n), 2 (direct moments) or 3 (indirect moments)");
  const rt_ctx::History& h = c->histSvgf;
  if(!h.plane[0][0] || h.state.last < 0) return fail(c, RT_ERR_NO_TARGET, "rt_denoiser_readback: no frame has been rendered in SVGF mode since the last rt_resize");
  const size_t px = (which & 1) ? size_t(c->W / 2) * (c->H / 2) : size_t(c->W) * c->H;
  if(bytes != px * (which < 2 ? sizeof(float4) : sizeof(float2))) return fail(c, RT_ERR_INVALID_ARG, "rt_denoiser_readback: size mismatch");
  return readbackDrained(c, h.plane[h.state.last][which], dst, bytes);
}

// ---- rt_set_gi_spatial: ReSTIR GI spatial reuse (csrc/gi_spatial.hip); the settings are host state read when a frame is enqueued
int rt_set_gi_spatial(rt_ctx* c, const rt_gi_spatial* s)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!s) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: NULL settings");
  if(s->mode != RT_GI_SPATIAL_OFF && s->mode != RT_GI_SPATIAL_ON && s->mode != RT_GI_SPATIAL_VISIBILITY)
    return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: mode must be RT_GI_SPATIAL_OFF, RT_GI_SPATIAL_ON or RT_GI_SPATIAL_VISIBILITY");
  if(s->samples < 0 || s->samples > 16) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: samples must lie in 0..16");
  if(s->radius < 1 || s->radius > 64) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: radius must lie in 1..64");
  if(!(s->normalThreshold >= -1.0f && s->normalThreshold <= 1.0f)) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: normalThreshold must lie in [-1, 1]");
  if(!(s->depthThreshold > 0.0f && std::isfinite(s->depthThreshold))) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: depthThreshold must be positive and finite");
  if(!(s->jacobianMax >= 1.0f && std::isfinite(s->jacobianMax))) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: jacobianMax must be >= 1 and finite");
  if(s->reserved[0] != 0 || s->reserved[1] != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_gi_spatial: reserved fields must be 0");
  if(std::memcmp(&c->gis, s, sizeof(rt_gi_spatial)) == 0) return RT_OK;
  if(s->mode != c->gis.mode) {   // the indirect stream's share of the frame, which the stream priorities were decided on, has changed
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    reopenPriorityDecision(c);
  }
  c->gis = *s;
  return RT_OK;
}

int rt_get_gi_spatial(rt_ctx* c, rt_gi_spatial* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->gis;
  return RT_OK;
}

int rt_gi_spatial_readback(rt_ctx* c, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(!c->gisResv || !c->gisWritten) return fail(c, RT_ERR_NO_TARGET, "rt_gi_spatial_readback: no frame has been rendered with GI spatial reuse on since the last rt_resize");
  if(bytes != size_t(c->W / 2) * (c->H / 2) * sizeof(rt_indirect_reservoir)) return fail(c, RT_ERR_INVALID_ARG, "rt_gi_spatial_readback: size mismatch");
  return readbackDrained(c, c->gisResv, dst, bytes);
}

// ---- rt_set_taa: temporal anti-aliasing (csrc/taa.hip); the settings are host state read when a frame is enqueued
int rt_set_taa(rt_ctx* c, const rt_taa* t)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!t) return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: NULL settings");
  if(t->mode != RT_TAA_OFF && t->mode != RT_TAA_ON) return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: mode must be RT_TAA_OFF or RT_TAA_ON");
  if(t->jitterPhases < 0 || t->jitterPhases > 16) return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: jitterPhases must lie in 0..16");
  if(!(t->alpha > 0.0f && t->alpha <= 1.0f)) return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: alpha must lie in (0, 1]");
  if(!(t->clipGamma > 0.0f && std::isfinite(t->clipGamma))) return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: clipGamma must be positive and finite");
  for(int32_t r : t->reserved) if(r != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: reserved fields must be 0");
  if(t->mode == RT_TAA_ON && c->ups.mode != RT_UPSCALE_OFF)
    return fail(c, RT_ERR_INVALID_ARG, "rt_set_taa: temporal upsampling is on (rt_set_upscale), which brings its own jitter and resolve; switch it off first");
  if(std::memcmp(&c->taa, t, sizeof(rt_taa)) == 0) return RT_OK;
  if(t->mode != c->taa.mode) {   // compose's share of the frame, which the stream priorities were decided on, has changed
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    reopenPriorityDecision(c);
  }
  c->taa = *t;
  c->histTaa.state.invalidate();
  return RT_OK;
}

int rt_get_taa(rt_ctx* c, rt_taa* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->taa;
  return RT_OK;
}

int rt_taa_reset(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  c->histTaa.state.invalidate();
  return RT_OK;
}

int rt_taa_readback(rt_ctx* c, int which, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(which < 0 || which > 2) return fail(c, RT_ERR_INVALID_ARG, "rt_taa_readback: which must be 0 (direct), 1 (indirect) or 2 (history length)");
  const rt_ctx::History& h = c->histTaa;
  if(!h.plane[0][0] || h.state.last < 0) return fail(c, RT_ERR_NO_TARGET, "rt_taa_readback: no frame has been resolved since the last rt_resize");
  const size_t px = size_t(c->W) * c->H;
  if(bytes != px * (which < 2 ? sizeof(float4) : sizeof(float))) return fail(c, RT_ERR_INVALID_ARG, "rt_taa_readback: size mismatch");
  return readbackDrained(c, h.plane[h.state.last][which], dst, bytes);
}

// radical inverse of k in `base` as the exact fraction num / base^digits, divided once in IEEE double
static double radicalInverse(int k, int base)
{
  long long num = 0, den = 1;
  for(; k > 0; k /= base) { num = num * base + k % base; den *= base; }
  return double(num) / double(den);
}

// the one implementation of rt_taa_jitter_camera / rt_upscale_jitter_camera: the jittered camera and the offset (dx, dy) in pixels
static rt_scene_camera jitterCamera(const rt_scene_camera& in, int frames, int jitterPhases, int width, int height, float delta[2])
{
  rt_scene_camera cam = in;
  delta[0] = delta[1] = 0.0f;
  if(jitterPhases > 0) {
    const int k = ((frames % jitterPhases) + jitterPhases) % jitterPhases + 1;
    const float dx = float(radicalInverse(k, 2) - 0.5), dy = float(radicalInverse(k, 3) - 0.5);
    delta[0] = dx; delta[1] = dy;
    const float ox = (2.0f * dx) / float(width), oy = (2.0f * dy) / float(height);
    float* m = cam.projInverse.m;
    for(int r = 0; r < 4; r++) {
      const float a = m[0 + r] * ox, b = m[4 + r] * oy;   // (-ffp-contract=off: no fused multiply-add)
      m[12 + r] = (m[12 + r] + a) + b;
    }
  }
  return cam;
}

int rt_taa_jitter_camera(const rt_scene_camera* in, int frames, int jitterPhases, int width, int height, rt_scene_camera* out)
{
  if(!in || !out || jitterPhases < 0 || jitterPhases > 16 || width < 1 || height < 1) return RT_ERR_INVALID_ARG;
  float delta[2];
  *out = jitterCamera(*in, frames, jitterPhases, width, height, delta);
  return RT_OK;
}

// ---- rt_set_upscale: temporal upsampling (csrc/upscale.hip); the settings are host state read when a frame is enqueued
int rt_upscale_jitter_camera(const rt_scene_camera* in, int frames, int jitterPhases, int width, int height, rt_scene_camera* out, float delta[2])
{
  if(!in || !out || jitterPhases < 0 || jitterPhases > 64 || width < 1 || height < 1) return RT_ERR_INVALID_ARG;
  float d[2];
  *out = jitterCamera(*in, frames, jitterPhases, width, height, d);
  if(delta) { delta[0] = d[0]; delta[1] = d[1]; }
  return RT_OK;
}

int rt_set_upscale(rt_ctx* c, const rt_upscale* u)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!u) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: NULL settings");
  if(u->mode != RT_UPSCALE_OFF && u->mode != RT_UPSCALE_TEMPORAL) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: mode must be RT_UPSCALE_OFF or RT_UPSCALE_TEMPORAL");
  if(u->outWidth < 0 || u->outHeight < 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: outWidth and outHeight must not be negative");
  if(u->jitterPhases < 0 || u->jitterPhases > 64) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: jitterPhases must lie in 0..64");
  if(!(u->alpha > 0.0f && u->alpha <= 1.0f)) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: alpha must lie in (0, 1]");
  if(!(u->clipGamma > 0.0f && std::isfinite(u->clipGamma))) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: clipGamma must be positive and finite");
  for(int32_t r : u->reserved) if(r != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: reserved fields must be 0");
  if(u->mode == RT_UPSCALE_TEMPORAL) {
    if(u->outWidth < 1 || u->outHeight < 1) return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: outWidth and outHeight must be at least 1");
    if(c->W > 0 && !upscaleRatioOk(c->W, c->H, u->outWidth, u->outHeight))
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: the output size must satisfy W <= outWidth <= 4 W and H <= outHeight <= 4 H for the render size rt_resize set");
    if(c->taa.mode != RT_TAA_OFF)
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_upscale: TAA is on (rt_set_taa); temporal upsampling brings its own jitter and resolve, switch TAA off first");
  }
  if(std::memcmp(&c->ups, u, sizeof(rt_upscale)) == 0) return RT_OK;
  const bool sizeChange = c->histUps.plane[0][0] && (u->outWidth != c->upsW || u->outHeight != c->upsH);
  if(u->mode != c->ups.mode || sizeChange) {
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    if(u->mode != c->ups.mode) reopenPriorityDecision(c);   // compose's share of the frame, which the stream priorities were decided on, has changed
    if(sizeChange) freeUpscaleHistory(c);
  }
  c->ups = *u;
  c->histUps.state.invalidate();
  return RT_OK;
}

int rt_get_upscale(rt_ctx* c, rt_upscale* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->ups;
  return RT_OK;
}

int rt_upscale_reset(rt_ctx* c)
{
  if(!c) return RT_ERR_INVALID_ARG;
  c->histUps.state.invalidate();
  return RT_OK;
}

int rt_upscale_readback(rt_ctx* c, int which, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(which < 0 || which > 3) return fail(c, RT_ERR_INVALID_ARG, "rt_upscale_readback: which must be 0 (direct), 1 (indirect), 2 (history length) or 3 (LDR)");
  const rt_ctx::History& h = c->histUps;
  if(!h.plane[0][0] || h.state.last < 0) return fail(c, RT_ERR_NO_TARGET, "rt_upscale_readback: no frame has been resolved since the upsampling history was last freed");
  if(which == 3 && !c->upsLdrWritten) return fail(c, RT_ERR_NO_TARGET, "rt_upscale_readback: rt_upscale_tonemap has not run since the upsampling history was allocated");
  const size_t px = size_t(c->upsW) * c->upsH;
  if(bytes != px * (which < 2 ? sizeof(float4) : sizeof(float))) return fail(c, RT_ERR_INVALID_ARG, "rt_upscale_readback: size mismatch");
  return readbackDrained(c, which == 3 ? c->upsLdr : h.plane[h.state.last][which], dst, bytes);
}

int rt_upscale_tonemap(rt_ctx* c, const rt_tonemapper* tm, int frames)
{
  if(!c || !tm) return RT_ERR_INVALID_ARG;
  void* const* hist = c->histUps.plane[rt::frameParity(frames)];
  if(!hist[0] || !c->histUps.state.holds(frames))
    return fail(c, RT_ERR_NO_TARGET, "rt_upscale_tonemap: this frame was not resolved (rt_set_upscale), or its history has been overwritten or freed");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, joinInFlight(c));  // the resolved images of `frames` are complete once the pass (side stream) is done
  RT_HIP(c, launchTonemap(c->stream, static_cast<const float4*>(hist[0]), static_cast<const float4*>(hist[1]), c->upsRowSums, c->upsMean, *tm, 0,
                          c->upsW, c->upsH, static_cast<uint32_t*>(c->upsLdr), c->upsMipD, c->upsMipI));
  c->upsLdrWritten = true;
  return RT_OK;
}

// ---- rt_set_object_motion: object motion vectors (the RT_OM builds of csrc/stages.hip; include/rt_abi.h "Object motion vectors")
int rt_set_object_motion(rt_ctx* c, int mode)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(mode != RT_OBJECT_MOTION_OFF && mode != RT_OBJECT_MOTION_ON && mode != RT_OBJECT_MOTION_VERTEX)
    return fail(c, RT_ERR_INVALID_ARG, "rt_set_object_motion: mode must be RT_OBJECT_MOTION_OFF, RT_OBJECT_MOTION_ON or RT_OBJECT_MOTION_VERTEX");
  if(mode == c->objMotion) return RT_OK;
  const bool firstVertex = mode == RT_OBJECT_MOTION_VERTEX && !c->vmEver;
  if(firstVertex || (mode != RT_OBJECT_MOTION_OFF && c->W > 0 && (!c->omInst || (mode == RT_OBJECT_MOTION_VERTEX && !c->vmDelta)))) {
    // (a context that was resized, or given its scene, before the mode was first switched on)
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    if(mode == RT_OBJECT_MOTION_VERTEX) c->vmEver = true;
    int rc;
    if(mode == RT_OBJECT_MOTION_VERTEX && (rc = allocVertexMotionPlane(c))) return rc;
    if(c->W > 0 && (rc = allocObjectMotion(c))) return rc;
  }
  c->objMotion = mode;
  return RT_OK;
}

int rt_vertex_motion_readback(rt_ctx* c, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(!c->vmDelta || !c->vmDeltaValid) return fail(c, RT_ERR_NO_TARGET, "rt_vertex_motion_readback: no frame has been rendered with per-vertex motion vectors on since the last rt_resize");
  if(bytes != size_t(c->W) * c->H * sizeof(float4)) return fail(c, RT_ERR_INVALID_ARG, "rt_vertex_motion_readback: size mismatch");
  return readbackDrained(c, c->vmDelta, dst, bytes);
}

int rt_object_motion_readback(rt_ctx* c, void* dst, size_t bytes)
{
  if(!c || !dst) return RT_ERR_INVALID_ARG;
  if(!c->omInst || !c->omInstValid) return fail(c, RT_ERR_NO_TARGET, "rt_object_motion_readback: no frame has been rendered with object motion vectors on since the last rt_resize");
  if(bytes != size_t(c->W) * c->H * sizeof(uint32_t)) return fail(c, RT_ERR_INVALID_ARG, "rt_object_motion_readback: size mismatch");
  return readbackDrained(c, c->omInst, dst, bytes);
}

int rt_object_motion_camera(const rt_scene_camera* cam, const float prevObjectToWorld[12], const float curObjectToWorld[12], rt_scene_camera* out)
{
  if(!cam || !prevObjectToWorld || !curObjectToWorld || !out) return RT_ERR_INVALID_ARG;
  rt_scene_camera r = *cam;
  const float* P = prevObjectToWorld; const float* C = curObjectToWorld;
  float Pi[12], Ci[12], detP = 0.f, detC = 0.f;
  bool usable = std::memcmp(P, C, 12 * sizeof(float)) != 0;   // P == C bit for bit: the camera's own values, copied
  if(usable) {
    inverseAffine(P, Pi, &detP);
    inverseAffine(C, Ci, &detC);
    usable = detP != 0.0f && detC != 0.0f && std::isfinite(detP) && std::isfinite(detC);
    for(int a = 0; a < 12 && usable; a++) usable = std::isfinite(P[a]) && std::isfinite(C[a]) && std::isfinite(Pi[a]) && std::isfinite(Ci[a]);
  }
  if(usable) {
    // M = P · inverse(C), rows of 4 (the layout of rt_instance::objectToWorld); sums left to right, the translation last
    float M[12];
    for(int row = 0; row < 3; row++)
      for(int col = 0; col < 4; col++) {
        const float v = (P[4 * row] * Ci[col] + P[4 * row + 1] * Ci[4 + col]) + P[4 * row + 2] * Ci[8 + col];
        M[4 * row + col] = col == 3 ? v + P[4 * row + 3] : v;
      }
    // lastProjView_i = lastProjView · M (column-major m[c * 4 + r]; M's fourth row is 0 0 0 1)
    const float* L = cam->lastProjView.m;
    for(int row = 0; row < 4; row++)
      for(int col = 0; col < 4; col++) {
        const float v = (L[row] * M[col] + L[4 + row] * M[4 + col]) + L[8 + row] * M[8 + col];
        r.lastProjView.m[4 * col + row] = col == 3 ? v + L[12 + row] : v;
      }
    // lastPosition_i = C · (inverse(P) · lastPosition)
    float q[3], w[3];
    xformPointRaw(Pi, cam->lastPosition.x, cam->lastPosition.y, cam->lastPosition.z, q);
    xformPointRaw(C, q[0], q[1], q[2], w);
    r.lastPosition = rt_vec3{w[0], w[1], w[2]};
  }
  *out = r;
  return RT_OK;
}

int rt_set_overlap(rt_ctx* c, int mode)
{
  if(!c || mode < 0 || mode > 3) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  const bool hadShort = c->overlap >= 2;
  c->overlap = mode;
  if((mode >= 2) != hadShort) return ensureStackOverflow(c);   // the short LDS stacks of frames in flight spill into an HBM area that serial schedules do not hold
  return RT_OK;
}

/* Priorities of the indirect and the filter stream of the frames-in-flight schedule (levels -1 low, 0 normal, +1 high; the main stream keeps the level it was
 * created with).  Which setting is fastest depends on the workload (profiles/r05_prio_by_config_ab.txt); unset, the context decides at its first frame
 * (rt_render_frame: the rule and its data).  Best called BEFORE the first frame: a stream created after others exist may share a hardware queue with them.
 * Results are identical under every setting. */
int rt_set_stream_priorities(rt_ctx* c, int indirectLevel, int filterLevel)
{
  if(!c || indirectLevel < -1 || indirectLevel > 1 || filterLevel < -1 || filterLevel > 1) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  c->prioDecided = c->prioExplicit = true;   // an explicit choice: the probe-frame rule stays out of it, also after rt_resize / a new scene
  if(c->prio[1] == indirectLevel && c->prio[2] == filterLevel) return RT_OK;
  c->prio[1] = indirectLevel; c->prio[2] = filterLevel;
  c->indStream = c->sideStream = nullptr;   // (selected — and created, once per level — on first use: ensureOverlapStreams; streams of other levels stay alive, idle)
  return RT_OK;
}

/* The levels in use and the measurement behind them: filterShare = filters / (direct + indirect) of the last probe frame, every stage alone (-1: no frame yet, or the
 * levels were set explicitly / by RESTIR_PRIO); decided = 0 while the probe frames have not all been rendered. */
int rt_get_stream_priorities(rt_ctx* c, int* indirectLevel, int* filterLevel, float* filterShare, int* decided)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(indirectLevel) *indirectLevel = c->prio[1];
  if(filterLevel) *filterLevel = c->prio[2];
  if(filterShare) *filterShare = c->filterShare;
  if(decided) *decided = c->prioDecided ? 1 : 0;
  return RT_OK;
}

/* The context's three streams of the frames-in-flight schedule, for a host that issues the stages itself (rt_run_stage + rt_set_stream: restir_amd/tiled.py,
 * csrc/mgpu.cpp).  Creates the filter and the indirect stream if they do not exist yet — with the current levels, in the order the schedule was tuned for (filter
 * stream first, then the indirect stream, nothing in between) — so that such a host runs on the SAME stream layout as rt_render_frame instead of on streams from
 * another pool created whenever (round-5 finding: a stream's place in the process's creation order is worth 15-75 % of a frame).  Call it before anything else in the
 * process creates streams (torch's pool, RCCL's communicator).  The handles stay owned by the context. */
int rt_get_streams(rt_ctx* c, void** mainStream, void** indirectStream, void** filterStream)
{
  if(!c) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  if(indirectStream || filterStream) {   // (asking for the main stream alone creates nothing: csrc/mgpu.cpp creates a rank's other two on its first frame in flight)
    RT_HIP(c, ensureOverlapStreams(c));
    c->prioDecided = true;   // the levels these streams were created with stand: a later rt_render_frame does not probe and switch
  }
  if(mainStream) *mainStream = c->ownStream;
  if(indirectStream) *indirectStream = c->indStream;
  if(filterStream) *filterStream = c->sideStream;
  return RT_OK;
}

/* Where this context's streams sit in the process's creation order: created = HIP streams this LIBRARY has created in the process so far (all contexts; streams made by
 * the host — torch's pool, RCCL — are not visible to it), index[0..2] = creation index of the main / indirect / filter stream in use (-1: not created yet).  bench.py
 * prints it with every N > 1 line (`stream_layout`). */
int rt_get_stream_layout(rt_ctx* c, int* created, int index[3])
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(created) *created = g_streamsCreated.load();
  if(index) { index[0] = c->mainIdx; index[1] = c->indStream ? c->indIdx[c->prio[1] + 1] : -1; index[2] = c->sideStream ? c->sideIdx[c->prio[2] + 1] : -1; }
  return RT_OK;
}

/* ---- moving instances: leaf-record rewrite + BVH8 refit (include/rt_abi.h "Moving instances", csrc/refit.hip) ---- */
}  // extern "C"

// what the calls that change a built tree open with; the message carries the caller's name
static int needTree(rt_ctx* c, const char* who)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(c->haveScene && c->haveAccel) return RT_OK;
  c->err = std::string(who) + (c->haveScene ? ": rt_build_accel has not run" : ": no scene uploaded");
  return c->haveScene ? RT_ERR_NO_ACCEL : RT_ERR_NO_SCENE;
}

// the per-instance bit tables of k_refit_tris (dDirty, dFlip): one bit per instance and a spare word; bit i is set where pred(i)
static size_t instanceWords(size_t nInst) { return (nInst + 31) / 32 + 1; }
template <class P> static std::vector<uint32_t> instanceBits(size_t nInst, P pred)
{
  std::vector<uint32_t> w(instanceWords(nInst), 0u);
  for(size_t i = 0; i < nInst; i++) if(pred(i)) w[i >> 5] |= 1u << (i & 31u);
  return w;
}

// largest |world coordinate| over the triangles of instance i under matrix m: the builder's expression (buildBvh8, flatten), per instance
static float meshCoordMax(const rt_ctx* c, uint32_t primMesh, const float* m)
{
  const rt_prim_mesh& pm = c->primMeshes[primMesh];
  float sm = 0.f;
  for(uint32_t k = 0; k < pm.indexCount; k++) {
    const rt_vec3& q = c->vertices[pm.vertexOffset + c->indices[pm.firstIndex + k]].position;
    float w[3];
    xformPointRaw(m, q.x, q.y, q.z, w);
    for(int a = 0; a < 3; a++) sm = std::max(sm, std::fabs(w[a]));
  }
  return sm;
}
static float instanceCoordMax(const rt_ctx* c, uint32_t i, const float* m) { return meshCoordMax(c, c->instances[i].primMesh, m); }

// what every update needs and no frame does, derived once per tree from the device arrays: the record -> node map, the level ranges, the per-instance maxima
static int ensureRefitState(rt_ctx* c)
{
  rt_ctx::Refit& R = c->refit;
  if(R.ready) return RT_OK;
  const size_t nNodes = c->ds.numNodes, nRecs = c->ds.numTris, nInst = c->instances.size();
  std::vector<Node8> nodes(nNodes);
  RT_HIP(c, hipMemcpy(nodes.data(), c->ds.nodes, nNodes * sizeof(Node8), hipMemcpyDeviceToHost));
  R.inst.resize(nInst);
  if(nInst) RT_HIP(c, hipMemcpy(R.inst.data(), c->ds.instances, nInst * sizeof(DevInstance), hipMemcpyDeviceToHost));
  // the builder emits wide nodes breadth-first: the nodes of a level are a contiguous range that starts where the level above ends
  R.levels.clear();
  std::vector<uint32_t> recNode(std::max<size_t>(nRecs, 1), 0u);
  uint32_t first = 0, count = 1;
  while(count > 0 && size_t(first) + count <= nNodes) {
    R.levels.push_back({first, count});
    uint32_t next = 0;
    for(uint32_t n = first; n < first + count; n++) {
      const Node8& N = nodes[n];
      next += uint32_t(__builtin_popcount(N.imask));
      for(int s = 0; s < 8; s++) {
        if(N.meta[s] == 0 || ((N.imask >> s) & 1u)) continue;
        const uint32_t cnt = uint32_t(__builtin_popcount(uint32_t(N.meta[s]) >> 5)), off = uint32_t(N.meta[s]) & 31u;
        for(uint32_t q = 0; q < cnt; q++) if(size_t(N.triBase) + off + q < nRecs) recNode[size_t(N.triBase) + off + q] = n;
      }
    }
    first += count; count = next;
  }
  if(size_t(first) != nNodes) return fail(c, RT_ERR_INVALID_ARG, "rt_update_instances: the tree's levels are not contiguous node ranges");
  { const int rc = syncHostVertices(c); if(rc) return rc; }
  R.instMax.resize(nInst); R.flip.resize(nInst);
  for(uint32_t i = 0; i < nInst; i++) {
    R.instMax[i] = instanceCoordMax(c, i, c->instances[i].objectToWorld);
    float inv[12], det;
    inverseAffine(R.inst[i].o2w, inv, &det);
    R.flip[i] = det < 0.0f;
  }
  const size_t words = instanceWords(nInst);
  int rc;
  const uint32_t* up = nullptr;
  if((rc = allocZeroed(c, c->accelAllocs, words, &R.dDirty))) return rc;
  if((rc = allocZeroed(c, c->accelAllocs, words, &R.dFlip))) return rc;
  if((rc = upload(c, c->accelAllocs, recNode.data(), recNode.size(), &up))) return rc;
  R.dRecNode = const_cast<uint32_t*>(up);
  if((rc = allocZeroed(c, c->accelAllocs, std::max<size_t>(nNodes, 1), &R.dNodeDirty))) return rc;
  if((rc = allocZeroed(c, c->accelAllocs, 4, &R.dCounters))) return rc;
  if(const hipError_t he = ensureEvents(c->evRefit)) return hipFail(c, "hipEventCreate(&e)", he);
  R.treePad = c->ds.triPad;
  R.ready = true;
  return RT_OK;
}

// The argument block of the refit kernels (refitTail, and the full-mode pass that ends a device build): the tree arrays, the table the records are made from, the
// bit tables and counters; the mesh arrays are the scene's.
static RefitArgs refitArgs(const rt_ctx* c, Node8* nodes, Tri48* tris, const uint32_t* recNode, uint32_t* nodeDirty, const TriRef* triRef, const DevInstance* instances,
                           const uint32_t* dirtyBits, const uint32_t* flipBits, uint32_t* counters, uint32_t numRecs, float pad, bool full)
{
  RefitArgs a{};
  a.nodes = nodes; a.tris = tris; a.triRef = triRef; a.instances = instances;
  a.primMeshes = c->ds.primMeshes; a.vertices = c->ds.vertices; a.indices = c->ds.indices;
  a.dirtyBits = dirtyBits; a.flipBits = flipBits; a.recNode = recNode; a.nodeDirty = nodeDirty; a.counters = counters;
  a.numRecs = numRecs; a.pad = pad; a.full = full ? 1 : 0;
  return a;
}

// The refit every update ends with (rt_update_instances, rt_update_vertices, rt_update_skins).  dirty[i] != 0: instance i moved or deformed; R.inst, R.instMax and
// R.flip already hold its new state, and the caller has recorded evRefit[0] and enqueued what the kernels read (instance rows, vertices).  From the pad to R.stats:
// the dirty and flip words, the cleared node marks and counters, k_refit_tris, k_refit_level deepest level first, the counters, evRefit[1], one synchronise.
static int refitTail(rt_ctx* c, const std::vector<uint8_t>& dirty)
{
  dropPrimaryReplay(c);   // leaf records are about to be rewritten
  rt_ctx::Refit& R = c->refit;
  const uint32_t count = uint32_t(dirty.size() - std::count(dirty.begin(), dirty.end(), uint8_t(0)));   // the predicate of the dirty bits: != 0
  const std::vector<uint32_t> dirtyBits = instanceBits(dirty.size(), [&](size_t i) { return dirty[i] != 0; });
  // k_refit_tris rewrites TRI_FLIP of every dirty record: the handedness of the instance's current matrix
  const std::vector<uint32_t> flipBits = instanceBits(dirty.size(), [&](size_t i) { return dirty[i] && R.flip[i]; });
  const float triPad = triPadOf(R.instMax);
  const bool full = triPad > R.treePad && c->ds.numTris > 0;
  if(triPad > R.treePad) R.treePad = triPad;
  hipStream_t s = c->stream;
  RT_HIP(c, hipMemcpyAsync(R.dDirty, dirtyBits.data(), dirtyBits.size() * 4, hipMemcpyHostToDevice, s));
  RT_HIP(c, hipMemcpyAsync(R.dFlip, flipBits.data(), flipBits.size() * 4, hipMemcpyHostToDevice, s));
  RT_HIP(c, hipMemsetAsync(R.dNodeDirty, 0, std::max<size_t>(c->ds.numNodes, 1) * 4, s));
  RT_HIP(c, hipMemsetAsync(R.dCounters, 0, 16, s));
  uint32_t counters[4] = {0, 0, 0, 0};
  if(c->ds.numTris > 0 && (count > 0 || full)) {
    const RefitArgs a = refitArgs(c, const_cast<Node8*>(c->ds.nodes), const_cast<Tri48*>(c->ds.tris), R.dRecNode, R.dNodeDirty, c->ds.triRef, c->ds.instances,
                                  R.dDirty, R.dFlip, R.dCounters, c->ds.numTris, R.treePad, full);
    RT_HIP(c, launchRefitTris(s, a));
    for(size_t l = R.levels.size(); l-- > 0;) RT_HIP(c, launchRefitLevel(s, a, R.levels[l].first, R.levels[l].second));
    RT_HIP(c, hipMemcpyAsync(counters, R.dCounters, 16, hipMemcpyDeviceToHost, s));
  }
  // bound triangle-light records of the refitted instances follow them (csrc/light_records.hip): the instance rows and the vertices are in place on this stream
  rt_ctx::Lights& L = c->lights;
  uint32_t lightsRewritten = 0;
  if(L.bound) {
    RT_HIP(c, hipMemsetAsync(L.dCounter, 0, 4, s));
    RT_HIP(c, hipEventRecord(c->evLights[0], s));
    if(count > 0) {
      LightRecArgs la{};
      la.records = const_cast<rt_trig_light*>(c->ds.trigLights); la.sources = L.dSources; la.instances = c->ds.instances; la.primMeshes = c->ds.primMeshes;
      la.vertices = c->ds.vertices; la.indices = c->ds.indices; la.dirtyBits = R.dDirty; la.counter = L.dCounter; la.numRecs = L.bound; la.all = 0u;
      RT_HIP(c, launchLightRecords(s, la));
    }
    RT_HIP(c, hipEventRecord(c->evLights[1], s));
    RT_HIP(c, hipMemcpyAsync(&lightsRewritten, L.dCounter, 4, hipMemcpyDeviceToHost, s));
  }
  RT_HIP(c, hipEventRecord(c->evRefit[1], s));
  RT_HIP(c, hipStreamSynchronize(s));
  if(L.bound) {
    L.stats.rewritten = lightsRewritten; L.stats.lightBytesCopied = 0u; L.stats.ms = 0.f;
    (void)hipEventElapsedTime(&L.stats.ms, c->evLights[0], c->evLights[1]);
  }
  c->ds.triPad = triPad;
  c->refN = 0;   // the scene changed: the reference sums start again
  R.stats = rt_refit_stats{};
  R.stats.instances = count; R.stats.leafRecords = counters[0]; R.stats.nodes = counters[1]; R.stats.levels = uint32_t(R.levels.size());
  R.stats.fullRefit = full ? 1u : 0u; R.stats.triPad = triPad; R.stats.treePad = R.treePad;
  (void)hipEventElapsedTime(&R.stats.ms, c->evRefit[0], c->evRefit[1]);
  return RT_OK;
}

// One device instance row from an object-to-world matrix (rt_update_instances, rt_set_instances): the builder's own expression (buildBvh8, flatten), inverse
// included.  Returns why the matrix is refused, or nullptr; *flip tells whether it mirrors (TRI_FLIP).
static const char* makeInstanceRow(const float o2w[12], uint32_t primMesh, uint32_t flags, DevInstance& out, bool* flip)
{
  for(int a = 0; a < 12; a++) if(!std::isfinite(o2w[a])) return "non-finite matrix entry";
  memcpy(out.o2w, o2w, sizeof(out.o2w));
  float det;
  inverseAffine(out.o2w, out.w2o, &det);
  if(!(det != 0.0f) || !std::isfinite(det)) return "singular matrix";
  for(int a = 0; a < 12; a++) if(!std::isfinite(out.w2o[a])) return "the matrix has no finite inverse";
  out.primMesh = primMesh; out.flags = flags; out.pad[0] = out.pad[1] = 0;
  *flip = det < 0.0f;
  return nullptr;
}

extern "C" {

int rt_update_instances(rt_ctx* c, uint32_t count, const uint32_t* ids, const float* xf)
{
  if(int rc = needTree(c, "rt_update_instances")) return rc;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  if(count && (!ids || !xf)) return fail(c, RT_ERR_INVALID_ARG, "rt_update_instances: NULL ids / matrices");
  const size_t nInst = c->instances.size();
  // the whole call is checked before anything changes
  std::vector<DevInstance> rows(count);
  std::vector<uint8_t> flip(count, 0);
  {
    std::vector<bool> seen(nInst, false);
    for(uint32_t k = 0; k < count; k++) {
      if(ids[k] >= nInst) return fail(c, RT_ERR_INVALID_ARG, "rt_update_instances: instance id out of range");
      if(seen[ids[k]]) return fail(c, RT_ERR_INVALID_ARG, "rt_update_instances: duplicate instance id");
      seen[ids[k]] = true;
      bool mirrored;
      if(const char* why = makeInstanceRow(xf + 12 * k, c->instances[ids[k]].primMesh, c->instances[ids[k]].flags, rows[k], &mirrored))
        return fail(c, RT_ERR_INVALID_ARG, (std::string("rt_update_instances: ") + why).c_str());
      flip[k] = mirrored;
    }
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // v1: joins the frames in flight
  int rc;
  if((rc = ensureRefitState(c))) return rc;
  rt_ctx::Refit& R = c->refit;
  for(uint32_t k = 0; k < count; k++) if((rc = syncHostVertices(c, int(c->instances[ids[k]].primMesh)))) return rc;   // instanceCoordMax reads the context's copy
  std::vector<uint8_t> moved(nInst, 0);
  if(c->omPrev.size() != nInst) { c->omPrev.assign(nInst, std::array<float, 12>{}); c->omMoved.assign(nInst, 0); c->omPending = false; }
  for(uint32_t k = 0; k < count; k++) {
    const uint32_t i = ids[k];
    if(!c->omMoved[i]) {   // the matrix of the last rendered frame, recorded once: a second update before the next frame keeps it
      memcpy(c->omPrev[i].data(), c->instances[i].objectToWorld, sizeof(rows[k].o2w));
      c->omMoved[i] = 1; c->omPending = true;
    }
    memcpy(c->instances[i].objectToWorld, rows[k].o2w, sizeof(rows[k].o2w));
    R.inst[i] = rows[k];
    R.instMax[i] = instanceCoordMax(c, i, rows[k].o2w);
    R.flip[i] = flip[k];
    moved[i] = 1;
  }
  hipStream_t s = c->stream;
  RT_HIP(c, hipEventRecord(c->evRefit[0], s));
  DevInstance* dInst = const_cast<DevInstance*>(c->ds.instances);
  if(count * 4 > nInst) RT_HIP(c, hipMemcpyAsync(dInst, R.inst.data(), nInst * sizeof(DevInstance), hipMemcpyHostToDevice, s));
  else for(uint32_t k = 0; k < count; k++) RT_HIP(c, hipMemcpyAsync(dInst + ids[k], &rows[k], sizeof(DevInstance), hipMemcpyHostToDevice, s));
  return refitTail(c, moved);
}

int rt_update_lights(rt_ctx* c, const rt_trig_light* trig, uint32_t numTrig, const rt_punc_light* punc, uint32_t numPunc, const rt_light_buf_info* info)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_update_lights: no scene uploaded");
  if(!info || numTrig != c->ds.lightInfo.trigLightSize || numPunc != c->ds.lightInfo.puncLightSize || info->trigLightSize != numTrig || info->puncLightSize != numPunc)
    return fail(c, RT_ERR_INVALID_ARG, "rt_update_lights: the light counts must equal the uploaded ones");
  if((numTrig && !trig) || (numPunc && !punc)) return fail(c, RT_ERR_INVALID_ARG, "rt_update_lights: NULL light array");
  for(uint32_t i = 0; i < numTrig; i++)
    if(trig[i].matIndex >= c->materials.size() || trig[i].impSamp.alias < 0 || uint32_t(trig[i].impSamp.alias) >= numTrig)
      return fail(c, RT_ERR_INVALID_ARG, "rt_update_lights: triangle light with a bad material or alias index");
  for(uint32_t i = 0; i < numPunc; i++)
    if(punc[i].impSamp.alias < 0 || uint32_t(punc[i].impSamp.alias) >= numPunc) return fail(c, RT_ERR_INVALID_ARG, "rt_update_lights: punctual light with a bad alias index");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  if(numTrig) RT_HIP(c, hipMemcpy(const_cast<rt_trig_light*>(c->ds.trigLights), trig, numTrig * sizeof(rt_trig_light), hipMemcpyHostToDevice));
  if(numPunc) RT_HIP(c, hipMemcpy(const_cast<rt_punc_light*>(c->ds.puncLights), punc, numPunc * sizeof(rt_punc_light), hipMemcpyHostToDevice));
  c->ds.lightInfo.trigSampProb = info->trigSampProb;
  c->refN = 0;
  c->lights.stats.rewritten = 0u; c->lights.stats.ms = 0.f;   // the binding stays in place
  c->lights.stats.lightBytesCopied = uint32_t(numTrig * sizeof(rt_trig_light) + numPunc * sizeof(rt_punc_light));
  return RT_OK;
}

}  // extern "C"

// The device build both rt_rebuild_accel and rt_set_instances run, on a stream that holds what the caller has enqueued for it (flip bits, and for a new table its
// rows and records; w.n, w.table and the options are set).  `a`: the full-mode refit block of the target set, over numInst instances.  Clears the counters, marks
// every instance moved, builds, records evRebuild[3] and synchronises.  A failure leaves the stream idle and only the target set and the working buffers written;
// the code and the context's message carry `who`.
static int runDeviceBuild(rt_ctx* c, const char* who, hipStream_t s, AccelBuildWork& work, const AccelBuildSet& target, const RefitArgs& a, size_t numInst,
                          const AlphaRec* alphaRec, AccelBuildResult& res)
{
  hipError_t he = hipMemsetAsync(const_cast<uint32_t*>(a.dirtyBits), 0xff, instanceWords(numInst) * 4, s);
  if(he == hipSuccess) he = hipMemsetAsync(a.counters, 0, 16, s);
  int br = ACCEL_BUILD_HIP;
  if(he == hipSuccess) br = accelBuildRun(s, work, target, a, alphaRec, STACK_MAX, c->evRebuild + 1, res, &he);
  if(br == ACCEL_BUILD_OK) {
    if((he = hipEventRecord(c->evRebuild[3], s)) == hipSuccess) he = hipStreamSynchronize(s);
    if(he == hipSuccess) return RT_OK;
    br = ACCEL_BUILD_HIP;
  }
  (void)hipStreamSynchronize(s);
  if(br == ACCEL_BUILD_HIP) return hipFail(c, who, he);
  c->err = std::string(who) + ": " + (br == ACCEL_BUILD_TOO_DEEP ? "BVH8 deeper than the traversal stack" : accelBuildWhy(br));
  const bool ofScene = br == ACCEL_BUILD_TOO_DEEP || br == ACCEL_BUILD_PLOC_ITERATIONS;   // every other code: a builder invariant, not the caller's argument
  return ofScene ? RT_ERR_INVALID_ARG : RT_ERR_HIP;
}

// The context adopts a tree the device builder has completed (rt_rebuild_accel, rt_set_instances).  `next` is c->ds with the caller's own arrays and the new pad;
// the tree is set `ts` of `W`, the buffers the build ran in; the node and record counts, the traversal stack and rt_accel_stats' numbers follow from `res`.  Where
// the new stack cannot be allocated the previous tree stays, with its stack.  Otherwise the update calls work on the new tree (its maps come from the build),
// W.stats tells of the build, the reference sums start again and the seed plane is emptied: the records are in a new order.  *adopted (optional) tells a caller
// with state of its own to swap which of the two it was; a code with the tree adopted is the seed plane's.
static int adoptDeviceTree(rt_ctx* c, DevScene next, rt_ctx::Rebuild& W, int ts, const AccelBuildResult& res, uint32_t n, bool* adopted = nullptr)
{
  if(adopted) *adopted = false;
  const AccelBuildSet& T = W.set[ts];
  const int depth = int(res.levels.size());
  const int stackTotal = std::max(8, ((depth + 1 + 3) / 4) * 4);
  const DevScene old = c->ds;
  next.nodes = T.nodes; next.tris = T.tris; next.alphaByTri = T.alphaByTri;
  c->ds = next;
  c->ds.numNodes = res.nodes; c->ds.numTris = n;
  if(stackTotal != old.stackTotal) {
    c->ds.stackTotal = stackTotal; c->ds.stackEntries = stackTotal;
    if(const int rc = ensureStackOverflow(c)) {
      const std::string msg = c->err;
      c->ds = old; c->ds.stackOvf = c->ds.stackOvfInd = nullptr; c->ds.stackOvfThreads = 0;
      (void)ensureStackOverflow(c);
      c->err = msg;
      return rc;
    }
  }
  if(adopted) *adopted = true;
  c->numNodes = res.nodes; c->numRefs = n; c->spatialSplits = 0; c->maxDepth = depth;
  c->sahNodeSteps = c->sahTriSteps = 0;   // (the host builder's SAH expectation: not computed on the device)
  W.cur = ts;
  rt_ctx::Refit& R = c->refit;
  R.levels = res.levels; R.dRecNode = T.recNode; R.dNodeDirty = W.work.nodeDirty; R.treePad = next.triPad;
  rt_rebuild_stats st{};
  st.triangles = n; st.nodes = res.nodes; st.levels = st.maxDepth = uint32_t(depth); st.triPad = next.triPad; st.iterations = W.work.iterations;
  (void)hipEventElapsedTime(&st.ms, c->evRebuild[0], c->evRebuild[3]);
  (void)hipEventElapsedTime(&st.sortMs, c->evRebuild[1], c->evRebuild[2]);
  W.stats = st;
  c->refN = 0;
  return resetSeedPlane(c);
}

// The options of rt_set_rebuild_options go into the working state of the next build; the first PLOC build on these buffers allocates PLOC's own into `pool`
// (*allocated tells).  A failure leaves `w` and `pool` as they were.
static hipError_t applyRebuildOptions(const rt_ctx* c, AccelBuildWork& w, std::vector<void*>& pool, bool* allocated)
{
  *allocated = false;
  w.builder = c->rebuildOpt.builder; w.radius = uint32_t(c->rebuildOpt.radius); w.maxIterations = uint32_t(c->rebuildOpt.maxIterations);
  return w.builder == ACCEL_BUILDER_PLOC ? accelBuildAllocPloc(w, pool, allocated) : hipSuccess;
}

extern "C" {

/* ---- the builder of the device rebuild (include/rt_abi.h "The PLOC builder"): the call builds nothing and drops nothing ---- */
int rt_set_rebuild_options(rt_ctx* c, const rt_rebuild_options* o)
{
  if(!c || !o) return RT_ERR_INVALID_ARG;
  if(o->builder != RT_REBUILD_LBVH && o->builder != RT_REBUILD_PLOC) return fail(c, RT_ERR_INVALID_ARG, "rt_set_rebuild_options: builder must be RT_REBUILD_LBVH or RT_REBUILD_PLOC");
  if(o->radius < 0 || o->radius > ACCEL_PLOC_RADIUS_MAX) return fail(c, RT_ERR_INVALID_ARG, "rt_set_rebuild_options: radius must be 1..64, or 0 for the default");
  if(o->maxIterations < 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_rebuild_options: maxIterations must be positive, or 0 for the default");
  if(o->reserved != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_rebuild_options: reserved must be 0");
  c->rebuildOpt = *o;
  if(o->radius == 0) c->rebuildOpt.radius = ACCEL_PLOC_RADIUS_DEFAULT;
  if(o->maxIterations == 0) c->rebuildOpt.maxIterations = ACCEL_PLOC_ITERATIONS_DEFAULT;
  return RT_OK;
}

int rt_get_rebuild_options(rt_ctx* c, rt_rebuild_options* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->rebuildOpt;
  return RT_OK;
}

/* ---- rebuilding on the device: LBVH or PLOC -> BVH8 (include/rt_abi.h "Rebuilding on the device", csrc/accel_build.hip) ---- */
int rt_rebuild_accel(rt_ctx* c)
{
  if(int rc = needTree(c, "rt_rebuild_accel")) return rc;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // drains the frames in flight, like rt_update_instances
  int rc;
  if((rc = ensureRefitState(c))) return rc;
  rt_ctx::Refit& R = c->refit;
  rt_ctx::Rebuild& B = c->rebuild;
  const uint32_t n = uint32_t(c->numTris);
  hipStream_t s = c->stream;
  if(!B.ready) {   // the first rebuild after a host build: buffers, and the per-triangle table from the host tree's records (still the context's tree)
    hipError_t e = accelBuildAlloc(B.work, B.set, n, c->rebuildAllocs);
    const bool queued = e == hipSuccess;
    if(e == hipSuccess) e = launchAccelTable(s, c->ds.tris, c->ds.numTris, B.work);
    if(e == hipSuccess) e = ensureEvents(c->evRebuild);
    if(e != hipSuccess) {   // nothing of a first rebuild that failed is kept: the next call starts again
      if(queued) (void)hipStreamSynchronize(s);
      freePool(c->rebuildAllocs); B = rt_ctx::Rebuild{};
      return hipFail(c, "rt_rebuild_accel", e);
    }
    B.ready = true;
  }
  {
    bool allocated = false;
    const hipError_t e = applyRebuildOptions(c, B.work, c->rebuildAllocs, &allocated);
    if(e != hipSuccess) return hipFail(c, "rt_rebuild_accel", e);
  }
  const float triPad = triPadOf(R.instMax);   // the pad of the scene as it is now (kept by the update calls)
  RT_HIP(c, hipEventRecord(c->evRebuild[0], s));
  if(n == 0) {   // no triangles: the single empty node stays
    rt_rebuild_stats st{};
    st.triPad = triPad; st.nodes = uint32_t(c->numNodes); st.levels = st.maxDepth = uint32_t(c->maxDepth);
    c->refN = 0;   // the reference sums start again
    B.stats = st;
    return resetSeedPlane(c);
  }
  // every instance's handedness, as the update calls keep it
  const std::vector<uint32_t> flipBits = instanceBits(c->instances.size(), [&](size_t i) { return R.flip[i] != 0; });
  RT_HIP(c, hipMemcpyAsync(R.dFlip, flipBits.data(), flipBits.size() * 4, hipMemcpyHostToDevice, s));
  const int target = B.cur == 0 ? 1 : 0;
  const AccelBuildSet& T = B.set[target];
  const RefitArgs a = refitArgs(c, T.nodes, T.tris, T.recNode, B.work.nodeDirty, c->ds.triRef, c->ds.instances, R.dDirty, R.dFlip, R.dCounters, n, triPad, true);
  AccelBuildResult res;
  // a build that failed leaves the context's tree as it was: only the other set and the working buffers were written
  if((rc = runDeviceBuild(c, "rt_rebuild_accel", s, B.work, T, a, c->instances.size(), c->ds.alphaRec, res))) return rc;
  DevScene next = c->ds;
  next.triPad = triPad;
  return adoptDeviceTree(c, next, B, target, res, n);
}

int rt_get_rebuild_stats(rt_ctx* c, rt_rebuild_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->rebuild.stats;
  return RT_OK;
}

}  // extern "C"

/* ---- adding and removing instances (include/rt_abi.h "Adding and removing instances", csrc/instances.hip) ---- */
// the scene's light rule (host/scene.cpp createTrigLightBuffer): a prim mesh whose material's emissive luminance exceeds 1e-2 has triangle-light records
static float luminance(const rt_vec3& e) { return e.x * 0.2126f + e.y * 0.7152f + e.z * 0.0722f; }
static bool emissiveMesh(const rt_ctx* c, uint32_t primMesh)
{
  const rt_prim_mesh& pm = c->primMeshes[primMesh];
  return luminance(c->materials[size_t(pm.materialIndex > 0 ? pm.materialIndex : 0)].emissiveFactor) > 1e-2f;
}

// hipMalloc into a pool, for a run of allocations that share one error: nothing once an earlier one has failed
template <class T> static void pooledAlloc(hipError_t& e, std::vector<void*>& pool, size_t bytes, T** out)
{
  if(e != hipSuccess) return;
  void* p = nullptr;
  e = hipMalloc(&p, bytes);
  if(e == hipSuccess) { pool.push_back(p); *out = static_cast<T*>(p); }
}

// the buffers of rt_set_instances at a capacity: the rebuild's working buffers and two trees, and what the expansion writes, twice
static hipError_t allocInstanceBuffers(rt_ctx::Rebuild& B, uint32_t triCap, uint32_t instCap, std::vector<void*>& pool)
{
  hipError_t e = accelBuildAlloc(B.work, B.set, triCap, pool);
  auto get = [&](size_t bytes, auto** out) { pooledAlloc(e, pool, bytes, out); };
  B.table[0] = B.work.table;
  get(size_t(triCap) * sizeof(Tri48), &B.table[1]);
  for(int k = 0; k < 2; k++) { get(size_t(triCap) * sizeof(TriRef), &B.triRef[k]); get(size_t(instCap) * sizeof(DevInstance), &B.inst[k]); }
  get((size_t(instCap) + 1) * 4, &B.prefix);
  get(instanceWords(instCap) * 4, &B.dDirty); get(instanceWords(instCap) * 4, &B.dFlip); get(16, &B.dCounters);
  if(e == hipSuccess) { B.triCap = triCap; B.instCap = instCap; B.icur = 0; B.cur = -1; B.instReady = true; B.ready = true; }
  return e;
}

// the templates of prim mesh `mesh` (alphaTemplate per triangle, texture addresses of this device) at their place in the device arrays
static int makeMeshTemplates(rt_ctx* c, uint32_t mesh, uint32_t* bytesUploaded)
{
  rt_ctx::InstTemplates& TP = c->inst;
  if(const int rc = syncHostVertices(c, int(mesh))) return rc;   // (the texcoords are read from the context's copy)
  const rt_prim_mesh& pm = c->primMeshes[mesh];
  const uint32_t nt = pm.indexCount / 3;
  std::vector<AlphaRec> alpha(nt);
  std::vector<std::array<uint32_t, 4>> omm(nt);
  OmmCache cache;
  for(uint32_t p = 0; p < nt; p++) {
    int32_t tex = -1;
    alphaTemplate(c, pm, p, cache, alpha[p], tex, omm[p]);
    if(tex >= 0) alpha[p].bgra = c->devTextures[size_t(tex)].bgra;
  }
  const size_t first = size_t(TP.meshAlphaBase[mesh]) + 1;
  if(nt) {
    RT_HIP(c, hipMemcpy(TP.dAlpha + first, alpha.data(), size_t(nt) * sizeof(AlphaRec), hipMemcpyHostToDevice));
    RT_HIP(c, hipMemcpy(TP.dOmm + first, omm.data(), size_t(nt) * 16, hipMemcpyHostToDevice));
  }
  *bytesUploaded += nt * uint32_t(sizeof(AlphaRec) + 16);
  TP.meshMade[mesh] = 1;
  return RT_OK;
}

/* ---- emitters: triangle-light records derived from the instance table (include/rt_abi.h "Emitters", csrc/light_derive.hip) ---- */
// What the host contributes to the derived list of a table: the emitting instances and their first records, the alias entries, the count and trigSampProb.
struct EmitPlan {
  std::vector<uint32_t> ids, prefix;     // emitting instances ascending; prefix has one word more (the record count)
  std::vector<rt_impt_samp> alias;       // per record
  uint32_t records = 0;
  float trigSampProb = 0.f;
};

// bytes a plan moves host -> device: the alias entries, the prefix words and the ids (the formula of include/rt_abi.h)
static uint32_t emitPlanBytes(const EmitPlan& P) { return uint32_t(P.alias.size() * sizeof(rt_impt_samp) + (P.prefix.size() + P.ids.size()) * 4); }

// The plan of `instances` under the templates (meshFirstRow[m] < 0: prim mesh m has none).  RT_ERR_INVALID_ARG for an instance of an emissive prim mesh
// without a template.  The alias table is the host Scene's (createTrigLightBuffer): weights luminance(emissiveFactor), total summed in record order.
static int planEmitters(rt_ctx* c, const char* who, uint32_t numInstances, const rt_instance* instances, const std::vector<int64_t>& meshFirstRow,
                        const std::vector<uint32_t>& meshRows, float puncWeight, EmitPlan& P)
{
  uint64_t recs = 0;
  std::vector<float> distrib;
  for(uint32_t i = 0; i < numInstances; i++) {
    const uint32_t mesh = instances[i].primMesh;
    if(meshFirstRow[mesh] < 0) {
      if(emissiveMesh(c, mesh)) {
        c->err = std::string(who) + ": instance " + std::to_string(i) + ": its emissive prim mesh " + std::to_string(mesh) + " has no emitter template";
        return RT_ERR_INVALID_ARG;
      }
      continue;
    }
    P.ids.push_back(i);
    P.prefix.push_back(uint32_t(recs));
    recs += meshRows[mesh];
    if(recs > 0x7fffffffull) { c->err = std::string(who) + ": more than 2^31 - 1 triangle-light records"; return RT_ERR_INVALID_ARG; }
    const rt_vec3& e = c->materials[size_t(c->primMeshes[mesh].materialIndex)].emissiveFactor;   // (a template needs a material: rt_set_emitter_meshes)
    distrib.insert(distrib.end(), meshRows[mesh], luminance(e));
  }
  P.prefix.push_back(uint32_t(recs));
  P.records = uint32_t(recs);
  float total = 0.f;
  for(const float w : distrib) total += w;
  if(P.records) {
    const std::vector<rth::AliasBucket> table = rth::buildAliasTable(distrib);
    P.alias.resize(P.records);
    for(size_t k = 0; k < distrib.size(); k++) P.alias[k] = rt_impt_samp{table[k].failId, table[k].prob, distrib[k] / total, distrib[size_t(table[k].failId)] / total};
  }
  // Scene::setInstances' rule: with no light of either kind the value stays
  P.trigSampProb = (P.records > 0 || c->ds.lightInfo.puncLightSize > 0) ? total / (total + puncWeight) : c->ds.lightInfo.trigSampProb;
  return RT_OK;
}

// one set of derived light buffers with 1/8 slack over the counts
static hipError_t allocEmitSet(rt_ctx::Emit::Set& S, uint32_t records, uint32_t emitting)
{
  const size_t recCap = std::max<size_t>(size_t(records) + records / 8, 1), emitCap = std::max<size_t>(size_t(emitting) + emitting / 8, 1);
  hipError_t e = hipSuccess;
  auto get = [&](size_t bytes, auto** out) { pooledAlloc(e, S.pool, bytes, out); };
  get(recCap * sizeof(rt_trig_light), &S.rec); get(recCap * sizeof(rt_light_source), &S.src); get(recCap * sizeof(rt_impt_samp), &S.alias);
  get((emitCap + 1) * 4, &S.prefix); get(emitCap * 4, &S.ids);
  if(e == hipSuccess) { S.recCap = uint32_t(std::min<size_t>(recCap, 0xffffffffu)); S.emitCap = uint32_t(std::min<size_t>(emitCap, 0xffffffffu)); }
  else freePool(S.pool);
  return e;
}

// the plan's words into the staging arrays of S, then k_light_expand between evEmit[0] and evEmit[1], on the main stream; records / sources: where it writes
static hipError_t enqueueLightExpand(rt_ctx* c, const EmitPlan& P, const rt_ctx::Emit::Set& S, const DevInstance* dInst, const rt_emitter_row* dRows,
                                     const uint32_t* dMeshFirstRow, rt_trig_light* records, rt_light_source* sources)
{
  hipStream_t s = c->stream;
  hipError_t he;
  if(P.records && (he = hipMemcpyAsync(S.alias, P.alias.data(), P.alias.size() * sizeof(rt_impt_samp), hipMemcpyHostToDevice, s)) != hipSuccess) return he;
  if((he = hipMemcpyAsync(S.prefix, P.prefix.data(), P.prefix.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return he;
  if(!P.ids.empty() && (he = hipMemcpyAsync(S.ids, P.ids.data(), P.ids.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return he;
  if((he = hipEventRecord(c->evEmit[0], s)) != hipSuccess) return he;
  LightExpandArgs x{};
  x.prefix = S.prefix; x.ids = S.ids; x.meshFirstRow = dMeshFirstRow; x.rows = dRows; x.alias = S.alias; x.instances = dInst;
  x.primMeshes = c->ds.primMeshes; x.vertices = c->ds.vertices; x.indices = c->ds.indices; x.records = records; x.sources = sources;
  x.numEmit = uint32_t(P.ids.size()); x.numRecs = P.records;
  if((he = launchLightExpand(s, x)) != hipSuccess) return he;
  return hipEventRecord(c->evEmit[1], s);
}

// the derived (instance, triangle) list becomes the light-source binding (the counter of the refit tail stays)
static void installDerivedBinding(rt_ctx* c, const EmitPlan& P, size_t numInstances, rt_light_source* dSources)
{
  rt_ctx::Lights& L = c->lights;
  uint32_t* const counter = L.dCounter;
  L = rt_ctx::Lights{};
  L.bound = P.records; L.dSources = dSources; L.dCounter = counter;
  L.instances.assign(numInstances, 0);
  for(const uint32_t i : P.ids) L.instances[i] = 1;
  L.stats.bound = P.records;
}

extern "C" {

int rt_set_instances(rt_ctx* c, uint32_t numInstances, const rt_instance* instances)
{
  if(int rc = needTree(c, "rt_set_instances")) return rc;
  // ---- the whole table is checked before anything changes
  if(!instances) return fail(c, RT_ERR_INVALID_ARG, "rt_set_instances: NULL instance table");
  if(numInstances == 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_instances: an instance table needs at least one instance");
  const size_t nOld = c->instances.size();
  std::vector<DevInstance> rows(numInstances);
  std::vector<uint32_t> prefix(size_t(numInstances) + 1, 0u);
  uint64_t total = 0;
  auto refuse = [&](uint32_t i, const char* what) { c->err = "rt_set_instances: instance " + std::to_string(i) + ": " + what; return RT_ERR_INVALID_ARG; };
  for(uint32_t i = 0; i < numInstances; i++) {
    const rt_instance& in = instances[i];
    if(in.primMesh >= c->primMeshes.size()) return refuse(i, "prim mesh out of range");
    bool mirrored;
    if(const char* why = makeInstanceRow(in.objectToWorld, in.primMesh, in.flags, rows[i], &mirrored)) return refuse(i, why);
    prefix[i] = uint32_t(total) | (mirrored ? INST_PREFIX_FLIP : 0u);
    total += c->primMeshes[in.primMesh].indexCount / 3;
    if(total > uint64_t(INST_PREFIX_MASK)) return refuse(i, "the table has more than 2^31 - 1 triangles");
  }
  if(total == 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_instances: the table has no triangles");
  prefix[numInstances] = uint32_t(total);
  const bool derive = c->emit.on;   // the emitter mode: the light records follow from the table, so the emitter rule gives way to the template rule
  EmitPlan plan;
  if(derive) {
    if(const int prc = planEmitters(c, "rt_set_instances", numInstances, instances, c->emit.meshFirstRow, c->emit.meshRows, c->emit.puncWeight, plan)) return prc;
  } else if(c->ds.lightInfo.trigLightSize > 0) {   // the emitter rule: light records, alias table and binding name instances by index
    for(uint32_t i = 0; i < nOld; i++)
      if((emissiveMesh(c, c->instances[i].primMesh) || (i < c->lights.instances.size() && c->lights.instances[i])) && (i >= numInstances || memcmp(&c->instances[i], &instances[i], sizeof(rt_instance)) != 0))
        return refuse(i, "an emissive instance must stay in place, byte for byte (move it with rt_update_instances)");
    for(uint32_t i = 0; i < numInstances; i++)
      if(emissiveMesh(c, instances[i].primMesh) && !(i < nOld && emissiveMesh(c, c->instances[i].primMesh)))
        return refuse(i, "a new instance of an emissive prim mesh (its triangle-light records would be missing)");
  }
  const uint32_t n = uint32_t(total);
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // drains the frames in flight, like rt_rebuild_accel
  rt_ctx::Refit& R = c->refit;
  rt_ctx::Rebuild& B = c->rebuild;
  rt_ctx::InstTemplates& TP = c->inst;
  int rc;
  rt_instances_stats st{};
  st.instances = numInstances; st.triangles = n;
  {
    size_t same = 0;
    while(same < nOld && same < numInstances && memcmp(&c->instances[same], &instances[same], sizeof(rt_instance)) == 0) same++;
    st.added = uint32_t(numInstances - same); st.removed = uint32_t(nOld - same);
  }
  // ---- the pad: triPadOf over the new instances' maxima; an instance that stays where it was keeps the maximum the update calls maintain
  std::vector<float> instMax(numInstances);
  std::vector<uint8_t> flip(numInstances);
  for(uint32_t i = 0; i < numInstances; i++) {
    flip[i] = uint8_t(prefix[i] >> 31);
    if(R.ready && i < nOld && memcmp(&c->instances[i], &instances[i], sizeof(rt_instance)) == 0) { instMax[i] = R.instMax[i]; continue; }
    if((rc = syncHostVertices(c, int(instances[i].primMesh)))) return rc;   // meshCoordMax reads the context's copy: skinned and morphed meshes are current on the device only
    instMax[i] = meshCoordMax(c, instances[i].primMesh, rows[i].o2w);
  }
  const float triPad = triPadOf(instMax);
  // ---- templates, once per prim mesh
  if(!TP.dAlpha) {
    std::vector<uint32_t> base(c->primMeshes.size(), 0u);
    uint64_t meshTris = 0;
    for(size_t m = 0; m < c->primMeshes.size(); m++) { base[m] = uint32_t(meshTris); meshTris += c->primMeshes[m].indexCount / 3; }
    if(meshTris >= 0xffffffffull) return fail(c, RT_ERR_INVALID_ARG, "rt_set_instances: the prim meshes have more than 2^32 - 2 triangles");
    const uint32_t* up = nullptr;
    rc = allocZeroed(c, c->instAllocs, size_t(meshTris) + 1, &TP.dAlpha);
    if(!rc) rc = allocZeroed(c, c->instAllocs, size_t(meshTris) + 1, &TP.dOmm);
    if(!rc) rc = upload(c, c->instAllocs, base.data(), base.size(), &up);
    if(rc) { freePool(c->instAllocs); TP = rt_ctx::InstTemplates{}; return rc; }
    TP.dMeshAlphaBase = const_cast<uint32_t*>(up);
    TP.meshAlphaBase = base; TP.meshMade.assign(base.size(), 0); TP.numAlpha = size_t(meshTris) + 1;
    st.bytesUploaded += uint32_t(base.size() * 4);
  }
  for(uint32_t i = 0; i < numInstances; i++)
    if(!(instances[i].flags & RT_INST_FORCE_OPAQUE) && !TP.meshMade[instances[i].primMesh])
      if((rc = makeMeshTemplates(c, instances[i].primMesh, &st.bytesUploaded))) return rc;
  // ---- capacity: a table that does not fit the buffers gets new ones; the old ones go once the new tree is in place
  const bool fits = B.instReady && n <= B.triCap && numInstances <= B.instCap;
  rt_ctx::Rebuild fresh;
  std::vector<void*> freshPool;
  if(!fits) {
    const uint32_t triCap = uint32_t(std::min<uint64_t>(uint64_t(n) + n / 8, INST_PREFIX_MASK)), instCap = numInstances + numInstances / 8;
    const hipError_t e = allocInstanceBuffers(fresh, triCap, instCap, freshPool);
    if(e != hipSuccess) { freePool(freshPool); return hipFail(c, "rt_set_instances", e); }
    st.reallocated = 1u;
  }
  rt_ctx::Rebuild& W = fits ? B : fresh;
  // the emitter mode's light buffers: the set the context does not use, or a new one with slack where that is absent or too small
  rt_ctx::Emit& EM = c->emit;
  const int es = EM.cur == 0 ? 1 : 0;
  rt_ctx::Emit::Set freshSet;
  const bool setFits = !derive || (EM.set[es].rec && plan.records <= EM.set[es].recCap && plan.ids.size() <= EM.set[es].emitCap);
  // what a call that fails puts back, from here to the swap: the shared working buffers describe the context's table again, new buffers go
  auto giveUp = [&] { if(fits) { B.work.n = uint32_t(c->numTris); B.work.table = B.table[B.icur]; } else freePool(freshPool); freePool(freshSet.pool); };
  auto giveUpHip = [&](hipError_t e) { giveUp(); return hipFail(c, "rt_set_instances", e); };
  if(!setFits) {
    const hipError_t e = allocEmitSet(freshSet, plan.records, uint32_t(plan.ids.size()));
    if(e != hipSuccess) return giveUpHip(e);
  }
  rt_ctx::Emit::Set& LS = setFits ? EM.set[es] : freshSet;
  {   // the builder of rt_set_rebuild_options; PLOC's buffers go into the pool of the working buffers they belong to
    bool allocated = false;
    const hipError_t e = applyRebuildOptions(c, W.work, fits ? c->rebuildAllocs : freshPool, &allocated);
    if(e != hipSuccess) return giveUpHip(e);
    if(allocated) st.reallocated = 1u;
  }
  {
    hipError_t e = derive ? ensureEvents(c->evEmit) : hipSuccess;
    if(e == hipSuccess) e = ensureEvents(c->evRebuild);
    if(e == hipSuccess) e = ensureEvents(c->evInst);
    if(e == hipSuccess) e = ensureEvents(c->evRefit);
    if(e != hipSuccess) return giveUpHip(e);
  }
  const int ti = fits ? 1 - B.icur : 0, ts = fits ? (B.cur == 0 ? 1 : 0) : 0;
  const AccelBuildSet& T = W.set[ts];
  hipStream_t s = c->stream;
  // ---- the table's own work ahead of the build: rows and prefix, the expansion (it writes the flip bits), the emitter mode's light records.  Like the build, it
  // writes only spare and working buffers: the context's table, tree and records stay until the swap
  hipError_t he;
  do {   // (one pass: a HIP error leaves through `break` with `he` set)
    if((he = hipEventRecord(c->evRebuild[0], s)) != hipSuccess) break;
    if((he = hipMemcpyAsync(W.inst[ti], rows.data(), size_t(numInstances) * sizeof(DevInstance), hipMemcpyHostToDevice, s)) != hipSuccess) break;
    if((he = hipMemcpyAsync(W.prefix, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess) break;
    if((he = hipEventRecord(c->evInst[0], s)) != hipSuccess) break;
    InstExpandArgs x{};
    x.prefix = W.prefix; x.instances = W.inst[ti]; x.meshAlphaBase = TP.dMeshAlphaBase; x.ommTemplate = TP.dOmm;
    x.triRef = W.triRef[ti]; x.table = W.table[ti]; x.flipBits = W.dFlip; x.numInst = numInstances; x.numTris = n;
    if((he = launchExpandInstances(s, x)) != hipSuccess) break;
    if((he = hipEventRecord(c->evInst[1], s)) != hipSuccess) break;
    // the light records and the binding of the new table, into the spare set: the new instance rows are in place on this stream
    if(derive) he = enqueueLightExpand(c, plan, LS, W.inst[ti], EM.dRows, EM.dMeshFirstRow, LS.rec, LS.src);
  } while(false);
  if(he != hipSuccess) { (void)hipStreamSynchronize(s); return giveUpHip(he); }
  W.work.n = n; W.work.table = W.table[ti];
  const RefitArgs a = refitArgs(c, T.nodes, T.tris, T.recNode, W.work.nodeDirty, W.triRef[ti], W.inst[ti], W.dDirty, W.dFlip, W.dCounters, n, triPad, true);
  AccelBuildResult res;
  if((rc = runDeviceBuild(c, "rt_set_instances", s, W.work, T, a, numInstances, TP.dAlpha, res))) { giveUp(); return rc; }
  st.bytesUploaded += uint32_t(size_t(numInstances) * sizeof(DevInstance) + prefix.size() * 4 + 24);   // (24: the seed of the build's centre bounds, accelBuildRun)
  // ---- swap
  DevScene next = c->ds;
  next.triRef = W.triRef[ti]; next.instances = W.inst[ti]; next.alphaRec = TP.dAlpha; next.triPad = triPad;
  if(derive) { next.trigLights = LS.rec; next.lightInfo.trigLightSize = plan.records; next.lightInfo.trigSampProb = plan.trigSampProb; }
  bool adopted;
  rc = adoptDeviceTree(c, next, W, ts, res, n, &adopted);   // (a code with the tree adopted: the seed plane's reset; it is returned once the table is in place too)
  if(!adopted) { giveUp(); return rc; }
  if(!fits) { freePool(c->rebuildAllocs); c->rebuildAllocs.swap(freshPool); B = fresh; }
  if(derive) {   // lights and tree change hands together
    if(!setFits) { freePool(EM.set[es].pool); EM.set[es] = std::move(freshSet); freshSet.pool.clear(); }
    EM.cur = es;
    installDerivedBinding(c, plan, numInstances, EM.set[es].src);
    rt_emitter_stats lightStats{};
    lightStats.enabled = 1u; lightStats.records = plan.records; lightStats.emittingInstances = uint32_t(plan.ids.size()); lightStats.bytesUploaded = emitPlanBytes(plan);
    lightStats.reallocated = setFits ? 0u : 1u;
    (void)hipEventElapsedTime(&lightStats.expandMs, c->evEmit[0], c->evEmit[1]);
    EM.stats = lightStats;
  }
  B.icur = ti;
  c->instances.assign(instances, instances + numInstances);
  c->numTris = n;
  // rt_update_instances and the deform calls work on the new table: the per-instance state and the device words at its capacity
  R.ready = true;
  R.inst = rows; R.instMax = instMax; R.flip = flip;
  R.dDirty = B.dDirty; R.dFlip = B.dFlip; R.dCounters = B.dCounters;
  if(c->deform.dOut && numInstances > c->deform.coordCap) { freePool(c->deformAllocs); c->deform.dCoordJobs = nullptr; c->deform.dOut = nullptr; c->deform.coordCap = 0; }
  c->omPrev.clear(); c->omMoved.clear(); c->omPending = false;   // every instance's previous matrix is its current one
  st.ms = B.stats.ms;
  (void)hipEventElapsedTime(&st.expandMs, c->evInst[0], c->evInst[1]);
  TP.stats = st;
  return rc;
}

int rt_get_instances_stats(rt_ctx* c, rt_instances_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->inst.stats;
  return RT_OK;
}

int rt_get_refit_stats(rt_ctx* c, rt_refit_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->refit.stats;
  return RT_OK;
}

int rt_accel_readback(rt_ctx* c, int which, void* dst, size_t bytes)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveAccel) return fail(c, RT_ERR_NO_ACCEL, "rt_accel_readback: rt_build_accel has not run");
  const void* src = nullptr; size_t want = 0;
  switch(which) {
    case RT_ACCEL_NODES: src = c->ds.nodes; want = size_t(c->ds.numNodes) * sizeof(Node8); break;
    case RT_ACCEL_TRIS: src = c->ds.tris; want = size_t(c->ds.numTris) * sizeof(Tri48); break;
    case RT_ACCEL_INSTANCES: src = c->ds.instances; want = c->instances.size() * sizeof(DevInstance); break;
    case RT_ACCEL_ALPHA: src = c->ds.alphaRec; want = numAlphaRecords(c) * sizeof(AlphaRec); break;
    default: return fail(c, RT_ERR_INVALID_ARG, "rt_accel_readback: which must be RT_ACCEL_NODES / _TRIS / _INSTANCES / _ALPHA");
  }
  if(which == RT_ACCEL_ALPHA && bytes % sizeof(AlphaRec) == 0 && bytes < want) want = bytes;   // a prefix of the records (the templates hold every prim mesh's)
  if(bytes != want || (want && !dst)) return fail(c, RT_ERR_INVALID_ARG, "rt_accel_readback: size mismatch");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  if(want) RT_HIP(c, hipMemcpy(dst, src, want, hipMemcpyDeviceToHost));
  if(which == RT_ACCEL_ALPHA) {   // the texel address names a texture of this device: its index instead, all ones for none
    AlphaRec* recs = static_cast<AlphaRec*>(dst);
    std::unordered_map<const uint8_t*, uint64_t> indexOf;
    for(size_t t = c->devTextures.size(); t-- > 0;) indexOf[c->devTextures[t].bgra] = t;
    for(size_t i = 0; i < want / sizeof(AlphaRec); i++) {
      const auto it = recs[i].bgra ? indexOf.find(recs[i].bgra) : indexOf.end();
      const uint64_t id = it == indexOf.end() ? ~0ull : it->second;
      memcpy(&recs[i].bgra, &id, 8);
    }
  }
  return RT_OK;
}

/* ---- deforming meshes: vertex updates and GPU skinning + the refit of rt_update_instances (include/rt_abi.h "Deforming meshes", csrc/deform.hip) ---- */
}  // extern "C"

/* ---- editing materials and textures (include/rt_abi.h "Editing materials and textures", csrc/materials.hip, csrc/opacity_map.h) ---- */
// the alpha records DevScene::alphaRec holds: the templates' once rt_set_instances has put them in force, else the host tree's
static size_t numAlphaRecords(const rt_ctx* c) { return (c->inst.dAlpha && c->ds.alphaRec == c->inst.dAlpha) ? c->inst.numAlpha : c->hostNumAlpha; }

// the device words of the re-derivation, for `numAlpha` alpha records and the scene's materials; the two events
static int ensureMaterialState(rt_ctx* c, size_t numAlpha)
{
  rt_ctx::Materials& M = c->mat;
  if(const hipError_t he = ensureEvents(c->evMat)) return hipFail(c, "hipEventCreate(&e)", he);
  const size_t words = (c->materials.size() + 31) / 32 + 1;
  if(M.dDirty && numAlpha <= M.alphaCap && words <= M.dirtyWords) return RT_OK;
  freePool(c->matAllocs);
  const rt_material_stats keep = M.stats;
  M = rt_ctx::Materials{};
  M.stats = keep;
  const size_t cap = numAlpha + numAlpha / 8 + 1;
  int rc = allocZeroed(c, c->matAllocs, words, &M.dDirty);
  if(!rc) rc = allocZeroed(c, c->matAllocs, cap, &M.dOwner);
  if(!rc) rc = allocZeroed(c, c->matAllocs, cap, &M.dOwners);
  if(!rc) rc = allocZeroed(c, c->matAllocs, size_t(MAT_CNT_WORDS), &M.dCounters);
  if(!rc) rc = allocZeroed(c, c->matAllocs, cap, &M.dOmm);
  if(rc) { freePool(c->matAllocs); M = rt_ctx::Materials{}; M.stats = keep; return rc; }
  RT_HIP(c, hipDeviceSynchronize());   // the zero fills ran on the null stream, which the context's (non-blocking) streams do not wait for
  M.alphaCap = cap; M.dirtyWords = words;
  return RT_OK;
}

// What both edits end with.  dirty[m] != 0: the alpha records of material m's triangles are stale; the caller has drained the context, recorded evMat[0] and
// enqueued its copies (material rows, texels) on the main stream, and the context's tables hold the edit.  With a tree and a dirty material: the templates of
// meshes no alpha-tested instance uses are dropped, then select, build and scatter (csrc/materials.hip); evMat[1], one synchronise, `st` filled in.
static int rederiveAlpha(rt_ctx* c, const std::vector<uint8_t>& dirty, rt_material_stats& st)
{
  hipStream_t s = c->stream;
  st.dirtyMaterials = uint32_t(dirty.size() - std::count(dirty.begin(), dirty.end(), uint8_t(0)));
  uint32_t counters[MAT_CNT_WORDS] = {0, 0, 0, 0};
  if(c->haveAccel && st.dirtyMaterials > 0) {
    rt_ctx::InstTemplates& TP = c->inst;
    const bool inForce = TP.dAlpha && c->ds.alphaRec == TP.dAlpha;
    auto materialOfMesh = [&](size_t mesh) { const int32_t mi = c->primMeshes[mesh].materialIndex; return size_t(mi > 0 ? mi : 0); };
    // A template nothing in the tree refers to is not re-derived: the next table that needs it makes it from the edited tables.  A live mesh's templates all
    // have a leaf record: rt_set_instances expands one table row per (instance, triangle) pair and the device builder emits every row, degenerate triangles
    // included (accel_build.h: the record count of a device tree is the triangle count), so the select pass below reaches every template of a live mesh.
    if(TP.dAlpha) {
      std::vector<uint8_t> live(c->primMeshes.size(), 0);
      if(inForce) for(const rt_instance& in : c->instances) if(!(in.flags & RT_INST_FORCE_OPAQUE)) live[in.primMesh] = 1;
      for(size_t mesh = 0; mesh < c->primMeshes.size(); mesh++) {
        if(!TP.meshMade[mesh] || live[mesh] || !dirty[materialOfMesh(mesh)]) continue;
        const size_t first = size_t(TP.meshAlphaBase[mesh]) + 1, nt = c->primMeshes[mesh].indexCount / 3;
        if(nt) {
          RT_HIP(c, hipMemsetAsync(TP.dAlpha + first, 0, nt * sizeof(AlphaRec), s));
          RT_HIP(c, hipMemsetAsync(TP.dOmm + first, 0, nt * 16, s));
        }
        TP.meshMade[mesh] = 0;
      }
    }
    const size_t numAlpha = numAlphaRecords(c);
    if(c->ds.numTris > 0 && numAlpha > 0) {
      if(const int rc = ensureMaterialState(c, numAlpha)) return rc;
      rt_ctx::Materials& M = c->mat;
      std::vector<uint32_t> bits(M.dirtyWords, 0u);
      for(size_t m = 0; m < dirty.size(); m++) if(dirty[m]) bits[m >> 5] |= 1u << (m & 31u);
      MaterialArgs a{};
      a.tris = const_cast<Tri48*>(c->ds.tris); a.alphaByTri = const_cast<AlphaRec*>(c->ds.alphaByTri);
      a.table = c->rebuild.ready ? c->rebuild.work.table : nullptr;
      a.triRef = c->ds.triRef; a.instances = c->ds.instances; a.primMeshes = c->ds.primMeshes; a.materials = c->ds.materials; a.textures = c->ds.textures;
      a.alphaRec = const_cast<AlphaRec*>(c->ds.alphaRec); a.ommPlane = inForce ? TP.dOmm : M.dOmm;
      a.dirtyBits = M.dDirty; a.owner = M.dOwner; a.owners = M.dOwners; a.counters = M.dCounters;
      a.numRecs = c->ds.numTris; a.numGlobal = uint32_t(c->numTris); a.numAlpha = uint32_t(numAlpha); a.numInstances = uint32_t(c->instances.size());
      a.numPrimMeshes = uint32_t(c->primMeshes.size()); a.numMaterials = uint32_t(c->materials.size()); a.numTextures = uint32_t(c->devTextures.size());
      RT_HIP(c, hipMemcpyAsync(M.dDirty, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, s));
      RT_HIP(c, hipMemsetAsync(M.dOwner, 0xff, numAlpha * 4, s));
      RT_HIP(c, hipMemsetAsync(M.dCounters, 0, sizeof(counters), s));
      RT_HIP(c, launchMaterialSelect(s, a));
      RT_HIP(c, hipMemcpyAsync(counters, M.dCounters, sizeof(counters), hipMemcpyDeviceToHost, s));
      RT_HIP(c, hipStreamSynchronize(s));   // the build's grid is the owner count
      if(counters[MAT_CNT_OWNERS] > numAlpha) return fail(c, RT_ERR_HIP, "material edit: more owners than alpha records");   // never: one owner per record
      RT_HIP(c, launchMaterialBuild(s, a, counters[MAT_CNT_OWNERS]));
      if(counters[MAT_CNT_SELECTED] > 0) RT_HIP(c, launchMaterialScatter(s, a));
      RT_HIP(c, hipMemcpyAsync(counters, M.dCounters, sizeof(counters), hipMemcpyDeviceToHost, s));
      st.bytesUploaded += uint32_t(bits.size() * 4);
    }
  }
  RT_HIP(c, hipEventRecord(c->evMat[1], s));
  RT_HIP(c, hipStreamSynchronize(s));
  st.alphaRecords = counters[MAT_CNT_OWNERS]; st.leafRecords = counters[MAT_CNT_SELECTED];
  st.texelsScanned = (uint64_t(counters[MAT_CNT_TEXELS_HI]) << 32) | counters[MAT_CNT_TEXELS_LO];
  (void)hipEventElapsedTime(&st.ms, c->evMat[0], c->evMat[1]);
  c->refN = 0;   // the scene changed: the reference sums start again
  c->mat.stats = st;
  return RT_OK;
}

extern "C" {

int rt_update_materials(rt_ctx* c, uint32_t count, const uint32_t* ids, const rt_material* rows)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_update_materials: no scene uploaded");
  if(count && (!ids || !rows)) return fail(c, RT_ERR_INVALID_ARG, "rt_update_materials: NULL ids / rows");
  // the whole call is checked before anything changes
  const size_t nMat = c->materials.size();
  auto refuse = [&](uint32_t id, const char* what) { c->err = "rt_update_materials: material " + std::to_string(id) + ": " + what; return RT_ERR_INVALID_ARG; };
  {
    std::vector<bool> seen(nMat, false);
    for(uint32_t k = 0; k < count; k++) {
      if(ids[k] >= nMat) return refuse(ids[k], "id out of range");
      if(seen[ids[k]]) return refuse(ids[k], "listed twice");
      seen[ids[k]] = true;
      if(const char* why = checkMaterialRow(rows[k], int32_t(c->numTextures))) return refuse(ids[k], why);
      const float was = luminance(c->materials[ids[k]].emissiveFactor), is = luminance(rows[k].emissiveFactor);
      if((was > 1e-2f) != (is > 1e-2f))
        return refuse(ids[k], "the row moves the material across the scene's light rule (luminance of emissiveFactor > 1e-2): the emissive meshes are fixed by the scene");
      if(c->emit.on && was > 1e-2f && !(was == is))
        return refuse(ids[k], "the emitter mode is on and the row changes the luminance of an emissive material (the derived alias table would go stale)");
    }
  }
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // joins the frames in flight, like rt_update_instances
  if(const hipError_t he = ensureEvents(c->evMat)) return hipFail(c, "hipEventCreate(&e)", he);
  hipStream_t s = c->stream;
  RT_HIP(c, hipEventRecord(c->evMat[0], s));
  std::vector<uint8_t> dirty(nMat, 0);
  rt_material* dMat = const_cast<rt_material*>(c->ds.materials);
  for(uint32_t k = 0; k < count; k++) {
    rt_material& m = c->materials[ids[k]];
    const rt_material& n = rows[k];
    // the alpha-relevant fields, bitwise: what the alpha records and micro-maps were derived from
    if(memcmp(&m.pbrBaseColorFactor.w, &n.pbrBaseColorFactor.w, 4) || memcmp(&m.alphaCutoff, &n.alphaCutoff, 4) || m.alphaMode != n.alphaMode ||
       m.pbrBaseColorTexture != n.pbrBaseColorTexture)
      dirty[ids[k]] = 1;
    m = n;
    RT_HIP(c, hipMemcpyAsync(dMat + ids[k], &m, sizeof(rt_material), hipMemcpyHostToDevice, s));
  }
  rt_material_stats st{};
  st.materialsWritten = count; st.bytesUploaded = uint32_t(count * sizeof(rt_material));
  return rederiveAlpha(c, dirty, st);
}

int rt_update_texture(rt_ctx* c, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* bgra, size_t rowPitchBytes)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_update_texture: no scene uploaded");
  auto refuse = [&](const char* what) { c->err = "rt_update_texture: texture " + std::to_string(texture) + ": " + what; return RT_ERR_INVALID_ARG; };
  if(texture >= c->numTextures) return refuse("out of range");
  const DevTexture T = c->devTextures[texture];
  if(w == 0 || h == 0) return refuse("empty rectangle");
  if(uint64_t(x) + w > uint64_t(T.w) || uint64_t(y) + h > uint64_t(T.h)) return refuse("the rectangle leaves the texture");
  if(rowPitchBytes < size_t(w) * 4) return refuse("rowPitchBytes is less than 4 w");
  if(!bgra) return refuse("NULL texels");
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  if(const hipError_t he = ensureEvents(c->evMat)) return hipFail(c, "hipEventCreate(&e)", he);
  hipStream_t s = c->stream;
  RT_HIP(c, hipEventRecord(c->evMat[0], s));
  uint8_t* dTex = const_cast<uint8_t*>(T.bgra) + (size_t(y) * size_t(T.w) + x) * 4;
  RT_HIP(c, hipMemcpy2DAsync(dTex, size_t(T.w) * 4, bgra, rowPitchBytes, size_t(w) * 4, h, hipMemcpyHostToDevice, s));
  // the context's alpha plane and its hash (rt_build_accel's cache key)
  std::vector<uint8_t>& plane = c->hostAlpha[texture];
  bool alphaChanged = false;
  for(uint32_t r = 0; r < h; r++) {
    uint8_t* dst = plane.data() + (size_t(y) + r) * size_t(T.w) + x;
    const uint8_t* src = bgra + size_t(r) * rowPitchBytes + 3;
    for(uint32_t q = 0; q < w; q++) { const uint8_t v = src[size_t(q) * 4]; if(dst[q] != v) { dst[q] = v; alphaChanged = true; } }
  }
  std::vector<uint8_t> dirty(c->materials.size(), 0);
  if(alphaChanged) {
    uint64_t h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull;
    hashBytes(plane.data(), plane.size(), h0, h1);
    c->alphaHash[texture] = {h0, h1};
    for(size_t m = 0; m < c->materials.size(); m++) if(c->materials[m].pbrBaseColorTexture == int32_t(texture)) dirty[m] = 1;
  }
  rt_material_stats st{};
  st.bytesUploaded = uint32_t(size_t(w) * h * 4);
  return rederiveAlpha(c, dirty, st);
}

int rt_get_material_stats(rt_ctx* c, rt_material_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->mat.stats;
  return RT_OK;
}

int rt_opacity_map(const rt_opacity_map_desc* d, const uint8_t* bgra, uint32_t omm[4])
{
  if(!d || !omm || (bgra && (d->w <= 0 || d->h <= 0))) return RT_ERR_INVALID_ARG;
  ommBuildSerial(d->uv, d->baseAlpha, d->cutoff, d->alphaMode, d->w, d->h, d->wrapS, d->wrapT, bgra ? bgra + 3 : nullptr, 4, omm);
  return RT_OK;
}

}  // extern "C"

/* ---- the environment (include/rt_abi.h "The environment", csrc/env_accel.hip, csrc/env_accel.h) ---- */
// one device array of the environment's, at least `count` elements: kept when it is large enough, else freed and made again (cap follows)
template <class T> static int ensureEnvArray(rt_ctx* c, T** p, size_t* cap, size_t count)
{
  if(*p && *cap >= count) return RT_OK;
  if(*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
  void* d = nullptr;
  RT_HIP(c, hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
  *p = static_cast<T*>(d); *cap = count;
  return RT_OK;
}
static uint64_t envDeviceBytes(const rt_ctx::Env& E)
{
  uint64_t b = 0;
  for(const auto& p : E.pair) b += (p.texels ? p.cap * 16 : 0) + (p.accel ? p.cap * sizeof(rt_impt_samp) : 0);
  if(E.dArea) b += E.areaCap * 4;
  if(E.dW) b += E.workCap * (sizeof(uint64_t) + sizeof(EnvU128) + 4) + ((E.workCap + ENV_SCAN_TILE - 1) / ENV_SCAN_TILE) * sizeof(EnvBlockSum) + ENV_CNT_WORDS * 4;
  return b;
}

extern "C" {

int rt_set_environment(rt_ctx* c, int width, int height, const float* rgba32f, const rt_impt_samp* accel)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_set_environment: no scene uploaded");
  if(width < 0 || height < 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_environment: negative size");
  // the 1 x 1 black map of rt_upload_scene
  static const float black[4] = {0, 0, 0, 0};
  static const rt_impt_samp one{0, 1.0f, 0.0f, 0.0f};
  if(width == 0 || height == 0 || !rgba32f) { width = height = 1; rgba32f = black; accel = &one; }
  const uint64_t n = uint64_t(width) * uint64_t(height);
  if(n > 0x7fffffffull) return fail(c, RT_ERR_INVALID_ARG, "rt_set_environment: more than 2^31 - 1 texels (alias is an int32)");
  if(!accel && n > ENV_MAX_TEXELS) return fail(c, RT_ERR_INVALID_ARG, "rt_set_environment: more than 2^23 texels and no table: the device build's integer range");
  if(accel) {   // the copy path's checks run on the host: the table as rt_upload_scene checks it, the texels for +inf
    for(uint64_t i = 0; i < n; i++)
      if(accel[i].alias < 0 || uint64_t(accel[i].alias) >= n) return fail(c, RT_ERR_INVALID_ARG, "rt_set_environment: environment alias table entry out of range");
    for(uint64_t i = 0; i < n; i++)
      if(envIsPosInf(rgba32f[i * 4]) || envIsPosInf(rgba32f[i * 4 + 1]) || envIsPosInf(rgba32f[i * 4 + 2]))
        return fail(c, RT_ERR_INVALID_ARG, "rt_set_environment: a texel is +inf");
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // joins the frames in flight, like the other edits
  if(const hipError_t he = ensureEvents(c->evEnv)) return hipFail(c, "hipEventCreate(&e)", he);
  rt_ctx::Env& E = c->env;
  hipStream_t s = c->stream;
  const int target = E.live == 0 ? 1 : 0;   // the pair DevScene does not name
  rt_ctx::Env::Pair& P = E.pair[target];
  if(P.cap < n) {
    if(P.texels) (void)hipFree(P.texels);
    if(P.accel) (void)hipFree(P.accel);
    P = rt_ctx::Env::Pair{};
    size_t cap = 0;
    float4* t = nullptr;
    int rc = ensureEnvArray(c, &t, &cap, size_t(n));
    P.texels = reinterpret_cast<float*>(t);
    if(!rc) { cap = 0; rc = ensureEnvArray(c, &P.accel, &cap, size_t(n)); }
    if(rc) { if(P.texels) (void)hipFree(P.texels); P = rt_ctx::Env::Pair{}; return rc; }
    P.cap = size_t(n);
  }
  uint32_t counters[ENV_CNT_WORDS] = {};
  std::vector<float> area;
  RT_HIP(c, hipEventRecord(c->evEnv[0], s));
  RT_HIP(c, hipMemcpyAsync(P.texels, rgba32f, size_t(n) * 16, hipMemcpyHostToDevice, s));
  if(accel) RT_HIP(c, hipMemcpyAsync(P.accel, accel, size_t(n) * sizeof(rt_impt_samp), hipMemcpyHostToDevice, s));
  else {
    int rc = ensureEnvArray(c, &E.dArea, &E.areaCap, size_t(height));
    if(!rc && !(E.dW && E.workCap >= n)) {
      for(void* p : {static_cast<void*>(E.dW), static_cast<void*>(E.dP), static_cast<void*>(E.dIdx), static_cast<void*>(E.dBlockSums), static_cast<void*>(E.dCounters)})
        if(p) (void)hipFree(p);
      E.dW = nullptr; E.dP = nullptr; E.dIdx = nullptr; E.dBlockSums = nullptr; E.dCounters = nullptr; E.workCap = 0;
      size_t cap = 0;
      const size_t tiles = (size_t(n) + ENV_SCAN_TILE - 1) / ENV_SCAN_TILE;
      rc = ensureEnvArray(c, &E.dW, &cap, size_t(n));
      if(!rc) { cap = 0; rc = ensureEnvArray(c, &E.dP, &cap, size_t(n)); }
      if(!rc) { cap = 0; rc = ensureEnvArray(c, &E.dIdx, &cap, size_t(n)); }
      if(!rc) { cap = 0; rc = ensureEnvArray(c, &E.dBlockSums, &cap, tiles); }
      if(!rc) { cap = 0; rc = ensureEnvArray(c, &E.dCounters, &cap, size_t(ENV_CNT_WORDS)); }
      if(!rc) E.workCap = size_t(n);
    }
    if(rc) return rc;
    area.resize(size_t(height));
    envRowAreas(width, height, area.data());
    EnvBuildArgs a{};
    a.texels = P.texels; a.area = E.dArea; a.accel = P.accel; a.W = E.dW; a.P = E.dP; a.idx = E.dIdx; a.blockSums = E.dBlockSums; a.counters = E.dCounters;
    a.n = uint32_t(n); a.w = uint32_t(width);
    RT_HIP(c, hipMemcpyAsync(E.dArea, area.data(), area.size() * 4, hipMemcpyHostToDevice, s));
    RT_HIP(c, hipMemsetAsync(E.dCounters, 0, sizeof(counters), s));
    RT_HIP(c, launchEnvAccelBuild(s, a));
    RT_HIP(c, hipMemcpyAsync(counters, E.dCounters, sizeof(counters), hipMemcpyDeviceToHost, s));
  }
  RT_HIP(c, hipEventRecord(c->evEnv[1], s));
  RT_HIP(c, hipStreamSynchronize(s));
  if(!accel && counters[ENV_CNT_BAD]) return fail(c, RT_ERR_INVALID_ARG, "rt_set_environment: a texel is +inf, or its importance or luminance overflows to +inf");
  // accepted: DevScene takes the pair
  dropPrimaryReplay(c);   // miss pixels carry the environment's radiance in the G-buffer
  E.live = target;
  c->ds.env = P.texels; c->ds.envAccel = P.accel; c->ds.envW = width; c->ds.envH = height;
  c->refN = 0;            // the scene changed: the reference sums start again
  rt_environment_stats st{};
  st.width = width; st.height = height;
  if(!accel) {
    float M, ML;
    memcpy(&M, &counters[ENV_CNT_MAX_IMP], 4); memcpy(&ML, &counters[ENV_CNT_MAX_LUM], 4);
    const uint64_t T = uint64_t(counters[ENV_CNT_T]) | (uint64_t(counters[ENV_CNT_T + 1]) << 32), TL = uint64_t(counters[ENV_CNT_TL]) | (uint64_t(counters[ENV_CNT_TL + 1]) << 32);
    st.integral = float(envUnscale(T, envScaleExp(M)));
    st.average = float(envUnscale(TL, envScaleExp(ML)) / double(n));
    st.numSmall = counters[ENV_CNT_SMALL]; st.numLarge = uint32_t(n) - st.numSmall;
    st.builtOnDevice = 1;
  }
  (void)hipEventElapsedTime(&st.ms, c->evEnv[0], c->evEnv[1]);
  st.deviceBytes = envDeviceBytes(E);
  E.stats = st;
  return RT_OK;
}

int rt_environment_readback(rt_ctx* c, int which, void* dst, size_t bytes)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_environment_readback: no scene uploaded");
  if(which != RT_ENV_TEXELS && which != RT_ENV_ACCEL) return fail(c, RT_ERR_INVALID_ARG, "rt_environment_readback: which must be RT_ENV_TEXELS / RT_ENV_ACCEL");
  const size_t want = size_t(c->ds.envW) * size_t(c->ds.envH) * 16;
  if(bytes != want || !dst) return fail(c, RT_ERR_INVALID_ARG, "rt_environment_readback: size mismatch");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  RT_HIP(c, hipMemcpy(dst, which == RT_ENV_TEXELS ? static_cast<const void*>(c->ds.env) : static_cast<const void*>(c->ds.envAccel), want, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_get_environment_stats(rt_ctx* c, rt_environment_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->env.stats;
  out->width = c->haveScene ? c->ds.envW : 0; out->height = c->haveScene ? c->ds.envH : 0;
  out->deviceBytes = envDeviceBytes(c->env);
  return RT_OK;
}

static bool envHostArgsOk(int width, int height, const void* rgba32f, const void* out)
{
  return rgba32f && out && width >= 1 && height >= 1 && uint64_t(width) * uint64_t(height) <= ENV_MAX_TEXELS;
}
int rt_env_accel(int width, int height, const float* rgba32f, rt_impt_samp* out, float* integral, float* average)
{
  if(!envHostArgsOk(width, height, rgba32f, out)) return RT_ERR_INVALID_ARG;
  try {
    EnvAccelResult r;
    if(envAccelHost(width, height, rgba32f, out, r)) return RT_ERR_INVALID_ARG;
    if(integral) *integral = r.integral;
    if(average) *average = r.average;
  } catch(...) { return RT_ERR_OOM; }
  return RT_OK;
}
int rt_env_importance(int width, int height, const float* rgba32f, float* out)
{
  if(!envHostArgsOk(width, height, rgba32f, out)) return RT_ERR_INVALID_ARG;
  try {
    std::vector<rt_impt_samp> table(size_t(width) * size_t(height));
    EnvAccelResult r;
    if(envAccelHost(width, height, rgba32f, table.data(), r, out)) return RT_ERR_INVALID_ARG;
  } catch(...) { return RT_ERR_OOM; }
  return RT_OK;
}

}  // extern "C"

// the context's copy of the vertices of skinned meshes is refreshed here, at the top of what reads it, not by rt_update_skins (mesh < 0: every stale mesh)
static int syncHostVertices(rt_ctx* c, int mesh)
{
  rt_ctx::Deform& D = c->deform;
  for(size_t k = 0; k < D.skins.size(); k++) {
    if(!D.stale[k] || (mesh >= 0 && uint32_t(mesh) != D.skins[k].primMesh)) continue;
    const rt_prim_mesh& pm = c->primMeshes[D.skins[k].primMesh];
    if(pm.vertexCount) RT_HIP(c, hipMemcpy(c->vertices.data() + pm.vertexOffset, c->ds.vertices + pm.vertexOffset, size_t(pm.vertexCount) * sizeof(rt_vertex), hipMemcpyDeviceToHost));
    D.stale[k] = 0;
  }
  rt_ctx::Morph& M = c->morph;   // morph-only meshes (a morphed mesh that has a skin marks the skin)
  for(size_t k = 0; k < M.sets.size(); k++) {
    if(!M.stale[k] || (mesh >= 0 && uint32_t(mesh) != M.sets[k].primMesh)) continue;
    const rt_prim_mesh& pm = c->primMeshes[M.sets[k].primMesh];
    if(pm.vertexCount) RT_HIP(c, hipMemcpy(c->vertices.data() + pm.vertexOffset, c->ds.vertices + pm.vertexOffset, size_t(pm.vertexCount) * sizeof(rt_vertex), hipMemcpyDeviceToHost));
    M.stale[k] = 0;
  }
  return RT_OK;
}

static int ensureDeformBuffers(rt_ctx* c)
{
  rt_ctx::Deform& D = c->deform;
  if(D.dOut) return RT_OK;
  const size_t nInst = c->instances.size();
  int rc;
  if((rc = allocZeroed(c, c->deformAllocs, std::max<size_t>(nInst, 1), &D.dCoordJobs))) return rc;
  if((rc = allocZeroed(c, c->deformAllocs, nInst + 1, &D.dOut))) return rc;
  D.coordCap = nInst;
  if(const hipError_t he = ensureEvents(c->evDeform)) return hipFail(c, "hipEventCreate(&e)", he);
  return RT_OK;
}

// the posed rows of one deformed mesh before their commit: `count` rows from pool[first] (the skins' staging buffer, or the morph pool's for a morph-only mesh);
// *stale is set by the commit (the context's copy of the mesh is then older than the device rows)
struct StagedMesh { uint32_t mesh; const rt_vertex* pool; uint32_t first, count; uint8_t* stale; };

// What rt_update_vertices, rt_update_skins and rt_update_morphs share.  `meshes`: the deformed prim meshes.  staged != nullptr: the pose is in staging rows (the
// kernels have been enqueued after evRefit[0] / evDeform[0]), one entry per mesh; it is committed to the live array only when no staged position is non-finite,
// else the call is refused with nothing changed.  Then the coordinate maxima of every instance of those meshes (k_inst_coord_max, one launch per staging pool)
// go into R.instMax, and refitTail does the rest as for rt_update_instances.
static int deformRefit(rt_ctx* c, const char* who, const std::vector<uint32_t>& meshes, const std::vector<StagedMesh>* staged, uint32_t verticesWritten, uint32_t bytesCopied)
{
  rt_ctx::Refit& R = c->refit;
  rt_ctx::Deform& D = c->deform;
  const size_t nInst = c->instances.size();
  hipStream_t s = c->stream;
  std::vector<int32_t> deformed(c->primMeshes.size(), -1);   // -1: not deformed; else the mesh's entry in `staged` (0 without staging)
  for(size_t k = 0; k < meshes.size(); k++) deformed[meshes[k]] = staged ? int32_t(k) : 0;
  std::vector<const rt_vertex*> pools;                        // the arrays the coordinate maxima are read from
  if(!staged) pools.push_back(c->ds.vertices);
  else for(const StagedMesh& sm : *staged) if(std::find(pools.begin(), pools.end(), sm.pool) == pools.end()) pools.push_back(sm.pool);
  std::vector<CoordJob> jobs;
  std::vector<uint8_t> dirty(nInst, 0);
  struct Launch { size_t first, count; uint32_t threads; };
  std::vector<Launch> launches;
  for(const rt_vertex* pool : pools) {
    Launch l{jobs.size(), 0, 0};
    for(uint32_t i = 0; i < nInst; i++) {
      const uint32_t m = c->instances[i].primMesh;
      if(deformed[m] < 0 || (staged && (*staged)[size_t(deformed[m])].pool != pool)) continue;
      dirty[i] = 1;
      const rt_prim_mesh& pm = c->primMeshes[m];
      CoordJob j{};
      j.threadBase = l.threads; j.indexCount = pm.indexCount; j.firstIndex = pm.firstIndex; j.instance = i;
      j.vertexBase = staged ? (*staged)[size_t(deformed[m])].first : pm.vertexOffset;
      jobs.push_back(j);
      l.threads += (pm.indexCount + 63u) & ~63u;
    }
    l.count = jobs.size() - l.first;
    launches.push_back(l);
  }
  std::vector<uint32_t> out(jobs.size() + 1, 0u);
  if(!staged) RT_HIP(c, hipMemsetAsync(D.dOut, 0, 4, s));   // (the staged paths cleared the counter ahead of their kernels)
  if(!jobs.empty()) {
    RT_HIP(c, hipMemsetAsync(D.dOut + 1, 0, jobs.size() * 4, s));
    RT_HIP(c, hipMemcpyAsync(D.dCoordJobs, jobs.data(), jobs.size() * sizeof(CoordJob), hipMemcpyHostToDevice, s));
    for(size_t p = 0; p < pools.size(); p++) {
      if(!launches[p].count) continue;
      CoordMaxArgs ca{};
      ca.vertices = pools[p]; ca.indices = c->ds.indices; ca.instances = c->ds.instances; ca.jobs = D.dCoordJobs + launches[p].first;
      ca.numJobs = uint32_t(launches[p].count); ca.numThreads = launches[p].threads; ca.out = D.dOut + 1 + launches[p].first;
      RT_HIP(c, launchInstCoordMax(s, ca));
    }
  }
  RT_HIP(c, hipMemcpyAsync(out.data(), D.dOut, out.size() * 4, hipMemcpyDeviceToHost, s));
  RT_HIP(c, hipStreamSynchronize(s));
  if(staged && out[0] != 0u) { c->err = std::string(who) + ": the pose yields a non-finite position"; return RT_ERR_INVALID_ARG; }   // only staging rows were written
  if(staged) {   // commit: staging rows -> live rows, on the stream ahead of the refit
    for(const StagedMesh& sm : *staged) {
      const rt_prim_mesh& pm = c->primMeshes[sm.mesh];
      if(sm.count) if(const int rc = capturePrevPositions(c, s, sm.mesh)) return rc;   // per-vertex motion vectors: the rendered frame's positions, ahead of the commit
      if(sm.count) RT_HIP(c, hipMemcpyAsync(const_cast<rt_vertex*>(c->ds.vertices) + pm.vertexOffset, sm.pool + sm.first, size_t(sm.count) * sizeof(rt_vertex), hipMemcpyDeviceToDevice, s));
      *sm.stale = 1;
    }
    RT_HIP(c, hipEventRecord(c->evDeform[1], s));
  }
  for(size_t k = 0; k < jobs.size(); k++) memcpy(&R.instMax[jobs[k].instance], &out[1 + k], 4);
  if(const int rc = refitTail(c, dirty)) return rc;
  D.stats = rt_deform_stats{};
  D.stats.meshes = uint32_t(meshes.size()); D.stats.vertices = verticesWritten; D.stats.instances = uint32_t(jobs.size()); D.stats.vertexBytesCopied = bytesCopied;
  D.stats.ms = R.stats.ms;
  if(staged) (void)hipEventElapsedTime(&D.stats.skinMs, c->evDeform[0], c->evDeform[1]);
  return RT_OK;
}

// The posing kernels of a call that involves morph sets, then deformRefit.  One item per mesh: its skin (or -1) with the joint matrices to use, its morph set (or
// -1) with the weights to use.  A set poses with k_morph when it has an active target or when its mesh has no skin (no active target: the rest rows are copied);
// a skin poses with k_skin from the staging range in place when k_morph wrote it, else from the rest pose as rt_update_skins always did.
struct PoseItem { int32_t skin; const float* mats; int32_t set; const float* weights; };

static int poseAndRefit(rt_ctx* c, const char* who, const std::vector<PoseItem>& items, uint32_t* activeOut)
{
  rt_ctx::Deform& D = c->deform;
  rt_ctx::Morph& M = c->morph;
  std::vector<MorphJob> mjobs;
  std::vector<MorphActive> active;
  std::vector<SkinJob> fromRest, inPlace;
  std::vector<float> matsRest, matsInPlace;
  std::vector<StagedMesh> staged;
  std::vector<uint32_t> meshes;
  uint32_t mthreads = 0, vertices = 0;
  for(const PoseItem& it : items) {
    const uint32_t mesh = it.skin >= 0 ? D.skins[size_t(it.skin)].primMesh : M.sets[size_t(it.set)].primMesh;
    const uint32_t V = c->primMeshes[mesh].vertexCount;
    const uint32_t first = it.skin >= 0 ? D.restFirst[size_t(it.skin)] : M.restFirst[size_t(it.set)];
    bool morphed = false;
    if(it.set >= 0) {
      const rt_morph_set& ms = M.sets[size_t(it.set)];
      MorphJob j{};
      j.threadBase = mthreads; j.count = V; j.restFirst = first; j.firstDelta = ms.firstDelta; j.firstActive = uint32_t(active.size()); j.planes = ms.planes;
      j.pool = it.skin >= 0 ? 0u : 1u;
      for(uint32_t t = 0; t < ms.targetCount; t++) if(it.weights[t] != 0.0f) active.push_back(MorphActive{t, it.weights[t]});
      j.numActive = uint32_t(active.size()) - j.firstActive;
      morphed = j.numActive != 0u || it.skin < 0;
      if(morphed) { mjobs.push_back(j); mthreads += (V + 63u) & ~63u; }
    }
    if(it.skin >= 0) {
      const rt_skin& sk = D.skins[size_t(it.skin)];
      std::vector<SkinJob>& jobs = morphed ? inPlace : fromRest;
      std::vector<float>& mats = morphed ? matsInPlace : matsRest;
      SkinJob j{};
      j.threadBase = jobs.empty() ? 0u : jobs.back().threadBase + jobs.back().count;
      j.count = V; j.restFirst = first; j.firstInfluence = sk.firstInfluence; j.firstJoint = uint32_t(mats.size() / 12);
      jobs.push_back(j);
      mats.insert(mats.end(), it.mats, it.mats + size_t(sk.jointCount) * 12);
    }
    staged.push_back(StagedMesh{mesh, it.skin >= 0 ? D.dStaged : M.dStaged, first, V, it.skin >= 0 ? &D.stale[size_t(it.skin)] : &M.stale[size_t(it.set)]});
    meshes.push_back(mesh);
    vertices += V;
  }
  if(activeOut) *activeOut = uint32_t(active.size());
  for(SkinJob& j : inPlace) j.firstJoint += uint32_t(matsRest.size() / 12);   // one matrix array: the from-rest skins' first
  matsRest.insert(matsRest.end(), matsInPlace.begin(), matsInPlace.end());
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // v1: joins the frames in flight
  int rc;
  if((rc = ensureRefitState(c))) return rc;
  if((rc = ensureDeformBuffers(c))) return rc;
  if(const hipError_t he = ensureEvents(c->evMorph)) return hipFail(c, "hipEventCreate(&e)", he);
  hipStream_t s = c->stream;
  RT_HIP(c, hipEventRecord(c->evRefit[0], s));
  RT_HIP(c, hipEventRecord(c->evDeform[0], s));
  RT_HIP(c, hipMemsetAsync(D.dOut, 0, 4, s));
  RT_HIP(c, hipEventRecord(c->evMorph[0], s));
  if(!mjobs.empty()) {
    RT_HIP(c, hipMemcpyAsync(M.dJobs, mjobs.data(), mjobs.size() * sizeof(MorphJob), hipMemcpyHostToDevice, s));
    if(!active.empty()) RT_HIP(c, hipMemcpyAsync(M.dActive, active.data(), active.size() * sizeof(MorphActive), hipMemcpyHostToDevice, s));
    MorphArgs a{};
    a.rest0 = D.dRest; a.staged0 = D.dStaged; a.rest1 = M.dRest; a.staged1 = M.dStaged; a.deltas = M.dDeltas; a.active = M.dActive; a.jobs = M.dJobs;
    a.numJobs = uint32_t(mjobs.size()); a.numThreads = mthreads; a.nonFinite = D.dOut;
    RT_HIP(c, launchMorph(s, a));
  }
  RT_HIP(c, hipEventRecord(c->evMorph[1], s));
  if(!fromRest.empty() || !inPlace.empty()) {
    RT_HIP(c, hipMemcpyAsync(D.dJoints, matsRest.data(), matsRest.size() * sizeof(float), hipMemcpyHostToDevice, s));
    if(!fromRest.empty()) RT_HIP(c, hipMemcpyAsync(D.dSkinJobs, fromRest.data(), fromRest.size() * sizeof(SkinJob), hipMemcpyHostToDevice, s));
    if(!inPlace.empty()) RT_HIP(c, hipMemcpyAsync(D.dSkinJobs + fromRest.size(), inPlace.data(), inPlace.size() * sizeof(SkinJob), hipMemcpyHostToDevice, s));
    SkinArgs a{};
    a.influences = D.dInfluences; a.joints = D.dJoints; a.nonFinite = D.dOut; a.staged = D.dStaged;
    if(!fromRest.empty()) {
      a.rest = D.dRest; a.jobs = D.dSkinJobs; a.numJobs = uint32_t(fromRest.size()); a.numThreads = fromRest.back().threadBase + fromRest.back().count;
      RT_HIP(c, launchSkin(s, a));
    }
    if(!inPlace.empty()) {   // the morphed rows are the skin's input: every thread reads and writes its own staging row
      a.rest = D.dStaged; a.jobs = D.dSkinJobs + fromRest.size(); a.numJobs = uint32_t(inPlace.size()); a.numThreads = inPlace.back().threadBase + inPlace.back().count;
      RT_HIP(c, launchSkin(s, a));
    }
  }
  return deformRefit(c, who, meshes, &staged, vertices, 0u);
}

extern "C" {

int rt_update_vertices(rt_ctx* c, uint32_t primMesh, uint32_t firstVertex, uint32_t count, const rt_vertex* rows)
{
  if(int rc = needTree(c, "rt_update_vertices")) return rc;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  if(primMesh >= c->primMeshes.size()) return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: prim mesh out of range");
  const rt_prim_mesh& pm = c->primMeshes[primMesh];
  if(uint64_t(firstVertex) + count > pm.vertexCount) return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: vertex range outside the prim mesh");
  if(count && !rows) return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: NULL rows");
  if(!c->deform.skinOfMesh.empty() && c->deform.skinOfMesh[primMesh] >= 0) return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: the prim mesh has a skin");
  if(!c->morph.setOfMesh.empty() && c->morph.setOfMesh[primMesh] >= 0) return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: the prim mesh has a morph set");
  const size_t base = size_t(pm.vertexOffset) + firstVertex;
  for(uint32_t k = 0; k < count; k++) {
    const rt_vertex& v = rows[k];
    if(!std::isfinite(v.position.x) || !std::isfinite(v.position.y) || !std::isfinite(v.position.z)) return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: non-finite position");
    if(memcmp(&v.texcoord, &c->vertices[base + k].texcoord, sizeof(rt_vec2)) != 0)
      return fail(c, RT_ERR_INVALID_ARG, "rt_update_vertices: texcoord differs from the uploaded row (alpha records and micro-maps were derived from it)");
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // v1: joins the frames in flight
  int rc;
  if((rc = ensureRefitState(c))) return rc;
  if((rc = ensureDeformBuffers(c))) return rc;
  hipStream_t s = c->stream;
  RT_HIP(c, hipEventRecord(c->evRefit[0], s));
  std::vector<uint32_t> meshes;
  if(count) {
    memcpy(c->vertices.data() + base, rows, size_t(count) * sizeof(rt_vertex));
    if((rc = capturePrevPositions(c, s, primMesh))) return rc;   // per-vertex motion vectors: the rendered frame's positions, ahead of the new rows
    RT_HIP(c, hipMemcpyAsync(const_cast<rt_vertex*>(c->ds.vertices) + base, c->vertices.data() + base, size_t(count) * sizeof(rt_vertex), hipMemcpyHostToDevice, s));
    meshes.push_back(primMesh);
  }
  return deformRefit(c, "rt_update_vertices", meshes, nullptr, count, count * uint32_t(sizeof(rt_vertex)));
}

int rt_set_skins(rt_ctx* c, uint32_t numSkins, const rt_skin* skins, uint64_t numInfluences, const rt_skin_influence* influences)
{
  if(!c) return RT_ERR_INVALID_ARG;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_set_skins: no scene uploaded");
  if(numSkins && !skins) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: NULL skins");
  if(!c->morph.sets.empty()) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: morph sets exist (skins first: remove the sets with rt_set_morph_targets, set the skins, set the sets again)");
  std::vector<int32_t> skinOfMesh(c->primMeshes.size(), -1);
  std::vector<uint32_t> restFirst(numSkins, 0u);
  uint64_t totalVerts = 0, totalJoints = 0;
  for(uint32_t k = 0; k < numSkins; k++) {
    const rt_skin& sk = skins[k];
    if(sk.primMesh >= c->primMeshes.size()) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: prim mesh out of range");
    if(skinOfMesh[sk.primMesh] >= 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: prim mesh listed twice");
    skinOfMesh[sk.primMesh] = int32_t(k);
    if(sk.jointCount == 0 || sk.jointCount > 65536u) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: jointCount must be 1 .. 65536");
    const rt_prim_mesh& pm = c->primMeshes[sk.primMesh];
    if(uint64_t(sk.firstInfluence) + pm.vertexCount > numInfluences || (pm.vertexCount && !influences))
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: influence range outside the array");
    for(uint32_t v = 0; v < pm.vertexCount; v++) {
      const rt_skin_influence& in = influences[size_t(sk.firstInfluence) + v];
      for(int q = 0; q < 4; q++) {
        if(in.joint[q] >= sk.jointCount) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: joint index beyond the skin's jointCount");
        if(!std::isfinite(in.weight[q])) return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: non-finite weight");
      }
    }
    if(c->lights.bound == 0 && !c->emit.on && emissiveMesh(c, sk.primMesh))   // with a binding the refit tail rewrites the records
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_skins: the prim mesh is emissive (its triangle-light records hold world positions); deform it with rt_update_vertices + rt_update_lights");
    restFirst[k] = uint32_t(totalVerts);
    totalVerts += pm.vertexCount; totalJoints += sk.jointCount;
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  int rc;
  if((rc = syncHostVertices(c))) return rc;   // the stale marks go with the old skins
  rt_ctx::Deform& D = c->deform;
  freePool(c->skinAllocs);
  D.skins.clear(); D.restFirst.clear(); D.skinOfMesh.clear(); D.stale.clear();
  D.dRest = D.dStaged = nullptr; D.dInfluences = nullptr; D.dJoints = nullptr; D.dSkinJobs = nullptr;
  c->skinMats.assign(numSkins, std::vector<float>());
  c->refN = 0;
  if(numSkins == 0) return RT_OK;
  const rt_skin_influence* ip = nullptr;
  if((rc = allocZeroed(c, c->skinAllocs, size_t(totalVerts), &D.dRest))) return rc;
  if((rc = allocZeroed(c, c->skinAllocs, size_t(totalVerts), &D.dStaged))) return rc;
  if((rc = upload(c, c->skinAllocs, influences, size_t(numInfluences), &ip))) return rc;
  D.dInfluences = const_cast<rt_skin_influence*>(ip);
  if((rc = allocZeroed(c, c->skinAllocs, size_t(totalJoints) * 12, &D.dJoints))) return rc;
  if((rc = allocZeroed(c, c->skinAllocs, numSkins, &D.dSkinJobs))) return rc;
  for(uint32_t k = 0; k < numSkins; k++) {   // the rest pose: the context's current rows
    const rt_prim_mesh& pm = c->primMeshes[skins[k].primMesh];
    if(pm.vertexCount) RT_HIP(c, hipMemcpy(D.dRest + restFirst[k], c->ds.vertices + pm.vertexOffset, size_t(pm.vertexCount) * sizeof(rt_vertex), hipMemcpyDeviceToDevice));
  }
  RT_HIP(c, hipDeviceSynchronize());
  D.skins.assign(skins, skins + numSkins);
  D.restFirst = restFirst; D.skinOfMesh = skinOfMesh; D.stale.assign(numSkins, 0);
  return RT_OK;
}

int rt_update_skins(rt_ctx* c, uint32_t count, const uint32_t* skinIds, const float* mats)
{
  if(int rc = needTree(c, "rt_update_skins")) return rc;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  rt_ctx::Deform& D = c->deform;
  if(D.skins.empty()) return fail(c, RT_ERR_INVALID_ARG, "rt_update_skins: no skins (rt_set_skins)");
  if(count && (!skinIds || !mats)) return fail(c, RT_ERR_INVALID_ARG, "rt_update_skins: NULL ids / matrices");
  std::vector<SkinJob> jobs(count);
  std::vector<uint32_t> ids(skinIds, skinIds + count), meshes;
  uint32_t threads = 0, joints = 0;
  {
    std::vector<bool> seen(D.skins.size(), false);
    for(uint32_t k = 0; k < count; k++) {
      if(ids[k] >= D.skins.size()) return fail(c, RT_ERR_INVALID_ARG, "rt_update_skins: skin id out of range");
      if(seen[ids[k]]) return fail(c, RT_ERR_INVALID_ARG, "rt_update_skins: duplicate skin id");
      seen[ids[k]] = true;
      const rt_skin& sk = D.skins[ids[k]];
      for(size_t a = 0; a < size_t(sk.jointCount) * 12; a++)
        if(!std::isfinite(mats[size_t(joints) * 12 + a])) return fail(c, RT_ERR_INVALID_ARG, "rt_update_skins: non-finite matrix entry");
      SkinJob& j = jobs[k];
      j = SkinJob{};
      j.threadBase = threads; j.count = c->primMeshes[sk.primMesh].vertexCount; j.restFirst = D.restFirst[ids[k]]; j.firstInfluence = sk.firstInfluence; j.firstJoint = joints;
      threads += j.count; joints += sk.jointCount;
      meshes.push_back(sk.primMesh);
    }
  }
  // the matrices become the skin's stored pose once the call has succeeded (rt_update_morphs re-poses a morphed skin with them)
  const auto keepMats = [&]() {
    size_t at = 0;
    for(uint32_t k = 0; k < count; k++) {
      const size_t n = size_t(D.skins[ids[k]].jointCount) * 12;
      c->skinMats[ids[k]].assign(mats + at, mats + at + n);
      at += n;
    }
  };
  {   // a listed skin whose mesh has a morph set with a stored weight that is not zero: morph, then skin.  Otherwise the path below, as without morph sets.
    const rt_ctx::Morph& M = c->morph;
    bool morphed = false;
    for(uint32_t k = 0; k < count && !M.sets.empty(); k++) {
      const int32_t set = M.setOfMesh[D.skins[ids[k]].primMesh];
      if(set >= 0) for(float w : M.weights[size_t(set)]) morphed = morphed || w != 0.0f;
    }
    if(morphed) {
      std::vector<PoseItem> items;
      size_t at = 0;
      for(uint32_t k = 0; k < count; k++) {
        const int32_t set = M.setOfMesh[D.skins[ids[k]].primMesh];
        items.push_back(PoseItem{int32_t(ids[k]), mats + at, set, set >= 0 ? M.weights[size_t(set)].data() : nullptr});
        at += size_t(D.skins[ids[k]].jointCount) * 12;
      }
      if(const int rc = poseAndRefit(c, "rt_update_skins", items, nullptr)) return rc;
      keepMats();
      return RT_OK;
    }
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));   // v1: joins the frames in flight
  int rc;
  if((rc = ensureRefitState(c))) return rc;
  if((rc = ensureDeformBuffers(c))) return rc;
  hipStream_t s = c->stream;
  RT_HIP(c, hipEventRecord(c->evRefit[0], s));
  RT_HIP(c, hipEventRecord(c->evDeform[0], s));
  RT_HIP(c, hipMemsetAsync(D.dOut, 0, 4, s));
  if(count) {
    RT_HIP(c, hipMemcpyAsync(D.dSkinJobs, jobs.data(), jobs.size() * sizeof(SkinJob), hipMemcpyHostToDevice, s));
    RT_HIP(c, hipMemcpyAsync(D.dJoints, mats, size_t(joints) * 12 * sizeof(float), hipMemcpyHostToDevice, s));
    SkinArgs a{};
    a.rest = D.dRest; a.staged = D.dStaged; a.influences = D.dInfluences; a.joints = D.dJoints; a.jobs = D.dSkinJobs;
    a.numJobs = count; a.numThreads = threads; a.nonFinite = D.dOut;
    RT_HIP(c, launchSkin(s, a));
  }
  std::vector<StagedMesh> staged(count);
  for(uint32_t k = 0; k < count; k++) staged[k] = StagedMesh{meshes[k], D.dStaged, jobs[k].restFirst, jobs[k].count, &D.stale[ids[k]]};
  if((rc = deformRefit(c, "rt_update_skins", meshes, &staged, threads, 0u))) return rc;
  keepMats();
  return RT_OK;
}

/* ---- morph targets (include/rt_abi.h "Morph targets", csrc/morph.hip) ---- */
int rt_set_morph_targets(rt_ctx* c, uint32_t numSets, const rt_morph_set* sets, uint64_t numDeltas, const rt_morph_delta* deltas)
{
  if(!c) return RT_ERR_INVALID_ARG;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_set_morph_targets: no scene uploaded");
  if(numSets && !sets) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: NULL sets");
  const rt_ctx::Deform& D = c->deform;
  std::vector<int32_t> setOfMesh(c->primMeshes.size(), -1);
  std::vector<uint32_t> restFirst(numSets, 0u);
  uint64_t poolVerts = 0, totalTargets = 0;
  for(uint32_t k = 0; k < numSets; k++) {
    const rt_morph_set& ms = sets[k];
    if(ms.primMesh >= c->primMeshes.size()) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: prim mesh out of range");
    if(setOfMesh[ms.primMesh] >= 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: prim mesh listed twice");
    setOfMesh[ms.primMesh] = int32_t(k);
    if(ms.targetCount == 0 || ms.targetCount > 4096u) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: targetCount must be 1 .. 4096");
    if(ms.planes & ~uint32_t(RT_MORPH_NORMALS | RT_MORPH_TANGENTS)) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: unknown planes bits");
    const rt_prim_mesh& pm = c->primMeshes[ms.primMesh];
    const uint64_t P = 1u + ((ms.planes & RT_MORPH_NORMALS) ? 1u : 0u) + ((ms.planes & RT_MORPH_TANGENTS) ? 1u : 0u);
    const uint64_t rows = uint64_t(ms.targetCount) * P * pm.vertexCount;
    if(uint64_t(ms.firstDelta) + rows > numDeltas || (rows && !deltas)) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: delta range outside the array");
    for(uint64_t r = 0; r < rows; r++) {
      const float* d = deltas[size_t(ms.firstDelta + r)].d;
      if(!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: non-finite delta");
    }
    if(c->lights.bound == 0 && !c->emit.on && emissiveMesh(c, ms.primMesh))   // the rule of rt_set_skins
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_morph_targets: the prim mesh is emissive (its triangle-light records hold world positions); deform it with rt_update_vertices + rt_update_lights");
    if(D.skinOfMesh.empty() || D.skinOfMesh[ms.primMesh] < 0) { restFirst[k] = uint32_t(poolVerts); poolVerts += pm.vertexCount; }
    totalTargets += ms.targetCount;
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  int rc;
  if((rc = syncHostVertices(c))) return rc;   // the stale marks go with the old sets
  rt_ctx::Morph& M = c->morph;
  const rt_morph_stats keep = M.stats;
  freePool(c->morphAllocs);
  M = rt_ctx::Morph{};
  M.stats = keep;
  c->refN = 0;
  if(numSets == 0) return RT_OK;
  const rt_morph_delta* dp = nullptr;
  if((rc = upload(c, c->morphAllocs, deltas, size_t(numDeltas), &dp))) return rc;
  M.dDeltas = const_cast<rt_morph_delta*>(dp);
  if((rc = allocZeroed(c, c->morphAllocs, size_t(poolVerts), &M.dRest))) return rc;
  if((rc = allocZeroed(c, c->morphAllocs, size_t(poolVerts), &M.dStaged))) return rc;
  if((rc = allocZeroed(c, c->morphAllocs, numSets, &M.dJobs))) return rc;
  if((rc = allocZeroed(c, c->morphAllocs, size_t(totalTargets), &M.dActive))) return rc;
  for(uint32_t k = 0; k < numSets; k++) {   // the rest pose of a morph-only mesh: the context's current rows
    const rt_prim_mesh& pm = c->primMeshes[sets[k].primMesh];
    if(!D.skinOfMesh.empty() && D.skinOfMesh[sets[k].primMesh] >= 0) continue;
    if(pm.vertexCount) RT_HIP(c, hipMemcpy(M.dRest + restFirst[k], c->ds.vertices + pm.vertexOffset, size_t(pm.vertexCount) * sizeof(rt_vertex), hipMemcpyDeviceToDevice));
  }
  RT_HIP(c, hipDeviceSynchronize());
  M.sets.assign(sets, sets + numSets);
  M.setOfMesh = setOfMesh; M.restFirst = restFirst; M.stale.assign(numSets, 0);
  M.weights.resize(numSets);
  for(uint32_t k = 0; k < numSets; k++) M.weights[k].assign(sets[k].targetCount, 0.0f);
  return RT_OK;
}

int rt_update_morphs(rt_ctx* c, uint32_t count, const uint32_t* setIds, const float* weights)
{
  if(int rc = needTree(c, "rt_update_morphs")) return rc;
  dropPrimaryReplay(c);   // settled primary visibility does not outlive this call
  rt_ctx::Morph& M = c->morph;
  const rt_ctx::Deform& D = c->deform;
  if(M.sets.empty()) return fail(c, RT_ERR_INVALID_ARG, "rt_update_morphs: no morph sets (rt_set_morph_targets)");
  if(count && (!setIds || !weights)) return fail(c, RT_ERR_INVALID_ARG, "rt_update_morphs: NULL ids / weights");
  std::vector<PoseItem> items;
  std::vector<size_t> at(count, 0);
  size_t total = 0;
  {
    std::vector<bool> seen(M.sets.size(), false);
    for(uint32_t k = 0; k < count; k++) {
      const uint32_t id = setIds[k];
      if(id >= M.sets.size()) return fail(c, RT_ERR_INVALID_ARG, "rt_update_morphs: set id out of range");
      if(seen[id]) return fail(c, RT_ERR_INVALID_ARG, "rt_update_morphs: duplicate set id");
      seen[id] = true;
      const rt_morph_set& ms = M.sets[id];
      for(uint32_t t = 0; t < ms.targetCount; t++)
        if(!std::isfinite(weights[total + t])) return fail(c, RT_ERR_INVALID_ARG, "rt_update_morphs: non-finite weight");
      const int32_t skin = D.skinOfMesh.empty() ? -1 : D.skinOfMesh[ms.primMesh];
      if(skin >= 0 && c->skinMats[size_t(skin)].empty())
        return fail(c, RT_ERR_INVALID_ARG, "rt_update_morphs: the set's prim mesh has a skin that rt_update_skins has not posed yet (pose the skin first)");
      items.push_back(PoseItem{skin, skin >= 0 ? c->skinMats[size_t(skin)].data() : nullptr, int32_t(id), weights + total});
      at[k] = total;
      total += ms.targetCount;
    }
  }
  uint32_t activeTargets = 0;
  if(const int rc = poseAndRefit(c, "rt_update_morphs", items, &activeTargets)) return rc;   // (refused: only staging rows were written)
  for(uint32_t k = 0; k < count; k++) M.weights[setIds[k]].assign(weights + at[k], weights + at[k] + M.sets[setIds[k]].targetCount);
  M.stats = rt_morph_stats{};
  M.stats.sets = count; M.stats.vertices = D.stats.vertices; M.stats.targetsApplied = activeTargets; M.stats.instances = D.stats.instances;
  M.stats.ms = D.stats.ms;
  (void)hipEventElapsedTime(&M.stats.morphMs, c->evMorph[0], c->evMorph[1]);
  return RT_OK;
}

int rt_get_morph_stats(rt_ctx* c, rt_morph_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->morph.stats;
  return RT_OK;
}

int rt_vertices_readback(rt_ctx* c, uint64_t firstVertex, uint64_t count, rt_vertex* dst)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_vertices_readback: no scene uploaded");
  if(firstVertex > c->vertices.size() || count > c->vertices.size() - firstVertex || (count && !dst)) return fail(c, RT_ERR_INVALID_ARG, "rt_vertices_readback: range outside the vertex array");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  if(count) RT_HIP(c, hipMemcpy(dst, c->ds.vertices + firstVertex, size_t(count) * sizeof(rt_vertex), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_get_deform_stats(rt_ctx* c, rt_deform_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->deform.stats;
  return RT_OK;
}

/* ---- light sources: triangle-light records that follow the instances the refit tail refits (include/rt_abi.h "Light sources", csrc/light_records.hip) ---- */
int rt_set_light_sources(rt_ctx* c, uint32_t numTrig, const rt_light_source* sources)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_set_light_sources: no scene uploaded");
  if(c->emit.on) return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: the emitter mode is on (the binding is derived from the instance table; rt_set_emitter_meshes with 0 meshes switches it off)");
  rt_ctx::Lights& L = c->lights;
  if(numTrig == 0) {
    for(const rt_skin& sk : c->deform.skins)
      if(emissiveMesh(c, sk.primMesh))   // the rule of rt_set_skins
        return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: a skin on an emissive prim mesh needs the binding (remove the skin first)");
    for(const rt_morph_set& ms : c->morph.sets)
      if(emissiveMesh(c, ms.primMesh))
        return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: a morph set on an emissive prim mesh needs the binding (remove the set first)");
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, syncAll(c));
    freePool(c->lightAllocs);
    L = rt_ctx::Lights{};
    return RT_OK;
  }
  if(numTrig != c->ds.lightInfo.trigLightSize) return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: numTrig must equal the uploaded trigLightSize");
  if(!sources) return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: NULL sources");
  const size_t nInst = c->instances.size();
  for(uint32_t k = 0; k < numTrig; k++) {
    if(sources[k].instance >= nInst) return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: instance index out of range");
    if(sources[k].triangle >= c->primMeshes[c->instances[sources[k].instance].primMesh].indexCount / 3u)
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: triangle beyond the prim mesh's index list");
  }
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  std::vector<rt_trig_light> recs(numTrig), eval(numTrig);
  RT_HIP(c, hipMemcpy(recs.data(), c->ds.trigLights, size_t(numTrig) * sizeof(rt_trig_light), hipMemcpyDeviceToHost));
  for(uint32_t k = 0; k < numTrig; k++)
    if(recs[k].matIndex != uint32_t(c->primMeshes[c->instances[sources[k].instance].primMesh].materialIndex))
      return fail(c, RT_ERR_INVALID_ARG, "rt_set_light_sources: a record's matIndex differs from its prim mesh's materialIndex");
  // The binding must describe the records: the update kernel, for all records, into a scratch array; v0 v1 v2 must come out bit for bit.  Nothing of the context
  // changes before that holds: the candidate lives in a pool of its own.
  std::vector<void*> fresh, temp;
  const rt_light_source* dSrc = nullptr;
  rt_trig_light* dScratch = nullptr;
  uint32_t* dCounter = nullptr;
  const DevInstance* dInst = c->haveAccel ? c->ds.instances : nullptr;
  int rc = upload(c, fresh, sources, size_t(numTrig), &dSrc);
  if(!rc) rc = allocZeroed(c, fresh, 1, &dCounter);
  if(!rc) rc = allocZeroed(c, temp, size_t(numTrig), &dScratch);
  if(!rc && !dInst) {   // before rt_build_accel there are no device instance rows: the kernel reads objectToWorld and primMesh of a row
    std::vector<DevInstance> rows(std::max<size_t>(nInst, 1), DevInstance{});
    for(size_t i = 0; i < nInst; i++) { memcpy(rows[i].o2w, c->instances[i].objectToWorld, sizeof(rows[i].o2w)); rows[i].primMesh = c->instances[i].primMesh; }
    rc = upload(c, temp, rows.data(), rows.size(), &dInst);
  }
  hipError_t he = hipSuccess;
  if(!rc) {
    LightRecArgs la{};
    la.records = dScratch; la.sources = dSrc; la.instances = dInst; la.primMeshes = c->ds.primMeshes; la.vertices = c->ds.vertices; la.indices = c->ds.indices;
    la.dirtyBits = nullptr; la.counter = dCounter; la.numRecs = numTrig; la.all = 1u;
    he = hipDeviceSynchronize();   // allocZeroed cleared dScratch and dCounter on the null stream; the context's stream does not wait for it implicitly (as in rt_resize)
    if(he == hipSuccess) he = launchLightRecords(c->stream, la);
    if(he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if(he == hipSuccess) he = hipMemcpy(eval.data(), dScratch, size_t(numTrig) * sizeof(rt_trig_light), hipMemcpyDeviceToHost);
    if(he == hipSuccess) he = ensureEvents(c->evLights);
  }
  freePool(temp);
  if(rc || he != hipSuccess) {
    freePool(fresh);
    return rc ? rc : hipFail(c, "rt_set_light_sources", he);
  }
  for(uint32_t k = 0; k < numTrig; k++)
    if(memcmp(&recs[k].v0, &eval[k].v0, 3 * sizeof(rt_vec3)) != 0) {
      freePool(fresh);
      c->err = "rt_set_light_sources: record " + std::to_string(k) + " does not hold the positions of triangle " + std::to_string(sources[k].triangle) +
               " of instance " + std::to_string(sources[k].instance) + " (stale records: rt_update_lights first)";
      return RT_ERR_INVALID_ARG;
    }
  freePool(c->lightAllocs);
  c->lightAllocs = fresh;
  L = rt_ctx::Lights{};
  L.bound = numTrig; L.dSources = const_cast<rt_light_source*>(dSrc); L.dCounter = dCounter;
  L.instances.assign(nInst, 0);
  for(uint32_t k = 0; k < numTrig; k++) L.instances[sources[k].instance] = 1;
  L.stats.bound = numTrig;
  return RT_OK;
}

int rt_lights_readback(rt_ctx* c, int which, void* dst, size_t bytes)
{
  if(!c) return RT_ERR_INVALID_ARG;
  if(!c->haveScene) return fail(c, RT_ERR_NO_SCENE, "rt_lights_readback: no scene uploaded");
  const void* src = nullptr; size_t want = 0;
  switch(which) {
    case RT_LIGHTS_TRIG: src = c->ds.trigLights; want = size_t(c->ds.lightInfo.trigLightSize) * sizeof(rt_trig_light); break;
    case RT_LIGHTS_PUNC: src = c->ds.puncLights; want = size_t(c->ds.lightInfo.puncLightSize) * sizeof(rt_punc_light); break;
    default: return fail(c, RT_ERR_INVALID_ARG, "rt_lights_readback: which must be RT_LIGHTS_TRIG / _PUNC");
  }
  if(bytes != want || (want && !dst)) return fail(c, RT_ERR_INVALID_ARG, "rt_lights_readback: size mismatch");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  if(want) RT_HIP(c, hipMemcpy(dst, src, want, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_get_light_stats(rt_ctx* c, rt_light_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->lights.stats;
  return RT_OK;
}

/* ---- emitters: the mode's switch (include/rt_abi.h "Emitters") ---- */
int rt_set_emitter_meshes(rt_ctx* c, uint32_t numMeshes, const rt_emitter_mesh* meshes, uint32_t numRows, const rt_emitter_row* rows, float puncLightWeight)
{
  if(int rc = needTree(c, "rt_set_emitter_meshes")) return rc;
  rt_ctx::Emit& EM = c->emit;
  if(numMeshes == 0) {   // off: records, binding and lightInfo stay; the templates go with the next switch-on or upload
    EM.on = false;
    EM.stats.enabled = 0u;
    return RT_OK;
  }
  if(!meshes || (numRows && !rows)) return fail(c, RT_ERR_INVALID_ARG, "rt_set_emitter_meshes: NULL template array");
  if(!std::isfinite(puncLightWeight) || puncLightWeight < 0.f) return fail(c, RT_ERR_INVALID_ARG, "rt_set_emitter_meshes: puncLightWeight must be finite and not negative");
  auto refuse = [&](uint32_t m, const std::string& what) { c->err = "rt_set_emitter_meshes: template " + std::to_string(m) + ": " + what; return RT_ERR_INVALID_ARG; };
  std::vector<int64_t> first(c->primMeshes.size(), -1);
  std::vector<uint32_t> count(c->primMeshes.size(), 0u);
  for(uint32_t m = 0; m < numMeshes; m++) {
    const rt_emitter_mesh& em = meshes[m];
    if(em.primMesh >= c->primMeshes.size()) return refuse(m, "prim mesh out of range");
    if(first[em.primMesh] >= 0) return refuse(m, "prim mesh " + std::to_string(em.primMesh) + " is listed twice");
    const rt_prim_mesh& pm = c->primMeshes[em.primMesh];
    if(pm.materialIndex < 0 || !emissiveMesh(c, em.primMesh)) return refuse(m, "prim mesh " + std::to_string(em.primMesh) + " is not emissive by the scene's light rule");
    if(uint64_t(em.firstRow) + em.rowCount > numRows) return refuse(m, "row range outside rows");
    for(uint32_t r = em.firstRow; r < em.firstRow + em.rowCount; r++) {
      if(rows[r].triangle >= pm.indexCount / 3u) return refuse(m, "row " + std::to_string(r) + ": triangle beyond the prim mesh's index list");
      for(const float v : rows[r].uv) if(!std::isfinite(v)) return refuse(m, "row " + std::to_string(r) + ": non-finite uv");
    }
    first[em.primMesh] = int64_t(em.firstRow); count[em.primMesh] = em.rowCount;
  }
  EmitPlan plan;
  if(const int rc = planEmitters(c, "rt_set_emitter_meshes", uint32_t(c->instances.size()), c->instances.data(), first, count, puncLightWeight, plan)) return rc;
  if(plan.records != c->ds.lightInfo.trigLightSize) {
    c->err = "rt_set_emitter_meshes: the templates derive " + std::to_string(plan.records) + " records, the device holds " + std::to_string(c->ds.lightInfo.trigLightSize);
    return RT_ERR_INVALID_ARG;
  }
  if(memcmp(&plan.trigSampProb, &c->ds.lightInfo.trigSampProb, 4) != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_set_emitter_meshes: the derived trigSampProb differs from the device's (puncLightWeight)");
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  // Templates, the plan's words, scratch records and the candidate binding in pools of their own: nothing of the context changes before the derived records equal the
  // device's in all 96 bytes.
  std::vector<void*> fresh, binding, temp;
  std::vector<uint32_t> firstWords(first.size());
  for(size_t m = 0; m < first.size(); m++) firstWords[m] = first[m] < 0 ? 0u : uint32_t(first[m]);
  const rt_emitter_row* dRows = nullptr;
  const uint32_t* dFirst = nullptr;
  const rt_light_source* noSrc = nullptr; const rt_light_source* dSrc = nullptr;
  uint32_t* dCounter = nullptr;
  rt_trig_light* dScratch = nullptr;
  rt_ctx::Emit::Set S;   // staging only: its arrays live in temp
  const uint32_t n = plan.records;
  int rc = upload(c, fresh, rows, size_t(numRows), &dRows);
  if(!rc) rc = upload(c, fresh, firstWords.data(), firstWords.size(), &dFirst);
  if(!rc) rc = upload(c, binding, noSrc, size_t(n), &dSrc);
  if(!rc) rc = allocZeroed(c, binding, 1, &dCounter);
  if(!rc) rc = allocZeroed(c, temp, size_t(n), &dScratch);
  if(!rc) rc = allocZeroed(c, temp, size_t(n), &S.alias);
  if(!rc) rc = allocZeroed(c, temp, plan.prefix.size(), &S.prefix);
  if(!rc) rc = allocZeroed(c, temp, plan.ids.size(), &S.ids);
  std::vector<rt_trig_light> recs(n), eval(n);
  hipError_t he = hipSuccess;
  if(!rc) {
    he = hipDeviceSynchronize();   // the arrays above were cleared on the null stream (as in rt_set_light_sources)
    if(he == hipSuccess) he = ensureEvents(c->evLights);
    if(he == hipSuccess) he = ensureEvents(c->evEmit);
    if(he == hipSuccess) he = enqueueLightExpand(c, plan, S, c->ds.instances, dRows, dFirst, dScratch, const_cast<rt_light_source*>(dSrc));
    if(he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if(he == hipSuccess && n) he = hipMemcpy(eval.data(), dScratch, size_t(n) * sizeof(rt_trig_light), hipMemcpyDeviceToHost);
    if(he == hipSuccess && n) he = hipMemcpy(recs.data(), c->ds.trigLights, size_t(n) * sizeof(rt_trig_light), hipMemcpyDeviceToHost);
  }
  freePool(temp);
  if(rc || he != hipSuccess) {
    freePool(fresh); freePool(binding);
    return rc ? rc : hipFail(c, "rt_set_emitter_meshes", he);
  }
  for(uint32_t k = 0; k < n; k++)
    if(memcmp(&recs[k], &eval[k], sizeof(rt_trig_light)) != 0) {
      freePool(fresh); freePool(binding);
      const uint32_t e = uint32_t(std::upper_bound(plan.prefix.begin(), plan.prefix.end() - 1, k) - plan.prefix.begin()) - 1u;
      c->err = "rt_set_emitter_meshes: record " + std::to_string(k) + " on the device differs from the one derived for row " + std::to_string(k - plan.prefix[e]) +
               " of instance " + std::to_string(plan.ids[e]) + " (stale records: rt_update_lights first)";
      return RT_ERR_INVALID_ARG;
    }
  freePool(c->emitAllocs); c->emitAllocs = fresh;
  freePool(c->lightAllocs); c->lightAllocs = binding;
  c->lights.dCounter = dCounter;
  installDerivedBinding(c, plan, c->instances.size(), const_cast<rt_light_source*>(dSrc));
  EM.on = true;
  EM.meshFirstRow = first; EM.meshRows = count; EM.puncWeight = puncLightWeight;
  EM.dRows = const_cast<rt_emitter_row*>(dRows); EM.dMeshFirstRow = const_cast<uint32_t*>(dFirst);
  EM.stats = rt_emitter_stats{};
  EM.stats.enabled = 1u; EM.stats.records = n; EM.stats.emittingInstances = uint32_t(plan.ids.size());
  EM.stats.bytesUploaded = uint32_t(size_t(numRows) * sizeof(rt_emitter_row) + firstWords.size() * 4) + emitPlanBytes(plan);
  (void)hipEventElapsedTime(&EM.stats.expandMs, c->evEmit[0], c->evEmit[1]);
  return RT_OK;
}

int rt_get_emitter_stats(rt_ctx* c, rt_emitter_stats* out)
{
  if(!c || !out) return RT_ERR_INVALID_ARG;
  *out = c->emit.stats;
  return RT_OK;
}

/* extra introspection used by bench.py / DESIGN.md numbers (not part of the reference-facing surface) */
int rt_accel_stats(rt_ctx* c, uint64_t* numNodes, uint64_t* numTris, int* maxDepth)
{
  if(!c || !c->haveAccel) return RT_ERR_NO_ACCEL;
  if(numNodes) *numNodes = c->numNodes;
  if(numTris) *numTris = c->numTris;
  if(maxDepth) *maxDepth = c->maxDepth;
  return RT_OK;
}

/* tree quality: leaf records (references: > triangles when spatial splits duplicated some), spatial splits taken, and the SAH expectation of node / triangle
 * steps of a ray that hits the root box */
int rt_accel_quality(rt_ctx* c, uint64_t* references, uint64_t* spatialSplits, double* sahNodeSteps, double* sahTriSteps)
{
  if(!c || !c->haveAccel) return RT_ERR_NO_ACCEL;
  if(references) *references = c->numRefs;
  if(spatialSplits) *spatialSplits = c->spatialSplits;
  if(sahNodeSteps) *sahNodeSteps = c->sahNodeSteps;
  if(sahTriSteps) *sahTriSteps = c->sahTriSteps;
  return RT_OK;
}

#if RT_WAVEPROF
/* measurement builds only (scripts/wave_profile.py): read and clear the per-wave profile records kept in the hitRec scratch */
int rt_debug_wave_profile(rt_ctx* c, void* dst, size_t bytes)
{
  if(!c || !dst || c->W == 0) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  bytes = std::min(bytes, WAVEPROF_RECORDS * 64);
  RT_HIP(c, hipMemcpy(dst, c->scratch.waveProf, bytes, hipMemcpyDeviceToHost));
  RT_HIP(c, hipMemset(c->scratch.waveProf, 0, bytes));
  RT_HIP(c, hipDeviceSynchronize());
  return RT_OK;
}
#endif

int rt_measure_valu_peak(rt_ctx* c, int variant, int wavesPerSimd, double* waveInstPerSec)
{
  if(!c || !waveInstPerSec || variant < 0 || variant > 1 || wavesPerSimd < 1 || wavesPerSimd > 8) return RT_ERR_INVALID_ARG;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, syncAll(c));
  double seconds = 0.0;
  RT_HIP(c, measureValuIssue(c->stream, variant, wavesPerSimd, waveInstPerSec, &seconds));
  return RT_OK;
}

}  // extern "C"

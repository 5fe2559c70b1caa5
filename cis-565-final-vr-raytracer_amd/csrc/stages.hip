// stages.hip — the per-frame kernels of the ReSTIR DI+GI path on gfx950.
//
//   k_direct_stage     direct_stage.comp:150-288  (live)     primary ray + G-buffer + M-candidate RIS + shadow ray + temporal reuse + shade
//   k_direct_gen       direct_gen.comp:77-149     (compiled by the reference, dispatch disabled: renderer.cpp:166-168)
//   k_direct_reuse     direct_reuse.comp:102-153  (idem, renderer.cpp:170-171)
//   k_indirect_stage   indirect_stage.comp:129-309, half resolution, tile-level multi-bounce
//
// Launch shape: one wave64 per 8x8 pixel tile (= the reference's 8x8 workgroups, host_device.h:31-38), 1-D grid with
// an XCD-aware tile order: consecutive workgroup ids land on different XCDs (observed b % 8), so XCD x gets the x-th
// contiguous band of tile rows and its private 4 MiB L2 sees one compact screen region + the BVH subtrees under it.
// This file is compiled once per entry of STAGE_BUILDS in build.py (-D<switch>=1 per switch of the entry; no stub files): the table is the one statement of which
// builds exist, stage_select.h holds the same names and the rule that picks one per launch, DESIGN.md §28 says how to add one.  The switches (below): RT_SKY / RT_COUNT /
// RT_LAT for the plain builds, RT_OM for contexts with object motion vectors on, RT_VM for per-vertex motion vectors, RT_REPLAY for the direct stage of a camera at
// rest; what the switches do not reach is in filters.hip.
//   RT_SKY = 1    procedural sun & sky code paths compiled in.  Keeping sun_and_sky() out of the default kernels saves 13 VGPRs
//                 in k_direct_stage — the procedural sky is the rarely used mode (default in_use = 0, sample_example.hpp:202).
//   RT_COUNT = 1  traversal / shading counters (rt_set_counting) are flushed at the end of the traced kernels.  Without the
//                 flush the compiler removes the per-round counter increments from the traversal loops: -1.7 % frame time.
//   RT_LAT = 1    the traced kernels for SMALL launches (row bands of a multi-GPU frame, small images): the latency-mode traversal round of
//                 traverse.h and two waves per SIMD worth of registers.  Only k_direct_stage and k_indirect_stage are compiled; the rayless second half of
//                 the direct stage (k_direct_spatial) forwards to the throughput build.  rt_api.cpp picks per launch (launch size; rt_set_traversal forces).  Same bits.
#ifndef RT_SKY
#define RT_SKY 0
#endif
#ifndef RT_COUNT
#define RT_COUNT 0
#endif
#ifndef RT_LAT
#define RT_LAT 0
#endif
//   RT_OM = 1     object motion vectors (rt_set_object_motion): k_direct_stage and k_indirect_stage take a DevObjMotion, store the primary hit's
//                 instance per pixel and read lastProjView / lastPosition of the temporal lookup from the per-instance table instead of from the camera.  Every
//                 expression stays what it is; k_direct_spatial (no temporal lookup) forwards to base / sky; no counting build, no direct_gen / direct_reuse.
#ifndef RT_OM
#define RT_OM 0
#endif
//   RT_VM = 1     per-vertex motion vectors (rt_set_object_motion mode RT_OBJECT_MOTION_VERTEX): the same two kernels take a DevVtxMotion, store the
//                 instance image and the delta x_prev - state.position per pixel, and run the temporal lookups of both stages with the previous world position
//                 of the material point under the pixel (stage_common.h vmPrevPosition) and the camera's own lastProjView / lastPosition.  Forwards like RT_OM.
#ifndef RT_VM
#define RT_VM 0
#endif
//   RT_REPLAY = 1 settled primary visibility: k_direct_stage alone, taking a DevVis.  A RECORD launch traces the primary ray as every build does and
//                 then once more, culling by deterministic accepts only, to store what a camera at rest needs to know of it; REPLAY launches re-test the stored
//                 records with the frame's seed and run no traversal loop for the primary ray.  Base and sky, each with its counting form; no latency or
//                 object-motion form.  Every other stage and the rayless half of the direct stage forward to the plain build.
#ifndef RT_REPLAY
#define RT_REPLAY 0
#endif
#if RT_REPLAY && (RT_OM || RT_VM || RT_LAT)
#error "primary replay exists for the throughput builds without motion vectors only"
#endif
#if (RT_OM || RT_VM) && RT_COUNT
#error "object motion vectors have no counting build"
#endif
#if RT_OM && RT_VM
#error "RT_OM and RT_VM are two builds"
#endif
// RT_OM_PARAM / RT_OM_ARG: the motion-vector argument of the device functions between the kernels and the shading, RT_OM_KPARAM: of the kernels
#if RT_OM
#define RT_OM_PARAM , const DevObjMotion& OM
#define RT_OM_KPARAM , DevObjMotion OM
#define RT_OM_ARG , OM
#elif RT_VM
#define RT_OM_PARAM , const DevVtxMotion& OM
#define RT_OM_KPARAM , DevVtxMotion OM
#define RT_OM_ARG , OM
#else
#define RT_OM_PARAM
#define RT_OM_KPARAM
#define RT_OM_ARG
#endif
#if RT_LAT && RT_COUNT
#error "the counting build exists for the throughput kernels only"
#endif
// The build's namespace, pasted from the switches: environment, then _lat, then _om / _vm / _rp, then _cnt (the names of RT_STAGE_BUILDS, stage_select.h).
// RT_FORWARD, for the builds that hold a part of the kernels only: the plain build of the same environment and counting, which launches the rest.
#if RT_SKY
#define RT_NS_ENV sky
#else
#define RT_NS_ENV base
#endif
#if RT_LAT
#define RT_NS_LAT _lat
#else
#define RT_NS_LAT
#endif
#if RT_OM
#define RT_NS_FORM _om
#elif RT_VM
#define RT_NS_FORM _vm
#elif RT_REPLAY
#define RT_NS_FORM _rp
#else
#define RT_NS_FORM
#endif
#if RT_COUNT
#define RT_NS_CNT _cnt
#else
#define RT_NS_CNT
#endif
#define RT_NS_PASTE_(a, b, c, d) a##b##c##d
#define RT_NS_PASTE(a, b, c, d) RT_NS_PASTE_(a, b, c, d)
#define RT_VARIANT RT_NS_PASTE(RT_NS_ENV, RT_NS_LAT, RT_NS_FORM, RT_NS_CNT)
#if RT_LAT || RT_OM || RT_VM || RT_REPLAY
#define RT_FORWARD RT_NS_PASTE(RT_NS_ENV, , , RT_NS_CNT)
#endif
#include "stage_common.h"
#include <algorithm>

namespace rt {
namespace RT_VARIANT {

// ------------------------------------------------------------------------------------------------------------
// direct_stage.comp
// ------------------------------------------------------------------------------------------------------------
// launch bounds of the two traced kernels, re-measured in round 2 under the final schedule (frames in flight, ms/frame, same box):
// (direct, indirect) waves per SIMD = (5,5) 3.155, (4,5) 3.121, (4,4) 3.29, (5,4) 3.59, (3,5) 3.16, (4,6) 3.15  =>  (4, 5)
// and again in round 4 on the build whose traversal stacks and filters had given LDS back (profiles/r04_launch_bounds_ab.txt, two boxes):
// (4,5) 2.987 / 2.993, (5,5) 2.901 / 2.893, (6,5) 2.891, (5,4) 2.923, (4,4) 2.995, (5,6) 2.904, (6,6) 2.920  =>  (5, 5): 96 VGPRs and 31 spilled
// values (60 B of scratch per lane, none of it inside a traversal loop) buy a fifth wave per SIMD.
#ifndef RT_DIRECT_LB
#define RT_DIRECT_LB 5
#endif
// ReSTIRDirect (direct_stage.comp:150-270) cut at its one shadow ray, so that the ray can be traced by whatever the build uses (the lane's own
// traversal loop in the throughput build, the workgroup's ray pool in the latency build) while both builds share every line of shading:
//   directPre   primary hit -> G-buffer, motion vector, M-candidate RIS (or the single DirectLight sample); returns whether a shadow ray is needed
//   directPost  visibility of the winner, temporal reuse, reservoir store, shading, result store
struct DirectCont {
  State state; f3 wo, radiance; i2 motionIdx;
  rt_direct_reservoir resv; uint32_t lid;
  float pdf;     // kind 2: pdf of the single light sample (kept in resv.lightSample)
#if RT_OM
  uint32_t inst; // instance of the primary hit
#elif RT_VM
  float reprojDepth;   // length(lastPosition - x_prev): all of x_prev that crosses the shadow-ray trace, beside motionIdx
#endif
  int kind;      // 0: radiance is final (miss, emitter, debug view), 1: RIS reservoir, 2: single sample (ReSTIRState none)
};
RT_DEV float occlusionDist(const Ray& ray, f3 statePos, float dist)   // Occlusion, pathtrace.glsl:18-22
{
  return ((dist - rt_abs(ray.origin.x - statePos.x)) - rt_abs(ray.origin.y - statePos.y)) - rt_abs(ray.origin.z - statePos.z);
}
RT_DEV bool directPre(Ctx& c, const DevFrame& F RT_OM_PARAM, const rt_state& st, i2 px, const Ray& r, DirectCont& K, Ray& shadowRay, float& shadowDist)
{
  const size_t index = size_t(px.y) * st.size.x + px.x;
  K.kind = 0; K.radiance = mk3(0.0f);
  if(c.hit.t >= RT_INFINITY) {  // :155-159
    F.thisG[index] = make_uint4(rt_f2u(RT_INFINITY), 0u, 0u, RT_INVALID_MAT_ID);
    storeMotion(F, px, i2{0, 0});
#if RT_OM
    OM.instImage[index] = 0xffffffffu;
#elif RT_VM
    OM.instImage[index] = 0xffffffffu;
    OM.delta[index] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#endif
    K.radiance = c.EnvRadiance(r.direction);
    return false;
  }
  State& state = K.state;
  state = c.GetState(r.direction);
  c.GetMaterials(state, r);
#if RT_OM
  K.inst = gLoadU32(&c.S.triRef[c.hit.gid].inst);
  OM.instImage[index] = K.inst;
  K.motionIdx = createMotionIndexOm(c, OM, K.inst, state.position);
#elif RT_VM
  {
    const uint32_t inst = gLoadU32(&c.S.triRef[c.hit.gid].inst);
    OM.instImage[index] = inst;
    const f3 xPrev = vmPrevPosition(c, OM, inst, state.position);
    const f3 d = xPrev - state.position;
    OM.delta[index] = make_float4(d.x, d.y, d.z, 0.0f);
    K.motionIdx = createMotionIndex(c, xPrev);
    K.reprojDepth = length(mk3(c.cam.lastPosition) - xPrev);
  }
#else
  K.motionIdx = createMotionIndex(c, state.position);
#endif
  const uint4 gInfo = encodeGeometryInfo(state, c.hit.t);
  storeMotion(F, px, K.motionIdx);
  F.thisG[index] = gInfo;
  if(st.debugging_mode > RT_DBG_INDIRECT_STAGE) { K.radiance = c.DebugInfo(state); return false; }
  if(state.isEmitter) { K.radiance = state.mat.emission; return false; }
  K.wo = -r.direction;
  state.mat.albedo = mk3(1.0f);
  K.resv = zeroDirectResv();
  K.lid = 0xffffffffu;
  if(st.ReSTIRState == RT_RESTIR_NONE) {  // DirectLight, pathtrace.glsl:205-220
    K.kind = 2;
    rt_light_sample ls;
    K.pdf = c.SampleDirectLightNoVisibility(state.position, ls);
    K.resv.lightSample = ls;
    if(Ctx::IsPdfInvalid(K.pdf)) return false;
    shadowRay = Ray{OffsetRay(state.position, state.ffnormal), mk3(ls.wi)};
    shadowDist = occlusionDist(shadowRay, state.position, ls.dist);
    return true;
  }
  K.kind = 1;
  return risCandidatesNoVisibility(c, state, K.wo, K.resv, K.lid, shadowRay, shadowDist);
}
RT_DEV void directPost(Ctx& c, const DevFrame& F RT_OM_PARAM, const rt_state& st, const rt_scene_camera& cam, i2 px, DirectCont& K, bool occluded)
{
  const size_t index = size_t(px.y) * st.size.x + px.x;
  const bool spatial = st.ReSTIRState == RT_RESTIR_SPATIAL || st.ReSTIRState == RT_RESTIR_SPATIOTEMPORAL;
  bool deferred = false;
  f3 radiance = K.radiance;
  if(K.kind != 0) {
    State& state = K.state;
    const f3 wo = K.wo;
    f3 direct = mk3(0.0f);
    if(K.kind == 2) {
      const rt_light_sample ls = K.resv.lightSample;
      if(!Ctx::IsPdfInvalid(K.pdf) && !occluded)
        direct = mk3(ls.Li) * metallicWorkflowBSDF(state.mat, state.ffnormal, wo, mk3(ls.wi)) * rt_max(dot(state.ffnormal, mk3(ls.wi)), 0.0f) / K.pdf;
    } else {
      rt_direct_reservoir& resv = K.resv;
      uint32_t lid = K.lid;
      if(occluded) resv.weight = 0.0f;
      if(st.ReSTIRState == RT_RESTIR_TEMPORAL || st.ReSTIRState == RT_RESTIR_SPATIOTEMPORAL) {
#if RT_OM
        const float reprojDepth = length(omLastPosition(OM, cam, K.inst) - state.position);
#elif RT_VM
        const float reprojDepth = K.reprojDepth;
#else
        const float reprojDepth = length(mk3(cam.lastPosition) - state.position);
#endif
        rt_direct_reservoir temporal; uint32_t tlid = 0xffffffffu;
        if(findTemporalNeighborDirect(F, st, state.normal, reprojDepth, state.matID, K.motionIdx, temporal, tlid)) {
          if(!resvInvalidW(temporal.weight)) { if(resvMerge(resv, temporal, rnd(c.seed))) lid = tlid; }
        }
      }
      rt_direct_reservoir tempResv = resv;
      if(resvInvalidW(tempResv.weight)) { tempResv.num = 0; tempResv.weight = 0.f; }
      resvClamp(tempResv, st.RISSampleNum * st.reservoirClamp);
      F.thisDirectResv[index] = tempResv;  // saveNewReservoir
      F.thisLightId[index] = lid;
      if(spatial) {
        // Spatial / spatiotemporal reuse (:224-255) reads the reservoirs its neighbours cache here.  The reference orders
        // that with workgroup barriers only (neighbours in other workgroups race); this build finishes the pixel in a
        // second kernel (k_direct_spatial) once every pixel of the launch has cached its reservoir.
        if(resvInvalidW(resv.weight)) { resv.num = 0; resv.weight = 0.f; }  // resvCheckValidity(resv) :231
        F.tempDirectResv[index] = resv;                                      // cacheTempReservoir :234
        SurfRec sr;
        sr.position = toR(state.position); sr.normal = toR(state.normal); sr.ffnormal = toR(state.ffnormal); sr.emission = toR(state.mat.emission);
        sr.roughness = state.mat.roughness; sr.metallic = state.mat.metallic; sr.matID = state.matID; sr.seed = c.seed;
        F.surf[index] = sr;
        deferred = true;
      } else {
        const rt_light_sample ls = resv.lightSample;
        if(!resvInvalidW(resv.weight)) {
          f3 LiBsdf = mk3(ls.Li) * metallicWorkflowBSDF(state.mat, state.ffnormal, wo, mk3(ls.wi));
          direct = LiBsdf / resvToScalar(LiBsdf) * resv.weight / float(resv.num);
        }
      }
    }
    if(rt_isnan(direct.x) || rt_isnan(direct.y) || rt_isnan(direct.z)) direct = mk3(0.0f);
    radiance = HDRToLDR(c.clampRadiance(state.mat.emission + direct));
  }
  if(spatial) F.status[index] = deferred ? 1u : 0u;
  if(!deferred) {
    const f3 pixelColor = c.clampRadiance(radiance);
    storeImg(F.thisDirectResult, F, px, mk4(pixelColor, 1.0f));  // :286
  }
}

#if RT_LAT
// ---- latency build: a workgroup of NW waves per 8x8 tile.  Wave 0 owns the 64 pixels (everything that is not traversal runs there, one lane per pixel,
// exactly the code of the throughput build); rays go through the workgroup's LDS pool and every wave traces them eight lanes per ray (tracePoolWide).
struct WideLds { uint2* stacks; float4* pool; unsigned char* list; uint32_t* ctrl; };   // ctrl: [0] rays listed, [1] cursor, [2] wave 0 has finished
__host__ __device__ inline size_t wideWaveStride(int stackEntries) { return size_t(stackEntries) * WIDE_RAYS + GANG_BOX_UINT2; }   // per wave: 8 stack columns + the gang mailbox (uint2 units)
RT_DEV WideLds wideLds(uint2* base, int stackEntries, int nWaves)
{
  WideLds L;
  L.stacks = base;
  L.pool = reinterpret_cast<float4*>(base + size_t(nWaves) * wideWaveStride(stackEntries));
  L.list = reinterpret_cast<unsigned char*>(L.pool + 128 * POOL_SLOT_F4);
  L.ctrl = reinterpret_cast<uint32_t*>(L.list + 128);
  return L;
}
inline size_t wideLdsBytes(int stackEntries, int nWaves) { return size_t(nWaves) * wideWaveStride(stackEntries) * sizeof(uint2) + 128 * 32 + 128 + 16; }
// wave 0, all 64 lanes: list the slots its lanes filled (slot 2 * lane: closest-hit ray, 2 * lane + 1: any-hit ray)
RT_DEV void poolPublish(const WideLds& L, bool hasC, bool hasS)
{
  const int lane = int(threadIdx.x) & 63;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const unsigned long long mC = __ballot(hasC ? 1 : 0), mS = __ballot(hasS ? 1 : 0);
  const int nC = __popcll(mC);
  if(hasC) L.list[__popcll(mC & lt)] = (unsigned char)(lane * 2);
  if(hasS) L.list[nC + __popcll(mS & lt)] = (unsigned char)((lane * 2 + 1) | 0x80);
  if(lane == 0) { L.ctrl[0] = uint32_t(nC + __popcll(mS)); L.ctrl[1] = 0u; L.ctrl[2] = 0u; }
}
// every wave of the workgroup (REC: results carry the leaf record of their hit, poolGetRec)
template <bool REC>
RT_DEV void groupTrace(const DevScene& S, const WideLds& L, TravCounters& tc)
{
  __syncthreads();
  const int wave = int(threadIdx.x) >> 6;
  tracePoolWide<REC>(S, L.pool, L.list, int(L.ctrl[0]), &L.ctrl[1], L.stacks + size_t(wave) * wideWaveStride(S.stackEntries), tc);
  __syncthreads();
}

#ifndef RT_LAT_DIRECT_WAVES
#define RT_LAT_DIRECT_WAVES 4   // 128 VGPRs: two workgroups per CU (151 VGPRs and one workgroup at 2: 15-30 % slower on every band, scripts/variants_ab.sh with -DRT_LAT_DIRECT_WAVES=2)
#endif
__global__ __launch_bounds__(512, RT_LAT_DIRECT_WAVES) void k_direct_stage(DevScene S, DevFrame F RT_OM_KPARAM, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  extern __shared__ uint2 s_stack[];
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int wave = int(threadIdx.x) >> 6, lane = int(threadIdx.x) & 63;
  const WideLds L = wideLds(s_stack, S.stackEntries, int(blockDim.x) >> 6);
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  const bool mine = wave == 0 && !(px.x >= st.size.x || px.y >= rowEnd);
#if RT_WAVEPROF
  const uint64_t p0 = clock64(), w0 = wall_clock64();
  uint64_t p1 = 0, p2 = 0, p3 = 0, p4 = 0;
#endif
  Ctx c(S, st, cam, nullptr);
  Ray r{mk3(0.0f), mk3(0.0f)};
  if(mine) {
    c.imageCoords = px;
    c.seed = tea(uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x), st.time);  // :279
    r = c.raySpawn(px, i2{st.size.x, st.size.y});
    c.nClosest++;
    poolPut(L.pool, lane * 2, r.origin, r.direction, RT_INFINITY, c.seed);
  }
  if(wave == 0) poolPublish(L, mine, false);
#if RT_WAVEPROF
  p1 = clock64();
#endif
  groupTrace<true>(S, L, c.tc);
#if RT_WAVEPROF
  p2 = clock64();
#endif
  DirectCont K;
  Ray shadowRay{mk3(0.0f), mk3(0.0f)};
  float shadowDist = 0.0f;
  bool wantShadow = false;
  if(mine) {
    c.hit = poolGet(L.pool, lane * 2);
    // The latency build WRITES the seed plane (DevFrame::seedOut), so that a context whose launches switch between the builds (RT_TRAVERSAL_AUTO) keeps it
    // warm, and does not test the seed: its rays go through the workgroup pool, whose slots have no room for a seeded hit, and it never runs a full frame.
    F.seedOut[size_t(px.y) * st.size.x + px.x] = poolGetRec(L.pool, lane * 2);
    wantShadow = directPre(c, F RT_OM_ARG, st, px, r, K, shadowRay, shadowDist);
    if(wantShadow) { c.nAny++; poolPut(L.pool, lane * 2 + 1, shadowRay.origin, shadowRay.direction, shadowDist, c.seed); }
  }
  if(wave == 0) poolPublish(L, false, wantShadow);
#if RT_WAVEPROF
  p3 = clock64();
#endif
  groupTrace<false>(S, L, c.tc);
#if RT_WAVEPROF
  p4 = clock64();
#endif
  if(mine) directPost(c, F RT_OM_ARG, st, cam, px, K, wantShadow && poolGet(L.pool, lane * 2 + 1).gid != 0xffffffffu);
#if RT_WAVEPROF
  {  // record: 0 x | 1 y | 2 workgroup cycles | 3 primary trace | 4 shadow trace | 5 node-only rounds (max over waves) | 6 rounds with triangles | 7 raygen | 8 cyc node rounds | 9 cyc tri rounds | 10 pre | 11 post | 15 ticks
    uint32_t* rec = F.waveProf + size_t(blockIdx.x) * 16;
    const uint64_t p5 = clock64();
    if(wave == 0 && lane == 0) {
      rec[0] = uint32_t(tile.x); rec[1] = uint32_t(tile.y); rec[2] = uint32_t(p5 - p0); rec[3] = uint32_t(p2 - p1); rec[4] = uint32_t(p4 - p3);
      rec[7] = uint32_t(p1 - p0); rec[10] = uint32_t(p3 - p2); rec[11] = uint32_t(p5 - p4); rec[15] = uint32_t(wall_clock64() - w0);
    }
    if(lane == 0) { atomicMax(&rec[5], c.tc.rN); atomicMax(&rec[6], c.tc.rT); atomicMax(&rec[8], c.tc.cN); atomicMax(&rec[9], c.tc.cT); atomicAdd(&rec[12], c.tc.rC); atomicAdd(&rec[13], c.tc.rN + c.tc.rT);   // 12 / (8 x 13) = share of the ray slots in use
      uint32_t* acc = F.waveProf + size_t(65535) * 16;   // launch totals: cycles by phase of the triangle step, [7] = steps, [8] = cycles of rounds with a triangle step
      for(int k = 0; k < 7; k++) atomicAdd(&acc[k], c.tc.ph[k] >> 4);
      atomicAdd(&acc[7], c.tc.ph[7]);
      atomicAdd(&acc[8], c.tc.cT >> 4);
      for(int k = 0; k < 3; k++) atomicAdd(&acc[9 + k], c.tc.nph[k] >> 4);
      atomicAdd(&acc[12], c.tc.nph[3]); }
  }
#endif
}
#elif RT_REPLAY
// ---- settled primary visibility ----------------------------------------------------------------------------------------------------------------
// For a fixed ray and scene every candidate that passes the geometric part of triCandidateGeom (intersection, range, padded box) is a DETERMINISTIC accept (opaque,
// or opacity micro-map cell state 1) or STOCHASTIC (cell state 0 or 2: the verdict draws from (ray seed, triangle id)).  With d* the lexicographic minimum of
// (t, globalId) over the deterministic accepts, the frame's hit is the minimum over the accepted members of R = {d*} + {stochastic candidates in front of d*}; R
// depends on (ray, scene) only.  The kind of a candidate, by the tests and in the order of triCandidateGeom: 0 rejected, 1 deterministic accept, 2 stochastic.
RT_DEV int recordCandidateKind(const DevScene& S, const TriRegs& Q, f3 o, f3 d, float curT, uint32_t curG, float& t, uint32_t& gid)
{
  const uint4 a = Q.a, b = Q.b, c = Q.c, om = Q.om;
  Tri48 R;
  R.v0x = rt_u2f(a.x); R.v0y = rt_u2f(a.y); R.v0z = rt_u2f(a.z); R.e1x = rt_u2f(a.w);
  R.e1y = rt_u2f(b.x); R.e1z = rt_u2f(b.y); R.e2x = rt_u2f(b.z); R.e2y = rt_u2f(b.w);
  R.e2z = rt_u2f(c.x); R.globalId = c.y; R.flags = c.z; R.alphaIdx = c.w;
  gid = R.globalId;
  float u, v;
  if(!intersectTri(R, o, d, t, u, v)) return 0;
  if(!(t > 0.0f && t < RT_INFINITY)) return 0;
  if(!(t < curT || (t == curT && R.globalId < curG))) return 0;
  if(!hitInsidePaddedBox(R, o, d, S.triPad, t)) return 0;
  if(R.flags & TRI_OPAQUE) return 1;
  const int ci = min(int(u * 8.0f), 7), cj = min(int(v * 8.0f), 7);
  const int cell = cj * 8 + ci;
  const uint32_t word = (cell < 16) ? om.x : ((cell < 32) ? om.y : ((cell < 48) ? om.z : om.w));
  return ((word >> ((cell & 15) * 2)) & 3u) == 1u ? 1 : 2;
}
// The recording traversal: a closest-hit traversal whose best-so-far (T.hit.t, T.hit.gid) is the best DETERMINISTIC accept, so that the slab test and the range
// test cull by those alone, and that appends every stochastic candidate it meets in front of it to the pixel's list.  A candidate appended early can end up behind
// the final d*: the replay's closer-than-best rule rejects it.  One step per lane and iteration, no vote: this runs once per stay of the camera.
RT_DEV void recordPrimary(const DevScene& S, const Ray& r, uint2* stack, const DevVis& V, uint32_t pix, uint32_t npix, TravCounters& tc)
{
  Trav T;
  bool live = travInit<0>(T, r.origin, r.direction, RT_INFINITY, 0u);
  uint32_t det = VIS_NO_DET, cnt = 0u;
  bool overflow = false;
  while(live) {
    if(travHasTris(T)) {
      const uint32_t bit = 31u - uint32_t(__clz(int(T.tgroup.y)));
      T.tgroup.y &= ~(1u << bit);
      tc.tris++;
      const uint32_t idx = T.tgroup.x + bit;
      float t; uint32_t gid;
      const int kind = recordCandidateKind(S, triLoad(S, idx), T.o, T.d, T.hit.t, T.hit.gid, t, gid);
      if(kind == 1) { T.hit.t = t; T.hit.gid = gid; det = idx; }
      else if(kind == 2) {
        if(cnt < V.K) { V.list[size_t(cnt) * npix + pix] = idx; cnt++; }
        else overflow = true;
      }
    } else travNode(S, T, stack, tc);
    live = travHasTris(T) || travHasNodes(T);
  }
  V.det[pix] = det;
  V.count[pix] = overflow ? VIS_OVERFLOW : cnt;
}
// The replay: d* first, then the listed candidates, each through the ordinary triCandidate with this frame's seed and the ordinary closer-than-best rule — the
// (t, gid, u, v) bits the traversal would return, with no node step.  Returns the record of the hit (the next frame's seed), 0xffffffff at a miss.
RT_DEV uint32_t replayPrimary(Ctx& c, const Ray& r, const DevVis& V, uint32_t pix, uint32_t npix, uint32_t cnt)
{
  RayHit h; h.t = RT_INFINITY; h.gid = 0xffffffffu; h.u = 0.f; h.v = 0.f;
  uint32_t rec = 0xffffffffu;
  cnt = min(cnt, V.K);
  for(uint32_t i = 0; i <= cnt; i++) {
    const uint32_t e = gLoadU32(i == 0u ? V.det + pix : V.list + (size_t(i - 1u) * npix + pix));
    if(e >= c.S.numTris) continue;   // VIS_NO_DET
    c.tc.tris++;
    float t, u, v; uint32_t gid;
    if(triCandidate(c.S, e, r.origin, r.direction, false, RT_INFINITY, h.t, h.gid, c.seed, t, u, v, gid, c.tc)) { h.t = t; h.gid = gid; h.u = u; h.v = v; rec = e; }
  }
  c.hit = h;
  return rec;
}
// Two kernels, so that the replay — the one that runs every frame — carries no recording traversal
template <bool RECORD>
__global__ __launch_bounds__(64, RT_DIRECT_LB) void k_direct_stage(DevScene S, DevFrame F, DevVis V, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  extern __shared__ uint2 s_stack[];
#if RT_WAVEPROF
  const uint64_t prof_c0 = clock64(), prof_w0 = wall_clock64();
#endif
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  if(px.x >= st.size.x || px.y >= rowEnd) return;

  Ctx c(S, st, cam, s_stack + lane);
  c.imageCoords = px;
  c.seed = tea(uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x), st.time);  // :279
  const Ray r = c.raySpawn(px, i2{st.size.x, st.size.y});
  {  // The primary ray.  RECORD: today's seeded trace for this frame's hit, then the recording traversal.  REPLAY: a pixel whose list fits re-tests its records; a
     // pixel in OVERFLOW runs today's seeded trace (in a partial wave, which the trace's ballots allow for).  A replayed query counts as a query (nClosest), and the
     // seed plane is written every frame so that it is warm when motion starts.
    const uint32_t pix = uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x), npix = uint32_t(st.size.x) * uint32_t(st.size.y);
    const uint32_t cnt = RECORD ? VIS_OVERFLOW : gLoadU32(V.count + pix);
    uint32_t rec;
    if(cnt == VIS_OVERFLOW) {
      const uint32_t seedTri = F.seedIn ? gLoadU32(F.seedIn + pix) : 0xffffffffu;
      rec = c.ClosestHitSeeded(r, seedTri);
    } else {
      c.nClosest++;
      rec = replayPrimary(c, r, V, pix, npix, cnt);
    }
    if(RECORD) recordPrimary(S, r, c.stack, V, pix, npix, c.tc);
    F.seedOut[size_t(px.y) * st.size.x + px.x] = rec;
  }
  DirectCont K;
  Ray shadowRay{mk3(0.0f), mk3(0.0f)};
  float shadowDist = 0.0f;
  const bool wantShadow = directPre(c, F, st, px, r, K, shadowRay, shadowDist);
  const bool occluded = wantShadow && c.AnyHit(shadowRay, shadowDist);
  directPost(c, F, st, cam, px, K, occluded);
  flushCounters(F, c);
#if RT_WAVEPROF
  waveProfFlush(F, c, tile.x, tile.y, prof_c0, prof_w0);
#endif
}
#else
__global__ __launch_bounds__(64, RT_DIRECT_LB) void k_direct_stage(DevScene S, DevFrame F RT_OM_KPARAM, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  extern __shared__ uint2 s_stack[];
#if RT_WAVEPROF
  const uint64_t prof_c0 = clock64(), prof_w0 = wall_clock64();
#endif
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  if(px.x >= st.size.x || px.y >= rowEnd) return;

  Ctx c(S, st, cam, s_stack + lane);
  c.imageCoords = px;
  c.seed = tea(uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x), st.time);  // :279
  const Ray r = c.raySpawn(px, i2{st.size.x, st.size.y});
  {  // The primary ray, seeded with the record this pixel hit last frame (DevFrame::seedIn); the record of this frame's hit is the next frame's seed, stored
     // before the shading so that it is not live across it.  The read indexes with the 32-bit pixel number the seed hash above already holds and the write with
     // directPre's own `index` expression, so that no address of the plane has to survive the traversal loop (a shared 64-bit index did: 8 B more scratch).
    const uint32_t seedTri = F.seedIn ? gLoadU32(F.seedIn + (uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x))) : 0xffffffffu;
    const uint32_t rec = c.ClosestHitSeeded(r, seedTri);
    F.seedOut[size_t(px.y) * st.size.x + px.x] = rec;
  }
  DirectCont K;
  Ray shadowRay{mk3(0.0f), mk3(0.0f)};
  float shadowDist = 0.0f;
  const bool wantShadow = directPre(c, F RT_OM_ARG, st, px, r, K, shadowRay, shadowDist);
  const bool occluded = wantShadow && c.AnyHit(shadowRay, shadowDist);
  directPost(c, F RT_OM_ARG, st, cam, px, K, occluded);
  flushCounters(F, c);
#if RT_WAVEPROF
  waveProfFlush(F, c, tile.x, tile.y, prof_c0, prof_w0);
#endif
}
#endif

#if !RT_LAT && !RT_OM && !RT_VM && !RT_REPLAY   // (to the end of k_direct_reuse: the throughput builds' three kernels without a latency or an object-motion form)
// Second half of direct_stage.comp's ReSTIRDirect for the spatial modes (:86-121, 236-262): two rounds of five neighbour
// merges from the cached reservoirs, the final merge and the shading.  No rays.
// The 10 x 10 block of cached reservoirs around the 8 x 8 tile (every neighbour lies within one pixel) is staged in LDS once and the
// ten neighbour reads of a pixel come from there (north_star design list: LDS neighbour-reservoir tile).  Against the global gather,
// Sponza-class 1080p, serial: 135 -> 90 us per launch, VMEM reads 1.46 M -> 0.46 M, SQ_WAIT_ANY -62 % (profiles/r02_spatial_lds_ab.txt).
__global__ __launch_bounds__(64) void k_direct_spatial(DevScene S, DevFrame F, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  __shared__ uint32_t s_nb[100 * 9];
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  const int nbx0 = tile.x * 8 - 1, nby0 = rowBegin + tile.y * 8 - 1;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(F.tempDirectResv);
    for(int k = lane; k < 100; k += 64) {
      const int rx = nbx0 + k % 10, ry = nby0 + k / 10;
      if(rx >= 0 && ry >= 0 && rx < st.size.x && ry < st.size.y) {
        const size_t o = (size_t(ry) * st.size.x + rx) * 9;
#pragma unroll
        for(int w = 0; w < 9; w++) s_nb[k * 9 + w] = src[o + w];
      }
    }
    __syncthreads();
  }
  if(px.x >= st.size.x || px.y >= rowEnd) return;
  const size_t index = size_t(px.y) * st.size.x + px.x;
  if(F.status[index] != 1u) return;
  Ctx c(S, st, cam, nullptr);
  c.imageCoords = px;
  const SurfRec sr = F.surf[index];
  c.seed = sr.seed;
  rt_direct_reservoir resv = F.tempDirectResv[index];
  const uint4 g = F.thisG[index];
  const f3 pnorm = decompress_unit_vec(g.y);          // loadThisGeometryInfo(imageCoords, ...): the pixel's own G-buffer entry
  const float pdepth = rt_u2f(g.x), depth = pdepth;   // prd.hitT is what encodeGeometryInfo stored in .x
  const f3 normal = mk3(sr.normal), ffnormal = mk3(sr.ffnormal);
  const i2 size{st.size.x, st.size.y};
  rt_direct_reservoir spatial = zeroDirectResv();
  for(int round = 0; round < 2; round++) {
    rt_direct_reservoir agg = zeroDirectResv();
    bool valid = false;
    for(int i = 0; i < 5; i++) {
      const float r0 = rnd(c.seed), r1 = rnd(c.seed);
      const f2 p = toConcentricDisk(mk2(r0, r1));
      const i2 q{rt_ftoi((float(px.x) + p.x) + 0.5f), rt_ftoi((float(px.y) + p.y) + 0.5f)};
      if(!inBound(q, size)) continue;
      if(dot(normal, pnorm) < 0.5f || rt_abs(depth - pdepth) > depth * 0.1f) continue;
      rt_direct_reservoir nb;
      {
        const uint32_t* e = s_nb + ((q.y - nby0) * 10 + (q.x - nbx0)) * 9;
        uint32_t* d = reinterpret_cast<uint32_t*>(&nb);
#pragma unroll
        for(int w = 0; w < 9; w++) d[w] = e[w];
      }
      if(!resvInvalidW(nb.weight)) { resvMerge(agg, nb, rnd(c.seed)); valid = true; }
    }
    if(valid && !resvInvalidW(agg.weight)) resvMerge(spatial, agg, rnd(c.seed));
  }
  if(!resvInvalidW(spatial.weight)) resvMerge(resv, spatial, rnd(c.seed));
  const Ray r = c.raySpawn(px, size);
  const f3 wo = -r.direction;
  Material mat;
  mat.albedo = mk3(1.0f); mat.emission = mk3(sr.emission); mat.metallic = sr.metallic; mat.roughness = sr.roughness; mat.ior = 0.f; mat.transmission = 0.f;
  f3 direct = mk3(0.0f);
  const rt_light_sample ls = resv.lightSample;
  if(!resvInvalidW(resv.weight)) {
    const f3 LiBsdf = mk3(ls.Li) * metallicWorkflowBSDF(mat, ffnormal, wo, mk3(ls.wi));
    direct = LiBsdf / resvToScalar(LiBsdf) * resv.weight / float(resv.num);
  }
  if(rt_isnan(direct.x) || rt_isnan(direct.y) || rt_isnan(direct.z)) direct = mk3(0.0f);
  const f3 radiance = HDRToLDR(c.clampRadiance(mat.emission + direct));
  storeImg(F.thisDirectResult, F, px, mk4(c.clampRadiance(radiance), 1.0f));
}

// ------------------------------------------------------------------------------------------------------------
// direct_gen.comp / direct_reuse.comp
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_direct_gen(DevScene S, DevFrame F, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  extern __shared__ uint2 s_stack[];
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  if(px.x >= st.size.x || px.y >= rowEnd) return;
  Ctx c(S, st, cam, s_stack + lane);
  c.imageCoords = px;
  const size_t index = size_t(px.y) * st.size.x + px.x;
  c.seed = tea(uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x), st.time);  // direct_gen.comp:146
  const Ray r = c.raySpawn(px, i2{st.size.x, st.size.y});
  c.ClosestHit(r);
  rt_direct_reservoir resv = zeroDirectResv();
  uint32_t lid = 0xffffffffu;
  if(c.hit.t >= RT_INFINITY * 0.8f) {  // :86
    uint4 g = make_uint4(rt_f2u(RT_INFINITY), 0u, 0u, RT_INVALID_MAT_ID);
    updateGeometryAlbedo(g, c.EnvRadiance(r.direction));
    F.thisG[index] = g;
    storeMotion(F, px, i2{0, 0});
  } else {
    State state = c.GetState(r.direction);
    c.GetMaterials(state, r);
    storeMotion(F, px, createMotionIndex(c, state.position));
    uint4 g = encodeGeometryInfo(state, c.hit.t);
    if(st.debugging_mode > RT_DBG_INDIRECT_STAGE) updateGeometryAlbedo(g, c.DebugInfo(state));
    else if(state.isEmitter) updateGeometryAlbedo(g, state.mat.emission);
    else {
      state.mat.albedo = mk3(1.0f);
      risCandidates(c, state, -r.direction, resv, lid);
    }
    F.thisG[index] = g;
  }
  F.thisDirectResv[index] = resv;
  F.thisLightId[index] = lid;
  flushCounters(F, c);
}

__global__ __launch_bounds__(64) void k_direct_reuse(DevScene S, DevFrame F, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  if(px.x >= st.size.x || px.y >= rowEnd) return;
  Ctx c(S, st, cam, nullptr);
  c.imageCoords = px;
  const int index = px.y * st.size.x + px.x;
  c.seed = tea(uint32_t(index + st.size.x * st.size.y), st.time);  // direct_reuse.comp:109
  const Ray ray = c.raySpawn(px, i2{st.size.x, st.size.y});
  GState state; float depth;
  if(!stateFromGBuffer(F.thisG[index], ray, state, depth)) { storeImg(F.thisDirectResult, F, px, mk4(0, 0, 0, 0)); return; }
  f3 direct = mk3(0.0f);
  rt_direct_reservoir resv = F.thisDirectResv[index];
  uint32_t lid = F.thisLightId[index];
  const rt_light_sample ls = resv.lightSample;  // captured before the merge (direct_reuse.comp:124)
  const i2 motionIdx = loadMotion(F, px);
  if(st.ReSTIRState == RT_RESTIR_TEMPORAL || st.ReSTIRState == RT_RESTIR_SPATIOTEMPORAL) {
    const float reprojDepth = length(mk3(cam.lastPosition) - state.position);
    rt_direct_reservoir temporal; uint32_t tlid = 0xffffffffu;
    if(findTemporalNeighborDirect(F, st, state.normal, reprojDepth, state.matID, motionIdx, temporal, tlid)) {
      if(!resvInvalidW(temporal.weight)) { if(resvMerge(resv, temporal, rnd(c.seed))) lid = tlid; }
    }
  }
  if(!resvInvalidW(resv.weight)) direct = mk3(ls.Li);  // :143
  resvClamp(resv, st.RISSampleNum * st.reservoirClamp);
  if(resvInvalidW(resv.weight)) { resv.num = 0; resv.weight = 0.f; }
  if(rt_isnan(direct.x) || rt_isnan(direct.y) || rt_isnan(direct.z)) direct = mk3(0.0f);
  F.thisDirectResv[index] = resv;
  F.thisLightId[index] = lid;
  storeImg(F.thisDirectResult, F, px, mk4(HDRToLDR(c.clampRadiance(direct)), 1.0f));
}

#endif  // !RT_LAT && !RT_OM && !RT_VM && !RT_REPLAY

#if !RT_REPLAY   // (to the end of k_indirect_stage: the replay builds hold the first half of the direct stage only)
// ------------------------------------------------------------------------------------------------------------
// indirect_stage.comp
// ------------------------------------------------------------------------------------------------------------
// ReSTIRIndirect, indirect_stage.comp:228-268 (+ findTemporalNeighbor :74-108): temporal lookup, reservoir update, shading
// of the half-resolution pixel.  Shared by the generic indirect kernel body and the multi-tile single-bounce body.
RT_DEV void restirIndirectFinish(Ctx& c, const DevFrame& F RT_OM_PARAM, const rt_state& st, const rt_scene_camera& cam, i2 px, i2 indSize, const GState& primState, f3 primWo,
                                 rt_gi_sample gi, float primSamplePdf)
{
  f3 indirect = mk3(0.0f);
  rt_indirect_reservoir resv;
  resv.giSample.L = rt_vec3{0, 0, 0}; resv.giSample.xv = rt_vec3{0, 0, 0}; resv.giSample.nv = rt_vec3{0, 0, 0};
  resv.giSample.xs = rt_vec3{0, 0, 0}; resv.giSample.ns = rt_vec3{0, 0, 0}; resv.giSample.pHat = 0.f;
  resv.num = 0; resv.weight = 0.f; resv.bigW = 0.f;
  if(st.ReSTIRState == RT_RESTIR_TEMPORAL || st.ReSTIRState == RT_RESTIR_SPATIOTEMPORAL) {
#if RT_OM
    const float reprojDepth = length(omLastPosition(OM, cam, OM.instImage[size_t(px.y * 2) * F.W + px.x * 2]) - primState.position);
#elif RT_VM
    const float4 dv = gLoadF4(OM.delta + (size_t(px.y * 2) * F.W + px.x * 2));
    const float reprojDepth = length(mk3(cam.lastPosition) - (primState.position + mk3(dv.x, dv.y, dv.z)));
#else
    const float reprojDepth = length(mk3(cam.lastPosition) - primState.position);
#endif
    const i2 motionIdx = loadMotion(F, i2{px.x * 2, px.y * 2});
    if(motionIdx.x >= 0 && motionIdx.x < F.W && motionIdx.y >= 0 && motionIdx.y < F.H && (motionIdx.y < F.histRow0 || motionIdx.y >= F.histRow1)) *F.histMiss = 1u;
    const uint4 lg = loadG(F.lastG, F, motionIdx);
    const f3 pnorm = decompress_unit_vec(lg.y);
    const float pdepth = rt_u2f(lg.x);
    const uint32_t matHash = lg.w & 0xFF000000u;
    const i2 coord{motionIdx.x / 2, motionIdx.y / 2};
    if(inBound(coord, indSize)) {
      if(hash8bit(primState.matID) == matHash) {
        if(dot(primState.ffnormal, pnorm) > 0.5f && reprojDepth < pdepth * 1.1f) resv = F.lastIndirectResv[size_t(coord.y) * indSize.x + coord.x];
      }
    }
  }
  float sampleWeight = 0.0f;
  if(GISampleValid(gi)) {
    gi.pHat = resvToScalar(mk3(gi.L));  // pHatIndirect :61-66
    sampleWeight = gi.pHat / primSamplePdf;
    if(rt_isnan(sampleWeight) || sampleWeight < 0.0f) sampleWeight = 0.0f;
  }
  {  // resvUpdate :54-60
    const float rr = rnd(c.seed);
    resv.weight += sampleWeight; resv.num += 1;
    if(rr * resv.weight < sampleWeight) resv.giSample = gi;
  }
  if(resvInvalidW(resv.weight)) { resv.num = 0; resv.weight = 0.f; resv.bigW = 0.f; }
  resvClamp(resv, st.reservoirClamp * 2);
  F.thisIndirectResv[size_t(px.y) * indSize.x + px.x] = resv;  // saveNewReservoir

  gi = resv.giSample;
  if(!resvInvalidW(resv.weight) && GISampleValid(gi)) {
    const f3 primWi = normalize(mk3(gi.xs) - mk3(gi.xv));
    Material pm = primState.mat;
    pm.albedo = mk3(1.0f);
    const float bigW = resv.weight / (resvToScalar(mk3(resv.giSample.L)) * float(resv.num));  // bigWIndirect :68-70
    indirect = mk3(gi.L) * metallicWorkflowBSDF(pm, mk3(gi.nv), primWo, primWi) * satDot(mk3(gi.nv), primWi) * bigW;
  }
  f3 pixelColor = HDRToLDR(c.clampRadiance(indirect));
  pixelColor = c.clampRadiance(pixelColor);
  storeImg(F.denoiseIndA, F, px, mk4(pixelColor, 1.0f));
}

#if !RT_LAT
// ---- single-bounce tiles, K tiles per wave ----------------------------------------------------------------------------------
// 75 % of the tiles stop after one bounce + one NEE shadow ray (TILED_MULTIBOUNCE, :283-288): per path one closest-hit ray,
// then at most one any-hit ray.  With one tile per wave the ray pool holds fewer rays than the wave has lanes (sky pixels,
// paths that left the scene), and every lane then waits for the slowest ray: 77 % of the lane-rounds of these tiles were
// idle.  Here a wave owns K such tiles; what a path carries between its three phases is small (seed, pdf, direction /
// hit point, normal, pending NEE term), so K paths per lane stay in registers, both traces run over a pool of up to 64 K
// rays, and lanes pull rays until the pool is dry.  Same arithmetic, same RNG draw order per path as the generic body.
template <int K>
RT_DEV void indirectSingleBounceTiles(const DevScene& S, const DevFrame& F RT_OM_PARAM, const rt_state& st, const rt_scene_camera& cam, int rowBegin, int rowEnd, int tilesX,
                                      const uint32_t* tiles /* K entries */, int nTilesHere, uint2* s_stack)
{
  const int lane = int(threadIdx.x);
  const i2 indSize{st.size.x / 2, st.size.y / 2};
  float4* pool = reinterpret_cast<float4*>(s_stack + size_t(S.stackEntries) * 64);
#if RT_WAVEPROF
  const uint64_t prof_c0 = clock64(), prof_w0 = wall_clock64();
#endif
  Ctx c(S, st, cam, s_stack + lane);
  struct Path { i2 px; uint32_t seed; float primSamplePdf; f3 a, b, pend; bool hasSurface, nvSet, shadow; };
  // a: sampleWi between phase 0 and 1, gi.xs afterwards; b: gi.ns; pend: the NEE term waiting for its visibility
  Path P[K];
  uint32_t have = 0;
  // ---- phase 0: G-buffer decode, BSDF sample, park the bounce ray (depth 1 of pathTraceIndirect, :129-226) ---------------------
#pragma unroll
  for(int k = 0; k < K; k++) {
    Path& p = P[k];
    p.hasSurface = false; p.nvSet = false; p.shadow = false; p.primSamplePdf = 0.0f; p.a = mk3(0.0f); p.b = mk3(0.0f); p.pend = mk3(0.0f);
    const int t = int(tiles[k < nTilesHere ? k : 0]);
    const int ty = t / tilesX, tx = t - ty * tilesX;
    p.px = i2{tx * 8 + (lane & 7), rowBegin + ty * 8 + (lane >> 3)};
    p.seed = tea(uint32_t(indSize.x) * uint32_t(p.px.y) + uint32_t(p.px.x), st.time);  // :280
    if(lane == 0) (void)rnd(p.seed);  // invocation 0 drew the tile flag from its own stream (:283-288); the flag is known here
    const bool inImage = k < nTilesHere && !(p.px.x >= indSize.x || p.px.y >= indSize.y || p.px.y >= rowEnd);
    if(!inImage) continue;
    const Ray ray = c.raySpawn(p.px, indSize);
    GState g0; float depth;
    if(!stateFromGBuffer(loadG(F.thisG, F, i2{p.px.x * 2, p.px.y * 2}), ray, g0, depth)) { storeImg(F.denoiseIndA, F, p.px, mk4(0, 0, 0, 0)); continue; }
    p.hasSurface = true;
    g0.position += g0.ffnormal * 2e-2f;  // :299
    Material m = g0.mat; m.albedo = mk3(1.0f);
    if(st.maxDepth < 1) continue;
    c.seed = p.seed;
    f3 wi = mk3(0.0f); float pdf = 0.0f;
    (void)c.Sample(m, -ray.direction, g0.ffnormal, wi, pdf);
    p.seed = c.seed;
    if(Ctx::IsPdfInvalid(pdf)) continue;
    p.primSamplePdf = pdf; p.nvSet = true; p.a = wi;
    c.nClosest++;
    poolPut(pool, k * 64 + lane, OffsetRay(g0.position, g0.ffnormal), wi, RT_INFINITY, p.seed);
    have |= 1u << k;
  }
  tracePoolTiles<K, false>(S, pool, have, c.stack, c.tc);
  // ---- phase 1: the hit; NEE sample of depth 2 -> shadow ray; the BSDF sample depth 2 draws before it stops (:169-176) ------
  uint32_t haveS = 0;
#pragma unroll
  for(int k = 0; k < K; k++) {
    Path& p = P[k];
    if(!((have >> k) & 1u)) continue;
    const f3 wi = p.a;
    c.hit = poolGet(pool, k * 64 + lane);
    const Ray ray0 = c.raySpawn(p.px, indSize);
    GState g0; float depth;
    stateFromGBuffer(loadG(F.thisG, F, i2{p.px.x * 2, p.px.y * 2}), ray0, g0, depth);
    g0.position += g0.ffnormal * 2e-2f;
    if(c.hit.t >= RT_INFINITY - 1e-4f) {  // :183-195, depth 1
      p.a = g0.position + wi * RT_INFINITY * 0.8f; p.b = -wi;
      continue;
    }
    const Ray ray{OffsetRay(g0.position, g0.ffnormal), wi};
    State state = c.GetState(ray.direction);
    c.GetMaterials(state, ray);
    p.a = state.position; p.b = state.ffnormal;  // gi.xs / gi.ns, emitter or not (:197-215)
    if(state.isEmitter || st.maxDepth < 2) continue;
    c.seed = p.seed;
    const f3 wo = -ray.direction;
    if(st.MIS > 0) {  // SampleDirectLight (pathtrace.glsl:185-203) minus its visibility test; throughput is 1 in these tiles
      rt_light_sample ls;
      const float lightPdf = c.SampleDirectLightNoVisibility(state.position, ls);
      if(!Ctx::IsPdfInvalid(lightPdf)) {
        const f3 lwi = mk3(ls.wi);
        const f3 so = OffsetRay(state.position, state.ffnormal);
        const float maxDist = ((ls.dist - rt_abs(so.x - state.position.x)) - rt_abs(so.y - state.position.y)) - rt_abs(so.z - state.position.z);  // Occlusion :18-22
        c.nAny++;
        poolPut(pool, k * 64 + lane, so, lwi, maxDist, c.seed);
        haveS |= 1u << k; p.shadow = true;
        const float BSDFPdf = metallicWorkflowPdf(state.mat, state.ffnormal, wo, lwi);
        const float weight = MISw(st, lightPdf, BSDFPdf);
        p.pend = mk3(ls.Li) * metallicWorkflowBSDF(state.mat, state.ffnormal, wo, lwi) * absDot(state.ffnormal, lwi) * mk3(1.0f) / lightPdf * weight;
      }
    }
    f3 w2 = mk3(0.0f); float pdf2 = 0.0f;
    (void)c.Sample(state.mat, wo, state.ffnormal, w2, pdf2);  // depth 2 samples the BSDF, then `if(!multiBounce) break`
    p.seed = c.seed;
  }
  // (slots of the bounce rays were read above; the shadow rays reuse them)
  tracePoolTiles<K, true>(S, pool, haveS, c.stack, c.tc);
  // ---- phase 2: visibility of the NEE term, then ReSTIRIndirect ------------------------------------------------------------------
#pragma unroll
  for(int k = 0; k < K; k++) {
    Path& p = P[k];
    if(!p.hasSurface) continue;
    rt_gi_sample gi = newGISample();
    const Ray ray0 = c.raySpawn(p.px, indSize);
    GState primState; float depth;
    stateFromGBuffer(loadG(F.thisG, F, i2{p.px.x * 2, p.px.y * 2}), ray0, primState, depth);
    primState.position += primState.ffnormal * 2e-2f;
    if(p.nvSet) { gi.xv = toR(primState.position); gi.nv = toR(primState.ffnormal); gi.xs = toR(p.a); gi.ns = toR(p.b); }
    if(p.shadow && poolGet(pool, k * 64 + lane).gid == 0xffffffffu) gi.L = toR(mk3(gi.L) + p.pend);  // not occluded
    c.seed = p.seed;
    c.imageCoords = p.px;
    restirIndirectFinish(c, F RT_OM_ARG, st, cam, p.px, indSize, primState, -ray0.direction, gi, p.primSamplePdf);
  }
#if RT_WAVEPROF
  // (round 5: the K-tile waves were missing from the profile — 75 % of the stage's tiles; their record is keyed by the first tile, bit 17 marks the kind)
  { const int t0 = int(tiles[0]); waveProfFlush(F, c, (t0 % tilesX) | 0x20000, t0 / tilesX, prof_c0, prof_w0); }
#endif
  flushCounters(F, c);
}

#endif  // !RT_LAT

// 5 waves/SIMD (96 VGPRs, a few more spills) instead of 4: the stage alone is no faster, but with frames in flight its waves
// share the SIMDs with the next frame's direct stage and the frame is 2.7 % shorter (3, 4, 6 measured: 3.96 / 3.47 / 3.42 vs 3.37 ms)
#ifndef RT_INDIRECT_LB
#define RT_INDIRECT_LB 5
#endif
#if RT_LAT
// latency build: a workgroup of NW waves per half-res tile; wave 0 runs the paths of the 64 pixels (the body below), the other waves only serve the
// workgroup's ray pool: after every path vertex wave 0 lists the vertex's rays, all waves trace them eight lanes per ray, wave 0 goes on shading
// (4 waves per SIMD = 128 VGPRs: two of these workgroups per CU, and beside one of them two direct-stage waves per SIMD — with 165 registers the next
//  frame's direct stage, which runs beside this kernel when frames are in flight, had one wave slot per SIMD left: profiles/r03_mgpu_period_ab.txt)
__global__ __launch_bounds__(512, 4) void k_indirect_stage(DevScene S, DevFrame F RT_OM_KPARAM, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY, int cap,
                                                       const uint32_t* lists, uint32_t* counts, int subShift, int sbK, int genericBlocks)
#else
__global__ __launch_bounds__(64, RT_INDIRECT_LB) void k_indirect_stage(DevScene S, DevFrame F RT_OM_KPARAM, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY, int cap,
                                                          const uint32_t* lists, uint32_t* counts, int subShift, int sbK, int genericBlocks)
#endif
{
  // subShift > 0 (small launches: row bands of a multi-GPU frame, small images): a tile is split over 2 or 4 waves that own
  // 32 / 16 of its pixels each; the other lanes of each wave have no path and only serve the wave's ray pool.  With fewer
  // paths per wave the majority-vote loop runs fewer rounds per ray, and the idle SIMDs of an under-filled chip get work:
  // the latency of the longest multi-bounce tile — the floor of a small launch — drops.  Results do not change.
  extern __shared__ uint2 s_stack[];
#if RT_WAVEPROF
  const uint64_t prof_c0 = clock64(), prof_w0 = wall_clock64();
#endif
  TileCoord tile;
  const int part = (int(blockIdx.x) >> 3) & ((1 << subShift) - 1);
  {
    const int L = int(blockIdx.x), xcd = L & 7;
    const int nf = int(counts[xcd * 2]), nb = int(counts[xcd * 2 + 1]);
#if !RT_LAT
    if(sbK > 0 && L >= genericBlocks) {  // single-bounce tiles of this XCD, sbK per wave (from the back of its list)
      const int w = (L - genericBlocks) >> 3, first = w * sbK;
      if(first >= nb) return;
      uint32_t t[3] = {0u, 0u, 0u};
      const int n = min(sbK, nb - first);
      for(int k = 0; k < n; k++) t[k] = lists[size_t(xcd) * cap + (cap - 1 - (first + k))];
      if(sbK == 3) indirectSingleBounceTiles<3>(S, F RT_OM_ARG, st, cam, rowBegin, rowEnd, tilesX, t, n, s_stack);
      else indirectSingleBounceTiles<2>(S, F RT_OM_ARG, st, cam, rowBegin, rowEnd, tilesX, t, n, s_stack);  // (4 per wave was measured: slower, spills)
      return;
    }
#endif
    const int k = (L >> 3) >> subShift;
    tile.valid = sbK > 0 ? (k < nf) : (k < nf + nb);
    const uint32_t t = tile.valid ? lists[size_t(xcd) * cap + (k < nf ? k : cap - 1 - (k - nf))] : 0u;
    tile.y = int(t) / tilesX; tile.x = int(t) - tile.y * tilesX;
  }
  if(!tile.valid) return;
#if RT_LAT
  const WideLds WL = wideLds(s_stack, S.stackEntries, int(blockDim.x) >> 6);
  if((int(threadIdx.x) >> 6) != 0) {   // helper waves: trace whatever wave 0 lists until it says it is done
    TravCounters htc{};
    for(;;) {
      __syncthreads();
      if(WL.ctrl[2] != 0u) break;
      tracePoolWide<false>(S, WL.pool, WL.list, int(WL.ctrl[0]), &WL.ctrl[1], WL.stacks + size_t(int(threadIdx.x) >> 6) * wideWaveStride(S.stackEntries), htc);
      __syncthreads();
    }
    return;
  }
#endif
  const int lane = int(threadIdx.x);
  const i2 indSize{st.size.x / 2, st.size.y / 2};
  const int rowsPerPart = 8 >> subShift;
  const bool hasPixel = (lane >> 3) < rowsPerPart;
  const i2 px{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + part * rowsPerPart + (lane >> 3)};
#if RT_LAT
  Ctx c(S, st, cam, nullptr);
#else
  Ctx c(S, st, cam, s_stack + lane);
#endif
  c.imageCoords = px;
  c.seed = tea(uint32_t(indSize.x) * uint32_t(px.y) + uint32_t(px.x), st.time);  // :280
  // TILED_MULTIBOUNCE (:283-288): invocation 0 of the workgroup draws the tile flag from its own stream (and so advances
  // it); the flag is wave-uniform here, so it costs one readfirstlane instead of shared memory + barrier.  Waves that own
  // another part of the tile recompute the flag from a copy of that pixel's stream.
  int mb = 0;
  if(lane == 0) {
    if(part == 0) mb = rnd(c.seed) < 0.25f ? 1 : 0;
    else { uint32_t s0 = tea(uint32_t(indSize.x) * uint32_t(rowBegin + tile.y * 8) + uint32_t(tile.x * 8), st.time); mb = rnd(s0) < 0.25f ? 1 : 0; }
  }
  const bool multiBounce = __builtin_amdgcn_readfirstlane(mb) != 0;
  // Lanes without a pixel / without a surface stay in the kernel: they trace rays of the other lanes (tracePool).
#if RT_LAT
  float4* pool = WL.pool;
#else
  float4* pool = reinterpret_cast<float4*>(s_stack + size_t(S.stackEntries) * 64);
#endif
  const bool inImage = hasPixel && !(px.x >= indSize.x || px.y >= indSize.y || px.y >= rowEnd);
  Ray ray = c.raySpawn(px, indSize);

  GState g0; float depth;
  bool alive = inImage && stateFromGBuffer(loadG(F.thisG, F, i2{px.x * 2, px.y * 2}), ray, g0, depth);
  const bool hasSurface = alive;
  if(inImage && !hasSurface) storeImg(F.denoiseIndA, F, px, mk4(0, 0, 0, 0));
  if(!alive) { g0 = GState{}; }
  g0.position += g0.ffnormal * 2e-2f;  // :299

  // ---- pathTraceIndirect, :129-226 --------------------------------------------------------------------------
  // Per path vertex the reference traces the NEE shadow ray, then samples the BSDF and traces the bounce ray.  Neither
  // trace advances prd.seed here (DESIGN.md deviation 1), so both rays of a vertex are known before either is traced:
  // they go to the wave's ray pool together, and the results are applied in the reference's order afterwards.
  f3 throughput = mk3(multiBounce ? 4.0f : 1.0f);
  const f3 primWo = -ray.direction;
  const GState primState = g0;
  rt_gi_sample gi = newGISample();
  float primSamplePdf = 0.0f;
  State state = zeroState();
  state.position = g0.position; state.normal = g0.normal; state.ffnormal = g0.ffnormal; state.mat = g0.mat; state.matID = g0.matID;
  state.mat.albedo = mk3(1.0f);
  for(int depthI = 1; depthI <= st.maxDepth; depthI++) {
    bool hasShadow = false, hasBounce = false;
    f3 pendingAdd = mk3(0.0f), sampleWi = mk3(0.0f);
    float samplePdf = 0.0f;
    if(alive) {
      const f3 wo = -ray.direction;
      if(depthI > 1 && st.MIS > 0) {  // SampleDirectLight (pathtrace.glsl:185-203) minus its visibility test
        rt_light_sample ls;
        const float lightPdf = c.SampleDirectLightNoVisibility(state.position, ls);
        if(!Ctx::IsPdfInvalid(lightPdf)) {
          const f3 wi = mk3(ls.wi);
          const f3 so = OffsetRay(state.position, state.ffnormal);
          const float maxDist = ((ls.dist - rt_abs(so.x - state.position.x)) - rt_abs(so.y - state.position.y)) - rt_abs(so.z - state.position.z);  // Occlusion :18-22
          c.nAny++;
          poolPut(pool, lane * 2 + 1, so, wi, maxDist, c.seed);
          hasShadow = true;
          const float BSDFPdf = metallicWorkflowPdf(state.mat, state.ffnormal, wo, wi);
          const float weight = MISw(st, lightPdf, BSDFPdf);
          pendingAdd = mk3(ls.Li) * metallicWorkflowBSDF(state.mat, state.ffnormal, wo, wi) * absDot(state.ffnormal, wi) * throughput / lightPdf * weight;
        }
      }
      const f3 sampleBSDF = c.Sample(state.mat, wo, state.ffnormal, sampleWi, samplePdf);
      if(Ctx::IsPdfInvalid(samplePdf)) alive = false;
      else if(depthI > 1 && !multiBounce) alive = false;
      else {
        if(depthI > 1) throughput *= sampleBSDF / samplePdf * absDot(state.ffnormal, sampleWi);
        else {
          primSamplePdf = samplePdf;
          gi.xv = toR(state.position);
          gi.nv = toR(state.ffnormal);
        }
        ray.origin = OffsetRay(state.position, state.ffnormal);
        ray.direction = sampleWi;
        c.nClosest++;
        poolPut(pool, lane * 2, ray.origin, ray.direction, RT_INFINITY, c.seed);
        hasBounce = true;
      }
    }
    if(__ballot((hasShadow || hasBounce) ? 1 : 0) == 0ull) break;  // wave-uniform
#if RT_LAT
    poolPublish(WL, hasBounce, hasShadow);
#if RT_WAVEPROF
    { const uint64_t g0 = clock64(); groupTrace<false>(S, WL, c.tc); c.cycClosest += uint32_t(clock64() - g0); c.cycAny++; }   // [3] cycles in the pool traces, [4] their number
#else
    groupTrace<false>(S, WL, c.tc);
#endif
#else
    tracePool(S, pool, hasBounce, hasShadow, c.stack, c.tc);
#endif
    if(hasShadow && poolGet(pool, lane * 2 + 1).gid == 0xffffffffu) gi.L = toR(mk3(gi.L) + pendingAdd);  // not occluded
    if(hasBounce) {
      c.hit = poolGet(pool, lane * 2);
      if(c.hit.t >= RT_INFINITY - 1e-4f) {
        if(depthI > 1) {
          float lightPdf;
          const f3 Li = c.EnvEval(sampleWi, lightPdf);
          const float weight = MISw(st, samplePdf, lightPdf);
          gi.L = toR(mk3(gi.L) + Li * throughput * weight);
        } else {
          gi.xs = toR(state.position + sampleWi * RT_INFINITY * 0.8f);
          gi.ns = toR(-sampleWi);
        }
        alive = false;
      } else {
        state = c.GetState(ray.direction);
        c.GetMaterials(state, ray);
        if(state.isEmitter) {
          if(depthI > 1) {
            float lightPdf;
            const f3 Li = c.LightEval(state, c.hit.t, sampleWi, lightPdf);
            const float weight = MISw(st, samplePdf, lightPdf);
            gi.L = toR(mk3(gi.L) + Li * throughput * weight);
          } else {
            gi.xs = toR(state.position);
            gi.ns = toR(state.ffnormal);
          }
          alive = false;
        } else if(depthI == 1) { gi.xs = toR(state.position); gi.ns = toR(state.ffnormal); }
      }
    }
    // Russian roulette (:218-224) is compiled out in the reference (`#ifndef RR`, pathtrace.glsl:2)
  }
#if RT_LAT
  if(lane == 0) WL.ctrl[2] = 1u;   // release the helper waves
  __syncthreads();
#endif
#if RT_WAVEPROF
  waveProfFlush(F, c, tile.x | (multiBounce ? 0x10000 : 0), tile.y, prof_c0, prof_w0);
#endif
  if(!hasSurface) { flushCounters(F, c); return; }

  restirIndirectFinish(c, F RT_OM_ARG, st, cam, px, indSize, primState, primWo, gi, primSamplePdf);
  flushCounters(F, c);
}

#endif  // !RT_REPLAY

// ------------------------------------------------------------------------------------------------------------
// host-side launch (one entry of Renderer::run's dispatch list, renderer.cpp:163-205)
// ------------------------------------------------------------------------------------------------------------
// One signature for every build (stages.h); of `X` a build reads the one pointer that its kernels take by value: RT_OM om, RT_VM vm, RT_REPLAY vis.
hipError_t launchStage(hipStream_t stream, const DevScene& Sin, const DevFrame& F, const StageExtra& X, const rt_state& st, const rt_scene_camera& cam, int stage, int level,
                       int rowBegin, int rowEnd)
{
#if RT_OM
  const DevObjMotion& OM = *X.om;
#elif RT_VM
  const DevVtxMotion& OM = *X.vm;
#elif RT_REPLAY
  const DevVis& V = *X.vis;
  if(stage != RT_STAGE_DIRECT) return hipErrorInvalidValue;   // the build holds k_direct_stage alone
#endif
  DevScene S = Sin;
#if RT_LAT
  S.stackEntries = S.stackTotal + (S.gangMax > 0 ? GANG_EXTRA : 0);   // one column per RAY (8 per wave): the whole stack fits in LDS (+ the room gang mode expands into)
  const int nWaves = 8;   // waves per tile workgroup of the latency kernels (3 / 4 / 6 measured: slower, profiles/r03_band_chunk_ab.txt)
#else
  S.stackEntries = F.stackLds > 0 ? std::min(F.stackLds, S.stackTotal) : S.stackTotal;   // LDS part of the traversal stack for this launch
#endif
  if(stage == RT_STAGE_INDIRECT) S.stackOvf = Sin.stackOvfInd;   // a direct-kind kernel of the next frame can be in flight beside it
  const bool needOvf = S.stackTotal > S.stackEntries;
  const bool half = stage == RT_STAGE_INDIRECT;
  const int gw = half ? st.size.x / 2 : st.size.x, gh = half ? st.size.y / 2 : st.size.y;
  if(rowEnd <= 0 || rowEnd > gh) rowEnd = gh;
  if(rowBegin < 0) rowBegin = 0;
  if(rowBegin >= rowEnd || gw <= 0) return hipSuccess;
  const int tilesX = (gw + 7) / 8, tilesY = (rowEnd - rowBegin + 7) / 8;
  const dim3 grid(tileGrid(tilesX, tilesY)), block(64);
  const size_t lds = size_t(S.stackEntries) * 64 * sizeof(uint2);
  const bool spatial = st.ReSTIRState == RT_RESTIR_SPATIAL || st.ReSTIRState == RT_RESTIR_SPATIOTEMPORAL;
  switch(stage) {
    case RT_STAGE_DIRECT:
      // (a K-tiles-per-wave variant of this kernel — primary and shadow rays through the LDS ray pool, pixel state in the scratch
      //  records between the traces — was measured: 1.77 -> 2.6 ms; the coherent primary rays gain nothing from the pool and the
      //  split shading costs more than the shorter tail saves.  The single-bounce indirect tiles are where pooling pays.)
      // `level` selects the halves of the stage for hosts that must exchange the cached reservoirs of neighbouring rows in between
      // (row-tiled multi-GPU frames with spatial reuse): 0 = the whole stage, 1 = k_direct_stage only, 2 = k_direct_spatial only
      if(level < 0 || level > 2 || (level != 0 && !spatial)) return hipErrorInvalidValue;
#if RT_LAT
      if(level != 2) hipLaunchKernelGGL(k_direct_stage, grid, dim3(64 * nWaves), wideLdsBytes(S.stackEntries, nWaves), stream, S, F RT_OM_ARG, st, cam, rowBegin, rowEnd, tilesX, tilesY);
#elif RT_REPLAY
      if(!V.det || !V.count || !V.list || rowBegin != 0 || rowEnd != gh) return hipErrorInvalidValue;   // full frames only: the planes are indexed by pixel
      if(needOvf && grid.x * 64u > S.stackOvfThreads) return hipErrorInvalidConfiguration;
      if(level != 2) {
        if(V.record) hipLaunchKernelGGL(k_direct_stage<true>, grid, block, lds, stream, S, F, V, st, cam, rowBegin, rowEnd, tilesX, tilesY);
        else hipLaunchKernelGGL(k_direct_stage<false>, grid, block, lds, stream, S, F, V, st, cam, rowBegin, rowEnd, tilesX, tilesY);
      }
#else
      if(needOvf && grid.x * 64u > S.stackOvfThreads) return hipErrorInvalidConfiguration;   // overflow area missing / too small: an internal sizing error, not the caller's
      if(level != 2) hipLaunchKernelGGL(k_direct_stage, grid, block, lds, stream, S, F RT_OM_ARG, st, cam, rowBegin, rowEnd, tilesX, tilesY);
#endif
      // the rayless half (spatial modes): the plain build's kernel
#ifdef RT_FORWARD
      if(level != 1 && spatial) return rt::RT_FORWARD::launchStage(stream, Sin, F, X, st, cam, stage, 2, rowBegin, rowEnd);
#else
      if(level != 1 && spatial) hipLaunchKernelGGL(k_direct_spatial, grid, block, 0, stream, S, F, st, cam, rowBegin, rowEnd, tilesX, tilesY);
#endif
      break;
#if !RT_REPLAY
    case RT_STAGE_INDIRECT: {
      // per-XCD tile lists: capacity = the tiles one XCD can own under the striped mapping
      const int cap = int(tileGrid(tilesX, tilesY) / 8);
      (void)launchIndTileOrder(stream, st, rowBegin, tilesX, tilesY, cap, F.tileOrder, F.qcount + 192);   // filters.hip: longest tiles first
#if RT_LAT
      // one workgroup per tile, multi-bounce tiles first (same lists)
      hipLaunchKernelGGL(k_indirect_stage, grid, dim3(64 * nWaves), wideLdsBytes(S.stackEntries, nWaves), stream, S, F RT_OM_ARG, st, cam, rowBegin, rowEnd, tilesX, tilesY, cap,
                         (const uint32_t*)F.tileOrder, F.qcount + 192, 0, 0, int(grid.x));
#else
      // under ~2 waves per SIMD (1024 SIMDs) the launch is latency bound: split tiles over more waves
      static const int subEnv = getenv("RESTIR_IND_SUB") ? atoi(getenv("RESTIR_IND_SUB")) : -1;
      const int nTiles = tilesX * tilesY;
      const int subShift = subEnv >= 0 ? subEnv : (nTiles <= 1536 ? 2 : (nTiles <= 3072 ? 1 : 0));
      // throughput-bound launches: single-bounce tiles go K per wave (indirectSingleBounceTiles; 3 per wave: fewer wave instructions than 2, frames
      // in flight -1.3 %, the stage alone +4 %); latency-bound ones keep one (part of a) tile per wave
      const int sbK = subShift > 0 ? 0 : 3;
      const unsigned genericBlocks = grid.x << subShift;
      const unsigned sbBlocks = sbK > 0 ? 8u * unsigned((cap + sbK - 1) / sbK) : 0u;
      const size_t poolBytes = std::max<size_t>(POOL_BYTES, size_t(sbK) * 64 * 33);
      if(needOvf && (genericBlocks + sbBlocks) * 64u > S.stackOvfThreads) return hipErrorInvalidConfiguration;
      hipLaunchKernelGGL(k_indirect_stage, dim3(genericBlocks + sbBlocks), block, lds + poolBytes, stream, S, F RT_OM_ARG, st, cam, rowBegin, rowEnd, tilesX, tilesY, cap,
                         (const uint32_t*)F.tileOrder, F.qcount + 192, subShift, sbK, int(genericBlocks));
#endif
      break;
    }
#endif
#if !RT_LAT && !RT_OM && !RT_VM && !RT_REPLAY   // the two stages the reference compiles but does not dispatch: throughput builds only
    case RT_STAGE_DIRECT_GEN:
      if(needOvf && grid.x * 64u > S.stackOvfThreads) return hipErrorInvalidConfiguration;   // overflow area missing / too small: an internal sizing error, not the caller's
      hipLaunchKernelGGL(k_direct_gen, grid, block, lds, stream, S, F, st, cam, rowBegin, rowEnd, tilesX, tilesY);
      break;
    case RT_STAGE_DIRECT_REUSE: hipLaunchKernelGGL(k_direct_reuse, grid, block, 0, stream, S, F, st, cam, rowBegin, rowEnd, tilesX, tilesY); break;
#endif
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace RT_VARIANT
}  // namespace rt

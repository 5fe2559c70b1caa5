// reference.hip — the progressive ground-truth path tracer behind rt_reference_render.
//
//   k_reference        one sample of the integral the real-time frame approximates, for every pixel of a row band, added to fp64 sums
//   k_reference_mean   float(sum / n) of one component -> RGBA32F (readback, tonemap)
//
// Per sample and pixel (include/rt_abi.h states the contract):
//   primary ray     Ctx::raySpawn — the pipeline's ray (direct_stage.comp:279-281), no extra jitter
//   miss            direct = EnvRadiance(dir)
//   emitter         direct = emission, the path ends (direct_stage.comp:172-174)
//   vertex 1        direct = emission + ONE SampleDirectLight sample with its shadow ray, weight 1, BSDF with the material's real albedo
//   vertices 2..    pathTraceIndirect's integrand (indirect_stage.comp:129-226): NEE with the power heuristic when MIS > 0, BSDF-sampled env / emitter
//                   hits at depth > 1 with their MIS weight; every path multi-bounce, throughput starting at 1, the real albedo at vertex 1
// No firefly clamp, no HDR->LDR encoding, no reservoirs.  Every shading function is Ctx's (shading.h); MISw is stage_common.h's.
// Launch shape: one thread per pixel, an 8x8 tile per wave64, the whole traversal stack in LDS (the serial stages' stack); one sample per launch.
// This file is compiled twice: as is, and with -DRT_SKY=1 (REFERENCE_BUILDS in build.py; the stages' split, see stages.hip).
#ifndef RT_SKY
#define RT_SKY 0
#endif
#define RT_COUNT 0   // the reference mode does not feed rt_get_counters
#include "stage_common.h"
#include "reference.h"

#if RT_SKY
#define RT_REF_NS ref_sky
#else
#define RT_REF_NS ref_base
#endif

namespace rt {
namespace RT_REF_NS {

// One sample of pixel px; c.seed is the sample's seed.  The order of the random draws is the order of the calls below (tests/refpt_checker.cpp restates it).
RT_DEV void referenceSample(Ctx& c, const rt_state& st, i2 px, f3& direct, f3& indirect)
{
  direct = mk3(0.0f); indirect = mk3(0.0f);
  Ray ray = c.raySpawn(px, i2{st.size.x, st.size.y});
  c.ClosestHit(ray);
  if(c.hit.t >= RT_INFINITY) { direct = c.EnvRadiance(ray.direction); return; }
  State state = c.GetState(ray.direction);
  c.GetMaterials(state, ray);
  if(state.isEmitter) { direct = state.mat.emission; return; }
  // vertex 1, the direct stage's integrand without reuse: one light sample, its shadow ray inside SampleDirectLight
  {
    const f3 wo = -ray.direction;
    f3 Li = mk3(0.0f), wi = mk3(0.0f);
    const float pdf = c.SampleDirectLight(state, Li, wi);
    f3 d = mk3(0.0f);
    if(!Ctx::IsPdfInvalid(pdf)) d = Li * metallicWorkflowBSDF(state.mat, state.ffnormal, wo, wi) * rt_max(dot(state.ffnormal, wi), 0.0f) / pdf;
    if(hasNan(d)) d = mk3(0.0f);
    direct = state.mat.emission + d;
  }
  // vertices 2..maxDepth, pathTraceIndirect's integrand; the depth-1 bounce carries the vertex-1 BSDF weight in `throughput`
  f3 throughput = mk3(1.0f);
  for(int depth = 1; depth <= st.maxDepth; depth++) {
    const f3 wo = -ray.direction;
    if(depth > 1 && st.MIS > 0) {
      f3 Li = mk3(0.0f), wi = mk3(0.0f);
      const float lightPdf = c.SampleDirectLight(state, Li, wi);
      if(!Ctx::IsPdfInvalid(lightPdf)) {
        const float BSDFPdf = metallicWorkflowPdf(state.mat, state.ffnormal, wo, wi);
        const float weight = MISw(st, lightPdf, BSDFPdf);
        indirect = indirect + Li * metallicWorkflowBSDF(state.mat, state.ffnormal, wo, wi) * absDot(state.ffnormal, wi) * throughput / lightPdf * weight;
      }
    }
    f3 sampleWi = mk3(0.0f);
    float samplePdf = 0.0f;
    const f3 sampleBSDF = c.Sample(state.mat, wo, state.ffnormal, sampleWi, samplePdf);
    if(Ctx::IsPdfInvalid(samplePdf)) break;
    throughput = throughput * (sampleBSDF / samplePdf * absDot(state.ffnormal, sampleWi));
    ray = Ray{OffsetRay(state.position, state.ffnormal), sampleWi};
    c.ClosestHit(ray);
    if(c.hit.t >= RT_INFINITY - 1e-4f) {
      if(depth > 1) {
        float lightPdf;
        const f3 Li = c.EnvEval(sampleWi, lightPdf);
        indirect = indirect + Li * throughput * MISw(st, samplePdf, lightPdf);
      }
      break;
    }
    state = c.GetState(ray.direction);
    c.GetMaterials(state, ray);
    if(state.isEmitter) {
      if(depth > 1) {
        float lightPdf;
        const f3 Li = c.LightEval(state, c.hit.t, sampleWi, lightPdf);
        indirect = indirect + Li * throughput * MISw(st, samplePdf, lightPdf);
      }
      break;
    }
  }
  if(hasNan(indirect)) indirect = mk3(0.0f);
}

#ifndef RT_REF_LB
#define RT_REF_LB 4
#endif
__global__ __launch_bounds__(64, RT_REF_LB) void k_reference(DevScene S, rt_state st, rt_scene_camera cam, double* acc, uint32_t sample, int rowBegin, int rowEnd, int tilesX)
{
  extern __shared__ uint2 s_stack[];
  const int lane = int(threadIdx.x);
  const int ty = int(blockIdx.x) / tilesX, tx = int(blockIdx.x) - ty * tilesX;
  const i2 px{tx * 8 + (lane & 7), rowBegin + ty * 8 + (lane >> 3)};
  if(px.x >= st.size.x || px.y >= rowEnd) return;
  Ctx c(S, st, cam, s_stack + lane);
  c.imageCoords = px;
  c.seed = tea(uint32_t(st.size.x) * uint32_t(px.y) + uint32_t(px.x), tea(sample, REF_SEED_SALT));
  f3 direct, indirect;
  referenceSample(c, st, px, direct, indirect);
  double* a = acc + (size_t(px.y) * size_t(st.size.x) + size_t(px.x)) * REF_ACC_DOUBLES;
  a[0] += double(direct.x); a[1] += double(direct.y); a[2] += double(direct.z);
  a[3] += double(indirect.x); a[4] += double(indirect.y); a[5] += double(indirect.z);
}

hipError_t launchReference(hipStream_t stream, const DevScene& Sin, const rt_state& st, const rt_scene_camera& cam, double* acc, uint32_t sample, int rowBegin, int rowEnd)
{
  DevScene S = Sin;
  S.stackEntries = S.stackTotal;   // the whole stack in LDS: the overflow areas of the stages are never touched
  const int tilesX = (st.size.x + 7) / 8, tilesY = (rowEnd - rowBegin + 7) / 8;
  if(tilesX <= 0 || tilesY <= 0) return hipSuccess;
  const size_t lds = size_t(S.stackEntries) * 64 * sizeof(uint2);
  hipLaunchKernelGGL(k_reference, dim3(unsigned(tilesX * tilesY)), dim3(64), lds, stream, S, st, cam, acc, sample, rowBegin, rowEnd, tilesX);
  return hipGetLastError();
}

}  // namespace RT_REF_NS

#if !RT_SKY
__global__ __launch_bounds__(256) void k_reference_mean(const double* acc, uint32_t n, int component, size_t pixels, float4* out)
{
  const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
  if(i >= pixels) return;
  if(n == 0u) { out[i] = make_float4(0.f, 0.f, 0.f, 1.f); return; }
  const double* a = acc + i * REF_ACC_DOUBLES;
  const double dn = double(n);
  double r, g, b;
  if(component == 2) { r = (a[0] + a[3]) / dn; g = (a[1] + a[4]) / dn; b = (a[2] + a[5]) / dn; }
  else { const int o = component * 3; r = a[o] / dn; g = a[o + 1] / dn; b = a[o + 2] / dn; }
  out[i] = make_float4(float(r), float(g), float(b), 1.f);
}

hipError_t launchReferenceMean(hipStream_t stream, const double* acc, uint32_t n, int component, size_t pixels, float4* out)
{
  if(pixels == 0) return hipSuccess;
  hipLaunchKernelGGL(k_reference_mean, dim3(unsigned((pixels + 255) / 256)), dim3(256), 0, stream, acc, n, component, pixels, out);
  return hipGetLastError();
}
#endif

}  // namespace rt

// refpt_checker.cpp — CPU restatement of the reference mode (rt_reference_render, csrc/reference.hip) for the tests.
// TEST INFRASTRUCTURE: built by tests/test_reference_cpu.py / tests/test_gpu_reference.py together with oracle/orc_scene.cpp, with the oracle's flags.
// Every shading function is the oracle's (oracle/orc_shading.h); this file restates only the estimator of include/rt_abi.h "Reference mode" — the
// order of the calls, hence of the random draws — and the determinism contract (seed per (x, y, W, s), fp64 sums in sample order, float(sum / n)).
#include "../oracle/orc_shading.h"
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace {
using namespace orc;

constexpr uint32_t REF_SEED_SALT = 0x52454631u;   // csrc/reference.h

float MISw(const rt_state& st, float f, float g) { return (st.MIS > 0) ? powerHeuristic(f, g) : 1.0f; }   // stage_common.h MISw

// one sample of pixel px (csrc/reference.hip referenceSample)
void referenceSample(Shader& c, const rt_state& st, ivec2 px, vec3& direct, vec3& indirect)
{
  direct = V3(0.0f); indirect = V3(0.0f);
  Ray ray = c.raySpawn(px, ivec2{st.size.x, st.size.y});
  c.ClosestHit(ray);
  if(c.hitT >= RT_INFINITY) { direct = c.EnvRadiance(ray.direction); return; }
  State state = c.GetState(ray.direction);
  c.GetMaterials(state, ray);
  if(state.isEmitter) { direct = state.mat.emission; return; }
  {
    const vec3 wo = -ray.direction;
    vec3 Li = V3(0.0f), wi = V3(0.0f);
    const float pdf = c.SampleDirectLight(state, Li, wi);
    vec3 d = V3(0.0f);
    if(!Shader::IsPdfInvalid(pdf)) d = Li * c.BSDF(state, wo, state.ffnormal, wi) * rt_max(dot(state.ffnormal, wi), 0.0f) / pdf;
    if(hasNan(d)) d = V3(0.0f);
    direct = state.mat.emission + d;
  }
  vec3 throughput = V3(1.0f);
  for(int depth = 1; depth <= st.maxDepth; depth++) {
    const vec3 wo = -ray.direction;
    if(depth > 1 && st.MIS > 0) {
      vec3 Li = V3(0.0f), wi = V3(0.0f);
      const float lightPdf = c.SampleDirectLight(state, Li, wi);
      if(!Shader::IsPdfInvalid(lightPdf)) {
        const float BSDFPdf = c.Pdf(state, wo, state.ffnormal, wi);
        const float weight = MISw(st, lightPdf, BSDFPdf);
        indirect = indirect + Li * c.BSDF(state, wo, state.ffnormal, wi) * absDot(state.ffnormal, wi) * throughput / lightPdf * weight;
      }
    }
    vec3 sampleWi = V3(0.0f);
    float samplePdf = 0.0f;
    const vec3 sampleBSDF = c.Sample(state, wo, state.ffnormal, sampleWi, samplePdf);
    if(Shader::IsPdfInvalid(samplePdf)) break;
    throughput = throughput * (sampleBSDF / samplePdf * absDot(state.ffnormal, sampleWi));
    ray = Ray{OffsetRay(state.position, state.ffnormal), sampleWi};
    c.ClosestHit(ray);
    if(c.hitT >= RT_INFINITY - 1e-4f) {
      if(depth > 1) {
        float lightPdf;
        const vec3 Li = c.EnvEval(sampleWi, lightPdf);
        indirect = indirect + Li * throughput * MISw(st, samplePdf, lightPdf);
      }
      break;
    }
    state = c.GetState(ray.direction);
    c.GetMaterials(state, ray);
    if(state.isEmitter) {
      if(depth > 1) {
        float lightPdf;
        const vec3 Li = c.LightEval(state, c.hitT, sampleWi, lightPdf);
        indirect = indirect + Li * throughput * MISw(st, samplePdf, lightPdf);
      }
      break;
    }
  }
  if(hasNan(indirect)) indirect = V3(0.0f);
}

struct Checker {
  Scene scene;
  rt_scene_camera cam{};
  int W = 0, H = 0;
  uint32_t n = 0;
  std::vector<double> acc;   // 6 per pixel: direct rgb, indirect rgb
  std::atomic<uint64_t> rays{0};   // ClosestHit + AnyHit queries of the last refpt_render
};
}  // namespace

extern "C" {

void* refpt_create(const rt_scene_desc* d)
{
  Checker* k = new Checker();
  k->scene.upload(d);
  k->scene.build();
  return k;
}
void refpt_destroy(void* p) { delete static_cast<Checker*>(p); }
void refpt_set_camera(void* p, const rt_scene_camera* cam) { static_cast<Checker*>(p)->cam = *cam; static_cast<Checker*>(p)->n = 0; }
void refpt_set_sun_and_sky(void* p, const rt_sun_and_sky* ss) { static_cast<Checker*>(p)->scene.sunAndSky = *ss; static_cast<Checker*>(p)->n = 0; }
void refpt_resize(void* p, int w, int h)
{
  Checker* k = static_cast<Checker*>(p);
  k->W = w; k->H = h; k->n = 0;
  k->acc.assign(size_t(w) * h * 6, 0.0);
}
uint64_t refpt_rays(void* p) { return static_cast<Checker*>(p)->rays; }
void refpt_reset(void* p) { static_cast<Checker*>(p)->n = 0; }
uint32_t refpt_samples(void* p) { return static_cast<Checker*>(p)->n; }

// adds `samples` samples per pixel, rows spread over `threads` threads (the result does not depend on it)
int refpt_render(void* p, const rt_state* st, int samples, int threads)
{
  Checker* k = static_cast<Checker*>(p);
  if(samples < 0 || st->size.x != k->W || st->size.y != k->H) return RT_ERR_INVALID_ARG;
  if(k->n == 0) std::fill(k->acc.begin(), k->acc.end(), 0.0);
  const uint32_t n0 = k->n;
  k->rays = 0;
  Counters::local() = Counters::Local{};
  auto rows = [&](int t, int nt) {
    for(int y = t; y < k->H; y += nt)
      for(int x = 0; x < k->W; x++) {
        double* a = &k->acc[(size_t(y) * k->W + x) * 6];
        for(int s = 0; s < samples; s++) {
          Shader c(k->scene, *st, k->cam);
          c.imageCoords = ivec2{x, y};
          c.seed = tea(uint32_t(k->W) * uint32_t(y) + uint32_t(x), tea(n0 + uint32_t(s), REF_SEED_SALT));
          vec3 direct, indirect;
          referenceSample(c, *st, ivec2{x, y}, direct, indirect);
          a[0] += double(direct.x); a[1] += double(direct.y); a[2] += double(direct.z);
          a[3] += double(indirect.x); a[4] += double(indirect.y); a[5] += double(indirect.z);
        }
      }
    Counters::Local& l = Counters::local();
    k->rays += l.closestHitRays + l.anyHitRays;
    l = Counters::Local{};
  };
  const int nt = std::max(1, threads);
  std::vector<std::thread> pool;
  for(int t = 1; t < nt; t++) pool.emplace_back(rows, t, nt);
  rows(0, nt);
  for(std::thread& th : pool) th.join();
  k->n += uint32_t(samples);
  return RT_OK;
}

// RGBA32F mean of component 0 / 1 / 2 (rt_reference_readback): float(sum / n), a = 1; n == 0 gives (0, 0, 0, 1)
int refpt_readback(void* p, int component, float* dst)
{
  Checker* k = static_cast<Checker*>(p);
  if(component < 0 || component > 2) return RT_ERR_INVALID_ARG;
  const size_t np = size_t(k->W) * k->H;
  const double dn = double(k->n);
  for(size_t i = 0; i < np; i++) {
    const double* a = &k->acc[i * 6];
    float* o = dst + 4 * i;
    if(k->n == 0) { o[0] = o[1] = o[2] = 0.f; }
    else if(component == 2) { o[0] = float((a[0] + a[3]) / dn); o[1] = float((a[1] + a[4]) / dn); o[2] = float((a[2] + a[5]) / dn); }
    else { const int c = component * 3; o[0] = float(a[c] / dn); o[1] = float(a[c + 1] / dn); o[2] = float(a[c + 2] / dn); }
    o[3] = 1.f;
  }
  return RT_OK;
}

}  // extern "C"

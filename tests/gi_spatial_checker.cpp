// gi_spatial_checker.cpp — CPU restatement of the ReSTIR GI spatial reuse pass (rt_set_gi_spatial, csrc/gi_spatial.hip) for the tests.
// TEST INFRASTRUCTURE: built by tests/gi_spatial.py together with oracle/orc_scene.cpp, with the oracle's flags.  Scalar code over include/rt_detmath.h
// (IEEE sqrt and divisions, no contraction) and the oracle's decoders, BSDF and any-hit; every expression is the kernel's — the GPU tests compare the
// pass's reservoirs and RT_BUF_DENOISE_IND_A word for word.  Inputs are the frame's G-buffer and the indirect reservoirs the indirect stage wrote.
#include "../oracle/orc_shading.h"
#include <cstring>

namespace {
using namespace orc;

const uint32_t GI_SPATIAL_SALT = 0x47495350u;
const float GI_SKY_COORD = 1e20f;

bool skySample(vec3 xs) { return rt_abs(xs.x) >= GI_SKY_COORD || rt_abs(xs.y) >= GI_SKY_COORD || rt_abs(xs.z) >= GI_SKY_COORD; }
float jacobian(vec3 xr, vec3 xn, vec3 xs, vec3 ns)
{
  const vec3 vr = xr - xs, vn = xn - xs;
  const float dr2 = dot(vr, vr), dn2 = dot(vn, vn);
  const float cr = rt_abs(dot(ns, vr)) / rt_sqrt(dr2);
  const float cn = rt_abs(dot(ns, vn)) / rt_sqrt(dn2);
  return (cr * dn2) / (cn * dr2);
}
bool jacobianOk(float J, float jmax) { return !(rt_isnan(J) || rt_isinf(J) || J > jmax || J < 1.0f / jmax); }
bool resvInvalidW(float w) { return rt_isnan(w) || w < 0.0f; }
bool GISampleValid(const rt_gi_sample& s) { return s.nv.x < 1.1f && !hasNan(toV(s.L)); }

// getIndirectStateFromGBuffer (pathtrace.glsl:277-313)
bool stateFromGBuffer(const uint32_t* g, const Ray& ray, State& s, float& depth)
{
  depth = rt_u2f(g[0]);
  if(depth >= RT_INFINITY * 0.8f) return false;
  s.position = ray.origin + ray.direction * depth;
  s.normal = decompress_unit_vec(g[1]);
  s.ffnormal = dot(s.normal, ray.direction) <= 0.0f ? s.normal : -s.normal;
  s.mat.albedo = xyz(unpackUnorm4x8(g[3]));
  s.mat.emission = V3(0.f);
  const vec4 matInfo = unpackUnorm4x8(g[2]);
  s.mat.metallic = matInfo.x;
  s.mat.roughness = matInfo.y;
  s.mat.ior = matInfo.z * RT_MAX_IOR_MINUS_ONE + 1.f;
  s.mat.transmission = matInfo.w;
  s.matID = g[3] >> 24;
  return true;
}

struct Checker { Scene scene; };
}  // namespace

extern "C" {

void* gis_create(const rt_scene_desc* d)
{
  Checker* k = new Checker();
  k->scene.upload(d);
  k->scene.build();
  return k;
}
void gis_destroy(void* p) { delete static_cast<Checker*>(p); }

// J of the hand-built cases (sky samples: 1) and whether the tap passes the jacobianMax test
float gis_jacobian(const float* xr, const float* xn, const float* xs, const float* ns, float jacobianMax, int* accepted)
{
  const vec3 s = V3(xs[0], xs[1], xs[2]);
  const float J = skySample(s) ? 1.0f : jacobian(V3(xr[0], xr[1], xr[2]), V3(xn[0], xn[1], xn[2]), s, V3(ns[0], ns[1], ns[2]));
  *accepted = jacobianOk(J, jacobianMax) ? 1 : 0;
  return J;
}

// One frame's pass.  thisG: W x H x uint4; resv: (W/2) x (H/2) reservoirs; out: the pass's reservoirs; indA: RGBA32F, row pitch W, updated in place
// (pixels without a surface keep what they hold).  taps (optional, (W/2) x (H/2)): the number of accepted taps per pixel.
int gis_run(void* p, const rt_state* st, const rt_scene_camera* cam, const rt_gi_spatial* s, const uint32_t* thisG, const rt_indirect_reservoir* resv,
            rt_indirect_reservoir* out, float* indA, int32_t* taps)
{
  Checker* k = static_cast<Checker*>(p);
  const int W = st->size.x, H = st->size.y;
  const ivec2 indSize{W / 2, H / 2};
  const float invJmax = 1.0f / s->jacobianMax;
  const int span = 2 * s->radius + 1;
  for(int y = 0; y < indSize.y; y++)
    for(int x = 0; x < indSize.x; x++) {
      const size_t idx = size_t(y) * indSize.x + x;
      Shader c(k->scene, *st, *cam);
      c.imageCoords = ivec2{x, y};
      const Ray ray = c.raySpawn(ivec2{x, y}, indSize);
      const uint32_t* gp = thisG + (size_t(2 * y) * W + 2 * x) * 4;
      State g0; float dp;
      if(taps) taps[idx] = 0;
      if(!stateFromGBuffer(gp, ray, g0, dp)) { std::memset(&out[idx], 0, sizeof(rt_indirect_reservoir)); continue; }
      g0.position += g0.ffnormal * 2e-2f;
      const vec3 xr = g0.position, nr = g0.ffnormal, wo = -ray.direction, np = g0.normal;
      const uint32_t hp = gp[3] & 0xFF000000u;
      c.seed = tea(uint32_t(indSize.x) * uint32_t(y) + uint32_t(x), tea(st->time, GI_SPATIAL_SALT));
      rt_indirect_reservoir rs = resv[idx];
      for(int t = 0; t < s->samples; t++) {
        const float u1 = rnd(c.seed), u2 = rnd(c.seed), rr = rnd(c.seed);
        const int ox = rt_ftoi(rt_floor(u1 * float(span))) - s->radius, oy = rt_ftoi(rt_floor(u2 * float(span))) - s->radius;
        if(ox == 0 && oy == 0) continue;
        const int qx = x + ox, qy = y + oy;
        if(qx < 0 || qy < 0 || qx >= indSize.x || qy >= indSize.y) continue;
        const uint32_t* gq = thisG + (size_t(2 * qy) * W + 2 * qx) * 4;
        const float dq = rt_u2f(gq[0]);
        if(dq >= RT_INFINITY * 0.8f) continue;
        if((gq[3] & 0xFF000000u) != hp) continue;
        if(!(dot(np, decompress_unit_vec(gq[1])) >= s->normalThreshold)) continue;
        if(!(rt_abs(dq - dp) <= s->depthThreshold * dp)) continue;
        const rt_indirect_reservoir& rq = resv[size_t(qy) * indSize.x + qx];
        if(rq.num == 0u || resvInvalidW(rq.weight) || !GISampleValid(rq.giSample)) continue;
        const vec3 xs = toV(rq.giSample.xs), ns = toV(rq.giSample.ns);
        const bool sky = skySample(xs);
        const vec3 toS = sky ? -ns : xs - xr;
        if(!(dot(nr, toS) > 0.0f)) continue;
        const float J = sky ? 1.0f : jacobian(xr, toV(rq.giSample.xv), xs, ns);
        if(rt_isnan(J) || rt_isinf(J) || J > s->jacobianMax || J < invJmax) continue;
        if(s->mode == RT_GI_SPATIAL_VISIBILITY) {
          float tmax = RT_INFINITY;
          vec3 dir = toS;
          if(!sky) {
            tmax = length(toS) - 2e-2f;
            if(tmax <= 0.0f) continue;
            dir = normalize(toS);
          }
          if(c.AnyHit(Ray{xr, dir}, tmax)) continue;
        }
        const float w = rq.weight * J;
        rs.weight += w; rs.num += rq.num;
        if(rr * rs.weight < w) { rs.giSample = rq.giSample; rs.giSample.xv = toR(xr); rs.giSample.nv = toR(nr); }
        if(taps) taps[idx]++;
      }
      out[idx] = rs;
      vec3 indirect = V3(0.0f);
      const rt_gi_sample gi = rs.giSample;
      if(!resvInvalidW(rs.weight) && GISampleValid(gi)) {
        const vec3 primWi = normalize(toV(gi.xs) - toV(gi.xv));
        State ps = g0;
        ps.mat.albedo = V3(1.0f);
        const float bigW = rs.weight / (resvToScalar(toV(gi.L)) * float(rs.num));
        indirect = toV(gi.L) * c.BSDF(ps, wo, toV(gi.nv), primWi) * satDot(toV(gi.nv), primWi) * bigW;
      }
      vec3 pixelColor = HDRToLDR(c.clampRadiance(indirect));
      pixelColor = c.clampRadiance(pixelColor);
      float* o = indA + (size_t(y) * W + x) * 4;
      o[0] = pixelColor.x; o[1] = pixelColor.y; o[2] = pixelColor.z; o[3] = 1.0f;
    }
  return RT_OK;
}

}  // extern "C"

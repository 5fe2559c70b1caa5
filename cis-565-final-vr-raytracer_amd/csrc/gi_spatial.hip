// gi_spatial.hip — ReSTIR GI spatial reuse (rt_set_gi_spatial; include/rt_abi.h states the contract).
//
// The reference's indirect stage reuses path samples temporally only (indirect_stage.comp:228-268 ignores eSpatial / eSpatiotemporal).  This pass adds
// the spatial step of ReSTIR GI (Ouyang et al. 2021) after the indirect stage, at half resolution.  It reads only what is final for the frame (this frame's
// G-buffer and the indirect reservoirs the stage wrote after temporal reuse), so every pixel is a pure function of its inputs:
//
//   k_gi_spatial   receiver x_r / n_r = the indirect stage's decode of the G-buffer at 2p (position moved 2e-2 along ffnormal); r_s starts as the pixel's own
//                  reservoir; per tap: u1, u2, rr from the pass's stream tea(indW*y + x, tea(time, 'GISP')), offset in [-R, R]^2, geometry tests against
//                  the neighbour's G-buffer, the neighbour reservoir's validity, the receiver hemisphere, the Jacobian of the reconnection shift
//                  (sky samples: J = 1), in mode 2 an any-hit visibility ray from x_r; merge w = W_q * J (pHat = luminance(L) is the same at every receiver)
//                  by resvMerge's rule, the sample moving to (x_r, n_r).  Shading: restirIndirectFinish's expressions -> RT_BUF_DENOISE_IND_A.
//
// Numerics (include/rt_detmath.h): IEEE sqrt and divisions, no contraction — tests/gi_spatial_checker.cpp restates every expression on the CPU and the GPU
// tests compare word for word.  Neighbour reservoirs (76 B) are gathered from global memory: a radius-10 halo does not fit in LDS.
// Launch shape: one thread per half-resolution pixel, an 8 x 8 tile per wave64 in the stages' XCD-striped order, the whole traversal stack in LDS (the
// reference mode's launch).  Visibility evaluates no sky, so one compilation serves both sky models.
#define RT_COUNT 0   // the pass does not feed rt_get_counters
#include "stage_common.h"
#include "gi_spatial.h"

namespace rt {
namespace {

constexpr uint32_t GI_SPATIAL_SALT = 0x47495350u;   // "GISP"
constexpr float GI_SKY_COORD = 1e20f;                // |x_s| component of a sky sample (x + wi * RT_INFINITY * 0.8, indirect_stage.comp)

RT_DEV bool giSkySample(f3 xs) { return rt_abs(xs.x) >= GI_SKY_COORD || rt_abs(xs.y) >= GI_SKY_COORD || rt_abs(xs.z) >= GI_SKY_COORD; }

// |dot(n_s, v_r)| / |v_r| * |v_n|^2 / (|dot(n_s, v_n)| / |v_n| * |v_r|^2), left to right; v_r = x_r - x_s, v_n = x_n - x_s
RT_DEV float giJacobian(f3 xr, f3 xn, f3 xs, f3 ns)
{
  const f3 vr = xr - xs, vn = xn - xs;
  const float dr2 = dot(vr, vr), dn2 = dot(vn, vn);
  const float cr = rt_abs(dot(ns, vr)) / rt_sqrt(dr2);
  const float cn = rt_abs(dot(ns, vn)) / rt_sqrt(dn2);
  return (cr * dn2) / (cn * dr2);
}

#ifndef RT_GI_SPATIAL_LB
#define RT_GI_SPATIAL_LB 4
#endif
__global__ __launch_bounds__(64, RT_GI_SPATIAL_LB) void k_gi_spatial(DevScene S, rt_state st, rt_scene_camera cam, GiSpatialArgs A, int tilesX, int tilesY)
{
  extern __shared__ uint2 s_stack[];
  const TileCoord tile = tileOf(tilesX, tilesY);
  const int lane = int(threadIdx.x);
  const i2 indSize{A.W / 2, A.H / 2};
  const i2 px{tile.x * 8 + (lane & 7), tile.y * 8 + (lane >> 3)};
  if(!tile.valid || px.x >= indSize.x || px.y >= indSize.y) return;
  const size_t idx = size_t(px.y) * indSize.x + px.x;
  Ctx c(S, st, cam, s_stack + lane);
  c.imageCoords = px;
  const Ray ray = c.raySpawn(px, indSize);
  const uint4 gp = A.thisG[size_t(px.y * 2) * A.W + px.x * 2];
  GState g0; float dp;
  if(!stateFromGBuffer(gp, ray, g0, dp)) {   // no surface: IND_A stays as the indirect stage wrote it; a zero reservoir
    rt_indirect_reservoir z;
    z.giSample.L = rt_vec3{0, 0, 0}; z.giSample.xv = rt_vec3{0, 0, 0}; z.giSample.nv = rt_vec3{0, 0, 0};
    z.giSample.xs = rt_vec3{0, 0, 0}; z.giSample.ns = rt_vec3{0, 0, 0}; z.giSample.pHat = 0.f;
    z.num = 0; z.weight = 0.f; z.bigW = 0.f;
    A.out[idx] = z;
    return;
  }
  g0.position += g0.ffnormal * 2e-2f;   // indirect_stage.comp:299
  const f3 xr = g0.position, nr = g0.ffnormal, wo = -ray.direction;
  const f3 np = g0.normal;
  const uint32_t hp = gp.w & 0xFF000000u;
  c.seed = tea(uint32_t(indSize.x) * uint32_t(px.y) + uint32_t(px.x), tea(st.time, GI_SPATIAL_SALT));
  const float invJmax = 1.0f / A.jacobianMax;
  const int span = 2 * A.radius + 1;
  rt_indirect_reservoir rs = A.resv[idx];
  for(int k = 0; k < A.samples; k++) {
    const float u1 = rnd(c.seed), u2 = rnd(c.seed), rr = rnd(c.seed);
    const i2 o{rt_ftoi(rt_floor(u1 * float(span))) - A.radius, rt_ftoi(rt_floor(u2 * float(span))) - A.radius};
    if(o.x == 0 && o.y == 0) continue;
    const i2 q{px.x + o.x, px.y + o.y};
    if(q.x < 0 || q.y < 0 || q.x >= indSize.x || q.y >= indSize.y) continue;
    const uint4 gq = A.thisG[size_t(q.y * 2) * A.W + q.x * 2];
    const float dq = rt_u2f(gq.x);
    if(dq >= RT_INFINITY * 0.8f) continue;                       // no surface at q: its reservoir is stale
    if((gq.w & 0xFF000000u) != hp) continue;
    if(!(dot(np, decompress_unit_vec(gq.y)) >= A.normalThreshold)) continue;
    if(!(rt_abs(dq - dp) <= A.depthThreshold * dp)) continue;
    const rt_indirect_reservoir rq = A.resv[size_t(q.y) * indSize.x + q.x];
    if(rq.num == 0u || resvInvalidW(rq.weight) || !GISampleValid(rq.giSample)) continue;
    const f3 xs = mk3(rq.giSample.xs), ns = mk3(rq.giSample.ns);
    const bool sky = giSkySample(xs);
    const f3 toS = sky ? -ns : xs - xr;
    if(!(dot(nr, toS) > 0.0f)) continue;
    const float J = sky ? 1.0f : giJacobian(xr, mk3(rq.giSample.xv), xs, ns);
    if(rt_isnan(J) || rt_isinf(J) || J > A.jacobianMax || J < invJmax) continue;
    if(A.mode == RT_GI_SPATIAL_VISIBILITY) {
      float tmax = RT_INFINITY;
      f3 dir = toS;
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
  }
  A.out[idx] = rs;
  // restirIndirectFinish's shading (stages.hip)
  f3 indirect = mk3(0.0f);
  const rt_gi_sample gi = rs.giSample;
  if(!resvInvalidW(rs.weight) && GISampleValid(gi)) {
    const f3 primWi = normalize(mk3(gi.xs) - mk3(gi.xv));
    Material pm = g0.mat;
    pm.albedo = mk3(1.0f);
    const float bigW = rs.weight / (resvToScalar(mk3(gi.L)) * float(rs.num));
    indirect = mk3(gi.L) * metallicWorkflowBSDF(pm, mk3(gi.nv), wo, primWi) * satDot(mk3(gi.nv), primWi) * bigW;
  }
  f3 pixelColor = HDRToLDR(c.clampRadiance(indirect));
  pixelColor = c.clampRadiance(pixelColor);
  A.indA[size_t(px.y) * A.W + px.x] = make_float4(pixelColor.x, pixelColor.y, pixelColor.z, 1.0f);
}

}  // namespace

hipError_t launchGiSpatial(hipStream_t stream, const DevScene& Sin, const rt_state& st, const rt_scene_camera& cam, const GiSpatialArgs& A)
{
  DevScene S = Sin;
  S.stackEntries = S.stackTotal;   // the whole stack in LDS: the overflow areas of the stages are never touched
  const int tilesX = (A.W / 2 + 7) / 8, tilesY = (A.H / 2 + 7) / 8;
  if(tilesX <= 0 || tilesY <= 0) return hipSuccess;
  const size_t lds = size_t(S.stackEntries) * 64 * sizeof(uint2);
  hipLaunchKernelGGL(k_gi_spatial, dim3(tileGrid(tilesX, tilesY)), dim3(64), lds, stream, S, st, cam, A, tilesX, tilesY);
  return hipGetLastError();
}

}  // namespace rt

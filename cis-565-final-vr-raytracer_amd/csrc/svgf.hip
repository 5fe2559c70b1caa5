// svgf.hip — variance-guided spatiotemporal denoiser (rt_set_denoiser RT_DENOISER_SVGF; include/rt_abi.h).
//
// The reference's README names it as the filter it wanted ("Future Work -> Better Denoiser": the A-Trous filter treats every tap as having the same
// variance and over-blurs indirect light; SVGF drives the same kernel with a per-pixel variance).  It filters the signal the A-Trous chain filters —
// the demodulated HDRToLDR(clampRadiance(x)) colour of the direct image (full resolution) and of the indirect image (half resolution, G-buffer read
// at 2p) — so an A/B of the two differs in the filter only.  Per component, in this order:
//
//   k_svgf_temporal   decode this frame's geometry (normal, material hash, the A-Trous chain's reconstructed position); reproject to
//                     q = motion(p) (direct) / motion(2p) >> 1 (indirect); q is consistent when it lies in the grid and the previous G-buffer at q
//                     (2q for indirect) has the same material hash, dot(n, n_prev) > 0.9 and |cam.lastPosition - position| < depth_prev * 1.05
//                     (findTemporalNeighborDirect's test).  n = consistent ? min(n_prev + 1, cap) : 1, a = max(alphaC, 1/n), am = max(alphaM, 1/n),
//                     C = mix(C_prev, c, a), m1 = mix(m1_prev, l, am), m2 = mix(m2_prev, l*l, am), l = luminance(c), mix(x, y, t) = x * (1 - t) + y * t.
//                     A pixel without a valid material clears its history.
//   k_svgf_variance   n >= 4: var = max(0, m2 - m1^2); else the same from the moments of the 7 x 7 neighbourhood (j outer, i inner) weighted by the
//                     A-Trous normal and depth terms wN * wD, same material only.  Writes (C, var).
//   k_svgf_atrous     level l (step 2^l): 5 x 5 gather (j outer, i inner), weight wL * wN * wD * kGauss with
//                     wL = exp(-(|l_p - l_q| / (phiLum * sqrt(g3x3(var)_p) + 1e-10))), g3x3 = (1/4, 1/8, 1/16) over the in-grid 3 x 3 pixels of the
//                     level's input variance; colour = sum(w c) / sum(w), variance = sum(w^2 var) / sum(w)^2 with the A-Trous zero-weight, NaN and
//                     range guard; level 0's colour becomes the colour history; the last level applies LDRToHDR and writes (colour, 1).
// Numerics (include/rt_detmath.h): rt_exp, IEEE sqrt and divisions, no contraction — tests/svgf_checker.cpp restates every expression on the CPU and
// the GPU tests compare word for word.  Every weight is a plain per-pixel gather: the luminance term depends on p's variance, so the symmetric-pair
// evaluation of k_denoise_lds does not apply.
// Launch shape: one wave64 per 8 x 8 tile, the XCD-striped tile order of the stages (tileOf).
#define RT_COUNT 0
#include "filter_common.h"
#include "svgf.h"

namespace rt {
namespace {

RT_DEV float svgfMix(float x, float y, float t) { return x * (1.0f - t) + y * t; }
RT_DEV float svgfNormW(f3 n, f3 nq, float sigN) { return rt_min(1.0f, rt_exp(-(dot(n - nq, n - nq) / sigN))); }
RT_DEV float svgfDepthW(f3 p, f3 pq, float sigD) { return rt_exp(-(dot(p - pq, p - pq) / sigD)) + 1e-2f; }

struct SvgfPix { i2 p; bool valid; size_t idx; };
RT_DEV SvgfPix svgfPixel(const SvgfArgs& A, int tilesX, int tilesY)
{
  const TileCoord tile = tileOf(tilesX, tilesY);
  const int lane = int(threadIdx.x);
  SvgfPix r;
  r.p = i2{tile.x * 8 + (lane & 7), tile.y * 8 + (lane >> 3)};
  r.valid = tile.valid && r.p.x < A.bx && r.p.y < A.by;
  r.idx = size_t(r.p.y) * A.bx + r.p.x;
  return r;
}

template <bool IND>
__global__ __launch_bounds__(64) void k_svgf_temporal(SvgfArgs A, rt_scene_camera cam, int tilesX, int tilesY)
{
  const SvgfPix P = svgfPixel(A, tilesX, tilesY);
  if(!P.valid) return;
  const i2 bound{A.bx, A.by};
  const i2 gc = IND ? i2{P.p.x * 2, P.p.y * 2} : P.p;
  const uint4 g = A.thisG[size_t(gc.y) * A.W + gc.x];
  const f3 norm = decompress_unit_vec(g.y);
  const f3 pos = cameraPosDenoise(cam, gc, rt_u2f(g.x), bound);
  const uint32_t hash = g.w & 0xFF000000u;
  A.geomN[P.idx] = make_float4(norm.x, norm.y, norm.z, rt_u2f(hash));
  A.geomP[P.idx] = make_float4(pos.x, pos.y, pos.z, 0.f);
  if(hash == RT_INVALID_MAT_ID) {
    A.histC[P.idx] = make_float4(0.f, 0.f, 0.f, 0.f);
    A.histM[P.idx] = make_float2(0.f, 0.f);
    return;
  }
  const float4 cin = A.noisy[size_t(P.p.y) * A.W + P.p.x];
  const f3 c = mk3(cin.x, cin.y, cin.z);
  float4 cp = make_float4(0.f, 0.f, 0.f, 0.f);
  float2 mp = make_float2(0.f, 0.f);
  int n = 1;
  if(A.histValid) {
    const short2 mv = A.motion[size_t(gc.y) * A.W + gc.x];
    const i2 q = IND ? i2{int(mv.x) >> 1, int(mv.y) >> 1} : i2{int(mv.x), int(mv.y)};
    if(q.x >= 0 && q.y >= 0 && q.x < bound.x && q.y < bound.y) {
      const i2 gq = IND ? i2{q.x * 2, q.y * 2} : q;
      const uint4 pg = A.lastG[size_t(gq.y) * A.W + gq.x];
      const f3 pnorm = decompress_unit_vec(pg.y);
      const float pdepth = rt_u2f(pg.x);
      const float reprojDepth = length(mk3(cam.lastPosition) - pos);
      if((pg.w & 0xFF000000u) == hash && dot(norm, pnorm) > 0.9f && reprojDepth < pdepth * 1.05f) {
        const size_t qi = size_t(q.y) * A.bx + q.x;
        cp = A.prevC[qi]; mp = A.prevM[qi];
        n = min(int(cp.w) + 1, A.cap);
      }
    }
  }
  const float inv = 1.0f / float(n);
  const float a = rt_max(A.alphaC, inv), am = rt_max(A.alphaM, inv);
  const float l = luminance(c);
  A.histC[P.idx] = make_float4(svgfMix(cp.x, c.x, a), svgfMix(cp.y, c.y, a), svgfMix(cp.z, c.z, a), float(n));
  A.histM[P.idx] = make_float2(svgfMix(mp.x, l, am), svgfMix(mp.y, l * l, am));
}

template <bool IND>
__global__ __launch_bounds__(64) void k_svgf_variance(SvgfArgs A, int tilesX, int tilesY)
{
  const SvgfPix P = svgfPixel(A, tilesX, tilesY);
  if(!P.valid) return;
  float4* dst = A.bufA + size_t(P.p.y) * A.W + P.p.x;
  const float4 gn = A.geomN[P.idx];
  const uint32_t hash = rt_f2u(gn.w);
  if(hash == RT_INVALID_MAT_ID) { *dst = make_float4(0.f, 0.f, 0.f, 0.f); return; }
  const float4 C = A.histC[P.idx];
  float m1, m2;
  if(C.w >= 4.0f) {
    const float2 M = A.histM[P.idx];
    m1 = M.x; m2 = M.y;
  } else {
    const f3 norm = mk3(gn.x, gn.y, gn.z);
    const float4 gp = A.geomP[P.idx];
    const f3 pos = mk3(gp.x, gp.y, gp.z);
    float s1 = 0.f, s2 = 0.f, sw = 0.f;
    for(int j = -3; j <= 3; j++)
      for(int i = -3; i <= 3; i++) {
        const i2 q{P.p.x + i, P.p.y + j};
        if(q.x < 0 || q.y < 0 || q.x >= A.bx || q.y >= A.by) continue;
        const size_t qi = size_t(q.y) * A.bx + q.x;
        const float4 qn = A.geomN[qi];
        if(rt_f2u(qn.w) != hash) continue;
        const float4 qp = A.geomP[qi];
        const float w = svgfNormW(norm, mk3(qn.x, qn.y, qn.z), A.sigN) * svgfDepthW(pos, mk3(qp.x, qp.y, qp.z), A.sigD);
        const float2 M = A.histM[qi];
        s1 += w * M.x; s2 += w * M.y; sw += w;
      }
    m1 = s1 / sw; m2 = s2 / sw;
  }
  const float v = m2 - m1 * m1;
  *dst = make_float4(C.x, C.y, C.z, (v > 0.0f) ? v : 0.0f);   // (a NaN variance becomes 0)
}

template <bool IND>
__global__ __launch_bounds__(64) void k_svgf_atrous(SvgfArgs A, const float4* src, float4* dst, int level, int tilesX, int tilesY)
{
  const SvgfPix P = svgfPixel(A, tilesX, tilesY);
  if(!P.valid) return;
  const int last = IND ? SVGF_LEVELS_INDIRECT - 1 : SVGF_LEVELS_DIRECT - 1;
  const int step = 1 << level;
  const float4 gn = A.geomN[P.idx];
  const uint32_t hash = rt_f2u(gn.w);
  f3 res = mk3(0.0f);
  float var = 0.0f;
  if(hash != RT_INVALID_MAT_ID) {
    const f3 norm = mk3(gn.x, gn.y, gn.z);
    const float4 gp = A.geomP[P.idx];
    const f3 pos = mk3(gp.x, gp.y, gp.z);
    const float4 cc = src[size_t(P.p.y) * A.W + P.p.x];
    const float lp = luminance(mk3(cc.x, cc.y, cc.z));
    float gv = 0.0f;
    for(int j = -1; j <= 1; j++)
      for(int i = -1; i <= 1; i++) {
        const i2 q{P.p.x + i, P.p.y + j};
        if(q.x < 0 || q.y < 0 || q.x >= A.bx || q.y >= A.by) continue;
        const float k = (i == 0 && j == 0) ? 0.25f : ((i == 0 || j == 0) ? 0.125f : 0.0625f);
        gv += k * src[size_t(q.y) * A.W + q.x].w;
      }
    const float denom = A.phiLum * rt_sqrt(gv) + 1e-10f;
    f3 sum = mk3(0.0f);
    float sumV = 0.0f, sumW = 0.0f;
    for(int j = -2; j <= 2; j++)
      for(int i = -2; i <= 2; i++) {
        const i2 q{P.p.x + i * step, P.p.y + j * step};
        if(q.x < 0 || q.y < 0 || q.x >= A.bx || q.y >= A.by) continue;
        const size_t qi = size_t(q.y) * A.bx + q.x;
        const float4 qn = A.geomN[qi];
        if(rt_f2u(qn.w) != hash) continue;
        const float4 qp = A.geomP[qi];
        const float4 cq = src[size_t(q.y) * A.W + q.x];
        const float wL = rt_exp(-(rt_abs(lp - luminance(mk3(cq.x, cq.y, cq.z))) / denom));
        const float w = ((wL * svgfNormW(norm, mk3(qn.x, qn.y, qn.z), A.sigN)) * svgfDepthW(pos, mk3(qp.x, qp.y, qp.z), A.sigD)) * kGauss[i + 2][j + 2];
        sum += mk3(cq.x, cq.y, cq.z) * w;
        sumV += (w * w) * cq.w;
        sumW += w;
      }
    if(sumW < 1e-5f) { res = mk3(0.0f); var = 0.0f; }
    else { res = sum / sumW; var = sumV / (sumW * sumW); }
    if(hasNan(res) || res.x < 0 || res.y < 0 || res.z < 0 || res.x > 1e8f || res.y > 1e8f || res.z > 1e8f) { res = mk3(0.0f); var = 0.0f; }
    if(!(var >= 0.0f)) var = 0.0f;
  }
  if(level == 0) {   // SVGF's feedback: the filtered colour becomes the colour history (n stays)
    const float n = A.histC[P.idx].w;
    A.histC[P.idx] = make_float4(res.x, res.y, res.z, n);
  }
  float4* o = dst + size_t(P.p.y) * A.W + P.p.x;
  if(level == last) { res = LDRToHDR(res); *o = make_float4(res.x, res.y, res.z, 1.0f); }
  else *o = make_float4(res.x, res.y, res.z, var);
}

template <bool IND>
hipError_t launchStep(hipStream_t stream, const SvgfArgs& A, const rt_scene_camera& cam, int step)
{
  const int tilesX = (A.bx + 7) / 8, tilesY = (A.by + 7) / 8;
  if(tilesX <= 0 || tilesY <= 0) return hipSuccess;
  const dim3 grid(tileGrid(tilesX, tilesY)), block(64);
  const int levels = IND ? SVGF_LEVELS_INDIRECT : SVGF_LEVELS_DIRECT;
  if(step == 0) hipLaunchKernelGGL(k_svgf_temporal<IND>, grid, block, 0, stream, A, cam, tilesX, tilesY);
  else if(step == 1) hipLaunchKernelGGL(k_svgf_variance<IND>, grid, block, 0, stream, A, tilesX, tilesY);
  else {
    const int l = step - 2;
    if(l >= levels) return hipErrorInvalidValue;
    // (colour, variance): bufA -> bufB -> bufA ... ; the last level writes `out`
    const float4* src = (l & 1) ? A.bufB : A.bufA;
    float4* dst = (l == levels - 1) ? A.out : ((l & 1) ? A.bufA : A.bufB);
    hipLaunchKernelGGL(k_svgf_atrous<IND>, grid, block, 0, stream, A, src, dst, l, tilesX, tilesY);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launchSvgfStep(hipStream_t stream, const SvgfArgs& A, const rt_scene_camera& cam, bool ind, int step)
{
  if(step < 0 || step >= svgfSteps(ind)) return hipErrorInvalidValue;
  return ind ? launchStep<true>(stream, A, cam, step) : launchStep<false>(stream, A, cam, step);
}

}  // namespace rt

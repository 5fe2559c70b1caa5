// filters.hip — the stages of a frame that trace no ray and shade nothing, compiled ONCE (RT_SKY / RT_COUNT / RT_LAT of stages.hip do not reach them):
//   k_denoise_geom<IND> + k_denoise_lds<IND,FAST>   denoise_common.glsl + denoise_direct.comp / denoise_indirect.comp: one edge-avoiding A-Trous level
//   k_compose                                       compose.comp:23-43
//   k_ind_tile_order                                longest-first tile lists of the indirect stage, launched by every build of it
// Launch shape and tile order: stages.hip.
#define RT_COUNT 0
#include "filter_common.h"
#include <algorithm>

namespace rt {

// loadThisGeometry (denoise_common.glsl:42-55) hoisted out of the 25-tap loop: every pixel's normal, material hash and
// reconstructed position are decoded once per frame instead of once per tap per level (the reference re-derives them
// 25 x 9 times per pixel: 2 mat-vec + 2 normalisations each).  Same expressions => same bits.
template <bool IND>
__global__ __launch_bounds__(64) void k_denoise_geom(DevFrame F, rt_state st, rt_scene_camera cam, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 bound = IND ? i2{st.size.x / 2, st.size.y / 2} : i2{st.size.x, st.size.y};
  const i2 coord{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  if(coord.x >= bound.x || coord.y >= bound.y || coord.y >= rowEnd) return;
  const i2 gc = IND ? i2{coord.x * 2, coord.y * 2} : coord;
  const uint4 g = loadG(F.thisG, F, gc);
  const f3 norm = decompress_unit_vec(g.y);
  const f3 pos = cameraPosDenoise(cam, gc, rt_u2f(g.x), bound);
  const size_t idx = size_t(coord.y) * bound.x + coord.x;
  (IND ? F.geomNh : F.geomN)[idx] = make_float4(norm.x, norm.y, norm.z, rt_u2f(g.w & 0xFF000000u));
  (IND ? F.geomPh : F.geomP)[idx] = make_float4(pos.x, pos.y, pos.z, 0.f);
}

// exp(x) for x <= 0, bit-identical to rt_exp() on that domain (same range reduction, polynomial and scaling; the
// x > 88.7 early-out of rt_exp cannot trigger) but with selects instead of branches.
RT_DEV float expNonPositive(float x)
{
  const float z = rt_floor(rt_fma(x, 1.44269504088896341f, 0.5f));
  // n = (int)z wherever it matters: z <= 0 here, and below -127 (x < -88.4) the result is forced to 0 further down, so the
  // conversion is clamped instead of range-checked; a NaN clamps to -127 and e = NaN * 0
  const int n = int(fmaxf(z, -127.0f));
  float r = rt_fma(z, -0.693359375f, x);
  r = rt_fma(z, 2.12194440e-4f, r);
  const float rr = r * r;
  float p = 1.9875691500E-4f;
  p = rt_fma(p, r, 1.3981999507E-3f);
  p = rt_fma(p, r, 8.3334519073E-3f);
  p = rt_fma(p, r, 4.1665795894E-2f);
  p = rt_fma(p, r, 1.6666665459E-1f);
  p = rt_fma(p, r, 5.0000001201E-1f);
  p = rt_fma(p, rr, r);
  p = p + 1.0f;
  // rt_exp scales in two steps, (p * 2^a) * 2^b with a + b = n, so that results below the normal range round once; for
  // x >= -87.34 n >= -126, 2^n is a normal number and p * 2^n is the same single rounding.  Below that the result is 0.
  float e = p * rt_u2f(uint32_t(n + 127) << 23);
  // NaN in => NaN out through the arithmetic (rt_exp returns its argument, i.e. possibly another NaN payload; every caller
  // turns a NaN weight into the same cleared pixel)
  return (x < -87.33654475055310f) ? 0.0f : e;
}

// a / b for a uniform divisor b with y = RN(1 / b) precomputed by an IEEE division: q = RN(a*y), r = a - b*q (exact, fma),
// q' = RN(q + r*y) is the correctly rounded quotient (Markstein 1990, Theorem 7.1: holds when y is the correctly rounded
// reciprocal and no intermediate leaves the normal range).  launchDenoiseLevel enables this path only for 1e-6 <= b <= 1e6; then the
// residual r is a normal number whenever |a/b| >= 2^-25, and below that exp(-a/b) is exactly 1 whatever the last bit of the
// quotient.  Above 1e30 (a * y could overflow for the smallest divisors) and for a non-finite a the plain division runs.
template <bool FAST>
RT_DEV float divUniform(float a, float b, float y)
{
  if(!FAST) return a / b;
  const float q = a * y;
  const float r = __builtin_fmaf(-b, q, a);
  const float q2 = __builtin_fmaf(r, y, q);
  return (a <= 1.0e30f) ? q2 : a / b;   // (kept as a branch: measured 10 % faster filters than a select of `a`)
}

// ------------------------------------------------------------------------------------------------------------
// waveletFilter on chip.  The weight of tap q in pixel p's sum is, bit for bit, the weight of tap p in pixel q's sum:
// |a - b| = |b - a|, (a - b)^2 = (b - a)^2 component by component, the material test is symmetric and the 5x5 kernel is
// point symmetric.  On ONE a-trous sub-lattice (the pixels with equal coordinates modulo 2^level) the dilated stencil is a dense 5 x 5,
// so a workgroup that stages a lattice tile and its 2-pixel ring in LDS can evaluate every pair weight once: 12 "forward" offsets per pixel,
// backward taps from the neighbour's forward weights.  (A 256-thread / 16 x 16 tile version and the per-pixel gather were the first two
// forms of this filter; both are superseded by k_denoise_lds below and were removed in round 3 — profiles/r02_denoise_*_ab.txt.)
// ------------------------------------------------------------------------------------------------------------
constexpr int DT_NFWD = 12;
// forward half of the stencil in (i, j), j > 0 or (j == 0 and i > 0)
__device__ constexpr int8_t kFwdI[DT_NFWD] = {1, 2, -2, -1, 0, 1, 2, -2, -1, 0, 1, 2};
__device__ constexpr int8_t kFwdJ[DT_NFWD] = {0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2};
RT_DEV int fwdIndex(int i, int j) { return j == 0 ? i - 1 : (j == 1 ? 4 + i : 9 + i); }   // inverse of the two tables

template <bool IND, bool FAST>
RT_DEV float denoisePairWeight(f3 color, float lum, f3 norm, f3 pos, f3 colorQ, float lumQ, f3 normQ, f3 posQ, float gauss, float sigL, float sigN, float sigD, float yL,
                               float yN, float yD)
{
  const float distColor = IND ? dot(color - colorQ, color - colorQ) : rt_abs(lum - lumQ);
  const float wColor = expNonPositive(-divUniform<FAST>(distColor, sigL, yL)) + 1e-2f;
  const float distNorm2 = dot(norm - normQ, norm - normQ);
  const float wNorm = rt_min(1.0f, expNonPositive(-divUniform<FAST>(distNorm2, sigN, yN)));
  const float distPos2 = dot(pos - posQ, pos - posQ);
  const float wDepth = expNonPositive(-divUniform<FAST>(distPos2, sigD, yD)) + 1e-2f;
  return wColor * wNorm * wDepth * gauss;
}

// k_denoise_lds: a 64-thread workgroup takes an 8 x 8 tile of one a-trous sub-lattice, stages colour (+ luminance), normal + material hash and
// position of the tile and its 2-pixel ring (12 x 12 lattice pixels, 6.9 KB) and every lane takes its 25 taps from there: 7 global loads per lane
// instead of the 75 of a per-pixel gather (which kept the texture-address path 66-82 % busy, profiles/r02_denoise_lds_ab.txt); its one-wave
// workgroups fit into any free wave slot beside the traversal kernels of the frames in flight.
// Every pair weight is evaluated once: a lane owns its pixel's 12 forward weights and the centre weight; a backward
// tap takes the neighbour's forward weight when that neighbour is one of the tile's 64 pixels (71 % of the backward taps), the other 222 (pixel, offset)
// pairs of a tile are the same for every tile — a compile-time list, fetched before the first barrier and worked off in four full-wave passes.  17 weight
// evaluations per lane instead of 25 (-20 % executed VALU instructions); the weights travel through the LDS that held normals and positions, which are
// dead by then.  Same expressions and the accumulation order of the reference's loops (j outer, i inner): bit-identical to a per-pixel gather.
constexpr int DL_T = 8, DL_S = DL_T + 4;
// the (pixel p, forward offset k) pairs whose backward partner q = p - offset(k) lies outside the tile, offsets ascending, pixels ascending within an offset:
// pair = LDS index of p | LDS index of q << 8 in the staged 12 x 12 block, gauss = the kernel factor of the offset, base[k] = first pair of offset k
struct BwdPairs { uint32_t pair[256]; float gauss[256]; int16_t base[DT_NFWD + 1]; };
constexpr float kGaussFwdC[DT_NFWD] = {.0983f, .0219f, .0133f, .0596f, .0983f, .0596f, .0133f, .0030f, .0133f, .0219f, .0133f, .0030f};
constexpr BwdPairs makeBwdPairs()
{
  BwdPairs t{};
  int n = 0;
  for(int k = 0; k < DT_NFWD; k++) {
    const int i = kFwdI[k], j = kFwdJ[k];
    t.base[k] = int16_t(n);
    for(int p = 0; p < 64; p++) {
      const int qx = (p & 7) - i, qy = (p >> 3) - j;
      if(qx < 0 || qx > 7 || qy < 0) {
        const int pidx = ((p >> 3) + 2) * 12 + ((p & 7) + 2), qidx = pidx - j * 12 - i;
        t.pair[n] = uint32_t(pidx | (qidx << 8)); t.gauss[n] = kGaussFwdC[k]; n++;
      }
    }
  }
  t.base[DT_NFWD] = int16_t(n);
  return t;
}
__device__ constexpr BwdPairs kBwdPairs = makeBwdPairs();
constexpr int DL_NBWD = makeBwdPairs().base[DT_NFWD];
static_assert(DL_NBWD == 222, "backward pair list");
// slot of pixel (x, y)'s directly evaluated backward weight for forward offset k = (i, j): its rank in kBwdPairs.  Rows y < j lie outside with all 8 pixels,
// the rows below with |i| pixels each (x < i for i > 0, x > 7 + i for i < 0)
RT_DEV int bwdSlot(int k, int i, int j, int x, int y)
{
  const int ai = i < 0 ? -i : i;
  const int inRow = i > 0 ? x : x - (8 - ai);
  const int r = y < j ? 8 * y + x : 8 * j + (y - j) * ai + inRow;
  return kBwdPairs.base[k] + r;
}

template <bool IND, bool FAST>
__global__ __launch_bounds__(64) void k_denoise_lds(DevFrame F, rt_state st, const float4* src, float4* dst, int level, int rowBegin, int rowEnd, int tilesX, int tilesY,
                                                     float yL, float yN, float yD)
{
  __shared__ float4 sC[DL_S * DL_S];
  __shared__ float4 sNP[2 * DL_S * DL_S];
  float4* sN = sNP; float4* sP = sNP + DL_S * DL_S;
  const int step = 1 << level;
  const int total = tilesX * tilesY * step * step, perXcd = (total + 7) / 8;
  const int local = int(blockIdx.x >> 3);
  const int work = int(blockIdx.x & 7u) * perXcd + local;
  if(local >= perXcd || work >= total) return;
  const int sub = work % (step * step), tileIdx = work / (step * step);
  const int a = sub % step, b = sub / step;
  const int X0 = (tileIdx % tilesX) * DL_T, Y0 = (tileIdx / tilesX) * DL_T;
  const i2 bound = IND ? i2{st.size.x / 2, st.size.y / 2} : i2{st.size.x, st.size.y};
  const float sigLumin = IND ? st.sigLuminIndirect : st.sigLuminDirect;
  const float sigNormal = IND ? st.sigNormalIndirect : st.sigNormalDirect;
  const float sigDepth = IND ? st.sigDepthIndirect : st.sigDepthDirect;
  const int last = IND ? 4 : 3;
  const float4* gN = IND ? F.geomNh : F.geomN;
  const float4* gP = IND ? F.geomPh : F.geomP;
  const int lane = int(threadIdx.x);
#pragma unroll
  for(int it = 0; it < 3; it++) {
    const int idx = lane + 64 * it;
    if(idx < DL_S * DL_S) {
      const int lx = idx % DL_S, ly = idx / DL_S;
      const int px = a + step * (X0 - 2 + lx), py = rowBegin + b + step * (Y0 - 2 + ly);
      float4 c = make_float4(0.f, 0.f, 0.f, 0.f), n = make_float4(0.f, 0.f, 0.f, rt_u2f(RT_INVALID_MAT_ID)), q = make_float4(0.f, 0.f, 0.f, 0.f);
      if(px >= 0 && py >= 0 && px < bound.x && py < bound.y) {
        const size_t gi = size_t(py) * bound.x + px;
        n = gN[gi]; q = gP[gi];
        c = src[size_t(py) * F.W + px];
        c.w = IND ? 0.0f : luminance(mk3(c.x, c.y, c.z));
      }
      sC[idx] = c; sN[idx] = n; sP[idx] = q;
    }
  }
  uint32_t pr[4]; float pg[4];
#pragma unroll
  for(int r = 0; r < 4; r++) { const int idx = min(r * 64 + lane, DL_NBWD - 1); pr[r] = kBwdPairs.pair[idx]; pg[r] = kBwdPairs.gauss[idx]; }
  __syncthreads();
  const int ux = lane & 7, uy = lane >> 3;
  const int cidx = (uy + 2) * DL_S + (ux + 2);
  const float4 cN = sN[cidx], cC = sC[cidx], cP = sP[cidx];
  const uint32_t hash = rt_f2u(cN.w);
  const f3 color = mk3(cC.x, cC.y, cC.z), norm = mk3(cN.x, cN.y, cN.z), pos = mk3(cP.x, cP.y, cP.z);
  float wf[DT_NFWD];
#pragma unroll
  for(int k = 0; k < DT_NFWD; k++) {
    const int qidx = cidx + kFwdJ[k] * DL_S + kFwdI[k];
    const float4 qN = sN[qidx];
    float w = -1.0f;
    if(hash != RT_INVALID_MAT_ID && rt_f2u(qN.w) == hash) {
      const float4 qP = sP[qidx], qC = sC[qidx];
      w = denoisePairWeight<IND, FAST>(color, cC.w, norm, pos, mk3(qC.x, qC.y, qC.z), qC.w, mk3(qN.x, qN.y, qN.z), mk3(qP.x, qP.y, qP.z), kGauss[kFwdI[k] + 2][kFwdJ[k] + 2],
                                       sigLumin, sigNormal, sigDepth, yL, yN, yD);
    }
    wf[k] = w;
  }
  float wb[4];
#pragma unroll
  for(int r = 0; r < 4; r++) {
    float w = -1.0f;
    if(r * 64 + lane < DL_NBWD) {
      const int pidx = int(pr[r] & 0xffu), qidx = int(pr[r] >> 8);
      const float4 pN = sN[pidx], qN = sN[qidx];
      const uint32_t ph = rt_f2u(pN.w);
      if(ph != RT_INVALID_MAT_ID && rt_f2u(qN.w) == ph) {
        const float4 pC = sC[pidx], pP = sP[pidx], qC = sC[qidx], qP = sP[qidx];
        w = denoisePairWeight<IND, FAST>(mk3(pC.x, pC.y, pC.z), pC.w, mk3(pN.x, pN.y, pN.z), mk3(pP.x, pP.y, pP.z), mk3(qC.x, qC.y, qC.z), qC.w, mk3(qN.x, qN.y, qN.z),
                                         mk3(qP.x, qP.y, qP.z), pg[r], sigLumin, sigNormal, sigDepth, yL, yN, yD);
      }
    }
    wb[r] = w;
  }
  __syncthreads();
  float* sW = reinterpret_cast<float*>(sNP);
#pragma unroll
  for(int k = 0; k < DT_NFWD; k++) sW[k * 64 + lane] = wf[k];
#pragma unroll
  for(int r = 0; r < 4; r++) if(r * 64 + lane < DL_NBWD) sW[DT_NFWD * 64 + r * 64 + lane] = wb[r];
  __syncthreads();
  const i2 coord{a + step * (X0 + ux), rowBegin + b + step * (Y0 + uy)};
  if(coord.x >= bound.x || coord.y >= bound.y || coord.y >= rowEnd) return;
  f3 res = mk3(0.0f);
  if(hash != RT_INVALID_MAT_ID) {
    f3 sum = mk3(0.0f);
    float sumWeight = 0.0f;
#pragma unroll
    for(int j = -2; j <= 2; j++)
#pragma unroll
      for(int i = -2; i <= 2; i++) {
        float w;
        if(i == 0 && j == 0) {
          // the pixel with itself: every distance is x - x = 0 for finite inputs (NaN otherwise), every exponential exp(-0) = 1, the weight a constant — evaluated
          // with the general expression's own float operations, in its order.  A wave with a non-finite pixel takes the general path (scalar branch).
          const float dl = IND ? dot(color - color, color - color) : rt_abs(cC.w - cC.w);
#ifndef RT_NO_CENTRE_SHORTCUT
          // Only in the FAST instantiation: there every sigma has been checked to lie in [1e-6, 1e6] (uniformDivOk), so 0 / sigma = 0.  With sigma = 0 or NaN the
          // general expression is 0 / 0 = NaN and the reference clears the pixel — that case must take the general path.
          if(FAST && __ballot((dl == 0.0f && dot(norm - norm, norm - norm) == 0.0f && dot(pos - pos, pos - pos) == 0.0f) ? 0 : 1) == 0ull) w = (((1.0f + 1e-2f) * 1.0f) * (1.0f + 1e-2f)) * kGauss[2][2];
          else
#endif
          w = denoisePairWeight<IND, FAST>(color, cC.w, norm, pos, color, cC.w, norm, pos, kGauss[2][2], sigLumin, sigNormal, sigDepth, yL, yN, yD);
        }
        else if(j > 0 || (j == 0 && i > 0)) w = wf[fwdIndex(i, j)];
        else {
          const int k = fwdIndex(-i, -j), qx = ux + i, qy = uy + j;
          const bool inside = qx >= 0 && qx <= 7 && qy >= 0;
          w = sW[inside ? k * 64 + qy * 8 + qx : DT_NFWD * 64 + bwdSlot(k, -i, -j, ux, uy)];
        }
        if(w != -1.0f) {
          const float4 q = sC[cidx + j * DL_S + i];
          sum += mk3(q.x, q.y, q.z) * w;
          sumWeight += w;
        }
      }
    res = (sumWeight < 1e-5f) ? mk3(0.0f) : sum / sumWeight;
    if(hasNan(res) || res.x < 0 || res.y < 0 || res.z < 0 || res.x > 1e8f || res.y > 1e8f || res.z > 1e8f) res = mk3(0.0f);
  }
  if(level == last) res = LDRToHDR(res);
  storeImg(dst, F, coord, mk4(res, 1.0f));
}

// ------------------------------------------------------------------------------------------------------------
// compose.comp:23-43
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_compose(DevFrame F, rt_state st, int rowBegin, int rowEnd, int tilesX, int tilesY)
{
  const TileCoord tile = tileOf(tilesX, tilesY);
  if(!tile.valid) return;
  const int lane = int(threadIdx.x);
  const i2 coord{tile.x * 8 + (lane & 7), rowBegin + tile.y * 8 + (lane >> 3)};
  if(coord.x >= st.size.x || coord.y >= st.size.y || coord.y >= rowEnd) return;
  const float4* indSrc = (st.denoise > 0) ? F.denoiseIndB : F.denoiseIndA;
  const i2 half{coord.x / 2, coord.y / 2};
  if(st.modulate == 0) {
    storeImg(F.thisIndirectResult, F, coord, loadImg(indSrc, F, half));
  } else {
    const f3 albedo = xyz(unpackUnorm4x8(loadG(F.thisG, F, coord).w));
    const f3 direct = xyz(loadImg(F.thisDirectResult, F, coord)) * albedo;
    const f3 indirect = xyz(loadImg(indSrc, F, half)) * albedo;
    storeImg(F.thisDirectResult, F, coord, mk4(direct, 1.0f));
    storeImg(F.thisIndirectResult, F, coord, mk4(indirect, 1.0f));
  }
}

// Longest-first tile order for the indirect stage: the 25 % multi-bounce tiles (indirect_stage.comp:283-288) run up to
// maxDepth bounces while the rest stop after one, so they are dispatched first and the short tiles fill the tail.
// One thread per tile recomputes the tile flag exactly as the stage does and appends the tile to its XCD's list
// (multi-bounce from the front, single-bounce from the back).  Only the order changes, never a result.
__global__ __launch_bounds__(256) void k_ind_tile_order(rt_state st, int rowBegin, int tilesX, int tilesY, int cap, uint32_t* lists, uint32_t* counts)
{
  // one workgroup per XCD list; list positions come from LDS counters (8 k global atomics on 16 addresses cost 95 us)
  __shared__ uint32_t s_cnt[2];
  const int xcd = int(blockIdx.x);
  if(threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t* list = lists + size_t(xcd) * cap;
  const int indW = st.size.x / 2;
  const int G = tileChunk(tilesX, tilesY), nTiles = tilesX * tilesY;
  const int chunks = (nTiles + G - 1) / G;
  for(int s = xcd; s < chunks; s += 8) {
    for(int i = int(threadIdx.x); i < G; i += int(blockDim.x)) {
      const int ti = s * G + i;
      if(ti >= nTiles) continue;
      const int ty = ti / tilesX, tx = ti - ty * tilesX;
      uint32_t seed = tea(uint32_t(indW) * uint32_t(rowBegin + ty * 8) + uint32_t(tx * 8), st.time);
      const bool mb = rnd(seed) < 0.25f;
      const uint32_t t = uint32_t(ty * tilesX + tx);
      if(mb) list[atomicAdd(&s_cnt[0], 1u)] = t;
      else list[cap - 1 - int(atomicAdd(&s_cnt[1], 1u))] = t;
    }
  }
  __syncthreads();
  if(threadIdx.x < 2) counts[xcd * 2 + threadIdx.x] = s_cnt[threadIdx.x];
}

// divUniform's fast path: the divisor must keep every intermediate in the normal range (see there)
static bool uniformDivOk(float s) { return s >= 1e-6f && s <= 1e6f; }

// one level of an a-trous chain on the one-wave LDS-staged kernel
template <bool IND>
static void launchDenoiseLevel(hipStream_t stream, const DevFrame& F, const rt_state& st, const float4* src, float4* dst, int level, int rowBegin, int rowEnd, int gw)
{
  const float sL = IND ? st.sigLuminIndirect : st.sigLuminDirect, sN = IND ? st.sigNormalIndirect : st.sigNormalDirect, sD = IND ? st.sigDepthIndirect : st.sigDepthDirect;
  const int stp = 1 << level, ltx = ((gw + stp - 1) / stp + DL_T - 1) / DL_T, lty = ((rowEnd - rowBegin + stp - 1) / stp + DL_T - 1) / DL_T;
  const unsigned nwg = 8u * unsigned((ltx * lty * stp * stp + 7) / 8);
  if(uniformDivOk(sL) && uniformDivOk(sN) && uniformDivOk(sD))
    hipLaunchKernelGGL((k_denoise_lds<IND, true>), dim3(nwg), dim3(64), 0, stream, F, st, src, dst, level, rowBegin, rowEnd, ltx, lty, 1.0f / sL, 1.0f / sN, 1.0f / sD);
  else
    hipLaunchKernelGGL((k_denoise_lds<IND, false>), dim3(nwg), dim3(64), 0, stream, F, st, src, dst, level, rowBegin, rowEnd, ltx, lty, 0.f, 0.f, 0.f);
}

hipError_t launchIndTileOrder(hipStream_t stream, const rt_state& st, int rowBegin, int tilesX, int tilesY, int cap, uint32_t* lists, uint32_t* counts)
{
  hipLaunchKernelGGL(k_ind_tile_order, dim3(8), dim3(256), 0, stream, st, rowBegin, tilesX, tilesY, cap, lists, counts);
  return hipGetLastError();
}

hipError_t launchFilterStage(hipStream_t stream, const DevFrame& F, const rt_state& st, const rt_scene_camera& cam, int stage, int level, int rowBegin, int rowEnd)
{
  const bool half = stage == RT_STAGE_DENOISE_INDIRECT;
  const int gw = half ? st.size.x / 2 : st.size.x, gh = half ? st.size.y / 2 : st.size.y;
  if(rowEnd <= 0 || rowEnd > gh) rowEnd = gh;
  if(rowBegin < 0) rowBegin = 0;
  if(rowBegin >= rowEnd || gw <= 0) return hipSuccess;
  const int tilesX = (gw + 7) / 8, tilesY = (rowEnd - rowBegin + 7) / 8;
  const dim3 grid(tileGrid(tilesX, tilesY)), block(64);
  switch(stage) {
    case RT_STAGE_DENOISE_DIRECT: {
      // DirectResult -> DirA -> DirB -> DirA -> DirectResult (denoise_direct.comp:152-172)
      const float4* src[4] = {F.thisDirectResult, F.denoiseDirA, F.denoiseDirB, F.denoiseDirA};
      float4* dst[4] = {F.denoiseDirA, F.denoiseDirB, F.denoiseDirA, F.thisDirectResult};
      if(level < 0 || level > 3) return hipErrorInvalidValue;
      if(level == 0) {  // decode the band's geometry plus the halo rows the widest level (2*2^3) will tap
        const int g0 = std::max(0, rowBegin - 16) & ~7, g1 = std::min(gh, rowEnd + 16);
        const int gty = (g1 - g0 + 7) / 8;
        hipLaunchKernelGGL(k_denoise_geom<false>, dim3(tileGrid(tilesX, gty)), block, 0, stream, F, st, cam, g0, g1, tilesX, gty);
      }
      launchDenoiseLevel<false>(stream, F, st, src[level], dst[level], level, rowBegin, rowEnd, gw);
      break;
    }
    case RT_STAGE_DENOISE_INDIRECT: {
      // IndA -> IndB -> IndA -> thisIndirectResult (scratch) -> IndA -> IndB (denoise_indirect.comp:146-171)
      if(st.denoise == 0) return hipSuccess;
      const float4* src[5] = {F.denoiseIndA, F.denoiseIndB, F.denoiseIndA, F.thisIndirectResult, F.denoiseIndA};
      float4* dst[5] = {F.denoiseIndB, F.denoiseIndA, F.thisIndirectResult, F.denoiseIndA, F.denoiseIndB};
      if(level < 0 || level > 4) return hipErrorInvalidValue;
      if(level == 0) {  // halo = 2*2^4 half-res rows
        const int g0 = std::max(0, rowBegin - 32) & ~7, g1 = std::min(gh, rowEnd + 32);
        const int gty = (g1 - g0 + 7) / 8;
        hipLaunchKernelGGL(k_denoise_geom<true>, dim3(tileGrid(tilesX, gty)), block, 0, stream, F, st, cam, g0, g1, tilesX, gty);
      }
      launchDenoiseLevel<true>(stream, F, st, src[level], dst[level], level, rowBegin, rowEnd, gw);
      break;
    }
    case RT_STAGE_COMPOSE: hipLaunchKernelGGL(k_compose, grid, block, 0, stream, F, st, rowBegin, rowEnd, tilesX, tilesY); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rt

// env_accel.h — THE statement of the environment map's importance table (rt_impt_samp {alias, q, pdf, aliasPdf} per texel), for the host (rt_env_accel) and for
// the device (csrc/env_accel.hip, rt_set_environment with accel == NULL).  "The environment" in include/rt_abi.h, DESIGN.md §33.  No dependency on the context;
// host and device compile the same expressions.
//
// The rule.  n = w h <= 2^23 texels, texel i in row y.
//   1. mx_i = max(r, max(g, b)) as std::max orders it; imp_i = area[y] * mx_i in fp32 where mx_i > 0 and the product > 0, else 0 (NaN, negative, zero).  area[y]
//      comes from the host (envRowAreas: the expressions of HdrSampling::createEnvironmentAccel; the device's cos is not the host's).  lum_i = luminance(r, g, b),
//      0 where it is not > 0.  A texel with +inf in r, g or b, or whose imp or lum overflows to +inf, refuses the whole map.
//   2. M = max imp_i.  M == 0: the identity table (alias = i, q = 1, pdf = aliasPdf = 0), integral 0; it falls out of the steps below with every W = 0 and
//      every texel large, the pdf being 0 where the integral is.
//   3. e = envScaleExp(M): M 2^e in [2^39, 2^40).  W_i = imp_i 2^e rounded to nearest even, an integer below 2^40 (envQuantise: integer shifts of the float's
//      bits).  T = sum W_i < 2^63.  integral = float(double(T) 2^-e).
//   4. i is small when n W_i < T, else large.  In index order the smalls have deficits d = T - n W (0 < d <= T), the larges excesses x = n W - T; Di is the
//      inclusive prefix sum of d over the smalls (Dx = Di - d the exclusive one), E the inclusive prefix sum of x over the larges.  128-bit sums (EnvU128).
//   5. small k: alias = the first large j with E[j] >= Dx[k]; q = 1 - (g(Di[k]) - g(Dx[k])) 2^-24, where g(X) = floor((X 2^24 + floor(T / 2)) / T) marks a
//      cumulative amount on the grid of 2^-24 steps (envGrid).
//   6. large j: k* = the first small with Di[k*] > E[j].  None (always so for the last large, as sum d = sum x): q = 1, alias = itself.  Else the overdraft
//      Di[k*] - E[j] lies in (0, T], q = 1 - (g(Di[k*]) - g(E[j])) 2^-24, alias = large j + 1.
//   7. pdf_i = mxc_i * (1.0f / integral) in fp32, mxc = mx where mx > 0 else 0; aliasPdf_i = pdf[alias_i].
//   8. average = float((double(TL) 2^-eL) / double(n)): the luminances quantised and summed as in 3 with their own maximum.
// Every sum is an integer sum: the table does not depend on the order or the shape of whatever adds them up.  The table is exact: texel i is drawn with
// probability (q_i + sum over k with alias_k = i of (1 - q_k)) / n; in grid steps that sum telescopes to 2^24 + g(E[j]) - g(E[j-1]) for large j, whatever the number
// of smalls that alias to it, and is 2^24 - (g(Di[k]) - g(Dx[k])) for small k: within one step of 2^-24 of n W_i / T (q rounded per texel in fp32 would let the
// errors of thousands of smalls add up on one large).
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "../../include/rt_abi.h"
#include "../../include/rt_detmath.h"

namespace rt {

enum : uint32_t { ENV_MAX_TEXELS = 1u << 23 };

struct EnvU128 { uint64_t lo, hi; };
RT_HD EnvU128 envU128(uint64_t v) { EnvU128 r; r.lo = v; r.hi = 0; return r; }
RT_HD EnvU128 envAdd(EnvU128 a, EnvU128 b) { EnvU128 r; r.lo = a.lo + b.lo; r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u); return r; }
RT_HD EnvU128 envSub(EnvU128 a, EnvU128 b) { EnvU128 r; r.lo = a.lo - b.lo; r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u); return r; }
RT_HD bool envLess(EnvU128 a, EnvU128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

RT_HD uint32_t envFloatBits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
RT_HD bool envIsPosInf(float v) { return envFloatBits(v) == 0x7f800000u; }

// step 1 for one texel.  false: the texel refuses the map.
RT_HD bool envTexel(float area, float r, float g, float b, float& imp, float& mxc, float& lum)
{
  const float gb = g < b ? b : g;            // std::max(g, b)
  const float mx = r < gb ? gb : r;          // std::max(r, std::max(g, b))
  const float v = area * mx;
  mxc = mx > 0.0f ? mx : 0.0f;
  imp = (mx > 0.0f && v > 0.0f) ? v : 0.0f;
  const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;   // luminance()
  lum = l > 0.0f ? l : 0.0f;
  return !(envIsPosInf(r) || envIsPosInf(g) || envIsPosInf(b) || envIsPosInf(imp) || envIsPosInf(lum));   // (std::max lets a NaN in r hide an inf in g: each channel is asked)
}

// step 3: the e with M 2^e in [2^39, 2^40), for a finite M > 0 (subnormals included)
RT_HD int envScaleExp(float M)
{
  const uint32_t u = envFloatBits(M), eb = (u >> 23) & 0xffu, m = u & 0x7fffffu;
  if(eb != 0u) return 39 - (int(eb) - 127);                // M in [2^(eb-127), 2^(eb-126))
  int p = 0;                                                // M = m 2^-149, highest set bit p
  for(uint32_t t = m; t > 1u; t >>= 1) p++;
  return 39 - (p - 149);
}
// v 2^e rounded to nearest even, for 0 <= v <= M finite and e = envScaleExp(M): below 2^40
RT_HD uint64_t envQuantise(float v, int e)
{
  const uint32_t u = envFloatBits(v), eb = (u >> 23) & 0xffu;
  const uint64_t m = eb ? uint64_t((u & 0x7fffffu) | 0x800000u) : uint64_t(u & 0x7fffffu);   // v = m 2^(max(eb, 1) - 150)
  const int s = int(eb ? eb : 1u) - 150 + e;
  if(m == 0u) return 0u;
  if(s >= 0) return s < 40 ? m << s : 0u;                    // (s <= 39 as v 2^e < 2^40; the guard keeps the shift defined for any input)
  const int rs = -s;
  if(rs > 25) return 0u;                                     // m < 2^24: below one half
  const uint64_t q = m >> rs, rem = m & ((uint64_t(1) << rs) - 1u), half = uint64_t(1) << (rs - 1);
  return q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
}
// double(T) 2^-e, exact: the power of two is built from its bits (|e| <= 190)
RT_HD double envUnscale(uint64_t T, int e)
{
  const uint64_t bits = uint64_t(1023 - e) << 52;
  double p; __builtin_memcpy(&p, &bits, 8);
  return double(T) * p;
}
RT_HD bool envIsSmall(uint64_t W, uint32_t n, uint64_t T) { return uint64_t(n) * W < T; }
RT_HD float envPdf(float mxc, float integral) { return integral > 0.0f ? mxc * (1.0f / integral) : 0.0f; }

// steps 5 and 6: q lives on the grid of multiples of 2^-24 (every one of them in [0, 1] is an fp32 number).  envGrid(X, T) = floor((X 2^24 + floor(T / 2)) / T):
// a cumulative deficit or excess X (< 2^87) in grid steps, rounded.  It is monotone in X, and envGrid(X + t T, T) = envGrid(X, T) + t 2^24 for an integer t: the two
// facts the exactness argument in DESIGN.md section 33 needs.  The division is the schoolbook one with two 32-bit digits (Knuth D for a 128-bit numerator whose
// high word is below the divisor): the numerator's high word is below T because X <= n T and n <= 2^23; anything else returns all ones and the caller clamps.
enum : uint32_t { ENV_GRID = 1u << 24 };
RT_HD uint64_t envGrid(EnvU128 X, uint64_t T)
{
  uint64_t u1 = (X.hi << 24) | (X.lo >> 40), u0 = X.lo << 24;
  const uint64_t half = T >> 1, b = uint64_t(1) << 32;
  u0 += half; u1 += u0 < half ? 1u : 0u;
  if(T == 0u || u1 >= T) return ~uint64_t(0);
  const int s = __builtin_clzll(T);                          // normalise: the divisor's top bit set
  const uint64_t v = T << s, vn1 = v >> 32, vn0 = v & 0xffffffffu;
  const uint64_t un32 = s ? (u1 << s) | (u0 >> (64 - s)) : u1, un10 = u0 << s, un1 = un10 >> 32, un0 = un10 & 0xffffffffu;
  uint64_t q1 = un32 / vn1, rhat = un32 - q1 * vn1;
  while(q1 >= b || q1 * vn0 > b * rhat + un1) { q1--; rhat += vn1; if(rhat >= b) break; }
  const uint64_t un21 = un32 * b + un1 - q1 * v;
  uint64_t q0 = un21 / vn1;
  rhat = un21 - q0 * vn1;
  while(q0 >= b || q0 * vn0 > b * rhat + un0) { q0--; rhat += vn1; if(rhat >= b) break; }
  return q1 * b + q0;
}
// a number of grid steps taken from a full bucket: q = (2^24 - steps) 2^-24, exact in fp32
RT_HD float envGridQ(uint64_t steps) { return float(uint32_t(ENV_GRID - (steps < ENV_GRID ? uint32_t(steps) : ENV_GRID))) * 5.9604644775390625e-8f; }

// steps 5 and 6 for rank r of the compacted order: ranks [0, S) are the smalls in index order, [S, n) the larges; idx[r] is the texel, P[r] its inclusive prefix
// (Di for a small, E for a large).  Writes alias and q of texel idx[r].
RT_HD void envAssign(uint32_t r, uint32_t S, uint32_t n, uint64_t T, const EnvU128* P, const uint32_t* idx, const uint64_t* W, int32_t& alias, float& q)
{
  const uint32_t i = idx[r];
  if(r < S) {
    const EnvU128 Dx = envSub(P[r], envU128(T - uint64_t(n) * W[i]));
    uint32_t lo = S, hi = n;                                 // the first large with E >= Dx: one exists, as Dx < sum d = E[last]
    while(lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if(envLess(P[mid], Dx)) lo = mid + 1u; else hi = mid; }
    if(lo >= n) lo = n - 1u;                                 // never: keeps the index inside the arrays whatever P holds
    alias = int32_t(idx[lo]);
    q = envGridQ(envGrid(P[r], T) - envGrid(Dx, T));         // what the small gives away: its deficit between two rounded marks of the cumulative deficit
    return;
  }
  const EnvU128 E = P[r];
  uint32_t lo = 0, hi = S;                                   // the first small with Di > E
  while(lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if(envLess(E, P[mid])) hi = mid; else lo = mid + 1u; }
  if(lo >= S || r + 1u >= n) { alias = int32_t(i); q = 1.0f; return; }
  alias = int32_t(idx[r + 1u]);
  q = envGridQ(envGrid(P[lo], T) - envGrid(E, T));           // the overdraft, between the marks of Di[k*] and E[j]
}

// ---- host only (plain functions: no device code is made of them) ----
// step 1's row areas, on the host: exactly the expressions of HdrSampling::createEnvironmentAccel (host/hdr_sampling.cpp)
inline void envRowAreas(int w, int h, float* area)
{
  float cosTheta0 = 1.0f;
  const float stepPhi = float(2.0 * M_PI) / float(uint32_t(w));
  const float stepTheta = float(M_PI) / float(uint32_t(h));
  for(uint32_t y = 0; y < uint32_t(h); ++y) {
    const float cosTheta1 = cosf(float(y + 1) * stepTheta);
    area[y] = (cosTheta0 - cosTheta1) * stepPhi;
    cosTheta0 = cosTheta1;
  }
}

struct EnvAccelResult { float integral = 0.f, average = 0.f; uint32_t numSmall = 0, numLarge = 0; };

// The whole rule on the host: out[n].  0, or 1 when a texel refuses the map (out untouched).  impOut (optional, n floats): step 1's importances.
inline int envAccelHost(int w, int h, const float* rgba, rt_impt_samp* out, EnvAccelResult& res, float* impOut = nullptr)
{
  const uint32_t n = uint32_t(w) * uint32_t(h);
  std::vector<float> area(static_cast<size_t>(h)), imp(n), mxc(n), lum(n);
  envRowAreas(w, h, area.data());
  float M = 0.f, ML = 0.f;
  bool ok = true;
  for(uint32_t i = 0; i < n; i++) {
    const float* t = rgba + size_t(i) * 4;
    ok = envTexel(area[i / uint32_t(w)], t[0], t[1], t[2], imp[i], mxc[i], lum[i]) && ok;
    if(imp[i] > M) M = imp[i];
    if(lum[i] > ML) ML = lum[i];
  }
  if(!ok) return 1;
  if(impOut) memcpy(impOut, imp.data(), size_t(n) * 4);
  const int e = envScaleExp(M), eL = envScaleExp(ML);       // (a maximum of 0 gives sums of 0: the identity table falls out of the steps below)
  std::vector<uint64_t> W(n);
  uint64_t T = 0, TL = 0;
  for(uint32_t i = 0; i < n; i++) { W[i] = envQuantise(imp[i], e); T += W[i]; TL += envQuantise(lum[i], eL); }
  res.integral = float(envUnscale(T, e));
  res.average = float(envUnscale(TL, eL) / double(n));
  uint32_t S = 0;
  for(uint32_t i = 0; i < n; i++) if(envIsSmall(W[i], n, T)) S++;
  std::vector<EnvU128> P(n);
  std::vector<uint32_t> idx(n);
  EnvU128 D = envU128(0), E = envU128(0);
  uint32_t ks = 0, kl = S;
  for(uint32_t i = 0; i < n; i++) {
    const uint64_t nW = uint64_t(n) * W[i];
    if(nW < T) { D = envAdd(D, envU128(T - nW)); P[ks] = D; idx[ks++] = i; }
    else { E = envAdd(E, envU128(nW - T)); P[kl] = E; idx[kl++] = i; }
  }
  for(uint32_t r = 0; r < n; r++) envAssign(r, S, n, T, P.data(), idx.data(), W.data(), out[idx[r]].alias, out[idx[r]].q);
  for(uint32_t i = 0; i < n; i++) out[i].pdf = envPdf(mxc[i], res.integral);
  for(uint32_t i = 0; i < n; i++) out[i].aliasPdf = out[size_t(out[i].alias)].pdf;
  res.numSmall = S; res.numLarge = n - S;
  return 0;
}

#if defined(__HIPCC__)
}  // namespace rt
#include <hip/hip_runtime.h>
namespace rt {
// ---- the device build (csrc/env_accel.hip) ----------------------------------------------------------------------------------------------------------------
// the counter words, cleared before the first pass
enum : int { ENV_CNT_MAX_IMP = 0, ENV_CNT_MAX_LUM = 1, ENV_CNT_BAD = 2, ENV_CNT_SMALL = 3, ENV_CNT_T = 4 /* and 5 */, ENV_CNT_TL = 6 /* and 7 */, ENV_CNT_WORDS = 8 };
enum : uint32_t { ENV_SCAN_BLOCK = 256, ENV_SCAN_ITEMS = 4, ENV_SCAN_TILE = ENV_SCAN_BLOCK * ENV_SCAN_ITEMS };
struct EnvBlockSum { EnvU128 d, x; uint32_t small, pad[3]; };   // 48 B: what one scan tile adds to the three prefixes

struct EnvBuildArgs {
  const float* texels;       // n RGBA32F
  const float* area;         // h floats
  rt_impt_samp* accel;       // n: the staging table
  uint64_t* W;               // n
  EnvU128* P;                // n: Di of the smalls at [0, S), E of the larges at [S, n)
  uint32_t* idx;             // n: the texel of every rank
  EnvBlockSum* blockSums;    // ceil(n / ENV_SCAN_TILE)
  uint32_t* counters;        // ENV_CNT_WORDS
  uint32_t n, w;
};
// every pass of the build, in order, on `stream`; nothing is read back
hipError_t launchEnvAccelBuild(hipStream_t stream, const EnvBuildArgs& a);
#endif

}  // namespace rt

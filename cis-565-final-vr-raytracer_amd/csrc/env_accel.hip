// env_accel.hip — the kernels of rt_set_environment's device build (env_accel.h states the rule), compiled once.  Wave64 throughout, 256 threads per
// workgroup, one thread per texel unless noted.  Every cross-workgroup sum is an integer atomic or an integer prefix, so no result depends on the launch shape or
// on the order in which workgroups run.
//   k_env_importance  step 1: importance and luminance per texel, their two maxima (wave shuffle, LDS across the four waves, one atomicMax on the float's bits
//                     per workgroup: the values are >= 0, so the bits order as the floats do) and the refusal flag.
//   k_env_quantise    step 3: W per texel (stored; importance and luminance are computed again from the texel rather than kept) and the two integer sums T
//                     and TL, one 64-bit atomicAdd each per workgroup.
//   k_env_block_sums  step 4, first of three: per scan tile of 1024 texels the number of smalls, the sum of their deficits and the sum of the larges' excesses.
//   k_env_scan_blocks one workgroup: the exclusive prefix of the tile sums, in place; the number of smalls to the counters.
//   k_env_apply       per tile again: the inclusive prefixes inside the tile on top of the tile's offset.  Small number k goes to rank k, large number j to rank
//                     S + j: both compactions are stable (index order), P[rank] is the prefix (Di or E), idx[rank] the texel.
//   k_env_assign      steps 5 and 6, one thread per rank: the two binary searches of envAssign over P and the two grid marks (envGrid) q is the difference of.
//   k_env_pdf         step 7: pdf from the texel, aliasPdf from the alias's texel (the same expression: pdf[alias] bit for bit, without a pass in between).
// Integer, fp32 and double arithmetic in the order env_accel.h writes it; the unit is built with -ffp-contract=off like every other.  Every index is below n by
// construction (ranks are counts of texels below n; alias is idx[] of a rank below n); the assign pass clamps its search result all the same.
#include "env_accel.h"
#include "dev_math.h"

namespace rt {
namespace {

constexpr uint32_t ENV_BLOCK = 256;

__device__ __forceinline__ float waveMax(float v)
{
  for(int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(v, o); v = t > v ? t : v; }
  return v;
}
__device__ __forceinline__ uint64_t waveSum(uint64_t v)
{
  for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_importance(const EnvBuildArgs a)
{
  __shared__ float sImp[ENV_BLOCK / 64], sLum[ENV_BLOCK / 64];
  const uint32_t i = blockIdx.x * ENV_BLOCK + threadIdx.x;
  float imp = 0.f, mxc = 0.f, lum = 0.f;
  bool ok = true;
  if(i < a.n) {
    const float4 t = gLoadF4(a.texels + size_t(i) * 4);
    ok = envTexel(a.area[i / a.w], t.x, t.y, t.z, imp, mxc, lum);
  }
  if(!ok) { imp = 0.f; lum = 0.f; }   // (the map is refused; the maxima stay finite)
  if(__ballot(!ok) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(a.counters + ENV_CNT_BAD, 1u);
  imp = waveMax(imp); lum = waveMax(lum);
  if((threadIdx.x & 63u) == 0u) { sImp[threadIdx.x >> 6] = imp; sLum[threadIdx.x >> 6] = lum; }
  __syncthreads();
  if(threadIdx.x == 0u) {
    for(uint32_t k = 1; k < ENV_BLOCK / 64; k++) { imp = sImp[k] > imp ? sImp[k] : imp; lum = sLum[k] > lum ? sLum[k] : lum; }
    if(imp > 0.f) atomicMax(a.counters + ENV_CNT_MAX_IMP, envFloatBits(imp));
    if(lum > 0.f) atomicMax(a.counters + ENV_CNT_MAX_LUM, envFloatBits(lum));
  }
}

__device__ __forceinline__ float maxOf(const uint32_t* counters, int which) { return __uint_as_float(gLoadU32(counters + which)); }
__device__ __forceinline__ uint64_t sumOf(const uint32_t* counters, int which) { return uint64_t(gLoadU32(counters + which)) | (uint64_t(gLoadU32(counters + which + 1)) << 32); }

__global__ __launch_bounds__(ENV_BLOCK) void k_env_quantise(const EnvBuildArgs a)
{
  __shared__ uint64_t sT[ENV_BLOCK / 64], sL[ENV_BLOCK / 64];
  const uint32_t i = blockIdx.x * ENV_BLOCK + threadIdx.x;
  const int e = envScaleExp(maxOf(a.counters, ENV_CNT_MAX_IMP)), eL = envScaleExp(maxOf(a.counters, ENV_CNT_MAX_LUM));
  uint64_t w = 0, l = 0;
  if(i < a.n) {
    const float4 t = gLoadF4(a.texels + size_t(i) * 4);
    float imp, mxc, lum;
    const bool ok = envTexel(a.area[i / a.w], t.x, t.y, t.z, imp, mxc, lum);
    if(ok) { w = envQuantise(imp, e); l = envQuantise(lum, eL); }
    a.W[i] = w;
  }
  w = waveSum(w); l = waveSum(l);
  if((threadIdx.x & 63u) == 0u) { sT[threadIdx.x >> 6] = w; sL[threadIdx.x >> 6] = l; }
  __syncthreads();
  if(threadIdx.x == 0u) {
    for(uint32_t k = 1; k < ENV_BLOCK / 64; k++) { w += sT[k]; l += sL[k]; }
    if(w) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + ENV_CNT_T), static_cast<unsigned long long>(w));
    if(l) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + ENV_CNT_TL), static_cast<unsigned long long>(l));
  }
}

// what one texel adds to the three prefixes
struct EnvItem { EnvU128 d, x; uint32_t small; };
__device__ __forceinline__ EnvItem itemZero() { EnvItem r; r.d = envU128(0); r.x = envU128(0); r.small = 0; return r; }
__device__ __forceinline__ EnvItem itemAdd(const EnvItem& p, const EnvItem& q) { EnvItem r; r.d = envAdd(p.d, q.d); r.x = envAdd(p.x, q.x); r.small = p.small + q.small; return r; }
__device__ __forceinline__ EnvItem itemOf(const EnvBuildArgs& a, uint32_t i, uint64_t T)
{
  EnvItem r = itemZero();
  if(i < a.n) {
    const uint64_t nW = uint64_t(a.n) * a.W[i];
    if(nW < T) { r.d = envU128(T - nW); r.small = 1; }
    else r.x = envU128(nW - T);
  }
  return r;
}

// the inclusive prefix of one value per thread over the workgroup (Hillis-Steele in LDS: eight steps of 256 threads; the sums are integers, any order gives the same)
__device__ __forceinline__ EnvItem blockScanInclusive(EnvItem v, EnvItem* s)
{
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for(uint32_t o = 1; o < ENV_SCAN_BLOCK; o <<= 1) {
    EnvItem u = itemZero();
    if(t >= o) u = s[t - o];
    __syncthreads();
    if(t >= o) { v = itemAdd(u, v); s[t] = v; }
    __syncthreads();
  }
  return v;
}

__global__ __launch_bounds__(ENV_SCAN_BLOCK) void k_env_block_sums(const EnvBuildArgs a)
{
  __shared__ EnvItem s[ENV_SCAN_BLOCK];
  const uint64_t T = sumOf(a.counters, ENV_CNT_T);
  const uint32_t first = blockIdx.x * ENV_SCAN_TILE + threadIdx.x * ENV_SCAN_ITEMS;
  EnvItem v = itemZero();
  for(uint32_t k = 0; k < ENV_SCAN_ITEMS; k++) v = itemAdd(v, itemOf(a, first + k, T));
  v = blockScanInclusive(v, s);
  if(threadIdx.x == ENV_SCAN_BLOCK - 1u) {
    EnvBlockSum b; b.d = v.d; b.x = v.x; b.small = v.small; b.pad[0] = b.pad[1] = b.pad[2] = 0;
    a.blockSums[blockIdx.x] = b;
  }
}

__global__ __launch_bounds__(ENV_SCAN_BLOCK) void k_env_scan_blocks(const EnvBuildArgs a, uint32_t numTiles)
{
  __shared__ EnvItem s[ENV_SCAN_BLOCK];
  const uint32_t per = (numTiles + ENV_SCAN_BLOCK - 1u) / ENV_SCAN_BLOCK;
  const uint32_t b0 = threadIdx.x * per, b1 = b0 + per < numTiles ? b0 + per : numTiles;
  EnvItem v = itemZero();
  for(uint32_t b = b0; b < b1; b++) { const EnvBlockSum x = a.blockSums[b]; EnvItem u; u.d = x.d; u.x = x.x; u.small = x.small; v = itemAdd(v, u); }
  const EnvItem incl = blockScanInclusive(v, s);
  // exclusive prefix of this thread's first tile = the inclusive prefix of the thread before
  EnvItem run = threadIdx.x ? s[threadIdx.x - 1u] : itemZero();
  for(uint32_t b = b0; b < b1; b++) {
    const EnvBlockSum x = a.blockSums[b];
    EnvBlockSum o; o.d = run.d; o.x = run.x; o.small = run.small; o.pad[0] = o.pad[1] = o.pad[2] = 0;
    a.blockSums[b] = o;
    EnvItem u; u.d = x.d; u.x = x.x; u.small = x.small;
    run = itemAdd(run, u);
  }
  if(threadIdx.x == ENV_SCAN_BLOCK - 1u) a.counters[ENV_CNT_SMALL] = incl.small;
}

__global__ __launch_bounds__(ENV_SCAN_BLOCK) void k_env_apply(const EnvBuildArgs a)
{
  __shared__ EnvItem s[ENV_SCAN_BLOCK];
  const uint64_t T = sumOf(a.counters, ENV_CNT_T);
  const uint32_t S = gLoadU32(a.counters + ENV_CNT_SMALL);
  const uint32_t first = blockIdx.x * ENV_SCAN_TILE + threadIdx.x * ENV_SCAN_ITEMS;
  EnvItem it[ENV_SCAN_ITEMS];
  EnvItem v = itemZero();
  for(uint32_t k = 0; k < ENV_SCAN_ITEMS; k++) { it[k] = itemOf(a, first + k, T); v = itemAdd(v, it[k]); }
  const EnvItem incl = blockScanInclusive(v, s);
  const EnvBlockSum base = a.blockSums[blockIdx.x];
  EnvItem run; run.d = base.d; run.x = base.x; run.small = base.small;
  if(threadIdx.x) run = itemAdd(run, s[threadIdx.x - 1u]);
  (void)incl;
  for(uint32_t k = 0; k < ENV_SCAN_ITEMS; k++) {
    const uint32_t i = first + k;
    if(i >= a.n) break;
    const uint32_t smallsBefore = run.small;
    run = itemAdd(run, it[k]);
    // small number `smallsBefore` -> rank smallsBefore; large number i - smallsBefore -> rank S + that.  Both < n: S counts the smalls of all n texels.
    const uint32_t rank = it[k].small ? smallsBefore : S + (i - smallsBefore);
    if(rank < a.n) { a.P[rank] = it[k].small ? run.d : run.x; a.idx[rank] = i; }
  }
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_assign(const EnvBuildArgs a)
{
  const uint32_t r = blockIdx.x * ENV_BLOCK + threadIdx.x;
  if(r >= a.n) return;
  const uint64_t T = sumOf(a.counters, ENV_CNT_T);
  uint32_t S = gLoadU32(a.counters + ENV_CNT_SMALL);
  if(S > a.n) S = a.n;
  const uint32_t i = a.idx[r];
  if(i >= a.n) return;
  int32_t alias; float q;
  envAssign(r, S, a.n, T, a.P, a.idx, a.W, alias, q);
  if(uint32_t(alias) >= a.n) alias = int32_t(i);   // never: an alias outside the table must not reach the shaders
  a.accel[i].alias = alias;
  a.accel[i].q = q;
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_pdf(const EnvBuildArgs a)
{
  const uint32_t i = blockIdx.x * ENV_BLOCK + threadIdx.x;
  if(i >= a.n) return;
  const int e = envScaleExp(maxOf(a.counters, ENV_CNT_MAX_IMP));
  const float integral = float(envUnscale(sumOf(a.counters, ENV_CNT_T), e));
  uint32_t j = uint32_t(a.accel[i].alias);
  if(j >= a.n) j = i;
  float imp, mxc, lum;
  const float4 t = gLoadF4(a.texels + size_t(i) * 4);
  (void)envTexel(0.f, t.x, t.y, t.z, imp, mxc, lum);
  a.accel[i].pdf = envPdf(mxc, integral);
  const float4 u = gLoadF4(a.texels + size_t(j) * 4);
  (void)envTexel(0.f, u.x, u.y, u.z, imp, mxc, lum);
  a.accel[i].aliasPdf = envPdf(mxc, integral);
}

}  // namespace

hipError_t launchEnvAccelBuild(hipStream_t stream, const EnvBuildArgs& a)
{
  if(a.n == 0u || a.w == 0u || a.n > ENV_MAX_TEXELS) return hipErrorInvalidValue;
  const uint32_t blocks = (a.n + ENV_BLOCK - 1u) / ENV_BLOCK, tiles = (a.n + ENV_SCAN_TILE - 1u) / ENV_SCAN_TILE;
  hipLaunchKernelGGL(k_env_importance, dim3(blocks), dim3(ENV_BLOCK), 0, stream, a);
  hipLaunchKernelGGL(k_env_quantise, dim3(blocks), dim3(ENV_BLOCK), 0, stream, a);
  hipLaunchKernelGGL(k_env_block_sums, dim3(tiles), dim3(ENV_SCAN_BLOCK), 0, stream, a);
  hipLaunchKernelGGL(k_env_scan_blocks, dim3(1), dim3(ENV_SCAN_BLOCK), 0, stream, a, tiles);
  hipLaunchKernelGGL(k_env_apply, dim3(tiles), dim3(ENV_SCAN_BLOCK), 0, stream, a);
  hipLaunchKernelGGL(k_env_assign, dim3(blocks), dim3(ENV_BLOCK), 0, stream, a);
  hipLaunchKernelGGL(k_env_pdf, dim3(blocks), dim3(ENV_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rt

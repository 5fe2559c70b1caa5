// morph.hip — the kernel of rt_update_morphs (include/rt_abi.h "Morph targets"), compiled once.
//   k_morph   one thread per vertex of the listed sets: rest row + w_a * delta row of every ACTIVE target, in ascending target index -> staged row.  The host builds
//             the active list (weight != 0), so a target that is off costs nothing and the kernel never multiplies by zero.  The delta array is target-major: the
//             lanes of a wave read consecutive 16-byte rows of one plane of one target.  A job starts at a multiple of 64 threads, so the trip count of the loop over
//             the active list is the same for every lane of a wave.  Non-finite positions are counted into the counter k_skin uses: the host commits a pose only
//             when it stayed zero.
// It reads planes x 16 B x active targets per vertex; at the mesh sizes measured it is bound by the latency of the loop's loads, not by those bytes (DESIGN.md
// §23), hence four targets per trip.  tests/morph_checker.cpp restates the arithmetic in plain C++; its order is stated in include/rt_abi.h.
#include "morph.h"
#include "shading.h"

namespace rt {
namespace {

constexpr int MORPH_BLOCK = 256;
constexpr int MORPH_BATCH = 4;      // targets whose rows are loaded together

__device__ __forceinline__ void gStoreU4(void* p, uint4 v) { u32x4_t w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; *(RT_AS_GLOBAL u32x4_t*)p = w; }

// the job a thread belongs to: the last one whose threadBase is <= t (the search of csrc/deform.hip, restated: that translation unit stays as it is)
__device__ __forceinline__ uint32_t jobOf(const MorphJob* jobs, uint32_t numJobs, uint32_t t)
{
  uint32_t lo = 0, hi = numJobs;
  while(hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if(gLoadU32(jobs + mid) <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// normalize(v) packed, or the rest pose's value where v has no direction (the rule of rt_update_skins)
__device__ __forceinline__ uint32_t packDirection(f3 v, uint32_t restPacked)
{
  const float d = (v.x * v.x + v.y * v.y) + v.z * v.z;
  const float inv = 1.0f / rt_sqrt(d);
  if(!(d > 0.0f) || rt_isinf(d) || rt_isinf(inv)) return restPacked;
  return compress_unit_vec(mk3(v.x * inv, v.y * inv, v.z * inv));
}

__global__ __launch_bounds__(MORPH_BLOCK) void k_morph(const MorphArgs a)
{
  const uint32_t t = blockIdx.x * MORPH_BLOCK + threadIdx.x;
  bool bad = false;
  if(t < a.numThreads) {
    const MorphJob* job = a.jobs + jobOf(a.jobs, a.numJobs, t);
    const uint4 j0 = gLoadU4(job);                                           // threadBase, count, restFirst, firstDelta
    const uint4 j1 = gLoadU4(reinterpret_cast<const uint4*>(job) + 1);       // firstActive, numActive, planes, pool
    const uint32_t v = t - j0.x;
    if(v < j0.y) {
      const rt_vertex* src = (j1.w ? a.rest1 : a.rest0) + j0.z + v;
      rt_vertex* dst = (j1.w ? a.staged1 : a.staged0) + j0.z + v;
      const float4 r0 = gLoadF4(src);                                        // position.xyz, normal bits
      const uint4 r1 = gLoadU4(reinterpret_cast<const uint4*>(src) + 1);     // texcoord.xy, tangent bits, colour
      float px = r0.x, py = r0.y, pz = r0.z;
      uint32_t nrm = __float_as_uint(r0.w), tng = r1.z;
      const bool hasN = (j1.z & RT_MORPH_NORMALS) != 0u, hasT = (j1.z & RT_MORPH_TANGENTS) != 0u;
      const bool doN = hasN && j1.y != 0u && nrm != 0xffffffffu, doT = hasT && j1.y != 0u && tng != 0xffffffffu;
      f3 n = mk3(0.0f), u = mk3(0.0f);
      if(doN) n = decompress_unit_vec(nrm);
      if(doT) u = decompress_unit_vec(tng);
      const size_t V = j0.y, planeRows = size_t(1u + (hasN ? 1u : 0u) + (hasT ? 1u : 0u)) * V;
      const rt_morph_delta* mine = a.deltas + j0.w + v;
      const MorphActive* act = a.active + j1.x;
      // Four targets per trip (wave-uniform trip count): the pairs, then every delta row of the four, are in flight together before the sums, which stay in
      // ascending target order.  One target per trip measured one memory latency per target.  A trip's unused slots re-read its first pair and are not summed.
      for(uint32_t k = 0; k < j1.y; k += MORPH_BATCH) {
        const uint32_t live = min(j1.y - k, uint32_t(MORPH_BATCH));
        uint2 tw[MORPH_BATCH];
        float4 dp[MORPH_BATCH], dn[MORPH_BATCH], dt[MORPH_BATCH];
#pragma unroll
        for(uint32_t i = 0; i < MORPH_BATCH; i++) tw[i] = gLoadU2(act + k + (i < live ? i : 0u));
#pragma unroll
        for(uint32_t i = 0; i < MORPH_BATCH; i++) {
          const rt_morph_delta* row = mine + size_t(tw[i].x) * planeRows;
          dp[i] = gLoadF4(row);
          dn[i] = doN ? gLoadF4(row + V) : make_float4(0.f, 0.f, 0.f, 0.f);
          dt[i] = doT ? gLoadF4(row + (hasN ? 2 * V : V)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for(uint32_t i = 0; i < MORPH_BATCH; i++) {
          if(i >= live) break;
          const float w = __uint_as_float(tw[i].y);
          px = px + w * dp[i].x; py = py + w * dp[i].y; pz = pz + w * dp[i].z;   // each product is rounded before its add (no contraction)
          if(doN) { n.x = n.x + w * dn[i].x; n.y = n.y + w * dn[i].y; n.z = n.z + w * dn[i].z; }
          if(doT) { u.x = u.x + w * dt[i].x; u.y = u.y + w * dt[i].y; u.z = u.z + w * dt[i].z; }
        }
      }
      bad = rt_isnan(px) || rt_isinf(px) || rt_isnan(py) || rt_isinf(py) || rt_isnan(pz) || rt_isinf(pz);
      if(doN) nrm = packDirection(n, nrm);
      if(doT) tng = packDirection(u, tng);
      gStoreU4(dst, make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), nrm));
      gStoreU4(reinterpret_cast<uint4*>(dst) + 1, make_uint4(r1.x, r1.y, tng, r1.w));
    }
  }
  const unsigned long long m = __ballot(bad);
  if((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(a.nonFinite, uint32_t(__popcll(m)));
}

}  // namespace

hipError_t launchMorph(hipStream_t stream, const MorphArgs& a)
{
  if(a.numThreads == 0) return hipSuccess;
  hipLaunchKernelGGL(k_morph, dim3((a.numThreads + MORPH_BLOCK - 1) / MORPH_BLOCK), dim3(MORPH_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rt

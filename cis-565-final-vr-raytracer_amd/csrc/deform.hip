// deform.hip — the two kernels of rt_update_skins / rt_update_vertices (include/rt_abi.h "Deforming meshes"), compiled once.
//   k_skin            one thread per vertex of the listed skins: rest row + influence row -> blend matrix -> staged row.  A pose is committed to the live vertex array
//                     by the host (a copy on the stream) only when no staged position is non-finite; the lanes that produced one are counted here.
//   k_inst_coord_max  one thread per (instance whose mesh deformed, index entry): the largest |world coordinate| of the instance, the number the hit rule's pad is
//                     a reduction of — the builder's expression that instanceCoordMax (csrc/rt_api.cpp) restates on the host.
// Both are bound by gathers, not arithmetic: 256 threads per workgroup, rows read and written as 16-byte (influences: 8-byte) vectors, joint matrices gathered as
// float4 rows (they differ per lane).  Every hand-off (skin -> commit copy -> coordinate maximum -> refit) crosses a kernel boundary on one stream.
// tests/skin_checker.cpp restates k_skin in plain C++; the arithmetic and its order are stated in include/rt_abi.h.
#include "deform.h"
#include "shading.h"

namespace rt {
namespace {

constexpr int DEFORM_BLOCK = 256;

__device__ __forceinline__ void gStoreU4(void* p, uint4 v) { u32x4_t w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; *(RT_AS_GLOBAL u32x4_t*)p = w; }

// the job a thread belongs to: the last one whose threadBase is <= t (threadBase is the first word of both job records, 32 B apart)
__device__ __forceinline__ uint32_t jobOf(const void* jobs, uint32_t numJobs, uint32_t t)
{
  uint32_t lo = 0, hi = numJobs;
  while(hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if(gLoadU32(static_cast<const char*>(jobs) + size_t(mid) * 32) <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// normalize(v) packed, or the rest pose's value where v has no direction (zero length, not finite, or a length whose reciprocal is not finite)
__device__ __forceinline__ uint32_t packDirection(f3 v, uint32_t restPacked)
{
  const float d = dot(v, v);
  const float inv = 1.0f / rt_sqrt(d);
  if(!(d > 0.0f) || rt_isinf(d) || rt_isinf(inv)) return restPacked;
  return compress_unit_vec(v * inv);
}

__global__ __launch_bounds__(DEFORM_BLOCK) void k_skin(const SkinArgs a)
{
  const uint32_t t = blockIdx.x * DEFORM_BLOCK + threadIdx.x;
  bool bad = false;
  if(t < a.numThreads) {
    const SkinJob* job = a.jobs + jobOf(a.jobs, a.numJobs, t);
    const uint4 j0 = gLoadU4(job);             // threadBase, count, restFirst, firstInfluence
    const uint32_t firstJoint = gLoadU32(&job->firstJoint);
    const uint32_t v = t - j0.x;
    if(v < j0.y) {
      const rt_vertex* src = a.rest + j0.z + v;
      const float4 r0 = gLoadF4(src);                                              // position.xyz, normal bits
      const uint4 r1 = gLoadU4(reinterpret_cast<const uint4*>(src) + 1);           // texcoord.xy, tangent bits, colour
      const uint2* inf = reinterpret_cast<const uint2*>(a.influences + j0.w + v);  // 24 B: joint[4] u16, weight[4]
      const uint2 jj = gLoadU2(inf), w01 = gLoadU2(inf + 1), w23 = gLoadU2(inf + 2);
      const uint32_t joint[4] = {jj.x & 0xffffu, jj.x >> 16, jj.y & 0xffffu, jj.y >> 16};
      const float w[4] = {__uint_as_float(w01.x), __uint_as_float(w01.y), __uint_as_float(w23.x), __uint_as_float(w23.y)};
      // B = ((w0 M[j0] + w1 M[j1]) + w2 M[j2]) + w3 M[j3], entry by entry; zero weights are not skipped
      float B[12];
      for(int k = 0; k < 4; k++) {
        const float* M = a.joints + size_t(firstJoint + joint[k]) * 12;
        for(int r = 0; r < 3; r++) {
          const float4 row = gLoadF4(M + 4 * r);
          const float p[4] = {w[k] * row.x, w[k] * row.y, w[k] * row.z, w[k] * row.w};
          for(int c = 0; c < 4; c++) B[4 * r + c] = k == 0 ? p[c] : B[4 * r + c] + p[c];
        }
      }
      float pos[3];
      xformPointRaw(B, r0.x, r0.y, r0.z, pos);
      bad = rt_isnan(pos[0]) || rt_isinf(pos[0]) || rt_isnan(pos[1]) || rt_isinf(pos[1]) || rt_isnan(pos[2]) || rt_isinf(pos[2]);
      // normal: sign(det B3) cof(B3) n; tangent: B3 t
      uint32_t nrm = __float_as_uint(r0.w), tng = r1.z;
      if(nrm != 0xffffffffu) {
        const float A = B[0], Bb = B[1], Cc = B[2], D = B[4], E = B[5], F = B[6], G = B[8], H = B[9], I = B[10];
        const float c00 = E * I - F * H, c01 = F * G - D * I, c02 = D * H - E * G;
        const float c10 = Cc * H - Bb * I, c11 = A * I - Cc * G, c12 = Bb * G - A * H;
        const float c20 = Bb * F - Cc * E, c21 = Cc * D - A * F, c22 = A * E - Bb * D;
        const float det = (A * c00 + Bb * c01) + Cc * c02;
        const float s = det < 0.0f ? -1.0f : 1.0f;
        const f3 n = decompress_unit_vec(nrm);
        const f3 m = mk3(s * ((c00 * n.x + c01 * n.y) + c02 * n.z), s * ((c10 * n.x + c11 * n.y) + c12 * n.z), s * ((c20 * n.x + c21 * n.y) + c22 * n.z));
        nrm = packDirection(m, nrm);
      }
      if(tng != 0xffffffffu) tng = packDirection(xformDir(B, decompress_unit_vec(tng)), tng);
      rt_vertex* dst = a.staged + j0.z + v;
      gStoreU4(dst, make_uint4(__float_as_uint(pos[0]), __float_as_uint(pos[1]), __float_as_uint(pos[2]), nrm));
      gStoreU4(reinterpret_cast<uint4*>(dst) + 1, make_uint4(r1.x, r1.y, tng, r1.w));
    }
  }
  const unsigned long long m = __ballot(bad);
  if((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(a.nonFinite, uint32_t(__popcll(m)));
}

__global__ __launch_bounds__(DEFORM_BLOCK) void k_inst_coord_max(const CoordMaxArgs a)
{
  const uint32_t t = blockIdx.x * DEFORM_BLOCK + threadIdx.x;
  uint32_t bits = 0u, jobIdx = 0u;
  if(t < a.numThreads) {
    jobIdx = jobOf(a.jobs, a.numJobs, t);
    const CoordJob* job = a.jobs + jobIdx;
    const uint4 j0 = gLoadU4(job);             // threadBase, indexCount, firstIndex, vertexBase
    const uint32_t k = t - j0.x;
    if(k < j0.y) {
      const DevInstance* di = a.instances + gLoadU32(&job->instance);
      float m[12];
      for(int r = 0; r < 3; r++) { const float4 row = gLoadF4(di->o2w + 4 * r); m[4 * r] = row.x; m[4 * r + 1] = row.y; m[4 * r + 2] = row.z; m[4 * r + 3] = row.w; }
      const float4 p = gLoadF4(a.vertices + j0.w + gLoadU32(a.indices + j0.z + k));
      float w[3];
      xformPointRaw(m, p.x, p.y, p.z, w);
      // |x| >= 0: the order of the bits as unsigned integers is the order of the floats, so the maximum is exact and independent of the order it is taken in
      bits = max(max(__float_as_uint(rt_abs(w[0])), __float_as_uint(rt_abs(w[1]))), __float_as_uint(rt_abs(w[2])));
    }
  }
  // a wave never spans two jobs (threadBase is a multiple of 64): reduce across it, one atomic per wave
  for(int off = 32; off > 0; off >>= 1) bits = max(bits, uint32_t(__shfl_xor(int(bits), off, 64)));
  if((threadIdx.x & 63u) == 0u && bits != 0u) atomicMax(a.out + jobIdx, bits);
}

}  // namespace

hipError_t launchSkin(hipStream_t stream, const SkinArgs& a)
{
  if(a.numThreads == 0) return hipSuccess;
  hipLaunchKernelGGL(k_skin, dim3((a.numThreads + DEFORM_BLOCK - 1) / DEFORM_BLOCK), dim3(DEFORM_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launchInstCoordMax(hipStream_t stream, const CoordMaxArgs& a)
{
  if(a.numThreads == 0) return hipSuccess;
  hipLaunchKernelGGL(k_inst_coord_max, dim3((a.numThreads + DEFORM_BLOCK - 1) / DEFORM_BLOCK), dim3(DEFORM_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rt

// light_derive.hip — the kernel of rt_set_emitter_meshes (include/rt_abi.h "Emitters"), compiled once.
//   k_light_expand    one thread per derived triangle-light record k: the emitting instance of k by an upper-bound binary search in the prefix words (an instance's
//                     records are contiguous in k, so the lanes of a wave walk the same few words, as in k_expand_instances), then the template row of
//                     (prim mesh, k - first record of the instance), the gathers and the arithmetic of k_light_records (instance rows -> prim mesh -> 3 indices ->
//                     3 vertices, xformPointRaw) and the alias entry of k.  All 96 bytes of the record are written, as six 16-byte stores, and the 8-byte
//                     (instance, triangle) source of the binding.
// Bound by the dependent gathers, and small (a few thousand records).  Plain typed global loads and stores: no atomics, no LDS.
// tests/light_derive_checker.cpp restates it in plain C++.
#include "light_derive.h"
#include "dev_math.h"

namespace rt {
namespace {

constexpr int DERIVE_BLOCK = 256;

__device__ __forceinline__ void gStoreU4(void* p, uint32_t x, uint32_t y, uint32_t z, uint32_t w) { u32x4_t v; v.x = x; v.y = y; v.z = z; v.w = w; *(RT_AS_GLOBAL u32x4_t*)p = v; }

__global__ __launch_bounds__(DERIVE_BLOCK) void k_light_expand(const LightExpandArgs a)
{
  const uint32_t k = blockIdx.x * DERIVE_BLOCK + threadIdx.x;
  if(k >= a.numRecs) return;
  // the first emitting instance whose first record is beyond k, less one
  uint32_t lo = 0, hi = a.numEmit;
  while(lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if(gLoadU32(a.prefix + mid) <= k) lo = mid + 1; else hi = mid;
  }
  const uint32_t e = lo - 1u;   // (prefix[0] = 0 <= k: lo >= 1)
  const uint32_t r = k - gLoadU32(a.prefix + e);
  const uint32_t inst = gLoadU32(a.ids + e);
  const DevInstance* di = a.instances + inst;
  float m[12];
  for(int q = 0; q < 3; q++) { const float4 v = gLoadF4(di->o2w + 4 * q); m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w; }
  const uint32_t mesh = gLoadU32(&di->primMesh);
  const rt_prim_mesh* pm = a.primMeshes + mesh;
  const uint32_t vertexOffset = gLoadU32(&pm->vertexOffset), firstIndex = gLoadU32(&pm->firstIndex), matIndex = gLoadU32(&pm->materialIndex);
  const rt_emitter_row* row = a.rows + (gLoadU32(a.meshFirstRow + mesh) + r);
  const uint4 t0 = gLoadU4(row), t1 = gLoadU4(reinterpret_cast<const char*>(row) + 16);   // (triangle, uv0.x uv0.y uv1.x) (uv1.y uv2.x uv2.y, pad)
  uint32_t w[9];
  for(int q = 0; q < 3; q++) {
    const uint32_t ix = gLoadU32(a.indices + firstIndex + 3 * t0.x + q);
    const float4 p = gLoadF4(a.vertices + vertexOffset + ix);   // (position.xyz, normal bits)
    float o[3];
    xformPointRaw(m, p.x, p.y, p.z, o);
    w[3 * q] = __float_as_uint(o[0]); w[3 * q + 1] = __float_as_uint(o[1]); w[3 * q + 2] = __float_as_uint(o[2]);
  }
  const uint4 al = gLoadU4(a.alias + k);
  // 96 bytes on a 16-byte aligned array: matIndex transformIndex | v0 v1 v2 | uv0 uv1 uv2 | impSamp | pad
  char* rec = reinterpret_cast<char*>(a.records + k);
  gStoreU4(rec, matIndex, 0xffffffffu, w[0], w[1]);
  gStoreU4(rec + 16, w[2], w[3], w[4], w[5]);
  gStoreU4(rec + 32, w[6], w[7], w[8], t0.y);
  gStoreU4(rec + 48, t0.z, t0.w, t1.x, t1.y);
  gStoreU4(rec + 64, t1.z, al.x, al.y, al.z);
  gStoreU4(rec + 80, al.w, 0u, 0u, 0u);
  gStoreU2(a.sources + k, make_uint2(inst, t0.x));
}

}  // namespace

hipError_t launchLightExpand(hipStream_t stream, const LightExpandArgs& a)
{
  if(a.numRecs == 0 || a.numEmit == 0) return hipSuccess;
  hipLaunchKernelGGL(k_light_expand, dim3((a.numRecs + DERIVE_BLOCK - 1) / DERIVE_BLOCK), dim3(DERIVE_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rt

// light_records.hip — the kernel of rt_set_light_sources (include/rt_abi.h "Light sources"), compiled once.
//   k_light_records   one thread per bound triangle-light record: where the record's source instance was refitted by this update (its bit in the refit tail's dirty
//                     words), v0 v1 v2 become xformPointRaw(objectToWorld, position[index]) of the source triangle — the gathers and the arithmetic of k_refit_tris
//                     (csrc/refit.hip) — stored to bytes 8..43 of the record.  No other byte of a record is written: matIndex / transformIndex in front and the
//                     texcoords, the alias entry and the padding behind depend on neither matrix nor position.
// Bound by dependent gathers (source -> instance rows + prim mesh -> 3 indices -> 3 vertices), not by arithmetic, and small (a few thousand records): one pass over
// all bound records with a dirty test, 256 threads per workgroup, the rewritten records counted with one ballot and one atomic per wave.
// tests/light_checker.cpp restates it in plain C++.
#include "light_records.h"
#include "dev_math.h"

namespace rt {
namespace {

constexpr int LIGHT_BLOCK = 256;

__device__ __forceinline__ void gStoreU32(void* p, uint32_t v) { *(RT_AS_GLOBAL uint32_t*)p = v; }
__device__ __forceinline__ void gStoreU4(void* p, uint4 v) { u32x4_t w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; *(RT_AS_GLOBAL u32x4_t*)p = w; }

__global__ __launch_bounds__(LIGHT_BLOCK) void k_light_records(const LightRecArgs a)
{
  const uint32_t i = blockIdx.x * LIGHT_BLOCK + threadIdx.x;
  bool dirty = false;
  if(i < a.numRecs) {
    const uint2 src = gLoadU2(a.sources + i);   // instance, triangle
    dirty = a.all != 0u || ((gLoadU32(a.dirtyBits + (src.x >> 5)) >> (src.x & 31u)) & 1u) != 0u;
    if(dirty) {
      const DevInstance* di = a.instances + src.x;
      float m[12];
      for(int k = 0; k < 3; k++) { const float4 r = gLoadF4(di->o2w + 4 * k); m[4 * k] = r.x; m[4 * k + 1] = r.y; m[4 * k + 2] = r.z; m[4 * k + 3] = r.w; }
      const rt_prim_mesh* pm = a.primMeshes + gLoadU32(&di->primMesh);
      const uint32_t vertexOffset = gLoadU32(&pm->vertexOffset), firstIndex = gLoadU32(&pm->firstIndex);
      uint32_t w[9];
      for(int k = 0; k < 3; k++) {
        const uint32_t ix = gLoadU32(a.indices + firstIndex + 3 * src.y + k);
        const float4 p = gLoadF4(a.vertices + vertexOffset + ix);   // (position.xyz, normal bits)
        float o[3];
        xformPointRaw(m, p.x, p.y, p.z, o);
        w[3 * k] = __float_as_uint(o[0]); w[3 * k + 1] = __float_as_uint(o[1]); w[3 * k + 2] = __float_as_uint(o[2]);
      }
      // bytes 8..43 of a 96-byte record on a 16-byte aligned array: 8 is 8-byte aligned, 16 is 16-byte aligned, 32 and 40 follow
      char* rec = reinterpret_cast<char*>(a.records + i);
      gStoreU2(rec + 8, make_uint2(w[0], w[1]));
      gStoreU4(rec + 16, make_uint4(w[2], w[3], w[4], w[5]));
      gStoreU2(rec + 32, make_uint2(w[6], w[7]));
      gStoreU32(rec + 40, w[8]);
    }
  }
  const unsigned long long m = __ballot(dirty);
  if((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(a.counter, uint32_t(__popcll(m)));
}

}  // namespace

hipError_t launchLightRecords(hipStream_t stream, const LightRecArgs& a)
{
  if(a.numRecs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_light_records, dim3((a.numRecs + LIGHT_BLOCK - 1) / LIGHT_BLOCK), dim3(LIGHT_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rt

// instances.hip — the kernels of rt_set_instances (instances.h), compiled once.  256 threads per workgroup:
//   k_expand_instances  one thread per new globalId g: the instance of g by a binary search in the prefix words (an instance's triangles are contiguous in g, so the
//                       lanes of a wave walk the same few words), then triRef[g] and the 64-byte table row of g — globalId, TRI_OPAQUE / TRI_NOCULL from the
//                       instance flags, alphaIdx and the micro-map from the prim mesh's templates.  A streaming kernel: per lane one 8-byte store (contiguous across the wave) and
//                       four 16-byte stores at a 64-byte lane stride — each of the four touches a quarter of every cache line of the wave's 4 KB range, which is
//                       whole only once all four have issued (the record layout of k_table / k_emit / k_refit_tris; 0.07 ms for 2.8 M records, not worth a transpose).
//   k_instance_flip     one thread per word of the per-instance flip bits k_refit_tris reads (bit 31 of the prefix words)
// Plain loads and stores; no arithmetic on floats.
#include "instances.h"
#include "dev_math.h"

namespace rt {
namespace {

constexpr int INST_BLOCK = 256;

__global__ __launch_bounds__(INST_BLOCK) void k_expand_instances(const InstExpandArgs a)
{
  const uint32_t g = blockIdx.x * INST_BLOCK + threadIdx.x;
  if(g >= a.numTris) return;
  // the first instance whose first globalId is beyond g, less one: instances without triangles are stepped over
  uint32_t lo = 0, hi = a.numInst;
  while(lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if((gLoadU32(a.prefix + mid) & INST_PREFIX_MASK) <= g) lo = mid + 1; else hi = mid;
  }
  const uint32_t inst = lo - 1u;   // (prefix[0] = 0 <= g: lo >= 1)
  const uint32_t prim = g - (gLoadU32(a.prefix + inst) & INST_PREFIX_MASK);
  const uint2 mf = gLoadU2(&a.instances[inst].primMesh);   // (primMesh, flags)
  uint32_t flags = 0, alphaIdx = 0;
  uint4 omm = make_uint4(0u, 0u, 0u, 0u);
  if(mf.y & RT_INST_FORCE_OPAQUE) flags |= TRI_OPAQUE;
  else {
    alphaIdx = gLoadU32(a.meshAlphaBase + mf.x) + prim + 1u;
    omm = gLoadU4(a.ommTemplate + alphaIdx);
  }
  if(mf.y & RT_INST_CULL_DISABLE) flags |= TRI_NOCULL;
  gStoreU2(a.triRef + g, make_uint2(inst, prim));
  uint4* dst = reinterpret_cast<uint4*>(a.table + g);
  dst[0] = make_uint4(0u, 0u, 0u, 0u);
  dst[1] = make_uint4(0u, 0u, 0u, 0u);
  dst[2] = make_uint4(0u, g, flags, alphaIdx);
  dst[3] = omm;
}

__global__ __launch_bounds__(INST_BLOCK) void k_instance_flip(const uint32_t* prefix, uint32_t numInst, uint32_t words, uint32_t* flipBits)
{
  const uint32_t w = blockIdx.x * INST_BLOCK + threadIdx.x;
  if(w >= words) return;
  uint32_t bits = 0;
  for(uint32_t b = 0; b < 32u; b++) {
    const uint32_t i = w * 32u + b;
    if(i < numInst && (gLoadU32(prefix + i) & INST_PREFIX_FLIP)) bits |= 1u << b;
  }
  flipBits[w] = bits;
}

}  // namespace

hipError_t launchExpandInstances(hipStream_t stream, const InstExpandArgs& a)
{
  if(a.numTris == 0 || a.numInst == 0) return hipSuccess;
  hipLaunchKernelGGL(k_expand_instances, dim3((a.numTris + INST_BLOCK - 1) / INST_BLOCK), dim3(INST_BLOCK), 0, stream, a);
  const uint32_t words = (a.numInst + 31u) / 32u + 1u;
  hipLaunchKernelGGL(k_instance_flip, dim3((words + INST_BLOCK - 1) / INST_BLOCK), dim3(INST_BLOCK), 0, stream, a.prefix, a.numInst, words, a.flipBits);
  return hipGetLastError();
}

}  // namespace rt

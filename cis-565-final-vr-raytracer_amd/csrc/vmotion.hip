// vmotion.hip — the previous-position plane of per-vertex motion vectors (rt_set_object_motion mode RT_OBJECT_MOTION_VERTEX).
// One 16-byte row per scene vertex.  The first deforming call for a mesh after a rendered frame copies the mesh's live positions here, on the stream ahead of its
// commit; the RT_VM builds of stages.hip read a row with one global_load_dwordx4.
#include "stages.h"

namespace rt {

__global__ __launch_bounds__(256) void k_capture_positions(const rt_vertex* __restrict__ vertices, float4* __restrict__ plane, uint32_t first, uint32_t count)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= count) return;
  const rt_vec3 p = vertices[size_t(first) + i].position;
  plane[size_t(first) + i] = make_float4(p.x, p.y, p.z, 0.0f);
}

hipError_t launchCapturePositions(hipStream_t stream, const rt_vertex* vertices, float4* plane, uint32_t first, uint32_t count)
{
  if(count == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_capture_positions, dim3((count + 255u) / 256u), dim3(256), 0, stream, vertices, plane, first, count);
  return hipGetLastError();
}

}  // namespace rt

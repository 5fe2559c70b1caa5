// gi_spatial.h — launcher of the ReSTIR GI spatial reuse pass (csrc/gi_spatial.hip, rt_set_gi_spatial).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
namespace rt {
// Everything the pass reads and writes.  Its own struct: DevFrame, which every existing kernel takes by value, stays as it is.
struct GiSpatialArgs {
  const uint4* thisG;                  // this frame's G-buffer (full resolution, row pitch W), read at 2p
  const rt_indirect_reservoir* resv;   // this frame's indirect reservoirs as the indirect stage wrote them ((W/2) x (H/2), compact)
  rt_indirect_reservoir* out;          // the spatially resampled reservoirs (same layout)
  float4* indA;                        // RT_BUF_DENOISE_IND_A (row pitch W, top-left quarter)
  int32_t W, H;                        // full-resolution size
  int32_t mode, samples, radius;       // rt_gi_spatial
  float normalThreshold, depthThreshold, jacobianMax;
};
hipError_t launchGiSpatial(hipStream_t stream, const DevScene& S, const rt_state& st, const rt_scene_camera& cam, const GiSpatialArgs& A);
}  // namespace rt

// taa.h — launcher of the temporal anti-aliasing resolve (csrc/taa.hip, rt_set_taa).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
namespace rt {
// Everything one resolve reads and writes.  Its own struct: DevFrame, which every existing kernel takes by value, stays as it is.
// Images are RGBA32F / f32 with a row pitch of W.
struct TaaArgs {
  const uint4* thisG; const uint4* lastG;           // G(f), G(f-1)
  const float4* curD; const float4* curI;           // this frame's RT_BUF_DIRECT_RESULT / RT_BUF_INDIRECT_RESULT (after compose)
  const float4* prevD; const float4* prevI; const float* prevN;   // the history of parity f-1 (resolved images, history length n)
  float4* outD; float4* outI; float* outN;          // the history of parity f
  int32_t W, H;
  int32_t histValid;                                // 0: every pixel starts without history (n = 1)
  float alpha, clipGamma;
};
constexpr int TAA_MAX_HISTORY = 1024;
hipError_t launchTaaResolve(hipStream_t stream, const TaaArgs& A, const rt_scene_camera& cam);
}  // namespace rt

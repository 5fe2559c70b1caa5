// upscale.h — launcher of the temporal upsampling resolve (csrc/upscale.hip, rt_set_upscale).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
namespace rt {
// Everything one resolve reads and writes.  Its own struct, like TaaArgs: DevFrame stays as it is.
// The frame's images (G-buffers, composed results) are W x H with a row pitch of W; the history is Wo x Ho with a row pitch of Wo.
struct UpscaleArgs {
  const uint4* thisG; const uint4* lastG;           // G(f), G(f-1): render size
  const float4* curD; const float4* curI;           // this frame's RT_BUF_DIRECT_RESULT / RT_BUF_INDIRECT_RESULT (after compose): render size
  const float4* prevD; const float4* prevI; const float* prevN;   // the history of parity f-1 (resolved images, history length n): output size
  float4* outD; float4* outI; float* outN;          // the history of parity f: output size
  int32_t W, H;                                     // render size
  int32_t Wo, Ho;                                   // output size
  int32_t histValid;                                // 0: every pixel starts without history (n = 1)
  float alpha, clipGamma;
  float dx, dy;                                     // this frame's jitter offset in render pixels (rt_upscale_jitter_camera's delta)
};
constexpr int UPSCALE_MAX_HISTORY = 1024;
hipError_t launchUpscaleResolve(hipStream_t stream, const UpscaleArgs& A, const rt_scene_camera& cam);
}  // namespace rt

// svgf.h — launchers of the variance-guided spatiotemporal denoiser (csrc/svgf.hip, rt_set_denoiser RT_DENOISER_SVGF).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
namespace rt {
// Everything one component's chain (direct: full resolution, indirect: half resolution) reads and writes.  Its own struct: DevFrame, which every
// existing kernel takes by value, stays as it is.  Images are RGBA32F with a row pitch of W (the half-resolution ones use the top-left quarter, like the
// A-Trous temporaries); history, moments and the decoded geometry are compact (row pitch bx).
struct SvgfArgs {
  const uint4* thisG; const uint4* lastG; const short2* motion;   // this frame's G-buffer and motion vectors, the previous frame's G-buffer (full resolution)
  const float4* noisy;            // HDRToLDR(clampRadiance(x)) demodulated colour of the stage
  float4* bufA; float4* bufB;     // level ping-pong: (colour, variance)
  float4* out;                    // the last level's target (LDRToHDR applied)
  float4* geomN; float4* geomP;   // (normal, material hash bits), (reconstructed position, 0) of this frame: the A-Trous chain's decode
  const float4* prevC; const float2* prevM;   // history of the previous frame: (colour, n), (m1, m2)
  float4* histC; float2* histM;               // history this frame writes
  int32_t W, H, bx, by;           // full-resolution size; the component's grid
  int32_t histValid;              // 0: every pixel starts without history (n = 1)
  int32_t cap;                    // historyCap
  float alphaC, alphaM, phiLum, sigN, sigD;
};
constexpr int SVGF_LEVELS_DIRECT = 4, SVGF_LEVELS_INDIRECT = 5;
// steps of one chain: 0 = temporal accumulation (+ geometry decode), 1 = variance, 2 + l = A-Trous level l.  Launched in order on one stream.
inline int svgfSteps(bool ind) { return 2 + (ind ? SVGF_LEVELS_INDIRECT : SVGF_LEVELS_DIRECT); }
hipError_t launchSvgfStep(hipStream_t stream, const SvgfArgs& A, const rt_scene_camera& cam, bool ind, int step);
}  // namespace rt

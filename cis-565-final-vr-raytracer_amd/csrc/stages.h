#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
#include "stage_select.h"
namespace rt {
constexpr int STACK_MAX = 64;  // LDS traversal stack entries per lane (8 B each) upper bound; rt_build_accel rejects deeper trees
// one entry of Renderer::run's dispatch list (renderer.cpp:163-205) on `stream`.
// The stages that trace rays or shade (direct, direct_gen, direct_reuse, indirect): stages.hip, compiled once per entry of STAGE_BUILDS in build.py, each build in
// the namespace of its name.  RT_STAGE_BUILDS (stage_select.h) is the list of those names; what each build holds is in the note at the top of stages.hip.  One
// signature for all: the motion builds and the replay builds find their argument in `X` (dev_scene.h).
#define RT_DECL_LAUNCH(ns)                                                                                                                                       \
  namespace ns {                                                                                                                                                 \
  hipError_t launchStage(hipStream_t stream, const DevScene& S, const DevFrame& F, const StageExtra& X, const rt_state& st, const rt_scene_camera& cam, int stage, \
                         int level, int rowBegin, int rowEnd);                                                                                                   \
  }
RT_STAGE_BUILDS(RT_DECL_LAUNCH)
#undef RT_DECL_LAUNCH
// csrc/vmotion.hip: rows [first, first + count) of the previous-position plane <- the positions of the live vertex rows (the capture ahead of a deforming commit)
hipError_t launchCapturePositions(hipStream_t stream, const rt_vertex* vertices, float4* plane, uint32_t first, uint32_t count);
// filters.hip, compiled once: every other stage (both A-Trous chains, compose; hipErrorInvalidValue for a level outside the chain or any other stage), and the
// tile-order pass that every build of the indirect stage launches ahead of k_indirect_stage
hipError_t launchFilterStage(hipStream_t stream, const DevFrame& F, const rt_state& st, const rt_scene_camera& cam, int stage, int level, int rowBegin, int rowEnd);
hipError_t launchIndTileOrder(hipStream_t stream, const rt_state& st, int rowBegin, int tilesX, int tilesY, int cap, uint32_t* lists, uint32_t* counts);

// uniform-only terms of sun_and_sky() (sky.h), one thread
struct SkyPre;
hipError_t launchSkyPrepare(hipStream_t stream, const rt_sun_and_sky& ss, SkyPre* out);
hipError_t launchTraceRays(hipStream_t stream, const DevScene& S, int n, const float4* rays, float4* out, int anyHit);
hipError_t launchPick(hipStream_t stream, const DevScene& S, const rt_mat4& viewInv, const rt_mat4& projInv, float pickX, float pickY, rt_pick_result* out);
// RenderOutput::run + post.frag as compute (post.hip)
// csrc/microbench.hip
hipError_t measureValuIssue(hipStream_t stream, int variant, int wavesPerSimd, double* waveInstPerSec, double* seconds);
hipError_t launchTonemap(hipStream_t stream, const float4* direct, const float4* indirect, double* rowSums, float* mean, const rt_tonemapper& tm, int dbg, int W, int H,
                         uint32_t* ldr, float4* mipD, float4* mipI);
}

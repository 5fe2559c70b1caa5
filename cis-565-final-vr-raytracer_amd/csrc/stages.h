#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
namespace rt {
constexpr int STACK_MAX = 64;  // LDS traversal stack entries per lane (8 B each) upper bound; rt_build_accel rejects deeper trees
// one entry of Renderer::run's dispatch list (renderer.cpp:163-205) on `stream`.
// The stages that trace rays or shade (direct, direct_gen, direct_reuse, indirect): stages.hip, compiled six times
//   base / sky          HDR environment only / sun & sky code paths compiled in
//   base_cnt / sky_cnt  the same with the counters of rt_set_counting flushed
//   base_lat / sky_lat  k_direct_stage and k_indirect_stage for small launches (latency-mode traversal); the direct stage's rayless half forwards to base / sky
#define RT_DECL_LAUNCH(ns)                                                                                                                              \
  namespace ns {                                                                                                                                        \
  hipError_t launchStage(hipStream_t stream, const DevScene& S, const DevFrame& F, const rt_state& st, const rt_scene_camera& cam, int stage, int level, \
                         int rowBegin, int rowEnd);                                                                                                     \
  }
RT_DECL_LAUNCH(base)
RT_DECL_LAUNCH(sky)
RT_DECL_LAUNCH(base_cnt)
RT_DECL_LAUNCH(sky_cnt)
RT_DECL_LAUNCH(base_lat)
RT_DECL_LAUNCH(sky_lat)
#undef RT_DECL_LAUNCH
// the four object-motion builds (RT_OM, stages_*om.hip): RT_STAGE_DIRECT and RT_STAGE_INDIRECT only, no counting form
#define RT_DECL_LAUNCH_OM(ns)                                                                                                                                  \
  namespace ns {                                                                                                                                               \
  hipError_t launchStage(hipStream_t stream, const DevScene& S, const DevFrame& F, const DevObjMotion& OM, const rt_state& st, const rt_scene_camera& cam,      \
                         int stage, int level, int rowBegin, int rowEnd);                                                                                      \
  }
RT_DECL_LAUNCH_OM(base_om)
RT_DECL_LAUNCH_OM(sky_om)
RT_DECL_LAUNCH_OM(base_lat_om)
RT_DECL_LAUNCH_OM(sky_lat_om)
#undef RT_DECL_LAUNCH_OM
// the four per-vertex-motion builds (RT_VM, stages_*vm.hip): the same two stages, no counting form
#define RT_DECL_LAUNCH_VM(ns)                                                                                                                                  \
  namespace ns {                                                                                                                                               \
  hipError_t launchStage(hipStream_t stream, const DevScene& S, const DevFrame& F, const DevVtxMotion& VM, const rt_state& st, const rt_scene_camera& cam,      \
                         int stage, int level, int rowBegin, int rowEnd);                                                                                      \
  }
RT_DECL_LAUNCH_VM(base_vm)
RT_DECL_LAUNCH_VM(sky_vm)
RT_DECL_LAUNCH_VM(base_lat_vm)
RT_DECL_LAUNCH_VM(sky_lat_vm)
#undef RT_DECL_LAUNCH_VM
// the four primary-replay builds (RT_REPLAY, stages_*rp*.hip): RT_STAGE_DIRECT only, base and sky, each with its counting form
#define RT_DECL_LAUNCH_RP(ns)                                                                                                                                  \
  namespace ns {                                                                                                                                               \
  hipError_t launchStage(hipStream_t stream, const DevScene& S, const DevFrame& F, const DevVis& V, const rt_state& st, const rt_scene_camera& cam,             \
                         int stage, int level, int rowBegin, int rowEnd);                                                                                      \
  }
RT_DECL_LAUNCH_RP(base_rp)
RT_DECL_LAUNCH_RP(sky_rp)
RT_DECL_LAUNCH_RP(base_rp_cnt)
RT_DECL_LAUNCH_RP(sky_rp_cnt)
#undef RT_DECL_LAUNCH_RP
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

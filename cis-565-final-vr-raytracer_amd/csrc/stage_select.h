// stage_select.h — which build of the traced stages runs a launch?  
//
// Plain C++ with no device or library dependency, so that the rule can be tested without a GPU (tests/test_stage_select_cpu.py).
//
// csrc/stages.hip is compiled once per entry of STAGE_BUILDS in build.py; RT_STAGE_BUILDS below is the same set of names, and every list of builds in the library
// (the enum here, the launchStage declarations of stages.h, the table of launchers in rt_api.cpp) is made from it.  The builds compute the same bits: a wrong choice
// costs time and fails no image comparison, which is why the choice is a pure function with a test of its own.
#pragma once
#include "primary_replay.h"

namespace rt {

// name = the build's namespace (stages.hip pastes it from its switches): environment, then _lat, then _om / _vm / _rp, then _cnt
#define RT_STAGE_BUILDS(X)                                                      \
  X(base) X(sky) X(base_cnt) X(sky_cnt) X(base_lat) X(sky_lat)                  \
  X(base_om) X(sky_om) X(base_lat_om) X(sky_lat_om)                             \
  X(base_vm) X(sky_vm) X(base_lat_vm) X(sky_lat_vm)                             \
  X(base_rp) X(sky_rp) X(base_rp_cnt) X(sky_rp_cnt)

enum StageBuild : int {
#define RT_STAGE_BUILD_ID(name) STAGE_BUILD_##name,
  RT_STAGE_BUILDS(RT_STAGE_BUILD_ID)
#undef RT_STAGE_BUILD_ID
  STAGE_BUILD_FILTERS,   // csrc/filters.hip, compiled once: both A-Trous chains and compose
  STAGE_BUILD_COUNT
};

inline const char* stageBuildName(int id)
{
  static const char* const names[STAGE_BUILD_COUNT] = {
#define RT_STAGE_BUILD_NAME(name) #name,
    RT_STAGE_BUILDS(RT_STAGE_BUILD_NAME)
#undef RT_STAGE_BUILD_NAME
    "filters"};
  return id >= 0 && id < STAGE_BUILD_COUNT ? names[id] : "?";
}

// the motion-vector form of the direct and the indirect stage (rt_set_object_motion)
enum StageMotion : int { STAGE_MOTION_NONE = 0, STAGE_MOTION_OBJECT = 1, STAGE_MOTION_VERTEX = 2 };

// RT_TRAVERSAL_AUTO takes the latency build for launches of at most this many 8x8 tiles (rt_api.cpp holds the defaults and what overrides them)
struct LatencyTiles { int direct, indirect; };

// The traced kernels exist twice: the throughput build (one ray per lane: full frames are bound by instruction issue) and the latency build (eight lanes per ray: a
// row band of a multi-GPU frame or a small image is bound by the dependent steps of its slowest rays).  Only the direct and the indirect stage have a latency
// build, and the counting build is a throughput build.  The tile count is that of the launch as launchStage sizes it: the indirect stage at half resolution, the row
// band clamped to the image.
inline bool latencyBuild(bool counting, int traversal, int stage, int width, int height, int rowBegin, int rowEnd, LatencyTiles maxTiles)
{
  if(counting || (stage != RT_STAGE_DIRECT && stage != RT_STAGE_INDIRECT)) return false;
  if(traversal == RT_TRAVERSAL_LATENCY) return true;
  if(traversal != RT_TRAVERSAL_AUTO) return false;
  const bool half = stage == RT_STAGE_INDIRECT;
  const int gw = half ? width / 2 : width, gh = half ? height / 2 : height;
  const int r1 = (rowEnd <= 0 || rowEnd > gh) ? gh : rowEnd, r0 = rowBegin < 0 ? 0 : rowBegin;
  const int rows = r1 > r0 ? r1 - r0 : 0;
  const long tiles = long((gw + 7) / 8) * long((rows + 7) / 8);
  return tiles <= (half ? maxTiles.indirect : maxTiles.direct);
}

// The build of one launch.  `latency` is latencyBuild's answer for it, `action` what the replay rule said (primary_replay.h; NORMAL for a launch that did not pass
// through it).  A RECORD or REPLAY launch is a direct stage of a throughput build (the caller made it eligible on those terms) and goes before the motion forms;
// the motion forms exist for the direct and the indirect stage without counting; everything else is the plain choice.
inline StageBuild stageBuild(bool sky, bool counting, bool latency, int stage, StageMotion motion, PrimaryReplayAction action)
{
  auto env = [sky](StageBuild base, StageBuild withSky) { return sky ? withSky : base; };
  if(stage == RT_STAGE_DENOISE_DIRECT || stage == RT_STAGE_DENOISE_INDIRECT || stage == RT_STAGE_COMPOSE) return STAGE_BUILD_FILTERS;
  const bool twoForms = stage == RT_STAGE_DIRECT || stage == RT_STAGE_INDIRECT;   // the stages with a latency and a motion form
  latency = latency && twoForms && !counting;
  if(action != PRIMARY_REPLAY_NORMAL && stage == RT_STAGE_DIRECT && !latency)
    return counting ? env(STAGE_BUILD_base_rp_cnt, STAGE_BUILD_sky_rp_cnt) : env(STAGE_BUILD_base_rp, STAGE_BUILD_sky_rp);
  if(motion != STAGE_MOTION_NONE && !counting && twoForms) {
    if(motion == STAGE_MOTION_OBJECT) return latency ? env(STAGE_BUILD_base_lat_om, STAGE_BUILD_sky_lat_om) : env(STAGE_BUILD_base_om, STAGE_BUILD_sky_om);
    return latency ? env(STAGE_BUILD_base_lat_vm, STAGE_BUILD_sky_lat_vm) : env(STAGE_BUILD_base_vm, STAGE_BUILD_sky_vm);
  }
  if(latency) return env(STAGE_BUILD_base_lat, STAGE_BUILD_sky_lat);
  return counting ? env(STAGE_BUILD_base_cnt, STAGE_BUILD_sky_cnt) : env(STAGE_BUILD_base, STAGE_BUILD_sky);
}

}  // namespace rt

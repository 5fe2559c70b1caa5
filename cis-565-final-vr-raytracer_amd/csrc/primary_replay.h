// primary_replay.h — when may the direct stage replay last frame's primary visibility instead of tracing it?  
//
// Plain C++ with no device or library dependency, so that the rule can be tested without a GPU (tests/test_primary_replay_cpu.py).
//
// For a camera at rest and an unchanged scene the primary ray of a pixel is the same bit for bit from frame to frame; all that changes is the stochastic
// alpha draw, keyed on (ray seed, triangle id).  One RECORD launch stores, per pixel, the leaf record of the closest deterministic accept and the records of
// the stochastic candidates in front of it (stages.hip, RT_REPLAY); REPLAY launches re-test those records with the frame's seed and skip the traversal.
//
// Trust lives HERE, in host state: the planes hold indices into a tree's leaf records for one camera, and nothing in them says which.  A launch may replay only
// in state VALID, which is entered by a recording and left at the first thing that can change what a primary ray hits.
#pragma once
#include <cstdint>
#include <cstring>
#include "../../include/rt_abi.h"

namespace rt {

enum PrimaryReplayAction : int { PRIMARY_REPLAY_NORMAL = 0, PRIMARY_REPLAY_RECORD = 1, PRIMARY_REPLAY_REPLAY = 2 };
enum PrimaryReplayStateId : int { PRIMARY_REPLAY_NONE = 0, PRIMARY_REPLAY_VALID = 1 };

// what Ctx::raySpawn reads of a launch: the two inverse matrices of the launch camera (jitter included) and the image size
struct PrimaryReplayView {
  float viewInverse[16];
  float projInverse[16];
  int32_t width, height;
};

// ... of a launch camera: projView, lastView, lastProjView, lastPosition and nbLights feed the temporal lookup and the shading, never the ray, and are not part of a view
inline PrimaryReplayView primaryReplayViewOf(const rt_scene_camera& cam, int32_t width, int32_t height)
{
  PrimaryReplayView v{};
  static_assert(sizeof v.viewInverse == sizeof cam.viewInverse && sizeof v.projInverse == sizeof cam.projInverse, "rt_mat4 is 16 floats");
  std::memcpy(v.viewInverse, &cam.viewInverse, sizeof v.viewInverse);
  std::memcpy(v.projInverse, &cam.projInverse, sizeof v.projInverse);
  v.width = width; v.height = height;
  return v;
}

struct PrimaryReplayState {
  int state = PRIMARY_REPLAY_NONE;
  bool haveView = false;        // `view` is the view of the previous full-frame direct launch, and nothing invalidating happened since
  PrimaryReplayView view{};
  int atRest = 0;               // consecutive launches that found the previous launch's view unchanged
};

// one direct launch, as far as the rule needs to know it
struct PrimaryReplayLaunch {
  PrimaryReplayView view;
  bool fullFrame;               // covers every row of the image (a row band never replays and drops the state)
  bool eligible;                // throughput build, no TAA, no object-motion mode, not switched off, planes available
};

inline bool primaryReplaySameView(const PrimaryReplayView& a, const PrimaryReplayView& b)
{
  // bitwise: -0.0f and 0.0f are different cameras here (they spawn the same rays, and a recording more is all that costs), NaN equals itself
  return std::memcmp(a.viewInverse, b.viewInverse, sizeof a.viewInverse) == 0 && std::memcmp(a.projInverse, b.projInverse, sizeof a.projInverse) == 0 &&
         a.width == b.width && a.height == b.height;
}

// anything that can change what a primary ray hits, or the order of the leaf records: back to NONE, and the next launch starts a new count
inline void primaryReplayInvalidate(PrimaryReplayState& s)
{
  s.state = PRIMARY_REPLAY_NONE;
  s.haveView = false;
  s.atRest = 0;
}

// The transition of one direct launch; returns what the launch does.  restFrames: at-rest launches that must precede a recording (at least 2: the second launch at
// a camera is the seeded trace's best case and is left alone, and a one-frame pause does not pay for a recording).
//   launch 1 at a camera: NORMAL (atRest 0)   launch 2: NORMAL (1)   ...   launch restFrames + 1: RECORD -> VALID   every later one: REPLAY
inline PrimaryReplayAction primaryReplayStep(PrimaryReplayState& s, const PrimaryReplayLaunch& l, int restFrames)
{
  if(restFrames < 2) restFrames = 2;
  if(!l.fullFrame || !l.eligible) { primaryReplayInvalidate(s); return PRIMARY_REPLAY_NORMAL; }
  if(!s.haveView || !primaryReplaySameView(s.view, l.view)) {
    s.state = PRIMARY_REPLAY_NONE;
    s.view = l.view; s.haveView = true; s.atRest = 0;
    return PRIMARY_REPLAY_NORMAL;
  }
  if(s.state == PRIMARY_REPLAY_VALID) return PRIMARY_REPLAY_REPLAY;
  if(s.atRest < restFrames) s.atRest++;
  if(s.atRest >= restFrames) { s.state = PRIMARY_REPLAY_VALID; return PRIMARY_REPLAY_RECORD; }
  return PRIMARY_REPLAY_NORMAL;
}

}  // namespace rt

// morph.h — morph targets (blend shapes) on the GPU (csrc/morph.hip, "Morph targets" in include/rt_abi.h).  k_morph turns rest rows and the
// ACTIVE targets of a set (weight != 0; the host builds that list) into staged rows.  A morph-only mesh's staged rows are committed like a skin's; a morphed and
// skinned mesh's staged rows are the input of a second k_skin launch (csrc/deform.hip, unchanged) that reads and writes the skin's staging range in place.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"

namespace rt {

struct MorphJob {         // one per morph set the call poses
  uint32_t threadBase;    // first thread of the job: a multiple of 64, so a wave never spans two jobs and the loop over the active list is wave-uniform
  uint32_t count;         // vertices of the prim mesh (V)
  uint32_t restFirst;     // first row of the mesh in the rest-pose / staging buffers of its pool
  uint32_t firstDelta;    // rt_morph_set::firstDelta
  uint32_t firstActive;   // first pair of the set in the call's active list
  uint32_t numActive;     // 0: the rest rows are copied
  uint32_t planes;        // rt_morph_set::planes
  uint32_t pool;          // 0: the skin's rest / staging buffers (the mesh has a skin), 1: the morph pool
};

struct MorphActive { uint32_t target; float weight; };   // one per target whose weight is not zero, ascending target index within a set

struct MorphArgs {
  const rt_vertex* rest0;  rt_vertex* staged0;   // pool 0
  const rt_vertex* rest1;  rt_vertex* staged1;   // pool 1
  const rt_morph_delta* deltas;
  const MorphActive* active;
  const MorphJob* jobs;
  uint32_t numJobs, numThreads;
  uint32_t* nonFinite;                           // the counter k_skin uses: staged positions that are not finite
};

static_assert(sizeof(MorphJob) == 32 && sizeof(MorphActive) == 8, "k_morph's job search reads threadBase at a 32-byte stride; the active list is read as 8-byte pairs");

// one thread per vertex of the listed sets (each job rounded up to whole waves)
hipError_t launchMorph(hipStream_t stream, const MorphArgs& a);

}  // namespace rt

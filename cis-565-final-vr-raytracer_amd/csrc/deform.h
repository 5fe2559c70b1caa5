// deform.h — deforming meshes: linear-blend skinning on the GPU and the per-instance coordinate maximum the hit rule's pad is a reduction of (csrc/deform.hip,
// "Deforming meshes" in include/rt_abi.h).  The kernels produce vertices and one number per instance; the leaf records and the boxes above them are
// rewritten by the kernels of csrc/refit.hip, unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"

namespace rt {

struct SkinJob {          // one per skin listed in an rt_update_skins call
  uint32_t threadBase;    // first thread of the job (running sum of the counts before it)
  uint32_t count;         // vertices of the skinned prim mesh
  uint32_t restFirst;     // first row of the mesh in the rest-pose / staging buffers
  uint32_t firstInfluence;
  uint32_t firstJoint;    // first matrix of the skin in the call's matrix array
  uint32_t pad[3];
};

struct SkinArgs {
  const rt_vertex* rest;              // the rows rt_set_skins captured
  rt_vertex* staged;                  // same layout: the posed rows, committed to the live array by the host when no position is non-finite
  const rt_skin_influence* influences;
  const float* joints;                // 12 floats per matrix, 3 x 4 row-major
  const SkinJob* jobs;
  uint32_t numJobs, numThreads;
  uint32_t* nonFinite;                // one counter: staged positions that are not finite
};

struct CoordJob {         // one per instance whose prim mesh deformed
  uint32_t threadBase;    // first thread of the job: a multiple of 64, so a wave never spans two jobs
  uint32_t indexCount;
  uint32_t firstIndex;
  uint32_t vertexBase;    // first row of the instance's prim mesh in `vertices`
  uint32_t instance;
  uint32_t pad[3];
};

struct CoordMaxArgs {
  const rt_vertex* vertices;          // the live array, or the staging buffer of a pose that has not been committed yet
  const uint32_t* indices;
  const DevInstance* instances;
  const CoordJob* jobs;
  uint32_t numJobs, numThreads;
  uint32_t* out;                      // per job: the bits of the largest |world coordinate| (cleared to 0 before the launch)
};

static_assert(sizeof(SkinJob) == 32 && sizeof(CoordJob) == 32, "the kernels' job search reads threadBase at a 32-byte stride");

// one thread per vertex of the listed skins
hipError_t launchSkin(hipStream_t stream, const SkinArgs& a);
// one thread per (job, index entry)
hipError_t launchInstCoordMax(hipStream_t stream, const CoordMaxArgs& a);

}  // namespace rt

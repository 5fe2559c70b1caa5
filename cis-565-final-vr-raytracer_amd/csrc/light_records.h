// light_records.h — emitters that follow moved and deformed geometry: rewrite v0 v1 v2 of the triangle-light records whose source triangle belongs to an instance
// the refit tail refits (csrc/light_records.hip, "Light sources" in include/rt_abi.h).  A record's positions are xformPoint(objectToWorld,
// position[index]) of its source triangle, the expression k_refit_tris (csrc/refit.hip) evaluates for the leaf records; every other byte of a record (matIndex,
// transformIndex, texcoords, the alias entry, the padding) depends on neither the matrix nor the positions and is never written.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"

namespace rt {

struct LightRecArgs {
  rt_trig_light* records;             // the device light array, or a scratch array of the same layout (the bind-time check)
  const rt_light_source* sources;     // sources[k]: the (instance, triangle) records[k] came from
  const DevInstance* instances;       // rows of the moved instances already hold the new matrices
  const rt_prim_mesh* primMeshes;
  const rt_vertex* vertices;          // the live array: a pose has been committed
  const uint32_t* indices;
  const uint32_t* dirtyBits;          // bit i: instance i was refitted by this update (not read when `all` is set)
  uint32_t* counter;                  // records rewritten (cleared before the launch)
  uint32_t numRecs;
  uint32_t all;                       // 1: every record is evaluated
};

// one thread per bound record
hipError_t launchLightRecords(hipStream_t stream, const LightRecArgs& a);

}  // namespace rt

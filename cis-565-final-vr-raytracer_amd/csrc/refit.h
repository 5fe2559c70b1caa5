// refit.h — moving instances without a rebuild: rewrite the leaf records of the moved instances and refit the BVH8 boxes above them (csrc/refit.hip,
// rt_update_instances in include/rt_abi.h).  The reference rebuilds its TLAS (src/accelstruct.cpp:132-162); here every (instance, triangle)
// pair is a world-space record, so the records move and the tree keeps its topology: meta, imask, childBase, triBase and the slot assignment never change.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"

namespace rt {

struct RefitArgs {
  Node8* nodes;
  Tri48* tris;
  const TriRef* triRef;
  const DevInstance* instances;      // rows of the moved instances already hold the new matrices
  const rt_prim_mesh* primMeshes;
  const rt_vertex* vertices;
  const uint32_t* indices;
  const uint32_t* dirtyBits;         // bit i: instance i moved in this update
  const uint32_t* flipBits;          // bit i: its new matrix has a negative determinant (TRI_FLIP)
  const uint32_t* recNode;           // leaf record -> the node whose slot holds it
  uint32_t* nodeDirty;               // per node, cleared before the update: 1 = a record under one of its leaf slots was rewritten / the node was refitted
  uint32_t* counters;                // [0] leaf records rewritten, [1] nodes refitted
  uint32_t numRecs;
  float pad;                         // the pad every recomputed leaf box is widened by
  int32_t full;                      // the pad grew: every leaf box is recomputed
};

// one thread per leaf record
hipError_t launchRefitTris(hipStream_t stream, const RefitArgs& a);
// one thread per node of the level [first, first + count); levels are launched deepest first
hipError_t launchRefitLevel(hipStream_t stream, const RefitArgs& a, uint32_t first, uint32_t count);

}  // namespace rt

// instances.h — rt_set_instances (include/rt_abi.h "Adding and removing instances"): a new instance table becomes the device builder's input on the
// GPU.  What a leaf record holds besides its position is a function of (prim mesh, triangle, instance flags) only, so it is made once per prim mesh on the host (the
// templates: one AlphaRec and one 16-byte opacity micro-map per triangle of the mesh) and expanded per (instance, triangle) pair by k_expand_instances; positions and
// TRI_FLIP come from k_refit_tris and the tree from accelBuildRun, as in every rebuild.  tests/instances_checker.cpp restates the expansion in plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_scene.h"

namespace rt {

// prefix word i: the first globalId of instance i in bits 0..30 (word numInst: the triangle count), bit 31: the instance's matrix mirrors (det < 0)
constexpr uint32_t INST_PREFIX_MASK = 0x7fffffffu, INST_PREFIX_FLIP = 0x80000000u;

struct InstExpandArgs {
  const uint32_t* prefix;         // numInst + 1 words, exclusive prefix of the per-instance triangle counts
  const DevInstance* instances;   // numInst rows
  const uint32_t* meshAlphaBase;  // per prim mesh: alphaIdx of its triangle p = meshAlphaBase[mesh] + p + 1
  const uint4* ommTemplate;       // per alphaIdx: the micro-map of that (mesh, triangle); valid for the meshes that have had a non-opaque instance
  TriRef* triRef;                 // out, numTris rows
  Tri48* table;                   // out, numTris rows: globalId, flags, alphaIdx, omm; position words zero
  uint32_t* flipBits;             // out, (numInst + 31) / 32 + 1 words: bit i = the mirror bit of prefix word i (RefitArgs::flipBits)
  uint32_t numInst, numTris;
};

// one thread per new globalId; then one thread per word of flipBits
hipError_t launchExpandInstances(hipStream_t stream, const InstExpandArgs& a);

}  // namespace rt

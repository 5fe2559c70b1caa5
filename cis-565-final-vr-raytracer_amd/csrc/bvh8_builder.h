#pragma once
#include <algorithm>
#include <vector>
#include "bvh8.h"
#include "dev_scene.h"

namespace rt {

struct BuildInput {
  const rt_scene_desc* scene;
};
struct BuildOutput {
  std::vector<Node8> nodes;
  std::vector<Tri48> tris;       // BVH leaf order
  std::vector<TriRef> triRef;    // by globalId
  std::vector<DevInstance> instances;
  int maxDepth = 0;
  double sahCost = 0;
  double sahNodeStepsQ = 0, sahTriStepsQ = 0;  // the same with the 8-bit quantised child boxes the traversal tests
  double sahNodeSteps = 0, sahTriSteps = 0;   // SAH expectation of node / triangle steps of a ray that hits the root box (wide tree, build-time boxes)
  uint64_t references = 0;                   // leaf records (= tris.size()): > the triangle count when spatial splits duplicated references
  uint64_t spatialSplits = 0, rotations = 0, reinsertions = 0;
  float pad = 0;
};
// Host-side build: flatten (instance, triangle) pairs to world space, binned-SAH BVH2, greedy collapse to 8-wide,
// octant-ordered slot assignment, conservative 8-bit quantisation.  Replaces AccelStructure::create
// (src/accelstruct.cpp:55-162: BLAS per prim mesh + TLAS per node, built by the Vulkan driver).
// plainTree: object splits only, no rotations / reinsertion — the tree of rounds 1-4, whatever the environment says (rt_build_accel's fallback when the quality passes
// made a tree deeper than the traversal stack).
bool buildBvh8(const rt_scene_desc& scene, BuildOutput& out, int threads, bool plainTree = false);
// 3x4 affine inverse of an instance matrix (R = world-to-object, *detOut = the determinant of the 3x3 block): the builder's, shared with rt_update_instances so that a
// moved instance's w2o bits equal a fresh build's
void inverseAffine(const float* M, float* R, float* detOut);
// The pad of the leaf boxes from every instance's largest |world coordinate|.  The one statement of the rule: the builder and the update / rebuild calls of rt_api.cpp
// reduce with it, so a refitted or rebuilt tree's pad has the bits of a fresh build's (a float maximum does not depend on the order).
inline float triPadOf(const std::vector<float>& instMax)
{
  float scale = 1e-3f;
  for(float v : instMax) scale = std::max(scale, v);
  return 2e-5f * scale;
}

}  // namespace rt

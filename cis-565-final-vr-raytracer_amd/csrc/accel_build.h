// accel_build.h — rt_rebuild_accel (include/rt_abi.h "Rebuilding on the device"): a new BVH8 topology built on the GPU from the context's current
// (moved) scene.  Morton order of the triangle box centres (63-bit keys, stable radix sort), a Karras binary radix tree over the sorted keys, a top-down collapse to
// 8-wide nodes in the layout of csrc/bvh8.h, level by level; the boxes are the refit kernel's (csrc/refit.hip, full mode over every node), so there is one quantiser.
// Every step is a pure function of the triangle set: two builds of one scene give the same words, and tests/accel_build_checker.cpp restates them in plain C++.
// The binary hierarchy has a second, opt-in builder (rt_set_rebuild_options): PLOC, bottom-up clustering along the Morton order with the area of the
// merged box as the distance.  It fills the same arrays in the same conventions, so the collapse, the emission and the boxes are shared; tests/ploc_checker.cpp
// restates it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <utility>
#include <vector>
#include "refit.h"

namespace rt {

// one tree: what a build writes and a frame / an update reads.  The context keeps two and swaps after a build that succeeded.
struct AccelBuildSet {
  Node8* nodes = nullptr;          // capacity = max(1, triangles): a wide node either has 8 children or only leaf slots with >= 4 triangles in all
  Tri48* tris = nullptr;           // one record per triangle, at its final position
  AlphaRec* alphaByTri = nullptr;  // DevScene::alphaByTri in the new leaf order
  uint32_t* recNode = nullptr;     // leaf record -> the node that holds it (RefitArgs::recNode)
};

// working buffers, allocated by the first rebuild of a scene and kept
struct AccelBuildWork {
  uint32_t n = 0, cap = 0;         // triangles, node capacity
  Tri48* table = nullptr;          // per globalId: the record of the host build (globalId, flags, alphaIdx, omm); v0 / e1 / e2 are rewritten by every rebuild
  float4* centre = nullptr;        // per globalId: box centre
  uint32_t* bounds = nullptr;      // 6 words: min / max of the centres, order-preserving encoding
  unsigned long long* keyIn = nullptr; unsigned long long* keyOut = nullptr;
  uint32_t* valIn = nullptr; uint32_t* valOut = nullptr;   // globalId, before / after the sort
  void* sortTemp = nullptr; size_t sortTempBytes = 0;      // hipcub: radix sort and scan
  uint2* child = nullptr;          // binary node -> (left, right); ids < n - 1 are internal nodes, n - 1 + j is the leaf of sorted position j
  uint2* range = nullptr;          // binary node -> (first, last) sorted position
  float4* boxLo = nullptr; float4* boxHi = nullptr;        // binary node box; boxLo.w = surface area
  uint32_t* stamp = nullptr;       // binary node -> the union round that made its box (0: not yet)
  uint32_t* wideRoot = nullptr;    // wide node -> the binary node it was opened from
  uint32_t* slotEntry = nullptr;   // wide node x 8 -> the binary node of the slot (~0u: empty)
  unsigned long long* count = nullptr; unsigned long long* scan = nullptr;   // per wide node: internal children << 32 | leaf triangles, and its exclusive sum over the level
  uint32_t* nodeDirty = nullptr;   // RefitArgs::nodeDirty for the new tree (capacity words)
  uint32_t* totals = nullptr;      // 4 words: internal children of the level, leaf triangles of the level, error flag, spare
  // what a build is asked for (rt_set_rebuild_options; the values in force, defaults filled in), and how many PLOC merge iterations the last one took
  int builder = 0; uint32_t radius = 0, maxIterations = 0, iterations = 0;
  // PLOC only, 76 B per triangle, allocated by the first PLOC build (accelBuildAllocPloc) into the pool of the buffers above: the clusters in Morton order, double
  // buffered (an iteration reads one and writes the other; never compacted in place), and every cluster's nearest neighbour.  The merge / keep flags and their scan
  // live in `count` / `scan`, which the collapse uses only later; the final leaf order is written to valIn, free after the sort.
  uint32_t* clId[2] = {nullptr, nullptr};      // cluster -> binary node id
  float4* clLo[2] = {nullptr, nullptr};        // cluster box; clHi.w holds the leaf count (bits)
  float4* clHi[2] = {nullptr, nullptr};
  uint32_t* clNn = nullptr;                    // cluster position -> position of its nearest neighbour in the window
};

struct AccelBuildResult {
  std::vector<std::pair<uint32_t, uint32_t>> levels;   // (first node, count), root level first
  uint32_t nodes = 0;
};

// TOO_DEEP and PLOC_ITERATIONS (no single cluster after maxIterations merge iterations) are properties of the scene; NO_ROOT / CAPACITY / COUNT / PLOC_NO_MERGE are
// invariants of the builder that did not hold, PLOC_SETUP a PLOC build started without its buffers or with a radius outside 1..64 (accelBuildWhy names them): never
// the mistake of a caller of the C interface
enum { ACCEL_BUILD_OK = 0, ACCEL_BUILD_TOO_DEEP = 1, ACCEL_BUILD_PLOC_ITERATIONS = 2, ACCEL_BUILD_HIP = 3, ACCEL_BUILD_NO_ROOT = 4, ACCEL_BUILD_CAPACITY = 5, ACCEL_BUILD_COUNT = 6,
       ACCEL_BUILD_PLOC_NO_MERGE = 7, ACCEL_BUILD_PLOC_SETUP = 8 };
enum { ACCEL_BUILDER_LBVH = 0, ACCEL_BUILDER_PLOC = 1, ACCEL_PLOC_RADIUS_MAX = 64, ACCEL_PLOC_RADIUS_DEFAULT = 16, ACCEL_PLOC_ITERATIONS_DEFAULT = 512 };
const char* accelBuildWhy(int code);

hipError_t accelBuildAlloc(AccelBuildWork& w, AccelBuildSet set[2], uint32_t triangles, std::vector<void*>& pool);
// PLOC's cluster buffers at the capacity of `w`, into `pool`; nothing when `w` has them.  *allocated (optional) tells whether it allocated.
hipError_t accelBuildAllocPloc(AccelBuildWork& w, std::vector<void*>& pool, bool* allocated);
// table[tris[r].globalId] = tris[r] for the numRecs records of a host-built tree (all references of a triangle carry the same words)
hipError_t launchAccelTable(hipStream_t stream, const Tri48* tris, uint32_t numRecs, const AccelBuildWork& w);
// The build.  `a` is the refit argument block of the target set (nodes / tris / recNode of `set`, nodeDirty of `w`, all instances marked moved, pad = the new pad);
// evSort[0..1] are recorded around the sort.  w.builder selects the binary hierarchy (PLOC needs accelBuildAllocPloc first); w.iterations is set.  Returns
// ACCEL_BUILD_*; with ACCEL_BUILD_HIP *err holds the HIP error.  After a failure the stream is idle; after ACCEL_BUILD_OK the box passes are still queued and the
// caller synchronises.
int accelBuildRun(hipStream_t stream, AccelBuildWork& w, const AccelBuildSet& set, const RefitArgs& a, const AlphaRec* alphaRec, int maxLevels, hipEvent_t evSort[2],
                  AccelBuildResult& out, hipError_t* err);

}  // namespace rt

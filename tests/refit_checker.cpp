// refit_checker.cpp — test infrastructure of rt_update_instances (include/rt_abi.h "Moving instances", csrc/refit.hip): a plain C++ restatement of the two
// kernels and of the host arithmetic around them, an independent check of a tree's soundness, and the builder's arrays for the CPU tests.
// Compiled by tests/refit.py together with csrc/bvh8_builder.cpp (g++, no GPU).  The restatement walks the tree by node depth and recomputes the pad over all
// triangles; the library keeps contiguous level ranges and per-instance maxima — the tests hold the two to the same words.
#include "../cis-565-final-vr-raytracer_amd/csrc/bvh8_builder.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace rt;

namespace {

struct B3 { float lo[3], hi[3]; };
B3 emptyBox() { B3 b; for(int a = 0; a < 3; a++) { b.lo[a] = 3e38f; b.hi[a] = -3e38f; } return b; }
void grow(B3& b, const float* p) { for(int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], p[a]); b.hi[a] = std::max(b.hi[a], p[a]); } }
void grow(B3& b, const B3& o) { for(int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], o.lo[a]); b.hi[a] = std::max(b.hi[a], o.hi[a]); } }

const uint8_t* qlo(const Node8& N, int a) { return a == 0 ? N.qlox : (a == 1 ? N.qloy : N.qloz); }
const uint8_t* qhi(const Node8& N, int a) { return a == 0 ? N.qhix : (a == 1 ? N.qhiy : N.qhiz); }
uint8_t* qlo(Node8& N, int a) { return a == 0 ? N.qlox : (a == 1 ? N.qloy : N.qloz); }
uint8_t* qhi(Node8& N, int a) { return a == 0 ? N.qhix : (a == 1 ? N.qhiy : N.qhiz); }
float origin(const Node8& N, int a) { return a == 0 ? N.px : (a == 1 ? N.py : N.pz); }
int expo(const Node8& N, int a) { return int(a == 0 ? N.ex : (a == 1 ? N.ey : N.ez)) - 127; }
bool occupied(const Node8& N, int s) { return N.meta[s] != 0; }
bool inner(const Node8& N, int s) { return (N.imask >> s) & 1u; }
uint32_t leafCount(const Node8& N, int s) { return uint32_t(__builtin_popcount(uint32_t(N.meta[s]) >> 5)); }
uint32_t leafFirst(const Node8& N, int s) { return N.triBase + (uint32_t(N.meta[s]) & 31u); }

// the box the traversal tests for slot s: origin + q * 2^e, in float, product first
B3 slotBox(const Node8& N, int s)
{
  B3 b;
  for(int a = 0; a < 3; a++) {
    const float step = std::ldexp(1.0f, expo(N, a));
    b.lo[a] = origin(N, a) + float(qlo(N, a)[s]) * step;
    b.hi[a] = origin(N, a) + float(qhi(N, a)[s]) * step;
  }
  return b;
}
B3 nodeBox(const Node8& N)
{
  B3 b = emptyBox();
  for(int s = 0; s < 8; s++) if(occupied(N, s)) grow(b, slotBox(N, s));
  return b;
}
void triVerts(const Tri48& T, float v[3][3])
{
  v[0][0] = T.v0x; v[0][1] = T.v0y; v[0][2] = T.v0z;
  v[1][0] = T.v0x + T.e1x; v[1][1] = T.v0y + T.e1y; v[1][2] = T.v0z + T.e1z;
  v[2][0] = T.v0x + T.e2x; v[2][1] = T.v0y + T.e2y; v[2][2] = T.v0z + T.e2z;
}
B3 paddedTriBox(const Tri48& T, float pad)
{
  float v[3][3];
  triVerts(T, v);
  B3 b = emptyBox();
  for(int k = 0; k < 3; k++) grow(b, v[k]);
  for(int a = 0; a < 3; a++) { b.lo[a] -= pad; b.hi[a] += pad; }
  return b;
}
// world position of a vertex: ((m0 x + m1 y) + m2 z) + m3 per row
void toWorld(const float* m, const rt_vec3& q, float* o)
{
  for(int r = 0; r < 3; r++) o[r] = ((m[4 * r] * q.x + m[4 * r + 1] * q.y) + m[4 * r + 2] * q.z) + m[4 * r + 3];
}

struct Built { BuildOutput bo; };

}  // namespace

extern "C" {

// ---- the builder's arrays (the CPU tests refit host-built trees) ----
void* rfc_build(const rt_scene_desc* scene, int threads)
{
  Built* b = new Built;
  if(!buildBvh8(*scene, b->bo, std::max(1, threads))) { delete b; return nullptr; }
  return b;
}
void rfc_free(void* h) { delete static_cast<Built*>(h); }
// out: nodes, leaf records, triangles, instances, wide-tree depth, spatial splits
void rfc_counts(void* h, uint64_t* out)
{
  const BuildOutput& bo = static_cast<Built*>(h)->bo;
  out[0] = bo.nodes.size(); out[1] = bo.tris.size(); out[2] = bo.triRef.size(); out[3] = bo.instances.size(); out[4] = uint64_t(bo.maxDepth); out[5] = bo.spatialSplits;
}
float rfc_pad(void* h) { return static_cast<Built*>(h)->bo.pad; }
// which: 0 nodes (80 B), 1 leaf records (64 B), 2 instances (112 B), 3 triRef (8 B)
void rfc_copy(void* h, int which, void* dst)
{
  const BuildOutput& bo = static_cast<Built*>(h)->bo;
  if(which == 0) memcpy(dst, bo.nodes.data(), bo.nodes.size() * sizeof(Node8));
  if(which == 1) memcpy(dst, bo.tris.data(), bo.tris.size() * sizeof(Tri48));
  if(which == 2) memcpy(dst, bo.instances.data(), bo.instances.size() * sizeof(DevInstance));
  if(which == 3) memcpy(dst, bo.triRef.data(), bo.triRef.size() * sizeof(TriRef));
}

// ---- rt_update_instances restated: the arrays are updated in place ----
// scene: primMeshes / vertices / indices (the instances come from `inst`).  treePad: in = the pad the boxes were last computed with, out = after the call.
// stats: leaf records rewritten, nodes refitted, levels, full refit.  Returns 0, or -1 for a call the library refuses (nothing is changed then).
int rfc_refit(Node8* nodes, uint32_t nNodes, Tri48* tris, uint32_t nRecs, const TriRef* triRef, uint32_t nTris, DevInstance* inst, uint32_t nInst,
              const rt_scene_desc* scene, const uint32_t* ids, const float* xf, uint32_t count, float* treePad, float* triPadOut, uint32_t* stats)
{
  (void)nTris;
  std::vector<uint8_t> dirty(nInst, 0), flip(nInst, 0);
  std::vector<DevInstance> rows(count);
  for(uint32_t k = 0; k < count; k++) {
    if(ids[k] >= nInst || dirty[ids[k]]) return -1;
    dirty[ids[k]] = 1;
    for(int a = 0; a < 12; a++) if(!std::isfinite(xf[12 * k + a])) return -1;
    rows[k] = inst[ids[k]];
    memcpy(rows[k].o2w, xf + 12 * k, 48);
    float det;
    inverseAffine(rows[k].o2w, rows[k].w2o, &det);
    if(det == 0.0f || !std::isfinite(det)) return -1;
    for(int a = 0; a < 12; a++) if(!std::isfinite(rows[k].w2o[a])) return -1;
    flip[ids[k]] = det < 0.0f;
  }
  for(uint32_t k = 0; k < count; k++) inst[ids[k]] = rows[k];

  // the pad of the moved scene, over ALL triangles
  float scale = 1e-3f;
  for(uint32_t i = 0; i < nInst; i++) {
    const rt_prim_mesh& pm = scene->primMeshes[inst[i].primMesh];
    for(uint32_t k = 0; k < pm.indexCount; k++) {
      float w[3];
      toWorld(inst[i].o2w, scene->vertices[pm.vertexOffset + scene->indices[pm.firstIndex + k]].position, w);
      for(int a = 0; a < 3; a++) scale = std::max(scale, std::fabs(w[a]));
    }
  }
  const float triPad = 2e-5f * scale;
  *triPadOut = triPad;
  const bool full = nRecs > 0 && triPad > *treePad;
  if(triPad > *treePad) *treePad = triPad;
  const float pad = *treePad;

  // leaf records
  uint32_t rewritten = 0;
  for(uint32_t r = 0; r < nRecs; r++) {
    Tri48& T = tris[r];
    const TriRef ref = triRef[T.globalId];
    if(!dirty[ref.inst]) continue;
    const rt_prim_mesh& pm = scene->primMeshes[inst[ref.inst].primMesh];
    float w[3][3];
    for(int k = 0; k < 3; k++) toWorld(inst[ref.inst].o2w, scene->vertices[pm.vertexOffset + scene->indices[pm.firstIndex + 3 * ref.prim + k]].position, w[k]);
    T.v0x = w[0][0]; T.v0y = w[0][1]; T.v0z = w[0][2];
    T.e1x = w[1][0] - w[0][0]; T.e1y = w[1][1] - w[0][1]; T.e1z = w[1][2] - w[0][2];
    T.e2x = w[2][0] - w[0][0]; T.e2y = w[2][1] - w[0][1]; T.e2z = w[2][2] - w[0][2];
    T.flags = flip[ref.inst] ? (T.flags | TRI_FLIP) : (T.flags & ~uint32_t(TRI_FLIP));
    rewritten++;
  }

  // nodes, deepest first
  std::vector<int> depth(nNodes, -1);
  std::vector<uint32_t> order;
  int levels = 0;
  if(nNodes) {
    depth[0] = 0; order.push_back(0);
    for(size_t h = 0; h < order.size(); h++) {
      const Node8& N = nodes[order[h]];
      levels = std::max(levels, depth[order[h]] + 1);
      uint32_t rel = 0;
      for(int s = 0; s < 8; s++) if(inner(N, s)) { const uint32_t c = N.childBase + rel++; depth[c] = depth[order[h]] + 1; order.push_back(c); }
    }
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return depth[x] > depth[y]; });
  std::vector<uint8_t> refitted(nNodes, 0);
  uint32_t nRefitted = 0;
  if(nRecs > 0 && (count > 0 || full))
  for(uint32_t n : order) {
    const Node8 O = nodes[n];
    bool touched[8] = {}, work = false;
    uint32_t rel = 0;
    for(int s = 0; s < 8; s++) {
      if(!occupied(O, s)) continue;
      if(inner(O, s)) { if(refitted[O.childBase + rel]) work = true; rel++; continue; }
      touched[s] = full;
      for(uint32_t q = 0; q < leafCount(O, s); q++) if(dirty[triRef[tris[leafFirst(O, s) + q].globalId].inst]) touched[s] = true;
      if(touched[s]) work = true;
    }
    if(!work) continue;
    B3 box[8], nb = emptyBox();
    rel = 0;
    for(int s = 0; s < 8; s++) {
      if(!occupied(O, s)) continue;
      if(inner(O, s)) box[s] = nodeBox(nodes[O.childBase + rel++]);
      else if(touched[s]) {
        box[s] = emptyBox();
        for(uint32_t q = 0; q < leafCount(O, s); q++) { float v[3][3]; triVerts(tris[leafFirst(O, s) + q], v); for(int k = 0; k < 3; k++) grow(box[s], v[k]); }
        for(int a = 0; a < 3; a++) { box[s].lo[a] -= pad; box[s].hi[a] += pad; }
      } else box[s] = slotBox(O, s);
      grow(nb, box[s]);
    }
    Node8 W = O;
    W.px = nb.lo[0]; W.py = nb.lo[1]; W.pz = nb.lo[2];
    int ex[3];
    for(int a = 0; a < 3; a++) {
      const float ext = nb.hi[a] - nb.lo[a], p = nb.lo[a];
      int e = -60;
      if(ext > 0) { int fe; std::frexp(ext / 255.f, &fe); e = fe; }
      ex[a] = std::max(-100, std::min(100, e));
      uint32_t pb, ob; const float po = origin(O, a);
      memcpy(&pb, &p, 4); memcpy(&ob, &po, 4);
      for(;;) {
        const float step = std::ldexp(1.0f, ex[a]);
        const bool sameGrid = pb == ob && ex[a] == expo(O, a);
        bool ok = true;
        for(int s = 0; s < 8 && ok; s++) {
          qlo(W, a)[s] = 0; qhi(W, a)[s] = 0;
          if(!occupied(O, s)) continue;
          if(!inner(O, s) && !touched[s] && sameGrid) { qlo(W, a)[s] = qlo(O, a)[s]; qhi(W, a)[s] = qhi(O, a)[s]; continue; }   // an untouched leaf slot on an unchanged grid keeps its bytes
          int ql = int(std::floor((double(box[s].lo[a]) - double(p)) / double(step)));
          ql = std::max(0, std::min(255, ql));
          while(ql > 0 && p + float(ql) * step > box[s].lo[a]) ql--;
          int qh = int(std::ceil((double(box[s].hi[a]) - double(p)) / double(step)));
          qh = std::max(0, qh);
          while(qh <= 255 && p + float(qh) * step < box[s].hi[a]) qh++;
          if(qh > 255) { ok = false; break; }
          qlo(W, a)[s] = uint8_t(ql); qhi(W, a)[s] = uint8_t(qh);
        }
        if(ok) break;
        ex[a]++;
      }
    }
    W.ex = uint8_t(ex[0] + 127); W.ey = uint8_t(ex[1] + 127); W.ez = uint8_t(ex[2] + 127);
    nodes[n] = W;
    refitted[n] = 1; nRefitted++;
  }
  stats[0] = rewritten; stats[1] = nRefitted; stats[2] = uint32_t(levels); stats[3] = full ? 1u : 0u;
  return 0;
}

// ---- soundness of a tree -------------------------------------------------------------------------------------------------------------------------------
// From the root: no occupied slot has qlo > qhi; every node and every leaf record is reached exactly once; every leaf record's triangle is covered by the box a ray
// must pass to reach it — the INTERSECTION of its leaf slot's box and the slot boxes of all its ancestors: the full triangle box widened by `pad` lies inside it.
// (Nesting is checked this way and not as "a child's decoded box lies inside its parent's slot box": the builder quantises the TRUE box of a child outward on every
// level's own grid, so in its trees a child's decoded box may stick out of its parent's slot box by less than a step of the child's grid while every triangle box
// stays inside both.  What soundness needs is the triangle boxes inside every box above them.)  The full box is required of every record of a triangle that has ONE
// reference and of every record of an instance flagged in strictInst (the instances refitted since the build; all of them after a full refit).  The builder
// bounds a spatial-split reference by the part of the triangle inside its cell, so for the references of a split triangle that were never refitted the
// requirement is the builder's own: every sample point of the triangle (vertices, edge points, interior points) lies in the box of at least one reference.
// Returns the number of violations; msg describes the first.
int rfc_check_tree(const Node8* nodes, uint32_t nNodes, const Tri48* tris, uint32_t nRecs, const TriRef* triRef, uint32_t nTris, const uint8_t* strictInst, float pad,
                   char* msg, int msgLen)
{
  int bad = 0;
  std::string first;
  auto report = [&](const std::string& s) { if(bad++ == 0) first = s; };
  std::vector<uint32_t> nodeSeen(nNodes, 0), recSeen(nRecs, 0), refsOf(nTris, 0);
  std::vector<B3> recBox(nRecs);
  for(uint32_t r = 0; r < nRecs; r++) { if(tris[r].globalId >= nTris) report("record " + std::to_string(r) + ": globalId out of range"); else refsOf[tris[r].globalId]++; }
  if(bad == 0 && nNodes) {
    std::vector<std::pair<uint32_t, B3>> stack;
    { B3 all; for(int a = 0; a < 3; a++) { all.lo[a] = -3e38f; all.hi[a] = 3e38f; } stack.push_back({0u, all}); }
    nodeSeen[0] = 1;
    while(!stack.empty()) {
      const uint32_t n = stack.back().first; const B3 above = stack.back().second; stack.pop_back();
      const Node8& N = nodes[n];
      uint32_t rel = 0;
      for(int s = 0; s < 8; s++) {
        if(!occupied(N, s)) { if(inner(N, s)) report("node " + std::to_string(n) + ": empty slot flagged internal"); continue; }
        for(int a = 0; a < 3; a++) if(qlo(N, a)[s] > qhi(N, a)[s]) report("node " + std::to_string(n) + " slot " + std::to_string(s) + ": qlo > qhi");
        B3 sb = slotBox(N, s);
        for(int a = 0; a < 3; a++) { sb.lo[a] = std::max(sb.lo[a], above.lo[a]); sb.hi[a] = std::min(sb.hi[a], above.hi[a]); }
        if(inner(N, s)) {
          const uint32_t c = N.childBase + rel++;
          if(c >= nNodes) { report("node " + std::to_string(n) + ": child out of range"); continue; }
          if(nodeSeen[c]++) { report("node " + std::to_string(c) + " reached twice"); continue; }
          stack.push_back({c, sb});
        } else {
          for(uint32_t q = 0; q < leafCount(N, s); q++) {
            const uint32_t r = leafFirst(N, s) + q;
            if(r >= nRecs) { report("node " + std::to_string(n) + ": leaf record out of range"); continue; }
            recSeen[r]++;
            recBox[r] = sb;
            const Tri48& T = tris[r];
            const bool strict = refsOf[T.globalId] == 1 || (strictInst && strictInst[triRef[T.globalId].inst]);
            if(!strict) continue;
            const B3 tb = paddedTriBox(T, pad);
            for(int a = 0; a < 3; a++) if(tb.lo[a] < sb.lo[a] || tb.hi[a] > sb.hi[a]) { report("record " + std::to_string(r) + ": padded triangle box outside the boxes above it"); break; }
          }
        }
      }
    }
    for(uint32_t n = 0; n < nNodes; n++) if(nodeSeen[n] != 1) report("node " + std::to_string(n) + " reached " + std::to_string(nodeSeen[n]) + " times");
    for(uint32_t r = 0; r < nRecs; r++) if(recSeen[r] != 1) report("record " + std::to_string(r) + " reached " + std::to_string(recSeen[r]) + " times");
    for(uint32_t g = 0; g < nTris; g++) if(refsOf[g] == 0) report("triangle " + std::to_string(g) + " has no leaf record");
    // split triangles whose references were never refitted: point coverage
    if(bad == 0) {
      std::vector<std::vector<uint32_t>> recsOf(nTris);
      for(uint32_t r = 0; r < nRecs; r++) { const uint32_t g = tris[r].globalId; if(refsOf[g] > 1 && !(strictInst && strictInst[triRef[g].inst])) recsOf[g].push_back(r); }
      for(uint32_t g = 0; g < nTris; g++) {
        if(recsOf[g].empty()) continue;
        const Tri48& T = tris[recsOf[g][0]];
        for(int i = 0; i <= 8; i++) for(int j = 0; i + j <= 8; j++) {
          const double u = i / 8.0, v = j / 8.0;
          const double p[3] = {double(T.v0x) + u * T.e1x + v * T.e2x, double(T.v0y) + u * T.e1y + v * T.e2y, double(T.v0z) + u * T.e1z + v * T.e2z};
          bool in = false;
          for(uint32_t r : recsOf[g]) {
            const B3& b = recBox[r];
            if(p[0] >= b.lo[0] && p[0] <= b.hi[0] && p[1] >= b.lo[1] && p[1] <= b.hi[1] && p[2] >= b.lo[2] && p[2] <= b.hi[2]) { in = true; break; }
          }
          if(!in) { report("triangle " + std::to_string(g) + ": a point of it lies in none of its references' slot boxes"); i = 9; break; }
        }
      }
    }
  }
  if(msg && msgLen > 0) snprintf(msg, size_t(msgLen), "%s", first.c_str());
  return bad;
}

}  // extern "C"

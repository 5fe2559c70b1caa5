// accel_build_checker.cpp — test infrastructure of rt_rebuild_accel (include/rt_abi.h "Rebuilding on the device", csrc/accel_build.hip): the device
// builder restated in plain sequential C++ — leaf records, Morton keys, stable sort, binary radix tree, collapse to 8-wide nodes, record emission — and a structural
// check of a tree.  Compiled by tests/accel_build.py together with tests/refit_checker.cpp and csrc/bvh8_builder.cpp (g++, -ffp-contract=off, no GPU); the boxes come
// from rfc_refit of refit_checker.cpp in its full mode, as the device's come from the refit kernel.  The restatement is written to be read, not to be fast: the
// hierarchy is built by recursive splitting of key ranges and the boxes by recursion, where the device runs one thread per node and rounds.
#include "../cis-565-final-vr-raytracer_amd/csrc/bvh8_builder.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace rt;

namespace {

struct Bx { float lo[3], hi[3]; };

// ((m0 x + m1 y) + m2 z) + m3 per row
void toWorld(const float* m, const rt_vec3& q, float* o)
{
  for(int r = 0; r < 3; r++) o[r] = ((m[4 * r] * q.x + m[4 * r + 1] * q.y) + m[4 * r + 2] * q.z) + m[4 * r + 3];
}
Bx triBounds(const Tri48& T)
{
  const float v[3][3] = {{T.v0x, T.v0y, T.v0z}, {T.v0x + T.e1x, T.v0y + T.e1y, T.v0z + T.e1z}, {T.v0x + T.e2x, T.v0y + T.e2y, T.v0z + T.e2z}};
  Bx b;
  for(int c = 0; c < 3; c++) { b.lo[c] = std::min(std::min(v[0][c], v[1][c]), v[2][c]); b.hi[c] = std::max(std::max(v[0][c], v[1][c]), v[2][c]); }
  return b;
}
uint64_t spread(uint32_t v) { uint64_t x = 0; for(int i = 0; i < 21; i++) x |= uint64_t((v >> i) & 1u) << (3 * i); return x; }

struct Bin {                       // the binary radix tree over sorted positions [first, last]
  uint32_t first, last; int left, right;   // children: node index, or -(position + 1) for a leaf
  Bx box; float area;
};

struct Builder {
  std::vector<uint64_t> key;       // sorted
  std::vector<uint32_t> gid;       // sorted position -> globalId
  std::vector<Tri48> rec;          // by globalId
  std::vector<Bin> bin;

  // first differing bit between positions a and b, counted from the top: the key, then the position
  int prefix(uint32_t a, uint32_t b) const
  {
    const uint64_t x = key[a] ^ key[b];
    if(x) return __builtin_clzll(x);
    return 64 + __builtin_clz(a ^ b);
  }
  // the node of [first, last], last > first: split where the highest differing bit of (first, last) changes
  int build(uint32_t first, uint32_t last)
  {
    const int me = int(bin.size());
    bin.push_back(Bin{});
    const int common = prefix(first, last);
    uint32_t split = first;          // the last position that shares more than `common` bits with `first`
    for(uint32_t lo = first, hi = last; lo < hi;) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if(prefix(first, mid) > common) { lo = mid; split = mid; } else hi = mid - 1;
    }
    const int l = split == first ? -int(first + 1) : build(first, split);
    const int r = split + 1 == last ? -int(last + 1) : build(split + 1, last);
    Bin& B = bin[size_t(me)];
    B.first = first; B.last = last; B.left = l; B.right = r;
    const Bx a = boxOf(l), b = boxOf(r);
    for(int c = 0; c < 3; c++) { B.box.lo[c] = std::min(a.lo[c], b.lo[c]); B.box.hi[c] = std::max(a.hi[c], b.hi[c]); }
    const float dx = B.box.hi[0] - B.box.lo[0], dy = B.box.hi[1] - B.box.lo[1], dz = B.box.hi[2] - B.box.lo[2];
    B.area = (dx * dy + dy * dz) + dz * dx;
    return me;
  }
  Bx boxOf(int id) const { return id < 0 ? triBounds(rec[gid[size_t(-id - 1)]]) : bin[size_t(id)].box; }
  uint32_t trisOf(int id) const { return id < 0 ? 1u : bin[size_t(id)].last - bin[size_t(id)].first + 1u; }
  uint32_t firstOf(int id) const { return id < 0 ? uint32_t(-id - 1) : bin[size_t(id)].first; }
};

}  // namespace

extern "C" {

// The device builder restated.  scene: primMeshes / vertices / indices; inst: the device instance rows (current matrices); table: per globalId the host build's record
// (globalId, flags, alphaIdx, omm are taken from it); nodesOut: room for max(1, nTris) nodes, recsOut for nTris records.  The node boxes are NOT computed here (origin,
// exponents and box bytes are left 0 / 127): rfc_refit in its full mode makes them.  counts: nodes, levels.  Returns 0, 1 = deeper than maxLevels, 2 = internal.
int abc_build(const rt_scene_desc* scene, const DevInstance* inst, uint32_t nInst, const TriRef* triRef, const Tri48* table, uint32_t nTris, int maxLevels,
              Node8* nodesOut, Tri48* recsOut, uint32_t* counts)
{
  counts[0] = counts[1] = 0;
  if(nTris == 0) return 2;
  Builder B;
  // 1. records
  std::vector<uint8_t> flip(nInst, 0);
  for(uint32_t i = 0; i < nInst; i++) { float inv[12], det; inverseAffine(inst[i].o2w, inv, &det); flip[i] = det < 0.0f; }
  B.rec.assign(table, table + nTris);
  for(uint32_t g = 0; g < nTris; g++) {
    Tri48& T = B.rec[g];
    if(T.globalId != g) return 2;
    const TriRef ref = triRef[g];
    const rt_prim_mesh& pm = scene->primMeshes[inst[ref.inst].primMesh];
    float w[3][3];
    for(int k = 0; k < 3; k++) toWorld(inst[ref.inst].o2w, scene->vertices[pm.vertexOffset + scene->indices[pm.firstIndex + 3 * ref.prim + k]].position, w[k]);
    T.v0x = w[0][0]; T.v0y = w[0][1]; T.v0z = w[0][2];
    T.e1x = w[1][0] - w[0][0]; T.e1y = w[1][1] - w[0][1]; T.e1z = w[1][2] - w[0][2];
    T.e2x = w[2][0] - w[0][0]; T.e2y = w[2][1] - w[0][1]; T.e2z = w[2][2] - w[0][2];
    T.flags = flip[ref.inst] ? (T.flags | TRI_FLIP) : (T.flags & ~uint32_t(TRI_FLIP));
  }
  // 2. keys: centre of the triangle box, normalised to the box of all centres, 21 bits per axis, x above y above z
  std::vector<float> cen(size_t(nTris) * 3);
  float cmin[3] = {3e38f, 3e38f, 3e38f}, cmax[3] = {-3e38f, -3e38f, -3e38f};
  for(uint32_t g = 0; g < nTris; g++) {
    const Bx b = triBounds(B.rec[g]);
    for(int c = 0; c < 3; c++) { const float v = 0.5f * (b.lo[c] + b.hi[c]); cen[size_t(g) * 3 + c] = v; cmin[c] = std::min(cmin[c], v); cmax[c] = std::max(cmax[c], v); }
  }
  std::vector<std::pair<uint64_t, uint32_t>> order(nTris);
  for(uint32_t g = 0; g < nTris; g++) {
    uint32_t q[3] = {0, 0, 0};
    for(int c = 0; c < 3; c++) {
      const float ext = cmax[c] - cmin[c];
      if(ext > 0.f) { const float t = (cen[size_t(g) * 3 + c] - cmin[c]) / ext; q[c] = std::min(2097151u, uint32_t(t * 2097152.0f)); }
    }
    order[g] = {(spread(q[0]) << 2) | (spread(q[1]) << 1) | spread(q[2]), g};
  }
  std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
  B.key.resize(nTris); B.gid.resize(nTris);
  for(uint32_t i = 0; i < nTris; i++) { B.key[i] = order[i].first; B.gid[i] = order[i].second; }
  // 3. hierarchy
  const int root = nTris > 1 ? B.build(0, nTris - 1) : -1;
  // 4. collapse, breadth-first
  std::vector<Node8> nodes(1, Node8{});
  std::vector<int> wideRoot(1, root);
  uint32_t recTop = 0, first = 0, count = 1;
  int levels = 0;
  while(count > 0) {
    if(levels >= maxLevels) return 1;
    levels++;
    const uint32_t childBase0 = first + count;
    uint32_t nextCount = 0;
    for(uint32_t nd = first; nd < first + count; nd++) {
      int ch[8]; int nc = 0;
      const int r = wideRoot[nd];
      if(B.trisOf(r) <= 3u) ch[nc++] = r;
      else {
        ch[nc++] = B.bin[size_t(r)].left; ch[nc++] = B.bin[size_t(r)].right;
        for(;;) {
          int pick = -1; float bestA = -1.f;
          for(int i = 0; i < nc; i++) if(B.trisOf(ch[i]) > 3u && B.bin[size_t(ch[i])].area > bestA) { bestA = B.bin[size_t(ch[i])].area; pick = i; }
          if(pick < 0 || nc == 8) break;
          const Bin& P = B.bin[size_t(ch[pick])];
          ch[pick] = P.left; ch[nc++] = P.right;
        }
      }
      // slots: the host builder's octant rule
      Bx cb[8], nb;
      for(int c = 0; c < 3; c++) { nb.lo[c] = 3e38f; nb.hi[c] = -3e38f; }
      for(int i = 0; i < nc; i++) { cb[i] = B.boxOf(ch[i]); for(int c = 0; c < 3; c++) { nb.lo[c] = std::min(nb.lo[c], cb[i].lo[c]); nb.hi[c] = std::max(nb.hi[c], cb[i].hi[c]); } }
      int inSlot[8] = {-1, -1, -1, -1, -1, -1, -1, -1}; bool done[8] = {};
      for(int round = 0; round < nc; round++) {
        float bestC = -3e38f; int bc = -1, bs = -1;
        for(int i = 0; i < nc; i++) {
          if(done[i]) continue;
          float d[3];
          for(int c = 0; c < 3; c++) d[c] = 0.5f * (cb[i].lo[c] + cb[i].hi[c]) - 0.5f * (nb.lo[c] + nb.hi[c]);
          for(int s = 0; s < 8; s++) {
            if(inSlot[s] >= 0) continue;
            const float v = (d[0] * ((s & 1) ? 1.f : -1.f) + d[1] * ((s & 2) ? 1.f : -1.f)) + d[2] * ((s & 4) ? 1.f : -1.f);
            if(v > bestC || bc < 0) { bestC = v; bc = i; bs = s; }
          }
        }
        done[bc] = true; inSlot[bs] = bc;
      }
      Node8 W{};
      W.ex = W.ey = W.ez = 127;
      W.childBase = childBase0 + nextCount; W.triBase = recTop;
      uint32_t off = 0;
      for(int s = 0; s < 8; s++) {
        if(inSlot[s] < 0) continue;
        const int id = ch[inSlot[s]];
        const uint32_t cnt = B.trisOf(id);
        if(cnt > 3u) {
          W.imask |= uint8_t(1u << s); W.meta[s] = uint8_t((1u << 5) | (24u + uint32_t(s)));
          wideRoot.push_back(id); nodes.push_back(Node8{}); nextCount++;
        } else {
          W.meta[s] = uint8_t((((1u << cnt) - 1u) << 5) | off);
          for(uint32_t q = 0; q < cnt; q++) recsOut[recTop + off + q] = B.rec[B.gid[B.firstOf(id) + q]];
          off += cnt;
        }
      }
      recTop += off;
      nodes[nd] = W;
    }
    first += count; count = nextCount;
  }
  if(recTop != nTris || nodes.size() > std::max<size_t>(nTris, 1)) return 2;
  memcpy(nodesOut, nodes.data(), nodes.size() * sizeof(Node8));
  counts[0] = uint32_t(nodes.size()); counts[1] = uint32_t(levels);
  return 0;
}

// Structure of a tree, independent of how it was built: root at 0; the nodes of a level are one contiguous range that starts where the level above ends; a node's
// internal children are contiguous from childBase in slot order and the children of consecutive nodes follow each other; meta well-formed (internal 0b00111sss with
// sss = its slot and the imask bit set; leaf: unary count 1..3 above an offset < 32, offsets running in slot order from 0; empty 0 with no imask bit); a node's leaf
// records contiguous from triBase and the nodes' record ranges following each other in node order; every globalId exactly once; nRecs == nTris; the depth (levels)
// equals `depth` and is <= stackMax.  Returns the number of violations; msg describes the first.
int abc_check_structure(const Node8* nodes, uint32_t nNodes, const Tri48* recs, uint32_t nRecs, uint32_t nTris, int depth, int stackMax, char* msg, int msgLen)
{
  int bad = 0;
  std::string firstMsg;
  auto report = [&](const std::string& s) { if(bad++ == 0) firstMsg = s; };
  if(nRecs != nTris) report("record count " + std::to_string(nRecs) + " != triangle count " + std::to_string(nTris));
  std::vector<uint32_t> seen(nTris, 0);
  for(uint32_t r = 0; r < nRecs; r++) { if(recs[r].globalId >= nTris) report("record " + std::to_string(r) + ": globalId out of range"); else seen[recs[r].globalId]++; }
  for(uint32_t g = 0; g < nTris; g++) if(seen[g] != 1) report("globalId " + std::to_string(g) + " appears " + std::to_string(seen[g]) + " times");
  uint32_t first = 0, count = nNodes ? 1 : 0, recTop = 0;
  int levels = 0;
  while(count > 0 && size_t(first) + count <= nNodes) {
    levels++;
    uint32_t next = 0;
    const uint32_t childTop = first + count;
    for(uint32_t n = first; n < first + count; n++) {
      const Node8& N = nodes[n];
      const std::string at = "node " + std::to_string(n);
      uint32_t inner = 0, off = 0;
      for(int s = 0; s < 8; s++) {
        const uint32_t m = N.meta[s];
        const bool in = (N.imask >> s) & 1u;
        if(m == 0) { if(in) report(at + ": empty slot flagged internal"); continue; }
        if(in) { if(m != ((1u << 5) | (24u + uint32_t(s)))) report(at + ": internal meta malformed"); inner++; continue; }
        const uint32_t un = m >> 5, cnt = uint32_t(__builtin_popcount(un));
        if(!(un == 1u || un == 3u || un == 7u)) report(at + ": leaf count not unary 1..3");
        if((m & 31u) != off) report(at + ": leaf offsets do not run in slot order");
        off += cnt;
      }
      if(off > 32u) report(at + ": more than 32 leaf records");   // (every slot's first offset is < 32 by the 5-bit field; the sum is bounded by 8 x 3)
      if(inner && N.childBase != childTop + next) report(at + ": children not contiguous in node order");
      if(off && N.triBase != recTop) report(at + ": leaf records not contiguous in node order");
      if(inner + off == 0 && nTris > 0) report(at + ": empty node");
      next += inner; recTop += off;
    }
    first += count; count = next;
  }
  if(first != nNodes || count != 0) report("levels are not contiguous node ranges covering all nodes");
  if(recTop != nRecs) report("leaf slots cover " + std::to_string(recTop) + " of " + std::to_string(nRecs) + " records");
  if(levels != depth) report("depth " + std::to_string(levels) + " != reported " + std::to_string(depth));
  if(levels > stackMax) report("deeper than the traversal stack");
  if(msg && msgLen > 0) snprintf(msg, size_t(msgLen), "%s", firstMsg.c_str());
  return bad;
}

}  // extern "C"

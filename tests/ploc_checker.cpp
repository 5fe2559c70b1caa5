// ploc_checker.cpp — test infrastructure of the PLOC builder of rt_rebuild_accel (include/rt_abi.h "The PLOC builder", csrc/accel_build.hip): the
// device build restated in plain sequential C++ with a builder selector.  Records, keys and the stable sort are §19's; the binary hierarchy is either the recursive
// LBVH of tests/accel_build_checker.cpp (its Builder, included below as source) or PLOC — a plain vector of clusters, a double loop for the neighbour search, a
// sequential merge, recursion for the leaf ranges —; ONE collapse and emission follows for both, restated here because the old checker's lives inside abc_build.
// With the LBVH selector the output equals abc_build's word for word (tests/test_ploc_cpu.py), which pins this collapse to the one the device is already held to.
// Compiled by tests/ploc.py together with tests/refit_checker.cpp and csrc/bvh8_builder.cpp (g++, -ffp-contract=off, no GPU); the boxes of the wide nodes come from
// rfc_refit in its full mode.  Written to be read, not to be fast.
#include "accel_build_checker.cpp"

namespace {

// the binary tree in the conventions of the device's BuildArrays: ids < n - 1 are internal nodes, n - 1 + p is the leaf at position p of `val`; node 0 is the root
struct Bvh2 {
  uint32_t n = 0;
  std::vector<uint32_t> left, right, first, last;   // per internal node: children, and the positions its leaves occupy in val
  std::vector<Bx> box; std::vector<float> area;      // per internal node
  std::vector<uint32_t> val;                         // position -> globalId
  const std::vector<Tri48>* rec = nullptr;           // by globalId

  bool leaf(uint32_t id) const { return id >= n - 1; }
  uint32_t trisOf(uint32_t id) const { return leaf(id) ? 1u : last[id] - first[id] + 1u; }
  uint32_t firstOf(uint32_t id) const { return leaf(id) ? id - (n - 1) : first[id]; }
  Bx boxOf(uint32_t id) const { return leaf(id) ? triBounds((*rec)[val[id - (n - 1)]]) : box[id]; }
};

float areaOf(const Bx& b)
{
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  return (dx * dy + dy * dz) + dz * dx;
}
Bx unionOf(const Bx& a, const Bx& b)
{
  Bx u;
  for(int c = 0; c < 3; c++) { u.lo[c] = std::min(a.lo[c], b.lo[c]); u.hi[c] = std::max(a.hi[c], b.hi[c]); }
  return u;
}

// the recursive LBVH of the old checker, renamed into the conventions above (its node indices are preorder, its leaves -(position + 1))
Bvh2 fromLbvh(Builder& B, uint32_t n)
{
  Bvh2 T;
  T.n = n; T.val = B.gid; T.rec = &B.rec;
  if(n > 1) B.build(0, n - 1);
  auto id = [&](int x) { return x < 0 ? n - 1 + uint32_t(-x - 1) : uint32_t(x); };
  for(const Bin& b : B.bin) {
    T.left.push_back(id(b.left)); T.right.push_back(id(b.right)); T.first.push_back(b.first); T.last.push_back(b.last);
    T.box.push_back(b.box); T.area.push_back(b.area);
  }
  return T;
}

struct Cluster { uint32_t id; Bx box; uint32_t count; };

// leaf ranges, top-down: a node with (f, l) gives its left child (f, f + countLeft - 1) and its right child the rest; a leaf that lands at position p takes it
void assignRanges(Bvh2& T, const std::vector<uint32_t>& sortedGid, uint32_t id, uint32_t f, uint32_t l)
{
  T.first[id] = f; T.last[id] = l;
  const uint32_t cntL = T.trisOf(T.left[id]);   // (an internal child still carries (0, count - 1) from its merge)
  uint32_t* ch[2] = {&T.left[id], &T.right[id]};
  const uint32_t from[2] = {f, f + cntL}, to[2] = {f + cntL - 1, l};
  for(int k = 0; k < 2; k++) {
    if(T.leaf(*ch[k])) { T.val[from[k]] = sortedGid[*ch[k] - (T.n - 1)]; *ch[k] = T.n - 1 + from[k]; }
    else assignRanges(T, sortedGid, *ch[k], from[k], to[k]);
  }
}

// PLOC over the sorted records: 0 = built, 3 = no single cluster after maxIterations iterations, 2 = an iteration merged nothing (cannot happen)
int ploc(Bvh2& T, const std::vector<uint32_t>& sortedGid, const std::vector<Tri48>& rec, uint32_t radius, uint32_t maxIterations, uint32_t* iterations,
         uint32_t* firstNn = nullptr)   // firstNn: room for n words, the neighbour every position chose in the first iteration
{
  const uint32_t n = uint32_t(sortedGid.size());
  T.n = n; T.rec = &rec; T.val = sortedGid;
  *iterations = 0;
  if(n < 2) return 0;
  T.left.assign(n - 1, 0); T.right.assign(n - 1, 0); T.first.assign(n - 1, 0); T.last.assign(n - 1, 0); T.box.assign(n - 1, Bx{}); T.area.assign(n - 1, 0.f);
  std::vector<Cluster> cl(n);
  for(uint32_t i = 0; i < n; i++) cl[i] = Cluster{n - 1 + i, triBounds(rec[sortedGid[i]]), 1u};
  uint32_t made = 0;
  while(cl.size() > 1) {
    if(*iterations >= maxIterations) return 3;
    const long m = long(cl.size()), R = long(radius);
    // 1. neighbour: the j of the window that minimises (d(i, j), min(i, j), max(i, j)).  Walking j upwards and keeping the first of equal distances is that order:
    //    for j < i the pair is (j, i), for j > i it is (i, j), and i > every j below it.
    std::vector<long> nn(size_t(m), -1);
    for(long i = 0; i < m; i++) {
      float best = 0.f;
      for(long j = std::max(0l, i - R); j <= std::min(m - 1, i + R); j++) {
        if(j == i) continue;
        const float d = areaOf(unionOf(cl[size_t(i)].box, cl[size_t(j)].box));
        if(nn[size_t(i)] < 0 || d < best) { best = d; nn[size_t(i)] = j; }
      }
    }
    if(firstNn && *iterations == 0) for(long i = 0; i < m; i++) firstNn[i] = uint32_t(nn[size_t(i)]);
    // 2.-4. merge mutual pairs at the lower position, drop the upper, keep the rest; merge q of this iteration is node n - 2 - (made + q)
    std::vector<Cluster> next;
    uint32_t q = 0;
    for(long i = 0; i < m; i++) {
      const long j = nn[size_t(i)];
      if(nn[size_t(j)] != i) { next.push_back(cl[size_t(i)]); continue; }
      if(j < i) continue;
      const Cluster &a = cl[size_t(i)], &b = cl[size_t(j)];
      const uint32_t id = n - 2 - (made + q);
      q++;
      T.left[id] = a.id; T.right[id] = b.id; T.box[id] = unionOf(a.box, b.box); T.area[id] = areaOf(T.box[id]);
      T.first[id] = 0; T.last[id] = a.count + b.count - 1;
      next.push_back(Cluster{id, T.box[id], a.count + b.count});
    }
    if(q == 0) return 2;
    made += q;
    cl.swap(next);
    ++*iterations;
  }
  if(made != n - 1 || cl[0].id != 0) return 2;
  assignRanges(T, sortedGid, 0, 0, n - 1);
  return 0;
}

// steps 1 and 2 of the build, as accel_build_checker.cpp has them inside abc_build: the records by globalId with the current world-space vertices and flip bit, and
// (key, globalId) in the stable Morton order.  false: the table is not in globalId order.
bool recordsAndOrder(const rt_scene_desc* scene, const DevInstance* inst, uint32_t nInst, const TriRef* triRef, const Tri48* table, uint32_t nTris,
                     std::vector<Tri48>& rec, std::vector<std::pair<uint64_t, uint32_t>>& order)
{
  // 1. records
  rec.assign(table, table + nTris);
  std::vector<uint8_t> flip(nInst, 0);
  for(uint32_t i = 0; i < nInst; i++) { float inv[12], det; inverseAffine(inst[i].o2w, inv, &det); flip[i] = det < 0.0f; }
  for(uint32_t g = 0; g < nTris; g++) {
    Tri48& T = rec[g];
    if(T.globalId != g) return false;
    const TriRef ref = triRef[g];
    const rt_prim_mesh& pm = scene->primMeshes[inst[ref.inst].primMesh];
    float w[3][3];
    for(int k = 0; k < 3; k++) toWorld(inst[ref.inst].o2w, scene->vertices[pm.vertexOffset + scene->indices[pm.firstIndex + 3 * ref.prim + k]].position, w[k]);
    T.v0x = w[0][0]; T.v0y = w[0][1]; T.v0z = w[0][2];
    T.e1x = w[1][0] - w[0][0]; T.e1y = w[1][1] - w[0][1]; T.e1z = w[1][2] - w[0][2];
    T.e2x = w[2][0] - w[0][0]; T.e2y = w[2][1] - w[0][1]; T.e2z = w[2][2] - w[0][2];
    T.flags = flip[ref.inst] ? (T.flags | TRI_FLIP) : (T.flags & ~uint32_t(TRI_FLIP));
  }
  // 2. keys and the stable sort
  std::vector<float> cen(size_t(nTris) * 3);
  float cmin[3] = {3e38f, 3e38f, 3e38f}, cmax[3] = {-3e38f, -3e38f, -3e38f};
  for(uint32_t g = 0; g < nTris; g++) {
    const Bx b = triBounds(rec[g]);
    for(int c = 0; c < 3; c++) { const float v = 0.5f * (b.lo[c] + b.hi[c]); cen[size_t(g) * 3 + c] = v; cmin[c] = std::min(cmin[c], v); cmax[c] = std::max(cmax[c], v); }
  }
  order.assign(nTris, {0, 0});
  for(uint32_t g = 0; g < nTris; g++) {
    uint32_t q[3] = {0, 0, 0};
    for(int c = 0; c < 3; c++) {
      const float ext = cmax[c] - cmin[c];
      if(ext > 0.f) { const float t = (cen[size_t(g) * 3 + c] - cmin[c]) / ext; q[c] = std::min(2097151u, uint32_t(t * 2097152.0f)); }
    }
    order[g] = {(spread(q[0]) << 2) | (spread(q[1]) << 1) | spread(q[2]), g};
  }
  std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
  return true;
}

}  // namespace

extern "C" {

enum { PLC_LBVH = 0, PLC_PLOC = 1 };

// The device build restated, with a builder selector.  Arguments as abc_build's; radius and maxIterations are the values in force (no 0 = default here).
// counts: nodes, levels, PLOC merge iterations (0 for LBVH).  sah: sum over the wide nodes of A(node) / A(root), and of A(node) / A(root) x the node's leaf records,
// A = the float area of the binary node the wide node was opened from (both 0 when the root has no area).
// Returns 0, 1 = deeper than maxLevels, 2 = internal, 3 = PLOC did not reach one cluster in maxIterations iterations.
int plc_build(const rt_scene_desc* scene, const DevInstance* inst, uint32_t nInst, const TriRef* triRef, const Tri48* table, uint32_t nTris, int maxLevels,
              int builder, uint32_t radius, uint32_t maxIterations, Node8* nodesOut, Tri48* recsOut, uint32_t* counts, double* sah)
{
  counts[0] = counts[1] = counts[2] = 0; sah[0] = sah[1] = 0.0;
  if(nTris == 0) return 2;
  std::vector<Tri48> rec;
  std::vector<std::pair<uint64_t, uint32_t>> order;
  if(!recordsAndOrder(scene, inst, nInst, triRef, table, nTris, rec, order)) return 2;
  // 3. the binary hierarchy
  Builder B;
  Bvh2 T;
  if(builder == PLC_LBVH) {
    B.rec = rec; B.key.resize(nTris); B.gid.resize(nTris);
    for(uint32_t i = 0; i < nTris; i++) { B.key[i] = order[i].first; B.gid[i] = order[i].second; }
    T = fromLbvh(B, nTris);
    T.rec = &rec;
  } else if(builder == PLC_PLOC) {
    std::vector<uint32_t> sortedGid(nTris);
    for(uint32_t i = 0; i < nTris; i++) sortedGid[i] = order[i].second;
    if(const int rc = ploc(T, sortedGid, rec, radius, maxIterations, &counts[2])) return rc;
  } else return 2;
  // 4. collapse, breadth-first: the wide root is binary node 0 (the only leaf when there is one triangle: id 0 = n - 1 + 0)
  const float rootArea = areaOf(T.boxOf(0));
  std::vector<Node8> nodes(1, Node8{});
  std::vector<uint32_t> wideRoot(1, 0u);
  uint32_t recTop = 0, first = 0, count = 1;
  int levels = 0;
  while(count > 0) {
    if(levels >= maxLevels) return 1;
    levels++;
    const uint32_t childBase0 = first + count;
    uint32_t nextCount = 0;
    for(uint32_t nd = first; nd < first + count; nd++) {
      uint32_t ch[8]; int nc = 0;
      const uint32_t r = wideRoot[nd];
      if(T.trisOf(r) <= 3u) ch[nc++] = r;
      else {
        ch[nc++] = T.left[r]; ch[nc++] = T.right[r];
        for(;;) {   // open the child of largest area, the first of equals, until 8
          int pick = -1; float bestA = -1.f;
          for(int i = 0; i < nc; i++) if(T.trisOf(ch[i]) > 3u && T.area[ch[i]] > bestA) { bestA = T.area[ch[i]]; pick = i; }
          if(pick < 0 || nc == 8) break;
          const uint32_t p = ch[pick];
          ch[pick] = T.left[p]; ch[nc++] = T.right[p];
        }
      }
      // slots: the host builder's octant rule
      Bx cb[8], nb;
      for(int c = 0; c < 3; c++) { nb.lo[c] = 3e38f; nb.hi[c] = -3e38f; }
      for(int i = 0; i < nc; i++) { cb[i] = T.boxOf(ch[i]); for(int c = 0; c < 3; c++) { nb.lo[c] = std::min(nb.lo[c], cb[i].lo[c]); nb.hi[c] = std::max(nb.hi[c], cb[i].hi[c]); } }
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
        const uint32_t id = ch[inSlot[s]], cnt = T.trisOf(id);
        if(cnt > 3u) {
          W.imask |= uint8_t(1u << s); W.meta[s] = uint8_t((1u << 5) | (24u + uint32_t(s)));
          wideRoot.push_back(id); nodes.push_back(Node8{}); nextCount++;
        } else {
          W.meta[s] = uint8_t((((1u << cnt) - 1u) << 5) | off);
          for(uint32_t q = 0; q < cnt; q++) recsOut[recTop + off + q] = rec[T.val[T.firstOf(id) + q]];
          off += cnt;
        }
      }
      if(rootArea > 0.f) {
        const double rel = double(areaOf(T.boxOf(r))) / double(rootArea);
        sah[0] += rel; sah[1] += rel * double(off);
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

// What the tests of the tiny scenes look at and plc_build does not report: sortedGid[p] = the globalId at Morton position p; firstNn[p] = the position the cluster at
// p chose in PLOC's first iteration; finalGid = the leaf order after the range pass, of which the first *leftLeaves belong to the root's left child (0 when there is
// one triangle).  Room for nTris words each.  Returns plc_build's codes.
int plc_inspect(const rt_scene_desc* scene, const DevInstance* inst, uint32_t nInst, const TriRef* triRef, const Tri48* table, uint32_t nTris, uint32_t radius,
                uint32_t maxIterations, uint32_t* sortedGid, uint32_t* firstNn, uint32_t* finalGid, uint32_t* leftLeaves)
{
  *leftLeaves = 0;
  if(nTris == 0) return 2;
  std::vector<Tri48> rec;
  std::vector<std::pair<uint64_t, uint32_t>> order;
  if(!recordsAndOrder(scene, inst, nInst, triRef, table, nTris, rec, order)) return 2;
  std::vector<uint32_t> gid(nTris);
  for(uint32_t i = 0; i < nTris; i++) gid[i] = sortedGid[i] = order[i].second;
  Bvh2 T;
  uint32_t iterations = 0;
  if(const int rc = ploc(T, gid, rec, radius, maxIterations, &iterations, firstNn)) return rc;
  memcpy(finalGid, T.val.data(), size_t(nTris) * 4);
  if(nTris > 1) *leftLeaves = T.trisOf(T.left[0]);
  return 0;
}

}  // extern "C"

// accel_build.hip — the kernels of rt_rebuild_accel (accel_build.h), compiled once.  One thread per element, 256 threads per workgroup:
//   k_table      host-built leaf record -> the per-globalId table (once per host build)
//   (k_refit_tris of csrc/refit.hip writes v0 / e1 / e2 / TRI_FLIP of every table row from the current instance matrices: the leaf-record arithmetic exists once)
//   k_centres    triangle -> box centre; min / max of the centres (wave reduction, then vector atomics on an order-preserving encoding: min / max are exact)
//   k_keys       centre -> 63-bit Morton key (21 bits per axis)
//   hipcub::DeviceRadixSort::SortPairs (stable; its input is in globalId order, so equal keys stay in globalId order)
//   k_hierarchy  Karras 2012: one thread per internal node of the binary radix tree, equal keys told apart by their sorted position
//   k_union      binary node boxes, bottom-up in rounds: a node takes its children's boxes only when an EARLIER launch wrote them (the round stamp), so every
//                hand-off crosses a kernel boundary and needs no fence; as many rounds as the tree is high
//   (PLOC, opt-in, in place of k_hierarchy and k_union) per iteration k_ploc_neighbour — nearest cluster within `radius` Morton positions by the area
//                of the union box, boxes staged in LDS —, k_ploc_flags, hipcub::DeviceScan::ExclusiveSum, k_ploc_merge — mutual pairs become nodes, the rest is
//                compacted into the other cluster buffer —; then k_ploc_ranges top-down, one launch per iteration's nodes: the leaf order the collapse needs
//   k_collapse   one thread per wide node of a level: opens the binary child of largest surface area until 8, assigns slots by the host builder's octant rule
//   hipcub::DeviceScan::ExclusiveSum over the level's (internal children, leaf triangles) counts
//   k_emit       child base / triangle base, the next level's nodes, the leaf records at their final positions
//   (k_refit_level of csrc/refit.hip, deepest level first, full mode with every node marked: origin, exponents and box bytes)
// Float arithmetic is compiled with contraction off and written with one operation order; tests/accel_build_checker.cpp repeats it.
#include "accel_build.h"
#include "dev_math.h"
#include <hipcub/hipcub.hpp>

namespace rt {
namespace {

constexpr int AB_BLOCK = 256;
constexpr uint32_t AB_EMPTY = 0xffffffffu;

__device__ __forceinline__ uint32_t orderedBits(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float orderedFloat(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// the box of a record: v0, v0 + e1, v0 + e2 (the expressions of k_refit_level's leaf boxes)
__device__ __forceinline__ void triBox(const Tri48* table, uint32_t g, float lo[3], float hi[3])
{
  const uint4* rec = reinterpret_cast<const uint4*>(table + g);
  const float4 r0 = gLoadF4(rec), r1 = gLoadF4(rec + 1);
  const float e2z = __uint_as_float(gLoadU32(rec + 2));
  const float v[3][3] = {{r0.x, r0.y, r0.z}, {r0.x + r0.w, r0.y + r1.x, r0.z + r1.y}, {r0.x + r1.z, r0.y + r1.w, r0.z + e2z}};
  for(int c = 0; c < 3; c++) { lo[c] = fminf(fminf(v[0][c], v[1][c]), v[2][c]); hi[c] = fmaxf(fmaxf(v[0][c], v[1][c]), v[2][c]); }
}

__global__ __launch_bounds__(AB_BLOCK) void k_table(const Tri48* tris, uint32_t numRecs, Tri48* table, uint32_t n)
{
  const uint32_t r = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(r >= numRecs) return;
  const uint4* src = reinterpret_cast<const uint4*>(tris + r);
  const uint4 w2 = gLoadU4(src + 2);
  if(w2.y >= n) return;
  uint4* dst = reinterpret_cast<uint4*>(table + w2.y);
  dst[0] = gLoadU4(src); dst[1] = gLoadU4(src + 1); dst[2] = w2; dst[3] = gLoadU4(src + 3);
}

__global__ __launch_bounds__(AB_BLOCK) void k_centres(const Tri48* table, uint32_t n, float4* centre, uint32_t* bounds)
{
  const uint32_t g = blockIdx.x * AB_BLOCK + threadIdx.x;
  float mn[3] = {3e38f, 3e38f, 3e38f}, mx[3] = {-3e38f, -3e38f, -3e38f};
  if(g < n) {
    float lo[3], hi[3];
    triBox(table, g, lo, hi);
    for(int c = 0; c < 3; c++) mn[c] = mx[c] = 0.5f * (lo[c] + hi[c]);
    centre[g] = make_float4(mn[0], mn[1], mn[2], 0.f);
  }
  for(int c = 0; c < 3; c++)
    for(int o = 32; o > 0; o >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64)); }
  if((threadIdx.x & 63) == 0 && blockIdx.x * AB_BLOCK + (threadIdx.x & ~63u) < n)
    for(int c = 0; c < 3; c++) { atomicMin(bounds + c, orderedBits(mn[c])); atomicMax(bounds + 3 + c, orderedBits(mx[c])); }
}

__device__ __forceinline__ unsigned long long spread21(uint32_t v)   // bit i -> bit 3 i
{
  unsigned long long x = v & 0x1fffffu;
  x = (x | (x << 32)) & 0x1f00000000ffffull;
  x = (x | (x << 16)) & 0x1f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

__global__ __launch_bounds__(AB_BLOCK) void k_keys(const float4* centre, const uint32_t* bounds, uint32_t n, unsigned long long* key, uint32_t* val)
{
  const uint32_t g = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(g >= n) return;
  const float4 c4 = centre[g];
  const float c[3] = {c4.x, c4.y, c4.z};
  uint32_t q[3];
  for(int a = 0; a < 3; a++) {
    const float lo = orderedFloat(bounds[a]), ext = orderedFloat(bounds[3 + a]) - lo;
    q[a] = 0;
    if(ext > 0.f) {   // an axis of zero extent maps to 0
      const float t = (c[a] - lo) / ext;
      q[a] = min(2097151u, uint32_t(t * 2097152.0f));
    }
  }
  key[g] = (spread21(q[0]) << 2) | (spread21(q[1]) << 1) | spread21(q[2]);
  val[g] = g;
}

// length of the common prefix of sorted positions i and j; equal keys are told apart by the position
__device__ __forceinline__ int delta(const unsigned long long* key, long long n, long long i, long long j)
{
  if(j < 0 || j >= n) return -1;
  const unsigned long long x = key[i] ^ key[j];
  return x ? __clzll((long long)x) : 64 + __clz(int(uint32_t(i) ^ uint32_t(j)));
}

__global__ __launch_bounds__(AB_BLOCK) void k_hierarchy(const unsigned long long* key, uint32_t n, uint2* child, uint2* range)
{
  const long long i = (long long)blockIdx.x * AB_BLOCK + threadIdx.x;
  const long long N = n;
  if(i >= N - 1) return;
  const int d = delta(key, N, i, i + 1) - delta(key, N, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = delta(key, N, i, i - d);
  long long lmax = 2;
  while(delta(key, N, i, i + lmax * d) > dmin) lmax *= 2;
  long long l = 0;
  for(long long t = lmax / 2; t >= 1; t /= 2) if(delta(key, N, i, i + (l + t) * d) > dmin) l += t;
  const long long j = i + l * d;
  const int dnode = delta(key, N, i, j);
  long long s = 0, t = l;
  do { t = (t + 1) >> 1; if(delta(key, N, i, i + (s + t) * d) > dnode) s += t; } while(t > 1);
  const long long gamma = i + s * d + (d < 0 ? -1 : 0);
  const long long lo = i < j ? i : j, hi = i < j ? j : i;
  const uint32_t left = lo == gamma ? uint32_t(N - 1 + gamma) : uint32_t(gamma);
  const uint32_t right = hi == gamma + 1 ? uint32_t(N - 1 + gamma + 1) : uint32_t(gamma + 1);
  child[i] = make_uint2(left, right);
  range[i] = make_uint2(uint32_t(lo), uint32_t(hi));
}

struct BuildArrays {
  const Tri48* table; const uint32_t* val; const uint2* child; const uint2* range; float4* boxLo; float4* boxHi; uint32_t* stamp;
  uint32_t n;
};

__global__ __launch_bounds__(AB_BLOCK) void k_union(const BuildArrays b, const uint32_t round)
{
  const uint32_t i = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(i + 1 >= b.n || b.stamp[i] != 0u) return;   // (its own stamp: only this thread ever writes it)
  const uint2 ch = b.child[i];
  const uint32_t id[2] = {ch.x, ch.y};
  float lo[2][3], hi[2][3];
  for(int k = 0; k < 2; k++) {
    if(id[k] >= b.n - 1) triBox(b.table, b.val[id[k] - (b.n - 1)], lo[k], hi[k]);
    else {
      // another thread of this launch may be storing this stamp: a relaxed agent-scope atomic load (and store below), so the access is no data race and stays where it is
      const uint32_t s = __hip_atomic_load(b.stamp + id[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if(s == 0u || s >= round) return;   // not made yet, or made by this launch: its box is taken in a later round
      const float4 l = b.boxLo[id[k]], h = b.boxHi[id[k]];
      lo[k][0] = l.x; lo[k][1] = l.y; lo[k][2] = l.z; hi[k][0] = h.x; hi[k][1] = h.y; hi[k][2] = h.z;
    }
  }
  float L[3], H[3];
  for(int c = 0; c < 3; c++) { L[c] = fminf(lo[0][c], lo[1][c]); H[c] = fmaxf(hi[0][c], hi[1][c]); }
  const float dx = H[0] - L[0], dy = H[1] - L[1], dz = H[2] - L[2];
  const float area = (dx * dy + dy * dz) + dz * dx;
  b.boxLo[i] = make_float4(L[0], L[1], L[2], area);
  b.boxHi[i] = make_float4(H[0], H[1], H[2], 0.f);
  __hip_atomic_store(b.stamp + i, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- PLOC: the binary hierarchy by bottom-up clustering along the Morton order.  One iteration is four launches — neighbour, flags, scan, merge —
// and every hand-off between workgroups crosses a launch boundary: no flag, no fence and no atomic inside a launch.  The clusters are double buffered.
struct PlocClusters { uint32_t* id; float4* lo; float4* hi; };   // position -> binary node, box; hi.w = leaf count (bits)

__global__ __launch_bounds__(AB_BLOCK) void k_ploc_init(const Tri48* table, const uint32_t* val, uint32_t n, PlocClusters c)
{
  const uint32_t i = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(i >= n) return;
  float lo[3], hi[3];
  triBox(table, val[i], lo, hi);
  c.id[i] = n - 1 + i;
  c.lo[i] = make_float4(lo[0], lo[1], lo[2], 0.f);
  c.hi[i] = make_float4(hi[0], hi[1], hi[2], __uint_as_float(1u));
}

// nn[i] = the position j of [i - R, i + R], j != i, that minimises (area of the union box, min(i, j), max(i, j)).  Walking j upwards and keeping the first of equal
// areas is that order: below i the pair is (j, i), above it (i, j), and i is larger than every j below it.  The block's boxes and a halo of R on each side are staged
// in LDS as six float planes, so consecutive lanes read consecutive words.
__global__ __launch_bounds__(AB_BLOCK) void k_ploc_neighbour(const float4* lo, const float4* hi, const uint32_t m, const int R, uint32_t* nn)
{
  __shared__ float pl[6][AB_BLOCK + 2 * ACCEL_PLOC_RADIUS_MAX];
  const long long base = (long long)blockIdx.x * AB_BLOCK - R;   // the position of plane word 0
  for(int t = threadIdx.x; t < AB_BLOCK + 2 * R; t += AB_BLOCK) {
    const long long p = base + t;
    if(p >= 0 && p < (long long)m) {
      const float4 l = lo[p], h = hi[p];
      pl[0][t] = l.x; pl[1][t] = l.y; pl[2][t] = l.z; pl[3][t] = h.x; pl[4][t] = h.y; pl[5][t] = h.z;
    }
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * AB_BLOCK + threadIdx.x;
  if(i >= (long long)m) return;
  const int me = int(threadIdx.x) + R;
  const long long first = i - R > 0 ? i - R : 0, last = i + R < (long long)m - 1 ? i + R : (long long)m - 1;
  const float l0 = pl[0][me], l1 = pl[1][me], l2 = pl[2][me], h0 = pl[3][me], h1 = pl[4][me], h2 = pl[5][me];
  float best = 0.f; int bt = -1;
  for(int t = int(first - base); t <= int(last - base); t++) {
    if(t == me) continue;
    const float dx = fmaxf(h0, pl[3][t]) - fminf(l0, pl[0][t]), dy = fmaxf(h1, pl[4][t]) - fminf(l1, pl[1][t]), dz = fmaxf(h2, pl[5][t]) - fminf(l2, pl[2][t]);
    const float d = (dx * dy + dy * dz) + dz * dx;
    if(bt < 0 || d < best) { best = d; bt = t; }
  }
  nn[i] = uint32_t(base + bt);   // (m >= 2: the window holds at least one other position)
}

// keep flag << 32 | merge flag: a mutual pair merges at its lower position and its upper position goes
__global__ __launch_bounds__(AB_BLOCK) void k_ploc_flags(const uint32_t* nn, const uint32_t m, unsigned long long* flags)
{
  const uint32_t i = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(i >= m) return;
  const uint32_t j = nn[i];
  const bool mutual = nn[j] == i;
  flags[i] = ((unsigned long long)(mutual && j < i ? 0u : 1u) << 32) | (mutual && i < j ? 1u : 0u);
}

struct PlocNodes { uint2* child; uint2* range; float4* boxLo; float4* boxHi; uint32_t n; };

// merge q of an iteration that `made` nodes precede makes node n - 2 - (made + q): the ids run downwards and the last merge of the build is node 0, the root.
// range holds (0, leaves - 1) until k_ploc_ranges places the node.
__global__ __launch_bounds__(AB_BLOCK) void k_ploc_merge(const PlocClusters in, const PlocClusters out, const uint32_t* nn, const unsigned long long* scan, const uint32_t m,
                                                         const uint32_t made, const PlocNodes b, uint32_t* totals)
{
  const uint32_t i = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(i >= m) return;
  const uint32_t j = nn[i];
  const bool mutual = nn[j] == i, keep = !(mutual && j < i), merge = mutual && i < j;
  const unsigned long long sc = scan[i];
  const uint32_t pos = uint32_t(sc >> 32), q = uint32_t(sc & 0xffffffffull);
  if(i == m - 1) { totals[0] = pos + (keep ? 1u : 0u); totals[1] = q + (merge ? 1u : 0u); }
  if(!keep) return;
  const float4 li = in.lo[i], hi = in.hi[i];
  if(!merge) { out.id[pos] = in.id[i]; out.lo[pos] = li; out.hi[pos] = hi; return; }
  if(made + q + 2u > b.n) return;   // never: n - 1 merges make one cluster of n, and the host counts them
  const float4 lj = in.lo[j], hj = in.hi[j];
  const float L[3] = {fminf(li.x, lj.x), fminf(li.y, lj.y), fminf(li.z, lj.z)}, H[3] = {fmaxf(hi.x, hj.x), fmaxf(hi.y, hj.y), fmaxf(hi.z, hj.z)};
  const float dx = H[0] - L[0], dy = H[1] - L[1], dz = H[2] - L[2];
  const float area = (dx * dy + dy * dz) + dz * dx;
  const uint32_t cnt = __float_as_uint(hi.w) + __float_as_uint(hj.w), id = b.n - 2u - (made + q);
  b.child[id] = make_uint2(in.id[i], in.id[j]);
  b.range[id] = make_uint2(0u, cnt - 1u);
  b.boxLo[id] = make_float4(L[0], L[1], L[2], area);
  b.boxHi[id] = make_float4(H[0], H[1], H[2], 0.f);
  out.id[pos] = id;
  out.lo[pos] = make_float4(L[0], L[1], L[2], 0.f);
  out.hi[pos] = make_float4(H[0], H[1], H[2], __uint_as_float(cnt));
}

// The leaf order: the collapse and the emission need a subtree's records contiguous in val, which a PLOC subtree is not in Morton order.  Top-down, one launch per
// iteration's block of ids, the root's first (a node's children were made by earlier iterations, so its parent's launch has placed it): a node at (f, l) puts its
// left child at (f, f + leavesLeft - 1) and its right child behind it; a leaf child takes its position p, writes its globalId to the final val[p] and is renamed
// n - 1 + p.  Only a node's parent writes its range, and it reads the (0, leaves - 1) of the merge before it does.
__global__ __launch_bounds__(AB_BLOCK) void k_ploc_ranges(const PlocNodes b, const uint32_t* valSorted, uint32_t* valFinal, const uint32_t firstId, const uint32_t count)
{
  const uint32_t k = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(k >= count) return;
  const uint32_t id = firstId + k;
  const uint2 r = b.range[id];
  uint2 ch = b.child[id];
  const uint32_t cntL = ch.x >= b.n - 1 ? 1u : b.range[ch.x].y + 1u;
  if(ch.x >= b.n - 1) { valFinal[r.x] = valSorted[ch.x - (b.n - 1)]; ch.x = b.n - 1 + r.x; }
  else b.range[ch.x] = make_uint2(r.x, r.x + cntL - 1u);
  if(ch.y >= b.n - 1) { valFinal[r.x + cntL] = valSorted[ch.y - (b.n - 1)]; ch.y = b.n - 1 + r.x + cntL; }
  else b.range[ch.y] = make_uint2(r.x + cntL, r.y);
  b.child[id] = ch;
}

__device__ __forceinline__ uint32_t trisOf(const BuildArrays& b, uint32_t id) { if(id >= b.n - 1) return 1u; const uint2 r = b.range[id]; return r.y - r.x + 1u; }

union NodeWords { Node8 n; uint4 w[5]; __device__ NodeWords() {} };

__global__ __launch_bounds__(AB_BLOCK) void k_collapse(const BuildArrays b, const uint32_t first, const uint32_t count, const uint32_t* wideRoot, uint32_t* slotEntry,
                                                       unsigned long long* counts, Node8* nodes)
{
  const uint32_t k = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(k >= count) return;
  const uint32_t nd = first + k;
  const uint32_t root = wideRoot[nd];
  uint32_t ch[8]; int nc = 0;
  if(trisOf(b, root) <= 3u) ch[nc++] = root;   // (only the root of a scene of <= 3 triangles)
  else {
    const uint2 c0 = b.child[root];
    ch[nc++] = c0.x; ch[nc++] = c0.y;
    for(;;) {   // open the child of largest surface area; the first of equals
      int pick = -1; float bestA = -1.f;
      for(int i = 0; i < nc; i++) if(trisOf(b, ch[i]) > 3u) { const float A = b.boxLo[ch[i]].w; if(A > bestA) { bestA = A; pick = i; } }
      if(pick < 0 || nc == 8) break;
      const uint2 c = b.child[ch[pick]];
      ch[pick] = c.x; ch[nc++] = c.y;
    }
  }
  // slot assignment: the host builder's rule — the child whose centre lies furthest towards corner s gets slot s, greedy best pair
  float d[8][3];
  {
    float lo[8][3], hi[8][3], nlo[3] = {3e38f, 3e38f, 3e38f}, nhi[3] = {-3e38f, -3e38f, -3e38f};
    for(int i = 0; i < nc; i++) {
      if(ch[i] >= b.n - 1) triBox(b.table, b.val[ch[i] - (b.n - 1)], lo[i], hi[i]);
      else {
        const float4 l = b.boxLo[ch[i]], h = b.boxHi[ch[i]];
        lo[i][0] = l.x; lo[i][1] = l.y; lo[i][2] = l.z; hi[i][0] = h.x; hi[i][1] = h.y; hi[i][2] = h.z;
      }
      for(int c = 0; c < 3; c++) { nlo[c] = fminf(nlo[c], lo[i][c]); nhi[c] = fmaxf(nhi[c], hi[i][c]); }
    }
    for(int i = 0; i < nc; i++) for(int c = 0; c < 3; c++) d[i][c] = 0.5f * (lo[i][c] + hi[i][c]) - 0.5f * (nlo[c] + nhi[c]);
  }
  int inSlot[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  uint32_t done = 0u;
  for(int r = 0; r < nc; r++) {
    float bestC = -3e38f; int bc = -1, bs = -1;
    for(int i = 0; i < nc; i++) {
      if((done >> i) & 1u) continue;
      for(int s = 0; s < 8; s++) {
        if(inSlot[s] >= 0) continue;
        const float c = (d[i][0] * ((s & 1) ? 1.f : -1.f) + d[i][1] * ((s & 2) ? 1.f : -1.f)) + d[i][2] * ((s & 4) ? 1.f : -1.f);
        if(c > bestC || bc < 0) { bestC = c; bc = i; bs = s; }
      }
    }
    done |= 1u << bc; inSlot[bs] = bc;
  }
  NodeWords W;
  for(int q = 0; q < 5; q++) W.w[q] = make_uint4(0u, 0u, 0u, 0u);
  W.n.ex = W.n.ey = W.n.ez = 127;
  uint32_t inner = 0, triOff = 0;
  for(int s = 0; s < 8; s++) {
    uint32_t e = AB_EMPTY;
    if(inSlot[s] >= 0) {
      e = ch[inSlot[s]];
      const uint32_t cnt = trisOf(b, e);
      if(cnt > 3u) { W.n.imask |= uint8_t(1u << s); W.n.meta[s] = uint8_t((1u << 5) | (24u + uint32_t(s))); inner++; }
      else { W.n.meta[s] = uint8_t((((1u << cnt) - 1u) << 5) | triOff); triOff += cnt; }
    }
    slotEntry[size_t(nd) * 8 + s] = e;
  }
  uint4* out = reinterpret_cast<uint4*>(nodes + nd);
  for(int q = 0; q < 5; q++) out[q] = W.w[q];
  counts[nd] = ((unsigned long long)inner << 32) | triOff;
}

struct EmitArrays {
  Node8* nodes; Tri48* tris; AlphaRec* alphaByTri; uint32_t* recNode; const AlphaRec* alphaRec;
  uint32_t* wideRoot; const uint32_t* slotEntry; const unsigned long long* counts; const unsigned long long* scan; uint32_t* totals;
  uint32_t cap;
};

__global__ __launch_bounds__(AB_BLOCK) void k_emit(const BuildArrays b, const EmitArrays e, const uint32_t first, const uint32_t count, const uint32_t triTop)
{
  const uint32_t k = blockIdx.x * AB_BLOCK + threadIdx.x;
  if(k >= count) return;
  const uint32_t nd = first + k;
  const unsigned long long sc = e.scan[nd], cn = e.counts[nd];
  const unsigned long long childBase = (unsigned long long)first + count + (sc >> 32), triBase = (unsigned long long)triTop + (sc & 0xffffffffull);
  if(k == count - 1) { e.totals[0] = uint32_t((sc >> 32) + (cn >> 32)); e.totals[1] = uint32_t((sc & 0xffffffffull) + (cn & 0xffffffffull)); }
  if(childBase + (cn >> 32) > e.cap || triBase + (cn & 0xffffffffull) > b.n) { atomicOr(e.totals + 2, 1u); return; }   // never, by the counting argument of accel_build.h: nothing is written past a buffer
  uint32_t* w = reinterpret_cast<uint32_t*>(e.nodes + nd);
  w[4] = uint32_t(childBase); w[5] = uint32_t(triBase);
  uint32_t rel = 0, off = 0;
  for(int s = 0; s < 8; s++) {
    const uint32_t id = e.slotEntry[size_t(nd) * 8 + s];
    if(id == AB_EMPTY) continue;
    const uint32_t cnt = trisOf(b, id);
    if(cnt > 3u) { e.wideRoot[uint32_t(childBase) + rel] = id; rel++; continue; }
    const uint32_t pos0 = id >= b.n - 1 ? id - (b.n - 1) : b.range[id].x;
    for(uint32_t q = 0; q < cnt; q++) {
      const uint32_t g = b.val[pos0 + q], pos = uint32_t(triBase) + off + q;
      const uint4* src = reinterpret_cast<const uint4*>(b.table + g);
      const uint4 w2 = gLoadU4(src + 2);
      uint4* dst = reinterpret_cast<uint4*>(e.tris + pos);
      dst[0] = gLoadU4(src); dst[1] = gLoadU4(src + 1); dst[2] = w2; dst[3] = gLoadU4(src + 3);
      uint4* ad = reinterpret_cast<uint4*>(e.alphaByTri + pos);
      if(w2.z & TRI_OPAQUE) for(int x = 0; x < 4; x++) ad[x] = make_uint4(0u, 0u, 0u, 0u);
      else { const uint4* as = reinterpret_cast<const uint4*>(e.alphaRec + w2.w); for(int x = 0; x < 4; x++) ad[x] = gLoadU4(as + x); }
      e.recNode[pos] = nd;
    }
    off += cnt;
  }
}

inline dim3 gridOf(uint32_t n) { return dim3((n + AB_BLOCK - 1) / AB_BLOCK); }

}  // namespace

hipError_t accelBuildAlloc(AccelBuildWork& w, AccelBuildSet set[2], uint32_t triangles, std::vector<void*>& pool)
{
  const size_t n = triangles, cap = n > 0 ? n : 1, nb = n > 1 ? n - 1 : 1;
  hipError_t e = hipSuccess;
  auto get = [&](size_t bytes, auto** out) {
    if(e != hipSuccess) return;
    void* p = nullptr;
    e = hipMalloc(&p, bytes > 0 ? bytes : 16);
    if(e == hipSuccess) { pool.push_back(p); *out = static_cast<std::remove_reference_t<decltype(**out)>*>(p); }
  };
  size_t sortBytes = 0, scanBytes = 0;
  {
    unsigned long long* k = nullptr; uint32_t* v = nullptr;
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, k, k, v, v, int(cap), 0, 63);
    if(e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, k, k, int(cap));
  }
  w.sortTempBytes = sortBytes > scanBytes ? sortBytes : scanBytes;
  get(cap * sizeof(Tri48), &w.table); get(cap * sizeof(float4), &w.centre); get(6 * 4, &w.bounds);
  get(cap * 8, &w.keyIn); get(cap * 8, &w.keyOut); get(cap * 4, &w.valIn); get(cap * 4, &w.valOut);
  { char* t = nullptr; get(w.sortTempBytes, &t); w.sortTemp = t; }
  get(nb * sizeof(uint2), &w.child); get(nb * sizeof(uint2), &w.range); get(nb * sizeof(float4), &w.boxLo); get(nb * sizeof(float4), &w.boxHi); get(nb * 4, &w.stamp);
  get(cap * 4, &w.wideRoot); get(cap * 8 * 4, &w.slotEntry); get(cap * 8, &w.count); get(cap * 8, &w.scan); get(cap * 4, &w.nodeDirty); get(16, &w.totals);
  for(int s = 0; s < 2; s++) { get(cap * sizeof(Node8), &set[s].nodes); get(cap * sizeof(Tri48), &set[s].tris); get(cap * sizeof(AlphaRec), &set[s].alphaByTri); get(cap * 4, &set[s].recNode); }
  if(e == hipSuccess) { w.n = triangles; w.cap = uint32_t(cap); }
  return e;
}

hipError_t accelBuildAllocPloc(AccelBuildWork& w, std::vector<void*>& pool, bool* allocated)
{
  if(allocated) *allocated = false;
  if(w.clNn) return hipSuccess;
  const size_t cap = w.cap > 0 ? w.cap : 1;
  const size_t before = pool.size();
  hipError_t e = hipSuccess;
  auto get = [&](size_t bytes, auto** out) {
    if(e != hipSuccess) return;
    void* p = nullptr;
    e = hipMalloc(&p, bytes);
    if(e == hipSuccess) { pool.push_back(p); *out = static_cast<std::remove_reference_t<decltype(**out)>*>(p); }
  };
  AccelBuildWork t = w;
  for(int k = 0; k < 2; k++) { get(cap * 4, &t.clId[k]); get(cap * sizeof(float4), &t.clLo[k]); get(cap * sizeof(float4), &t.clHi[k]); }
  get(cap * 4, &t.clNn);
  if(e != hipSuccess) {   // all or nothing: the work keeps no pointer to what is freed here
    while(pool.size() > before) { (void)hipFree(pool.back()); pool.pop_back(); }
    return e;
  }
  w = t;
  if(allocated) *allocated = true;
  return hipSuccess;
}

hipError_t launchAccelTable(hipStream_t stream, const Tri48* tris, uint32_t numRecs, const AccelBuildWork& w)
{
  if(numRecs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_table, gridOf(numRecs), dim3(AB_BLOCK), 0, stream, tris, numRecs, w.table, w.n);
  return hipGetLastError();
}

#define AB_HIP(call) do { const hipError_t e_ = (call); if(e_ != hipSuccess) { *err = e_; (void)hipStreamSynchronize(stream); return ACCEL_BUILD_HIP; } } while(0)

int accelBuildRun(hipStream_t stream, AccelBuildWork& w, const AccelBuildSet& set, const RefitArgs& a, const AlphaRec* alphaRec, int maxLevels, hipEvent_t evSort[2],
                  AccelBuildResult& out, hipError_t* err)
{
  const uint32_t n = w.n;
  out.levels.clear(); out.nodes = 0;
  if(n == 0) return ACCEL_BUILD_COUNT;
  // 1. records: the table rows get the current world-space vertices and flip bit (k_refit_tris with every instance marked; its node marks go to word 0)
  AB_HIP(hipMemsetAsync(set.recNode, 0, size_t(n) * 4, stream));
  {
    RefitArgs t = a;
    t.tris = w.table; t.numRecs = n; t.recNode = set.recNode;
    AB_HIP(launchRefitTris(stream, t));
  }
  // 2. order
  {
    static const uint32_t init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    AB_HIP(hipMemcpyAsync(w.bounds, init, sizeof(init), hipMemcpyHostToDevice, stream));
  }
  hipLaunchKernelGGL(k_centres, gridOf(n), dim3(AB_BLOCK), 0, stream, w.table, n, w.centre, w.bounds);
  hipLaunchKernelGGL(k_keys, gridOf(n), dim3(AB_BLOCK), 0, stream, w.centre, w.bounds, n, w.keyIn, w.valIn);
  AB_HIP(hipGetLastError());
  AB_HIP(hipEventRecord(evSort[0], stream));
  {
    size_t bytes = w.sortTempBytes;
    AB_HIP(hipcub::DeviceRadixSort::SortPairs(w.sortTemp, bytes, w.keyIn, w.keyOut, w.valIn, w.valOut, int(n), 0, 63, stream));
  }
  AB_HIP(hipEventRecord(evSort[1], stream));
  // 3. binary hierarchy and its boxes
  BuildArrays b{w.table, w.valOut, w.child, w.range, w.boxLo, w.boxHi, w.stamp, n};
  w.iterations = 0;
  if(w.builder == ACCEL_BUILDER_PLOC) {
    // 3'. PLOC: clusters in Morton order merge with their nearest neighbour within `radius` positions until one is left; the host reads the cluster count back once
    // per iteration, as the collapse below reads its level size.  The boxes are made at merge time, so k_union's rounds are not needed.
    if(!w.clNn || w.radius < 1u || w.radius > uint32_t(ACCEL_PLOC_RADIUS_MAX)) { (void)hipStreamSynchronize(stream); return ACCEL_BUILD_PLOC_SETUP; }
    b.val = w.valIn;   // the final leaf order (free since the sort)
    const PlocClusters cl[2] = {{w.clId[0], w.clLo[0], w.clHi[0]}, {w.clId[1], w.clLo[1], w.clHi[1]}};
    const PlocNodes pn{w.child, w.range, w.boxLo, w.boxHi, n};
    hipLaunchKernelGGL(k_ploc_init, gridOf(n), dim3(AB_BLOCK), 0, stream, w.table, w.valOut, n, cl[0]);
    AB_HIP(hipGetLastError());
    std::vector<std::pair<uint32_t, uint32_t>> blocks;   // per iteration: (nodes made before it, nodes it made)
    uint32_t m = n, made = 0;
    int cur = 0;
    while(m > 1) {
      if(w.iterations >= w.maxIterations) { (void)hipStreamSynchronize(stream); return ACCEL_BUILD_PLOC_ITERATIONS; }
      hipLaunchKernelGGL(k_ploc_neighbour, gridOf(m), dim3(AB_BLOCK), 0, stream, cl[cur].lo, cl[cur].hi, m, int(w.radius), w.clNn);
      hipLaunchKernelGGL(k_ploc_flags, gridOf(m), dim3(AB_BLOCK), 0, stream, w.clNn, m, w.count);
      AB_HIP(hipGetLastError());
      size_t bytes = w.sortTempBytes;
      AB_HIP(hipcub::DeviceScan::ExclusiveSum(w.sortTemp, bytes, w.count, w.scan, int(m), stream));
      hipLaunchKernelGGL(k_ploc_merge, gridOf(m), dim3(AB_BLOCK), 0, stream, cl[cur], cl[cur ^ 1], w.clNn, w.scan, m, made, pn, w.totals);
      AB_HIP(hipGetLastError());
      uint32_t totals[2] = {0, 0};
      AB_HIP(hipMemcpyAsync(totals, w.totals, 8, hipMemcpyDeviceToHost, stream));
      AB_HIP(hipStreamSynchronize(stream));
      if(totals[1] == 0u || totals[0] + totals[1] != m) return ACCEL_BUILD_PLOC_NO_MERGE;   // the smallest pair of the total order is always mutual
      blocks.push_back({made, totals[1]});
      made += totals[1]; m = totals[0]; cur ^= 1;
      w.iterations++;
    }
    if(made != n - 1) return ACCEL_BUILD_COUNT;
    if(n == 1) AB_HIP(hipMemcpyAsync(w.valIn, w.valOut, 4, hipMemcpyDeviceToDevice, stream));
    for(size_t t = blocks.size(); t-- > 0;)
      hipLaunchKernelGGL(k_ploc_ranges, gridOf(blocks[t].second), dim3(AB_BLOCK), 0, stream, pn, w.valOut, w.valIn, n - 1u - (blocks[t].first + blocks[t].second), blocks[t].second);
    AB_HIP(hipGetLastError());
  } else if(n > 1) {
    AB_HIP(hipMemsetAsync(w.stamp, 0, size_t(n - 1) * 4, stream));
    hipLaunchKernelGGL(k_hierarchy, gridOf(n - 1), dim3(AB_BLOCK), 0, stream, w.keyOut, n, w.child, w.range);
    AB_HIP(hipGetLastError());
    // a binary radix tree over 63 key bits + 32 position bits is at most 95 high; the root (node 0) is made last
    uint32_t rootStamp = 0, round = 0;
    while(rootStamp == 0u) {
      if(round >= 128u) return ACCEL_BUILD_NO_ROOT;
      for(int r = 0; r < 8; r++) { round++; hipLaunchKernelGGL(k_union, gridOf(n - 1), dim3(AB_BLOCK), 0, stream, b, round); }
      AB_HIP(hipGetLastError());
      AB_HIP(hipMemcpyAsync(&rootStamp, w.stamp, 4, hipMemcpyDeviceToHost, stream));
      AB_HIP(hipStreamSynchronize(stream));
    }
  }
  // 4. collapse, level by level
  EmitArrays e{set.nodes, set.tris, set.alphaByTri, set.recNode, alphaRec, w.wideRoot, w.slotEntry, w.count, w.scan, w.totals, w.cap};
  AB_HIP(hipMemsetAsync(w.wideRoot, 0, 4, stream));   // the root: internal node 0, or the only leaf
  AB_HIP(hipMemsetAsync(w.totals, 0, 16, stream));
  uint32_t first = 0, count = 1, triTop = 0;
  while(count > 0) {
    if(int(out.levels.size()) >= maxLevels) { (void)hipStreamSynchronize(stream); return ACCEL_BUILD_TOO_DEEP; }
    if(size_t(first) + count > w.cap) { (void)hipStreamSynchronize(stream); return ACCEL_BUILD_CAPACITY; }
    out.levels.push_back({first, count});
    hipLaunchKernelGGL(k_collapse, gridOf(count), dim3(AB_BLOCK), 0, stream, b, first, count, w.wideRoot, w.slotEntry, w.count, set.nodes);
    AB_HIP(hipGetLastError());
    size_t bytes = w.sortTempBytes;
    AB_HIP(hipcub::DeviceScan::ExclusiveSum(w.sortTemp, bytes, w.count + first, w.scan + first, int(count), stream));
    hipLaunchKernelGGL(k_emit, gridOf(count), dim3(AB_BLOCK), 0, stream, b, e, first, count, triTop);
    AB_HIP(hipGetLastError());
    uint32_t totals[4] = {0, 0, 0, 0};
    AB_HIP(hipMemcpyAsync(totals, w.totals, 16, hipMemcpyDeviceToHost, stream));
    AB_HIP(hipStreamSynchronize(stream));
    if(totals[2]) return ACCEL_BUILD_CAPACITY;
    first += count; count = totals[0]; triTop += totals[1];
  }
  if(triTop != n) return ACCEL_BUILD_COUNT;
  out.nodes = first;
  // 5. boxes: the refit kernel over every node, deepest level first
  AB_HIP(hipMemsetAsync(w.nodeDirty, 1, size_t(w.cap) * 4, stream));
  for(size_t l = out.levels.size(); l-- > 0;) AB_HIP(launchRefitLevel(stream, a, out.levels[l].first, out.levels[l].second));
  return ACCEL_BUILD_OK;
}
#undef AB_HIP

const char* accelBuildWhy(int code)
{
  switch(code) {
    case ACCEL_BUILD_TOO_DEEP: return "BVH8 deeper than the traversal stack";
    case ACCEL_BUILD_PLOC_ITERATIONS: return "PLOC did not reach one cluster within maxIterations merge iterations";
    case ACCEL_BUILD_PLOC_NO_MERGE: return "internal error: a PLOC iteration merged no pair";
    case ACCEL_BUILD_PLOC_SETUP: return "internal error: a PLOC build without its cluster buffers or with a radius outside 1..64";
    case ACCEL_BUILD_NO_ROOT: return "internal error: the binary tree's boxes did not reach the root in 128 rounds";
    case ACCEL_BUILD_CAPACITY: return "internal error: the wide nodes or leaf records of a level do not fit the buffers sized for them";
    case ACCEL_BUILD_COUNT: return "internal error: the leaf slots do not hold every triangle exactly once";
    default: return "the device build did not complete";
  }
}

}  // namespace rt

// refit.hip — the two kernels of rt_update_instances (include/rt_abi.h), compiled once.
//   k_refit_tris   one thread per leaf record: the records of moved instances get their new world-space v0 / e1 / e2 and flip bit; the node that holds the record is marked.
//   k_refit_level  one thread per node of one level, deepest level first: a marked node, or one with a refitted internal child, gets new child boxes on a new grid —
//                  the builder's quantiser (csrc/bvh8_builder.cpp, "quantisation grid") restated for the device.
// Both are bound by dependent 16-byte gathers (record -> triRef -> instance -> prim mesh -> 3 indices -> 3 vertices; node -> 8 children / 3 records per slot), not by
// arithmetic: one thread per item, 256 threads per workgroup, every record and node read and written as 16-byte vectors.  tests/refit_checker.cpp restates both in plain C++.
#include "refit.h"
#include "dev_math.h"

namespace rt {
namespace {

constexpr int REFIT_BLOCK = 256;

__device__ __forceinline__ bool bitOf(const uint32_t* bits, uint32_t i) { return (gLoadU32(bits + (i >> 5)) >> (i & 31u)) & 1u; }

struct Rec { uint4 w[4]; };   // a Tri48 as its four 16-byte words: (v0.xyz, e1.x) (e1.yz, e2.xy) (e2.z, globalId, flags, alphaIdx) (omm)

__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_tris(const RefitArgs a)
{
  const uint32_t i = blockIdx.x * REFIT_BLOCK + threadIdx.x;
  if(i >= a.numRecs) return;
  const uint4* rec = reinterpret_cast<const uint4*>(a.tris + i);
  const uint4 w2 = gLoadU4(rec + 2);
  const uint32_t inst = gLoadU2(a.triRef + w2.y).x;
  const bool dirty = bitOf(a.dirtyBits, inst);
  if(dirty) {
    const uint32_t prim = gLoadU2(a.triRef + w2.y).y;
    const DevInstance* di = a.instances + inst;
    float m[12];
    for(int k = 0; k < 3; k++) { const float4 r = gLoadF4(di->o2w + 4 * k); m[4 * k] = r.x; m[4 * k + 1] = r.y; m[4 * k + 2] = r.z; m[4 * k + 3] = r.w; }
    const rt_prim_mesh* pm = a.primMeshes + gLoadU32(&di->primMesh);
    const uint32_t vertexOffset = gLoadU32(&pm->vertexOffset), firstIndex = gLoadU32(&pm->firstIndex);
    float w[3][3];
    for(int k = 0; k < 3; k++) {
      const uint32_t ix = gLoadU32(a.indices + firstIndex + 3 * prim + k);
      const float4 p = gLoadF4(a.vertices + vertexOffset + ix);   // (position.xyz, normal bits)
      xformPointRaw(m, p.x, p.y, p.z, w[k]);
    }
    const float e1x = w[1][0] - w[0][0], e1y = w[1][1] - w[0][1], e1z = w[1][2] - w[0][2];
    const float e2x = w[2][0] - w[0][0], e2y = w[2][1] - w[0][1], e2z = w[2][2] - w[0][2];
    const uint32_t flags = (w2.z & ~uint32_t(TRI_FLIP)) | (bitOf(a.flipBits, inst) ? uint32_t(TRI_FLIP) : 0u);
    uint4* out = reinterpret_cast<uint4*>(a.tris + i);
    out[0] = make_uint4(__float_as_uint(w[0][0]), __float_as_uint(w[0][1]), __float_as_uint(w[0][2]), __float_as_uint(e1x));
    out[1] = make_uint4(__float_as_uint(e1y), __float_as_uint(e1z), __float_as_uint(e2x), __float_as_uint(e2y));
    out[2] = make_uint4(__float_as_uint(e2z), w2.y, flags, w2.w);
    atomicAdd(a.counters, 1u);
  }
  if(dirty || a.full) a.nodeDirty[gLoadU32(a.recNode + i)] = 1u;
}

struct Box3 { float lo[3], hi[3]; };

__device__ __forceinline__ void growPoint(Box3& b, float x, float y, float z)
{
  b.lo[0] = fminf(b.lo[0], x); b.lo[1] = fminf(b.lo[1], y); b.lo[2] = fminf(b.lo[2], z);
  b.hi[0] = fmaxf(b.hi[0], x); b.hi[1] = fmaxf(b.hi[1], y); b.hi[2] = fmaxf(b.hi[2], z);
}

// a node as the five 16-byte words it is read and written as
union NodeWords { Node8 n; uint4 w[5]; __device__ NodeWords() {} };

__device__ __forceinline__ void loadNode(const Node8* p, NodeWords& N)
{
  for(int k = 0; k < 5; k++) N.w[k] = gLoadU4(reinterpret_cast<const uint4*>(p) + k);
}

// the box a node's own planes describe: the union of its occupied slots' decoded boxes
__device__ void decodeNodeBox(const Node8& C, Box3& b)
{
  const float st[3] = {ldexpf(1.0f, int(C.ex) - 127), ldexpf(1.0f, int(C.ey) - 127), ldexpf(1.0f, int(C.ez) - 127)};
  for(int a = 0; a < 3; a++) { b.lo[a] = 3e38f; b.hi[a] = -3e38f; }
  for(int t = 0; t < 8; t++) {
    if(C.meta[t] == 0) continue;
    b.lo[0] = fminf(b.lo[0], C.px + float(C.qlox[t]) * st[0]); b.hi[0] = fmaxf(b.hi[0], C.px + float(C.qhix[t]) * st[0]);
    b.lo[1] = fminf(b.lo[1], C.py + float(C.qloy[t]) * st[1]); b.hi[1] = fmaxf(b.hi[1], C.py + float(C.qhiy[t]) * st[1]);
    b.lo[2] = fminf(b.lo[2], C.pz + float(C.qloz[t]) * st[2]); b.hi[2] = fmaxf(b.hi[2], C.pz + float(C.qhiz[t]) * st[2]);
  }
}

__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_level(const RefitArgs a, const uint32_t first, const uint32_t count)
{
  const uint32_t k = blockIdx.x * REFIT_BLOCK + threadIdx.x;
  if(k >= count) return;
  const uint32_t n = first + k;
  NodeWords N;
  loadNode(a.nodes + n, N);
  const Node8& O = N.n;
  bool work = a.nodeDirty[n] != 0u;
  {
    uint32_t rel = 0;
    for(int s = 0; s < 8; s++) if((O.imask >> s) & 1u) { if(a.nodeDirty[O.childBase + rel] != 0u) work = true; rel++; }
  }
  if(!work) return;

  // ---- the box of every occupied slot ----
  const uint8_t* oq[6] = {O.qlox, O.qloy, O.qloz, O.qhix, O.qhiy, O.qhiz};
  const float op[3] = {O.px, O.py, O.pz};
  const int oex[3] = {int(O.ex) - 127, int(O.ey) - 127, int(O.ez) - 127};
  Box3 box[8]; bool kept[8];
  Box3 nb;
  for(int c = 0; c < 3; c++) { nb.lo[c] = 3e38f; nb.hi[c] = -3e38f; }
  uint32_t rel = 0;
  for(int s = 0; s < 8; s++) {
    kept[s] = false;
    if(O.meta[s] == 0) continue;
    Box3& b = box[s];
    if((O.imask >> s) & 1u) {   // an internal child: its own box, from its (already refitted) planes
      NodeWords C;
      loadNode(a.nodes + O.childBase + rel, C);
      rel++;
      decodeNodeBox(C.n, b);
    } else {
      const uint32_t cnt = uint32_t(__popc(uint32_t(O.meta[s]) >> 5)), off = uint32_t(O.meta[s]) & 31u;
      bool touched = a.full != 0;
      for(uint32_t q = 0; q < cnt && !touched; q++) {
        const uint32_t gid = gLoadU4(reinterpret_cast<const uint4*>(a.tris + O.triBase + off + q) + 2).y;
        touched = bitOf(a.dirtyBits, gLoadU2(a.triRef + gid).x);
      }
      if(touched) {             // the full triangles of the slot, widened by the pad
        for(int c = 0; c < 3; c++) { b.lo[c] = 3e38f; b.hi[c] = -3e38f; }
        for(uint32_t q = 0; q < cnt; q++) {
          const uint4* rec = reinterpret_cast<const uint4*>(a.tris + O.triBase + off + q);
          const float4 r0 = gLoadF4(rec), r1 = gLoadF4(rec + 1);
          const float e2z = __uint_as_float(gLoadU32(rec + 2));
          growPoint(b, r0.x, r0.y, r0.z);
          growPoint(b, r0.x + r0.w, r0.y + r1.x, r0.z + r1.y);
          growPoint(b, r0.x + r1.z, r0.y + r1.w, r0.z + e2z);
        }
        for(int c = 0; c < 3; c++) { b.lo[c] -= a.pad; b.hi[c] += a.pad; }
      } else {                  // untouched: the box its bytes describe; the bytes stay where the grid of an axis stays
        kept[s] = true;
        for(int c = 0; c < 3; c++) {
          const float st = ldexpf(1.0f, oex[c]);
          b.lo[c] = op[c] + float(oq[c][s]) * st; b.hi[c] = op[c] + float(oq[c + 3][s]) * st;
        }
      }
    }
    for(int c = 0; c < 3; c++) { nb.lo[c] = fminf(nb.lo[c], b.lo[c]); nb.hi[c] = fmaxf(nb.hi[c], b.hi[c]); }
  }

  // ---- the builder's quantiser: smallest power-of-two step with extent / step <= 255, bumped until every child fits ----
  NodeWords W;
  for(int q = 0; q < 5; q++) W.w[q] = N.w[q];
  W.n.px = nb.lo[0]; W.n.py = nb.lo[1]; W.n.pz = nb.lo[2];
  uint8_t* wq[6] = {W.n.qlox, W.n.qloy, W.n.qloz, W.n.qhix, W.n.qhiy, W.n.qhiz};
  int ex[3];
  for(int c = 0; c < 3; c++) {
    const float ext = nb.hi[c] - nb.lo[c];
    int e = -60;
    if(ext > 0) { int fe; (void)frexpf(ext / 255.f, &fe); e = fe; }
    ex[c] = max(-100, min(100, e));
    const float p = nb.lo[c];
    const bool sameOrigin = __float_as_uint(p) == __float_as_uint(op[c]);
    for(;;) {
      const float step = ldexpf(1.0f, ex[c]);
      const bool sameGrid = sameOrigin && ex[c] == oex[c];
      bool ok = true;
      for(int s = 0; s < 8 && ok; s++) {
        if(O.meta[s] == 0) { wq[c][s] = 0; wq[c + 3][s] = 0; continue; }
        if(kept[s] && sameGrid) { wq[c][s] = oq[c][s]; wq[c + 3][s] = oq[c + 3][s]; continue; }
        const float lo = box[s].lo[c], hi = box[s].hi[c];
        int ql = int(floor((double(lo) - double(p)) / double(step)));
        ql = max(0, min(255, ql));
        while(ql > 0 && p + float(ql) * step > lo) ql--;
        int qh = int(ceil((double(hi) - double(p)) / double(step)));
        qh = max(0, qh);
        while(qh <= 255 && p + float(qh) * step < hi) qh++;
        if(qh > 255) { ok = false; break; }
        wq[c][s] = uint8_t(ql); wq[c + 3][s] = uint8_t(qh);
      }
      if(ok) break;
      ex[c]++;
    }
  }
  W.n.ex = uint8_t(ex[0] + 127); W.n.ey = uint8_t(ex[1] + 127); W.n.ez = uint8_t(ex[2] + 127);
  uint4* out = reinterpret_cast<uint4*>(a.nodes + n);
  for(int q = 0; q < 5; q++) out[q] = W.w[q];
  a.nodeDirty[n] = 1u;
  atomicAdd(a.counters + 1, 1u);
}

}  // namespace

hipError_t launchRefitTris(hipStream_t stream, const RefitArgs& a)
{
  if(a.numRecs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_refit_tris, dim3((a.numRecs + REFIT_BLOCK - 1) / REFIT_BLOCK), dim3(REFIT_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launchRefitLevel(hipStream_t stream, const RefitArgs& a, uint32_t first, uint32_t count)
{
  if(count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_refit_level, dim3((count + REFIT_BLOCK - 1) / REFIT_BLOCK), dim3(REFIT_BLOCK), 0, stream, a, first, count);
  return hipGetLastError();
}

}  // namespace rt

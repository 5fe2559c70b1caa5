// materials.hip — the kernels of rt_update_materials / rt_update_texture (materials.h), compiled once.  Wave64 throughout.
//   k_mat_select   one thread per leaf record, 256 per workgroup.  A record without TRI_OPAQUE is selected when the material of triRef[globalId] -> instance ->
//                  prim mesh is dirty (an index below 0 reads material 0, as the host's alphaTemplate does).  Several records may share one alphaIdx (spatial-split
//                  references on a host tree; every instance of a mesh after rt_set_instances): a compare-and-swap on owner[alphaIdx] elects one of them, the
//                  owners are compacted with one ballot and one atomic per wave.  Which reference wins differs from run to run; no output depends on it: every
//                  reference of an alphaIdx has the same material, and the build below reads nothing else of the record.
//   k_mat_build    one wave per owner.  Lane 0 rewrites the alpha record from the material and texture rows (the uvs stay: no edit changes them).  Lanes 0..35
//                  compute the 36 cell footprints (opacity_map.h ommCellFootprint, double arithmetic).  Then, cell by cell, the wave scans the footprint's box:
//                  the box is numbered row by row and lane l takes texels l, l + 64, ..., so the lanes of one load run along x and the dword loads of BGRA texels
//                  coalesce wherever the wrap does not fold them (alpha is byte 3).  min / max are reduced across the wave with xor shuffles, lane `cell`
//                  keeps the state (ommCellState), the four words are assembled in LDS and lane 0 stores them to ommPlane[alphaIdx].
//   k_mat_scatter  one thread per leaf record: a selected record copies the four words into Tri48::omm (and into the builder's table row of its triangle, where
//                  there is one) and the alpha record into alphaByTri.
// Integer and double arithmetic only; the unit is built with -ffp-contract=off like every other.  Every index read from a record is checked against its array
// before it is used: a record the host did not write comes back as "not selected", never as an access outside a buffer.
#include "materials.h"
#include "opacity_map.h"
#include "dev_math.h"

namespace rt {
namespace {

constexpr int MAT_BLOCK = 256;

__device__ __forceinline__ void gStoreU4(void* p, uint4 v) { u32x4_t w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; *(RT_AS_GLOBAL u32x4_t*)p = w; }

// (e2z, globalId, flags, alphaIdx): the third 16 bytes of a leaf record
__device__ __forceinline__ uint4 recordIds(const Tri48* t) { return gLoadU4(reinterpret_cast<const uint4*>(t) + 2); }

// the material of the triangle with this globalId, or 0xffffffff where an index on the way is outside its array
__device__ __forceinline__ uint32_t materialOf(const MaterialArgs& a, uint32_t g)
{
  if(g >= a.numGlobal) return 0xffffffffu;
  const uint32_t inst = gLoadU32(&a.triRef[g].inst);
  if(inst >= a.numInstances) return 0xffffffffu;
  const uint32_t mesh = gLoadU32(&a.instances[inst].primMesh);
  if(mesh >= a.numPrimMeshes) return 0xffffffffu;
  const int32_t mi = int32_t(gLoadU32(&a.primMeshes[mesh].materialIndex));
  const uint32_t m = mi > 0 ? uint32_t(mi) : 0u;
  return m < a.numMaterials ? m : 0xffffffffu;
}

// selected: not opaque, alphaIdx inside the records, material dirty
__device__ __forceinline__ bool selected(const MaterialArgs& a, uint32_t i, uint4& ids)
{
  ids = recordIds(a.tris + i);
  if((ids.z & TRI_OPAQUE) || ids.w >= a.numAlpha) return false;
  const uint32_t m = materialOf(a, ids.y);
  return m != 0xffffffffu && ((gLoadU32(a.dirtyBits + (m >> 5)) >> (m & 31u)) & 1u) != 0u;
}

__global__ __launch_bounds__(MAT_BLOCK) void k_mat_select(const MaterialArgs a)
{
  const uint32_t i = blockIdx.x * MAT_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
  bool sel = false, own = false;
  if(i < a.numRecs) {
    uint4 ids;
    sel = selected(a, i, ids);
    if(sel) own = atomicCAS(a.owner + ids.w, MAT_NO_OWNER, i) == MAT_NO_OWNER;
  }
  const unsigned long long ms = __ballot(sel), mo = __ballot(own);
  uint32_t base = 0;
  if(lane == 0u) {
    if(ms != 0ull) atomicAdd(a.counters + MAT_CNT_SELECTED, uint32_t(__popcll(ms)));
    if(mo != 0ull) base = atomicAdd(a.counters + MAT_CNT_OWNERS, uint32_t(__popcll(mo)));
  }
  base = __shfl(base, 0);
  if(own) a.owners[base + uint32_t(__popcll(mo & ((1ull << lane) - 1ull)))] = i;   // (at most one owner per alphaIdx: base + rank < numAlpha)
}

__global__ __launch_bounds__(64) void k_mat_build(const MaterialArgs a, const uint32_t numOwners)
{
  __shared__ uint32_t words[4];
  const uint32_t o = blockIdx.x, lane = threadIdx.x;
  if(o >= numOwners) return;
  const uint32_t rec = gLoadU32(a.owners + o);
  if(rec >= a.numRecs) return;                                   // (wave-uniform, like every early return here)
  const uint4 ids = recordIds(a.tris + rec);
  const uint32_t idx = ids.w, m = materialOf(a, ids.y);
  if(idx >= a.numAlpha || m == 0xffffffffu) return;
  // ---- the alpha record: the host's alphaTemplate, from the device tables
  AlphaRec r = a.alphaRec[idx];
  const rt_material* mat = a.materials + m;
  r.baseAlpha = mat->pbrBaseColorFactor.w; r.cutoff = mat->alphaCutoff; r.alphaMode = mat->alphaMode;
  const int32_t tex = mat->pbrBaseColorTexture;
  r.bgra = nullptr; r.w = r.h = r.wrapS = r.wrapT = r.filter = 0;
  if(tex > -1 && uint32_t(tex) < a.numTextures) {
    const DevTexture t = a.textures[tex];
    r.bgra = t.bgra; r.w = t.w; r.h = t.h; r.wrapS = t.wrapS; r.wrapT = t.wrapT; r.filter = t.filter;
  }
  if(lane == 0u) a.alphaRec[idx] = r;
  const bool scan = r.bgra != nullptr && r.w > 0 && r.h > 0;
  // ---- the footprints: lane k < 36 holds cell k in the order of the host loop (j outer, i inner, i + j < 8)
  int ci = 0, cj = 0;
  { int rem = int(lane); while(cj < 8 && rem >= 8 - cj) { rem -= 8 - cj; cj++; } ci = rem; }
  OmmFootprint f{0, 0, 0, 0};
  int valid = 0;
  if(lane < 36u && scan) {
    const float uv[6] = {r.uv0x, r.uv0y, r.uv1x, r.uv1y, r.uv2x, r.uv2y};
    valid = ommCellFootprint(uv, r.w, r.h, ci, cj, f) ? 1 : 0;
  }
  if(lane < 4u) words[lane] = 0u;
  __syncthreads();
  uint32_t state = 0u, texelsLo = 0u, texelsHi = 0u;
  for(int c = 0; c < 36; c++) {
    int lo = 255, hi = 255;                                      // no texture: the texel's alpha is 1
    if(scan) {
      if(!__shfl(valid, c)) continue;                            // unknown: the cell keeps state 0
      const int x0 = __shfl(f.x0, c), y0 = __shfl(f.y0, c);
      const int nx = __shfl(f.x1, c) - x0 + 1, ny = __shfl(f.y1, c) - y0 + 1;
      const uint32_t total = uint32_t(nx) * uint32_t(ny);        // <= 65536 (ommCellFootprint)
      const int stepY = 64 / nx, stepX = 64 % nx;
      int x = int(lane) % nx, y = int(lane) / nx;
      lo = 255; hi = 0;                                          // the neutral elements of the min / max over the box
      for(uint32_t t = lane; t < total; t += 64u) {
        const size_t xx = size_t(ommWrapTexel(x0 + x, r.w, r.wrapS)), yy = size_t(ommWrapTexel(y0 + y, r.h, r.wrapT));
        const int al = int(gLoadU32(r.bgra + (yy * size_t(r.w) + xx) * 4u) >> 24);
        lo = al < lo ? al : lo; hi = al > hi ? al : hi;
        x += stepX; y += stepY;
        if(x >= nx) { x -= nx; y++; }
      }
      for(int off = 32; off > 0; off >>= 1) {
        const int l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
      }
      const uint32_t before = texelsLo;
      texelsLo += total; texelsHi += texelsLo < before ? 1u : 0u;
    }
    const uint32_t s = ommCellState(lo, hi, r.baseAlpha, r.cutoff, r.alphaMode);
    if(int(lane) == c) state = s;
  }
  if(lane < 36u && state != 0u) { const int cell = cj * 8 + ci; atomicOr(&words[cell >> 4], state << ((cell & 15) * 2)); }
  __syncthreads();
  if(lane == 0u) {
    gStoreU4(a.ommPlane + idx, make_uint4(words[0], words[1], words[2], words[3]));
    if(texelsLo | texelsHi) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + MAT_CNT_TEXELS_LO), ((unsigned long long)texelsHi << 32) | texelsLo);
  }
}

__global__ __launch_bounds__(MAT_BLOCK) void k_mat_scatter(const MaterialArgs a)
{
  const uint32_t i = blockIdx.x * MAT_BLOCK + threadIdx.x;
  if(i >= a.numRecs) return;
  uint4 ids;
  if(!selected(a, i, ids)) return;
  const uint4 omm = gLoadU4(a.ommPlane + ids.w);
  gStoreU4(reinterpret_cast<uint4*>(a.tris + i) + 3, omm);
  if(a.table) gStoreU4(reinterpret_cast<uint4*>(a.table + ids.y) + 3, omm);   // (ids.y < numGlobal: materialOf)
  const uint4* src = reinterpret_cast<const uint4*>(a.alphaRec + ids.w);
  uint4* dst = reinterpret_cast<uint4*>(a.alphaByTri + i);
  for(int q = 0; q < 4; q++) gStoreU4(dst + q, gLoadU4(src + q));
}

inline dim3 gridOf(uint32_t n) { return dim3((n + MAT_BLOCK - 1) / MAT_BLOCK); }

}  // namespace

hipError_t launchMaterialSelect(hipStream_t stream, const MaterialArgs& a)
{
  if(a.numRecs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mat_select, gridOf(a.numRecs), dim3(MAT_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launchMaterialBuild(hipStream_t stream, const MaterialArgs& a, uint32_t numOwners)
{
  if(numOwners == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mat_build, dim3(numOwners), dim3(64), 0, stream, a, numOwners);
  return hipGetLastError();
}

hipError_t launchMaterialScatter(hipStream_t stream, const MaterialArgs& a)
{
  if(a.numRecs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mat_scatter, gridOf(a.numRecs), dim3(MAT_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rt

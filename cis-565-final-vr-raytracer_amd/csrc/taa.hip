// taa.hip — temporal anti-aliasing resolve (rt_set_taa; include/rt_abi.h).
//
// The last stage of the display path, between compose and rt_tonemap.  The context renders frame f with a camera whose projection is shifted by a
// sub-pixel offset (rt_taa_jitter_camera); this pass accumulates the jittered frames into a history per component (direct, indirect), so that a pixel
// converges to the box-filtered image instead of the point sample at its centre.  Per full-resolution pixel p:
//
//   no valid material   D, I pass through unchanged, n = 1.
//   reprojection        x = cameraPosDenoise(jittered camera, p, G-buffer distance); s = (ndc(lastProjView · x) · 0.5 + 0.5) · (W, H); q = floor(s).
//                       Consistent when q lies in the image and G(f-1) at q has the same material hash, dot(n, n_prev) > 0.9 and
//                       |lastPosition - x| < depth_prev · 1.05 (the direct stage's temporal test).
//   history sample      4 x 4 Catmull-Rom around s - 0.5, tap coordinates clamped to the image (j outer, i inner), per component.
//   clip                in YCoCg: mean mu and deviation sigma of the in-image 3 x 3 neighbourhood of this frame's image (j outer, i inner); the history
//                       sample is pulled along the segment towards mu onto the box mu ± clipGamma·sigma (t = max over channels of |d| / extent, d / t).
//   blend               n = consistent ? min(n_prev + 1, 1024) : 1; a = max(alpha, 1/n); out = mix(H_clipped, c, a), .w = 1.  An inconsistent pixel
//                       writes c itself (mix(·, c, 1)).
// Numerics (include/rt_detmath.h): IEEE divisions and square roots, no contraction — tests/taa_checker.cpp restates every expression on the CPU and the
// GPU tests compare word for word.  Launch shape: one wave64 per 8 x 8 tile, the XCD-striped tile order of the stages (tileOf).
#define RT_COUNT 0
#include "temporal_common.h"
#include "taa.h"

namespace rt {
namespace {

__global__ __launch_bounds__(64) void k_taa_resolve(TaaArgs A, rt_scene_camera cam, int tilesX, int tilesY)
{
  const TileCoord tile = tileOf(tilesX, tilesY);
  const int lane = int(threadIdx.x);
  const i2 p{tile.x * 8 + (lane & 7), tile.y * 8 + (lane >> 3)};
  if(!tile.valid || p.x >= A.W || p.y >= A.H) return;
  const size_t idx = size_t(p.y) * A.W + p.x;
  const float4 cd = A.curD[idx], ci = A.curI[idx];
  const uint4 g = A.thisG[idx];
  const uint32_t hash = g.w & 0xFF000000u;
  if(hash == RT_INVALID_MAT_ID) {
    A.outD[idx] = cd; A.outI[idx] = ci; A.outN[idx] = 1.0f;
    return;
  }
  bool consistent = false;
  f2 s = mk2(0.0f, 0.0f);
  int qx = 0, qy = 0;
  if(A.histValid) {
    const f3 x = cameraPosDenoise(cam, p, rt_u2f(g.x), i2{A.W, A.H});
    const f4 clip = mul(cam.lastProjView, mk4(x, 1.0f));
    const f3 ndc = xyz(clip) / clip.w;
    const f2 mv = mk2(ndc.x, ndc.y) * 0.5f + 0.5f;
    s = mv * mk2(float(A.W), float(A.H));
    const float fx = rt_floor(s.x), fy = rt_floor(s.y);
    if(fx >= 0.0f && fy >= 0.0f && fx < float(A.W) && fy < float(A.H)) {
      qx = int(fx); qy = int(fy);
      const uint4 pg = A.lastG[size_t(qy) * A.W + qx];
      const f3 norm = decompress_unit_vec(g.y), pnorm = decompress_unit_vec(pg.y);
      const float pdepth = rt_u2f(pg.x);
      const float reprojDepth = length(mk3(cam.lastPosition) - x);
      consistent = (pg.w & 0xFF000000u) == hash && dot(norm, pnorm) > 0.9f && reprojDepth < pdepth * 1.05f;
    }
  }
  if(!consistent) {
    A.outD[idx] = make_float4(cd.x, cd.y, cd.z, 1.0f); A.outI[idx] = make_float4(ci.x, ci.y, ci.z, 1.0f); A.outN[idx] = 1.0f;
    return;
  }
  const int n = min(int(A.prevN[size_t(qy) * A.W + qx]) + 1, TAA_MAX_HISTORY);
  const float a = rt_max(A.alpha, 1.0f / float(n));
  const float tx = s.x - 0.5f, ty = s.y - 0.5f;
  const float bxf = rt_floor(tx), byf = rt_floor(ty);
  float wx[4], wy[4];
  catmullRom(tx - bxf, wx);
  catmullRom(ty - byf, wy);
  const int bx = int(bxf), by = int(byf);
  for(int comp = 0; comp < 2; comp++) {
    const float4* cur = comp ? A.curI : A.curD;
    const float4 c = comp ? ci : cd;
    const f3 h = catmullRomSample(comp ? A.prevI : A.prevD, wx, wy, bx, by, A.W, A.H);
    const TaaComp box = neighbourhood(cur, p, A.W, A.H);
    const f3 hc = fromYCoCg(clipToBox(toYCoCg(h), box, A.clipGamma));
    const float4 o = make_float4(mixf(hc.x, c.x, a), mixf(hc.y, c.y, a), mixf(hc.z, c.z, a), 1.0f);
    (comp ? A.outI : A.outD)[idx] = o;
  }
  A.outN[idx] = float(n);
}

}  // namespace

hipError_t launchTaaResolve(hipStream_t stream, const TaaArgs& A, const rt_scene_camera& cam)
{
  const int tilesX = (A.W + 7) / 8, tilesY = (A.H + 7) / 8;
  if(tilesX <= 0 || tilesY <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_taa_resolve, dim3(tileGrid(tilesX, tilesY)), dim3(64), 0, stream, A, cam, tilesX, tilesY);
  return hipGetLastError();
}

}  // namespace rt

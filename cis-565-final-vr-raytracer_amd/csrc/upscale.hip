// upscale.hip — temporal upsampling resolve (rt_set_upscale; include/rt_abi.h "Temporal upsampling").
//
// The context renders frame f at the render size W x H with a camera whose projection is shifted by a sub-pixel offset delta (rt_upscale_jitter_camera), so that
// render pixel p is sampled at render-pixel position p + 0.5 + delta.  This pass, right after compose, accumulates the jittered frames into a history at the
// output size Wo x Ho per component (direct, indirect).  Per output pixel o:
//
//   sample geometry     rho = (float(W) / float(Wo), float(H) / float(Ho)); u = (o + 0.5) · rho; p = clamp(floor(u - delta), 0, (W - 1, H - 1));
//                       e = u - ((p + 0.5) + delta): from the nearest sample of this frame to the output pixel's centre, in render pixels.
//   no valid material   at p: D, I of p pass through unchanged, n = 1.
//   reprojection        TAA's, at the render size: x = cameraPosDenoise(jittered camera, p, G-buffer distance, (W, H)); sR = (ndc(lastProjView · x) · 0.5 + 0.5)
//                       · (W, H); q = floor(sR) must lie in the render image and G(f-1) at q pass the direct stage's temporal test (same material hash,
//                       dot(n, n_prev) > 0.9, |lastPosition - x| < depth_prev · 1.05).  History position sO = (sR + e) / rho; floor(sO) must lie in the output image.
//   inconsistent        or no valid history: out = (c.rgb, 1) with c = cur(p), n = 1 — nearest-sample upsampling.
//   history sample      n = min(n_prev(floor(sO)) + 1, 1024); 4 x 4 Catmull-Rom of the previous resolved image (Wo x Ho, taps clamped) around sO - 0.5.
//   clip                TAA's, in YCoCg, onto mu ± clipGamma·sigma of the in-image 3 x 3 render-size neighbourhood of p.
//   blend               kappa = max(0, 1 - |e.x| / rho.x) · max(0, 1 - |e.y| / rho.y): a sample on the output centre counts fully, one a whole output pixel
//                       away not at all; a = max(alpha · kappa, 1 / n); out = mix(H_clipped, c, a), .w = 1.
// Numerics (include/rt_detmath.h): IEEE divisions and square roots, no contraction — tests/upscale_checker.cpp restates every expression on the CPU and the
// GPU tests compare word for word.  Launch shape: one wave64 per 8 x 8 OUTPUT tile, the XCD-striped tile order of the stages (tileOf) over the output grid.
// Memory: plain global loads.  At ratio r about r² output pixels share one render pixel's G-buffer words, its two 3 x 3 boxes and (static camera) most of
// their 2 x 16 history taps; those repeats are cache hits within the wave (DESIGN.md §29 has the measured bytes).
#define RT_COUNT 0
#include "temporal_common.h"
#include "upscale.h"

namespace rt {
namespace {

__global__ __launch_bounds__(64) void k_upscale_resolve(UpscaleArgs A, rt_scene_camera cam, int tilesX, int tilesY)
{
  const TileCoord tile = tileOf(tilesX, tilesY);
  const int lane = int(threadIdx.x);
  const i2 o{tile.x * 8 + (lane & 7), tile.y * 8 + (lane >> 3)};
  if(!tile.valid || o.x >= A.Wo || o.y >= A.Ho) return;
  const size_t oidx = size_t(o.y) * A.Wo + o.x;
  // sample geometry
  const float rhoX = float(A.W) / float(A.Wo), rhoY = float(A.H) / float(A.Ho);
  const float ux = (float(o.x) + 0.5f) * rhoX, uy = (float(o.y) + 0.5f) * rhoY;
  const i2 p{int(rt_min(rt_max(rt_floor(ux - A.dx), 0.0f), float(A.W - 1))), int(rt_min(rt_max(rt_floor(uy - A.dy), 0.0f), float(A.H - 1)))};
  const float ex = ux - ((float(p.x) + 0.5f) + A.dx), ey = uy - ((float(p.y) + 0.5f) + A.dy);
  const size_t idx = size_t(p.y) * A.W + p.x;
  const float4 cd = A.curD[idx], ci = A.curI[idx];
  const uint4 g = A.thisG[idx];
  const uint32_t hash = g.w & 0xFF000000u;
  if(hash == RT_INVALID_MAT_ID) {
    A.outD[oidx] = cd; A.outI[oidx] = ci; A.outN[oidx] = 1.0f;
    return;
  }
  bool consistent = false;
  float sox = 0.0f, soy = 0.0f;
  int hx = 0, hy = 0;
  if(A.histValid) {
    const f3 x = cameraPosDenoise(cam, p, rt_u2f(g.x), i2{A.W, A.H});
    const f4 clip = mul(cam.lastProjView, mk4(x, 1.0f));
    const f3 ndc = xyz(clip) / clip.w;
    const f2 mv = mk2(ndc.x, ndc.y) * 0.5f + 0.5f;
    const f2 s = mv * mk2(float(A.W), float(A.H));
    const float fx = rt_floor(s.x), fy = rt_floor(s.y);
    if(fx >= 0.0f && fy >= 0.0f && fx < float(A.W) && fy < float(A.H)) {
      const int qx = int(fx), qy = int(fy);
      const uint4 pg = A.lastG[size_t(qy) * A.W + qx];
      const f3 norm = decompress_unit_vec(g.y), pnorm = decompress_unit_vec(pg.y);
      const float pdepth = rt_u2f(pg.x);
      const float reprojDepth = length(mk3(cam.lastPosition) - x);
      consistent = (pg.w & 0xFF000000u) == hash && dot(norm, pnorm) > 0.9f && reprojDepth < pdepth * 1.05f;
      // the history position of this output pixel, and the output pixel that holds it
      sox = (s.x + ex) / rhoX; soy = (s.y + ey) / rhoY;
      const float gx = rt_floor(sox), gy = rt_floor(soy);
      if(gx >= 0.0f && gy >= 0.0f && gx < float(A.Wo) && gy < float(A.Ho)) { hx = int(gx); hy = int(gy); }
      else consistent = false;
    }
  }
  if(!consistent) {
    A.outD[oidx] = make_float4(cd.x, cd.y, cd.z, 1.0f); A.outI[oidx] = make_float4(ci.x, ci.y, ci.z, 1.0f); A.outN[oidx] = 1.0f;
    return;
  }
  const int n = min(int(A.prevN[size_t(hy) * A.Wo + hx]) + 1, UPSCALE_MAX_HISTORY);
  const float kappa = rt_max(0.0f, 1.0f - rt_abs(ex) / rhoX) * rt_max(0.0f, 1.0f - rt_abs(ey) / rhoY);
  const float a = rt_max(A.alpha * kappa, 1.0f / float(n));
  const float tx = sox - 0.5f, ty = soy - 0.5f;
  const float bxf = rt_floor(tx), byf = rt_floor(ty);
  float wx[4], wy[4];
  catmullRom(tx - bxf, wx);
  catmullRom(ty - byf, wy);
  const int bx = int(bxf), by = int(byf);
  for(int comp = 0; comp < 2; comp++) {
    const float4* cur = comp ? A.curI : A.curD;
    const float4 c = comp ? ci : cd;
    const f3 h = catmullRomSample(comp ? A.prevI : A.prevD, wx, wy, bx, by, A.Wo, A.Ho);
    const TaaComp box = neighbourhood(cur, p, A.W, A.H);
    const f3 hc = fromYCoCg(clipToBox(toYCoCg(h), box, A.clipGamma));
    const float4 out = make_float4(mixf(hc.x, c.x, a), mixf(hc.y, c.y, a), mixf(hc.z, c.z, a), 1.0f);
    (comp ? A.outI : A.outD)[oidx] = out;
  }
  A.outN[oidx] = float(n);
}

}  // namespace

hipError_t launchUpscaleResolve(hipStream_t stream, const UpscaleArgs& A, const rt_scene_camera& cam)
{
  const int tilesX = (A.Wo + 7) / 8, tilesY = (A.Ho + 7) / 8;
  if(tilesX <= 0 || tilesY <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_upscale_resolve, dim3(tileGrid(tilesX, tilesY)), dim3(64), 0, stream, A, cam, tilesX, tilesY);
  return hipGetLastError();
}

}  // namespace rt

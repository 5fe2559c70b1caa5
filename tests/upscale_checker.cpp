// upscale_checker.cpp — CPU restatement of the temporal upsampling resolve (rt_set_upscale, csrc/upscale.hip; include/rt_abi.h "Temporal upsampling") for the tests.
// TEST INFRASTRUCTURE: built by tests/upscale.py together with oracle/orc_scene.cpp, with the oracle's flags.  Scalar code over include/rt_detmath.h (IEEE sqrt
// and divisions, no contraction) and the oracle's decoders; every expression and every summation order is the kernel's — the GPU tests compare the resolved
// images and the history length word for word.  The history bookkeeping (parity, validity) lives in tests/upscale.py; this file is one frame's pass.
#include "../oracle/orc_shading.h"
#include <algorithm>

namespace {
using namespace orc;

vec3 cameraPos(const rt_scene_camera& cam, ivec2 coord, float dist, ivec2 imageSize)   // denoise_common.glsl:27-40
{
  const vec2 pixelCenter = V2(float(coord.x), float(coord.y)) + 0.5f;
  const vec2 inUV = pixelCenter / V2(float(imageSize.x), float(imageSize.y));
  const vec2 d = inUV * 2.0f - 1.0f;
  const vec4 origin = mul(Shader::M(cam.viewInverse), V4(0, 0, 0, 1));
  const vec4 target = mul(Shader::M(cam.projInverse), V4(d.x, d.y, 1, 1));
  const vec4 direction = mul(Shader::M(cam.viewInverse), V4(normalize(xyz(target)), 0));
  return xyz(origin) + xyz(direction) * dist;
}
vec3 toYCoCg(vec3 c) { return V3((0.25f * c.x + 0.5f * c.y) + 0.25f * c.z, 0.5f * c.x - 0.5f * c.z, (-0.25f * c.x + 0.5f * c.y) - 0.25f * c.z); }
vec3 fromYCoCg(vec3 v)
{
  const float t = v.x - v.z;
  return V3(t + v.y, v.x + v.z, t - v.y);
}
void catmullRom(float fr, float w[4])
{
  w[0] = fr * (-0.5f + fr * (1.0f - 0.5f * fr));
  w[1] = 1.0f + (fr * fr) * (-2.5f + 1.5f * fr);
  w[2] = fr * (0.5f + fr * (2.0f - 1.5f * fr));
  w[3] = (fr * fr) * (-0.5f + 0.5f * fr);
}
void neighbourhood(const float* img, int px, int py, int W, int H, vec3& mu, vec3& sigma)
{
  vec3 s1 = V3(0.0f), s2 = V3(0.0f);
  int cnt = 0;
  for(int j = -1; j <= 1; j++)
    for(int i = -1; i <= 1; i++) {
      const int qx = px + i, qy = py + j;
      if(qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      const float* c = img + (size_t(qy) * W + qx) * 4;
      const vec3 v = toYCoCg(V3(c[0], c[1], c[2]));
      s1 += v;
      s2 += v * v;
      cnt++;
    }
  const float nf = float(cnt);
  mu = s1 / nf;
  const vec3 var = s2 / nf - mu * mu;
  sigma = V3(rt_sqrt(var.x > 0.0f ? var.x : 0.0f), rt_sqrt(var.y > 0.0f ? var.y : 0.0f), rt_sqrt(var.z > 0.0f ? var.z : 0.0f));
}
vec3 clipToBox(vec3 h, vec3 mu, vec3 sigma, float gamma)
{
  const vec3 d = h - mu;
  const vec3 e = sigma * gamma;
  float t = 1.0f;
  const float ad[3] = {rt_abs(d.x), rt_abs(d.y), rt_abs(d.z)}, ex[3] = {e.x, e.y, e.z};
  for(int k = 0; k < 3; k++)
    if(ad[k] > ex[k]) t = rt_max(t, ad[k] / ex[k]);
  if(t > 1.0f) return V3(mu.x + d.x / t, mu.y + d.y / t, mu.z + d.z / t);
  return h;
}
int clampTap(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
vec3 catmullRomSample(const float* img, const float* wx, const float* wy, int bx, int by, int W, int H)
{
  vec3 acc = V3(0.0f);
  for(int j = 0; j < 4; j++) {
    const int y = clampTap(by - 1 + j, H);
    for(int i = 0; i < 4; i++) {
      const int x = clampTap(bx - 1 + i, W);
      const float w = wx[i] * wy[j];
      const float* c = img + (size_t(y) * W + x) * 4;
      acc = acc + V3(c[0], c[1], c[2]) * w;
    }
  }
  return acc;
}
}  // namespace

extern "C" {
// One frame's resolve.  Buffers in the boundary layouts: G-buffers 4 x u32 / px and the frame's images RGBA32F at the render size W x H; the history (RGBA32F, n
// f32) at the output size Wo x Ho.  `cam` is the jittered camera, (dx, dy) its offset in render pixels (rt_upscale_jitter_camera).
// Optional outputs per output pixel: consistentOut (bytes, 1 where the history was used), kappaOut (f32, the confidence of this frame's sample; 0 elsewhere).
int upscale_resolve(int W, int H, int Wo, int Ho, const rt_scene_camera* cam, float dx, float dy, float alpha, float clipGamma, int histValid, const uint32_t* thisG,
                    const uint32_t* lastG, const float* curD, const float* curI, const float* prevD, const float* prevI, const float* prevN, float* outD, float* outI,
                    float* outN, uint8_t* consistentOut, float* kappaOut)
{
  const float rhoX = float(W) / float(Wo), rhoY = float(H) / float(Ho);
  for(int oy = 0; oy < Ho; oy++)
    for(int ox = 0; ox < Wo; ox++) {
      const size_t oidx = size_t(oy) * Wo + ox;
      const float ux = (float(ox) + 0.5f) * rhoX, uy = (float(oy) + 0.5f) * rhoY;
      const int px = int(rt_min(rt_max(rt_floor(ux - dx), 0.0f), float(W - 1))), py = int(rt_min(rt_max(rt_floor(uy - dy), 0.0f), float(H - 1)));
      const float ex = ux - ((float(px) + 0.5f) + dx), ey = uy - ((float(py) + 0.5f) + dy);
      const size_t idx = size_t(py) * W + px;
      const float* cd = curD + idx * 4; const float* ci = curI + idx * 4;
      const uint32_t* g = thisG + idx * 4;
      const uint32_t hash = g[3] & 0xFF000000u;
      if(consistentOut) consistentOut[oidx] = 0;
      if(kappaOut) kappaOut[oidx] = 0.0f;
      if(hash == RT_INVALID_MAT_ID) {
        for(int k = 0; k < 4; k++) { outD[oidx * 4 + k] = cd[k]; outI[oidx * 4 + k] = ci[k]; }
        outN[oidx] = 1.0f;
        continue;
      }
      bool consistent = false;
      float sox = 0.0f, soy = 0.0f;
      int hx = 0, hy = 0;
      if(histValid) {
        const vec3 x = cameraPos(*cam, ivec2{px, py}, rt_u2f(g[0]), ivec2{W, H});
        const vec4 clip = mul(Shader::M(cam->lastProjView), V4(x, 1.0f));
        const vec3 ndc = xyz(clip) / clip.w;
        const vec2 mv = V2(ndc.x, ndc.y) * 0.5f + 0.5f;
        const vec2 s = mv * V2(float(W), float(H));
        const float fx = rt_floor(s.x), fy = rt_floor(s.y);
        if(fx >= 0.0f && fy >= 0.0f && fx < float(W) && fy < float(H)) {
          const int qx = int(fx), qy = int(fy);
          const uint32_t* pg = lastG + (size_t(qy) * W + qx) * 4;
          const vec3 norm = decompress_unit_vec(g[1]), pnorm = decompress_unit_vec(pg[1]);
          const float pdepth = rt_u2f(pg[0]);
          const float reprojDepth = length(V3(cam->lastPosition.x, cam->lastPosition.y, cam->lastPosition.z) - x);
          consistent = (pg[3] & 0xFF000000u) == hash && dot(norm, pnorm) > 0.9f && reprojDepth < pdepth * 1.05f;
          sox = (s.x + ex) / rhoX; soy = (s.y + ey) / rhoY;
          const float gx = rt_floor(sox), gy = rt_floor(soy);
          if(gx >= 0.0f && gy >= 0.0f && gx < float(Wo) && gy < float(Ho)) { hx = int(gx); hy = int(gy); }
          else consistent = false;
        }
      }
      if(!consistent) {
        for(int k = 0; k < 3; k++) { outD[oidx * 4 + k] = cd[k]; outI[oidx * 4 + k] = ci[k]; }
        outD[oidx * 4 + 3] = 1.0f; outI[oidx * 4 + 3] = 1.0f; outN[oidx] = 1.0f;
        continue;
      }
      if(consistentOut) consistentOut[oidx] = 1;
      const int n = std::min(int(prevN[size_t(hy) * Wo + hx]) + 1, 1024);
      const float kappa = rt_max(0.0f, 1.0f - rt_abs(ex) / rhoX) * rt_max(0.0f, 1.0f - rt_abs(ey) / rhoY);
      if(kappaOut) kappaOut[oidx] = kappa;
      const float a = rt_max(alpha * kappa, 1.0f / float(n));
      const float tx = sox - 0.5f, ty = soy - 0.5f;
      const float bxf = rt_floor(tx), byf = rt_floor(ty);
      float wx[4], wy[4];
      catmullRom(tx - bxf, wx);
      catmullRom(ty - byf, wy);
      const int bx = int(bxf), by = int(byf);
      for(int comp = 0; comp < 2; comp++) {
        const float* cur = comp ? curI : curD;
        const float* c = comp ? ci : cd;
        const vec3 h = catmullRomSample(comp ? prevI : prevD, wx, wy, bx, by, Wo, Ho);
        vec3 mu, sigma;
        neighbourhood(cur, px, py, W, H, mu, sigma);
        const vec3 hc = fromYCoCg(clipToBox(toYCoCg(h), mu, sigma, clipGamma));
        float* o = (comp ? outI : outD) + oidx * 4;
        o[0] = mix(hc.x, c[0], a); o[1] = mix(hc.y, c[1], a); o[2] = mix(hc.z, c[2], a); o[3] = 1.0f;
      }
      outN[oidx] = float(n);
    }
  return 0;
}
}

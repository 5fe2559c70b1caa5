// temporal_common.h — what the two temporal resolves (taa.hip, upscale.hip) share bit for bit: the YCoCg transform, the Catmull-Rom weights and 4 x 4 history
// sample with clamped taps, the 3 x 3 YCoCg neighbourhood statistics and the clip along the segment towards the mean (include/rt_abi.h "Temporal
// anti-aliasing" states every expression).  Internal linkage: each translation unit gets its own copies, as it did when taa.hip held them.
#pragma once
#include "filter_common.h"

namespace rt {
namespace {

RT_DEV f3 toYCoCg(f3 c)
{
  return mk3((0.25f * c.x + 0.5f * c.y) + 0.25f * c.z, 0.5f * c.x - 0.5f * c.z, (-0.25f * c.x + 0.5f * c.y) - 0.25f * c.z);
}
RT_DEV f3 fromYCoCg(f3 v)
{
  const float t = v.x - v.z;
  return mk3(t + v.y, v.x + v.z, t - v.y);
}
// Catmull-Rom weights of the four taps at offsets -1, 0, 1, 2 from floor(t), fr = t - floor(t)
RT_DEV void catmullRom(float fr, float w[4])
{
  w[0] = fr * (-0.5f + fr * (1.0f - 0.5f * fr));
  w[1] = 1.0f + (fr * fr) * (-2.5f + 1.5f * fr);
  w[2] = fr * (0.5f + fr * (2.0f - 1.5f * fr));
  w[3] = (fr * fr) * (-0.5f + 0.5f * fr);
}

struct TaaComp {
  f3 mu, sigma;
};
RT_DEV TaaComp neighbourhood(const float4* img, i2 p, int W, int H)
{
  f3 s1 = mk3(0.0f), s2 = mk3(0.0f);
  int cnt = 0;
  for(int j = -1; j <= 1; j++)
    for(int i = -1; i <= 1; i++) {
      const int qx = p.x + i, qy = p.y + j;
      if(qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      const float4 c = img[size_t(qy) * W + qx];
      const f3 v = toYCoCg(mk3(c.x, c.y, c.z));
      s1 += v;
      s2 += v * v;
      cnt++;
    }
  TaaComp r;
  const float nf = float(cnt);
  r.mu = s1 / nf;
  const f3 var = s2 / nf - r.mu * r.mu;
  r.sigma = mk3(rt_sqrt(var.x > 0.0f ? var.x : 0.0f), rt_sqrt(var.y > 0.0f ? var.y : 0.0f), rt_sqrt(var.z > 0.0f ? var.z : 0.0f));
  return r;
}
RT_DEV f3 clipToBox(f3 h, const TaaComp& b, float gamma)
{
  const f3 d = h - b.mu;
  const f3 e = b.sigma * gamma;
  float t = 1.0f;
  const float ad[3] = {rt_abs(d.x), rt_abs(d.y), rt_abs(d.z)}, ex[3] = {e.x, e.y, e.z};
  for(int k = 0; k < 3; k++)
    if(ad[k] > ex[k]) t = rt_max(t, ad[k] / ex[k]);
  if(t > 1.0f) return mk3(b.mu.x + d.x / t, b.mu.y + d.y / t, b.mu.z + d.z / t);
  return h;
}
RT_DEV int clampTap(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
RT_DEV f3 catmullRomSample(const float4* img, const float* wx, const float* wy, int bx, int by, int W, int H)
{
  f3 acc = mk3(0.0f);
  for(int j = 0; j < 4; j++) {
    const int y = clampTap(by - 1 + j, H);
    for(int i = 0; i < 4; i++) {
      const int x = clampTap(bx - 1 + i, W);
      const float w = wx[i] * wy[j];
      const float4 c = img[size_t(y) * W + x];
      acc = acc + mk3(c.x, c.y, c.z) * w;
    }
  }
  return acc;
}

}  // namespace
}  // namespace rt

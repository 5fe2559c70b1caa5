// svgf_checker.cpp — CPU restatement of the SVGF denoiser (rt_set_denoiser RT_DENOISER_SVGF, csrc/svgf.hip) for the tests.
// TEST INFRASTRUCTURE: built by tests/svgf.py together with oracle/orc_scene.cpp, with the oracle's flags.  Scalar code over include/rt_detmath.h
// (rt_exp, IEEE sqrt and divisions, no contraction) and the oracle's decoders; every expression and every summation order is the kernels' — the GPU
// tests compare the result images and the history word for word.  The frame's noisy inputs (G-buffers, motion, the demodulated LDR colour) come from
// the oracle's DIRECT / INDIRECT stages; the filtered images go back into the oracle for its COMPOSE stage.
#include "../oracle/orc_shading.h"
#include <vector>

namespace {
using namespace orc;

const float kGauss[5][5] = {{.0030f, .0133f, .0219f, .0133f, .0030f},
                            {.0133f, .0596f, .0983f, .0596f, .0133f},
                            {.0219f, .0983f, .1621f, .0983f, .0219f},
                            {.0133f, .0596f, .0983f, .0596f, .0133f},
                            {.0030f, .0133f, .0219f, .0133f, .0030f}};

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
float mixf(float x, float y, float t) { return x * (1.0f - t) + y * t; }
float normW(vec3 n, vec3 nq, float sigN) { return rt_min(1.0f, rt_exp(-(dot(n - nq, n - nq) / sigN))); }
float depthW(vec3 p, vec3 pq, float sigD) { return rt_exp(-(dot(p - pq, p - pq) / sigD)) + 1e-2f; }

struct Comp {   // one component's history
  int bx = 0, by = 0;
  std::vector<float> C, M;       // (colour, n) x4, (m1, m2) x2 per pixel
};

struct Checker {
  int W = 0, H = 0;
  rt_denoiser den{RT_DENOISER_SVGF, 0.2f, 0.2f, 32, 4.0f, 4.0f, {0, 0}};
  Comp comp[2];
  bool valid = false; int parity = -1;

  // one component (ind = half resolution): noisy (row pitch W) -> out (row pitch W); history in / out
  void chain(const rt_state& st, const rt_scene_camera& cam, bool ind, bool histOk, const uint32_t* thisG, const uint32_t* lastG, const int16_t* motion,
             const float* noisy, float* out)
  {
    Comp& K = comp[ind ? 1 : 0];
    const int bx = ind ? W / 2 : W, by = ind ? H / 2 : H;
    const size_t np = size_t(bx) * by;
    std::vector<float> prevC = K.C, prevM = K.M;
    if(K.bx != bx || K.by != by) { prevC.assign(np * 4, 0.f); prevM.assign(np * 2, 0.f); }
    K.bx = bx; K.by = by; K.C.assign(np * 4, 0.f); K.M.assign(np * 2, 0.f);
    std::vector<vec3> gN(np), gP(np);
    std::vector<uint32_t> gH(np);
    const float sigN = ind ? st.sigNormalIndirect : st.sigNormalDirect, sigD = ind ? st.sigDepthIndirect : st.sigDepthDirect;
    const float phi = ind ? den.phiLumIndirect : den.phiLumDirect;
    // (a) temporal accumulation
    for(int y = 0; y < by; y++)
      for(int x = 0; x < bx; x++) {
        const size_t i = size_t(y) * bx + x;
        const ivec2 gc = ind ? ivec2{2 * x, 2 * y} : ivec2{x, y};
        const uint32_t* g = thisG + (size_t(gc.y) * W + gc.x) * 4;
        gN[i] = decompress_unit_vec(g[1]);
        gP[i] = cameraPos(cam, gc, rt_u2f(g[0]), ivec2{bx, by});
        gH[i] = g[3] & 0xFF000000u;
        if(gH[i] == RT_INVALID_MAT_ID) continue;   // history cleared (zeros)
        const float* cin = noisy + (size_t(y) * W + x) * 4;
        const vec3 c = V3(cin[0], cin[1], cin[2]);
        float cp[4] = {0, 0, 0, 0}, mp[2] = {0, 0};
        int n = 1;
        if(histOk) {
          const int16_t* mv = motion + (size_t(gc.y) * W + gc.x) * 2;
          const ivec2 q = ind ? ivec2{int(mv[0]) >> 1, int(mv[1]) >> 1} : ivec2{int(mv[0]), int(mv[1])};
          if(q.x >= 0 && q.y >= 0 && q.x < bx && q.y < by) {
            const ivec2 gq = ind ? ivec2{2 * q.x, 2 * q.y} : q;
            const uint32_t* pg = lastG + (size_t(gq.y) * W + gq.x) * 4;
            const vec3 pnorm = decompress_unit_vec(pg[1]);
            const float pdepth = rt_u2f(pg[0]);
            const vec3 lp = V3(cam.lastPosition.x, cam.lastPosition.y, cam.lastPosition.z);
            const float reproj = length(lp - gP[i]);
            if((pg[3] & 0xFF000000u) == gH[i] && dot(gN[i], pnorm) > 0.9f && reproj < pdepth * 1.05f) {
              const size_t qi = size_t(q.y) * bx + q.x;
              for(int k = 0; k < 4; k++) cp[k] = prevC[qi * 4 + k];
              mp[0] = prevM[qi * 2]; mp[1] = prevM[qi * 2 + 1];
              n = std::min(int(cp[3]) + 1, den.historyCap);
            }
          }
        }
        const float inv = 1.0f / float(n);
        const float a = rt_max(den.alphaColor, inv), am = rt_max(den.alphaMoments, inv);
        const float l = luminance(c);
        K.C[i * 4 + 0] = mixf(cp[0], c.x, a); K.C[i * 4 + 1] = mixf(cp[1], c.y, a); K.C[i * 4 + 2] = mixf(cp[2], c.z, a); K.C[i * 4 + 3] = float(n);
        K.M[i * 2 + 0] = mixf(mp[0], l, am); K.M[i * 2 + 1] = mixf(mp[1], l * l, am);
      }
    // (b) variance -> level input (colour, var)
    std::vector<float> cur(np * 4, 0.f), nxt(np * 4, 0.f);
    for(int y = 0; y < by; y++)
      for(int x = 0; x < bx; x++) {
        const size_t i = size_t(y) * bx + x;
        if(gH[i] == RT_INVALID_MAT_ID) continue;
        float m1, m2;
        if(K.C[i * 4 + 3] >= 4.0f) { m1 = K.M[i * 2]; m2 = K.M[i * 2 + 1]; }
        else {
          float s1 = 0.f, s2 = 0.f, sw = 0.f;
          for(int j = -3; j <= 3; j++)
            for(int ii = -3; ii <= 3; ii++) {
              const int qx = x + ii, qy = y + j;
              if(qx < 0 || qy < 0 || qx >= bx || qy >= by) continue;
              const size_t qi = size_t(qy) * bx + qx;
              if(gH[qi] != gH[i]) continue;
              const float w = normW(gN[i], gN[qi], sigN) * depthW(gP[i], gP[qi], sigD);
              s1 += w * K.M[qi * 2]; s2 += w * K.M[qi * 2 + 1]; sw += w;
            }
          m1 = s1 / sw; m2 = s2 / sw;
        }
        const float v = m2 - m1 * m1;
        for(int k = 0; k < 3; k++) cur[i * 4 + k] = K.C[i * 4 + k];
        cur[i * 4 + 3] = (v > 0.0f) ? v : 0.0f;
      }
    // (c) the levels
    const int levels = ind ? 5 : 4;
    for(int level = 0; level < levels; level++) {
      const int step = 1 << level;
      for(int y = 0; y < by; y++)
        for(int x = 0; x < bx; x++) {
          const size_t i = size_t(y) * bx + x;
          vec3 res = V3(0.0f);
          float var = 0.0f;
          if(gH[i] != RT_INVALID_MAT_ID) {
            const float lp = luminance(V3(cur[i * 4], cur[i * 4 + 1], cur[i * 4 + 2]));
            float gv = 0.0f;
            for(int j = -1; j <= 1; j++)
              for(int ii = -1; ii <= 1; ii++) {
                const int qx = x + ii, qy = y + j;
                if(qx < 0 || qy < 0 || qx >= bx || qy >= by) continue;
                const float k = (ii == 0 && j == 0) ? 0.25f : ((ii == 0 || j == 0) ? 0.125f : 0.0625f);
                gv += k * cur[(size_t(qy) * bx + qx) * 4 + 3];
              }
            const float denom = phi * rt_sqrt(gv) + 1e-10f;
            vec3 sum = V3(0.0f);
            float sumV = 0.0f, sumW = 0.0f;
            for(int j = -2; j <= 2; j++)
              for(int ii = -2; ii <= 2; ii++) {
                const int qx = x + ii * step, qy = y + j * step;
                if(qx < 0 || qy < 0 || qx >= bx || qy >= by) continue;
                const size_t qi = size_t(qy) * bx + qx;
                if(gH[qi] != gH[i]) continue;
                const vec3 cq = V3(cur[qi * 4], cur[qi * 4 + 1], cur[qi * 4 + 2]);
                const float wL = rt_exp(-(rt_abs(lp - luminance(cq)) / denom));
                const float w = ((wL * normW(gN[i], gN[qi], sigN)) * depthW(gP[i], gP[qi], sigD)) * kGauss[ii + 2][j + 2];
                sum += cq * w;
                sumV += (w * w) * cur[qi * 4 + 3];
                sumW += w;
              }
            if(sumW < 1e-5f) { res = V3(0.0f); var = 0.0f; }
            else { res = sum / sumW; var = sumV / (sumW * sumW); }
            if(hasNan(res) || res.x < 0 || res.y < 0 || res.z < 0 || res.x > 1e8f || res.y > 1e8f || res.z > 1e8f) { res = V3(0.0f); var = 0.0f; }
            if(!(var >= 0.0f)) var = 0.0f;
          }
          if(level == 0) { K.C[i * 4] = res.x; K.C[i * 4 + 1] = res.y; K.C[i * 4 + 2] = res.z; }
          if(level == levels - 1) {
            res = LDRToHDR(res);
            float* o = out + (size_t(y) * W + x) * 4;
            o[0] = res.x; o[1] = res.y; o[2] = res.z; o[3] = 1.0f;
          } else {
            nxt[i * 4] = res.x; nxt[i * 4 + 1] = res.y; nxt[i * 4 + 2] = res.z; nxt[i * 4 + 3] = var;
          }
        }
      cur.swap(nxt);
    }
  }
};
}  // namespace

extern "C" {
void* svgf_create(int W, int H)
{
  Checker* k = new Checker;
  k->W = W; k->H = H;
  return k;
}
void svgf_destroy(void* h) { delete static_cast<Checker*>(h); }
void svgf_set(void* h, const rt_denoiser* d) { Checker* k = static_cast<Checker*>(h); k->den = *d; k->valid = false; }
void svgf_reset(void* h) { static_cast<Checker*>(h)->valid = false; }
// One frame's filters (denoise > 0) or the history invalidation of a denoise == 0 frame.  Buffers in the boundary layouts: G-buffers 4 x u32 / px,
// motion 2 x i16 / px, noisy direct = RT_BUF_DIRECT_RESULT, noisy indirect = RT_BUF_DENOISE_IND_A (row pitch W); outputs likewise (W x H x 4 floats).
int svgf_frame(void* h, const rt_state* st, const rt_scene_camera* cam, int frames, const uint32_t* thisG, const uint32_t* lastG, const int16_t* motion,
               const float* noisyDir, const float* noisyInd, float* outDir, float* outInd)
{
  Checker* k = static_cast<Checker*>(h);
  if(st->size.x != k->W || st->size.y != k->H) return -1;
  if(st->denoise == 0) { k->valid = false; return 0; }
  const bool histOk = k->valid && k->parity == ((frames + 1) & 1);
  k->chain(*st, *cam, false, histOk, thisG, lastG, motion, noisyDir, outDir);
  k->chain(*st, *cam, true, histOk, thisG, lastG, motion, noisyInd, outInd);
  k->valid = true; k->parity = frames & 1;
  return 0;
}
// the history of the last frame: which = 0 direct colour + n, 1 indirect colour + n, 2 direct moments, 3 indirect moments (compact, like rt_denoiser_readback)
int svgf_history(void* h, int which, float* dst)
{
  Checker* k = static_cast<Checker*>(h);
  const Comp& K = k->comp[which & 1];
  const std::vector<float>& v = which < 2 ? K.C : K.M;
  std::copy(v.begin(), v.end(), dst);
  return 0;
}
}

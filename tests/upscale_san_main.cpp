// upscale_san_main.cpp — TEST INFRASTRUCTURE: a program of its own that drives tests/upscale_checker.cpp (with oracle/orc_scene.cpp) over hand-made frames,
// built by tests/test_upscale_cpu.py with -fsanitize=address,undefined and run once on the CPU.  Exit status 0 and "ok" on stdout when nothing was reported.
// Every buffer is a std::vector of exactly the size the contract names, so a tap, a neighbourhood or a history index outside its image is reported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../include/rt_abi.h"

extern "C" int upscale_resolve(int W, int H, int Wo, int Ho, const rt_scene_camera* cam, float dx, float dy, float alpha, float clipGamma, int histValid,
                               const uint32_t* thisG, const uint32_t* lastG, const float* curD, const float* curI, const float* prevD, const float* prevI,
                               const float* prevN, float* outD, float* outI, float* outN, uint8_t* consistentOut, float* kappaOut);

static void identity(rt_mat4& m) { std::memset(&m, 0, sizeof(m)); m.m[0] = m.m[5] = m.m[10] = m.m[15] = 1.0f; }

// A camera at the origin looking down -z through a 90 degree frustum; `shift` moves last frame's projection sideways (in NDC), `scale` zooms it, so that the
// reprojection lands in the image, on its borders and far outside; `poison` writes a NaN into lastProjView.
static rt_scene_camera camera(float shift, float scale, bool poison)
{
  rt_scene_camera c;
  std::memset(&c, 0, sizeof(c));
  identity(c.viewInverse); identity(c.projInverse); identity(c.projView); identity(c.lastView); identity(c.lastProjView);
  c.projInverse.m[10] = 0.0f; c.projInverse.m[14] = -1.0f;          // target = (x, y, -1): a ray through the image plane at z = -1
  // lastProjView: clip = (scale x + shift w, scale y, ., w = -z)
  c.lastProjView.m[0] = scale; c.lastProjView.m[5] = scale; c.lastProjView.m[8] = -shift; c.lastProjView.m[11] = -1.0f; c.lastProjView.m[15] = 0.0f;
  if(poison) c.lastProjView.m[12] = std::numeric_limits<float>::quiet_NaN();
  return c;
}

static int runSize(int W, int H, int Wo, int Ho)
{
  const size_t n = size_t(W) * H, no = size_t(Wo) * Ho;
  std::vector<uint32_t> g(n * 4), gl(n * 4);
  std::vector<float> cd(n * 4), ci(n * 4);
  for(size_t p = 0; p < n; p++) {
    const float depth = (p % 7 == 3) ? 1e30f : 1.0f + float(p % 5);
    std::memcpy(&g[4 * p], &depth, 4); std::memcpy(&gl[4 * p], &depth, 4);
    g[4 * p + 1] = gl[4 * p + 1] = 0u;
    g[4 * p + 3] = (p % 7 == 3) ? RT_INVALID_MAT_ID : 0x01000000u;
    gl[4 * p + 3] = (p % 11 == 5) ? 0x02000000u : 0x01000000u;
    for(int k = 0; k < 4; k++) { cd[4 * p + k] = 0.1f + float((p * 13 + k * 7) % 17); ci[4 * p + k] = 0.5f * cd[4 * p + k]; }
  }
  std::vector<float> D[2] = {std::vector<float>(no * 4, 0.25f), std::vector<float>(no * 4)}, I[2] = {std::vector<float>(no * 4, 0.5f), std::vector<float>(no * 4)};
  std::vector<float> N[2] = {std::vector<float>(no, 1023.0f), std::vector<float>(no)};
  std::vector<uint8_t> cons(no);
  std::vector<float> kappa(no);
  const float deltas[4][2] = {{0.0f, 0.0f}, {0.46875f, -0.4938272f}, {-0.49f, 0.49f}, {0.25f, -0.25f}};
  const float shifts[5] = {0.0f, 0.01f, 0.9f, -1.0f, 50.0f}, scales[3] = {1.0f, 0.5f, 3.0f};
  size_t accepted = 0;
  int f = 0;
  for(const auto& d : deltas)
    for(float shift : shifts)
      for(float scale : scales)
        for(int poison = 0; poison < 2; poison++)
          for(int hist = 0; hist < 2; hist++, f++) {
            const rt_scene_camera cam = camera(shift, scale, poison != 0);
            const int cur = f & 1, prev = cur ^ 1;
            if(upscale_resolve(W, H, Wo, Ho, &cam, d[0], d[1], 0.1f, 1.0f, hist, g.data(), gl.data(), cd.data(), ci.data(), D[prev].data(), I[prev].data(), N[prev].data(),
                               D[cur].data(), I[cur].data(), N[cur].data(), (f & 2) ? cons.data() : nullptr, (f & 2) ? kappa.data() : nullptr) != 0) return 1;
            for(size_t o = 0; o < no; o++) {
              if(!(N[cur][o] >= 1.0f && N[cur][o] <= 1024.0f)) return 2;
              if(!hist && N[cur][o] != 1.0f) return 3;
              if(poison && N[cur][o] != 1.0f) return 4;   // a NaN position is never consistent
              accepted += N[cur][o] > 1.0f;
            }
          }
  return accepted ? 0 : 5;   // (some configuration must have used the history, or the program exercised nothing)
}

int main()
{
  const int sizes[6][4] = {{24, 16, 48, 32}, {37, 27, 56, 41}, {16, 16, 16, 16}, {8, 8, 32, 32}, {1, 1, 3, 2}, {5, 3, 20, 4}};
  for(const auto& s : sizes) {
    const int rc = runSize(s[0], s[1], s[2], s[3]);
    if(rc) { printf("%d x %d -> %d x %d: step %d failed\n", s[0], s[1], s[2], s[3], rc); return 1; }
  }
  printf("ok\n");
  return 0;
}

// materials_san_main.cpp — TEST INFRASTRUCTURE: a program of its own over csrc/opacity_map.h (the micro-map rule the host and the device share), built by
// tests/test_materials_cpu.py with -fsanitize=address,undefined and run once on the CPU.  Every texture is exactly w x h x 4 bytes on the heap, so a texel read
// outside it is reported; conversions that cannot hold their value and signed overflow are reported by the undefined-behaviour checks.
// Exit status 0 and "ok" on stdout when nothing was reported and every expectation holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../cis-565-final-vr-raytracer_amd/csrc/opacity_map.h"

using namespace rt;

#define EXPECT(cond) do { if(!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } } while(0)

static std::vector<uint8_t> ramp(int w, int h)
{
  std::vector<uint8_t> t(size_t(w) * h * 4);
  for(int y = 0; y < h; y++)
    for(int x = 0; x < w; x++) {
      uint8_t* p = &t[(size_t(y) * w + x) * 4];
      p[0] = p[1] = p[2] = uint8_t(x * 7 + y);
      p[3] = x < w / 3 ? 0 : (x >= w - w / 3 ? 255 : uint8_t(40 + (x * 31 + y * 17) % 180));
    }
  return t;
}

static uint32_t stateOf(const uint32_t omm[4], int i, int j) { const int cell = j * 8 + i; return (omm[cell >> 4] >> ((cell & 15) * 2)) & 3u; }

// the map of one triangle; every cell of the lower-left half is 0..2, every other bit is clear
static bool build(const float uv[6], float base, float cutoff, int mode, int w, int h, int ws, int wt, const std::vector<uint8_t>* tex, uint32_t omm[4])
{
  ommBuildSerial(uv, base, cutoff, mode, w, h, ws, wt, tex ? tex->data() + 3 : nullptr, 4, omm);
  for(int j = 0; j < 8; j++)
    for(int i = 0; i < 8; i++) {
      const uint32_t s = stateOf(omm, i, j);
      if(i + j < 8 ? s > 2u : s != 0u) return false;
    }
  return true;
}

int main()
{
  const int wraps[3] = {RT_WRAP_REPEAT, RT_WRAP_CLAMP, RT_WRAP_MIRROR};
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  uint32_t omm[4];
  // ---- the wrap: every result inside [0, n), at the ends of int too
  for(int mode : wraps)
    for(int n : {1, 2, 19, 37, 64, 4096})
      for(int i : {-2147483647 - 1, -2147483647, -4097, -65, -1, 0, 1, 63, 64, 4095, 4096, 2147483647}) {
        const int r = ommWrapTexel(i, n, mode);
        EXPECT(r >= 0 && r < n);
      }
  // ---- the edge inputs: three texture sizes, all wrap pairs, both alpha modes, negative texcoords
  const std::vector<uint8_t> t1 = ramp(1, 1), t37 = ramp(37, 19), t64 = ramp(64, 64);
  const std::vector<uint8_t>* texs[3] = {&t1, &t37, &t64};
  const int sizes[3][2] = {{1, 1}, {37, 19}, {64, 64}};
  const float uvs[][6] = {{0.05f, 0.1f, 0.30f, 0.1f, 0.05f, 0.35f}, {0.70f, 0.2f, 0.95f, 0.2f, 0.70f, 0.45f}, {-1.95f, -0.9f, -1.70f, -0.9f, -1.95f, -0.65f},
                          {0.f, 0.f, 1.f, 0.f, 0.f, 1.f}, {3.70f, 7.2f, 3.95f, 7.2f, 3.70f, 7.45f}, {-5.f, 3.f, 9.f, 3.f, -5.f, 40.f}};
  unsigned seen[3] = {0, 0, 0};
  for(int t = 0; t < 3; t++)
    for(int ws : wraps)
      for(int wt : wraps)
        for(int mode : {RT_ALPHA_MASK, RT_ALPHA_BLEND})
          for(float base : {1.0f, 1.5f, 0.25f, 0.0f, -0.5f})
            for(const auto& uv : uvs) {
              EXPECT(build(uv, base, 0.5f, mode, sizes[t][0], sizes[t][1], ws, wt, texs[t], omm));
              for(int j = 0; j < 8; j++) for(int i = 0; i + j < 8; i++) seen[stateOf(omm, i, j)]++;
              if(base < 0.f) EXPECT((omm[0] | omm[1] | omm[2] | omm[3]) == 0u);
            }
  EXPECT(seen[0] > 0 && seen[1] > 0 && seen[2] > 0);
  // no texture: the base alpha alone decides, every cell alike
  { const float uv[6] = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f};
    EXPECT(build(uv, 0.8f, 0.5f, RT_ALPHA_MASK, 0, 0, 0, 0, nullptr, omm));
    for(int j = 0; j < 8; j++) for(int i = 0; i + j < 8; i++) EXPECT(stateOf(omm, i, j) == 1u);
    EXPECT(build(uv, 0.2f, 0.5f, RT_ALPHA_MASK, 0, 0, 0, 0, nullptr, omm));
    for(int j = 0; j < 8; j++) for(int i = 0; i + j < 8; i++) EXPECT(stateOf(omm, i, j) == 2u); }
  // ---- hostile texcoords: every cell unknown, nothing read
  const float hostile[][6] = {{nan, 0.1f, 0.3f, 0.1f, 0.05f, 0.5f}, {0.05f, 0.1f, inf, 0.1f, 0.05f, 0.5f}, {0.05f, -inf, 0.3f, 0.1f, 0.05f, 0.5f},
                              {3e38f, 3e38f, 3e38f, 3e38f, 3e38f, 3e38f}, {-3e38f, 0.f, 3e38f, 0.f, 0.f, 3e38f}, {1e20f, 1e20f, 1e20f, 1e20f, 1e20f, 1e20f},
                              {3.4e7f, 0.f, 3.4e7f, 0.f, 3.4e7f, 0.f},            // 64 x 3.4e7 = 2.2e9 texels: beyond int, span 0
                              {0.f, 0.f, 600.f, 0.f, 0.f, 1.f},                   // a span of 4800 texels per cell
                              {0.f, 0.f, 64.f, 0.f, 0.f, 96.f}};                  // 512 x 768 texels per cell on 64 x 64
  for(const auto& uv : hostile) {
    EXPECT(build(uv, 1.0f, 0.5f, RT_ALPHA_MASK, 64, 64, RT_WRAP_REPEAT, RT_WRAP_MIRROR, &t64, omm));
    EXPECT((omm[0] | omm[1] | omm[2] | omm[3]) == 0u);
  }
  // large but admitted coordinates just inside the bound: the box is scanned and wraps
  { const float c = 33554000.f;   // x 64 = 2147456000 < 2^31 - 4096
    const float uv[6] = {c, -c, c + 2.f, -c, c, -c + 2.f};
    EXPECT(build(uv, 1.0f, 0.5f, RT_ALPHA_MASK, 64, 64, RT_WRAP_MIRROR, RT_WRAP_REPEAT, &t64, omm)); }
  // ---- the scan limit: boxes of w * h texels just below, at and above 65536 (a 1 x 1 texture: every texel of the box is the one texel)
  { OmmFootprint f;
    const float in[6] = {0.f, 0.f, 8.f * 251.f, 0.f, 0.f, 8.f * 251.f};     // 251 + 4 = 255 per side: 65025 texels
    EXPECT(ommCellFootprint(in, 1, 1, 0, 0, f) && (f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) == 65025);
    const float at[6] = {0.f, 0.f, 8.f * 252.f, 0.f, 0.f, 8.f * 252.f};     // 256 per side: exactly 65536 texels, still scanned
    EXPECT(ommCellFootprint(at, 1, 1, 0, 0, f) && (f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) == 65536);
    const float over[6] = {0.f, 0.f, 8.f * 253.f, 0.f, 0.f, 8.f * 252.f};   // 257 x 256
    EXPECT(!ommCellFootprint(over, 1, 1, 0, 0, f));
    EXPECT(build(at, 1.0f, 0.5f, RT_ALPHA_MASK, 1, 1, RT_WRAP_CLAMP, RT_WRAP_REPEAT, &t1, omm));
    EXPECT(build(at, 1.0f, 0.5f, RT_ALPHA_MASK, 37, 19, RT_WRAP_MIRROR, RT_WRAP_REPEAT, &t37, omm));
    const float span[6] = {0.f, 0.f, 8.f * 4095.f, 0.f, 0.f, 1.f};          // 4095 texels wide: below the span limit, 4099 x 4 texels
    EXPECT(ommCellFootprint(span, 1, 1, 0, 0, f) && f.x1 - f.x0 + 1 == 4099);
    const float wide[6] = {0.f, 0.f, 8.f * 4096.f, 0.f, 0.f, 1.f};
    EXPECT(!ommCellFootprint(wide, 1, 1, 0, 0, f)); }
  // ---- the cell state at its margins
  EXPECT(ommCellState(255, 255, 1.0f, 0.5f, RT_ALPHA_MASK) == 1u && ommCellState(0, 0, 1.0f, 0.5f, RT_ALPHA_MASK) == 2u && ommCellState(0, 255, 1.0f, 0.5f, RT_ALPHA_MASK) == 0u);
  EXPECT(ommCellState(255, 255, 0.5f, 0.5f, RT_ALPHA_MASK) == 0u);                                  // inside the 1e-4 margin: unknown
  EXPECT(ommCellState(255, 255, 1.0f, 0.5f, RT_ALPHA_BLEND) == 0u && ommCellState(255, 255, 1.5f, 0.5f, RT_ALPHA_BLEND) == 1u);
  EXPECT(ommCellState(0, 0, 1.0f, 0.5f, RT_ALPHA_BLEND) == 2u && ommCellState(0, 1, 1.0f, 0.5f, RT_ALPHA_BLEND) == 0u);
  EXPECT(ommCellState(255, 255, nan, 0.5f, RT_ALPHA_MASK) == 0u && ommCellState(255, 255, 1.0f, nan, RT_ALPHA_MASK) == 0u);
  printf("ok states %u %u %u\n", seen[0], seen[1], seen[2]);
  return 0;
}

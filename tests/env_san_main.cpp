// env_san_main.cpp — TEST INFRASTRUCTURE: a program of its own over csrc/env_accel.h (the importance-table rule the host and the device share; rt_env_accel is
// envAccelHost) and tests/env_accel_checker.cpp, built by tests/test_environment_cpu.py with -fsanitize=address,undefined and run once on the CPU over the maps of
// tests/env.py.  Each argument is a file: int32 w, int32 h, then w h 4 floats.  Every array is exactly as long as the rule says on the heap, so a read or write
// outside it is reported; shifts, conversions and signed overflow are reported by the undefined-behaviour checks.  A map both sides refuse counts as agreement.
// Exit status 0 and "ok" on stdout when nothing was reported and both sides agree word for word on every map.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../cis-565-final-vr-raytracer_amd/csrc/env_accel.h"

extern "C" int evc_accel(int w, int h, const float* px, rt_impt_samp* out, float* integral, float* average, uint32_t* numSmall);

int main(int argc, char** argv)
{
  int maps = 0, refused = 0;
  for(int k = 1; k < argc; k++) {
    FILE* f = fopen(argv[k], "rb");
    int32_t wh[2];
    if(!f || fread(wh, 4, 2, f) != 2 || wh[0] < 1 || wh[1] < 1) { printf("%s: cannot read\n", argv[k]); return 1; }
    const size_t n = size_t(wh[0]) * size_t(wh[1]);
    std::vector<float> px(n * 4);
    if(fread(px.data(), 4, n * 4, f) != n * 4) { printf("%s: short file\n", argv[k]); return 1; }
    fclose(f);
    std::vector<rt_impt_samp> a(n), b(n);
    std::vector<float> imp(n);
    rt::EnvAccelResult r;
    float integral = 0.f, average = 0.f;
    uint32_t small = 0;
    const int ra = rt::envAccelHost(wh[0], wh[1], px.data(), a.data(), r, imp.data());
    const int rb = evc_accel(wh[0], wh[1], px.data(), b.data(), &integral, &average, &small);
    if(ra != rb) { printf("%s: refusal differs (%d, %d)\n", argv[k], ra, rb); return 1; }
    maps++;
    if(ra) { refused++; continue; }
    if(memcmp(a.data(), b.data(), n * sizeof(rt_impt_samp)) != 0 || memcmp(&integral, &r.integral, 4) != 0 || memcmp(&average, &r.average, 4) != 0 || small != r.numSmall ||
       r.numSmall + r.numLarge != n) {
      printf("%s: the rule and the checker differ\n", argv[k]);
      return 1;
    }
    for(size_t i = 0; i < n; i++)
      if(a[i].alias < 0 || size_t(a[i].alias) >= n || !(a[i].q >= 0.f && a[i].q <= 1.f)) { printf("%s: entry %zu out of range\n", argv[k], i); return 1; }
  }
  // the quantiser at its edges: the maximum lands in [2^39, 2^40), subnormals included; zero stays zero
  for(float M : {1.0f, 3.4e38f, 1.17549435e-38f, 1e-45f, 7e-42f, 12.566371f}) {
    const int e = rt::envScaleExp(M);
    const uint64_t W = rt::envQuantise(M, e);
    if(W < (uint64_t(1) << 39) || W >= (uint64_t(1) << 40) || rt::envQuantise(0.0f, e) != 0u || rt::envQuantise(1e-45f, e) > W) { printf("quantiser: M = %g\n", double(M)); return 1; }
  }
  // the grid division against the compiler's 128-bit one: T from 2^39 to just below 2^63, X from 0 to n T, at and around the multiples and half multiples of T
  { typedef unsigned __int128 u128;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for(int it = 0; it < 200000; it++) {
      const int tb = 40 + int(next() % 24);
      uint64_t T = (next() >> (64 - tb)) | (uint64_t(1) << (tb - 1));
      if(it % 7 == 0) T = (uint64_t(1) << 63) - 1 - (next() & 0xffu);
      const uint64_t n = 1 + next() % (uint64_t(1) << 23);
      u128 X = ((u128(next()) << 64) | next()) % (u128(n) * T + 1);
      if(it % 5 == 0) X = u128(next() % n) * T + ((next() & 1u) ? 0 : T / 2 + (next() & 3u)) ;
      if(it % 9 == 0) X = u128(n) * T - (next() & 0xffu) % (uint64_t(X) | 1u);
      rt::EnvU128 x; x.lo = uint64_t(X); x.hi = uint64_t(X >> 64);
      if(rt::envGrid(x, T) != uint64_t(((X << 24) + (T >> 1)) / T)) { printf("envGrid: case %d\n", it); return 1; }
    } }
  printf("ok maps %d refused %d\n", maps, refused);
  return 0;
}

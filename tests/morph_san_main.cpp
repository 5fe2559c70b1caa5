// morph_san_main.cpp — TEST INFRASTRUCTURE: a program of its own that drives tests/morph_checker.cpp, built by tests/test_morph_cpu.py with
// -fsanitize=address,undefined and run once on the CPU.  The arrays are exactly as long as the layout says, so a row read past a plane is reported.
// Exit status 0 and "ok" on stdout when nothing was reported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/rt_abi.h"

extern "C" uint32_t mpc_morph(const rt_vertex* rest, uint32_t count, const rt_morph_delta* deltas, uint32_t targetCount, uint32_t planes, const float* weights,
                              rt_vertex* out, uint32_t* active);
extern "C" uint32_t mpc_encode(float x, float y, float z);

int main()
{
  const uint32_t counts[4] = {0, 1, 63, 258};
  const uint32_t targets[3] = {1, 2, 9};
  for(uint32_t V : counts)
    for(uint32_t T : targets)
      for(uint32_t planes = 0; planes < 4; planes++) {
        const uint32_t P = 1 + (planes & 1) + (planes >> 1);
        std::vector<rt_vertex> rest(V), out(V);
        for(uint32_t v = 0; v < V; v++) {
          rest[v] = rt_vertex{};
          rest[v].position = rt_vec3{0.1f * float(v), 1.0f, -0.5f * float(v % 7)};
          rest[v].normal = v % 5 == 0 ? 0xffffffffu : mpc_encode(0.3f, float(v % 3) - 1.0f, 0.5f);
          rest[v].tangent = v % 6 == 1 ? 0xffffffffu : mpc_encode(1.0f, 0.1f * float(v % 4), 0.0f);
        }
        std::vector<rt_morph_delta> deltas(size_t(T) * P * V);
        for(size_t r = 0; r < deltas.size(); r++) deltas[r] = rt_morph_delta{{0.01f * float(r % 11), -0.02f * float(r % 5), 0.03f}, NAN};
        std::vector<float> w(T);
        for(uint32_t t = 0; t < T; t++) w[t] = t % 3 == 1 ? -0.0f : 0.5f - 0.4f * float(t);
        uint32_t active = 0;
        if(mpc_morph(rest.data(), V, deltas.data(), T, planes, w.data(), out.data(), &active) != 0) { printf("non-finite\n"); return 1; }
        uint32_t want = 0;
        for(float x : w) want += x != 0.0f ? 1u : 0u;
        if(active != want) { printf("active %u != %u\n", active, want); return 1; }
        // all weights zero: the rest rows, bit for bit
        std::fill(w.begin(), w.end(), 0.0f);
        if(mpc_morph(rest.data(), V, deltas.data(), T, planes, w.data(), out.data(), &active) != 0 || active != 0) return 1;
        if(V && memcmp(rest.data(), out.data(), size_t(V) * sizeof(rt_vertex)) != 0) { printf("zero weights changed a row\n"); return 1; }
        // an overflowing product is counted
        if(V) {
          w[0] = 3e38f;
          deltas[0].d[0] = 10.0f;
          if(mpc_morph(rest.data(), V, deltas.data(), T, planes, w.data(), out.data(), &active) == 0) { printf("overflow not counted\n"); return 1; }
        }
      }
  printf("ok\n");
  return 0;
}

// instances_san_main.cpp — TEST INFRASTRUCTURE: a program of its own that drives tests/instances_checker.cpp, built by tests/test_instances_cpu.py with
// -fsanitize=address,undefined and run once on the CPU.  The arrays are exactly as long as the layout says, so a word written past a table is reported.
// Exit status 0 and "ok" on stdout when nothing was reported and every verdict / expansion is the expected one.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/rt_abi.h"

extern "C" int isc_verdict(const rt_scene_desc* scene, const uint8_t* bound, uint32_t numInst, const rt_instance* inst, uint32_t* offender);
extern "C" uint32_t isc_expand(const rt_scene_desc* scene, uint32_t numInst, const rt_instance* inst, uint32_t* prefix, uint32_t* triRef, uint32_t* rec);
extern "C" int64_t isc_flatten(const rt_scene_desc* scene, int threads, uint32_t* triRef, uint32_t* flags);

static rt_instance instanceOf(uint32_t mesh, uint32_t flags, float x, float sx)
{
  rt_instance in{};
  in.objectToWorld[0] = sx; in.objectToWorld[5] = 1.f; in.objectToWorld[10] = 1.f; in.objectToWorld[3] = x;
  in.primMesh = mesh; in.flags = flags;
  return in;
}

#define EXPECT(cond) do { if(!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } } while(0)

int main()
{
  // three prim meshes over one vertex array: 5 triangles (plain), none, 2 triangles (emissive material)
  std::vector<rt_vertex> vertices(21);
  for(size_t v = 0; v < vertices.size(); v++) { vertices[v] = rt_vertex{}; vertices[v].position = rt_vec3{0.3f * float(v % 3), 0.2f * float(v / 3), 0.1f * float(v % 5)}; }
  std::vector<uint32_t> indices(21);
  for(uint32_t k = 0; k < 21; k++) indices[k] = k % 15;
  const rt_prim_mesh meshes[3] = {{0, 15, 0, 15, 0}, {0, 15, 15, 0, 0}, {15, 6, 15, 6, 1}};
  rt_material mats[2] = {};
  mats[1].emissiveFactor = rt_vec3{1.f, 1.f, 1.f};
  for(uint32_t k = 15; k < 21; k++) indices[k] = k - 15;
  std::vector<rt_instance> old = {instanceOf(2, 1, 0.f, 1.f), instanceOf(0, 1, 1.f, 1.f)};
  rt_trig_light lights[2] = {};
  rt_scene_desc d{};
  d.numPrimMeshes = 3; d.primMeshes = meshes;
  d.numVertices = vertices.size(); d.vertices = vertices.data();
  d.numIndices = indices.size(); d.indices = indices.data();
  d.numInstances = uint32_t(old.size()); d.instances = old.data();
  d.numMaterials = 2; d.materials = mats;
  d.trigLights = lights; d.lightInfo.trigLightSize = 2;
  uint32_t off = 0;
  // verdicts
  EXPECT(isc_verdict(&d, nullptr, 1, nullptr, &off) == 1);
  EXPECT(isc_verdict(&d, nullptr, 0, old.data(), &off) == 2);
  EXPECT(isc_verdict(&d, nullptr, 2, old.data(), &off) == 0);
  { std::vector<rt_instance> t = old; t[1].primMesh = 3; EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 3 && off == 1); }
  { std::vector<rt_instance> t = old; t[1].objectToWorld[7] = NAN; EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 4 && off == 1); }
  { std::vector<rt_instance> t = old; t[1].objectToWorld[5] = 0.f; EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 5 && off == 1); }
  { std::vector<rt_instance> t = old; t[1] = instanceOf(0, 1, 0.f, 1e-13f); t[1].objectToWorld[5] = t[1].objectToWorld[10] = 1e-13f; EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 6 && off == 1); }
  { std::vector<rt_instance> t = {old[0], instanceOf(1, 1, 0.f, 1.f)}; EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 0); }
  { std::vector<rt_instance> t = old; t[0].objectToWorld[3] = 0.5f; EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 9 && off == 0); }
  { std::vector<rt_instance> t = {old[1]}; EXPECT(isc_verdict(&d, nullptr, 1, t.data(), &off) == 9 && off == 0); }
  { std::vector<rt_instance> t = {old[0], old[1], old[0]}; EXPECT(isc_verdict(&d, nullptr, 3, t.data(), &off) == 10 && off == 2); }
  { const uint8_t bound[2] = {0, 1}; std::vector<rt_instance> t = old; t[1].objectToWorld[3] = 2.f;   // a bound instance is held in place like an emitter
    EXPECT(isc_verdict(&d, nullptr, 2, t.data(), &off) == 0); EXPECT(isc_verdict(&d, bound, 2, t.data(), &off) == 9 && off == 1);
    t = {old[0]}; EXPECT(isc_verdict(&d, nullptr, 1, t.data(), &off) == 0); EXPECT(isc_verdict(&d, bound, 1, t.data(), &off) == 9 && off == 1); }
  { rt_scene_desc e = d; e.trigLights = nullptr; std::vector<rt_instance> t = {old[1]}; EXPECT(isc_verdict(&e, nullptr, 1, t.data(), &off) == 0); }   // no triangle lights: no emitter rule
  { rt_scene_desc e = d; std::vector<rt_instance> o = {instanceOf(1, 1, 0.f, 1.f)}; e.numInstances = 1; e.instances = o.data(); e.trigLights = nullptr;
    EXPECT(isc_verdict(&e, nullptr, 1, o.data(), &off) == 8); }
  // expansions against the builder's flatten, over tables with instances that have no triangles first, between and last, mirrored and non-opaque ones
  const std::vector<std::vector<rt_instance>> tables = {
    {old[0], old[1]},
    {old[0], instanceOf(1, 1, 0.f, 1.f), instanceOf(0, 2, 2.f, -1.f), instanceOf(1, 0, 0.f, 1.f), instanceOf(1, 0, 0.f, 1.f), instanceOf(0, 0, 3.f, 2.f), instanceOf(1, 3, 0.f, -1.f)},
    {instanceOf(1, 1, 0.f, 1.f), old[1]},
  };
  for(const std::vector<rt_instance>& t : tables) {
    const uint32_t nI = uint32_t(t.size());
    std::vector<uint32_t> prefix(nI + 1);
    const uint32_t n = isc_expand(&d, nI, t.data(), prefix.data(), nullptr, nullptr);
    std::vector<uint32_t> ref(2 * size_t(n)), rec(3 * size_t(n)), bref(2 * size_t(n)), bflags(n);
    EXPECT(isc_expand(&d, nI, t.data(), prefix.data(), ref.data(), rec.data()) == n);
    rt_scene_desc e = d;
    e.numInstances = nI; e.instances = t.data();
    EXPECT(isc_flatten(&e, 2, bref.data(), bflags.data()) == int64_t(n));
    EXPECT(memcmp(ref.data(), bref.data(), ref.size() * 4) == 0);
    for(uint32_t g = 0; g < n; g++) {
      EXPECT(rec[3 * g] == g && rec[3 * g + 1] == (bflags[g] & ~4u));
      EXPECT(((prefix[ref[2 * g]] >> 31) != 0) == ((bflags[g] & 4u) != 0));
      EXPECT((rec[3 * g + 2] == 0) == ((rec[3 * g + 1] & 1u) != 0));
    }
  }
  printf("ok\n");
  return 0;
}

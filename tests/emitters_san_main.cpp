// emitters_san_main.cpp — TEST INFRASTRUCTURE: a program of its own that drives tests/light_derive_checker.cpp and Scene::emitterMeshes (host/scene.cpp), built by
// tests/test_emitters_cpu.py with -fsanitize=address,undefined and run once on the CPU.  The arrays are exactly as long as the counts say, so a record written past
// a list is reported.  Exit status 0 and "ok" on stdout when nothing was reported and the derived records equal the scene's own.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../cis-565-final-vr-raytracer_amd/host/scene.hpp"

extern "C" int64_t ldc_derive(const rt_scene_desc* d, const rt_instance* table, uint32_t numInstances, const rt_emitter_mesh* meshes, uint32_t numMeshes,
                              const rt_emitter_row* rows, float puncWeight, rt_trig_light* records, rt_light_source* sources, rt_light_buf_info* info, uint32_t* emitting);

using namespace rth;

// the checker's records for `table` against the records the scene computes for it
static int sameAsScene(Scene& scene, const std::vector<rt_instance>& table, const std::vector<rt_emitter_mesh>& meshes, const std::vector<rt_emitter_row>& rows)
{
  rt_light_buf_info info = scene.getDesc(nullptr).lightInfo;
  if(!scene.setInstances(table.data(), uint32_t(table.size()))) return 1;
  const rt_scene_desc d = scene.getDesc(nullptr);
  const int64_t n = ldc_derive(&d, table.data(), uint32_t(table.size()), meshes.data(), uint32_t(meshes.size()), rows.data(), scene.m_puncLightWeight, nullptr, nullptr, nullptr, nullptr);
  if(n != int64_t(d.lightInfo.trigLightSize)) return 2;
  const size_t count = size_t(n);
  std::vector<rt_trig_light> rec(count);
  std::vector<rt_light_source> src(count);
  uint32_t emitting = 0;
  if(ldc_derive(&d, table.data(), uint32_t(table.size()), meshes.data(), uint32_t(meshes.size()), rows.data(), scene.m_puncLightWeight, rec.data(), src.data(), &info, &emitting) != n) return 3;
  if(n && memcmp(rec.data(), d.trigLights, size_t(n) * sizeof(rt_trig_light)) != 0) return 4;
  const std::vector<rt_light_source> want = scene.lightSources();
  if(want.size() != src.size() || (n && memcmp(want.data(), src.data(), size_t(n) * sizeof(rt_light_source)) != 0)) return 5;
  if(memcmp(&info.trigSampProb, &d.lightInfo.trigSampProb, 4) != 0 || info.trigLightSize != d.lightInfo.trigLightSize) return 6;
  return 0;
}

int main()
{
  const struct { ProcScene kind; float scale; } scenes[2] = {{PROC_CORNELL, 1.0f}, {PROC_BISTRO_EXT, 0.004f}};
  for(const auto& sc : scenes) {
    Scene scene;
    if(!scene.loadFromGltfScene(makeProceduralScene(sc.kind, sc.scale, 3), "san")) { printf("scene failed\n"); return 1; }
    std::vector<rt_emitter_mesh> meshes;
    std::vector<rt_emitter_row> rows;
    scene.emitterMeshes(meshes, rows);
    if(meshes.empty() || rows.empty()) { printf("no templates\n"); return 1; }
    const rt_scene_desc d = scene.getDesc(nullptr);
    const std::vector<rt_instance> base(d.instances, d.instances + d.numInstances);
    std::vector<uint8_t> hasTemplate(d.numPrimMeshes, 0);
    for(const rt_emitter_mesh& m : meshes) hasTemplate[m.primMesh] = 1;
    std::vector<rt_instance> emit, plain;
    for(const rt_instance& in : base) (hasTemplate[in.primMesh] ? emit : plain).push_back(in);
    if(emit.empty() || plain.empty()) { printf("no emitter or no plain instance\n"); return 1; }
    rt_instance moved = emit[0];   // mirrored, non-uniformly scaled
    for(int r = 0; r < 3; r++) { moved.objectToWorld[4 * r] *= -1.25f; moved.objectToWorld[4 * r + 1] *= 0.5f; moved.objectToWorld[4 * r + 3] += 0.125f * float(r + 1); }
    std::vector<std::vector<rt_instance>> tables;
    tables.push_back(base);
    { std::vector<rt_instance> t = base; t.push_back(moved); tables.push_back(t); }                      // an emitter at the end
    { std::vector<rt_instance> t = base; t.insert(t.begin(), moved); tables.push_back(t); }              // ... at index 0
    { std::vector<rt_instance> t = plain; t.insert(t.begin() + 1, moved); tables.push_back(t); }         // the only emitter between plain instances
    tables.push_back(plain);                                                                            // no emitter
    tables.push_back(base);                                                                             // ... and back
    for(size_t k = 0; k < tables.size(); k++) {
      const int rc = sameAsScene(scene, tables[k], meshes, rows);
      if(rc) { printf("table %zu: step %d failed\n", k, rc); return 1; }
    }
    // an emissive mesh without a template: the first instance that uses it is named
    const std::vector<rt_emitter_mesh> fewer(meshes.begin() + 1, meshes.end());
    const rt_scene_desc d2 = scene.getDesc(nullptr);
    int64_t first = -1;
    for(size_t i = 0; i < base.size() && first < 0; i++) if(base[i].primMesh == meshes[0].primMesh) first = int64_t(i);
    if(ldc_derive(&d2, base.data(), uint32_t(base.size()), fewer.data(), uint32_t(fewer.size()), rows.data(), 0.f, nullptr, nullptr, nullptr, nullptr) != -1 - first) { printf("verdict failed\n"); return 1; }
    scene.destroy();
  }
  printf("ok\n");
  return 0;
}

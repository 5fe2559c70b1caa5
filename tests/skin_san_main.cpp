// skin_san_main.cpp — TEST INFRASTRUCTURE: a program of its own that drives tests/skin_checker.cpp and Scene::updateVertices (host/scene.cpp), built by
// tests/test_skin_cpu.py with -fsanitize=address,undefined and run once on the CPU.  Exit status 0 and "ok" on stdout when nothing was reported.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../cis-565-final-vr-raytracer_amd/host/scene.hpp"

extern "C" uint32_t skc_skin(const rt_vertex* rest, uint32_t count, const rt_skin_influence* infl, const float* joints, rt_vertex* out);

using namespace rth;

static int poseMesh(Scene& scene, uint32_t mesh, float angle)
{
  const rt_scene_desc d = scene.getDesc(nullptr);
  const rt_prim_mesh pm = d.primMeshes[mesh];
  std::vector<rt_vertex> rest(d.vertices + pm.vertexOffset, d.vertices + pm.vertexOffset + pm.vertexCount), out(pm.vertexCount);
  std::vector<rt_skin_influence> inf(pm.vertexCount);
  for(uint32_t v = 0; v < pm.vertexCount; v++) {
    inf[v] = rt_skin_influence{{0, 1, uint16_t(v % 2), 1}, {0.25f, 0.5f, 0.0f, 0.25f}};
    if(v % 4 == 3) inf[v] = rt_skin_influence{{0, 0, 0, 1}, {0.f, 0.f, 0.f, 1.f}};
  }
  const float c = std::cos(angle), s = std::sin(angle);
  const float joints[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, c, -s, 0, 0.01f, s, c, 0, 0, 0, 0, -1, 0.02f};   // identity; a turn about z that mirrors z
  if(skc_skin(rest.data(), pm.vertexCount, inf.data(), joints, out.data()) != 0) return 1;
  // the whole mesh, a partial range at its end, an empty range at its end; refusals: past the end, a mesh that does not exist
  if(!scene.updateVertices(mesh, 0, pm.vertexCount, out.data())) return 2;
  if(pm.vertexCount > 1 && !scene.updateVertices(mesh, pm.vertexCount - 1, 1, out.data() + pm.vertexCount - 1)) return 3;
  if(!scene.updateVertices(mesh, pm.vertexCount, 0, nullptr)) return 4;
  if(scene.updateVertices(mesh, pm.vertexCount, 1, out.data())) return 5;
  if(scene.updateVertices(d.numPrimMeshes, 0, 1, out.data())) return 6;
  const rt_scene_desc e = scene.getDesc(nullptr);
  for(uint32_t v = 0; v < pm.vertexCount; v++)
    if(e.vertices[pm.vertexOffset + v].position.x != out[v].position.x || e.vertices[pm.vertexOffset + v].normal != out[v].normal) return 7;
  if(e.lightInfo.trigLightSize != d.lightInfo.trigLightSize) return 8;
  return 0;
}

int main()
{
  const struct { ProcScene kind; float scale; } scenes[2] = {{PROC_CORNELL, 1.0f}, {PROC_BISTRO_EXT, 0.004f}};
  for(const auto& sc : scenes) {
    Scene scene;
    if(!scene.loadFromGltfScene(makeProceduralScene(sc.kind, sc.scale, 3), "san")) { printf("scene failed\n"); return 1; }
    const uint32_t n = scene.getDesc(nullptr).numPrimMeshes;
    for(uint32_t m = 0; m < n; m++) {
      const int rc = poseMesh(scene, m, 0.1f * float(m + 1));
      if(rc) { printf("mesh %u: step %d failed\n", m, rc); return 1; }
    }
    scene.destroy();
  }
  printf("ok\n");
  return 0;
}

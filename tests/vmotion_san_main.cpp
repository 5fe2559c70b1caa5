// vmotion_san_main.cpp — TEST INFRASTRUCTURE: a program of its own that drives tests/vmotion_checker.cpp (with oracle/orc_scene.cpp) on the two procedural test
// scenes, built by tests/test_vmotion_cpu.py with -fsanitize=address,undefined and run once on the CPU.  Exit status 0 and "ok" on stdout when nothing was reported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../cis-565-final-vr-raytracer_amd/host/scene.hpp"

extern "C" {
struct vmc_hit { uint32_t inst, prim; float u, v; };
void* vmc_create(const rt_scene_desc* d);
void vmc_destroy(void* p);
int vmc_run(void* p, const rt_state* st, const rt_scene_camera* cam, const float* prevPos, const uint8_t* meshDeformed, const float* prevO2W, const uint8_t* instMoved,
            const uint32_t* thisG, float* d, float* xprev, int32_t* motion32, int16_t* motion16, float* depthD, vmc_hit* hits, float* depthI);
}

using namespace rth;

static int runScene(Scene& scene, int W, int H)
{
  scene.updateCamera(W, H);
  const rt_scene_camera cam = scene.getCamera();
  const rt_scene_desc d = scene.getDesc(nullptr);
  rt_state st;
  std::memset(&st, 0, sizeof(st));
  st.size.x = W; st.size.y = H; st.time = 1000;
  void* k = vmc_create(&d);
  if(!k) return 1;
  const size_t n = size_t(W) * H, nh = size_t(W / 2) * (H / 2);
  std::vector<float> prevPos(size_t(d.numVertices) * 3), prevO2W(size_t(d.numInstances) * 12);
  for(uint32_t v = 0; v < d.numVertices; v++) {   // every vertex a little elsewhere one frame ago
    prevPos[3 * v] = d.vertices[v].position.x + 0.01f; prevPos[3 * v + 1] = d.vertices[v].position.y * 1.01f; prevPos[3 * v + 2] = d.vertices[v].position.z - 0.02f;
  }
  for(uint32_t i = 0; i < d.numInstances; i++) {
    std::memcpy(&prevO2W[12 * size_t(i)], d.instances[i].objectToWorld, 48);
    prevO2W[12 * size_t(i) + 3] += 0.05f;
  }
  std::vector<float> dl(n * 4), xp(n * 3), depthD(n), depthI(nh);
  std::vector<int32_t> m32(n * 2);
  std::vector<int16_t> m16(n * 2);
  std::vector<vmc_hit> hits(n);
  std::vector<uint32_t> g(n * 4, 0u);
  for(size_t p = 0; p < n; p++) {   // a G-buffer: every third pixel a miss, the others at depth 1 + p / n with a packed normal of zero bits
    float depth = (p % 3 == 0) ? 1e30f : 1.0f + float(p) / float(n);
    std::memcpy(&g[4 * p], &depth, 4);
  }
  // nothing flagged: every delta is zero, with and without the arrays
  std::vector<uint8_t> meshNone(d.numPrimMeshes, 0), instNone(d.numInstances, 0);
  for(int pass = 0; pass < 2; pass++) {
    if(vmc_run(k, &st, &cam, pass ? prevPos.data() : nullptr, pass ? meshNone.data() : nullptr, pass ? prevO2W.data() : nullptr, pass ? instNone.data() : nullptr, nullptr,
               dl.data(), xp.data(), m32.data(), m16.data(), depthD.data(), hits.data(), nullptr) != 0) return 2;
    for(float x : dl) if(x != 0.0f) return 3;
  }
  // everything flagged, mesh by mesh and instance by instance, then all at once with the half-resolution pass
  size_t hitPixels = 0, movedPixels = 0;
  for(uint32_t m = 0; m <= d.numPrimMeshes; m++) {
    std::vector<uint8_t> md(d.numPrimMeshes, m == d.numPrimMeshes ? 1 : 0), im(d.numInstances, m == d.numPrimMeshes ? 1 : 0);
    if(m < d.numPrimMeshes) md[m] = 1;
    if(m < d.numInstances) im[d.numInstances - 1 - m] = 1;
    const bool all = m == d.numPrimMeshes;
    if(vmc_run(k, &st, &cam, prevPos.data(), md.data(), prevO2W.data(), im.data(), all ? g.data() : nullptr, dl.data(), xp.data(), m32.data(), m16.data(), depthD.data(),
               hits.data(), all ? depthI.data() : nullptr) != 0) return 4;
    if(all)
      for(size_t p = 0; p < n; p++) {
        if(hits[p].inst == 0xffffffffu) { if(dl[4 * p] != 0.0f || m32[2 * p] != 0 || depthD[p] != 0.0f) return 5; continue; }
        hitPixels++;
        if(hits[p].inst >= d.numInstances) return 6;
        if(dl[4 * p] != 0.0f || dl[4 * p + 1] != 0.0f || dl[4 * p + 2] != 0.0f) movedPixels++;
        if(!std::isfinite(depthD[p])) return 7;
      }
  }
  vmc_destroy(k);
  if(hitPixels == 0 || movedPixels != hitPixels) { printf("%zu hit pixels, %zu with a delta\n", hitPixels, movedPixels); return 8; }
  return 0;
}

int main()
{
  const struct { ProcScene kind; float scale; } scenes[2] = {{PROC_CORNELL, 1.0f}, {PROC_BISTRO_EXT, 0.004f}};
  const int sizes[3][2] = {{16, 8}, {33, 17}, {1, 1}};
  for(const auto& sc : scenes) {
    Scene scene;
    if(!scene.loadFromGltfScene(makeProceduralScene(sc.kind, sc.scale, 3), "san")) { printf("scene failed\n"); return 1; }
    for(const auto& s : sizes) {
      if(s[0] == 1 && sc.kind != PROC_CORNELL) continue;   // (1 x 1: no half-resolution grid at all)
      const int rc = runScene(scene, s[0], s[1]);
      if(rc && !(s[0] == 1 && rc == 8)) { printf("%d x %d: step %d failed\n", s[0], s[1], rc); return 1; }
    }
    scene.destroy();
  }
  printf("ok\n");
  return 0;
}

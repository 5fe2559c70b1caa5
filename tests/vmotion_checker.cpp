// vmotion_checker.cpp — CPU restatement of what per-vertex motion vectors add to a frame (rt_set_object_motion mode RT_OBJECT_MOTION_VERTEX, the RT_VM builds of
// csrc/stages.hip; include/rt_abi.h "Per-vertex motion vectors") for the tests.
// TEST INFRASTRUCTURE: built by tests/vmotion.py together with oracle/orc_scene.cpp, with the oracle's flags; tests/vmotion_san_main.cpp drives it under the
// sanitizers.  Sequential C++ over include/rt_detmath.h (no contraction) and the oracle's raySpawn, closest hit and GetState, in the operation order of the
// definition.  Per full-resolution pixel: the delta d = x_prev - state.position, x_prev itself, the motion index (int32, and saturated to the int16 of
// RT_BUF_MOTION), the direct stage's reprojDepth and the hit (instance, primitive, u, v); per half-resolution pixel the indirect stage's reprojDepth, from the
// frame's G-buffer as getIndirectStateFromGBuffer reconstructs primState.
#include "../oracle/orc_shading.h"
#include <cstring>

namespace {
using namespace orc;

struct Checker { Scene scene; };

ivec2 createMotionIndex(const rt_scene_camera& cam, const rt_state& st, vec3 wpos)   // direct_stage.comp:125-139
{
  vec4 proj = mul(Shader::M(cam.lastProjView), V4(wpos, 1.0f));
  vec3 ndc = xyz(proj) / proj.w;
  vec2 mv = V2(ndc.x, ndc.y) * 0.5f + 0.5f;
  vec2 s = mv * V2(float(st.size.x), float(st.size.y));
  return ivec2{rt_ftoi(s.x), rt_ftoi(s.y)};
}
int16_t sat16(int v) { return int16_t(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }
}  // namespace

extern "C" {

struct vmc_hit { uint32_t inst, prim; float u, v; };   // inst = 0xffffffff at a miss

void* vmc_create(const rt_scene_desc* d)   // the CURRENT scene: moved matrices, deformed vertices
{
  Checker* k = new Checker();
  k->scene.upload(d);
  k->scene.build();
  return k;
}
void vmc_destroy(void* p) { delete static_cast<Checker*>(p); }

// prevPos: 3 floats per scene vertex (read only for the meshes with meshDeformed[m] != 0; may be NULL when none is); prevO2W: 12 floats per instance (read only
// where instMoved[i] != 0; may be NULL when none is).  thisG (W x H x uint4, the frame's G-buffer) and depthI may be NULL: no half-resolution output then.
int vmc_run(void* p, const rt_state* st, const rt_scene_camera* cam, const float* prevPos, const uint8_t* meshDeformed, const float* prevO2W, const uint8_t* instMoved,
            const uint32_t* thisG, float* d, float* xprev, int32_t* motion32, int16_t* motion16, float* depthD, vmc_hit* hits, float* depthI)
{
  Checker* k = static_cast<Checker*>(p);
  const Scene& S = k->scene;
  const int W = st->size.x, H = st->size.y;
  const vec3 lastPosition = toV(cam->lastPosition);
  for(int y = 0; y < H; y++)
    for(int x = 0; x < W; x++) {
      const size_t index = size_t(y) * W + x;
      Shader c(S, *st, *cam);
      c.imageCoords = ivec2{x, y};
      c.seed = tea(uint32_t(W) * uint32_t(y) + uint32_t(x), st->time);   // direct_stage.comp:279
      const Ray r = c.raySpawn(c.imageCoords, ivec2{W, H});
      c.ClosestHit(r);
      d[4 * index] = d[4 * index + 1] = d[4 * index + 2] = d[4 * index + 3] = 0.0f;
      xprev[3 * index] = xprev[3 * index + 1] = xprev[3 * index + 2] = 0.0f;
      motion32[2 * index] = motion32[2 * index + 1] = 0; motion16[2 * index] = motion16[2 * index + 1] = 0;
      depthD[index] = 0.0f;
      hits[index] = vmc_hit{0xffffffffu, 0u, 0.0f, 0.0f};
      if(c.hitT >= RT_INFINITY) continue;
      const State state = c.GetState(r.direction);
      const Tri& T = S.tris[c.hitTri];
      const uint32_t inst = T.inst;
      const uint32_t mesh = S.instances[inst].primMesh;
      hits[index] = vmc_hit{inst, T.prim, c.hitU, c.hitV};
      const bool moved = instMoved && instMoved[inst], deformed = meshDeformed && meshDeformed[mesh];
      vec3 xp = state.position;   // copied when nothing about the pixel's instance changed
      if(moved || deformed) {
        const rt_prim_mesh& geo = S.primMeshes[mesh];
        const uint32_t* tri = &S.indices[geo.firstIndex + 3 * T.prim];
        vec3 q[3];
        for(int j = 0; j < 3; j++) {
          const size_t v = size_t(geo.vertexOffset) + tri[j];
          q[j] = deformed ? V3(prevPos[3 * v], prevPos[3 * v + 1], prevPos[3 * v + 2]) : toV(S.vertices[v].position);
        }
        const vec3 bary = V3((1.0f - c.hitU) - c.hitV, c.hitU, c.hitV);
        const vec3 pos = (q[0] * bary.x + q[1] * bary.y) + q[2] * bary.z;
        const float* P = moved ? prevO2W + 12 * size_t(inst) : S.instances[inst].objectToWorld;
        xp.x = ((P[0] * pos.x + P[1] * pos.y) + P[2] * pos.z) + P[3];
        xp.y = ((P[4] * pos.x + P[5] * pos.y) + P[6] * pos.z) + P[7];
        xp.z = ((P[8] * pos.x + P[9] * pos.y) + P[10] * pos.z) + P[11];
      }
      const vec3 dv = xp - state.position;
      d[4 * index] = dv.x; d[4 * index + 1] = dv.y; d[4 * index + 2] = dv.z;
      xprev[3 * index] = xp.x; xprev[3 * index + 1] = xp.y; xprev[3 * index + 2] = xp.z;
      const ivec2 m = createMotionIndex(*cam, *st, xp);
      motion32[2 * index] = m.x; motion32[2 * index + 1] = m.y;
      motion16[2 * index] = sat16(m.x); motion16[2 * index + 1] = sat16(m.y);
      depthD[index] = length(lastPosition - xp);
    }
  if(!thisG || !depthI) return RT_OK;
  const ivec2 indSize{W / 2, H / 2};
  for(int y = 0; y < indSize.y; y++)
    for(int x = 0; x < indSize.x; x++) {
      const size_t idx = size_t(y) * indSize.x + x, full = size_t(2 * y) * W + 2 * x;
      depthI[idx] = 0.0f;
      Shader c(S, *st, *cam);
      const Ray ray = c.raySpawn(ivec2{x, y}, indSize);
      const uint32_t* g = thisG + full * 4;
      const float depth = rt_u2f(g[0]);   // getIndirectStateFromGBuffer, pathtrace.glsl:296-313
      if(depth >= RT_INFINITY * 0.8f) continue;
      vec3 position = ray.origin + ray.direction * depth;
      const vec3 normal = decompress_unit_vec(g[1]);
      const vec3 ffnormal = dot(normal, ray.direction) <= 0.0f ? normal : -normal;
      position += ffnormal * 2e-2f;   // indirect_stage.comp:299: primState is the offset state
      const vec3 dv = V3(d[4 * full], d[4 * full + 1], d[4 * full + 2]);
      depthI[idx] = length(lastPosition - (position + dv));
    }
  return RT_OK;
}

}  // extern "C"

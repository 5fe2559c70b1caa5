// light_checker.cpp — sequential CPU restatement of the light-record rewrite of rt_set_light_sources (include/rt_abi.h "Light sources") for the tests.
// TEST INFRASTRUCTURE: built by tests/lights.py with g++ -ffp-contract=off -fno-fast-math; shares no code with csrc/light_records.hip.  Plain fp32, one rounding
// per written operation, in the order of xformPointRaw: ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3].
// Input: the arrays of a scene description (prim meshes, vertices, indices, instances), the sources and the records; output: the records, rewritten in place.
// The GPU tests compare the device light array with lgc_rewrite's records word for word.
#include <cstdint>
#include <cstring>
#include "../include/rt_abi.h"

namespace {

rt_vec3 xform(const float* m, const rt_vec3& p)
{
  rt_vec3 o;
  o.x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
  o.y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
  o.z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
  return o;
}

}  // namespace

extern "C" {

// 0 when every source names an instance and a triangle that exist and every record's matIndex is its prim mesh's materialIndex; else 1 + the first bad record
uint32_t lgc_validate(const rt_prim_mesh* primMeshes, const rt_instance* instances, uint32_t numInstances, const rt_light_source* sources, uint32_t count, const rt_trig_light* records)
{
  for(uint32_t k = 0; k < count; k++) {
    if(sources[k].instance >= numInstances) return 1 + k;
    const rt_prim_mesh& pm = primMeshes[instances[sources[k].instance].primMesh];
    if(sources[k].triangle >= pm.indexCount / 3 || records[k].matIndex != uint32_t(pm.materialIndex)) return 1 + k;
  }
  return 0;
}

// rewrites v0 v1 v2 of every record whose source instance is dirty (dirty == NULL: every record); returns the number of records rewritten.
// No other byte of a record is touched.
uint32_t lgc_rewrite(const rt_prim_mesh* primMeshes, const rt_vertex* vertices, const uint32_t* indices, const rt_instance* instances, const rt_light_source* sources,
                     uint32_t count, const uint8_t* dirty, rt_trig_light* records)
{
  uint32_t rewritten = 0;
  for(uint32_t k = 0; k < count; k++) {
    const uint32_t inst = sources[k].instance;
    if(dirty && !dirty[inst]) continue;
    const rt_instance& in = instances[inst];
    const rt_prim_mesh& pm = primMeshes[in.primMesh];
    const uint32_t* ix = indices + pm.firstIndex + 3 * size_t(sources[k].triangle);
    const rt_vec3 w[3] = {xform(in.objectToWorld, vertices[pm.vertexOffset + ix[0]].position), xform(in.objectToWorld, vertices[pm.vertexOffset + ix[1]].position),
                          xform(in.objectToWorld, vertices[pm.vertexOffset + ix[2]].position)};
    memcpy(&records[k].v0, &w[0], sizeof(rt_vec3));
    memcpy(&records[k].v1, &w[1], sizeof(rt_vec3));
    memcpy(&records[k].v2, &w[2], sizeof(rt_vec3));
    rewritten++;
  }
  return rewritten;
}

}  // extern "C"

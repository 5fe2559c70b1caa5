// light_derive_checker.cpp — sequential CPU restatement of the derived triangle-light records of the emitter mode (include/rt_abi.h "Emitters") for the tests.
// TEST INFRASTRUCTURE: built by tests/emitters.py with g++ -ffp-contract=off -fno-fast-math; shares no code with csrc/light_derive.hip, csrc/rt_api.cpp or
// host/alias_table.hpp.  Plain fp32, one rounding per written operation.
// Input: the arrays of a scene description (prim meshes, vertices, indices, materials, lightInfo), an instance table, the templates and the punctual weight;
// output: the records (all 96 bytes), the binding and lightInfo.  The tests compare it with host Scene::setInstances and with the device light array word for word.
#include <cstdint>
#include <cstring>
#include <vector>
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

float weightOf(const rt_scene_desc& d, int32_t material)
{
  const rt_vec3& e = d.materials[material > 0 ? material : 0].emissiveFactor;
  return e.x * 0.2126f + e.y * 0.7152f + e.z * 0.0722f;
}

struct Bucket { float prob; int32_t id; };

// Vose's table as the reference builds it: weights scaled to mean 1, two stacks filled in index order, the most recent small bucket topped up from the most
// recent large one; what is left keeps its own index
void aliasTable(const std::vector<float>& weights, float total, std::vector<Bucket>& table)
{
  const int n = int(weights.size());
  const float scale = float(n) / total;
  std::vector<Bucket> large, small;
  table.assign(size_t(n), Bucket{0.f, 0});
  for(int i = 0; i < n; i++) {
    const float w = weights[size_t(i)] * scale;
    if(w > 1.f) large.push_back(Bucket{w, i}); else small.push_back(Bucket{w, i});
  }
  while(!large.empty() && !small.empty()) {
    Bucket b = large.back(), s = small.back();
    large.pop_back(); small.pop_back();
    table[size_t(s.id)] = Bucket{s.prob, b.id};
    b.prob -= (1.f - s.prob);
    if(b.prob > 1.f) large.push_back(b); else small.push_back(b);
  }
  for(const Bucket& b : large) table[size_t(b.id)] = b;
  for(const Bucket& b : small) table[size_t(b.id)] = b;
}

}  // namespace

extern "C" {

// The derived list of `table` (numInstances rows) under the templates.  Returns the record count, or -1 - i where instance i uses an emissive prim mesh (the
// scene's light rule) that has no template.  records / sources may be NULL (the count alone); emitting: instances that have a template; info: in, the lightInfo
// before the call (its punctual count, and the trigSampProb that stays where no light of either kind exists); out, the derived one.
int64_t ldc_derive(const rt_scene_desc* d, const rt_instance* table, uint32_t numInstances, const rt_emitter_mesh* meshes, uint32_t numMeshes, const rt_emitter_row* rows,
                   float puncWeight, rt_trig_light* records, rt_light_source* sources, rt_light_buf_info* info, uint32_t* emitting)
{
  std::vector<int64_t> templ(d->numPrimMeshes, -1);
  for(uint32_t m = 0; m < numMeshes; m++) templ[meshes[m].primMesh] = int64_t(m);
  std::vector<float> weights;
  uint32_t nEmit = 0;
  for(uint32_t i = 0; i < numInstances; i++) {
    const rt_prim_mesh& pm = d->primMeshes[table[i].primMesh];
    if(templ[table[i].primMesh] < 0) {
      if(weightOf(*d, pm.materialIndex) > 1e-2f) return -1 - int64_t(i);
      continue;
    }
    nEmit++;
    const rt_emitter_mesh& em = meshes[size_t(templ[table[i].primMesh])];
    for(uint32_t r = em.firstRow; r < em.firstRow + em.rowCount; r++) {
      const size_t k = weights.size();
      weights.push_back(weightOf(*d, pm.materialIndex));
      if(!records) continue;
      rt_trig_light t;
      memset(&t, 0, sizeof(t));
      t.matIndex = uint32_t(pm.materialIndex);
      t.transformIndex = 0xffffffffu;
      const uint32_t* ix = d->indices + pm.firstIndex + 3 * size_t(rows[r].triangle);
      t.v0 = xform(table[i].objectToWorld, d->vertices[pm.vertexOffset + ix[0]].position);
      t.v1 = xform(table[i].objectToWorld, d->vertices[pm.vertexOffset + ix[1]].position);
      t.v2 = xform(table[i].objectToWorld, d->vertices[pm.vertexOffset + ix[2]].position);
      memcpy(&t.uv0, rows[r].uv, 6 * sizeof(float));
      records[k] = t;
      if(sources) sources[k] = rt_light_source{i, rows[r].triangle};
    }
  }
  float total = 0.f;
  for(const float w : weights) total += w;
  if(records && !weights.empty()) {
    std::vector<Bucket> table2;
    aliasTable(weights, total, table2);
    for(size_t k = 0; k < weights.size(); k++)
      records[k].impSamp = rt_impt_samp{table2[k].id, table2[k].prob, weights[k] / total, weights[size_t(table2[k].id)] / total};
  }
  if(emitting) *emitting = nEmit;
  if(info) {
    info->trigLightSize = uint32_t(weights.size());
    if(info->puncLightSize > 0 || info->trigLightSize > 0) info->trigSampProb = total / (total + puncWeight);
  }
  return int64_t(weights.size());
}

}  // extern "C"

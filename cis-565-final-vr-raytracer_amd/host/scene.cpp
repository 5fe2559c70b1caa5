// scene.cpp — host Scene: the data products of the reference's Scene class (src/scene.cpp), minus Vulkan.
#include "scene.hpp"
#include "alias_table.hpp"
#include "pack.h"
#include <algorithm>
#include <cstdio>
#include <cstring>

namespace rth {

void Scene::destroy()
{
  m_gltf = GltfScene{};
  m_primMeshes.clear(); m_vertices.clear(); m_instances.clear(); m_materials.clear(); m_textures.clear();
  m_puncLights.clear(); m_trigLights.clear();
  m_lightBufInfo = rt_light_buf_info{};
  m_puncLightWeight = m_trigLightWeight = 0.f;
  m_stats = SceneStats{};
}

bool Scene::load(const std::string& filename)  // scene.cpp:57-125
{
  GltfScene g;
  std::string err;
  if(!loadGltfFile(filename, g, err)) { fprintf(stderr, "Scene::load: %s\n", err.c_str()); return false; }
  size_t slash = filename.find_last_of("/\\"), dot = filename.find_last_of('.');
  std::string stem = filename.substr(slash == std::string::npos ? 0 : slash + 1, dot == std::string::npos ? std::string::npos : dot - (slash == std::string::npos ? 0 : slash + 1));
  return loadFromGltfScene(std::move(g), stem);
}

bool Scene::loadFromGltfScene(GltfScene&& gltf, const std::string& name)
{
  destroy();
  m_gltf = std::move(gltf);
  m_sceneName = name;
  GltfScene& g = m_gltf;
  if(g.positions.empty() || g.primMeshes.empty() || g.nodes.empty()) return false;
  if(g.materials.empty()) g.materials.push_back(GltfMaterial{});
  const size_t nv = g.positions.size();
  // importDrawableNodes(..., Normal | Texcoord_0 | Tangent | Color_0) fills missing attributes (scene.cpp:73-74).
  // nvpro_core is not vendored; the fill rules below are this build's (DESIGN.md §Scene ingest).
  if(g.normals.size() != nv) {
    g.normals.assign(nv, V3{0, 0, 0});
    for(const GltfPrimMesh& pm : g.primMeshes)
      for(uint32_t i = 0; i + 2 < pm.indexCount; i += 3) {
        uint32_t a = pm.vertexOffset + g.indices[pm.firstIndex + i], b = pm.vertexOffset + g.indices[pm.firstIndex + i + 1], c = pm.vertexOffset + g.indices[pm.firstIndex + i + 2];
        V3 n = cross(g.positions[b] - g.positions[a], g.positions[c] - g.positions[a]);
        g.normals[a] = g.normals[a] + n; g.normals[b] = g.normals[b] + n; g.normals[c] = g.normals[c] + n;
      }
    for(V3& n : g.normals) n = length(n) > 0 ? normalize(n) : V3{0, 1, 0};
  }
  if(g.texcoords0.size() != nv) g.texcoords0.assign(nv, {0.f, 0.f});
  if(g.colors0.size() != nv) g.colors0.assign(nv, {1.f, 1.f, 1.f, 1.f});
  if(g.tangents.size() != nv) {
    g.tangents.resize(nv);
    for(size_t i = 0; i < nv; i++) {
      V3 n = g.normals[i];
      V3 c1 = cross(n, V3{0, 0, 1}), c2 = cross(n, V3{0, 1, 0});
      V3 t = normalize(length(c1) > length(c2) ? c1 : c2);
      g.tangents[i] = {t.x, t.y, t.z, 1.f};
    }
  }
  g.bboxMin = V3{3e38f, 3e38f, 3e38f}; g.bboxMax = V3{-3e38f, -3e38f, -3e38f};
  for(const GltfNode& nd : g.nodes) {
    const GltfPrimMesh& pm = g.primMeshes[nd.primMesh];
    for(uint32_t v = 0; v < pm.vertexCount; v++) {
      V3 p = xformPoint(nd.worldMatrix, g.positions[pm.vertexOffset + v]);
      g.bboxMin = {std::min(g.bboxMin.x, p.x), std::min(g.bboxMin.y, p.y), std::min(g.bboxMin.z, p.z)};
      g.bboxMax = {std::max(g.bboxMax.x, p.x), std::max(g.bboxMax.y, p.y), std::max(g.bboxMax.z, p.z)};
    }
  }
  // setCameraFromScene, scene.cpp:295-314
  if(!g.cameras.empty()) setCamera(g.cameras[0].eye, g.cameras[0].center, g.cameras[0].up, g.cameras[0].yfovDeg);
  else fitCamera();
  m_camera = rt_scene_camera{};
  m_camera.nbLights = int(g.lights.size());
  m_cameraInit = false;
  m_lastEye = V3{0, 0, 0};

  // scene.cpp:94-103
  createMaterialBuffer();
  createPuncLightBuffer();
  m_textures.clear();
  if(g.textures.empty()) { TextureImage w; w.bgra = {255, 255, 255, 255}; g.textures.push_back(w); }  // "cannot be empty" default (scene.cpp:575-583)
  for(const TextureImage& t : g.textures) m_textures.push_back(rt_texture{t.bgra.data(), t.width, t.height, t.wrapS, t.wrapT, t.magFilter, 0});
  createVertexBuffer();
  createInstanceDataBuffer();
  createTrigLightBuffer();
  if(m_lightBufInfo.puncLightSize > 0 || m_lightBufInfo.trigLightSize > 0)
    m_lightBufInfo.trigSampProb = m_trigLightWeight / (m_trigLightWeight + m_puncLightWeight);

  m_stats = SceneStats{};
  for(const GltfPrimMesh& pm : g.primMeshes) m_stats.triangles += pm.indexCount / 3;
  for(const GltfNode& nd : g.nodes) m_stats.instancedTriangles += g.primMeshes[nd.primMesh].indexCount / 3;
  m_stats.vertices = nv; m_stats.primMeshes = uint32_t(g.primMeshes.size()); m_stats.nodes = uint32_t(g.nodes.size());
  m_stats.materials = uint32_t(g.materials.size()); m_stats.textures = uint32_t(g.textures.size());
  m_stats.puncLights = m_lightBufInfo.puncLightSize; m_stats.trigLights = m_lightBufInfo.trigLightSize;
  return true;
}

void Scene::fitCamera()
{
  const GltfScene& g = m_gltf;
  V3 c = (g.bboxMin + g.bboxMax) * 0.5f;
  float r = length(g.bboxMax - g.bboxMin) * 0.5f;
  m_fov = 45.f;
  float d = r / std::tan(m_fov * 0.5f * 3.14159265f / 180.f);
  setCamera(c + V3{0, 0, d}, c, V3{0, 1, 0}, m_fov);
}

void Scene::createMaterialBuffer()  // scene.cpp:415-448
{
  m_materials.clear();
  for(const GltfMaterial& m : m_gltf.materials) {
    rt_material s{};
    s.pbrBaseColorFactor = rt_vec4{m.baseColorFactor[0], m.baseColorFactor[1], m.baseColorFactor[2], m.baseColorFactor[3]};
    s.pbrBaseColorTexture = m.baseColorTexture;
    s.pbrMetallicFactor = m.metallicFactor;
    s.pbrRoughnessFactor = m.roughnessFactor;
    s.pbrMetallicRoughnessTexture = m.metallicRoughnessTexture;
    s.emissiveTexture = m.emissiveTexture;
    s.emissiveFactor = rt_vec3{m.emissiveFactor[0], m.emissiveFactor[1], m.emissiveFactor[2]};
    s.normalTexture = m.normalTexture;
    s.normalTextureScale = m.normalTextureScale;
    s.transmissionFactor = m.transmissionFactor;
    s.transmissionTexture = m.transmissionTexture;
    s.ior = std::min(std::max(m.ior, 1.f), RT_MAX_IOR_MINUS_ONE + 1.f);
    s.alphaMode = m.alphaMode;
    s.alphaCutoff = m.alphaCutoff;
    m_materials.push_back(s);
  }
}

void Scene::createPuncLightBuffer()  // scene.cpp:319-353 + createPuncLightImptSampAccel :700-726
{
  m_puncLights.clear();
  for(const GltfLight& l : m_gltf.lights) {
    rt_punc_light p{};
    p.position = R3(xformPoint(l.worldMatrix, V3{0, 0, 0}));
    p.direction = R3(xformDir(l.worldMatrix, V3{0, 0, -1}));
    p.color = rt_vec3{l.color[0], l.color[1], l.color[2]};
    p.innerConeCos = std::cos(l.innerConeAngle);
    p.outerConeCos = std::cos(l.outerConeAngle);
    p.range = l.range;
    p.intensity = l.intensity;
    p.type = l.type;
    m_puncLights.push_back(p);
  }
  m_lightBufInfo.puncLightSize = uint32_t(m_puncLights.size());
  m_puncLightWeight = 0.f;
  if(!m_puncLights.empty()) {
    std::vector<float> distrib;
    float total = 0.f;
    for(const rt_punc_light& l : m_puncLights) {
      float power = luminance(&l.color.x) * l.intensity * 3.1416f * 4.f;
      distrib.push_back(power);
      total += power;
    }
    std::vector<AliasBucket> table = buildAliasTable(distrib);
    for(size_t i = 0; i < distrib.size(); i++)
      m_puncLights[i].impSamp = rt_impt_samp{table[i].failId, table[i].prob, distrib[i] / total, distrib[size_t(table[i].failId)] / total};
    m_puncLightWeight = total;
  }
}

void Scene::createVertexBuffer()  // scene.cpp:209-289
{
  const GltfScene& g = m_gltf;
  m_vertices.resize(g.positions.size());
  for(size_t i = 0; i < g.positions.size(); i++) {
    rt_vertex v{};
    v.position = R3(g.positions[i]);
    v.normal = compressUnitVec(g.normals[i].x, g.normals[i].y, g.normals[i].z);
    v.tangent = compressUnitVec(g.tangents[i][0], g.tangents[i][1], g.tangents[i][2]);
    v.texcoord = rt_vec2{g.texcoords0[i][0], g.texcoords0[i][1]};
    v.color = packUnorm4x8(g.colors0[i][0], g.colors0[i][1], g.colors0[i][2], g.colors0[i][3]);
    uint32_t bits = floatBits(v.texcoord.y);  // tangent handedness in the LSB of V (scene.cpp:249-257)
    if(g.tangents[i][3] > 0) bits |= 1u; else bits &= ~1u;
    v.texcoord.y = bitsFloat(bits);
    m_vertices[i] = v;
  }
  m_primMeshes.clear();
  for(const GltfPrimMesh& pm : g.primMeshes) m_primMeshes.push_back(rt_prim_mesh{pm.vertexOffset, pm.vertexCount, pm.firstIndex, pm.indexCount, pm.materialIndex});
}

void Scene::createInstanceDataBuffer()  // scene.cpp:179-195 (InstanceData rows == m_primMeshes) + accelstruct.cpp:132-162
{
  const GltfScene& g = m_gltf;
  m_instances.clear();
  for(const GltfNode& nd : g.nodes) {
    rt_instance in{};
    for(int r = 0; r < 3; r++) for(int c = 0; c < 4; c++) in.objectToWorld[r * 4 + c] = nd.worldMatrix.at(r, c);
    in.primMesh = uint32_t(nd.primMesh);
    const GltfMaterial& mat = g.materials[size_t(std::max(0, g.primMeshes[nd.primMesh].materialIndex))];
    if(mat.alphaMode == 0 || (mat.baseColorFactor[3] == 1.0f && mat.baseColorTexture == -1)) in.flags |= RT_INST_FORCE_OPAQUE;
    if(mat.doubleSided == 1) in.flags |= RT_INST_CULL_DISABLE;
    m_instances.push_back(in);
  }
}

void Scene::createTrigLightBuffer()  // scene.cpp:355-409 + createTrigLightImptSampAccel :741-772
{
  const GltfScene& g = m_gltf;
  m_trigLights.clear();
  for(const GltfNode& node : g.nodes) {
    const GltfPrimMesh& pm = g.primMeshes[node.primMesh];
    const GltfMaterial& mat = g.materials[size_t(std::max(0, pm.materialIndex))];
    if(luminance(mat.emissiveFactor) > 1e-2f) {
      for(uint32_t idx = pm.firstIndex; idx + 1 < pm.firstIndex + pm.indexCount; idx += 3) {  // `idx < first+count-1` (quirk 11)
        rt_trig_light t{};
        uint32_t i0 = g.indices[idx] + pm.vertexOffset, i1 = g.indices[idx + 1] + pm.vertexOffset, i2 = g.indices[idx + 2] + pm.vertexOffset;
        t.transformIndex = 0xffffffffu;  // `transforms.size()-1` on an empty vector (quirk 11); unused by the shaders
        t.matIndex = uint32_t(pm.materialIndex);
        t.v0 = R3(xformPoint(node.worldMatrix, g.positions[i0])); t.uv0 = rt_vec2{g.texcoords0[i0][0], g.texcoords0[i0][1]};
        t.v1 = R3(xformPoint(node.worldMatrix, g.positions[i1])); t.uv1 = rt_vec2{g.texcoords0[i1][0], g.texcoords0[i1][1]};
        t.v2 = R3(xformPoint(node.worldMatrix, g.positions[i2])); t.uv2 = rt_vec2{g.texcoords0[i2][0], g.texcoords0[i2][1]};
        m_trigLights.push_back(t);
      }
    }
  }
  m_trigLightWeight = 0.f;
  if(!m_trigLights.empty()) {
    std::vector<float> distrib;
    float total = 0.f;
    for(const rt_trig_light& t : m_trigLights) {
      float power = luminance(g.materials[t.matIndex].emissiveFactor);  // not area-weighted (scene.cpp:750-756)
      distrib.push_back(power);
      total += power;
    }
    std::vector<AliasBucket> table = buildAliasTable(distrib);
    for(size_t i = 0; i < m_trigLights.size(); i++)
      m_trigLights[i].impSamp = rt_impt_samp{table[i].failId, table[i].prob, distrib[i] / total, distrib[size_t(table[i].failId)] / total};
    m_trigLightWeight = total;
  }
  m_lightBufInfo.trigLightSize = uint32_t(m_trigLights.size());
}

std::vector<rt_light_source> Scene::lightSources() const
{
  const GltfScene& g = m_gltf;
  std::vector<rt_light_source> out;
  for(size_t n = 0; n < g.nodes.size(); n++) {   // the loops and the light rule of createTrigLightBuffer
    const GltfPrimMesh& pm = g.primMeshes[g.nodes[n].primMesh];
    const GltfMaterial& mat = g.materials[size_t(std::max(0, pm.materialIndex))];
    if(luminance(mat.emissiveFactor) > 1e-2f)
      for(uint32_t idx = pm.firstIndex; idx + 1 < pm.firstIndex + pm.indexCount; idx += 3)  // (quirk 11)
        out.push_back(rt_light_source{uint32_t(n), (idx - pm.firstIndex) / 3u});
  }
  return out;
}

void Scene::emitterMeshes(std::vector<rt_emitter_mesh>& meshes, std::vector<rt_emitter_row>& rows) const
{
  const GltfScene& g = m_gltf;
  meshes.clear(); rows.clear();
  for(size_t m = 0; m < g.primMeshes.size(); m++) {   // the light rule, the loop bound and the texcoords of createTrigLightBuffer, per prim mesh
    const GltfPrimMesh& pm = g.primMeshes[m];
    if(pm.materialIndex < 0 || !(luminance(g.materials[size_t(pm.materialIndex)].emissiveFactor) > 1e-2f)) continue;
    rt_emitter_mesh em{uint32_t(m), uint32_t(rows.size()), 0u, 0u};
    for(uint32_t idx = pm.firstIndex; idx + 1 < pm.firstIndex + pm.indexCount && idx + 2 < pm.firstIndex + pm.indexCount; idx += 3) {  // (quirk 11; a partial last triangle has no template row)
      rt_emitter_row r{};
      r.triangle = (idx - pm.firstIndex) / 3u;
      for(int k = 0; k < 3; k++) {
        const uint32_t v = g.indices[idx + k] + pm.vertexOffset;
        r.uv[2 * k] = g.texcoords0[v][0]; r.uv[2 * k + 1] = g.texcoords0[v][1];
      }
      rows.push_back(r);
    }
    em.rowCount = uint32_t(rows.size()) - em.firstRow;
    meshes.push_back(em);
  }
}

void Scene::updateCamera(int width, int height)  // scene.cpp:777-795
{
  const float aspect = float(width) / float(height);
  const M4 view = lookAt(m_eye, m_center, m_up);
  M4 proj = perspectiveVK(m_fov, aspect, 0.001f, 1000.0f);  // CAMERA_NEAR / CAMERA_FAR, host_device.h:151-152
  proj.at(0, 2) += .5f / float(width);                      // fixed half-pixel jitter (scene.cpp:783-787)
  proj.at(1, 2) += .5f / float(height);
  M4 prevViewInverse, prevProjView;
  memcpy(prevViewInverse.m, m_camera.viewInverse.m, sizeof(prevViewInverse.m));
  memcpy(prevProjView.m, m_camera.projView.m, sizeof(prevProjView.m));
  m_camera.lastProjView = toRt(prevProjView);
  m_camera.lastView = toRt(invert(prevViewInverse));
  m_camera.viewInverse = toRt(invert(view));
  m_camera.projInverse = toRt(invert(proj));
  m_camera.projView = toRt(proj * view);
  m_camera.lastPosition = R3(m_lastEye);  // `static eye` starts at 0 (scene.cpp:780)
  m_lastEye = m_eye;
  m_cameraInit = true;
}

bool Scene::updateInstances(const uint32_t* ids, const float* transforms, uint32_t count)
{
  for(uint32_t k = 0; k < count; k++) if(ids[k] >= m_gltf.nodes.size()) return false;
  for(uint32_t k = 0; k < count; k++) {
    M4 m = M4::identity();
    for(int r = 0; r < 3; r++) for(int c = 0; c < 4; c++) m.at(r, c) = transforms[12 * k + r * 4 + c];
    m_gltf.nodes[ids[k]].worldMatrix = m;
    memcpy(m_instances[ids[k]].objectToWorld, transforms + 12 * k, 12 * sizeof(float));
  }
  createTrigLightBuffer();   // (every emissive node: the records keep their order, and the alias table depends on the materials only)
  if(m_lightBufInfo.puncLightSize > 0 || m_lightBufInfo.trigLightSize > 0)
    m_lightBufInfo.trigSampProb = m_trigLightWeight / (m_trigLightWeight + m_puncLightWeight);
  return true;
}

bool Scene::setInstances(const rt_instance* instances, uint32_t count)
{
  if(!instances || count == 0) return false;
  for(uint32_t k = 0; k < count; k++) if(instances[k].primMesh >= m_gltf.primMeshes.size()) return false;
  m_gltf.nodes.resize(count);
  m_stats.instancedTriangles = 0;
  for(uint32_t k = 0; k < count; k++) {
    M4 m = M4::identity();
    for(int r = 0; r < 3; r++) for(int c = 0; c < 4; c++) m.at(r, c) = instances[k].objectToWorld[r * 4 + c];
    m_gltf.nodes[k].worldMatrix = m;
    m_gltf.nodes[k].primMesh = int(instances[k].primMesh);
    m_stats.instancedTriangles += m_gltf.primMeshes[instances[k].primMesh].indexCount / 3;
  }
  m_stats.nodes = count;
  m_instances.assign(instances, instances + count);
  createTrigLightBuffer();   // (as updateInstances; under the emitter rule the records keep their order and count)
  m_stats.trigLights = uint32_t(m_trigLights.size());
  if(m_lightBufInfo.puncLightSize > 0 || m_lightBufInfo.trigLightSize > 0)
    m_lightBufInfo.trigSampProb = m_trigLightWeight / (m_trigLightWeight + m_puncLightWeight);
  return true;
}

bool Scene::updateVertices(uint32_t primMesh, uint32_t first, uint32_t count, const rt_vertex* rows)
{
  if(primMesh >= m_gltf.primMeshes.size()) return false;
  const GltfPrimMesh& pm = m_gltf.primMeshes[primMesh];
  if(uint64_t(first) + count > pm.vertexCount || (count && !rows)) return false;
  for(uint32_t k = 0; k < count; k++) {
    const size_t i = size_t(pm.vertexOffset) + first + k;
    m_vertices[i] = rows[k];
    m_gltf.positions[i] = V3{rows[k].position.x, rows[k].position.y, rows[k].position.z};
  }
  createTrigLightBuffer();   // (as updateInstances: the records keep their order, the alias table depends on the materials only)
  if(m_lightBufInfo.puncLightSize > 0 || m_lightBufInfo.trigLightSize > 0)
    m_lightBufInfo.trigSampProb = m_trigLightWeight / (m_trigLightWeight + m_puncLightWeight);
  return true;
}

bool Scene::setMaterials(const uint32_t* ids, const rt_material* rows, uint32_t count, bool* lightsChanged)
{
  if(lightsChanged) *lightsChanged = false;
  if(count && (!ids || !rows)) return false;
  for(uint32_t k = 0; k < count; k++) {
    if(ids[k] >= m_materials.size() || ids[k] >= m_gltf.materials.size()) return false;
    const float* was = m_gltf.materials[ids[k]].emissiveFactor;
    const V3 e{rows[k].emissiveFactor.x, rows[k].emissiveFactor.y, rows[k].emissiveFactor.z};
    if((luminance(was) > 1e-2f) != (luminance(&e.x) > 1e-2f)) return false;   // the light rule: the emissive meshes are fixed by the scene
  }
  bool emission = false;
  for(uint32_t k = 0; k < count; k++) {
    m_materials[ids[k]] = rows[k];
    float* e = m_gltf.materials[ids[k]].emissiveFactor;
    const float n[3] = {rows[k].emissiveFactor.x, rows[k].emissiveFactor.y, rows[k].emissiveFactor.z};
    if(memcmp(e, n, sizeof(n)) != 0) { memcpy(e, n, sizeof(n)); emission = true; }
  }
  if(emission) {   // the records' weights and the alias table depend on the emission
    createTrigLightBuffer();
    if(m_lightBufInfo.puncLightSize > 0 || m_lightBufInfo.trigLightSize > 0)
      m_lightBufInfo.trigSampProb = m_trigLightWeight / (m_trigLightWeight + m_puncLightWeight);
    if(lightsChanged) *lightsChanged = true;
  }
  return true;
}

bool Scene::setTexture(uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* bgra, size_t rowPitchBytes)
{
  if(texture >= m_gltf.textures.size() || texture >= m_textures.size() || !bgra || w == 0 || h == 0 || rowPitchBytes < size_t(w) * 4) return false;
  TextureImage& t = m_gltf.textures[texture];
  if(uint64_t(x) + w > uint64_t(t.width) || uint64_t(y) + h > uint64_t(t.height) || t.bgra.size() < size_t(t.width) * size_t(t.height) * 4) return false;
  for(uint32_t r = 0; r < h; r++) memcpy(t.bgra.data() + ((size_t(y) + r) * size_t(t.width) + x) * 4, bgra + size_t(r) * rowPitchBytes, size_t(w) * 4);
  return true;
}

rt_scene_desc Scene::getDesc(const HdrSampling* env) const
{
  rt_scene_desc d{};
  d.numPrimMeshes = uint32_t(m_primMeshes.size()); d.primMeshes = m_primMeshes.data();
  d.numVertices = m_vertices.size(); d.vertices = m_vertices.data();
  d.numIndices = m_gltf.indices.size(); d.indices = m_gltf.indices.data();
  d.numInstances = uint32_t(m_instances.size()); d.instances = m_instances.data();
  d.numMaterials = uint32_t(m_materials.size()); d.materials = m_materials.data();
  d.numTextures = uint32_t(m_textures.size()); d.textures = m_textures.data();
  d.puncLights = m_puncLights.empty() ? nullptr : m_puncLights.data();
  d.trigLights = m_trigLights.empty() ? nullptr : m_trigLights.data();
  d.lightInfo = m_lightBufInfo;
  if(env && env->width() > 0) {
    d.envWidth = env->width(); d.envHeight = env->height();
    d.envRgba32f = env->pixels().data(); d.envAccel = env->accel().data();
  }
  return d;
}

}  // namespace rth

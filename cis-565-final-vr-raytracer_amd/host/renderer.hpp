// renderer.hpp — C++ host classes with the reference's stage-dispatcher / acceleration-structure interfaces
// (src/renderer.hpp:49-61, src/accelstruct.hpp:40-46) whose bodies are calls into the C-ABI of include/rt_abi.h.
// Header-only: link the application with librestir_hip.so (+ librestir_host.so for Scene / HdrSampling).
#pragma once
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/rt_abi.h"
#include "scene.hpp"

namespace rth {

// src/accelstruct.hpp:40-46: setup / create / destroy.  create() = BLAS per prim mesh + TLAS per node in the reference
// (accelstruct.cpp:55-162); here the scene arrays go to HBM and a flat BVH8 is built over them.
class AccelStructure {
 public:
  void setup(rt_ctx* ctx) { m_ctx = ctx; }
  bool create(const Scene& scene, const HdrSampling* env)
  {
    rt_scene_desc d = scene.getDesc(env);
    if(rt_upload_scene(m_ctx, &d) != RT_OK || rt_build_accel(m_ctx) != RT_OK) { fprintf(stderr, "AccelStructure::create: %s\n", rt_last_error(m_ctx)); return false; }
    // the scene knows which triangle every triangle-light record came from (include/rt_abi.h "Light sources"): bound here, the update calls move the emitters'
    // records with the geometry on the GPU, and skins on emissive meshes are accepted
    const std::vector<rt_light_source> src = scene.lightSources();
    if(d.trigLights && !src.empty() && rt_set_light_sources(m_ctx, uint32_t(src.size()), src.data()) != RT_OK) {
      fprintf(stderr, "AccelStructure::create: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  // Move instances without a rebuild (include/rt_abi.h "Moving instances"): ids + count x 12 floats (3 x 4 row-major).  The reference rebuilds its TLAS per frame
  // (accelstruct.cpp:132-162); here the moved instances' leaf records are rewritten and the BVH8 above them refitted on the GPU.
  bool update(const uint32_t* ids, const float* transforms, uint32_t count)
  {
    if(rt_update_instances(m_ctx, count, ids, transforms) != RT_OK) { fprintf(stderr, "AccelStructure::update: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // Scene::updateInstances (host side: instance table, triangle-light records) + update() + rt_update_lights with the records the scene recomputed
  bool update(Scene& scene, const uint32_t* ids, const float* transforms, uint32_t count)
  {
    if(!scene.updateInstances(ids, transforms, count)) { fprintf(stderr, "AccelStructure::update: instance id out of range\n"); return false; }
    if(!update(ids, transforms, count)) return false;
    const rt_scene_desc d = scene.getDesc(nullptr);
    if(rt_update_lights(m_ctx, d.trigLights, d.trigLights ? d.lightInfo.trigLightSize : 0, d.puncLights, d.puncLights ? d.lightInfo.puncLightSize : 0, &d.lightInfo) != RT_OK) {
      fprintf(stderr, "AccelStructure::update: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  // Deforming meshes (include/rt_abi.h "Deforming meshes"): host-computed rows for one prim mesh (the scene's copy and its triangle-light records follow, then the
  // device rows, the refit and the light records), or skins posed on the GPU from joint matrices (setSkins once, updateSkins per frame).
  bool updateVertices(Scene& scene, uint32_t primMesh, uint32_t first, uint32_t count, const rt_vertex* rows)
  {
    if(!scene.updateVertices(primMesh, first, count, rows)) { fprintf(stderr, "AccelStructure::updateVertices: prim mesh or range out of bounds\n"); return false; }
    const rt_scene_desc d = scene.getDesc(nullptr);
    if(rt_update_vertices(m_ctx, primMesh, first, count, rows) != RT_OK ||
       rt_update_lights(m_ctx, d.trigLights, d.trigLights ? d.lightInfo.trigLightSize : 0, d.puncLights, d.puncLights ? d.lightInfo.puncLightSize : 0, &d.lightInfo) != RT_OK) {
      fprintf(stderr, "AccelStructure::updateVertices: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  bool setSkins(const std::vector<rt_skin>& skins, const std::vector<rt_skin_influence>& influences)
  {
    if(rt_set_skins(m_ctx, uint32_t(skins.size()), skins.data(), influences.size(), influences.data()) != RT_OK) { fprintf(stderr, "AccelStructure::setSkins: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  bool updateSkins(const uint32_t* skinIds, const float* jointMatrices, uint32_t count)
  {
    if(rt_update_skins(m_ctx, count, skinIds, jointMatrices) != RT_OK) { fprintf(stderr, "AccelStructure::updateSkins: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // Morph targets (include/rt_abi.h "Morph targets"): deltas once (after setSkins where a mesh has both), weights per frame; a morphed mesh that has a skin is
  // skinned with the matrices of its last updateSkins.
  bool setMorphTargets(const std::vector<rt_morph_set>& sets, const std::vector<rt_morph_delta>& deltas)
  {
    if(rt_set_morph_targets(m_ctx, uint32_t(sets.size()), sets.data(), deltas.size(), deltas.data()) != RT_OK) { fprintf(stderr, "AccelStructure::setMorphTargets: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  bool updateMorphs(const uint32_t* setIds, const float* weights, uint32_t count)
  {
    if(rt_update_morphs(m_ctx, count, setIds, weights) != RT_OK) { fprintf(stderr, "AccelStructure::updateMorphs: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // A new topology for the moved scene, built on the GPU (include/rt_abi.h "Rebuilding on the device"): the host's remedy when rt_refit_stats::fullRefit is set
  // or the refitted tree has become slow.  The previous tree stays in place when it fails.
  bool rebuild()
  {
    if(rt_rebuild_accel(m_ctx) != RT_OK) { fprintf(stderr, "AccelStructure::rebuild: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // The builder of every later rebuild() / setInstances() (include/rt_abi.h "The PLOC builder"): RT_REBUILD_LBVH (default) or RT_REBUILD_PLOC, a tighter tree
  // that takes longer to build; radius / maxIterations 0 = the defaults.  Builds nothing.
  bool setRebuildOptions(int builder, int radius = 0, int maxIterations = 0)
  {
    const rt_rebuild_options o{builder, radius, maxIterations, 0};
    if(rt_set_rebuild_options(m_ctx, &o) != RT_OK) { fprintf(stderr, "AccelStructure::setRebuildOptions: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  rt_rebuild_options rebuildOptions() const { rt_rebuild_options o{}; (void)rt_get_rebuild_options(m_ctx, &o); return o; }
  // Add and remove instances without a new scene (include/rt_abi.h "Adding and removing instances"): the whole new table.  Emitters stay where they are in it.
  bool setInstances(const rt_instance* instances, uint32_t count)
  {
    if(rt_set_instances(m_ctx, count, instances) != RT_OK) { fprintf(stderr, "AccelStructure::setInstances: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // Scene::setInstances (host side: nodes, instance table, light records) + setInstances().  What the scene would refuse (an empty table, a prim mesh out of
  // range) is checked first and the device, whose checks are the stricter ones, is asked before the scene changes: a refused table changes neither.
  bool setInstances(Scene& scene, const rt_instance* instances, uint32_t count)
  {
    bool sceneTakesIt = instances && count > 0;
    for(uint32_t k = 0; sceneTakesIt && k < count; k++) sceneTakesIt = instances[k].primMesh < scene.getScene().primMeshes.size();
    if(!sceneTakesIt) { fprintf(stderr, "AccelStructure::setInstances: an empty table or a prim mesh out of range\n"); return false; }
    if(!setInstances(instances, count)) return false;
    if(!scene.setInstances(instances, count)) { fprintf(stderr, "AccelStructure::setInstances: the scene refused the table\n"); return false; }
    return true;
  }
  // Edit materials and texels without a new scene (include/rt_abi.h "Editing materials and textures"): the device is asked first, its checks are the stricter
  // ones; then the scene's own tables follow.  Only where an emission changed, and the scene recomputed its light records, are they handed over
  // (rt_update_lights), as update() does for a move (in the emitter mode the device has refused a row that changes an emitter's luminance before the scene is asked).
  bool setMaterials(Scene& scene, const uint32_t* ids, const rt_material* rows, uint32_t count)
  {
    if(rt_update_materials(m_ctx, count, ids, rows) != RT_OK) { fprintf(stderr, "AccelStructure::setMaterials: %s\n", rt_last_error(m_ctx)); return false; }
    bool lightsChanged = false;
    if(!scene.setMaterials(ids, rows, count, &lightsChanged)) { fprintf(stderr, "AccelStructure::setMaterials: the scene refused the rows\n"); return false; }
    if(!lightsChanged) return true;
    const rt_scene_desc d = scene.getDesc(nullptr);
    if(rt_update_lights(m_ctx, d.trigLights, d.trigLights ? d.lightInfo.trigLightSize : 0, d.puncLights, d.puncLights ? d.lightInfo.puncLightSize : 0, &d.lightInfo) != RT_OK) {
      fprintf(stderr, "AccelStructure::setMaterials: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  bool setTexture(Scene& scene, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* bgra, size_t rowPitchBytes)
  {
    if(rt_update_texture(m_ctx, texture, x, y, w, h, bgra, rowPitchBytes) != RT_OK) { fprintf(stderr, "AccelStructure::setTexture: %s\n", rt_last_error(m_ctx)); return false; }
    if(!scene.setTexture(texture, x, y, w, h, bgra, rowPitchBytes)) { fprintf(stderr, "AccelStructure::setTexture: the scene refused the rectangle\n"); return false; }
    return true;
  }
  // Swap the environment without a new scene (include/rt_abi.h "The environment"): the device builds the importance table; the HdrSampling then adopts texels,
  // table, integral and average, so that getIntegral() (rt_state.envMapLuminIntegInv = 1 / it) and getAverage() describe what the context uses.
  bool setEnvironment(HdrSampling& env, const float* rgba, int w, int h)
  {
    if(rt_set_environment(m_ctx, w, h, rgba, nullptr) != RT_OK) { fprintf(stderr, "AccelStructure::setEnvironment: %s\n", rt_last_error(m_ctx)); return false; }
    rt_environment_stats s{};
    (void)rt_get_environment_stats(m_ctx, &s);
    std::vector<rt_impt_samp> table(size_t(s.width) * size_t(s.height));
    std::vector<float> texels(table.size() * 4);
    if(rt_environment_readback(m_ctx, RT_ENV_ACCEL, table.data(), table.size() * sizeof(rt_impt_samp)) != RT_OK ||
       rt_environment_readback(m_ctx, RT_ENV_TEXELS, texels.data(), texels.size() * sizeof(float)) != RT_OK) {
      fprintf(stderr, "AccelStructure::setEnvironment: %s\n", rt_last_error(m_ctx));
      return false;
    }
    env.adoptEnvironment(texels.data(), s.width, s.height, table.data(), s.integral, s.average);   // (the texels as stored: 1 x 1 black for an empty map)
    return true;
  }
  rt_environment_stats environmentStats() const { rt_environment_stats s{}; (void)rt_get_environment_stats(m_ctx, &s); return s; }
  rt_material_stats materialStats() const { rt_material_stats s{}; (void)rt_get_material_stats(m_ctx, &s); return s; }
  rt_instances_stats instancesStats() const { rt_instances_stats s{}; (void)rt_get_instances_stats(m_ctx, &s); return s; }
  rt_rebuild_stats rebuildStats() const { rt_rebuild_stats s{}; (void)rt_get_rebuild_stats(m_ctx, &s); return s; }
  void destroy() {}  // owned by the context
 private:
  rt_ctx* m_ctx = nullptr;
};

// src/renderer.hpp:49-61
class Renderer {
 public:
  bool setup(int device = 0)  // renderer.cpp:62-73
  {
    if(rt_create(&m_ctx, device) != RT_OK) { fprintf(stderr, "Renderer::setup: %s\n", rt_last_error(nullptr)); return false; }
    return true;
  }
  void destroy() { if(m_ctx) rt_destroy(m_ctx); m_ctx = nullptr; }  // renderer.cpp:75-91
  // Object motion vectors (include/rt_abi.h "Object motion vectors"): temporal reuse follows moved instances; off by default
  bool setObjectMotion(bool on)
  {
    if(rt_set_object_motion(m_ctx, on ? RT_OBJECT_MOTION_ON : RT_OBJECT_MOTION_OFF) != RT_OK) { fprintf(stderr, "Renderer::setObjectMotion: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // Per-vertex motion vectors (include/rt_abi.h "Per-vertex motion vectors"): temporal reuse follows deformed meshes as well as moved instances
  bool setVertexMotion(bool on)
  {
    if(rt_set_object_motion(m_ctx, on ? RT_OBJECT_MOTION_VERTEX : RT_OBJECT_MOTION_OFF) != RT_OK) { fprintf(stderr, "Renderer::setVertexMotion: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // renderer.cpp:97-148: screen-space buffers for `size` (the reference also creates 7 pipelines + descriptor sets here)
  bool create(int width, int height, Scene* scene) { (void)scene; return update(width, height); }
  // renderer.cpp:154-206: the 12 dispatches of one frame
  bool run(const rt_state& state, int frames)
  {
    if(rt_render_frame(m_ctx, &state, frames) != RT_OK) { fprintf(stderr, "Renderer::run: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // (no counterpart in the reference, which records into one queue) priorities of the schedule's indirect / filter streams; unset, the context decides at its first frame
  bool setStreamPriorities(int indirectLevel, int filterLevel)
  {
    if(rt_set_stream_priorities(m_ctx, indirectLevel, filterLevel) != RT_OK) { fprintf(stderr, "Renderer::setStreamPriorities: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  const std::string name() { return std::string("HIP-gfx950"); }  // renderer.hpp:55 returns "RQ"
  bool update(int width, int height)  // renderer.cpp:209-225
  {
    m_width = width; m_height = height;
    if(rt_resize(m_ctx, width, height) != RT_OK) { fprintf(stderr, "Renderer::update: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  bool setCamera(const rt_scene_camera& cam) { return rt_set_camera(m_ctx, &cam) == RT_OK; }  // Scene::updateCamera's UBO upload
  // the two HDR images post.frag sums (post.frag:129); `frames` selects the ping-pong side like RenderOutput::getDescSet
  bool readResult(int frames, std::vector<float>& direct, std::vector<float>& indirect)
  {
    const size_t n = size_t(m_width) * m_height * 4;
    direct.resize(n); indirect.resize(n);
    return rt_readback(m_ctx, RT_BUF_DIRECT_RESULT0 + (frames & 1), direct.data(), n * sizeof(float)) == RT_OK
           && rt_readback(m_ctx, RT_BUF_INDIRECT_RESULT0 + (frames & 1), indirect.data(), n * sizeof(float)) == RT_OK;
  }
  // Reference mode (include/rt_abi.h, ABI 2.4): the progressive ground-truth path tracer the reference left as RtxState.accumulate / frame +
  // SampleExample::updateFrame's m_maxFrames (sample_example.cpp:176-204).  Adds `samples` samples per pixel; the sums reset by themselves when
  // the view, the size, the scene, the sun & sky or maxDepth / hdrMultiplier / environmentProb / MIS change.
  bool referenceRender(const rt_state& state, int samples)
  {
    if(rt_reference_render(m_ctx, &state, samples) != RT_OK) { fprintf(stderr, "Renderer::referenceRender: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  void referenceReset() { rt_reference_reset(m_ctx); }
  uint32_t referenceSamples()
  {
    uint32_t n = 0;
    rt_reference_samples(m_ctx, &n);
    return n;
  }
  // RGBA32F mean of component 0 (direct), 1 (indirect) or 2 (sum)
  bool readReference(int component, std::vector<float>& rgba)
  {
    rgba.resize(size_t(m_width) * m_height * 4);
    return rt_reference_readback(m_ctx, component, rgba.data(), rgba.size() * sizeof(float)) == RT_OK;
  }
  // Denoiser selection (include/rt_abi.h): the reference's A-Trous chain (default) or the variance-guided spatiotemporal filter its README asks for
  // ("Future Work -> Better Denoiser"); the SVGF history resets by itself on resize, a new scene / tree, a settings change and a frame with denoise == 0.
  bool setDenoiser(const rt_denoiser& d)
  {
    if(rt_set_denoiser(m_ctx, &d) != RT_OK) { fprintf(stderr, "Renderer::setDenoiser: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  rt_denoiser getDenoiser()
  {
    rt_denoiser d{};
    rt_get_denoiser(m_ctx, &d);
    return d;
  }
  bool denoiserReset() { return rt_denoiser_reset(m_ctx) == RT_OK; }
  // the SVGF history the last SVGF frame wrote: which = 0 direct colour + n (RGBA32F, W x H), 1 indirect colour + n (W/2 x H/2), 2 / 3 the moments
  // (2 x f32 per pixel) of direct / indirect.  False before the first SVGF frame after a resize.
  bool readDenoiserHistory(int which, std::vector<float>& out)
  {
    const size_t px = (which & 1) ? size_t(m_width / 2) * (m_height / 2) : size_t(m_width) * m_height;
    out.resize(px * (which < 2 ? 4 : 2));
    if(rt_denoiser_readback(m_ctx, which, out.data(), out.size() * sizeof(float)) != RT_OK) {
      fprintf(stderr, "Renderer::readDenoiserHistory: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  // ReSTIR GI spatial reuse (include/rt_abi.h): off by default; RT_GI_SPATIAL_ON resamples each half-resolution pixel's indirect reservoir with its
  // neighbours' after the indirect stage, RT_GI_SPATIAL_VISIBILITY also traces a shadow ray per accepted neighbour.  Nothing carries over between frames.
  bool setGiSpatial(const rt_gi_spatial& s)
  {
    if(rt_set_gi_spatial(m_ctx, &s) != RT_OK) { fprintf(stderr, "Renderer::setGiSpatial: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  rt_gi_spatial getGiSpatial()
  {
    rt_gi_spatial s{};
    rt_get_gi_spatial(m_ctx, &s);
    return s;
  }
  // the resampled reservoirs of the last frame rendered with the mode on, (W/2) x (H/2).  False before the first such frame after a resize.
  bool readGiSpatialReservoirs(std::vector<rt_indirect_reservoir>& out)
  {
    out.resize(size_t(m_width / 2) * (m_height / 2));
    if(rt_gi_spatial_readback(m_ctx, out.data(), out.size() * sizeof(rt_indirect_reservoir)) != RT_OK) {
      fprintf(stderr, "Renderer::readGiSpatialReservoirs: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  // Temporal anti-aliasing (include/rt_abi.h): off by default.  With RT_TAA_ON the context jitters the camera it renders each frame with (keep passing
  // unjittered matrices to setCamera) and resolves the frame into a history after compose; RenderOutput::run then shows the resolved frame.
  bool setTaa(const rt_taa& t)
  {
    if(rt_set_taa(m_ctx, &t) != RT_OK) { fprintf(stderr, "Renderer::setTaa: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  rt_taa getTaa()
  {
    rt_taa t{};
    rt_get_taa(m_ctx, &t);
    return t;
  }
  bool taaReset() { return rt_taa_reset(m_ctx) == RT_OK; }
  // the last resolved frame: direct and indirect RGBA32F (W x H).  False before the first resolved frame after a resize.
  bool readTaaResult(std::vector<float>& direct, std::vector<float>& indirect)
  {
    direct.resize(size_t(m_width) * m_height * 4);
    indirect.resize(direct.size());
    if(rt_taa_readback(m_ctx, 0, direct.data(), direct.size() * sizeof(float)) != RT_OK ||
       rt_taa_readback(m_ctx, 1, indirect.data(), indirect.size() * sizeof(float)) != RT_OK) {
      fprintf(stderr, "Renderer::readTaaResult: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  // Temporal upsampling (include/rt_abi.h): off by default.  With RT_UPSCALE_TEMPORAL the context keeps rendering at the size create() / update() set, with a
  // jittered camera (keep passing unjittered matrices to setCamera), and resolves each frame into a history at outWidth x outHeight after compose.  The
  // output-size frame is read with readUpscaleResult / upscaleTonemap; RenderOutput::run keeps showing the render-size frame.
  bool setUpscale(const rt_upscale& u)
  {
    if(rt_set_upscale(m_ctx, &u) != RT_OK) { fprintf(stderr, "Renderer::setUpscale: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  rt_upscale getUpscale()
  {
    rt_upscale u{};
    rt_get_upscale(m_ctx, &u);
    return u;
  }
  bool upscaleReset() { return rt_upscale_reset(m_ctx) == RT_OK; }
  // the last resolved frame: direct and indirect RGBA32F (outWidth x outHeight).  False before the first resolved frame.
  bool readUpscaleResult(std::vector<float>& direct, std::vector<float>& indirect)
  {
    const rt_upscale u = getUpscale();
    direct.resize(size_t(u.outWidth) * u.outHeight * 4);
    indirect.resize(direct.size());
    if(rt_upscale_readback(m_ctx, 0, direct.data(), direct.size() * sizeof(float)) != RT_OK ||
       rt_upscale_readback(m_ctx, 1, indirect.data(), indirect.size() * sizeof(float)) != RT_OK) {
      fprintf(stderr, "Renderer::readUpscaleResult: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  // the post pass over the resolved frame `frames` at the output size; rgba: outWidth x outHeight RGBA8, row-major, top row first
  bool upscaleTonemap(const rt_tonemapper& tm, int frames, std::vector<uint8_t>& rgba)
  {
    const rt_upscale u = getUpscale();
    rgba.resize(size_t(u.outWidth) * u.outHeight * 4);
    if(rt_upscale_tonemap(m_ctx, &tm, frames) != RT_OK || rt_upscale_readback(m_ctx, 3, rgba.data(), rgba.size()) != RT_OK) {
      fprintf(stderr, "Renderer::upscaleTonemap: %s\n", rt_last_error(m_ctx));
      return false;
    }
    return true;
  }
  rt_ctx* context() { return m_ctx; }
 private:
  rt_ctx* m_ctx = nullptr;
  int m_width = 0, m_height = 0;
};

// src/render_output.hpp:37-73: the display pass.  run() is the fullscreen post.frag draw (render_output.cpp:224-237) as a
// compute pass into an RGBA8 image; the two HDR result images themselves live in the context (RT_BUF_*_RESULT*).
class RenderOutput {
 public:
  rt_tonemapper m_tm{1.0f, 1.0f, 1.0f, 0.0f, 1.0f, 1.0f, {1.0f, 1.0f}, 0, 0.5f, 0.5f, 0};      // render_output.hpp:44-55
  rt_tonemapper m_depthTm{0.0f, 2.2f, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f}, 0, 0.0f, 0.0f, 0};  // render_output.hpp:56-60
  void setup(rt_ctx* ctx) { m_ctx = ctx; }
  void create(int width, int height) { update(width, height); }
  void update(int width, int height) { m_width = width; m_height = height; }
  void destroy() {}
  bool run(const rt_state& state, float zoom, rt_vec2 ratio, int frames)
  {
    rt_tonemapper tm = (state.debugging_mode == RT_DBG_DEPTH) ? m_depthTm : m_tm;  // render_output.cpp:228-230
    tm.zoom = zoom; tm.renderingRatio = ratio;
    if(rt_tonemap(m_ctx, &tm, state.debugging_mode, frames) != RT_OK) { fprintf(stderr, "RenderOutput::run: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // run() over the two means of the reference mode instead of a frame's result images
  bool runReference(float zoom, rt_vec2 ratio)
  {
    rt_tonemapper tm = m_tm;
    tm.zoom = zoom; tm.renderingRatio = ratio;
    if(rt_reference_tonemap(m_ctx, &tm) != RT_OK) { fprintf(stderr, "RenderOutput::runReference: %s\n", rt_last_error(m_ctx)); return false; }
    return true;
  }
  // the image the reference presents: RGBA8, row-major, top row first
  bool readImage(std::vector<uint8_t>& rgba)
  {
    rgba.resize(size_t(m_width) * m_height * 4);
    return rt_readback(m_ctx, RT_BUF_LDR, rgba.data(), rgba.size()) == RT_OK;
  }
 private:
  rt_ctx* m_ctx = nullptr;
  int m_width = 0, m_height = 0;
};

}  // namespace rth

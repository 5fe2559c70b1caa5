// restir_demo — the reference application's call order without the window (src/main.cpp:50-264, src/sample_example.cpp):
//   loadEnvironmentHdr -> loadScene (Scene::load + AccelStructure::create) -> createRender -> per frame:
//   updateFrame / Scene::updateCamera -> Renderer::run -> (post.frag's sum of the two HDR images, written to disk)
// Usage mirrors main.cpp:52-54:  restir_demo [-f scene.gltf | -p cornell|helmet|sponza|bistro|interior] [-e env.hdr]
//                                            [-w 1920] [-h 1080] [-n frames] [-o out] [-s scale] [-a autoExposure] [-r samples] [-d atrous|svgf] [-g off|on|vis] [-t off|on] [-u WxH]
// -d svgf: the variance-guided spatiotemporal denoiser (rt_set_denoiser, default settings) instead of the reference's A-Trous chain.
// -g on|vis: ReSTIR GI spatial reuse (rt_set_gi_spatial, default settings; vis = with a visibility ray per accepted neighbour).
// -t on: temporal anti-aliasing (rt_set_taa, default settings): the PFM and PNG show the resolved frame.  (-a is taken by autoExposure.)
// -u WxH: temporal upsampling (rt_set_upscale, default settings) to the output size W x H (between 1x and 4x of -w / -h per axis): the frames are rendered
//       at -w x -h, the PFM, PPM and PNG come from the resolved frame at the output size.  Not together with -t on.
// -r N: after the real-time frames, N samples per pixel of the reference mode (rt_reference_render: the converged image the frame estimates)
//       at the last frame's camera, tonemapped like the frame into <out>_reference.png.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include "renderer.hpp"

using namespace rth;

static const char* arg(int argc, char** argv, const char* key, const char* def)
{
  for(int i = 1; i + 1 < argc; i++) if(strcmp(argv[i], key) == 0) return argv[i + 1];
  return def;
}

int main(int argc, char** argv)
{
  const int W = atoi(arg(argc, argv, "-w", "1920")), H = atoi(arg(argc, argv, "-h", "1080")), frames = atoi(arg(argc, argv, "-n", "32"));
  const std::string file = arg(argc, argv, "-f", ""), proc = arg(argc, argv, "-p", "cornell"), envFile = arg(argc, argv, "-e", ""), out = arg(argc, argv, "-o", "frame");
  const float scale = float(atof(arg(argc, argv, "-s", "1.0")));

  HdrSampling sky;
  bool haveSky = false;
  if(!envFile.empty()) haveSky = sky.loadEnvironment(envFile);
  else if(proc != "cornell") { sky.makeSyntheticSky(2048, 1024, 5e4f, 7); haveSky = true; }

  Scene scene;
  scene.setup();
  if(!file.empty()) { if(!scene.load(file)) { fprintf(stderr, "cannot load %s\n", file.c_str()); return 1; } }
  else {
    const char* names[] = {"cornell", "helmet", "sponza", "bistro", "interior"};
    int kind = 0;
    for(int i = 0; i < 5; i++) if(proc == names[i]) kind = i;
    scene.loadFromGltfScene(makeProceduralScene(ProcScene(kind), scale, 1), proc);
  }
  const SceneStats& s = scene.getStat();
  printf("scene %s: %llu triangles (%llu instanced), %u materials, %u textures, %u emissive triangles\n", scene.getSceneName().c_str(),
         (unsigned long long)s.triangles, (unsigned long long)s.instancedTriangles, s.materials, s.textures, s.trigLights);

  Renderer render;
  if(!render.setup(0)) return 2;
  AccelStructure accel;
  accel.setup(render.context());
  if(!accel.create(scene, haveSky ? &sky : nullptr)) return 3;
  if(!render.create(W, H, &scene)) return 4;

  // RtxState as SampleExample fills it (sample_example.hpp:154-184, sample_example.cpp:87, 104-105)
  rt_state st{};
  st.maxDepth = 4; st.modulate = 1; st.fireflyClampThreshold = haveSky ? sky.getIntegral() * 4.f : 100.f; st.hdrMultiplier = 1.f;
  st.environmentProb = haveSky ? 0.25f : 0.f; st.ReSTIRState = RT_RESTIR_TEMPORAL; st.RISSampleNum = 4; st.reservoirClamp = 80;
  st.size = rt_ivec2{W, H}; st.envMapLuminIntegInv = haveSky ? 1.f / sky.getIntegral() : 0.f;
  st.lightLuminIntegInv = 1.f / (scene.m_trigLightWeight + scene.m_puncLightWeight); st.MIS = 1;
  st.sigLuminDirect = 0.4f; st.sigNormalDirect = 0.1f; st.sigDepthDirect = 0.02f; st.denoise = 1;
  st.sigLuminIndirect = 4.f; st.sigNormalIndirect = 0.4f; st.sigDepthIndirect = 1.f;

  const std::string denoiser = arg(argc, argv, "-d", "atrous");
  if(denoiser != "atrous" && denoiser != "svgf") { fprintf(stderr, "-d must be atrous or svgf\n"); return 11; }
  if(denoiser == "svgf") {
    rt_denoiser d = render.getDenoiser();
    d.mode = RT_DENOISER_SVGF;
    if(!render.setDenoiser(d)) return 11;
  }
  const std::string giSpatial = arg(argc, argv, "-g", "off");
  if(giSpatial != "off" && giSpatial != "on" && giSpatial != "vis") { fprintf(stderr, "-g must be off, on or vis\n"); return 12; }
  if(giSpatial != "off") {
    rt_gi_spatial g = render.getGiSpatial();
    g.mode = giSpatial == "vis" ? RT_GI_SPATIAL_VISIBILITY : RT_GI_SPATIAL_ON;
    if(!render.setGiSpatial(g)) return 12;
  }

  const std::string taaMode = arg(argc, argv, "-t", "off");
  if(taaMode != "off" && taaMode != "on") { fprintf(stderr, "-t must be off or on\n"); return 13; }
  if(taaMode == "on") {
    rt_taa t = render.getTaa();
    t.mode = RT_TAA_ON;
    if(!render.setTaa(t)) return 13;
  }

  const std::string upscaleSize = arg(argc, argv, "-u", "");
  int OW = W, OH = H;   // the size of the images written
  if(!upscaleSize.empty()) {
    if(sscanf(upscaleSize.c_str(), "%dx%d", &OW, &OH) != 2) { fprintf(stderr, "-u must be <width>x<height>\n"); return 14; }
    rt_upscale u = render.getUpscale();
    u.mode = RT_UPSCALE_TEMPORAL; u.outWidth = OW; u.outHeight = OH;
    if(!render.setUpscale(u)) return 14;
  }
  const bool upscaled = !upscaleSize.empty();

  auto t0 = std::chrono::steady_clock::now();
  for(int f = 0; f < frames; f++) {
    scene.updateCamera(W, H);
    render.setCamera(scene.getCamera());
    st.frame = f; st.time = 1000u + unsigned(f);
    if(!render.run(st, f)) return 5;
  }
  rt_sync(render.context());
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("%d frames %dx%d: %.3f ms/frame\n", frames, W, H, ms / frames);

  std::vector<float> d, i;
  if(upscaled ? !render.readUpscaleResult(d, i) : (taaMode == "on" ? !render.readTaaResult(d, i) : !render.readResult(frames - 1, d, i))) return 6;
  {  // PFM (bottom-up scanlines, little endian) of direct + indirect = the HDR frame
    std::ofstream pfm(out + ".pfm", std::ios::binary);
    pfm << "PF\n" << OW << " " << OH << "\n-1.0\n";
    for(int y = OH - 1; y >= 0; y--) for(int x = 0; x < OW; x++) { float c[3]; for(int k = 0; k < 3; k++) c[k] = d[(size_t(y) * OW + x) * 4 + k] + i[(size_t(y) * OW + x) * 4 + k]; pfm.write(reinterpret_cast<const char*>(c), 12); }
  }
  {  // the displayed frame: RenderOutput::run (post.frag: Uncharted 2 tone curve + dither) -> PPM + PNG
    RenderOutput offscreen;
    offscreen.setup(render.context());
    offscreen.create(W, H);
    offscreen.m_tm.autoExposure = atoi(arg(argc, argv, "-a", "0"));
    std::vector<uint8_t> rgba;
    if(upscaled) {   // the same post pass over the resolved frame at the output size
      rt_tonemapper tm = offscreen.m_tm;
      tm.zoom = 1.0f; tm.renderingRatio = rt_vec2{1.0f, 1.0f};
      if(!render.upscaleTonemap(tm, frames - 1, rgba)) return 7;
    } else if(!offscreen.run(st, 1.0f, rt_vec2{1.0f, 1.0f}, frames - 1) || !offscreen.readImage(rgba)) return 7;
    std::ofstream ppm(out + ".ppm", std::ios::binary);
    ppm << "P6\n" << OW << " " << OH << "\n255\n";
    for(size_t p = 0; p < size_t(OW) * OH; p++) ppm.write(reinterpret_cast<const char*>(&rgba[p * 4]), 3);
    if(!writePng(out + ".png", rgba.data(), OW, OH)) fprintf(stderr, "cannot write %s.png\n", out.c_str());
  }
  const int refSamples = atoi(arg(argc, argv, "-r", "0"));
  if(refSamples > 0) {
    const auto r0 = std::chrono::steady_clock::now();
    for(int done = 0; done < refSamples; done += 16)   // (calls of 16 samples: the sums do not depend on the split)
      if(!render.referenceRender(st, std::min(16, refSamples - done))) return 8;
    RenderOutput offscreen;
    offscreen.setup(render.context());
    offscreen.create(W, H);
    offscreen.m_tm.autoExposure = atoi(arg(argc, argv, "-a", "0"));
    std::vector<uint8_t> rgba;
    if(!offscreen.runReference(1.0f, rt_vec2{1.0f, 1.0f}) || !offscreen.readImage(rgba)) return 9;
    const double rms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count();
    printf("reference: %u samples per pixel %dx%d in %.1f ms\n", render.referenceSamples(), W, H, rms);
    if(!writePng(out + "_reference.png", rgba.data(), W, H)) { fprintf(stderr, "cannot write %s_reference.png\n", out.c_str()); return 10; }
  }
  render.destroy();
  return 0;
}

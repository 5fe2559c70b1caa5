// reference.h — launchers of the progressive ground-truth path tracer (csrc/reference.hip, rt_reference_render).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"
namespace rt {
// The seed of sample `sample` (0-based since the last reset) of pixel (x, y) of a W-wide image: tea(W * y + x, tea(sample, REF_SEED_SALT)).
// (include/rt_abi.h states the same formula; tests/refpt_checker.cpp restates it.)
constexpr uint32_t REF_SEED_SALT = 0x52454631u;   // "REF1"
// Per pixel six fp64 sums: direct rgb, indirect rgb (48 B).
constexpr int REF_ACC_DOUBLES = 6;
// One launch adds ONE sample to the pixels of rows [rowBegin, rowEnd); rt_api.cpp cuts the image into row bands of at most this many pixels.
constexpr int REF_BAND_PIXELS = 1 << 20;
#define RT_DECL_REF(ns)                                                                                                                      \
  namespace ns {                                                                                                                             \
  hipError_t launchReference(hipStream_t stream, const DevScene& S, const rt_state& st, const rt_scene_camera& cam, double* acc, uint32_t sample, \
                             int rowBegin, int rowEnd);                                                                                      \
  }
RT_DECL_REF(ref_base)   // HDR environment only (reference.hip)
RT_DECL_REF(ref_sky)    // procedural sun & sky compiled in (reference.hip with RT_SKY)
#undef RT_DECL_REF
// mean of `component` (0 direct, 1 indirect, 2 direct + indirect) over n samples -> RGBA32F, a = 1: float(sum / n) (component 2: float((direct + indirect) / n)),
// every operation in IEEE double, one rounding to float at the end; n == 0 gives (0, 0, 0, 1) and does not read `acc`
hipError_t launchReferenceMean(hipStream_t stream, const double* acc, uint32_t n, int component, size_t pixels, float4* out);
}  // namespace rt

// filter_common.h — what the screen-space passes share bit for bit: the A-Trous chain (filters.hip), SVGF (svgf.hip) and TAA (taa.hip) reconstruct
// a pixel's position with the one function below and weight their 5 x 5 taps with the one table.
#pragma once
#include "stage_common.h"

namespace rt {

// denoise_common.glsl:27-40: the direction is not re-normalised after the view transform
RT_DEV f3 cameraPosDenoise(const rt_scene_camera& cam, i2 coord, float dist, i2 imageSize)
{
  const f2 pixelCenter = mk2(float(coord.x), float(coord.y)) + 0.5f;
  const f2 inUV = pixelCenter / mk2(float(imageSize.x), float(imageSize.y));
  const f2 d = inUV * 2.0f - 1.0f;
  const f4 origin = mul(cam.viewInverse, mk4(0, 0, 0, 1));
  const f4 target = mul(cam.projInverse, mk4(d.x, d.y, 1, 1));
  const f4 direction = mul(cam.viewInverse, mk4(normalize(xyz(target)), 0));
  return xyz(origin) + xyz(direction) * dist;
}

__device__ constexpr float kGauss[5][5] = {{.0030f, .0133f, .0219f, .0133f, .0030f},
                                {.0133f, .0596f, .0983f, .0596f, .0133f},
                                {.0219f, .0983f, .1621f, .0983f, .0219f},
                                {.0133f, .0596f, .0983f, .0596f, .0133f},
                                {.0030f, .0133f, .0219f, .0133f, .0030f}};  // denoise_common.glsl:15-21

}  // namespace rt

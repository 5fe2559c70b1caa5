// opacity_map.h — THE statement of the opacity micro-map rule (Tri48::omm, bvh8.h), for the host (rt_build_accel, rt_set_instances' templates, rt_opacity_map) and
// for the device (csrc/materials.hip).  No dependency on the context; host and device compile the same expressions.
//
// Cell (i,j), i + j < 8, covers barycentrics u in [i/8,(i+1)/8], v in [j/8,(j+1)/8].  Its texture footprint is the bounding box of the four corners' texcoords,
// widened by the bilinear footprint and one texel of slack for float rounding; the cell is classified only when min/max alpha over that footprint decide HitTest
// (traceray_rq.glsl:86-101) with a safety margin.  Two functions state the rule; between them sits a min/max scan over the footprint's texels: serial on the host
// (ommBuildSerial below), one wave per triangle on the device.
//
// Arithmetic: double, in the order written, under the rule of include/rt_detmath.h (no contraction, no fast-math: both translation units are built with
// -ffp-contract=off).  Every product below is a float times k/8 (exact in double) or a double times an int; the sums round the same way on both targets.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/rt_abi.h"
#include "../../include/rt_detmath.h"

namespace rt {

// the texel box of a cell, inclusive, in unwrapped texel coordinates
struct OmmFootprint { int32_t x0, x1, y0, y1; };

enum : int { OMM_MAX_SPAN = 4096, OMM_MAX_TEXELS = 65536 };

RT_HD int ommWrapTexel(int i, int n, int mode)
{
  if(mode == RT_WRAP_CLAMP) return i < 0 ? 0 : (i >= n ? n - 1 : i);
  if(mode == RT_WRAP_MIRROR) { int p = 2 * n; int m = i % p; if(m < 0) m += p; return m < n ? m : p - 1 - m; }
  int m = i % n; if(m < 0) m += n;
  return m;
}

// Cell footprint.  uv = the triangle's raw texcoords (uv0 uv1 uv2), w x h = the texture (both > 0).  false: the cell stays unknown (state 0) —
//   a corner whose texel coordinate is not finite or not below 2^31 - 4096 in magnitude (the box must fit the int the wrap takes; a NaN texcoord lands here:
//   every corner of every cell carries all three texcoords, one of them with weight 0, and NaN * 0 is NaN),
//   a span of 4096 texels or more in x or y,
//   or more than 65536 texels in the box.
RT_HD bool ommCellFootprint(const float uv[6], int w, int h, int i, int j, OmmFootprint& f)
{
  double fx0 = 1e300, fx1 = -1e300, fy0 = 1e300, fy1 = -1e300;
  for(int c = 0; c < 4; c++) {
    const double u = (i + (c & 1)) / 8.0, v = (j + (c >> 1)) / 8.0, w0 = 1.0 - u - v;
    const double tx = double(uv[0]) * w0 + double(uv[2]) * u + double(uv[4]) * v, ty = double(uv[1]) * w0 + double(uv[3]) * u + double(uv[5]) * v;
    const double px = tx * w, py = ty * h;
    if(!(fabs(px) < 2147479552.0) || !(fabs(py) < 2147479552.0)) return false;
    fx0 = px < fx0 ? px : fx0; fx1 = fx1 < px ? px : fx1; fy0 = py < fy0 ? py : fy0; fy1 = fy1 < py ? py : fy1;
  }
  if(!(fx1 - fx0 < double(OMM_MAX_SPAN) && fy1 - fy0 < double(OMM_MAX_SPAN))) return false;
  const long long x0 = (long long)floor(fx0 - 0.5) - 1, x1 = (long long)floor(fx1 - 0.5) + 2;
  const long long y0 = (long long)floor(fy0 - 0.5) - 1, y1 = (long long)floor(fy1 - 0.5) + 2;
  if((x1 - x0 + 1) * (y1 - y0 + 1) > (long long)OMM_MAX_TEXELS) return false;
  f.x0 = int32_t(x0); f.x1 = int32_t(x1); f.y0 = int32_t(y0); f.y1 = int32_t(y1);
  return true;
}

// Cell state from the alpha bytes' minimum and maximum over the footprint (no texture: lo = hi = 255): 0 unknown, 1 HitTest accepts everywhere, 2 opacity 0 everywhere.
RT_HD uint32_t ommCellState(int lo, int hi, float baseAlpha, float cutoff, int alphaMode)
{
  const double amin = lo / 255.0, amax = hi / 255.0;
  const double omin = double(baseAlpha) * amin, omax = double(baseAlpha) * amax;
  if(!(baseAlpha >= 0.f)) return 0u;
  if(alphaMode == RT_ALPHA_MASK) {
    if(omin > double(cutoff) + 1e-4) return 1u;        // opacity 1 everywhere: rand > 1 never
    if(omax < double(cutoff) - 1e-4) return 2u;        // opacity 0 everywhere
  } else {
    if(omin >= 1.0 + 1e-4) return 1u;                  // blend: rand in [0,1) never exceeds opacity >= 1
    if(omax <= 0.0) return 2u;                         // exactly zero alpha
  }
  return 0u;
}

// cell (i,j) sits in bits 2 (cell & 15) of word cell >> 4, cell = 8 j + i
RT_HD void ommPutCell(uint32_t omm[4], int i, int j, uint32_t state)
{
  const int cell = j * 8 + i;
  omm[cell >> 4] |= state << ((cell & 15) * 2);
}

// The host's map of one triangle: the serial scan between the two functions.  alpha: the first alpha byte of a w x h texture whose texels are `stride` bytes
// apart (1: an alpha plane, 4: byte 3 of BGRA8 texels), or nullptr for no texture.
inline void ommBuildSerial(const float uv[6], float baseAlpha, float cutoff, int alphaMode, int w, int h, int wrapS, int wrapT, const uint8_t* alpha, size_t stride,
                           uint32_t omm[4])
{
  omm[0] = omm[1] = omm[2] = omm[3] = 0;
  for(int j = 0; j < 8; j++)
    for(int i = 0; i + j < 8; i++) {
      int lo = 255, hi = 255;
      if(alpha && w > 0 && h > 0) {
        OmmFootprint f;
        if(!ommCellFootprint(uv, w, h, i, j, f)) continue;   // unknown
        lo = 255; hi = 0;
        for(int y = f.y0; y <= f.y1; y++) {
          const size_t row = size_t(ommWrapTexel(y, h, wrapT)) * size_t(w);
          for(int x = f.x0; x <= f.x1; x++) {
            const int t = alpha[(row + size_t(ommWrapTexel(x, w, wrapS))) * stride];
            lo = t < lo ? t : lo; hi = t > hi ? t : hi;
          }
        }
      }
      ommPutCell(omm, i, j, ommCellState(lo, hi, baseAlpha, cutoff, alphaMode));
    }
}
}  // namespace rt

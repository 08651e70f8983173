// The per-pixel arithmetic of the detail lift's apply stage (lift.apply_reference), shared by ce_lift_apply_u8 (csrc/ce_lift.hip: a whole
// contiguous frame) and ce_boxlift_apply_paste_u8 (csrc/ce_boxlift.hip: a box of a larger canvas).  Every fp32 multiply, add and subtract
// is rounded on its own: each function switches contraction off for its own body, whatever its caller does.
#pragma once
#include "ce_common.h"

#define LF_CELL 8       // floats per coefficient cell: abar_rgb, bbar_rgb, g, 0

struct LaCell {
  float v[7];  // abar_rgb, bbar_rgb, g
};

__device__ __forceinline__ LaCell la_load(const float* __restrict__ coef, int y, int x, int W) {
  const float4* p = (const float4*)(coef + ((size_t)y * W + x) * LF_CELL);
  const float4 lo = p[0], hi = p[1];
  LaCell c;
  c.v[0] = lo.x, c.v[1] = lo.y, c.v[2] = lo.z, c.v[3] = lo.w, c.v[4] = hi.x, c.v[5] = hi.y, c.v[6] = hi.z;
  return c;
}

// The seven values of a pixel from its four corner cells: a * (1 - t) + b * t in the order of ce_preview_rgb_u8, along x, then along y;
// sx = 1 - tx and sy = 1 - ty are formed once per pixel and axis by the caller.
__device__ __forceinline__ void la_sample(const LaCell& c00, const LaCell& c01, const LaCell& c10, const LaCell& c11, float tx, float sx, float ty,
                                          float sy, float (&v)[7]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const float tl = c00.v[k] * sx, tr = c01.v[k] * tx;
    const float bl = c10.v[k] * sx, br = c11.v[k] * tx;
    const float top = tl + tr, bot = bl + br;
    const float l = top * sy, r = bot * ty;
    v[k] = l + r;
  }
}

// q = p + (a p + b): the photo's byte and its change
__device__ __forceinline__ float la_affine(float a, float b, float p) {
#pragma clang fp contract(off)
  const float m = a * p;
  const float e = m + b;
  return p + e;
}

// q + g (u - q): the fallback to the upsampled byte
__device__ __forceinline__ float la_fallback(float q, float g, float u) {
#pragma clang fp contract(off)
  const float d = u - q;
  const float m = g * d;
  return q + m;
}

// rint(clamp(q, 0, 255)), NaN -> 0  (fmaxf(NaN, 0) = 0)
__device__ __forceinline__ uint32_t la_byte(float q) { return (uint32_t)rintf(fminf(fmaxf(q, 0.0f), 255.0f)); }

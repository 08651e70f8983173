// Guided detail lift inside a focus box (chronoedit_amd/boxlift.py is the definition): stage 4 of the lift (csrc/ce_lift.hip) fused with the
// paste of the focused edit (csrc/ce_focus.hip, csrc/ce_clusters.hip).  The crop of a focused edit is lifted onto the photo's own bytes and
// goes straight through the photo-size mask into the canvas, IN PLACE; the lifted box is never written out, and nothing is computed for a
// pixel the mask leaves alone.
//
//   ce_boxlift_apply_paste_u8   P (the photo the crop was cut from), U (the frames' Lanczos upsample to the box, or NULL), the cells and
//                               the axis tables of the box, the mask (or NULL) -> canvas uint8 [F][src_h][src_w][3]
//
// The per-pixel arithmetic is ce_lift_apply_u8's (csrc/ce_lift_pixel.h), the blend ce_focus_paste_u8's (csrc/ce_common.h).
//
// One lane per run of up to BL_RUN consecutive pixels of one row of the box (blockIdx.y = frame), as in csrc/ce_layers.hip: the rows of a
// box start at any byte address, so lane 0 of a row takes its `head` - the 0..3 pixels in front of the row's first pixel at which the
// canvas allows dword access - and lane j >= 1 the BL_RUN pixels from head + BL_RUN (j - 1), the last of them the rest.  A whole run at such
// an address moves as dwords wherever the plane in question (canvas, P, U, mask: four different phases) is aligned there; heads,
// remainders and planes at odd phases move byte by byte.  The same bytes either way.  A pixel belongs to exactly one lane, which reads and
// writes its own canvas bytes: no order matters.  The lane reads its mask bytes first and leaves when all are 0 - a wave whose 64 runs lie
// outside the mask has left before a table entry or a corner cell is loaded.
#include "ce_common.h"
#include "ce_lift_pixel.h"

#define BL_RUN 8             // pixels per lane: 24 bytes, six dwords (a multiple of four pixels keeps every run at the head's phase)
#define BL_B (3 * BL_RUN)
#define BL_DW (BL_B / 4)

// nb <= BL_B bytes at p as dwords: whole dwords when nb == BL_B and p is 4-byte aligned, single bytes otherwise
__device__ __forceinline__ void bl_read(const uint8_t* __restrict__ p, int nb, uint32_t (&w)[BL_DW]) {
  if (nb == BL_B && !((uintptr_t)p & 3)) {
#pragma unroll
    for (int k = 0; k < BL_DW; ++k) w[k] = ((const uint32_t*)p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < BL_DW; ++k) w[k] = 0;
#pragma unroll
    for (int j = 0; j < BL_B; ++j)
      if (j < nb) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
  }
}

__global__ __launch_bounds__(256) void boxlift_apply_paste_kernel(const uint8_t* __restrict__ P, const uint8_t* __restrict__ U, const float* __restrict__ coef,
                                                                  const int* __restrict__ ix0, const int* __restrict__ ix1, const float* __restrict__ txs,
                                                                  const int* __restrict__ iy0, const int* __restrict__ iy1, const float* __restrict__ tys,
                                                                  const uint8_t* __restrict__ mask, uint8_t* canvas, int src_h, int src_w, int left, int top,
                                                                  int bw, int bh, int H, int W, int lpr) {
#pragma clang fp contract(off)
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= (long long)bh * lpr) return;
  const int y = (int)(k / lpr), j = (int)(k - (long long)y * lpr);
  const int f = blockIdx.y;
  uint8_t* cv = canvas + (size_t)f * src_h * src_w * 3;
  const unsigned long long P0 = (unsigned long long)(top + y) * src_w + left;  // the row's first pixel in the photo
  // cv + 3 p is 4-byte aligned <=> p % 4 == cv % 4 (3 * 3 = 9 = 1 mod 4)
  const int head = (int)((((unsigned long long)(uintptr_t)cv & 3ull) - P0) & 3ull);
  const int x0 = j == 0 ? 0 : head + BL_RUN * (j - 1);
  const int np = j == 0 ? min(head, bw) : min(BL_RUN, bw - x0);
  if (np <= 0) return;
  const int nb = 3 * np;
  // the mask first: a run under m == 0 everywhere is left as it is, before anything else is read
  uint32_t m[BL_RUN];
#pragma unroll
  for (int i = 0; i < BL_RUN; ++i) m[i] = 255u;
  if (mask) {
    const uint8_t* mp = mask + P0 + x0;
    uint32_t any_m = 0;
    if (np == BL_RUN && !((uintptr_t)mp & 3)) {
#pragma unroll
      for (int d = 0; d < BL_RUN / 4; ++d) {
        const uint32_t w = ((const uint32_t*)mp)[d];
        any_m |= w;
#pragma unroll
        for (int b = 0; b < 4; ++b) m[4 * d + b] = (w >> (8 * b)) & 255u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < BL_RUN; ++i) {
        m[i] = i < np ? (uint32_t)mp[i] : 0u;
        any_m |= m[i];
      }
    }
    if (!any_m) return;
  }
  // the row of the grid: the same two cell rows and weight for the whole run
  const float* cf = coef + (size_t)f * H * W * LF_CELL;
  const int ya = min(max(iy0[y], 0), H - 1), yb = min(max(iy1[y], 0), H - 1);
  const float ty = tys[y], sy = 1.0f - ty;
  uint32_t pw[BL_DW];
  bl_read(P + (size_t)(P0 + x0) * 3, nb, pw);
  // The corner cells stay in registers from pixel to pixel, as in ce_lift_apply_u8: a step of one cell reuses the right pair as the left one.
  int xa = -1, xb = -1;
  LaCell c00, c01, c10, c11;
  float q[BL_B], gq[BL_RUN];
  bool any_g = false;
#pragma unroll
  for (int i = 0; i < BL_RUN; ++i) {
    float v[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (i < np && m[i]) {  // (a pixel under m == 0 keeps its canvas bytes whatever q is: nothing is computed for it)
      const int X = x0 + i;
      const int nxa = min(max(ix0[X], 0), W - 1), nxb = min(max(ix1[X], 0), W - 1);
      const float tx = txs[X];
      if (nxa != xa || nxb != xb) {
        if (nxa == xb && xb >= 0) {
          c00 = c01, c10 = c11;
        } else if (nxa != xa) {
          c00 = la_load(cf, ya, nxa, W), c10 = la_load(cf, yb, nxa, W);
        }
        if (nxb == nxa) {
          c01 = c00, c11 = c10;
        } else {
          c01 = la_load(cf, ya, nxb, W), c11 = la_load(cf, yb, nxb, W);
        }
        xa = nxa, xb = nxb;
      }
      const float sx = 1.0f - tx;
      la_sample(c00, c01, c10, c11, tx, sx, ty, sy, v);
      any_g = any_g || v[6] != 0.0f;
    }
    gq[i] = v[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int b = 3 * i + c;
      const float p = (float)((pw[b >> 2] >> (8 * (b & 3))) & 255u);
      q[b] = la_affine(v[c], v[3 + c], p);
    }
  }
  if (U && any_g) {  // (g_up == 0 leaves q as it is: q + 0 * (U - q); U is read by a run that holds a pixel with g_up != 0)
    uint32_t uw[BL_DW];
    bl_read(U + (((size_t)f * bh + y) * bw + x0) * 3, nb, uw);
#pragma unroll
    for (int b = 0; b < BL_B; ++b) q[b] = la_fallback(q[b], gq[b / 3], (float)((uw[b >> 2] >> (8 * (b & 3))) & 255u));
  }
  uint8_t* d = cv + (size_t)(P0 + x0) * 3;
  if (np == BL_RUN) {  // (j >= 1: d is 4-byte aligned by the choice of head)
    uint32_t* dw = (uint32_t*)d;
    uint32_t cw[BL_DW], ow[BL_DW];
#pragma unroll
    for (int w = 0; w < BL_DW; ++w) cw[w] = dw[w], ow[w] = 0;
#pragma unroll
    for (int b = 0; b < BL_B; ++b) {
      const uint32_t old = (cw[b >> 2] >> (8 * (b & 3))) & 255u;
      ow[b >> 2] |= focus_blend8(old, la_byte(q[b]), m[b / 3]) << (8 * (b & 3));  // (m == 0: the old byte, exactly)
    }
#pragma unroll
    for (int w = 0; w < BL_DW; ++w) dw[w] = ow[w];
  } else {
#pragma unroll
    for (int b = 0; b < BL_B; ++b)
      if (b < nb && m[b / 3]) d[b] = (uint8_t)focus_blend8(d[b], la_byte(q[b]), m[b / 3]);
  }
}

// do [a, a + na) and [b, b + nb) share a byte?
static bool boxlift_overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

CE_API int ce_boxlift_apply_paste_u8(const void* P, const void* U, const float* coef, const int* ix0, const int* ix1, const float* tx, const int* iy0,
                                     const int* iy1, const float* ty, const void* mask, void* canvas, int F, int src_h, int src_w, int left, int top,
                                     int bw, int bh, int H, int W, hipStream_t stream) {
  if (!P || !coef || !ix0 || !ix1 || !tx || !iy0 || !iy1 || !ty || !canvas) return CE_ERR_ARG;
  if (F <= 0 || F > 65535 || src_h <= 0 || src_w <= 0 || bw <= 0 || bh <= 0 || H <= 0 || W <= 0) return CE_ERR_ARG;
  if (left < 0 || top < 0 || (long long)left + bw > src_w || (long long)top + bh > src_h) return CE_ERR_ARG;  // the box lies inside the image
  const long long plane = (long long)src_h * src_w;
  if (plane * 3 >= (1ll << 31) || (long long)H * W * LF_CELL * (long long)sizeof(float) >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)coef & 15) || (((uintptr_t)ix0 | (uintptr_t)ix1 | (uintptr_t)tx | (uintptr_t)iy0 | (uintptr_t)iy1 | (uintptr_t)ty) & 3)) return CE_ERR_ALIGN;
  // the pass works in place on the canvas while other lanes still read P, U and the mask: they share no byte with it
  const unsigned long long cbytes = (unsigned long long)F * plane * 3;
  if (boxlift_overlap(canvas, cbytes, P, (unsigned long long)plane * 3)) return CE_ERR_ARG;
  if (U && boxlift_overlap(canvas, cbytes, U, (unsigned long long)F * bh * bw * 3)) return CE_ERR_ARG;
  if (mask && boxlift_overlap(canvas, cbytes, mask, (unsigned long long)plane)) return CE_ERR_ARG;
  const int lpr = bw / BL_RUN + 2;  // the head, then at most ceil(bw / BL_RUN) runs
  const long long lanes = (long long)bh * lpr;
  hipLaunchKernelGGL(boxlift_apply_paste_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)F), dim3(256), 0, stream, (const uint8_t*)P,
                     (const uint8_t*)U, coef, ix0, ix1, tx, iy0, iy1, ty, (const uint8_t*)mask, (uint8_t*)canvas, src_h, src_w, left, top, bw, bh, H, W, lpr);
  return (int)hipGetLastError();
}

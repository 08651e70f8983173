// Sketch edits from an image editor's layers (chronoedit_amd/layers.py is the definition; both passes give its bits).  A layer is RGBA and its
// alpha is non-zero only under the brush; it reaches the device as its alpha bounding box only: uint8 [bh][bw][4], placed at (left, top) of
// the photo.  Both passes work IN PLACE inside that box and touch no byte outside it:
//
//   ce_layers_strokes_u8   plane [SH][SW]: 255 where the layer's alpha > threshold, every other byte left as it is (the caller zeroes the
//                          plane once; the layers of a value are OR-ed into it, in any order)
//   ce_layers_over_u8      canvas [SH][SW][3]: Image.alpha_composite of the layer over the opaque canvas, per channel
//                          focus_blend8(canvas, layer, alpha) - the arithmetic of ce_focus_paste_u8 (ce_common.h)
//
// One lane per run of up to four consecutive pixels of one row of the box.  Lane 0 of a row takes its `head`: the 0..3 pixels in front of the
// row's first pixel whose address allows the wide access; lane j >= 1 takes the four pixels from head + 4 (j - 1), the last of them the rest.
// A run of four at such an address moves as whole words (strokes: the layer's four pixels as one 16-byte load; over: the canvas's 12 bytes
// as three dwords, the layer's as one 16-byte load or four dwords); every other run - heads, remainders, bases at odd addresses - moves
// byte by byte.  The same bytes either way.  A pixel belongs to exactly one lane, which reads and writes its own addresses: no order matters.
#include "ce_common.h"

// The run of lane j in a row of bw pixels whose first `head` pixels stand alone -> its first pixel, and how many (<= 0: none).
__device__ __forceinline__ int layers_run(int j, int head, int bw, int& x0) {
  if (j == 0) {
    x0 = 0;
    return min(head, bw);
  }
  x0 = head + 4 * (j - 1);
  return min(4, bw - x0);
}

// n <= 4 pixels at s -> px[i] = r | g << 8 | b << 16 | a << 24
__device__ __forceinline__ void layers_load(const uint8_t* s, int n, uint32_t* px) {
  if (n == 4 && !((uintptr_t)s & 15)) {
    const uint4 v = *(const uint4*)s;
    px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
  } else if (!((uintptr_t)s & 3)) {
    for (int i = 0; i < n; ++i) px[i] = *(const uint32_t*)(s + 4 * i);
  } else {
    for (int i = 0; i < n; ++i) px[i] = (uint32_t)s[4 * i] | (uint32_t)s[4 * i + 1] << 8 | (uint32_t)s[4 * i + 2] << 16 | (uint32_t)s[4 * i + 3] << 24;
  }
}

// lpr = bw / 4 + 2 lanes per row: the head, then at most ceil(bw / 4) runs of four
__global__ __launch_bounds__(256) void layers_strokes_kernel(const uint8_t* __restrict__ layer, uint8_t* __restrict__ plane, int bw, int bh, int left, int top,
                                                             int SW, int lpr, uint32_t threshold) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= (long long)bh * lpr) return;
  const int y = (int)(k / lpr), j = (int)(k - (long long)y * lpr);
  const unsigned long long p0 = (unsigned long long)y * bw;  // the row's first pixel in the layer
  // layer + 4 p is 16-byte aligned <=> (layer / 4 + p) % 4 == 0, for a 4-byte aligned layer; otherwise no run is wide
  const uintptr_t a = (uintptr_t)layer;
  const int head = (a & 3) ? 0 : (int)((0ull - (unsigned long long)(a >> 2) - p0) & 3ull);
  int x0;
  const int n = layers_run(j, head, bw, x0);
  if (n <= 0) return;
  uint32_t px[4] = {0, 0, 0, 0};
  layers_load(layer + (size_t)(p0 + x0) * 4, n, px);
  uint8_t* d = plane + (size_t)(top + y) * SW + left + x0;
  for (int i = 0; i < n; ++i)
    if ((px[i] >> 24) > threshold) d[i] = 255;
}

__global__ __launch_bounds__(256) void layers_over_kernel(const uint8_t* __restrict__ layer, uint8_t* __restrict__ canvas, int bw, int bh, int left, int top,
                                                          int SW, int lpr) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= (long long)bh * lpr) return;
  const int y = (int)(k / lpr), j = (int)(k - (long long)y * lpr);
  const unsigned long long P0 = (unsigned long long)(top + y) * SW + left;  // the row's first pixel in the canvas
  // canvas + 3 P is 4-byte aligned <=> P % 4 == canvas % 4 (3 * 3 = 9 = 1 mod 4): a run of four pixels from there is three aligned dwords
  const int head = (int)((((unsigned long long)(uintptr_t)canvas & 3ull) - P0) & 3ull);
  int x0;
  const int n = layers_run(j, head, bw, x0);
  if (n <= 0) return;
  uint32_t px[4] = {0, 0, 0, 0};
  layers_load(layer + ((size_t)y * bw + x0) * 4, n, px);
  if (!((px[0] | px[1] | px[2] | px[3]) >> 24)) return;  // alpha 0 everywhere: the canvas stays
  uint8_t* d = canvas + (size_t)(P0 + x0) * 3;
  if (n == 4) {  // (d is 4-byte aligned by the choice of head)
    uint32_t* dw = (uint32_t*)d;
    const uint32_t w[3] = {dw[0], dw[1], dw[2]};
    uint32_t o[3] = {0, 0, 0};
#pragma unroll
    for (int b = 0; b < 12; ++b) {  // byte b of the run: pixel b / 3, channel b % 3
      const uint32_t p = px[b / 3];
      const uint32_t old = (w[b >> 2] >> (8 * (b & 3))) & 255u;
      o[b >> 2] |= focus_blend8(old, (p >> (8 * (b % 3))) & 255u, p >> 24) << (8 * (b & 3));
    }
    dw[0] = o[0], dw[1] = o[1], dw[2] = o[2];
  } else {
    for (int i = 0; i < n; ++i) {
      const uint32_t p = px[i], m = p >> 24;
      if (!m) continue;
      for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint8_t)focus_blend8(d[3 * i + c], (p >> (8 * c)) & 255u, m);
    }
  }
}

static int layers_check(const void* layer, const void* image, int bw, int bh, int left, int top, int SW, int SH, int bytes_per_pixel) {
  if (!layer || !image) return CE_ERR_ARG;
  if (SW <= 0 || SH <= 0 || bw <= 0 || bh <= 0) return CE_ERR_ARG;
  if (left < 0 || top < 0 || (long long)left + bw > SW || (long long)top + bh > SH) return CE_ERR_ARG;  // the box lies inside the photo
  if ((long long)SH * SW * bytes_per_pixel >= (1ll << 31) || (long long)bh * bw * 4 >= (1ll << 31)) return CE_ERR_SHAPE;
  // the layer's bytes and the image's share none: the passes work in place on the image while other lanes still read the layer
  const uintptr_t l0 = (uintptr_t)layer, l1 = l0 + (uintptr_t)bh * bw * 4, i0 = (uintptr_t)image, i1 = i0 + (uintptr_t)SH * SW * bytes_per_pixel;
  if (l0 < i1 && i0 < l1) return CE_ERR_ARG;
  return CE_OK;
}

CE_API int ce_layers_strokes_u8(const void* layer, int bw, int bh, int left, int top, void* plane, int SW, int SH, int threshold, hipStream_t stream) {
  const int rc = layers_check(layer, plane, bw, bh, left, top, SW, SH, 1);
  if (rc != CE_OK) return rc;
  if (threshold < 0 || threshold > 254) return CE_ERR_ARG;
  const int lpr = bw / 4 + 2;
  const long long lanes = (long long)bh * lpr;
  hipLaunchKernelGGL(layers_strokes_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)layer, (uint8_t*)plane, bw, bh, left,
                     top, SW, lpr, (uint32_t)threshold);
  return (int)hipGetLastError();
}

CE_API int ce_layers_over_u8(const void* layer, int bw, int bh, int left, int top, void* canvas, int SW, int SH, hipStream_t stream) {
  const int rc = layers_check(layer, canvas, bw, bh, left, top, SW, SH, 3);
  if (rc != CE_OK) return rc;
  const int lpr = bw / 4 + 2;
  const long long lanes = (long long)bh * lpr;
  hipLaunchKernelGGL(layers_over_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)layer, (uint8_t*)canvas, bw, bh, left, top,
                     SW, lpr);
  return (int)hipGetLastError();
}

// Focused region edits (chronoedit_amd/focus.py): the edit sees a crop of the photo around the mask, and its frames are pasted back into the
// photo at the photo's own resolution.  The two byte passes the existing ones (ce_image.hip) do not cover:
//
//   ce_focus_resample_l8   one 1-D pass of PIL's 8-bit resampler over SINGLE-channel bytes whose rows lie `pitch` bytes apart: a crop of the
//                          source-size mask is resampled where it lies.  Tables and arithmetic are ce_image_resample_u8's.
//   ce_focus_paste_u8      Image.paste(edit, (left, top), mask) into a copy of the photo, for F frames at once:
//                          t = s * (255 - m) + e * m + 128, out = ((t >> 8) + t) >> 8 inside the box, out = s outside.
//
// Conventions of ce_image.hip: integer-exact, lanes own four consecutive output bytes, aligned dword accesses when the row geometry keeps
// them aligned (a launch-uniform flag), byte by byte otherwise.
#include "ce_common.h"

// Horizontal pass: src rows of in_w bytes, `pitch` apart -> dst [H][out_w].  The taps of an output byte are count consecutive source bytes.
// WIDE (out_w % 4 == 0, dst 4-byte aligned): the four bytes lie in one row and leave as one dword.
template <bool WIDE>
__global__ __launch_bounds__(256) void focus_resample_h_kernel(const uint8_t* __restrict__ src, long long pitch, uint8_t* __restrict__ dst, int H, int in_w,
                                                               int out_w, const int* __restrict__ coeff, const int* __restrict__ bounds, int ksize) {
  const long long n = (long long)H * out_w;
  const long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= n) return;
  uint32_t o[4] = {0, 0, 0, 0};
  const int nb = (int)(n - b0 < 4 ? n - b0 : 4);
  for (int j = 0; j < nb; ++j) {
    const long long b = b0 + j;
    const int y = (int)(b / out_w), x = (int)(b - (long long)y * out_w);
    int first = bounds[2 * x], count = bounds[2 * x + 1];
    first = min(max(first, 0), in_w);
    count = min(min(count, ksize), in_w - first);  // a window never leaves the row, whatever the table says
    const int* k = coeff + (size_t)x * ksize;
    const uint8_t* s = src + (size_t)y * pitch + first;
    int ss = 1 << (CE_RESAMPLE_BITS - 1);
    for (int t = 0; t < count; ++t) ss += k[t] * (int)s[t];
    o[j] = resample_clip8(ss);
  }
  if (WIDE) {  // (nb == 4 on this path)
    *(uint32_t*)(dst + b0) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
  } else {
    for (int j = 0; j < nb; ++j) dst[b0 + j] = (uint8_t)o[j];
  }
}

// Vertical pass: src [in_h] rows of W bytes, `pitch` apart -> dst [out_h][W].  The taps of four consecutive output bytes are the same four
// bytes of count consecutive source rows.  WIDE (W % 4 == 0, pitch % 4 == 0, both bases 4-byte aligned): every access is one aligned dword.
template <bool WIDE>
__global__ __launch_bounds__(256) void focus_resample_v_kernel(const uint8_t* __restrict__ src, long long pitch, uint8_t* __restrict__ dst, int in_h, int out_h,
                                                               int W, const int* __restrict__ coeff, const int* __restrict__ bounds, int ksize) {
  const long long n = (long long)out_h * W;
  const long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= n) return;
  if (WIDE) {
    const int y = (int)(b0 / W), x = (int)(b0 - (long long)y * W);
    int first = bounds[2 * y], count = bounds[2 * y + 1];
    first = min(max(first, 0), in_h);
    count = min(min(count, ksize), in_h - first);
    const int* k = coeff + (size_t)y * ksize;
    const uint8_t* s = src + (size_t)first * pitch + x;
    int s0 = 1 << (CE_RESAMPLE_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
    for (int t = 0; t < count; ++t) {
      const int c = k[t];
      const uint32_t v = *(const uint32_t*)(s + (size_t)t * pitch);
      s0 += c * (int)(v & 255u);
      s1 += c * (int)((v >> 8) & 255u);
      s2 += c * (int)((v >> 16) & 255u);
      s3 += c * (int)(v >> 24);
    }
    *(uint32_t*)(dst + b0) = resample_clip8(s0) | resample_clip8(s1) << 8 | resample_clip8(s2) << 16 | resample_clip8(s3) << 24;
  } else {
    for (int j = 0; j < 4 && b0 + j < n; ++j) {
      const long long b = b0 + j;
      const int y = (int)(b / W), x = (int)(b - (long long)y * W);
      int first = bounds[2 * y], count = bounds[2 * y + 1];
      first = min(max(first, 0), in_h);
      count = min(min(count, ksize), in_h - first);
      const int* k = coeff + (size_t)y * ksize;
      const uint8_t* s = src + (size_t)first * pitch + x;
      int ss = 1 << (CE_RESAMPLE_BITS - 1);
      for (int t = 0; t < count; ++t) ss += k[t] * (int)s[(size_t)t * pitch];
      dst[b] = (uint8_t)resample_clip8(ss);
    }
  }
}

CE_API int ce_focus_resample_l8(const void* src, long long src_pitch, void* dst, int axis, int src_h, int src_w, int out_len, const int* coeff,
                                const int* bounds, int ksize, hipStream_t stream) {
  if (!src || !dst || !coeff || !bounds || src == dst) return CE_ERR_ARG;
  if (axis < 0 || axis > 1 || src_h <= 0 || src_w <= 0 || out_len <= 0 || ksize <= 0 || src_pitch < src_w) return CE_ERR_ARG;
  if ((long long)src_h * src_pitch >= (1ll << 31) || (long long)out_len * (axis ? src_w : src_h) >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)coeff | (uintptr_t)bounds) & 3) return CE_ERR_ALIGN;
  const long long groups = ((long long)out_len * (axis ? src_w : src_h) + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (axis == 0) {  // horizontal
    if (out_len % 4 == 0 && !((uintptr_t)dst & 3))
      hipLaunchKernelGGL(focus_resample_h_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)src, src_pitch, (uint8_t*)dst, src_h, src_w, out_len, coeff, bounds, ksize);
    else
      hipLaunchKernelGGL(focus_resample_h_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)src, src_pitch, (uint8_t*)dst, src_h, src_w, out_len, coeff, bounds, ksize);
  } else {
    if (src_w % 4 == 0 && src_pitch % 4 == 0 && !(((uintptr_t)src | (uintptr_t)dst) & 3))
      hipLaunchKernelGGL(focus_resample_v_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)src, src_pitch, (uint8_t*)dst, src_h, out_len, src_w, coeff, bounds, ksize);
    else
      hipLaunchKernelGGL(focus_resample_v_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)src, src_pitch, (uint8_t*)dst, src_h, out_len, src_w, coeff, bounds, ksize);
  }
  return (int)hipGetLastError();
}

// One lane per four consecutive bytes of one output frame (blockIdx.y = frame).  The group's first byte is split into (Y, X, channel) once
// and the other three follow by counting.  A byte outside the box, or under a mask byte of 0, is the source's and reads nothing else.
// WIDE (frame bytes % 4 == 0, src and out 4-byte aligned): the source group arrives and the result leaves as one dword.
template <bool WIDE>
__global__ __launch_bounds__(256) void focus_paste_kernel(const uint8_t* __restrict__ edit, const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask,
                                                          uint8_t* __restrict__ out, int SW, long long n, int left, int top, int bw, int bh) {
  const long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= n) return;
  const int f = blockIdx.y;
  const int nb = (int)(n - b0 < 4 ? n - b0 : 4);
  uint32_t o[4] = {0, 0, 0, 0};
  if (WIDE) {  // (nb == 4 on this path)
    const uint32_t v = *(const uint32_t*)(src + b0);
    o[0] = v & 255u, o[1] = (v >> 8) & 255u, o[2] = (v >> 16) & 255u, o[3] = v >> 24;
  } else {
    for (int j = 0; j < nb; ++j) o[j] = src[b0 + j];
  }
  const long long px = b0 / 3;
  int c = (int)(b0 - px * 3), Y = (int)(px / SW), X = (int)(px - (long long)Y * SW);
  const uint8_t* e = edit + (size_t)f * bh * bw * 3;
  for (int j = 0; j < nb; ++j) {
    const int y = Y - top, x = X - left;
    if (y >= 0 && y < bh && x >= 0 && x < bw) {
      const uint32_t m = mask ? (uint32_t)mask[(size_t)Y * SW + X] : 255u;
      if (m) o[j] = focus_blend8(o[j], e[((size_t)y * bw + x) * 3 + c], m);
    }
    if (++c == 3) {
      c = 0;
      if (++X == SW) X = 0, ++Y;
    }
  }
  uint8_t* d = out + (size_t)f * n + b0;
  if (WIDE) {
    *(uint32_t*)d = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
  } else {
    for (int j = 0; j < nb; ++j) d[j] = (uint8_t)o[j];
  }
}

CE_API int ce_focus_paste_u8(const void* edit, const void* src, const void* mask, void* out, int F, int src_h, int src_w, int left, int top,
                             int bw, int bh, hipStream_t stream) {
  if (!edit || !src || !out || out == edit || out == src || out == mask) return CE_ERR_ARG;
  if (F <= 0 || F > 65535 || src_h <= 0 || src_w <= 0 || bw <= 0 || bh <= 0) return CE_ERR_ARG;
  if (left < 0 || top < 0 || (long long)left + bw > src_w || (long long)top + bh > src_h) return CE_ERR_ARG;  // the box lies inside the image
  const long long n = (long long)src_h * src_w * 3;
  if (n >= (1ll << 31)) return CE_ERR_SHAPE;
  const long long groups = (n + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)F);
  if (n % 4 == 0 && !(((uintptr_t)src | (uintptr_t)out) & 3))
    hipLaunchKernelGGL(focus_paste_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)edit, (const uint8_t*)src, (const uint8_t*)mask, (uint8_t*)out,
                       src_w, n, left, top, bw, bh);
  else
    hipLaunchKernelGGL(focus_paste_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)edit, (const uint8_t*)src, (const uint8_t*)mask, (uint8_t*)out,
                       src_w, n, left, top, bw, bh);
  return (int)hipGetLastError();
}

// Image pre- and post-processing around the edit (chronoedit_amd/image_io.py): the byte passes that ran inside PIL and numpy on one host
// core - VideoProcessor.preprocess / CLIPImageProcessor in front of the encoders, VideoProcessor.postprocess_video behind the VAE.
//
//   ce_image_resample_u8     one 1-D pass of PIL's 8-bit resampler (Resample.c, ImagingResampleHorizontal_8bpc / ...Vertical_8bpc) over
//                            interleaved RGB bytes: ss = 2^21 + sum_k coeff[o][k] * src[first + k] in int32, out = clip(ss >> 22, 0, 255).
//                            The 22-bit fixed-point coefficients and the (first, count) windows are PIL's, computed on the host.
//   ce_image_u8_lut_planar   crop + per-channel 256-entry table lookup, interleaved bytes -> planar bf16 / fp32: every host-side
//                            "rescale, normalise, cast" chain is a function of (channel, byte) alone, so the table IS the chain.
//   ce_video_to_u8           [B][3][F][H][W] in [-1, 1] -> uint8 [B][F][H][W][3]: v * 0.5 + 0.5, clamp, * 255, round half to even -
//                            a multiply, an add and a multiply, each rounded on its own (no contraction), as eager torch / numpy do.
//
// All three are integer- or table-exact: the results are the host's bits.  They move a few tens of MB per edit, so the mapping is
// chosen for simplicity at the row tails: lanes own consecutive output bytes, the wide (dword / 16-byte) accesses are taken when the
// row geometry keeps them aligned (a launch-uniform flag) and every other launch runs the byte-wise body.
#include "ce_common.h"

// Horizontal pass: src [H][in_w][3] -> dst [H][out_w][3].  One lane per output pixel (three consecutive output bytes, lanes of a wave
// cover one contiguous run of an output row); its taps are count consecutive source pixels: overlapping windows that the L1 / L2 serve.
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int in_w, int out_w,
                                                         const int* __restrict__ coeff, const int* __restrict__ bounds, int ksize) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)H * out_w) return;
  const int y = (int)(idx / out_w), x = (int)(idx - (long long)y * out_w);
  int first = bounds[2 * x], count = bounds[2 * x + 1];
  first = min(max(first, 0), in_w);
  count = min(min(count, ksize), in_w - first);  // a window never leaves the row, whatever the table says
  const int* k = coeff + (size_t)x * ksize;
  const uint8_t* s = src + ((size_t)y * in_w + first) * 3;
  int s0 = 1 << (CE_RESAMPLE_BITS - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < count; ++t) {
    const int c = k[t];
    s0 += c * (int)s[3 * t];
    s1 += c * (int)s[3 * t + 1];
    s2 += c * (int)s[3 * t + 2];
  }
  uint8_t* d = dst + (size_t)idx * 3;
  d[0] = (uint8_t)resample_clip8(s0);
  d[1] = (uint8_t)resample_clip8(s1);
  d[2] = (uint8_t)resample_clip8(s2);
}

// Vertical pass: src [in_h][W][3] -> dst [out_h][W][3], rb = 3 W bytes per row.  One lane per four consecutive output bytes of the flat
// destination; its taps are the same four bytes of count consecutive source rows: fully coalesced.  WIDE (rb % 4 == 0, both bases
// 4-byte aligned): the four bytes lie in one row and every access is one aligned dword.  Otherwise a group may straddle a row end or
// the end of the image: byte by byte.
template <bool WIDE>
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int in_h, int out_h, int rb,
                                                         const int* __restrict__ coeff, const int* __restrict__ bounds, int ksize) {
  const long long n = (long long)out_h * rb;
  const long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= n) return;
  if (WIDE) {
    const int y = (int)(b0 / rb), xb = (int)(b0 - (long long)y * rb);
    int first = bounds[2 * y], count = bounds[2 * y + 1];
    first = min(max(first, 0), in_h);
    count = min(min(count, ksize), in_h - first);
    const int* k = coeff + (size_t)y * ksize;
    const uint8_t* s = src + (size_t)first * rb + xb;
    int s0 = 1 << (CE_RESAMPLE_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
    for (int t = 0; t < count; ++t) {
      const int c = k[t];
      const uint32_t v = *(const uint32_t*)(s + (size_t)t * rb);
      s0 += c * (int)(v & 255u);
      s1 += c * (int)((v >> 8) & 255u);
      s2 += c * (int)((v >> 16) & 255u);
      s3 += c * (int)(v >> 24);
    }
    *(uint32_t*)(dst + b0) = resample_clip8(s0) | resample_clip8(s1) << 8 | resample_clip8(s2) << 16 | resample_clip8(s3) << 24;
  } else {
    for (int j = 0; j < 4 && b0 + j < n; ++j) {
      const long long b = b0 + j;
      const int y = (int)(b / rb), xb = (int)(b - (long long)y * rb);
      int first = bounds[2 * y], count = bounds[2 * y + 1];
      first = min(max(first, 0), in_h);
      count = min(min(count, ksize), in_h - first);
      const int* k = coeff + (size_t)y * ksize;
      const uint8_t* s = src + (size_t)first * rb + xb;
      int ss = 1 << (CE_RESAMPLE_BITS - 1);
      for (int t = 0; t < count; ++t) ss += k[t] * (int)s[(size_t)t * rb];
      dst[b] = (uint8_t)resample_clip8(ss);
    }
  }
}

CE_API int ce_image_resample_u8(const void* src, void* dst, int axis, int src_h, int src_w, int out_len, const int* coeff, const int* bounds,
                                int ksize, hipStream_t stream) {
  if (!src || !dst || !coeff || !bounds || src == dst) return CE_ERR_ARG;
  if (axis < 0 || axis > 1 || src_h <= 0 || src_w <= 0 || out_len <= 0 || ksize <= 0) return CE_ERR_ARG;
  if ((long long)src_h * src_w * 3 >= (1ll << 31) || (long long)out_len * (axis ? src_w : src_h) * 3 >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)coeff | (uintptr_t)bounds) & 3) return CE_ERR_ALIGN;
  if (axis == 0) {  // horizontal
    const long long px = (long long)src_h * out_len;
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, src_h,
                       src_w, out_len, coeff, bounds, ksize);
  } else {
    const int rb = src_w * 3;
    const long long groups = ((long long)out_len * rb + 3) / 4;
    const dim3 grid((unsigned)((groups + 255) / 256));
    if (rb % 4 == 0 && !(((uintptr_t)src | (uintptr_t)dst) & 3))
      hipLaunchKernelGGL(resample_v_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, src_h, out_len, rb, coeff, bounds, ksize);
    else
      hipLaunchKernelGGL(resample_v_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, src_h, out_len, rb, coeff, bounds, ksize);
  }
  return (int)hipGetLastError();
}

// Crop + lookup: dst[c][y][x] = lut[c][src[top + y][left + x][c]].  T = the destination element as raw bits (uint16_t: bf16, uint32_t: fp32);
// the 3 x 256 table lives in LDS.  One lane per four consecutive pixels of an output row (12 source bytes, four elements per plane).
// WIDE_IN: the 12 bytes are three aligned dwords; WIDE_OUT (out_w % 4 == 0, dst 16-byte aligned): one vector store per plane.
template <typename T, bool WIDE_IN, bool WIDE_OUT>
__global__ __launch_bounds__(256) void lut_planar_kernel(const uint8_t* __restrict__ src, int src_w, int top, int left, int out_h, int out_w,
                                                         const T* __restrict__ lut, T* __restrict__ dst) {
  __shared__ T tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = lut[i];
  __syncthreads();
  const int gpr = (out_w + 3) >> 2;  // groups per row
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)out_h * gpr) return;
  const int y = (int)(g / gpr), x = (int)(g - (long long)y * gpr) * 4;
  const uint8_t* s = src + ((size_t)(top + y) * src_w + left + x) * 3;
  const int npx = min(4, out_w - x);
  uint8_t px[12];
  if (WIDE_IN) {  // (npx == 4 on this path: WIDE_IN is taken only together with out_w % 4 == 0)
    const uint32_t* s4 = (const uint32_t*)s;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const uint32_t v = s4[i];
      px[4 * i] = v & 255u, px[4 * i + 1] = (v >> 8) & 255u, px[4 * i + 2] = (v >> 16) & 255u, px[4 * i + 3] = v >> 24;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) px[i] = i < 3 * npx ? s[i] : (uint8_t)0;
  }
  const size_t plane = (size_t)out_h * out_w;
  T* d = dst + (size_t)y * out_w + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = tab[c * 256 + px[3 * i + c]];
    if (WIDE_OUT) {
      if constexpr (sizeof(T) == 2) {
        u32x2 o = {(uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16};
        *(u32x2*)(d + c * plane) = o;
      } else {
        u32x4 o = {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]};
        *(u32x4*)(d + c * plane) = o;
      }
    } else {
      for (int i = 0; i < npx; ++i) d[c * plane + i] = v[i];
    }
  }
}

template <typename T>
static int lut_planar_launch(const void* src, int src_w, int top, int left, int out_h, int out_w, const void* lut, void* dst, hipStream_t stream) {
  const long long groups = (long long)out_h * ((out_w + 3) / 4);
  const dim3 grid((unsigned)((groups + 255) / 256));
  const bool wide_out = out_w % 4 == 0 && !((uintptr_t)dst & 15);
  const bool wide_in = wide_out && (src_w * 3) % 4 == 0 && (left * 3) % 4 == 0 && !((uintptr_t)src & 3);
#define CE_LUT_LAUNCH(WI, WO)                                                                                                      \
  hipLaunchKernelGGL((lut_planar_kernel<T, WI, WO>), grid, dim3(256), 0, stream, (const uint8_t*)src, src_w, top, left, out_h, out_w, \
                     (const T*)lut, (T*)dst)
  if (wide_in) CE_LUT_LAUNCH(true, true);
  else if (wide_out) CE_LUT_LAUNCH(false, true);
  else CE_LUT_LAUNCH(false, false);
#undef CE_LUT_LAUNCH
  return (int)hipGetLastError();
}

CE_API int ce_image_u8_lut_planar(const void* src, int src_h, int src_w, int top, int left, int out_h, int out_w, const void* lut, void* dst,
                                  int dst_f32, hipStream_t stream) {
  if (!src || !lut || !dst || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0) return CE_ERR_ARG;
  if (top < 0 || left < 0 || (long long)top + out_h > src_h || (long long)left + out_w > src_w) return CE_ERR_ARG;  // the crop lies inside the source
  if ((long long)src_h * src_w * 3 >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)lut | (uintptr_t)dst) & (dst_f32 ? 3 : 1)) return CE_ERR_ALIGN;
  return dst_f32 ? lut_planar_launch<uint32_t>(src, src_w, top, left, out_h, out_w, lut, dst, stream)
                 : lut_planar_launch<uint16_t>(src, src_w, top, left, out_h, out_w, lut, dst, stream);
}

// (v * 0.5 + 0.5) clamped to [0, 1], times 255, rounded half to even: three fp32 roundings.  hipcc contracts `a * b + c` into one fma by
// default (and __fmul_rn / __fadd_rn are plain operators in its headers), hence the pragma.  fmaxf returns the other operand for a NaN:
// NaN -> 0; +inf -> 255, -inf -> 0.
__device__ __forceinline__ uint32_t video_u8(float v) {
#pragma clang fp contract(off)
  float f = v * 0.5f;
  f = f + 0.5f;
  f = fminf(fmaxf(f, 0.0f), 1.0f);
  return (uint32_t)rintf(f * 255.0f);
}

__device__ __forceinline__ float video_elem(const uint16_t* p, size_t i) { return bf16_bits_to_f32(p[i]); }
__device__ __forceinline__ float video_elem(const float* p, size_t i) { return p[i]; }

// One lane per P = 16 / sizeof(T) consecutive pixels of one frame: 16 bytes from each of the three colour planes, 3 P contiguous output
// bytes.  WIDE (H W % P == 0, src 16-byte and dst 4-byte aligned): the plane reads are one vector each and the output goes out as dwords;
// otherwise (a frame is no whole number of groups, so the planes lose their alignment) element by element with a tail in the last group.
template <typename T, bool WIDE>
__global__ __launch_bounds__(256) void video_to_u8_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst, int F, long long hw, long long frames) {
  constexpr int P = 16 / (int)sizeof(T);
  const long long gpf = (hw + P - 1) / P;  // groups per frame
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= frames * gpf) return;
  const long long bf = g / gpf, p0 = (g - bf * gpf) * P;
  const long long b = bf / F, f = bf - b * F;
  const T* s = src + ((size_t)b * 3 * F + f) * hw + p0;  // channel c: + c * F * hw
  const size_t cs = (size_t)F * hw;
  uint8_t* d = dst + ((size_t)bf * hw + p0) * 3;
  if (WIDE) {
    uint32_t u[3][P];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const u32x4 v = *(const u32x4*)(s + c * cs);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (sizeof(T) == 2) {
          u[c][2 * k] = video_u8(bf16lo(v[k]));
          u[c][2 * k + 1] = video_u8(bf16hi(v[k]));
        } else {
          u[c][k] = video_u8(__uint_as_float(v[k]));
        }
      }
    }
    uint32_t* d4 = (uint32_t*)d;
#pragma unroll
    for (int w = 0; w < 3 * P / 4; ++w) {
      uint32_t o = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int byte = 4 * w + j;
        o |= u[byte % 3][byte / 3] << (8 * j);
      }
      d4[w] = o;
    }
  } else {
    const int npx = (int)((hw - p0) < P ? (hw - p0) : P);
    for (int i = 0; i < npx; ++i)
      for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint8_t)video_u8(video_elem(s, c * cs + i));
  }
}

template <typename T>
static int video_to_u8_launch(const void* src, void* dst, int B, int F, long long hw, hipStream_t stream) {
  constexpr int P = 16 / (int)sizeof(T);
  const long long frames = (long long)B * F, groups = frames * ((hw + P - 1) / P);
  if (groups > 0x7fffffffll * 256) return CE_ERR_SHAPE;
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (hw % P == 0 && !((uintptr_t)src & 15) && !((uintptr_t)dst & 3))
    hipLaunchKernelGGL((video_to_u8_kernel<T, true>), grid, dim3(256), 0, stream, (const T*)src, (uint8_t*)dst, F, hw, frames);
  else
    hipLaunchKernelGGL((video_to_u8_kernel<T, false>), grid, dim3(256), 0, stream, (const T*)src, (uint8_t*)dst, F, hw, frames);
  return (int)hipGetLastError();
}

CE_API int ce_video_to_u8(const void* src, void* dst, int B, int F, int H, int W, int src_f32, hipStream_t stream) {
  if (!src || !dst || B <= 0 || F <= 0 || H <= 0 || W <= 0) return CE_ERR_ARG;
  if ((uintptr_t)src & (src_f32 ? 3 : 1)) return CE_ERR_ALIGN;
  const long long hw = (long long)H * W;
  return src_f32 ? video_to_u8_launch<float>(src, dst, B, F, hw, stream) : video_to_u8_launch<uint16_t>(src, dst, B, F, hw, stream);
}

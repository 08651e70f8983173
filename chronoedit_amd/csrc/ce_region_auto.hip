// Automatic edit regions (chronoedit_amd/auto_region.py): find the region of an instruction-only edit from the model's own estimate of the
// final image after a few dense steps, and continue as a region-limited edit (csrc/ce_region.hip).
//
//   ce_auto_region_change_f32   x0, z_src fp32 [B][C][T][h][w] -> d fp32 [h][w], on ONE latent frame:
//                               d = max over b of ((sum over c = 0..C-1, in that order, of (x0 - z_src)^2) / C)
//   ce_auto_region_otsu_f32     d -> thr (and dmax): Otsu's threshold over a 256-bin histogram of d, one workgroup, nothing read back
//   ce_auto_region_ramp_f32     seed = d > *thr -> w fp32 [h][w]: 1 within `dilate` cells (Chebyshev) of a seed, a linear ramp over the next
//                               `feather` cells, 0 beyond
//   ce_auto_region_mask_u8      w -> uint8 [8h][8w]: byte = rint(255.0f * w[Y / 8][X / 8]), the mask of the paste-back
//
// Every subtract, multiply, add and division is an fp32 operation rounded on its own (`#pragma clang fp contract(off)`, as in
// csrc/ce_region.hip); the histogram and its moments are integers, the between-class variance is evaluated in float64 from them: each pass is
// bit-equal to the torch expression of auto_region.py.  No scratch, no state, nothing allocated, no host read: capturable.
#include "ce_common.h"

// one cell of one sample: the channel sum in order, then the one division
__device__ __forceinline__ float auto_change_acc(float s, float x, float z) {
#pragma clang fp contract(off)
  const float df = x - z;
  const float sq = df * df;
  return s + sq;
}

__device__ __forceinline__ float auto_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// the maximum that keeps a NaN (torch.amax): a NaN cell stays a NaN in d and is never a seed
__device__ __forceinline__ float auto_max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// One lane per four neighbouring cells of the frame's plane (WIDE: plane % 4 == 0 and x0, z_src, d 16-byte aligned - every channel plane
// then starts aligned too) or per cell.  stride_c = T * plane elements between channels, stride_b = C * stride_c between samples.
template <bool WIDE>
__global__ __launch_bounds__(256) void auto_change_kernel(const float* __restrict__ x0, const float* __restrict__ z, float* __restrict__ d, int B,
                                                          int C, long long plane, long long stride_c, long long stride_b, long long frame_off) {
  constexpr int P = WIDE ? 4 : 1;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g * P >= plane) return;
  const long long p0 = g * P;
  const float fc = (float)C;
  float m[P];
  for (int b = 0; b < B; ++b) {
    const float* xs = x0 + (size_t)b * stride_b + frame_off + p0;
    const float* zs = z + (size_t)b * stride_b + frame_off + p0;
    float s[P];
#pragma unroll
    for (int j = 0; j < P; ++j) s[j] = 0.0f;
    for (int c = 0; c < C; ++c) {
      if (WIDE) {
        const u32x4 xv = *(const u32x4*)(xs + (size_t)c * stride_c), zv = *(const u32x4*)(zs + (size_t)c * stride_c);
#pragma unroll
        for (int j = 0; j < P; ++j) s[j] = auto_change_acc(s[j], __uint_as_float(xv[j]), __uint_as_float(zv[j]));
      } else {
        s[0] = auto_change_acc(s[0], xs[(size_t)c * stride_c], zs[(size_t)c * stride_c]);
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float v = auto_div(s[j], fc);
      m[j] = b == 0 ? v : auto_max_nan(m[j], v);
    }
  }
  if (WIDE) {
    const u32x4 o = {__float_as_uint(m[0]), __float_as_uint(m[1 % P]), __float_as_uint(m[2 % P]), __float_as_uint(m[3 % P])};
    *(u32x4*)(d + p0) = o;
  } else {
    d[p0] = m[0];
  }
}

CE_API int ce_auto_region_change_f32(const float* x0, const float* z_src, float* d, int B, int C, int T, int h, int w, int frame,
                                     hipStream_t stream) {
  if (!x0 || !z_src || !d || B <= 0 || C <= 0 || T <= 0 || h <= 0 || w <= 0 || frame < 0 || frame >= T) return CE_ERR_ARG;
  const long long plane = (long long)h * w;
  if (plane >= (1ll << 31) || (long long)B * C * T * plane >= (1ll << 40)) return CE_ERR_SHAPE;
  const uintptr_t all = (uintptr_t)x0 | (uintptr_t)z_src | (uintptr_t)d;
  if (all & 3) return CE_ERR_ALIGN;
  const long long stride_c = (long long)T * plane, stride_b = (long long)C * stride_c, frame_off = (long long)frame * plane;
  if (plane % 4 == 0 && !(all & 15)) {
    const long long groups = plane / 4;
    hipLaunchKernelGGL(auto_change_kernel<true>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, stream, x0, z_src, d, B, C, plane, stride_c,
                       stride_b, frame_off);
  } else {
    hipLaunchKernelGGL(auto_change_kernel<false>, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, stream, x0, z_src, d, B, C, plane, stride_c,
                       stride_b, frame_off);
  }
  return (int)hipGetLastError();
}

// ---- Otsu's threshold ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float auto_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// the bin of one cell: min(255, int(d * scale)); a NaN (of d, or of inf * 0) and anything negative go to bin 0
__device__ __forceinline__ int auto_bin(float dv, float scale) {
  const float v = auto_mul(dv, scale);
  if (!(v >= 0.0f)) return 0;
  return (int)(v < 255.0f ? v : 255.0f);
}

// ONE workgroup of 256 lanes: lane t owns bin t and candidate t.  dmax (NaN cells ignored), the histogram (integer atomics in LDS), then
// per candidate the cumulative count w0 and first moment s0 through bin t, the score (s0 N - S w0)^2 / (w0 (N - w0)) in float64 from the
// integers, and the arg-max with the lowest t winning a tie.
__global__ __launch_bounds__(256) void auto_otsu_kernel(const float* __restrict__ d, int n, float floor_v, float* __restrict__ thr,
                                                        float* __restrict__ dmax_out) {
  __shared__ float red_f[256];
  __shared__ int hist[256];
  __shared__ double score[256];
  __shared__ int best[256];
  const int t = threadIdx.x;
  float mx = 0.0f;  // d >= 0 or NaN: fmaxf drops the NaN
  for (int i = t; i < n; i += 256) mx = fmaxf(mx, d[i]);
  red_f[t] = mx;
  hist[t] = 0;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red_f[t] = fmaxf(red_f[t], red_f[t + s]);
    __syncthreads();
  }
  const float dmax = red_f[0];
  const float fl2 = auto_mul(floor_v, floor_v);
  if (!(dmax > 0.0f)) {  // nothing changed anywhere: no threshold any cell passes
    if (t == 0) {
      thr[0] = __uint_as_float(0x7f800000u);
      if (dmax_out) dmax_out[0] = dmax;
    }
    return;
  }
  const float scale = auto_div(256.0f, dmax);
  for (int i = t; i < n; i += 256) atomicAdd(&hist[auto_bin(d[i], scale)], 1);
  __syncthreads();
  long long w0 = 0, s0 = 0, S = 0;
  for (int i = 0; i < 256; ++i) {
    const long long c = hist[i];
    S += (long long)i * c;
    if (i <= t) w0 += c, s0 += (long long)i * c;
  }
  const long long N = n;
  const bool valid = w0 > 0 && w0 < N;
  double sc = -1.0;  // (a valid score is >= 0)
  if (valid) {
    const double num = (double)(s0 * N - S * w0);
    sc = (num * num) / (double)(w0 * (N - w0));
  }
  score[t] = sc;
  best[t] = valid ? t : 256;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const double a = score[t], b = score[t + s];
      const int ia = best[t], ib = best[t + s];
      if (b > a || (b == a && ib < ia)) score[t] = b, best[t] = ib;
    }
    __syncthreads();
  }
  if (t == 0) {
    const int tb = best[0] >= 256 ? 0 : best[0];  // a constant map: every cell in one bin, nothing to separate
    const float step = auto_div(dmax, 256.0f);
    const float v = auto_mul((float)(tb + 1), step);
    thr[0] = v > fl2 ? v : fl2;
    if (dmax_out) dmax_out[0] = dmax;
  }
}

CE_API int ce_auto_region_otsu_f32(const float* d, int n, float floor_v, float* thr, float* dmax, hipStream_t stream) {
  if (!d || !thr || n <= 0 || !(floor_v >= 0.0f)) return CE_ERR_ARG;
  if (n >= (1 << 24)) return CE_ERR_SHAPE;  // (255 n^2 stays far inside int64, and exact in float64's 53 bits at the 720p map)
  if (((uintptr_t)d | (uintptr_t)thr | (uintptr_t)dmax) & 3) return CE_ERR_ALIGN;
  hipLaunchKernelGGL(auto_otsu_kernel, dim3(1), dim3(256), 0, stream, d, n, floor_v, thr, dmax);
  return (int)hipGetLastError();
}

// ---- dilate + feather ----------------------------------------------------------------------------------------------------------------
// One lane per cell: the smallest Chebyshev distance r to a seed inside the (2R + 1)^2 window, R = dilate + feather <= 8 (the ramp does not
// rise with r, so the maximum over the seeds is the ramp of the nearest).  Cells outside the grid are no seeds.
__global__ __launch_bounds__(256) void auto_ramp_kernel(const float* __restrict__ d, const float* __restrict__ thr, float* __restrict__ w, int h,
                                                        int wl, int dilate, int feather) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= h * wl) return;
  const int y = g / wl, x = g - y * wl, R = dilate + feather;
  const float th = thr[0];
  int rmin = R + 1;
  const int y0 = y - R < 0 ? 0 : y - R, y1 = y + R >= h ? h - 1 : y + R;
  const int x0 = x - R < 0 ? 0 : x - R, x1 = x + R >= wl ? wl - 1 : x + R;
  for (int yy = y0; yy <= y1; ++yy) {
    const int dy = yy > y ? yy - y : y - yy;
    for (int xx = x0; xx <= x1; ++xx) {
      const int dx = xx > x ? xx - x : x - xx;
      const int r = dy > dx ? dy : dx;
      if (r < rmin && d[(size_t)yy * wl + xx] > th) rmin = r;
    }
  }
  float o = 0.0f;
  if (rmin <= dilate)
    o = 1.0f;
  else if (rmin <= R)
    o = auto_div((float)(feather + 1 - (rmin - dilate)), (float)(feather + 1));
  w[g] = o;
}

CE_API int ce_auto_region_ramp_f32(const float* d, const float* thr, float* w, int h, int wl, int dilate, int feather, hipStream_t stream) {
  if (!d || !thr || !w || d == (const float*)w || h <= 0 || wl <= 0 || dilate < 0 || feather < 0 || dilate + feather > 8) return CE_ERR_ARG;
  if ((long long)h * wl >= (1ll << 24)) return CE_ERR_SHAPE;
  if (((uintptr_t)d | (uintptr_t)thr | (uintptr_t)w) & 3) return CE_ERR_ALIGN;
  hipLaunchKernelGGL(auto_ramp_kernel, dim3((unsigned)((h * wl + 255) / 256)), dim3(256), 0, stream, d, thr, w, h, wl, dilate, feather);
  return (int)hipGetLastError();
}

// ---- the pixel mask --------------------------------------------------------------------------------------------------------------------
// byte = rint(255.0f * w) (half to even), clamped to 0..255; a NaN gives 0
__device__ __forceinline__ uint32_t auto_byte(float wv) {
  const float v = rintf(auto_mul(255.0f, wv));
  if (!(v >= 0.0f)) return 0u;
  return (uint32_t)(v < 255.0f ? v : 255.0f);
}

// One lane per cell and pixel row of it: eight equal bytes, one 8-byte store (WIDE: the mask 8-byte aligned; its rows are 8 wl bytes) or
// eight byte stores.
template <bool WIDE>
__global__ __launch_bounds__(256) void auto_mask_kernel(const float* __restrict__ w, uint8_t* __restrict__ mask, int h, int wl) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long rows = (long long)h * 8;
  if (g >= rows * wl) return;
  const long long Y = g / wl;
  const int x = (int)(g - Y * wl);
  const uint32_t b = auto_byte(w[(size_t)(Y >> 3) * wl + x]);
  uint8_t* dst = mask + (size_t)g * 8;  // = Y * (8 wl) + 8 x
  if (WIDE) {
    const uint32_t q = b * 0x01010101u;
    const u32x2 o = {q, q};
    *(u32x2*)dst = o;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = (uint8_t)b;
  }
}

CE_API int ce_auto_region_mask_u8(const float* w, void* mask, int h, int wl, hipStream_t stream) {
  if (!w || !mask || h <= 0 || wl <= 0) return CE_ERR_ARG;
  const long long groups = (long long)h * 8 * wl;
  if (groups * 8 >= (1ll << 31)) return CE_ERR_SHAPE;
  if ((uintptr_t)w & 3) return CE_ERR_ALIGN;
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (!((uintptr_t)mask & 7))
    hipLaunchKernelGGL(auto_mask_kernel<true>, grid, dim3(256), 0, stream, w, (uint8_t*)mask, h, wl);
  else
    hipLaunchKernelGGL(auto_mask_kernel<false>, grid, dim3(256), 0, stream, w, (uint8_t*)mask, h, wl);
  return (int)hipGetLastError();
}

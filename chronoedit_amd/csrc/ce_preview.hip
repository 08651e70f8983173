// Live previews (chronoedit_amd/preview.py): a cheap RGB estimate of the running edit from the scheduler's predict-x0 slot, and the Gram
// matrix the linear latent -> RGB map is fitted from on the loaded VAE.
//
//   ce_preview_rgb_u8     x0 (and z_src, w) fp32 [B][16][T][h][w], ONE latent frame -> uint8 [B][h s][w s][3]: the region composite per cell,
//                         the 16 -> 3 projection per cell, a bilinear upsample by s in {1, 2, 4, 8} (half-pixel centres), the byte of
//                         ce_video_to_u8
//   ce_preview_gram_f64   z fp32 [B][16][T][h][w] (one frame), y [B][3][8h][8w] fp32 / bf16 -> float64 [20][20] = sum over cells of v v^T,
//                         v = (z_0..z_15, 1, r, g, b), r g b the 8x8 box mean of the cell's pixels
//
// Every fp32 multiply, add and subtract is rounded on its own (`#pragma clang fp contract(off)`, as in csrc/ce_region_auto.hip): the preview is
// bit-equal to preview.rgb_u8_reference evaluated op by op.  The Gram matrix's products (exact: two fp32 factors) and sums are float64 in a
// fixed order - per-workgroup partials in the caller's scratch, added in workgroup order by a second launch, no atomics: two runs give the
// same bits.  No allocation, no state, no host read: capturable.
#include "ce_common.h"

#define PV_C 16         // latent channels
#define PV_TCY 4        // latent cells per workgroup tile, rows
#define PV_TCX 16       // ... and columns
#define PV_HY (PV_TCY + 2)  // with the one-cell halo the bilinear taps reach
#define PV_HX (PV_TCX + 2)

// u = (w * x) + ((1 - w) * z): the caller passes iw = 1 - w
__device__ __forceinline__ float pv_mix(float x, float z, float w, float iw) {
#pragma clang fp contract(off)
  const float a = w * x;
  const float b = iw * z;
  return a + b;
}

__device__ __forceinline__ float pv_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// p + f * u: one multiply, then one add
__device__ __forceinline__ float pv_acc(float p, float f, float u) {
#pragma clang fp contract(off)
  const float t = f * u;
  return p + t;
}

// a * (1 - t) + b * t
__device__ __forceinline__ float pv_lerp(float a, float b, float t) {
#pragma clang fp contract(off)
  const float s = 1.0f - t;
  const float l = a * s;
  const float r = b * t;
  return l + r;
}

// the byte of ce_video_to_u8 (csrc/ce_image.hip): (v * 0.5 + 0.5) clamped to [0, 1], times 255, half to even; NaN -> 0, +inf -> 255, -inf -> 0
__device__ __forceinline__ uint32_t pv_u8(float v) {
#pragma clang fp contract(off)
  float f = v * 0.5f;
  f = f + 0.5f;
  f = fminf(fmaxf(f, 0.0f), 1.0f);
  return (uint32_t)rintf(f * 255.0f);
}

// the source coordinate of output index o: (o + 0.5) / s - 0.5 clamped to [0, n - 1] (exact in fp32 for a power-of-two s) -> i0, i1, t
__device__ __forceinline__ void pv_tap(int o, float inv_s, int n, int& i0, int& i1, float& t) {
#pragma clang fp contract(off)
  float f = ((float)o + 0.5f) * inv_s;
  f = f - 0.5f;
  f = fminf(fmaxf(f, 0.0f), (float)(n - 1));
  const float fl = floorf(f);
  i0 = (int)fl;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  t = f - fl;
}

// One workgroup per PV_TCY x PV_TCX tile of latent cells and sample: the tile's cells and a one-cell halo are projected once into the LDS
// (one lane per cell, the 16 channels in order), then every lane interpolates its share of the tile's (PV_TCY s) x (PV_TCX s) pixels.  WIDE
// (w s % 4 == 0 and `out` 4-byte aligned: every pixel row then starts on a dword): one lane per four pixels of a row, three dword stores;
// otherwise one lane per pixel, three byte stores.
template <bool WIDE>
__global__ __launch_bounds__(256) void preview_rgb_kernel(const float* __restrict__ x0, const float* __restrict__ zs, const float* __restrict__ wt,
                                                          const float* __restrict__ fac, uint8_t* __restrict__ out, int T, int frame, int h, int w,
                                                          int scale) {
  __shared__ float proj[3][PV_HY][PV_HX];
  const int t = threadIdx.x;
  const int cx0 = blockIdx.x * PV_TCX, cy0 = blockIdx.y * PV_TCY, b = blockIdx.z;
  const size_t plane = (size_t)h * w;
  if (t < PV_HY * PV_HX) {
    const int ly = t / PV_HX, lx = t - ly * PV_HX;
    const int cy = cy0 - 1 + ly, cx = cx0 - 1 + lx;
    if (cy >= 0 && cy < h && cx >= 0 && cx < w) {
      const size_t cell = (size_t)cy * w + cx;
      const size_t base = ((size_t)b * PV_C * T + frame) * plane + cell;  // channel k: + k * T * plane
      const size_t cs = (size_t)T * plane;
      float p0 = fac[PV_C * 3 + 0], p1 = fac[PV_C * 3 + 1], p2 = fac[PV_C * 3 + 2];
      float wv = 0.0f, iw = 0.0f;
      if (wt) {
        wv = wt[cell];
        iw = pv_sub(1.0f, wv);
      }
      for (int k = 0; k < PV_C; ++k) {
        float u = x0[base + k * cs];
        if (wt) u = pv_mix(u, zs[base + k * cs], wv, iw);
        p0 = pv_acc(p0, fac[3 * k + 0], u);
        p1 = pv_acc(p1, fac[3 * k + 1], u);
        p2 = pv_acc(p2, fac[3 * k + 2], u);
      }
      proj[0][ly][lx] = p0;
      proj[1][ly][lx] = p1;
      proj[2][ly][lx] = p2;
    }
  }
  __syncthreads();
  const int th = (h - cy0 < PV_TCY ? h - cy0 : PV_TCY) * scale;  // the tile's pixels that lie inside the image
  const int tw = (w - cx0 < PV_TCX ? w - cx0 : PV_TCX) * scale;
  const int W = w * scale, H = h * scale;
  const float inv_s = 1.0f / (float)scale;
  constexpr int P = WIDE ? 4 : 1;
  const int gw = tw / P;  // (WIDE: tw is a multiple of 4 - PV_TCX s is, and so is w s)
  for (int g = t; g < th * gw; g += 256) {
    const int py = g / gw, px = (g - py * gw) * P;
    const int Y = cy0 * scale + py, X = cx0 * scale + px;
    int y0, y1;
    float ty;
    pv_tap(Y, inv_s, h, y0, y1, ty);
    const int ly0 = y0 - (cy0 - 1), ly1 = y1 - (cy0 - 1);
    uint32_t u[P][3];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      int xa, xb;
      float tx;
      pv_tap(X + j, inv_s, w, xa, xb, tx);
      const int lxa = xa - (cx0 - 1), lxb = xb - (cx0 - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = pv_lerp(proj[c][ly0][lxa], proj[c][ly0][lxb], tx);
        const float bot = pv_lerp(proj[c][ly1][lxa], proj[c][ly1][lxb], tx);
        u[j][c] = pv_u8(pv_lerp(top, bot, ty));
      }
    }
    uint8_t* d = out + (((size_t)b * H + Y) * W + X) * 3;
    if (WIDE) {
      uint32_t* d4 = (uint32_t*)d;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int byte = 4 * q + j;
          o |= u[(byte / 3) % P][byte % 3] << (8 * j);
        }
        d4[q] = o;
      }
    } else {
      d[0] = (uint8_t)u[0][0];
      d[1] = (uint8_t)u[0][1];
      d[2] = (uint8_t)u[0][2];
    }
  }
}

CE_API int ce_preview_rgb_u8(const float* x0, const float* z_src, const float* w, const float* factors, void* out, int B, int C, int T, int frame,
                             int h, int wl, int scale, hipStream_t stream) {
  if (!x0 || !factors || !out || B <= 0 || C != PV_C || T <= 0 || h <= 0 || wl <= 0 || frame < 0 || frame >= T) return CE_ERR_ARG;
  if ((z_src == nullptr) != (w == nullptr)) return CE_ERR_ARG;  // the composite takes both or neither
  if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return CE_ERR_ARG;
  const long long plane = (long long)h * wl;
  if (plane >= (1ll << 24) || (long long)B * C * T * plane >= (1ll << 40) || (long long)B * plane * scale * scale * 3 >= (1ll << 40)) return CE_ERR_SHAPE;
  const long long gx = (wl + PV_TCX - 1) / PV_TCX, gy = (h + PV_TCY - 1) / PV_TCY;
  if (gy > 65535 || B > 65535) return CE_ERR_SHAPE;
  if (((uintptr_t)x0 | (uintptr_t)z_src | (uintptr_t)w | (uintptr_t)factors) & 3) return CE_ERR_ALIGN;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  if (((long long)wl * scale) % 4 == 0 && !((uintptr_t)out & 3))
    hipLaunchKernelGGL(preview_rgb_kernel<true>, grid, dim3(256), 0, stream, x0, z_src, w, factors, (uint8_t*)out, T, frame, h, wl, scale);
  else
    hipLaunchKernelGGL(preview_rgb_kernel<false>, grid, dim3(256), 0, stream, x0, z_src, w, factors, (uint8_t*)out, T, frame, h, wl, scale);
  return (int)hipGetLastError();
}

// ---- the Gram matrix of the fit -------------------------------------------------------------------------------------------------------
#define PG_N 20                        // the vector of a cell: 16 latents, 1, r, g, b
#define PG_PAIRS (PG_N * (PG_N + 1) / 2)  // the upper triangle, row by row
#define PG_BATCH 64                    // cells a workgroup stages per round
#define PG_MAX_WG 1024

// the 8x8 box mean: an fp32 sum of the 64 values in row-major order, times 1 / 64
template <typename TY>
__device__ __forceinline__ float pg_box_mean(const TY* __restrict__ p, size_t pitch) {
#pragma clang fp contract(off)
  float s = 0.0f;
  for (int r = 0; r < 8; ++r)
    for (int q = 0; q < 8; ++q) {
      float v;
      if constexpr (sizeof(TY) == 2)
        v = bf16_bits_to_f32(p[r * pitch + q]);
      else
        v = p[r * pitch + q];
      s = s + v;
    }
  return s * 0.015625f;
}

// pair e of the upper triangle, row by row -> (i, j), i <= j
__device__ __forceinline__ void pg_pair(int e, int& i, int& j) {
  i = 0;
  while (e >= PG_N - i) e -= PG_N - i, ++i;
  j = i + e;
}

// Workgroup g takes the rounds g, g + gridDim.x, ... of PG_BATCH consecutive cells (cells counted over b, y, x).  Per round: lanes 0..191
// pool one colour of one cell, lanes 192..255 copy one cell's 16 latents; then lane e < 210 adds the round's products of its pair, in cell
// order, to its float64 sum.  partial[g][e] is written once.
template <typename TY>
__global__ __launch_bounds__(256) void preview_gram_kernel(const float* __restrict__ z, const TY* __restrict__ y, double* __restrict__ partial, int T,
                                                           int frame, int h, int w, long long cells) {
  __shared__ float v[PG_BATCH][PG_N + 1];  // (+1: lanes of one wave read the same two columns of different rows)
  const int t = threadIdx.x;
  const long long plane = (long long)h * w;
  int pi = 0, pj = 0;
  if (t < PG_PAIRS) pg_pair(t, pi, pj);
  double acc = 0.0;
  const long long rounds = (cells + PG_BATCH - 1) / PG_BATCH;
  for (long long r = blockIdx.x; r < rounds; r += gridDim.x) {
    const long long c0 = r * PG_BATCH;
    const int n = (int)(cells - c0 < PG_BATCH ? cells - c0 : PG_BATCH);
    const int lc = t & (PG_BATCH - 1), job = t / PG_BATCH;  // job 0..2: a colour, 3: the latents
    if (lc < n) {
      const long long cell = c0 + lc;
      const long long b = cell / plane, p = cell - b * plane;
      const int cy = (int)(p / w), cx = (int)(p - (long long)cy * w);
      if (job < 3) {
        const size_t pitch = (size_t)8 * w;
        const TY* src = y + (((size_t)b * 3 + job) * 8 * h + (size_t)8 * cy) * pitch + (size_t)8 * cx;
        v[lc][PV_C + 1 + job] = pg_box_mean<TY>(src, pitch);
      } else {
        const size_t cs = (size_t)T * plane;
        const float* src = z + ((size_t)b * PV_C * T + frame) * plane + p;
        for (int k = 0; k < PV_C; ++k) v[lc][k] = src[k * cs];
        v[lc][PV_C] = 1.0f;
      }
    }
    __syncthreads();
    if (t < PG_PAIRS)
      for (int c = 0; c < n; ++c) acc += (double)v[c][pi] * (double)v[c][pj];
    __syncthreads();
  }
  if (t < PG_PAIRS) partial[(size_t)blockIdx.x * PG_PAIRS + t] = acc;
}

// out[i][j] = out[j][i] = the partials of pair (i, j) added in workgroup order
__global__ __launch_bounds__(256) void preview_gram_sum_kernel(const double* __restrict__ partial, double* __restrict__ out, int groups) {
  const int t = threadIdx.x;
  if (t >= PG_PAIRS) return;
  int i, j;
  pg_pair(t, i, j);
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += partial[(size_t)g * PG_PAIRS + t];
  out[i * PG_N + j] = s;
  out[j * PG_N + i] = s;
}

CE_API int ce_preview_gram_f64(const float* z, int frame, const void* y, int y_bf16, double* out, void* scratch, size_t scratch_bytes, int B, int T,
                               int h, int wl, hipStream_t stream) {
  if (!z || !y || !out || !scratch || B <= 0 || T <= 0 || h <= 0 || wl <= 0 || frame < 0 || frame >= T) return CE_ERR_ARG;
  if (scratch_bytes < PG_PAIRS * sizeof(double)) return CE_ERR_ARG;
  const long long plane = (long long)h * wl, cells = (long long)B * plane;
  if (plane >= (1ll << 24) || (long long)B * PV_C * T * plane >= (1ll << 40) || cells * 192 >= (1ll << 40)) return CE_ERR_SHAPE;
  if (((uintptr_t)z & 3) || ((uintptr_t)y & (y_bf16 ? 1 : 3)) || (((uintptr_t)out | (uintptr_t)scratch) & 7)) return CE_ERR_ALIGN;
  const long long rounds = (cells + PG_BATCH - 1) / PG_BATCH;
  long long groups = (long long)(scratch_bytes / (PG_PAIRS * sizeof(double)));
  if (groups > PG_MAX_WG) groups = PG_MAX_WG;
  if (groups > rounds) groups = rounds;
  if (y_bf16)
    hipLaunchKernelGGL(preview_gram_kernel<uint16_t>, dim3((unsigned)groups), dim3(256), 0, stream, z, (const uint16_t*)y, (double*)scratch, T, frame, h,
                       wl, cells);
  else
    hipLaunchKernelGGL(preview_gram_kernel<float>, dim3((unsigned)groups), dim3(256), 0, stream, z, (const float*)y, (double*)scratch, T, frame, h, wl,
                       cells);
  const int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(preview_gram_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)scratch, out, (int)groups);
  return (int)hipGetLastError();
}

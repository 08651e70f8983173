// Guided detail lift (chronoedit_amd/lift.py): a whole-image edit made at the edit's size is carried up to the photo's pixel grid.  Per
// neighbourhood and colour an affine map a * I + b from the edit-size source L to the edit-size change d = E - L is fitted, the maps are
// smoothed, sampled bilinearly at the photo's pixel centres and applied to the photo's own bytes; where the affine model does not explain
// the change the plain Lanczos upsample of the edited frame takes over (the gate g).
//
//   ce_lift_fit_q16     L, E -> A, B = rint(65536 a), rint(65536 b) int32 [F][H][W][6]: exact integer box statistics, one double division
//   ce_lift_smooth_f32  A, B -> the box means abar, bbar in the coefficient cells fp32 [F][H][W][8] (g and the pad zeroed), and the
//                       residual of the smoothed model R = rint(256 min(res, 255)) int32 [F][H][W]
//   ce_lift_gate_f32    R -> g in slot 6 of the cells
//   ce_lift_apply_u8    P (and U), the cells, the axis tables -> uint8 [F][SH][SW][3]: the streaming pass
//
// lift.reference (CPU torch) is the definition; every pass is bit-equal to its stage.  The box sums are integers (that is what the fixed
// point is for): any summation order gives the same bits, so the three grid passes stage a tile and its halo in the LDS and sum separably.
// Every fp32 / fp64 multiply, add and subtract is rounded on its own (`#pragma clang fp contract(off)`, as in csrc/ce_preview.hip).
// No state, nothing allocated, no host read: every call is capturable.
#include "ce_common.h"
#include "ce_lift_pixel.h"  // LF_CELL, the corner cells and the per-pixel arithmetic of the apply stage (shared with csrc/ce_boxlift.hip)

#define LF_T 16         // a workgroup's tile: LF_T x LF_T cells, one lane per cell
#define LF_RMAX 16      // the largest radius: the staged side is LF_T + 2 r <= 48 cells

// the window [i - r, i + r] clipped to [0, n): its cell count along one axis
__device__ __forceinline__ int lf_span(int i, int r, int n) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

// ---- stage 1: the fit ------------------------------------------------------------------------------------------------------------------
// Per colour: the tile's I and d with the halo (0 outside the image: nothing is added for a clipped cell), the horizontal sums of
// (I, d, I I, I d) per staged row and tile column, then per lane the vertical sum and the division.  All sums fit int32 for r <= 16
// (1089 * 255 * 255 < 2^27).
__global__ __launch_bounds__(256) void lift_fit_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ E, int* __restrict__ AB, int H, int W,
                                                       int r, int eps_q, float max_gain) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) int lf_smem[];
  const int S = LF_T + 2 * r;
  int* vi = lf_smem;                    // [S][S]
  int* vd = vi + S * S;                 // [S][S]
  int4* hs = (int4*)(vd + S * S);       // [S][LF_T]  (S is even: 2 S S ints are a multiple of 16 bytes)
  const int t = threadIdx.x, f = blockIdx.z;
  const int x0 = blockIdx.x * LF_T, y0 = blockIdx.y * LF_T;
  const int ty = t / LF_T, tx = t - ty * LF_T;
  const int y = y0 + ty, x = x0 + tx;
  const size_t plane = (size_t)H * W;
  const uint8_t* Ef = E + (size_t)f * plane * 3;
  for (int c = 0; c < 3; ++c) {
    for (int i = t; i < S * S; i += 256) {
      const int ly = i / S, lx = i - ly * S;
      const int gy = y0 - r + ly, gx = x0 - r + lx;
      int I = 0, d = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const size_t o = ((size_t)gy * W + gx) * 3 + c;
        I = L[o];
        d = (int)Ef[o] - I;
      }
      vi[i] = I;
      vd[i] = d;
    }
    __syncthreads();
    for (int i = t; i < S * LF_T; i += 256) {
      const int ly = i / LF_T, ox = i - ly * LF_T;
      const int* pi = vi + ly * S + ox;
      const int* pd = vd + ly * S + ox;
      int4 s = {0, 0, 0, 0};
      for (int k = 0; k <= 2 * r; ++k) {
        const int I = pi[k], d = pd[k];
        s.x += I, s.y += d, s.z += I * I, s.w += I * d;
      }
      hs[i] = s;
    }
    __syncthreads();
    if (y < H && x < W) {
      int4 s = {0, 0, 0, 0};
      for (int k = 0; k <= 2 * r; ++k) {
        const int4 v = hs[(ty + k) * LF_T + tx];
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
      }
      const long long n = (long long)lf_span(y, r, H) * lf_span(x, r, W);
      const long long num = n * s.w - (long long)s.x * s.y;
      const long long den = n * s.z - (long long)s.x * s.x + (long long)eps_q * n * n;
      double q = (double)num / (double)den;  // (both below 2^53: the conversions are exact; den >= n n > 0)
      q = fmin(fmax(q, -(double)max_gain), (double)max_gain);
      const float a = (float)q;
      const double m = (double)a * (double)s.x;
      const double u = (double)s.y - m;
      const float b = (float)(u / (double)n);
      int* o = AB + ((size_t)f * plane + (size_t)y * W + x) * 6;
      o[c] = (int)rintf(a * 65536.0f);
      o[3 + c] = (int)rintf(b * 65536.0f);
    }
    __syncthreads();
  }
}

CE_API int ce_lift_fit_q16(const void* L, const void* E, int* AB, int F, int H, int W, int radius, int eps_q, float max_gain, hipStream_t stream) {
  if (!L || !E || !AB || F <= 0 || F > 65535 || H <= 0 || W <= 0) return CE_ERR_ARG;
  if (radius < 1 || radius > LF_RMAX || eps_q < 1 || eps_q > (1 << 30) || !(max_gain >= 1.0f && max_gain <= 8.0f)) return CE_ERR_ARG;
  if ((long long)H * W * 3 >= (1ll << 31) || (H + LF_T - 1) / LF_T > 65535) return CE_ERR_SHAPE;
  if ((uintptr_t)AB & 3) return CE_ERR_ALIGN;
  const int S = LF_T + 2 * radius;
  const size_t lds = (size_t)(2 * S * S) * sizeof(int) + (size_t)S * LF_T * sizeof(int4);
  const dim3 grid((unsigned)((W + LF_T - 1) / LF_T), (unsigned)((H + LF_T - 1) / LF_T), (unsigned)F);
  hipLaunchKernelGGL(lift_fit_kernel, grid, dim3(256), lds, stream, (const uint8_t*)L, (const uint8_t*)E, AB, H, W, radius, eps_q, max_gain);
  return (int)hipGetLastError();
}

// ---- stage 2: the smoothed maps and their residual -------------------------------------------------------------------------------------
// Per colour: A_c and B_c of the tile and its halo, their horizontal sums in int64, per lane the vertical sum, the two means and the
// colour's residual.  The lane then writes its whole cell (g = 0 and the pad: the cell is complete without a gate pass) and R.
__global__ __launch_bounds__(256) void lift_smooth_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ E, const int* __restrict__ AB,
                                                          float* __restrict__ coef, int* __restrict__ R, int H, int W, int r) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) int lf_smem[];
  const int S = LF_T + 2 * r;
  int* va = lf_smem;                         // [S][S]
  int* vb = va + S * S;                      // [S][S]
  long long* hs = (long long*)(vb + S * S);  // [S][LF_T][2]
  const int t = threadIdx.x, f = blockIdx.z;
  const int x0 = blockIdx.x * LF_T, y0 = blockIdx.y * LF_T;
  const int ty = t / LF_T, tx = t - ty * LF_T;
  const int y = y0 + ty, x = x0 + tx;
  const bool inside = y < H && x < W;
  const size_t plane = (size_t)H * W;
  const int* ABf = AB + (size_t)f * plane * 6;
  float mean[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float res = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int i = t; i < S * S; i += 256) {
      const int ly = i / S, lx = i - ly * S;
      const int gy = y0 - r + ly, gx = x0 - r + lx;
      int a = 0, b = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const int* p = ABf + ((size_t)gy * W + gx) * 6;
        a = p[c];
        b = p[3 + c];
      }
      va[i] = a;
      vb[i] = b;
    }
    __syncthreads();
    for (int i = t; i < S * LF_T; i += 256) {
      const int ly = i / LF_T, ox = i - ly * LF_T;
      const int* pa = va + ly * S + ox;
      const int* pb = vb + ly * S + ox;
      long long sa = 0, sb = 0;
      for (int k = 0; k <= 2 * r; ++k) sa += pa[k], sb += pb[k];
      hs[2 * i] = sa;
      hs[2 * i + 1] = sb;
    }
    __syncthreads();
    if (inside) {
      long long sa = 0, sb = 0;
      for (int k = 0; k <= 2 * r; ++k) {
        const long long* v = hs + 2 * ((ty + k) * LF_T + tx);
        sa += v[0], sb += v[1];
      }
      const double den = (double)((long long)lf_span(y, r, H) * lf_span(x, r, W) * 65536);
      const float abar = (float)((double)sa / den), bbar = (float)((double)sb / den);
      mean[c] = abar;
      mean[3 + c] = bbar;
      const size_t o = ((size_t)y * W + x) * 3 + c;
      const int I = L[o];
      const int d = (int)E[(size_t)f * plane * 3 + o] - I;
      const float m = abar * (float)I;
      const float e = m + bbar;
      res = fmaxf(res, fabsf((float)d - e));
    }
    __syncthreads();
  }
  if (inside) {
    const size_t cell = (size_t)f * plane + (size_t)y * W + x;
    float4* o = (float4*)(coef + cell * LF_CELL);
    o[0] = make_float4(mean[0], mean[1], mean[2], mean[3]);
    o[1] = make_float4(mean[4], mean[5], 0.0f, 0.0f);
    R[cell] = (int)rintf(fminf(res, 255.0f) * 256.0f);
  }
}

CE_API int ce_lift_smooth_f32(const void* L, const void* E, const int* AB, float* coef, int* R, int F, int H, int W, int radius, hipStream_t stream) {
  if (!L || !E || !AB || !coef || !R || F <= 0 || F > 65535 || H <= 0 || W <= 0 || radius < 1 || radius > LF_RMAX) return CE_ERR_ARG;
  if ((long long)H * W * 3 >= (1ll << 31) || (H + LF_T - 1) / LF_T > 65535) return CE_ERR_SHAPE;
  if ((((uintptr_t)AB | (uintptr_t)R) & 3) || ((uintptr_t)coef & 15)) return CE_ERR_ALIGN;
  const int S = LF_T + 2 * radius;
  const size_t lds = (size_t)(2 * S * S) * sizeof(int) + (size_t)S * LF_T * 2 * sizeof(long long);
  const dim3 grid((unsigned)((W + LF_T - 1) / LF_T), (unsigned)((H + LF_T - 1) / LF_T), (unsigned)F);
  hipLaunchKernelGGL(lift_smooth_kernel, grid, dim3(256), lds, stream, (const uint8_t*)L, (const uint8_t*)E, AB, coef, R, H, W, radius);
  return (int)hipGetLastError();
}

// ---- stage 3: the gate -----------------------------------------------------------------------------------------------------------------
// The box mean of R (a sum below 1089 * 65280 < 2^27: int32 holds it) -> g = clamp((mean - t0) / (t1 - t0), 0, 1) into slot 6 of the cell.
// The fp32 quotient is formed through double, which rounds a quotient of two fp32 values as an fp32 division does (53 >= 2 * 24 + 2).
__global__ __launch_bounds__(256) void lift_gate_kernel(const int* __restrict__ R, float* __restrict__ coef, int H, int W, int r, float t0, float t1) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) int lf_smem[];
  const int S = LF_T + 2 * r;
  int* vr = lf_smem;      // [S][S]
  int* hs = vr + S * S;   // [S][LF_T]
  const int t = threadIdx.x, f = blockIdx.z;
  const int x0 = blockIdx.x * LF_T, y0 = blockIdx.y * LF_T;
  const int ty = t / LF_T, tx = t - ty * LF_T;
  const int y = y0 + ty, x = x0 + tx;
  const size_t plane = (size_t)H * W;
  const int* Rf = R + (size_t)f * plane;
  for (int i = t; i < S * S; i += 256) {
    const int ly = i / S, lx = i - ly * S;
    const int gy = y0 - r + ly, gx = x0 - r + lx;
    vr[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? Rf[(size_t)gy * W + gx] : 0;
  }
  __syncthreads();
  for (int i = t; i < S * LF_T; i += 256) {
    const int ly = i / LF_T, ox = i - ly * LF_T;
    const int* p = vr + ly * S + ox;
    int s = 0;
    for (int k = 0; k <= 2 * r; ++k) s += p[k];
    hs[i] = s;
  }
  __syncthreads();
  if (y < H && x < W) {
    int s = 0;
    for (int k = 0; k <= 2 * r; ++k) s += hs[(ty + k) * LF_T + tx];
    const float m = (float)((double)s / (double)(lf_span(y, r, H) * lf_span(x, r, W) * 256));
    const float up = m - t0;
    const float dn = t1 - t0;
    const float g = (float)((double)up / (double)dn);
    coef[(f * plane + (size_t)y * W + x) * LF_CELL + 6] = fminf(fmaxf(g, 0.0f), 1.0f);
  }
}

CE_API int ce_lift_gate_f32(const int* R, float* coef, int F, int H, int W, int radius, float t0, float t1, hipStream_t stream) {
  if (!R || !coef || F <= 0 || F > 65535 || H <= 0 || W <= 0 || radius < 1 || radius > LF_RMAX) return CE_ERR_ARG;
  if (!(t0 >= 0.0f && t1 > t0 && t1 < INFINITY)) return CE_ERR_ARG;
  if ((long long)H * W * 3 >= (1ll << 31) || (H + LF_T - 1) / LF_T > 65535) return CE_ERR_SHAPE;
  if (((uintptr_t)R & 3) || ((uintptr_t)coef & 15)) return CE_ERR_ALIGN;
  const int S = LF_T + 2 * radius;
  const size_t lds = (size_t)(S * S + S * LF_T) * sizeof(int);
  const dim3 grid((unsigned)((W + LF_T - 1) / LF_T), (unsigned)((H + LF_T - 1) / LF_T), (unsigned)F);
  hipLaunchKernelGGL(lift_gate_kernel, grid, dim3(256), lds, stream, R, coef, H, W, radius, t0, t1);
  return (int)hipGetLastError();
}

// ---- stage 4: the apply ----------------------------------------------------------------------------------------------------------------
#define LA_PX 16            // pixels of one output frame a lane owns per round: 48 bytes, three 16-byte accesses
#define LA_B (3 * LA_PX)
#define LA_DW (LA_B / 4)
#define LA_MAX_WG 2048      // a memory-bound pass: at most about eight workgroups per CU, the rest by the grid stride

// LA_B bytes of a frame as LA_DW dwords: three 16-byte loads (WIDE), or nb single bytes
template <bool WIDE>
__device__ __forceinline__ void la_read(const uint8_t* __restrict__ p, int nb, uint32_t (&w)[LA_DW]) {
  if (WIDE) {  // (nb == LA_B on this path)
#pragma unroll
    for (int k = 0; k < LA_DW / 4; ++k) {
      const uint4 v = ((const uint4*)p)[k];
      w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < LA_DW; ++k) w[k] = 0;
#pragma unroll
    for (int j = 0; j < LA_B; ++j)
      if (j < nb) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
  }
}

// One lane per LA_PX consecutive pixels of one output frame (blockIdx.y = frame), rounds of gridDim.x * 256 groups: every lane starts on a
// pixel, so the pixel and colour of each of its bytes is known when the kernel is compiled.  The four corner cells stay in registers from
// pixel to pixel: along a row they change every SW / W pixels, and a step of one cell reuses the right pair as the left one - the
// coefficient grid is read from the L2 a few times per group, not four times per pixel.  a * (1 - t) + b * t is evaluated in the order of
// ce_preview_rgb_u8, 1 - t once per pixel and axis.  U is read only by a group that holds a pixel with g_up != 0 (g_up == 0 leaves q as it
// is: q + 0 * (U - q)).  WIDE (frame pixels % 16 == 0; P, U and out 16-byte aligned): 16-byte accesses; byte by byte otherwise.
template <bool WIDE>
__global__ __launch_bounds__(256) void lift_apply_kernel(const uint8_t* __restrict__ P, const uint8_t* __restrict__ U, const float* __restrict__ coef,
                                                         const int* __restrict__ ix0, const int* __restrict__ ix1, const float* __restrict__ txs,
                                                         const int* __restrict__ iy0, const int* __restrict__ iy1, const float* __restrict__ tys,
                                                         uint8_t* __restrict__ out, int SW, long long npx, int H, int W) {
#pragma clang fp contract(off)
  const int f = blockIdx.y;
  const float* cf = coef + (size_t)f * H * W * LF_CELL;
  const uint8_t* Uf = U ? U + (size_t)f * npx * 3 : nullptr;
  uint8_t* of = out + (size_t)f * npx * 3;
  const long long groups = (npx + LA_PX - 1) / LA_PX;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long p0 = gi * LA_PX, b0 = p0 * 3;
    const int np = (int)(npx - p0 < LA_PX ? npx - p0 : LA_PX), nb = 3 * np;
    uint32_t pw[LA_DW];
    la_read<WIDE>(P + b0, nb, pw);
    const int Y0 = (int)((uint32_t)p0 / (uint32_t)SW), X0 = (int)((uint32_t)p0 - (uint32_t)Y0 * (uint32_t)SW);  // (npx < 2^31 / 3)
    int X = X0, Y = Y0;
    // the column table entries of pixel i + 1 are asked for before pixel i is worked on: the loop never stops for them
    int nxa = ix0[X], nxb = ix1[X];
    float tx = txs[X];
    int xa = -1, xb = -1, ya = -1, yb = -1;
    LaCell c00, c01, c10, c11;
    float ty = 0.0f, sy = 0.0f;
    float q[LA_B], gq[LA_PX];
    bool any = false;
#pragma unroll
    for (int i = 0; i < LA_PX; ++i) {
      float v[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (i < np) {
        const int X1 = X + 1 == SW ? 0 : X + 1;
        int pxa = 0, pxb = 0;
        float ptx = 0.0f;
        if (i + 1 < np) pxa = ix0[X1], pxb = ix1[X1], ptx = txs[X1];
        nxa = min(max(nxa, 0), W - 1), nxb = min(max(nxb, 0), W - 1);
        if (i == 0 || X == 0) {  // a new row
          const int nya = min(max(iy0[Y], 0), H - 1), nyb = min(max(iy1[Y], 0), H - 1);
          if (nya != ya || nyb != yb) xa = xb = -1;  // (all four corners are reloaded below)
          ya = nya, yb = nyb;
          ty = tys[Y];
          sy = 1.0f - ty;
        }
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
        any = any || v[6] != 0.0f;
        nxa = pxa, nxb = pxb, tx = ptx;
        if ((X = X1) == 0) ++Y;
      }
      gq[i] = v[6];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int j = 3 * i + c;
        const float p = (float)((pw[j >> 2] >> (8 * (j & 3))) & 255u);
        q[j] = la_affine(v[c], v[3 + c], p);
      }
    }
    if (Uf && any) {
      uint32_t uw[LA_DW];
      la_read<WIDE>(Uf + b0, nb, uw);
#pragma unroll
      for (int j = 0; j < LA_B; ++j) q[j] = la_fallback(q[j], gq[j / 3], (float)((uw[j >> 2] >> (8 * (j & 3))) & 255u));
    }
    uint32_t ow[LA_DW];
#pragma unroll
    for (int k = 0; k < LA_DW; ++k) ow[k] = 0;
#pragma unroll
    for (int j = 0; j < LA_B; ++j) ow[j >> 2] |= la_byte(q[j]) << (8 * (j & 3));
    if (WIDE) {
#pragma unroll
      for (int k = 0; k < LA_DW / 4; ++k) ((uint4*)(of + b0))[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < LA_B; ++j)
        if (j < nb) of[b0 + j] = (uint8_t)(ow[j >> 2] >> (8 * (j & 3)));
    }
  }
}

CE_API int ce_lift_apply_u8(const void* P, const void* U, const float* coef, const int* ix0, const int* ix1, const float* tx, const int* iy0,
                            const int* iy1, const float* ty, void* out, int F, int SH, int SW, int H, int W, hipStream_t stream) {
  if (!P || !coef || !ix0 || !ix1 || !tx || !iy0 || !iy1 || !ty || !out || out == P || out == U) return CE_ERR_ARG;
  if (F <= 0 || F > 65535 || SH <= 0 || SW <= 0 || H <= 0 || W <= 0) return CE_ERR_ARG;
  const long long npx = (long long)SH * SW;
  if (npx * 3 >= (1ll << 31) || (long long)H * W * LF_CELL * (long long)sizeof(float) >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)coef & 15) || (((uintptr_t)ix0 | (uintptr_t)ix1 | (uintptr_t)tx | (uintptr_t)iy0 | (uintptr_t)iy1 | (uintptr_t)ty) & 3)) return CE_ERR_ALIGN;
  const long long need = ((npx + LA_PX - 1) / LA_PX + 255) / 256;
  long long gx = LA_MAX_WG / F;
  if (gx < 1) gx = 1;
  if (gx > need) gx = need;
  const dim3 grid((unsigned)gx, (unsigned)F);
  if (npx % LA_PX == 0 && !(((uintptr_t)P | (uintptr_t)U | (uintptr_t)out) & 15))
    hipLaunchKernelGGL(lift_apply_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)P, (const uint8_t*)U, coef, ix0, ix1, tx, iy0, iy1, ty,
                       (uint8_t*)out, SW, npx, H, W);
  else
    hipLaunchKernelGGL(lift_apply_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)P, (const uint8_t*)U, coef, ix0, ix1, tx, iy0, iy1, ty,
                       (uint8_t*)out, SW, npx, H, W);
  return (int)hipGetLastError();
}


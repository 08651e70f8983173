// Mask-aware detail lift (chronoedit_amd/rimlift.py is the definition): the first two grid passes of the lift inside a focus box, fitted
// under the region's weights.  A region edit leaves a tapered change d = w d* in a focused crop's frames (w = m / 255, m the edit-size
// weight plane); these passes fit the UNTAPERED map from it, so that the apply stage writes the edit at full strength and the paste's
// photo-size mask tapers it once.
//
//   ce_rimlift_fit_q16     L, E, M -> A, B = rint(65536 a), rint(65536 b) int32 [F][H][W][6]: the normal equations of 255 d ~ a (m I) + b m
//                          from exact integer box statistics
//   ce_rimlift_smooth_f32  A, B, M -> the m-weighted box means abar, bbar in the coefficient cells fp32 [F][H][W][8] (g and the pad zeroed),
//                          and the residual of the tapered model R = rint(256 min(res, 255)) int32 [F][H][W]
//
// ce_lift_gate_f32 and ce_boxlift_apply_paste_u8 follow, unchanged.  Both passes are bit-equal to their stage of rimlift.py and have the
// shape of csrc/ce_lift.hip: a 16 x 16 tile with its halo staged in the LDS, separable sums of integers (any order gives the same bits),
// every fp32 / fp64 multiply, add and subtract rounded on its own (`#pragma clang fp contract(off)`).  No state, nothing allocated, no
// host read: every call is capturable.
//
// What differs from ce_lift.hip is the width of the sums: with a weight in every term they no longer fit int32.  Per cell m <= 255,
// I <= 255, |d| <= 255, and a window holds at most 33 * 33 = 1089 cells:
//   T_q   = box(m m)      <= 1089 * 255^2 = 7.1e7    int32
//   T_md  = box(m d)      |.| <= 7.1e7               int32
//   T_qI  = box(m m I)    <= 1089 * 255^3 = 1.8e10   int64  (a row of 33 cells, 5.5e8, still fits int32: the horizontal pass adds in int32)
//   T_mId = box(m I d)    |.| <= 1.8e10              int64  (likewise)
//   T_qII = box(m m I I)  <= 1089 * 255^4 = 4.6e12   int64  (one cell reaches 4.2e9: the product itself is formed in 64 bits)
//   n_m   = box(m)        <= 1089 * 255 = 2.8e5      int32
//   box(m A), |A| <= 8 * 65536:     <= 1.5e11        int64  (one cell 1.3e8: an int32 product)
//   box(m B), |B| <= 4096 * 65536:  <= 7.5e13        int64  (one cell 6.8e10: a 64-bit product)
// All of them are below 2^53: the conversions to double are exact.
// The LDS is sized by the radius, as in ce_lift.hip; at the largest, r = 16, the staged side is 48 cells and a workgroup takes
// 48 * 48 * 4 + 48 * 16 * 32 = 33792 bytes (fit: m, I and d packed into one word per cell) or 48 * 48 * 9 + 48 * 16 * 24 = 39168 bytes
// (smooth) - below the 64 KiB a launch may ask for without an attribute, four workgroups per CU.
#include "ce_common.h"
#include "ce_lift_pixel.h"  // LF_CELL

#define RL_T 16      // a workgroup's tile: RL_T x RL_T cells, one lane per cell
#define RL_RMAX 16   // the largest radius: the staged side is RL_T + 2 r <= 48 cells
#define RL_BMAX 4096.0  // the bound of |b|: rint(65536 b) stays in int32 (rimlift.MAX_B)

struct RlFitRow {    // the horizontal sums of one staged row at one tile column
  long long qI, qII, mId;
  int q, md;
};
struct RlSmoothRow {
  long long a, b, n;
};

// ---- stage 1: the fit ------------------------------------------------------------------------------------------------------------------
// Per colour: the tile's (m, I, d) with the halo as one word per cell - m | I << 8 | (d + 255) << 16, and m = 0 outside the image, where
// every term vanishes with it -, the horizontal sums per staged row and tile column, then per lane the vertical sums and the two divisions.
__global__ __launch_bounds__(256) void rimlift_fit_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ E, const uint8_t* __restrict__ M,
                                                          int* __restrict__ AB, int H, int W, int r, int eps_q, float max_gain) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char rl_smem[];
  const int S = RL_T + 2 * r;
  RlFitRow* hs = (RlFitRow*)rl_smem;                              // [S][RL_T]
  unsigned* vc = (unsigned*)(rl_smem + (size_t)S * RL_T * sizeof(RlFitRow));  // [S][S]
  const int t = threadIdx.x, f = blockIdx.z;
  const int x0 = blockIdx.x * RL_T, y0 = blockIdx.y * RL_T;
  const int ty = t / RL_T, tx = t - ty * RL_T;
  const int y = y0 + ty, x = x0 + tx;
  const size_t plane = (size_t)H * W;
  const uint8_t* Ef = E + (size_t)f * plane * 3;
  for (int c = 0; c < 3; ++c) {
    for (int i = t; i < S * S; i += 256) {
      const int ly = i / S, lx = i - ly * S;
      const int gy = y0 - r + ly, gx = x0 - r + lx;
      unsigned v = 255u << 16;  // m = 0, I = 0, d = 0
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const size_t p = (size_t)gy * W + gx, o = p * 3 + c;
        const int I = L[o];
        v = (unsigned)M[p] | ((unsigned)I << 8) | ((unsigned)((int)Ef[o] - I + 255) << 16);
      }
      vc[i] = v;
    }
    __syncthreads();
    for (int i = t; i < S * RL_T; i += 256) {
      const int ly = i / RL_T, ox = i - ly * RL_T;
      const unsigned* pc = vc + ly * S + ox;
      int q = 0, md = 0, qI = 0, mId = 0;  // (a row of at most 33 cells: see the widths above)
      long long qII = 0;
      for (int k = 0; k <= 2 * r; ++k) {
        const unsigned v = pc[k];
        const int m = (int)(v & 255u), I = (int)((v >> 8) & 255u), d = (int)(v >> 16) - 255;
        const int mm = m * m, mI = m * I;
        q += mm, md += m * d, qI += mm * I, mId += mI * d;
        qII += (long long)mI * mI;
      }
      RlFitRow s;
      s.qI = qI, s.qII = qII, s.mId = mId, s.q = q, s.md = md;
      hs[i] = s;
    }
    __syncthreads();
    if (y < H && x < W) {
      long long qI = 0, qII = 0, mId = 0;
      int q = 0, md = 0;
      for (int k = 0; k <= 2 * r; ++k) {
        const RlFitRow v = hs[(ty + k) * RL_T + tx];
        qI += v.qI, qII += v.qII, mId += v.mId, q += v.q, md += v.md;
      }
      float a = 0.0f, b = 0.0f;
      if (q > 0) {
        // The sums are exact in double, the products are rounded.  I <= 255 gives T_qI^2 <= T_q T_qII <= 65025 T_q^2: the exact difference
        // is non-negative and the rounding error of its two products is below 2^-36 T_q^2, while the eps term is at least T_q^2 - more
        // than 2^30 times as much: den > 0.
        const double Tq = (double)q, Tmd = (double)md, TqI = (double)qI, TqII = (double)qII, TmId = (double)mId;
        const double p0 = Tq * TmId, p1 = TqI * Tmd;
        const double num = p0 - p1;
        const double p2 = Tq * TqII, p3 = TqI * TqI;
        const double var = p2 - p3;
        const double e0 = Tq * (double)eps_q;
        const double e1 = e0 * Tq;
        const double den = var + e1;
        const double n255 = num * 255.0;
        double qa = n255 / den;
        qa = fmin(fmax(qa, -(double)max_gain), (double)max_gain);
        a = (float)qa;
        const double u0 = Tmd * 255.0;
        const double u1 = (double)a * TqI;
        const double u = u0 - u1;
        double qb = u / Tq;
        qb = fmin(fmax(qb, -RL_BMAX), RL_BMAX);
        b = (float)qb;
      }
      int* o = AB + ((size_t)f * plane + (size_t)y * W + x) * 6;
      o[c] = (int)rintf(a * 65536.0f);
      o[3 + c] = (int)rintf(b * 65536.0f);
    }
    __syncthreads();
  }
}

CE_API int ce_rimlift_fit_q16(const void* L, const void* E, const void* M, int* AB, int F, int H, int W, int radius, int eps_q, float max_gain,
                              hipStream_t stream) {
  if (!L || !E || !M || !AB || F <= 0 || F > 65535 || H <= 0 || W <= 0) return CE_ERR_ARG;
  if (radius < 1 || radius > RL_RMAX || eps_q < 1 || eps_q > (1 << 30) || !(max_gain >= 1.0f && max_gain <= 8.0f)) return CE_ERR_ARG;
  if ((long long)H * W * 3 >= (1ll << 31) || (H + RL_T - 1) / RL_T > 65535) return CE_ERR_SHAPE;
  if ((uintptr_t)AB & 3) return CE_ERR_ALIGN;
  const int S = RL_T + 2 * radius;
  const size_t lds = (size_t)S * RL_T * sizeof(RlFitRow) + (size_t)S * S * sizeof(unsigned);
  const dim3 grid((unsigned)((W + RL_T - 1) / RL_T), (unsigned)((H + RL_T - 1) / RL_T), (unsigned)F);
  hipLaunchKernelGGL(rimlift_fit_kernel, grid, dim3(256), lds, stream, (const uint8_t*)L, (const uint8_t*)E, (const uint8_t*)M, AB, H, W, radius,
                     eps_q, max_gain);
  return (int)hipGetLastError();
}

// ---- stage 2: the weighted means of the maps and the residual of the tapered model ---------------------------------------------------------
// Per colour: A_c, B_c and m of the tile and its halo (m = 0 outside the image), the horizontal sums of m A, m B and m in int64, per lane
// the vertical sums, the two means and the colour's residual.  The lane then writes its whole cell (g = 0 and the pad) and R.
// w = fp32(m) / 255 is formed through double, which rounds a quotient of two fp32 values as an fp32 division does (53 >= 2 * 24 + 2).
__global__ __launch_bounds__(256) void rimlift_smooth_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ E, const uint8_t* __restrict__ M,
                                                             const int* __restrict__ AB, float* __restrict__ coef, int* __restrict__ R, int H, int W,
                                                             int r) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char rl_smem[];
  const int S = RL_T + 2 * r;
  RlSmoothRow* hs = (RlSmoothRow*)rl_smem;                        // [S][RL_T]
  int* va = (int*)(rl_smem + (size_t)S * RL_T * sizeof(RlSmoothRow));  // [S][S]
  int* vb = va + S * S;                                           // [S][S]
  uint8_t* vm = (uint8_t*)(vb + S * S);                           // [S][S]
  const int t = threadIdx.x, f = blockIdx.z;
  const int x0 = blockIdx.x * RL_T, y0 = blockIdx.y * RL_T;
  const int ty = t / RL_T, tx = t - ty * RL_T;
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
      int a = 0, b = 0, m = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const size_t p = (size_t)gy * W + gx;
        a = ABf[p * 6 + c];
        b = ABf[p * 6 + 3 + c];
        m = M[p];
      }
      va[i] = a;
      vb[i] = b;
      vm[i] = (uint8_t)m;
    }
    __syncthreads();
    for (int i = t; i < S * RL_T; i += 256) {
      const int ly = i / RL_T, ox = i - ly * RL_T;
      const int* pa = va + ly * S + ox;
      const int* pb = vb + ly * S + ox;
      const uint8_t* pm = vm + ly * S + ox;
      RlSmoothRow s = {0, 0, 0};
      for (int k = 0; k <= 2 * r; ++k) {
        const long long m = pm[k];
        s.a += m * pa[k], s.b += m * pb[k], s.n += m;
      }
      hs[i] = s;
    }
    __syncthreads();
    if (inside) {
      long long sa = 0, sb = 0, n = 0;
      for (int k = 0; k <= 2 * r; ++k) {
        const RlSmoothRow v = hs[(ty + k) * RL_T + tx];
        sa += v.a, sb += v.b, n += v.n;
      }
      float abar = 0.0f, bbar = 0.0f;
      if (n > 0) {
        const double den = (double)(n * 65536);
        abar = (float)((double)sa / den), bbar = (float)((double)sb / den);
      }
      mean[c] = abar;
      mean[3 + c] = bbar;
      const size_t p = (size_t)y * W + x, o = p * 3 + c;
      const int I = L[o];
      const int d = (int)E[(size_t)f * plane * 3 + o] - I;
      const float w = (float)((double)(float)M[p] / 255.0);
      const float m = abar * (float)I;
      const float u = m + bbar;
      const float e = u * w;
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

CE_API int ce_rimlift_smooth_f32(const void* L, const void* E, const void* M, const int* AB, float* coef, int* R, int F, int H, int W, int radius,
                                 hipStream_t stream) {
  if (!L || !E || !M || !AB || !coef || !R || F <= 0 || F > 65535 || H <= 0 || W <= 0 || radius < 1 || radius > RL_RMAX) return CE_ERR_ARG;
  if ((long long)H * W * 3 >= (1ll << 31) || (H + RL_T - 1) / RL_T > 65535) return CE_ERR_SHAPE;
  if ((((uintptr_t)AB | (uintptr_t)R) & 3) || ((uintptr_t)coef & 15)) return CE_ERR_ALIGN;
  const int S = RL_T + 2 * radius;
  const size_t lds = (size_t)S * RL_T * sizeof(RlSmoothRow) + (size_t)S * S * (2 * sizeof(int) + 1);
  const dim3 grid((unsigned)((W + RL_T - 1) / RL_T), (unsigned)((H + RL_T - 1) / RL_T), (unsigned)F);
  hipLaunchKernelGGL(rimlift_smooth_kernel, grid, dim3(256), lds, stream, (const uint8_t*)L, (const uint8_t*)E, (const uint8_t*)M, AB, coef, R, H,
                     W, radius);
  return (int)hipGetLastError();
}

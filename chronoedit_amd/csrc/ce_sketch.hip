// Sketch edits (chronoedit_amd/sketch.py): the region of an edit drawn on the photo is where the editor's composite differs from its
// background, grown and feathered AT THE PHOTO'S SIZE.  sketch.reference is the definition; every pass here is bit-equal to its stage.
//
//   ce_sketch_changed_u8   two RGB images -> the 0 / 255 plane: 255 where max over the channels of |composite - background| > threshold
//   ce_sketch_dilate_u8    one axis of the square maximum filter of a 0 / 255 plane, window [i - R, i + R] clipped to the image.  The input
//                          is binary by construction, so the pass COUNTS: out = 255 where the window holds a non-zero byte, else 0
//   ce_sketch_box_u8       one axis of the box mean, window [i - f, i + f] over the edge-replicated line: acc = the integer sum, n = 2 f + 1,
//                          ww = 2^24 / n (integer), out = (acc * ww + 2^23) >> 24 - PIL's BoxBlur for an integer radius
//
// Both filters are window SUMS, and neither costs more per pixel as the window grows:
//   horizontal  one workgroup per (row, run of SK_CHUNK output bytes): the run's input with its two halos is read once, coalesced, and its
//               exclusive prefix sum is built in the LDS (per lane four bytes, a wave scan by shuffles, the four wave totals through the LDS);
//               a window sum is then E[hi] - E[lo], two LDS reads whatever the radius.
//   vertical    one lane per four adjacent columns (a wave reads 256 consecutive bytes of a row) and per segment of 32 rows: the window sum
//               of the segment's first row is gathered once (the halo), then every next row adds the row entering the window and subtracts
//               the row leaving it.  The halo of a window of more than 128 rows is gathered from per-segment sums that a first launch writes
//               to the caller's scratch, so that neither the loads per output nor the chain of loads of one lane follow the radius, and the
//               grid is SW / 4 x SH / 32 lanes at every radius.
// Integers only: the result is exact and does not depend on the launch order.  No state; the one scratch is the caller's.
#include "ce_common.h"

#define SK_CHUNK 4096  // output bytes of one row per workgroup of the horizontal passes
#define SK_SUB 1024    // input bytes per scan round: 256 lanes x 4

// ---- changed ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sk_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

__device__ __forceinline__ uint32_t sk_byte(const uint32_t* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

// One lane per 16 pixels: 48 bytes of each image.  WIDE (all three bases 16-byte aligned): three 16-byte loads per image and one 16-byte
// store for every whole group; the last, partial group - and everything when a base is unaligned - goes byte by byte.
template <bool WIDE>
__global__ __launch_bounds__(256) void sketch_changed_kernel(const uint8_t* __restrict__ bg, const uint8_t* __restrict__ cp, uint8_t* __restrict__ out,
                                                             long long n, uint32_t thr) {
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (p0 >= n) return;
  if (WIDE && p0 + 16 <= n) {
    uint32_t a[12], b[12], o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const u32x4 va = *(const u32x4*)(bg + p0 * 3 + 16 * j), vb = *(const u32x4*)(cp + p0 * 3 + 16 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) a[4 * j + k] = va[k], b[4 * j + k] = vb[k];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t d = max(max(sk_absdiff(sk_byte(a, 3 * i), sk_byte(b, 3 * i)), sk_absdiff(sk_byte(a, 3 * i + 1), sk_byte(b, 3 * i + 1))),
                             sk_absdiff(sk_byte(a, 3 * i + 2), sk_byte(b, 3 * i + 2)));
      if (d > thr) o[i >> 2] |= 255u << ((i & 3) * 8);
    }
    u32x4 v;
    v[0] = o[0], v[1] = o[1], v[2] = o[2], v[3] = o[3];
    *(u32x4*)(out + p0) = v;
  } else {
    const int np = (int)(n - p0 < 16 ? n - p0 : 16);
    for (int i = 0; i < np; ++i) {
      const uint8_t* x = bg + (p0 + i) * 3;
      const uint8_t* y = cp + (p0 + i) * 3;
      const uint32_t d = max(max(sk_absdiff(x[0], y[0]), sk_absdiff(x[1], y[1])), sk_absdiff(x[2], y[2]));
      out[p0 + i] = d > thr ? 255 : 0;
    }
  }
}

CE_API int ce_sketch_changed_u8(const void* background, const void* composite, void* out, long long pixels, int threshold, hipStream_t stream) {
  if (!background || !composite || !out || out == background || out == composite) return CE_ERR_ARG;
  if (pixels <= 0 || threshold < 0 || threshold > 254) return CE_ERR_ARG;
  if (pixels * 3 >= (1ll << 31)) return CE_ERR_SHAPE;
  const dim3 grid((unsigned)(((pixels + 15) / 16 + 255) / 256));
  if (!(((uintptr_t)background | (uintptr_t)composite | (uintptr_t)out) & 15))
    hipLaunchKernelGGL(sketch_changed_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)background, (const uint8_t*)composite, (uint8_t*)out, pixels,
                       (uint32_t)threshold);
  else
    hipLaunchKernelGGL(sketch_changed_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)background, (const uint8_t*)composite, (uint8_t*)out, pixels,
                       (uint32_t)threshold);
  return (int)hipGetLastError();
}

// ---- the two filters ----------------------------------------------------------------------------------------------------------------
// What a byte adds to a window sum: itself (BOX), or whether it is set (dilation)
template <bool BOX>
__device__ __forceinline__ uint32_t sk_term(uint32_t byte) {
  return BOX ? byte : (byte ? 1u : 0u);
}

// The output byte of a window sum
template <bool BOX>
__device__ __forceinline__ uint32_t sk_result(uint32_t acc, uint32_t ww) {
  return BOX ? (uint32_t)(((unsigned long long)acc * ww + (1ull << 23)) >> 24) : (acc ? 255u : 0u);
}

// Horizontal.  blockIdx.x = row * chunks + chunk.  The chunk's outputs are x in [c0, c0 + cc); their windows read the line positions
// [c0 - r, c0 + cc + r), of which those outside [0, W) count as 0 here (BOX adds the replicated edge bytes per output below).  The scan starts at
// `off` <= c0 - r, moved down so that row + off is 4-byte aligned: E[k] = the sum of the terms of positions [off, off + k).  E holds
// rounds * SK_SUB entries (dynamic LDS, sized by the launch), rounds covering k up to c0 + cc + r - off.
// WIDE_OUT (W % 4 == 0 and dst 4-byte aligned): four outputs leave as one dword.
template <bool BOX, bool WIDE_OUT>
__global__ __launch_bounds__(256) void sketch_row_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int chunks, int r, uint32_t ww,
                                                         int rounds) {
  extern __shared__ __attribute__((aligned(16))) uint32_t E[];
  __shared__ uint32_t wave_total[2][4];
  const int y = blockIdx.x / chunks;
  const int c0 = (blockIdx.x - y * chunks) * SK_CHUNK;
  const int cc = min(SK_CHUNK, W - c0);
  const uint8_t* row = src + (size_t)y * W;
  const int off = (c0 - r) - (int)(((uintptr_t)row + (uintptr_t)(long long)(c0 - r)) & 3u);  // (two's complement: right for a negative c0 - r too)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t carry = 0;
  for (int s = 0; s < rounds; ++s) {
    const int k0 = s * SK_SUB + 4 * t;
    const int p = off + k0;
    uint32_t v[4] = {0, 0, 0, 0};
    if (p >= 0 && p + 4 <= W) {
      const uint32_t q = *(const uint32_t*)(row + p);  // (aligned: row + off is, and k0 is a multiple of 4)
      v[0] = sk_term<BOX>(q & 255u), v[1] = sk_term<BOX>((q >> 8) & 255u), v[2] = sk_term<BOX>((q >> 16) & 255u), v[3] = sk_term<BOX>(q >> 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p + j >= 0 && p + j < W) v[j] = sk_term<BOX>(row[p + j]);
    }
    const uint32_t mine = v[0] + v[1] + v[2] + v[3];
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[s & 1][wave] = incl;
    __syncthreads();  // (one barrier per round: the totals alternate between two slots)
    uint32_t before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t wt = wave_total[s & 1][w];
      if (w < wave) before += wt;
      all += wt;
    }
    carry += all;
    const uint32_t e0 = before + incl - mine;
    u32x4 e;
    e[0] = e0, e[1] = e0 + v[0], e[2] = e[1] + v[1], e[3] = e[2] + v[2];
    *(u32x4*)(E + k0) = e;
  }
  __syncthreads();
  const uint32_t first = BOX ? row[0] : 0u, last = BOX ? row[W - 1] : 0u;
  uint8_t* drow = dst + (size_t)y * W;
  for (int q = 4 * t; q < cc; q += SK_SUB) {
    uint32_t o[4] = {0, 0, 0, 0};
    const int nb = min(4, cc - q);
    for (int j = 0; j < nb; ++j) {
      const int x = c0 + q + j;
      uint32_t acc = E[x + r + 1 - off] - E[x - r - off];
      if (BOX) acc += first * (uint32_t)max(r - x, 0) + last * (uint32_t)max(x + r - (W - 1), 0);
      o[j] = sk_result<BOX>(acc, ww);
    }
    if (WIDE_OUT) {  // (cc is a multiple of 4 on this path: nb == 4)
      *(uint32_t*)(drow + c0 + q) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
    } else {
      for (int j = 0; j < nb; ++j) drow[c0 + q + j] = (uint8_t)o[j];
    }
  }
}

// Vertical.  blockIdx.x = segment * gx + column block; a lane owns four adjacent columns and the SK_SEG rows [y0, y0 + SK_SEG) of them, so a
// wave reads 256 consecutive bytes of a row.  WIDE (W % 4 == 0, all bases aligned): one aligned dword per row and lane; otherwise (a cropped
// photo's width, say) four byte accesses per row and lane into the same 256 bytes, the columns past W masked.  Rows outside [0, H) count as
// 0 in the running sum; BOX adds the replicated edge rows per output.
// The segment's first window [y0 - r, y0 + r] is summed once, row by row - or, BLOCKED (windows of more than 128 rows), from the sums of
// whole segments that a first launch leaves in the caller's scratch (uint16 [segments][W]: at most 32 x 255), with single rows only at the
// window's two ends: fewer than 64 row loads and (2 r + 1) / 32 eight-byte loads at any radius.
#define SK_SEG 32

template <bool WIDE>
__device__ __forceinline__ void sk_load4(const uint8_t* __restrict__ src, int W, int x0, int y, uint32_t* v) {
  if constexpr (WIDE) {
    const uint32_t q = *(const uint32_t*)(src + (size_t)y * W + x0);
    v[0] = q & 255u, v[1] = (q >> 8) & 255u, v[2] = (q >> 16) & 255u, v[3] = q >> 24;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = x0 + c < W ? src[(size_t)y * W + x0 + c] : 0u;
  }
}

// sums[j][x] = the sum of the terms of rows [j SK_SEG, min((j + 1) SK_SEG, H)) of column x
template <bool BOX, bool WIDE>
__global__ __launch_bounds__(64) void sketch_col_sums_kernel(const uint8_t* __restrict__ src, uint16_t* __restrict__ sums, int H, int W, int gx) {
  const int sg = blockIdx.x / gx;
  const int x0 = ((blockIdx.x - sg * gx) * 64 + threadIdx.x) * 4;
  if (x0 >= W) return;
  const int y0 = sg * SK_SEG, y1 = min(y0 + SK_SEG, H);
  uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll 8
  for (int y = y0; y < y1; ++y) {
    uint32_t v[4];
    sk_load4<WIDE>(src, W, x0, y, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += sk_term<BOX>(v[c]);
  }
  uint16_t* o = sums + (size_t)sg * W + x0;
  if constexpr (WIDE) {
    u32x2 q;
    q[0] = acc[0] | acc[1] << 16, q[1] = acc[2] | acc[3] << 16;
    *(u32x2*)o = q;  // (8-byte aligned: W % 4 == 0, x0 % 4 == 0, the scratch is)
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (x0 + c < W) o[c] = (uint16_t)acc[c];
  }
}

template <bool BOX, bool WIDE, bool BLOCKED>
__global__ __launch_bounds__(64) void sketch_col_kernel(const uint8_t* __restrict__ src, const uint16_t* __restrict__ sums, uint8_t* __restrict__ dst, int H,
                                                        int W, int gx, int r, uint32_t ww) {
  constexpr int COLS = 4;
  const int sg = blockIdx.x / gx;
  const int x0 = ((blockIdx.x - sg * gx) * 64 + threadIdx.x) * COLS;
  if (x0 >= W) return;
  const int y0 = sg * SK_SEG, y1 = min(y0 + SK_SEG, H);
  uint32_t acc[COLS], first[COLS], last[COLS];
#pragma unroll
  for (int c = 0; c < COLS; ++c) acc[c] = first[c] = last[c] = 0;
  auto add_rows = [&](int ya, int yb) {  // rows [ya, yb), all inside the image
#pragma unroll 4
    for (int y = ya; y < yb; ++y) {
      uint32_t v[COLS];
      sk_load4<WIDE>(src, W, x0, y, v);
#pragma unroll
      for (int c = 0; c < COLS; ++c) acc[c] += sk_term<BOX>(v[c]);
    }
  };
  if (BOX) sk_load4<WIDE>(src, W, x0, 0, first), sk_load4<WIDE>(src, W, x0, H - 1, last);
  const int wa = max(y0 - r, 0), wb = min(y0 + r, H - 1) + 1;  // the first row's window, clipped: rows [wa, wb)
  if constexpr (BLOCKED) {
    const int nseg = (H + SK_SEG - 1) / SK_SEG;
    const int ja = (wa + SK_SEG - 1) / SK_SEG;          // the first segment that starts inside the window
    const int jb = wb == H ? nseg : wb / SK_SEG;        // one past the last segment that ends inside it (the image's last one may be short)
    if (ja < jb) {
      add_rows(wa, ja * SK_SEG);
#pragma unroll 4
      for (int j = ja; j < jb; ++j) {
        const uint16_t* p = sums + (size_t)j * W + x0;
        if constexpr (WIDE) {
          const u32x2 q = *(const u32x2*)p;
          acc[0] += q[0] & 0xFFFFu, acc[1] += q[0] >> 16, acc[2] += q[1] & 0xFFFFu, acc[3] += q[1] >> 16;
        } else {
#pragma unroll
          for (int c = 0; c < COLS; ++c) acc[c] += x0 + c < W ? (uint32_t)p[c] : 0u;
        }
      }
      add_rows(min(jb * SK_SEG, wb), wb);
    } else {
      add_rows(wa, wb);
    }
  } else {
    add_rows(wa, wb);
  }
#pragma unroll 4
  for (int y = y0; y < y1; ++y) {
    uint32_t o[COLS];
    const uint32_t below = (uint32_t)max(r - y, 0), above = (uint32_t)max(y + r - (H - 1), 0);
#pragma unroll
    for (int c = 0; c < COLS; ++c) o[c] = sk_result<BOX>(BOX ? acc[c] + first[c] * below + last[c] * above : acc[c], ww);
    if constexpr (WIDE)
      *(uint32_t*)(dst + (size_t)y * W + x0) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
    else {
#pragma unroll
      for (int c = 0; c < COLS; ++c)
        if (x0 + c < W) dst[(size_t)y * W + x0 + c] = (uint8_t)o[c];
    }
    // the next row's window: row y + r + 1 enters, row y - r leaves.  Both loads are unconditional, from a row clamped into the image and
    // weighted 0 when the row lies outside it, so that the loads of several iterations are in flight at once
    const int enter = y + r + 1, leave = y - r;
    const uint32_t we = enter < H ? 1u : 0u, wl = leave >= 0 ? 1u : 0u;
    uint32_t ve[COLS], vl[COLS];
    sk_load4<WIDE>(src, W, x0, min(enter, H - 1), ve), sk_load4<WIDE>(src, W, x0, max(leave, 0), vl);
#pragma unroll
    for (int c = 0; c < COLS; ++c) acc[c] += we * sk_term<BOX>(ve[c]) - wl * sk_term<BOX>(vl[c]);
  }
}

// The scratch a vertical pass of this radius needs: none while the window holds at most 128 rows
static size_t sketch_scratch_bytes(int H, int W, int axis, int radius) {
  if (axis != 1 || 2 * radius + 1 <= 4 * SK_SEG) return 0;
  return (size_t)((H + SK_SEG - 1) / SK_SEG) * (size_t)W * sizeof(uint16_t);
}

template <bool BOX>
static int sketch_filter(const void* src, void* dst, int H, int W, int axis, int radius, int max_radius, void* scratch, size_t scratch_bytes,
                         hipStream_t stream) {
  if (!src || !dst || src == dst) return CE_ERR_ARG;
  if (H <= 0 || W <= 0 || axis < 0 || axis > 1 || radius < 0 || radius > max_radius) return CE_ERR_ARG;
  if ((long long)H * W >= (1ll << 31)) return CE_ERR_SHAPE;
  const size_t need = sketch_scratch_bytes(H, W, axis, radius);
  if (need && (!scratch || scratch_bytes < need || scratch == src || scratch == dst)) return CE_ERR_ARG;
  if (need && ((uintptr_t)scratch & 7)) return CE_ERR_ALIGN;
  const uint32_t ww = (1u << 24) / (uint32_t)(2 * radius + 1);
  const uint8_t* s = (const uint8_t*)src;
  uint8_t* d = (uint8_t*)dst;
  if (axis == 0) {
    const int chunks = (W + SK_CHUNK - 1) / SK_CHUNK;
    // E's last index is c0 + cc + r - off with off >= c0 - r - 3: at most min(W, SK_CHUNK) + 2 r + 3
    const int rounds = (min(W, SK_CHUNK) + 2 * radius + 3 + SK_SUB) / SK_SUB;
    const size_t lds = (size_t)rounds * SK_SUB * sizeof(uint32_t);  // (<= 13 rounds = 52 KiB at the largest radius)
    const dim3 grid((unsigned)((long long)H * chunks));
    if (W % 4 == 0 && !((uintptr_t)d & 3))
      hipLaunchKernelGGL((sketch_row_kernel<BOX, true>), grid, dim3(256), lds, stream, s, d, W, chunks, radius, ww, rounds);
    else
      hipLaunchKernelGGL((sketch_row_kernel<BOX, false>), grid, dim3(256), lds, stream, s, d, W, chunks, radius, ww, rounds);
  } else {
    // per output: two loads for the running sum and 1 / 32 of the first window's cost.  Windows up to 128 rows are summed row by row (2 to 6
    // loads per output); longer ones from the segment sums (one more load per output to make them, then < 64 rows and (2 r + 1) / 32
    // eight-byte loads per 32 outputs).  The grid is the same at every radius: one lane per four columns and 32 rows.
    const int segs = (H + SK_SEG - 1) / SK_SEG;
    const int gx = ((W + 3) / 4 + 63) / 64;
    const dim3 grid((unsigned)((long long)segs * gx));
    const bool wide = W % 4 == 0 && !(((uintptr_t)s | (uintptr_t)d) & 3);
    uint16_t* sums = (uint16_t*)scratch;
    if (need) {
      if (wide) {
        hipLaunchKernelGGL((sketch_col_sums_kernel<BOX, true>), grid, dim3(64), 0, stream, s, sums, H, W, gx);
        hipLaunchKernelGGL((sketch_col_kernel<BOX, true, true>), grid, dim3(64), 0, stream, s, (const uint16_t*)sums, d, H, W, gx, radius, ww);
      } else {
        hipLaunchKernelGGL((sketch_col_sums_kernel<BOX, false>), grid, dim3(64), 0, stream, s, sums, H, W, gx);
        hipLaunchKernelGGL((sketch_col_kernel<BOX, false, true>), grid, dim3(64), 0, stream, s, (const uint16_t*)sums, d, H, W, gx, radius, ww);
      }
    } else if (wide) {
      hipLaunchKernelGGL((sketch_col_kernel<BOX, true, false>), grid, dim3(64), 0, stream, s, (const uint16_t*)nullptr, d, H, W, gx, radius, ww);
    } else {
      hipLaunchKernelGGL((sketch_col_kernel<BOX, false, false>), grid, dim3(64), 0, stream, s, (const uint16_t*)nullptr, d, H, W, gx, radius, ww);
    }
  }
  return (int)hipGetLastError();
}

CE_API int ce_sketch_dilate_u8(const void* src, void* dst, int H, int W, int axis, int radius, void* scratch, size_t scratch_bytes, hipStream_t stream) {
  return sketch_filter<false>(src, dst, H, W, axis, radius, 4096, scratch, scratch_bytes, stream);
}

CE_API int ce_sketch_box_u8(const void* src, void* dst, int H, int W, int axis, int radius, void* scratch, size_t scratch_bytes, hipStream_t stream) {
  return sketch_filter<true>(src, dst, H, W, axis, radius, 1024, scratch, scratch_bytes, stream);
}

// Host arithmetic of the large-tile GEMM launchers: the split-K plan of the last round and the encoding of K-segmented operands.
// Pure functions of their arguments - no HIP header, no runtime call (the CU count comes in as an argument) - so that
// tools/gemm_plan_host_check.cpp checks them against brute force without a GPU.
#pragma once
#include <stdint.h>

// error codes returned by every extern "C" launcher (include/chronoedit_hip.h)
#define CE_OK 0
#define CE_ERR_ARG (-1)
#define CE_ERR_SHAPE (-2)
#define CE_ERR_ALIGN (-3)

// Split-K plan of the large-tile GEMMs: the `tail` workgroups of a partially filled last round (tiles % cus) are cut along K into `split`
// pieces, each writing an fp32 slab of slab_bytes that a second launch sums.  The largest split <= min(cus / tail, 8) that gives every piece
// an even number of the kt K-tiles and whose slabs fit in ws_bytes (0: no scratch); 1: the tail runs whole.
inline int ce_split_k(int tail, int kt, int cus, long long slab_bytes, long long ws_bytes) {
  if (tail <= 0) return 1;
  for (int s = cus / tail < 8 ? cus / tail : 8; s >= 2; --s)
    if (kt % (2 * s) == 0 && tail * s * slab_bytes <= ws_bytes) return s;
  return 1;
}

// What a launcher, its kernel and its reduce kernel agree on: workgroups [0, t_full) take whole tiles, workgroup t_full + i * split + s takes
// piece s of tail tile t_full + i and writes slab i * split + s of the scratch; reduce_grid workgroups (one per 128 x 128 quadrant of a tail
// tile) sum the slabs.  tail == 0 and split == 1 when the last round runs whole; last_round is its fill (tiles % cus) either way.
struct CeGemmPlan {
  int tiles_m, tiles_n, last_round, t_full, tail, split, grid, reduce_grid;
};
// may_split == false: a form with no reduce kernel (the transposed store, the two-level segmented operand) or a caller that found the cut
// does not pay.  ws_bytes: the scratch the caller passed, 0 without one.
inline CeGemmPlan ce_gemm_plan(int M, int N, int bm, int bn, int kt, int cus, long long ws_bytes, bool may_split) {
  CeGemmPlan p;
  p.tiles_m = (M + bm - 1) / bm;
  p.tiles_n = (N + bn - 1) / bn;
  const long long nwg = (long long)p.tiles_m * p.tiles_n;
  p.last_round = (int)(nwg % cus);
  p.split = may_split ? ce_split_k(p.last_round, kt, cus, (long long)bm * bn * sizeof(float), ws_bytes) : 1;
  p.tail = p.split == 1 ? 0 : p.last_round;
  p.t_full = (int)(nwg - p.tail);
  p.grid = p.t_full + p.tail * p.split;
  p.reduce_grid = 4 * p.tail;
  return p;
}

// K-segmented operand of the large-tile GEMMs: the kernels find the segment of K-tile t as (t * magic) >> 16, i.e. t / tps for tps = seg_k / bk
// K-tiles per segment.  The magic when seg_k is a whole number of K-tiles and the product is exact for every t < kt, 0 otherwise.
inline uint32_t ce_seg_magic(int seg_k, int bk, int kt) {
  if (seg_k <= 0 || seg_k % bk) return 0;
  const int tps = seg_k / bk;
  const uint32_t magic = 65536u / (uint32_t)tps + 1u;
  for (int t = 0; t < kt; ++t)
    if ((int)((uint32_t)t * magic >> 16) != t / tps) return 0;
  return magic;
}

// Column k of a segmented bf16 operand lives at (k / seg_k) * seg_stride + k % seg_k (elements), so K-tile t starts at byte
// t * bk * 2 + ((t * magic) >> 16) * extra, extra = (seg_stride - seg_k) * 2.  Which register holds that sum decides how far it may reach:
//   CE_SEG_U32_EXTRA   stage_half (ce_gemm256.hip) forms ((t * magic) >> 16) * extra in an unsigned 32-bit term and adds t * bk * 2 and the
//                      base in 64 bits: extra times the segment boundaries at or below K (K / seg_k) stays below 2^32;
//   CE_SEG_I32_OFFSET  koff (ce_gemm256w4.hip, ce_gemm384.hip) keeps the whole K-tile offset in a signed int, the scalar offset of a buffer
//                      load: extra times the segments K columns touch (ceil(K / seg_k)) plus the K * 2 bytes of a row stays below 2^31.
// Both bounds are taken at column K, not at the start of the last K-tile: the signed one charges one segment and one K-tile more than the
// largest offset a kernel forms, the unsigned one a segment more when K % seg_k == 0 - a DMA address that wraps is not worth that margin.
// (K / seg_k and ceil(K / seg_k) differ only when K % seg_k != 0, which ce_gemm_bf16_res rejects and the convolutions'
// ce_gemm256w4_seg2_launch does not.)
enum CeSegWidth { CE_SEG_U32_EXTRA, CE_SEG_I32_OFFSET };
struct CeSeg {
  uint32_t magic = 0, extra = 0;  // 0, 0: a plain row-major operand
};
// seg_k <= 0 or >= K: plain (CE_OK, seg untouched).  CE_ERR_SHAPE: seg_k is no whole number of K-tiles, the stride is shorter than the
// segment, or the offset does not fit its register.
inline int ce_seg_encode(int seg_k, long long seg_stride, int K, int bk, int kt, CeSegWidth width, CeSeg& seg) {
  if (seg_k <= 0 || seg_k >= K) return CE_OK;
  const uint32_t magic = ce_seg_magic(seg_k, bk, kt);
  const long long extra = (seg_stride - seg_k) * 2;  // bytes on top of the contiguous advance
  if (!magic || extra < 0) return CE_ERR_SHAPE;
  if (width == CE_SEG_U32_EXTRA ? extra * (K / seg_k) >= (1ll << 32) : extra * ((K + seg_k - 1) / seg_k) + (long long)K * 2 >= (1ll << 31))
    return CE_ERR_SHAPE;
  seg.magic = magic;
  seg.extra = (uint32_t)extra;
  return CE_OK;
}

// Second level of a two-level segmented A (ce_gemm256w4_seg2_launch): column k lives at (k / seg2_k) * seg2_stride + ((k % seg2_k) / seg_k) *
// seg_stride + k % seg_k, seg2_k a multiple of seg_k (the caller checks).  koff_a (ce_gemm256w4.hip) adds ((t * magic2) >> 16) * extra2 to the
// first level's signed offset - which has already advanced seg2_k / seg_k first-level strides per second-level segment, hence the difference
// in extra2.  The reach - last second-level segment, all of its first-level segments, one segment's columns - stays below 2^31.
inline int ce_seg2_encode(int seg_k, long long seg_stride, int seg2_k, long long seg2_stride, int K, int bk, int kt, CeSeg& seg2) {
  if (seg2_k >= K) return CE_OK;
  const uint32_t magic = ce_seg_magic(seg2_k, bk, kt);
  if (!magic) return CE_ERR_SHAPE;
  const long long inner = (long long)(seg2_k / seg_k) * seg_stride;
  const long long extra = (seg2_stride - inner) * 2;
  const long long reach = ((long long)(K - 1) / seg2_k) * seg2_stride * 2 + inner * 2 + (long long)seg_k * 2;
  if (extra < 0 || reach >= (1ll << 31)) return CE_ERR_SHAPE;
  seg2.magic = magic;
  seg2.extra = (uint32_t)extra;
  return CE_OK;
}

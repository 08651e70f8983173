// csrc/ce_gemm_plan.h against brute force, on the host - built by tools/gemm_plan_host_check.py (and tests/test_host_cpu.py) with
// -fsanitize=address,undefined; no HIP, no GPU.  What it shows: for every segmented operand the header accepts, the K-tile offsets the kernels
// form (their registers' widths emulated) are the operand's definition and fit; every operand it rejects breaks a rule the header states; every
// last-round plan is consistent with what the kernels, the reduce kernels and the slab layout assume, and no larger split was possible.
// Exit status 0 and a last line "... OK", or the first failure and status 1.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <vector>

#include "ce_gemm_plan.h"

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      printf("FAILED %s: ", #cond);               \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      exit(1);                                    \
    }                                             \
  } while (0)

static const int BK = 64;  // K-tile of the bf16 kernels (columns)
typedef long long i64;

// column k of a segmented operand, in bytes, from its definition (64-bit)
static i64 def1(i64 k, i64 seg_k, i64 stride) { return 2 * ((k / seg_k) * stride + k % seg_k); }
static i64 def2(i64 k, i64 seg_k, i64 stride, i64 seg2_k, i64 stride2) {
  return 2 * ((k / seg2_k) * stride2 + ((k % seg2_k) / seg_k) * stride + k % seg_k);
}
static bool fits(i64 v, CeSegWidth w) { return w == CE_SEG_U32_EXTRA ? (v >= 0 && v < (1ll << 32)) : (v >= -(1ll << 31) && v < (1ll << 31)); }

// the rules of ce_seg_encode, each from a loop over the columns instead of the header's divisions; 0 = none broken
enum Rule { NONE = 0, NOT_TILES, SHORT_STRIDE, AT_COLUMN_K };
static Rule broken_rule(int seg_k, i64 stride, int K, CeSegWidth w) {
  if (seg_k % BK) return NOT_TILES;
  if (stride < seg_k) return SHORT_STRIDE;
  i64 starts_below_K = 0, starts_up_to_K = 0;  // segment starts in [0, K) = segments touched; in (0, K] = boundaries at or below K
  for (int k = 0; k <= K; ++k)
    if (k % seg_k == 0) {
      starts_below_K += k < K;
      starts_up_to_K += k > 0;
    }
  const i64 extra = 2 * (stride - seg_k);
  if (w == CE_SEG_U32_EXTRA ? !fits(extra * starts_up_to_K, w) : !fits(extra * starts_below_K + 2ll * K, w)) return AT_COLUMN_K;
  return NONE;
}
// does the register of some K-tile t < kt really overflow?
static bool really_overflows(int seg_k, i64 stride, int K, CeSegWidth w) {
  for (int t = 0; t < K / BK; ++t) {
    const i64 k = (i64)t * BK;
    if (!fits(w == CE_SEG_U32_EXTRA ? def1(k, seg_k, stride) - 2 * k : def1(k, seg_k, stride), w)) return true;
  }
  return false;
}

static long n_seg = 0, n_acc = 0, n_rej = 0, n_margin = 0, n_floor_differs = 0;

static void check_seg(int seg_k, i64 stride, int K, CeSegWidth w) {
  const int kt = K / BK;
  CeSeg s;
  const int rc = ce_seg_encode(seg_k, stride, K, BK, kt, w, s);
  ++n_seg;
  if (seg_k <= 0 || seg_k >= K) {
    CHECK(rc == CE_OK && s.magic == 0 && s.extra == 0, "plain operand seg_k %d K %d", seg_k, K);
    return;
  }
  const Rule rule = broken_rule(seg_k, stride, K, w);
  CHECK((rc == CE_OK) == (rule == NONE) && (rc == CE_OK || rc == CE_ERR_SHAPE), "seg_k %d stride %lld K %d width %d: rc %d, rule %d", seg_k, stride, K, (int)w, rc,
        (int)rule);
  if (w == CE_SEG_I32_OFFSET && seg_k % BK == 0 && stride >= seg_k) {
    // ce_gemm384.hip's former bound (K / seg_k where ce_gemm256w4.hip had ceil): the same decision whenever K % seg_k == 0, which is all
    // ce_gemm_bf16_res lets through to it - so the two share CE_SEG_I32_OFFSET
    const bool floor_ok = 2 * (stride - seg_k) * (K / seg_k) + 2ll * K < (1ll << 31);
    if (K % seg_k == 0) CHECK(floor_ok == (rc == CE_OK), "floor and ceil forms differ at K %% seg_k == 0: seg_k %d stride %lld K %d", seg_k, stride, K);
    else n_floor_differs += floor_ok != (rc == CE_OK);
  }
  if (rc != CE_OK) {
    ++n_rej;
    if (rule == AT_COLUMN_K && !really_overflows(seg_k, stride, K, w)) ++n_margin;  // rejected by the stated margin (column K), no t < kt overflows yet
    return;
  }
  ++n_acc;
  for (int t = 0; t < kt; ++t) {
    const uint32_t segment = ((uint32_t)t * s.magic) >> 16;
    i64 off;
    if (w == CE_SEG_U32_EXTRA) {
      const uint32_t term = segment * s.extra;  // (wraps like the kernel's register would)
      CHECK((i64)term == (i64)segment * s.extra, "u32 term wraps: seg_k %d stride %lld K %d t %d", seg_k, stride, K, t);
      off = (i64)term + (i64)t * (BK * 2);
    } else {
      off = (i64)t * (BK * 2) + (i64)segment * s.extra;
      CHECK(fits(off, w) && fits((i64)segment * s.extra, w), "int offset wraps: seg_k %d stride %lld K %d t %d", seg_k, stride, K, t);
    }
    CHECK(off == def1((i64)t * BK, seg_k, stride) && off + 2 * (BK - 1) == def1((i64)t * BK + BK - 1, seg_k, stride), "offset: seg_k %d stride %lld K %d t %d",
          seg_k, stride, K, t);
  }
}

// largest stride (multiple of 8, >= lo) for which pred holds, pred monotone; lo - 8 when it never does
template <typename Pred>
static i64 edge(i64 lo, Pred pred) {
  if (!pred(lo)) return lo - 8;
  i64 a = lo, b = 1ll << 40;
  while (b - a > 8) {
    const i64 m = (a + (b - a) / 2) / 8 * 8;
    if (pred(m)) a = m; else b = m;
  }
  return a;
}

static void sweep_segments() {
  const int seg_ks[] = {64, 128, 192, 320, 640, 1152, 1280, 2560, 5120, 32, 96, 100, 65, 63, 1, 0, -64, 1 << 20};
  const int Ks[] = {128, 640, 1152, 2944, 5120, 5184, 10368, 13824};
  for (CeSegWidth w : {CE_SEG_U32_EXTRA, CE_SEG_I32_OFFSET})
    for (int K : Ks)
      for (int seg_k : seg_ks) {
        std::vector<i64> strides = {0, 8, (i64)seg_k - 8, seg_k, (i64)seg_k + 8, 4096, 5120ll * 7200, 1ll << 31, 1ll << 33};
        if (seg_k > 0 && seg_k < K && seg_k % BK == 0) {
          // around the last stride the header takes and around the last one no register overflows on (they differ by the column-K margin)
          const i64 e_header = edge(seg_k, [&](i64 s) { CeSeg t; return ce_seg_encode(seg_k, s, K, BK, K / BK, w, t) == CE_OK; });
          const i64 e_real = edge(seg_k, [&](i64 s) { return !really_overflows(seg_k, s, K, w); });
          CHECK(e_header <= e_real, "the header takes a stride that overflows: seg_k %d K %d", seg_k, K);
          for (i64 e : {e_header, e_real})
            for (i64 d : {-16, -8, 0, 8, 16}) strides.push_back(e + d);
        }
        for (i64 s : strides) check_seg(seg_k, s, K, w);
      }
  // the shapes the project runs: the all-to-all's receive layout (K = 5120 in 2, 4, 8 segments of a rank's rows) and the K-slab-major weights
  for (CeSegWidth w : {CE_SEG_U32_EXTRA, CE_SEG_I32_OFFSET}) {
    for (int ranks : {2, 4, 8})
      for (i64 rows : {900, 1800, 3600, 7200}) {
        CeSeg s;
        CHECK(ce_seg_encode(5120 / ranks, rows * (5120 / ranks), 5120, BK, 80, w, s) == CE_OK, "receive layout %d ranks %lld rows", ranks, rows);
        check_seg(5120 / ranks, rows * (5120 / ranks), 5120, w);
      }
    for (int K : {5120, 13824})
      for (i64 N : {5120, 13824, 15360}) {
        CeSeg s;
        CHECK(ce_seg_encode(64, N * 64, K, BK, K / BK, w, s) == CE_OK, "K-slab-major weights N %lld K %d", N, K);
        check_seg(64, N * 64, K, w);
      }
  }
}

// the two-level operand of the convolutions (ce_conv.hip): Cin channels, frames of Hp x Wp pixels, KT x 3 x 3 taps
static long n_seg2 = 0, n_seg2_acc = 0;
static void check_seg2(int seg_k, i64 stride, int seg2_k, i64 stride2, int K) {
  const int kt = K / BK;
  CeSeg s1, s2;
  ++n_seg2;
  if (ce_seg_encode(seg_k, stride, K, BK, kt, CE_SEG_I32_OFFSET, s1) != CE_OK) return;  // (the first level's own rules: check_seg)
  const int rc = ce_seg2_encode(seg_k, stride, seg2_k, stride2, K, BK, kt, s2);
  if (seg2_k >= K) {
    CHECK(rc == CE_OK && s2.magic == 0 && s2.extra == 0, "one second-level segment");
    return;
  }
  // the rules of ce_seg2_encode from loops: whole K-tiles; a second-level stride no shorter than the first-level strides inside it; the reach
  i64 inner_segments = 0, last2 = 0;
  for (int k = 0; k < seg2_k; ++k) inner_segments += k % seg_k == 0;
  for (int k = 0; k < K; ++k)
    if (k % seg2_k == 0) last2 = k / seg2_k;
  const bool ok = seg2_k % BK == 0 && stride2 >= inner_segments * stride && 2 * (last2 * stride2 + inner_segments * stride + seg_k) < (1ll << 31);
  CHECK((rc == CE_OK) == ok && (rc == CE_OK || rc == CE_ERR_SHAPE), "seg2: seg_k %d stride %lld seg2_k %d stride2 %lld K %d: rc %d", seg_k, stride, seg2_k,
        stride2, K, rc);
  if (rc != CE_OK) return;
  ++n_seg2_acc;
  for (int t = 0; t < kt; ++t) {
    const i64 o1 = (i64)t * (BK * 2) + (i64)(((uint32_t)t * s1.magic) >> 16) * s1.extra;  // koff
    const i64 o2 = (i64)(((uint32_t)t * s2.magic) >> 16) * s2.extra;                      // what koff_a adds
    CHECK(fits(o1, CE_SEG_I32_OFFSET) && fits(o2, CE_SEG_U32_EXTRA) && fits(o1 + o2, CE_SEG_I32_OFFSET), "seg2 offset wraps: t %d", t);
    CHECK(o1 + o2 == def2((i64)t * BK, seg_k, stride, seg2_k, stride2) && o1 + o2 + 2 * (BK - 1) == def2((i64)t * BK + BK - 1, seg_k, stride, seg2_k, stride2),
          "seg2 offset: seg_k %d stride %lld seg2_k %d stride2 %lld K %d t %d", seg_k, stride, seg2_k, stride2, K, t);
  }
}
static void sweep_seg2() {
  for (int Cin : {32, 96, 192, 384})
    for (int KT : {1, 3})
      for (int H : {1, 6, 90, 360, 720})
        for (int W : {1, 5, 160, 640, 1280}) {
          const int Hp = H + 2, Wp = W + 2;
          const int seg = (3 * Cin + 63) / 64 * 64, kpad = (KT * 3 * (seg / 64) + 1) / 2 * 2 * 64;
          check_seg2(seg, (i64)Wp * Cin, 3 * seg, (i64)Hp * Wp * Cin, kpad);
          check_seg(seg, (i64)Wp * Cin, kpad, CE_SEG_I32_OFFSET);
        }
  // around the reach's edge, and second-level strides around the first level's advance
  for (i64 stride2 : {0ll, 5760ll - 8, 5760ll, 5760ll + 8, (1ll << 28), (1ll << 29) - 2880 - 320, (1ll << 29) - 2880 - 320 + 8, 357913941ll / 8 * 8, 1ll << 30, 1ll << 34})
    check_seg2(320, 1920, 960, stride2, 2944);
  check_seg2(320, 1920, 1000, 1 << 20, 2944);  // (no whole K-tiles)
}

static long n_plan = 0, n_split = 0;
static void check_plan(int M, int N, int bm, int bn, int kt, int cus, i64 scratch, bool may_split) {
  const CeGemmPlan p = ce_gemm_plan(M, N, bm, bn, kt, cus, scratch, may_split);
  ++n_plan;
  int tm = 0, tn = 0;  // tiles that cover M and N, counted
  while ((i64)tm * bm < M) ++tm;
  while ((i64)tn * bn < N) ++tn;
  const i64 slab = (i64)bm * bn * 4;
  CHECK(p.tiles_m == tm && p.tiles_n == tn && p.last_round == (tm * tn) % cus, "tiles: M %d N %d %d x %d cus %d", M, N, bm, bn, cus);
  CHECK(p.split >= 1 && p.split <= 8 && (p.tail == 0) == (p.split == 1), "tail %d split %d", p.tail, p.split);
  CHECK(p.t_full + p.tail == tm * tn && p.grid == p.t_full + p.tail * p.split && p.reduce_grid == 4 * p.tail, "grid: M %d N %d %d x %d cus %d", M, N, bm, bn, cus);
  if (!may_split) CHECK(p.split == 1, "split where none is allowed");
  if (p.split > 1) {
    ++n_split;
    CHECK(p.tail == p.last_round && p.tail * p.split <= cus && kt % (2 * p.split) == 0 && (i64)p.tail * p.split * slab <= scratch,
          "split %d: tail %d kt %d cus %d scratch %lld", p.split, p.tail, kt, cus, scratch);
  }
  if (may_split && p.last_round > 0)  // no larger split would have done
    for (int s = p.split + 1; s <= 8 && s <= cus / p.last_round; ++s)
      CHECK(!(kt % (2 * s) == 0 && (i64)p.last_round * s * slab <= scratch), "split %d taken where %d fits: M %d N %d %d x %d kt %d cus %d scratch %lld", p.split, s,
            M, N, bm, bn, kt, cus, scratch);
}
static void sweep_plans() {
  const int tiles[5][2] = {{256, 256}, {384, 256}, {288, 256}, {256, 128}, {256, 96}};
  const i64 GEMM_WS_BYTES = 256ll * 384 * 256 * 4;  // chronoedit_amd/ops.py
  for (const auto& t : tiles) {
    const int bm = t[0], bn = t[1];
    for (int M : {1, bm - 1, bm, bm + 1, 2 * bm, 3 * bm + 1, 7200, 14400, 13068, 26136})
      for (int N : {8, bn - 1, bn, bn + 1, 5 * bn, 5120, 13824})
        for (int cus : {1, 8, 255, 256, 304})
          for (int kt : {2, 4, 6, 12, 16, 40, 46, 80, 108, 216})
            for (i64 scratch : {0ll, (i64)bm * bn * 4, GEMM_WS_BYTES})
              for (bool may_split : {true, false}) check_plan(M, N, bm, bn, kt, cus, scratch, may_split);
  }
}

int main() {
  sweep_segments();
  sweep_seg2();
  sweep_plans();
  CHECK(n_acc > 500 && n_rej > 500 && n_margin > 0 && n_seg2_acc > 50 && n_split > 1000, "the sweep lost its cases: %ld %ld %ld %ld %ld", n_acc, n_rej, n_margin,
        n_seg2_acc, n_split);
  printf("gemm_plan_host_check: %ld segmented operands (%ld taken, %ld refused, %ld of those by the column-K margin alone; floor/ceil differ on %ld with K %% seg_k != 0), "
         "%ld two-level operands (%ld taken), %ld plans (%ld split): OK\n",
         n_seg, n_acc, n_rej, n_margin, n_floor_differs, n_seg2, n_seg2_acc, n_plan, n_split);
  return 0;
}

// Connected components (chronoedit_amd/components.py): what a lane does in the tile labelling, the border merge and the compress pass of
// csrc/ce_components.hip, as functions that ALSO compile for the host - tools/components_host_check.cpp runs them one "lane" after the
// other under the host sanitizers against the Python definition before anything goes to a device.
//
// A label plane L is int32 [H][W]: -1 for background; for a foreground pixel p = y * W + x the index of another foreground pixel of its
// component, L[p] <= p (a root: L[p] == p).  Every writer keeps both properties: labels start at an index <= p of the same row run, and
// the only later write is an atomic minimum with an index of the same component.  So a walk along L strictly descends, and it ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD static inline
#endif

#define CC_TW 64  // a tile: one row is one 64-bit mask, the ballot of a wave
#define CC_TH 32

CC_HD int cc_atomic_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(p, v);  // (device scope: the border merge's nodes are shared by workgroups on every XCD)
#else
  const int o = *p;
  if (v < o) *p = v;
  return o;
#endif
}

CC_HD int cc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
  return *(const volatile int*)p;
#endif
}

// The root above node a (a foreground node).  A stale value is an earlier parent: still of the component, only a longer way.
CC_HD int cc_find(const int* L, int a) {
  // ends: the walk goes on only to a strictly smaller, non-negative index - at most a steps, whatever the memory holds
  for (int p = cc_load(L + a); p >= 0 && p < a; p = cc_load(L + a)) a = p;
  return a;
}

// Join the components of the foreground nodes a and b.  The value the atomic RETURNS decides: old == a, and a was a root that now hangs
// below b; old < a, and somebody had hung a elsewhere meanwhile - whichever of old and b the minimum kept below a, the other one is
// joined to it by going on with (old, b).
CC_HD void cc_union(int* L, int a, int b) {
  // ends: every retry replaces the larger node of the pair by a strictly smaller one (old < a, and b < a already)
  for (;;) {
    a = cc_find(L, a), b = cc_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = cc_atomic_min(L + a, b);
    if (old >= a || old < 0) return;  // (old == a: joined.  Anything else cannot be, and ends the loop too)
    a = old;
  }
}

// First column of the row run that holds column x of a row with the foreground bits `m`
CC_HD int cc_run_start(uint64_t m, int x) {
  const uint64_t below = ~m & ((1ull << x) - 1ull);  // the background columns left of x
  return below ? 64 - __builtin_clzll(below) : 0;
}

CC_HD bool cc_bit(uint64_t m, int x) { return x >= 0 && x < CC_TW && ((m >> x) & 1ull); }

// ---- the tile: rows[CC_TH] foreground masks, P[CC_TH * CC_TW] parents in TILE-LOCAL indices r * CC_TW + x -----------------------------------
// pass 1: a pixel starts below the first pixel of its row run: most pixels never need another parent
CC_HD void cc_tile_init(const uint64_t* rows, int* P, int r, int x) {
  P[r * CC_TW + x] = cc_bit(rows[r], x) ? r * CC_TW + cc_run_start(rows[r], x) : -1;
}

// pass 2: join pixel (r, x) with the row above.  One union per pair of touching runs is enough, so a pixel leaves to its left neighbour
// what that one does anyway, and looks diagonally only where the pixel straight above is background (up - left and up - right of a set
// `up` belong to up's run)
CC_HD void cc_tile_link(const uint64_t* rows, int* P, int r, int x) {
  if (r == 0 || !cc_bit(rows[r], x)) return;
  const uint64_t me = rows[r], up = rows[r - 1];
  const int i = r * CC_TW + x, u = (r - 1) * CC_TW + x;
  if (cc_bit(up, x)) {
    if (!(cc_bit(me, x - 1) && cc_bit(up, x - 1))) cc_union(P, i, u);
  } else {
    if (cc_bit(up, x - 1) && !cc_bit(me, x - 1)) cc_union(P, i, u - 1);
    if (cc_bit(up, x + 1) && !cc_bit(me, x + 1)) cc_union(P, i, u + 1);
  }
}

// pass 3: the tile-local root as an index of the plane; (ty0, tx0) the tile's first pixel
CC_HD int cc_tile_label(const int* P, int r, int x, int ty0, int tx0, int W) {
  if (P[r * CC_TW + x] < 0) return -1;
  const int root = cc_find(P, r * CC_TW + x);
  return (ty0 + root / CC_TW) * W + tx0 + root % CC_TW;
}

// ---- the borders: item k of a plane's (H - 1) / CC_TH horizontal borders (W pixels each: the first row of a tile row against the row
// above, all three neighbours, so the corners are covered) and then of its (W - 1) / CC_TW vertical ones (H pixels each: the first column of a
// tile column against the column on its left) ----------------------------------------------------------------------------------------
CC_HD long long cc_border_items(int H, int W) { return (long long)((H - 1) / CC_TH) * W + (long long)((W - 1) / CC_TW) * H; }

CC_HD bool cc_fg(const int* L, int H, int W, int y, int x) { return y >= 0 && y < H && x >= 0 && x < W && cc_load(L + (long long)y * W + x) >= 0; }

CC_HD void cc_border_merge(int* L, int H, int W, long long k) {
  const long long nh = (long long)((H - 1) / CC_TH) * W;
  if (k < nh) {
    const int y = (int)(k / W + 1) * CC_TH, x = (int)(k % W);
    if (!cc_fg(L, H, W, y, x)) return;
    const int p = y * W + x;
    if (cc_fg(L, H, W, y - 1, x)) {
      cc_union(L, p, p - W);
    } else {
      if (cc_fg(L, H, W, y - 1, x - 1)) cc_union(L, p, p - W - 1);
      if (cc_fg(L, H, W, y - 1, x + 1)) cc_union(L, p, p - W + 1);
    }
  } else {
    const long long j = k - nh;
    const int x = (int)(j / H + 1) * CC_TW, y = (int)(j % H);
    if (!cc_fg(L, H, W, y, x)) return;
    const int p = y * W + x;
    if (cc_fg(L, H, W, y, x - 1)) {
      cc_union(L, p, p - 1);
    } else {
      if (cc_fg(L, H, W, y - 1, x - 1)) cc_union(L, p, p - W - 1);
      if (cc_fg(L, H, W, y + 1, x - 1)) cc_union(L, p, p + W - 1);
    }
  }
}

// ---- compress: every label becomes its root, in place.  A reader that meets a label already replaced meets the root itself -------------------
CC_HD void cc_compress(int* L, long long p) {
  const int l = cc_load(L + p);
  if (l < 0 || l == (int)p) return;
  const int root = cc_find(L, l);
  if (root != l) L[p] = root;
}

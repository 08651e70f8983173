// The lane functions of csrc/ce_components_core.h run on the host, one "lane" after the other, in the order of the device's phases (tile
// init | tile link | tile label | border merge | compress) - built by tools/components_host_check.py with -fsanitize=address,undefined and
// compared there with components.reference.  What this can show: an index out of bounds, a wrong neighbour rule, a tile or border that is
// not covered.  What it cannot: anything about concurrency.
//   components_host_check IN OUT     IN: records of int32 H, int32 W, H * W bytes;  OUT: per record H * W int32 labels
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ce_components_core.h"

static void roots(const std::vector<uint8_t>& plane, std::vector<int>& L, int H, int W, bool backwards) {
  const int tiles_x = (W + CC_TW - 1) / CC_TW, tiles_y = (H + CC_TH - 1) / CC_TH;
  for (int tile = 0; tile < tiles_x * tiles_y; ++tile) {
    const int ty0 = (tile / tiles_x) * CC_TH, tx0 = (tile % tiles_x) * CC_TW;
    std::vector<uint64_t> rows(CC_TH, 0);  // (exact sizes on the heap: the sanitizer sees every overrun)
    std::vector<int> P(CC_TH * CC_TW, 12345678);
    for (int r = 0; r < CC_TH; ++r)
      for (int x = 0; x < CC_TW; ++x)
        if (ty0 + r < H && tx0 + x < W && plane[(size_t)(ty0 + r) * W + tx0 + x]) rows[r] |= 1ull << x;
    for (int t = 0; t < CC_TH * CC_TW; ++t) cc_tile_init(rows.data(), P.data(), t / CC_TW, t % CC_TW);
    for (int k = 0; k < CC_TH * CC_TW; ++k) {
      const int t = backwards ? CC_TH * CC_TW - 1 - k : k;
      cc_tile_link(rows.data(), P.data(), t / CC_TW, t % CC_TW);
    }
    for (int t = 0; t < CC_TH * CC_TW; ++t) {
      const int r = t / CC_TW, x = t % CC_TW;
      if (ty0 + r < H && tx0 + x < W) L[(size_t)(ty0 + r) * W + tx0 + x] = cc_tile_label(P.data(), r, x, ty0, tx0, W);
    }
  }
  const long long items = cc_border_items(H, W);
  for (long long k = 0; k < items; ++k) cc_border_merge(L.data(), H, W, backwards ? items - 1 - k : k);
  for (long long p = 0; p < (long long)H * W; ++p) cc_compress(L.data(), backwards ? (long long)H * W - 1 - p : p);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hw[2], records = 0;
  while (fread(hw, sizeof(int), 2, in) == 2) {
    const int H = hw[0], W = hw[1];
    if (H <= 0 || W <= 0 || (long long)H * W > (1 << 26)) return 3;
    std::vector<uint8_t> plane((size_t)H * W);
    if (fread(plane.data(), 1, plane.size(), in) != plane.size()) return 3;
    std::vector<int> fwd((size_t)H * W, 0x5a5a5a5a), bwd((size_t)H * W, -7);
    roots(plane, fwd, H, W, false);
    roots(plane, bwd, H, W, true);  // another order of the unions: the same labels
    if (fwd != bwd) {
      fprintf(stderr, "record %d (%d x %d): the labels depend on the order\n", records, H, W);
      return 1;
    }
    fwrite(fwd.data(), sizeof(int), fwd.size(), out);
    ++records;
  }
  fclose(in), fclose(out);
  printf("%d records\n", records);
  return 0;
}

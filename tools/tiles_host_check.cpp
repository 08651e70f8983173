// The host launchers of csrc/ce_tiles.hip under AddressSanitizer and UBSan, as a stand-alone program (tools/tiles_host_check.py builds it):
// every rejection the header declares.  Each of these calls returns from the launcher's argument checks, before any HIP call: the program
// initialises no device and launches nothing, wherever it runs, and the host buffers it passes are never dereferenced.  The valid path needs
// a device and device memory and is NOT exercised here: tests/test_exact_tiles_gpu.py runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "chronoedit_hip.h"

int main() {
  std::vector<float> t(4 * 16 * 8 * 12 + 4), c(16 * 12 * 20 + 4);
  int ox[2] = {0, 8}, oy[2] = {0, 4}, gap[2] = {0, 13}, dec[2] = {8, 0}, many[17] = {0};
  int bad = 0;
  auto expect = [&](int rc, int want, const char* what) {
    if (rc != want) std::printf("FAIL %s: %d != %d\n", what, rc, want), ++bad;
  };
  for (int k = 0; k < 2; ++k) {  // 0: fuse (tiles -> canvas), 1: scatter (canvas -> tiles): one argument check
    auto f = [&](const float* a, float* b, int nx, int ny, const int* x, const int* y, int planes, int th, int tw, int ch, int cw) {
      return k ? ce_tiles_scatter_f32(b, (float*)a, nx, ny, x, y, planes, th, tw, ch, cw, nullptr)
               : ce_tiles_fuse_f32(a, b, nx, ny, x, y, planes, th, tw, ch, cw, nullptr);
    };
    expect(f(nullptr, c.data(), 2, 2, ox, oy, 16, 8, 12, 12, 20), -1, "NULL tiles");
    expect(f(t.data(), nullptr, 2, 2, ox, oy, 16, 8, 12, 12, 20), -1, "NULL canvas");
    expect(f(t.data(), t.data(), 2, 2, ox, oy, 16, 8, 12, 12, 20), -1, "tiles == canvas");
    expect(f(t.data(), c.data(), 2, 2, nullptr, oy, 16, 8, 12, 12, 20), -1, "NULL ox");
    expect(f(t.data(), c.data(), 2, 2, ox, nullptr, 16, 8, 12, 12, 20), -1, "NULL oy");
    expect(f(t.data(), c.data(), 2, 2, gap, oy, 16, 8, 12, 12, 25), -1, "a gap between neighbours");
    expect(f(t.data(), c.data(), 2, 2, dec, oy, 16, 8, 12, 12, 20), -1, "decreasing origins");
    expect(f(t.data(), c.data(), 2, 2, ox, oy, 16, 8, 12, 12, 24), -1, "the last tile not flush with the canvas");
    expect(f(t.data(), c.data(), 17, 1, many, oy, 16, 8, 12, 12, 20), -1, "17 origins on an axis");
    expect(f(t.data(), c.data(), 4, 5, many, many, 16, 8, 12, 12, 20), -1, "20 tiles");
    expect(f(t.data(), c.data(), 0, 2, ox, oy, 16, 8, 12, 12, 20), -1, "no tile");
    expect(f(t.data(), c.data(), 2, 2, ox, oy, 0, 8, 12, 12, 20), -1, "no plane");
    expect(f(t.data(), c.data(), 2, 2, ox, oy, 1 << 24, 8, 12, 12, 20), -2, "2^31 cells");
    expect(f((const float*)((char*)t.data() + 2), c.data(), 2, 2, ox, oy, 16, 8, 12, 12, 20), -3, "a base 2 bytes off");
  }
  std::vector<uint8_t> fr(4 * 64 * 96 * 3), out(96 * 160 * 3);
  int px[2] = {0, 64}, py[2] = {0, 32}, pgap[2] = {0, 97};
  auto blend = [&](const void* f, void* o, int nx, const int* x, int F, int H, int W) {
    return ce_tiles_blend_u8(f, o, nx, 2, x, py, F, 64, 96, H, W, nullptr);
  };
  expect(blend(nullptr, out.data(), 2, px, 1, 96, 160), -1, "blend: NULL frames");
  expect(blend(fr.data(), nullptr, 2, px, 1, 96, 160), -1, "blend: NULL out");
  expect(blend(fr.data(), fr.data(), 2, px, 1, 96, 160), -1, "blend: out == frames");
  expect(blend(fr.data(), out.data(), 2, px, 0, 96, 160), -1, "blend: no frame");
  expect(blend(fr.data(), out.data(), 2, px, 65536, 96, 160), -1, "blend: 65536 frames");
  expect(blend(fr.data(), out.data(), 2, px, 1, 97, 160), -1, "blend: a target higher than the canvas");
  expect(blend(fr.data(), out.data(), 2, px, 1, 96, 161), -1, "blend: a target wider than the canvas");
  expect(blend(fr.data(), out.data(), 2, pgap, 1, 96, 160), -1, "blend: a gap");
  expect(blend(fr.data(), out.data(), 17, px, 1, 96, 160), -1, "blend: 17 origins");
  expect(blend(fr.data(), out.data(), 2, nullptr, 1, 96, 160), -1, "blend: NULL ox");
  std::printf(bad ? "FAILED\n" : "ok: every rejection as declared\n");
  return bad ? 1 : 0;
}

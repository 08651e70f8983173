// Tiled edits (chronoedit_amd/tiles.py): one canvas of latents is denoised as overlapping model-size tiles, the samples of one batched pass.
//
//   ce_tiles_fuse_f32      tiles -> canvas, behind every scheduler update: per canvas cell the mean of the covering tiles' cells under
//                          separable integer tent weights, accumulated in double in ascending tile index, one division, one rounding.
//   ce_tiles_scatter_f32   canvas -> tiles: every tile cell takes its canvas cell (also: the noise canvas cut into the tiles before step 0).
//   ce_tiles_blend_u8      the decoded tiles' bytes -> the target frame: (sum of w e + W / 2) / W in exact integers, tents in pixels.
//
// The grid of tiles is separable: nx origins on x, ny on y, tile t = iy * nx + ix at (ox[ix], oy[iy]).  The origins travel by value in the
// kernel's arguments (a captured launch keeps them), so the launchers check the whole geometry on the host before anything runs: a lane
// never forms an address from an unchecked origin.  No atomics, no host read, no allocation, no state; every loop is bounded by 16.
// Every product and add of the fusion is rounded on its own (`#pragma clang fp contract(off)`, as in csrc/ce_lift.hip).
#include "ce_common.h"

#define CE_TILES_MAX 16

struct TileGrid {
  int nx, ny;
  int ox[CE_TILES_MAX], oy[CE_TILES_MAX];
};

// origins o[0..n) of tiles of side T covering [0, C): o[0] = 0, o[n - 1] + T = C, strictly increasing, no gap
static bool tiles_axis_ok(const int* o, int n, int T, int C) {
  if (!o || n < 1 || n > CE_TILES_MAX || T <= 0 || C < T || o[0] != 0 || (long long)o[n - 1] + T != C) return false;
  for (int i = 1; i < n; ++i)
    if (o[i] <= o[i - 1] || o[i] > o[i - 1] + T) return false;
  return true;
}

static bool tiles_grid(TileGrid& g, int nx, int ny, const int* ox, const int* oy, int tw, int th, int cw, int ch) {
  if (nx < 1 || ny < 1 || nx > CE_TILES_MAX || ny > CE_TILES_MAX || nx * ny > CE_TILES_MAX) return false;
  if (!tiles_axis_ok(ox, nx, tw, cw) || !tiles_axis_ok(oy, ny, th, ch)) return false;
  g.nx = nx, g.ny = ny;
  for (int i = 0; i < CE_TILES_MAX; ++i) g.ox[i] = i < nx ? ox[i] : 0, g.oy[i] = i < ny ? oy[i] : 0;
  return true;
}

// V consecutive cells of a row move as one access when every row start allows it: tw, cw and every x origin multiples of V, bases aligned
static bool tiles_wide(const TileGrid& g, int tw, int cw, const void* a, const void* b) {
  if (tw % 4 || cw % 4 || (((uintptr_t)a | (uintptr_t)b) & 15)) return false;
  for (int i = 0; i < g.nx; ++i)
    if (g.ox[i] % 4) return false;
  return true;
}

__device__ __forceinline__ int tent(int x, int T) { return min(x + 1, T - x); }

// One lane per V consecutive canvas cells of a row (V = 4: one 16-byte access per tile and for the canvas; the V cells lie under the same
// tiles because every origin is a multiple of V).  tiles = [n][planes][th][tw], canvas = [planes][ch][cw].
template <int V>
__global__ __launch_bounds__(256) void tiles_fuse_kernel(const float* __restrict__ tiles, float* __restrict__ canvas, TileGrid g, int planes, int th, int tw,
                                                         int ch, int cw) {
#pragma clang fp contract(off)
  const int gw = cw / V;
  const long long total = (long long)planes * ch * gw;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int X = (int)(idx % gw) * V;
  const int Y = (int)((idx / gw) % ch);
  const int p = (int)(idx / ((long long)gw * ch));
  double acc[V];
  long long wsum[V];
  bool first = true;
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.0, wsum[j] = 0;
  for (int iy = 0; iy < g.ny; ++iy) {
    const int y = Y - g.oy[iy];
    if (y < 0 || y >= th) continue;
    const int wy = tent(y, th);
    for (int ix = 0; ix < g.nx; ++ix) {
      const int x = X - g.ox[ix];
      if (x < 0 || x >= tw) continue;  // (V > 1: x + V <= tw follows from the multiples)
      const float* s = tiles + (((size_t)(iy * g.nx + ix) * planes + p) * th + y) * tw + x;
      float v[V];
      if constexpr (V == 4) {
        const f32x4 q = *(const f32x4*)s;
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
      } else {
        v[0] = s[0];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int w = wy * tent(x + j, tw);
        const double prod = (double)w * (double)v[j];
        acc[j] = first ? prod : acc[j] + prod;
        wsum[j] += w;
      }
      first = false;
    }
  }
  float* d = canvas + ((size_t)p * ch + Y) * cw + X;
  if constexpr (V == 4) {
    f32x4 q;
    q[0] = (float)(acc[0] / (double)wsum[0]), q[1] = (float)(acc[1] / (double)wsum[1]);
    q[2] = (float)(acc[2] / (double)wsum[2]), q[3] = (float)(acc[3] / (double)wsum[3]);
    *(f32x4*)d = q;
  } else {
    d[0] = (float)(acc[0] / (double)wsum[0]);
  }
}

// One lane per V consecutive cells of a tile row.
template <int V>
__global__ __launch_bounds__(256) void tiles_scatter_kernel(const float* __restrict__ canvas, float* __restrict__ tiles, TileGrid g, int planes, int th, int tw,
                                                            int ch, int cw) {
  const int gw = tw / V;
  const long long total = (long long)g.nx * g.ny * planes * th * gw;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % gw) * V;
  long long r = idx / gw;
  const int y = (int)(r % th);
  r /= th;
  const int p = (int)(r % planes);
  const int t = (int)(r / planes);
  const int iy = t / g.nx, ix = t - iy * g.nx;
  const float* s = canvas + ((size_t)p * ch + g.oy[iy] + y) * cw + g.ox[ix] + x;
  float* d = tiles + (((size_t)t * planes + p) * th + y) * tw + x;
  if constexpr (V == 4)
    *(f32x4*)d = *(const f32x4*)s;
  else
    d[0] = s[0];
}

static int tiles_latent_args(TileGrid& g, const void* tiles, const void* canvas, int nx, int ny, const int* ox, const int* oy, int planes, int th, int tw,
                             int ch, int cw) {
  if (!tiles || !canvas || tiles == canvas || planes <= 0) return CE_ERR_ARG;
  if (!tiles_grid(g, nx, ny, ox, oy, tw, th, cw, ch)) return CE_ERR_ARG;
  if ((long long)planes * ch * cw >= (1ll << 31) || (long long)nx * ny * planes * th * tw >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)tiles | (uintptr_t)canvas) & 3) return CE_ERR_ALIGN;
  return CE_OK;
}

CE_API int ce_tiles_fuse_f32(const float* tiles, float* canvas, int nx, int ny, const int* ox, const int* oy, int planes, int th, int tw, int ch,
                             int cw, hipStream_t stream) {
  TileGrid g;
  const int rc = tiles_latent_args(g, tiles, canvas, nx, ny, ox, oy, planes, th, tw, ch, cw);
  if (rc != CE_OK) return rc;
  if (tiles_wide(g, tw, cw, tiles, canvas)) {
    const long long total = (long long)planes * ch * (cw / 4);
    hipLaunchKernelGGL(tiles_fuse_kernel<4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tiles, canvas, g, planes, th, tw, ch, cw);
  } else {
    const long long total = (long long)planes * ch * cw;
    hipLaunchKernelGGL(tiles_fuse_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tiles, canvas, g, planes, th, tw, ch, cw);
  }
  return (int)hipGetLastError();
}

CE_API int ce_tiles_scatter_f32(const float* canvas, float* tiles, int nx, int ny, const int* ox, const int* oy, int planes, int th, int tw, int ch,
                                int cw, hipStream_t stream) {
  TileGrid g;
  const int rc = tiles_latent_args(g, tiles, canvas, nx, ny, ox, oy, planes, th, tw, ch, cw);
  if (rc != CE_OK) return rc;
  if (tiles_wide(g, tw, cw, tiles, canvas)) {
    const long long total = (long long)nx * ny * planes * th * (tw / 4);
    hipLaunchKernelGGL(tiles_scatter_kernel<4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, canvas, tiles, g, planes, th, tw, ch, cw);
  } else {
    const long long total = (long long)nx * ny * planes * th * tw;
    hipLaunchKernelGGL(tiles_scatter_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, canvas, tiles, g, planes, th, tw, ch, cw);
  }
  return (int)hipGetLastError();
}

// One lane per four consecutive bytes of one output frame (blockIdx.y = frame), as ce_focus_paste_u8: the group's first byte is split into
// (Y, X, channel) once and the other three follow by counting.  frames = [n][F][TH][TW][3], out = [F][H][W][3] with H <= CH, W <= CW.
// WIDE (frame bytes % 4 == 0, out 4-byte aligned): the result leaves as one dword.  The sums are 64-bit; the division is 32-bit whenever
// numerator and denominator both fit, which the kernel tests (always, at model-size tiles: 16 tiles * 640 * 360 * 255 < 2^32).
template <bool WIDE>
__global__ __launch_bounds__(256) void tiles_blend_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, TileGrid g, int F, int TH, int TW,
                                                          int W, long long n) {
  const long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= n) return;
  const int f = blockIdx.y;
  const int nb = (int)(n - b0 < 4 ? n - b0 : 4);
  uint32_t o[4] = {0, 0, 0, 0};
  const long long px = b0 / 3;
  int c = (int)(b0 - px * 3), Y = (int)(px / W), X = (int)(px - (long long)Y * W);
  const size_t tile_bytes = (size_t)TH * TW * 3;
  for (int j = 0; j < nb; ++j) {
    unsigned long long num = 0, den = 0;
    for (int iy = 0; iy < g.ny; ++iy) {
      const int y = Y - g.oy[iy];
      if (y < 0 || y >= TH) continue;
      const unsigned long long wy = (unsigned long long)tent(y, TH);
      for (int ix = 0; ix < g.nx; ++ix) {
        const int x = X - g.ox[ix];
        if (x < 0 || x >= TW) continue;
        const unsigned long long w = wy * (unsigned long long)tent(x, TW);
        const uint8_t* e = frames + ((size_t)(iy * g.nx + ix) * F + f) * tile_bytes + ((size_t)y * TW + x) * 3 + c;
        num += w * (unsigned long long)e[0];
        den += w;
      }
    }
    num += den >> 1;  // (den >= 1: the launcher checked that the tiles cover the canvas)
    o[j] = ((num | den) >> 32) == 0 ? (uint32_t)num / (uint32_t)den : (uint32_t)(num / den);
    if (++c == 3) {
      c = 0;
      if (++X == W) X = 0, ++Y;
    }
  }
  uint8_t* d = out + (size_t)f * n + b0;
  if (WIDE) {  // (nb == 4 on this path)
    *(uint32_t*)d = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
  } else {
    for (int j = 0; j < nb; ++j) d[j] = (uint8_t)o[j];
  }
}

CE_API int ce_tiles_blend_u8(const void* frames, void* out, int nx, int ny, const int* ox, const int* oy, int F, int TH, int TW, int H, int W,
                             hipStream_t stream) {
  if (!frames || !out || frames == out || F <= 0 || F > 65535 || H <= 0 || W <= 0 || TH <= 0 || TW <= 0) return CE_ERR_ARG;
  if (!ox || !oy || nx < 1 || ny < 1 || nx > CE_TILES_MAX || ny > CE_TILES_MAX) return CE_ERR_ARG;
  const long long CW = (long long)ox[nx - 1] + TW, CH = (long long)oy[ny - 1] + TH;  // the canvas the tiles span; the target is its top left part
  if (CW >= (1ll << 31) || CH >= (1ll << 31) || W > CW || H > CH) return CE_ERR_ARG;
  TileGrid g;
  if (!tiles_grid(g, nx, ny, ox, oy, TW, TH, (int)CW, (int)CH)) return CE_ERR_ARG;
  const long long n = (long long)H * W * 3;
  if (n >= (1ll << 31) || (long long)nx * ny * F * TH * TW * 3 >= (1ll << 40) || (long long)TH * TW * 3 >= (1ll << 31)) return CE_ERR_SHAPE;
  const long long groups = (n + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)F);
  if (n % 4 == 0 && !((uintptr_t)out & 3))
    hipLaunchKernelGGL(tiles_blend_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)frames, (uint8_t*)out, g, F, TH, TW, W, n);
  else
    hipLaunchKernelGGL(tiles_blend_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)frames, (uint8_t*)out, g, F, TH, TW, W, n);
  return (int)hipGetLastError();
}

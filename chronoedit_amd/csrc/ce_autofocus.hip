// Auto-focused edits (chronoedit_amd/autofocus.py): an instruction-only edit finds its region on the whole photo (the scout), lifts the detected
// mask to the photo's size ON THE DEVICE and goes on as a focused region edit of the crop.  The two passes nothing else covers:
//
//   ce_autofocus_bbox_u8      the half-open bounding box of mask > 0 and the count of non-zero bytes, over rows `pitch` bytes apart (a box's view
//                             of the photo-size mask is reduced where it lies): what focus.mask_bbox and a sum do on the host, without the
//                             12 MB read.  Integers only: the result does not depend on the launch order.
//   ce_autofocus_restart_f32  the warm start: the scout's estimate of the final image, cropped and bilinearly resampled to the crop's latent
//                             grid through host-made tables, noised to the level of the step the focused pass starts at:
//                             out = (1 - s) * R(x0) + s * eps, every fp32 operation rounded on its own (`#pragma clang fp contract(off)`, as
//                             in csrc/ce_region.hip), optionally rounded to a bf16 value.
#include <limits.h>

#include "ce_common.h"

// out <- {W, H, 0, 0, 0}: the neutral element of (min, min, max, max, sum), which is also what an empty mask leaves
__global__ void autofocus_bbox_init_kernel(int* __restrict__ out, int H, int W) {
  if (blockIdx.x == 0 && threadIdx.x < 5) out[threadIdx.x] = threadIdx.x == 0 ? W : threadIdx.x == 1 ? H : 0;
}

// bit 8 j of the result = (byte j of v != 0)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) {
  v |= v >> 4;
  v |= v >> 2;
  v |= v >> 1;
  return v & 0x01010101u;
}

struct BoxAcc {
  int minx, miny, maxx, maxy, cnt;  // maxx / maxy are one past the last hit
};

__device__ __forceinline__ void box_hit(BoxAcc& a, int x_lo, int x_hi, int n) {
  a.minx = min(a.minx, x_lo);
  a.maxx = max(a.maxx, x_hi + 1);
  a.cnt += n;
}

// blockIdx.y walks the rows (stride gridDim.y), blockIdx.x * 256 + threadIdx.x the 16-byte groups of a row (stride gridDim.x * 256).  A row
// is split where IT lies: `head` bytes up to the first 16-byte boundary, whole aligned uint4 groups, a tail of < 16 bytes; head and tail go
// byte by byte to the first lanes of the row's first workgroup.  Per lane -> per wave (shuffles) -> per workgroup (LDS) -> five atomics.
__global__ __launch_bounds__(256) void autofocus_bbox_kernel(const uint8_t* __restrict__ mask, long long pitch, int H, int W, int* __restrict__ out) {
  BoxAcc a = {INT_MAX, INT_MAX, 0, 0, 0};
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    const uint8_t* row = mask + (size_t)y * (size_t)pitch;
    const int head = min(W, (int)((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u));
    const int nvec = (W - head) >> 4;
    const int tail0 = head + (nvec << 4);
    const int before = a.cnt;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < nvec; v += gridDim.x * 256) {
      const int x0 = head + (v << 4);
      const u32x4 q = *(const u32x4*)(row + x0);  // (16-byte aligned: x0 - head is a multiple of 16)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t nz = nonzero_bytes(q[j]);
        if (nz) box_hit(a, x0 + 4 * j + ((__ffs((int)nz) - 1) >> 3), x0 + 4 * j + ((31 - __clz((int)nz)) >> 3), __popc(nz));
      }
    }
    if (blockIdx.x == 0) {
      const int t = threadIdx.x;
      const int x = t < head ? t : tail0 + (t - head);  // lanes [0, head): the head; the next W - tail0 lanes: the tail
      if (x < W && (t < head || x >= tail0) && row[x]) box_hit(a, x, x, 1);
    }
    if (a.cnt != before) {
      a.miny = min(a.miny, y);
      a.maxy = max(a.maxy, y + 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.minx = min(a.minx, __shfl_xor(a.minx, o, 64));
    a.miny = min(a.miny, __shfl_xor(a.miny, o, 64));
    a.maxx = max(a.maxx, __shfl_xor(a.maxx, o, 64));
    a.maxy = max(a.maxy, __shfl_xor(a.maxy, o, 64));
    a.cnt += __shfl_xor(a.cnt, o, 64);
  }
  __shared__ int part[4][5];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[wave][0] = a.minx, part[wave][1] = a.miny, part[wave][2] = a.maxx, part[wave][3] = a.maxy, part[wave][4] = a.cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      a.minx = min(a.minx, part[k][0]), a.miny = min(a.miny, part[k][1]);
      a.maxx = max(a.maxx, part[k][2]), a.maxy = max(a.maxy, part[k][3]);
      a.cnt += part[k][4];
    }
    if (a.cnt) {
      atomicMin(out + 0, a.minx), atomicMin(out + 1, a.miny);
      atomicMax(out + 2, a.maxx), atomicMax(out + 3, a.maxy);
      atomicAdd(out + 4, a.cnt);
    }
  }
}

CE_API int ce_autofocus_bbox_u8(const void* mask, long long pitch, int H, int W, int* out, hipStream_t stream) {
  if (!mask || !out || H <= 0 || W <= 0 || pitch < W) return CE_ERR_ARG;
  if ((long long)H * W >= (1ll << 31)) return CE_ERR_SHAPE;  // the count is a 32-bit integer
  if ((uintptr_t)out & 3) return CE_ERR_ALIGN;
  hipLaunchKernelGGL(autofocus_bbox_init_kernel, dim3(1), dim3(64), 0, stream, out, H, W);
  const int groups = (W + 15) / 16;
  const int gx = min(max((groups + 255) / 256, 1), 16);
  const int gy = min(H, max(512 / gx, 1));  // (every workgroup ends in five atomics on the same five words: few workgroups, many rows each)
  hipLaunchKernelGGL(autofocus_bbox_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, stream, (const uint8_t*)mask, pitch, H, W, out);
  return (int)hipGetLastError();
}

// v = the bilinear sample, then the noising: seven fp32 operations for v, four for the mix, each rounded on its own
__device__ __forceinline__ float restart_value(float a00, float a01, float a10, float a11, float fx, float fy, float s, float e) {
#pragma clang fp contract(off)
  const float top = a00 + fx * (a01 - a00);
  const float bot = a10 + fx * (a11 - a10);
  const float v = top + fy * (bot - top);
  const float keep = 1.0f - s;
  const float kv = keep * v;
  const float se = s * e;
  return kv + se;
}

// One lane per output element of all C * T planes.  The tables are the host's (autofocus.restart_tables); an index outside the grid is
// clamped into it, whatever the table says.
template <bool BF16>
__global__ __launch_bounds__(256) void autofocus_restart_kernel(const float* __restrict__ x0, const float* __restrict__ eps, float* __restrict__ out,
                                                                const int* __restrict__ ix0, const int* __restrict__ ix1, const float* __restrict__ fx,
                                                                const int* __restrict__ iy0, const int* __restrict__ iy1, const float* __restrict__ fy, float s,
                                                                long long n, int h, int w) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long row = i / w;
  const int x = (int)(i - row * w);
  const long long plane = row / h;
  const int y = (int)(row - plane * h);
  const int xa = min(max(ix0[x], 0), w - 1), xb = min(max(ix1[x], 0), w - 1);
  const int ya = min(max(iy0[y], 0), h - 1), yb = min(max(iy1[y], 0), h - 1);
  const float* p = x0 + plane * h * w;
  const float r = restart_value(p[ya * w + xa], p[ya * w + xb], p[yb * w + xa], p[yb * w + xb], fx[x], fy[y], s, eps[i]);
  out[i] = BF16 ? round_bf16(r) : r;
}

CE_API int ce_autofocus_restart_f32(const float* x0, const float* eps, float* out, const int* ix0, const int* ix1, const float* fx, const int* iy0,
                                    const int* iy1, const float* fy, float s, int planes, int h, int w, int bf16_state, hipStream_t stream) {
  if (!x0 || !eps || !out || !ix0 || !ix1 || !fx || !iy0 || !iy1 || !fy || out == x0) return CE_ERR_ARG;
  if (planes <= 0 || h <= 0 || w <= 0) return CE_ERR_ARG;
  if ((long long)h * w >= (1ll << 31)) return CE_ERR_SHAPE;
  const long long n = (long long)planes * h * w;
  if ((n + 255) / 256 >= (1ll << 31)) return CE_ERR_SHAPE;
  if (((uintptr_t)x0 | (uintptr_t)eps | (uintptr_t)out | (uintptr_t)ix0 | (uintptr_t)ix1 | (uintptr_t)fx | (uintptr_t)iy0 | (uintptr_t)iy1 | (uintptr_t)fy) & 3)
    return CE_ERR_ALIGN;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (bf16_state)
    hipLaunchKernelGGL(autofocus_restart_kernel<true>, grid, dim3(256), 0, stream, x0, eps, out, ix0, ix1, fx, iy0, iy1, fy, s, n, h, w);
  else
    hipLaunchKernelGGL(autofocus_restart_kernel<false>, grid, dim3(256), 0, stream, x0, eps, out, ix0, ix1, fx, iy0, iy1, fy, s, n, h, w);
  return (int)hipGetLastError();
}

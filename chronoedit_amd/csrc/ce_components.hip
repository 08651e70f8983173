// Connected components of a byte plane at the photo's size (chronoedit_amd/components.py is the definition; every pass here gives its bits).
// Foreground is a non-zero byte, the neighbourhood is 8-connected, and a component's label is the smallest index y * W + x of its pixels -
// a label no order of evaluation can change, which is what lets these passes be compared bit for bit.
//
//   ce_components_roots_i32   plane -> labels.  Three launches, the block-based union-find of Komura / Playne and Hawick:
//                               tile     a workgroup labels a CC_TH x CC_TW tile in the LDS: a row of the tile is one wave ballot, a pixel starts
//                                        below the first pixel of its row run, one union per pair of touching runs of adjacent rows, and
//                                        every pixel leaves with its tile-local root as an index of the plane
//                               border   one lane per pixel of a tile's first row / first column: unions across the border, with a
//                                        device-scope atomicMin whose RETURNED value decides (csrc/ce_components_core.h)
//                               compress every label becomes its root
//   ce_components_sums_i32    labels (+ a weight plane) -> at each root the number of its component's pixels whose weight byte is non-zero,
//                             0 elsewhere: one integer atomicAdd per wave and distinct root, a root that goes on added once when it ends
//   ce_components_keep_u8     plane, labels, sums -> the plane without the components below a weight; the weight is a number, or a
//                             fraction num / den of the heaviest component's, taken from device memory: nothing is read back
//   ce_components_seeds_f32 / ce_components_masked_f32   the automatic region's seed plane d > thr and d' = kept ? d : -1
//
// Every loop ends by construction (the reason stands at the loop), no workgroup waits for another one, and the phases are separate
// launches.  Integers and integer atomics only: the results do not depend on the order of arrival.  No state; the scratch is the caller's.
#include "ce_common.h"
#include "ce_components_core.h"

// ---- roots ------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = tile row * tiles_x + tile column; 256 lanes: wave w owns the tile's rows w, w + 4, ..., a lane one column
__global__ __launch_bounds__(256) void components_tile_kernel(const uint8_t* __restrict__ plane, int* __restrict__ labels, int H, int W, int tiles_x) {
  __shared__ uint64_t rows[CC_TH];
  __shared__ int P[CC_TH * CC_TW];
  const int ty0 = (blockIdx.x / tiles_x) * CC_TH, tx0 = (blockIdx.x % tiles_x) * CC_TW;
  const int x = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool in_x = tx0 + x < W;
#pragma unroll
  for (int r = wave; r < CC_TH; r += 4) {
    const bool fg = in_x && ty0 + r < H && plane[(size_t)(ty0 + r) * W + tx0 + x] != 0;
    const uint64_t m = __ballot(fg);
    if (x == 0) rows[r] = m;
  }
  __syncthreads();
#pragma unroll
  for (int r = wave; r < CC_TH; r += 4) cc_tile_init(rows, P, r, x);
  __syncthreads();
  for (int r = wave; r < CC_TH; r += 4) cc_tile_link(rows, P, r, x);
  __syncthreads();
  for (int r = wave; r < CC_TH; r += 4)
    if (in_x && ty0 + r < H) labels[(size_t)(ty0 + r) * W + tx0 + x] = cc_tile_label(P, r, x, ty0, tx0, W);
}

__global__ __launch_bounds__(256) void components_border_kernel(int* __restrict__ labels, int H, int W, long long items) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < items) cc_border_merge(labels, H, W, k);
}

__global__ __launch_bounds__(256) void components_compress_kernel(int* __restrict__ labels, long long n) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < n) cc_compress(labels, p);
}

static int components_shape(int H, int W) {
  if (H <= 0 || W <= 0) return CE_ERR_ARG;
  if ((long long)H * W >= (1ll << 31)) return CE_ERR_SHAPE;
  return CE_OK;
}

CE_API int ce_components_roots_i32(const void* plane, int* labels, int H, int W, hipStream_t stream) {
  if (!plane || !labels || plane == (const void*)labels) return CE_ERR_ARG;
  if (const int e = components_shape(H, W)) return e;
  if ((uintptr_t)labels & 3) return CE_ERR_ALIGN;
  const int tiles_x = (W + CC_TW - 1) / CC_TW, tiles_y = (H + CC_TH - 1) / CC_TH;
  const long long n = (long long)H * W, items = cc_border_items(H, W);
  hipLaunchKernelGGL(components_tile_kernel, dim3((unsigned)((long long)tiles_x * tiles_y)), dim3(256), 0, stream, (const uint8_t*)plane, labels, H, W, tiles_x);
  if (items) {  // (a plane of one tile has no border, and its labels are roots already)
    hipLaunchKernelGGL(components_border_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, labels, H, W, items);
    hipLaunchKernelGGL(components_compress_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, labels, n);
  }
  return (int)hipGetLastError();
}

// ---- sums -------------------------------------------------------------------------------------------------------------------------
#define CC_MAX_BLOCKS 4096  // of the passes that walk the plane in a loop: 16 workgroups per CU, and at most that many atomics per counter

// A workgroup owns `span` consecutive pixels (a multiple of 256), a wave 64 neighbours of a row per trip.  One add per wave and distinct
// root - and a root that goes on from trip to trip (inside a large component: all of them) is added once, when it ends: `pend` is the
// wave's open (root, count), uniform over the wave.
__global__ __launch_bounds__(256) void components_sums_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ weight, int* __restrict__ sums,
                                                              long long n, long long span) {
  const long long begin = (long long)blockIdx.x * span, end = min(begin + span, n);
  const int lane = threadIdx.x & 63;
  int pend_root = -1, pend_count = 0;
  // ends: i grows by 256 per trip up to `end`; the trip count is the same for every lane of the workgroup
  for (long long i = begin; i < end; i += 256) {
    const long long p = i + threadIdx.x;
    int root = -1;
    if (p < end && (!weight || weight[p] != 0)) root = labels[p];
    if (root >= n) root = -1;  // (no label of ce_components_roots_i32: never an address)
    uint64_t left = __ballot(root >= 0);
    // ends: every round takes at least the leader's own bit out of `left`, so at most 64 rounds
    while (left) {
      const int leader = __ffsll((unsigned long long)left) - 1;
      const int r0 = __shfl(root, leader, 64);
      const uint64_t same = __ballot(root == r0) & left;
      if (r0 == pend_root) {
        pend_count += __popcll(same);
      } else {
        if (lane == 0 && pend_count) atomicAdd(sums + pend_root, pend_count);
        pend_root = r0, pend_count = __popcll(same);
      }
      left &= ~(same | (1ull << leader));
    }
  }
  if (lane == 0 && pend_count) atomicAdd(sums + pend_root, pend_count);
}

CE_API int ce_components_sums_i32(const int* labels, const void* weight, int* sums, int H, int W, hipStream_t stream) {
  if (!labels || !sums || labels == sums || weight == (const void*)labels || weight == (const void*)sums) return CE_ERR_ARG;
  if (const int e = components_shape(H, W)) return e;
  if (((uintptr_t)labels | (uintptr_t)sums) & 3) return CE_ERR_ALIGN;
  const long long n = (long long)H * W;
  const hipError_t z = hipMemsetAsync(sums, 0, (size_t)n * sizeof(int), stream);
  if (z != hipSuccess) return (int)z;
  const long long span = ((n + CC_MAX_BLOCKS - 1) / CC_MAX_BLOCKS + 255) / 256 * 256;
  hipLaunchKernelGGL(components_sums_kernel, dim3((unsigned)((n + span - 1) / span)), dim3(256), 0, stream, labels, (const uint8_t*)weight, sums, n, span);
  return (int)hipGetLastError();
}

// ---- keep -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

static unsigned components_loop_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < CC_MAX_BLOCKS ? b : CC_MAX_BLOCKS);
}

// counters[3] <- the largest weight at a root (counters zeroed by the call): per lane, per wave, per workgroup, one atomicMax
__global__ __launch_bounds__(256) void components_largest_kernel(const int* __restrict__ labels, const int* __restrict__ sums, int* __restrict__ counters,
                                                                 long long n) {
  __shared__ int part[4];
  int v = 0;
  // ends: p grows by a fixed positive stride up to n
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256)
    if (labels[p] == (int)p) v = max(v, sums[p]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = max(max(part[0], part[1]), max(part[2], part[3]));
    if (v > 0) atomicMax(counters + 3, v);
  }
}

// The least weight kept: min_weight, or (den > 0) ceil(num * largest / den) in 64-bit integers
__device__ __forceinline__ int components_threshold(const int* counters, int min_weight, int num, int den) {
  if (den <= 0) return min_weight;
  return (int)(((long long)num * counters[3] + den - 1) / den);
}

__global__ __launch_bounds__(256) void components_keep_kernel(const uint8_t* __restrict__ plane, const int* __restrict__ labels, const int* __restrict__ sums,
                                                              uint8_t* __restrict__ out, int* __restrict__ counters, int min_weight, int num, int den,
                                                              long long n) {
  __shared__ int part[4][3];
  const int thr = components_threshold(counters, min_weight, num, den);
  int kept = 0, dropped = 0, lost = 0;
  // ends: p grows by a fixed positive stride up to n
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
    const int label = labels[p];
    const int root = label < n ? label : -1;  // (no label of ce_components_roots_i32: never an address)
    const int w = root >= 0 ? sums[root] : 0;
    const bool keep = root >= 0 && w >= thr;
    out[p] = keep ? plane[p] : (uint8_t)0;
    if (root == (int)p) kept += keep, dropped += !keep, lost += keep ? 0 : w;
  }
  kept = wave_sum_i32(kept), dropped = wave_sum_i32(dropped), lost = wave_sum_i32(lost);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][0] = kept, part[threadIdx.x >> 6][1] = dropped, part[threadIdx.x >> 6][2] = lost;
  __syncthreads();
  if (threadIdx.x < 3) {  // lane j: counter j, one add per workgroup
    const int v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v) atomicAdd(counters + threadIdx.x, v);
  }
}

CE_API int ce_components_keep_u8(const void* plane, const int* labels, const int* sums, void* out, int* counters, int min_weight, int num, int den, int H,
                                 int W, hipStream_t stream) {
  if (!plane || !labels || !sums || !out || !counters) return CE_ERR_ARG;
  if (out == plane || out == (const void*)labels || out == (const void*)sums || out == (void*)counters) return CE_ERR_ARG;
  if (den < 0 || den > 65536 || (den == 0 && min_weight < 1) || (den > 0 && (num < 1 || num >= den))) return CE_ERR_ARG;
  if (const int e = components_shape(H, W)) return e;
  if (((uintptr_t)labels | (uintptr_t)sums | (uintptr_t)counters) & 3) return CE_ERR_ALIGN;
  const long long n = (long long)H * W;
  const hipError_t z = hipMemsetAsync(counters, 0, 4 * sizeof(int), stream);
  if (z != hipSuccess) return (int)z;
  const dim3 grid(components_loop_blocks(n));
  hipLaunchKernelGGL(components_largest_kernel, grid, dim3(256), 0, stream, labels, sums, counters, n);
  hipLaunchKernelGGL(components_keep_kernel, grid, dim3(256), 0, stream, (const uint8_t*)plane, labels, sums, (uint8_t*)out, counters, min_weight, num, den, n);
  return (int)hipGetLastError();
}

// ---- the automatic region's two passes (chronoedit_amd/auto_region.py) -------------------------------------------------------------
__global__ __launch_bounds__(256) void components_seeds_kernel(const float* __restrict__ d, const float* __restrict__ thr, uint8_t* __restrict__ seeds, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) seeds[i] = d[i] > thr[0] ? 255 : 0;  // (a NaN is no seed, as in the ramp pass)
}

__global__ __launch_bounds__(256) void components_masked_kernel(const float* __restrict__ d, const uint8_t* __restrict__ kept, float* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = kept[i] ? d[i] : -1.0f;
}

CE_API int ce_components_seeds_f32(const float* d, const float* thr, void* seeds, int n, hipStream_t stream) {
  if (!d || !thr || !seeds || n <= 0 || seeds == (const void*)d || seeds == (const void*)thr) return CE_ERR_ARG;
  if (((uintptr_t)d | (uintptr_t)thr) & 3) return CE_ERR_ALIGN;
  hipLaunchKernelGGL(components_seeds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d, thr, (uint8_t*)seeds, n);
  return (int)hipGetLastError();
}

CE_API int ce_components_masked_f32(const float* d, const void* kept, float* out, int n, hipStream_t stream) {
  if (!d || !kept || !out || n <= 0 || out == d || (const void*)out == kept) return CE_ERR_ARG;
  if (((uintptr_t)d | (uintptr_t)out) & 3) return CE_ERR_ALIGN;
  hipLaunchKernelGGL(components_masked_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d, (const uint8_t*)kept, out, n);
  return (int)hipGetLastError();
}

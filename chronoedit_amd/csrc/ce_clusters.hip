// Sketch edits with one crop per group of stroke clusters (chronoedit_amd/clusters.py is the definition; every pass here gives its bits).
// The clusters are the 8-connected components of the grown plane that ce_components.hip labels; what these passes add is what a host needs to
// turn them into crops, and what a photo needs to take several crops back:
//
//   ce_clusters_table_i32   labels, sums, kept -> one row per kept cluster, in ascending label order: label, the half-open bounding box of
//                           its pixels, their number, its weight.  Three launches and a 4-byte memset:
//                             append   a root position under a non-zero kept byte appends its label through ONE counter (the order of
//                                      arrival is whatever it is; the counter ends as the exact number of kept clusters)
//                             rank     one workgroup: a label's row is the number of smaller labels; every row is initialised here
//                             pixels   a workgroup reduces min / max / count of its run of pixels into a copy of the table in the LDS - a
//                                      wave whose pixels share one root reduces them in registers first, and keeps the sum open from trip
//                                      to trip - and flushes the rows it touched with global atomicMin / atomicMax / atomicAdd
//   ce_clusters_select_u8   labels, kept, table, group_of_row, g -> 255 under the kept pixels of the clusters of group g, else 0
//   ce_clusters_paste_u8    Image.paste(edit[f], (left, top), mask) into a canvas of F frames IN PLACE: the later crops of one photo
//
// Every loop ends by construction (the reason stands at the loop), no workgroup waits for another one, the phases are separate launches.
// Integers and integer atomics only: the results do not depend on the order of arrival.  No state; the scratch is the caller's.
#include "ce_common.h"

#define CL_ROWS 256           // rows of the table (clusters.ROWS)
#define CL_COLS 8             // label, left, top, right, bottom, pixels, weight, 0
#define CL_MAX_BLOCKS 4096    // of the passes that walk the plane in a loop
#define CL_NO_LABEL 0x7fffffff

// The row of `label` in the ascending list lab[0 .. CL_ROWS) (padded with CL_NO_LABEL), or -1.
__device__ __forceinline__ int clusters_find(const int* lab, int label) {
  int lo = 0;
  // ends: a fixed number of halvings, 128 down to 1; lo stays below CL_ROWS (it grows by at most 255 in all)
#pragma unroll
  for (int step = CL_ROWS / 2; step > 0; step >>= 1)
    if (lab[lo + step] <= label) lo += step;
  return lab[lo] == label ? lo : -1;
}

// ---- table ------------------------------------------------------------------------------------------------------------------------
// counters[0] (zeroed by the call) <- the number of kept clusters; counters[1 + slot] <- the label that drew `slot`, while slot < CL_ROWS
__global__ __launch_bounds__(256) void clusters_append_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ kept, int* __restrict__ counters,
                                                              long long n) {
  // ends: p grows by a fixed positive stride up to n
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
    if (labels[p] == (int)p && kept[p] != 0) {
      const int slot = atomicAdd(counters, 1);
      if (slot >= 0 && slot < CL_ROWS) counters[1 + slot] = (int)p;
    }
  }
}

// One workgroup, lane i = slot i and row i.  Labels are distinct, so the ranks of the c = min(count, CL_ROWS) labels are 0 .. c - 1.
__global__ __launch_bounds__(CL_ROWS) void clusters_rank_kernel(const int* __restrict__ sums, const int* __restrict__ counters, int* __restrict__ table,
                                                                int H, int W) {
  __shared__ int lab[CL_ROWS];
  const int i = threadIdx.x;
  const int c = min(max(counters[0], 0), CL_ROWS);
  const long long n = (long long)H * W;
  // (slot i < c was written by the append pass, with a pixel's index; the clamp keeps whatever else stands there from being an address)
  const int mine = i < c ? (int)min(max((long long)counters[1 + i], 0ll), n - 1) : CL_NO_LABEL;
  lab[i] = mine;
  __syncthreads();
  if (i >= c) {
    int* row = table + (size_t)i * CL_COLS;
#pragma unroll
    for (int k = 0; k < CL_COLS; ++k) row[k] = 0;
  } else {
    int rank = 0;
    // ends: c <= CL_ROWS trips
    for (int j = 0; j < c; ++j) rank += lab[j] < mine;
    int* r = table + (size_t)rank * CL_COLS;
    r[0] = mine, r[1] = W, r[2] = H, r[3] = 0, r[4] = 0, r[5] = 0, r[6] = sums[mine], r[7] = 0;
  }
}

struct ClusterBox {
  int l, t, r, b, n;
};

__device__ __forceinline__ void clusters_lds_add(int* acc, int row, const ClusterBox& v) {
  int* a = acc + row * 5;
  atomicMin(a + 0, v.l), atomicMin(a + 1, v.t), atomicMax(a + 2, v.r), atomicMax(a + 3, v.b), atomicAdd(a + 4, v.n);
}

// A workgroup owns `span` consecutive pixels (a multiple of 256), a wave 64 neighbours per trip.  `pend` is the wave's open (root, box,
// count), uniform over the wave: a wave inside one cluster - nearly all of them - touches the LDS once, when the root changes or the run ends.
__global__ __launch_bounds__(256) void clusters_pixels_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ kept, const int* __restrict__ counters,
                                                              int* __restrict__ table, int W, long long n, long long span) {
  __shared__ int lab[CL_ROWS];
  __shared__ int acc[CL_ROWS * 5];
  const int i = threadIdx.x;
  // (column 0 is the rank pass's; this pass changes columns 1 .. 5 only, and reads them nowhere)
  lab[i] = i < min(counters[0], CL_ROWS) ? table[(size_t)i * CL_COLS] : CL_NO_LABEL;
  acc[i * 5 + 0] = 0x7fffffff, acc[i * 5 + 1] = 0x7fffffff, acc[i * 5 + 2] = 0, acc[i * 5 + 3] = 0, acc[i * 5 + 4] = 0;
  __syncthreads();
  const long long begin = (long long)blockIdx.x * span, end = min(begin + span, n);
  const int lane = threadIdx.x & 63;
  int pend_root = -1;
  ClusterBox pend = {0, 0, 0, 0, 0};
  // ends: q grows by 256 per trip up to `end`; the trip count is the same for every lane of the workgroup
  for (long long q = begin; q < end; q += 256) {
    const long long p = q + threadIdx.x;
    int root = -1;
    if (p < end && kept[p] != 0) root = labels[p];
    if (root >= n) root = -1;  // (no label of ce_components_roots_i32)
    const uint64_t fg = __ballot(root >= 0);
    if (!fg) continue;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const int r0 = __shfl(root, __ffsll((unsigned long long)fg) - 1, 64);
    if (__ballot(root >= 0 && root != r0) == 0) {  // one root in this wave's 64 pixels: reduce in registers
      ClusterBox v = {root >= 0 ? x : 0x7fffffff, root >= 0 ? y : 0x7fffffff, root >= 0 ? x + 1 : 0, root >= 0 ? y + 1 : 0, 0};
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        v.l = min(v.l, __shfl_xor(v.l, o, 64)), v.t = min(v.t, __shfl_xor(v.t, o, 64));
        v.r = max(v.r, __shfl_xor(v.r, o, 64)), v.b = max(v.b, __shfl_xor(v.b, o, 64));
      }
      v.n = __popcll(fg);
      if (r0 == pend_root) {
        pend.l = min(pend.l, v.l), pend.t = min(pend.t, v.t), pend.r = max(pend.r, v.r), pend.b = max(pend.b, v.b), pend.n += v.n;
      } else {
        if (lane == 0 && pend_root >= 0) {
          const int row = clusters_find(lab, pend_root);
          if (row >= 0) clusters_lds_add(acc, row, pend);
        }
        pend_root = r0, pend = v;
      }
    } else if (root >= 0) {  // a wave across clusters: every pixel for itself
      const int row = clusters_find(lab, root);
      if (row >= 0) clusters_lds_add(acc, row, ClusterBox{x, y, x + 1, y + 1, 1});
    }
  }
  if (lane == 0 && pend_root >= 0) {
    const int row = clusters_find(lab, pend_root);
    if (row >= 0) clusters_lds_add(acc, row, pend);
  }
  __syncthreads();
  if (acc[i * 5 + 4] > 0) {  // lane i: row i, touched by this workgroup
    int* row = table + (size_t)i * CL_COLS;
    atomicMin(row + 1, acc[i * 5 + 0]), atomicMin(row + 2, acc[i * 5 + 1]), atomicMax(row + 3, acc[i * 5 + 2]), atomicMax(row + 4, acc[i * 5 + 3]);
    atomicAdd(row + 5, acc[i * 5 + 4]);
  }
}

static int clusters_shape(int H, int W) {
  if (H <= 0 || W <= 0) return CE_ERR_ARG;
  if ((long long)H * W >= (1ll << 31)) return CE_ERR_SHAPE;
  return CE_OK;
}

static unsigned clusters_loop_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < CL_MAX_BLOCKS ? b : CL_MAX_BLOCKS);
}

CE_API int ce_clusters_table_i32(const int* labels, const int* sums, const void* kept, int* table, int* counters, int rows, int H, int W,
                                 hipStream_t stream) {
  if (!labels || !sums || !kept || !table || !counters || rows != CL_ROWS) return CE_ERR_ARG;
  if (table == counters || table == labels || table == sums || counters == labels || counters == sums || kept == (const void*)table ||
      kept == (const void*)counters)
    return CE_ERR_ARG;
  if (const int e = clusters_shape(H, W)) return e;
  if (((uintptr_t)labels | (uintptr_t)sums | (uintptr_t)table | (uintptr_t)counters) & 3) return CE_ERR_ALIGN;
  const long long n = (long long)H * W;
  const hipError_t z = hipMemsetAsync(counters, 0, sizeof(int), stream);
  if (z != hipSuccess) return (int)z;
  hipLaunchKernelGGL(clusters_append_kernel, dim3(clusters_loop_blocks(n)), dim3(256), 0, stream, labels, (const uint8_t*)kept, counters, n);
  hipLaunchKernelGGL(clusters_rank_kernel, dim3(1), dim3(CL_ROWS), 0, stream, sums, (const int*)counters, table, H, W);
  const long long span = ((n + CL_MAX_BLOCKS - 1) / CL_MAX_BLOCKS + 255) / 256 * 256;
  hipLaunchKernelGGL(clusters_pixels_kernel, dim3((unsigned)((n + span - 1) / span)), dim3(256), 0, stream, labels, (const uint8_t*)kept, (const int*)counters,
                     table, W, n, span);
  return (int)hipGetLastError();
}

// ---- select -----------------------------------------------------------------------------------------------------------------------
// WIDE (labels 16-byte, kept and out 4-byte aligned): a lane owns four consecutive pixels - one 16-byte label load, one dword of kept
// bytes, one dword out; the plane's last 1 .. 3 pixels and the other path move single elements.  The same bytes come out.
template <bool WIDE>
__global__ __launch_bounds__(256) void clusters_select_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ kept, const int* __restrict__ table,
                                                              const int* __restrict__ group_of_row, int g, uint8_t* __restrict__ out, long long n) {
  __shared__ int lab[CL_ROWS];
  __shared__ int grp[CL_ROWS];
  {
    const int i = threadIdx.x;
    const int* row = table + (size_t)i * CL_COLS;
    lab[i] = row[5] > 0 ? row[0] : CL_NO_LABEL;  // (the rows with pixels are the first ones, in ascending label order)
    grp[i] = group_of_row[i];
  }
  __syncthreads();
  // ends: b0 grows by a fixed positive stride up to n
  for (long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; b0 < n; b0 += (long long)gridDim.x * 1024) {
    int L[4] = {-1, -1, -1, -1};
    uint32_t k = 0;
    const int nb = (int)(n - b0 < 4 ? n - b0 : 4);
    if (WIDE && nb == 4) {
      const int4 v = *(const int4*)(labels + b0);
      L[0] = v.x, L[1] = v.y, L[2] = v.z, L[3] = v.w;
      k = *(const uint32_t*)(kept + b0);
    } else {
      for (int j = 0; j < nb; ++j) L[j] = labels[b0 + j], k |= (uint32_t)kept[b0 + j] << (8 * j);
    }
    uint32_t o = 0;
    int last = -1, hit = 0;  // (neighbours mostly share their root: one search for a run of equal labels)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nb && L[j] >= 0 && ((k >> (8 * j)) & 255u)) {
        if (L[j] != last) {
          const int row = clusters_find(lab, L[j]);
          last = L[j], hit = row >= 0 && grp[row] == g;
        }
        if (hit) o |= 255u << (8 * j);
      }
    }
    if (WIDE && nb == 4) {
      *(uint32_t*)(out + b0) = o;
    } else {
      for (int j = 0; j < nb; ++j) out[b0 + j] = (uint8_t)(o >> (8 * j));
    }
  }
}

CE_API int ce_clusters_select_u8(const int* labels, const void* kept, const int* table, const int* group_of_row, int g, void* out, int H, int W,
                                 hipStream_t stream) {
  if (!labels || !kept || !table || !group_of_row || !out || g < 0) return CE_ERR_ARG;
  if (out == kept || out == (const void*)labels || out == (const void*)table || out == (const void*)group_of_row) return CE_ERR_ARG;
  if (const int e = clusters_shape(H, W)) return e;
  if (((uintptr_t)labels | (uintptr_t)table | (uintptr_t)group_of_row) & 3) return CE_ERR_ALIGN;
  const long long n = (long long)H * W;
  const dim3 grid(clusters_loop_blocks((n + 3) / 4));
  if (!((uintptr_t)labels & 15) && !(((uintptr_t)kept | (uintptr_t)out) & 3))
    hipLaunchKernelGGL(clusters_select_kernel<true>, grid, dim3(256), 0, stream, labels, (const uint8_t*)kept, table, group_of_row, g, (uint8_t*)out, n);
  else
    hipLaunchKernelGGL(clusters_select_kernel<false>, grid, dim3(256), 0, stream, labels, (const uint8_t*)kept, table, group_of_row, g, (uint8_t*)out, n);
  return (int)hipGetLastError();
}

// ---- paste ------------------------------------------------------------------------------------------------------------------------
// One lane per pixel of the box (blockIdx.y = frame): its mask byte, then its three bytes of the canvas and of the edit.  A pixel under a
// mask byte of 0 is left as it is.  The arithmetic is ce_focus_paste_u8's.
__global__ __launch_bounds__(256) void clusters_paste_kernel(const uint8_t* __restrict__ edit, const uint8_t* __restrict__ mask, uint8_t* __restrict__ canvas,
                                                             int SH, int SW, int left, int top, int bw, int bh) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= (long long)bw * bh) return;
  const int y = (int)(k / bw), x = (int)(k - (long long)y * bw);
  const size_t px = (size_t)(top + y) * SW + left + x;
  const uint32_t m = mask ? (uint32_t)mask[px] : 255u;
  if (!m) return;
  const uint8_t* e = edit + ((size_t)blockIdx.y * bh * bw + (size_t)k) * 3;
  uint8_t* c = canvas + ((size_t)blockIdx.y * SH * SW + px) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t t = (uint32_t)c[ch] * (255u - m) + (uint32_t)e[ch] * m + 128u;
    c[ch] = (uint8_t)(((t >> 8) + t) >> 8);
  }
}

CE_API int ce_clusters_paste_u8(const void* edit, const void* mask, void* canvas, int F, int src_h, int src_w, int left, int top, int bw, int bh,
                                hipStream_t stream) {
  if (!edit || !canvas || canvas == edit || canvas == mask) return CE_ERR_ARG;
  if (F <= 0 || F > 65535 || src_h <= 0 || src_w <= 0 || bw <= 0 || bh <= 0) return CE_ERR_ARG;
  if (left < 0 || top < 0 || (long long)left + bw > src_w || (long long)top + bh > src_h) return CE_ERR_ARG;  // the box lies inside the image
  if ((long long)src_h * src_w * 3 >= (1ll << 31)) return CE_ERR_SHAPE;
  const long long pixels = (long long)bw * bh;
  hipLaunchKernelGGL(clusters_paste_kernel, dim3((unsigned)((pixels + 255) / 256), (unsigned)F), dim3(256), 0, stream, (const uint8_t*)edit,
                     (const uint8_t*)mask, (uint8_t*)canvas, src_h, src_w, left, top, bw, bh);
  return (int)hipGetLastError();
}

// Sparse region edits (chronoedit_amd/sparse_region.py): the gather / scatter layer around the unchanged GEMM and attention kernels.
// A sparse step runs the DiT on Na ACTIVE token rows per sample (ids = their sorted, unique token indices in [0, N), the same for every
// sample) and keeps every layer's K and V^T of all N tokens in a per-edit cache that the self-attention reads.
//
//   ce_sparse_patchify_bf16       x [C][T][H][W], ids -> cols [Na][Kpad]: the rows ce_patchify_bf16 gives for the listed tokens.
//   ce_sparse_scatter_rows_bf16   src [B*Na][lds] -> dst [B*N][ldd]: row b*Na + a goes to row b*N + ids[a] (K after norm + RoPE).
//   ce_sparse_scatter_vt_bf16     fresh V of the active tokens -> columns b*N + ids[a] of the cached V^T [D][ldvt]; the source is V^T
//                                 [D][lds] (column b*Na + a: what the transposed-store GEMM leaves) or row-major V [B*Na][lds].
//   ce_sparse_unpatchify_bf16     head rows y [Na][ldy], ids -> the 2 x 2 cells of those tokens in out [Cout][T][H][W].
//
// Pure data movement: every pass is bit-equal to its indexing expression, and nothing outside the listed rows / columns / cells is written.
// ids are int32 or int64 (ids_i64) in device memory; the host validates them once per edit (sparse_region.validate_ids).  An id outside
// [0, N) is skipped by every pass all the same - one unsigned compare keeps a stale list from writing out of bounds.
//
// Thread mappings follow the way active ids come - in runs along W.  Row passes: consecutive lanes own consecutive 16-byte chunks of one
// row (a D = 5120 row is 160 lanes of contiguous traffic on both sides).  Column passes (V^T, unpatchify): consecutive lanes own
// consecutive ids, so a run of ids is a run of consecutive 2-byte columns on the scattered side and the other side is contiguous.
// No scratch, no state, nothing allocated, no host read: every call is capturable.
#include "ce_common.h"

namespace {

template <typename I>
__device__ __forceinline__ long long sparse_id(const void* ids, int a) { return (long long)((const I*)ids)[a]; }

// one lane per element of cols [Na][Kpad], k = c*4 + dh*2 + dw fastest (the order of patchify_kernel, csrc/ce_rowops.hip)
template <typename I>
__global__ __launch_bounds__(256) void sparse_patchify_kernel(const bf16* __restrict__ x, const void* __restrict__ ids, bf16* __restrict__ cols,
                                                              int C, int T, int H, int W, int Kpad, int Na) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Na * Kpad) return;
  const int k = (int)(idx % Kpad), a = (int)(idx / Kpad);
  const int h2 = H >> 1, w2 = W >> 1;
  const long long tok = sparse_id<I>(ids, a);
  bf16 v = (bf16)0.f;
  if (k < C * 4 && (unsigned long long)tok < (unsigned long long)T * h2 * w2) {
    const int c = k >> 2, dh = (k >> 1) & 1, dw = k & 1;
    const int wq = (int)(tok % w2), hq = (int)((tok / w2) % h2), t = (int)(tok / ((long long)w2 * h2));
    v = x[(((size_t)c * T + t) * H + (hq * 2 + dh)) * W + wq * 2 + dw];
  }
  cols[idx] = v;
}

// one lane per 16-byte chunk of a source row; chunks of a row are consecutive lanes
template <typename I>
__global__ __launch_bounds__(256) void sparse_scatter_rows_kernel(const bf16* __restrict__ src, int lds, bf16* __restrict__ dst, int ldd,
                                                                  const void* __restrict__ ids, int Na, int N, int B, int chunks) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)B * Na * chunks) return;
  const int ch = (int)(g % chunks);
  const long long r = g / chunks;  // b*Na + a
  const int a = (int)(r % Na), b = (int)(r / Na);
  const long long tok = sparse_id<I>(ids, a);
  if ((unsigned long long)tok >= (unsigned long long)N) return;
  const u32x4 v = *(const u32x4*)(src + (size_t)r * lds + (size_t)ch * 8);
  *(u32x4*)(dst + ((size_t)b * N + (size_t)tok) * ldd + (size_t)ch * 8) = v;
}

// source V^T [D][lds]: one lane per (d, b, a), a fastest - a contiguous read, and one contiguous 2-byte column run per run of ids
template <typename I>
__global__ __launch_bounds__(256) void sparse_scatter_vt_kernel(const bf16* __restrict__ src, int lds, bf16* __restrict__ vt, int ldvt,
                                                                const void* __restrict__ ids, int Na, int N, int B, int D) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)B * Na;
  if (g >= per * D) return;
  const int c = (int)(g % per), d = (int)(g / per);  // c = b*Na + a
  const int a = c % Na, b = c / Na;
  const long long tok = sparse_id<I>(ids, a);
  if ((unsigned long long)tok >= (unsigned long long)N) return;
  vt[(size_t)d * ldvt + (size_t)b * N + (size_t)tok] = src[(size_t)d * lds + c];
}

// source row-major V [B*Na][lds]: a 64 (rows) x 64 (channels) tile through LDS - read with lanes along the channels, written with lanes
// along the ids (the +1 column keeps the transposed read off one bank)
template <typename I>
__global__ __launch_bounds__(256) void sparse_scatter_vt_rows_kernel(const bf16* __restrict__ src, int lds, bf16* __restrict__ vt, int ldvt,
                                                                     const void* __restrict__ ids, int Na, int N, int B, int D) {
  __shared__ uint16_t tile[64][65];
  const int r0 = blockIdx.x * 64, d0 = blockIdx.y * 64;
  const int rows = B * Na;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;  // 4 groups of 64 lanes
  const uint16_t* s = (const uint16_t*)src;
  for (int i = grp; i < 64; i += 4) {
    const int r = r0 + i, d = d0 + lane;
    tile[i][lane] = (r < rows && d < D) ? s[(size_t)r * lds + d] : (uint16_t)0;
  }
  __syncthreads();
  const int r = r0 + lane;
  if (r >= rows) return;
  const int a = r % Na, b = r / Na;
  const long long tok = sparse_id<I>(ids, a);
  if ((unsigned long long)tok >= (unsigned long long)N) return;
  uint16_t* o = (uint16_t*)vt + (size_t)b * N + (size_t)tok;
  for (int j = grp; j < 64; j += 4)
    if (d0 + j < D) o[(size_t)(d0 + j) * ldvt] = tile[lane][j];
}

// one lane per output element of the listed tokens: (c, dh, a, dw), dw fastest then a - a run of ids is a run of consecutive w
template <typename I>
__global__ __launch_bounds__(256) void sparse_unpatchify_kernel(const bf16* __restrict__ y, int ldy, const void* __restrict__ ids,
                                                                bf16* __restrict__ out, int Cout, int T, int H, int W, int Na) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Cout * 4 * Na) return;
  const int dw = (int)(idx & 1);
  const int a = (int)((idx >> 1) % Na);
  const int q = (int)((idx >> 1) / Na);  // c*2 + dh
  const int dh = q & 1, c = q >> 1;
  const int h2 = H >> 1, w2 = W >> 1;
  const long long tok = sparse_id<I>(ids, a);
  if ((unsigned long long)tok >= (unsigned long long)T * h2 * w2) return;
  const int wq = (int)(tok % w2), hq = (int)((tok / w2) % h2), t = (int)(tok / ((long long)w2 * h2));
  out[(((size_t)c * T + t) * H + (hq * 2 + dh)) * W + wq * 2 + dw] = y[(size_t)a * ldy + (dh * 2 + dw) * Cout + c];
}

inline bool sparse_grid(long long work, unsigned* blocks) {
  const long long b = (work + 255) / 256;
  if (b <= 0 || b > 0x7fffffffll) return false;
  *blocks = (unsigned)b;
  return true;
}

}  // namespace

CE_API int ce_sparse_patchify_bf16(const void* x, const void* ids, int ids_i64, void* cols, int C, int T, int H, int W, int Kpad, int Na,
                                   hipStream_t stream) {
  if (!x || !ids || !cols || C <= 0 || T <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || Kpad < C * 4 || Na <= 0) return CE_ERR_ARG;
  if ((long long)T * (H / 2) * (W / 2) >= (1ll << 31)) return CE_ERR_SHAPE;
  if ((uintptr_t)ids & (ids_i64 ? 7 : 3)) return CE_ERR_ALIGN;
  unsigned blocks;
  if (!sparse_grid((long long)Na * Kpad, &blocks)) return CE_ERR_SHAPE;
  if (ids_i64)
    hipLaunchKernelGGL(sparse_patchify_kernel<long long>, dim3(blocks), dim3(256), 0, stream, (const bf16*)x, ids, (bf16*)cols, C, T, H, W, Kpad, Na);
  else
    hipLaunchKernelGGL(sparse_patchify_kernel<int>, dim3(blocks), dim3(256), 0, stream, (const bf16*)x, ids, (bf16*)cols, C, T, H, W, Kpad, Na);
  return (int)hipGetLastError();
}

CE_API int ce_sparse_scatter_rows_bf16(const void* src, int lds, void* dst, int ldd, const void* ids, int ids_i64, int Na, int N, int B,
                                       int D, hipStream_t stream) {
  if (!src || !dst || !ids || src == (const void*)dst || Na <= 0 || N <= 0 || Na > N || B <= 0 || D <= 0) return CE_ERR_ARG;
  if ((D & 7) || lds < D || ldd < D || (long long)B * N >= (1ll << 31)) return CE_ERR_SHAPE;
  if ((lds & 7) || (ldd & 7) || (((uintptr_t)src | (uintptr_t)dst) & 15) || ((uintptr_t)ids & (ids_i64 ? 7 : 3))) return CE_ERR_ALIGN;
  unsigned blocks;
  if (!sparse_grid((long long)B * Na * (D / 8), &blocks)) return CE_ERR_SHAPE;
  if (ids_i64)
    hipLaunchKernelGGL(sparse_scatter_rows_kernel<long long>, dim3(blocks), dim3(256), 0, stream, (const bf16*)src, lds, (bf16*)dst, ldd, ids, Na, N, B, D / 8);
  else
    hipLaunchKernelGGL(sparse_scatter_rows_kernel<int>, dim3(blocks), dim3(256), 0, stream, (const bf16*)src, lds, (bf16*)dst, ldd, ids, Na, N, B, D / 8);
  return (int)hipGetLastError();
}

CE_API int ce_sparse_scatter_vt_bf16(const void* src, int lds, int src_rows, void* vt, int ldvt, const void* ids, int ids_i64, int Na, int N,
                                     int B, int D, hipStream_t stream) {
  if (!src || !vt || !ids || src == (const void*)vt || Na <= 0 || N <= 0 || Na > N || B <= 0 || D <= 0) return CE_ERR_ARG;
  if ((long long)B * N >= (1ll << 31) || ldvt < (long long)B * N || lds < (src_rows ? D : (long long)B * Na)) return CE_ERR_SHAPE;
  if ((((uintptr_t)src | (uintptr_t)vt) & 1) || ((uintptr_t)ids & (ids_i64 ? 7 : 3))) return CE_ERR_ALIGN;
  if (src_rows) {
    const long long rb = ((long long)B * Na + 63) / 64, db = (D + 63) / 64;
    if (rb > 0x7fffffffll || db > 65535) return CE_ERR_SHAPE;
    const dim3 grid((unsigned)rb, (unsigned)db);
    if (ids_i64)
      hipLaunchKernelGGL(sparse_scatter_vt_rows_kernel<long long>, grid, dim3(256), 0, stream, (const bf16*)src, lds, (bf16*)vt, ldvt, ids, Na, N, B, D);
    else
      hipLaunchKernelGGL(sparse_scatter_vt_rows_kernel<int>, grid, dim3(256), 0, stream, (const bf16*)src, lds, (bf16*)vt, ldvt, ids, Na, N, B, D);
    return (int)hipGetLastError();
  }
  unsigned blocks;
  if (!sparse_grid((long long)B * Na * D, &blocks)) return CE_ERR_SHAPE;
  if (ids_i64)
    hipLaunchKernelGGL(sparse_scatter_vt_kernel<long long>, dim3(blocks), dim3(256), 0, stream, (const bf16*)src, lds, (bf16*)vt, ldvt, ids, Na, N, B, D);
  else
    hipLaunchKernelGGL(sparse_scatter_vt_kernel<int>, dim3(blocks), dim3(256), 0, stream, (const bf16*)src, lds, (bf16*)vt, ldvt, ids, Na, N, B, D);
  return (int)hipGetLastError();
}

CE_API int ce_sparse_unpatchify_bf16(const void* y, int ldy, const void* ids, int ids_i64, void* out, int Cout, int T, int H, int W, int Na,
                                     hipStream_t stream) {
  if (!y || !ids || !out || Cout <= 0 || T <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || ldy < 4 * Cout || Na <= 0) return CE_ERR_ARG;
  if ((long long)T * (H / 2) * (W / 2) >= (1ll << 31)) return CE_ERR_SHAPE;
  if ((uintptr_t)ids & (ids_i64 ? 7 : 3)) return CE_ERR_ALIGN;
  unsigned blocks;
  if (!sparse_grid((long long)Cout * 4 * Na, &blocks)) return CE_ERR_SHAPE;
  if (ids_i64)
    hipLaunchKernelGGL(sparse_unpatchify_kernel<long long>, dim3(blocks), dim3(256), 0, stream, (const bf16*)y, ldy, ids, (bf16*)out, Cout, T, H, W, Na);
  else
    hipLaunchKernelGGL(sparse_unpatchify_kernel<int>, dim3(blocks), dim3(256), 0, stream, (const bf16*)y, ldy, ids, (bf16*)out, Cout, T, H, W, Na);
  return (int)hipGetLastError();
}

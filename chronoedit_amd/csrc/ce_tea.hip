// TeaCache step skipping (wan_video_new_chronoedit.py:1190-1239): the three device passes behind chronoedit_amd/teacache.py.
//
//   ce_tea_rel_l1_bf16   per scheduled step i >= 1: sum_j |bf16(T[i][j] - T[i-1][j])| and sum_j |T[i-1][j]| over the rows of the stacked
//                        time-projection outputs (:1219, the numerator and denominator of the relative L1 distance; the means and
//                        the quotient are three bf16 roundings on the host).  One workgroup per row, fp32 accumulation in a fixed order
//                        (lane-serial, butterfly within a wave, the four waves in order): the same bits on every run.
//   ce_tea_store_bf16    r <- bf16(x - r)  (:1233-1235, previous_residual = hidden_states - previous_hidden_states), in place on the saved
//                        patch-embedded tokens.
//   ce_tea_apply_bf16    x <- bf16(x + r)  (:1237-1239, hidden_states + previous_residual), in place on the token matrix.
//
//   ce_tea_store_dist_bf16   calibration (teacache.fit_coefficients): the store pass that also measures how far the new residual is from the
//                        previous step's - sum |r_new - prev| and sum |prev| over all elements, the numerator and denominator of the
//                        quantity a skipped step gets wrong.  Same residual bits as ce_tea_store_bf16; fp32 sums in a fixed order.
//
// The token passes are HBM-bound streams (2 reads + 1 write of 2 bytes per element, the measuring pass 3 reads + 1 write): 16-byte
// accesses, two vectors of each operand in flight per lane, at most 2048 workgroups that grid-stride the rest.
#include "ce_common.h"

template <bool SUB>
__device__ __forceinline__ u32x4 tea_combine(const u32x4 a, const u32x4 b) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float al = bf16lo(a[k]), ah = bf16hi(a[k]), bl = bf16lo(b[k]), bh = bf16hi(b[k]);
    o[k] = SUB ? pack_bf16(al - bl, ah - bh) : pack_bf16(al + bl, ah + bh);
  }
  return o;
}

// SUB: r = x - r (written to r); otherwise x = x + r (written to x).  The destination aliases one source element for element: every
// lane reads its own 16 bytes before it writes them, no other lane touches them.
template <bool SUB>
__global__ __launch_bounds__(256) void tea_token_kernel(u32x4* x, u32x4* r, long long nv) {
  const long long stride = (long long)gridDim.x * 256;
  u32x4* dst = SUB ? r : x;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < nv; i += 2 * stride) {
    const u32x4 a0 = x[i], b0 = r[i], a1 = x[i + stride], b1 = r[i + stride];
    dst[i] = tea_combine<SUB>(a0, b0);
    dst[i + stride] = tea_combine<SUB>(a1, b1);
  }
  if (i < nv) dst[i] = tea_combine<SUB>(x[i], r[i]);
}

template <bool SUB>
static int tea_token_launch(void* x, void* r, long long count, hipStream_t stream) {
  if (!x || !r || count <= 0) return CE_ERR_ARG;
  if (count % 8) return CE_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)r) & 15) return CE_ERR_ALIGN;
  const long long nv = count / 8;
  long long blocks = (nv + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(tea_token_kernel<SUB>, dim3((unsigned)blocks), dim3(256), 0, stream, (u32x4*)x, (u32x4*)r, nv);
  return (int)hipGetLastError();
}

CE_API int ce_tea_store_bf16(const void* x, void* r, long long count, hipStream_t stream) {
  return tea_token_launch<true>(const_cast<void*>(x), r, count, stream);
}

CE_API int ce_tea_apply_bf16(void* x, const void* r, long long count, hipStream_t stream) {
  return tea_token_launch<false>(x, const_cast<void*>(r), count, stream);
}

// The store pass with the two distance sums.  Every sum is taken in an order that `count` alone decides: a lane adds its elements one by one
// in index order (vector by vector along its grid stride), the 64 lanes of a wave meet in a butterfly, the four waves are added in order, the
// workgroup's pair goes to part[2 * block], and tea_dist_finish_kernel adds the workgroups' pairs.  No atomics: the same bits on every run.
__device__ __forceinline__ u32x4 tea_store_dist(const u32x4 a, const u32x4 b, const u32x4 q, float& sd, float& sp) {
  const u32x4 o = tea_combine<true>(a, b);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ql = bf16lo(q[k]), qh = bf16hi(q[k]);
    sd += fabsf(bf16lo(o[k]) - ql);  // the STORED (bf16) residual against the previous one, the difference itself stays fp32
    sd += fabsf(bf16hi(o[k]) - qh);
    sp += fabsf(ql);
    sp += fabsf(qh);
  }
  return o;
}

__global__ __launch_bounds__(256) void tea_store_dist_kernel(const u32x4* x, u32x4* r, const u32x4* prev, float* part, long long nv) {
  __shared__ float wv[2][4];
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float sd = 0.0f, sp = 0.0f;
  for (; i + stride < nv; i += 2 * stride) {
    const u32x4 a0 = x[i], b0 = r[i], q0 = prev[i], a1 = x[i + stride], b1 = r[i + stride], q1 = prev[i + stride];
    r[i] = tea_store_dist(a0, b0, q0, sd, sp);
    r[i + stride] = tea_store_dist(a1, b1, q1, sd, sp);
  }
  if (i < nv) r[i] = tea_store_dist(x[i], r[i], prev[i], sd, sp);
  sd = wave_sum(sd);
  sp = wave_sum(sp);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    wv[0][wave] = sd;
    wv[1][wave] = sp;
  }
  __syncthreads();
  if (threadIdx.x < 2) part[2 * blockIdx.x + threadIdx.x] = ((wv[threadIdx.x][0] + wv[threadIdx.x][1]) + wv[threadIdx.x][2]) + wv[threadIdx.x][3];
}

// wave w adds column w of the `nparts` workgroup pairs: lane l takes pairs l, l + 64, ... in index order, then the butterfly
__global__ __launch_bounds__(128) void tea_dist_finish_kernel(const float* __restrict__ part, int nparts, float* __restrict__ sums) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float s = 0.0f;
  for (int j = lane; j < nparts; j += 64) s += part[2 * j + w];
  s = wave_sum(s);
  if (lane == 0) sums[w] = s;
}

static bool tea_overlap(const void* a, const void* b, long long bytes) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + (uintptr_t)bytes && q < p + (uintptr_t)bytes;
}

CE_API int ce_tea_store_dist_bf16(const void* x, void* r, const void* prev, float* sums, float* scratch, long long scratch_bytes, long long count,
                                  hipStream_t stream) {
  if (!x || !r || !prev || !sums || !scratch || count <= 0) return CE_ERR_ARG;
  if (count % 8) return CE_ERR_SHAPE;
  if ((((uintptr_t)x | (uintptr_t)r | (uintptr_t)prev) & 15) || (((uintptr_t)sums | (uintptr_t)scratch) & 3)) return CE_ERR_ALIGN;
  const long long nv = count / 8;
  long long blocks = (nv + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (scratch_bytes < blocks * 2 * (long long)sizeof(float)) return CE_ERR_ARG;
  if (tea_overlap(prev, r, count * 2) || tea_overlap(prev, x, count * 2)) return CE_ERR_ARG;  // prev is read after r has been written
  hipLaunchKernelGGL(tea_store_dist_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const u32x4*)x, (u32x4*)r, (const u32x4*)prev, scratch, nv);
  hipLaunchKernelGGL(tea_dist_finish_kernel, dim3(1), dim3(128), 0, stream, (const float*)scratch, (int)blocks, sums);
  return (int)hipGetLastError();
}

// block i: row i against row i - 1 (block 0 writes the zero row)
__global__ __launch_bounds__(256) void tea_rel_l1_kernel(const u32x4* __restrict__ T, float* __restrict__ out, int nv) {
  __shared__ float part[2][4];
  const int row = blockIdx.x;
  if (row == 0) {
    if (threadIdx.x < 2) out[threadIdx.x] = 0.0f;
    return;
  }
  const u32x4* cur = T + (size_t)row * nv;
  const u32x4* prev = cur - nv;
  float sd = 0.0f, sp = 0.0f;
  for (int v = threadIdx.x; v < nv; v += 256) {
    const u32x4 c = cur[v], p = prev[v];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float pl = bf16lo(p[k]), ph = bf16hi(p[k]);
      sd += fabsf(round_bf16(bf16lo(c[k]) - pl));  // the reference subtracts bf16 tensors: the difference is a bf16 value
      sd += fabsf(round_bf16(bf16hi(c[k]) - ph));
      sp += fabsf(pl);
      sp += fabsf(ph);
    }
  }
  sd = wave_sum(sd);
  sp = wave_sum(sp);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[0][wave] = sd;
    part[1][wave] = sp;
  }
  __syncthreads();
  if (threadIdx.x < 2) out[2 * row + threadIdx.x] = ((part[threadIdx.x][0] + part[threadIdx.x][1]) + part[threadIdx.x][2]) + part[threadIdx.x][3];
}

CE_API int ce_tea_rel_l1_bf16(const void* T, int S, int n, float* out, hipStream_t stream) {
  if (!T || !out || S <= 0 || n <= 0) return CE_ERR_ARG;
  if (n % 8) return CE_ERR_SHAPE;
  if (((uintptr_t)T & 15) || ((uintptr_t)out & 3)) return CE_ERR_ALIGN;
  hipLaunchKernelGGL(tea_rel_l1_kernel, dim3((unsigned)S), dim3(256), 0, stream, (const u32x4*)T, out, n / 8);
  return (int)hipGetLastError();
}

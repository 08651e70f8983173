// Weight-side LoRA merge: W = bf16_rne(fp32(W0) + sum_i scales[i] * (B_i . A_i)), the kernel behind switching adapters between
// edits (chronoedit_amd/weights.py LoraMixin.set_adapters / disable_lora).  Replaces the host-side `b.float() @ a.float()` of
// fuse_lora (PEFT's merge through diffusers, scripts/run_inference_diffusers.py:349-376) on the switchable path.
//
// Bound: HBM streaming (read W0, write W: 4 bytes per element) plus 2*N*K*R flops of rank products on the bf16 MFMA; B [N, R] and
// A [R, K] are small (L2 resident across the grid).  Measured on the MI355X at the 14B block shapes (profiles/notes_lora.md): 3.4 TB/s
// with no adapter (a plain copy reaches 5.1), 2.8 at rank 32, 2.1 at rank 128 - 19 / 23 / 31 ms for all 40 blocks.  What holds it
// below the copy rate is this kernel's LDS work, not HBM: the 2-byte reads and writes at accumulator positions, and per 32-rank
// chunk a barrier and sixteen 2-byte transposing writes per lane.
//
// Kernel: one workgroup of 4 waves (2 x 2) per 128 x 128 tile of W, each wave a 64 x 64 sub-tile as 4 x 4 accumulators of
// v_mfma_f32_16x16x32_bf16 (M axis = rows n of W, fed by B; N axis = columns k of W, fed by A; contraction = the rank).
//   * the W0 tile comes in with 16-byte row-contiguous loads into LDS; every lane takes the elements at ITS accumulator positions from
//     there as the fp32 running sum, and the rounded result goes back to the same LDS slots and out with 16-byte row-contiguous stores.
//     The whole tile of W0 is read before the first store, so W may alias W0.
//   * B fragments are 8 consecutive ranks of one row: a 16-byte global load per lane, no staging.
//   * A is [R, K]: the contraction index is the SLOW axis, the MFMA operand wants it fastest.  Each 32-rank chunk of the tile's 128
//     columns is transposed on its way into LDS (16-byte global loads, 2-byte LDS writes into [k][rank] rows of 80 bytes; the fragment
//     reads are then conflict-free ds_read_b128), double-buffered: one barrier per chunk.
//   * per adapter a fresh fp32 dot accumulator; after its last chunk sum = sum + scale * dot (a multiply and an add, as the contract
//     states), adapters in order; one rounding to bf16 at the end.
#include "ce_common.h"

namespace {

constexpr int TN = 128, TK = 128, RC = 32;
constexpr int MAX_ADAPTERS = 8;
constexpr int W_LD = TK * 2 + 16;    // bytes per staged W row: +16 keeps the 2-byte reads at accumulator positions off one bank
constexpr int AT_LD = (RC + 8) * 2;  // bytes per [k] row of the transposed A chunk (80: 16-byte aligned, b128 reads conflict-free)

struct LoraArgs {
  const bf16* B[MAX_ADAPTERS];
  const bf16* A[MAX_ADAPTERS];
  int rank[MAX_ADAPTERS];
  float scale[MAX_ADAPTERS];
  int n;
};

__global__ __launch_bounds__(256, 2) void lora_merge_kernel(const bf16* W0, int ldw0, bf16* W, int ldw, int N, int K,
                                                          int tiles_k, LoraArgs args) {
  __shared__ __attribute__((aligned(16))) unsigned char sW[TN * W_LD];
  __shared__ __attribute__((aligned(16))) unsigned char sA[2][TK * AT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = (blockIdx.x / tiles_k) * TN, k0 = (blockIdx.x % tiles_k) * TK;

  // ---- W0 tile -> LDS (16 B per lane, row-contiguous; rows >= N and columns >= K as zeros, never stored)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int c = tid + 256 * t;
    const int rl = c >> 4, cc = c & 15;
    const int n = n0 + rl, k = k0 + cc * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n < N && k < K) v = *reinterpret_cast<const u32x4*>(W0 + (size_t)n * ldw0 + k);
    *reinterpret_cast<u32x4*>(sW + rl * W_LD + cc * 16) = v;
  }
  __syncthreads();

  // C fragment layout (16x16x32): column = lane & 15, row = 4 * (lane >> 4) + reg
  f32x4 sum[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wm * 64 + i * 16 + fg * 4 + r, cl = wn * 64 + j * 16 + fr;
        sum[i][j][r] = bf16_bits_to_f32(*reinterpret_cast<const uint16_t*>(sW + rl * W_LD + cl * 2));
      }

  // staging map of one A chunk [32 ranks][128 columns] = 512 pieces of 16 B, two per thread: piece p = (k chunk, rank)
  int st_r[2], st_kc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int p = tid + 256 * q;
    st_r[q] = (p >> 2) & 31;
    st_kc[q] = ((p >> 7) << 2) | (p & 3);
  }
  int b_row[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) b_row[i] = min(n0 + wm * 64 + i * 16 + fr, N - 1);

  int it = 0;
  for (int a = 0; a < args.n; ++a) {
    const bf16* __restrict__ Ba = args.B[a];
    const bf16* __restrict__ Aa = args.A[a];
    const int R = args.rank[a];
    f32x4 dot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < R; c0 += RC, ++it) {
      unsigned char* buf = sA[it & 1];
      u32x4 ra[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int k = k0 + st_kc[q] * 8;
        ra[q] = u32x4{0u, 0u, 0u, 0u};
        if (k < K) ra[q] = *reinterpret_cast<const u32x4*>(Aa + (size_t)(c0 + st_r[q]) * K + k);
      }
      bf16x8 bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) bfr[i] = *reinterpret_cast<const bf16x8*>(Ba + (size_t)b_row[i] * R + c0 + fg * 8);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        unsigned char* d = buf + (st_kc[q] * 8) * AT_LD + st_r[q] * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          *reinterpret_cast<uint16_t*>(d + (2 * e) * AT_LD) = (uint16_t)(ra[q][e] & 0xffffu);
          *reinterpret_cast<uint16_t*>(d + (2 * e + 1) * AT_LD) = (uint16_t)(ra[q][e] >> 16);
        }
      }
      // one barrier per chunk: the buffer written here was last read two chunks ago, and every thread has passed the barrier of
      // the chunk in between since
      __syncthreads();
      bf16x8 afr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        afr[j] = *reinterpret_cast<const bf16x8*>(buf + (wn * 64 + j * 16 + fr) * AT_LD + fg * 16);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dot[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[i], afr[j], dot[i][j], 0, 0, 0);
    }
    const float s = args.scale[a];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[i][j][r] = mul_then_add(dot[i][j][r], s, sum[i][j][r]);
  }

  // ---- bf16(sum) back to the lane's own LDS slots, then 16-byte row-contiguous stores
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wm * 64 + i * 16 + fg * 4 + r, cl = wn * 64 + j * 16 + fr;
        *reinterpret_cast<bf16*>(sW + rl * W_LD + cl * 2) = (bf16)sum[i][j][r];
      }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int c = tid + 256 * t;
    const int rl = c >> 4, cc = c & 15;
    const int n = n0 + rl, k = k0 + cc * 8;
    if (n < N && k < K) *reinterpret_cast<u32x4*>(W + (size_t)n * ldw + k) = *reinterpret_cast<const u32x4*>(sW + rl * W_LD + cc * 16);
  }
}

}  // namespace

CE_API int ce_lora_merge_bf16(const void* W0, int ldw0, void* W, int ldw, int N, int K, int n_adapters, const void* const* B,
                              const void* const* A, const int* ranks, const float* scales, hipStream_t stream) {
  if (W0 == nullptr || W == nullptr || N <= 0 || K <= 0 || n_adapters < 0 || ldw0 < K || ldw < K) return CE_ERR_ARG;
  if (n_adapters > 0 && (B == nullptr || A == nullptr || ranks == nullptr || scales == nullptr)) return CE_ERR_ARG;
  if (n_adapters > MAX_ADAPTERS || K % 64 || N % 8) return CE_ERR_SHAPE;
  if (ldw0 % 8 || ldw % 8 || ((uintptr_t)W0 & 15) || ((uintptr_t)W & 15)) return CE_ERR_ALIGN;
  LoraArgs args = {};
  args.n = n_adapters;
  for (int i = 0; i < n_adapters; ++i) {
    if (B[i] == nullptr || A[i] == nullptr) return CE_ERR_ARG;
    if (ranks[i] <= 0 || ranks[i] % RC || ranks[i] > 512) return CE_ERR_SHAPE;
    if (((uintptr_t)B[i] & 15) || ((uintptr_t)A[i] & 15)) return CE_ERR_ALIGN;
    args.B[i] = reinterpret_cast<const bf16*>(B[i]);
    args.A[i] = reinterpret_cast<const bf16*>(A[i]);
    args.rank[i] = ranks[i];
    args.scale[i] = scales[i];
  }
  const int tiles_n = (N + TN - 1) / TN, tiles_k = (K + TK - 1) / TK;
  hipLaunchKernelGGL(lora_merge_kernel, dim3(tiles_n * tiles_k), dim3(256), 0, stream, reinterpret_cast<const bf16*>(W0), ldw0,
                     reinterpret_cast<bf16*>(W), ldw, N, K, tiles_k, args);
  return (int)hipGetLastError();
}

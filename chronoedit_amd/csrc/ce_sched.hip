// K19: classifier-free-guidance combine + one flow-UniPC (order <= 2, bh2, predict-x0) update,
// fused into a single pass over the latents.  HBM-bound: algorithmic bytes per element =
// 2*2 (two bf16 predictions) + 4*4 (x, x_last, m0, m1 read) + 4*4 (written back).
//
// Reference semantics:
//   pipeline_chronoedit.py:736      noise = uncond + g * (cond - uncond)          (bf16 arithmetic)
//   fm_solvers_unipc.py:335-337     x0 = sample - sigma_t * model_output
//   fm_solvers_unipc.py:501-641     UniC corrector  (linear in last_sample, m0, m1, x0)
//   fm_solvers_unipc.py:365-499     UniP predictor  (linear in sample, m0, m1)
//   fm_solvers_unipc.py:706-751     history shift / last_sample bookkeeping
// All scalar coefficients (host-side lambda/h/phi/rho math of :420-468,:560-620) are precomputed
// per step by chronoedit_amd/scheduler.py into a device table, so the update needs no host
// sync and is hipGraph-capturable.
//
// coef[0] = guidance scale g        coef[1] = sigma_t
// coef[2] = use_corrector (0/1)     coef[3..6]  = corrector weights on (x_last, m0, m1, x0)
// coef[7..9] = predictor weights on (x_corrected, x0_new (= new m0), m0_old (= new m1))
//
// ce_cfg_unipc_step_delta is the same pass for the loop with guidance reuse: it stores, reuses or measures the guidance direction (+ 2 bytes
// per element written or read; measuring reads up to four more).
#include "ce_common.h"

// MODE: what the pass does with the guidance direction d = bf16(c - u), the intermediate the combine forms (chronoedit_amd/guidance.py):
//   CFG_PLAIN    nothing - ce_cfg_unipc_step
//   CFG_STORE    delta[i] = d                                                        (a "pair" step; v_uncond given)
//   CFG_REUSE    d = delta[i] (read only), u' = bf16(c - d), v = bf16(u' + bf16(g * d))  (a "reuse" step; v_uncond null) - line :736 applied
//                to (c, u') with the stored d standing for bf16(c - u')
//   CFG_MEASURE  CFG_STORE into slot `slot` of a ring delta[A][n], A <= 4, that also sums (d - ring[(slot - a) mod A][i])^2 for every age
//                a = 1..A (age A is the slot's own old content, read before the lane overwrites it) and d^2
// From v on all modes are the same instructions.
enum { CFG_PLAIN = 0, CFG_STORE = 1, CFG_REUSE = 2, CFG_MEASURE = 3 };
#define CFG_MAX_AGE 4
#define CFG_SUMS (CFG_MAX_AGE + 1)  // sums per workgroup in the scratch: ages 1..4 (unused ones stay 0), then d^2

template <int MODE>
__global__ __launch_bounds__(256) void cfg_unipc_kernel(const bf16* __restrict__ v_cond, const bf16* __restrict__ v_uncond,
                                                        float* __restrict__ x, float* __restrict__ x_last,
                                                        float* __restrict__ m0, float* __restrict__ m1,
                                                        float* __restrict__ x0_out, const float* __restrict__ coef,
                                                        bf16* delta, float* __restrict__ part, int ring, int slot,
                                                        long long n, int flags) {
  const float g = coef[0], sigma = coef[1];
  const bool use_corr = coef[2] != 0.f;
  const float a0 = coef[3], a1 = coef[4], a2 = coef[5], a3 = coef[6];
  const float p0 = coef[7], p1 = coef[8], p2 = coef[9];
  const long long stride = (long long)gridDim.x * blockDim.x;
  float acc[CFG_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float v = (float)v_cond[i];
    if (MODE == CFG_REUSE) {
      const float d = (float)delta[i];
      const float u = round_bf16(v - d);
      v = round_bf16(u + round_bf16(g * d));
    } else if (MODE != CFG_PLAIN || v_uncond != nullptr) {
      const float u = (float)v_uncond[i];
      // bf16 tensor arithmetic of the reference: each op rounds to bf16
      const float d = round_bf16(v - u);
      v = round_bf16(u + round_bf16(g * d));
      if (MODE == CFG_STORE) delta[i] = (bf16)d;
      if (MODE == CFG_MEASURE) {
#pragma unroll
        for (int a = 1; a <= CFG_MAX_AGE; ++a) {
          if (a <= ring) {
            int s = slot - a;
            if (s < 0) s += ring;
            const float e = d - (float)delta[(long long)s * n + i];
            acc[a - 1] += e * e;
          }
        }
        acc[CFG_MAX_AGE] += d * d;
        delta[(long long)slot * n + i] = (bf16)d;
      }
    }
    const float xs = x[i];
    float x0 = xs - ((flags & 1) ? round_bf16(sigma * v) : sigma * v);
    // flags & 2 = reference-precision trajectory: the reference's latents, x0 prediction and scheduler history are bf16 TENSORS
    // (pipeline_chronoedit.py:681 passes torch.bfloat16 to prepare_latents), so x0 is rounded before UniC consumes it and the
    // corrected sample before UniP does; storage stays fp32, the values are bf16
    if (flags & 2) x0 = round_bf16(x0);
    const float m0o = m0[i], m1o = m1[i];
    float xc = xs;
    if (use_corr) {
      xc = a0 * x_last[i] + a1 * m0o + a2 * m1o + a3 * x0;
    }
    if (flags & 2) xc = round_bf16(xc);
    float xn = p0 * xc + p1 * x0 + p2 * m0o;
    if (flags & 2) xn = round_bf16(xn);
    const float x0s = x0;
    x[i] = xn;
    x_last[i] = xc;
    m1[i] = m0o;
    m0[i] = x0s;
    if (x0_out != nullptr) x0_out[i] = x0;
  }
  if (MODE == CFG_MEASURE) {
    // every sum in an order that n and the grid alone decide (the scheme of ce_tea_store_dist_bf16): a lane adds its elements in index order,
    // the 64 lanes of a wave meet in a butterfly, the four waves are added in order, cfg_measure_finish_kernel adds the workgroups.  No atomics.
    __shared__ float wv[CFG_SUMS][4];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CFG_SUMS; ++k) {
      const float s = wave_sum(acc[k]);
      if ((threadIdx.x & 63) == 0) wv[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < CFG_SUMS) part[CFG_SUMS * blockIdx.x + threadIdx.x] = ((wv[threadIdx.x][0] + wv[threadIdx.x][1]) + wv[threadIdx.x][2]) + wv[threadIdx.x][3];
  }
}

// wave w adds sum w of the `nparts` workgroups: lane l takes workgroups l, l + 64, ... in index order, then the butterfly.  The row of the
// table holds the `ring` age sums first, then sum d^2.
__global__ __launch_bounds__(64 * CFG_SUMS) void cfg_measure_finish_kernel(const float* __restrict__ part, int nparts, int ring, float* __restrict__ row) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float s = 0.0f;
  for (int j = lane; j < nparts; j += 64) s += part[CFG_SUMS * j + w];
  s = wave_sum(s);
  if (lane == 0) {
    if (w < ring) row[w] = s;
    if (w == CFG_MAX_AGE) row[ring] = s;
  }
}

static unsigned cfg_unipc_blocks(long long n) {
  long long blocks = (n + 255) / 256;
  return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

CE_API int ce_cfg_unipc_step(const void* v_cond, const void* v_uncond, float* x, float* x_last, float* m0, float* m1,
                                 float* x0_out, const float* coef, const void* reserved, long long n, int flags,
                                 hipStream_t stream) {
  (void)reserved;
  if (!v_cond || !x || !x_last || !m0 || !m1 || !coef || n <= 0) return CE_ERR_ARG;
  hipLaunchKernelGGL(cfg_unipc_kernel<CFG_PLAIN>, dim3(cfg_unipc_blocks(n)), dim3(256), 0, stream, (const bf16*)v_cond,
                     (const bf16*)v_uncond, x, x_last, m0, m1, x0_out, coef, (bf16*)nullptr, (float*)nullptr, 0, 0, n, flags);
  return (int)hipGetLastError();
}

CE_API int ce_cfg_unipc_step_delta(const void* v_cond, const void* v_uncond, float* x, float* x_last, float* m0, float* m1, float* x0_out,
                                   const float* coef, void* delta, long long n, int flags, int ring, int slot, float* scratch,
                                   long long scratch_bytes, float* table, int row, hipStream_t stream) {
  if (!v_cond || !x || !x_last || !m0 || !m1 || !coef || !delta || n <= 0) return CE_ERR_ARG;
  if (ring < 0 || ring > CFG_MAX_AGE) return CE_ERR_ARG;
  if ((uintptr_t)delta & 1) return CE_ERR_ALIGN;
  const unsigned blocks = cfg_unipc_blocks(n);
  bf16* d = (bf16*)delta;
  if (ring == 0) {
    if (v_uncond)
      hipLaunchKernelGGL(cfg_unipc_kernel<CFG_STORE>, dim3(blocks), dim3(256), 0, stream, (const bf16*)v_cond, (const bf16*)v_uncond, x, x_last,
                         m0, m1, x0_out, coef, d, (float*)nullptr, 0, 0, n, flags);
    else
      hipLaunchKernelGGL(cfg_unipc_kernel<CFG_REUSE>, dim3(blocks), dim3(256), 0, stream, (const bf16*)v_cond, (const bf16*)nullptr, x, x_last,
                         m0, m1, x0_out, coef, d, (float*)nullptr, 0, 0, n, flags);
    return (int)hipGetLastError();
  }
  // measuring is an option of the store mode
  if (!v_uncond || !scratch || !table || slot < 0 || slot >= ring || row < 0) return CE_ERR_ARG;
  if (((uintptr_t)scratch | (uintptr_t)table) & 3) return CE_ERR_ALIGN;
  if (scratch_bytes < (long long)blocks * CFG_SUMS * (long long)sizeof(float)) return CE_ERR_ARG;
  hipLaunchKernelGGL(cfg_unipc_kernel<CFG_MEASURE>, dim3(blocks), dim3(256), 0, stream, (const bf16*)v_cond, (const bf16*)v_uncond, x, x_last, m0,
                     m1, x0_out, coef, d, scratch, ring, slot, n, flags);
  hipLaunchKernelGGL(cfg_measure_finish_kernel, dim3(1), dim3(64 * CFG_SUMS), 0, stream, (const float*)scratch, (int)blocks, ring,
                     table + (size_t)row * (size_t)(ring + 1));
  return (int)hipGetLastError();
}

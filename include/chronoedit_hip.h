/* C ABI of libchronoedit_hip.so — the MI355X (gfx950) kernels behind the ChronoEdit DiT hot path.
 *
 * Conventions (SURVEY.md §8b "C-ABI for the HIP library"):
 *   - plain pointers + sizes; no torch types; every pointer is a DEVICE pointer unless noted;
 *   - no allocation, no synchronisation, no host reads inside: every launcher only enqueues
 *     kernels on `stream`, so whole denoising steps are hipGraph-capturable;
 *   - the caller owns every buffer; the library is stateless;
 *   - return value: 0 = ok, CE_ERR_* (<0) = rejected arguments (nothing was launched),
 *     >0 = hipError_t of the launch.  Never throws.
 *   - bf16 tensors are raw 16-bit patterns (`void*`); "ld*" are row strides in ELEMENTS.
 *
 * Each entry point cites the reference interface (file:line under /root/reference) it replaces.
 */
#ifndef CHRONOEDIT_HIP_H
#define CHRONOEDIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define CE_OK 0
#define CE_ERR_ARG (-1)
#define CE_ERR_SHAPE (-2)
#define CE_ERR_ALIGN (-3)

/* GEMM epilogues */
#define CE_EPI_BIAS 0      /* C = bf16(A.W^T + bias) */
#define CE_EPI_BIAS_GELU 1 /* C = bf16(gelu_tanh(bf16(A.W^T + bias)))   diffusers FeedForward("gelu-approximate") */
#define CE_EPI_GATE_RES 2  /* C = bf16(res + bf16(A.W^T + bias) * gate[n]); gate == NULL -> 1 */
#define CE_EPI_BIAS_GELU_ERF 3 /* exact-erf GELU: diffusers FeedForward("gelu") of the image embedder */
#define CE_EPI_BIAS_ROW 6      /* C = bf16(A.W^T + bias[m]): bias along the ROWS of C - a product taken with the operand roles swapped
                                * (V^T = W_v.X^T: the attention kernel's V^T operand straight out of the projection, no transpose pass) */
#define CE_EPI_BIAS_T 7        /* C is [N][ldc] and holds the TRANSPOSE: C[n][m] = bf16(A.W^T[m][n] + bias[n]) - the same V^T as CE_EPI_BIAS_ROW
                                * gives with the operands swapped, but M stays the token count (round 6: 760 tiles of 384 rows = 2.97 rounds of
                                * 256 CUs where the swapped product is 1140 tiles of 256 = 4.45 rounds with a split-K tail); shapes the large-tile
                                * kernel does not take run as that swapped product: the same sums either way.  M % 8 == 0, N % 8 == 0 */
#define CE_EPI_F32 4           /* C is float* (ldc in floats): raw fp32 A.W^T, no bias (VAE mid-block attention scores) */

/* y = LayerNorm_fp32(x, eps) * a[d] + b[d] -> bf16.   One wave64 per row; D % 8 == 0, D <= 5120.
 * ab_rows > 0: row m uses a/b + (m / ab_rows) * ab_stride (one AdaLN vector pair per sample when samples are stacked).
 * Replaces `(self.norm1(h.float()) * (1 + scale) + shift).type_as(h)` and FP32LayerNorm(affine)
 * (chronoedit_diffusers/transformer_chronoedit.py:279,284,289,460). */
int ce_ln_affine_bf16(const void* x, void* y, const float* a, const float* b, int M, int D, int ldx, int ldy, float eps,
                      int ab_rows, int ab_stride, hipStream_t stream);

/* In place: x = RMSNorm_across_heads(x; w, eps), then (cos_sin != NULL) 3-D RoPE on (even, odd)
 * channel pairs of every head; cos_sin = [rope_rows or M][head_dim/2][2] fp32 (cos, sin), row m uses entry m % rope_rows.
 * (x2, w2) optional: a second tensor with the same geometry handled by the same launch (q and k of a fused buffer).
 * Replaces attn.norm_q / norm_k / norm_added_k + apply_rotary_emb
 * (transformer_chronoedit.py:62-65,73-79,85). */
int ce_rmsnorm_rope_bf16(void* x, const float* w, void* x2, const float* w2, const float* cos_sin, int M, int D, int ld,
                         int head_dim, float eps, int rope_rows, hipStream_t stream);

/* C[M,N] = epilogue(A[M,K] . W[N,K]^T + bias[N]); bf16 in/out, fp32 accumulate on MFMA.
 * K % 64 == 0, N % 8 == 0; res may alias C.  gate_rows > 0: row m uses gate[(m / gate_rows) * N + n] (one gate
 * vector per sample when several samples' tokens are stacked along M); gate_rows == 0: one gate vector.  Replaces every nn.Linear on the path
 * (transformer_chronoedit.py:58-60,84-86,106, FeedForward :262, patch_embedding :429, proj_out :461).
 * K-SEGMENTED A operand: column k of A lives at A + (k / a_seg_k) * a_seg_stride + m * lda + k % a_seg_k (elements; a_seg_k % 64 == 0,
 * K % a_seg_k == 0; a_seg_k == 0: plain row-major A).  This is the layout the second Ulysses all-to-all leaves the attention output in -
 * [source rank = head group][local token][D / W] - so the out-projection reads it in place instead of a gather pass (reference design:
 * chronoedit_diffsynth/wan_video_new_chronoedit.py:330-355; the reference's xfuser path materialises the gathered tensor).
 * K-segmented W likewise (w_seg_k, w_seg_stride).  seg_k = 64 and ld = 64 is the K-slab-major packing [K/64][rows][64]: every 16 KiB
 * half-tile the 256-tile kernel streams by LDS-DMA is then ONE contiguous block (measured L2->LDS stream rate 21.7 vs 18.3 TB/s for the
 * row-strided form, profiles/r02_l2_pattern_probe.txt).  Segmented W needs the 256-tile kernel (K % 128 == 0), else CE_ERR_SHAPE.
 * ws / ws_bytes: the split-K scratch.  The large-tile kernels cut the tiles that would run as a partially filled last round of workgroups
 * along K into fp32 slabs (256 KiB each for a 256 x 256 tile, 384 KiB for 384 x 256, at most one per CU), which a second launch sums and
 * applies the epilogue to.  ws == NULL: no split, every tile runs whole; otherwise ws_bytes bounds the split (and enters the macro-tile
 * choice, ce_gemm_bf16_tile_rows).  ws is device memory owned by the caller; the library never allocates and keeps no state a launch
 * reads except its read-only tables.  The caller guarantees that no other stream uses ws while the launch is queued. */
int ce_gemm_bf16(const void* A, const void* W, void* C, const float* bias, int epilogue, const float* gate, const void* res,
                 int M, int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, int a_seg_k, long long a_seg_stride,
                 int w_seg_k, long long w_seg_stride, void* ws, size_t ws_bytes, hipStream_t stream);

/* ce_gemm_bf16 with a ROW PERIOD on the residual of CE_EPI_GATE_RES: output row m reads residual row m % res_rows (res is [res_rows][ldres];
 * res_rows == 0: row m, i.e. ce_gemm_bf16 itself; other epilogues take res_rows == 0 only).  Samples stacked along M that share one residual
 * - the guidance pair in front of its first cross-attention - fan out here without a copy: M = 2 n rows of A, n rows of res, 2 n rows of C.
 * res must NOT alias C then (a row of C would be written while another tile still reads it as the second sample's residual).  The
 * register-direct epilogues of the large tiles take res_rows >= their tile height; a shorter period runs on the 8-wave 256-tile kernel. */
int ce_gemm_bf16_res(const void* A, const void* W, void* C, const float* bias, int epilogue, const float* gate, const void* res,
                     int M, int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, int res_rows, int a_seg_k,
                     long long a_seg_stride, int w_seg_k, long long w_seg_stride, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- The alternative kernel bodies (A/B partners of the measurement tools and the body-equivalence tests) are NOT selectable through this
 * library: libchronoedit_hip.so picks every kernel from the call's own shape and keeps no state a launch reads.  The
 * selectors live in a second build of the same sources, libchronoedit_hip_diag.so (include/chronoedit_hip_diag.h, -DCE_DIAGNOSTICS), which
 * tools/ and tests/ load beside this one. ---- */


/* Which macro tile ce_gemm_bf16 runs a LARGE product on when the choice is automatic: 384 or 288 (x 256, ce_gemm384.hip) or 256 (x 256,
 * ce_gemm256w4.hip) rows - the one whose tile count falls better on `cus` compute units (full rounds + the last round, which is cut
 * along K when the split-K workspace of `ws_bytes` bytes allows it).  A pure function: no device is touched.  0: invalid arguments. */
int ce_gemm_bf16_tile_rows(int M, int N, int K, int cus, long long ws_bytes);

/* O = softmax(Q K1^T * scale) V1 [ + softmax(Q K2^T * scale) V2 ], per head, head_dim == 128, bf16.
 * Each segment's result is rounded to bf16 before the add (SDPA output dtype).
 * Replaces F.scaled_dot_product_attention at transformer_chronoedit.py:91-104. */
int ce_attention_bf16(const void* Q, const void* K1, const void* V1, int len1, int ldk1, int ldv1, const void* K2,
                      const void* V2, int len2, int ldk2, int ldv2, void* O, int Nq, int H, int head_dim, int ldq, int ldo,
                      float softmax_scale, hipStream_t stream);

/* The same for `batch` samples stacked along the rows of every operand (sample b owns rows [b Nq, (b+1) Nq) of Q / O
 * and rows [b len, (b+1) len) of each K/V segment; strides as above), in ONE launch: the cond / uncond forwards of a
 * classifier-free-guidance step (pipeline_chronoedit.py:715-735) are independent, and 2x the workgroups per launch
 * halves the partially filled last round.  batch == 1 is ce_attention_bf16. */
int ce_attention_batched_bf16(const void* Q, const void* K1, const void* V1, int len1, int ldk1, int ldv1, const void* K2,
                              const void* V2, int len2, int ldk2, int ldv2, void* O, int Nq, int H, int head_dim, int ldq,
                              int ldo, float softmax_scale, int batch, hipStream_t stream);

/* The same self-attention (one KV segment, `batch` samples per launch) with V handed over TRANSPOSED: Vt [H * 128][ldvt] bf16, row =
 * head channel, column = key, sample b's keys in columns [b len, (b + 1) len); ldvt >= (batch - 1) len + 64 ceil(len / 64), every
 * column up to ldvt finite (ce_v_transpose_bf16 zeroes the padding); len even when batch > 1 (dword-aligned sample offsets).
 * K and V^T tiles both reach LDS by LDS-DMA - no register
 * staging, no in-kernel transpose; the arithmetic and its order per row are those of ce_attention_batched_bf16.
 * Replaces the same F.scaled_dot_product_attention call (transformer_chronoedit.py:91-96). */
int ce_attention_vt_bf16(const void* Q, const void* K, const void* Vt, int len, int ldk, int ldvt, void* O, int Nq, int H, int head_dim,
                         int ldq, int ldo, float softmax_scale, int batch, hipStream_t stream);

/* Cross-attention - TWO key / value segments with a softmax each, the two outputs added in bf16 (transformer_chronoedit.py:91-104: text
 * and image keys) - with both V operands handed over transposed: V1t [H*128][ldv1t], V2t [H*128][ldv2t], sample b's keys at columns
 * [b*vt_cols, b*vt_cols + len) of its segment's V^T (vt_cols even, >= len; ldv*t >= (batch-1)*vt_cols + 64*ceil(len/64); every column
 * read - a sample's tail strip runs into the next sample's keys or the padding - is finite and meets P = 0).  K1 / K2 as in
 * ce_attention_batched_bf16 (samples stacked along the rows).  The K and V^T tiles of both segments reach LDS by LDS-DMA. */
int ce_attention_2seg_vt_bf16(const void* Q, const void* K1, const void* V1t, int len1, int ldk1, int ldv1t, int vt_cols1, const void* K2,
                              const void* V2t, int len2, int ldk2, int ldv2t, int vt_cols2, void* O, int Nq, int H, int head_dim, int ldq,
                              int ldo, float softmax_scale, int batch, hipStream_t stream);

/* ce_attention_2seg_vt_bf16 with the samples' strides spelled out, so that an operand can be ONE tensor for all samples: q_rows = rows of Q
 * between consecutive samples (>= Nq; ce_attention_2seg_vt_bf16 passes Nq) or 0 = every sample reads the same Nq query rows; k1_rows /
 * k2_rows = rows of K1 / K2 between samples (>= len; the stacked form passes len) or 0 = the segment - K and V^T - is shared (its vt_cols
 * is ignored, ldv*t >= 64*ceil(len/64)).  O is always per sample, [batch*Nq][ldo].  The two forwards of a guidance step share the image
 * context in every block (k2_rows = 0) and, in front of the first cross-attention, the queries (q_rows = 0).  Same products in the same
 * order as the stacked form run on physically duplicated operands: bit-equal results. */
int ce_attention_2seg_vt_strided_bf16(const void* Q, const void* K1, const void* V1t, int len1, int ldk1, int ldv1t, int vt_cols1,
                                      const void* K2, const void* V2t, int len2, int ldk2, int ldv2t, int vt_cols2, void* O, int Nq, int H,
                                      int head_dim, int ldq, int ldo, float softmax_scale, int batch, int q_rows, int k1_rows, int k2_rows,
                                      hipStream_t stream);

/* ce_attention_2seg_vt_strided_bf16 with segment 1 cut and weighted per sample.  valid1: int32 [batch] on the device, 1 <= valid1[b] <= len1 -
 * sample b attends keys [0, valid1[b]) of segment 1 only, and its key-tile loop ends at ceil(valid1[b] / 64).  w1: fp32 [batch] on the device -
 * the logit of key valid1[b] - 1 gets + w1[b] in the log2 domain (after the multiplication by softmax_scale log2 e): that key counts 2^w1[b]
 * times in the softmax, so a run of m identical trailing keys (the zero-padded tail of a text context) is ONE key with w1 = log2 m.  The
 * kernel reads both arrays (nothing of them on the host): a captured launch follows their content.  valid1[b] = len1 and w1[b] = 0 give
 * ce_attention_2seg_vt_strided_bf16 bit for bit.  Strides, segment 2 and the shared forms as there; len1 / k1_rows / vt_cols1 describe the
 * operand as stored.  A valid1[b] outside [1, len1] is not reported (the host never sees the array): the kernel clamps it into the range -
 * 0 or a negative count behaves as 1, a count above len1 as len1 - and never reads a key past len1
 * (pinned by tests/test_exact_cross_attention_gpu.py). */
int ce_attention_2seg_vt_weighted_bf16(const void* Q, const void* K1, const void* V1t, int len1, int ldk1, int ldv1t, int vt_cols1,
                                       const void* K2, const void* V2t, int len2, int ldk2, int ldv2t, int vt_cols2, void* O, int Nq, int H,
                                       int head_dim, int ldq, int ldo, float softmax_scale, int batch, int q_rows, int k1_rows, int k2_rows,
                                       const void* valid1, const void* w1, hipStream_t stream);

/* ce_attention_2seg_vt_bf16 with its output written as the MX fp8 operand of the out-projection that follows it in the fp8 mode
 * (transformer_chronoedit.py:106 `attn.to_out[0]`; no counterpart in the reference): o8 e4m3 [batch Nq][ldo8] (ldo8 % 16 == 0) + one
 * E8M0 scale per 32 channels in the tiled layout of ce_gemm_mxfp8 (rows = batch Nq, K = H head_dim, K % 128 == 0) - bit-identical to
 * ce_attention_2seg_vt_bf16 followed by ce_quant_rows_mxfp8 (a 32-channel block of a query row is two lanes' accumulator registers). */
int ce_attention_2seg_vt_quant_bf16(const void* Q, const void* K1, const void* V1t, int len1, int ldk1, int ldv1t, int vt_cols1, const void* K2,
                                    const void* V2t, int len2, int ldk2, int ldv2t, int vt_cols2, void* o8, void* scale8, int Nq, int H,
                                    int head_dim, int ldq, int ldo8, float softmax_scale, int batch, hipStream_t stream);

/* ce_attention_vt_bf16 over the BLOCKED row layout an all-to-all leaves behind when every rank sent [sample][local token] rows
 * (Ulysses sequence parallelism with the guidance pair batched: chronoedit_amd/parallel.py): token g of sample b sits in row
 * (g / blk_rows) blk_stride + b blk_rows + g % blk_rows of Q, K and O (blk_rows = tokens per rank, a multiple of 64; blk_stride =
 * batch * blk_rows); Nq = query tokens per sample (a multiple of blk_rows), len = VALID keys per sample (the tail of the last block
 * is padding); Vt plain per sample, sample b's keys at columns [b vt_sample_cols, ...) (ce_v_transpose_blocked_bf16).  A key tile
 * never straddles a block, so the layout costs one scalar multiply-high per tile.  Replaces the gather + permute copies around
 * F.scaled_dot_product_attention in the reference's sequence-parallel path (wan_video_new_chronoedit.py:330-355 via xfuser). */
int ce_attention_vt_blocked_bf16(const void* Q, const void* K, const void* Vt, int len, int ldk, int ldvt, void* O, int Nq, int H, int head_dim,
                                 int ldq, int ldo, float softmax_scale, int batch, int blk_rows, int blk_stride, int vt_sample_cols,
                                 hipStream_t stream);

/* v in the blocked row layout above -> vt [H * 128][ldvt] plain per sample (sample b at columns [b vt_sample_cols, ...), columns past
 * n_keys zeroed); vt_sample_cols a multiple of 64, ldvt >= batch * vt_sample_cols. */
int ce_v_transpose_blocked_bf16(const void* v, int ldv, void* vt, int ldvt, int n_keys, int H, int batch, int blk_rows, int blk_stride,
                                int vt_sample_cols, hipStream_t stream);

/* v [n_keys][ldv] bf16 (head h at columns [128 h, 128 h + 128)) -> vt [H * 128][ldvt] (ldvt >= n_keys, multiple of 8; columns
 * [n_keys, ldvt) zeroed): the producer of ce_attention_vt_bf16's V operand. */
int ce_v_transpose_bf16(const void* v, int ldv, void* vt, int ldvt, int n_keys, int H, hipStream_t stream);


/* out[dim] = [cos(t f_i), sin(t f_i)], f_i = 1e4^(-i/(dim/2)), fp32; t is a device int64.
 * Replaces diffusers Timesteps(flip_sin_to_cos=True, downscale_freq_shift=0)
 * (transformer_chronoedit.py:137,153). */
int ce_timestep_sinusoid(const int64_t* t, float* out, int dim, hipStream_t stream);

/* Same table from a FLOATING-POINT timestep (device fp32): the reference's two sibling stacks hand the scheduler's float
 * timesteps to sinusoidal_embedding_1d (wan_video_dit_chronoedit.py:83-87, wan2pt1.py:191-200; call sites
 * wan_video_new_chronoedit.py:1383, wan2pt1.py:812). */
int ce_timestep_sinusoid_f32(const float* t, float* out, int dim, hipStream_t stream);

/* y[N] = post(W[N,K] . pre(x[K]) + bias); W fp32 (w_is_bf16 = 0) or bf16.
 * flags: 1 = pre: x <- bf16(silu(x)); 2 = post: silu; 4 = post: round result to bf16 (still stored fp32).
 * Replaces TimestepEmbedding + act_fn + time_proj (transformer_chronoedit.py:153-159). */
int ce_gemv(const void* W, int w_is_bf16, const float* x, const float* bias, float* y, int N, int K, int flags,
            hipStream_t stream);

/* mod[L][J][D] = table[L][J][D] + v[(v_rows==1 ? 0 : j)][D], plus 1.0 on rows j with bit j of one_mask set.
 * Replaces `(scale_shift_table + temb.float()).chunk(6)` and the `(1 + scale)` terms
 * (transformer_chronoedit.py:274-279,289,451,460). */
int ce_modulation(const float* table, const float* v, float* mod, int L, int J, int D, int v_rows, int one_mask,
                  hipStream_t stream);

/* im2col of the k = s = (1,2,2) patch Conv3d: x [C][T][H][W] -> cols [T*(H/2)*(W/2)][Kpad] (zero padded).
 * Replaces patch_embedding + flatten/transpose (transformer_chronoedit.py:429-430). */
int ce_patchify_bf16(const void* x, void* cols, int C, int T, int H, int W, int Kpad, hipStream_t stream);

/* The same for token rows [row0, row0 + nrows) only (cols has nrows rows; rows past the last token are zero): the local
 * shard of a sequence-parallel rank (zero pad: wan_video_new_chronoedit.py:1450-1453). */
int ce_patchify_rows_bf16(const void* x, void* cols, int C, int T, int H, int W, int Kpad, int row0, int nrows, hipStream_t stream);

/* Ulysses send side fused into the RMSNorm(+RoPE) pass.  For each of nt (<= 3) column blocks of x [M][ldx] (block i = columns
 * [col_i, col_i + D)): w_i != NULL -> RMSNorm across the D channels * w_i, then RoPE when cos_sin != NULL (as
 * ce_rmsnorm_rope_bf16); w_i == NULL -> copy (v).  Output: send[r][m][i][D/W] for destination rank r = n / (D/W), i.e. the
 * contiguous per-destination chunks all_to_all_single needs (no permute pass).  Replaces the q/k/v head-scatter of the
 * reference's sequence-parallel attention (wan_video_new_chronoedit.py:330-355 via xfuser) after
 * transformer_chronoedit.py:62-79. */
int ce_rope_scatter_bf16(const void* x, int ldx, void* send, int M, int D, int W, int nt, int col0, const float* w0, int col1,
                         const float* w1, int col2, const float* w2, const float* cos_sin, int head_dim, float eps,
                         int rope_rows, hipStream_t stream);

/* y [N][ldy] (col = (dh*2+dw)*Cout + c) -> out [Cout][T][H][W].
 * Replaces the reshape/permute/flatten at transformer_chronoedit.py:463-467. */
int ce_unpatchify_bf16(const void* y, void* out, int Cout, int T, int H, int W, int ldy, hipStream_t stream);

/* One denoising-loop tail, fused over the latents (n elements):
 *   v   = v_uncond ? bf16(u + bf16(g * bf16(c - u))) : c            pipeline_chronoedit.py:736
 *   x0  = x - sigma * v                                              fm_solvers_unipc.py:335-337
 *   xc  = use_corr ? a0*x_last + a1*m0 + a2*m1 + a3*x0 : x           UniC, fm_solvers_unipc.py:501-641
 *   x   = p0*xc + p1*x0 + p2*m0 ; x_last = xc ; m1 = m0 ; m0 = x0    UniP + history, :365-499,706-751
 * coef = device float[10] {g, sigma, use_corr, a0..a3, p0..p2} precomputed on the host per step.
 * flags bit0: round sigma*v to bf16 (the reference multiplies a 0-dim fp32 sigma into a bf16 tensor).
 * flags bit1: round the stored x, x_last and m0 to bf16 values (the reference keeps latents and scheduler history as bf16
 *             tensors, pipeline_chronoedit.py:681,739): the "reference-precision trajectory" mode of the pipeline.
 * Replaces scheduler.step + the CFG line of ChronoEditPipeline.__call__ (pipeline_chronoedit.py:736-739). */
int ce_cfg_unipc_step(const void* v_cond, const void* v_uncond, float* x, float* x_last, float* m0, float* m1,
                      float* x0_out, const float* coef, const void* reserved, long long n, int flags, hipStream_t stream);

/* ce_cfg_unipc_step for a loop that runs the unconditional sample only on planned steps (chronoedit_amd/guidance.py).  Everything
 * ce_cfg_unipc_step takes, plus the guidance direction d = bf16(c - u), the intermediate the combine already forms, in `delta` (bf16):
 *   store   (v_uncond given, ring == 0): the five outputs of ce_cfg_unipc_step bit for bit, and delta[i] = d.  delta: n elements.
 *   reuse   (v_uncond null,  ring == 0): delta is only read: u' = bf16(c - d), v = bf16(u' + bf16(g * d)) - line :736 applied to
 *           (c, u') with the stored d standing for bf16(c - u'); from v on as ce_cfg_unipc_step.
 *   measure (v_uncond given, 1 <= ring <= 4): store mode into slot `slot` of a ring delta[ring][n] that first sums, over all elements,
 *           (d - ring[(slot - a) mod ring])^2 for every age a = 1..ring (age `ring` is the slot's own old content) and d^2: fp32, per
 *           workgroup into `scratch` (>= 5 floats per workgroup, at most 2048 workgroups: 40960 bytes always suffice), then by a
 *           second launch into table[row * (ring + 1) + {0..ring-1: the ages, ring: d^2}].  Fixed summation order, no atomics: the
 *           same bits on every run.  Which ages hold a direction at all is the caller's knowledge.
 * scratch / table / slot / row are ignored when ring == 0.  Every scalar comes from coef or the arguments: capturable. */
int ce_cfg_unipc_step_delta(const void* v_cond, const void* v_uncond, float* x, float* x_last, float* m0, float* m1, float* x0_out,
                            const float* coef, void* delta, long long n, int flags, int ring, int slot, float* scratch,
                            long long scratch_bytes, float* table, int row, hipStream_t stream);

/* ---- Wan-2.1 VAE (chronoedit/_src/tokenizers/wan2pt1.py; call sites pipeline_chronoedit.py:442,776-781) ----------
 * Activation frames are channels-last with a 1-pixel zero border: [H+2][W+2][C] bf16. */

/* Implicit-GEMM conv: out[t][h][w][co] = bias[co] + sum_{kt,kh,kw,ci} W[co][(kt,kh,kw)][ci] *
 *   in_frames[t*st + kt][h*ss + kh + in_off_h][w*ss + kw + in_off_w][ci]   (+ res_frames[t][...] when given).
 * in_frames / out_frames / res_frames are HOST arrays of device frame pointers (<= 16): temporal causal padding is
 * expressed by listing cache / zero frames in front.  weight [Cout][KT*KH*KW][Cin] bf16; Cin % 32 == 0, Cout % 8 == 0.
 * Output pixel (h,w) is stored at [(h+out_border)*out_Wp + (w+out_border)]*out_cstride + out_coff + co.
 * Replaces CausalConv3d / nn.Conv2d of Encoder3d/Decoder3d (wan2pt1.py:42-60,99-112,195-203,237-238). */
int ce_conv_igemm_bf16(const void* const* in_frames, int n_in_frames, const void* weight, const float* bias,
                       void* const* out_frames, int n_out_frames, const void* const* res_frames, int Cin, int Cout, int KT,
                       int KH, int KW, int st, int ss, int H_out, int W_out, int in_Wp, int in_off_h, int in_off_w, int out_Wp,
                       int out_border, int out_cstride, int out_coff, hipStream_t stream);

/* The decoder's head conv (Decoder3d.head, wan2pt1.py:401-403: CausalConv3d(96, 3, 3, padding=1)) as a bandwidth kernel: stride-1
 * 3 x 3 x 3 (KT = 3) or 1 x 3 x 3 (KT = 1) of Cin = 96 onto Cout <= 4 channels.  Same frames, addressing and result as
 * ce_conv_igemm_bf16 with st = ss = 1, in_off = 0 and no residual (weight [>= Cout][KT*9][96] bf16, bias fp32 [>= Cout] or NULL);
 * channels Cout..3 of an output pixel - and 4..7 when out_cstride - out_coff >= 8 - are written as zeros.  The three kernel rows ride
 * in the matrix instruction's output rows, so one pass over ten input rows yields eight output rows. */
int ce_conv3d_head_bf16(const void* const* in_frames, int n_in_frames, const void* weight, const float* bias, void* const* out_frames,
                        int n_out_frames, int Cin, int Cout, int KT, int H_out, int W_out, int in_Wp, int out_Wp, int out_border,
                        int out_cstride, int out_coff, hipStream_t stream);

/* The stride-1 3 x 3 (KT = 1) / 3 x 3 x 3 (KT = 3) convolutions of wide layers on the 256 x 256 x 64 LDS-DMA GEMM (same result as
 * ce_conv_igemm_bf16 with st = ss = 1, in_off = 0, out_border = 1): on bordered frames of one contiguous stack the A rows of the
 * implicit GEMM are linear in memory and the taps are constant offsets, so the product runs on the large-tile kernel and the border
 * positions it computes along the way are zeroed again.
 *   in_stack  [T_out + KT - 1 frames + ONE zeroed slack frame][H+2][W+2][Cin] bf16: for KT = 3 the first two frames are the causal
 *             padding / cache frames (CausalConv3d, wan2pt1.py:42-60), frame t of the output reads frames t .. t + KT - 1
 *   weight    [Cout][ldw] bf16: column ((kt*3 + kh) * S + kw * Cin + ci), S = 3*Cin rounded up to a multiple of 64 (zero columns in
 *             between when Cin = 96), zero from KT*3*S up to ldw >= the K-tile count rounded up to even x 64
 *   out_stack [T_out][H+2][W+2][out_cstride] (channels [0, Cout) written, borders zeroed); res_stack: same geometry, added, or NULL
 *   n_tile    256, 128 or 96: width of the macro tile (256 x 256 with 128 x 128 wave tiles | 256 x 128 with 128 x 64 | 256 x 96 with
 *             128 x 48); 1 (round 6; Cout == 96 and Cin 32, 96 or 192 only): not a GEMM tile - 512 positions x 96 channels per workgroup with
 *             the input slab itself in the LDS, the kw taps as position offsets (the same weight matrix, the same result up to the
 *             summation order), two waves per SIMD; 2: the same with one wave per SIMD (its A/B partner); 0 = 1 where it applies (the
 *             full-resolution layers of the VAE), else whichever tile wastes less of Cout
 * Cin % 32 == 0, Cout % 8 == 0. */
int ce_conv3d_gemm_bf16(const void* in_stack, const void* weight, int ldw, const float* bias, void* out_stack, const void* res_stack,
                        int T_out, int H, int W, int Cin, int Cout, int KT, int out_cstride, int n_tile, hipStream_t stream);

/* ce_conv3d_gemm_bf16 (same in_stack / weight / out_stack / res_stack operands and geometry) with the NEXT layer's RMS_norm (+ SiLU) applied in
 * the epilogue: with y = bf16(conv(in) + bias) [then bf16(res + y)], normed_stack = [silu]( RMS_norm(y) * gamma ) - ce_rms_silu_bf16's formula on
 * the rounded values it would have read.  Cout == 96 and Cin 32 / 96 / 192 only (the kernel whose lanes hold all 96 channels of a position);
 * gamma fp32 [96]; normed_stack has out_stack's geometry (borders zeroed).
 *   out_stack == NULL (then res_stack == NULL): y is never written - CausalConv3d -> RMS_norm -> SiLU inside a ResidualBlock (wan2pt1.py:195-200);
 *   out_stack != NULL: y to out_stack AND its normalised form to normed_stack (the next block's shortcut and first norm, :186-220, or the
 *                      head's norm, :401-403): the pass that would have re-read y is gone. */
int ce_conv3d_gemm_rms_silu_bf16(const void* in_stack, const void* weight, int ldw, const float* bias, void* out_stack, const void* res_stack,
                                 void* normed_stack, int T_out, int H, int W, int Cin, int Cout, int KT, int out_cstride, const float* gamma,
                                 int apply_silu, hipStream_t stream);

/* y = [silu]( x / max(||x||_2, 1e-12) * sqrt(C) * gamma ) per pixel over C channels; x, y are stacks of npix/(H*W) frames
 * with in_border / out_border zero borders (the interiors are written, never the border).  C % 8 == 0, C <= 512.
 * Replaces RMS_norm (+ nn.SiLU) (wan2pt1.py:63-75,193-200). */
int ce_rms_silu_bf16(const void* x, void* y, const float* gamma, long long npix, int C, int H, int W, int in_border,
                     int out_border, int apply_silu, hipStream_t stream);

/* Zero the one-pixel border of T frames [H+2][W+2][ld] (channels [0, C)): for buffers that were not zero-filled and whose producer
 * writes interiors only (the border is the zero padding of the next convolution). */
int ce_zero_border_bf16(void* frames, int T, int H, int W, int C, int ld, hipStream_t stream);

/* nearest-exact 2x spatial upsample of T bordered frames [H+2][W+2][C] -> [2H+2][2W+2][C] (wan2pt1.py:78-83,99-104). */
int ce_upsample2x_bf16(const void* x, void* y, int T, int C, int H, int W, hipStream_t stream);

/* O [Nq][ldo] = softmax(Q K^T * softmax_scale) V for ONE attention head of dimension C (128 or 384) as a single flash-style kernel
 * (no [Nq, Nk] score matrix in memory): Q [Nq][ldq], K [Nk][ldk] bf16 rows; Vt [C][ldvt] = V transposed, keys contiguous, ldvt >=
 * 64 ceil(Nk / 64) with the padding columns finite (zero).  Replaces the scaled_dot_product_attention of the Wan VAE's mid-block
 * AttentionBlock (chronoedit/_src/tokenizers/wan2pt1.py:247-255: one head over the h*w positions of a frame).
 * ws / ws_bytes (round 6; may be NULL / 0): caller-owned scratch for a split of the KEY axis - when the 128-row query blocks alone leave most
 * CUs idle (113 blocks at the 14 400 positions of a 720p frame) up to four workgroups share a query block's keys, write un-normalised fp32
 * partial results (nsplit * Nq * (C + 2) * 4 bytes) and a second launch merges them; without a workspace one workgroup walks all keys. */
int ce_attention_1head_bf16(const void* Q, const void* K, const void* Vt, void* O, int Nq, int Nk, int C, int ldq, int ldk, int ldvt,
                            int ldo, float softmax_scale, void* ws, long long ws_bytes, hipStream_t stream);

/* probs[m][0:npad] = bf16(softmax(scale * scores[m][0:n])) (zeros beyond n); scores fp32.  Mid-block attention
 * (wan2pt1.py:247-252) runs as GEMM (CE_EPI_F32) -> this -> GEMM. */
int ce_softmax_rows_f32_bf16(const float* scores, void* probs, int M, int n, int npad, int ld, int ldp, float scale,
                             hipStream_t stream);

/* ---- fp8 (OCP e4m3) path of BASELINE.json configs[4].  The reference has no fp8 inference code: the contract is defined
 * here (per-row activation scales, per-output-channel weight scales, fp32 accumulation on the MX matrix instruction) ---- */

/* q[m][k] = fp8_e4m3(x[m][k] / s[m]), s[m] = max_k |x[m][k]| / 448 (1 for an all-zero row); x bf16 [M][ldx], q bytes [M][ldq].
 * Used for activations (per token row) and, once at load time, for nn.Linear weights (per output channel). */
int ce_quant_rows_fp8(const void* x, void* q, float* scale, int M, int K, int ldx, int ldq, hipStream_t stream);

/* ce_ln_affine_bf16 followed by ce_quant_rows_fp8 in one pass: q / scale are the quantisation of the bf16 row that
 * ce_ln_affine_bf16 would have written (bit-identical to the two-launch form). */
int ce_ln_affine_fp8(const void* x, void* q, float* scale, const float* a, const float* b, int M, int D, int ldx, int ldq, float eps,
                     int ab_rows, int ab_stride, hipStream_t stream);

/* C = epilogue(sa[m] * sw[n] * (Aq Wq^T)[m][n] + bias[n]); Aq [M][lda], Wq [N][ldw] fp8 e4m3 bytes, C bf16; K % 256 == 0.
 * Epilogues 0 (bias), 1 (bias + tanh GELU), 2 (gated residual) and the split-K scratch ws / ws_bytes as ce_gemm_bf16. */
int ce_gemm_fp8(const void* Aq, const void* Wq, void* C, const float* sa, const float* sw, const float* bias, int epilogue,
                const float* gate, const void* res, int M, int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows,
                void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- the MX form of the fp8 GEMMs (round 4; BASELINE.json configs[4] "fp8 weights"): OCP MXFP8 operands - e4m3 elements with one E8M0
 * scale per 32 consecutive K elements of a row, scale = the smallest power of two with amax / scale <= 448 (2^-126 for an all-zero block:
 * the non-saturating choice - with the OCP floor rule 2^(floor(log2 amax) - 8) an eighth of the blocks have their largest elements clipped),
 * elements RNE(x / scale) - and the block scales applied INSIDE the matrix pipe by v_mfma_scale_f32_16x16x128_f8f6f4.
 * Scale bytes are stored in the order the GEMM reads them.
 * A operand (activations; every producer of this library writes it): [ceil(rows / 128)][K / 128][4][16][8], i.e. the scale of elements
 * [128 t + 32 g, + 32) of row r at byte ((r / 128 * (K / 128) + t) * 4 + g) * 128 + (r % 16) * 8 + (r / 16) % 8.
 * W operand (weights; round 6): [ceil(rows / 128)][K / 128][4][128], the same byte with r % 128 in place of (r % 16) * 8 + (r / 16) % 8 - the
 * GEMM feeds fragment G of a wave tile with the weight rows G + 8 i, so that a lane's eight accumulators are eight CONSECUTIVE output columns
 * (the epilogue stores straight from registers, csrc/ce_gemm_fp8w4.hip), and a lane's eight scale bytes are consecutive in this order.
 * A scale buffer holds ceil(rows / 128) * (K / 128) * 512 bytes in either order.
 * The reference has no fp8 path: the contract is oracle.dit_oracle.mx_quant / linear_mxfp8. ---- */

/* x bf16 [M][ldx] -> q e4m3 bytes [M][ldq] + scale8 in the A order (above).  K % 128 == 0.  Activations (per token row). */
int ce_quant_rows_mxfp8(const void* x, void* q, void* scale8, int M, int K, int ldx, int ldq, hipStream_t stream);

/* The same with scale8 in the W order: the weight operand of ce_gemm_mxfp8 / ce_gemm_mxfp8_gelu_quant, quantised once at load time. */
int ce_quant_rows_mxfp8_w(const void* x, void* q, void* scale8, int M, int K, int ldx, int ldq, hipStream_t stream);

/* ce_ln_affine_bf16 followed by ce_quant_rows_mxfp8 in one pass (the quantisation of the bf16 row ce_ln_affine_bf16 would have written). */
int ce_ln_affine_mxfp8(const void* x, void* q, void* scale8, const float* a, const float* b, int M, int D, int ldx, int ldq, float eps,
                       int ab_rows, int ab_stride, hipStream_t stream);

/* C = epilogue(sum_blocks 2^(ea + ew) (Aq Wq^T)_block + bias[n]); Aq [M][lda], Wq [N][ldw] e4m3 bytes with their scale buffers sa8 (A order) / sw8 (W order),
 * C bf16; K % 256 == 0, N % 8 == 0.  Epilogues 0 (bias), 1 (bias + tanh GELU), 2 (gated residual; gate rows per sample >= 256 or one gate)
 * as ce_gemm_bf16; the one-wave-per-SIMD main loop of csrc/ce_gemm_fp8w4.hip, split-K tail through ws / ws_bytes as ce_gemm_bf16. */
int ce_gemm_mxfp8(const void* Aq, const void* Wq, void* C, const void* sa8, const void* sw8, const float* bias, int epilogue, const float* gate,
                  const void* res, int M, int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, void* ws, size_t ws_bytes,
                  hipStream_t stream);

/* The FFN-up form: q_out / qs_out = ce_quant_rows_mxfp8( bf16( gelu_tanh( bf16( Aq Wq^T + bias ) ) ) ) - the bias + GELU epilogue emits the
 * NEXT GEMM's MX operand directly (bit-identical to ce_gemm_mxfp8 with epilogue 1 followed by ce_quant_rows_mxfp8; the bf16 matrix is
 * never written: an MX block is 32 consecutive output columns = four adjacent 16-byte chunks of the staged row, so its scale needs no
 * row-wide reduction).  q_out e4m3 bytes [M][ldq], qs_out the tiled scales of an [M][N] operand.  N % 128 == 0, K % 256 == 0.
 * Split-K scratch ws / ws_bytes as ce_gemm_bf16. */
int ce_gemm_mxfp8_gelu_quant(const void* Aq, const void* Wq, const void* sa8, const void* sw8, const float* bias, void* q_out, void* qs_out,
                             int M, int N, int K, int lda, int ldw, int ldq, void* ws, size_t ws_bytes, hipStream_t stream);


/* ---- MXFP8 self-attention of the fp8 mode ("fp8 weights+attn", BASELINE.json configs[4]).  Contract (csrc/ce_attn_fp8.hip,
 * oracle/dit_oracle.py::attention_mxfp8): Q, K quantised to OCP MXFP8 - e4m3 elements, one E8M0 scale per 32 head channels - V per
 * 32 keys, products on v_mfma_scale_f32_32x32x64_f8f6f4, P = exp2(S - offset) <= 8 in e4m3 (offset = a row maximum - 3), fp32
 * accumulation; replaces
 * F.scaled_dot_product_attention at transformer_chronoedit.py:91-104 in that mode. ---- */

/* ce_rmsnorm_rope_bf16 that writes MXFP8 instead of bf16: q8 [M][ldq8] e4m3 bytes, scale8 [M][D/32] E8M0 bytes (x is not modified);
 * the bf16-rounded value is multiplied by post_scale before the quantisation - softmax_scale * log2(e) for q (the scores then leave
 * the matrix pipe in the exp2 domain), 1 for k.  transformer_chronoedit.py:62-65,73-79. */
int ce_rmsnorm_rope_mxfp8(const void* x, const float* w, const float* cos_sin, void* q8, void* scale8, int M, int D, int ldx, int ldq8,
                          int head_dim, float eps, int rope_rows, float post_scale, hipStream_t stream);

/* V [batch * n_tokens][ldv] bf16 (head h = columns 128 h ..) -> V^T tiles v8t [batch][H][128][npad] e4m3 bytes + sv
 * [batch][H][npad/64][128][2] E8M0 bytes (npad = n_tokens rounded up to 64, zero keys at the end).  Inside every 64-key tile position
 * 32 g + j holds key 32 (j >> 4) + (j & 3) + 8 ((j & 15) >> 2) + 4 g - the order of the P operand in the matrix unit's accumulator
 * registers; one scale per 32 CONSECUTIVE keys (sv[..][t][d][beta] covers keys 64 t + 32 beta .. of channel d). */
int ce_v_mxfp8_transpose(const void* v, int ldv, void* v8t, void* sv, int n_tokens, int batch, int H, int npad, hipStream_t stream);

/* O [batch * Nq][ldo] bf16 = attention over the operands above (q8 / k8 row strides in bytes, head h at byte column 128 h; sq / sk
 * [rows][H * 4]); head_dim == 128. */
int ce_attention_mxfp8(const void* q8, const void* sq, const void* k8, const void* sk, const void* v8t, const void* sv, void* O, int Nq,
                       int Nkv, int npad, int H, int head_dim, int ldq8, int ldk8, int ldo, int batch, hipStream_t stream);

/* ce_attention_mxfp8 with its output written as the out-projection's MX fp8 operand (o8 / scale8 as in ce_attention_2seg_vt_quant_bf16):
 * bit-identical to ce_attention_mxfp8 followed by ce_quant_rows_mxfp8; always the software-pipelined body. */
int ce_attention_mxfp8_quant(const void* q8, const void* sq, const void* k8, const void* sk, const void* v8t, const void* sv, void* o8,
                             void* scale8, int Nq, int Nkv, int npad, int H, int head_dim, int ldq8, int ldk8, int ldo8, int batch,
                             hipStream_t stream);

/* Second segment of a TWO-segment attention under the same contract - the cross-attention, out = bf16(SDPA(q, k_text, v_text)) +
 * bf16(SDPA(q, k_image, v_image)) (transformer_chronoedit.py:96-107): as ce_attention_mxfp8 / ce_attention_mxfp8_quant on the second
 * segment's operands, with the bf16 rows o_add [batch Nq][ldadd] (the first segment's result, from a plain ce_attention_mxfp8 call) added to
 * this segment's bf16-rounded result.  The sum goes to O (bf16 [batch Nq][ldo]; may be o_add itself) or, quantised exactly as
 * ce_quant_rows_mxfp8 would quantise it, to o8 / scale8 (the out-projection's MX operand) - exactly one of O and o8 is non-NULL. */
int ce_attention_mxfp8_add(const void* q8, const void* sq, const void* k8, const void* sk, const void* v8t, const void* sv, const void* o_add,
                           int ldadd, void* O, int ldo, void* o8, void* scale8, int ldo8, int Nq, int Nkv, int npad, int H, int head_dim,
                           int ldq8, int ldk8, int batch, hipStream_t stream);



/* ---- conditioning encoders (run once per edit, outside the loop: pipeline_chronoedit.py:205-254; the arithmetic is
 * transformers==4.57.1 CLIPVisionModel / UMT5EncoderModel, restated in oracle/clip_oracle.py, oracle/umt5_oracle.py) ---- */

/* batch0 x batch1 independent C = A W^T products with two-level element strides (head within sample); epilogue 0 (bias,
 * bf16 C) or 4 (fp32 C, no bias).  The per-head Q K^T and P V products of the encoders' attention. */
int ce_gemm_batched_bf16(const void* A, const void* W, void* C, const float* bias, int epilogue, int M, int N, int K, int lda,
                         int ldw, int ldc, int batch0, int batch1, long long sA0, long long sA1, long long sW0, long long sW1,
                         long long sC0, long long sC1, hipStream_t stream);

/* cols[(b gh + py) gw + px][c P P + y P + x] = img[b][c][py P + y][px P + x], zero padded to Kpad columns: the im2col of
 * CLIPVisionEmbeddings.patch_embedding (Conv2d, kernel = stride = P, no bias). */
int ce_im2col_patch2d_bf16(const void* img, void* cols, int B, int C, int H, int W, int P, int Kpad, hipStream_t stream);

/* out[i][:] = table[ids[i]][:] (ids int64, clamped to [0, vocab)): UMT5Stack.embed_tokens. */
int ce_gather_rows_bf16(const void* table, const long long* ids, void* out, int n, int D, int ldt, int ldo, int vocab,
                        hipStream_t stream);

/* y = bf16(bf16(x * rsqrt(mean(x^2) + eps)) * w), statistics in fp32, w bf16: UMT5LayerNorm.forward. */
int ce_rmsnorm_bf16(const void* x, void* y, const void* w, int M, int D, int ldx, int ldy, float eps, hipStream_t stream);

/* probs[b][h][q][:] = softmax_k(scores[b][h][q][k] + table[bucket_lut[k - q + Lq - 1]][h]) over keys k < valid_len[b]
 * (fp32 in, bf16 out, columns [Lk, ldp) written as zeros); table / bucket_lut may both be NULL (no bias), valid_len may be
 * NULL (no padding mask).  A sample with valid_len[b] <= 0 has no key to attend: all its probabilities are written as zeros (never NaN).
 * UMT5Attention: position bias + extended attention mask + softmax in fp32. */
int ce_softmax_t5_bf16(const float* scores, void* probs, int batch, int heads, int Lq, int Lk, int ld, int ldp,
                       const int* bucket_lut, const float* table, const int* valid_len, hipStream_t stream);

/* Weight-side LoRA merge (csrc/ce_lora.hip): what switching adapters between edits costs instead of reloading the weights.
 *   W[n,k] = bf16_rne( fp32(W0[n,k]) + sum_i scales[i] * dot_i[n,k] ),   dot_i[n,k] = sum_r B_i[n,r] * A_i[r,k]
 * dot_i is the fp32-accumulated sum of the bf16 products over adapter i's rank (bf16 MFMA); each dot_i is multiplied by its fp32 scale
 * and the terms are added onto fp32(W0) in adapter order (a multiply and an add each); the result is rounded to bf16 once.
 * W0 = the pristine base, bf16 [N, K] (row stride ldw0); W = the destination, bf16 [N, K] (row stride ldw) - it may alias W0 (every
 * element is read before it is written) or be a row view of a taller buffer.  B[i] = bf16 [N, ranks[i]], A[i] = bf16 [ranks[i], K],
 * both row-major and contiguous, 16-byte aligned.  B, A (arrays of device pointers), ranks and scales are HOST arrays, read before the
 * call returns; the library keeps no state.  n_adapters == 0 copies W0 into W; at most 8 adapters per call.
 * K % 64 == 0, N % 8 == 0 (as ce_gemm_bf16); ranks multiples of 32 and <= 512 (the caller zero-pads others); ldw0, ldw multiples of 8.
 * Replaces PEFT's merge behind pipe.fuse_lora / set_adapters (scripts/run_inference_diffusers.py:349-376) on the switchable path. */
int ce_lora_merge_bf16(const void* W0, int ldw0, void* W, int ldw, int N, int K, int n_adapters, const void* const* B,
                       const void* const* A, const int* ranks, const float* scales, hipStream_t stream);

/* ---- TeaCache step skipping (csrc/ce_tea.hip; wan_video_new_chronoedit.py:1190-1239, chronoedit_amd/teacache.py) ----
 * ce_tea_rel_l1_bf16: T = bf16 [S, n], one time-projection row per scheduled step (contiguous, 16-byte aligned); out = fp32 [S, 2]:
 *   out[i][0] = sum_j |bf16(T[i][j] - T[i-1][j])|,  out[i][1] = sum_j |T[i-1][j]|  for i >= 1,  out[0] = {0, 0}.
 * fp32 accumulation in a fixed order (one workgroup per row): bit-identical from run to run.  n % 8 == 0, otherwise -2.
 * ce_tea_store_bf16: r[k] <- bf16(float(x[k]) - float(r[k])) - on entry r holds the tokens saved in front of the block stack, x the
 *   tokens behind it; afterwards r is the stack's residual (TeaCache.store, :1233).
 * ce_tea_apply_bf16: x[k] <- bf16(float(x[k]) + float(r[k])) (TeaCache.update, :1237).
 * Both: bf16, `count` elements, count % 8 == 0 (otherwise -2), x and r 16-byte aligned (otherwise -3), round to nearest even.
 * ce_tea_store_dist_bf16: ce_tea_store_bf16 (the same bits in r) that also measures, for calibrating the rescaling polynomial,
 *   sums[0] = sum_k |float(r_new[k]) - float(prev[k])|,  sums[1] = sum_k |prev[k]|  (fp32; the difference is not rounded to bf16).
 *   prev = bf16 [count], the previous step's residual: only read, 16-byte aligned, must overlap neither r nor x (otherwise -1).
 *   The sums are accumulated in fp32 in an order that `count` alone decides (lane-serial, butterfly within a wave, the waves in order,
 *   one pair per workgroup into `scratch`, the pairs added by a second small launch): no atomics, the same bits on every run.
 *   scratch: caller-owned, 4-byte aligned, at least 8 bytes per workgroup = 8 * min(2048, ceil(count / 2048)) bytes (16 KiB always
 *   suffices; a smaller one returns -1); the library keeps no state.  On any error nothing is launched. */
int ce_tea_rel_l1_bf16(const void* T, int S, int n, float* out, hipStream_t stream);
int ce_tea_store_bf16(const void* x, void* r, long long count, hipStream_t stream);
int ce_tea_apply_bf16(void* x, const void* r, long long count, hipStream_t stream);
int ce_tea_store_dist_bf16(const void* x, void* r, const void* prev, float* sums, float* scratch, long long scratch_bytes, long long count,
                           hipStream_t stream);

/* ---- image pre- and post-processing (csrc/ce_image.hip; chronoedit_amd/image_io.py): the byte passes of VideoProcessor.preprocess,
 * CLIPImageProcessor and VideoProcessor.postprocess_video (pipeline_chronoedit.py:247-256,673,801), bit-equal to PIL / numpy ----
 * ce_image_resample_u8: ONE 1-D pass of PIL's 8-bit resampler over interleaved RGB bytes.  src = uint8 [src_h][src_w][3];
 *   axis 0 (horizontal): dst = uint8 [src_h][out_len][3];  axis 1 (vertical): dst = uint8 [out_len][src_w][3].
 *   coeff = int32 [out_len][ksize] (22-bit fixed point), bounds = int32 [out_len][2] = (first, count) along the resampled axis, both in
 *   device memory, 4-byte aligned.  Per output index o and channel: ss = 2^21 + sum_{k < count} coeff[o][k] * src[first + k] (int32),
 *   out = clip(ss >> 22, 0, 255) with an arithmetic shift.  count is clipped to ksize and to the source extent.  src != dst.
 * ce_image_u8_lut_planar: dst[c][y][x] = lut[c][src[top + y][left + x][c]] for c < 3, y < out_h, x < out_w.  src = uint8 [src_h][src_w][3];
 *   lut = [3][256] and dst = [3][out_h][out_w] (contiguous) of bf16 (dst_f32 == 0) or fp32 (dst_f32 != 0), copied as bits.  The crop
 *   must lie inside the source (otherwise -1).
 * ce_video_to_u8: src = [B][3][F][H][W] of bf16 (src_f32 == 0) or fp32, contiguous; dst = uint8 [B][F][H][W][3].  Per element, in fp32 with
 *   every operation rounded on its own: f = v * 0.5 + 0.5, clamped to [0, 1], u = rint(f * 255) (half to even).  NaN gives 0.
 * No state, no scratch, nothing allocated: every call is capturable.  An image of 2^31 bytes or more returns -2. */
int ce_image_resample_u8(const void* src, void* dst, int axis, int src_h, int src_w, int out_len, const int* coeff, const int* bounds,
                         int ksize, hipStream_t stream);
int ce_image_u8_lut_planar(const void* src, int src_h, int src_w, int top, int left, int out_h, int out_w, const void* lut, void* dst,
                           int dst_f32, hipStream_t stream);
int ce_video_to_u8(const void* src, void* dst, int B, int F, int H, int W, int src_f32, hipStream_t stream);

/* ---- region-limited edits (csrc/ce_region.hip; chronoedit_amd/region.py): keep the source outside a caller-given mask - the flow-matching
 * form of the loop of diffusers' inpaint pipelines, latents = (1 - mask) * scale_noise(image_latents, t_next, noise) + mask * latents.
 * Every *, + and - below is an fp32 operation rounded on its own (no contraction): each pass is bit-equal to the eager torch expression.
 * ce_region_weights_u8: mask = uint8 [H][W] (255 = edit, 0 = keep, greys are weights), H and W multiples of 8 (otherwise -1);
 *   w = fp32 [H/8][W/8], w[i][j] = float(sum of the 64 bytes of tile (i, j)) / 16320.0f: the 8x8 box mean.  All-255 gives exactly 1.0f.
 * ce_region_blend_f32: in place on x (fp32 [n]), after a scheduler step:
 *     k = (1.0f - s) * z_src[i] + s * eps[i],   x[i] = w[i % plane] * x[i] + (1.0f - w[i % plane]) * k,   s = *sigma_next
 *   z_src, eps = fp32 [n]; w = fp32 [plane] (plane = h * w of the latents: broadcast over batch, channel and frame); n % plane == 0.
 *   sigma_next points to ONE float in device memory, read by the kernel: the loop stages the step's value there and one captured graph
 *   serves every step.  w == 1 leaves x bit-unchanged, w == 0 gives exactly k, s == 0 gives k == z_src.
 *   flags bit1: round the stored x to a bf16 value (ce_cfg_unipc_step's "reference-precision trajectory").  All pointers 4-byte aligned.
 * ce_region_composite: v = [B][3][F][H][W] of bf16 (v_is_bf16 != 0) or fp32, src = bf16 [B][3][H][W], mask = uint8 [H][W],
 *   out = fp32 [B][3][F][H][W] (not v):  m = float(mask[y][x]) / 255.0f,  out = m * v + (1.0f - m) * src[b][c][y][x]  - mask and source
 *   broadcast over the frames, the mask over samples and channels.  Where the mask is 0, out == float(src) for every finite v.
 * No state, no scratch, nothing allocated, no host read: every call is capturable. */
int ce_region_weights_u8(const void* mask, float* w, int H, int W, hipStream_t stream);
int ce_region_blend_f32(float* x, const float* z_src, const float* eps, const float* w, const float* sigma_next, long long n,
                        long long plane, int flags, hipStream_t stream);
int ce_region_composite(const void* v, int v_is_bf16, const void* src, const void* mask, float* out, int B, int F, int H, int W,
                        hipStream_t stream);

/* ---- automatic edit regions (csrc/ce_region_auto.hip; chronoedit_amd/auto_region.py): the region of an instruction-only edit, found from the
 * model's estimate of the final image after a few dense steps.  Every fp32 operation below is rounded on its own (no contraction); each pass
 * is bit-equal to the torch expression of auto_region.py.
 * ce_auto_region_change_f32: x0, z_src = fp32 [B][C][T][h][w] (contiguous), d = fp32 [h][w], on latent frame `frame` alone:
 *     d[y][x] = max over b of ((sum over c = 0..C-1, in that order, of (x0 - z_src)^2) / float(C));  a NaN stays a NaN.
 * ce_auto_region_otsu_f32: d = fp32 [n] (>= 0 or NaN) -> *thr, and *dmax when dmax is not NULL.  dmax = max(d) (NaNs ignored);
 *   scale = 256.0f / dmax;  bin = min(255, int(d * scale)), a NaN in bin 0;  t = the lowest arg-max over the t in 0..255 with 0 < w0 < n of
 *   (s0 n - S w0)^2 / (w0 (n - w0)) - w0, s0 = the cumulative count and sum of i n_i through bin t, S = s0 of bin 255; integers, the
 *   expression in float64 - or 0 when no t qualifies;  *thr = max(float(t + 1) * (dmax / 256.0f), floor * floor).  dmax == 0: *thr = +inf.
 *   One workgroup; n < 2^24, floor >= 0.
 * ce_auto_region_ramp_f32: seed = d > *thr (thr in device memory);  w[y][x] = ramp(r), r = the smallest Chebyshev distance to a seed within
 *   R = dilate + feather <= 8 cells (0 when there is none; cells outside the grid are no seeds): ramp(r) = 1.0f for r <= dilate, else
 *   float(feather + 1 - (r - dilate)) / float(feather + 1).  d and w = fp32 [h][wl], not the same buffer.
 * ce_auto_region_mask_u8: w = fp32 [h][wl] -> mask = uint8 [8 h][8 wl], byte = rint(255.0f * w[Y / 8][X / 8]) (half to even, clamped to
 *   0..255): what ce_region_composite and ce_region_weights_u8 take; w in {0, 1} comes back from the latter unchanged.
 * No state, no scratch, nothing allocated, no host read: every call is capturable.  fp32 pointers 4-byte aligned. */
int ce_auto_region_change_f32(const float* x0, const float* z_src, float* d, int B, int C, int T, int h, int w, int frame,
                              hipStream_t stream);
int ce_auto_region_otsu_f32(const float* d, int n, float floor_v, float* thr, float* dmax, hipStream_t stream);
int ce_auto_region_ramp_f32(const float* d, const float* thr, float* w, int h, int wl, int dilate, int feather, hipStream_t stream);
int ce_auto_region_mask_u8(const float* w, void* mask, int h, int wl, hipStream_t stream);

/* ---- sparse region edits (csrc/ce_sparse.hip; chronoedit_amd/sparse_region.py): the gather / scatter layer of a step that runs the DiT on
 * the Na ACTIVE token rows per sample only.  ids = Na sorted, unique token indices in [0, N) - int32, or int64 when ids_i64 != 0 - in device
 * memory, the same for every sample; the host validates them once per edit, and an id outside [0, N) is skipped by every pass.
 * Pure data movement: bit-equal to the indexing expression, nothing outside the listed rows / columns / cells is written.
 * ce_sparse_patchify_bf16: x [C][T][H][W] -> cols [Na][Kpad]: row a = row ids[a] of ce_patchify_bf16's result.
 * ce_sparse_scatter_rows_bf16: src [B*Na][lds] -> dst [B*N][ldd] (D columns, D % 8 == 0; lds, ldd multiples of 8, both pointers 16-byte
 *   aligned): row b*Na + a goes to row b*N + ids[a] - K after norm + RoPE into the cached K.
 * ce_sparse_scatter_vt_bf16: the fresh V of the active tokens -> columns b*N + ids[a] of vt [D][ldvt] (ldvt >= B*N).  src_rows == 0: src is
 *   V^T [D][lds], sample b's active token a in column b*Na + a (what the transposed-store GEMM, CE_EPI_BIAS_T, leaves); src_rows != 0: src is
 *   row-major V [B*Na][lds], transposed on the way.  Columns not listed, the padding columns among them, are not written.
 * ce_sparse_unpatchify_bf16: y [Na][ldy] (col = (dh*2+dw)*Cout + c, as ce_unpatchify_bf16) -> the 2 x 2 cells of token ids[a] in
 *   out [Cout][T][H][W].
 * No state, no scratch, nothing allocated, no host read: every call is capturable. */
int ce_sparse_patchify_bf16(const void* x, const void* ids, int ids_i64, void* cols, int C, int T, int H, int W, int Kpad, int Na,
                            hipStream_t stream);
int ce_sparse_scatter_rows_bf16(const void* src, int lds, void* dst, int ldd, const void* ids, int ids_i64, int Na, int N, int B, int D,
                                hipStream_t stream);
int ce_sparse_scatter_vt_bf16(const void* src, int lds, int src_rows, void* vt, int ldvt, const void* ids, int ids_i64, int Na, int N, int B,
                              int D, hipStream_t stream);
int ce_sparse_unpatchify_bf16(const void* y, int ldy, const void* ids, int ids_i64, void* out, int Cout, int T, int H, int W, int Na,
                              hipStream_t stream);

/* ---- focused region edits (csrc/ce_focus.hip; chronoedit_amd/focus.py): the edit runs on a crop of the photo around the mask and is pasted
 * back into the photo at the photo's own size.  Both passes are integer-exact, bit-equal to the installed PIL.
 * ce_focus_resample_l8: ONE 1-D pass of PIL's 8-bit resampler over SINGLE-channel bytes: ce_image_resample_u8's tables and arithmetic
 *   (ss = 2^21 + sum_k coeff[o][k] * src[first + k], out = clip(ss >> 22, 0, 255)).  src = src_h rows of src_w bytes, row y at
 *   src + y * src_pitch (src_pitch >= src_w, otherwise -1): a crop of a larger image is read where it lies.  dst is contiguous:
 *   axis 0 (horizontal) uint8 [src_h][out_len], axis 1 (vertical) uint8 [out_len][src_w].  src != dst.  With image_io.resize_tables(...,
 *   "bilinear"), horizontal then vertical equals Image.resize(..., Image.BILINEAR) of an "L" image.
 * ce_focus_paste_u8: edit = uint8 [F][bh][bw][3] (the frames, scaled to the box), src = uint8 [src_h][src_w][3] (the photo), mask = uint8
 *   [src_h][src_w] at the photo's size or NULL (= 255 everywhere), out = uint8 [F][src_h][src_w][3], aliasing no input.  Outside the box
 *   [top, top + bh) x [left, left + bw) out = src.  Inside, per byte, with m = mask[Y][X], s = src, e = edit[f][Y - top][X - left][c], in
 *   32-bit integers:  t = s * (255 - m) + e * m + 128,  out = ((t >> 8) + t) >> 8  - Image.paste(edit, (left, top), mask).  m == 0 gives s
 *   and m == 255 gives e exactly.  A box that leaves the image returns -1; F <= 65535.
 * No state, no scratch, nothing allocated: every call is capturable.  An image of 2^31 bytes or more returns -2. */
int ce_focus_resample_l8(const void* src, long long src_pitch, void* dst, int axis, int src_h, int src_w, int out_len, const int* coeff,
                         const int* bounds, int ksize, hipStream_t stream);
int ce_focus_paste_u8(const void* edit, const void* src, const void* mask, void* out, int F, int src_h, int src_w, int left, int top, int bw,
                      int bh, hipStream_t stream);

/* ---- auto-focused edits (csrc/ce_autofocus.hip; chronoedit_amd/autofocus.py): an instruction-only edit finds its region on the whole photo,
 * lifts the detected mask to the photo's size on the device and goes on as a focused region edit of the crop.
 * ce_autofocus_bbox_u8: mask = H rows of W bytes, row y at mask + y * pitch (pitch >= W, otherwise -1: a box's view of a larger mask is
 *   reduced where it lies) -> out = int32 [5]: left, top, right, bottom (half open) of mask > 0, then the count of non-zero bytes.  An empty
 *   mask gives W, H, 0, 0, 0.  `out` is initialised by a leading launch of the call itself; integers only, so the result is exact and does
 *   not depend on the launch order.  H * W < 2^31 (otherwise -2).
 * ce_autofocus_restart_f32: x0, eps, out = fp32 [planes][h][w] (contiguous; out != x0), ix0, ix1 = int32 [w], fx = fp32 [w], iy0, iy1 =
 *   int32 [h], fy = fp32 [h] in device memory (an index outside the grid is clamped into it).  With a00 = x0[p][iy0[y]][ix0[x]], a01 =
 *   x0[p][iy0[y]][ix1[x]], a10 = x0[p][iy1[y]][ix0[x]], a11 = x0[p][iy1[y]][ix1[x]]:
 *     top = a00 + fx * (a01 - a00),  bot = a10 + fx * (a11 - a10),  v = top + fy * (bot - top),  out = (1 - s) * v + s * eps[p][y][x]
 *   every operation an fp32 operation rounded on its own (no contraction); bf16_state != 0: out is rounded to a bf16 value (fp32 storage).
 * No state, no scratch, nothing allocated, no host read: every call is capturable.  int32 / fp32 pointers 4-byte aligned (otherwise -3). */
int ce_autofocus_bbox_u8(const void* mask, long long pitch, int H, int W, int* out, hipStream_t stream);
int ce_autofocus_restart_f32(const float* x0, const float* eps, float* out, const int* ix0, const int* ix1, const float* fx, const int* iy0,
                             const int* iy1, const float* fy, float s, int planes, int h, int w, int bf16_state, hipStream_t stream);

/* ---- live previews (csrc/ce_preview.hip; chronoedit_amd/preview.py): an RGB estimate of the running edit from the scheduler's predict-x0
 * slot through a fitted linear map, and the Gram matrix that map is fitted from.  Every fp32 operation is rounded on its own.
 * ce_preview_rgb_u8: x0 (and z_src) = fp32 [B][C = 16][T][h][w] (contiguous), on latent frame `frame`; w = fp32 [h][w]; z_src and w are both
 *   given or both NULL; factors = fp32 [17][3] (rows 0..15 channel weights, row 16 the bias); out = uint8 [B][h scale][w scale][3], scale in
 *   {1, 2, 4, 8}.  Per cell: u_k = (w * x0_k) + ((1 - w) * z_k), or x0_k without w;  p_c = factors[16][c], then for k = 0..15 in order
 *   p_c = p_c + factors[k][c] * u_k.  Per pixel, half-pixel centres: fy = (Y + 0.5) / scale - 0.5 clamped to [0, h - 1], y0 = floor(fy),
 *   y1 = min(y0 + 1, h - 1), ty = fy - y0, the same along X;  top = p(y0, x0) * (1 - tx) + p(y0, x1) * tx, bot likewise on y1,
 *   v = top * (1 - ty) + bot * ty;  the byte is ce_video_to_u8's: rint(clamp(v * 0.5 + 0.5, 0, 1) * 255), NaN -> 0.  Every byte of out is written.
 * ce_preview_gram_f64: z = fp32 [B][16][T][h][w] on latent frame `frame`; y = [B][3][8 h][8 w] of fp32 (y_bf16 == 0) or bf16;
 *   out = float64 [20][20] = sum over samples and cells of v v^T, v = (z_0..z_15, 1, r, g, b), r / g / b = (the fp32 sum of the cell's 8 x 8
 *   pixels in row-major order) * 0.015625f.  Products and sums are float64 in a fixed order: per-workgroup partials in `scratch` (8-byte
 *   aligned, at least 1680 bytes - otherwise -1; more lets more workgroups run, up to 1024 x 1680), added in workgroup order by a second
 *   launch.  The same arguments give the same bits.
 * No state, nothing allocated, no host read: every call is capturable.  fp32 pointers 4-byte aligned (otherwise -3). */
int ce_preview_rgb_u8(const float* x0, const float* z_src, const float* w, const float* factors, void* out, int B, int C, int T, int frame,
                      int h, int wl, int scale, hipStream_t stream);
int ce_preview_gram_f64(const float* z, int frame, const void* y, int y_bf16, double* out, void* scratch, size_t scratch_bytes, int B, int T,
                        int h, int wl, hipStream_t stream);

/* ---- guided detail lift (csrc/ce_lift.hip; chronoedit_amd/lift.py): a whole-image edit made at the edit's size is carried up to the photo's
 * pixel grid.  lift.reference (CPU torch) is the definition; every pass is bit-equal to its stage.  L = uint8 [H][W][3] (the photo resized to
 * the edit's size), E = uint8 [F][H][W][3] (the frames), P = uint8 [SH][SW][3] (the photo), U = uint8 [F][SH][SW][3] (the frames' Lanczos
 * upsample) or NULL.  Box sums run over the window [y - r, y + r] x [x - r, x + r] clipped to the image, n = its cell count, r = radius in
 * 1..16 (otherwise -1).  Every fp32 / fp64 operation is rounded on its own.
 * ce_lift_fit_q16: per frame, cell and colour, I = L_c, d = E_c - I; the integer box sums S_I, S_d, S_II, S_Id; in int64
 *   num = n S_Id - S_I S_d, den = n S_II - S_I^2 + eps_q n^2 (eps_q in 1..2^30: squared bytes; both below 2^53);
 *   a = fp32(clamp(double(num) / double(den), -max_gain, max_gain)), 1 <= max_gain <= 8;  b = fp32((double(S_d) - double(a) * double(S_I)) /
 *   double(n));  AB = int32 [F][H][W][6] = rint(65536 a_rgb), rint(65536 b_rgb).
 * ce_lift_smooth_f32: the int64 box sums of A and B -> abar = fp32(double(sum A) / double(65536 n)), bbar likewise;  res = max over colours
 *   of |float(d) - (abar * float(I) + bbar)|;  coef = fp32 [F][H][W][8] = abar_rgb, bbar_rgb, 0, 0 (16-byte aligned);  R = int32 [F][H][W] =
 *   rint(256 min(res, 255)).
 * ce_lift_gate_f32: coef[..][6] = clamp((fp32(double(box sum R) / double(256 n)) - t0) / (t1 - t0), 0, 1), 0 <= t0 < t1 (otherwise -1).
 *   Without this call g = 0: no fallback.
 * ce_lift_apply_u8: ix0, ix1 = int32 [SW], tx = fp32 [SW], iy0, iy1 = int32 [SH], ty = fp32 [SH] in device memory: the corner cells and
 *   weight of every photo column and row (lift.axis_table; an index outside the grid is clamped into it).  Per output byte, p = float(P),
 *   c00 .. c11 the four corner cells:  top = c00 * (1 - tx) + c01 * tx, bot likewise, v = top * (1 - ty) + bot * ty, for abar_c, bbar_c and g;
 *   q = p + (a_up * p + b_up);  with U: q = q + g_up * (float(U) - q);  out = rint(clamp(q, 0, 255)), NaN -> 0.  out = uint8 [F][SH][SW][3],
 *   aliasing no input; every byte is written.  U is not read where g_up == 0.  16-byte accesses when SH * SW % 16 == 0 and P, U, out are
 *   16-byte aligned, byte by byte otherwise - the same bytes.
 * What follows from the arithmetic: E == L gives out == P byte for byte (a = b = g = 0, p + (0 p + 0) = p); wherever E == L over the
 * +-(3 r + 1)-cell neighbourhood of a pixel's four corners, the pixel is P's; wherever g_up == 1 the pixel is U's.
 * No state, nothing allocated, no host read: every call is capturable.  F <= 65535.  A plane of 2^31 bytes or more (H * W * 3, SH * SW * 3,
 * H * W * 32) returns -2; AB, R and the tables 4-byte, coef 16-byte aligned (otherwise -3). */
int ce_lift_fit_q16(const void* L, const void* E, int* AB, int F, int H, int W, int radius, int eps_q, float max_gain, hipStream_t stream);
int ce_lift_smooth_f32(const void* L, const void* E, const int* AB, float* coef, int* R, int F, int H, int W, int radius, hipStream_t stream);
int ce_lift_gate_f32(const int* R, float* coef, int F, int H, int W, int radius, float t0, float t1, hipStream_t stream);
int ce_lift_apply_u8(const void* P, const void* U, const float* coef, const int* ix0, const int* ix1, const float* tx, const int* iy0,
                     const int* iy1, const float* ty, void* out, int F, int SH, int SW, int H, int W, hipStream_t stream);

/* ---- sketch edits (csrc/ce_sketch.hip; chronoedit_amd/sketch.py): the region of an edit drawn on the photo is where the editor's composite
 * differs from its background, grown and feathered at the photo's size.  sketch.reference (CPU torch) is the definition; every pass is
 * bit-equal to its stage.  Planes are uint8 [H][W], contiguous.
 * ce_sketch_changed_u8: background, composite = uint8 [pixels][3] -> out = uint8 [pixels]: 255 where max over the three channels of
 *   |composite - background| > threshold, else 0.  threshold in 0..254 (otherwise -1).  16-byte accesses when all three pointers are
 *   16-byte aligned, byte by byte otherwise - the same bytes.
 * ce_sketch_dilate_u8: one axis (0: along a row, 1: along a column) of the maximum filter of a 0 / 255 plane, the window [i - radius,
 *   i + radius] clipped to the image: dst = 255 where the window holds a non-zero byte of src, else 0 (the input is binary by construction,
 *   so the pass counts).  radius in 0..4096 (otherwise -1).
 * ce_sketch_box_u8: one axis of the box mean, the window [i - radius, i + radius] over the line continued by its edge bytes: acc = the
 *   integer sum of the 2 radius + 1 bytes, ww = 2^24 / (2 radius + 1) in integers, dst = (acc * ww + 2^23) >> 24 - PIL's BoxBlur for an
 *   integer radius.  radius in 0..1024 (otherwise -1).
 * What a pass costs per byte: along a row a window sum is the difference of two entries of a prefix sum built in the LDS (up to 52 KiB of it
 *   at the largest radius) - the run of 4096 outputs reads 2 radius more input bytes, nothing else follows the radius.  Along a column it is
 *   a running sum (two loads per output) over segments of 32 rows, four adjacent columns per lane; the first window of a segment is summed
 *   row by row while it holds at most 128 rows (radius <= 63: 2 to 6 loads per output), and from per-segment sums otherwise: a first launch
 *   writes uint16 [ceil(H / 32)][W] to `scratch`, and a segment then gathers fewer than 64 rows and (2 radius + 1) / 32 eight-byte entries -
 *   the one term that still follows the radius, at most 8 such loads per output at radius 4096.  The grid does not depend on the radius.
 *   W % 4 != 0, or a base that is not 4-byte aligned: the column passes keep four columns per lane but move single bytes (the same
 *   bytes come out; measured 2 - 4 times slower, profiles/notes_sketch.md).
 * scratch: needed when axis == 1 and radius >= 64: at least ceil(H / 32) * W * 2 bytes, 8-byte aligned (otherwise -1 / -3), aliasing neither
 *   plane; ignored (may be NULL) otherwise.
 * out / dst alias no input (otherwise -1); every byte of it is written.  No state, nothing allocated, no host read: every call is
 * capturable.  Integers only: the result is exact and does not depend on the launch order.  An image of 2^31 bytes or more (pixels * 3,
 * H * W) returns -2. */
int ce_sketch_changed_u8(const void* background, const void* composite, void* out, long long pixels, int threshold, hipStream_t stream);
int ce_sketch_dilate_u8(const void* src, void* dst, int H, int W, int axis, int radius, void* scratch, size_t scratch_bytes,
                        hipStream_t stream);
int ce_sketch_box_u8(const void* src, void* dst, int H, int W, int axis, int radius, void* scratch, size_t scratch_bytes, hipStream_t stream);

/* ---- connected components of a byte plane (csrc/ce_components.hip; chronoedit_amd/components.py): speckle removal for sketched and
 * detected regions.  Foreground is a non-zero byte, the neighbourhood is 8-connected; components.reference (numpy, on row runs) is the
 * definition and every pass gives its bits.  Planes are [H][W], contiguous, H * W < 2^31 (otherwise -2); int32 planes 4-byte aligned
 * (otherwise -3); byte planes at any address.
 * ce_components_roots_i32: plane uint8 -> labels int32: for a foreground pixel the smallest index y * W + x of its component, -1 for
 *   background.  Three launches: 32 x 64 tiles labelled in the LDS (row runs, then a union-find over touching runs), unions across the tile
 *   borders by device-scope atomicMin whose returned value decides, and a pass that replaces every label by its root.  Every byte of
 *   `labels` is written; it needs no initialisation.
 * ce_components_sums_i32: labels (+ weight uint8, or NULL: every pixel counts) -> sums int32: at a root's own position the number of its
 *   component's pixels whose weight byte is non-zero, 0 everywhere else.  One integer atomic per wave and distinct root, a root that goes
 *   on along a workgroup's run of pixels added once.
 * ce_components_keep_u8: out = plane where the component's weight is >= the least weight kept, else 0; counters int32 [4] = components
 *   kept, components dropped, weight dropped, largest weight (zeroed by the call).  den == 0: the least weight is min_weight >= 1;
 *   0 < num < den <= 65536: it is ceil(num * largest / den), computed on the device in 64-bit integers - nothing is read back.
 * ce_components_seeds_f32: seeds[i] = d[i] > thr[0] ? 255 : 0 (thr in device memory; a NaN is no seed).
 * ce_components_masked_f32: out[i] = kept[i] != 0 ? d[i] : -1 - the change map of an automatic region without its dropped seeds.
 * Outputs alias no input (otherwise -1).  No state, nothing allocated, no host read, no wait between workgroups: every call is capturable.
 * Integers and integer atomics only: the results are exact and do not depend on the launch order. */
int ce_components_roots_i32(const void* plane, int* labels, int H, int W, hipStream_t stream);
int ce_components_sums_i32(const int* labels, const void* weight, int* sums, int H, int W, hipStream_t stream);
int ce_components_keep_u8(const void* plane, const int* labels, const int* sums, void* out, int* counters, int min_weight, int num, int den,
                          int H, int W, hipStream_t stream);
int ce_components_seeds_f32(const float* d, const float* thr, void* seeds, int n, hipStream_t stream);
int ce_components_masked_f32(const float* d, const void* kept, float* out, int n, hipStream_t stream);

/* ---- sketch edits with one crop per group of stroke clusters (csrc/ce_clusters.hip; chronoedit_amd/clusters.py is the definition and every
 * pass gives its bits).  labels / sums are ce_components_roots_i32's / ce_components_sums_i32's planes of the grown plane, kept the plane
 * ce_components_keep_u8 left of it (or the grown plane itself).  Planes are [H][W], contiguous, H * W < 2^31 (otherwise -2); int32 planes
 * and arrays 4-byte aligned (otherwise -3); byte planes at any address.  The table is int32 [256][8].
 * ce_clusters_table_i32: one row per KEPT cluster - a root position p (labels[p] == p) with kept[p] != 0 - in ascending label order:
 *   label, left, top, right, bottom (the half-open bounding box of the pixels with that label and a non-zero kept byte), their number,
 *   sums[label], 0.  counters = int32 [1 + rows]: counters[0] <- the number of kept clusters, exact whatever it is; the rest is the call's
 *   scratch.  Rows at and after the count are 0; with a count above `rows` the rows are unspecified (the first `rows` labels to arrive).
 *   rows must be 256 (otherwise -1: a caller with another table in mind is refused, not written past).  A 4-byte memset and three
 *   launches: the roots append their labels through counters[0]; one workgroup ranks them (row = the number of smaller labels) and
 *   initialises every row; a pixel pass finds its row by binary search, reduces min / max / count per workgroup in the LDS and flushes
 *   the rows it touched with atomicMin / atomicMax / atomicAdd.  `table` and `counters` need no initialisation and alias nothing.
 * ce_clusters_select_u8: out[p] = 255 where kept[p] != 0 and labels[p] is the label of a row i of `table` (as the call above left it) with
 *   group_of_row[i] == g, else 0.  group_of_row = int32 [256] in device memory; g >= 0.  Labels 16-byte, kept and out 4-byte aligned: four
 *   pixels per lane, one 16-byte label load; otherwise element by element - the same bytes.  out aliases no input (otherwise -1).
 * ce_clusters_paste_u8: Image.paste(edit[f], (left, top), mask) into canvas[f] IN PLACE, for every frame: edit = uint8 [F][bh][bw][3],
 *   mask = uint8 [src_h][src_w] at the photo's size or NULL (= 255 everywhere), canvas = uint8 [F][src_h][src_w][3].  Only bytes of the box
 *   [top, top + bh) x [left, left + bw) are touched, each reading and writing its own address, with ce_focus_paste_u8's arithmetic:
 *   t = c * (255 - m) + e * m + 128, c = ((t >> 8) + t) >> 8; under m == 0 nothing is written.  A box that leaves the image returns -1;
 *   F <= 65535; canvas aliases neither edit nor mask.  The first crop of a photo goes through ce_focus_paste_u8, which builds the canvas.
 * No state, nothing allocated, no host read, no wait between workgroups, every loop bounded: every call is capturable.  Integers and integer
 * atomics only: the results are exact and do not depend on the launch order. */
int ce_clusters_table_i32(const int* labels, const int* sums, const void* kept, int* table, int* counters, int rows, int H, int W,
                          hipStream_t stream);
int ce_clusters_select_u8(const int* labels, const void* kept, const int* table, const int* group_of_row, int g, void* out, int H, int W,
                          hipStream_t stream);
int ce_clusters_paste_u8(const void* edit, const void* mask, void* canvas, int F, int src_h, int src_w, int left, int top, int bw, int bh,
                         hipStream_t stream);

/* ---- sketch edits from an image editor's layers (csrc/ce_layers.hip; chronoedit_amd/layers.py is the definition and both passes give its
 * bits).  layer = uint8 [bh][bw][4], RGBA: the layer's alpha bounding box, placed at (left, top) of the photo of SW x SH pixels.  Both calls
 * work IN PLACE and touch only bytes of the box [top, top + bh) x [left, left + bw); a box that leaves the photo returns -1.
 * ce_layers_strokes_u8: plane = uint8 [SH][SW]: plane[p] = 255 where the layer's alpha > threshold, every other byte is left as it is - on a
 *   plane the caller zeroed, the layers of a value give "255 where max over the layers of alpha > threshold".  threshold in 0..254
 *   (otherwise -1).
 * ce_layers_over_u8: canvas = uint8 [SH][SW][3]: Image.alpha_composite(canvas, layer) over an opaque canvas, per channel
 *   u = s * a + d * (255 - a) + 128, d = ((u >> 8) + u) >> 8 - ce_focus_paste_u8's arithmetic with the alpha as the mask; under a == 0
 *   the byte stays.
 * One lane per run of up to four pixels of a row.  Where the row address allows it a run moves as whole words - strokes: the layer's four
 *   pixels as one 16-byte load; over: the canvas's twelve bytes as three aligned dwords, the layer's as one 16-byte load or four dwords -,
 *   and the pixels in front of a row's first such address, its remainder, and everything at a base that is not 4-byte aligned move byte by
 *   byte: the same bytes.  Any base address, any width.
 * layer aliases neither plane nor canvas (otherwise -1).  No state, nothing allocated, no host read: every call is capturable.  Integers
 * only: exact, and a pixel is read and written by one lane.  A photo or a box of 2^31 bytes or more returns -2. */
int ce_layers_strokes_u8(const void* layer, int bw, int bh, int left, int top, void* plane, int SW, int SH, int threshold, hipStream_t stream);
int ce_layers_over_u8(const void* layer, int bw, int bh, int left, int top, void* canvas, int SW, int SH, hipStream_t stream);

/* ---- guided detail lift inside a focus box (csrc/ce_boxlift.hip; chronoedit_amd/boxlift.py is the definition and the pass gives its bits):
 * stage 4 of the lift fused with the paste of a focused edit.
 * ce_boxlift_apply_paste_u8: works IN PLACE on canvas = uint8 [F][src_h][src_w][3], inside the box [top, top + bh) x [left, left + bw).
 *   P = uint8 [src_h][src_w][3], the photo the crop was cut from, read at (top + y, left + x);  U = uint8 [F][bh][bw][3], the frames'
 *   Lanczos upsample to the box, or NULL;  coef = fp32 [F][H][W][8], the cells ce_lift_smooth_f32 / ce_lift_gate_f32 left (16-byte aligned);
 *   ix0, ix1 = int32 [bw], tx = fp32 [bw], iy0, iy1 = int32 [bh], ty = fp32 [bh] in device memory: lift.tables((bw, bh), (H, W)) - the box is
 *   what the grid covers (an index outside the grid is clamped into it);  mask = uint8 [src_h][src_w] at the photo's size, or NULL (= 255
 *   everywhere).  Per byte of the box, with m the mask byte of its pixel and c the canvas byte:
 *     q = ce_lift_apply_u8's value, by the same fp32 operations in the same order, each rounded on its own (csrc/ce_lift_pixel.h holds them
 *     for both): p = float(P), top = c00 * (1 - tx) + c01 * tx, bot likewise, v = top * (1 - ty) + bot * ty for abar_c, bbar_c and g;
 *     q = p + (a_up * p + b_up);  with U: q = q + g_up * (float(U) - q);  e = rint(clamp(q, 0, 255)), NaN -> 0;
 *     t = c * (255 - m) + e * m + 128, c = ((t >> 8) + t) >> 8 - ce_focus_paste_u8's arithmetic.
 *   Under m == 0 nothing is computed, read from U or written; U is not read by a run of pixels whose g_up are all 0.  Only bytes of the box
 *   are touched, each by one lane that reads and writes its own addresses.  One lane per run of up to eight pixels of a row: lane 0 of a
 *   row takes the 0..3 pixels in front of the row's first pixel at which the canvas allows dword access, the others eight pixels each
 *   from there; a whole run moves as dwords in every plane (canvas, P, U, mask) that is aligned at it, and byte by byte otherwise - the
 *   same bytes.  A run whose mask bytes are all 0 leaves before a table entry or a cell is loaded.  Any base address, any width.
 *   A box that leaves the image, or F > 65535, returns -1; so do P, U or a mask that share a byte with the canvas.  An image of 2^31 bytes
 *   or more (src_h * src_w * 3, H * W * 32) returns -2; the tables 4-byte, coef 16-byte aligned (otherwise -3).
 * No state, no scratch, nothing allocated, no host read: the call is capturable. */
int ce_boxlift_apply_paste_u8(const void* P, const void* U, const float* coef, const int* ix0, const int* ix1, const float* tx, const int* iy0,
                              const int* iy1, const float* ty, const void* mask, void* canvas, int F, int src_h, int src_w, int left, int top,
                              int bw, int bh, int H, int W, hipStream_t stream);

/* ---- mask-aware detail lift (csrc/ce_rimlift.hip; chronoedit_amd/rimlift.py is the definition and both passes give its bits): stages 1 and
 * 2 of the lift inside a focus box, fitted under the region's weights, so that the apply stage writes the edit at full strength and the
 * paste's mask tapers it once.  L, E, AB, coef, R and radius are ce_lift_fit_q16's / ce_lift_smooth_f32's; M = uint8 [H][W], the edit-size
 * weight plane m, shared by the frames and the colours; box() is the sum over the window [y - r, y + r] x [x - r, x + r] clipped to the image.
 * ce_rimlift_fit_q16: per frame, cell and colour, I = L_c, d = E_c - I; the exact integer sums T_q = box(m m), T_md = box(m d) (int32),
 *   T_qI = box(m m I), T_qII = box(m m I I), T_mId = box(m I d) (int64; all below 2^53) - the normal equations of 255 d ~ a (m I) + b m.
 *   In double, every operation rounded on its own:  num = T_q * T_mId - T_qI * T_md;  den = (T_q * T_qII - T_qI * T_qI) + (T_q * eps_q) * T_q;
 *   where T_q > 0 (den > 0 there: the eps term exceeds the rounding error of the products 2^30 times):
 *   a = fp32(clamp((num * 255) / den, -max_gain, max_gain)),  b = fp32(clamp((T_md * 255 - double(a) * T_qI) / T_q, -4096, 4096));
 *   where T_q == 0: a = b = 0.  AB = int32 [F][H][W][6] = rint(65536 a_rgb), rint(65536 b_rgb).
 * ce_rimlift_smooth_f32: n_m = box(m); abar = fp32(double(box(m A)) / double(65536 n_m)) where n_m > 0, else 0, bbar likewise (int64 sums);
 *   w = fp32(m) / 255;  res = max over colours of |float(d) - (abar * float(I) + bbar) * w| - the residual of the TAPERED model;
 *   coef = fp32 [F][H][W][8] = abar_rgb, bbar_rgb, 0, 0 (16-byte aligned);  R = int32 [F][H][W] = rint(256 min(res, 255)).
 * ce_lift_gate_f32 and ce_boxlift_apply_paste_u8 follow, unchanged: q = p + (a_up * p + b_up) is then the untapered edit.
 * What follows from the arithmetic: M == 0 gives zero cells and R = 256 min(|d|, 255) maximised over the colours; E == L gives a = b = 0.
 * No state, nothing allocated, no host read: every call is capturable.  F <= 65535; radius 1..16, eps_q 1..2^30, max_gain 1..8, sizes > 0 and
 * no NULL pointer (otherwise -1).  A plane of 2^31 bytes or more (H * W * 3) returns -2; AB and R 4-byte, coef 16-byte aligned (otherwise -3). */
int ce_rimlift_fit_q16(const void* L, const void* E, const void* M, int* AB, int F, int H, int W, int radius, int eps_q, float max_gain,
                       hipStream_t stream);
int ce_rimlift_smooth_f32(const void* L, const void* E, const void* M, const int* AB, float* coef, int* R, int F, int H, int W, int radius,
                          hipStream_t stream);

/* ---- tiled edits (csrc/ce_tiles.hip; chronoedit_amd/tiles.py is the definition and the three passes give its bits): one canvas of latents is
 * denoised as overlapping model-size tiles, the samples of one batched pass.  The tiles form a separable grid: nx origins on x, ny on y,
 * tile t = iy * nx + ix (row-major: the batch order) at (ox[ix], oy[iy]).  ox = int [nx], oy = int [ny] are HOST arrays, read by the launcher
 * and passed to the kernel by value; per axis, for tiles of side T on a canvas side C: 1 <= n, o[0] = 0, o[n - 1] + T = C, strictly
 * increasing, o[i + 1] <= o[i] + T (no gap); nx * ny <= 16 - anything else returns -1 before a launch.  A tile's weight at its own
 * coordinates (x, y) is wx * wy with the integer tent w(x) = min(x + 1, T - x): any number of tiles may cover a cell.
 * ce_tiles_fuse_f32: tiles = fp32 [nx * ny][planes][th][tw] -> canvas = fp32 [planes][ch][cw].  Per canvas cell, in double:
 *   acc = sum over the covering tiles in ascending t of double(w_t) * double(x_t), every product and every add rounded on its own (the first
 *   product is taken as it is), one division by double(sum of w_t), one rounding to fp32.  A cell under one tile keeps that tile's value
 *   (w x / w is exact in double; a NaN stays a NaN), and tiles that agree on a cell return it bit for bit (the sum of w_t x is exact too).
 * ce_tiles_scatter_f32: canvas -> tiles, every tile cell takes its canvas cell: a copy (also cuts the noise canvas into the tiles).
 *   Both: one lane per four consecutive cells of a row as one 16-byte access where tw, cw and every ox are multiples of 4 and both bases are
 *   16-byte aligned, one cell per lane otherwise - the same bits.  tiles == canvas or a NULL returns -1; planes * ch * cw or n * planes * th *
 *   tw of 2^31 or more returns -2; a base that is not 4-byte aligned returns -3.
 * ce_tiles_blend_u8: frames = uint8 [nx * ny][F][TH][TW][3] (the decoded tiles, ce_video_to_u8's layout) -> out = uint8 [F][H][W][3], the
 *   top left H x W of the canvas the tiles span (H <= oy[ny - 1] + TH, W <= ox[nx - 1] + TW, origins in pixels).  Per pixel, channel and
 *   frame out = (sum of w_t e_t + Wt / 2) / Wt with Wt = sum of w_t, tents in pixels, integer division, 64-bit sums.  One lane per four
 *   consecutive bytes of a frame, stored as one dword where H * W * 3 is a multiple of 4 and out is 4-byte aligned, byte by byte otherwise:
 *   any base address.  F <= 65535 (otherwise -1); a frame of 2^31 bytes or more returns -2.
 * No atomics, no state, nothing allocated, no device-side read of the host: every call is capturable, every loop bounded by 16. */
int ce_tiles_fuse_f32(const float* tiles, float* canvas, int nx, int ny, const int* ox, const int* oy, int planes, int th, int tw, int ch,
                      int cw, hipStream_t stream);
int ce_tiles_scatter_f32(const float* canvas, float* tiles, int nx, int ny, const int* ox, const int* oy, int planes, int th, int tw, int ch,
                         int cw, hipStream_t stream);
int ce_tiles_blend_u8(const void* frames, void* out, int nx, int ny, const int* ox, const int* oy, int F, int TH, int TW, int H, int W,
                      hipStream_t stream);

/* ---- a RCCL communicator owned by the library (csrc/ce_comm.hip): the exchanges of the sequence-parallel forward as C-ABI calls on the
 * caller's stream.  Replaces the torch.distributed collectives of the reference's sequence-parallel path (xfuser's Ulysses all-to-all behind
 * chronoedit_diffsynth/wan_video_new_chronoedit.py:330-355, the final all_gather :1495-1498) where the caller needs a step with
 * exchanges under hipGraph capture: these calls create no Work objects and nothing polls them.  RCCL is not linked - ce_comm_load()
 * dlopen()s the librccl.so the process already uses (the one torch ships).  All return CE_OK or CE_ERR_ARG (the RCCL error text goes to
 * stderr). */
int ce_comm_load(const char* librccl_path);
/* 128 bytes: ncclGetUniqueId, called by ONE rank; the caller distributes the bytes to the other ranks (any transport). */
int ce_comm_unique_id(void* id128);
/* ncclCommInitRank on the CURRENT device - collective over the `world` ranks that share id128; *comm_out is the handle of the other calls. */
int ce_comm_init(void** comm_out, const void* id128, int rank, int world);
/* ncclCommDestroy + free of the handle.  UNSAFE on the stack this library was validated on (RCCL 2.26.6 inside torch 2.10, next to
 * torch.distributed's own process group): the call blocks for good even on a one-rank communicator (tools/owned_comm_probe.py,
 * profiles/r04_owned_comm_probe.txt), so the Python side never calls it - it keeps ONE communicator per (group, device) for the life of
 * the process instead (parallel.OwnedComm.get).  Exported for hosts whose RCCL tears down cleanly. */
int ce_comm_destroy(void* comm);
/* send / recv: `world` chunks of bytes_per_peer bytes, chunk p to / from rank p (all_to_all_single with equal splits), as one grouped
 * batch of ncclSend / ncclRecv on `stream`.  Buffers must stay valid until the stream has passed the call. */
int ce_comm_all_to_all(void* comm, const void* send, void* recv, size_t bytes_per_peer, hipStream_t stream);
/* recv = every rank's bytes_per_rank-byte block, in rank order (ncclAllGather on `stream`). */
int ce_comm_all_gather(void* comm, const void* send, void* recv, size_t bytes_per_rank, hipStream_t stream);

/* How the loaded library was compiled - a constant, no device is touched: bit 0 = the diagnostic build (libchronoedit_hip_diag.so,
 * include/chronoedit_hip_diag.h), bit 1 = -DF8_A3, bits 4-7 = F8_DMA_SCHED, bits 8-15 = F8_ABLATE (non-zero: a timing-only build of the MX fp8
 * GEMM with one ingredient compiled out; its results are garbage and chronoedit_amd.hiplib.load refuses it).  The product build returns 0x10. */
int ce_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* CHRONOEDIT_HIP_H */

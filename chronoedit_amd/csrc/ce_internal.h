// The library's cross-file helpers: hidden `extern "C"` functions one translation unit defines and another calls.  Declared HERE ONLY and
// included by the defining file and by every caller, so the compiler checks each definition against the one declaration (C linkage: a
// hand-written re-declaration that drifts still links, and the call passes shifted arguments).
#pragma once
#include "ce_common.h"

// ---- bf16 large-tile GEMMs (callers: ce_gemm.hip's dispatcher; the w4 and 384 launchers fall back to ce_gemm256_launch)
// returns 1 when the 256-tile kernels can take the shape
extern "C" int ce_gemm256_supported(int M, int N, int K, int lda, int ldw);
extern "C" int ce_gemm256_launch(const void* A, const void* W, void* C, const float* bias, int epilogue, const float* gate, const void* res, int M,
                                 int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, int res_rows, int a_seg_k, long long a_seg_stride,
                                 int w_seg_k, long long w_seg_stride, float* ws, size_t ws_bytes, hipStream_t stream);  // ce_gemm256.hip
extern "C" int ce_gemm384_launch(const void* A, const void* W, void* C, const float* bias, int epilogue, const float* gate, const void* res, int M,
                                 int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, int res_rows, int a_seg_k, long long a_seg_stride,
                                 int w_seg_k, long long w_seg_stride, float* ws, size_t ws_bytes, hipStream_t stream);  // ce_gemm384.hip
extern "C" int ce_gemm288_launch(const void* A, const void* W, void* C, const float* bias, int epilogue, const float* gate, const void* res, int M,
                                 int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, int res_rows, int a_seg_k, long long a_seg_stride,
                                 int w_seg_k, long long w_seg_stride, float* ws, size_t ws_bytes, hipStream_t stream);
// nsa: 3 = A ring of three K-tile stages (160 KiB of LDS), 2 = two (128 KiB), 1 = three stages and ONE barrier per K-tile
extern "C" int ce_gemm256w4_launch(const void* A, const void* W, void* C, const float* bias, int epilogue, const float* gate, const void* res, int M,
                                   int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows, int res_rows, int a_seg_k, long long a_seg_stride,
                                   int w_seg_k, long long w_seg_stride, int nsa, float* ws, size_t ws_bytes, hipStream_t stream);  // ce_gemm256w4.hip
// A with two nested segment levels (ce_conv.hip); n_tile: 256, 128 or 96
extern "C" int ce_gemm256w4_seg2_launch(const void* A, const void* W, void* C, const float* bias, int epilogue, const void* res, int M, int N, int K,
                                        int lda, int ldw, int ldc, int ldres, int a_seg_k, long long a_seg_stride, int a_seg2_k,
                                        long long a_seg2_stride, int n_tile, hipStream_t stream);
// the split-K reduce of ce_gemm256w4.hip's slab layout for another producer (ce_gemm_fp8w4.hip)
extern "C" int ce_gemm256w4_reduce_launch(int epilogue, void* C, const float* bias, const float* gate, const void* res, int M, int N, int ldc,
                                          int ldres, int gate_rows, int res_rows, int tiles_m, int tiles_n, int t_full, int split, const float* ws,
                                          int tail, hipStream_t stream);
// ---- fp8 GEMM, one wave per SIMD (ce_gemm_fp8w4.hip; caller: ce_gemm_fp8.hip)
extern "C" int ce_gemm_fp8w4_launch(const void* Aq, const void* Wq, void* C, const float* sa, const float* sw, const float* bias, int epilogue,
                                    const float* gate, const void* res, int M, int N, int K, int lda, int ldw, int ldc, int ldres, int gate_rows,
                                    float* ws, size_t ws_bytes, hipStream_t stream);
// ---- the 16 x 16 x 32 body of the plain-layout V^T attention (ce_attn16.hip, linked into the diagnostic library only; caller: ce_attn.hip
// under CE_DIAGNOSTICS.  Declared without the guard because ce_attn16.hip itself is compiled without the define.)
extern "C" int ce_attn16_launch(const void* Q, const void* K, const void* Vt, int len, int ldk, int ldvt, void* O, int Nq, int H, int ldq, int ldo,
                                float sl2, int batch, int cus, hipStream_t stream);
#ifdef CE_DIAGNOSTICS
extern "C" void ce_gemm256_set_staggered(int on);                                  // ce_gemm256.hip; caller: ce_set_gemm_variant
extern "C" int ce_diag_mx_exact_hits(unsigned long long* out, int reset);         // ce_attn_fp8.hip; caller: ce_attn.hip
#endif

/*
 * fairygen_hip_qk8_fused.h — second extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here word for
 * word: return codes, no allocation, no host synchronisation, every launch on `stream`, capturable): the e4m3 operands of
 * fg_attn_fwd_qk8_bf16 (fairygen_hip_qk8.h) written by the RMSNorm+RoPE pass itself.  The recipe is fairygen_hip_qk8.h's, unchanged: on
 * the same inputs these entry points write the q8, sq, k8, sk and key mean that fg_rmsnorm_rope_bf16 followed by fg_attn_quant_qk_bf16
 * writes, byte for byte — the key mean where its fp64 sum is exact (8 significand bits + the exponent spread of the non-zero values +
 * log2 N below 53 bits), which is where the order of a sum cannot show.  The base ABI and fairygen_hip_qk8.h are unchanged by it; it
 * carries a version of its own.  tests/test_attention_qk8_fused.py holds the comparison, the argument, stream and capture checks.
 */
#ifndef FAIRYGEN_HIP_QK8_FUSED_H
#define FAIRYGEN_HIP_QK8_FUSED_H

#include "fairygen_hip_qk8.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_qk8_fused_version(void);     /* version of this extension, currently 1 */

/* Bytes of the key-statistics partials for `rows` keys of C channels: P records per channel (an fp64 sum, a minimum, a maximum: 16
 * bytes), P a function of rows alone.  -1 on rows < 1 or a C that is not a positive multiple of 128 up to 4096. */
int64_t fg_attn_qk8_fused_scratch_bytes(int64_t rows, int C);

/* x (rows, C) bf16 with leading dimension ldx, weight (C), the rope tables and table_f32 as for fg_rmsnorm_rope_bf16, C = num_heads * 128.
 * fg_rmsnorm_rope_q8_bf16: the normed, rotated row never leaves as bf16: q8 (rows, C) e4m3 bytes (8-byte aligned) and sq (rows,
 * num_heads) fp32, one scale per row and head.  One launch.
 * fg_rmsnorm_rope_kstats_bf16: k_out (rows, C) bf16 contiguous — fg_rmsnorm_rope_bf16's bytes — and, to `partials` (16-byte aligned,
 * fg_attn_qk8_fused_scratch_bytes), every workgroup's per-channel sum, minimum and maximum of the rows it walked.  One launch; every
 * record of the buffer is written (a workgroup without a row writes 0, +inf, -inf).
 * fg_attn_quant_k_bf16: k (N, H*128) bf16 with leading dimension ldk and the partials written for these N rows -> kbar (H*128 fp32,
 * 16-byte aligned; the mean), sk (H) and k8 (N, H*128) e4m3 bytes (8-byte aligned).  Two launches: the reduction of the partials
 * (sk from the channel extremes: fp32 rounding is monotone, so max_rows |fl(k - kbar)| = max(fl(kmax - kbar), fl(kbar - kmin))), then
 * the quantise pass. */
int fg_rmsnorm_rope_q8_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                            void* q8, float* sq, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream);
int fg_rmsnorm_rope_kstats_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                                void* k_out, void* partials, int64_t partials_bytes, int64_t rows, int C, int num_heads, float eps,
                                fg_stream_t stream);
int fg_attn_quant_k_bf16(const void* k, int64_t ldk, const void* partials, int64_t partials_bytes, void* k8, float* sk, float* kbar,
                         int64_t N, int H, int D, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

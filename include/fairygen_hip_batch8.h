/*
 * fairygen_hip_batch8.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the whole e4m3 attention chain — the operand
 * producers of fairygen_hip.h and fairygen_hip_pv8.h and the three kernels fg_attn_fwd_qk8_bf16, fg_attn_fwd_pv8_bf16 and
 * fg_attn_fwd_cross8_bf16 — on a batch of B >= 1 elements in ONE stream-ordered launch sequence, the launches of the single-element
 * entry point with one more grid dimension.  The main header, the other extension headers and their versions stay as they are; a host
 * that wants these entry points includes this header, checks fg_attn_batch8_version() and binds them next to the other tables
 * (INTEGRATION.md).  tests/test_attention_batch8.py holds the contract, the argument checks, the stream and capture checks.
 *
 * THE CONTRACT.  For every batch element b, the bytes written for b — operands, scales, attention output — are those the
 * single-element entry point of the same name without `_b` writes when it is called on element b alone.  Every statistic (key mean, sk,
 * sv, sq) is per element and head; nothing is shared between elements.  The device code of an element IS the single-element kernel's:
 * the batched kernels offset their pointers by the element's strides and run the same body.
 *
 * Arguments: those of the single-element entry point, then B (1..65535), with one batch stride behind every batched operand.  A stride
 * counts elements of its operand's type (bf16 for q, k, v, x, out; bytes for the e4m3 operands, scratch and partials; floats for the
 * scales), must cover one element of the operand and keep the operand's alignment for every b.  Each operand of ONE element stays under
 * the 4 GiB span the kernels state.  The two fused producers take x as the B * rows rows of one matrix (leading dimension ldx) and
 * write q8 / sq / k_out as B * rows dense rows; the RoPE table is one element's and indexed by the row inside the element.
 *
 * Split-KV: fg_attn_fwd_qk8_bf16_b and fg_attn_fwd_pv8_bf16_b plan every element as the single-element entry point plans it when it is
 * offered workspace_bytes / B rounded down to 16: element b's partials live in that share.  B * fg_attn_workspace_bytes(1, Nq, Nkv, H)
 * bytes give the plan of the unrestricted single-element call.  The merge launch covers the batch as well.
 */
#ifndef FAIRYGEN_HIP_BATCH8_H
#define FAIRYGEN_HIP_BATCH8_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_batch8_version(void);        /* version of this extension, currently 1 */

/* fg_attn_quant_qk_bf16 per element: q, k (B, N, H*128) bf16 with ld and batch stride -> q8, k8 (B, N, H*128), sq (B, N, H), sk (B, H);
 * scratch: H*128 floats per element (scratch_bytes: ONE element's block, bs_scratch its stride in bytes, a multiple of 16). */
int fg_attn_quant_qk_bf16_b(const void* q, int64_t ldq, int64_t bs_q, const void* k, int64_t ldk, int64_t bs_k, void* q8, int64_t bs_q8,
                            void* k8, int64_t bs_k8, float* sq, int64_t bs_sq, float* sk, int64_t bs_sk, void* scratch,
                            int64_t scratch_bytes, int64_t bs_scratch, int B, int64_t N, int H, int D, fg_stream_t stream);

/* fg_rmsnorm_rope_q8_bf16 on x (B * rows, C): q8 (B * rows, C) and sq (B * rows, H) dense; the table has `rows` rows. */
int fg_rmsnorm_rope_q8_bf16_b(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                              void* q8, float* sq, int B, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream);

/* fg_rmsnorm_rope_kstats_bf16 on x (B * rows, C): k_out (B * rows, C) dense and one partials block per element
 * (fg_attn_qk8_fused_scratch_bytes(rows, C) each; partials_bytes: ONE block, bs_partials its stride in bytes, a multiple of 16). */
int fg_rmsnorm_rope_kstats_bf16_b(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                                  void* k_out, void* partials, int64_t partials_bytes, int64_t bs_partials, int B, int64_t rows, int C,
                                  int num_heads, float eps, fg_stream_t stream);

/* fg_attn_quant_k_bf16 per element: k with ldk and batch stride, the partials blocks above -> k8 (B, N, H*128), sk (B, H), kbar (B, C). */
int fg_attn_quant_k_bf16_b(const void* k, int64_t ldk, int64_t bs_k, const void* partials, int64_t partials_bytes, int64_t bs_partials,
                           void* k8, int64_t bs_k8, float* sk, int64_t bs_sk, float* kbar, int64_t bs_kbar, int B, int64_t N, int H, int D,
                           fg_stream_t stream);

/* fg_attn_quant_vt_bf16 per element: v with ldv and batch stride -> v8t (B, H, 128, Nkp), the padding included, and sv (B, H, 128);
 * scratch: fg_attn_pv8_scratch_bytes(N, H) per element (scratch_bytes: ONE block, bs_scratch its stride in bytes, a multiple of 16). */
int fg_attn_quant_vt_bf16_b(const void* v, int64_t ldv, int64_t bs_v, void* v8t, int64_t bs_v8t, float* sv, int64_t bs_sv, void* scratch,
                            int64_t scratch_bytes, int64_t bs_scratch, int B, int64_t N, int H, int D, fg_stream_t stream);

/* fg_attn_fwd_qk8_bf16 per element -> out (B, Nq, H*128) bf16.  workspace: see "Split-KV" above. */
int fg_attn_fwd_qk8_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq, const float* sk,
                           int64_t bs_sk, const void* v, int64_t ldv, int64_t bs_v, void* out, int64_t bs_out, int B, int64_t Nq,
                           int64_t Nkv, int H, int D, float scale, void* workspace, int64_t workspace_bytes, fg_stream_t stream);

/* fg_attn_fwd_pv8_bf16 per element -> out (B, Nq, H*128) bf16.  workspace: see "Split-KV" above. */
int fg_attn_fwd_pv8_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq, const float* sk,
                           int64_t bs_sk, const void* v8t, int64_t bs_v8t, const float* sv, int64_t bs_sv, void* out, int64_t bs_out,
                           int B, int64_t Nq, int64_t Nkv, int H, int D, float scale, void* workspace, int64_t workspace_bytes,
                           fg_stream_t stream);

/* fg_attn_fwd_cross8_bf16 per element -> out (B, Nq, H*128) bf16: B * H * G workgroups, G = min(ceil(Nq / 256), max(1, CUs / (B * H))),
 * each with one head's K8 and V8^T of ONE element resident in LDS.  A query row's arithmetic does not depend on the workgroup that
 * holds it.  The first call of a process reserves the dynamic LDS of the batched kernel (hipFuncSetAttribute), which a capture may hold. */
int fg_attn_fwd_cross8_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq, const float* sk,
                              int64_t bs_sk, const void* v8t, int64_t bs_v8t, const float* sv, int64_t bs_sv, void* out, int64_t bs_out,
                              int B, int64_t Nq, int64_t Nkv, int H, int D, float scale, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_BATCH8_H */

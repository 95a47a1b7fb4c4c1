/*
 * fairygen_hip_qk8.h — extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here word for word: return
 * codes, no allocation, no host synchronisation, every launch on `stream`, capturable): the opt-in self-attention with an 8-bit Q K^T
 * product.  The base ABI (fg_version, the symbols fairygen_hip.h declares) is unchanged by it; the extension carries a version of its
 * own, so a host that does not use it binds nothing new.  tests/test_attention_qk8.py holds the recipe, the argument checks, the
 * stream and capture checks.
 */
#ifndef FAIRYGEN_HIP_QK8_H
#define FAIRYGEN_HIP_QK8_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_qk8_version(void);           /* version of this extension, currently 1 */

/* The form the reference's flash_attention takes when the sageattention package is present (models/wan_video_dit.py:48-52: sageattn with
 * q, k, v): e4m3 Q K^T with K mean-smoothing, P V in bf16.  One head at a time, q and k (N, 128) after RMSNorm and RoPE:
 *   kbar = mean of k over its N rows (per channel: the fp64 sum, divided by N, rounded once to fp32); k' = fp32(k) - kbar;
 *   sk = max(max|k'| / 448, 2^-20), one per head; k8 = e4m3(k' / sk), round-to-nearest-even, saturating at +-448;
 *   sq[r] = max(max|q[r]| / 448, 2^-20), one per row and head; q8 = e4m3(q / sq[r]);
 *   out = softmax(scale * sq[r] * sk * (q8 k8^T)) v — the product accumulated in fp32 by the plain (unscaled) e4m3 MFMA, the online
 *   softmax, the bf16 P and the bf16 P V of the 8-wave kernel behind fg_attn_fwd_bf16.  q . kbar is constant along a row: dropped.
 * fg_attn_quant_qk_bf16: q, k (N, H*128) bf16 with leading dimensions ldq / ldk -> q8, k8 (N, H*128) e4m3 bytes (8-byte aligned),
 * sq (N, H) and sk (H) fp32.  Two launches on `stream`; scratch: H*128 floats (the column means), 16-byte aligned.  One batch element.
 * fg_attn_fwd_qk8_bf16: q8 (Nq, H*128), k8 (Nkv, H*128), sq (Nq, H), sk (H) as written above (q8, k8 16-byte aligned), v (Nkv, H*128)
 * bf16 with leading dimension ldv, out (Nq, H*128) bf16 contiguous.  workspace: as for fg_attn_fwd_bf16, sized by fg_attn_workspace_bytes
 * with B = 1.  Any Nkv >= 1; cross-attention is not meant to take it. */
int fg_attn_quant_qk_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, void* q8, void* k8, float* sq, float* sk,
                          void* scratch, int64_t scratch_bytes, int64_t N, int H, int D, fg_stream_t stream);
int fg_attn_fwd_qk8_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v, int64_t ldv, void* out,
                         int64_t Nq, int64_t Nkv, int H, int D, float scale, void* workspace, int64_t workspace_bytes,
                         fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

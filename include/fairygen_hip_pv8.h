/*
 * fairygen_hip_pv8.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged): the
 * self-attention with BOTH matrix products on the 8-bit MFMA.  The main header and its version stay as they are; a host that wants
 * these entry points includes this header, checks fg_attn_pv8_version() and binds them next to the main table.
 * tests/test_attention_pv8.py holds the recipe, the argument checks, the stream and capture checks.
 *
 * The reference's flash_attention calls sageattn(q, k, v) when that package is present (models/wan_video_dit.py:48-52); on current
 * parts that is an 8-bit Q K^T and an fp8 P V with fp32 accumulation.  fg_attn_fwd_qk8_bf16 (main header) is the first half; the recipe
 * of the second, per head, with q8, k8, sq, sk and the key mean exactly as there:
 *   sv[c] = max(max over the Nkv keys of |v[j][c]| / 448, 2^-20), one fp32 per head and channel;
 *   v8 = e4m3(v / sv[c]), round-to-nearest-even, saturating at +-448;
 *   p  = the kernel's fp32 probability relative to its running row maximum, which the deferred rescale lets lag by at most T = 3 bits:
 *        p <= 2^3;  P8 = e4m3(c p) with c = 2^5 (c 2^T = 256 <= 448), c folded into the exponent's argument;
 *   row sums: the fp32 sums of the same c p before rounding;  O^T += V8^T P8^T on the plain (unscaled) e4m3 MFMA, fp32 accumulation;
 *   out[r][ch] = acc sv[ch] / (c l): c cancels against the row sum; sv multiplies the accumulators before the split-KV partials too.
 * Layout of v8t: (H, 128, Nkp) bytes, Nkp = Nkv rounded up to a multiple of 64, the padding bytes zero.  Inside each 64-key tile byte
 * p of a channel row holds key 32 ((p >> 4) & 1) + 8 ((p & 15) >> 2) + 4 (p >> 5) + (p & 3) of the tile: the order in which the
 * kernel's S^T accumulators hold the scores of a query row (fairygen_amd.hip.PV8_KEY_ORDER is this table).
 */
#ifndef FAIRYGEN_HIP_PV8_H
#define FAIRYGEN_HIP_PV8_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_pv8_version(void);           /* version of this extension, currently 1 */

/* Bytes of the scratch fg_attn_quant_vt_bf16 wants for N keys of H heads: one fp32 record per channel from each of up to 256 row
 * strides.  -1 on N < 1 or H outside 1..65535. */
int64_t fg_attn_pv8_scratch_bytes(int64_t N, int H);

/* v (N, H*128) bf16 with leading dimension ldv (the column slice of the qkv buffer) -> v8t (H, 128, Nkp) e4m3 bytes and sv (H, 128)
 * fp32, both 16-byte aligned.  Two launches on `stream`: the per-channel maxima of up to 256 row strides to `scratch` (16-byte aligned,
 * fg_attn_pv8_scratch_bytes), then the pass that reduces them (a maximum is order-independent: sv is exact) and writes the transposed
 * bytes, the padding of the last tile included, on every call.  No atomics; one batch element. */
int fg_attn_quant_vt_bf16(const void* v, int64_t ldv, void* v8t, float* sv, void* scratch, int64_t scratch_bytes, int64_t N, int H,
                          int D, fg_stream_t stream);

/* fg_attn_fwd_qk8_bf16 with v8t and sv as written above in place of v: out (Nq, H*128) bf16 contiguous.  q8, k8, v8t, sv, out 16-byte
 * aligned (sq, sk: 4); head_dim 128; K8, one head of V8^T and O must each span < 4 GiB.  workspace: as for fg_attn_fwd_bf16, sized by
 * fg_attn_workspace_bytes with B = 1.  Any Nkv >= 1 (Nkp is derived from it); cross-attention is not meant to take it. */
int fg_attn_fwd_pv8_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v8t, const float* sv, void* out,
                         int64_t Nq, int64_t Nkv, int H, int D, float scale, void* workspace, int64_t workspace_bytes,
                         fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_PV8_H */

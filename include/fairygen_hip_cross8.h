/*
 * fairygen_hip_cross8.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): cross-attention with both matrix products on
 * the 8-bit MFMA and one head's K8 and V8^T resident in LDS.  The main header and its version stay as they are; a host that wants these
 * entry points includes this header, checks fg_attn_cross8_version() and binds them next to the main table.
 * tests/test_attention_cross8.py holds the parity criterion, the argument checks, the stream and capture checks.
 *
 * The reference's flash_attention calls sageattn(q, k, v) for every attention call, cross-attention over the text context included
 * (models/wan_video_dit.py:48-52).  The operands and the recipe are those of fg_attn_fwd_pv8_bf16 (fairygen_hip_pv8.h): q8 / sq and
 * k8 / sk as fg_attn_quant_qk_bf16 or the fused producers write them, v8t (H, 128, Nkp) in the tile order of
 * fairygen_amd.hip.PV8_KEY_ORDER with zero padding and sv as fg_attn_quant_vt_bf16 writes them; T = 3, c = 2^5, 64-key tiles in
 * ascending order, the ragged last tile masked, out = acc sv / l.  At e4m3 a key is 128 B of K8 and 128 B of V8^T per head, so a workgroup
 * loads its head's Nkv keys once — 256 * Nkp bytes of the 160 KiB of LDS it may declare, and nothing besides: Nkv <= 640 — and walks
 * many 256-row query blocks against them: H * G workgroups, G = min(ceil(Nq / 256), max(1, CUs / H)), one barrier each, none between
 * workgroups.  A query row's arithmetic does not depend on the workgroup that holds it: the output is BIT FOR BIT that of
 * fg_attn_fwd_pv8_bf16 called without a workspace on the same operands.
 */
#ifndef FAIRYGEN_HIP_CROSS8_H
#define FAIRYGEN_HIP_CROSS8_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_cross8_version(void);        /* version of this extension, currently 1 */

/* The largest Nkv fg_attn_fwd_cross8_bf16 takes: 640, the keys whose K8 and V8^T tiles fill 160 KiB.  At least 512, a multiple of 64. */
int64_t fg_attn_cross8_max_kv(void);

/* q8 (Nq, H*128) and k8 (Nkv, H*128) e4m3, sq (Nq, H), sk (H), v8t (H, 128, Nkp) e4m3, sv (H, 128) -> out (Nq, H*128) bf16 contiguous.
 * q8, k8, v8t, sv, out 16-byte aligned (sq, sk: 4); head_dim 128; 1 <= Nkv <= fg_attn_cross8_max_kv(); O must span < 4 GiB.  One launch
 * on `stream`, no workspace; the first call of a process reserves the dynamic LDS (hipFuncSetAttribute), which a capture may hold. */
int fg_attn_fwd_cross8_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v8t, const float* sv, void* out,
                            int64_t Nq, int64_t Nkv, int H, int D, float scale, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_CROSS8_H */

/*
 * fairygen_hip_cross8s.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the e4m3 cross-attention of
 * fairygen_hip_cross8.h (one head's K8 and V8^T resident in LDS) with V mean-smoothed, what the reference's sageattn package ships as
 * smooth_v and applies to cross-attention as to self-attention.  The main header and its version stay as they are; a host that wants
 * these entry points includes this header, checks fg_attn_cross8s_version() and binds them next to the main table.
 * tests/test_attention_cross8s.py holds the parity criterion, the argument checks, the stream and capture checks.
 *
 * Why: the text context of the DiT is zeroed behind the prompt's length and the k / v Linears act row by row, so several hundred of its
 * 512 keys carry ONE V row and the key mean of a channel is close to that row.  The unsmoothed recipe takes its row sum before P is
 * rounded to e4m3: it returns that common row multiplied by P's rounding defect, and sv = max|v| / 448 spends the e4m3 range on
 * |pad row| + spread.  Here the operands are those of the smoothing V producer of fairygen_hip_smoothv.h — v8t holds e4m3((v - mu) / sv)
 * in the unchanged layout, mu (H, 128) fp32 the key mean of every head and channel — and an output row is
 *   out[r][ch] = bf16(fl32(fl32(fl32(acc sv[ch]) * fl32(1 / l)) + mu[h][ch])): a product, a sum, ONE rounding to bf16,
 * which is exact in the mean (softmax rows sum to 1).  Everything else is fairygen_hip_cross8.h: Nkv <= 640 (the limit that header's
 * query reports), H * G workgroups (B * H * G batched), one barrier, no workspace; mu is read from global memory in the epilogue, the
 * LDS holds the tiles and nothing besides.  On operands written by the smoothing V producer the output is BIT FOR BIT that of the
 * smoothed self-attention entry point of fairygen_hip_smoothv.h called without a workspace on the same operands — the yardstick
 * fairygen_hip_cross8.h holds its kernel to against the kernel of fairygen_hip_pv8.h.  A V that is the same for all keys comes back
 * bit for bit.  The operands of the two forms do not mix: unsmoothed v8t / sv belong with fairygen_hip_cross8.h.
 */
#ifndef FAIRYGEN_HIP_CROSS8S_H
#define FAIRYGEN_HIP_CROSS8S_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_cross8s_version(void);       /* version of this extension, currently 1 */

/* The single-element entry point of fairygen_hip_cross8.h (its arguments, its checks, its grid) with mu behind sv: q8 (Nq, H*128) and
 * k8 (Nkv, H*128) e4m3, sq (Nq, H), sk (H), v8t (H, 128, Nkp) e4m3, sv (H, 128), mu (H, 128) fp32 -> out (Nq, H*128) bf16 contiguous.
 * q8, k8, v8t, sv, mu, out 16-byte aligned (sq, sk: 4), mu not null; head_dim 128; 1 <= Nkv <= 640; O must span < 4 GiB.  A refused
 * call launches nothing.  One launch on `stream`, no workspace; the first call of a process reserves the dynamic LDS
 * (hipFuncSetAttribute), which a capture may hold. */
int fg_attn_fwd_cross8s_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v8t, const float* sv,
                             const float* mu, void* out, int64_t Nq, int64_t Nkv, int H, int D, float scale, fg_stream_t stream);

/* The batched cross-attention entry point of fairygen_hip_batch8.h (its arguments, its checks, its strides) with mu, bs_mu behind
 * sv, bs_sv; bs_mu in floats, a multiple of 4 and at least H*128.  Workgroup (h * G + g, b) works on element b alone and writes the
 * bytes of the entry point above on that element's operands.  The first call reserves the dynamic LDS as above. */
int fg_attn_fwd_cross8s_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq,
                               const float* sk, int64_t bs_sk, const void* v8t, int64_t bs_v8t, const float* sv, int64_t bs_sv,
                               const float* mu, int64_t bs_mu, void* out, int64_t bs_out, int B, int64_t Nq, int64_t Nkv, int H, int D,
                               float scale, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_CROSS8S_H */

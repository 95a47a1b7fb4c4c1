/*
 * fairygen_hip_smoothv.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged: no
 * allocation, no host synchronisation, stream-ordered launches only): the e4m3 P V self-attention of fairygen_hip_pv8.h with V
 * mean-smoothed, what the reference's sageattn package ships as smooth_v.  The main header and its version stay as they are; a host
 * that wants these entry points includes this header, checks fg_attn_smoothv_version() and binds them next to the main table
 * (INTEGRATION.md).  tests/test_attention_smoothv.py holds the recipe, the argument checks, the stream and capture checks.
 *
 * Why: in the recipe of fairygen_hip_pv8.h the row sum l is taken before P is rounded to e4m3, so sum_j P8_j / (c l) is not 1, and the part
 * of a V channel that all keys share — its mean — comes out multiplied by that defect although softmax . const = const; and
 * sv = max|v| / 448 spends the e4m3 range on |mean| + spread.  The recipe here ("e4m3 P V with smoothed V"), per head h and
 * channel c over the Nkv keys, with q8, k8, sq, sk, P8, c, the row sums, the layout of v8t, the key order inside a tile and the zero
 * padding exactly as in fairygen_hip_pv8.h:
 *   mu[h][c] = fl32((fp64 sum over the keys of v[j][c]) / Nkv).  The sum has a fixed order: with parts = min(ceil(Nkv / 16), 256) row
 *              strides, stride p adds in fp64 (w0 + w1) + (w2 + w3), w_i the sum of the rows 4 p + i + 4 parts n, n = 0, 1, .. in that
 *              order; the total is (the strides 0, 2, 4, .. added in that order) + (the strides 1, 3, 5, .. likewise).  It depends on
 *              Nkv alone, not on a launch grid; where the fp64 sum of the bf16 values is exact (always, short of a channel that spans
 *              more than about 29 binades) it is THE sum;
 *   d[j][c]  = fl32(v[j][c] - mu[h][c]);
 *   sv[h][c] = max(max_j |d[j][c]| / 448, 2^-20), the maximum as max(fl32(vmax - mu), fl32(mu - vmin)): fl32(v - mu) is monotone in v;
 *   v8       = e4m3(d / sv), round-to-nearest-even, saturating at +-448;
 *   out[r][ch] = bf16(fl32(fl32(acc sv[ch]) * fl32(1 / (c l))) + mu[ch]): a product, a sum, ONE rounding to bf16 — with split-KV where the
 *              combined row is rounded (the partials carry no mean).
 * A channel that is the same for all keys therefore comes back bit for bit: mu is that value, v8t is zero, sv the floor.
 */
#ifndef FAIRYGEN_HIP_SMOOTHV_H
#define FAIRYGEN_HIP_SMOOTHV_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_smoothv_version(void);       /* version of this extension, currently 1 */

/* Bytes of the scratch fg_attn_quant_vt_smooth_bf16 wants for N keys of H heads: per channel and row stride (up to 256) an fp64 sum, an
 * fp32 minimum and an fp32 maximum.  -1 on N < 1 or H outside 1..65535. */
int64_t fg_attn_smoothv_scratch_bytes(int64_t N, int H);

/* fg_attn_quant_vt_bf16 (fairygen_hip_pv8.h) in the smoothing form: v (N, H*128) bf16 with leading dimension ldv -> v8t (H, 128, Nkp) e4m3
 * bytes of v - mu, sv (H, 128) and mu (H, 128) fp32, all 16-byte aligned.  Two launches on `stream`, no atomics: the records of the row
 * strides to `scratch` (16-byte aligned, fg_attn_smoothv_scratch_bytes), then the pass that reduces them, writes mu and sv and the
 * transposed bytes, the padding of the last tile included, on every call.  One batch element. */
int fg_attn_quant_vt_smooth_bf16(const void* v, int64_t ldv, void* v8t, float* sv, float* mu, void* scratch, int64_t scratch_bytes,
                                 int64_t N, int H, int D, fg_stream_t stream);

/* The same on B elements in the same two launches, every statistic per element.  Batch strides as in fairygen_hip_batch8.h: bs_v in bf16
 * elements (a multiple of 8), bs_v8t in bytes (of 16), bs_sv and bs_mu in floats (of 4), bs_scratch in bytes (of 16); scratch_bytes is
 * what ONE element has.  Element b writes the bytes of the entry point above on its own operands. */
int fg_attn_quant_vt_smooth_bf16_b(const void* v, int64_t ldv, int64_t bs_v, void* v8t, int64_t bs_v8t, float* sv, int64_t bs_sv, float* mu,
                                   int64_t bs_mu, void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B, int64_t N, int H, int D,
                                   fg_stream_t stream);

/* fg_attn_fwd_pv8_bf16 (fairygen_hip_pv8.h: its arguments, its checks, its workspace) on the v8t, sv and mu written above: mu (H, 128)
 * fp32, 16-byte aligned, is added to every output row in fp32 before the rounding to bf16. */
int fg_attn_fwd_pv8s_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v8t, const float* sv, const float* mu,
                          void* out, int64_t Nq, int64_t Nkv, int H, int D, float scale, void* workspace, int64_t workspace_bytes,
                          fg_stream_t stream);

/* fg_attn_fwd_pv8_bf16_b (fairygen_hip_batch8.h) likewise; bs_mu in floats, a multiple of 4.  Element b computes the bytes of the entry
 * point above on its own operands and a 1/B share of the workspace. */
int fg_attn_fwd_pv8s_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq, const float* sk,
                            int64_t bs_sk, const void* v8t, int64_t bs_v8t, const float* sv, int64_t bs_sv, const float* mu, int64_t bs_mu,
                            void* out, int64_t bs_out, int B, int64_t Nq, int64_t Nkv, int H, int D, float scale, void* workspace,
                            int64_t workspace_bytes, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_SMOOTHV_H */

/*
 * fairygen_hip_shard8s.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the e4m3 operands of the 8-bit
 * self-attention with V mean-smoothed (the recipe of fairygen_hip_smoothv.h) when the N keys are sharded by rows over W ranks and K / V
 * are all-gathered (fairygen_amd.sequence_parallel, attn_mode="allgather").  It is fairygen_hip_shard8.h with a record that carries for V
 * what it carries for K.  The main header and its version stay as they are; a host that wants these entry points includes this header,
 * checks fg_attn_shard8s_version() and binds them next to the main table.  tests/test_attention_shard8s.py holds the
 * property, the argument checks, the stream and capture checks.
 *
 * Each rank reduces its own rows to one RECORD, the W records are all-gathered (W * 32 * C bytes), and every rank reduces them in rank
 * order to the same scales.  For K, with sum, lo, hi the total, the minimum and the maximum over the records, as in fairygen_hip_shard8.h:
 *   kbar = (float)(sum / (double)N),  sk = max(max over the head of max(hi - kbar, kbar - lo) / 448, 2^-20),  k8 = e4m3((k - kbar) / sk);
 * for V the recipe of fairygen_hip_smoothv.h, word for word, per channel c:
 *   mu[c] = fl32((fp64 sum over the ranks, in rank order, of vsum_w[c]) / N),
 *   sv[c] = max(max(fl32(vmax[c] - mu[c]), fl32(mu[c] - vmin[c])) / 448, 2^-20)      fl32(v - mu) is monotone in v,
 *   v8    = e4m3(fl32(v - mu[c]) / sv[c]), round-to-nearest-even, saturating at +-448, ROW-MAJOR;
 * fg_attn_shard8_vt (fairygen_hip_shard8.h) then makes v8t from the gathered bytes, unchanged, and the attention entry point of
 * fairygen_hip_smoothv.h takes v8t, sv and mu.
 *
 * Exactness.  Minima and maxima do not depend on the order.  The unsharded mu has a summation order fixed by Nkv
 * (fairygen_hip_smoothv.h); the sum here has another one: a rank's rows in the order below, then the ranks in rank order.  The two are
 * the same number whenever the fp64 sum of the channel's bf16 values is exact — always, short of a channel that spans more than about 29
 * binades: N values of 8 significant bits whose exponents differ by at most e need e + 8 + ceil(log2 N) <= 53 bits.  Then, for any
 * partition of the rows [0, N) into W contiguous shards, some possibly empty, in any rank order, the gathered v8t and every rank's mu and
 * sv are byte for byte what the smoothing V producer of fairygen_hip_smoothv.h writes on the unsharded rows, and k8, sk and kbar are the
 * bytes of fairygen_hip_shard8.h, i.e. of the unsharded key producers.  The key sum stands under the condition fairygen_hip.h states.
 *
 * Layout of a record of C = H * 128 channels, 32 * C bytes, 16-byte aligned:
 *   bytes [0, 8 C)       C fp64   sum over the rank's rows of k[.][c]
 *   bytes [8 C, 12 C)    C fp32   minimum of k[.][c]
 *   bytes [12 C, 16 C)   C fp32   maximum of k[.][c]
 *   bytes [16 C, 24 C)   C fp64   sum over the rank's rows of v[.][c]
 *   bytes [24 C, 28 C)   C fp32   minimum of v[.][c]
 *   bytes [28 C, 32 C)   C fp32   maximum of v[.][c]
 * (no maximum of |v|: sv comes from the minimum and maximum around the mean).  A rank without rows launches nothing and contributes the
 * neutral record: sums 0, minima +inf, maxima -inf.
 */
#ifndef FAIRYGEN_HIP_SHARD8S_H
#define FAIRYGEN_HIP_SHARD8S_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_shard8s_version(void);       /* version of this extension, currently 1 */

/* Bytes of one record of C channels: 32 * C.  -1 unless C is a multiple of 128 in 128..4096. */
int64_t fg_attn_shard8s_record_bytes(int C);

/* Bytes of the scratch fg_attn_shard8s_stats wants for `rows` rows of v with C channels: per channel and row stride (min(ceil(rows / 16),
 * 256) of them) an fp64 sum, an fp32 minimum and an fp32 maximum, 16 bytes.  -1 on rows < 1 or a C fg_attn_shard8s_record_bytes refuses. */
int64_t fg_attn_shard8s_scratch_bytes(int64_t rows, int C);

/* This rank's record.  partials: what fg_rmsnorm_rope_kstats_bf16 left for this rank's `rows` rows of C = H * 128 channels
 * (fg_attn_qk8_fused_scratch_bytes(rows, C)); v: (rows, C) bf16 with leading dimension ldv, REQUIRED (the record exists for the smoothing
 * form).  One launch walks v once with 16-byte loads and leaves the statistics of parts = min(ceil(rows / 16), 256) row strides in
 * `scratch` (fg_attn_shard8s_scratch_bytes): stride p adds in fp64 (w0 + w1) + (w2 + w3), w_i the sum of the rows 4 p + i + 4 parts n,
 * n = 0, 1, .. in that order.  One launch adds the key partials and the strides in fp64 — thread group g of 8 the records g, g + 8, .. in
 * that order, then group 0 + group 1 + .. + group 7: an order that depends on `rows` alone — joins the extremes and writes `record`
 * (fg_attn_shard8s_record_bytes).  No atomics, nothing waits on another workgroup.  partials, v, record, scratch: 16-byte aligned. */
int fg_attn_shard8s_stats(const void* partials, int64_t partials_bytes, const void* v, int64_t ldv, void* record, int64_t record_bytes,
                          void* scratch, int64_t scratch_bytes, int64_t rows, int H, int D, fg_stream_t stream);

/* records: the W gathered records, (W, 32 * C) contiguous; N: the key count of all ranks.  One launch reduces them — in rank order, the
 * same on every rank — to kbar (C fp32, the key mean), sk (H fp32), sv (C fp32) and mu (C fp32, the key mean of v); one launch converts
 * this rank's rows: k (rows, C) bf16 with ldk -> k8 (rows, C) e4m3; v (rows, C) bf16 with ldv -> v8 (rows, C) e4m3 ROW-MAJOR,
 * e4m3(fl32(v - mu[c]) / sv[c]).  All operands are required.  1 <= rows <= N.  records, k, v, kbar, sv, mu: 16-byte aligned (k8, v8: 8;
 * sk: 4). */
int fg_attn_shard8s_quant(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, const void* v,
                          int64_t ldv, void* k8, void* v8, float* sk, float* kbar, float* sv, float* mu, int64_t rows, int H, int D,
                          fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_SHARD8S_H */

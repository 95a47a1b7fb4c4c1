/*
 * fairygen_hip_shard8.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the e4m3 operands of the 8-bit
 * self-attention (fg_attn_fwd_qk8_bf16, and fg_attn_fwd_pv8_bf16 of fairygen_hip_pv8.h) when the N keys are sharded by rows over W ranks
 * and K / V are all-gathered (fairygen_amd.sequence_parallel, attn_mode="allgather").  The main header and its version stay as they
 * are; a host that wants these entry points includes this header, checks fg_attn_shard8_version() and binds them next to the main table.
 * tests/test_attention_shard8.py holds the property, the argument checks, the stream and capture checks.
 *
 * The key mean, the per-head key scale sk and the per-channel value scale sv are statistics over all N keys.  Each rank reduces its own
 * rows to one RECORD, the W records are all-gathered (W * 20 * C bytes), and every rank reduces them to the same scales:
 *   m = (float)(sum / (double)N),  sk = max(max over the head of max(hi - m, m - lo) / 448, 2^-20),  sv[c] = max(vmax[c] / 448, 2^-20),
 * the expressions of fg_attn_quant_k_bf16 and fg_attn_quant_vt_bf16.  Minima and maxima do not depend on the order; the fp64 sums do not
 * under the exact-sum condition fairygen_hip.h states for the fused producers.  So for any partition of the rows [0, N) into W contiguous
 * shards the gathered k8 and v8t and every rank's sk, key mean and sv are byte for byte what fg_rmsnorm_rope_kstats_bf16 +
 * fg_attn_quant_k_bf16 and fg_attn_quant_vt_bf16 write on the unsharded rows — and the bytes on the wire are the e4m3 bytes.
 *
 * Layout of a record of C = H * 128 channels, 20 * C bytes, 16-byte aligned:
 *   bytes [0, 8 C)      C fp64   sum over the rank's rows of k[.][c]
 *   bytes [8 C, 12 C)   C fp32   minimum of k[.][c]
 *   bytes [12 C, 16 C)  C fp32   maximum of k[.][c]
 *   bytes [16 C, 20 C)  C fp32   maximum of |v[.][c]|  (0 where no v was given)
 * A rank without rows launches nothing and contributes the neutral record: sum 0, minimum +inf, maximum -inf, |v| maximum 0.
 */
#ifndef FAIRYGEN_HIP_SHARD8_H
#define FAIRYGEN_HIP_SHARD8_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_shard8_version(void);        /* version of this extension, currently 1 */

/* Bytes of one record of C channels: 20 * C.  -1 unless C is a multiple of 128 in 128..4096. */
int64_t fg_attn_shard8_record_bytes(int C);

/* Bytes of the scratch fg_attn_shard8_stats wants for `rows` rows of v with C channels: one fp32 per channel from each of up to 256 row
 * strides.  -1 on rows < 1 or a C fg_attn_shard8_record_bytes refuses. */
int64_t fg_attn_shard8_scratch_bytes(int64_t rows, int C);

/* This rank's record.  partials: what fg_rmsnorm_rope_kstats_bf16 left for this rank's `rows` rows of C = H * 128 channels
 * (fg_attn_qk8_fused_scratch_bytes(rows, C)); v: (rows, C) bf16 with leading dimension ldv, or NULL (then scratch may be NULL too).
 * With v one launch leaves the |v| maxima of up to 256 row strides in `scratch` (fg_attn_shard8_scratch_bytes); one launch adds the
 * partial sums in fp64, joins the extremes and writes `record` (fg_attn_shard8_record_bytes).  partials, v, record, scratch: 16-byte
 * aligned. */
int fg_attn_shard8_stats(const void* partials, int64_t partials_bytes, const void* v, int64_t ldv, void* record, int64_t record_bytes,
                         void* scratch, int64_t scratch_bytes, int64_t rows, int H, int D, fg_stream_t stream);

/* records: the W gathered records, (W, 20 * C) contiguous; N: the key count of all ranks.  One launch reduces them — in the same order
 * on every rank — to kbar (C fp32, the key mean), sk (H fp32) and, with v, sv (C fp32); one launch converts this rank's rows:
 * k (rows, C) bf16 with ldk -> k8 (rows, C) e4m3 as fg_attn_quant_k_bf16 writes them; v (rows, C) bf16 with ldv, or NULL (then v8 and sv
 * may be NULL) -> v8 (rows, C) e4m3 ROW-MAJOR, e4m3(v / sv[c]).  1 <= rows <= N.  records, k, v, kbar, sv: 16-byte aligned (k8, v8: 8;
 * sk: 4). */
int fg_attn_shard8_quant(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, const void* v,
                         int64_t ldv, void* k8, void* v8, float* sk, float* kbar, float* sv, int64_t rows, int H, int D,
                         fg_stream_t stream);

/* The gathered v8 (N, H * 128) row-major e4m3 bytes -> v8t (H, 128, Nkp), Nkp = N rounded up to a multiple of 64, in the tile order of
 * fg_attn_quant_vt_bf16 (fairygen_amd.hip.PV8_KEY_ORDER); the padding of the last tile is written as zero on every call.  A pass of its
 * own because a rank's row count is no multiple of 64: tiles straddle ranks.  v8, v8t: 16-byte aligned. */
int fg_attn_shard8_vt(const void* v8, void* v8t, int64_t N, int H, int D, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_SHARD8_H */

/*
 * fairygen_hip_shard8b.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the producers of fairygen_hip_shard8.h and
 * fairygen_hip_shard8s.h on a BATCH of B elements that share the row count — the stacked CFG forward (both branches in one pass) on a
 * rank of the K / V all-gather layout.  The main header and its version stay as they are; a host that wants these entry points includes
 * this header, checks fg_attn_shard8b_version() and binds them next to the main table.
 * tests/test_attention_shard8b.py holds the property, the argument checks, the stream and capture checks.
 *
 * Every entry point is its single-element form with a batch: one launch sequence per batch, the element in the grid, every statistic per
 * element and head, and per element the bytes the single-element entry point writes on that element alone.  The recipes, the record
 * layouts and the exactness statement are those of the two headers above, word for word.
 *
 * Layouts.
 *   records of a rank      (B, 20 * C) or (B, 32 * C) bytes, contiguous: element b's record at b * record bytes
 *   gathered records       (W, B, record bytes) contiguous: rank w's record of element b at (w * B + b) * record bytes
 *   kbar, sv, mu           (B, C) fp32;  sk (B, H) fp32
 *   k8, v8                 (B, rows, C) e4m3 contiguous, v8 ROW-MAJOR
 *   v8t                    (B, H, 128, Nkp) e4m3 contiguous, Nkp = N rounded up to 64
 * Inputs take an element stride behind their leading dimension: bs_k, bs_v in elements (bf16), bs_partials, bs_scratch, bs_v8 in bytes.
 * A rank without rows launches nothing and contributes B neutral records.  1 <= B <= 65535.
 */
#ifndef FAIRYGEN_HIP_SHARD8B_H
#define FAIRYGEN_HIP_SHARD8B_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_attn_shard8b_version(void);       /* version of this extension, currently 1 */

/* The stats entry point of fairygen_hip_shard8.h on B elements.  partials: what the batched key-statistics pass of fairygen_hip_batch8.h
 * left, element b's block (partials_bytes of it, at least the key producer's scratch bytes for (rows, C)) at b * bs_partials; v: element b's (rows, C) bf16 rows with leading dimension ldv at
 * b * bs_v, or NULL (the |v| maxima are then written as 0 and scratch is not used); records: (B, 20 * C), records_bytes in all; scratch:
 * element b's scratch, the single form's scratch bytes for (rows, C) (scratch_bytes of them), at b * bs_scratch.  Two launches for the batch (one
 * without v).  partials, v, records, scratch: 16-byte aligned; bs_partials, bs_scratch multiples of 16, bs_v a multiple of 8. */
int fg_attn_shard8_stats_b(const void* partials, int64_t partials_bytes, int64_t bs_partials, const void* v, int64_t ldv, int64_t bs_v,
                           void* records, int64_t records_bytes, void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B,
                           int64_t rows, int H, int D, fg_stream_t stream);

/* The quant entry point of fairygen_hip_shard8.h on B elements.  records: the gathered (W, B, 20 * C); N: the key count of all ranks, per element.  One launch
 * reduces them per element — in rank order — to kbar (B, C), sk (B, H) and, with v, sv (B, C); one launch converts this rank's rows of
 * every element: k (rows, C) bf16 with ldk at b * bs_k -> k8 (B, rows, C); v likewise -> v8 (B, rows, C) ROW-MAJOR.  v, v8, sv: all
 * three or none.  1 <= rows <= N.  Alignment as the single form's; bs_k, bs_v multiples of 8. */
int fg_attn_shard8_quant_b(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, int64_t bs_k,
                           const void* v, int64_t ldv, int64_t bs_v, void* k8, void* v8, float* sk, float* kbar, float* sv, int B,
                           int64_t rows, int H, int D, fg_stream_t stream);

/* The vt entry point of fairygen_hip_shard8.h on B elements: the gathered v8 of element b, (N, C) e4m3 row-major, at b * bs_v8 bytes -> v8t (B, H, 128, Nkp) in
 * the tile order of PV8_KEY_ORDER, padding zero.  bs_v8 >= N * C, a multiple of 16: a gathered buffer whose elements lie W * chunk rows
 * apart is read where it is, no compaction copy when W * chunk != N.  v8, v8t: 16-byte aligned. */
int fg_attn_shard8_vt_b(const void* v8, int64_t bs_v8, void* v8t, int B, int64_t N, int H, int D, fg_stream_t stream);

/* The stats entry point of fairygen_hip_shard8s.h on B elements: fg_attn_shard8_stats_b with v REQUIRED, records (B, 32 * C) and element
 * b's scratch, that single form's scratch bytes for (rows, C), at b * bs_scratch. */
int fg_attn_shard8s_stats_b(const void* partials, int64_t partials_bytes, int64_t bs_partials, const void* v, int64_t ldv, int64_t bs_v,
                            void* records, int64_t records_bytes, void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B,
                            int64_t rows, int H, int D, fg_stream_t stream);

/* The quant entry point of fairygen_hip_shard8s.h on B elements: fg_attn_shard8_quant_b on the gathered (W, B, 32 * C) records, all operands required, mu (B, C)
 * behind sv; v8 = e4m3(fl32(v - mu[b][c]) / sv[b][c]). */
int fg_attn_shard8s_quant_b(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, int64_t bs_k,
                            const void* v, int64_t ldv, int64_t bs_v, void* k8, void* v8, float* sk, float* kbar, float* sv, float* mu,
                            int B, int64_t rows, int H, int D, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_SHARD8B_H */

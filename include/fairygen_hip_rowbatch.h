/*
 * fairygen_hip_rowbatch.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the DiT row kernels that read a per-row
 * table — the AdaLN modulation rows, the RoPE table — on a batch of B >= 1 elements that SHARE that table, in ONE launch: the launch of
 * the single-element entry point with one more grid dimension.  The main header, the other extension headers and their versions stay
 * as they are; a host that wants these entry points includes this header, checks fg_dit_rowbatch_version() and binds them next to the
 * other tables.  tests/test_row_kernels_batched.py holds the contract, the argument checks, the stream and capture checks.
 *
 * What a batch is here: the forwards of one denoise step that differ only in their text context (the CFG pair) stacked on dim 0.  Their
 * token rows differ, their time rows and their grid do not, so the modulation table and the RoPE table are ONE element's.
 *
 * THE CONTRACT, that of fairygen_hip_batch8.h.  For every batch element b, the bytes written for b are those the entry point of the same
 * name without `_b` writes when it is called on element b alone (its `rows` rows of x / y / out, the same tables).  The device code of an
 * element IS the single-element kernel's: the batched kernels offset their pointers by the element and run the same body; no workgroup
 * holds rows of two elements.
 *
 * Arguments: those of the single-element entry point with B (1..65535) in front of rows.  `rows`, `mod_rows` (1, 2 or rows) and
 * `first_rows` (0..rows) count INSIDE one element.  x, y and every output are the B * rows dense rows of one matrix (C wide);
 * fg_rmsnorm_rope_bf16_b keeps ldx for its input, as the fused producers of fairygen_hip_batch8.h do, and writes B * rows dense rows.
 * The tables have the rows of ONE element (mod_rows rows of mod_ld; `rows` rows of RoPE) and are indexed by the row inside the element.
 *
 * The row kernels that read no per-row table — fg_ln_affine_bf16, fg_rmsnorm_rope_bf16 with NULL tables — take the B * rows rows as
 * they are and have no form here; nor have the grouped RoPE form and fg_lora_apply_bf16's gate.  The fp8-output norms have theirs in
 * fairygen_hip_rowbatch8.h.
 */
#ifndef FAIRYGEN_HIP_ROWBATCH_H
#define FAIRYGEN_HIP_ROWBATCH_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_dit_rowbatch_version(void);       /* version of this extension, currently 1 */

/* fg_ln_modulate_bf16 per element: out[b] = modulate(LN(x[b])) with the table rows of the row inside the element. */
int fg_ln_modulate_bf16_b(const void* x, const void* shift, const void* scale, void* out, int B, int64_t rows, int C, float eps,
                          int64_t mod_rows, int64_t first_rows, int64_t mod_ld, fg_stream_t stream);

/* fg_gate_residual_bf16 per element: out[b] = x[b] + gate * y[b] (gate NULL: x + y; mod_rows / first_rows are then not read). */
int fg_gate_residual_bf16_b(const void* x, const void* y, const void* gate, void* out, int B, int64_t rows, int C, int64_t mod_rows,
                            int64_t first_rows, int64_t mod_ld, fg_stream_t stream);

/* fg_residual_ln_bf16 per element: x_out[b] = x[b] + gate * y[b], norm_out[b] = its norm; mode 0: p0 / p1 = shift / scale vectors of
 * the table, mode 1: p0 / p1 = weight / bias (C values, no table row). */
int fg_residual_ln_bf16_b(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1, void* norm_out,
                          int mode, int B, int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                          fg_stream_t stream);

/* fg_rmsnorm_rope_bf16 on x (B * rows, C) with leading dimension ldx -> out (B * rows, C) dense; the table (fp32 interleaved in cos_tab,
 * the fp64 pair, or none) has `rows` rows. */
int fg_rmsnorm_rope_bf16_b(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                           void* out, int B, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_ROWBATCH_H */

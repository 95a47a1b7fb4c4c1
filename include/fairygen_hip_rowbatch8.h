/*
 * fairygen_hip_rowbatch8.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the DiT norms that read the AdaLN modulation
 * table by row number AND hand their row to an fp8 Linear — as e4m3 bytes and one fp32 scale per row, no bf16 row — on a batch of B >= 1
 * elements that SHARE that table, in ONE launch.  It is to fg_ln_modulate_fp8_bf16 / fg_residual_ln_fp8_bf16 what
 * fairygen_hip_rowbatch.h is to the bf16-output norms.  The main header, the other extension headers and their versions stay as they
 * are; a host that wants these entry points includes this header, checks fg_dit_rowbatch8_version() and binds them next to the other
 * tables.  tests/test_row_kernels_batched_fp8.py holds the contract, the argument checks, the stream and capture checks.
 *
 * What a batch is here: that of fairygen_hip_rowbatch.h — the forwards of one denoise step that differ only in their text context (the
 * CFG pair) stacked on dim 0; the modulation table is ONE element's.
 *
 * THE CONTRACT, that of fairygen_hip_rowbatch.h.  For every batch element b, the bytes written for b — the e4m3 rows, the row scales,
 * x_out — are those the entry point of the same name without `_b` writes when it is called on element b alone (its `rows` rows, the same
 * table).  The device code of an element IS the single-element kernel's body: the batched kernels offset their pointers by the element
 * and run it; no workgroup holds rows of two elements.
 *
 * Arguments: those of the single-element entry point with B (1..65535) in front of rows.  `rows`, `mod_rows` (1, 2 or rows) and
 * `first_rows` (0..rows) count INSIDE one element.  x, y, x_out and the e4m3 output are the B * rows dense rows of one matrix (C wide),
 * the scales B * rows floats.  The table has the rows of ONE element (mod_rows rows of mod_ld) and is indexed by the row inside the
 * element.  The checks are the single-element entry point's on one element, then B.
 *
 * The two-output norms (fg_ln_modulate_dual_bf16, fg_ln_affine_dual_bf16) have no form here: they serve unfused hot-loaded adapters only.
 */
#ifndef FAIRYGEN_HIP_ROWBATCH8_H
#define FAIRYGEN_HIP_ROWBATCH8_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_dit_rowbatch8_version(void);      /* version of this extension, currently 1 */

/* fg_ln_modulate_fp8_bf16 per element: (out_fp8[b], out_scale[b]) = the row-quantised modulate(LN(x[b])) with the table rows of the
 * row inside the element. */
int fg_ln_modulate_fp8_bf16_b(const void* x, const void* shift, const void* scale, void* out_fp8, float* out_scale,
                              int B, int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                              float fp8_max, fg_stream_t stream);

/* fg_residual_ln_fp8_bf16 per element: x_out[b] = x[b] + gate * y[b] (gate NULL: x + y), (norm_fp8[b], norm_scale[b]) = its row-quantised
 * norm; mode 0: p0 / p1 = shift / scale vectors of the table, mode 1: p0 / p1 = weight / bias (C values, no table row).  x_out may be x. */
int fg_residual_ln_fp8_bf16_b(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1,
                              void* norm_fp8, float* norm_scale, int mode, int B, int64_t rows, int C, float eps,
                              int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_ROWBATCH8_H */

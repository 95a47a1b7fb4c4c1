/*
 * fairygen_hip_lorabatch.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): what unfused hot-loaded LoRA adapters need
 * on a batch of B >= 1 elements that SHARE their gate / modulation table, in ONE launch — the adapter kernel, whose gated mode reads its
 * gate row by row number, and the two-output modulate norm that hands an fp8 Linear its e4m3 row AND the adapter its bf16 row.  It is
 * to fg_lora_apply_bf16 / fg_ln_modulate_dual_bf16 what fairygen_hip_rowbatch.h is to the bf16-output norms.  The main header, the
 * other extension headers and their versions stay as they are; a host that wants these entry points includes this header, checks
 * fg_dit_lorabatch_version() and binds them next to the other tables.  tests/test_lora_apply_batched.py holds the
 * contract, the argument checks and the capture checks.
 *
 * What a batch is here: that of fairygen_hip_rowbatch.h — the forwards of one denoise step that differ only in their text context (the
 * CFG pair) stacked on dim 0; the tables, and the adapter's A and B, are ONE element's.
 *
 * THE CONTRACT, that of fairygen_hip_rowbatch.h.  For every batch element b, the bytes written for b are those the entry point of the
 * same name without `_b` writes when it is called on element b alone (its rows, the same table, the same A and B).  The device code of
 * an element IS the single-element kernel's body: the batched kernels offset their pointers by the element (a 64-bit offset) and run it;
 * the second grid dimension is the element, so no workgroup holds rows of two elements.
 *
 * The two-output affine norm (fg_ln_affine_dual_bf16) reads no table by row number, so it needs no form here: a host calls it on all
 * B * rows rows.
 */
#ifndef FAIRYGEN_HIP_LORABATCH_H
#define FAIRYGEN_HIP_LORABATCH_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_dit_lorabatch_version(void);      /* version of this extension, currently 1 */

/* fg_lora_apply_bf16 per element.  Arguments: its own with B (1..65535) in front of M; M is the rows of ONE element, and first_rows
 * and the gate table's row rule (mode 2, gate_rows == 2: rows below first_rows read row 0, the others row 1) count INSIDE the element.
 * x and out are the B * M rows of one matrix each, with the leading dimensions ldx and ldc: element b starts at row b * M.  So each of
 * x and out must have ONE fixed row stride across the elements — a contiguous (B, M, .) tensor fits, and so does a column slice of one;
 * elements at any other distance do not.  a, b and the gate table are one element's, shared by all.  The checks are
 * fg_lora_apply_bf16's on one element, then B and B * M < 2^31.  No further span check is needed for the batch: the kernel adds the
 * element's offset (b * M * ldx, b * M * ldc) to the pointers in 64 bits, and behind it the rows are addressed as in the
 * single-element kernel (64-bit row * leading dimension), so the single-element 31-bit tile-span checks cover every element. */
int fg_lora_apply_bf16_b(const void* x, int64_t ldx, const void* a, const void* b, void* out, int64_t ldc, int B, int64_t M, int64_t K,
                         int64_t Ng, int64_t R, int64_t G, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                         int64_t first_rows, fg_stream_t stream);

/* fg_ln_modulate_dual_bf16 per element: (out[b], out_fp8[b], out_scale[b]) = its three outputs on x[b] with the table rows of the row
 * inside the element.  Arguments: its own with B (1..65535) in front of rows; rows, mod_rows (1, 2 or rows) and first_rows (0..rows)
 * count inside one element.  x, out and out_fp8 are the B * rows dense rows of one matrix (C wide), out_scale B * rows floats. */
int fg_ln_modulate_dual_bf16_b(const void* x, const void* shift, const void* scale, void* out, void* out_fp8, float* out_scale,
                               int B, int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                               float fp8_max, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_LORABATCH_H */

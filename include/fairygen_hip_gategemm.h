/*
 * fairygen_hip_gategemm.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation): the persistent GEMM's gated residual store
 * (mode 2, c = bf16(c + bf16(gate[row] * bf16(acc + bias)))) on a BATCH of elements that share a two-row gate table, in ONE launch.
 * fg_gemm_epilogue_bf16_s / fg_gemm_fp8_bf16_s pick the gate row of an output row by `row >= first_rows` over the rows of the launch,
 * so a host that stacks B elements of P rows each (the CFG pair of one denoise step, clips of a batch) had to launch them once per
 * element.  The two entry points here take the period P and count the rule inside the element:
 *
 *     output row r reads gate row 0 iff (r mod rows_per_element) < first_rows, else gate row 1.
 *
 * The main header, the other extension headers and their versions stay as they are; a host that wants these entry points includes
 * this header, checks fg_gemm_gate_period_version() and binds them next to the other tables.
 * tests/test_gemm_periodic_gate.py holds the contract and the argument checks.
 *
 * They are a second instantiation of the same generated kernel (csrc/gen_gemm_p.py --gate-period) and of its reduce kernel: same tiles,
 * same unit plan for a shape, same k order, same rounding points.  All three store paths follow the rule (whole 256 x 256 tiles, the
 * k-range pieces added up by the reduce kernel, the 64-column pieces).  The kernels of the entry points without the period are what
 * they were, instruction for instruction (profiles/gategemm_isa_diff.log).
 */
#ifndef FAIRYGEN_HIP_GATEGEMM_H
#define FAIRYGEN_HIP_GATEGEMM_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_gemm_gate_period_version(void);      /* version of this extension, currently 1 */

/* fg_gemm_epilogue_bf16_s with the gate rule counted inside an element.  Arguments: its own, with rows_per_element behind first_rows.
 * mode must be 2 and gate_rows 2: every other mode has no row rule and stays on fg_gemm_epilogue_bf16_s (FG_EINVAL here).
 * rows_per_element > 0; M need not be a multiple of it (the last element is then short).  first_rows counts inside the element:
 * below 0 it is 0, above rows_per_element it is rows_per_element (every row on gate row 0).
 * rows_per_element must be at least 256, the height of a tile, so that a tile meets at most one element boundary — or at least M,
 * where there is no boundary at all; anything else is FG_EINVAL.  With rows_per_element >= M the bytes written are those of
 * fg_gemm_epilogue_bf16_s with the same first_rows.  a, c and scale_a are the M rows of the whole batch (element b starts at row
 * b * rows_per_element), w, bias and the gate table are shared.  workspace, sched, workgroups and every other check: as
 * fg_gemm_epilogue_bf16_s; fg_gemm_workspace_bytes and fg_gemm_sched_bytes give the sizes, for M rows. */
int fg_gemm_epilogue_bf16_sp(const void* a, int64_t lda, const void* w, const void* bias, void* c, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                             int64_t first_rows, int64_t rows_per_element, void* workspace, void* sched, int workgroups,
                             fg_stream_t stream);

/* ... and fg_gemm_fp8_bf16_s likewise (e4m3 operands, scale_a one fp32 value per row of the batch). */
int fg_gemm_fp8_bf16_sp(const void* a_fp8, int64_t lda, const float* scale_a, const void* w_fp8, const void* bias, void* c, int64_t ldc,
                        int64_t M, int64_t N, int64_t K, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                        int64_t first_rows, int64_t rows_per_element, void* workspace, void* sched, int workgroups,
                        fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_GATEGEMM_H */

/*
 * fairygen_hip.h — C ABI of libfairygen_hip.so, the MI355X (gfx950) kernels behind FairyGen's animation
 * hot path (diffsynth WanVideoPipeline -> Wan2.2-TI2V-5B denoise loop -> Wan2.2 VAE decode).
 *
 * The reference is pure Python/PyTorch and has no FFI; each entry point below replaces the ATen op
 * sequence of one reference call site (cited per function, paths relative to
 * /root/reference/animation/).  A host binds them with ctypes:
 * tensor.data_ptr() for buffers, torch.cuda.current_stream().cuda_stream for `stream`.
 *
 * Contract (all functions):
 *   - return 0 on success, a negative FG_E* code on error; fg_last_error() gives a thread-local message;
 *   - no allocation, no ownership transfer, no host synchronisation: the caller passes every buffer,
 *     work is enqueued asynchronously on `stream` (a hipStream_t; NULL = the default stream);
 *   - re-entrant across streams and devices, no mutable global state;
 *     every launch of an entry point (its second kernel included: the attention combine, the GEMM's reduce) goes to `stream`, the
 *     first call of a process included, so a call may be recorded by a stream capture (tests/test_stream_contract.py: every entry point
 *     captured on a side stream and replayed, ordered behind a producer on a side stream, and as the first launch of a process;
 *     fg_cfg_euler_dev_bf16, the entry point of ABI 8: tests/test_graph_step.py);
 *   - the documented exception to the two points above: fg_gemm_epilogue_bf16 and fg_gemm_fp8_bf16 keep the scheduler block of their
 *     kernel inside the library, per (device, stream) — allocation and a device-wide synchronisation on the first call on a stream, a
 *     lock on every call, not capturable into a graph before that first call.  fg_gemm_epilogue_bf16_s / fg_gemm_fp8_bf16_s are the
 *     same launches on a block the caller owns and keep the contract;
 *   - all tensors are contiguous row-major device buffers unless a leading dimension (`ld*`, in
 *     ELEMENTS) is given; bf16 = IEEE bfloat16 bits; pointers must be 16-byte aligned and the channel
 *     counts multiples of 8 (checked, FG_EINVAL).  Where a function names a weaker alignment, that one is what it checks: 8 bytes for
 *     the fp8 outputs, bias / gate of the GEMMs and bias / residual / out of fg_conv3d_cl_bf16; 4 bytes for scale_a.  The fp32 scale
 *     outputs (out_scale, norm_scale, scale) are written one float at a time and no alignment is checked for them.  The kernels that
 *     access single elements take any element-aligned pointer and check NO alignment (a misaligned pointer is not rejected):
 *     fg_cfg_euler_bf16, fg_cfg_euler_dev_bf16 (vector accesses when every pointer is 16-byte aligned), fg_softmax_rows_f32_bf16, fg_softmax_bias_bf16, fg_conv_pack_weight_bf16, fg_vae_latent_to_cl_bf16,
 *     fg_vae_latent_from_cl_bf16, fg_vae_unpatchify_bf16, fg_vae_patchify_bf16, fg_avgdown3d_add_bf16, fg_video_to_uint8,
 *     fg_vae_tile_accumulate_bf16, fg_vae_tile_finalize_bf16 (tests/test_buffer_contract.py);
 *   - token tensors are "b s (n d)" exactly like the reference's AttentionModule
 *     (models/wan_video_dit.py:113-120); VAE activations are channels-last (T,H,W,C) inside the
 *     decoder, NCTHW only at fg_vae_* boundary kernels;
 *   - the DiT token kernels compute every row independently of the other rows of the call: a call on the rows [lo, hi) with row-sliced
 *     operands, the same tables and first_rows' = clamp(first_rows - lo, 0, hi - lo) (0 and rows included) writes the bits the full
 *     call writes to those rows — what token sharding rests on (tests/test_token_shard_invariance.py).  The exceptions: the k-split
 *     pieces of the GEMMs (with a workspace the plan depends on M), the split-KV of fg_attn_fwd_bf16 (with a workspace the plan
 *     depends on Nq), and the 4-wave attention kernel's deferred rescale, decided per wave: once a row maximum moves by more than
 *     2^6 between KV tiles a query row's bits may depend on the rows that share its wave.
 */
#ifndef FAIRYGEN_HIP_H
#define FAIRYGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_OK        0
#define FG_EINVAL   (-1)   /* bad shape / alignment / unsupported size */
#define FG_ELAUNCH  (-2)   /* hipLaunch failed (message has the HIP error string) */

typedef void* fg_stream_t;   /* hipStream_t */

int         fg_version(void);            /* ABI version, currently 8 */
const char* fg_last_error(void);         /* thread-local, valid until the next failing call */

/* ------------------------------------------------------------------ DiT token-side kernels (HBM-bound)
 * "Modulation rows": AdaLN shift/scale/gate vectors live in a small (mod_rows, *, C) table; row r of a
 * vector starts at ptr + r*mod_ld elements.  mod_rows==1: one row for all tokens (T2V mode);
 * mod_rows==2: tokens [0,first_rows) use row 0 and the rest row 1 (TI2V mode: first latent frame is at
 * t=0, pipelines/wan_video.py:1218-1228); mod_rows==rows: one row per token (the reference's literal
 * (1,N,6,C) layout).  mod_rows == 2 ALWAYS means the split, also when rows == 2: a call on two token rows with a two-row table
 * and first_rows == 0 reads table row 1 for both (a TI2V token shard behind the first latent frame).  A per-token table of two
 * rows is the split with first_rows == 1, and a caller has to pass it so (fairygen_amd.hip.ModTable(per_token=True) does);
 * first_rows in [0, rows], 0 and rows included.  Pinned by tests/test_row_kernel_shapes.py. */

/* out = bf16(bf16(bf16(LN(x)) * bf16(1+scale)) + shift): nn.LayerNorm(elementwise_affine=False) followed by
 * modulate(), models/wan_video_dit.py:63-64,205-206,224,227 and Head.forward :261-268. */
int fg_ln_modulate_bf16(const void* x, const void* shift, const void* scale, void* out,
                        int64_t rows, int C, float eps,
                        int64_t mod_rows, int64_t first_rows, int64_t mod_ld, fg_stream_t stream);

/* out = LN(x)*w + b (norm3, models/wan_video_dit.py:207,226). */
int fg_ln_affine_bf16(const void* x, const void* w, const void* b, void* out,
                      int64_t rows, int C, float eps, fg_stream_t stream);

/* out = x + gate*y (GateModule, models/wan_video_dit.py:188-193,225,228) or x + y when gate==NULL (:226).
 * out may alias x. */
int fg_gate_residual_bf16(const void* x, const void* y, const void* gate, void* out,
                          int64_t rows, int C,
                          int64_t mod_rows, int64_t first_rows, int64_t mod_ld, fg_stream_t stream);

/* Fused residual + next norm: x_out = x + gate*y (gate may be NULL); then
 *   mode 0: norm_out = LN(x_out) modulated by (shift, scale) as fg_ln_modulate_bf16,
 *   mode 1: norm_out = LN(x_out)*w + b (p0 = w, p1 = b; mod_* ignored for the norm).
 * One pass over HBM instead of two (models/wan_video_dit.py:225-227, and :228 -> next block's :224).
 * x_out may alias x. */
int fg_residual_ln_bf16(const void* x, const void* y, const void* gate, void* x_out,
                        const void* p0, const void* p1, void* norm_out, int mode,
                        int64_t rows, int C, float eps,
                        int64_t mod_rows, int64_t first_rows, int64_t mod_ld, fg_stream_t stream);

/* fg_ln_modulate_bf16 / fg_residual_ln_bf16 for a norm whose ONLY consumer is an fp8 Linear (the fp8 mode of the DiT blocks:
 * AutoWrappedLinear.fp8_linear, core/vram/layers.py:331-342, after models/wan_video_dit.py:224-228): instead of the bf16 row, the
 * normalised row leaves as e4m3 bytes out_fp8 / norm_fp8 (rows, C) and one fp32 scale per row — bit for bit what
 * fg_fp8_quant_rows_bf16 (act 0) makes of the bf16 row, without writing and re-reading it.  fp8_max: 448 for e4m3fn. */
int fg_ln_modulate_fp8_bf16(const void* x, const void* shift, const void* scale, void* out_fp8, float* out_scale,
                            int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                            float fp8_max, fg_stream_t stream);
int fg_residual_ln_fp8_bf16(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1,
                            void* norm_fp8, float* norm_scale, int mode, int64_t rows, int C, float eps,
                            int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max, fg_stream_t stream);

/* The norms of a DiT block in the fp8 Linear mode when hot-loaded LoRA adapters are attached (AutoWrappedLinear.forward,
 * core/vram/layers.py:429-436: fp8_linear(x) for the base product, then lora_forward on the SAME bf16 x): the normalised row has two
 * consumers, so it leaves in both forms in one pass — out (rows, C) bf16, bit for bit fg_ln_modulate_bf16's / fg_ln_affine_bf16's result
 * (models/wan_video_dit.py:224,227 and :226), and out_fp8 (rows, C) e4m3 + out_scale (rows) fp32, byte for byte what
 * fg_ln_modulate_fp8_bf16 / fg_fp8_quant_rows_bf16 (act 0) make of that row.  The affine form takes no residual input: in this mode the
 * residual add that precedes norm3 happens in fg_gemm_fp8_bf16's store (mode 2).  out_fp8 8-byte aligned; fp8_max: 448 for e4m3fn. */
int fg_ln_modulate_dual_bf16(const void* x, const void* shift, const void* scale, void* out, void* out_fp8, float* out_scale,
                             int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                             float fp8_max, fg_stream_t stream);
int fg_ln_affine_dual_bf16(const void* x, const void* w, const void* b, void* out, void* out_fp8, float* out_scale,
                           int64_t rows, int C, float eps, float fp8_max, fg_stream_t stream);

/* nn.Linear of the DiT blocks (models/wan_video_dit.py:130-133,156-159,208-209): c[M,N] = a[M,K] w[N,K]^T + bias[N], bf16 in and
 * out, fp32 accumulation, bias added to the accumulator before the bf16 rounding — alone or with the op that follows it in the block
 * folded into the store (:188-193 GateModule, :208 nn.GELU(approximate='tanh'), :225-228):
 *   mode 0: c = bf16(acc + bias)                                   (nn.Linear)
 *   mode 2: c = bf16(c + bf16(gate * bf16(acc + bias)))            (x = x + gate * Linear(.), x read in place from c)
 *   mode 3: c = bf16(c + bf16(acc + bias))                         (x = x + Linear(.))
 *   mode 4: c = bf16(gelu_tanh(bf16(acc + bias)))                  (ffn.0 + GELU)
 * with the bf16 rounding points of the reference's separate ops.  a has leading dimension lda, c ldc (elements); w is the row-major
 * (out_features, in_features) weight.  gate: a table of gate_rows (1 or 2) rows of N values, row stride gate_ld elements; with 2 rows,
 * output rows < first_rows use row 0 (the first latent frame's t = 0 modulation), the others row 1.  N %% 256 == 0, K %% 128 == 0.
 * Persistent kernel: one workgroup per CU of the device takes 256 x 256 output tiles from a per-XCD cursor (csrc/gen_gemm_p.py).  The tiles left
 * over after the last whole round of the CUs are finished as pieces: with `workspace` (fg_gemm_workspace_bytes(M, N, K) bytes of
 * device memory, 16-byte aligned; may be NULL) and K >= 6144 or at most 8 rounds of tiles per CU cut along K into fp32 partial sums that a second small kernel adds in k
 * order before the same epilogue — those elements' fp32 summation is then grouped per piece (fixed for a given shape and device; every
 * other element is one full-K accumulation in k order); otherwise cut into 64-column pieces, every element accumulated in k order. */
int64_t fg_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int fg_gemm_epilogue_bf16(const void* a, int64_t lda, const void* w, const void* bias, void* c, int64_t ldc,
                          int64_t M, int64_t N, int64_t K, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                          int64_t first_rows, void* workspace, fg_stream_t stream);

/* Caller-owned scheduler state of the persistent GEMM.  The kernel's per-XCD unit cursors and its done counter live in a block of
 * fg_gemm_sched_bytes() bytes of device memory (16-byte aligned; the size is a constant, no device needed to ask).  A block must be in
 * its initial state before its first launch: fg_gemm_sched_reset enqueues that on `stream` (one asynchronous memset: no host
 * synchronisation, capturable).  Every launch leaves the block in the initial state again (its last workgroup clears it), so launches
 * need no reset between them; after a launch that did not run to its end (killed, faulted) the block is undefined and
 * fg_gemm_sched_reset repairs it.  ONE block serves launches that are ordered with respect to each other — one stream, or one captured
 * graph; launches that may run concurrently (two streams) need a block each, and likewise a `workspace` each.
 * fg_gemm_epilogue_bf16_s / fg_gemm_fp8_bf16_s: fg_gemm_epilogue_bf16 / fg_gemm_fp8_bf16 with that block as an argument — the same
 * kernels, plan and bits — and no other state: no allocation, no lock, no table, no host synchronisation, from the first call on a
 * stream on, so a stream capture can record them (with the reset, if wanted, as the first node).  workgroups: 0 = one per CU (or what
 * the fg_gemm_debug_grid diagnostic has set for the process); else the number of workgroups to launch, a multiple of the XCD count up
 * to the CU count — the units are fixed by the shape, the result is bit-identical for every value.  sched NULL or misaligned, or any
 * other workgroups value: FG_EINVAL. */
int64_t fg_gemm_sched_bytes(void);
int fg_gemm_sched_reset(void* sched, fg_stream_t stream);
int fg_gemm_epilogue_bf16_s(const void* a, int64_t lda, const void* w, const void* bias, void* c, int64_t ldc,
                            int64_t M, int64_t N, int64_t K, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                            int64_t first_rows, void* workspace, void* sched, int workgroups, fg_stream_t stream);

/* Hot-loaded (unfused) LoRA adapters of one Linear, AutoWrappedLinear.lora_forward (core/vram/layers.py:417-436: `out = out + x @ A^T @ B^T`
 * per adapter, in the pipeline dtype), for the adapters stacked along the rank and for G column groups that share the input x
 * (G = 3: q | k | v on the fused qkv buffer; else 1), in ONE launch next to fg_gemm_epilogue_bf16:
 *     t_g = bf16(x[M, K] A_g[R, K]^T),  l_g = bf16(t_g[M, R] B_g[Ng, R]^T)      (fp32 accumulate, one rounding each)
 *     out[:, g*Ng:(g+1)*Ng] = epi(out[:, g*Ng:(g+1)*Ng], l_g)
 * mode 0: l (plain write);  1: out + l;  2: out + bf16(gate * l), the gate table as in mode 2 of fg_gemm_epilogue_bf16 (1 or 2 rows of
 * gate_ld elements, rows < first_rows take row 0; here 16-byte aligned rows);  4: gelu_tanh(bf16(out + l)), the GEMM's GELU.
 * x: leading dimension ldx; out: leading dimension ldc >= G*Ng; a: the stacked (G*R, K) matrix (alpha folded in), b: the stacked
 * (G*Ng, R) matrix, both contiguous.  R is the per-group rank, padded by the host with zero rows of A / zero columns of B to 32, 64, 96
 * or 128; K %% 64 == 0, Ng %% 64 == 0, 1 <= G <= 4, ldx %% 8 == 0, ldc %% 8 == 0.  Rows >= M and columns >= G*Ng are not touched.
 * x is read once per pass: one pass for G = 1 and for (G = 3, R = 32), else one per group. */
int fg_lora_apply_bf16(const void* x, int64_t ldx, const void* a, const void* b, void* out, int64_t ldc, int64_t M, int64_t K,
                       int64_t Ng, int64_t R, int64_t G, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                       int64_t first_rows, fg_stream_t stream);

/* One LoRA adapter folded into one Linear's weight, lora/general.py fuse_lora_to_base_model (fairygen_amd/lora.py:38-58 restates it:
 * `weight + alpha * torch.mm(up, down)` in the pipeline dtype), with the original kept by the caller so the fuse can be undone:
 *     d = bf16(B[N, R] A[R, K])  (fp32 accumulate over R, one rounding),  d = bf16(alpha * d),  w' = bf16(w_src + d)
 * w_src (N, K) with leading dimension ld_src; w_dst (N, K) with its own ld_dst: w_src itself (same ld: in place) or memory that does not
 * overlap it, e.g. the row range of q, k or v in a block's fused QKV weight.  w_dst_fp8 (may be NULL; rows ld_fp8 bytes apart): the same
 * w' cast to OCP e4m3 with unit scale, the bytes of w'.to(float8_e4m3fn) for every value (like that cast it does not saturate: |w'| up
 * to 464 rounds to 448, larger values and NaN become the NaN byte with the sign); it must not overlap w_src or w_dst.  a_t is A TRANSPOSED, a contiguous (K, R) matrix, b a contiguous
 * (N, R) one; R is the rank padded by the host with zero columns to 32, 64, 96 or 128.  N %% 64 == 0, K %% 64 == 0, ld_src %% 8 == 0,
 * ld_dst %% 8 == 0, ld_fp8 %% 16 == 0, all pointers 16-byte aligned.  Every element of w is read once and written once; nothing else of
 * size (N, K) exists.  No allocation, no host synchronisation. */
int fg_lora_fuse_bf16(const void* w_src, int64_t ld_src, void* w_dst, int64_t ld_dst, void* w_dst_fp8, int64_t ld_fp8, const void* a_t,
                      const void* b, int64_t N, int64_t K, int64_t R, float alpha, fg_stream_t stream);

/* Diagnostics for the persistent GEMM's unit scheduler: launch only `workgroups` workgroups (a multiple of the XCD count, at most one
 * per CU; 0 = one per CU again).  The units of a launch are fixed by the shape; workgroups take them from per-XCD cursors, so the result
 * is bit-identical with any number of workgroups — as when other kernels (RCCL) hold some CUs.  Process-wide (an atomic word): it is
 * what a launch with workgroups == 0, and every launch of the two entry points without that argument, uses; the per-call `workgroups`
 * of the _s forms is the re-entrant way.  For those two entry points the library keeps 256 bytes of device memory per (device, stream)
 * it has launched a GEMM on (the cursors; cleared by the last workgroup of every launch). */
int fg_gemm_debug_grid(int workgroups);

/* The matmul of AutoWrappedLinear.fp8_linear (core/vram/layers.py:343-357: torch._scaled_mm(x_fp8, w_fp8.T, scale_a (rows, 1),
 * scale_b = ones (1, out), bias, out_dtype = bf16)) on the same persistent kernel with e4m3 operands (OCP float8_e4m3fn,
 * v_mfma_f32_32x32x64_f8f6f4): y = bf16((acc * scale_a[row]) + bias[col]) — one fp32 rounding per operation, as the library op —
 * followed by the epilogue `mode` of fg_gemm_epilogue_bf16 (0, 2, 3, 4) on y.  a_fp8: (M, K) bytes with leading dimension lda,
 * w_fp8: (N, K) row-major, scale_a: M fp32 values (fg_fp8_quant_rows_bf16 / the fp8-output norm kernels produce a_fp8 and scale_a).
 * N %% 256 == 0, K %% 256 == 0, lda %% 16 == 0; workspace as above (taken for K >= 12288 or at most 8 rounds of tiles per CU). */
int fg_gemm_fp8_bf16(const void* a_fp8, int64_t lda, const float* scale_a, const void* w_fp8, const void* bias, void* c, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                     int64_t first_rows, void* workspace, fg_stream_t stream);
/* ... on a caller-owned scheduler block: see fg_gemm_sched_bytes. */
int fg_gemm_fp8_bf16_s(const void* a_fp8, int64_t lda, const float* scale_a, const void* w_fp8, const void* bias, void* c, int64_t ldc,
                       int64_t M, int64_t N, int64_t K, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                       int64_t first_rows, void* workspace, void* sched, int workgroups, fg_stream_t stream);

/* RMSNorm over the full row (all heads), * weight, then optional 3-D RoPE on adjacent pairs:
 * RMSNorm.forward models/wan_video_dit.py:99-110 + rope_apply :91-96 (SelfAttention.forward :140-144,
 * CrossAttention.forward :176-177 with cos==sin==NULL).  x has leading dimension ldx (so q/k slices of a
 * fused QKV projection work), out is (rows, C) contiguous.
 * table_f32 == 0: cos_tab / sin_tab are fp64 (rows, head_dim/2) tables, the real / imag parts of the reference's
 *   complex128 table (pipelines/wan_video.py:1271-1275), and the rotation is done in fp64 exactly like rope_apply.
 * table_f32 != 0 (the default of the pipeline): cos_tab is ONE interleaved fp32 table (rows, head_dim/2, {cos, sin}) —
 *   the fp64 table rounded once — sin_tab is NULL, and the rotation is two fp32 FMAs per output: the fp64 rotation
 *   costs 43 us of VALU per call on top of the 77 us HBM time at N = 27 280 (2.8 -> 4.3 TB/s); the bf16 output
 *   differs from the fp64 mode in < 0.2 % of the elements, by one bf16 ulp (tests/test_hip_kernels.py). */
int fg_rmsnorm_rope_bf16(const void* x, int64_t ldx, const void* weight,
                         const void* cos_tab, const void* sin_tab, int table_f32, void* out,
                         int64_t rows, int C, int num_heads, float eps, fg_stream_t stream);

/* Same arithmetic, head-group-major output for the sequence-parallel Ulysses exchange (the reference's
 * xfuser path re-lays q/k out inside xFuserLongContextAttention, utils/xfuser/xdit_context_parallel.py:125-146):
 * column block g = col / group_cols of row r is written to out + g*out_group_stride + r*out_ld + col % group_cols,
 * i.e. straight into the all-to-all send buffer (block g = the heads of rank g). */
int fg_rmsnorm_rope_grouped_bf16(const void* x, int64_t ldx, const void* weight,
                                 const void* cos_tab, const void* sin_tab, int table_f32, void* out,
                                 int64_t rows, int C, int num_heads, float eps,
                                 int group_cols, int64_t out_group_stride, int64_t out_ld, fg_stream_t stream);

/* dst[g*dst_group_stride + r*dst_ld + c] = src[g*src_group_stride + r*src_ld + c] for g < groups, r < rows, c < cols
 * (strides in elements): the v columns into the Ulysses send buffer, and the received head-group blocks back to
 * "b s (n d)" rows before the o projection (xdit_context_parallel.py:139-145, the reference's rearranges). */
int fg_copy_groups_bf16(const void* src, int64_t src_group_stride, int64_t src_ld,
                        void* dst, int64_t dst_group_stride, int64_t dst_ld,
                        int groups, int64_t rows, int cols, fg_stream_t stream);

/* Activation side of the reference's fp8 Linear, AutoWrappedLinear.fp8_linear (core/vram/layers.py:321-357): per row of
 * x (rows, C; leading dimension ldx) scale[r] = max(bf16(max|x_r| / fp8_max), 1) and out_fp8[r] = e4m3fn(x_r / (scale[r] + 1e-8))
 * (OCP e4m3, torch.float8_e4m3fn; round to nearest even) — the arguments of the torch._scaled_mm call the reference makes
 * (row-wise scale_a, unit scale_b, bf16 bias).  act 1 applies GELU(tanh) first (ffn.2's input = nn.GELU(ffn.0(x)), rounded
 * to bf16 like the module output; optionally also written to act_out (rows, C)), act 0 quantises x as is.  fp8_max = 448. */
int fg_fp8_quant_rows_bf16(const void* x, int64_t ldx, void* out_fp8, float* scale, void* act_out,
                           int64_t rows, int C, int act, float fp8_max, fg_stream_t stream);

/* Elementwise activation, out may alias x.  kind 0: SiLU (time_embedding / time_projection,
 * models/wan_video_dit.py:312-318); kind 1: GELU(tanh) (ffn / text_embedding, :208-209,307-311). */
int fg_act_bf16(const void* x, void* out, int64_t n, int kind, fg_stream_t stream);

/* Non-causal softmax attention, head_dim 128: flash_attention()/AttentionModule,
 * models/wan_video_dit.py:27-60,113-120 (SDPA semantics: softmax(q k^T * scale) v, fp32 accumulate).
 * q:(B,Nq,H*128) k,v:(B,Nkv,H*128) with leading dimensions ldq/ldk/ldv (elements between token rows) and
 * batch strides Nq*ldq etc.; out (B,Nq,H*128) contiguous.  bf16 MFMA, fp32 online softmax.
 * workspace (optional, may be NULL/0): fg_attn_workspace_bytes(B,Nq,Nkv,H) bytes of scratch let the launcher cut
 * the tail q-blocks (or, for short query ranges such as a 1/8 token shard, every q-block) into KV ranges that are
 * merged by a second small kernel, so that the workgroup count fills the 256 CUs evenly; results are the same up
 * to fp32 summation order.  K/V of one batch element must span < 4 GiB.
 * scale: any positive value.  Self-attention shapes (Nkv > 1024) run a hand-scheduled 4-wave kernel in one of two forms with the same
 * result contract: when scale * log2(e) is a power of two (to 1e-6: pass 2^e / log2(e)) Q^T is pre-multiplied by it — exact in bf16 — and
 * the exponent needs no per-score multiply; for any other scale (e.g. 1/sqrt(128)) the scores of the exact operands are scaled in fp32.
 * A caller that wants the faster form for 1/sqrt(d) folds the factor 2^-e / sqrt(d) * log2(e) into q itself (wan_video_dit.py does,
 * through q's RoPE table). */
int64_t fg_attn_workspace_bytes(int B, int64_t Nq, int64_t Nkv, int H);
/* Diagnostic: the decomposition the launcher picks for this shape and workspace size: the last R q-blocks of every
 * (batch, head) are cut into S KV ranges (R == 0: no split). */
int fg_attn_split_choice(int B, int64_t Nq, int64_t Nkv, int H, int64_t workspace_bytes, int* R, int* S);
int fg_attn_fwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                     void* out, int B, int64_t Nq, int64_t Nkv, int H, int D, float scale,
                     void* workspace, int64_t workspace_bytes, fg_stream_t stream);

/* One scheduler step on the latent: pred = nega + cfg*(posi - nega) (pipelines/wan_video.py:302);
 * out = latents + pred*dsigma (FlowMatchScheduler.step, diffusion/flow_match.py:144-154), each op rounded
 * to bf16 like the reference's tensor arithmetic; nega==NULL means cfg_scale==1 (pred = posi).
 * out may alias latents. */
int fg_cfg_euler_bf16(const void* latents, const void* posi, const void* nega, void* out,
                      int64_t n, float cfg_scale, float dsigma, fg_stream_t stream);

/* fg_cfg_euler_bf16 for a step that is recorded once and replayed (a captured graph freezes by-value arguments): the same arithmetic with
 * the same rounding points, with dsigma = dsigma_table[*step] read by the kernel — dsigma_table: fp32 device memory, one entry per step
 * of the schedule; step: one int32 in device memory, 0 <= *step < entries (not checked: the host owns both) and advanced by the host's
 * own stream-ordered work, not here.  first != NULL also re-pins latent frame 0 in the same pass (latents[:, :, 0:1] = first of the
 * TI2V loop, pipelines/wan_video.py:304-305): with out laid out (C, T, H, W), frame_stride = T*H*W and first_n = H*W, element i of out
 * with i % frame_stride < first_n takes first[(i / frame_stride) * first_n + i % frame_stride] (first: (C, 1, H, W) contiguous bf16)
 * instead; n must be a multiple of frame_stride.  nega == NULL as above.  out may alias latents.  8-element vector accesses when
 * latents, posi, nega and out are all 16-byte aligned, single elements otherwise and for the n % 8 elements at the end. */
int fg_cfg_euler_dev_bf16(const void* latents, const void* posi, const void* nega, void* out,
                          int64_t n, float cfg_scale, const float* dsigma_table, const int* step,
                          const void* first, int64_t first_n, int64_t frame_stride, fg_stream_t stream);

/* ------------------------------------------------------------------------------- VAE decode kernels
 * Channels-last activations: (T,H,W,C) bf16.  */

/* RMS_norm over channels (+ optional SiLU): models/wan_video_vae.py:55-70 and the nn.SiLU after it
 * (:275-279,885): y = silu(bf16(bf16(bf16(x/max(||x||,1e-12)) * sqrt(C)) * gamma)). */
int fg_vae_rmsnorm_silu_bf16(const void* x, const void* gamma, void* out,
                             int64_t pixels, int C, int apply_silu, fg_stream_t stream);

/* Repack a Conv3d/Conv2d weight (Cout,Cin,kt,kh,kw) bf16 -> [kt*kh*kw][Cout_pad][Cin_pad] bf16 with
 * Cin_pad = roundup(Cin,64), Cout_pad = roundup(Cout,128) (zero filled).  fg_conv_packed_bytes gives the size. */
int64_t fg_conv_packed_bytes(int Cout, int Cin, int kt, int kh, int kw);
int fg_conv_pack_weight_bf16(const void* w, void* packed, int Cout, int Cin, int kt, int kh, int kw,
                             fg_stream_t stream);

/* Causal conv as implicit GEMM on MFMA: CausalConv3d.forward models/wan_video_vae.py:33-52 (kt in {1,3},
 * kh==kw in {1,3}, stride 1, "same" spatial zero padding, causal time padding); resample == 1: the Conv2d after
 * nearest-exact 2x upsampling in Resample38 (:242-251; input is (.,H/2,W/2,Cin)); resample == 2: the encoder's
 * ZeroPad2d((0,1,0,1)) + Conv2d(3, stride 2) of Resample38 downsample (:253-263; input is (.,2H,2W,Cin)).
 * x: (T + kt-1, Hin, Win, Cin) — the first kt-1 frames are the layer's feature cache, i.e. the previous input
 * frames that the reference concatenates in front (:46-49), zeros on the first chunk / after 'Rep'; output frame
 * t reads input frames t .. t+kt-1.  out (T,H,W,Cout), or with time_interleave!=0 (Resample.forward :153-156,
 * Cout = 2*Cout2): out (2T,H,W,Cout2) with channel block j of frame t written to frame 2t+j.
 * residual (same shape as out, or NULL) is added after the bf16 rounding of conv+bias (ResidualBlock :301).
 * Cin % 8 == 0; Cout % 4 == 0; input and packed weights < 3.75 GiB each (32-bit buffer offsets).
 * The shapes and rounding points are pinned by tests/test_conv_shapes.py. */
int fg_conv3d_cl_bf16(const void* x, const void* w_packed, const void* bias,
                      const void* residual, void* out,
                      int T, int H, int W, int Cin, int Cout, int kt, int ks,
                      int resample, int time_interleave, fg_stream_t stream);
/* Diagnostic: the tile variant fg_conv3d_cl_bf16 launches for an output of (T,H,W,Cout): 256 = conv3d_cl_w4_kernel or
 * conv3d_cl_256p_kernel (256x256x64 tile, LDS-DMA staging) when it fills the chip, else 128 = conv3d_cl_kernel (128x128x64). */
int fg_conv_tile_choice(int T, int H, int W, int Cout);

/* out = main + DupUp3D(x): models/wan_video_vae.py:417-439,510-512.  x (T,H,W,Cin); main/out
 * (T*ft - drop, H*fs, W*fs, Cout) where drop = ft-1 if first_chunk.  Cout % 8 == 0; x, main and out
 * 16-byte aligned (x is read with 16-byte vector loads when Cin % 8 == 0). */
int fg_dupup3d_add_bf16(const void* x, const void* main_path, void* out,
                        int T, int H, int W, int Cin, int Cout, int ft, int fs, int first_chunk,
                        fg_stream_t stream);

/* Row softmax of fp32 scores * scale -> bf16 probabilities (VAE mid AttentionBlock,
 * models/wan_video_vae.py:331-336; its two GEMMs stay on hipBLASLt).  scale > 0 and finite: the row maximum
 * is taken of the unscaled scores and subtracted before the multiplication. */
int fg_softmax_rows_f32_bf16(const float* scores, void* probs, int64_t rows, int64_t cols, float scale,
                             fg_stream_t stream);

/* Layout boundary: latent NCTHW (C,T,H,W) -> channels-last (T,H,W,C) with the de-normalisation
 * z/scale[1] + scale[0] of VideoVAE38_.decode (models/wan_video_vae.py:1328-1331): mean/inv_std are bf16 (C). */
int fg_vae_latent_to_cl_bf16(const void* z, const void* mean, const void* inv_std, void* out,
                             int C, int T, int H, int W, fg_stream_t stream);

/* Decoder head output (T,H,W,12) channels-last -> unpatchify(…,2) (models/wan_video_vae.py:214-224,1349)
 * -> frames [t0, t0+T) of a (3,F,2H,2W) NCTHW video; clamp to [-1,1] when do_clamp
 * (single_decode :1215). */
int fg_vae_unpatchify_bf16(const void* x, void* video, int T, int H, int W, int F, int t0, int do_clamp,
                           fg_stream_t stream);

/* Tiled-decode feathering (WanVideoVAE.tiled_decode models/wan_video_vae.py:1124-1149, masks :1081-1100):
 * values[:, :, y0:y0+th, x0:x0+tw] += tile*mask ; weight[...] += mask, bf16 accumulators like the
 * reference; mask(y,x) = min(ramp_h(y), ramp_w(x)), ramps of width border_h/border_w on non-bound sides.
 * values (C,F,Hv,Wv), weight (F,Hv,Wv), tile (C,F,th,tw) (C = 3 decode, 48 tiled_encode :1176-1201).
 * bound bits: 1 top, 2 bottom, 4 left, 8 right.  An axis with a free side needs border <= tile length (FG_EINVAL otherwise, as
 * the reference's slice assignment raises there); a tile shorter than two borders takes the second ramp where the two overlap. */
int fg_vae_tile_accumulate_bf16(const void* tile, void* values, void* weight,
                                int C, int F, int Hv, int Wv, int th, int tw, int y0, int x0,
                                int border_h, int border_w, int bound_bits, fg_stream_t stream);

/* values = values / weight, clamped to [-1,1] when do_clamp (decode :1150-1151; encode :1202 does not clamp). */
int fg_vae_tile_finalize_bf16(void* values, const void* weight, int C, int F, int Hv, int Wv, int do_clamp,
                              fg_stream_t stream);

/* Encoder boundary (first-frame conditioning, VideoVAE38_.encode models/wan_video_vae.py:1298-1323):
 * video (3,T,H,W) NCTHW -> patchify(.,2) (:199-211) -> channels-last (T,H/2,W/2,16): 12 channels + 4 zeros, so the
 * 12->dim conv1 reads whole 16-byte chunks (its packed weights are zero beyond channel 12). */
int fg_vae_patchify_bf16(const void* video, void* out, int T, int H, int W, fg_stream_t stream);

/* out = main + AvgDown3D(x): Down_ResidualBlock shortcut (models/wan_video_vae.py:363-395,474).  x (T,H,W,Cin);
 * main/out (ceil(T/ft),H/fs,W/fs,Cout); a missing leading frame counts as zeros (the reference pads in front). */
int fg_avgdown3d_add_bf16(const void* x, const void* main_path, void* out,
                          int T, int H, int W, int Cin, int Cout, int ft, int fs, fg_stream_t stream);

/* Encoder tail (:1314-1321): x (T,H,W,Cx) channels-last, mu = first Z channels; out (Z,T,H,W) = (mu - mean) * inv_std. */
int fg_vae_latent_from_cl_bf16(const void* x, const void* mean, const void* inv_std, void* out,
                               int Z, int Cx, int T, int H, int W, fg_stream_t stream);

/* (3,F,H,W) bf16 in [-1,1] -> (F,H,W,3) uint8 by ((x+1)*127.5).clip(0,255) truncation
 * (BasePipeline.vae_output_to_video, diffusion/base_pipeline.py:128-143). */
int fg_video_to_uint8(const void* video, void* out_u8, int F, int H, int W, fg_stream_t stream);

/* ------------------------------------------------------------------------ umT5 text encoder helpers
 * (WanTextEncoder runs twice per clip before the loop; its GEMMs stay on hipBLASLt, T5LayerNorm is
 * fg_rmsnorm_rope_bf16 without tables.) */

/* T5Attention softmax, models/wan_video_text_encoder.py:72-87: probs = softmax over keys of
 * bf16(scores + bias), bias replaced by finfo(bf16).min where key_mask[c] == 0 (key_mask may be NULL);
 * scores/bias/probs (rows, cols) bf16, fp32 softmax, no 1/sqrt(d) scaling. */
int fg_softmax_bias_bf16(const void* scores, const void* bias, const int* key_mask, void* probs,
                         int64_t rows, int64_t cols, fg_stream_t stream);

/* T5FeedForward gate, :19-22,109-111: out = fc1 * (0.5*g*(1+tanh(sqrt(2/pi)*(g+0.044715*g^3)))), each tensor op of
 * that expression rounded to bf16 as the reference's explicit GELU module does. */
int fg_gated_gelu_bf16(const void* fc1, const void* gate, void* out, int64_t n, fg_stream_t stream);

/* ------------------------------------------------------------- e4m3 Q K^T self-attention (opt-in)
 * The self-attention with an 8-bit Q K^T product, under the contract above.  tests/test_attention_qk8.py holds the recipe, the argument
 * checks, the stream and capture checks. */

int fg_attn_qk8_version(void);           /* version of this extension, currently 1 */

/* The form the reference's flash_attention takes when the sageattention package is present (models/wan_video_dit.py:48-52: sageattn with
 * q, k, v): e4m3 Q K^T with K mean-smoothing, P V in bf16.  One head at a time, q and k (N, 128) after RMSNorm and RoPE:
 *   kbar = mean of k over its N rows (per channel: the fp64 sum, divided by N, rounded once to fp32); k' = fp32(k) - kbar;
 *   sk = max(max|k'| / 448, 2^-20), one per head; k8 = e4m3(k' / sk), round-to-nearest-even, saturating at +-448;
 *   sq[r] = max(max|q[r]| / 448, 2^-20), one per row and head; q8 = e4m3(q / sq[r]);
 *   out = softmax(scale * sq[r] * sk * (q8 k8^T)) v — the product accumulated in fp32 by the plain (unscaled) e4m3 MFMA, the online
 *   softmax, the bf16 P and the bf16 P V of the 8-wave kernel behind fg_attn_fwd_bf16.  q . kbar is constant along a row: dropped.
 * fg_attn_quant_qk_bf16: q, k (N, H*128) bf16 with leading dimensions ldq / ldk -> q8, k8 (N, H*128) e4m3 bytes (8-byte aligned),
 * sq (N, H) and sk (H) fp32.  Two launches on `stream`; scratch: H*128 floats (the column means), 16-byte aligned.  One batch element.
 * fg_attn_fwd_qk8_bf16: q8 (Nq, H*128), k8 (Nkv, H*128), sq (Nq, H), sk (H) as written above (q8, k8 16-byte aligned), v (Nkv, H*128)
 * bf16 with leading dimension ldv, out (Nq, H*128) bf16 contiguous.  workspace: as for fg_attn_fwd_bf16, sized by fg_attn_workspace_bytes
 * with B = 1.  Any Nkv >= 1; cross-attention is not meant to take it. */
int fg_attn_quant_qk_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, void* q8, void* k8, float* sq, float* sk,
                          void* scratch, int64_t scratch_bytes, int64_t N, int H, int D, fg_stream_t stream);
int fg_attn_fwd_qk8_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v, int64_t ldv, void* out,
                         int64_t Nq, int64_t Nkv, int H, int D, float scale, void* workspace, int64_t workspace_bytes,
                         fg_stream_t stream);

/* ------------------------------------------- the e4m3 operands written by the RMSNorm+RoPE pass
 * The operands of fg_attn_fwd_qk8_bf16 written by the RMSNorm+RoPE pass itself, by the recipe above, unchanged: on the same inputs these
 * entry points write the q8, sq, k8, sk and key mean that fg_rmsnorm_rope_bf16 followed by fg_attn_quant_qk_bf16 writes, byte for byte —
 * the key mean where its fp64 sum is exact (8 significand bits + the exponent spread of the non-zero values + log2 N below 53 bits),
 * which is where the order of a sum cannot show.  tests/test_attention_qk8_fused.py holds the comparison, the argument, stream and
 * capture checks. */

int fg_attn_qk8_fused_version(void);     /* version of this extension, currently 1 */

/* Bytes of the key-statistics partials for `rows` keys of C channels: P records per channel (an fp64 sum, a minimum, a maximum: 16
 * bytes), P a function of rows alone.  -1 on rows < 1 or a C that is not a positive multiple of 128 up to 4096. */
int64_t fg_attn_qk8_fused_scratch_bytes(int64_t rows, int C);

/* x (rows, C) bf16 with leading dimension ldx, weight (C), the rope tables and table_f32 as for fg_rmsnorm_rope_bf16, C = num_heads * 128.
 * fg_rmsnorm_rope_q8_bf16: the normed, rotated row never leaves as bf16: q8 (rows, C) e4m3 bytes (8-byte aligned) and sq (rows,
 * num_heads) fp32, one scale per row and head.  One launch.
 * fg_rmsnorm_rope_kstats_bf16: k_out (rows, C) bf16 contiguous — fg_rmsnorm_rope_bf16's bytes — and, to `partials` (16-byte aligned,
 * fg_attn_qk8_fused_scratch_bytes), every workgroup's per-channel sum, minimum and maximum of the rows it walked.  One launch; every
 * record of the buffer is written (a workgroup without a row writes 0, +inf, -inf).
 * fg_attn_quant_k_bf16: k (N, H*128) bf16 with leading dimension ldk and the partials written for these N rows -> kbar (H*128 fp32,
 * 16-byte aligned; the mean), sk (H) and k8 (N, H*128) e4m3 bytes (8-byte aligned).  Two launches: the reduction of the partials
 * (sk from the channel extremes: fp32 rounding is monotone, so max_rows |fl(k - kbar)| = max(fl(kmax - kbar), fl(kbar - kmin))), then
 * the quantise pass. */
int fg_rmsnorm_rope_q8_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                            void* q8, float* sq, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream);
int fg_rmsnorm_rope_kstats_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                                void* k_out, void* partials, int64_t partials_bytes, int64_t rows, int C, int num_heads, float eps,
                                fg_stream_t stream);
int fg_attn_quant_k_bf16(const void* k, int64_t ldk, const void* partials, int64_t partials_bytes, void* k8, float* sk, float* kbar,
                         int64_t N, int H, int D, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_H */

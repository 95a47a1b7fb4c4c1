"""ctypes binding of libfairygen_hip.so (C ABI: include/fairygen_hip.h).

This is the ONLY compute backend of the package.  There is no CPU or eager-PyTorch fallback: if the
library is missing, or a tensor is not a contiguous bf16 tensor on a HIP device, the call raises.
PyTorch is used for device memory, streams and the plain GEMMs (hipBLASLt) only.
"""
import ctypes
import os

import torch

# FAIRYGEN_HIP_LIB: load an alternative build of the same ABI (kernel A/B experiments); still no fallback.
_LIB_PATH = os.environ.get("FAIRYGEN_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfairygen_hip.so")
_lib = None

ABI_VERSION = 8
QK8_ABI_VERSION = 1       # fg_attn_qk8_version: the e4m3 Q K^T self-attention
QK8F_ABI_VERSION = 1      # fg_attn_qk8_fused_version: its operands written by the RMSNorm+RoPE pass

_i64, _i32, _f32, _vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p

# The entry points that take a stream and return int: name -> argtypes.  With _QUERIES, what include/fairygen_hip.h declares.
_SIGNATURES = {
    "fg_ln_modulate_bf16": [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _i64, _i64, _i64, _vp],
    "fg_ln_affine_bf16": [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp],
    "fg_ln_modulate_fp8_bf16": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _i64, _i64, _i64, _f32, _vp],
    "fg_residual_ln_fp8_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _f32, _vp],
    "fg_ln_modulate_dual_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _i64, _i64, _i64, _f32, _vp],
    "fg_ln_affine_dual_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _f32, _vp],
    "fg_gate_residual_bf16": [_vp, _vp, _vp, _vp, _i64, _i32, _i64, _i64, _i64, _vp],
    "fg_residual_ln_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _vp],
    "fg_rmsnorm_rope_bf16": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _f32, _vp],
    "fg_rmsnorm_rope_grouped_bf16": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _f32, _i32, _i64, _i64, _vp],
    "fg_copy_groups_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i64, _i32, _vp],
    "fg_fp8_quant_rows_bf16": [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _vp],
    "fg_act_bf16": [_vp, _vp, _i64, _i32, _vp],
    "fg_gemm_epilogue_bf16": [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _vp],
    "fg_gemm_fp8_bf16": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _vp],
    "fg_gemm_sched_reset": [_vp, _vp],
    "fg_gemm_epilogue_bf16_s": [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _i32, _vp],
    "fg_gemm_fp8_bf16_s": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _i32, _vp],
    "fg_lora_apply_bf16": [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp],
    "fg_attn_fwd_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _i64, _i64, _i32, _i32, _f32, _vp, _i64, _vp],
    "fg_cfg_euler_bf16": [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _vp],
    "fg_vae_rmsnorm_silu_bf16": [_vp, _vp, _vp, _i64, _i32, _i32, _vp],
    "fg_conv_pack_weight_bf16": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_conv3d_cl_bf16": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_dupup3d_add_bf16": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_softmax_rows_f32_bf16": [_vp, _vp, _i64, _i64, _f32, _vp],
    "fg_vae_latent_to_cl_bf16": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "fg_vae_unpatchify_bf16": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_vae_tile_accumulate_bf16": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_vae_tile_finalize_bf16": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_vae_patchify_bf16": [_vp, _vp, _i32, _i32, _i32, _vp],
    "fg_avgdown3d_add_bf16": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_vae_latent_from_cl_bf16": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "fg_video_to_uint8": [_vp, _vp, _i32, _i32, _i32, _vp],
    "fg_softmax_bias_bf16": [_vp, _vp, _vp, _vp, _i64, _i64, _vp],
    "fg_gated_gelu_bf16": [_vp, _vp, _vp, _i64, _vp],
    "fg_lora_fuse_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _f32, _vp],
    "fg_cfg_euler_dev_bf16": [_vp, _vp, _vp, _vp, _i64, _f32, _vp, _vp, _vp, _i64, _i64, _vp],
    "fg_attn_quant_qk_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp],
    "fg_attn_fwd_qk8_bf16": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _f32, _vp, _i64, _vp],
    "fg_rmsnorm_rope_q8_bf16": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i32, _i32, _f32, _vp],
    "fg_rmsnorm_rope_kstats_bf16": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _vp],
    "fg_attn_quant_k_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _vp],
}
# The host-only functions (no stream, nothing launched): name -> (restype, argtypes).
_QUERIES = {
    "fg_version": (_i32, []),
    "fg_last_error": (ctypes.c_char_p, []),
    "fg_conv_packed_bytes": (_i64, [_i32] * 5),
    "fg_attn_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32]),
    "fg_attn_split_choice": (_i32, [_i32, _i64, _i64, _i32, _i64, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "fg_conv_tile_choice": (_i32, [_i32] * 4),
    "fg_gemm_workspace_bytes": (_i64, [_i64] * 3),
    "fg_gemm_debug_grid": (_i32, [_i32]),
    "fg_gemm_sched_bytes": (_i64, []),
    "fg_attn_qk8_version": (_i32, []),
    "fg_attn_qk8_fused_version": (_i32, []),
    "fg_attn_qk8_fused_scratch_bytes": (_i64, [_i64, _i32]),
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + list(_QUERIES))      # what include/fairygen_hip.h declares

# The extension of include/fairygen_hip_pv8.h (self-attention with the P V product on the e4m3 MFMA too): a second pair of tables, bound
# and version-checked by load() next to the first; the main table, its header and ABI_VERSION do not change for it.
PV8_ABI_VERSION = 1       # fg_attn_pv8_version
_PV8_SIGNATURES = {
    "fg_attn_quant_vt_bf16": [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp],
    "fg_attn_fwd_pv8_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _vp, _i64, _vp],
}
_PV8_QUERIES = {
    "fg_attn_pv8_version": (_i32, []),
    "fg_attn_pv8_scratch_bytes": (_i64, [_i64, _i32]),
}
PV8_SYMBOLS = sorted(list(_PV8_SIGNATURES) + list(_PV8_QUERIES))    # what include/fairygen_hip_pv8.h declares
# Byte p of a 64-key tile of v8t holds key PV8_KEY_ORDER[p] of the tile: the order in which a lane of the attention kernel holds the
# scores of its query row (lane half p >> 5, score sub-tile (p >> 4) & 1, accumulator register p & 15)
PV8_KEY_ORDER = tuple(32 * ((p >> 4) & 1) + 8 * ((p & 15) >> 2) + 4 * (p >> 5) + (p & 3) for p in range(64))
PV8_LOG2_C, PV8_DEFER_LOG2 = 5, 3     # P8 = e4m3(2^5 p), p <= 2^3 under the deferred rescale of the e4m3 P V form: 2^8 <= 448

# The extension of include/fairygen_hip_shard8.h (the e4m3 operands of a token shard whose K / V are all-gathered): a third pair of tables.
SHARD8_ABI_VERSION = 1    # fg_attn_shard8_version
_SHARD8_SIGNATURES = {
    "fg_attn_shard8_stats": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp],
    "fg_attn_shard8_quant": [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp],
    "fg_attn_shard8_vt": [_vp, _vp, _i64, _i32, _i32, _vp],
}
_SHARD8_QUERIES = {
    "fg_attn_shard8_version": (_i32, []),
    "fg_attn_shard8_record_bytes": (_i64, [_i32]),
    "fg_attn_shard8_scratch_bytes": (_i64, [_i64, _i32]),
}
SHARD8_SYMBOLS = sorted(list(_SHARD8_SIGNATURES) + list(_SHARD8_QUERIES))    # what include/fairygen_hip_shard8.h declares

# The extension of include/fairygen_hip_cross8.h (e4m3 cross-attention with a head's K8 and V8^T resident in LDS): a fourth pair of tables.
CROSS8_ABI_VERSION = 1    # fg_attn_cross8_version
_CROSS8_SIGNATURES = {
    "fg_attn_fwd_cross8_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _vp],
}
_CROSS8_QUERIES = {
    "fg_attn_cross8_version": (_i32, []),
    "fg_attn_cross8_max_kv": (_i64, []),
}
CROSS8_SYMBOLS = sorted(list(_CROSS8_SIGNATURES) + list(_CROSS8_QUERIES))    # what include/fairygen_hip_cross8.h declares

# The extension of include/fairygen_hip_batch8.h (the whole e4m3 attention chain on a batch, one launch sequence): a fifth pair of tables.
BATCH8_ABI_VERSION = 1    # fg_attn_batch8_version
_BATCH8_SIGNATURES = {
    "fg_attn_quant_qk_bf16_b": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i64,
                                _i32, _i32, _vp],
    "fg_rmsnorm_rope_q8_bf16_b": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _vp],
    "fg_rmsnorm_rope_kstats_bf16_b": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _i64, _i32, _i32, _f32, _vp],
    "fg_attn_quant_k_bf16_b": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_quant_vt_bf16_b": [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_fwd_qk8_bf16_b": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _f32, _vp,
                               _i64, _vp],
    "fg_attn_fwd_pv8_bf16_b": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _f32,
                               _vp, _i64, _vp],
    "fg_attn_fwd_cross8_bf16_b": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _i32,
                                  _f32, _vp],
}
_BATCH8_QUERIES = {
    "fg_attn_batch8_version": (_i32, []),
}
BATCH8_SYMBOLS = sorted(list(_BATCH8_SIGNATURES) + list(_BATCH8_QUERIES))    # what include/fairygen_hip_batch8.h declares

# The extension of include/fairygen_hip_rowbatch.h (the row kernels that read a per-row table, on a batch that shares the table): a sixth pair.
ROWBATCH_ABI_VERSION = 1  # fg_dit_rowbatch_version
_ROWBATCH_SIGNATURES = {
    "fg_ln_modulate_bf16_b": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _vp],
    "fg_gate_residual_bf16_b": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i64, _i64, _i64, _vp],
    "fg_residual_ln_bf16_b": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _vp],
    "fg_rmsnorm_rope_bf16_b": [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _i32, _i64, _i32, _i32, _f32, _vp],
}
_ROWBATCH_QUERIES = {
    "fg_dit_rowbatch_version": (_i32, []),
}
ROWBATCH_SYMBOLS = sorted(list(_ROWBATCH_SIGNATURES) + list(_ROWBATCH_QUERIES))    # what include/fairygen_hip_rowbatch.h declares

# The extension of include/fairygen_hip_rowbatch8.h (the same batches, the norms whose row leaves as e4m3 bytes and a scale): a seventh pair.
ROWBATCH8_ABI_VERSION = 1  # fg_dit_rowbatch8_version
_ROWBATCH8_SIGNATURES = {
    "fg_ln_modulate_fp8_bf16_b": [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _f32, _vp],
    "fg_residual_ln_fp8_bf16_b": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _f32, _vp],
}
_ROWBATCH8_QUERIES = {
    "fg_dit_rowbatch8_version": (_i32, []),
}
ROWBATCH8_SYMBOLS = sorted(list(_ROWBATCH8_SIGNATURES) + list(_ROWBATCH8_QUERIES))    # what include/fairygen_hip_rowbatch8.h declares

# The extension of include/fairygen_hip_lorabatch.h (the same batches, what unfused hot-loaded adapters need: the adapter kernel and the
# two-output modulate norm): an eighth pair.
LORABATCH_ABI_VERSION = 1  # fg_dit_lorabatch_version
_LORABATCH_SIGNATURES = {
    "fg_lora_apply_bf16_b": [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp],
    "fg_ln_modulate_dual_bf16_b": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _i64, _i64, _i64, _f32, _vp],
}
_LORABATCH_QUERIES = {
    "fg_dit_lorabatch_version": (_i32, []),
}
LORABATCH_SYMBOLS = sorted(list(_LORABATCH_SIGNATURES) + list(_LORABATCH_QUERIES))    # what include/fairygen_hip_lorabatch.h declares

# The extension of include/fairygen_hip_up2phase.h (the VAE decoder's nearest-2x upsample + 3x3 conv as four 2x2 phase convs): a ninth pair.
UP2PHASE_ABI_VERSION = 1  # fg_conv_up2phase_version
_UP2PHASE_SIGNATURES = {
    "fg_conv_up2phase_pack_bf16": [_vp, _vp, _i32, _i32, _vp],
    "fg_conv3d_up2_phase_bf16": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
}
_UP2PHASE_QUERIES = {
    "fg_conv_up2phase_version": (_i32, []),
    "fg_conv_up2phase_packed_bytes": (_i64, [_i32] * 2),
}
UP2PHASE_SYMBOLS = sorted(list(_UP2PHASE_SIGNATURES) + list(_UP2PHASE_QUERIES))    # what include/fairygen_hip_up2phase.h declares

# The extension of include/fairygen_hip_gategemm.h (the persistent GEMM's gated store with its row rule counted inside the elements of a
# batch that shares a two-row gate table): a tenth pair.  The _s signatures with rows_per_element behind first_rows.
GATEGEMM_ABI_VERSION = 1  # fg_gemm_gate_period_version
_GATEGEMM_SIGNATURES = {
    "fg_gemm_epilogue_bf16_sp": [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i32, _vp],
    "fg_gemm_fp8_bf16_sp": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i32, _vp],
}
_GATEGEMM_QUERIES = {
    "fg_gemm_gate_period_version": (_i32, []),
}
GATEGEMM_SYMBOLS = sorted(list(_GATEGEMM_SIGNATURES) + list(_GATEGEMM_QUERIES))    # what include/fairygen_hip_gategemm.h declares
GEMM_GATE_MIN_PERIOD = 256      # rows_per_element below the tile height is refused unless it covers all rows (one element)

# The extension of include/fairygen_hip_smoothv.h (the e4m3 P V self-attention with V mean-smoothed: the key mean of every channel leaves V
# before it is quantised and joins the output row before it is rounded): an eleventh pair.  The pv8 signatures with mu behind sv.
SMOOTHV_ABI_VERSION = 1   # fg_attn_smoothv_version
_SMOOTHV_SIGNATURES = {
    "fg_attn_quant_vt_smooth_bf16": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp],
    "fg_attn_quant_vt_smooth_bf16_b": [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_fwd_pv8s_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _vp, _i64, _vp],
    "fg_attn_fwd_pv8s_bf16_b": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32,
                                _i32, _f32, _vp, _i64, _vp],
}
_SMOOTHV_QUERIES = {
    "fg_attn_smoothv_version": (_i32, []),
    "fg_attn_smoothv_scratch_bytes": (_i64, [_i64, _i32]),
}
SMOOTHV_SYMBOLS = sorted(list(_SMOOTHV_SIGNATURES) + list(_SMOOTHV_QUERIES))    # what include/fairygen_hip_smoothv.h declares

# The extension of include/fairygen_hip_cross8s.h (the e4m3 cross-attention with V mean-smoothed: the operands of the smoothing V producer,
# the key mean added where an output row is rounded): a twelfth pair.  The cross8 signatures with mu (and bs_mu) behind sv (and bs_sv).
CROSS8S_ABI_VERSION = 1   # fg_attn_cross8s_version
_CROSS8S_SIGNATURES = {
    "fg_attn_fwd_cross8s_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _vp],
    "fg_attn_fwd_cross8s_bf16_b": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _i64,
                                   _i32, _i32, _f32, _vp],
}
_CROSS8S_QUERIES = {
    "fg_attn_cross8s_version": (_i32, []),
}
CROSS8S_SYMBOLS = sorted(list(_CROSS8S_SIGNATURES) + list(_CROSS8S_QUERIES))    # what include/fairygen_hip_cross8s.h declares

# The extension of include/fairygen_hip_shard8s.h (the operands of a token shard for the e4m3 P V form with V mean-smoothed: a record that
# carries the fp64 sum, the minimum and the maximum of v beside those of k): a thirteenth pair.  The shard8 signatures, mu behind sv.
SHARD8S_ABI_VERSION = 1   # fg_attn_shard8s_version
_SHARD8S_SIGNATURES = {
    "fg_attn_shard8s_stats": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp],
    "fg_attn_shard8s_quant": [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp],
}
_SHARD8S_QUERIES = {
    "fg_attn_shard8s_version": (_i32, []),
    "fg_attn_shard8s_record_bytes": (_i64, [_i32]),
    "fg_attn_shard8s_scratch_bytes": (_i64, [_i64, _i32]),
}
SHARD8S_SYMBOLS = sorted(list(_SHARD8S_SIGNATURES) + list(_SHARD8S_QUERIES))    # what include/fairygen_hip_shard8s.h declares

# The extension of include/fairygen_hip_shard8b.h (the producers of the two token-shard extensions on a batch: the stacked CFG forward on a
# rank of the K / V all-gather layout): a fourteenth pair, the thirteenth extension.  The single forms' signatures with an element stride
# behind every input's leading dimension and B in front of the row count.
SHARD8B_ABI_VERSION = 1   # fg_attn_shard8b_version
_SHARD8B_SIGNATURES = {
    "fg_attn_shard8_stats_b": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_shard8_quant_b": [_vp, _i64, _i32, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_shard8_vt_b": [_vp, _i64, _vp, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_shard8s_stats_b": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i64, _i32, _i32, _vp],
    "fg_attn_shard8s_quant_b": [_vp, _i64, _i32, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp],
}
_SHARD8B_QUERIES = {
    "fg_attn_shard8b_version": (_i32, []),
}
SHARD8B_SYMBOLS = sorted(list(_SHARD8B_SIGNATURES) + list(_SHARD8B_QUERIES))    # what include/fairygen_hip_shard8b.h declares


class HipLibraryError(RuntimeError):
    pass


def library_path():
    return _LIB_PATH


def load():
    """Load libfairygen_hip.so (built by __graft_entry__.build() / make -C fairygen_amd/csrc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipLibraryError(
            f"{_LIB_PATH} not found: build it with `make -C fairygen_amd/csrc` (or __graft_entry__.build()). "
            "fairygen_amd has no CPU / PyTorch fallback for its kernels.")
    lib = ctypes.CDLL(_LIB_PATH)
    for name, argtypes in list(_SIGNATURES.items()) + list(_PV8_SIGNATURES.items()) + list(_SHARD8_SIGNATURES.items()) + \
            list(_CROSS8_SIGNATURES.items()) + list(_BATCH8_SIGNATURES.items()) + list(_ROWBATCH_SIGNATURES.items()) + \
            list(_ROWBATCH8_SIGNATURES.items()) + list(_LORABATCH_SIGNATURES.items()) + list(_UP2PHASE_SIGNATURES.items()) + \
            list(_GATEGEMM_SIGNATURES.items()) + list(_SMOOTHV_SIGNATURES.items()) + list(_CROSS8S_SIGNATURES.items()) + \
            list(_SHARD8S_SIGNATURES.items()) + list(_SHARD8B_SIGNATURES.items()):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _i32, argtypes
    for name, (restype, argtypes) in list(_QUERIES.items()) + list(_PV8_QUERIES.items()) + list(_SHARD8_QUERIES.items()) + \
            list(_CROSS8_QUERIES.items()) + list(_BATCH8_QUERIES.items()) + list(_ROWBATCH_QUERIES.items()) + \
            list(_ROWBATCH8_QUERIES.items()) + list(_LORABATCH_QUERIES.items()) + list(_UP2PHASE_QUERIES.items()) + \
            list(_GATEGEMM_QUERIES.items()) + list(_SMOOTHV_QUERIES.items()) + list(_CROSS8S_QUERIES.items()) + \
            list(_SHARD8S_QUERIES.items()) + list(_SHARD8B_QUERIES.items()):
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    for name, expected, what in (("fg_version", ABI_VERSION, ""), ("fg_attn_qk8_version", QK8_ABI_VERSION, " (e4m3 Q K^T extension)"),
                                 ("fg_attn_qk8_fused_version", QK8F_ABI_VERSION, " (fused e4m3 producers)"),
                                 ("fg_attn_pv8_version", PV8_ABI_VERSION, " (e4m3 P V extension)"),
                                 ("fg_attn_shard8_version", SHARD8_ABI_VERSION, " (e4m3 operands of a token shard)"),
                                 ("fg_attn_cross8_version", CROSS8_ABI_VERSION, " (e4m3 cross-attention, K8 / V8^T in LDS)"),
                                 ("fg_attn_batch8_version", BATCH8_ABI_VERSION, " (e4m3 attention on batches)"),
                                 ("fg_dit_rowbatch_version", ROWBATCH_ABI_VERSION, " (row kernels on batches that share a table)"),
                                 ("fg_dit_rowbatch8_version", ROWBATCH8_ABI_VERSION, " (fp8-output norms on batches that share a table)"),
                                 ("fg_dit_lorabatch_version", LORABATCH_ABI_VERSION, " (hot-loaded adapters on batches that share a table)"),
                                 ("fg_conv_up2phase_version", UP2PHASE_ABI_VERSION, " (upsample conv as four 2x2 phase convs)"),
                                 ("fg_gemm_gate_period_version", GATEGEMM_ABI_VERSION, " (gated GEMM store on batches that share a gate table)"),
                                 ("fg_attn_smoothv_version", SMOOTHV_ABI_VERSION, " (e4m3 P V with mean-smoothed V)"),
                                 ("fg_attn_cross8s_version", CROSS8S_ABI_VERSION, " (e4m3 cross-attention with mean-smoothed V)"),
                                 ("fg_attn_shard8s_version", SHARD8S_ABI_VERSION, " (e4m3 operands of a token shard, V mean-smoothed)"),
                                 ("fg_attn_shard8b_version", SHARD8B_ABI_VERSION, " (e4m3 operands of a token shard on batches)")):
        if getattr(lib, name)() != expected:
            raise HipLibraryError(f"ABI mismatch{what}: library {getattr(lib, name)()} != binding {expected}")
    _lib = lib
    return lib


def _call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise HipLibraryError(f"{name} failed ({rc}): {lib.fg_last_error().decode()}")


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dev(t, name, dtype=torch.bfloat16):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise HipLibraryError(f"{name}: expected a tensor on a HIP device, got {getattr(t, 'device', type(t))} "
                              "(no CPU fallback)")
    if t.dtype != dtype:
        raise HipLibraryError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _rows(t, name):
    """View (..., C) contiguous as (rows, C)."""
    _dev(t, name)
    if not t.is_contiguous():
        raise HipLibraryError(f"{name}: must be contiguous")
    return t.numel() // t.shape[-1], t.shape[-1]


def _rows2d(t, who, cols="C"):
    """(..., C) with a dense last dim as the 2-D (rows, C) view the fg_* kernels take with a row stride: a contiguous tensor of any rank,
    a strided 2-D one (a column slice of a wider buffer) or a strided (1, rows, C).  `who` prefixes the error."""
    if t.stride(-1) != 1:
        raise HipLibraryError(f"{who}: last dim must be dense")
    t2 = t.reshape(-1, t.shape[-1]) if t.is_contiguous() else (t.squeeze(0) if t.dim() == 3 else t)
    if t2.dim() != 2:
        raise HipLibraryError(f"{who}: strided input must be 2-D (rows, {cols}) or (1, rows, {cols})")
    return t2


class ModTable:
    """AdaLN modulation rows: tensor (mod_rows, K, C) bf16; vector j of row r = table[r, j].

    mod_rows 1 (T2V), 2 (TI2V: tokens < first_rows use row 0) or N (per token).

    A table of TWO rows is always the TI2V split, also on a call of two token rows: that is the only two-row table the model builds
    (wan_video_dit.py forward_tokens_steps: R = 1 or 2 distinct rows, and a token shard behind the first latent frame arrives with
    first_rows = 0, both of its tokens on row 1).  per_token=True states the other meaning — row r of the call reads row r of the
    table, which must then have as many rows as the call — and is what makes a two-row per-token table reach the kernels as
    first_rows = 1 (rows [0, 1) on row 0, the rest on row 1: the same thing); first_rows is not used with it."""

    def __init__(self, table, first_rows=0, per_token=False):
        _dev(table, "mod table")
        assert table.dim() == 3 and table.is_contiguous()
        self.table, self.first_rows, self.per_token = table, int(first_rows), bool(per_token)
        self.mod_rows, self.k, self.c = table.shape
        self.ld = self.k * self.c

    def vec(self, j):
        return ctypes.c_void_p(self.table.data_ptr() + 2 * j * self.c)


def _mod_args(mod, rows):
    """(mod_rows, first_rows, mod_ld) of a row-kernel launch on `rows` token rows (the rule of mod_rows == rows == 2: ModTable)."""
    if mod.per_token:
        if mod.mod_rows != rows:
            raise HipLibraryError(f"per-token modulation table has {mod.mod_rows} rows; the call has {rows}")
        return mod.mod_rows, (1 if rows == 2 else 0), mod.ld
    if mod.mod_rows not in (1, 2, rows):
        raise HipLibraryError(f"modulation table has {mod.mod_rows} rows; expected 1, 2 or {rows}")
    return mod.mod_rows, mod.first_rows, mod.ld


def _batch_rows(who, x, batch):
    """(B, rows, C) of a row-kernel call on a batch that shares its table (include/fairygen_hip_rowbatch.h): x contiguous, its rows B equal
    runs of `rows`; the table arguments then count inside one element.  batch None / 1: one element, (1, all rows, C)."""
    total, c = _rows(x, "x")
    b = 1 if batch is None else int(batch)
    if b < 1 or total % b:
        raise HipLibraryError(f"{who}: batch={batch} does not divide the {total} rows of x")
    return b, total // b, c


# ------------------------------------------------------------------------------------- DiT kernels
def ln_modulate(x, mod, shift_idx, scale_idx, eps, out=None, batch=None):
    """batch=B > 1: x is B elements of rows / B rows each that share `mod`, whose rows are indexed inside the element
    (fg_ln_modulate_bf16_b; per element the bytes of the call on that element alone)."""
    b, rows, c = _batch_rows("ln_modulate", x, batch)
    out = torch.empty_like(x) if out is None else out
    if b > 1:
        _call("fg_ln_modulate_bf16_b", _ptr(x), mod.vec(shift_idx), mod.vec(scale_idx), _ptr(out), b, rows, c, eps,
              *_mod_args(mod, rows), _stream(x))
        return out
    _call("fg_ln_modulate_bf16", _ptr(x), mod.vec(shift_idx), mod.vec(scale_idx), _ptr(out), rows, c, eps,
          *_mod_args(mod, rows), _stream(x))
    return out


def ln_affine(x, w, b, eps, out=None):
    rows, c = _rows(x, "x")
    _dev(w, "w"), _dev(b, "b")
    out = torch.empty_like(x) if out is None else out
    _call("fg_ln_affine_bf16", _ptr(x), _ptr(w), _ptr(b), _ptr(out), rows, c, eps, _stream(x))
    return out


def gate_residual(x, y, mod=None, gate_idx=None, out=None, batch=None):
    """batch: as ln_modulate's (fg_gate_residual_bf16_b)."""
    b, rows, c = _batch_rows("gate_residual", x, batch)
    _rows(y, "y")
    out = torch.empty_like(x) if out is None else out
    if b > 1:
        margs = (1, 0, 0) if mod is None else _mod_args(mod, rows)
        _call("fg_gate_residual_bf16_b", _ptr(x), _ptr(y), None if mod is None else mod.vec(gate_idx), _ptr(out), b, rows, c, *margs, _stream(x))
        return out
    if mod is None:
        _call("fg_gate_residual_bf16", _ptr(x), _ptr(y), None, _ptr(out), rows, c, 1, 0, 0, _stream(x))
    else:
        _call("fg_gate_residual_bf16", _ptr(x), _ptr(y), mod.vec(gate_idx), _ptr(out), rows, c,
              *_mod_args(mod, rows), _stream(x))
    return out


def _ln_modulate_args(who, x, mod, gate_idx, shift_idx, scale_idx, norm_mod, batch=None):
    """(gate, shift, scale, affine flag, table args) of a residual + modulate(LN) launch."""
    norm_mod = mod if norm_mod is None else norm_mod
    if (norm_mod.mod_rows, norm_mod.first_rows, norm_mod.ld, norm_mod.per_token) != (mod.mod_rows, mod.first_rows, mod.ld, mod.per_token):
        raise HipLibraryError(f"{who}: gate and norm tables must share rows / first_rows / ld / per_token")
    gate = mod.vec(gate_idx) if gate_idx is not None else None
    return gate, norm_mod.vec(shift_idx), norm_mod.vec(scale_idx), 0, _mod_args(mod, _batch_rows(who, x, batch)[1])


def _ln_affine_args(x, w, b, mod, gate_idx, batch=None):
    """(gate, weight, bias, affine flag, table args) of a residual + affine LN launch."""
    _dev(w, "w"), _dev(b, "b")
    if mod is None:
        return None, _ptr(w), _ptr(b), 1, (1, 0, 0)
    return mod.vec(gate_idx), _ptr(w), _ptr(b), 1, _mod_args(mod, _batch_rows("residual_ln_affine", x, batch)[1])


def _residual_ln(x, y, eps, x_out, norm_out, gate, p1, p2, affine, margs, fp8=False, batch=None):
    """x_out = x + gate*y, then LN(x_out) with the operands p1, p2 (shift / scale vectors, or weight / bias with affine = 1): as a bf16
    row in norm_out (fg_residual_ln_bf16) or, fp8, as (e4m3 rows, scales) (fg_residual_ln_fp8_bf16).  batch=B > 1: B elements that
    share the table (fg_residual_ln_bf16_b; fp8: fg_residual_ln_fp8_bf16_b, the pair on all B * rows rows), margs counted inside one
    element."""
    b, rows, c = _batch_rows("residual_ln", x, batch)
    _rows(y, "y")
    x_out = torch.empty_like(x) if x_out is None else x_out
    if b > 1:
        if fp8:
            q, sc = _fp8_rows_out(x)
            _call("fg_residual_ln_fp8_bf16_b", _ptr(x), _ptr(y), gate, _ptr(x_out), p1, p2, _ptr(q), _ptr(sc), affine, b, rows, c, eps, *margs,
                  FP8_E4M3FN_MAX, _stream(x))
            return x_out, (q, sc)
        norm_out = torch.empty_like(x) if norm_out is None else norm_out
        _call("fg_residual_ln_bf16_b", _ptr(x), _ptr(y), gate, _ptr(x_out), p1, p2, _ptr(norm_out), affine, b, rows, c, eps, *margs, _stream(x))
        return x_out, norm_out
    if fp8:
        q, sc = _fp8_rows_out(x)
        _call("fg_residual_ln_fp8_bf16", _ptr(x), _ptr(y), gate, _ptr(x_out), p1, p2, _ptr(q), _ptr(sc), affine, rows, c, eps, *margs,
              FP8_E4M3FN_MAX, _stream(x))
        return x_out, (q, sc)
    norm_out = torch.empty_like(x) if norm_out is None else norm_out
    _call("fg_residual_ln_bf16", _ptr(x), _ptr(y), gate, _ptr(x_out), p1, p2, _ptr(norm_out), affine, rows, c, eps, *margs, _stream(x))
    return x_out, norm_out


def residual_ln_modulate(x, y, mod, gate_idx, shift_idx, scale_idx, eps, x_out=None, norm_out=None, norm_mod=None, batch=None):
    """x_out = x + gate*y (gate_idx None: x + y); norm_out = modulate(LN(x_out)).

    gate comes from `mod`, shift/scale from `norm_mod` (default: `mod`); both tables must have the same
    number of rows, first_rows and leading dimension.  batch: as ln_modulate's."""
    return _residual_ln(x, y, eps, x_out, norm_out, *_ln_modulate_args("residual_ln_modulate", x, mod, gate_idx, shift_idx, scale_idx, norm_mod, batch),
                        batch=batch)


def residual_ln_affine(x, y, w, b, eps, mod=None, gate_idx=None, x_out=None, norm_out=None, batch=None):
    """x_out = x + gate*y (mod None: x + y); norm_out = LN(x_out)*w + b.  batch: as ln_modulate's (the gate table is per element)."""
    return _residual_ln(x, y, eps, x_out, norm_out, *_ln_affine_args(x, w, b, mod, gate_idx, batch), batch=batch)


def _fp8_pair(rows, c, device):
    return (torch.empty((rows, c), dtype=torch.float8_e4m3fn, device=device),
            torch.empty((rows, 1), dtype=torch.float32, device=device))


def _fp8_rows_out(x):
    return _fp8_pair(*_rows(x, "x"), x.device)


def ln_modulate_fp8(x, mod, shift_idx, scale_idx, eps, batch=None):
    """ln_modulate whose result goes to an fp8 Linear only: (x_fp8 (rows, C) e4m3fn, scale (rows, 1) fp32) = what fp8_quant_rows
    makes of ln_modulate(x, ...), without the bf16 row in HBM.  batch: as ln_modulate's (fg_ln_modulate_fp8_bf16_b); the pair is
    still that of all the rows of x — the operand of one GEMM."""
    b, rows, c = _batch_rows("ln_modulate_fp8", x, batch)
    q, sc = _fp8_rows_out(x)
    if b > 1:
        _call("fg_ln_modulate_fp8_bf16_b", _ptr(x), mod.vec(shift_idx), mod.vec(scale_idx), _ptr(q), _ptr(sc), b, rows, c, eps,
              *_mod_args(mod, rows), FP8_E4M3FN_MAX, _stream(x))
        return q, sc
    _call("fg_ln_modulate_fp8_bf16", _ptr(x), mod.vec(shift_idx), mod.vec(scale_idx), _ptr(q), _ptr(sc), rows, c, eps,
          *_mod_args(mod, rows), FP8_E4M3FN_MAX, _stream(x))
    return q, sc


def ln_modulate_dual(x, mod, shift_idx, scale_idx, eps, out=None, batch=None):
    """ln_modulate for a norm that feeds an fp8 Linear AND a hot-loaded adapter: returns (out, (x_fp8, scale)) — the bf16 row of
    ln_modulate and the pair of ln_modulate_fp8, bit for bit, in one pass over x.  batch: as ln_modulate's (fg_ln_modulate_dual_bf16_b,
    include/fairygen_hip_lorabatch.h); the pair is that of all the rows of x."""
    b, rows, c = _batch_rows("ln_modulate_dual", x, batch)
    out = torch.empty_like(x) if out is None else _dev(out, "out")
    q, sc = _fp8_rows_out(x)
    if b > 1:
        _call("fg_ln_modulate_dual_bf16_b", _ptr(x), mod.vec(shift_idx), mod.vec(scale_idx), _ptr(out), _ptr(q), _ptr(sc), b, rows, c, eps,
              *_mod_args(mod, rows), FP8_E4M3FN_MAX, _stream(x))
        return out, (q, sc)
    _call("fg_ln_modulate_dual_bf16", _ptr(x), mod.vec(shift_idx), mod.vec(scale_idx), _ptr(out), _ptr(q), _ptr(sc), rows, c, eps,
          *_mod_args(mod, rows), FP8_E4M3FN_MAX, _stream(x))
    return out, (q, sc)


def ln_affine_dual(x, w, b, eps, out=None):
    """ln_affine (norm3) with both outputs: returns (out, (x_fp8, scale)) = (ln_affine(x, ...), fp8_quant_rows of it) in one pass."""
    rows, c = _rows(x, "x")
    _dev(w, "w"), _dev(b, "b")
    out = torch.empty_like(x) if out is None else _dev(out, "out")
    q, sc = _fp8_rows_out(x)
    _call("fg_ln_affine_dual_bf16", _ptr(x), _ptr(w), _ptr(b), _ptr(out), _ptr(q), _ptr(sc), rows, c, eps, FP8_E4M3FN_MAX, _stream(x))
    return out, (q, sc)


def residual_ln_modulate_fp8(x, y, mod, gate_idx, shift_idx, scale_idx, eps, x_out=None, norm_mod=None, batch=None):
    """residual_ln_modulate with the normalised row as (fp8 rows, scales): returns x_out, (x_fp8, scale).  batch: as ln_modulate's
    (fg_residual_ln_fp8_bf16_b)."""
    return _residual_ln(x, y, eps, x_out, None,
                        *_ln_modulate_args("residual_ln_modulate_fp8", x, mod, gate_idx, shift_idx, scale_idx, norm_mod, batch), fp8=True, batch=batch)


def residual_ln_affine_fp8(x, y, w, b, eps, mod=None, gate_idx=None, x_out=None, batch=None):
    """residual_ln_affine with the normalised row as (fp8 rows, scales): returns x_out, (x_fp8, scale).  batch: as ln_modulate's."""
    return _residual_ln(x, y, eps, x_out, None, *_ln_affine_args(x, w, b, mod, gate_idx, batch), fp8=True, batch=batch)


def _rope_tables(who, cos, sin, rows, half):
    """fg_rmsnorm_rope_bf16's table modes: (cos, sin, table_f32) checked against the row count."""
    if cos is not None and sin is None:
        _dev(cos, "rope table", torch.float32)
        if cos.shape != (rows, half, 2) or not cos.is_contiguous():
            raise HipLibraryError(f"{who}: the fp32 rope table must be ({rows}, {half}, 2) contiguous")
        return 1
    if cos is not None:
        _dev(cos, "cos", torch.float64), _dev(sin, "sin", torch.float64)
        if cos.shape != (rows, half) or not cos.is_contiguous() or sin.shape != (rows, half) or not sin.is_contiguous():
            raise HipLibraryError(f"{who}: rope tables must be ({rows}, {half}) contiguous")
    return 0


def rmsnorm_rope(x, weight, num_heads, eps, cos=None, sin=None, out=None, grouped=None, batch=None):
    """x: (..., C) possibly a column slice of a wider row-major buffer (stride(-2) = ld).

    RoPE tables: cos and sin fp64 (rows, head_dim/2) -> the reference's fp64 rotation; or cos = ONE fp32 interleaved
    (rows, head_dim/2, 2) table {cos, sin} with sin=None -> fp32 FMA rotation (the fast default of the pipeline).

    grouped=(dst, group_cols, group_stride, ld): write column block g of row r to the 1-D view
    dst[g*group_stride + r*ld : ... + group_cols] instead of a (rows, C) tensor (Ulysses send buffer); returns dst.

    batch=B > 1: x (B, rows, C) — B elements that share the RoPE table of `rows` rows, indexed by the row inside the element
    (fg_rmsnorm_rope_bf16_b); x may be a column slice with batch stride rows * ld; out (B, rows, C) dense; no grouped form."""
    _dev(x, "x"), _dev(weight, "weight")
    c = x.shape[-1]
    if batch is not None and int(batch) > 1:
        ld = _ld_rows(x, "x")
        if grouped is not None or x.shape[0] != int(batch):
            raise HipLibraryError(f"rmsnorm_rope: batch={batch} needs x (B, rows, C) and no grouped destination")
        b, rows = x.shape[:2]
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
        if out.shape != x.shape or not out.is_contiguous():
            raise HipLibraryError("rmsnorm_rope: out of a batch must be contiguous and of x's shape")
        f32tab = _rope_tables("rmsnorm_rope", cos, sin, rows, c // num_heads // 2)
        _call("fg_rmsnorm_rope_bf16_b", _ptr(x), ld, _ptr(weight), _ptr(cos), _ptr(sin), f32tab, _ptr(out), b, rows, c, num_heads, eps,
              _stream(x))
        return out
    x2 = _rows2d(x, "rmsnorm_rope")
    rows, ld = x2.shape[0], x2.stride(0)
    if grouped is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    f32tab = _rope_tables("rmsnorm_rope", cos, sin, rows, c // num_heads // 2)
    if grouped is not None:
        dst, group_cols, group_stride, out_ld = grouped
        _dev(dst, "grouped dst")
        groups = c // group_cols
        if dst.dim() != 1 or dst.stride(0) != 1 or \
                (groups - 1) * group_stride + max(rows - 1, 0) * out_ld + group_cols > dst.numel():
            raise HipLibraryError("rmsnorm_rope: grouped destination too small for the requested layout")
        _call("fg_rmsnorm_rope_grouped_bf16", _ptr(x2), ld, _ptr(weight), _ptr(cos), _ptr(sin), f32tab, _ptr(dst), rows, c,
              num_heads, eps, group_cols, group_stride, out_ld, _stream(x))
        return dst
    _call("fg_rmsnorm_rope_bf16", _ptr(x2), ld, _ptr(weight), _ptr(cos), _ptr(sin), f32tab, _ptr(out), rows, c, num_heads,
          eps, _stream(x))
    return out


def copy_groups(src, src_group_stride, src_ld, dst, dst_group_stride, dst_ld, groups, rows, cols):
    """dst[g*dst_group_stride + r*dst_ld + c] = src[g*src_group_stride + r*src_ld + c]; src / dst are 1-D views that
    start at the first element to move (strides in elements)."""
    _dev(src, "src"), _dev(dst, "dst")
    for t, gs, ld, name in ((src, src_group_stride, src_ld, "src"), (dst, dst_group_stride, dst_ld, "dst")):
        if t.dim() != 1 or t.stride(0) != 1 or (groups - 1) * gs + max(rows - 1, 0) * ld + cols > t.numel():
            raise HipLibraryError(f"copy_groups: {name} view too small for the requested layout")
    _call("fg_copy_groups_bf16", _ptr(src), src_group_stride, src_ld, _ptr(dst), dst_group_stride, dst_ld, groups, rows,
          cols, _stream(src))
    return dst


_gemm_workspace = {}      # (device, stream) -> scratch for the k-split pieces of a GEMM's last round (one fp32 tile per CU, reused)
_gemm_sched = {}          # (device, stream) -> the scheduler block of the launches on that stream (fg_gemm_sched_bytes, reset when created)
_gemm_sched_dirty = set()      # keys whose last launch raised: the block is reset before its next use


def _gemm_key(x):
    return (x.device, torch.cuda.current_stream(x.device).cuda_stream)      # concurrent streams must share neither block nor scratch


def gemm_sched_reset(sched):
    """Put a scheduler block into its initial state, stream-ordered on the current stream of its device (fg_gemm_sched_reset: one
    asynchronous memset, capturable).  Needed once before a block's first launch, and after a launch that did not run to its end."""
    _gemm_sched_check("gemm_sched_reset", sched, sched.device if isinstance(sched, torch.Tensor) else None)
    _call("fg_gemm_sched_reset", _ptr(sched), _stream(sched))
    return sched


def gemm_state(device=None):
    """(sched, workspace) for GEMM launches that are ordered with respect to each other and owned by the caller — a stream of its own,
    a captured graph: a fresh scheduler block, reset on the current stream of `device`, and k-split scratch of the matching size.
    Pass them as gemm_epilogue(..., sched=sched, workspace=workspace).  Concurrent streams need a pair each."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise HipLibraryError(f"gemm_state: expected a HIP device, got {device} (no CPU fallback)")
    lib = load()
    sched = torch.empty(lib.fg_gemm_sched_bytes(), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):      # the scratch size is one fp32 tile per CU of THAT device
        workspace = torch.empty(lib.fg_gemm_workspace_bytes(256, 256, 256), dtype=torch.uint8, device=device)
    return gemm_sched_reset(sched), workspace


def _gemm_sched_check(name, sched, device):
    if not isinstance(sched, torch.Tensor) or sched.device.type != "cuda" or (device is not None and sched.device != device):
        raise HipLibraryError(f"{name}: sched must be a tensor on the HIP device of the operands (no CPU fallback)")
    if not sched.is_contiguous() or sched.numel() * sched.element_size() < load().fg_gemm_sched_bytes():
        raise HipLibraryError(f"{name}: sched must be a contiguous block of at least {load().fg_gemm_sched_bytes()} bytes (hip.gemm_state)")


def _gemm_block(name, x, sched):
    """(block, key): the caller's block (key None), or the one kept for the current (device, stream)."""
    if sched is not None:
        _gemm_sched_check(name, sched, x.device)
        return sched, None
    key = _gemm_key(x)
    block = _gemm_sched.get(key)
    if block is None:
        block = _gemm_sched[key] = torch.empty(load().fg_gemm_sched_bytes(), dtype=torch.uint8, device=x.device)
        _gemm_sched_dirty.add(key)
    if key in _gemm_sched_dirty:
        _call("fg_gemm_sched_reset", _ptr(block), _stream(x))
        _gemm_sched_dirty.discard(key)
    return block, key


def _gemm_launch(name, key, *args):
    try:
        _call(name, *args)
    except HipLibraryError:
        if key is not None:
            _gemm_sched_dirty.add(key)
        raise


def gemm_workspace_need(m, n, k_bytes):
    """Bytes of k-split scratch that workspace=True gives an (m, n) GEMM over k_bytes operand bytes per row; 0: it runs without.  A caller
    with scratch of its own (hip.gemm_state) that wants the bits of workspace=True passes its tensor where this is positive, False elsewhere."""
    tiles = ((m + 255) // 256) * (n // 256)
    return max(load().fg_gemm_workspace_bytes(m, n, k_bytes), 0) if (k_bytes // 128 >= 96 or tiles <= 8 * 256) else 0


def _gemm_ws(x, m, n, k_bytes, workspace):
    """The k-split scratch, only where fg_gemm_* would use it: at least 96 k-steps of 128 operand bytes, or at most 8 rounds of tiles per CU
    (GemmCall::enqueue in csrc/dit_gemm.hip; 256 CUs assumed here — a spare allocation on other devices, never a missing one).  `workspace`:
    True (the scratch kept per (device, stream)), False / None (none), or the caller's own scratch tensor (hip.gemm_state)."""
    if isinstance(workspace, torch.Tensor):
        if workspace.device != x.device or not workspace.is_contiguous() or \
                workspace.numel() * workspace.element_size() < load().fg_gemm_workspace_bytes(m, n, k_bytes):
            raise HipLibraryError("gemm: the workspace tensor must be contiguous, on the operands' device, of fg_gemm_workspace_bytes (hip.gemm_state)")
        return workspace
    need = gemm_workspace_need(m, n, k_bytes) if workspace else 0
    if need <= 0:
        return None
    key = _gemm_key(x)
    ws = _gemm_workspace.get(key)
    if ws is None or ws.numel() < need:
        ws = _gemm_workspace[key] = torch.empty(need, dtype=torch.uint8, device=x.device)
    return ws


def _gemm_out(name, x, m, n, out, residual):
    if out is None:
        if residual:
            raise HipLibraryError(f"{name}: residual=True needs the contiguous residual stream as `out`")
        return torch.empty(x.shape[:-1] + (n,), dtype=torch.bfloat16, device=x.device)
    _dev(out, "out")
    if not out.is_contiguous() or out.numel() != m * n:
        raise HipLibraryError(f"{name}: `out` must be a contiguous bf16 tensor of {m} x {n} elements")
    return out


def _gemm_mode(name, residual, mod, gate_idx, act, n):
    """(mode, gate pointer, gate rows, gate ld, first rows) of the fg_gemm_* epilogue."""
    if act not in (None, "gelu_tanh") or (act is not None and residual):
        raise HipLibraryError(f"{name}: act must be None or 'gelu_tanh', and not combined with residual=True")
    if residual and mod is not None:
        if mod.mod_rows not in (1, 2) or mod.c != n or mod.per_token:
            raise HipLibraryError(f"{name}: the gate table must have 1 or 2 rows of N values (no per-token table)")
        return 2, mod.vec(gate_idx), mod.mod_rows, mod.ld, mod.first_rows
    return (3 if residual else 4 if act else 0), None, 1, n, 0


def gemm_epilogue(x, weight, bias, out=None, residual=False, mod=None, gate_idx=None, workspace=True, act=None, sched=None, workgroups=0,
                  rows_per_element=None):
    """Linear on the persistent MFMA kernel.  residual=False: out = act(x @ weight^T + bias), act None or "gelu_tanh" (applied to the
    bf16-rounded Linear output and rounded again, like nn.Linear followed by nn.GELU).  residual=True: `out` holds the residual
    stream and becomes out + gate * (x @ weight^T + bias) (gate = vector gate_idx of `mod`, or 1 when mod is None), with the
    reference's rounding points (GateModule, models/wan_video_dit.py:188-193).  workspace=False: no k-split of the last round's tiles
    (every element one k-ordered accumulation, independent of the row count); a tensor: the caller's scratch.  sched: a caller-managed
    scheduler block (hip.gemm_state; default: the block kept for the current (device, stream)); workgroups: how many workgroups to launch
    (0: one per CU) — same bits for every value.  The launch is fg_gemm_epilogue_bf16_s: nothing but stream-ordered work, capturable.
    rows_per_element=P (None: the call as it has always been, on that entry point): the rows are a batch of elements of P rows each that
    share a two-row `mod`, whose first_rows counts inside the element — row r takes gate row 0 iff r % P < first_rows
    (fg_gemm_epilogue_bf16_sp, include/fairygen_hip_gategemm.h: residual=True with a two-row table only, P >= 256 or >= the rows)."""
    _dev(x, "x"), _dev(weight, "weight"), _dev(bias, "bias")
    k = x.shape[-1]
    n = weight.shape[0]
    if weight.shape != (n, k) or not weight.is_contiguous() or bias.shape != (n,):
        raise HipLibraryError("gemm_epilogue: weight must be a contiguous (N, K) tensor, bias (N,)")
    x2 = _rows2d(x, "gemm_epilogue", "K")
    m, lda = x2.shape[0], x2.stride(0)
    out = _gemm_out("gemm_epilogue", x, m, n, out, residual)
    mode, gate, gate_rows, gate_ld, first = _gemm_mode("gemm_epilogue", residual, mod, gate_idx, act, n)
    ws = _gemm_ws(x, m, n, 2 * k, workspace)
    block, key = _gemm_block("gemm_epilogue", x, sched)
    if rows_per_element is not None:
        _gemm_launch("fg_gemm_epilogue_bf16_sp", key, _ptr(x2), lda, _ptr(weight), _ptr(bias), _ptr(out), n, m, n, k, mode, gate, gate_rows, gate_ld,
                     first, int(rows_per_element), _ptr(ws), _ptr(block), workgroups, _stream(x))
        return out
    _gemm_launch("fg_gemm_epilogue_bf16_s", key, _ptr(x2), lda, _ptr(weight), _ptr(bias), _ptr(out), n, m, n, k, mode, gate, gate_rows, gate_ld, first,
                 _ptr(ws), _ptr(block), workgroups, _stream(x))
    return out


def gemm_fp8(x_fp8, scale_a, weight_fp8, bias, out=None, residual=False, mod=None, gate_idx=None, workspace=True, act=None, lead_shape=None,
             sched=None, workgroups=0, rows_per_element=None):
    """torch._scaled_mm(x_fp8, weight_fp8.T, scale_a (rows, 1), ones (1, out), bias, out_dtype=bf16) of AutoWrappedLinear.fp8_linear
    (core/vram/layers.py:343-357) on the persistent kernel's e4m3 form, with the epilogues of gemm_epilogue.  x_fp8: (rows, K)
    float8_e4m3fn, scale_a: (rows, 1) fp32 (both from fp8_quant_rows / the fp8-output norm kernels), weight_fp8: (N, K) float8_e4m3fn.
    Returns (*lead_shape, N) bf16 (default lead_shape: (rows,)).  workspace / sched / workgroups as gemm_epilogue (fg_gemm_fp8_bf16_s);
    rows_per_element as gemm_epilogue's (fg_gemm_fp8_bf16_sp)."""
    _dev(x_fp8, "x_fp8", torch.float8_e4m3fn), _dev(weight_fp8, "weight_fp8", torch.float8_e4m3fn), _dev(bias, "bias")
    _dev(scale_a, "scale_a", torch.float32)
    if x_fp8.dim() != 2 or x_fp8.stride(1) != 1 or not weight_fp8.is_contiguous() or weight_fp8.dim() != 2:
        raise HipLibraryError("gemm_fp8: x_fp8 must be (rows, K) with a dense last dim, weight_fp8 a contiguous (N, K) tensor")
    (m, k), n = x_fp8.shape, weight_fp8.shape[0]
    if weight_fp8.shape[1] != k or bias.shape != (n,) or scale_a.numel() != m or not scale_a.is_contiguous():
        raise HipLibraryError("gemm_fp8: shapes of weight_fp8 (N, K), bias (N,), scale_a (rows, 1) do not match x_fp8 (rows, K)")
    lead = (m,) if lead_shape is None else tuple(lead_shape)
    if out is None and not residual:
        out = torch.empty(lead + (n,), dtype=torch.bfloat16, device=x_fp8.device)
    out = _gemm_out("gemm_fp8", x_fp8, m, n, out, residual)
    mode, gate, gate_rows, gate_ld, first = _gemm_mode("gemm_fp8", residual, mod, gate_idx, act, n)
    ws = _gemm_ws(x_fp8, m, n, k, workspace)
    block, key = _gemm_block("gemm_fp8", x_fp8, sched)
    if rows_per_element is not None:
        _gemm_launch("fg_gemm_fp8_bf16_sp", key, _ptr(x_fp8), x_fp8.stride(0), _ptr(scale_a), _ptr(weight_fp8), _ptr(bias), _ptr(out), n, m, n, k, mode,
                     gate, gate_rows, gate_ld, first, int(rows_per_element), _ptr(ws), _ptr(block), workgroups, _stream(x_fp8))
        return out
    _gemm_launch("fg_gemm_fp8_bf16_s", key, _ptr(x_fp8), x_fp8.stride(0), _ptr(scale_a), _ptr(weight_fp8), _ptr(bias), _ptr(out), n, m, n, k, mode, gate,
                 gate_rows, gate_ld, first, _ptr(ws), _ptr(block), workgroups, _stream(x_fp8))
    return out


LORA_RANK_TILE, LORA_MAX_RANK, LORA_MAX_GROUPS = 32, 128, 4      # fg_lora_apply_bf16: per-group rank padded to 32s, at most 128; column groups
_LORA_MODES = {"write": 0, "add": 1, "gate": 2, "gelu_tanh": 4}


def _rows2d_b(t, who, batch):
    """(2-D view, rows of one element) of a lora_apply operand on a batch of `batch` elements: (B, rows, C) — or its (B * rows, C) view —
    with a dense last dim and ONE row stride across the elements, so that it is the B * rows rows of one strided matrix: a contiguous
    tensor, or a column slice of one.  `who` prefixes the error."""
    if not isinstance(t, torch.Tensor) or t.dim() < 2 or t.stride(-1) != 1:
        raise HipLibraryError(f"{who}: expected (B, rows, C) with a dense last dim")
    if t.is_contiguous():
        t2 = t.reshape(-1, t.shape[-1])
    elif t.dim() == 2:
        t2 = t
    elif t.dim() == 3 and (t.shape[0] == 1 or t.shape[1] == 1 or t.stride(0) == t.shape[1] * t.stride(1)):
        # the stride of a dimension of size 1 says nothing: one row per element, the elements ARE the rows
        t2 = t.as_strided((t.shape[0] * t.shape[1], t.shape[2]), (t.stride(1) if t.shape[1] > 1 else t.stride(0), 1))
    else:
        raise HipLibraryError(f"{who}: batch={batch} needs the elements at one row stride — the B * rows rows of one strided matrix "
                              f"(shape {tuple(t.shape)}, strides {tuple(t.stride())})")
    if t2.shape[0] % batch:
        raise HipLibraryError(f"{who}: batch={batch} does not divide the {t2.shape[0]} rows")
    return t2, t2.shape[0] // batch


def lora_apply(x, a, b, out, groups=1, mode="add", mod=None, gate_idx=None, batch=None):
    """Hot-loaded LoRA adapters of one Linear (AutoWrappedLinear.lora_forward, core/vram/layers.py:417-436) on fg_lora_apply_bf16, in place
    on `out`: with l_g = bf16(bf16(x @ a_g^T) @ b_g^T) for each of the `groups` column groups of `out` (3: q | k | v of the fused
    projection), mode "write": out_g = l_g; "add": out_g += l_g; "gate": out_g += gate * l_g (gate = vector gate_idx of `mod`, as
    gemm_epilogue's residual form); "gelu_tanh": out_g = gelu_tanh(out_g + l_g).  x (..., K) with a dense last dim (2-D / (1, rows, K)
    when strided), out likewise with groups * Ng columns; a: (groups * R, K) the stacked alpha * A, b: (groups * Ng, R) the stacked B,
    R a multiple of 32 up to 128 (WanModel pads with zeros).
    batch=B > 1: x and out are (B, rows, .) — B elements that share a, b and `mod`, whose first_rows counts inside the element — each
    with a dense last dim and one row stride across the elements (a contiguous tensor or a column slice of one; anything else raises);
    every mode goes to fg_lora_apply_bf16_b (include/fairygen_hip_lorabatch.h): per element the bytes of the call on that element alone.
    batch None / 1: the call as it has always been."""
    nb = 1 if batch is None else int(batch)
    if nb < 1:
        raise HipLibraryError(f"lora_apply: batch={batch}")
    if nb > 1:      # the layout first: what the batch means is decided before anything else is looked at
        (x2, rows_e), (o2, rows_o) = _rows2d_b(x, "lora_apply x", nb), _rows2d_b(out, "lora_apply out", nb)
    _dev(x, "x"), _dev(a, "a"), _dev(b, "b"), _dev(out, "out")
    if mode not in _LORA_MODES:
        raise HipLibraryError(f"lora_apply: mode must be one of {sorted(_LORA_MODES)}")
    k, n = x.shape[-1], out.shape[-1]
    if not a.is_contiguous() or not b.is_contiguous() or a.dim() != 2 or b.dim() != 2:
        raise HipLibraryError("lora_apply: a and b must be contiguous matrices")
    if nb == 1:
        x2, o2 = _rows2d(x, "lora_apply x"), _rows2d(out, "lora_apply out")
    if x2.shape[0] != o2.shape[0]:
        raise HipLibraryError("lora_apply: x and out must have the same rows")
    r = b.shape[1]
    if groups < 1 or n % groups or a.shape != (groups * r, k) or b.shape[0] != n:
        raise HipLibraryError(f"lora_apply: a {tuple(a.shape)} / b {tuple(b.shape)} do not fit x (.., {k}) -> out (.., {n}) in {groups} group(s)")
    gate, gate_rows, gate_ld, first = None, 1, n, 0
    if mode == "gate":
        if mod is None or mod.mod_rows not in (1, 2) or mod.c != n or mod.per_token:
            raise HipLibraryError("lora_apply: mode 'gate' needs a ModTable of 1 or 2 rows of N values (no per-token table)")
        gate, gate_rows, gate_ld, first = mod.vec(gate_idx), mod.mod_rows, mod.ld, mod.first_rows
    if nb > 1:
        _call("fg_lora_apply_bf16_b", _ptr(x2), x2.stride(0), _ptr(a), _ptr(b), _ptr(o2), o2.stride(0), nb, rows_e, k, n // groups, r, groups,
              _LORA_MODES[mode], gate, gate_rows, gate_ld, first, _stream(x))
        return out
    _call("fg_lora_apply_bf16", _ptr(x2), x2.stride(0), _ptr(a), _ptr(b), _ptr(o2), o2.stride(0), x2.shape[0], k, n // groups, r, groups,
          _LORA_MODES[mode], gate, gate_rows, gate_ld, first, _stream(x))
    return out


def lora_fuse_ok(n, k, rank):
    """Shapes fg_lora_fuse_bf16 takes: features in 64s, rank (before padding to 32s) up to 128."""
    return n % 64 == 0 and k % 64 == 0 and 1 <= rank <= LORA_MAX_RANK


def lora_fuse(w, a_t, b, alpha=1.0, out=None, out_fp8=None):
    """One adapter folded into one Linear's weight (lora/general.py fuse_lora_to_base_model) on fg_lora_fuse_bf16:
    out = bf16(w + bf16(alpha * bf16(b @ a_t^T))).  w (N, K) with a dense last dim; out: None (in place on w) or an (N, K) view that does
    not overlap w, e.g. the rows of q in a block's fused QKV weight; out_fp8: optional (N, K) float8_e4m3fn view that receives
    out.to(float8_e4m3fn).  a_t: (K, R) = A^T, b: (N, R), both contiguous with zero columns up to R, a multiple of 32 up to 128."""
    _dev(w, "w"), _dev(a_t, "a_t"), _dev(b, "b")
    out = w if out is None else _dev(out, "out")
    if out_fp8 is not None:
        _dev(out_fp8, "out_fp8", torch.float8_e4m3fn)
    views = [w, out] + ([out_fp8] if out_fp8 is not None else [])
    if any(t.dim() != 2 or t.stride(1) != 1 or t.shape != w.shape for t in views):
        raise HipLibraryError("lora_fuse: w, out and out_fp8 must be (N, K) matrices of one shape with a dense last dim")
    n, k = w.shape
    r = b.shape[-1]
    if not a_t.is_contiguous() or not b.is_contiguous() or a_t.shape != (k, r) or b.shape != (n, r):
        raise HipLibraryError(f"lora_fuse: a_t {tuple(a_t.shape)} / b {tuple(b.shape)} must be contiguous ({k}, R) and ({n}, R)")
    _call("fg_lora_fuse_bf16", _ptr(w), w.stride(0), _ptr(out), out.stride(0), _ptr(out_fp8), out_fp8.stride(0) if out_fp8 is not None else 0,
          _ptr(a_t), _ptr(b), n, k, r, float(alpha), _stream(w))
    return out


FP8_E4M3FN_MAX = 448.0


def fp8_quant_rows(x, act=None):
    """Per-row dynamic fp8 quantisation of AutoWrappedLinear.fp8_linear (core/vram/layers.py:331-342).
    x (..., C) bf16 with dense last dim (may be a column slice, 2-D/3-D) -> (x_fp8 (rows, C) float8_e4m3fn,
    scale_a (rows, 1) fp32).  act="gelu_tanh" applies the activation (rounded to bf16) before quantising."""
    _dev(x, "x")
    c = x.shape[-1]
    x2 = _rows2d(x, "fp8_quant_rows")
    rows, ld = x2.shape[0], x2.stride(0)
    out, scale = _fp8_pair(rows, c, x.device)
    _call("fg_fp8_quant_rows_bf16", _ptr(x2), ld, _ptr(out), _ptr(scale), None, rows, c,
          {None: 0, "gelu_tanh": 1}[act], FP8_E4M3FN_MAX, _stream(x))
    return out, scale


def activation(x, kind, out=None):
    _dev(x, "x")
    if not x.is_contiguous():
        raise HipLibraryError("activation: must be contiguous")
    out = x if out is None else out
    _call("fg_act_bf16", _ptr(x), _ptr(out), x.numel(), {"silu": 0, "gelu_tanh": 1}[kind], _stream(x))
    return out


def _ld_rows(t, name):
    """(B, N, HD) with dense last dim and B stride = N*ld."""
    _dev(t, name)
    if t.dim() != 3 or t.stride(2) != 1:
        raise HipLibraryError(f"{name}: expected (B, N, H*D) with dense last dim")
    ld = t.stride(1)
    if t.shape[0] > 1 and t.stride(0) != t.shape[1] * ld:
        raise HipLibraryError(f"{name}: batch stride must be N*ld")
    return ld


_attn_workspace = {}      # (device, stream) -> scratch tensor for the split-KV partials (grown on demand, reused)


def _attn_ws(device, b, nq, nkv, num_heads, workspace, per_element=False):
    """(ws, need): the split-KV scratch of an attention launch and the bytes it wants (0: none).  ws is the tensor of the caller's list
    `workspace`, or with None the one kept for (device, current stream); either is grown here when it is smaller than need.
    per_element (the batched e4m3 forms, include/fairygen_hip_batch8.h): b shares of what ONE element's plan wants."""
    need = b * load().fg_attn_workspace_bytes(1, nq, nkv, num_heads) if per_element else load().fg_attn_workspace_bytes(b, nq, nkv, num_heads)
    if workspace is not None:
        ws = workspace[0] if workspace else None
        if need > 0 and (ws is None or ws.numel() < need or ws.device != device):
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            workspace[:] = [ws]
    else:
        key = (device, torch.cuda.current_stream(device).cuda_stream)      # concurrent streams must not share scratch
        ws = _attn_workspace.get(key)
        if need > 0 and (ws is None or ws.numel() < need):
            ws = _attn_workspace[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws, need


def _ws_args(ws, need):
    """The (scratch pointer, bytes) arguments of an attention launch from _attn_ws's pair: no pointer where the plan wants none."""
    return _ptr(ws) if need > 0 else None, need


def _softmax_scale(d, scale):
    return float(d) ** -0.5 if scale is None else float(scale)


def _flat(pairs, strides):
    """The C arguments of (tensor, element stride) pairs: the pointers, each followed by its stride for a batched (_b) entry point."""
    return [a for t, s in pairs for a in ((_ptr(t), s) if strides else (_ptr(t),))]


def pow2_softmax_scale(head_dim):
    """(scale', f) with scale' * log2(e) = the power of two next to head_dim^-0.5 * log2(e) and f = their ratio (1.0201 for d = 128):
    softmax(scale' (f q) k^T) = softmax(q k^T / sqrt(d)), and fg_attn_fwd_bf16 runs its pre-multiplied form exactly for scale'."""
    import math
    sl = float(head_dim) ** -0.5 * math.log2(math.e)
    p = 2.0 ** round(math.log2(sl))
    return p / math.log2(math.e), sl / p


def attention(q, k, v, num_heads, out=None, scale=None, workspace=None):
    """softmax(scale q k^T) v with scale = 1 / sqrt(d) by default, "b s (n d)" in and out (AttentionModule semantics).  workspace: the
    caller's split-KV scratch (a list that holds one uint8 tensor or nothing yet: grown here on demand, as the scratch kept per (device,
    stream) is, which a captured graph must not use — its key outlives the graph); same bits either way."""
    ldq, ldk, ldv = _ld_rows(q, "q"), _ld_rows(k, "k"), _ld_rows(v, "v")
    b, nq, hd = q.shape
    nkv = k.shape[1]
    d = hd // num_heads
    out = torch.empty((b, nq, hd), dtype=q.dtype, device=q.device) if out is None else out
    _call("fg_attn_fwd_bf16", _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(out), b, nq, nkv, num_heads, d, _softmax_scale(d, scale),
          *_ws_args(*_attn_ws(q.device, b, nq, nkv, num_heads, workspace)), _stream(q))
    return out


# The e4m3 attention wrappers below take one element — operands without a batch dimension, activations (1, N, H*D) — or, with a leading
# batch dimension B > 1 on all of them, a batch on the _b entry points (include/fairygen_hip_batch8.h).  `lead` is that leading shape,
# (B,) or (); one body serves both.
def _lead(b):
    return (b,) if b > 1 else ()


def attention_qk8_scratch(n, num_heads, head_dim, device, batch=1):
    """The buffers fg_attn_quant_qk_bf16 fills for (n, num_heads * head_dim) q and k: (q8, k8, sq, sk, kbar scratch).  batch > 1: the
    same five with a leading batch dimension, for the batched entry points (include/fairygen_hip_batch8.h)."""
    hd, lead = num_heads * head_dim, _lead(batch)
    return tuple(torch.empty(lead + shape, dtype=dtype, device=device) for shape, dtype in (
        ((n, hd), torch.float8_e4m3fn), ((n, hd), torch.float8_e4m3fn), ((n, num_heads), torch.float32), ((num_heads,), torch.float32),
        ((hd,), torch.float32)))


def attn_quant_qk(q, k, num_heads, bufs=None):
    """The e4m3 operands of attention_qk8 from q, k (1, N, H*128) bf16 (column slices with a leading dimension are fine): K mean-smoothed with
    one scale per head, Q with one scale per row and head (include/fairygen_hip.h).  bufs: attention_qk8_scratch's tuple, else allocated.
    A batch (B, N, H*128): fg_attn_quant_qk_bf16_b, every statistic per element."""
    ldq, ldk = _ld_rows(q, "q"), _ld_rows(k, "k")
    b, n, hd = q.shape
    if b < 1 or k.shape != q.shape:
        raise HipLibraryError(f"attn_quant_qk: q and k must both be (1, N, H*D), got {tuple(q.shape)} and {tuple(k.shape)}")
    lead = _lead(b)
    bufs = attention_qk8_scratch(n, num_heads, hd // num_heads, q.device, b) if bufs is None else bufs
    q8, k8, sq, sk, kbar = bufs
    ok = q8.shape == lead + (n, hd) and k8.shape == lead + (n, hd) and sq.shape == lead + (n, num_heads)
    if lead:
        ok = ok and sk.shape == (b, num_heads) and kbar.shape == (b, hd) and all(t.is_contiguous() for t in bufs)
        args = (_ptr(q), ldq, q.stride(0), _ptr(k), ldk, k.stride(0), *_flat([(q8, n * hd), (k8, n * hd), (sq, n * num_heads), (sk, num_heads)], True),
                _ptr(kbar), hd * 4, hd * 4, b)
    else:      # one element: sk and the key-mean scratch go by size, the scratch may be larger
        ok = ok and sk.numel() == num_heads and kbar.numel() >= hd
        args = (_ptr(q), ldq, _ptr(k), ldk, _ptr(q8), _ptr(k8), _ptr(sq), _ptr(sk), _ptr(kbar), kbar.numel() * 4)
    if not ok:
        raise HipLibraryError(f"attn_quant_qk: bufs do not match {'(B, N, H*D)' if lead else '(N, H*D)'}")
    _call("fg_attn_quant_qk_bf16_b" if lead else "fg_attn_quant_qk_bf16", *args, n, num_heads, hd // num_heads, _stream(q))
    return bufs


def attention_pv8_scratch(n, num_heads, head_dim, device, batch=1, smooth=False):
    """The buffers fg_attn_quant_vt_bf16 fills for (n, num_heads * head_dim) v: (v8t (H, 128, n rounded up to 64) e4m3, sv (H, 128) fp32,
    the statistics scratch).  batch > 1: the same three with a leading batch dimension (include/fairygen_hip_batch8.h).  smooth: the
    four of fg_attn_quant_vt_smooth_bf16 (include/fairygen_hip_smoothv.h) — its larger scratch, and mu (H, 128) fp32 behind it."""
    if head_dim != 128:
        raise HipLibraryError(f"attention_pv8_scratch: only head_dim 128 is supported (got {head_dim})")
    need = (load().fg_attn_smoothv_scratch_bytes if smooth else load().fg_attn_pv8_scratch_bytes)(n, num_heads)
    if need < 0:
        raise HipLibraryError(f"attention_pv8_scratch: {load().fg_last_error().decode()}")
    lead = _lead(batch)
    return (torch.empty(lead + (num_heads, head_dim, (n + 63) // 64 * 64), dtype=torch.float8_e4m3fn, device=device),
            torch.empty(lead + (num_heads, head_dim), dtype=torch.float32, device=device),
            torch.empty(lead + (need,), dtype=torch.uint8, device=device)) + \
        ((torch.empty(lead + (num_heads, head_dim), dtype=torch.float32, device=device),) if smooth else ())


def attn_quant_vt(v, num_heads, bufs=None, smooth=False):
    """The e4m3 V operand of the e4m3 P V form from v (1, N, H*128) bf16 (a column slice with a leading dimension is fine): one scale per
    head and channel, the bytes transposed and tile-ordered by PV8_KEY_ORDER (include/fairygen_hip_pv8.h).  bufs: attention_pv8_scratch's.
    smooth: the key mean of every channel taken out first (fg_attn_quant_vt_smooth_bf16, include/fairygen_hip_smoothv.h); bufs and the
    result are then attention_pv8_scratch(smooth=True)'s four, mu last."""
    if len(bufs if bufs is not None else ()) not in (0, 4 if smooth else 3):
        raise HipLibraryError(f"attn_quant_vt: bufs must be attention_pv8_scratch(smooth={bool(smooth)})'s")
    ldv = _ld_rows(v, "v")
    b, n, hd = v.shape
    if b < 1:
        raise HipLibraryError(f"attn_quant_vt: v must be (1, N, H*D), got {tuple(v.shape)}")
    lead, d, nkp = _lead(b), hd // num_heads, (n + 63) // 64 * 64      # a batch: the _b entry points, sv (and mu) per element
    bufs = attention_pv8_scratch(n, num_heads, d, v.device, b, smooth) if bufs is None else bufs
    v8t, sv, scratch = bufs[:3]
    mu = tuple(bufs[3:])
    if v8t.shape != lead + (num_heads, d, nkp) or any(t.shape != lead + (num_heads, d) for t in (sv,) + mu) or \
            (lead and (scratch.dim() != 2 or scratch.shape[0] != b)) or not all(t.is_contiguous() for t in (bufs if lead else (v8t,) + mu)):
        raise HipLibraryError(f"attn_quant_vt: bufs do not match {'(B, N, H*D)' if lead else '(N, H*D)'}")
    outs = _flat([(v8t, hd * nkp), (sv, hd)] + [(m, hd) for m in mu], lead)
    _call("fg_attn_quant_vt" + ("_smooth" if smooth else "") + "_bf16" + ("_b" if lead else ""), _ptr(v), ldv, *((v.stride(0),) if lead else ()),
          *outs, _ptr(scratch), *((scratch.shape[1], scratch.stride(0), b) if lead else (scratch.numel(),)), n, num_heads, d, _stream(v))
    return bufs


def attention_qk8_pre(q8, k8, sq, sk, v, num_heads, out=None, scale=None, workspace=None, pv8=False, pv8_bufs=None, smooth=False):
    """fg_attn_fwd_qk8_bf16 on operands that are quantised already (attn_quant_qk's, or the fused producers'): q8 (Nq, H*128), k8 (Nkv,
    H*128) e4m3, sq (Nq, H), sk (H), v (1, Nkv, H*128) bf16 -> (1, Nq, H*128); the model calls it with Nq = Nkv.  workspace as in
    attention().  pv8: the P V product in e4m3 too — fg_attn_quant_vt_bf16 on v (into pv8_bufs: attention_pv8_scratch's tuple, else
    allocated), then fg_attn_fwd_pv8_bf16.  smooth (with pv8): V mean-smoothed — attn_quant_vt(smooth=True), then fg_attn_fwd_pv8s_bf16
    (include/fairygen_hip_smoothv.h); pv8_bufs is then attention_pv8_scratch(smooth=True)'s."""
    if smooth and not pv8:
        raise HipLibraryError("attention_qk8_pre: smooth=True is a form of the e4m3 P V product (pv8=True)")
    ldv = _ld_rows(v, "v")
    b, nkv, hd = v.shape
    lead = _lead(b) if q8.dim() == 3 else ()      # a batch of operands (attn_quant_qk's, or the fused producers', on a batch)
    nq, d = q8.shape[-2], hd // num_heads
    if lead:
        if q8.shape != (b, nq, hd) or k8.shape != (b, nkv, hd) or sq.shape != (b, nq, num_heads) or sk.shape != (b, num_heads) or \
                not all(t.is_contiguous() for t in (q8, k8, sq, sk)):
            raise HipLibraryError(f"attention_qk8_pre: k8 and sk for v {tuple(v.shape)}, sq for q8 {tuple(q8.shape)}, all contiguous")
    elif b != 1 or q8.shape != (nq, hd) or k8.shape != (nkv, hd) or sq.shape != (nq, num_heads) or sk.numel() != num_heads:
        raise HipLibraryError(f"attention_qk8_pre: one batch element, k8 and sk for v {tuple(v.shape)}, sq for q8 {tuple(q8.shape)}")
    if pv8:
        vbufs = attn_quant_vt(v, num_heads, pv8_bufs, smooth)
        return attention_pv8_pre(q8, k8, sq, sk, vbufs[0], vbufs[1], num_heads, out=out, scale=scale, workspace=workspace,
                                 mu=vbufs[3] if smooth else None)
    out = torch.empty((b, nq, hd), dtype=v.dtype, device=v.device) if out is None else out
    ws = _attn_ws(v.device, b, nq, nkv, num_heads, workspace, per_element=bool(lead))
    _call("fg_attn_fwd_qk8_bf16" + ("_b" if lead else ""), *_flat([(q8, nq * hd), (k8, nkv * hd), (sq, nq * num_heads), (sk, num_heads)], lead),
          _ptr(v), ldv, *((v.stride(0),) if lead else ()), *_flat([(out, nq * hd)], lead), *lead, nq, nkv, num_heads, d, _softmax_scale(d, scale),
          *_ws_args(*ws), _stream(v))
    return out


def _operands8(who, q8, k8, sq, sk, v8t, sv, num_heads, mu):
    """(B or None, Nq, H*D, Nkv, D) of six ready e4m3 operands (and mu, or None, shaped like sv): one element's, or with a leading batch
    dimension on all of them a batch's, each then contiguous."""
    if mu is not None and (mu.shape != sv.shape or mu.dtype != torch.float32 or not mu.is_contiguous()):
        raise HipLibraryError(f"{who}: mu must be fp32, contiguous and shaped like sv {tuple(sv.shape)}")
    lead = tuple(q8.shape[:1]) if q8.dim() == 3 else ()
    (nq, hd), nkv = q8.shape[-2:], k8.shape[-2]
    d = hd // num_heads
    ok = k8.shape == lead + (nkv, hd) and sq.shape == lead + (nq, num_heads) and v8t.shape == lead + (num_heads, d, (nkv + 63) // 64 * 64)
    if lead:
        ok = ok and sk.shape == lead + (num_heads,) and sv.shape == lead + (num_heads, d) and all(t.is_contiguous() for t in (q8, k8, sq, sk, v8t, sv))
    else:      # one element: sk and sv go by size (a token shard hands them over flat)
        ok = ok and sk.numel() == num_heads and sv.numel() == hd and v8t.is_contiguous()
    if not ok:
        raise HipLibraryError(f"{who}: k8, sq, sk, v8t, sv do not match " + (f"the batch q8 {tuple(q8.shape)} and {nkv} keys (all contiguous)"
                                                                              if lead else f"q8 {tuple(q8.shape)} and {nkv} keys"))
    return (lead[0] if lead else None), nq, hd, nkv, d


def _fwd8(base, q8, k8, sq, sk, v8t, sv, mu, out, b, nq, hd, nkv, num_heads, tail):
    """One launch of fg_attn_fwd_<base>[s]_bf16[_b]: s with mu, _b with a batch b (every operand then followed by its element stride);
    tail: what follows the head size — the scale, and the workspace pair of the kernels that take one."""
    ops = [(q8, nq * hd), (k8, nkv * hd), (sq, nq * num_heads), (sk, num_heads), (v8t, v8t.stride(0)), (sv, hd)] + \
        ([(mu, hd)] if mu is not None else []) + [(out, nq * hd)]
    _call(f"fg_attn_fwd_{base}{'s' if mu is not None else ''}_bf16{'_b' if b else ''}", *_flat(ops, b), *((b,) if b else ()), nq, nkv, num_heads,
          hd // num_heads, *tail, _stream(q8))
    return out


def attention_pv8_pre(q8, k8, sq, sk, v8t, sv, num_heads, out=None, scale=None, workspace=None, mu=None):
    """fg_attn_fwd_pv8_bf16 on operands that are ALL ready: q8 (Nq, H*128), k8 (Nkv, H*128) e4m3, sq (Nq, H), sk (H), v8t (H, 128, Nkv
    rounded up to 64) e4m3 and sv (H, 128) as attn_quant_vt or attn_shard8_vt left them -> (1, Nq, H*128) bf16.  Nq need not be Nkv (a
    token shard's queries against all keys).  workspace as in attention().  With a leading batch dimension on all six: the batched form.
    mu: attn_quant_vt(smooth=True)'s key means of v, shaped like sv — fg_attn_fwd_pv8s_bf16 / _b, which add them to the output rows."""
    b, nq, hd, nkv, d = _operands8("attention_pv8_pre", q8, k8, sq, sk, v8t, sv, num_heads, mu)
    out = torch.empty((b or 1, nq, hd), dtype=torch.bfloat16, device=q8.device) if out is None else out
    ws = _attn_ws(q8.device, b or 1, nq, nkv, num_heads, workspace, per_element=b is not None)
    return _fwd8("pv8", q8, k8, sq, sk, v8t, sv, mu, out, b, nq, hd, nkv, num_heads, (_softmax_scale(d, scale), *_ws_args(*ws)))


def attention_cross8_max_kv():
    """The most keys attention_cross8_pre takes (fg_attn_cross8_max_kv: 640, what 160 KiB of LDS hold of a head's K8 and V8^T)."""
    return int(load().fg_attn_cross8_max_kv())


def attention_cross8_pre(q8, k8, sq, sk, v8t, sv, num_heads, out=None, scale=None, mu=None):
    """fg_attn_fwd_cross8_bf16 (include/fairygen_hip_cross8.h) on attention_pv8_pre's operands, Nkv <= attention_cross8_max_kv(): every
    workgroup keeps its head's K8 and V8^T in LDS and walks many query blocks against them.  One launch, no workspace; the bits of
    attention_pv8_pre without one.  With a leading batch dimension on all six: fg_attn_fwd_cross8_bf16_b, each workgroup on ONE element.
    mu: attn_quant_vt(smooth=True)'s key means of v, shaped like sv, with that call's v8t and sv — fg_attn_fwd_cross8s_bf16 / _b
    (include/fairygen_hip_cross8s.h), which add them to the output rows: the bits of attention_pv8_pre(mu=) without a workspace."""
    b, nq, hd, nkv, d = _operands8("attention_cross8_pre", q8, k8, sq, sk, v8t, sv, num_heads, mu)
    out = torch.empty((b or 1, nq, hd), dtype=torch.bfloat16, device=q8.device) if out is None else out
    return _fwd8("cross8", q8, k8, sq, sk, v8t, sv, mu, out, b, nq, hd, nkv, num_heads, (_softmax_scale(d, scale),))


# ---- the e4m3 operands of a token shard (include/fairygen_hip_shard8.h); with a leading batch dimension B > 1 on their tensors the same
# wrappers take the batched entry points of include/fairygen_hip_shard8b.h (the stacked CFG forward on a shard); B = 1 is the single form
def attn_shard8_record_bytes(c):
    need = load().fg_attn_shard8_record_bytes(c)
    if need < 0:
        raise HipLibraryError(f"attn_shard8_record_bytes: {load().fg_last_error().decode()}")
    return need


def attn_shard8_neutral_record(c, device, batch=1):
    """The record of a rank without rows (sum 0, minimum +inf, maximum -inf, |v| maximum 0) as (20 * c,) uint8 on `device`; batch=B > 1:
    B of them, (B, 20 * c)."""
    rec = torch.zeros(attn_shard8_record_bytes(c), dtype=torch.uint8)
    rec[8 * c:12 * c].view(torch.float32).fill_(float("inf"))
    rec[12 * c:16 * c].view(torch.float32).fill_(float("-inf"))
    return (rec.expand(batch, -1).contiguous() if batch > 1 else rec).to(device)


def _shard8_stats(smooth, partials, rows, num_heads, v, record):
    """attn_shard8_stats / attn_shard8s_stats: one element (partials flat, v (1, rows, C)), or B > 1 (partials (B, bytes), v (B, rows, C))."""
    who = "attn_shard8s_stats" if smooth else "attn_shard8_stats"
    c = num_heads * 128
    _dev(partials, "partials", torch.uint8)
    lead = (partials.shape[0],) if partials.dim() == 2 and partials.shape[0] > 1 else ()
    b = lead[0] if lead else 1
    unit = (attn_shard8s_record_bytes if smooth else attn_shard8_record_bytes)(c)
    record = torch.empty(lead + (unit,), dtype=torch.uint8, device=partials.device) if record is None else record
    scratch, ldv, need = None, 0, 0
    if v is not None:
        ldv = _ld_rows(v, "v")
        if v.shape != (b, rows, c):
            raise HipLibraryError(f"{who}: v must be ({b}, {rows}, {c}), got {tuple(v.shape)}")
        need = (load().fg_attn_shard8s_scratch_bytes if smooth else load().fg_attn_shard8_scratch_bytes)(rows, c)
        if need < 0:
            raise HipLibraryError(f"{who}: {load().fg_last_error().decode()}")
        scratch = torch.empty(lead + (need,), dtype=torch.uint8, device=v.device)
    if lead:
        if partials.stride(1) != 1 or record.shape != (b, unit) or not record.is_contiguous():
            raise HipLibraryError(f"{who}: a batch takes partials (B, bytes) and records (B, {unit}) contiguous")
        _call(f"fg_attn_shard8{'s' if smooth else ''}_stats_b", _ptr(partials), partials.shape[1], partials.stride(0), _ptr(v), ldv,
              v.stride(0) if v is not None else 0, _ptr(record), record.numel(), _ptr(scratch), need, need, b, rows, num_heads, 128,
              _stream(partials))
        return record
    _call(f"fg_attn_shard8{'s' if smooth else ''}_stats", _ptr(partials), partials.numel(), _ptr(v), ldv, _ptr(record), record.numel(), _ptr(scratch),
          need, rows, num_heads, 128, _stream(partials))
    return record


def attn_shard8_stats(partials, rows, num_heads, v=None, record=None):
    """This rank's statistics record from rmsnorm_rope_kstats's partials of its `rows` local k rows and, for the e4m3 P V form, its v
    (1, rows, H*128) bf16 (a column slice is fine; None: the |v| maxima are written as 0) -> (20 * H * 128,) uint8.  A batch — partials
    (B, bytes), v (B, rows, H*128) — gives (B, 20 * H * 128) from one launch sequence (fg_attn_shard8_stats_b)."""
    return _shard8_stats(False, partials, rows, num_heads, v, record)


def _shard8_quant(smooth, records, n, k, num_heads, v, k8, v8):
    """attn_shard8_quant / attn_shard8s_quant: k (1, rows, C) with records (W, bytes), or k (B, rows, C), B > 1, with records (W, B, bytes)."""
    who = "attn_shard8s_quant" if smooth else "attn_shard8_quant"
    ldk = _ld_rows(k, "k")
    b, rows, hd = k.shape
    _dev(records, "records", torch.uint8)
    lead = _lead(b)
    if b < 1 or hd != num_heads * 128 or records.dim() != 2 + len(lead) or not records.is_contiguous() or (lead and records.shape[1] != b):
        raise HipLibraryError(f"{who}: k must be (B, rows, H*128) and records (W, bytes) — (W, B, bytes) with B > 1 — got {tuple(k.shape)}, "
                              f"{tuple(records.shape)}")
    f8, dev = torch.float8_e4m3fn, k.device
    k8 = torch.empty(lead + (rows, hd), dtype=f8, device=dev) if k8 is None else k8
    sk, kbar = torch.empty(lead + (num_heads,), dtype=torch.float32, device=dev), torch.empty(lead + (hd,), dtype=torch.float32, device=dev)
    sv = mu = None
    ldv = 0
    if v is not None:
        ldv = _ld_rows(v, "v")
        v8 = torch.empty(lead + (rows, hd), dtype=f8, device=dev) if v8 is None else v8
        sv = torch.empty(lead + (num_heads, 128), dtype=torch.float32, device=dev)
        mu = torch.empty(lead + (num_heads, 128), dtype=torch.float32, device=dev) if smooth else None
        if v.shape != k.shape or v8.shape != lead + (rows, hd) or not v8.is_contiguous():
            raise HipLibraryError(f"{who}: v and v8 must match k")
    if k8.shape != lead + (rows, hd) or not k8.is_contiguous():
        raise HipLibraryError(f"{who}: k8 must be {'(B, ' if lead else '('}rows, H*128) contiguous")
    outs = (_ptr(k8), _ptr(v8) if v is not None else None, _ptr(sk), _ptr(kbar), _ptr(sv)) + ((_ptr(mu),) if smooth else ())
    if lead:
        _call(f"fg_attn_shard8{'s' if smooth else ''}_quant_b", _ptr(records), records.numel(), records.shape[0], n, _ptr(k), ldk, k.stride(0),
              _ptr(v), ldv, v.stride(0) if v is not None else 0, *outs, b, rows, num_heads, 128, _stream(k))
    else:
        _call(f"fg_attn_shard8{'s' if smooth else ''}_quant", _ptr(records), records.numel(), records.shape[0], n, _ptr(k), ldk, _ptr(v), ldv,
              *outs, rows, num_heads, 128, _stream(k))
    return (k8, (v8 if v is not None else None), sk, kbar, sv) + ((mu,) if smooth else ())


def attn_shard8_quant(records, n, k, num_heads, v=None, k8=None, v8=None):
    """The gathered records (W, 20 * H * 128) uint8 and the key count n of all ranks -> the scales every rank agrees on, and this rank's
    rows converted: k (1, rows, H*128) bf16 -> k8 (rows, H*128) e4m3; v likewise -> v8 ROW-MAJOR (None without v).  Returns (k8, v8, sk
    (H), kbar (H*128), sv (H, 128) or None).  A batch — k, v (B, rows, H*128), records (W, B, 20 * H * 128) — gives the five with a leading
    B from one launch sequence (fg_attn_shard8_quant_b), every statistic per element."""
    return _shard8_quant(False, records, n, k, num_heads, v, k8, v8)


def attn_shard8_vt(v8, num_heads, v8t=None):
    """The gathered v8 (N, H*128) row-major e4m3 -> v8t (H, 128, N rounded up to 64) in the tile order of PV8_KEY_ORDER, padding zero.
    A batch: v8 (B, N, H*128) with dense rows whose elements may lie further apart than N rows (a gathered slab of W * chunk rows per
    element is read where it is) -> v8t (B, H, 128, Nkp) from one launch (fg_attn_shard8_vt_b)."""
    if v8.dim() == 3 and v8.shape[0] > 1:
        b, n, hd = v8.shape
        if v8.dtype not in (torch.float8_e4m3fn, torch.uint8) or v8.device.type != "cuda" or hd != num_heads * 128 or v8.stride(2) != 1 or \
                v8.stride(1) != hd:
            raise HipLibraryError("attn_shard8_vt: a batch of v8 must be (B, N, H*128) e4m3 on a HIP device with dense rows")
        shape = (b, num_heads, 128, (n + 63) // 64 * 64)
        v8t = torch.empty(shape, dtype=torch.float8_e4m3fn, device=v8.device) if v8t is None else v8t
        if v8t.shape != shape or not v8t.is_contiguous():
            raise HipLibraryError(f"attn_shard8_vt: v8t must be {shape} contiguous")
        _call("fg_attn_shard8_vt_b", _ptr(v8), v8.stride(0), _ptr(v8t), b, n, num_heads, 128, _stream(v8))
        return v8t
    if v8.dtype not in (torch.float8_e4m3fn, torch.uint8) or v8.device.type != "cuda" or v8.dim() != 2 or not v8.is_contiguous() or \
            v8.shape[1] != num_heads * 128:
        raise HipLibraryError("attn_shard8_vt: v8 must be a contiguous (N, H*128) e4m3 tensor on a HIP device")
    n = v8.shape[0]
    shape = (num_heads, 128, (n + 63) // 64 * 64)
    v8t = torch.empty(shape, dtype=torch.float8_e4m3fn, device=v8.device) if v8t is None else v8t
    if v8t.shape != shape or not v8t.is_contiguous():
        raise HipLibraryError(f"attn_shard8_vt: v8t must be {shape} contiguous")
    _call("fg_attn_shard8_vt", _ptr(v8), _ptr(v8t), n, num_heads, 128, _stream(v8))
    return v8t


# ---- the same with V mean-smoothed (include/fairygen_hip_shard8s.h)
def attn_shard8s_record_bytes(c):
    need = load().fg_attn_shard8s_record_bytes(c)
    if need < 0:
        raise HipLibraryError(f"attn_shard8s_record_bytes: {load().fg_last_error().decode()}")
    return need


def attn_shard8s_neutral_record(c, device, batch=1):
    """The record of a rank without rows (sums 0, minima +inf, maxima -inf, of k and of v) as (32 * c,) uint8 on `device`; batch=B > 1:
    B of them, (B, 32 * c)."""
    rec = torch.zeros(attn_shard8s_record_bytes(c), dtype=torch.uint8)
    for at in (8 * c, 24 * c):
        rec[at:at + 4 * c].view(torch.float32).fill_(float("inf"))
        rec[at + 4 * c:at + 8 * c].view(torch.float32).fill_(float("-inf"))
    return (rec.expand(batch, -1).contiguous() if batch > 1 else rec).to(device)


def attn_shard8s_stats(partials, rows, num_heads, v, record=None):
    """This rank's statistics record from rmsnorm_rope_kstats's partials of its `rows` local k rows and its v (1, rows, H*128) bf16 (a
    column slice is fine) -> (32 * H * 128,) uint8: per channel the fp64 sum, the minimum and the maximum of k, then of v.  A batch:
    attn_shard8_stats's, (B, 32 * H * 128) (fg_attn_shard8s_stats_b)."""
    if v is None:
        raise HipLibraryError("attn_shard8s_stats: v is required (the record exists for the smoothing form)")
    return _shard8_stats(True, partials, rows, num_heads, v, record)


def attn_shard8s_quant(records, n, k, num_heads, v, k8=None, v8=None):
    """The gathered records (W, 32 * H * 128) uint8 and the key count n of all ranks -> the scales every rank agrees on, and this rank's
    rows converted: k (1, rows, H*128) bf16 -> k8 (rows, H*128) e4m3; v likewise -> v8 = e4m3((v - mu) / sv) ROW-MAJOR.  Returns (k8, v8,
    sk (H), kbar (H*128), sv (H, 128), mu (H, 128)): attn_shard8_vt(v8 of all ranks), sv and mu are attention_pv8_pre(mu=)'s.  A batch:
    attn_shard8_quant's, records (W, B, 32 * H * 128) (fg_attn_shard8s_quant_b)."""
    if v is None:
        raise HipLibraryError("attn_shard8s_quant: v is required")
    return _shard8_quant(True, records, n, k, num_heads, v, k8, v8)


def attention_qk8(q, k, v, num_heads, out=None, scale=None, workspace=None, bufs=None, pv8=False, pv8_bufs=None, smooth=False):
    """attention() for self-attention of one batch element with the e4m3 Q K^T product (the reference's sageattn branch,
    models/wan_video_dit.py:48-52): fg_attn_quant_qk_bf16, then fg_attn_fwd_qk8_bf16.  workspace as in attention(); bufs: the quantised
    operands' buffers when the caller owns them (a captured step), else allocated per call.  pv8 / pv8_bufs / smooth: attention_qk8_pre's."""
    if v.shape != q.shape:
        raise HipLibraryError(f"attention_qk8: self-attention only, q, k, v of one shape (got v {tuple(v.shape)})")
    q8, k8, sq, sk, _ = attn_quant_qk(q, k, num_heads, bufs)
    return attention_qk8_pre(q8, k8, sq, sk, v, num_heads, out=out, scale=scale, workspace=workspace, pv8=pv8, pv8_bufs=pv8_bufs, smooth=smooth)


def attention_qk8_fused_scratch(n, num_heads, head_dim, device, batch=1):
    """The buffers of the fused producers for (n, num_heads * head_dim) q and k: attention_qk8_scratch's five (q8, k8, sq, sk, the key
    mean) and the key-statistics partials rmsnorm_rope_kstats hands to attn_quant_k."""
    return attention_qk8_scratch(n, num_heads, head_dim, device, batch) + \
        (torch.empty(_lead(batch) + (_kstats_bytes("attention_qk8_fused_scratch", n, num_heads * head_dim),), dtype=torch.uint8, device=device),)


def _kstats_bytes(who, rows, c):
    need = load().fg_attn_qk8_fused_scratch_bytes(rows, c)
    if need < 0:
        raise HipLibraryError(f"{who}: {load().fg_last_error().decode()}")
    return need


def _norm_rows(x, who):
    """(lead, rows, row stride) of the input of a fused producer: plain rows (_rows2d), or with B > 1 elements (B, rows, C) the rows of
    each (_ld_rows) — the _b entry points, the RoPE table per element."""
    if x.dim() == 3 and x.shape[0] > 1:
        return (x.shape[0],), x.shape[1], _ld_rows(x, "x")
    x2 = _rows2d(x, who)
    return (), x2.shape[0], x2.stride(0)


def rmsnorm_rope_q8(x, weight, num_heads, eps, cos=None, sin=None, q8=None, sq=None):
    """rmsnorm_rope (head_dim 128, plain rows) whose row leaves as the e4m3 q operand of attention_qk8_pre: (q8 (rows, C), sq (rows,
    num_heads)), the bytes attn_quant_qk makes of rmsnorm_rope's output, which is never written.  A batch (B, rows, C): both with a
    leading B (fg_rmsnorm_rope_q8_bf16_b)."""
    _dev(x, "x"), _dev(weight, "weight")
    c = x.shape[-1]
    lead, rows, ld = _norm_rows(x, "rmsnorm_rope_q8")
    f32tab = _rope_tables("rmsnorm_rope_q8", cos, sin, rows, c // num_heads // 2)
    q8 = torch.empty(lead + (rows, c), dtype=torch.float8_e4m3fn, device=x.device) if q8 is None else q8
    sq = torch.empty(lead + (rows, num_heads), dtype=torch.float32, device=x.device) if sq is None else sq
    if q8.shape != lead + (rows, c) or sq.shape != lead + (rows, num_heads) or not q8.is_contiguous() or not sq.is_contiguous():
        raise HipLibraryError(f"rmsnorm_rope_q8: q8 must be {'(B, rows, C), sq (B, ' if lead else '(rows, C), sq ('}rows, num_heads), contiguous")
    _call("fg_rmsnorm_rope_q8_bf16" + ("_b" if lead else ""), _ptr(x), ld, _ptr(weight), _ptr(cos), _ptr(sin), f32tab, _ptr(q8), _ptr(sq), *lead,
          rows, c, num_heads, eps, _stream(x))
    return q8, sq


def rmsnorm_rope_kstats(x, weight, num_heads, eps, cos=None, sin=None, out=None, partials=None):
    """rmsnorm_rope (head_dim 128, plain rows) that also leaves the key statistics of the rows it wrote: (k, partials), k rmsnorm_rope's
    bytes, partials (attention_qk8_fused_scratch's last buffer, else allocated) for attn_quant_k.  A batch (B, rows, C): one partials
    block per element, (B, bytes) (fg_rmsnorm_rope_kstats_bf16_b)."""
    _dev(x, "x"), _dev(weight, "weight")
    c = x.shape[-1]
    lead, rows, ld = _norm_rows(x, "rmsnorm_rope_kstats")
    f32tab = _rope_tables("rmsnorm_rope_kstats", cos, sin, rows, c // num_heads // 2)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    if out.shape != x.shape or not out.is_contiguous():
        raise HipLibraryError("rmsnorm_rope_kstats: out must be contiguous and of x's shape")
    if partials is None:
        partials = torch.empty(lead + (_kstats_bytes("rmsnorm_rope_kstats", rows, c),), dtype=torch.uint8, device=x.device)
    if lead and (partials.dim() != 2 or partials.shape[0] != lead[0] or partials.stride(1) != 1):
        raise HipLibraryError("rmsnorm_rope_kstats: partials of a batch must be (B, bytes)")
    _call("fg_rmsnorm_rope_kstats_bf16" + ("_b" if lead else ""), _ptr(x), ld, _ptr(weight), _ptr(cos), _ptr(sin), f32tab, _ptr(out), _ptr(partials),
          *((partials.shape[1], partials.stride(0)) + lead if lead else (partials.numel(),)), rows, c, num_heads, eps, _stream(x))
    return out, partials


def attn_quant_k(k, partials, num_heads, k8=None, sk=None, kbar=None):
    """The e4m3 k operand from rmsnorm_rope_kstats's pair: k (1, N, H*128) bf16 -> (k8 (N, H*128), sk (H), the key mean (H*128)).  A batch
    (B, N, H*128) with its (B, bytes) partials: the three with a leading B (fg_attn_quant_k_bf16_b)."""
    ldk = _ld_rows(k, "k")
    b, n, hd = k.shape
    if b < 1:
        raise HipLibraryError(f"attn_quant_k: k must be (1, N, H*D), got {tuple(k.shape)}")
    lead = _lead(b)
    k8 = torch.empty(lead + (n, hd), dtype=torch.float8_e4m3fn, device=k.device) if k8 is None else k8
    sk = torch.empty(lead + (num_heads,), dtype=torch.float32, device=k.device) if sk is None else sk
    kbar = torch.empty(lead + (hd,), dtype=torch.float32, device=k.device) if kbar is None else kbar
    if lead:
        if k8.shape != (b, n, hd) or sk.shape != (b, num_heads) or kbar.shape != (b, hd) or partials.dim() != 2 or partials.shape[0] != b or \
                not all(t.is_contiguous() for t in (k8, sk, kbar)):
            raise HipLibraryError("attn_quant_k: k8, sk, kbar, partials do not match (B, N, H*D)")
        _call("fg_attn_quant_k_bf16_b", _ptr(k), ldk, k.stride(0), _ptr(partials), partials.shape[1], partials.stride(0),
              *_flat([(k8, n * hd), (sk, num_heads), (kbar, hd)], True), b, n, num_heads, hd // num_heads, _stream(k))
        return k8, sk, kbar
    if k8.shape != (n, hd) or sk.numel() != num_heads or kbar.numel() < hd:      # one element: sk and the key mean go by size
        raise HipLibraryError("attn_quant_k: k8, sk, kbar do not match (N, H*D)")
    _call("fg_attn_quant_k_bf16", _ptr(k), ldk, _ptr(partials), partials.numel(), _ptr(k8), _ptr(sk), _ptr(kbar), n, num_heads, hd // num_heads,
          _stream(k))
    return k8, sk, kbar


def cfg_euler(latents, posi, nega, cfg_scale, dsigma, out=None):
    _dev(latents, "latents"), _dev(posi, "posi")
    assert latents.is_contiguous() and posi.is_contiguous() and (nega is None or nega.is_contiguous())
    out = torch.empty_like(latents) if out is None else out
    _call("fg_cfg_euler_bf16", _ptr(latents), _ptr(posi), _ptr(nega), _ptr(out), latents.numel(), float(cfg_scale),
          float(dsigma), _stream(latents))
    return out


def cfg_euler_dev(latents, posi, nega, cfg_scale, dsigma_table, step, first=None, out=None):
    """cfg_euler for a step that is captured once and replayed (fg_cfg_euler_dev_bf16): dsigma = dsigma_table[step], read on the device —
    dsigma_table (steps,) fp32, step one int32 element on the device, 0 <= step < steps (the caller's to keep).  first: the (1, C, 1, H, W)
    conditioning latent of latents (1, C, T, H, W); the result then has it as frame 0, as latents[:, :, 0:1] = first after cfg_euler."""
    _dev(latents, "latents"), _dev(posi, "posi"), _dev(dsigma_table, "dsigma_table", torch.float32), _dev(step, "step", torch.int32)
    out = torch.empty_like(latents) if out is None else _dev(out, "out")
    if nega is not None:
        _dev(nega, "nega")
    if any(t.device != latents.device for t in (posi, dsigma_table, step, out) + (() if nega is None else (nega,)) + (() if first is None else (first,))):
        raise HipLibraryError("cfg_euler_dev: all operands must be on one HIP device")
    if any(not t.is_contiguous() or t.shape != latents.shape for t in (latents, posi, out) + (() if nega is None else (nega,))):
        raise HipLibraryError("cfg_euler_dev: latents, posi, nega and out must be contiguous tensors of one shape")
    if dsigma_table.dim() != 1 or not dsigma_table.is_contiguous() or dsigma_table.numel() < 1 or step.numel() != 1:
        raise HipLibraryError("cfg_euler_dev: dsigma_table must be a contiguous (steps,) fp32 tensor and step one int32 element")
    first_n = frame_stride = 0
    if first is not None:
        _dev(first, "first")
        if latents.dim() != 5 or latents.shape[0] != 1 or first.shape != latents.shape[:2] + (1,) + latents.shape[3:] or not first.is_contiguous():
            raise HipLibraryError(f"cfg_euler_dev: first must be the contiguous (1, C, 1, H, W) frame of latents (1, C, T, H, W), got {tuple(first.shape)} "
                                  f"for {tuple(latents.shape)}")
        first_n = latents.shape[3] * latents.shape[4]
        frame_stride = latents.shape[2] * first_n
    _call("fg_cfg_euler_dev_bf16", _ptr(latents), _ptr(posi), _ptr(nega), _ptr(out), latents.numel(), float(cfg_scale), _ptr(dsigma_table),
          _ptr(step), _ptr(first), first_n, frame_stride, _stream(latents))
    return out


# ------------------------------------------------------------------------------------- VAE kernels
def vae_rmsnorm_silu(x, gamma, silu=True, out=None):
    pixels, c = _rows(x, "x")
    _dev(gamma, "gamma")
    out = torch.empty_like(x) if out is None else out
    _call("fg_vae_rmsnorm_silu_bf16", _ptr(x), _ptr(gamma), _ptr(out), pixels, c, int(silu), _stream(x))
    return out


def conv_pack_weight(w):
    """(Cout,Cin,kt,kh,kw) or (Cout,Cin,kh,kw) bf16 -> packed buffer for conv3d_cl."""
    _dev(w, "w")
    w = w.contiguous()
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin, kt, kh, kw = w.shape
    nbytes = load().fg_conv_packed_bytes(cout, cin, kt, kh, kw)
    packed = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    _call("fg_conv_pack_weight_bf16", _ptr(w), _ptr(packed), cout, cin, kt, kh, kw, _stream(w))
    return packed


def conv3d_cl(x, w_packed, bias, cout, kt, ks, residual=None, upsample2x=False, time_interleave=False, out=None,
              downsample2x=False):
    """x (T + kt-1, Hin, Win, Cin) channels-last, the first kt-1 frames being the causal history (feature cache)
    -> (T,H,W,Cout) [or (2T,H,W,Cout/2) with time_interleave]."""
    _dev(x, "x"), _dev(w_packed, "w_packed"), _dev(bias, "bias")
    assert x.dim() == 4 and x.is_contiguous() and x.shape[0] > kt - 1
    t, hin, win, cin = x.shape[0] - (kt - 1), x.shape[1], x.shape[2], x.shape[3]
    assert not (upsample2x and downsample2x)
    h, w = (hin * 2, win * 2) if upsample2x else ((hin // 2, win // 2) if downsample2x else (hin, win))
    oshape = (2 * t, h, w, cout // 2) if time_interleave else (t, h, w, cout)
    out = torch.empty(oshape, dtype=x.dtype, device=x.device) if out is None else out
    assert tuple(out.shape) == oshape and out.is_contiguous()
    if residual is not None:
        _dev(residual, "residual")
        assert tuple(residual.shape) == oshape and residual.is_contiguous()
    _call("fg_conv3d_cl_bf16", _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(out), t, h, w,
          cin, cout, kt, ks, 1 if upsample2x else (2 if downsample2x else 0), int(time_interleave), _stream(x))
    return out


def conv_up2_phase_ok(cin, kt, ks):
    """Whether the nearest-2x upsample conv of these sizes has the phase form (include/fairygen_hip_up2phase.h): the 1x3x3 conv, Cin % 64 == 0."""
    return kt == 1 and ks == 3 and cin % 64 == 0


def conv_up2_phase_pack_weight(w):
    """(Cout,Cin,1,3,3) or (Cout,Cin,3,3) bf16 -> the 16 summed tap matrices (4 phases x 2x2 taps) for conv3d_up2_phase."""
    _dev(w, "w")
    w = w.contiguous()
    if w.dim() == 5:
        assert w.shape[2] == 1
        w = w.squeeze(2)
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    nbytes = load().fg_conv_up2phase_packed_bytes(cout, cin)
    if nbytes <= 0:
        raise HipLibraryError(f"conv_up2_phase_pack_weight: no phase form for Cout={cout} Cin={cin}")
    packed = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    _call("fg_conv_up2phase_pack_bf16", _ptr(w), _ptr(packed), cout, cin, _stream(w))
    return packed


def conv3d_up2_phase(x, w_phase, bias, cout, kt=1, ks=3, out=None):
    """x (T, Hin, Win, Cin) channels-last -> (T, 2 Hin, 2 Win, Cout): conv3d_cl(upsample2x=True) as four 2x2 convs over x, one per
    output phase, on conv_up2_phase_pack_weight's weights."""
    _dev(x, "x"), _dev(w_phase, "w_phase"), _dev(bias, "bias")
    assert x.dim() == 4 and x.is_contiguous()
    t, hin, win, cin = x.shape
    oshape = (t, 2 * hin, 2 * win, cout)
    out = torch.empty(oshape, dtype=x.dtype, device=x.device) if out is None else out
    assert tuple(out.shape) == oshape and out.is_contiguous()
    if w_phase.numel() * 2 != load().fg_conv_up2phase_packed_bytes(cout, cin):
        raise HipLibraryError(f"conv3d_up2_phase: w_phase is not the phase-packed weight of a ({cout}, {cin}, 1, 3, 3) conv")
    _call("fg_conv3d_up2_phase_bf16", _ptr(x), _ptr(w_phase), _ptr(bias), _ptr(out), t, 2 * hin, 2 * win, cin, cout, kt, ks, _stream(x))
    return out


def conv3d_up2(x, w_packed, w_phase, bias, cout, kt, ks, out=None):
    """The nearest-2x upsample + conv of Resample38: the phase form where the shape has one (conv_up2_phase_ok) and w_phase is given,
    conv3d_cl(upsample2x=True) on w_packed otherwise."""
    if w_phase is not None and conv_up2_phase_ok(x.shape[-1], kt, ks):
        return conv3d_up2_phase(x, w_phase, bias, cout, out=out)
    return conv3d_cl(x, w_packed, bias, cout, kt, ks, upsample2x=True, out=out)


def dupup3d_add(x, main, cout, ft, fs, first_chunk, out=None):
    _dev(x, "x"), _dev(main, "main")
    t, h, w, cin = x.shape
    oshape = (t * ft - (ft - 1 if first_chunk else 0), h * fs, w * fs, cout)
    assert tuple(main.shape) == oshape and main.is_contiguous() and x.is_contiguous()
    out = torch.empty_like(main) if out is None else out
    _call("fg_dupup3d_add_bf16", _ptr(x), _ptr(main), _ptr(out), t, h, w, cin, cout, ft, fs, int(first_chunk),
          _stream(x))
    return out


def softmax_rows(scores, scale):
    _dev(scores, "scores", torch.float32)
    assert scores.dim() == 2 and scores.is_contiguous()
    probs = torch.empty(scores.shape, dtype=torch.bfloat16, device=scores.device)
    _call("fg_softmax_rows_f32_bf16", _ptr(scores), _ptr(probs), scores.shape[0], scores.shape[1], float(scale),
          _stream(scores))
    return probs


def vae_latent_to_cl(z, mean, inv_std):
    """(C,T,H,W) -> (T,H,W,C) de-normalised."""
    _dev(z, "z"), _dev(mean, "mean"), _dev(inv_std, "inv_std")
    assert z.dim() == 4 and z.is_contiguous()
    c, t, h, w = z.shape
    out = torch.empty((t, h, w, c), dtype=z.dtype, device=z.device)
    _call("fg_vae_latent_to_cl_bf16", _ptr(z), _ptr(mean), _ptr(inv_std), _ptr(out), c, t, h, w, _stream(z))
    return out


def vae_unpatchify(x, video, t0, clamp):
    """x (T,H,W,12) -> video[:, t0:t0+T] of (3,F,2H,2W)."""
    _dev(x, "x"), _dev(video, "video")
    t, h, w, c = x.shape
    assert c == 12 and x.is_contiguous() and video.is_contiguous()
    assert video.shape[0] == 3 and video.shape[2] == 2 * h and video.shape[3] == 2 * w
    _call("fg_vae_unpatchify_bf16", _ptr(x), _ptr(video), t, h, w, video.shape[1], t0, int(clamp), _stream(x))
    return video


def vae_tile_accumulate(tile, values, weight, y0, x0, border_h, border_w, bounds):
    _dev(tile, "tile"), _dev(values, "values"), _dev(weight, "weight")
    c, f, th, tw = tile.shape
    _, _, hv, wv = values.shape
    assert tile.is_contiguous() and values.is_contiguous() and weight.is_contiguous() and values.shape[0] == c
    bits = sum(1 << i for i, bnd in enumerate(bounds) if bnd)
    _call("fg_vae_tile_accumulate_bf16", _ptr(tile), _ptr(values), _ptr(weight), c, f, hv, wv, th, tw, y0, x0,
          border_h, border_w, bits, _stream(tile))


def vae_tile_finalize(values, weight, clamp=True):
    c, f, hv, wv = values.shape
    _call("fg_vae_tile_finalize_bf16", _ptr(values), _ptr(weight), c, f, hv, wv, int(clamp), _stream(values))
    return values


def vae_patchify(video):
    """(3,T,H,W) -> (T,H/2,W/2,16) channels-last (12 patch channels + 4 zero channels)."""
    _dev(video, "video")
    assert video.dim() == 4 and video.shape[0] == 3 and video.is_contiguous()
    _, t, h, w = video.shape
    out = torch.empty((t, h // 2, w // 2, 16), dtype=video.dtype, device=video.device)
    _call("fg_vae_patchify_bf16", _ptr(video), _ptr(out), t, h, w, _stream(video))
    return out


def avgdown3d_add(x, main, ft, fs):
    _dev(x, "x"), _dev(main, "main")
    t, h, w, cin = x.shape
    cout = main.shape[-1]
    assert tuple(main.shape) == ((t + ft - 1) // ft, h // fs, w // fs, cout) and x.is_contiguous() and main.is_contiguous()
    out = torch.empty_like(main)
    _call("fg_avgdown3d_add_bf16", _ptr(x), _ptr(main), _ptr(out), t, h, w, cin, cout, ft, fs, _stream(x))
    return out


def vae_latent_from_cl(x, mean, inv_std, z_dim):
    """(T,h,w,Cx) -> (z_dim,T,h,w) normalised latent."""
    _dev(x, "x"), _dev(mean, "mean"), _dev(inv_std, "inv_std")
    t, h, w, cx = x.shape
    assert x.is_contiguous()
    out = torch.empty((z_dim, t, h, w), dtype=x.dtype, device=x.device)
    _call("fg_vae_latent_from_cl_bf16", _ptr(x), _ptr(mean), _ptr(inv_std), _ptr(out), z_dim, cx, t, h, w, _stream(x))
    return out


def video_to_uint8(video):
    """(3,F,H,W) bf16 in [-1,1] -> (F,H,W,3) uint8."""
    _dev(video, "video")
    assert video.is_contiguous()
    _, f, h, w = video.shape
    out = torch.empty((f, h, w, 3), dtype=torch.uint8, device=video.device)
    _call("fg_video_to_uint8", _ptr(video), _ptr(out), f, h, w, _stream(video))
    return out


# ----------------------------------------------------------------------------- umT5 text encoder helpers
def softmax_bias(scores, bias, key_mask=None):
    """scores, bias (rows, cols) bf16; key_mask (cols,) int32 or None -> probs bf16."""
    _dev(scores, "scores"), _dev(bias, "bias")
    assert scores.dim() == 2 and scores.shape == bias.shape and scores.is_contiguous() and bias.is_contiguous()
    if key_mask is not None:
        _dev(key_mask, "key_mask", torch.int32)
        assert key_mask.shape == (scores.shape[1],) and key_mask.is_contiguous()
    probs = torch.empty_like(scores)
    _call("fg_softmax_bias_bf16", _ptr(scores), _ptr(bias), _ptr(key_mask), _ptr(probs), scores.shape[0], scores.shape[1],
          _stream(scores))
    return probs


def gated_gelu(fc1, gate):
    _dev(fc1, "fc1"), _dev(gate, "gate")
    assert fc1.shape == gate.shape and fc1.is_contiguous() and gate.is_contiguous()
    out = torch.empty_like(fc1)
    _call("fg_gated_gelu_bf16", _ptr(fc1), _ptr(gate), _ptr(out), fc1.numel(), _stream(fc1))
    return out

"""Wan2.2-TI2V-5B DiT on MI355X: parameter layout of the reference, compute on the HIP kernels.

Mirror of ``diffsynth/models/wan_video_dit.py`` (``WanModel`` :271-336, ``DiTBlock`` :195-229,
``SelfAttention`` :123-146, ``CrossAttention`` :149-185, ``Head`` :252-268): same constructor kwargs,
same parameter names and shapes, so reference checkpoints, LoRA files and the key-hash model
identification (``core/loader/file.py:117-121``) keep working.  The modules hold parameters only; the
arithmetic is in ``forward_tokens_steps`` below, built from ``fairygen_amd.hip`` kernels: one block body whose
Linears go through ``_BlockLinears`` — this repo's persistent MFMA GEMM (bf16 or e4m3, with the residual / gate /
GELU stores) by default, hipBLASLt (``F.linear``, ``torch._scaled_mm``) where ``FAIRYGEN_GEMM`` / ``FAIRYGEN_FP8_GEMM`` or
the shape say so — and whose norms hand over an ``Act``; its attention goes through ``_BlockAttention`` — bf16, or the e4m3 forms of
``enable_qk8_attention``.  The embedding and head Linears are ``F.linear``.  Nothing here runs on CPU tensors — the HIP library raises.
"""
import math
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip, tuning


def sinusoidal_embedding_1d(dim, position):
    """fp64 sinusoid [cos | sin] (reference :67-71); position is a small CPU tensor here."""
    sinusoid = torch.outer(position.to(torch.float64),
                           torch.pow(10000.0, -torch.arange(dim // 2, dtype=torch.float64).div(dim // 2)))
    return torch.cat([sinusoid.cos(), sinusoid.sin()], dim=1).to(position.dtype)


def precompute_freqs_cis(dim, end=1024, theta=10000.0):
    """complex128 rotation table of one axis (reference :82-88)."""
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2, device="cpu")[: dim // 2].double() / dim))
    freqs = torch.outer(torch.arange(end, device="cpu"), freqs)      # explicit cpu: models are built under device("meta")
    return torch.polar(torch.ones_like(freqs), freqs)


def precompute_freqs_cis_3d(dim, end=1024, theta=10000.0):
    """(frame, height, width) tables; head_dim split d-2*(d//3), d//3, d//3 (reference :74-79)."""
    return (precompute_freqs_cis(dim - 2 * (dim // 3), end, theta),
            precompute_freqs_cis(dim // 3, end, theta),
            precompute_freqs_cis(dim // 3, end, theta))


# The bias-GEMMs of the 30 blocks (hipBLASLt behind PyTorch, as north_star leaves them).  Module-level seams so that
# bench.py can put HIP events around exactly these launches (its hipBLASLt roofline entry); looked up at call time.
def gemm_bias(x, weight, bias):
    return F.linear(x, weight, bias)


def gemm_bias_gelu(x, weight, bias):
    """ffn.0 with GELU(tanh) applied to the fp32 accumulator in the hipBLASLt epilogue; x (b, n, K) contiguous: b * n rows of one GEMM."""
    return torch._addmm_activation(bias, x.reshape(-1, x.shape[-1]), weight.t(), use_gelu=True).view(x.shape[:-1] + (weight.shape[0],))


def gemm_bias_tuned(x, weight, bias):
    return tuning.linear(x, weight, bias)      # table: better hipBLASLt solution at the multi-GPU shard sizes


# The DiT Linears that run on this repo's own persistent MFMA kernel (fg_gemm_epilogue_bf16 / fg_gemm_fp8_bf16, csrc/gen_gemm_p.py) —
# also seams for bench.py.  FAIRYGEN_GEMM = "all" (default): every Linear of the 30 blocks — qkv, the self-attention o with the
# gate_msa add in its store, cross-attention q and o (+ residual), ffn.0 with GELU(tanh) in its epilogue, ffn.2 with the gate_mlp add —
# so a denoise step launches no library GEMM inside the blocks; "fused": qkv and ffn.0 (+ GELU in the hipBLASLt epilogue) stay on the
# library (round 2's default); "fused-ffn2": ffn.2 as well; "lib": everything on hipBLASLt.  Measurements: DESIGN.md §5.
GEMM_BACKEND = os.environ.get("FAIRYGEN_GEMM", "all")
GEMM_MIN_TILES = 64      # round 2 asked for two rounds of the CUs (512 tiles); see own_gemm_ok
# hot_backend="fused": how an adapter is folded into a weight.  "hip" (default): fg_lora_fuse_bf16 where it takes the Linear, torch ops
# for the others; "torch": the reference's three torch ops on the device for every Linear (the A/B leg of tools/hot_lora_step.py --swap).
LORA_FUSE = os.environ.get("FAIRYGEN_LORA_FUSE", "hip")
FP8_FOLD = os.environ.get("FAIRYGEN_FP8_FOLD", "1") != "0"      # fp8 mode: norm kernels emit (e4m3 rows, scales) directly
FP8_GEMM = os.environ.get("FAIRYGEN_FP8_GEMM", "own")           # fp8 mode: "own" = fg_gemm_fp8_bf16, "lib" = torch._scaled_mm (hipBLASLt)


def own_gemm_ok(rows, n, k):
    """Shapes the persistent kernel takes: 256-column tiles, 128-byte k-steps in pairs, and enough tiles to be worth a 256-workgroup
    launch.  Round 2 asked for two rounds of the CUs (512 tiles); measured at the 8- / 4- / 2-rank shard sizes (3 410 / 6 820 / 13 640
    rows) the kernel is within 5 % of the library on every shape with one round or less, 1.6x faster on ffn.2 (K = 14 336:
    1 154 vs 739 TFLOP/s at 3 410 rows), and the fused residual store replaces a separate pass."""
    return GEMM_BACKEND != "lib" and n % 256 == 0 and k % 128 == 0 and ((rows + 255) // 256) * (n // 256) >= GEMM_MIN_TILES


# **state: nothing (the scheduler block and scratch hip keeps per (device, stream)), or the sched= / workspace= of a caller that owns
# them (_BlockLinears.state: a captured denoise step).
def gemm_bias_own(x, weight, bias, **state):
    return hip.gemm_epilogue(x, weight, bias, **state)


def gemm_bias_gelu_own(x, weight, bias, **state):
    """ffn.0 + nn.GELU(approximate='tanh') (models/wan_video_dit.py:208): GELU on the bf16-rounded Linear output in the GEMM's store."""
    return hip.gemm_epilogue(x, weight, bias, act="gelu_tanh", **state)


def gemm_fp8_own(xq, scale_a, w8, bias, batch=1, **state):
    """fp8_linear's matmul on the e4m3 form of the persistent kernel: (rows, K) e4m3 x (N, K) e4m3 -> (1, rows, N) bf16.  batch=B (passed
    by a stacked forward only): the rows are B elements' and the result is (B, rows / B, N), still one GEMM."""
    return hip.gemm_fp8(xq, scale_a, w8, bias, lead_shape=(batch, xq.shape[0] // batch), **state)


def fp8_own_ok(n, k):
    """Shapes fg_gemm_fp8_bf16 takes (and FAIRYGEN_FP8_GEMM leaves to it); everything else goes to torch._scaled_mm."""
    return FP8_GEMM == "own" and n % 256 == 0 and k % 256 == 0


def gemm_residual(x, a, weight, bias, mod=None, gate_idx=None, **state):
    """x (the residual stream, contiguous, updated in place) += gate * Linear(a); gate = vector gate_idx of mod, or 1."""
    return hip.gemm_epilogue(a, weight, bias, out=x, residual=True, mod=mod, gate_idx=gate_idx, **state)


# The gated stores of a stacked forward with enable_stacked_cfg(periodic_gate=True): ONE launch on the rows of all elements, the two-row
# gate table read by the row inside the element (include/fairygen_hip_gategemm.h).  Seams like the ones above.
def gemm_residual_periodic(x, a, weight, bias, mod, gate_idx, rows_per_element, **state):
    """x (B, rows, N), in place, += gate * Linear(a), a (B, rows, K); gate row 0 for the first mod.first_rows rows of every element."""
    return hip.gemm_epilogue(a, weight, bias, out=x, residual=True, mod=mod, gate_idx=gate_idx, rows_per_element=rows_per_element, **state)


def gemm_fp8_residual_periodic(x, xq, scale_a, w8, bias, mod, gate_idx, rows_per_element, **state):
    """... the e4m3 form: xq / scale_a are the quantised rows of all elements."""
    return hip.gemm_fp8(xq, scale_a, w8, bias, out=x, residual=True, mod=mod, gate_idx=gate_idx, rows_per_element=rows_per_element, **state)


def stack_hot_loras(per_group, shapes, device, dtype):
    """The operands of hip.lora_apply for column groups that share an input: per_group[g] = [(alpha * A (r, K), B (Ng, r)), ...] (may be
    empty), shapes[g] = (K, Ng).  Per group the adapters are concatenated along the rank — sum_i (x A_i^T) B_i^T = (x [A_i]^T) [B_i]^T, the
    same sum with one rounding instead of one per adapter — and zero-padded to the kernel's rank R (the largest group's, in 32s).
    Returns (A (G * R, K), B (G * Ng, R)), or None when a group's stacked rank is above the kernel's 128."""
    rank = max(sum(a.shape[0] for a, _ in ads) for ads in per_group)
    r = -(-max(rank, 1) // hip.LORA_RANK_TILE) * hip.LORA_RANK_TILE
    if r > hip.LORA_MAX_RANK:
        return None
    a_st = torch.zeros((len(per_group), r, shapes[0][0]), dtype=dtype, device=device)
    b_st = [torch.zeros((ng, r), dtype=dtype, device=device) for _, ng in shapes]
    for g, ads in enumerate(per_group):
        at = 0
        for a, b in ads:
            a_st[g, at:at + a.shape[0]] = a.to(device=device, dtype=dtype)
            b_st[g][:, at:at + a.shape[0]] = b.to(device=device, dtype=dtype)
            at += a.shape[0]
    return a_st.view(-1, shapes[0][0]), torch.cat(b_st, 0).contiguous()


class Act(NamedTuple):
    """What a norm hands to the Linears behind it: the bf16 row, its (e4m3 rows, row scales) pair, or both — _BlockLinears decides which
    once per forward.  An fp8 Linear that gets the bf16 row only quantises it itself (fg_fp8_quant_rows_bf16).  nb: the elements of a
    stacked forward (WanModel.enable_stacked_cfg) behind a pair without a bf16 row — the pair is (nb * rows, C), one GEMM operand.  With
    both fields on a stacked activation (unfused adapters in the fp8 mode) the bf16 row is (B, rows, C) and says the batch; the pair is
    still that of all B * rows rows."""
    bf16: Optional[torch.Tensor] = None
    q8: Optional[tuple] = None
    nb: int = 1

    @property
    def batch(self):
        return self.bf16.shape[0] if self.bf16 is not None and self.bf16.dim() == 3 else self.nb

    @property
    def rows(self):
        return self.bf16.shape[-2] if self.bf16 is not None else self.q8[0].shape[0] // self.nb

    @property
    def total_rows(self):
        """The rows of the GEMM behind it: `rows`, times the batch of a stacked forward (WanModel.enable_stacked_cfg)."""
        return self.bf16.numel() // self.bf16.shape[-1] if self.bf16 is not None else self.q8[0].shape[0]


class _BlockLinears:
    """How the Linears and norms of the blocks run in ONE forward: the mode decisions (bf16 / fp8 Linears, hot-loaded adapters and their
    backend, which GEMMs are this repo's own) taken once, the norm kernels that fill the Act fields those Linears read, and the two forms a
    block Linear has — `plain` and `residual`.  Per Linear, `pack` is WanModel._hot_pack's answer: the stacked operands of
    fg_lora_apply_bf16, False (its adapters take the reference's torch ops, WanModel._hot) or None (no adapter)."""

    def __init__(self, model, mod_rows, owned=None):
        self.model, self.eps = model, model.eps
        # None, or what a captured step owns in place of the state hip keeps per (device, stream), which must not be recorded into a graph
        # (its key outlives the capture stream): .sched / .workspace (hip.gemm_state) for the own GEMMs; attention's part: _BlockAttention
        self.owned = owned
        self.fp8 = fp8 = model.fp8_dtype
        self.hot = hot = bool(model.hot_loras)
        # adapters on fg_lora_apply_bf16 next to the own GEMMs, bf16 or fp8 (comment on hot_lora_backend, WanVideoPipeline.load_lora)
        self.hip_hot = hip_hot = hot and model.hot_lora_backend == "hip"
        # fp8 mode: the norms of a block feed fp8 Linears only, so they write (e4m3 rows, scales) and no bf16 row (FAIRYGEN_FP8_FOLD); an
        # adapter reads the bf16 row too: both outputs in one pass on the "hip" backend, the bf16 row and a separate quantisation on "torch"
        self.want_bf16 = fp8 is None or hot or not FP8_FOLD
        self.want_q8 = fp8 is not None and (hip_hot if hot else FP8_FOLD)
        # x += gate * Linear(a) can happen in the GEMM's store: gates of one or two time rows, and adapters, if any, on the HIP kernel
        self.own = mod_rows in (1, 2) and (hip_hot if hot else fp8 is None)
        # fp8 Linears without HIP adapters: ffn.0 hands on its pre-activation and GELU(tanh) is fused into the quantisation of ffn.2's input
        self.gelu_in_quant = fp8 is not None and not hip_hot

    # ---- the norms: modulate(LN(x)), LN(x) * w + b, each alone or behind x += gate * y, and the bare x += gate * y
    def modulate(self, x, mod, shift_idx, scale_idx, out=None):
        if self.want_bf16 and self.want_q8:      # a stacked forward: both fields of all rows, the bf16 one (B, rows, C)
            return Act(*hip.ln_modulate_dual(x, mod, shift_idx, scale_idx, self.eps, out=out, batch=self.batch_of(x)))
        if self.want_q8:
            nb = self.batch_of(x)
            return Act(None, hip.ln_modulate_fp8(x, mod, shift_idx, scale_idx, self.eps, batch=nb), nb or 1)
        return Act(hip.ln_modulate(x, mod, shift_idx, scale_idx, self.eps, out=out, batch=self.batch_of(x)))

    @staticmethod
    def batch_of(x):
        """batch= of the row kernels that read a table by the row inside the element: the leading dimension of a stacked forward
        (WanModel.enable_stacked_cfg; the bf16 norms, the fp8-output ones and — enable_stacked_cfg(hot_lora=True) — the two-output one
        of unfused adapters get there), None for the one element every other forward has."""
        return x.shape[0] if x.dim() == 3 and x.shape[0] > 1 else None

    def affine(self, x, norm):
        """norm3 on its own has no fp8-only kernel: the bf16 row, which the fp8 Linear behind it quantises.  It reads no table by row
        number, so a stacked activation is simply all its rows, in either form."""
        if self.want_bf16 and self.want_q8:
            return Act(*hip.ln_affine_dual(x, norm.weight, norm.bias, self.eps))
        return Act(hip.ln_affine(x, norm.weight, norm.bias, self.eps))

    def gate_residual(self, x, y, mod, gate_idx):
        return hip.gate_residual(x, y, mod if gate_idx is not None else None, gate_idx, out=x, batch=self.batch_of(x))

    def residual_modulate(self, x, y, mod, gate_idx, norm_mod, shift_idx, scale_idx, out=None):
        if self.want_bf16 and self.want_q8:      # no fused kernel with both outputs
            x = self.gate_residual(x, y, mod, gate_idx)
            return x, self.modulate(x, norm_mod, shift_idx, scale_idx, out)
        if self.want_q8:
            nb = self.batch_of(x)
            x, q8 = hip.residual_ln_modulate_fp8(x, y, mod, gate_idx, shift_idx, scale_idx, self.eps, x_out=x, norm_mod=norm_mod, batch=nb)
            return x, Act(None, q8, nb or 1)
        x, h = hip.residual_ln_modulate(x, y, mod, gate_idx, shift_idx, scale_idx, self.eps, x_out=x, norm_out=out, norm_mod=norm_mod,
                                        batch=self.batch_of(x))
        return x, Act(h)

    def residual_affine(self, x, y, mod, gate_idx, norm):
        if self.want_bf16 and self.want_q8:
            x = self.gate_residual(x, y, mod, gate_idx)
            return x, self.affine(x, norm)
        if self.want_q8:
            nb = self.batch_of(x)
            x, q8 = hip.residual_ln_affine_fp8(x, y, norm.weight, norm.bias, self.eps, mod, gate_idx, x_out=x, batch=nb)
            return x, Act(None, q8, nb or 1)
        x, h = hip.residual_ln_affine(x, y, norm.weight, norm.bias, self.eps, mod, gate_idx, x_out=x, batch=self.batch_of(x))
        return x, Act(h)

    # ---- the Linears
    def state(self, rows, n, k_bytes):
        """The sched= / workspace= of an own GEMM of (rows, n) over k_bytes operand bytes per row: none in an eager forward; the owner's
        block, and its scratch exactly where workspace=True would have used hip's (same k-split, same bits)."""
        if self.owned is None:
            return {}
        return {"sched": self.owned.sched, "workspace": self.owned.workspace if hip.gemm_workspace_need(rows, n, k_bytes) > 0 else False}

    def q8(self, a):
        return a.q8 if a.q8 is not None else hip.fp8_quant_rows(a.bf16, None)

    def plain(self, a, names, weight, bias, w8, own=False, gelu=False, hip_adapters=True):
        """Linear (+ the adapters of `names`: the column groups of a fused projection) (+ GELU(tanh)) of the Act `a` -> (1, rows, N) bf16
        ((B, rows, N) from the Act of a stacked forward: one GEMM on its B * rows rows).
        weight / w8: the bf16 and e4m3 (None in bf16 mode) forms; own: bf16 mode, the own GEMM may take this Linear (FAIRYGEN_GEMM).
        gelu (ffn.0): the result is nn.GELU's output — except with gelu_in_quant, where it is the pre-activation."""
        m, fp8 = self.model, self.fp8
        n, k = weight.shape
        rows = a.total_rows      # a stacked forward: the rows of all elements in one GEMM
        stacked = {"batch": a.batch} if a.batch > 1 else {}      # ... whose fp8 form returns (B, rows / B, N)
        own = fp8 is None and own and own_gemm_ok(rows, n, k)
        if hip_adapters and self.hip_hot and (fp8 is None or fp8_own_ok(n, k)):
            pack = m._hot_pack(names)
        elif gelu:      # an adapter adds to the pre-activation: only a Linear that has one gives up its fused GELU
            pack = False if any(nm in m.hot_loras for nm in names) else None
        else:
            pack = False if self.hot else None
        if gelu and pack is False:
            own = False      # the reference's ops for this Linear: library GEMM, adapters, GELU
        if gelu and pack is None and not self.gelu_in_quant:      # nothing between the Linear and its GELU: into the GEMM's store where one takes it
            if fp8 is not None and fp8_own_ok(n, k):
                return hip.gemm_fp8(*a.q8, w8, bias, act="gelu_tanh", lead_shape=(a.batch, rows // a.batch), **self.state(rows, n, k))
            if own:
                return gemm_bias_gelu_own(a.bf16, weight, bias, **self.state(rows, n, 2 * k))
            if fp8 is None and m.gelu_epilogue:      # GELU(tanh) in the hipBLASLt epilogue: one pass less over the (n, ffn) tensor
                return gemm_bias_gelu(a.bf16, weight, bias)
        if fp8 is not None:
            y = m._scaled_linear(*self.q8(a), w8, bias, **stacked, **self.state(rows, n, k))
        else:
            y = gemm_bias_own(a.bf16, weight, bias, **self.state(rows, n, 2 * k)) if own else gemm_bias(a.bf16, weight, bias)
        nb = a.batch if a.batch > 1 else None      # stacked: the adapter kernel takes the batch (include/fairygen_hip_lorabatch.h)
        if gelu and pack:      # GELU moves from the GEMM's store into the adapter kernel's
            return hip.lora_apply(a.bf16, pack[0], pack[1], y, mode="gelu_tanh", batch=nb)
        m._hot_apply(names, a.bf16, y, pack, batch=nb)
        return hip.activation(y, "gelu_tanh") if gelu and not self.gelu_in_quant else y

    def residual(self, x, a, name, weight, bias, w8, mod, gate_idx, affine=None, modulate=None, out=None, tuned=False, store_ok=True,
                 gelu=False):
        """x (the residual stream, in place) += gate * (Linear(a) + adapters of `name`), gate = vector gate_idx of mod (None: 1), then the
        norm behind it: affine = the LayerNorm module, or modulate = (table, shift_idx, scale_idx) with `out` an old bf16 row to write
        into, or neither (last block).  Returns (x, Act or None).  Two forms (AutoWrappedLinear.forward, core/vram/layers.py:429-436, then
        GateModule; the gate distributes over Linear + adapter): the add in the GEMM's store (fg_gemm_epilogue_bf16 / fg_gemm_fp8_bf16)
        and in fg_lora_apply_bf16, then the norm alone; or a plain GEMM, the adapters, and the fused residual + norm kernel.
        a: bf16; gelu: it is ffn.0's pre-activation (gelu_in_quant).  tuned / store_ok: ffn.2's library GEMM comes from the tuning table,
        and FAIRYGEN_GEMM=fused-ffn2 keeps it there.
        A stacked forward (a: (B, rows, K), B > 1; fp8 Linears without adapters take the second form): the store picks its gate row by
        `row >= first_rows` over the rows of the launch, so with a two-row gate table it is launched once per element on the element's
        rows (fp8: and on the element's quantised rows) — the batch-1 forward's launch, the batch-1 forward's bits; with one gate row or
        none, one launch takes all B * rows rows.  enable_stacked_cfg(periodic_gate=True) replaces the per-element launches by ONE launch
        of fg_gemm_epilogue_bf16_sp / fg_gemm_fp8_bf16_sp on the B * rows rows, whose gate rule counts inside the element
        (rows_per_element = rows; elements below the kernel's 256 rows stay per element) — own_gemm_ok is then asked about B * rows.
        The adapters behind the stores are ONE fg_lora_apply_bf16_b launch either way: its gate rule counts inside the element
        (enable_stacked_cfg(hot_lora=True)).
        The other form runs its GEMM on B * rows rows and the batched row kernels (include/fairygen_hip_rowbatch.h) do the gate."""
        m, fp8 = self.model, self.fp8
        n, k = weight.shape
        gmod = mod if gate_idx is not None else None
        pack = m._hot_pack((name,)) if self.hip_hot else False if name in m.hot_loras else None
        nb = a.shape[0]
        per_element = nb > 1 and gmod is not None and gmod.mod_rows == 2
        periodic = per_element and m.stacked_cfg_periodic_gate and a.shape[1] >= hip.GEMM_GATE_MIN_PERIOD
        per_element = per_element and not periodic
        rows = a.shape[1] if per_element else nb * a.shape[1]      # of one store launch
        if self.own and store_ok and pack is not False and (own_gemm_ok(rows, n, k) if fp8 is None else fp8_own_ok(n, k)):
            if fp8 is not None:      # the quantisation is per row: one pass over all rows, whichever way the store is launched
                aq, asc = hip.fp8_quant_rows(a)
            if periodic and fp8 is None:
                gemm_residual_periodic(x, a, weight, bias, gmod, gate_idx, a.shape[1], **self.state(rows, n, 2 * k))
            elif periodic:
                gemm_fp8_residual_periodic(x, aq, asc, w8, bias, gmod, gate_idx, a.shape[1], **self.state(rows, n, k))
            elif per_element and fp8 is None:
                for e in range(nb):
                    gemm_residual(x[e:e + 1], a[e:e + 1], weight, bias, gmod, gate_idx, **self.state(rows, n, 2 * k))
            elif per_element:
                for e in range(nb):
                    hip.gemm_fp8(aq[e * rows:(e + 1) * rows], asc[e * rows:(e + 1) * rows], w8, bias, out=x[e:e + 1], residual=True, mod=gmod,
                                 gate_idx=gate_idx, **self.state(rows, n, k))
            elif fp8 is None:
                gemm_residual(x, a, weight, bias, gmod, gate_idx, **self.state(rows, n, 2 * k))
            else:
                hip.gemm_fp8(aq, asc, w8, bias, out=x, residual=True, mod=gmod, gate_idx=gate_idx, **self.state(rows, n, k))
            if pack:
                hip.lora_apply(a, pack[0], pack[1], x, mode="add" if gmod is None else "gate", mod=gmod, gate_idx=gate_idx,
                               batch=nb if nb > 1 else None)
            if affine is not None:
                return x, self.affine(x, affine)
            return x, self.modulate(x, *modulate, out=out) if modulate is not None else None
        if fp8 is None:
            y = (gemm_bias_tuned if tuned else gemm_bias)(a, weight, bias)
        else:
            # stacked: the quantisation is per row, so all nb * rows rows are one pass and one GEMM, and y comes back (nb, rows, N)
            y = m._scaled_linear(*hip.fp8_quant_rows(a, "gelu_tanh" if gelu else None), w8, bias, **({"batch": nb} if nb > 1 else {}),
                                 **self.state(nb * a.shape[1], n, k))
        if pack is not None:      # only then is nn.GELU's bf16 output needed
            m._hot_apply((name,), hip.activation(a.clone(), "gelu_tanh") if gelu else a, y, pack, batch=nb if nb > 1 else None)
        if affine is not None:
            return self.residual_affine(x, y, mod, gate_idx, affine)
        if modulate is not None:
            return self.residual_modulate(x, y, mod, gate_idx, *modulate, out=out)
        return self.gate_residual(x, y, mod, gate_idx), None


# enable_qk8_attention(): self-attention over more keys than this runs the e4m3 Q K^T kernel; at or below it (where fg_attn_fwd_bf16 itself
# leaves its 4-wave kernel) the bf16 kernel runs
QK8_MIN_KV = 1024


def takes_cross8_attention(model, attn, n_kv, batch):
    """enable_qk8_attention(cross=True): the stock AttentionModule of cross-attention, one batch element, a context whose K8 and V8^T fit
    the LDS (hip.attention_cross8_max_kv(): 640 keys).  Anything else keeps the bf16 kernel."""
    return bool(model.cross8_attention) and type(attn) is AttentionModule and (batch == 1 or bool(model.stacked_cfg)) and \
        1 <= n_kv <= hip.attention_cross8_max_kv()


def takes_qk8_attention(model, attn, n_kv, batch):
    """Whether a block's self-attention over n_kv keys runs the e4m3 Q K^T kernel: the mode on, the stock AttentionModule, more than
    QK8_MIN_KV keys, one batch element.  n_kv is the TOTAL key count: all ranks' on a token shard (_BlockAttention.self_attention_steps)."""
    return bool(model.qk8_attention) and type(attn) is AttentionModule and n_kv > QK8_MIN_KV and (batch == 1 or bool(model.stacked_cfg))


def dense_tokens(t):
    """What an exchange of a stacked forward on a token shard hands back, (B, N, C) views of a gathered slab whose elements lie
    world * chunk rows apart, as the operand the batched attention kernels take (batch stride N * ld): the view itself when the slab has
    no padding rows (world * chunk == N), else one compaction copy.  One element is never copied."""
    return t if t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1) else t.contiguous()


class _BlockAttention:
    """How the attention of the blocks runs in ONE forward, next to _BlockLinears: the forms enable_qk8_attention switched on (the model's
    flags, read once; whether a call takes them is takes_qk8_attention / takes_cross8_attention, asked once per attention), what a
    captured step owns in place of per-call allocations, and the two paths — self_attention_steps between the q | k | v Linear and o,
    cross_attention from norm3's row to the operand of o."""

    def __init__(self, model, lin, owned=None):
        self.model, self.lin, self.eps = model, lin, model.eps
        # None, or a captured step (_BlockLinears.owned): .attn_workspace, the split-KV scratch, and .attn_qk8_bufs, the e4m3 operands
        self.owned = owned
        self.fused = model.qk8_fused_producer                                   # the RMSNorm+RoPE pass writes the e4m3 q / k operands
        self.pv8, self.smooth = model.pv8_attention, model.smoothv_attention    # P V in e4m3 too; with V mean-smoothed
        self.cross_smooth = model.smoothv_cross_attention                       # the e4m3 cross-attention with V mean-smoothed

    def _owned(self, kind, n, num_heads, head_dim, device, make):
        """A captured step's buffers of one kind and shape — make(n, num_heads, head_dim, device), once, one set for all blocks (a block's
        are consumed before the next block writes them, in stream order); None in an eager forward, where the binding allocates."""
        if self.owned is None:
            return None
        key = (kind, n, num_heads, head_dim, device)
        if key not in self.owned.attn_qk8_bufs:
            self.owned.attn_qk8_bufs[key] = make(n, num_heads, head_dim, device)
        return self.owned.attn_qk8_bufs[key]

    def workspace(self):
        """The workspace= of an attention call: a captured step's own split-KV scratch; nothing in an eager forward, so that the seams
        tools replace (hip.attention behind AttentionModule) are called as they have always been."""
        return {} if self.owned is None else {"workspace": self.owned.attn_workspace}

    def attention(self, attn, q, k, v, scale=None):
        """The bf16 form, through the block's AttentionModule (plug point (iii))."""
        return attn(q, k, v, **({} if scale is None else {"scale": scale}), **self.workspace())

    def pv8_kw(self, v, num_heads):
        """The pv8= / smooth= / pv8_bufs= of an e4m3 self-attention call on v (1, N, H*D): nothing unless enable_qk8_attention(pv8=True); a
        captured step owns v8t, sv and the statistics scratch — with smooth_v=True also mu, and the larger scratch of that form."""
        if not self.pv8:
            return {}
        bufs = self._owned("pv8s" if self.smooth else "pv8", v.shape[1], num_heads, v.shape[2] // num_heads, v.device,
                           lambda *shape: hip.attention_pv8_scratch(*shape, smooth=self.smooth))
        return {"pv8": True, "smooth": self.smooth, "pv8_bufs": bufs}

    # ---- self-attention
    def self_attention(self, sa, qkv, rq, rk, scale, e4m3):
        """The unsharded block, from the q | k | v buffer (B, N, 3 C).  bf16: the two RMSNorm+RoPE passes, then the AttentionModule.
        e4m3 (takes_qk8_attention said so), two-step: the same two passes, then hip.attention_qk8 (quantise, attend).  e4m3 with
        enable_qk8_attention(fused_producer=True): the pass of q writes the e4m3 rows and their scales and no bf16 q, that of k writes
        bf16 k and the key statistics, one pass converts k — the bytes of the two-step form (tests/test_attention_qk8_fused.py)."""
        nh, eps = sa.attn.num_heads, self.eps
        c = qkv.shape[-1] // 3
        shape = (qkv.shape[1], nh, c // nh, qkv.device)
        v = qkv[..., 2 * c:]
        if e4m3 and self.fused:
            q8, k8, sq, sk, kbar, parts = self._owned("qk8-fused", *shape, hip.attention_qk8_fused_scratch) or \
                hip.attention_qk8_fused_scratch(*shape, qkv.shape[0])
            k, _ = hip.rmsnorm_rope_kstats(qkv[..., c:2 * c], sa.norm_k.weight, nh, eps, *rk, partials=parts)
            hip.rmsnorm_rope_q8(qkv[..., :c], sa.norm_q.weight, nh, eps, *rq, q8=q8, sq=sq)
            hip.attn_quant_k(k, parts, nh, k8, sk, kbar)
            return hip.attention_qk8_pre(q8, k8, sq, sk, v, nh, scale=scale, **self.workspace(), **self.pv8_kw(v, nh))
        nb = self.lin.batch_of(qkv)
        k = hip.rmsnorm_rope(qkv[..., c:2 * c], sa.norm_k.weight, nh, eps, *rk, batch=nb)
        q = hip.rmsnorm_rope(qkv[..., :c], sa.norm_q.weight, nh, eps, *rq, batch=nb)
        if e4m3:
            return hip.attention_qk8(q, k, v, nh, scale=scale, bufs=self._owned("qk8", *shape, hip.attention_qk8_scratch), **self.workspace(),
                                     **self.pv8_kw(v, nh))
        return self.attention(sa.attn, q, k, v, scale)

    def self_attention_steps(self, i, sa, qkv, rq, rk, scale, shard, shard_total):
        """Block i's self-attention from its q | k | v buffer: (B, n, C).  Yields i right after each exchange of a token-sharded run has
        been started.  The e4m3 form is decided once, on the key count of all ranks: a shard of 200 rows of 1 600 keys takes it."""
        sharded = shard is not None and shard.active
        e4m3 = takes_qk8_attention(self.model, sa.attn, shard_total if sharded else qkv.shape[1], qkv.shape[0])
        if not sharded:
            return self.self_attention(sa, qkv, rq, rk, scale, e4m3)
        nh, eps = sa.attn.num_heads, self.eps
        c = qkv.shape[-1] // 3
        v = qkv[..., 2 * c:]
        if shard.attn_mode == "ulysses":
            # token shard -> head shard (all N tokens of 24/P heads), attention, head shard -> token shard.  The
            # norm+RoPE kernels and one strided copy write q | k | v straight into the all-to-all send buffer.
            n_loc, p_, size, hl = qkv.shape[1], shard.world_size, shard.chunk(shard_total), shard.heads_local(nh)
            g = c // nh * hl
            send = shard.ulysses_send_buffer(shard_total, c, qkv, n_loc)           # (P, chunk, 3, g)
            flat, layout = send.view(-1), (g, size * 3 * g, 3 * g)
            hip.rmsnorm_rope(qkv[..., :c], sa.norm_q.weight, nh, eps, *rq, grouped=(flat, *layout))
            hip.rmsnorm_rope(qkv[..., c:2 * c], sa.norm_k.weight, nh, eps, *rk, grouped=(flat[g:], *layout))
            hip.copy_groups(qkv.view(-1)[2 * c:], g, 3 * c, flat[2 * g:], size * 3 * g, 3 * g, p_, n_loc, g)
            pending = shard.ulysses_exchange_async(send, shard_total)
            yield i
            qg, kg, vg = pending.wait()
            o_full = shard.ulysses_out_buffer(shard_total, g, qkv)
            out = o_full[:shard_total].unsqueeze(0)
            if e4m3:      # all N tokens of this rank's heads: every statistic is local
                hip.attention_qk8(qg, kg, vg, hl, out=out, scale=scale, **self.pv8_kw(vg, hl))
            else:
                hip.attention(qg, kg, vg, hl, out=out, scale=scale)
            pending = shard.ulysses_out_async(o_full, shard_total, n_loc)
            yield i
            a = torch.empty((1, n_loc, c), dtype=qkv.dtype, device=qkv.device)
            hip.copy_groups(pending.wait_blocks().view(-1), size * g, g, a.view(-1), g, c, p_, n_loc, g)
            return a
        if e4m3:
            return (yield from self._shard8_steps(i, sa, qkv, rq, rk, scale, shard, shard_total))
        nb = self.lin.batch_of(qkv)      # a stacked forward on the shard (enable_stacked_cfg(sharded=True)): ONE exchange carries both elements
        k = hip.rmsnorm_rope(qkv[..., c:2 * c], sa.norm_k.weight, nh, eps, *rk, batch=nb)
        pending = shard.all_gather_kv_async(k, v, shard_total)
        q = hip.rmsnorm_rope(qkv[..., :c], sa.norm_q.weight, nh, eps, *rq, batch=nb)
        yield i
        k, v = pending.wait()
        return self.attention(sa.attn, q, dense_tokens(k), dense_tokens(v), scale)

    def _shard8_steps(self, i, sa, qkv, rq, rk, scale, shard, shard_total):
        """Block i's self-attention in the e4m3 form on the K / V all-gather layout (enable_qk8_attention(sharded=True),
        include/fairygen_hip_shard8.h): this rank's queries against all N keys.  Two exchanges, a yield after each has been started: the
        ranks' statistics records (20 * C bytes each), from which every rank derives the unsharded key mean, sk and sv; then k8 and v (with
        pv8: v8) through all_gather_kv_async, as uint8 views.  A rank without rows launches nothing and sends the neutral record.
        With smooth_v (enable_qk8_attention(sharded="all"), include/fairygen_hip_shard8s.h) the record has 32 * C bytes — the fp64 sum,
        the minimum and the maximum of v beside those of k — every rank derives the unsharded mu and sv from them, v8 is e4m3((v - mu) / sv)
        and the attention adds mu back; the exchanges and their sizes, the record apart, are the same.
        qkv (B, n, 3 C) with B > 1 (the stacked CFG forward on the shard, enable_stacked_cfg(sharded=True)): the same two exchanges, each
        carrying both elements — B records per rank, the (B, rows, C) bytes — and one launch sequence per step on the batched producers
        (include/fairygen_hip_shard8b.h, include/fairygen_hip_batch8.h); every statistic is per element."""
        nh, eps, pv8 = sa.attn.num_heads, self.eps, self.pv8
        smooth = pv8 and self.smooth
        c = qkv.shape[-1] // 3
        nb, n_loc, dev = qkv.shape[0], qkv.shape[1], qkv.device
        v = qkv[..., 2 * c:]
        if n_loc:
            k, parts = hip.rmsnorm_rope_kstats(qkv[..., c:2 * c], sa.norm_k.weight, nh, eps, *rk)
            record = hip.attn_shard8s_stats(parts, n_loc, nh, v) if smooth else hip.attn_shard8_stats(parts, n_loc, nh, v if pv8 else None)
        else:
            record = (hip.attn_shard8s_neutral_record if smooth else hip.attn_shard8_neutral_record)(c, dev, nb)
        pending = shard.all_gather_records_async(record)
        yield i
        if nb > 1:
            return (yield from self._shard8_batch_tail(i, qkv, rq, sa, k if n_loc else None, pending, scale, shard, shard_total))
        if n_loc:
            q8, sq = hip.rmsnorm_rope_q8(qkv[..., :c], sa.norm_q.weight, nh, eps, *rq)      # overlaps the record exchange
            if smooth:
                k8, v8, sk, _, sv, mu = hip.attn_shard8s_quant(pending.wait(), shard_total, k, nh, v)
            else:
                (k8, v8, sk, _, sv), mu = hip.attn_shard8_quant(pending.wait(), shard_total, k, nh, v if pv8 else None), None
            k8, v_send = k8.view(torch.uint8), (v8.view(torch.uint8) if pv8 else v[0])
        else:
            pending.wait()
            k8 = torch.empty((0, c), dtype=torch.uint8, device=dev)
            v_send = k8 if pv8 else v[0]
        pending = shard.all_gather_kv_async(k8.unsqueeze(0), v_send.unsqueeze(0), shard_total)
        yield i
        k8f, vf = pending.wait()
        if not n_loc:
            return torch.empty((1, 0, c), dtype=qkv.dtype, device=dev)
        k8f = k8f[0].view(torch.float8_e4m3fn)
        if pv8:
            return hip.attention_pv8_pre(q8, k8f, sq, sk, hip.attn_shard8_vt(vf[0].contiguous(), nh), sv, nh, scale=scale, mu=mu)
        return hip.attention_qk8_pre(q8, k8f, sq, sk, vf, nh, scale=scale)

    def _shard8_batch_tail(self, i, qkv, rq, sa, k, pending, scale, shard, shard_total):
        """_shard8_steps behind its first exchange for B > 1 elements: the scales and this rank's e4m3 rows per element, the second
        exchange — k8 and v (with pv8: v8) of both elements — and the batched attention.  The gathered k8 (and a bf16 v) is compacted to
        (B, N, C) only when world * chunk != N; the gathered v8 is transposed where it lies (hip.attn_shard8_vt takes the element stride)."""
        nh, eps, pv8 = sa.attn.num_heads, self.eps, self.pv8
        smooth = pv8 and self.smooth
        c = qkv.shape[-1] // 3
        nb, n_loc, dev = qkv.shape[0], qkv.shape[1], qkv.device
        v = qkv[..., 2 * c:]
        if n_loc:
            q8, sq = hip.rmsnorm_rope_q8(qkv[..., :c], sa.norm_q.weight, nh, eps, *rq)      # overlaps the record exchange
            if smooth:
                k8, v8, sk, _, sv, mu = hip.attn_shard8s_quant(pending.wait(), shard_total, k, nh, v)
            else:
                (k8, v8, sk, _, sv), mu = hip.attn_shard8_quant(pending.wait(), shard_total, k, nh, v if pv8 else None), None
            k8, v_send = k8.view(torch.uint8), (v8.view(torch.uint8) if pv8 else v)
        else:
            pending.wait()
            k8 = torch.empty((nb, 0, c), dtype=torch.uint8, device=dev)
            v_send = k8 if pv8 else v
        pending = shard.all_gather_kv_async(k8, v_send, shard_total)
        yield i
        k8f, vf = pending.wait()
        if not n_loc:
            return torch.empty((nb, 0, c), dtype=qkv.dtype, device=dev)
        k8f = dense_tokens(k8f).view(torch.float8_e4m3fn)
        if pv8:
            return hip.attention_pv8_pre(q8, k8f, sq, sk, hip.attn_shard8_vt(vf, nh), sv, nh, scale=scale, mu=mu)
        return hip.attention_qk8_pre(q8, k8f, sq, sk, dense_tokens(vf), nh, scale=scale)

    # ---- cross-attention
    def cross_attention(self, i, ca, h, ctx, kv_cache, wkv, bkv, w8):
        """Block i's cross-attention (reference :170-185) from h = norm3(x) against the context, both Acts: the q Linear and its norm,
        the block's context operands — computed from the k | v Linear (wkv, bkv: DiTBlock.fused_weights') on the context rows, or read
        back from kv_cache, which holds them once per denoise loop — and the attention; returns the operand of o.
        bf16: the operands are (k after norm_k, v).  e4m3 (enable_qk8_attention(cross=True), takes_cross8_attention): the q norm writes
        the e4m3 rows and their scales and no bf16 q (the RMSNorm pass without a RoPE table; a captured step owns the pair), and the
        operands are (k8, sk, v8t, sv) — the RMSNorm pass of k that also leaves the key statistics, the key conversion behind it, and
        fg_attn_quant_vt_bf16 on v.  With smooth_v_cross=True the V producer is the smoothing one and the key means of v follow as a
        fifth tensor, mu."""
        lin, nh, eps = self.lin, ca.attn.num_heads, self.eps
        rows = h.bf16 if h.bf16 is not None else h.q8[0]
        if rows.shape[-2] == 0:      # a token shard without rows: nothing to attend from, nothing is launched
            return torch.empty((h.batch, 0, ca.q.weight.shape[0]), dtype=ca.q.weight.dtype, device=rows.device)
        q = lin.plain(h, (f"blocks.{i}.cross_attn.q",), ca.q.weight, ca.q.bias, w8[2], own=lin.own)
        e4m3 = takes_cross8_attention(self.model, ca.attn, ctx.rows, q.shape[0])
        if e4m3:
            q8, sq = self._owned("cross8-q", q.shape[1], nh, q.shape[2] // nh, q.device, lambda n, heads, hd, dev: (
                torch.empty((n, heads * hd), dtype=torch.float8_e4m3fn, device=dev), torch.empty((n, heads), dtype=torch.float32, device=dev))) \
                or (None, None)
            q8, sq = hip.rmsnorm_rope_q8(q, ca.norm_q.weight, nh, eps, q8=q8, sq=sq)
        else:
            q = hip.rmsnorm_rope(q, ca.norm_q.weight, nh, eps)
        if kv_cache is not None and i in kv_cache:
            ops = kv_cache[i]
        else:      # 512 context rows, once per denoise loop with a kv_cache: library GEMM, adapters on the reference's torch ops
            kv = lin.plain(ctx, (f"blocks.{i}.cross_attn.k", f"blocks.{i}.cross_attn.v"), wkv, bkv, w8[3], hip_adapters=False)
            c = kv.shape[-1] // 2
            if e4m3:
                k, parts = hip.rmsnorm_rope_kstats(kv[..., :c], ca.norm_k.weight, nh, eps)
                k8, sk, _ = hip.attn_quant_k(k, parts, nh)
                vbufs = hip.attn_quant_vt(kv[..., c:], nh, smooth=self.cross_smooth)      # (v8t, sv, scratch[, mu])
                ops = (k8, sk, vbufs[0], vbufs[1]) + tuple(vbufs[3:])
            else:
                ops = (hip.rmsnorm_rope(kv[..., :c], ca.norm_k.weight, nh, eps, batch=lin.batch_of(kv)), kv[..., c:])
            if kv_cache is not None:
                kv_cache[i] = ops
        if not e4m3:
            return self.attention(ca.attn, q, *ops)
        k8, sk, v8t, sv = ops[:4]
        return hip.attention_cross8_pre(q8, k8, sq, sk, v8t, sv, nh, mu=ops[4] if self.cross_smooth else None)


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))


class AttentionModule(nn.Module):
    """Plug point (iii) of the reference (:113-120): "b s (n d)" bf16 in and out, on the MFMA kernel."""

    def __init__(self, num_heads):
        super().__init__()
        self.num_heads = num_heads

    def forward(self, q, k, v, scale=None, workspace=None):
        if workspace is None:      # the eager call, as it has always been made: hip.attention is a seam that tools wrap with this signature
            return hip.attention(q, k, v, self.num_heads, scale=scale)
        return hip.attention(q, k, v, self.num_heads, scale=scale, workspace=workspace)


class SelfAttention(nn.Module):
    def __init__(self, dim, num_heads, eps=1e-6):
        super().__init__()
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.q, self.k, self.v, self.o = (nn.Linear(dim, dim) for _ in range(4))
        self.norm_q, self.norm_k = RMSNorm(dim, eps=eps), RMSNorm(dim, eps=eps)
        self.attn = AttentionModule(num_heads)


class CrossAttention(nn.Module):
    def __init__(self, dim, num_heads, eps=1e-6, has_image_input=False):
        super().__init__()
        if has_image_input:
            raise NotImplementedError("has_image_input=True (Wan2.1 I2V CLIP branch) is outside the TI2V-5B hot path")
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.q, self.k, self.v, self.o = (nn.Linear(dim, dim) for _ in range(4))
        self.norm_q, self.norm_k = RMSNorm(dim, eps=eps), RMSNorm(dim, eps=eps)
        self.has_image_input = has_image_input
        self.attn = AttentionModule(num_heads)


class DiTBlock(nn.Module):
    def __init__(self, has_image_input, dim, num_heads, ffn_dim, eps=1e-6):
        super().__init__()
        self.dim, self.num_heads, self.ffn_dim, self.eps = dim, num_heads, ffn_dim, eps
        self.self_attn = SelfAttention(dim, num_heads, eps)
        self.cross_attn = CrossAttention(dim, num_heads, eps, has_image_input=has_image_input)
        self.norm1 = nn.LayerNorm(dim, eps=eps, elementwise_affine=False)
        self.norm2 = nn.LayerNorm(dim, eps=eps, elementwise_affine=False)
        self.norm3 = nn.LayerNorm(dim, eps=eps)
        self.ffn = nn.Sequential(nn.Linear(dim, ffn_dim), nn.GELU(approximate="tanh"), nn.Linear(ffn_dim, dim))
        self.modulation = nn.Parameter(torch.randn(1, 6, dim) / dim ** 0.5)
        self._fused = None
        self._fp8 = None

    def fp8_weights(self, dtype):
        """The block's Linear weights cast to fp8 once (the reference casts on every call, core/vram/layers.py:342 — same
        values): [Wq;Wk;Wv], Wo, cross Wq, cross [Wk;Wv], cross Wo, ffn.0, ffn.2.  Rebuilt after load / LoRA fuse."""
        if self._fp8 is None or self._fp8[0] != dtype:
            wqkv, _, wkv_c, _ = self.fused_weights()
            sa, ca = self.self_attn, self.cross_attn
            ws = (wqkv, sa.o.weight, ca.q.weight, wkv_c, ca.o.weight, self.ffn[0].weight, self.ffn[2].weight)
            self._fp8 = (dtype, tuple(w.to(dtype).contiguous() for w in ws))
        return self._fp8[1]

    def fused_weights(self):
        """[Wq;Wk;Wv] and [Wk;Wv] (cross) concatenated once, so the three projections of a token tensor are
        ONE hipBLASLt GEMM.  Rebuilt after load_state_dict / LoRA fuse (see WanModel.invalidate_fused)."""
        if self._fused is None:
            sa, ca = self.self_attn, self.cross_attn
            self._fused = (
                torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], 0).contiguous(),
                torch.cat([sa.q.bias, sa.k.bias, sa.v.bias], 0).contiguous(),
                torch.cat([ca.k.weight, ca.v.weight], 0).contiguous(),
                torch.cat([ca.k.bias, ca.v.bias], 0).contiguous(),
            )
        return self._fused


class Head(nn.Module):
    def __init__(self, dim, out_dim, patch_size, eps):
        super().__init__()
        self.dim, self.patch_size, self.eps = dim, patch_size, eps
        self.norm = nn.LayerNorm(dim, eps=eps, elementwise_affine=False)
        self.head = nn.Linear(dim, out_dim * math.prod(patch_size))
        self.modulation = nn.Parameter(torch.randn(1, 2, dim) / dim ** 0.5)


class WanModel(nn.Module):
    def __init__(self, dim, in_dim, ffn_dim, out_dim, text_dim, freq_dim, eps, patch_size, num_heads, num_layers,
                 has_image_input, has_image_pos_emb=False, has_ref_conv=False, add_control_adapter=False,
                 in_dim_control_adapter=24, seperated_timestep=False, require_vae_embedding=True,
                 require_clip_embedding=True, fuse_vae_embedding_in_latents=False):
        super().__init__()
        if has_image_input or has_ref_conv or add_control_adapter:
            raise NotImplementedError("CLIP image branch / ref_conv / camera adapter belong to other Wan variants "
                                      "(out of scope: SURVEY.md §2.1 rows 12)")
        self.dim, self.in_dim, self.out_dim, self.freq_dim = dim, in_dim, out_dim, freq_dim
        self.num_heads, self.eps = num_heads, eps
        self.has_image_input = has_image_input
        self.patch_size = tuple(patch_size)
        self.seperated_timestep = seperated_timestep
        self.require_vae_embedding = require_vae_embedding
        self.require_clip_embedding = require_clip_embedding
        self.fuse_vae_embedding_in_latents = fuse_vae_embedding_in_latents
        self.has_image_pos_emb, self.has_ref_conv, self.control_adapter = has_image_pos_emb, has_ref_conv, None

        self.patch_embedding = nn.Conv3d(in_dim, dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.text_embedding = nn.Sequential(nn.Linear(text_dim, dim), nn.GELU(approximate="tanh"), nn.Linear(dim, dim))
        self.time_embedding = nn.Sequential(nn.Linear(freq_dim, dim), nn.SiLU(), nn.Linear(dim, dim))
        self.time_projection = nn.Sequential(nn.SiLU(), nn.Linear(dim, dim * 6))
        self.blocks = nn.ModuleList([DiTBlock(has_image_input, dim, num_heads, ffn_dim, eps) for _ in range(num_layers)])
        self.head = Head(dim, out_dim, self.patch_size, eps)
        self.freqs = precompute_freqs_cis_3d(dim // num_heads)
        self._rope_cache = {}
        # "f32" (default): RoPE as two fp32 FMAs on a table rounded once from the reference's complex128 one (the fp64
        # rotation costs 43 us of VALU per call on a 77 us HBM-bound kernel; < 0.2 % of the outputs move, by 1 bf16 ulp).
        # "f64": the reference's arithmetic exactly (rope_apply upcasts to complex128).
        self.rope_mode = "f32"
        # True (with rope_mode "f32" and the stock AttentionModule): self-attention's 1/sqrt(d) * log2(e) = 2^-3 * 1.0201 is split — the
        # 1.0201 goes into q's fp32 RoPE table (q is rounded to bf16 once, as before, from a value 2 % larger), attention is called with
        # scale' = 2^-3 / log2(e), for which the kernel's pre-multiplied form (64 VALU operations fewer per tile and wave, -4 % time) is
        # exact.  False: q as the reference rounds it, the kernel's plain form.
        self.fold_attn_scale = True
        # True: GELU(tanh) applied to the fp32 accumulator in the hipBLASLt epilogue of ffn.0 (one pass less over the
        # (n, ffn) tensor, -1.9 % per forward; verified to be the tanh form, tools/gelu_epilogue_check.py; <= 1 bf16 ulp
        # from the reference's "round, then GELU" order).  False: GEMM, then fg_act_bf16 on the rounded output.
        self.gelu_epilogue = True
        # hot-loaded (unfused) LoRA adapters: module name -> [(alpha*A (r,in), B (out,r)), ...]; see add_hot_lora
        self.hot_loras = {}
        # how the block Linears evaluate them: "torch" (default): _hot, the reference's arithmetic op by op on library GEMMs; "hip": the
        # adapters of a Linear stacked (stack_hot_loras) and applied by fg_lora_apply_bf16 next to the own GEMM's fused store, the bf16
        # GEMM's or, in the fp8 Linear mode, fg_gemm_fp8_bf16's (_BlockLinears.plain / .residual; the adapter reads the bf16 activation)
        # "fused": the adapters are folded into the weights one at a time (fg_lora_fuse_bf16) and the originals kept, so clear_hot_loras()
        # can put them back; hot_loras stays empty and the forward is the adapter-free one (add_hot_lora)
        self.hot_lora_backend = "torch"
        self._hot_packs = {}
        # backend "fused": module name -> the Linear's weight as it was before its first adapter
        self._fused_stash = {}
        # fp8 Linear mode of the blocks (None = bf16 GEMMs); see enable_fp8_linear
        self.fp8_dtype = None
        self._ones = {}
        # e4m3 Q K^T in self-attention (False = bf16); see enable_qk8_attention
        self.qk8_attention = False
        # ... with its operands written by the RMSNorm+RoPE pass (True) or by the quantise pass behind it (False); the same bits
        self.qk8_fused_producer = False
        # ... and with the P V product in e4m3 too (enable_qk8_attention(pv8=True)); False: P V in bf16
        self.pv8_attention = False
        # ... with V mean-smoothed in that product (enable_qk8_attention(pv8=True, smooth_v=True)); False: V quantised as it is
        self.smoothv_attention = False
        # ... and on token-sharded layouts (enable_qk8_attention(sharded=True)); False: an active shard raises
        self.qk8_sharded = False
        # ... and cross-attention in the e4m3 form too (enable_qk8_attention(pv8=True, cross=True)); False: cross-attention in bf16
        self.cross8_attention = False
        # ... with V of the context mean-smoothed in it (enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True)); False: as it is
        self.smoothv_cross_attention = False
        # a merged CFG call (cfg_merge=True) as ONE forward on x (2, N, dim) instead of two batch-1 forwards; see enable_stacked_cfg
        self.stacked_cfg = False
        # ... also when the blocks' Linears run in the fp8 mode (enable_stacked_cfg(fp8_linear=True)); False: that combination raises
        self.stacked_cfg_fp8 = False
        # ... also with unfused adapters on hot_backend="hip" (enable_stacked_cfg(hot_lora=True)); False: that combination raises
        self.stacked_cfg_hot_lora = False
        # ... with the two-row gated stores of the pair in ONE GEMM launch (enable_stacked_cfg(periodic_gate=True)); False: one per element
        self.stacked_cfg_periodic_gate = False
        # ... also on an active token shard of the K / V all-gather layout (enable_stacked_cfg(sharded=True)); False: an active shard raises
        self.stacked_cfg_sharded = False

    # ------------------------------------------------------------------ load-time hooks
    def invalidate_fused(self):
        for blk in self.blocks:
            blk._fused = None
            blk._fp8 = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_fused()
        self._fused_stash = {}      # the new weights are the new originals
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_fused()
        self._rope_cache = {}
        self._hot_packs = {}
        self._fused_stash = {name: fn(w) for name, w in self._fused_stash.items()}
        return out

    # ------------------------------------------------------------------ fp8 Linear mode (core/vram/layers.py:312,321-357)
    def enable_fp8_linear(self, dtype=torch.float8_e4m3fn):
        """Run the ten Linears of every DiT block like AutoWrappedLinear.fp8_linear when its computation_dtype is fp8:
        per-row dynamic activation scale (fg_fp8_quant_rows_bf16), weights cast to e4m3 with unit scale, bf16 bias,
        the row-scaled e4m3 matmul with bf16 output on fg_gemm_fp8_bf16 (or torch._scaled_mm: FAIRYGEN_FP8_GEMM=lib).  dtype None switches back to bf16 GEMMs.  The small
        embedding / head Linears (< 1 % of the FLOPs) stay bf16.  gfx950's fp8 GEMM takes the OCP format only, so
        torch.float8_e4m3fnuz (the MI300-era flavour the reference also accepts) is refused."""
        if dtype is not None and dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{dtype}: the gfx950 fp8 GEMM (hipBLASLt behind torch._scaled_mm) takes "
                                      "torch.float8_e4m3fn (OCP e4m3) only")
        self.fp8_dtype = dtype
        self.invalidate_fused()
        return self

    # ------------------------------------------------------------------ e4m3 Q K^T self-attention (models/wan_video_dit.py:48-52)
    def enable_qk8_attention(self, flag=True, fused_producer=False, pv8=False, sharded=False, cross=False, smooth_v=False,
                             smooth_v_cross=False):
        """Run self-attention of every block like the reference's flash_attention does when the sageattention package is present
        (sageattn(q, k, v)): Q K^T from e4m3 operands — K mean-smoothed with one scale per head, Q with one scale per row and head
        (fg_attn_quant_qk_bf16) — on fg_attn_fwd_qk8_bf16; softmax and P V as before, v in bf16.  Only the stock AttentionModule of
        self-attention over more than QK8_MIN_KV keys takes it; cross-attention (512 keys, 1.9 % of the attention FLOPs) stays bf16.
        q is then rounded as the reference rounds it (attn_scale: no factor folded into its RoPE table).  Composes with
        enable_fp8_linear, hot adapters and graph=True; token-sharded layouts raise unless sharded=True (below).
        fused_producer: the RMSNorm+RoPE pass itself writes the operands (fg_rmsnorm_rope_q8_bf16, fg_rmsnorm_rope_kstats_bf16,
        fg_attn_quant_k_bf16: q never exists as bf16, k is read once, not three times); False keeps the quantise pass behind the two
        norms, the form a plain call has always had and tests/test_attention_qk8.py pins to the oracle by its launches.  Both write the
        same bytes, so the forward does not depend on it; ModelConfig(attention_dtype=...) asks for the fused producers.
        pv8: the other half of sageattn on current parts — P V on the e4m3 MFMA as well (include/fairygen_hip_pv8.h): v leaves
        fg_attn_quant_vt_bf16 as e4m3 bytes, transposed, with one scale per head and channel, and fg_attn_fwd_pv8_bf16 takes the place of
        fg_attn_fwd_qk8_bf16.  It is a form of this mode (it needs flag), has its routing, works behind either producer path and
        composes with the same things; ModelConfig(attention_pv_dtype=...) asks for it.
        sharded: off by default, and then an active token shard raises.  True lets the mode (either form) run on a token-sharded layout
        whose total key count exceeds QK8_MIN_KV; a shorter sequence keeps the bf16 sharded path.  attn_mode="ulysses": a rank holds all N
        tokens of its heads behind the first all-to-all, every statistic is local, and the received views go through attention_qk8.
        attn_mode="allgather" (include/fairygen_hip_shard8.h): each rank reduces its rows to one record per block (per channel the fp64 key
        sum, the key minimum and maximum, the maximum of |v|: 20 * C bytes), the records are all-gathered, every rank derives the same key
        mean, sk and sv from them, and the K / V all-gather moves the e4m3 bytes (k8; with pv8 also v8) in place of bf16.  For any split
        of the rows the gathered operands and the scales are byte for byte those of the unsharded mode, where the fp64 key sum is exact
        (include/fairygen_hip.h); the attention kernels are the same.  Composes with enable_fp8_linear, hot adapters and cfg_parallel=2 (the
        shard is then the half-group); graph=True with a shard raises as before; attn_mode="windows" has no exchange in a forward and
        is not affected.  No multi-GPU hardware run of this project exists: the mode is tested with emulated ranks on one GPU.
        sharded="all": every e4m3 form that is switched on also runs on an active token shard — what True covers, and smooth_v, cross
        and smooth_v_cross, which True keeps refusing.  smooth_v on attn_mode="allgather" (include/fairygen_hip_shard8s.h): the record
        carries for v what it carries for k (fp64 sum, minimum, maximum: 32 * C bytes in place of 20 * C), every rank derives the
        unsharded mu and sv from the W records, v8 = e4m3((v - mu) / sv) crosses the wire and fg_attn_fwd_pv8s_bf16 adds mu back; the
        operands are byte for byte the unsharded smoothing producer's where the fp64 sums are exact.  On attn_mode="ulysses" it is
        local like every other statistic.  cross / smooth_v_cross: the context is whole on every rank and the kernel is row-wise in
        the queries, so a shard's queries give that shard's rows and nothing is exchanged.  A rank without rows launches nothing.
        Any other value of sharded raises ValueError; m.qk8_sharded holds the value given.
        cross: cross-attention over the text context in the e4m3 form as well, as the reference's sageattn call covers it
        (include/fairygen_hip_cross8.h).  It needs flag and pv8 (the operands are those of the e4m3 P V form).  Only the stock
        AttentionModule, one batch element and a context of at most hip.attention_cross8_max_kv() keys take it (takes_cross8_attention).
        The q norm writes e4m3 rows and their scales and no bf16 q (fg_rmsnorm_rope_q8_bf16 without a RoPE table); a block's context is
        quantised where its k | v rows are computed — once per denoise loop with a kv_cache, which then holds (k8, sk, v8t, sv) in place
        of (k, v); per call without one (sliding windows) — and fg_attn_fwd_cross8_bf16 keeps a head's K8 and V8^T in LDS while it walks
        the query blocks.  Composes with enable_fp8_linear, hot adapters and graph=True (the captured step owns the q8 / sq buffers, the
        context operands live in the loop's kv_cache).  An active token shard raises NotImplementedError, with sharded=True too:
        sharded="all" asks for it (above).
        smooth_v: off by default.  The e4m3 P V product with V mean-smoothed, what sageattn ships as smooth_v
        (include/fairygen_hip_smoothv.h): the key mean of every head and channel leaves v before it is quantised
        (fg_attn_quant_vt_smooth_bf16 in place of fg_attn_quant_vt_bf16) and joins the output row in fp32 before its rounding to bf16
        (fg_attn_fwd_pv8s_bf16 in place of fg_attn_fwd_pv8_bf16), so the rounding of P no longer scales the part of V that all keys
        share and the e4m3 range covers the spread alone.  It needs pv8 (ValueError without), has its routing, works behind either
        producer path and composes with enable_fp8_linear, hot adapters, graph=True (the captured step owns mu next to sv) and the
        stacked CFG forward (the batched entry points).  It does not run on token shards with sharded=True or False: the mean spans
        every rank's keys and the statistics record of include/fairygen_hip_shard8.h carries no V sum — together with sharded=True it
        raises ValueError here, and an active shard raises NotImplementedError at the forward; sharded="all" exchanges the record that
        has one (above).  With cross=True it smooths self-attention
        only: the e4m3 cross-attention has a switch of its own (below).
        smooth_v_cross: off by default, independent of smooth_v.  The same smoothing for the e4m3 cross-attention
        (include/fairygen_hip_cross8s.h): the context is zeroed behind the prompt's length and the k / v Linears act row by row, so most
        of its 512 keys carry one V row, which the unsmoothed recipe returns scaled by P's rounding defect.  With it a block's context
        goes through fg_attn_quant_vt_smooth_bf16, the kv_cache holds (k8, sk, v8t, sv, mu), still quantised once per denoise loop, and
        fg_attn_fwd_cross8s_bf16 (batched: _b, the stacked CFG forward) takes the place of fg_attn_fwd_cross8_bf16.  It needs flag, pv8
        and cross (ValueError without, and nothing changes); composes with what cross composes with, graph=True included (the context
        is quantised in the eager first step, replays only read it); an active token shard raises as for cross, and runs as cross
        does with sharded="all"."""
        if pv8 and not flag:
            raise ValueError("enable_qk8_attention(pv8=True) needs the e4m3 Q K^T mode on (flag=True)")
        if not (isinstance(sharded, bool) or sharded == "all"):
            raise ValueError(f"enable_qk8_attention(sharded={sharded!r}): sharded is False, True (self-attention qk8 / pv8 on token shards) or "
                             "'all' (every e4m3 form that is switched on)")
        if sharded and not flag:
            raise ValueError("enable_qk8_attention(sharded=True) needs the e4m3 Q K^T mode on (flag=True)")
        if cross and not (flag and pv8):
            raise ValueError("enable_qk8_attention(cross=True) needs the e4m3 Q K^T mode and its e4m3 P V form on (flag=True, pv8=True)")
        if smooth_v and not (flag and pv8):
            raise ValueError("enable_qk8_attention(smooth_v=True) needs the e4m3 Q K^T mode and its e4m3 P V form on (flag=True, pv8=True): "
                             "it is V of that product that is mean-smoothed")
        if smooth_v and sharded is True:
            raise ValueError("enable_qk8_attention(smooth_v=True, sharded=True): the key mean of V spans every rank's keys and the statistics "
                             "record of the sharded mode (include/fairygen_hip_shard8.h) has no V sum; run token shards without smooth_v, or "
                             "with sharded='all' (the record of include/fairygen_hip_shard8s.h)")
        if smooth_v_cross and not (flag and pv8 and cross):
            raise ValueError("enable_qk8_attention(smooth_v_cross=True) needs the e4m3 cross-attention on (flag=True, pv8=True, cross=True): "
                             "it is V of that product that is mean-smoothed")
        self.qk8_attention = bool(flag)
        self.qk8_fused_producer = bool(flag) and bool(fused_producer)
        self.pv8_attention = bool(flag) and bool(pv8)
        self.qk8_sharded = sharded if flag else False      # False, True or "all"
        self.cross8_attention = bool(flag) and bool(pv8) and bool(cross)
        self.smoothv_attention = bool(flag) and bool(pv8) and bool(smooth_v)
        self.smoothv_cross_attention = self.cross8_attention and bool(smooth_v_cross)
        return self

    # ------------------------------------------------------------------ the stacked CFG forward
    def enable_stacked_cfg(self, flag=True, fp8_linear=False, hot_lora=False, periodic_gate=False, sharded=False):
        """Opt-in, off by default: a merged CFG call (cfg_merge=True: the positive and the negative context batched, wan_video.py
        model_fn_wan_video_steps) runs ONE forward on the residual stream (2, N, dim) instead of two batch-1 forwards one after the other.
        The time rows, the modulation tables and the RoPE tables are one element's and shared; the row kernels that read them take the
        batch through include/fairygen_hip_rowbatch.h; the plain Linears, the ungated residual store and the gated one with a single gate
        row run on 2 N rows in one GEMM; the gated store with two gate rows (TI2V) is launched per element (_BlockLinears.residual);
        attention runs with B = 2 — bf16, or with the e4m3 modes on the batched entry points of include/fairygen_hip_batch8.h.  Block 0's
        self-attention half does not see the context and is computed once on N rows (CFG_SHARE_PREFIX).  With the switch off every path
        is what it was.  What it does not take raises NotImplementedError at the merged call (check_stacked_cfg).  DESIGN.md §5.
        fp8_linear: off by default, and then a model in the fp8 Linear mode (enable_fp8_linear) raises at the merged call.  True lets the
        stacked forward run in that mode too: the norms that hand their row to an fp8 Linear take the batch through
        include/fairygen_hip_rowbatch8.h and leave ONE (2 N, C) e4m3 operand with its 2 N row scales, every fp8 Linear is one GEMM on 2 N
        rows (the context's k | v on 2 L), the per-row quantisation in front of o and ffn.2 is one pass over 2 N rows, and the gates run
        on the batched row kernels — as in the batch-1 fp8 forward, none of them in a GEMM's store.  FAIRYGEN_FP8_FOLD=0 (bf16 norms, then
        the quantisation pass) works stacked as well.
        hot_lora: off by default, and then a model with unfused hot-loaded adapters raises at the merged call.  True lets the stacked
        forward run with adapters on hot_backend="hip" (hot_backend="torch" keeps raising): the adapter kernel and the two-output
        modulate norm take the batch through include/fairygen_hip_lorabatch.h — one fg_lora_apply_bf16_b launch per adapted Linear, its
        gate rule counted inside the element — and in the fp8 Linear mode (with fp8_linear=True) the gated store of fg_gemm_fp8_bf16 is
        launched per element where the gate table has two rows (_BlockLinears.residual).  Linears whose shapes the kernel refuses take
        the reference's torch ops, which are row-wise.  Like fp8_linear it is stated with every call: a call that does not restate it
        clears it, and enable_stacked_cfg(False) clears all three.
        periodic_gate: off by default, and then nothing changes.  True runs the gated store with two gate rows (TI2V: self_attn.o and
        ffn.2) as ONE launch on the 2 N rows instead of one per element: fg_gemm_epilogue_bf16_sp / fg_gemm_fp8_bf16_sp
        (include/fairygen_hip_gategemm.h) read the gate row by the row inside the element, rows_per_element = N — the same kernel body
        with another row rule, the same rounding points; the unit plan is that of 2 N rows, so the fp32 summation order of the tiles
        that end up as k-range pieces may differ from the per-element launches'.  Composes with fp8_linear and hot_lora (the adapter
        launch behind the store is unchanged); stated with every call like them.  Elements below 256 rows keep the per-element launches.
        sharded: off by default, and then an active token shard raises at the merged call.  True lets the merged call on an active token
        shard of the K / V all-gather layout (attn_mode="allgather", cfg_parallel=1) run ONE stacked forward on the rank's rows, residual
        stream (2, n_local, dim): the local rows and RoPE rows are sliced as for a batch-1 forward, block 0's shared self-attention half
        runs once with B = 1 exchanges, every later block's exchange carries both elements — one per block in bf16; two with the e4m3
        modes (enable_qk8_attention(sharded=True) or sharded="all"), the statistics records then come from the batched producers of
        include/fairygen_hip_shard8b.h — so a block has as many exchanges as in a batch-1 forward, and a rank without rows sends B neutral
        records and no rows; the head output (2, n_local, out) is all-gathered where the caller asks.  Composes with fp8_linear and
        periodic_gate, which are row-wise (periodic_gate: rows_per_element is n_local; below 256 rows the per-element launches stay).
        Not carried, and refused by check_stacked_cfg on an active shard: unfused hot-loaded adapters (hot_lora) — open work, the adapter
        launches are row-wise and expected to compose, but that has not been run or tested; and the fp8 Linear mode TOGETHER with any e4m3
        attention form (enable_qk8_attention on, with or without pv8 / smooth_v / cross) — fp8 Linears with the full e4m3 stack measured
        0.119 from the unsharded stacked forward against the 0.0745 bound of tests/test_stacked_cfg_sharded.py, cause not established, and
        fp8 Linears with qk8 / pv8 alone were never run.  fp8_linear with bf16 attention and the e4m3 forms with bf16 Linears are taken
        and tested.  attn_mode="ulysses" raises (the grouped
        RMSNorm+RoPE destination has no batched form), and so do attn_mode="windows", cfg_parallel=2 with cfg_merge, graph=True with a
        shard and TeaCache, as without the switch.  Stated with every call like the others.  No multi-GPU hardware run exists: the ranks
        are emulated on one GPU (tests/test_stacked_cfg_sharded.py)."""
        self.stacked_cfg = bool(flag)
        self.stacked_cfg_fp8 = bool(flag) and bool(fp8_linear)
        self.stacked_cfg_hot_lora = bool(flag) and bool(hot_lora)
        self.stacked_cfg_periodic_gate = bool(flag) and bool(periodic_gate)
        self.stacked_cfg_sharded = bool(flag) and bool(sharded)
        return self

    def check_stacked_cfg(self, context_batch, shard=None, sliding_window=False):
        """What a merged call must not meet while enable_stacked_cfg is on; decided on the host before anything is launched.  The fp8 Linear
        mode passes only with enable_stacked_cfg(fp8_linear=True), unfused adapters only on hot_backend="hip" with
        enable_stacked_cfg(hot_lora=True), an active token shard only on the K / V all-gather layout with enable_stacked_cfg(sharded=True);
        everything else raises with them as without."""
        if self.fp8_dtype is not None and not self.stacked_cfg_fp8:
            raise NotImplementedError("stacked_cfg with enable_fp8_linear: the stacked forward takes the fp8 Linear mode only when it is asked "
                                      "to, enable_stacked_cfg(fp8_linear=True)")
        if self.hot_loras and not self.stacked_cfg_hot_lora:
            raise NotImplementedError(f"stacked_cfg with hot-loaded adapters on hot_backend={self.hot_lora_backend!r}: fg_lora_apply_bf16's gate "
                                      "has no batched form; hot_backend='fused' adapters are plain weights and work")
        if self.hot_loras and self.hot_lora_backend != "hip":
            raise NotImplementedError(f"stacked_cfg(hot_lora=True) with hot-loaded adapters on hot_backend={self.hot_lora_backend!r}: the stacked "
                                      "forward takes unfused adapters on hot_backend='hip' only (fg_lora_apply_bf16_b); hot_backend='fused' "
                                      "adapters are plain weights and work")
        if shard is not None and shard.active and not self.stacked_cfg_sharded:
            raise NotImplementedError("stacked_cfg with an active token shard: the stacked forward has no exchange")
        if shard is not None and shard.active and self.hot_loras:
            raise NotImplementedError("stacked_cfg(sharded=True) with unfused hot-loaded adapters: open work, not a limit of the kernels — the "
                                      "adapter launches are row-wise and are expected to compose, but the stacked forward has not been run or "
                                      "tested with adapters on token shards; hot_backend='fused' adapters are plain weights and work")
        if shard is not None and shard.active and self.fp8_dtype is not None and self.qk8_attention:
            raise NotImplementedError("stacked_cfg(sharded=True) with enable_fp8_linear AND enable_qk8_attention: the fp8 Linears together with "
                                      "an e4m3 attention form are not carried on token shards — with the full e4m3 stack the stacked forward "
                                      "on emulated ranks was 0.119 from the unsharded stacked forward against a bound of 0.0745, cause not "
                                      "established; run the shard with one of the two (fp8 Linears with bf16 attention, or e4m3 attention "
                                      "with bf16 Linears)")
        if shard is not None and shard.active and shard.attn_mode == "ulysses":
            raise NotImplementedError("stacked_cfg(sharded=True) with attn_mode='ulysses': the grouped RMSNorm+RoPE destination of the all-to-all "
                                      "send buffer has no batched form; the stacked forward runs on the K / V all-gather layout "
                                      "(attn_mode='allgather')")
        if shard is not None and shard.active and shard.attn_mode != "allgather":
            raise NotImplementedError(f"stacked_cfg(sharded=True) with attn_mode={shard.attn_mode!r}: windows are not part of the batch; the "
                                      "stacked forward runs on the K / V all-gather layout (attn_mode='allgather')")
        if sliding_window:
            raise NotImplementedError("stacked_cfg with sliding windows: windows are not part of the batch")
        if context_batch != 2:
            raise NotImplementedError(f"stacked_cfg stacks the CFG pair: a context batch of 2, not {context_batch}")

    def check_qk8_layout(self, shard):
        """What an active token shard must not meet: the e4m3 mode without sharded=, and smooth_v, cross and smooth_v_cross (which needs
        cross) without sharded="all"."""
        every = self.qk8_sharded == "all"
        if self.smoothv_attention and not every and shard is not None and shard.active:
            raise NotImplementedError("enable_qk8_attention(smooth_v=True) with a token-sharded layout: the key mean of V spans every rank's "
                                      "keys and the statistics record of the sharded mode has no V sum; switch it off (smooth_v=False) for a "
                                      "sharded run, or ask for the record that has one (sharded='all')")
        if self.cross8_attention and not every and shard is not None and shard.active:
            raise NotImplementedError("enable_qk8_attention(cross=True) with a token-sharded layout: the e4m3 cross-attention has not been "
                                      "run on token shards; switch it off (cross=False) for a sharded run, or ask for it (sharded='all')")
        if self.qk8_attention and not self.qk8_sharded and shard is not None and shard.active:
            raise NotImplementedError("enable_qk8_attention() with a token-sharded layout: the key mean and the per-head key scale of the e4m3 "
                                      "Q K^T form span all ranks' tokens and would need a collective; enable_qk8_attention(sharded=True) "
                                      "runs that exchange")

    def _scaled_linear(self, xq, scale_a, w8, bias, batch=1, **state):
        """fp8_linear's matmul (:347-354: torch._scaled_mm with row-wise scale_a, unit scale_b, bf16 bias, bf16 out): on this repo's e4m3
        MFMA kernel (fg_gemm_fp8_bf16), or — FAIRYGEN_FP8_GEMM=lib, and for shapes the kernel does not take — the library call itself.
        (1, rows, N); batch=B (a stacked forward): (B, rows / B, N) from the one matmul on all rows."""
        n = w8.shape[0]
        if fp8_own_ok(n, xq.shape[1]):
            return gemm_fp8_own(xq, scale_a, w8, bias, **({"batch": batch} if batch > 1 else {}), **state)
        key = (n, xq.device)
        if key not in self._ones:
            self._ones[key] = torch.ones((1, n), dtype=torch.float32, device=xq.device)
        return torch._scaled_mm(xq, w8.T, scale_a=scale_a, scale_b=self._ones[key], bias=bias,
                                out_dtype=torch.bfloat16).view(batch, xq.shape[0] // batch, n)

    # ------------------------------------------------------------------ hot-loaded LoRA (core/vram/layers.py:417-436)
    def check_hot_backend(self, backend):
        """Adapters of the restorable fused backend and unfused ones do not mix on one module: the stash must stay the adapter-free weight."""
        if backend == "fused" and self.hot_loras:
            raise ValueError(f"hot_backend='fused' while unfused ('torch' / 'hip') adapters are attached to {len(self.hot_loras)} Linears: "
                             "call clear_lora() first")
        if backend != "fused" and getattr(self, "_fused_stash", None):
            raise ValueError(f"hot_backend={backend!r} while restorable fused adapters are attached to {len(self._fused_stash)} Linears: "
                             "call clear_lora() first")

    def add_hot_lora(self, name, lora_a, lora_b, alpha=1.0):
        """Attach an adapter to Linear `name` ("blocks.3.self_attn.q", ...) so that clear_hot_loras() can remove it again.
        hot_lora_backend "torch" / "hip": unfused; the Linear's output becomes linear(x) + x @ A^T @ B^T, evaluated left to right in the
        pipeline dtype like AutoWrappedLinear.lora_forward (`lora_a` already carries alpha, base_pipeline.py:258; `alpha` stays 1).
        "fused": the weight becomes bf16(w + bf16(alpha * bf16(B A))), fuse_lora_to_base_model's arithmetic (`lora_a` WITHOUT alpha: the
        reference rounds alpha * (B A) after the product), and the original is kept on the device (_fuse_hot).  Adapters stack."""
        try:
            mod = self.get_submodule(name)
        except AttributeError:
            mod = None
        if not isinstance(mod, nn.Linear):
            raise KeyError(f"{name} is not a Linear of this model")
        if lora_a.shape[1] != mod.in_features or lora_b.shape[0] != mod.out_features or lora_a.shape[0] != lora_b.shape[1]:
            raise ValueError(f"LoRA shapes {tuple(lora_a.shape)}, {tuple(lora_b.shape)} do not fit {name} "
                             f"({mod.in_features} -> {mod.out_features})")
        backend = getattr(self, "hot_lora_backend", "torch")
        self.check_hot_backend(backend)
        w = mod.weight
        lora_a, lora_b = lora_a.to(device=w.device, dtype=w.dtype), lora_b.to(device=w.device, dtype=w.dtype)
        self._hot_packs = {}
        if backend == "fused":
            return self._fuse_hot(name, w, lora_a, lora_b, alpha)
        if alpha != 1.0:
            raise ValueError("add_hot_lora: on the unfused backends lora_a carries alpha; `alpha` is for hot_lora_backend 'fused'")
        self.hot_loras.setdefault(name, []).append((lora_a.contiguous(), lora_b.contiguous()))

    def _block_copies(self, name):
        """The derived copies that hold the weight of block Linear `name`: (block, slot and first row in DiTBlock.fused_weights() or None,
        slot and first row in DiTBlock.fp8_weights()); None for a Linear outside the blocks, which has no copies."""
        parts = name.split(".")
        if parts[0] != "blocks" or len(parts) != 4:
            return None
        blk, dim = self.blocks[int(parts[1])], self.dim
        where = {"self_attn.q": (0, 0, 0, 0), "self_attn.k": (0, dim, 0, dim), "self_attn.v": (0, 2 * dim, 0, 2 * dim), "self_attn.o": (None, 0, 1, 0),
                 "cross_attn.q": (None, 0, 2, 0), "cross_attn.k": (2, 0, 3, 0), "cross_attn.v": (2, dim, 3, dim), "cross_attn.o": (None, 0, 4, 0),
                 "ffn.0": (None, 0, 5, 0), "ffn.2": (None, 0, 6, 0)}.get(parts[2] + "." + parts[3])
        return where and (blk,) + where

    @torch.no_grad()
    def _fuse_hot(self, name, w, lora_a, lora_b, alpha):
        """hot_lora_backend "fused": one adapter into the weight `w` of Linear `name`, in place, with the original stashed before the first.
        fg_lora_fuse_bf16 where it takes the Linear (bf16, features in 64s, rank up to 128), else — and for every Linear with
        FAIRYGEN_LORA_FUSE=torch — the reference's torch ops on the device.  The block's derived copies follow: the kernel writes the e4m3 copy along with the weight where one exists, the rows in the
        fused QKV / cross KV weight are copied from the new weight; on the torch-op path the block's copies are dropped and rebuilt by the
        next forward."""
        if w.device.type != "cuda":
            raise hip.HipLibraryError(f"add_hot_lora: hot_backend='fused' rewrites weights on a HIP device, {name} is on {w.device} (no CPU fallback)")
        if name not in self._fused_stash:
            self._fused_stash[name] = w.detach().clone()
        n, k = w.shape
        rank = lora_a.shape[0]
        copies = self._block_copies(name)
        if LORA_FUSE == "hip" and w.dtype == torch.bfloat16 and w.is_contiguous() and hip.lora_fuse_ok(n, k, rank):
            r = -(-rank // hip.LORA_RANK_TILE) * hip.LORA_RANK_TILE
            if r == rank:
                a_t, b = lora_a.T.contiguous(), lora_b.contiguous()
            else:
                a_t, b = torch.zeros((k, r), dtype=w.dtype, device=w.device), torch.zeros((n, r), dtype=w.dtype, device=w.device)
                a_t[:, :rank], b[:, :rank] = lora_a.T, lora_b
            w8 = None
            if copies is not None and copies[0]._fp8 is not None:
                w8 = copies[0]._fp8[1][copies[3]][copies[4]:copies[4] + n]
            hip.lora_fuse(w.data, a_t, b, alpha, out_fp8=w8)
            if copies is not None and copies[1] is not None and copies[0]._fused is not None:
                copies[0]._fused[copies[1]][copies[2]:copies[2] + n].copy_(w)
        else:
            w.add_(alpha * torch.mm(lora_b, lora_a))
            if copies is not None:
                copies[0]._fused = copies[0]._fp8 = None

    @torch.no_grad()
    def clear_hot_loras(self):
        """Drop every adapter attached through add_hot_lora: the unfused ones are forgotten, the weights of the "fused" backend get their
        stashed originals back (bit for bit).  Returns the number of Linears that carried one."""
        n = len(self.hot_loras) + len(self._fused_stash)
        self.hot_loras = {}
        self._hot_packs = {}
        if self._fused_stash:
            for name, w0 in self._fused_stash.items():
                self.get_submodule(name).weight.copy_(w0)
            self._fused_stash = {}
            self.invalidate_fused()
        return n

    def _hot(self, name, x, out):
        """out (+)= sum of the adapters of `name` applied to x; `out` may be a column slice of a fused projection."""
        for a, b in self.hot_loras.get(name, ()):
            out += (x @ a.T) @ b.T
        return out

    def _hot_pack(self, names):
        """hot_lora_backend "hip": the stacked operands (A, B) of the Linears `names` (one, or q, k, v of a block: column groups of one
        output that share the input), built once and kept until the adapters or the device change.  None: no adapter on any of them.
        False: shapes fg_lora_apply_bf16 refuses (stacked rank above 128, in- or out-features not a multiple of 64) — the caller takes
        the "torch" path for that Linear."""
        if names not in self._hot_packs:
            per_group = [self.hot_loras.get(n, ()) for n in names]
            pack = None
            if any(per_group):
                ws = [self.get_submodule(n).weight for n in names]
                fits = all(w.shape == ws[0].shape and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0 for w in ws) and len(names) <= hip.LORA_MAX_GROUPS
                pack = (fits and stack_hot_loras(per_group, [(w.shape[1], w.shape[0]) for w in ws], ws[0].device, ws[0].dtype)) or False
            self._hot_packs[names] = pack
        return self._hot_packs[names]

    def _hot_apply(self, names, x, out, pack, batch=None):
        """out += the adapters of the Linears `names` (column groups of out) applied to x.  pack: what _hot_pack(names) gave — one
        fg_lora_apply_bf16 launch (batch=B, a stacked forward: fg_lora_apply_bf16_b on x, out (B, rows, .)); False — _hot per Linear on
        its column slice (row-wise torch ops, any leading shape); None — nothing to add."""
        if pack:
            return hip.lora_apply(x, pack[0], pack[1], out, groups=len(names), mode="add", batch=batch)
        if pack is False:
            c = out.shape[-1] // len(names)
            for j, nm in enumerate(names):
                self._hot(nm, x, out[..., j * c:(j + 1) * c])
        return out

    # ------------------------------------------------------------------ host-side tables
    def rope_tables(self, f, h, w, device):
        """(cos, sin) of the per-token complex table, tokens frame-major (pipelines/wan_video.py:1271-1275): two fp64
        (N, 64) tensors in rope_mode "f64"; in rope_mode "f32" two interleaved fp32 (N, 64, 2) tensors {cos, sin}: the table for k and
        the table for q (the same one, or multiplied by the folded softmax-scale factor: attn_scale())."""
        fold = self.attn_scale()[1]
        key = (f, h, w, str(device), self.rope_mode, fold)
        if key not in self._rope_cache:
            tab = torch.cat([
                self.freqs[0][:f].view(f, 1, 1, -1).expand(f, h, w, -1),
                self.freqs[1][:h].view(1, h, 1, -1).expand(f, h, w, -1),
                self.freqs[2][:w].view(1, 1, w, -1).expand(f, h, w, -1),
            ], dim=-1).reshape(f * h * w, -1)
            if self.rope_mode == "f32":
                cs = torch.stack([tab.real, tab.imag], dim=-1)
                cs_k = cs.to(torch.float32).contiguous().to(device)
                self._rope_cache = {key: (cs_k, cs_k if fold == 1.0 else (cs * fold).to(torch.float32).contiguous().to(device))}
            else:
                self._rope_cache = {key: (tab.real.contiguous().to(device), tab.imag.contiguous().to(device))}
        return self._rope_cache[key]

    def attn_scale(self):
        """(scale passed to self-attention or None for 1/sqrt(d), factor folded into q's RoPE table)."""
        if self.qk8_attention:      # the fold is a device of the bf16 kernel's pre-multiplied form: plain q, 1/sqrt(d) said out loud
            return float(self.dim // self.num_heads) ** -0.5, 1.0
        if self.fold_attn_scale and self.rope_mode == "f32" and all(type(b.self_attn.attn) is AttentionModule for b in self.blocks):
            return hip.pow2_softmax_scale(self.dim // self.num_heads)
        return None, 1.0

    def patchify(self, x):
        """Conv3d with kernel == stride == (1,p,p) is a GEMM over unfolded patches; returns frame-major
        tokens (b, f*h*w, dim) and the grid (reference :338-344 + pipelines/wan_video.py:1260-1261)."""
        b, c, t, hh, ww = x.shape
        pt, ph, pw = self.patch_size
        f, h, w = t // pt, hh // ph, ww // pw
        cols = x.view(b, c, f, pt, h, ph, w, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(b, f * h * w, c * pt * ph * pw)
        wmat = self.patch_embedding.weight.view(self.dim, -1)
        return F.linear(cols, wmat, self.patch_embedding.bias), (f, h, w)

    def unpatchify(self, x, grid_size):
        """'b (f h w) (x y z c) -> b c (f x) (h y) (w z)' (reference :346-351)."""
        f, h, w = grid_size
        px, py, pz = self.patch_size
        b = x.shape[0]
        x = x.view(b, f, h, w, px, py, pz, self.out_dim).permute(0, 7, 1, 4, 2, 5, 3, 6)
        return x.reshape(b, self.out_dim, f * px, h * py, w * pz)

    def _empty_rank_steps(self, x, blocks, shard, shard_total, att, cfg_prefix, nb=1):
        """The forward of a rank of the K / V all-gather layout that holds no token rows (the ceil split leaves trailing ranks empty when
        N is small against the world): it launches nothing, takes its part in every exchange of every block — the neutral statistics
        record and no k8 / v rows in the e4m3 form, no k / v rows in bf16 — in the order the other ranks run them, cfg_prefix included,
        and returns an empty head output (1, 0, out).  nb > 1 (the stacked CFG forward on the shard): the exchanges carry nb elements —
        nb neutral records, no rows — except block 0's when x is one element (its shared self-attention half runs with B = 1 exchanges
        on every rank); the head output is (nb, 0, out)."""
        c = self.dim
        for i, blk in enumerate(blocks):
            qkv = x.new_empty((x.shape[0] if i == 0 else nb, 0, 3 * c))
            if cfg_prefix is not None and i == 0:
                if "owner" in cfg_prefix:      # the other branch of the step runs block 0's exchanges
                    while "x_sa" not in cfg_prefix:
                        yield i
                    cfg_prefix.pop("x_sa")
                    cfg_prefix["taken"] = True
                    continue
                cfg_prefix["owner"] = True
            if takes_qk8_attention(self, blk.self_attn.attn, shard_total, 1):
                yield from att._shard8_steps(i, blk.self_attn, qkv, None, None, None, shard, shard_total)
            else:
                pending = shard.all_gather_kv_async(qkv[..., c:2 * c], qkv[..., 2 * c:], shard_total)
                yield i
                pending.wait()
            if cfg_prefix is not None and i == 0:
                cfg_prefix["x_sa"] = x
        return x.new_empty((nb, 0, self.head.head.weight.shape[0]))

    def _self_attention_steps(self, i, blk, mod, x, h, cos, sin, shard, shard_total, lin, att, w8, norm3=True):
        """Block i's self-attention half (reference :139-146, :225-226): h = modulate(norm1(x)) in (an Act); returns the residual stream
        after x += gate_msa * o(attn(...)) and h = norm3(x).  Yields right after each exchange of a token-sharded run has been started.
        lin, att: the _BlockLinears and _BlockAttention of this forward; w8: the block's e4m3 weights (Nones in bf16 mode).  norm3=False: no
        h (returns None for it): the stacked forward computes block 0's half once and norms the copies.  x (B, n, dim) with B > 1 (the
        stacked forward, unsharded): the RoPE tables are one element's, the norm kernels and attention take the batch."""
        wqkv, bqkv, _, _ = blk.fused_weights()
        sa = blk.self_attn
        # one GEMM for q | k | v, and one adapter launch on the fused buffer (hip backend) or one per projection on its column slice
        qkv = lin.plain(h, tuple(f"blocks.{i}.self_attn.{nm}" for nm in "qkv"), wqkv, bqkv, w8[0], own=GEMM_BACKEND == "all")
        # rope tables per operand: fp64 (cos, sin) for both, or the fp32 interleaved tables of k and q (rope_tables)
        rk, rq = ((cos, None), (sin, None)) if cos.dtype == torch.float32 else ((cos, sin), (cos, sin))
        scale = self.attn_scale()[0]      # None (1/sqrt(d)), or the power-of-two form that goes with the pre-multiplied q table
        a = yield from att.self_attention_steps(i, sa, qkv, rq, rk, scale, shard, shard_total)
        # x += gate_msa*y ; h = norm3(x)  (reference :225-226)
        return lin.residual(x, a, f"blocks.{i}.self_attn.o", sa.o.weight, sa.o.bias, w8[1], mod, 2, affine=blk.norm3 if norm3 else None)

    # ------------------------------------------------------------------ the 30-block token forward
    def forward_tokens(self, x, context, mod_rows_t, t_rows, first_rows, rope, shard=None, shard_total=None, tea_cache=None,
                       skip_blocks=False, cfg_prefix=None, kv_cache=None, owned=None):
        """Run forward_tokens_steps to completion (single branch)."""
        gen = self.forward_tokens_steps(x, context, mod_rows_t, t_rows, first_rows, rope, shard, shard_total, tea_cache, skip_blocks,
                                        cfg_prefix, kv_cache, owned)
        while True:
            try:
                next(gen)
            except StopIteration as done:
                return done.value

    def forward_tokens_steps(self, x, context, mod_rows_t, t_rows, first_rows, rope, shard=None, shard_total=None,
                             tea_cache=None, skip_blocks=False, cfg_prefix=None, kv_cache=None, owned=None):
        """Generator form of the 30-block forward: yields right after each of a block's exchanges has been STARTED
        (token-sharded runs only: the K/V all-gather, or the two Ulysses all-to-alls), so a driver can interleave two
        independent forwards (the CFG branches) and let one branch's compute hide the other's xGMI traffic.
        Returns (StopIteration.value) the head output.

        x (1,n,dim) local tokens; context (1,L,dim) embedded text; t_rows (R,dim) distinct time embeddings
        (R = 1 or 2), mod_rows_t (R,6,dim) their projections; tokens < first_rows use row 0.
        rope = (cos, sin) for the LOCAL tokens.  shard: optional fairygen_amd.sequence_parallel.TokenShard —
        its attn_mode picks the exchange around self-attention (shard_total = N, all ranks' tokens).
        tea_cache / skip_blocks: the wan_video.TeaCache of this CFG branch and its verdict for this step — a skipped step
        re-applies the cached residual instead of running the 30 blocks, a computed one stores the new residual
        (pipelines/wan_video.py:1297-1300,1316-1317,1375-1376).
        cfg_prefix: a dict shared by the forwards of ONE denoise step that differ only in `context` (the CFG branches,
        pipelines/wan_video.py:296-301).  Nothing before block 0's cross-attention sees the context, so the residual stream after
        block 0's self-attention (norm1 + modulate, qkv, RMSNorm + RoPE, attention and its exchanges, o, gate) is the same tensor in
        both: the first forward to get there leaves a copy, the other one takes it instead of computing it (bit-identical: the
        kernels are deterministic).  A forward that arrives while the other is still inside that self-attention (lockstep
        interleave) yields until the copy is there.
        kv_cache: a dict that lives as long as `context` and the weights stay what they are (one denoise loop): block i's
        cross-attention keys (after norm_k) and values depend on nothing else, so they are computed at the first step and read
        back at the others (reference :172-177 recomputes them every step).
        owned: the scheduler block and scratch of a caller that records this forward into a graph (_BlockLinears.owned; same bits).
        The stacked CFG forward (enable_stacked_cfg): context (2, L, dim), everything else ONE element's.  x (1, n, dim): block 0's
        self-attention half, which does not see the context, is computed once on n rows and copied into both halves of the (2, n, dim)
        residual stream; x (2, n, dim): that half runs stacked as well.  Returns the head output (2, n, out).  With
        enable_stacked_cfg(sharded=True) and an active shard of the K / V all-gather layout, x is the rank's rows and every exchange of a
        stacked block carries both elements (_BlockAttention.self_attention_steps)."""
        eps = self.eps
        cos, sin = rope
        x = x.contiguous()
        nb = context.shape[0]
        sharded = shard is not None and shard.active
        if nb > 1 and (not self.stacked_cfg or x.shape[0] not in (1, nb) or tea_cache is not None or cfg_prefix is not None or owned is not None
                       or (sharded and not (self.stacked_cfg_sharded and shard.attn_mode == "allgather"))):
            raise ValueError("forward_tokens_steps: a context batch is the stacked CFG forward (enable_stacked_cfg): unsharded — or, with "
                             "enable_stacked_cfg(sharded=True), on the K / V all-gather layout — no TeaCache, no cfg_prefix, not recorded")
        blocks = list(self.blocks)
        if skip_blocks:
            blocks, x = [], tea_cache.update(x)
        fp8 = self.fp8_dtype
        self.check_qk8_layout(shard)
        lin = _BlockLinears(self, mod_rows_t.shape[0], owned)      # the mode decisions of this forward: the Linears and norms,
        att = _BlockAttention(self, lin, owned)                    # and attention
        if x.shape[1] == 0 and tea_cache is None and shard is not None and shard.active and shard.attn_mode == "allgather":
            return (yield from self._empty_rank_steps(x, blocks, shard, shard_total, att, cfg_prefix, nb))
        ctx = Act(context, hip.fp8_quant_rows(context) if fp8 is not None else None)      # the text context is the same for all blocks
        mods = [hip.ModTable((blk.modulation.to(mod_rows_t.dtype) + mod_rows_t).contiguous(), first_rows) for blk in blocks]
        h = lin.modulate(x, mods[0], 0, 1) if blocks else None
        for i, blk in enumerate(blocks):
            mod = mods[i]
            _, _, wkv_c, bkv_c = blk.fused_weights()
            ca, ffn0, ffn2 = blk.cross_attn, blk.ffn[0], blk.ffn[2]
            w8 = blk.fp8_weights(fp8) if fp8 is not None else (None,) * 7
            if cfg_prefix is not None and i == 0 and "owner" in cfg_prefix:
                if cfg_prefix.get("taken"):
                    raise RuntimeError("cfg_prefix is shared by exactly two forwards of one step (one computes block 0's self-attention half, "
                                       "one takes it): a third consumer of the same dict")
                spins = 0
                while "x_sa" not in cfg_prefix:      # the other branch is inside block 0's self-attention: let it run
                    spins += 1
                    if spins > 100000:
                        raise RuntimeError("cfg_prefix: the forward that owns block 0's self-attention half never published it (the two "
                                           "forwards of a step must be advanced in turns, or run one after the other)")
                    yield i
                x = cfg_prefix.pop("x_sa")
                cfg_prefix["taken"] = True
                h = lin.affine(x, blk.norm3)
            elif x.shape[0] != nb:      # stacked, i == 0: once on n rows, then norm3 over the copies' rows
                x, _ = yield from self._self_attention_steps(i, blk, mod, x, h, cos, sin, shard, shard_total, lin, att, w8, norm3=False)
                x = x.expand(nb, -1, -1).contiguous()
                h = lin.affine(x, blk.norm3)
            else:
                if cfg_prefix is not None and i == 0:
                    cfg_prefix["owner"] = True
                # --- self attention (reference :139-146)
                x, h = yield from self._self_attention_steps(i, blk, mod, x, h, cos, sin, shard, shard_total, lin, att, w8)
                if cfg_prefix is not None and i == 0:
                    cfg_prefix["x_sa"] = x.clone()
            # --- cross attention (reference :170-185)
            ac = att.cross_attention(i, ca, h, ctx, kv_cache, wkv_c, bkv_c, w8)
            # x += y ; h = modulate(norm2(x))  (reference :226-227); with both norm outputs wanted, norm3's bf16 row is written over
            x, h = lin.residual(x, ac, f"blocks.{i}.cross_attn.o", ca.o.weight, ca.o.bias, w8[4], mod, None, modulate=(mod, 3, 4),
                                out=h.bf16 if lin.want_q8 else None)
            # --- ffn (reference :208-209,228); x += gate_mlp*y is followed by the NEXT block's modulate(norm1(x)), written over norm2's row
            f = lin.plain(h, (f"blocks.{i}.ffn.0",), ffn0.weight, ffn0.bias, w8[5], own=GEMM_BACKEND == "all", gelu=True)
            x, h = lin.residual(x, f, f"blocks.{i}.ffn.2", ffn2.weight, ffn2.bias, w8[6], mod, 5,
                                modulate=(mods[i + 1], 0, 1) if i + 1 < len(blocks) else None, out=h.bf16,
                                tuned=True, store_ok=GEMM_BACKEND != "fused-ffn2", gelu=lin.gelu_in_quant)
        if tea_cache is not None and blocks:
            tea_cache.store(x)
        # --- head (reference :261-268): table (R,2,C) = modulation + t
        hm = hip.ModTable((self.head.modulation.to(t_rows.dtype) + t_rows.unsqueeze(1)).contiguous(), first_rows)
        if nb > 1:      # stacked: the head table per element, one Linear on all rows (through the seam, like the blocks' library GEMMs)
            x = x if x.shape[0] == nb else x.expand(nb, -1, -1).contiguous()
            return gemm_bias(hip.ln_modulate(x, hm, 0, 1, eps, batch=nb), self.head.head.weight, self.head.head.bias)
        h = hip.ln_modulate(x, hm, 0, 1, eps)
        return F.linear(h, self.head.head.weight, self.head.head.bias)

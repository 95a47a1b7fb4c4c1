"""The buffer contract of the C ABI (include/fairygen_hip.h): a kernel touches the bytes its shape arguments name and nothing else.

The hot kernels handle ragged edges by hardware range checks (a buffer descriptor sized from the shape arguments: out-of-range loads
return zeros, out-of-range stores are dropped) instead of clamps, so every num_records, row clamp and tail mask has to be exact.  The
older tests use exactly-sized operands of their own allocation, where a read past the end returns zeros and a write past the end lands
in another tensor nobody looks at.  Here every operand is a view inside a larger allocation (`embed`): inputs sit between bands of NaN
(bf16 / fp32 / fp64 NaN, e4m3 0x7F), outputs between bands of a sentinel bit pattern, at least 16 rows wide and a full tile of the kernel
under test (256 rows of a GEMM / conv output, 64 keys of K / V) where that is cheap.  Criterion of every guarded call:
  (a) every guard byte is unchanged (compared as integers);
  (b) the valid region is torch.equal to the same call on compact, exactly-sized tensors: a leading dimension or a neighbour changes
      addresses, never the order of a sum, so no tolerance applies — and a NaN that leaked in fails it;
  (c) the compact result meets the criterion the project already uses for that kernel against the CPU oracle (imported from
      test_hip_kernels.py: assert_close_bf16 at 1 ulp for the row kernels, err <= 2 * err_ref + floor for the MFMA kernels); where an
      existing test holds (c) for the same shape (the GEMM shapes), (a) and (b) are enough.

Coverage per entry point (guard = sentinel bands round the outputs, poison = NaN bands round the inputs, strided = ld > row with NaN
gap columns, batch = B = 2, alias = out aliasing an input, reject = FG_EINVAL calls in test_argument_checks, see there for which preconditions):
  fg_attn_fwd_bf16                         guard poison strided batch reject   (short-KV, direct, split + combine, both 4-wave forms)
  fg_attn_split_choice / _workspace_bytes  reject (used by the attention cases to tell which results must be bit-equal)
  fg_gemm_epilogue_bf16_s, fg_gemm_fp8_bf16_s   guard poison strided (lda > K, ldc > N, workspace tail) reject; modes 0, 2, 3, 4
  fg_gemm_epilogue_bf16, fg_gemm_fp8_bf16  reject (the same launches; bit-equality to the _s forms: test_gemm_sched_state.py)
  fg_conv3d_cl_bf16, fg_conv_pack_weight_bf16   guard poison reject   (hand-scheduled 256 tile, compiler-scheduled 256 tile, 128 tile)
  fg_ln_modulate_bf16, fg_ln_affine_bf16   guard poison reject
  fg_gate_residual_bf16, fg_residual_ln_bf16    guard poison alias reject
  fg_ln_modulate_fp8_bf16, fg_residual_ln_fp8_bf16, fg_ln_modulate_dual_bf16, fg_ln_affine_dual_bf16   guard poison reject (alias: x_out)
  fg_rmsnorm_rope_bf16                     guard poison strided reject
  fg_fp8_quant_rows_bf16                   guard poison strided reject
  fg_vae_rmsnorm_silu_bf16                 guard poison reject
  fg_act_bf16, fg_cfg_euler_bf16           guard poison alias reject
  fg_softmax_rows_f32_bf16, fg_softmax_bias_bf16   guard poison reject
  fg_vae_unpatchify_bf16 (frame window), fg_dupup3d_add_bf16, fg_avgdown3d_add_bf16, fg_vae_latent_to_cl_bf16,
  fg_vae_latent_from_cl_bf16, fg_vae_patchify_bf16, fg_video_to_uint8   guard poison reject
  fg_rmsnorm_rope_grouped_bf16, fg_copy_groups_bf16   guard poison strided reject   (send buffer with pad rows, gap columns, tail)
  fg_gated_gelu_bf16, fg_vae_tile_accumulate_bf16, fg_vae_tile_finalize_bf16, fg_lora_apply_bf16   reject only
Left out: fg_lora_apply_bf16 (guard / poison / strided: test_hot_lora_kernel.py, test_fp8_hot_lora.py), fg_gemm_sched_reset /
fg_gemm_debug_grid / fg_gemm_sched_bytes (test_gemm_sched_state.py), the tile feathering pair (in place by definition: the canvas IS
the operand; test_tile_blend), fg_gated_gelu_bf16 (elementwise, contiguous, no shape edge beyond n % 8).

Finding of the argument checks: the header promised 16-byte alignment checks for "all functions", while the scalar-access helpers
(fg_cfg_euler_bf16, the softmaxes, the layout boundary kernels, the tile feathering pair, fg_conv_pack_weight_bf16) need element
alignment only and check none, and fg_conv3d_cl_bf16 / the GEMMs need 8 bytes for bias / residual / out resp. bias / gate: the
header now says so (no rejection is promised for those), and test_argument_checks keeps to what it says.

Cost: the CPU reference work of the module (oracle attention and fp32 / bf16 convolutions, the rest is negligible) takes about 2 s on a
16-thread host; the whole module 4 s of pytest time (6 s of wall time) on an MI355X, where test_hip_kernels.py takes 15 s.
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import seeded
from oracle import wan_dit, wan_vae
from oracle import pipeline as opipe
from test_hip_kernels import ATTN_FLOOR, CONV_FLOOR, _cl, _crand, _ncthw, assert_close_bf16, dev, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# one fill for both roles: a NaN in every floating type (bf16 0x7FA5, fp32 / fp64 from repeating the bytes is no NaN, so they are set
# per width), 0x7F = NaN in e4m3fn, and a bit pattern no kernel here produces in an integer output
_FILL = {1: 0x7F, 2: 0x7FA5, 4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}
GEMM_TILE, KV_TILE = 256, 64


class Guards:
    """The embedded operands of one call: embed() as often as needed, the call, then check()."""

    def __init__(self):
        self.items = []

    def embed(self, t, rows_before=16, rows_after=16, cols_left=0, cols_right=0):
        view, big, (r0, r1, c0, c1) = embed(t, rows_before, rows_after, cols_left, cols_right, with_buffer=True)
        bits = big.view(_BITS[big.element_size()])
        self.items.append((bits, bits.clone(), (r0, r1, c0, c1)))
        return view

    def check(self, what):
        """(a): every byte outside the views is what it was."""
        torch.cuda.synchronize()
        for i, (bits, before, (r0, r1, c0, c1)) in enumerate(self.items):
            after = bits.clone()
            after[r0:r1, c0:c1] = before[r0:r1, c0:c1]
            if not torch.equal(after, before):
                bad = (after != before).nonzero()
                raise AssertionError(f"{what}: operand {i}: {bad.shape[0]} guard elements changed; first at (row, col) {bad[0].tolist()}, "
                                     f"last at {bad[-1].tolist()}; the view is rows [{r0}, {r1}) x cols [{c0}, {c1})")


def embed(t, rows_before=16, rows_after=16, cols_left=0, cols_right=0, fill=None, with_buffer=False):
    """A device view with the shape and data of `t` (..., C) inside a larger allocation of rows of cols_left + C + cols_right elements,
    with rows_before / rows_after rows in front and behind; everything outside the view holds `fill` (default: the NaN / sentinel bit
    pattern of the element width).  Without side columns the view is contiguous; with them its rows have the wide leading dimension."""
    c = t.shape[-1]
    t2 = t.contiguous().reshape(-1, c)
    rows, esz = t2.shape[0], t.element_size()
    assert rows_before % 16 == 0 and (cols_left * esz) % 16 == 0, "the view must stay 16-byte aligned"
    ld = cols_left + c + cols_right
    bits = torch.full((rows_before + rows + rows_after, ld), _FILL[esz] if fill is None else fill, dtype=_BITS[esz], device="cuda")
    big = bits.view(t.dtype)
    region = (rows_before, rows_before + rows, cols_left, cols_left + c)
    view = big[region[0]:region[1], region[2]:region[3]]
    bits[region[0]:region[1], region[2]:region[3]].copy_(t2.view(_BITS[esz]))
    view = view.unflatten(0, tuple(t.shape[:-1])) if t.dim() > 1 else view.reshape(t.shape)
    if t.dim() > 1 and ld == c:
        assert view.is_contiguous()
    return (view, big, region) if with_buffer else view


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@gpu
def test_embed_helper_catches_a_stray_write():
    """The helper itself: the view has the data, the alignment and the wide strides; its surroundings are NaN; a write inside the view
    passes check(), one element next to it (a gap column, the row after the last) fails it."""
    for dtype in (torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn, torch.uint8):
        g = Guards()
        t = torch.arange(80).reshape(2, 5, 8).to(dtype)
        v = g.embed(t, 16, 32, 16, 16)
        bits, _, (r0, r1, c0, c1) = g.items[0]
        assert v.shape == t.shape and v.stride() == (5 * 40, 40, 1) and v.data_ptr() % 16 == 0 and (r0, r1, c0, c1) == (16, 26, 16, 24)
        assert torch.equal(v.contiguous().cpu().view(bits.dtype), t.view(bits.dtype))
        if dtype.is_floating_point:
            assert torch.isnan(bits.view(dtype)[0].float()).all() and torch.isnan(bits.view(dtype)[r0, :c0].float()).all(), dtype
        bits[r0:r1, c0:c1] ^= 1
        g.check("writes inside the view")
        for r, c in ((r1 - 1, c1), (r1, c0), (r0, c0 - 1)):
            bits[r, c] ^= 1
            with pytest.raises(AssertionError, match="guard elements changed"):
                g.check("stray write")
            bits[r, c] ^= 1
        g.check("restored")


def _close(got, want, what, mag=None, rate=2e-3):
    """assert_close_bf16 at 1 ulp, with its default bound on the fraction of elements that differ from the oracle at all, or the rate the
    existing test of the same kernel uses."""
    assert_close_bf16(got, want, 1.0, what, mag=mag, max_mismatch=rate)


# ------------------------------------------------------------------------------------------------------------------ 1. attention
def _split_choice(hip, b, nq, nkv, heads, ws=True):
    lib = hip.load()
    R, S = ctypes.c_int(), ctypes.c_int()
    need = lib.fg_attn_workspace_bytes(b, nq, nkv, heads) if ws else 0
    assert lib.fg_attn_split_choice(b, nq, nkv, heads, need, ctypes.byref(R), ctypes.byref(S)) == 0
    return R.value, S.value, need


def _attn(hip, q, k, v, heads, out, scale=None, ws=True):
    """fg_attn_fwd_bf16 on any (B, N, H*128) views with batch stride N * ld; ws False: no workspace, every q-block one direct workgroup.
    The workspace gets a sentinel tail of its own."""
    b, nq, hd = q.shape
    nkv = k.shape[1]

    def ld(t):      # elements between token rows (the stride of a dimension of size 1 says nothing: take the batch stride, or the row)
        lead = t.stride(1) if t.shape[1] > 1 else (t.stride(0) if b > 1 else hd)
        assert t.stride(2) == 1 and (b == 1 or t.stride(0) == t.shape[1] * lead)
        return lead
    assert out.is_contiguous()
    need = _split_choice(hip, b, nq, nkv, heads, ws)[2]
    wsb = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device="cuda") if need else None
    hip._call("fg_attn_fwd_bf16", _p(q), ld(q), _p(k), ld(k), _p(v), ld(v), _p(out), b, nq, nkv, heads, 128,
              128 ** -0.5 if scale is None else float(scale), _p(wsb), need, _stream())
    if need:
        assert (wsb[need:] == 0x5A).all(), "the attention workspace was written past fg_attn_workspace_bytes"
    return out


def _attn_oracle(got, q, k, v, heads, fold, what):
    """(c) per batch element: error to the fp32 oracle <= 2x the error of the oracle's own bf16 op + ATTN_FLOOR (test_hip_kernels._attn_case)."""
    for b in range(q.shape[0]):
        qb, kb, vb = q[b:b + 1], k[b:b + 1], v[b:b + 1]
        plain32 = wan_dit.attention(qb.float(), kb.float(), vb.float(), heads)
        ref32 = plain32 if fold == 1.0 else wan_dit.attention(qb.float() / fold, kb.float(), vb.float(), heads)
        err_ref = (wan_dit.attention(qb, kb, vb, heads).float() - plain32).abs().max().item()
        err = (got[b:b + 1].float().cpu() - ref32).abs().max().item()
        print(f"{what} b={b}: err {err:.5f}, bf16 oracle {err_ref:.5f}")
        assert err <= 2 * err_ref + ATTN_FLOOR, f"{what}, batch element {b}: err {err} vs reference-bf16 err {err_ref}"


def _attn_data(nq, nkv, heads, seed):
    """Two batch elements with clearly different data: element 1 has sharper logits and values around +1."""
    c = heads * 128
    q = torch.cat([seeded((1, nq, c), seed), seeded((1, nq, c), seed + 3, scale=2.0)])
    k = torch.cat([seeded((1, nkv, c), seed + 1), seeded((1, nkv, c), seed + 4)])
    v = torch.cat([seeded((1, nkv, c), seed + 2), (seeded((1, nkv, c), seed + 5).float() * 0.5 + 1.0).to(torch.bfloat16)])
    return q, k, v


ATTN_CASES = [      # name, Nq, Nkv, heads, form, workspace, split expected for B = 2.  Nkv = 28 mod 64 (540, 1500; 1000 is 40 mod 64), Nq not a multiple of 256
    ("short-kv", 300, 540, 2, "plain", True, False),                 # attn_fwd_kernel<> (Nkv <= 1024)
    ("short-kv-split", 300, 1000, 8, "plain", True, True),           # ... its pieces + combine
    ("switch-1024", 300, 1024, 2, "plain", True, None),              # the last Nkv of the short-KV kernel
    ("switch-1025", 300, 1025, 2, "plain", True, None),              # the first of the 4-wave kernel: one key in the 17th tile
    ("w4-direct", 300, 1500, 2, "plain", False, False),              # attn_fwd_w4_kernel<false>, every q-block direct
    ("w4-direct-pow2", 300, 1500, 2, "pow2", False, False),          # attn_fwd_w4_kernel<true>
    ("w4-split", 300, 1500, 2, "plain", True, True),                 # pieces + combine
    ("w4-split-pow2", 300, 1500, 2, "pow2", True, True),
    ("nq-1", 1, 77, 1, "plain", True, False),
    ("nkv-1", 300, 1, 1, "plain", True, False),
    ("nq-1-nkv-1", 1, 1, 1, "plain", True, False),
    ("nq-1-w4", 1, 1500, 1, "pow2", True, None),
]


@gpu
@pytest.mark.parametrize("name,nq,nkv,heads,form,ws,split", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_batch_guard_poison(hip, name, nq, nkv, heads, form, ws, split):
    """fg_attn_fwd_bf16 with B = 2 (b = bh / H in the direct workgroups, the split pieces, the combine kernel and the generated 4-wave
    kernel), and with q, k, v as views whose neighbours are NaN: the rows after Q, K and V (for batch element 0 of a B = 2 call that is
    element 1 — here made of other data — and after element 1 the NaN band) and the other columns of a wide row.  A masked key with
    p = 0 times a NaN in V is NaN, so "masked" and "happens to read zeros" differ here."""
    scale, fold = (None, 1.0) if form == "plain" else hip.pow2_softmax_scale(128)
    q, k, v = _attn_data(nq, nkv, heads, 300)
    choice2 = _split_choice(hip, 2, nq, nkv, heads, ws)[:2]
    if split is not None:
        assert (choice2[0] > 0) == split, f"{name}: fg_attn_split_choice gives (R, S) = {choice2}"
    dq, dk, dv = dev(q), dev(k), dev(v)
    compact = _attn(hip, dq, dk, dv, heads, torch.empty_like(dq), scale, ws)
    assert torch.isfinite(compact.float()).all()
    _attn_oracle(compact, q, k, v, heads, fold, name)
    # B = 2, every operand strided inside NaN, the output inside sentinel rows
    g = Guards()
    got = _attn(hip, g.embed(q, 16, KV_TILE, 64, 8), g.embed(k, 16, KV_TILE, 8, 64), g.embed(v, 16, KV_TILE, 128, 0), heads,
                g.embed(torch.empty_like(q), 16, 256), scale, ws)
    g.check(f"{name}, B = 2")
    assert torch.equal(got, compact), f"{name}: B = 2 on strided views in NaN differs from the compact call"
    # B = 1 on each element: the same bits when the decomposition is the same (or none), else the oracle criterion
    choice1 = _split_choice(hip, 1, nq, nkv, heads, ws)[:2]
    for b in range(2):
        one = _attn(hip, dq[b:b + 1], dk[b:b + 1], dv[b:b + 1], heads, torch.empty_like(dq[b:b + 1]), scale, ws)
        if choice1 == choice2 or (choice1[0] == 0 and choice2[0] == 0):
            assert torch.equal(compact[b:b + 1], one), f"{name}: out[{b}] of the B = 2 call differs from the B = 1 call on element {b}"
        else:
            _attn_oracle(one, q[b:b + 1], k[b:b + 1], v[b:b + 1], heads, fold, f"{name} B=1")
        g = Guards()      # B = 1 with NaN rows right after Q, K and V
        got1 = _attn(hip, g.embed(q[b:b + 1], 16, KV_TILE, 8, 8), g.embed(k[b:b + 1], 16, KV_TILE, 8, 8), g.embed(v[b:b + 1], 16, KV_TILE, 8, 8),
                     heads, g.embed(torch.empty_like(q[b:b + 1]), 16, 256), scale, ws)
        g.check(f"{name}, B = 1, element {b}")
        assert torch.equal(got1, one), f"{name}: B = 1 with NaN after Q / K / V differs from the compact call (element {b})"


@gpu
@pytest.mark.parametrize("form", ["plain", "pow2"])
@pytest.mark.parametrize("ws", [True, False], ids=["split", "direct"])
def test_attention_batch_on_fused_qkv(hip, form, ws):
    """The production layout with B = 2: q, k, v are the column slices of ONE (2, N, 3 * H * 128) buffer; N = 1500 = 23 KV tiles + 28
    keys = 5 q-blocks + 220 rows, on the 4-wave kernel in both forms, direct and split.  Then B = 1 on element 0 of a buffer whose
    element 1 is NaN: what lies past the end of batch 0 is the next batch element."""
    heads, n = 2, 1500
    c = heads * 128
    scale, fold = (None, 1.0) if form == "plain" else hip.pow2_softmax_scale(128)
    q, k, v = _attn_data(n, n, heads, 320)
    qkv = torch.cat([q, k, v], dim=-1)
    assert (_split_choice(hip, 2, n, n, heads, ws)[0] > 0) == ws
    compact = _attn(hip, dev(q), dev(k), dev(v), heads, torch.empty((2, n, c), dtype=torch.bfloat16, device="cuda"), scale, ws)
    _attn_oracle(compact, q, k, v, heads, fold, f"fused {form}")
    g = Guards()
    d = g.embed(qkv, 16, KV_TILE)
    got = _attn(hip, d[..., :c], d[..., c:2 * c], d[..., 2 * c:], heads, g.embed(torch.empty_like(q), 16, 256), scale, ws)
    g.check("fused qkv, B = 2")
    assert torch.equal(got, compact)
    one = _attn(hip, dev(q[:1]), dev(k[:1]), dev(v[:1]), heads, torch.empty((1, n, c), dtype=torch.bfloat16, device="cuda"), scale, ws)
    d[1] = float("nan")
    g2 = Guards()
    got = _attn(hip, d[:1, :, :c], d[:1, :, c:2 * c], d[:1, :, 2 * c:], heads, g2.embed(torch.empty_like(q[:1]), 16, 256), scale, ws)
    g2.check("fused qkv, B = 1")
    assert torch.equal(got, one), "B = 1 on element 0 of a fused buffer whose element 1 is NaN"


# ------------------------------------------------------------------------------------------------------------------ 2. GEMM
GEMM_BF16 = [(700, 256, 768), (4200, 512, 4096), (10500, 128, 2048), (3410, 3072, 3072),                              # test_gemm_epilogue
             (4200, 6144, 4096), (600, 14336, 3072), (8300, 14336, 512), (66200, 6144, 256), (3410, 14336, 3072)]     # test_gemm_epilogue_ksplit
GEMM_FP8 = [(700, 3072, 768), (4200, 1024, 4096), (600, 14336, 3072)]                                                 # test_gemm_fp8


@gpu
@pytest.mark.parametrize("fp8,M,K,N", [(False,) + s for s in GEMM_BF16] + [(True,) + s for s in GEMM_FP8])
def test_gemm_guard_poison_strided(hip, fp8, M, K, N):
    """The persistent GEMM in both operand types, modes 0, 2, 3, 4, on the ragged shapes of test_gemm_epilogue / _ksplit / test_gemm_fp8
    (which hold the oracle criterion for them).  Rows past M are "clamped to the last row: those rows are never stored" and idle lanes
    are sent out of range (csrc/gen_gemm_p.py): (1) through the wrappers, a / scale_a / w between NaN rows and `out` a row slice of a
    sentinel buffer with a whole tile behind it; (2) through the raw _s entry points, lda > K with NaN gap columns, ldc > N with
    sentinel gap columns, and a workspace longer than fg_gemm_workspace_bytes whose tail must survive (k-split shapes write partial
    sums there).  Every result equals the compact wrapper call bit for bit."""
    lib = hip.load()
    x, w, b = _crand((M, K), 401, 0.5), _crand((N, K), 402, 0.05), _crand((N,), 403, 0.2)
    res, table = _crand((M, N), 404), _crand((2, 6, N), 405)
    first = M - 200
    if fp8:
        x[5] *= 300.0
        x, sc = hip.fp8_quant_rows(x)
        w = w.to(torch.float8_e4m3fn)
        assert sc[5].item() > 1.0

    def wrapper(a, s, wt, bias, out, mode, mod):
        kw = dict(out=out, residual=mode in (2, 3), mod=mod if mode == 2 else None, gate_idx=5 if mode == 2 else None,
                  act="gelu_tanh" if mode == 4 else None)
        return hip.gemm_fp8(a, s, wt, bias, **kw) if fp8 else hip.gemm_epilogue(a, wt, bias, **kw)

    def start(mode):      # what `out` holds before the call: the residual stream, or nothing
        return res.clone() if mode in (2, 3) else torch.empty_like(res)

    mod = hip.ModTable(table, first)
    compact = {mode: wrapper(x, sc if fp8 else None, w, b, start(mode), mode, mod) for mode in (0, 2, 3, 4)}
    assert torch.isfinite(compact[0].float()).all() and not torch.equal(compact[2], compact[3])
    sched, _ = hip.gemm_state()
    need = lib.fg_gemm_workspace_bytes(M, N, K)
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    gap = 16      # elements of both types: 16 or 32 bytes
    for mode in (0, 2, 3, 4):
        g = Guards()
        got = wrapper(g.embed(x, 16, GEMM_TILE), g.embed(sc, 16, GEMM_TILE) if fp8 else None, g.embed(w, 16, GEMM_TILE), g.embed(b),
                      g.embed(start(mode), 16, GEMM_TILE), mode, hip.ModTable(g.embed(table), first))
        g.check(f"gemm {M}x{K}x{N} mode {mode} (wrapper)")
        assert torch.equal(got, compact[mode]), f"mode {mode}: operands between NaN rows, out inside a sentinel buffer"
        g = Guards()
        a_s, c_s = g.embed(x, 16, GEMM_TILE, gap, gap), g.embed(start(mode), 16, GEMM_TILE, 8, 24)
        sc_s = g.embed(sc, 16, GEMM_TILE) if fp8 else None
        tail = (None if mode != 2 else mod.vec(5), mod.mod_rows if mode == 2 else 1, mod.ld if mode == 2 else N, first if mode == 2 else 0,
                _p(ws), _p(sched), 0, _stream())
        if fp8:
            hip._call("fg_gemm_fp8_bf16_s", _p(a_s), a_s.stride(0), _p(sc_s), _p(w), _p(b), _p(c_s), c_s.stride(0), M, N, K, mode, *tail)
        else:
            hip._call("fg_gemm_epilogue_bf16_s", _p(a_s), a_s.stride(0), _p(w), _p(b), _p(c_s), c_s.stride(0), M, N, K, mode, *tail)
        g.check(f"gemm {M}x{K}x{N} mode {mode} (lda = K + {2 * gap}, ldc = N + 32)")
        assert torch.equal(c_s, compact[mode]), f"mode {mode}: lda > K, ldc > N"
        assert (ws[need:] == 0x5A).all(), "the workspace was written past fg_gemm_workspace_bytes"


# ------------------------------------------------------------------------------------------------------------------ 3. conv3d
def _conv_ref(x, w, b, prev, res, kt, ks, resample, interleave, dtype):
    """fp32 / bf16 F.conv3d reference of fg_conv3d_cl_bf16's modes (wan_vae.causal_conv3d for the causal form); NCTHW."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    if resample == 0:
        y = wan_vae.causal_conv3d({"c.weight": w, "c.bias": b}, "c", x, None if prev is None else prev.to(dtype))
    else:
        frames = x[0].permute(1, 0, 2, 3)
        if resample == 1:
            frames = F.interpolate(frames.float(), scale_factor=(2.0, 2.0), mode="nearest-exact").to(dtype)
            y = F.conv2d(frames, w[:, :, 0], b, padding=ks // 2)
        else:
            y = F.conv2d(F.pad(frames, (0, 1, 0, 1)), w[:, :, 0], b, stride=2)
        y = y.permute(1, 0, 2, 3).unsqueeze(0)
    if interleave:
        _, c2, t, h, w_ = y.shape
        y = y.reshape(1, 2, c2 // 2, t, h, w_)
        y = torch.stack((y[:, 0], y[:, 1]), 3).reshape(1, c2 // 2, 2 * t, h, w_)
    return y if res is None else y + res.to(dtype)


CONV_CASES = [      # name, kernel, Cin, Cout, kt, ks, T, H, W (output), resample, interleave, residual
    # hand-scheduled 256 tile (conv3d_cl_w4_kernel): T*H*W = 16 401 = 64 * 256 + 17
    ("w4-3x3x3-res", "w4", 64, 256, 3, 3, 3, 71, 77, 0, False, True),
    ("w4-1x1x1", "w4", 64, 256, 1, 1, 3, 71, 77, 0, False, False),
    ("w4-stride2", "w4", 64, 256, 1, 3, 3, 71, 77, 2, False, False),
    ("w4-upsample-res", "w4", 64, 256, 1, 3, 1, 130, 130, 1, False, True),        # 16 900 = 66 * 256 + 4
    # compiler-scheduled 256 tile (conv3d_cl_256p_kernel): Cin % 64 != 0, or interleave with Cout / 2 = 128
    ("256p-cin96", "256p", 96, 256, 1, 3, 3, 71, 77, 0, False, True),
    ("256p-interleave", "256p", 64, 256, 3, 1, 3, 71, 77, 0, True, False),
    # 128 tile (conv3d_cl_kernel): Cout = 12 -> cout_pad = 128, columns past Cout must not be written; ragged last pixel tile
    ("128-cout12-res", "128", 64, 12, 3, 3, 2, 9, 7, 0, False, True),
    ("128-cin48-upsample", "128", 48, 64, 1, 3, 2, 10, 12, 1, False, False),
    ("128-stride2-res", "128", 64, 64, 1, 3, 2, 5, 7, 2, False, True),
    ("128-interleave-1x1", "128", 64, 128, 3, 1, 2, 5, 7, 0, True, True),
    ("128-1x1x1", "128", 96, 48, 1, 1, 3, 5, 7, 0, False, False),
]


@gpu
@pytest.mark.parametrize("name,kernel,cin,cout,kt,ks,T,H,W,resample,interleave,residual", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3d_guard_poison(hip, name, kernel, cin, cout, kt, ks, T, H, W, resample, interleave, residual):
    """fg_conv3d_cl_bf16 on each of its three kernels with a ragged last pixel tile: x (with its history frames) and the packed weights
    between NaN bands — spatial padding, pixels past M and channels past Cin are out-of-range offsets (kOOB) that must read zeros, never
    a neighbour — and out / residual between sentinel bands of a whole tile (conv3d_cl_w4_kernel hands its generated body the remaining
    output bytes).  Criterion (c) as test_conv3d_cl: error to the fp32 conv <= 2x the bf16 conv's + CONV_FLOOR."""
    lib = hip.load()
    cout2 = cout // 2 if interleave else cout
    tile = lib.fg_conv_tile_choice(T, H, W, cout)
    takes_w4 = cin % 64 == 0 and cout2 % 256 == 0
    assert (tile, takes_w4) == {"w4": (256, True), "256p": (256, False), "128": (128, takes_w4)}[kernel], (tile, takes_w4)
    assert (T * H * W) % tile != 0, "the last pixel tile must be ragged"
    hin, win = (H // 2, W // 2) if resample == 1 else ((2 * H, 2 * W) if resample == 2 else (H, W))
    x = seeded((1, cin, T, hin, win), 500)
    prev = seeded((1, cin, 2, hin, win), 501) if kt == 3 else None
    w = seeded((cout, cin, kt, ks, ks), 502, scale=(cin * kt * ks * ks) ** -0.5)
    b = seeded((cout,), 503, scale=0.1)
    oshape = (1, cout2, 2 * T if interleave else T, H, W)
    res = seeded(oshape, 504) if residual else None
    ref32 = _conv_ref(x, w, b, prev, res, kt, ks, resample, interleave, torch.float32)
    ref16 = _conv_ref(x, w, b, prev, res, kt, ks, resample, interleave, torch.bfloat16).float()
    xin = _cl(x if prev is None else torch.cat([prev, x], dim=2))
    packed = hip.conv_pack_weight(dev(w))
    kw = dict(upsample2x=resample == 1, downsample2x=resample == 2, time_interleave=interleave)
    compact = hip.conv3d_cl(dev(xin), packed, dev(b), cout, kt, ks, residual=None if res is None else dev(_cl(res)), **kw)
    err_ref, err = (ref16 - ref32).abs().max().item(), (_ncthw(compact.cpu()).float() - ref32).abs().max().item()
    print(f"{name}: err {err:.5f}, bf16 conv {err_ref:.5f}")
    assert err <= 2 * err_ref + CONV_FLOOR, f"{name}: conv err {err} vs reference-bf16 err {err_ref}"
    g = Guards()
    out = g.embed(torch.empty(compact.shape, dtype=torch.bfloat16), 16, 256)
    got = hip.conv3d_cl(g.embed(xin, 16, 256), g.embed(packed.view(-1, 64), 16, 256).view(-1), g.embed(b), cout, kt, ks,
                        residual=None if res is None else g.embed(_cl(res), 16, 256), out=out, **kw)
    g.check(name)
    assert torch.equal(got, compact), f"{name}: operands between NaN bands, out / residual between sentinel bands"


# ------------------------------------------------------------------------------------------------------------------ 4. row kernels
ROW_C = [8, 520, 3080, 4096]      # one vector; a partial last lane group (65 and 385 vectors); the documented maximum
ROW_N = [1, 5, 13]                # four rows per workgroup: 1, 4 + 1, 12 + 1


def _mod_rows(table, rows, first, j):
    idx = (torch.arange(rows) >= first).long()
    return table[idx, j].unsqueeze(0)


@gpu
@pytest.mark.parametrize("rows", ROW_N)
@pytest.mark.parametrize("C", ROW_C)
def test_norm_rows_guard_poison_alias(hip, C, rows):
    """fg_ln_modulate*, fg_ln_affine*, fg_gate_residual, fg_residual_ln*: inputs between NaN rows, every output between sentinel rows;
    x_out / out aliasing x gives the bits of the non-aliased call ("out may alias x": each lane reads its vectors before it writes them)."""
    eps, first = 1e-6, rows // 3
    x, y = seeded((1, rows, C), 601), seeded((1, rows, C), 602)
    table = seeded((2, 6, C), 603, scale=0.5)
    wt, bs = (1 + 0.1 * seeded((C,), 604)).to(torch.bfloat16), (0.1 * seeded((C,), 605)).to(torch.bfloat16)
    dx, dy, dw, db = dev(x), dev(y), dev(wt), dev(bs)
    mod = hip.ModTable(dev(table), first)
    shift, scale, gate = (_mod_rows(table, rows, first, j) for j in (0, 1, 2))

    def fresh():      # a new set of guarded operands
        g = Guards()
        return g, g.embed(x), g.embed(y), hip.ModTable(g.embed(table), first), g.embed(wt), g.embed(bs)

    def sent(g, dtype=torch.bfloat16, cols=C):
        return g.embed(torch.empty((1, rows, cols)).to(dtype) if cols == C else torch.empty((rows, cols), dtype=dtype))

    # ln_modulate / ln_affine
    c_mod, c_aff = hip.ln_modulate(dx, mod, 0, 1, eps), hip.ln_affine(dx, dw, db, eps)
    _close(c_mod, wan_dit.layer_norm(x, eps) * (1 + scale) + shift, "ln_modulate", mag=shift)
    _close(c_aff, wan_dit.layer_norm(x, eps, wt, bs), "ln_affine", mag=bs)
    g, gx, gy, gmod, gw, gb = fresh()
    assert torch.equal(hip.ln_modulate(gx, gmod, 0, 1, eps, out=sent(g)), c_mod)
    assert torch.equal(hip.ln_affine(gx, gw, gb, eps, out=sent(g)), c_aff)
    g.check("ln_modulate / ln_affine")
    # gate_residual, plain and aliased
    c_gate, c_add = hip.gate_residual(dx, dy, mod, 2), hip.gate_residual(dx, dy)
    assert torch.equal(c_gate.cpu(), x + gate * y) and torch.equal(c_add.cpu(), x + y)
    g, gx, gy, gmod, gw, gb = fresh()
    assert torch.equal(hip.gate_residual(gx, gy, gmod, 2, out=sent(g)), c_gate)
    assert torch.equal(hip.gate_residual(gx, gy, out=sent(g)), c_add)
    assert torch.equal(hip.gate_residual(gx, gy, gmod, 2, out=gx), c_gate), "gate_residual(out=x)"
    g.check("gate_residual")
    # residual + norm, both modes, plain and aliased
    c_xo, c_no = hip.residual_ln_modulate(dx, dy, mod, 2, 0, 1, eps)
    assert torch.equal(c_xo, c_gate)
    _close(c_no, wan_dit.layer_norm(c_gate.cpu(), eps) * (1 + scale) + shift, "res+modulate", mag=shift)
    a_xo, a_no = hip.residual_ln_affine(dx, dy, dw, db, eps, mod, 2)
    assert torch.equal(a_xo, c_gate)
    _close(a_no, wan_dit.layer_norm(c_gate.cpu(), eps, wt, bs), "res+affine", mag=bs)
    g, gx, gy, gmod, gw, gb = fresh()
    xo, no = hip.residual_ln_modulate(gx, gy, gmod, 2, 0, 1, eps, x_out=sent(g), norm_out=sent(g))
    assert torch.equal(xo, c_xo) and torch.equal(no, c_no)
    xo, no = hip.residual_ln_affine(gx, gy, gw, gb, eps, gmod, 2, x_out=sent(g), norm_out=sent(g))
    assert torch.equal(xo, a_xo) and torch.equal(no, a_no)
    g.check("residual_ln")
    for affine in (False, True):
        g, gx, gy, gmod, gw, gb = fresh()
        xo, no = (hip.residual_ln_affine(gx, gy, gw, gb, eps, gmod, 2, x_out=gx, norm_out=sent(g)) if affine else
                  hip.residual_ln_modulate(gx, gy, gmod, 2, 0, 1, eps, x_out=gx, norm_out=sent(g)))
        g.check("residual_ln(x_out=x)")
        assert torch.equal(xo, c_gate) and torch.equal(no, a_no if affine else c_no), f"residual_ln (affine {affine}) with x_out = x"
    # the fp8 / dual forms, raw (the wrappers allocate their outputs): bytes and scales of fg_fp8_quant_rows_bf16 on the bf16 rows
    q_mod, s_mod = hip.fp8_quant_rows(c_mod)
    q_aff, s_aff = hip.fp8_quant_rows(c_aff)
    q_rm, s_rm = hip.fp8_quant_rows(c_no)
    q_ra, s_ra = hip.fp8_quant_rows(a_no)
    f8, f32, mx, st = torch.float8_e4m3fn, torch.float32, hip.FP8_E4M3FN_MAX, _stream()

    def same8(q, s, wq, wsc, what):
        assert torch.equal(q.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(s, wsc), what

    g, gx, gy, gmod, gw, gb = fresh()
    margs = (gmod.mod_rows, first, gmod.ld)
    q, s = sent(g, f8), sent(g, f32, 1)
    hip._call("fg_ln_modulate_fp8_bf16", _p(gx), gmod.vec(0), gmod.vec(1), _p(q), _p(s), rows, C, eps, *margs, mx, st)
    same8(q[0], s, q_mod, s_mod, "ln_modulate_fp8")
    o, q, s = sent(g), sent(g, f8), sent(g, f32, 1)
    hip._call("fg_ln_modulate_dual_bf16", _p(gx), gmod.vec(0), gmod.vec(1), _p(o), _p(q), _p(s), rows, C, eps, *margs, mx, st)
    same8(q[0], s, q_mod, s_mod, "ln_modulate_dual")
    assert torch.equal(o, c_mod)
    o, q, s = sent(g), sent(g, f8), sent(g, f32, 1)
    hip._call("fg_ln_affine_dual_bf16", _p(gx), _p(gw), _p(gb), _p(o), _p(q), _p(s), rows, C, eps, mx, st)
    same8(q[0], s, q_aff, s_aff, "ln_affine_dual")
    assert torch.equal(o, c_aff)
    xo, q, s = sent(g), sent(g, f8), sent(g, f32, 1)
    hip._call("fg_residual_ln_fp8_bf16", _p(gx), _p(gy), gmod.vec(2), _p(xo), gmod.vec(0), gmod.vec(1), _p(q), _p(s), 0, rows, C, eps, *margs, mx, st)
    same8(q[0], s, q_rm, s_rm, "residual_ln_fp8 (modulate)")
    assert torch.equal(xo, c_gate)
    q, s = sent(g, f8), sent(g, f32, 1)      # affine, with x_out aliasing x
    hip._call("fg_residual_ln_fp8_bf16", _p(gx), _p(gy), gmod.vec(2), _p(gx), _p(gw), _p(gb), _p(q), _p(s), 1, rows, C, eps, *margs, mx, st)
    same8(q[0], s, q_ra, s_ra, "residual_ln_fp8 (affine, x_out = x)")
    assert torch.equal(gx, c_gate)
    g.check("fp8 / dual norms")


@gpu
@pytest.mark.parametrize("rows", ROW_N)
@pytest.mark.parametrize("C,heads", [(8, 1), (520, 5), (3080, 7), (4096, 32)])
def test_rmsnorm_rope_and_fp8_quant_strided(hip, C, heads, rows):
    """fg_rmsnorm_rope_bf16 (fp64 tables, the fp32 table, no table) and fg_fp8_quant_rows_bf16 (act 0 and 1 with act_out) on a column
    slice whose gap columns and neighbour rows are NaN (ldx > C), tables between NaN rows, outputs between sentinel rows."""
    eps = 1e-6
    x = seeded((1, rows, C), 611, scale=2.0)
    wt = (1 + 0.1 * seeded((C,), 612)).to(torch.bfloat16)
    table = wan_dit.rope_table_3d(C // heads, 1, 1, rows)
    cos, sin = table.real.reshape(rows, -1).contiguous(), table.imag.reshape(rows, -1).contiguous()
    cs = torch.stack([cos, sin], dim=-1).to(torch.float32).contiguous()
    want = wan_dit.rope_apply(wan_dit.rms_norm(x, wt, eps), table, heads)
    dx, dw = dev(x), dev(wt)
    c64 = hip.rmsnorm_rope(dx, dw, heads, eps, dev(cos), dev(sin))
    c32 = hip.rmsnorm_rope(dx, dw, heads, eps, dev(cs))
    c00 = hip.rmsnorm_rope(dx, dw, heads, eps)
    _close(c64, want, "rmsnorm+rope")
    _close(c32, want, "rmsnorm+rope (fp32 table)")
    _close(c00, wan_dit.rms_norm(x, wt, eps), "rmsnorm")
    g = Guards()
    gx, gw = g.embed(x, 16, 16, 24, 8), g.embed(wt)
    out = lambda: g.embed(torch.empty((1, rows, C), dtype=torch.bfloat16))      # noqa: E731
    assert torch.equal(hip.rmsnorm_rope(gx, gw, heads, eps, g.embed(cos), g.embed(sin), out=out()), c64)
    assert torch.equal(hip.rmsnorm_rope(gx, gw, heads, eps, g.embed(cs), out=out()), c32)
    assert torch.equal(hip.rmsnorm_rope(gx, gw, heads, eps, out=out()), c00)
    g.check("rmsnorm_rope")
    # fp8_quant_rows: the reference's fp8_linear activation path, bit for bit without an activation (test_fp8_quant_rows)
    x2 = x[0].clone()
    x2[0] *= 400.0
    q0, s0 = hip.fp8_quant_rows(dev(x2))
    want_scale = torch.clamp(x2.abs().amax(-1, keepdim=True) / 448.0, min=1.0).float()
    assert torch.equal(s0.cpu(), want_scale) and want_scale[0].item() > 1.0
    assert torch.equal(q0.cpu().view(torch.uint8), (x2 / (want_scale + 1e-8)).to(torch.float8_e4m3fn).view(torch.uint8))
    q1, s1 = hip.fp8_quant_rows(dev(x2), "gelu_tanh")
    _close(hip.activation(dev(x2).clone(), "gelu_tanh"), F.gelu(x2, approximate="tanh"), "gelu before the quantisation", rate=0.05)      # test_activations_and_cfg_euler
    qg, sg = hip.fp8_quant_rows(hip.activation(dev(x2).clone(), "gelu_tanh"))
    assert torch.equal(q1.view(torch.uint8), qg.view(torch.uint8)) and torch.equal(s1, sg), "act 1 == quantised fg_act_bf16"
    g = Guards()
    gx = g.embed(x2, 16, 16, 24, 8)
    for act, wq, wsc in ((0, q0, s0), (1, q1, s1)):
        q, s = g.embed(torch.empty((rows, C)).to(torch.float8_e4m3fn)), g.embed(torch.empty((rows, 1), dtype=torch.float32))
        ao = g.embed(torch.empty((rows, C), dtype=torch.bfloat16)) if act else None
        hip._call("fg_fp8_quant_rows_bf16", _p(gx), gx.stride(0), _p(q), _p(s), _p(ao), rows, C, act, hip.FP8_E4M3FN_MAX, _stream())
        assert torch.equal(q.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(s, wsc), f"fp8_quant_rows act {act}"
        if act:
            assert torch.equal(ao, hip.activation(dev(x2).clone(), "gelu_tanh")), "act_out"
    g.check("fp8_quant_rows")


@gpu
@pytest.mark.parametrize("rows", ROW_N)
@pytest.mark.parametrize("C,heads,P", [(8, 1, 1), (520, 5, 5), (3080, 7, 7), (4096, 32, 4)])
def test_ulysses_packing_guard_poison_strided(hip, C, heads, P, rows):
    """fg_rmsnorm_rope_grouped_bf16 and fg_copy_groups_bf16 as the Ulysses exchange uses them — the only row kernel with its own output
    addressing (group_cols, out_group_stride, out_ld).  q, k, v are column slices of one fused (rows, 3C) buffer with NaN gap columns
    and NaN rows round it, the tables sit between NaN rows; the send buffer has P head-group blocks of rows + 3 token rows (pad rows
    behind every block), rows of 3 * g + 8 elements (q | k | v | gap) and bands in front and behind, all sentinel.  After the three
    calls the WHOLE buffer, compared as integers, is the sentinel image with the plain kernels' results laid into the q, k and v cells:
    nothing between the groups, in the gap columns, in the pad rows or behind the last block is written.  Then the receive side:
    head-group blocks back to token rows of a wider, sentinel-filled destination."""
    eps, g, size = 1e-6, C // P, rows + 3
    ld = 3 * g + 8
    qkv = seeded((1, rows, 3 * C), 641)
    wt = (1 + 0.1 * seeded((C,), 642)).to(torch.bfloat16)
    table = wan_dit.rope_table_3d(C // heads, 1, 1, rows)
    cos, sin = table.real.reshape(rows, -1).contiguous(), table.imag.reshape(rows, -1).contiguous()
    cs = torch.stack([cos, sin], dim=-1).to(torch.float32).contiguous()
    d, dw = dev(qkv), dev(wt)
    plain = {"q64": hip.rmsnorm_rope(d[..., :C].contiguous(), dw, heads, eps, dev(cos), dev(sin))[0],
             "q32": hip.rmsnorm_rope(d[..., :C].contiguous(), dw, heads, eps, dev(cs))[0],
             "k": hip.rmsnorm_rope(d[..., C:2 * C].contiguous(), dw, heads, eps)[0], "v": d[0, :, 2 * C:]}
    gd = Guards()
    gx, gw = gd.embed(qkv, 16, 16, 8, 8), gd.embed(wt)
    ldx = 3 * C + 16
    src_flat = gd.items[0][0].view(torch.bfloat16).view(-1)[16 * ldx + 8:]          # 1-D view from the first element of the fused rows
    i16 = lambda t: t.contiguous().view(torch.int16)      # noqa: E731
    for form in ("q64", "q32"):
        bits = torch.full((16 + P * size + 16, ld), _FILL[2], dtype=torch.int16, device="cuda")
        flat = bits.view(torch.bfloat16).view(-1)[16 * ld:]
        layout = (g, size * ld, ld)
        tabs = (gd.embed(cos), gd.embed(sin)) if form == "q64" else (gd.embed(cs),)
        hip.rmsnorm_rope(gx[..., :C], gw, heads, eps, *tabs, grouped=(flat, *layout))
        hip.rmsnorm_rope(gx[..., C:2 * C], gw, heads, eps, grouped=(flat[g:], *layout))
        hip.copy_groups(src_flat[2 * C:], g, ldx, flat[2 * g:], size * ld, ld, P, rows, g)
        want = torch.full_like(bits, _FILL[2])
        cells = want[16:16 + P * size].view(P, size, ld)
        for j, name in enumerate((form, "k", "v")):
            cells[:, :rows, j * g:(j + 1) * g] = i16(plain[name].unflatten(-1, (P, g)).transpose(0, 1))
        torch.cuda.synchronize()
        bad = (bits != want).nonzero()
        assert bad.numel() == 0, f"{form}: {bad.shape[0]} elements of the send buffer differ from the sentinel image; first at (row, col) {bad[0].tolist()}"
        # receive side: block p, token r -> row r, columns [p * g, (p + 1) * g) of a destination with gap columns
        ga = Guards()
        a = ga.embed(torch.empty((rows, C), dtype=torch.bfloat16), 16, 16, 8, 8)
        a_flat = ga.items[0][0].view(torch.bfloat16).view(-1)[16 * (C + 16) + 8:]
        hip.copy_groups(flat[2 * g:], size * ld, ld, a_flat, g, C + 16, P, rows, g)
        ga.check("copy_groups back to token rows")
        assert torch.equal(a, plain["v"])
    gd.check("ulysses packing inputs")


@gpu
@pytest.mark.parametrize("pixels", [1, 5, 17])               # 8 pixels per workgroup below 257 channels, 4 above
@pytest.mark.parametrize("C", [8, 256, 264, 520, 2048])      # one vector; the last width of the 32-lane form and the first of the 64-lane form; the maximum
def test_vae_rmsnorm_guard_poison(hip, C, pixels):
    x = seeded((1, C, 1, 1, pixels), 621, scale=2.0)
    gm = (1 + 0.1 * seeded((C, 1, 1, 1), 622)).to(torch.bfloat16)
    want = F.silu(wan_vae.rms_norm_c({"n.gamma": gm}, "n", x))
    compact = hip.vae_rmsnorm_silu(dev(_cl(x)), dev(gm.view(-1)), True)
    _close(_ncthw(compact.cpu()), want, "vae rmsnorm")
    g = Guards()
    got = hip.vae_rmsnorm_silu(g.embed(_cl(x)), g.embed(gm.view(-1)), True, out=g.embed(torch.empty_like(_cl(x))))
    g.check("vae_rmsnorm_silu")
    assert torch.equal(got, compact)


@gpu
def test_elementwise_alias(hip):
    """fg_act_bf16 in place and fg_cfg_euler_bf16(out = latents) give the bits of the call into a separate buffer; guards round all."""
    x = seeded((5, 1000, 8), 631, scale=3.0)
    for kind, ref in (("silu", F.silu), ("gelu_tanh", lambda t: F.gelu(t, approximate="tanh"))):
        g = Guards()
        gx = g.embed(x)
        sep = hip.activation(gx, kind, out=g.embed(torch.empty_like(x)))
        _close(sep, ref(x), kind, rate=0.05)
        assert torch.equal(hip.activation(gx, kind), sep) and gx.data_ptr() != sep.data_ptr(), f"{kind} in place"
        g.check(kind)
    lat, p, n_ = seeded((1, 48, 3, 7, 9), 632), seeded((1, 48, 3, 7, 9), 633), seeded((1, 48, 3, 7, 9), 634)      # 9 072 elements: no whole number of workgroups
    sig, _ = opipe.wan_sigmas(4)
    for nega in (n_, None):
        g = Guards()
        gl, gp, gn = g.embed(lat), g.embed(p), None if nega is None else g.embed(nega)
        cfg = 5.0 if nega is not None else 1.0
        sep = hip.cfg_euler(gl, gp, gn, cfg, float(sig[2] - sig[1]), out=g.embed(torch.empty_like(lat)))
        assert torch.equal(sep.cpu(), opipe.euler_step(p if nega is None else n_ + 5.0 * (p - n_), 1, lat, sig))
        assert torch.equal(hip.cfg_euler(gl, gp, gn, cfg, float(sig[2] - sig[1]), out=gl), sep), "cfg_euler(out=latents)"
        g.check("cfg_euler")


# ------------------------------------------------------------------------------------------------------------------ 5. VAE / text helpers
@gpu
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1560, 3000])      # one workgroup of 256 threads per row
def test_softmax_guard_poison(hip, cols):
    rows = 5
    s = seeded((rows, cols), 701, torch.float32, scale=20.0)
    g = Guards()
    probs = g.embed(torch.empty((rows, cols), dtype=torch.bfloat16))
    hip._call("fg_softmax_rows_f32_bf16", _p(g.embed(s)), _p(probs), rows, cols, 0.25, _stream())
    g.check("softmax_rows")
    assert torch.equal(probs, hip.softmax_rows(dev(s), 0.25))
    assert (probs.float().cpu() - torch.softmax(s * 0.25, dim=-1)).abs().max().item() < 4e-3
    sb, bias = seeded((rows, cols), 702, scale=4.0), seeded((rows, cols), 703)
    for keep in (cols, max(1, 3 * cols // 4)):
        mask = torch.zeros(cols, dtype=torch.int32)
        mask[:keep] = 1
        bm = bias.clone().masked_fill_(mask.view(1, -1) == 0, torch.finfo(torch.bfloat16).min)
        want = torch.softmax((sb + bm).float(), dim=-1).to(torch.bfloat16)
        g = Guards()
        probs = g.embed(torch.empty((rows, cols), dtype=torch.bfloat16))
        hip._call("fg_softmax_bias_bf16", _p(g.embed(sb)), _p(g.embed(bias)), _p(g.embed(mask)) if keep < cols else None, _p(probs), rows, cols, _stream())
        g.check("softmax_bias")
        assert torch.equal(probs, hip.softmax_bias(dev(sb), dev(bias), dev(mask) if keep < cols else None))
        _close(probs, want, "softmax_bias", rate=0.02)
        assert not probs[:, keep:].any()


@gpu
def test_vae_boundary_kernels_guard_poison(hip):
    """The layout boundary kernels and the two resampling shortcuts: inputs between NaN bands, outputs between sentinel bands;
    fg_vae_unpatchify_bf16 into a frame window [t0, t0 + T) of a longer video: the frames outside it are untouched."""
    st = _stream()
    mean, inv_std = torch.tensor(wan_vae.VAE38_MEAN).to(torch.bfloat16), (1.0 / torch.tensor(wan_vae.VAE38_STD)).to(torch.bfloat16)
    # unpatchify
    x = seeded((1, 12, 3, 5, 7), 711, scale=0.8)
    g = Guards()
    video = g.embed(torch.zeros((3, 6, 10, 14), dtype=torch.bfloat16))
    sentinel = torch.tensor(0x7FA5, dtype=torch.int16)
    video.view(torch.int16).fill_(sentinel)
    hip.vae_unpatchify(g.embed(_cl(x)), video, 2, True)
    g.check("vae_unpatchify")
    assert torch.equal(video[:, 2:5].cpu(), wan_vae.unpatchify2(x)[0].clamp(-1, 1))
    assert (video[:, :2].view(torch.int16) == sentinel).all() and (video[:, 5:].view(torch.int16) == sentinel).all(), "frames outside [t0, t0 + T)"
    # latent_to_cl / latent_from_cl
    z = seeded((1, 48, 2, 3, 5), 712)
    g = Guards()
    out = g.embed(torch.empty((2, 3, 5, 48), dtype=torch.bfloat16))
    hip._call("fg_vae_latent_to_cl_bf16", _p(g.embed(z[0])), _p(g.embed(mean)), _p(g.embed(inv_std)), _p(out), 48, 2, 3, 5, st)
    g.check("latent_to_cl")
    assert torch.equal(_ncthw(out.cpu()), z / inv_std.view(1, 48, 1, 1, 1) + mean.view(1, 48, 1, 1, 1))
    h96 = seeded((1, 96, 1, 3, 5), 713)
    g = Guards()
    out = g.embed(torch.empty((48, 1, 3, 5), dtype=torch.bfloat16))
    hip._call("fg_vae_latent_from_cl_bf16", _p(g.embed(_cl(h96))), _p(g.embed(mean)), _p(g.embed(inv_std)), _p(out), 48, 96, 1, 3, 5, st)
    g.check("latent_from_cl")
    assert torch.equal(out.cpu().unsqueeze(0), (h96[:, :48] - mean.view(1, 48, 1, 1, 1)) * inv_std.view(1, 48, 1, 1, 1))
    # patchify / video_to_uint8
    vid = seeded((1, 3, 2, 6, 10), 714, scale=0.5)
    g = Guards()
    out = g.embed(torch.empty((2, 3, 5, 16), dtype=torch.bfloat16))
    hip._call("fg_vae_patchify_bf16", _p(g.embed(vid[0])), _p(out), 2, 6, 10, st)
    g.check("patchify")
    assert torch.equal(_ncthw(out.cpu()[..., :12]), wan_vae.patchify2(vid)) and not out[..., 12:].any()
    v8 = seeded((3, 2, 5, 7), 715, scale=0.7).clamp(-1.2, 1.2)
    g = Guards()
    out = g.embed(torch.empty((2, 5, 7, 3), dtype=torch.uint8))
    hip._call("fg_video_to_uint8", _p(g.embed(v8)), _p(out), 2, 5, 7, st)
    g.check("video_to_uint8")
    assert torch.equal(out.cpu(), opipe.video_to_uint8(v8))
    # dupup3d_add: the vector-load form, the gather forms, Cin % 8 != 0
    for cin, cout, ft, fs, first in ((64, 64, 2, 2, True), (256, 64, 1, 2, False), (256, 32, 2, 2, False), (32, 48, 1, 2, False), (12, 24, 2, 2, True)):
        xs = seeded((1, cin, 2, 3, 5), 716)
        sc = wan_vae.dup_up3d(xs, cout, ft, fs, first)
        main = seeded(tuple(sc.shape), 717)
        g = Guards()
        got = hip.dupup3d_add(g.embed(_cl(xs)), g.embed(_cl(main)), cout, ft, fs, first, out=g.embed(torch.empty_like(_cl(main))))
        g.check(f"dupup3d {cin}->{cout}")
        assert torch.equal(_ncthw(got.cpu()), main + sc), (cin, cout, ft, fs, first)
    # avgdown3d_add (the wrapper allocates its output)
    for cin, cout, ft, fs, T in ((32, 32, 1, 2, 1), (32, 64, 2, 2, 1), (32, 64, 2, 2, 5), (64, 64, 1, 1, 2)):
        xs = seeded((1, cin, T, 6, 10), 718)
        sc = wan_vae.avg_down3d(xs, cout, ft, fs)
        main = seeded(tuple(sc.shape), 719)
        g = Guards()
        out = g.embed(torch.empty_like(_cl(main)))
        hip._call("fg_avgdown3d_add_bf16", _p(g.embed(_cl(xs))), _p(g.embed(_cl(main))), _p(out), T, 6, 10, cin, cout, ft, fs, st)
        g.check(f"avgdown3d {cin}->{cout}")
        assert torch.equal(out, hip.avgdown3d_add(dev(_cl(xs)), dev(_cl(main)), ft, fs))
        assert_close_bf16(_ncthw(out.cpu()), main + sc, 1.0, f"avgdown {cin}->{cout} ft{ft} fs{fs}", mag=main, max_mismatch=0.02)


# ------------------------------------------------------------------------------------------------------------------ 6. argument checks
def _argcheck_specs(P, gemm_ws):
    """(entry point, good arguments, {label: {argument index: broken value}}): P() is a fresh 16-byte aligned buffer address."""
    e, mx = 1e-6, 448.0
    S = []

    def add(name, args, breaks):
        S.append((name, args, breaks))

    a = [P(), P(), P(), P(), 5, 64, e, 1, 0, 64, None]
    add("fg_ln_modulate_bf16", a, {"x + 8 bytes": {0: a[0] + 8}, "out + 8 bytes": {3: a[3] + 8}, "C % 8": {5: 60}, "C > 4096": {5: 4104}, "mod_rows": {7: 3},
                                   "first_rows > rows": {8: 6}, "mod_ld % 8": {9: 60}, "null shift": {1: None}, "shift + 8": {1: a[1] + 8}, "scale + 8": {2: a[2] + 8}})
    a = [P(), P(), P(), P(), 5, 64, e, None]
    add("fg_ln_affine_bf16", a, {"x + 8": {0: a[0] + 8}, "w + 8": {1: a[1] + 8}, "b + 8": {2: a[2] + 8}, "out + 8": {3: a[3] + 8}, "C % 8": {5: 60}, "C > 4096": {5: 4104}, "null out": {3: None}})
    a = [P(), P(), P(), P(), 5, 64, 1, 0, 64, None]
    add("fg_gate_residual_bf16", a, {"x + 8": {0: a[0] + 8}, "out + 8": {3: a[3] + 8}, "y + 8": {1: a[1] + 8}, "gate + 8": {2: a[2] + 8}, "C % 8": {5: 60}, "C > 4096": {5: 4104}, "mod_rows": {6: 3},
                                     "mod_ld % 8": {8: 60}})
    a = [P(), P(), P(), P(), P(), P(), P(), 0, 5, 64, e, 1, 0, 64, None]
    add("fg_residual_ln_bf16", a, {"mode": {7: 2}, "norm_out + 8": {6: a[6] + 8}, "x + 8": {0: a[0] + 8}, "y + 8": {1: a[1] + 8}, "gate + 8": {2: a[2] + 8}, "x_out + 8": {3: a[3] + 8}, "p0 + 8": {4: a[4] + 8}, "p1 + 8": {5: a[5] + 8}, "mod_ld % 8": {13: 60}, "C % 8": {9: 60}, "C > 4096": {9: 4104}, "mod_rows": {11: 3}, "null p0": {4: None}})
    a = [P(), P(), P(), P(), P(), 5, 64, e, 1, 0, 64, mx, None]
    add("fg_ln_modulate_fp8_bf16", a, {"out_fp8 + 4": {3: a[3] + 4}, "fp8_max": {11: 0.0}, "C > 4096": {6: 4104}, "C % 8": {6: 60}, "x + 8": {0: a[0] + 8}})
    a = [P(), P(), P(), P(), P(), P(), P(), P(), 0, 5, 64, e, 1, 0, 64, mx, None]
    add("fg_residual_ln_fp8_bf16", a, {"mode": {8: 2}, "norm_fp8 + 4": {6: a[6] + 4}, "fp8_max": {15: 0.0}, "C > 4096": {10: 4104}, "null norm_scale": {7: None}})
    a = [P(), P(), P(), P(), P(), P(), 5, 64, e, 1, 0, 64, mx, None]
    add("fg_ln_modulate_dual_bf16", a, {"out + 8": {3: a[3] + 8}, "out_fp8 + 4": {4: a[4] + 4}, "fp8_max": {12: 0.0}, "C % 8": {7: 60}})
    a = [P(), P(), P(), P(), P(), P(), 5, 64, e, mx, None]
    add("fg_ln_affine_dual_bf16", a, {"out + 8": {3: a[3] + 8}, "out_fp8 + 4": {4: a[4] + 4}, "fp8_max": {9: 0.0}, "C > 4096": {7: 4104}})
    for s_form in (False, True):
        tail = [P(), 0, None] if s_form else [None]      # sched, workgroups, stream
        a = [P(), 256, P(), P(), P(), 256, 256, 256, 256, 0, None, 1, 0, 0, P(gemm_ws)] + tail
        add("fg_gemm_epilogue_bf16" + ("_s" if s_form else ""), a, {
            "N % 256": {7: 250}, "K % 128": {8: 192}, "lda < K": {1: 128}, "ldc < N": {5: 128}, "lda % 8": {1: 260}, "a + 8": {0: a[0] + 8},
            "c + 8": {4: a[4] + 8}, "mode": {9: 1}, "mode 2 without a gate": {9: 2}, "workspace + 8": {14: a[14] + 8}, "M = 0": {6: 0}, "null bias": {3: None}})
        a = [P(), 256, P(), P(), P(), P(), 256, 256, 256, 256, 0, None, 1, 0, 0, P(gemm_ws)] + tail
        add("fg_gemm_fp8_bf16" + ("_s" if s_form else ""), a, {
            "K % 256": {9: 128}, "lda % 16": {1: 264}, "null scale_a": {2: None}, "N % 256": {8: 250}, "ldc < N": {6: 128}, "w + 8": {3: a[3] + 8}, "mode": {10: 5}})
    a = [P(), 64, P(), P(), P(), 64, 8, 64, 64, 32, 1, 0, None, 1, 64, 0, None]
    add("fg_lora_apply_bf16", a, {"K % 64": {7: 32}, "rank": {9: 48}, "groups": {10: 5}, "ldx % 8": {1: 68}, "ldc < G * Ng": {5: 56}, "mode": {11: 3}, "out + 8": {4: a[4] + 8}})
    a = [P(), 64, P(), None, None, 0, P(), 5, 64, 2, e, None]
    add("fg_rmsnorm_rope_bf16", a, {"ldx < C": {1: 56}, "ldx % 8": {1: 68}, "C % 8": {8: 60, 1: 64}, "C % heads": {9: 3}, "x + 8": {0: a[0] + 8},
                                    "fp32 mode without a table": {5: 1}, "one fp64 table": {3: P()}, "cos + 8": {3: P() + 8, 4: P()}, "sin + 8": {3: P(), 4: P() + 8}, "fp32 table + 8": {3: P() + 8, 5: 1},
                                    "weight + 8": {2: a[2] + 8}, "out + 8": {6: a[6] + 8}, "C > 4096": {8: 4104, 1: 4104}})
    a = [P(), 64, P(), None, None, 0, P(), 5, 64, 2, e, 32, 160, 32, None]
    add("fg_rmsnorm_rope_grouped_bf16", a, {"group_cols does not divide C": {11: 24}, "out_ld < group_cols": {13: 16}, "group stride % 8": {12: 156}, "ldx < C": {1: 56}})
    a = [P(), 160, 32, P(), 160, 32, 2, 5, 32, None]
    add("fg_copy_groups_bf16", a, {"cols % 8": {8: 12}, "src_ld < cols": {2: 16}, "dst_ld % 8": {5: 36}, "src + 8": {0: a[0] + 8}, "groups = 0": {6: 0}})
    a = [P(), 16384, P(), P(), None, 5, 64, 0, mx, None]
    add("fg_fp8_quant_rows_bf16", a, {"ldx < C": {1: 56}, "C % 8": {6: 60}, "C > 14336": {6: 14344}, "act": {7: 2}, "act_out without act": {4: P()}, "fp8_max": {8: 0.0},
                                      "out_fp8 + 4": {2: a[2] + 4}, "ldx % 8": {1: 16388}})
    a = [P(), P(), 64, 0, None]
    add("fg_act_bf16", a, {"n % 8": {2: 60}, "kind": {3: 2}, "x + 8": {0: a[0] + 8}, "out + 8": {1: a[1] + 8}})
    a = [P(), 128, P(), 128, P(), 128, P(), 1, 8, 8, 1, 128, 0.1, None, 0, None]
    add("fg_attn_fwd_bf16", a, {"D != 128": {11: 64}, "B = 0": {7: 0}, "H = 0": {10: 0}, "Nkv = 0": {9: 0}, "ldq < H * D": {1: 120}, "ldk % 8": {3: 132}, "scale": {12: 0.0},
                                "q + 8": {0: a[0] + 8}, "k + 8": {2: a[2] + 8}, "v + 8": {4: a[4] + 8}, "out + 8": {6: a[6] + 8}, "K of 4 GiB": {9: 1 << 24, 3: 128}, "Q of 4 GiB": {8: 1 << 24},
                                "ldv % 8": {5: 132}, "ldv < H * D": {5: 120}, "workspace bytes without a workspace": {14: 64}, "workspace + 8": {13: P() + 8, 14: 64},
                                "null v": {4: None}})
    a = [P(), P(), None, P(), 64, 1.0, 0.1, None]
    add("fg_cfg_euler_bf16", a, {"null latents": {0: None}, "n < 0": {4: -1}})
    a = [P(), P(), P(), 5, 64, 1, None]
    add("fg_vae_rmsnorm_silu_bf16", a, {"C % 8": {4: 60}, "C > 2048": {4: 2056}, "x + 8": {0: a[0] + 8}, "null gamma": {1: None}})
    add("fg_conv_pack_weight_bf16", [P(), P(), 8, 8, 1, 1, 1, None], {"Cout = 0": {2: 0}, "null packed": {1: None}})
    a = [P(), P(), P(), None, P(), 1, 4, 4, 8, 8, 1, 1, 0, 0, None]
    add("fg_conv3d_cl_bf16", a, {"Cin % 8": {8: 12}, "Cout % 4": {9: 6}, "kt": {10: 2}, "ks": {11: 2}, "resample": {12: 3}, "stride 2 without the 3x3 kernel": {12: 2},
                                 "upsample with odd H": {12: 1, 6: 5}, "upsample with kt = 3": {12: 1, 10: 3}, "interleave with Cout % 8": {13: 1, 9: 12},
                                 "x + 8": {0: a[0] + 8}, "out + 4": {4: a[4] + 4}, "T = 0": {5: 0}, "null bias": {2: None}, "w_packed + 8": {1: a[1] + 8}, "bias + 4": {2: a[2] + 4},
                                 "residual + 4": {3: P() + 4}, "x of 3.75 GiB": {5: 60000, 6: 2048, 7: 2048}})
    a = [P(), P(), P(), 1, 2, 2, 8, 8, 1, 2, 0, None]
    add("fg_dupup3d_add_bf16", a, {"Cout % 8": {7: 12}, "ft": {8: 3}, "Cout * factor % Cin": {6: 24}, "x + 8": {0: a[0] + 8}, "out + 8": {2: a[2] + 8}})
    add("fg_softmax_rows_f32_bf16", [P(), P(), 5, 8, 1.0, None], {"rows = 0": {2: 0}, "cols = 0": {3: 0}, "null scores": {0: None},
                                                                    "scale = 0": {4: 0.0}, "scale < 0": {4: -0.25}, "scale = inf": {4: float("inf")}, "scale = nan": {4: float("nan")}})
    add("fg_vae_latent_to_cl_bf16", [P(), P(), P(), P(), 4, 1, 2, 2, None], {"C = 0": {4: 0}, "null z": {0: None}})
    add("fg_vae_unpatchify_bf16", [P(), P(), 2, 2, 2, 4, 1, 0, None], {"t0 + T > F": {6: 3}, "t0 < 0": {6: -1}, "T = 0": {2: 0}})
    add("fg_vae_tile_accumulate_bf16", [P(), P(), P(), 3, 1, 8, 8, 4, 4, 2, 2, 2, 2, 0, None],
        {"y0 + th > Hv": {9: 6}, "x0 < 0": {10: -1}, "border wider than the tile": {11: 6}, "null weight": {2: None}})
    add("fg_vae_tile_finalize_bf16", [P(), P(), 3, 1, 8, 8, 1, None], {"C = 0": {2: 0}, "null weight": {1: None}})
    add("fg_vae_patchify_bf16", [P(), P(), 1, 4, 4, None], {"odd H": {3: 5}, "odd W": {4: 5}})
    add("fg_avgdown3d_add_bf16", [P(), P(), P(), 2, 4, 4, 8, 8, 1, 2, None], {"H % fs": {4: 5}, "ft": {8: 3}, "Cin * factor % Cout": {7: 12}, "null x": {0: None}})
    add("fg_vae_latent_from_cl_bf16", [P(), P(), P(), P(), 4, 8, 1, 2, 2, None], {"Cx < Z": {5: 2}, "null mean": {1: None}})
    add("fg_video_to_uint8", [P(), P(), 1, 4, 4, None], {"F = 0": {2: 0}, "null out": {1: None}})
    add("fg_softmax_bias_bf16", [P(), P(), None, P(), 5, 8, None], {"rows = 0": {4: 0}, "cols = 0": {5: 0}, "null bias": {1: None}})
    a = [P(), P(), P(), 64, None]
    add("fg_gated_gelu_bf16", a, {"n % 8": {3: 60}, "fc1 + 8": {0: a[0] + 8}, "out + 8": {2: a[2] + 8}})
    return S


def test_argument_checks():
    """Every entry point of the header, one call per precondition it documents and checks — every shape rule, range and leading dimension,
    and the alignment of the pointers named in _argcheck_specs (each pointer of the kernels of cases 1 to 4; a representative pointer
    of the others) — with exactly that precondition broken: FG_EINVAL and a
    message that names the function, from the host check, before any launch.  With a device every pointer is a real zeroed 4 MiB buffer
    (the shapes are tiny: a check that were missing would launch inside owned memory) and the unbroken call must succeed first;
    without one the pointers are fake and only the rejections are checked."""
    from fairygen_amd import hip
    lib = hip.load()
    have_dev = torch.cuda.is_available()
    keep = []

    def P(nbytes=1 << 22):
        if not have_dev:
            keep.append(None)
            return (len(keep) + 16) << 22
        keep.append(torch.zeros(max(nbytes, 1 << 22), dtype=torch.uint8, device="cuda"))
        assert keep[-1].data_ptr() % 16 == 0
        return keep[-1].data_ptr()

    def call(name, args):
        conv = [ctypes.c_void_p(v) if t is ctypes.c_void_p and v is not None else v for v, t in zip(args, getattr(lib, name).argtypes)]
        return getattr(lib, name)(*conv)

    specs = _argcheck_specs(P, lib.fg_gemm_workspace_bytes(256, 256, 256))
    covered = {s[0] for s in specs}
    skipped = {      # entry point -> "file::test" that holds its argument checks
        "fg_gemm_sched_reset": "test_gemm_sched_state.py::test_s_entry_points_validate_sched_and_workgroups",
        "fg_lora_fuse_bf16": "test_lora_fuse_kernel.py::test_argument_checks",
        "fg_cfg_euler_dev_bf16": "test_graph_step.py::test_cfg_euler_dev_argument_checks",
        "fg_attn_quant_qk_bf16": "test_attention_qk8.py::test_argument_checks",
        "fg_attn_fwd_qk8_bf16": "test_attention_qk8.py::test_argument_checks",
        "fg_rmsnorm_rope_q8_bf16": "test_attention_qk8_fused.py::test_argument_checks",
        "fg_rmsnorm_rope_kstats_bf16": "test_attention_qk8_fused.py::test_argument_checks",
        "fg_attn_quant_k_bf16": "test_attention_qk8_fused.py::test_argument_checks",
    }
    assert covered | set(skipped) == set(hip._SIGNATURES) and not covered & set(skipped), sorted(set(hip._SIGNATURES) - covered - set(skipped))
    for name, home in skipped.items():
        path, test = home.split("::")
        assert f"\ndef {test}(" in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), path)).read(), f"{name}: {home} does not exist"
    for name, args, breaks in specs:
        assert len(args) == len(getattr(lib, name).argtypes), name
        if have_dev:
            assert call(name, args) == 0, f"{name}: the unbroken call failed: {lib.fg_last_error().decode()}"
            torch.cuda.synchronize()
        for label, change in breaks.items():
            bad = list(args)
            for i, v in change.items():
                bad[i] = v
            rc = call(name, bad)
            msg = lib.fg_last_error().decode() if rc != 0 else ""
            assert rc == -1 and name.removesuffix("_s") in msg, f"{name} with {label}: returned {rc} ({msg!r}), expected FG_EINVAL naming the function"
    if have_dev:
        torch.cuda.synchronize()
    with pytest.raises(hip.HipLibraryError, match="fg_softmax_rows_f32_bf16"):      # as the wrappers see it: the kernel's row maximum is that of the unscaled scores
        hip._call("fg_softmax_rows_f32_bf16", ctypes.c_void_p(P()), ctypes.c_void_p(P()), 5, 8, -0.25, None)
    R, S_ = ctypes.c_int(), ctypes.c_int()
    assert lib.fg_attn_split_choice(0, 8, 8, 1, 0, ctypes.byref(R), ctypes.byref(S_)) == -1 and b"fg_attn_split_choice" in lib.fg_last_error()
    assert lib.fg_attn_split_choice(1, 8, 8, 1, 0, None, ctypes.byref(S_)) == -1
    assert lib.fg_attn_workspace_bytes(0, 8, 8, 1) == 0 and lib.fg_gemm_workspace_bytes(256, 250, 256) == 0 and lib.fg_conv_packed_bytes(0, 8, 1, 1, 1) == 0

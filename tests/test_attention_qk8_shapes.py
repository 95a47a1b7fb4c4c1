"""The e4m3 attention entry points (include/fairygen_hip.h) at every width and KV length they accept.

tests/test_attention_qk8.py and tests/test_attention_qk8_fused.py pin the recipe at the shapes the tiny and the full DiT use: 2 and 24
heads, Nq = Nkv in {1 100, 2 049}.  The headers accept every C = num_heads * 128 <= 4 096 and "any Nkv >= 1"; this file runs the rest,
with the helpers, references and criteria of those two files (imported, not copied) and nothing loosened.

Entry point, the instantiation or path each case reaches, and how that was confirmed:
  fg_rmsnorm_rope_kstats_bf16   rmsnorm_rope_kstats_kernel<F32TAB, NV>, NV = ceil(C / 512) (the launcher's switch): heads 1, 4 -> NV 1
                     (partial, full); 5, 8 -> 2; 9, 12 -> 3; 16 -> 4; 17, 20 -> 5; 28 -> 7; 31, 32 -> 8 (partial: the last vector slot is
                     live in 48 or 16 of the 64 lanes; full = C = 4 096, the maximum).  With the 2 and 24 heads (NV 1 and 6) of the older
                     file every NV in 1..8 runs — held by test_every_instantiation_is_named — in both F32TAB forms (table modes "f32" /
                     "f64"; "none" takes the fp64 form without a table).  N = 70: fg_attn_qk8_fused_scratch_bytes gives 8 records
                     (asserted), so 8 workgroups x 4 rows walk the rows in three passes, the last one (rows 64..69) ragged.  N = 3: seven
                     of the eight workgroups have no row and leave the neutral record.
  fg_rmsnorm_rope_q8_bf16       the kMaxVec loop with `vi < nvec` live in part of the lanes (the same head counts).
  fg_attn_quant_k_bf16          attn_k_finalise_kernel and attn_quant_k_kernel at h * 128 for h up to 31, P = 8 records.
  fg_attn_quant_qk_bf16         attn_k_stats_kernel and attn_quant_qk_kernel at 1, 5, 17, 32 heads against the CPU recipe (the yardstick
                     of the three above must itself be right at these widths), and at every width above as that yardstick.
  fg_attn_fwd_qk8_bf16          attn_fwd_kernel<true> at 3 heads (odd: bh % H, the XCD remap over 3 or 6 workgroups) on one
                     key, fewer keys than a tile, one full tile, a ragged second tile, Nq < 256, Nq = 2 x 256 + 1, Nkv = 1 024 and 1 025,
                     Nq != Nkv in both directions; every case without a workspace (direct workgroups only) and with the default one.
                     fg_attn_split_choice (asserted): (R, S) = (1, 2) for (64, 1 000), (256, 1 024), (70, 1 300) and (2, 2) for
                     (257, 1 025) with the workspace — pieces + attn_combine_kernel — and (0, 1) for the other six and for every case
                     without one.
  fg_attn_qk8_fused_scratch_bytes, the version helpers   through the calls above (8 records at N = 70 and N = 3).

Tie counts (bytes of q8 and k8 together that differ from the emulation, which may happen only where the quotient lies within one fp32 ulp
of an e4m3 rounding tie and in at most 0.1 % of the elements), for 1, 5, 17, 32 heads.  The recipe with x * (1 / s) on the CPU: N = 3:
0 / 768, 0 / 3 840, 1 / 13 056, 7 / 24 576 (0.028 %); N = 70: 1 / 17 920, 23 / 89 600, 54 / 304 640, 145 / 573 440 (0.025 %).  The kernel on
the MI355X: 0 bytes differ in all eight cases (its division is IEEE's), with 0 .. 1 401 quotients within an ulp of a tie.

Cost: the unmarked self-checks take 4 s of pytest time on a CPU-only host, imports included (1.6 s of test time); the whole file, 79
tests, 3.6 s of pytest time on an MI355X, the slowest test 0.4 s (the first to touch the device).
"""
import functools

import pytest
import torch

import test_attention_qk8 as qk8
import test_attention_qk8_fused as fused
from conftest import seeded
from fairygen_amd import hip as _hip
from test_attention_qk8 import hip  # noqa: F401  (the module fixture)
from test_buffer_contract import Guards, _split_choice
from test_hip_kernels import ATTN_FLOOR

gpu = pytest.mark.gpu
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ A. the producers
WIDTH_HEADS = (1, 4, 5, 8, 9, 12, 16, 17, 20, 28, 31, 32)
EXTRA_HEADS = (5, 32)       # these also run without a rope table and at N = 3
WIDTH_N = 70                # 8 workgroups x 4 rows: passes over rows 0..31, 32..63 and the ragged 64..69


def variants_of(heads):
    return ("normal", "offset") + (("flat-head", "zero-row") if heads == 5 else ())


def producer_cases():
    for n, some in ((WIDTH_N, WIDTH_HEADS), (3, EXTRA_HEADS)):
        for heads in some:
            for mode in ("f32", "f64") + (("none",) if heads in EXTRA_HEADS else ()):
                yield n, heads, mode


def test_every_instantiation_is_named():
    """NV = ceil(C / 512) over the head counts here and in tests/test_attention_qk8_fused.py: all eight; here NV 1, 2, 3, 5 and 8 also with
    a head count that is no multiple of 4 (the last vector slot live in part of the lanes), and the maximum C = 4 096."""
    nv = lambda heads: (heads * 128 + 511) // 512      # noqa: E731
    assert {nv(h) for h in WIDTH_HEADS} | {nv(h) for _, h in fused.SHAPES} == set(range(1, 9))
    assert {nv(h) for h in WIDTH_HEADS if h % 4} == {1, 2, 3, 5, 8} and {nv(h) for h in WIDTH_HEADS if h % 4 == 0} == {1, 2, 3, 4, 5, 7, 8}
    assert max(WIDTH_HEADS) * 128 == 4096


def test_width_inputs_lie_where_the_sum_is_exact():
    """The condition of the comparison of the key mean, as tests/test_attention_qk8_fused.py holds it for its shapes: on the CPU
    emulation of the norm, with 2 bits in hand; the GPU test repeats the count on the kernel's own keys."""
    for n, heads in sorted({(n, heads) for n, heads, _ in producer_cases()}):
        for variant in variants_of(heads):
            fused.check_sum_is_exact(n, heads, variant)


@gpu
@pytest.mark.parametrize("n,heads,mode", list(producer_cases()))
def test_producers_at_every_width(hip, n, heads, mode):  # noqa: F811
    """fg_rmsnorm_rope_kstats_bf16, fg_rmsnorm_rope_q8_bf16 and fg_attn_quant_k_bf16 equal hip.rmsnorm_rope x 2 -> hip.attn_quant_qk byte
    for byte on poisoned, guarded buffers (test_producers_equal_the_two_step_path's check, exact_sum_bits <= 52 included)."""
    c = heads * 128
    assert hip.load().fg_attn_qk8_fused_scratch_bytes(n, c) == 8 * 16 * c, "8 records: the walk this case is for"
    fused.check_producers(hip, n, heads, mode, variants_of(heads))


QUANT_CASES = [(n, heads) for heads in (1, 5, 17, 32) for n in (3, WIDTH_N)]


def test_recipe_tie_exemption_is_rare_at_these_widths():
    """test_recipe_tie_exemption_is_rare on the cases below: the recipe with its quotient formed as x * (1 / s) differs from the emulation
    only at rounding ties and in fewer than 0.1 % of the elements (counts: the module docstring)."""
    for n, heads in QUANT_CASES:
        qk8.check_tie_exemption(n, heads)


@gpu
@pytest.mark.parametrize("n,heads", QUANT_CASES)
def test_quant_qk_at_these_widths(hip, n, heads):  # noqa: F811
    """fg_attn_quant_qk_bf16 against quant_emu under test_quant_qk_against_the_recipe's criterion: scales and key mean equal, bytes equal
    outside rounding ties, at most 0.1 % of them at one.  Measured on the MI355X: no byte differs in any of the eight cases (the module
    docstring has the counts)."""
    qk8.check_quant_qk(hip, n, heads)


# ------------------------------------------------------------------------------------------------------------------ B. the KV edges
KV_HEADS = 3
KV_CASES = ((1, 1), (31, 5), (256, 64), (300, 77), (64, 1000), (513, 512), (256, 1024), (257, 1025), (1300, 70), (70, 1300))
EXACT_CASES = ((64, 1000), (257, 1025), (1300, 70), (70, 1300))
GUARD_CASES = ((300, 77), (257, 1025), (70, 1300))
SPLITS = {(64, 1000): (1, 2), (256, 1024): (1, 2), (257, 1025): (2, 2), (70, 1300): (1, 2)}      # with the workspace; every other case (0, 1)
WS = pytest.mark.parametrize("ws", [False, True], ids=["direct", "workspace"])


def quantise(hip, q, k, heads):  # noqa: F811
    """q (Nq, C), k (Nkv, C) bf16 on the device -> q8, k8, sq, sk of fg_attn_quant_qk_bf16.  Nq != Nkv: two calls, each with zeros for
    the operand it is not about, so that sk and the key mean come from these Nkv keys and nothing else."""
    if q.shape == k.shape:
        return tuple(hip.attn_quant_qk(q[None], k[None], heads)[:4])
    q8, _, sq, _, _ = hip.attn_quant_qk(q[None], torch.zeros_like(q)[None], heads)
    _, k8, _, sk, _ = hip.attn_quant_qk(torch.zeros_like(k)[None], k[None], heads)
    return q8, k8, sq, sk


def fwd(hip, q8, k8, sq, sk, v, heads, ws, out=None):  # noqa: F811
    """fg_attn_fwd_qk8_bf16 on device operands, v (1, Nkv, C).  ws True: hip.attention_qk8_pre with its default workspace; False: no
    workspace at all, every q-block one direct workgroup."""
    if ws:
        return hip.attention_qk8_pre(q8, k8, sq, sk, v, heads, out=out)
    nq, nkv, c = q8.shape[0], k8.shape[0], heads * 128
    out = torch.empty((1, nq, c), dtype=BF16, device="cuda") if out is None else out
    hip._call("fg_attn_fwd_qk8_bf16", hip._ptr(q8), hip._ptr(k8), hip._ptr(sq), hip._ptr(sk), hip._ptr(v), hip._ld_rows(v, "v"), hip._ptr(out),
              nq, nkv, heads, 128, 128 ** -0.5, None, 0, hip._stream(v))
    return out


def split_of(hip, nq, nkv, ws):  # noqa: F811
    """(R, S) of fg_attn_split_choice for the launch fwd() makes, held to what the case is meant to reach."""
    R, S, _ = _split_choice(hip, 1, nq, nkv, KV_HEADS, ws)
    assert (R, S) == (SPLITS.get((nq, nkv), (0, 1)) if ws else (0, 1)), f"Nq = {nq}, Nkv = {nkv}: fg_attn_split_choice gives {(R, S)}"
    return R, S


@functools.lru_cache(maxsize=None)
def kv_case(nq, nkv):
    """N(0, 1) q, k, v; the operands hip.attn_quant_qk makes of them (on the device); the fp64 emulation on those bytes.  Once per shape."""
    c = KV_HEADS * 128
    q, k, v = seeded((nq, c), 5000 + nq), seeded((nkv, c), 6000 + nkv), seeded((nkv, c), 7000 + nkv)
    ops = quantise(_hip, q.cuda(), k.cuda(), KV_HEADS)
    torch.cuda.synchronize()
    q8, k8, sq, sk = (t.cpu() for t in ops)
    _, _, sq_emu, sk_emu, _, _ = qk8.quant_emu(q, k, KV_HEADS)
    assert torch.equal(sq, sq_emu) and torch.equal(sk, sk_emu), "the scales are not those of these queries and these keys"
    ref = qk8.attn_emu(q8, k8, sq, sk, v, KV_HEADS)
    err_ref = (ref.to(BF16).double() - ref).abs().max().item()
    return ops, v, ref, err_ref


@gpu
@WS
@pytest.mark.parametrize("nq,nkv", KV_CASES)
def test_attention_qk8_at_the_kv_edges(hip, nq, nkv, ws):  # noqa: F811
    """max|hip - emu_f64| <= 2 max|bf16(emu_f64) - emu_f64| + ATTN_FLOOR with attn_emu on the same q8, k8, sq, sk bytes — the criterion
    of test_attention_qk8_against_the_recipe; one query on one key returns that key's v row bit for bit."""
    ops, v, ref, err_ref = kv_case(nq, nkv)
    R, S = split_of(hip, nq, nkv, ws)
    got = fwd(hip, *ops, v.cuda()[None], KV_HEADS, ws)
    torch.cuda.synchronize()
    got = got[0].cpu()
    assert got.shape == (nq, KV_HEADS * 128)
    assert torch.isfinite(got.float()).all(), f"{(~torch.isfinite(got.float())).sum().item()} elements are not finite"
    err = (got.double() - ref).abs().max().item()
    print(f"qk8 attention Nq = {nq}, Nkv = {nkv}, {KV_HEADS} heads, {'workspace' if ws else 'direct'}: (R, S) = {(R, S)}, err {err:.3e}, "
          f"bf16(emu) err {err_ref:.3e}")
    assert err <= 2 * err_ref + ATTN_FLOOR, f"err {err} vs {err_ref}"
    if (nq, nkv) == (1, 1):
        assert torch.equal(got, v), "one key: the output is its v row"


def exact_must(nkv):
    """Key 0, the last key, the first and the last key of the ragged last tile (of the last tile where none is ragged)."""
    return (0, nkv - 1, (nkv - 1) // 64 * 64, nkv - 1)


def test_exact_case_construction_at_the_kv_edges():
    """test_exact_case_construction for Nq != Nkv and 3 heads: the gap condition, the exact scales and bytes, the fp64 emulation equal
    to the index expectation, and the named keys selected (1 025 keys: the zero row of the odd count is key 512, the last key is live)."""
    for nq, nkv in EXACT_CASES:
        qk8.check_exact_case(nq, nkv, KV_HEADS, exact_must(nkv))


@gpu
@WS
@pytest.mark.parametrize("nq,nkv", EXACT_CASES)
def test_attention_qk8_exact_at_the_kv_edges(hip, nq, nkv, ws):  # noqa: F811
    """test_attention_qk8_exact for Nq != Nkv: out[r] is the one-hot v row of the key query r selects, bit for bit — a dropped or doubled
    key, which the max-abs bound has room for at ~1 000 keys, changes a row."""
    q, k, v, want, _ = qk8.exact_case(nq, nkv, KV_HEADS, exact_must(nkv))
    split_of(hip, nq, nkv, ws)
    got = fwd(hip, *quantise(hip, q.cuda(), k.cuda(), KV_HEADS), v.cuda()[None], KV_HEADS, ws)
    torch.cuda.synchronize()
    bad = (got[0].cpu() != want).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {nq} rows differ from the selected v row, first {bad[:8].tolist()}"


@gpu
@WS
@pytest.mark.parametrize("nq,nkv", GUARD_CASES)
def test_attention_qk8_guarded(hip, nq, nkv, ws):  # noqa: F811
    """q8, k8, sq, sk and v as views between bands of NaN (0x7F bytes for e4m3), v with NaN columns inside its leading dimension, out
    between sentinel bands: a key row read past Nkv or a sq row past Nq turns the result non-finite, a write past out shows in the
    bands.  The result equals the unguarded call's bit for bit."""
    ops, v, _, _ = kv_case(nq, nkv)
    plain = fwd(hip, *ops, v.cuda()[None], KV_HEADS, ws)
    g = Guards()
    q8, k8, sq, sk = (g.embed(t, 16, 64) for t in ops)
    out = g.embed(torch.empty((1, nq, KV_HEADS * 128), dtype=BF16), 16, 256)
    got = fwd(hip, q8, k8, sq, sk, g.embed(v[None], 16, 64, 128, 8), KV_HEADS, ws, out=out)
    g.check(f"Nq = {nq}, Nkv = {nkv}, {'workspace' if ws else 'direct'}")
    assert got.data_ptr() == out.data_ptr() and torch.isfinite(got.float()).all()
    assert torch.equal(got, plain), f"{(got != plain).sum().item()} elements differ from the call on compact operands"


# ------------------------------------------------------------------------------------------------------------------ C. composed
@gpu
def test_composed_attention_at_five_heads(hip):  # noqa: F811
    """hip.attention_qk8 end to end at C = 640 (NV = 2, partial) over 1 100 tokens on strided q | k | v column slices: the fused producers
    -> fg_attn_fwd_qk8_bf16 equal the two-step composition (test_composed_attention_equals_the_two_step_path's check)."""
    fused.check_composed_attention(hip, 1100, 5)

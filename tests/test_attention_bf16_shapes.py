"""fg_attn_fwd_bf16 at every KV residue, KV-range length and ragged q-block, on inputs that show a leaked or a dropped key.

The older attention tests (test_hip_kernels.py, test_exact_arithmetic.py, test_buffer_contract.py) cannot see a wrong mask of the ragged
last KV tile: keys at positions >= Nkv arrive as ZEROS through the bounded buffer descriptor, so on N(0, 1) data a leaked key has logit 0,
V = 0 and weight ~1 / Nkv (it shrinks an output of ~Nkv^-1/2 by 1 / Nkv: 3e-5 on the 4-wave kernel against ATTN_FLOOR = 2e-3), and in the
gather construction it lies 181 nats below the selected key.  Here every real logit lies far below 0, so one zero key wins the softmax.

Inputs ("sink" and "deep", _case): per head a sign vector u in {+-1}^128, sign vectors m_i per query row and n_j per key, all bf16-exact:
  sink   q_i = 4 u + m_i / 2,   k_j = -9/16 u + n_j / 8   (logits -25.5 +- 0.5 nats),  anchors k_j = -3/8 u + n_j / 8     (-17 nats)
  deep   q_i = 16 u + m_i / 2,  k_j = -u + n_j / 64       (logits -181 +- 0.25 nats),  anchors k_j = -61/64 u + n_j / 64  (-172.5 nats)
The anchors — position 0, the first key of the last tile and position Nkv - 1 (fewer where they coincide) — lie 8.5 nats above the rest;
V = 1 + N(0, 1) / 4, the anchor rows shifted by +3, +4 and +5 on the channels c % 3 = 0, 1 and 2.  Every correct output element is O(1); one leaked zero key takes
> 99.9 % of the weight, a dropped anchor moves the output by >= 10 x the allowance (asserted per case).  (The magnitudes differ from the ones the sweep was first
sketched with — q = 2 u, anchors 5.7 nats up — because those put the anchors at -5.7 nats, above the -8 the self-check asks of EVERY real
logit, and left a dropped anchor at 11 x the allowance at Nkv = 2 112; one scalar shift per anchor left the middle one between the other
two, where dropping it can move nothing; n_j / 32 in the deep keys left anchor weights too uneven.  The conditions are untouched.)  The deep variant has an answer only
if the running maximum starts at -inf or at the first tile's maximum: a kernel that starts it at 0, or lets a zero score of a masked key
or of a prefetched tile into a row maximum, returns 0 / 0 or zeros.
Criterion, the project's own: error to wan_dit.attention in fp32 <= 2 x the error of the oracle's bf16 result + ATTN_FLOOR, the output
finite, nothing loosened; for the power-of-two scale the fp32 reference is the oracle on q / fold (test_attention_w4_deferred_rescale).
The unmarked self-checks hold for every case of every table, against both references where a case runs both forms: the fp32 reference
with one all-zero key and V row appended, and with any one anchor removed, differs from the true one by >= 10 x the case's allowance;
every real logit < -8 nats (sink) / < -120 nats (deep); the oracle's bf16 result is finite; the tables cover what is claimed below.

Entry point fg_attn_fwd_bf16; kernel and path per test, and how that was confirmed (kernel: the Nkv threshold of the dispatch in
csrc/attention.hip; body of the 4-wave kernel: the scale — 1 / sqrt(d) -> attn_fwd_w4_kernel<false>, hip.pow2_softmax_scale(128) -> <true>;
direct workgroups: no workspace, so fg_attn_split_choice gives (0, 1), asserted; pieces + attn_combine_kernel: S > 1 asserted from
fg_attn_split_choice with fg_attn_workspace_bytes):
  test_kv_sweep_direct   Nq = 70, H = 1: one ragged q-block (waves 3..7 of the 8-wave template and waves 2..3 of the 4-wave kernel own
                     no valid row).  attn_fwd_kernel<>: every Nkv in 1..128 (nt = 1, 2 x all 64 residues), one Nkv per nt in 3..16 with
                     residue 17 nt mod 64, 1 023, 1 024.  attn_fwd_w4_kernel<false> and <true>: every Nkv in 1 025..1 088 (nt = 17, all 64
                     residues), nt = 18, 19, 20 at residues 0, 1, 31, 32, 33, 63 (every nt & 3 = every tail copy, ragged and whole),
                     2 049 and 2 112.  sink and deep.
  test_kv_sweep_split    the shapes of the above that split with the default workspace: Nkv = 976, 1 023, 1 024 on the template (nt = 16)
                     and every 4-wave shape, both bodies, sink and deep; each result also against the direct one.
  test_split_shapes      (70, 1 381, 1), (70, 1 509, 1), (257, 1 025 + r, 1), (300, 1 000 + r, 24), (700, 2 700 + r, 24), r in 0, 1, 37.
  test_split_table_covers_every_piece_length   the measured (R, S) and piece lengths (sp + 1) nt // S - sp nt // S of all of these.
  test_nq_sweep          Nq in 1 .. 511 (NQ_SWEEP) at Nkv = 100 (template) and 1 061 (4-wave, both bodies; direct and split): out lies in
                     NaN bands (Guards) and is NaN before the call: a written row >= Nq and an unwritten row < Nq both fail.
  test_remap_sweep       H x ceil(Nq / 256) = 1..9 and 16 direct workgroups (every total_direct & 7, a second slot), H in 1, 2, 3.
  test_batch_of_two      B = 2 at Nq = 70, element 1 of another seed, q | k | v column slices of one (2 Nkv, 3 C) buffer in NaN.
  test_gather_edges      test_exact_arithmetic's gather (each query row reaches its own key, bit for bit) at (129, 65), (257, 127),
                     (257, 1 061), (513, 1 089), both scales.

Measured on an MI355X (256 CUs), all of it with this file:
  * every GPU test passes, the deep variant included, on all three kernels: no kernel change came out of the sweep.
  * (R, S) from fg_attn_split_choice with the default workspace, and the piece lengths in tiles: (70, 976 | 1 023 | 1 024, 1) -> (1, 2),
    8 + 8; (70, 1 025..1 088, 1) -> (1, 2), 8 + 9; nt = 18 -> (1, 2), 9 + 9; nt = 19 -> (1, 2), 9 + 10; nt = 20 -> (1, 2), 10 + 10;
    (70, 2 049 | 2 112, 1) -> (1, 4), 8 + 8 + 8 + 9; (70, 1 381, 1) -> (1, 2), 11 + 11; (70, 1 509, 1) -> (1, 3), 8 + 8 + 8;
    (257, 1 025 | 1 026 | 1 062, 1) -> (2, 2), 8 + 9; (300, 1 000 | 1 001, 24) -> (2, 2), 8 + 8 (template); (300, 1 037, 24) -> (2, 2),
    8 + 9 (4-wave); (700, 2 700 | 2 701 | 2 737, 24) -> (3, 3), 14 + 14 + 15.  Last pieces of the 4-wave kernel: 8, 9, 10, 11, 15 tiles,
    the others 8, 9, 10, 11, 14: every length mod 4 in both.  The template's pieces are 8 + 8 in every case and cannot be anything else
    (choose_split needs S * 8 <= nt, the template runs nt <= 16): "both parities among the template's pieces" holds for the ring parity
    (every piece runs fast steps of both parities and a two-step tail), not for the range length; odd lengths run direct (nt = 3..15).
  * split against direct: with the allowance alone as the bound, (700, 2 700, 24) sink lies 0.03125 apart — one bf16 ulp of an element in
    [4, 8) — against an allowance of 0.02937, both results within the allowance of the fp32 reference.  The bound is therefore the
    allowance plus one bf16 ulp of the element (_split_and_direct).
  * mutations, one at a time on a scratch copy (tests that fail: this file | the attention tests of test_hip_kernels.py |
    test_exact_arithmetic.py | test_buffer_contract.py):
      `>= Nkv` -> `> Nkv` in mask_tile (attn_fwd_body.inc)      17 of 74 | 2 (test_attention_shapes (300, 77) and (31, 5)) | 0 | 2 (nkv-1)
                                                                 (141 of the template's 144 KV lengths: all but the whole tiles)
      V_THR one key too large (gen_attn_w4.py)                  48 of 74 | 0 | 0 | 0   (79 of the 84 4-wave KV lengths, each body)
      `4 hh` dropped from V_THR                                 48 of 74 | 0 | 0 | 0   (69 of 84, each body)
  * cost: the 74 GPU tests take 5.7 s of pytest time, CPU references included, the slowest 0.28 s ((700, 2 737, 24)); the other sweep
    files report 3 to 8 s, so nothing was thinned.  The 9 unmarked self-checks (526 cases, about 3 700 oracle calls) take 6.5 s of pytest
    time on an 8-thread CPU-only host (not measured on the GPU host).
"""
import functools
from collections import namedtuple

import pytest
import torch

from fairygen_amd import hip as _hip
from oracle import wan_dit
from test_buffer_contract import Guards, _attn, _split_choice
from test_exact_arithmetic import MIN_GAP_NATS, _gather_case, _gather_on_gpu
from test_hip_kernels import ATTN_FLOOR, dev, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
POW2_SCALE, FOLD = _hip.pow2_softmax_scale(128)
W4_MIN = 1025                    # the dispatch of csrc/attention.hip: Nkv > 1024 -> attn_fwd_w4_kernel
LOGIT_BELOW = {"sink": -8.0, "deep": -120.0}
ANCHOR_SHIFT = (3.0, 4.0, 5.0)   # added to the V rows of: position 0, the first key of the last tile, position Nkv - 1, each on its own
                                 # third of the channels (c % 3 = 0, 1, 2): no anchor row lies between the other two in every channel
MARGIN = 10.0                    # a leaked zero key / a dropped anchor moves the fp32 reference by >= MARGIN x the allowance


def _tiles(nkv):
    return (nkv + 63) // 64


def _forms(nkv):
    return ("plain", "pow2") if nkv >= W4_MIN else ("plain",)


# ------------------------------------------------------------------------------------------------------------------ the case tables
NQ = 70
SHORT_KV = list(range(1, 129)) + [64 * (nt - 1) + 17 * nt % 64 for nt in range(3, 17)] + [1023, 1024]
W4_KV = list(range(1025, 1089)) + [64 * nt if r == 0 else 64 * (nt - 1) + r for nt in (18, 19, 20) for r in (0, 1, 31, 32, 33, 63)] + [2049, 2112]
SHORT_SPLIT_KV = [n for n in SHORT_KV if _tiles(n) == 16]           # S * 8 <= nt in choose_split: the template splits at 16 tiles only
SPLIT_SHAPES = [(70, 1381, 1), (70, 1509, 1)] + [(nq, nkv + r, heads) for nq, nkv, heads in ((257, 1025, 1), (300, 1000, 24), (700, 2700, 24))
                                                  for r in (0, 1, 37)]
NQ_SWEEP = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511)
NQ_SWEEP_KV = (100, 1061)
REMAP = [(1, 1), (2, 1), (3, 1), (2, 2), (1, 5), (3, 2), (1, 7), (2, 4), (3, 3), (2, 8)]      # (H, q-blocks): 1..9 and 16 workgroups
GATHER_EDGES = [(129, 65, 1), (257, 127, 2), (257, 1061, 2), (513, 1089, 1)]


def _groups(values, size):
    return [values[i:i + size] for i in range(0, len(values), size)]


SHORT_GROUPS, W4_GROUPS = _groups(SHORT_KV, 36), _groups(W4_KV, 28)
KV_SWEEP = [("short", "plain", g) for g in SHORT_GROUPS] + [("w4", form, g) for form in ("plain", "pow2") for g in W4_GROUPS]
KV_SWEEP_SPLIT = [("short", "plain", SHORT_SPLIT_KV)] + [("w4", form, g) for form in ("plain", "pow2") for g in W4_GROUPS]


def _sweep_id(p):
    return f"{p[0]}-{p[1]}-{p[2][0]}..{p[2][-1]}"


def _remap_nq(blocks):
    return 256 * (blocks - 1) + NQ


def _all_keys():
    """Every (nq, nkv, heads, kind, seed) that some GPU test runs."""
    keys = []
    for kind in ("sink", "deep"):
        keys += [(NQ, nkv, 1, kind, 0) for nkv in SHORT_KV + W4_KV]
        keys += [(nq, nkv, heads, kind, 0) for nq, nkv, heads in SPLIT_SHAPES]
    keys += [(nq, nkv, 1, "sink", 0) for nkv in NQ_SWEEP_KV for nq in NQ_SWEEP]
    keys += [(_remap_nq(blocks), nkv, heads, "sink", 0) for nkv in NQ_SWEEP_KV for heads, blocks in REMAP]
    keys += [(NQ, nkv, 2, "sink", seed) for nkv in NQ_SWEEP_KV for seed in (0, 1)]
    return sorted(set(keys))


# ------------------------------------------------------------------------------------------------------------------ the construction
Case = namedtuple("Case", "q k v anchors")
Refs = namedtuple("Refs", "plain32 err_ref finite16")


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _anchors(nkv):
    """(position, shift of its V row (128,)): position 0, the first key of the last tile, the last key; one entry where they coincide."""
    roles = {}
    for role, (pos, shift) in enumerate(zip((0, 64 * (_tiles(nkv) - 1), nkv - 1), ANCHOR_SHIFT)):
        roles[pos] = shift * (torch.arange(128) % 3 == role).float()
    return sorted(roles.items())


@functools.lru_cache(maxsize=None)
def _case(nq, nkv, heads, kind, seed=0):
    g = torch.Generator("cpu").manual_seed(77000 + 1000003 * seed + 131 * nq + 7 * nkv + heads + (0 if kind == "sink" else 500000))
    u, m, n = _signs((1, heads, 128), g), _signs((nq, heads, 128), g), _signs((nkv, heads, 128), g)
    if kind == "sink":
        q, k, ka = 4 * u + m / 2, -9 / 16 * u + n / 8, -3 / 8 * u + n / 8
    else:
        q, k, ka = 16 * u + m / 2, -u + n / 64, -61 / 64 * u + n / 64
    v = 1 + torch.randn((nkv, heads, 128), generator=g) / 4
    anchors = _anchors(nkv)
    for pos, shift in anchors:
        k[pos] = ka[pos]
        v[pos] += shift
    q16, k16, v16 = (t.reshape(1, -1, heads * 128).to(BF16) for t in (q, k, v))
    assert torch.equal(q16.float().view_as(q), q) and torch.equal(k16.float().view_as(k), k), "q and k are bf16 numbers"
    return Case(q16, k16, v16, tuple(pos for pos, _ in anchors))


@functools.lru_cache(maxsize=None)
def _refs(*key):
    """The fp32 oracle on the bf16 operands, and the yardstick: the error of the oracle's own bf16 result against it."""
    c, heads = _case(*key), key[2]
    plain32 = wan_dit.attention(c.q.float(), c.k.float(), c.v.float(), heads)
    ref16 = wan_dit.attention(c.q, c.k, c.v, heads).float()
    return Refs(plain32, (ref16 - plain32).abs().max().item(), bool(torch.isfinite(ref16).all()))


@functools.lru_cache(maxsize=None)
def _ref32(form, *key):
    """The fp32 reference of a form: softmax(scale' q k^T) = softmax((q / fold) k^T / sqrt(d))."""
    if form == "plain":
        return _refs(*key).plain32
    c = _case(*key)
    return wan_dit.attention(c.q.float() / FOLD, c.k.float(), c.v.float(), key[2])


def _allowance(*key):
    return 2 * _refs(*key).err_ref + ATTN_FLOOR


def _verdict(got, form, key, what):
    """None, or why `got` misses the criterion (the loops collect these, so that one run names every Nkv that fails)."""
    got = got.float().cpu()
    if not torch.isfinite(got).all():
        return f"{what}: {(~torch.isfinite(got)).sum().item()} of {got.numel()} elements are not finite"
    err, allow = (got - _ref32(form, *key)).abs().max().item(), _allowance(*key)
    print(f"{what}: err {err:.5f}, allowance {allow:.5f}")
    return None if err <= allow else f"{what}: err {err:.5f} > 2 x {_refs(*key).err_ref:.5f} + {ATTN_FLOOR}"


# ------------------------------------------------------------------------------------------------------------------ CPU self-checks
def _check_construction(key):
    nq, nkv, heads, kind, _ = key
    c, refs = _case(*key), _refs(*key)
    what = f"{kind} ({nq}, {nkv}, {heads})"
    assert refs.finite16, f"{what}: the oracle's bf16 result is not finite"
    assert set(c.anchors) == {0, 64 * (_tiles(nkv) - 1), nkv - 1}, what
    allow = _allowance(*key)
    k32, v32 = c.k.float(), c.v.float()
    zero = torch.zeros((1, 1, heads * 128))
    top = float("-inf")
    for form in _forms(nkv):
        q32 = c.q.float() / (1.0 if form == "plain" else FOLD)
        ref = _ref32(form, *key)
        leak = wan_dit.attention(q32, torch.cat([k32, zero], 1), torch.cat([v32, zero], 1), heads)
        moved = (leak - ref).abs().max().item()
        assert moved >= MARGIN * allow, f"{what}, {form}: a leaked zero key moves the reference by {moved:.4f}, the allowance is {allow:.4f}"
        for a in c.anchors if nkv > 1 else ():
            keep = torch.arange(nkv) != a
            moved = (wan_dit.attention(q32, k32[:, keep], v32[:, keep], heads) - ref).abs().max().item()
            assert moved >= MARGIN * allow, f"{what}, {form}: without the anchor at {a} the reference moves by {moved:.4f}, the allowance is {allow:.4f}"
    for h in range(heads):      # the largest logit: of the plain form (the folded one is 2 % smaller in magnitude; checked with it)
        cols = slice(128 * h, 128 * (h + 1))
        top = max(top, (c.q.float()[0, :, cols] @ k32[0, :, cols].T).max().item() * 128 ** -0.5)
    assert top < LOGIT_BELOW[kind] and top / FOLD < LOGIT_BELOW[kind], f"{what}: largest logit {top:.1f} nats"


ALL_KEYS = _all_keys()


@pytest.mark.parametrize("part", range(8))
def test_construction_shows_a_leak_and_a_drop(part):
    """Every case of every table (an eighth of them per test)."""
    for key in ALL_KEYS[part::8]:
        _check_construction(key)


def test_tables_cover_what_the_docstring_claims():
    res = lambda nkv: nkv % 64      # noqa: E731
    for nt in (1, 2):
        assert {res(n) for n in SHORT_KV if _tiles(n) == nt} == set(range(64)), nt
    per_nt = {nt: [n for n in SHORT_KV if _tiles(n) == nt] for nt in range(3, 17)}
    assert all(len(v) >= 1 for v in per_nt.values()) and len({res(v[0]) for v in per_nt.values()}) == 14
    assert all(res(v[0]) == 17 * nt % 64 != 0 for nt, v in per_nt.items())
    assert {1023, 1024} <= set(SHORT_KV) and max(SHORT_KV) == 1024 and min(W4_KV) == W4_MIN
    assert {nt & 1 for nt in map(_tiles, SHORT_KV)} == {0, 1}      # direct workgroups of the template: both parities of the range length
    assert {res(n) for n in W4_KV if _tiles(n) == 17} == set(range(64))
    for nt in (18, 19, 20):
        assert {res(n) for n in W4_KV if _tiles(n) == nt} == {0, 1, 31, 32, 33, 63}, nt
    for ragged in (False, True):      # every tail copy of the 4-wave body ((t - t_begin) & 3 of the last steps), whole and ragged last tile
        assert {_tiles(n) & 3 for n in W4_KV if (res(n) != 0) == ragged} == {0, 1, 2, 3}
    assert {2049, 2112} <= set(W4_KV)
    assert sorted(n for g in SHORT_GROUPS for n in g) == sorted(SHORT_KV) and sorted(n for g in W4_GROUPS for n in g) == sorted(W4_KV)
    assert SHORT_SPLIT_KV == [976, 1023, 1024]
    counts = [heads * blocks for heads, blocks in REMAP]
    assert counts == list(range(1, 10)) + [16] and {c & 7 for c in counts} == set(range(8)) and {h for h, _ in REMAP} == {1, 2, 3}
    assert all(nq * nkv * heads <= 700 * 2763 * 24 for nq, nkv, heads, _, _ in ALL_KEYS)
    # Nq: whole waves without a valid row on both kernels (32 rows a wave on the template, 64 on the 4-wave kernel), every Nq mod 256 edge
    assert {nq % 256 for nq in NQ_SWEEP} >= {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255}
    for nq, nkv, heads in GATHER_EDGES:
        assert _gather_case(nq, nkv, heads).gap_nats >= MIN_GAP_NATS


# ------------------------------------------------------------------------------------------------------------------ GPU
def _nan_out(b, nq, heads):
    return torch.full((b, nq, heads * 128), float("nan"), dtype=BF16, device="cuda")


def _run(hip, key, form, ws, out=None):
    c, (nq, _, heads) = _case(*key), key[:3]
    return _attn(hip, dev(c.q), dev(c.k), dev(c.v), heads, _nan_out(1, nq, heads) if out is None else out, None if form == "plain" else POW2_SCALE, ws)


def _pieces(nkv, S):
    nt = _tiles(nkv)
    return [(sp + 1) * nt // S - sp * nt // S for sp in range(S)]


@gpu
@pytest.mark.parametrize("kind", ["sink", "deep"])
@pytest.mark.parametrize("sweep", KV_SWEEP, ids=_sweep_id)
def test_kv_sweep_direct(hip, sweep, kind):
    """Section 2 of the docstring: one direct workgroup over the whole KV range, no workspace."""
    kernel, form, nkvs = sweep
    failed = []
    for nkv in nkvs:
        assert (nkv >= W4_MIN) == (kernel == "w4") and _split_choice(hip, 1, NQ, nkv, 1, ws=False)[:2] == (0, 1)
        key = (NQ, nkv, 1, kind, 0)
        failed.append(_verdict(_run(hip, key, form, ws=False), form, key, f"{kernel} {form} {kind} direct, Nkv = {nkv}"))
    failed = [f for f in failed if f]
    assert not failed, f"{len(failed)} of {len(nkvs)} KV lengths fail:\n" + "\n".join(failed)


def _split_and_direct(hip, key, form, failed):
    nq, nkv, heads = key[:3]
    R, S, _ = _split_choice(hip, 1, nq, nkv, heads)
    what = f"{form} {key[3]} ({nq}, {nkv}, {heads}), (R, S) = ({R}, {S})"
    assert R > 0 and S > 1, f"{what}: meant to run pieces + attn_combine_kernel"
    got = _run(hip, key, form, ws=True)
    failed.append(_verdict(got, form, key, what))
    direct = _run(hip, key, form, ws=False)
    failed.append(_verdict(direct, form, key, what + " without a workspace"))
    if torch.isfinite(got.float()).all() and torch.isfinite(direct.float()).all():
        # The two against each other: both are bf16 roundings of fp32 results, and two fp32 values that agree to the allowance may round
        # to neighbouring bf16 numbers, so the bound is the allowance plus one bf16 ulp of the element (2^-8 relative at the least).
        # Measured with the allowance alone: (700, 2700, 24) sink lies 0.03125 apart, one ulp of an element in [4, 8), allowance 0.02937.
        d = direct.float()
        ulp = torch.exp2(torch.floor(torch.log2(d.abs().clamp_min(2.0 ** -100))) - 7)
        over = ((got.float() - d).abs() - ulp).max().item()
        if over > _allowance(*key):
            failed.append(f"{what}: split and direct results lie {over:.5f} + 1 ulp apart, allowance {_allowance(*key):.5f}")


@gpu
@pytest.mark.parametrize("kind", ["sink", "deep"])
@pytest.mark.parametrize("sweep", KV_SWEEP_SPLIT, ids=_sweep_id)
def test_kv_sweep_split(hip, sweep, kind):
    """Section 3: the same shapes cut into KV ranges (each piece starts its own running maximum; the last one ends in the ragged tile)."""
    kernel, form, nkvs = sweep
    failed = []
    for nkv in nkvs:
        assert (nkv >= W4_MIN) == (kernel == "w4")
        _split_and_direct(hip, (NQ, nkv, 1, kind, 0), form, failed)
    failed = [f for f in failed if f]
    assert not failed, f"{len(failed)} checks of {len(nkvs)} KV lengths fail:\n" + "\n".join(failed)


@gpu
@pytest.mark.parametrize("kind", ["sink", "deep"])
@pytest.mark.parametrize("nq,nkv,heads", SPLIT_SHAPES)
def test_split_shapes(hip, nq, nkv, heads, kind):
    """Section 3, the fixed shapes: R = 2 with a one-row q-block; 24 heads on both kernels, all q-blocks cut."""
    failed = []
    for form in _forms(nkv):
        _split_and_direct(hip, (nq, nkv, heads, kind, 0), form, failed)
    failed = [f for f in failed if f]
    assert not failed, "\n".join(failed)


@gpu
def test_split_table_covers_every_piece_length(hip):
    """The KV ranges the split cases above run, from the (R, S) the library reports (nothing predicted on the host): among the pieces of
    the 4-wave kernel every length mod 4 (the tail copy its last steps run in) both for the last piece of a range list — the one that may
    end in the ragged tile — and for the others.  The template's pieces: choose_split cuts only where S * 8 <= nt, and the template runs
    nt <= 16, so its pieces are 8 + 8 tiles whatever the shape: both ring parities run in every piece (the fast loop runs pairs of steps
    and the tail has two steps), an odd range length does not occur in a piece; odd lengths run as direct workgroups (nt = 3..15)."""
    last, others, short = set(), set(), set()
    shapes = [(NQ, nkv, 1) for nkv in SHORT_SPLIT_KV + W4_KV] + SPLIT_SHAPES
    for nq, nkv, heads in shapes:
        R, S, _ = _split_choice(hip, 1, nq, nkv, heads)
        assert R > 0 and S > 1, (nq, nkv, heads, R, S)
        lengths = _pieces(nkv, S)
        print(f"({nq}, {nkv}, {heads}): (R, S) = ({R}, {S}), nt = {_tiles(nkv)}, pieces of {lengths} tiles")
        assert sum(lengths) == _tiles(nkv) and min(lengths) >= 8
        if nkv >= W4_MIN:
            last.add(lengths[-1] % 4)
            others |= {n % 4 for n in lengths[:-1]}
        else:
            short |= set(lengths)
    assert last == {0, 1, 2, 3} and others == {0, 1, 2, 3}, (last, others)
    assert short == {8}, short


@gpu
@pytest.mark.parametrize("nkv,form", [(nkv, form) for nkv in NQ_SWEEP_KV for form in _forms(nkv)])
def test_nq_sweep(hip, nkv, form):
    """Section 4: rows >= Nq are clamped to Nq - 1 (template) or read as zeros (4-wave kernel) and must not be stored; rows < Nq must be."""
    failed = []
    for nq in NQ_SWEEP:
        key = (nq, nkv, 1, "sink", 0)
        for ws in (False, True) if nkv >= W4_MIN else (False,):
            g = Guards()
            out = g.embed(torch.full((1, nq, 128), float("nan"), dtype=BF16), 16, 256)
            got = _run(hip, key, form, ws, out)
            g.check(f"Nq = {nq}, Nkv = {nkv}, {form}, workspace {ws}")
            failed.append(_verdict(got, form, key, f"Nq = {nq}, Nkv = {nkv}, {form}, workspace {ws}"))
    failed = [f for f in failed if f]
    assert not failed, "\n".join(failed)


@gpu
@pytest.mark.parametrize("nkv,form", [(nkv, form) for nkv in NQ_SWEEP_KV for form in _forms(nkv)])
def test_remap_sweep(hip, nkv, form):
    """Section 4: the XCD remap of the direct workgroups at every total_direct & 7 (a (head, q-block) nobody computes stays NaN)."""
    failed = []
    for heads, blocks in REMAP:
        key = (_remap_nq(blocks), nkv, heads, "sink", 0)
        assert _split_choice(hip, 1, key[0], nkv, heads, ws=False)[:2] == (0, 1)
        failed.append(_verdict(_run(hip, key, form, ws=False), form, key, f"{heads} heads x {blocks} q-blocks, Nkv = {nkv}, {form}"))
    failed = [f for f in failed if f]
    assert not failed, "\n".join(failed)


@gpu
@pytest.mark.parametrize("nkv,form", [(nkv, form) for nkv in NQ_SWEEP_KV for form in _forms(nkv)])
def test_batch_of_two(hip, nkv, form):
    """Section 4: B = 2, two heads, element 1 from another seed; q, k and v are column slices of ONE (2 Nkv, 3 C) buffer (q in the first
    2 Nq rows of its columns, the rest NaN), so what follows element 0 of every operand is element 1 and the row pitch is 3 C."""
    heads, c = 2, 256
    keys = [(NQ, nkv, heads, "sink", seed) for seed in (0, 1)]
    cases = [_case(*key) for key in keys]
    buf = torch.full((2 * nkv, 3 * c), float("nan"), dtype=BF16)
    buf[:2 * NQ, :c] = torch.cat([x.q[0] for x in cases])
    buf[:, c:2 * c] = torch.cat([x.k[0] for x in cases])
    buf[:, 2 * c:] = torch.cat([x.v[0] for x in cases])
    scale = None if form == "plain" else POW2_SCALE
    for ws in (False, True):
        g = Guards()
        d = g.embed(buf, 16, 64)
        q, k, v = d[:2 * NQ, :c].unflatten(0, (2, NQ)), d[:, c:2 * c].unflatten(0, (2, nkv)), d[:, 2 * c:].unflatten(0, (2, nkv))
        got = _attn(hip, q, k, v, heads, g.embed(torch.full((2, NQ, c), float("nan"), dtype=BF16), 16, 256), scale, ws)
        g.check(f"B = 2, Nkv = {nkv}, {form}, workspace {ws}")
        failed = [_verdict(got[b:b + 1], form, keys[b], f"B = 2, element {b}, Nkv = {nkv}, {form}, workspace {ws}") for b in range(2)]
        assert not any(failed), failed
        if not ws:      # direct workgroups: the bits of the B = 1 call on compact operands
            for b in range(2):
                assert torch.equal(got[b:b + 1], _run(hip, keys[b], form, ws=False)), f"element {b} differs from the B = 1 call"


@gpu
@pytest.mark.parametrize("form", ["plain", "pow2"])
@pytest.mark.parametrize("nq,nkv,heads", GATHER_EDGES)
def test_gather_edges(hip, nq, nkv, heads, form):
    """Section 4: every query row reaches its own key (bit for bit) one row and one key past a q-block, a tile and the 4-wave threshold."""
    for ws in (False, True):
        _gather_on_gpu(hip, nq, nkv, heads, form=form, ws=ws)

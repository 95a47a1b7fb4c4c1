"""The MFMA kernels on inputs whose correct result is exact: the tolerance becomes torch.equal.

The older tests of the GEMMs, attention and the convolutions hold `err <= 2 * err_ref + floor` on N(0, 1) data, which leaves room for
one wrong term: one key of a flat softmax row moves the output by |v| / Nkv ~ 5e-4 < ATTN_FLOOR, one product of the K = 14 336 GEMM
by 0.01 < its allowance of 0.017.  Here the operands are built so that every correct implementation gives the same bits whatever its
summation order, k-split, split-KV merge or deferred rescale, and the expectation is an index or integer computation:

1. Attention as a gather.  Key rows are random +-1 vectors of length 128, query row i is 16 * k[sel(i, head)], V entries are
   round(16 * randn) / 16 clamped to +-63/16.  The logit of a selected key is 16 * 128 * scale = 181 nats (177 with the power-of-two
   scale); every other key lies >= 80 nats below (asserted per shape; measured 91 to 152), so its weight is below 2^-115 and vanishes
   against a result that is a multiple of 2^-6.  The first 8 key slots of every 64 are duplicated half a sequence away (another tile
   and, on the split paths, another KV range) and one group of four equal key rows contains the last key: the expected output is
   the mean of the 1, 2 or 4 V rows whose key row equals the selected one — itself a bf16 number, no softmax in the reference.
2. GEMMs on small integers.  A in {0, +-1} with min(K, 256) non-zeros per row at positions drawn per row, W in {+-1}, bias in
   [-8, 8], gate tables in [-2, 2], residual in [-64, 64]: every partial sum in any order, the workspace round trip and the reduce
   kernel are exact in fp32, and with max |expected| <= 256 (asserted, a condition and not a measurement) every expected value is a
   bf16 number and a change of +-1 in any accumulator is visible.  The e4m3 GEMM takes the same integers with scale_a rows in
   {1, 2, 4}; a row of scale s carries 256 / s^2 non-zeros, so that s * acc has the spread of an unscaled row and the same
   <= 256 condition holds (with 256 non-zeros in every row 4 * acc reaches ~360 and the condition cannot be met).
3. Convolutions: inputs in {0, +-1} at a density of ~200 active terms per output, weights +-1, bias and residual as above;
   expectation from the oracle's convolution in fp64.
4. Hot-LoRA kernels: x with 32 non-zeros per row, alpha * A in {+-2}, B with two +-1 per row (apply); A, B dense +-1 and alpha = 2
   (fuse): the intermediates the header names (bf16(x A^T), bf16(. B^T); bf16(B A), bf16(alpha .), the sum) are integers <= 256.

Paths covered per entry point, and how each was confirmed:
  fg_attn_fwd_bf16   short-KV kernel (Nkv <= 1024) direct and split + combine; Nkv = 1024 / 1025 (last of the short-KV kernel, first of
                     the 4-wave kernel); the 4-wave kernel in both bodies (1 / sqrt(d) and hip.pow2_softmax_scale), direct (no
                     workspace), with the default workspace and on the split-KV path; B = 2; q | k | v slices of one buffer.
                     Confirmed by fg_attn_split_choice (asserted where the issue of a case is its path, printed otherwise); the
                     kernel by the Nkv threshold of the dispatch (csrc/attention.hip) and the scale.
  fg_gemm_epilogue_bf16(_s), fg_gemm_fp8_bf16(_s)   through hip.gemm_epilogue / hip.gemm_fp8 on the shapes of test_gemm_epilogue,
                     test_gemm_epilogue_ksplit and test_gemm_fp8 (the unit plan decides the path: 64-column pieces, whole tiles, cut
                     tails, k-range pieces + gemm_reduce_kernel), modes 0, 2, 3, 4, lda > K.  That the K >= 6 144 shapes run k-range
                     pieces is held by test_gemm_epilogue_ksplit on the same shapes (k-split output differs from workspace=False on
                     non-integer data); here both must equal the integers.
  fg_conv3d_cl_bf16  128 tile, compiler-scheduled 256 tile, hand-scheduled 256 tile, upsample2x, downsample2x, time_interleave,
                     residual.  Confirmed by fg_conv_tile_choice and the launcher's Cin % 64 / Cout % 256 rule, as test_buffer_contract.
  fg_lora_apply_bf16, fg_lora_fuse_bf16   ranks 16 (padded to 32) and 128; modes add and gate (two gate rows); the e4m3 copy.

Cost: the unmarked self-checks (the host suite's share: operands, fp32 / fp64 references, gap checks, both oracles) take 6 s of pytest
time on a 16-thread host; the GPU cases, CPU references included, 8 s of pytest time on an MI355X (test_buffer_contract.py: 4 s,
test_hip_kernels.py: 15 s), the slowest being the GEMM shapes at under 1 s each.
"""
import functools
from collections import namedtuple

import pytest
import torch

from oracle import wan_dit
from test_buffer_contract import _attn, _conv_ref, _split_choice
from test_hip_kernels import _cl, _ncthw, assert_gelu_of, dev, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
BOUND = 256          # |value| <= 2^8: every integer is a bf16 number
MIN_GAP_NATS = 80.0


def _ints(shape, lo, hi, g, device="cpu"):
    """Uniform integers in [lo, hi] as bf16."""
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).to(BF16)


def _signs(shape, g, device="cpu"):
    return (torch.randint(0, 2, shape, generator=g, device=device, dtype=torch.int8) * 2 - 1).to(BF16)


def _sparse_signs(rows, cols, nnz, g, device="cpu"):
    """(rows, cols) in {0, +-1} with exactly nnz non-zeros per row (a number or one per row) at positions drawn per row."""
    s = _signs((rows, cols), g, device)
    per_row = torch.as_tensor(nnz, device=device).expand(rows).clamp(max=cols)
    top = int(per_row.max().item())
    if top >= cols and int(per_row.min().item()) >= cols:
        return s
    r = torch.rand((rows, cols), generator=g, device=device)
    kth = r.topk(top, dim=1).values.gather(1, (per_row - 1).view(-1, 1))      # the nnz-th largest draw of the row
    return s * (r >= kth).to(BF16)


def _exact_int(t, what, bound=BOUND):
    """The condition the module rests on: integer values of magnitude <= bound (so bf16 holds them)."""
    t = t.double()
    assert torch.equal(t, t.round()) and t.abs().max().item() <= bound, f"{what}: max |value| {t.abs().max().item()} (integers <= {bound} required)"
    return t.to(torch.float32).to(BF16)


def _assert_same(got, want, what, describe=None):
    """torch.equal, and on a failure the places that differ."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got.float() != want.float()).nonzero()
    lines = [f"  {tuple(i.tolist())}: got {got[tuple(i)].item()}, want {want[tuple(i)].item()}" + (describe(i) if describe else "") for i in bad[:24]]
    raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} elements differ (first at {bad[0].tolist()}, last at {bad[-1].tolist()})\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------------ 1. attention as a gather
Gather = namedtuple("Gather", "q k v want sel members count gap_nats")


def _key_groups(nkv):
    """members (Nkv, 4) and count (Nkv,): the positions whose key row equals that of position j (padded with -1)."""
    half, last = nkv // 2, nkv - 1
    src = list(range(nkv))
    sources = [p for p in range(half) if p % 64 < 8]          # targets p + half lie in [half, 2 * half): no chains
    for p in sources:
        src[p + half] = p
    taken = set(sources) | {p + half for p in sources}
    free = [j for j in range(last) if j not in taken]
    group = [last] if last not in taken else [src[last] if src[last] != last else last - half, last]
    need = 4 - len(group)
    if len(free) >= need + 1:
        group += [free[(i + 1) * len(free) // (need + 1)] for i in range(need)]
        assert len(set(group)) == 4
        for m in group:
            src[m] = min(group)
    else:
        assert nkv < 64, "every sequence of a tile or more has a group of four that includes the last key"
    members = torch.full((nkv, 4), -1, dtype=torch.long)
    count = torch.zeros(nkv, dtype=torch.long)
    for j, c in enumerate(src):
        members[c, count[c]] = j
        count[c] += 1
    src = torch.tensor(src)
    return src, members[src], count[src]


@functools.lru_cache(maxsize=None)
def _gather_case(nq, nkv, heads, batch=1):
    g = torch.Generator("cpu").manual_seed(9000 + nq + 3 * nkv + 7 * heads + 11 * batch)
    src, members, count = _key_groups(nkv)
    base = _signs((batch, nkv, heads, 128), g)
    k = base[:, src]
    v = (torch.randn((batch, nkv, heads, 128), generator=g) * 16).round().clamp(-63, 63).div(16).to(BF16)
    sel = torch.empty((batch, heads, nq), dtype=torch.long)
    for b in range(batch):
        perm = torch.randperm(nkv, generator=g)          # another order per batch element, another window of it per head
        for h in range(heads):
            sel[b, h] = perm[(torch.arange(nq) + h * (nq + 37)) % nkv]
    bi, hi = torch.arange(batch).view(-1, 1, 1), torch.arange(heads).view(1, -1, 1)
    q = (16 * k[bi, sel, hi].float()).to(BF16).permute(0, 2, 1, 3)                       # (B, Nq, H, 128)
    # the expectation: an index computation
    idx = members[sel]                                                                    # (B, H, Nq, 4)
    rows = v.float()[bi.unsqueeze(-1), idx.clamp(min=0), hi.unsqueeze(-1)] * (idx >= 0).unsqueeze(-1)
    want32 = (rows.sum(3) / count[sel].unsqueeze(-1)).permute(0, 2, 1, 3)
    want = want32.to(BF16)
    assert torch.equal(want.float(), want32), "the mean of 1, 2 or 4 V rows is a bf16 number"
    # the gap: q . k = 2048 on the keys of the selected group, and how far below the others lie
    gap = float("inf")
    scale = min(128 ** -0.5, 0.125 / 1.4426950408889634)          # the smaller of the two scales the tests pass
    for b in range(batch):
        for h in range(heads):
            dots = q[b, :, h].float() @ k[b, :, h].float().T
            mine = torch.zeros_like(dots, dtype=torch.bool).scatter_(1, torch.where(idx[b, h] >= 0, idx[b, h], idx[b, h, :, :1]), True)
            assert (dots[mine] == 2048).all() and mine.sum(1).equal(count[sel[b, h]])
            gap = min(gap, (2048 - dots.masked_fill(mine, float("-inf")).max().item()) * scale)
    shape = (batch, -1, heads * 128)
    return Gather(q.reshape(shape), k.reshape(shape), v.reshape(shape), want.reshape(shape), sel, members, count, gap)


def _describe_rows(case, heads):
    def describe(i):
        b, row, h = i[0].item(), i[1].item(), i[2].item() // 128
        key = case.sel[b, h, row].item()
        return f"  (batch {b}, row {row}, head {h}, column {i[2].item() % 128}) selected key {key}, equal key rows at {[m for m in case.members[key].tolist() if m >= 0]}"
    return describe


def _assert_gather(got, case, heads, what):
    got, want = got.cpu(), case.want
    if not torch.equal(got, want):
        b, n, _ = want.shape
        rows = (got.view(b, n, heads, 128).float() != want.view(b, n, heads, 128).float()).any(-1).nonzero()
        print(f"{what}: (batch, row, head) -> selected key of the {rows.shape[0]} rows that differ:")
        for bb, row, h in rows[:200].tolist():
            print(f"  ({bb}, {row}, {h}) -> key {case.sel[bb, h, row].item()} of {[m for m in case.members[case.sel[bb, h, row]].tolist() if m >= 0]}")
    _assert_same(got, want, what, _describe_rows(case, heads))


ATTN_ALL = [(31, 5, 1, 1), (300, 77, 2, 1), (513, 512, 3, 1), (64, 1000, 2, 1), (300, 1000, 24, 1), (300, 1024, 2, 1), (300, 1025, 2, 1),
            (300, 1500, 2, 1), (300, 1500, 2, 2), (1100, 1025, 2, 1), (1560, 1560, 2, 1), (700, 2700, 24, 1)]


@pytest.mark.parametrize("nq,nkv,heads,batch", ATTN_ALL)
def test_gather_construction(nq, nkv, heads, batch):
    """Every shape the GPU cases use: logit gap >= 80 nats, the groups are what the text says, sel covers what it should; at the two
    smallest shapes the oracle's attention in fp32 and in bf16 equals the index expectation bit for bit."""
    c = _gather_case(nq, nkv, heads, batch)
    print(f"gather ({nq}, {nkv}, {heads}) x {batch}: smallest logit gap {c.gap_nats:.1f} nats")
    assert c.gap_nats >= MIN_GAP_NATS
    sizes = set(c.count.tolist())
    assert sizes <= {1, 2, 4} and (nkv < 64 or (sizes == {1, 2, 4} and c.count[nkv - 1] == 4))
    pairs = [j for j in range(nkv // 2) if j % 64 < 8 and c.count[j] == 2]
    assert all(c.members[j].tolist()[:2] == [j, j + nkv // 2] for j in pairs) and (nkv < 16 or pairs)
    for b in range(batch):
        seen = [set(c.sel[b, h].tolist()) for h in range(heads)]
        if nq >= nkv:
            assert all(len(s) == nkv for s in seen), "every key position is selected in every head"
        if heads * nq >= nkv:
            assert len(set().union(*seen)) == nkv
        assert heads == 1 or not torch.equal(c.sel[b, 0], c.sel[b, 1])
    assert batch == 1 or not torch.equal(c.sel[0], c.sel[1])
    if nkv <= 77:
        assert torch.equal(wan_dit.attention(c.q.float(), c.k.float(), c.v.float(), heads), c.want.float()), "fp32 oracle"
        assert torch.equal(wan_dit.attention(c.q, c.k, c.v, heads), c.want), "bf16 oracle"


def _gather_on_gpu(hip, nq, nkv, heads, batch=1, form="plain", ws=True, split=None, fused=False):
    c = _gather_case(nq, nkv, heads, batch)
    assert c.gap_nats >= MIN_GAP_NATS
    scale = None if form == "plain" else hip.pow2_softmax_scale(128)[0]
    R, S, _ = _split_choice(hip, batch, nq, nkv, heads, ws)
    what = f"attention as a gather ({nq}, {nkv}, {heads}) x {batch}, {form}, (R, S) = ({R}, {S})"
    print(what)
    if split is not None:
        assert (R > 0 and S > 1) == split, what
    if fused:
        d = dev(torch.cat([c.q, c.k, c.v], dim=-1))
        hd = heads * 128
        q, k, v = d[..., :hd], d[..., hd:2 * hd], d[..., 2 * hd:]
    else:
        q, k, v = dev(c.q), dev(c.k), dev(c.v)
    got = _attn(hip, q, k, v, heads, torch.empty((batch, nq, heads * 128), dtype=BF16, device="cuda"), scale, ws)
    _assert_gather(got, c, heads, what)


@gpu
@pytest.mark.parametrize("nq,nkv,heads,split", [(31, 5, 1, False), (300, 77, 2, False), (64, 1000, 2, None),      # short-KV kernel
                                                  (513, 512, 3, False),                                            # ... direct: 8 tiles, nothing to cut
                                                  (300, 1000, 24, True),                                           # ... pieces + combine
                                                  (300, 1024, 2, None), (300, 1025, 2, None)])                     # the last Nkv of it, the first of the 4-wave kernel
def test_attention_gather_short_kv(hip, nq, nkv, heads, split):
    _gather_on_gpu(hip, nq, nkv, heads, split=split)


@gpu
@pytest.mark.parametrize("form", ["plain", "pow2"])
@pytest.mark.parametrize("nq,nkv,heads,ws,split", [(300, 1500, 2, False, False),      # every q-block one direct workgroup
                                                     (300, 1500, 2, True, None),
                                                     (1560, 1560, 2, True, None),       # every key selected by some row of every head
                                                     (1100, 1025, 2, True, None),       # one key in the 17th tile, every key selected
                                                     (700, 2700, 24, True, True)])      # every q-block cut into KV ranges + combine
def test_attention_gather_w4(hip, nq, nkv, heads, ws, split, form):
    _gather_on_gpu(hip, nq, nkv, heads, form=form, ws=ws, split=split)


@gpu
def test_attention_gather_batch_and_fused_qkv(hip):
    _gather_on_gpu(hip, 300, 1500, 2, batch=2, form="pow2", split=True)          # B = 2, another sel per batch element; split (test_buffer_contract)
    _gather_on_gpu(hip, 1560, 1560, 2, form="pow2", fused=True)                  # q | k | v of one (N, 3C) buffer


# ------------------------------------------------------------------------------------------------------ 2. GEMMs on small integers
GEMM_BF16 = [(700, 256, 768), (4200, 512, 4096), (10500, 128, 2048), (600, 14336, 3072), (8300, 14336, 512), (66200, 6144, 256)]
GEMM_FP8 = [(700, 3072, 768), (4200, 1024, 4096), (600, 14336, 3072)]


def _gemm_operands(M, K, N, device, fp8=False):
    g = torch.Generator(device).manual_seed(5000 + M + K + N)
    scale = None
    nnz = min(K, 256)
    if fp8:
        scale = 2.0 ** torch.randint(0, 3, (M, 1), generator=g, device=device).float()
        nnz = (256 / scale.view(-1) ** 2).long()
    a = _sparse_signs(M, K, nnz, g, device)
    w, bias = _signs((N, K), g, device), _ints((N,), -8, 8, g, device)
    res, table = _ints((M, N), -64, 64, g, device), _ints((2, 6, N), -2, 2, g, device)
    return a, w, bias, scale, res, table


def _gemm_expected(a, w, bias, scale, res, table, first, rows, dtype=torch.float32):
    """The integers A W^T + b (times scale_a) and the residual forms on `rows`, on the CPU in `dtype`."""
    a, w, bias, res, table = (t.cpu() for t in (a[rows], w, bias, res[rows], table))
    y = a.to(dtype) @ w.to(dtype).T
    y = (y if scale is None else scale[rows].cpu().to(dtype) * y) + bias.to(dtype)
    gate = table[(rows >= first).long(), 5].to(dtype)
    return y, res.to(dtype) + gate * y, res.to(dtype) + y


def _class_change(M):
    """A first_rows inside the last row tile of 256."""
    start = (M - 1) // 256 * 256
    return start + max(1, (M - start) // 2)


@pytest.mark.parametrize("M,K,N,fp8", [(700, 256, 768, False), (300, 512, 256, False), (40, 14336, 256, False), (300, 1024, 256, True)])
def test_integer_gemm_construction(M, K, N, fp8):
    """The construction on the CPU: exactly min(K, 256) non-zeros per row (256 / s^2 in a row of scale s), fp32 == fp64, every value
    an integer within the bound, operands exact in e4m3."""
    a, w, bias, scale, res, table = _gemm_operands(M, K, N, "cpu", fp8)
    nnz = (a != 0).sum(1)
    assert torch.equal(nnz, torch.full((M,), min(K, 256)) if not fp8 else (256 / scale.view(-1) ** 2).long())
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(w.unique().tolist()) == {-1.0, 1.0}
    assert K <= 256 or not torch.equal(a[0] != 0, a[1] != 0), "positions are drawn per row"
    assert not fp8 or (set(scale.unique().tolist()) == {1.0, 2.0, 4.0} and torch.equal(a.to(F8).to(BF16), a) and torch.equal(w.to(F8).to(BF16), w))
    rows, first = torch.arange(M), _class_change(M)
    assert (M - 1) // 256 * 256 < first < M
    for t32, t64 in zip(_gemm_expected(a, w, bias, scale, res, table, first, rows), _gemm_expected(a, w, bias, scale, res, table, first, rows, torch.float64)):
        assert torch.equal(t32.double(), t64)
        _exact_int(t32, "expected value")


def _gemm_rows(M):
    return torch.arange(M) if M < 20000 else torch.cat([torch.arange(0, 300), torch.arange(M // 2, M // 2 + 300), torch.arange(M - 300, M)])


@gpu
@pytest.mark.parametrize("M,K,N", GEMM_BF16)
def test_gemm_integers(hip, M, K, N):
    """fg_gemm_epilogue_bf16_s on integer operands: the result IS the integer A W^T + b (torch.equal), with and without the k-split
    workspace, through the residual epilogues (expected from the independent reference, not from the kernel's own y; the gate class
    changes inside the last row tile), GELU of the exactly known y, and from a strided A (lda > K)."""
    a, w, bias, _, res, table = _gemm_operands(M, K, N, "cuda")
    rows, first = _gemm_rows(M), _class_change(M)
    what = f"gemm {M}x{K}x{N}"
    y16, gated16, plain16 = (_exact_int(t, what) for t in _gemm_expected(a, w, bias, None, res, table, first, rows))
    y = hip.gemm_epilogue(a, w, bias)
    _assert_same(y[rows], y16, what)
    if K >= 6144:
        y_nows = hip.gemm_epilogue(a, w, bias, workspace=False)
        _assert_same(y_nows[rows], y16, what + ", no workspace")
        assert torch.equal(y, y_nows), what + ": k-split and single accumulation differ outside the sampled rows"      # the left-over tiles may lie there
    got = hip.gemm_epilogue(a, w, bias, out=res.clone(), residual=True, mod=hip.ModTable(table, first), gate_idx=5)
    _assert_same(got[rows], gated16, what + ", mode 2")
    got = hip.gemm_epilogue(a, w, bias, out=res.clone(), residual=True)
    _assert_same(got[rows], plain16, what + ", mode 3")
    assert_gelu_of(hip.gemm_epilogue(a, w, bias, act="gelu_tanh")[rows], y16, what + " + gelu")
    if M <= 700:
        wide = torch.full((M, K + 128), float("nan"), dtype=BF16, device="cuda")
        wide[:, 64:64 + K] = a
        _assert_same(hip.gemm_epilogue(wide[:, 64:64 + K], w, bias)[rows], y16, what + ", lda = K + 128")


@gpu
@pytest.mark.parametrize("M,K,N", GEMM_FP8)
def test_gemm_fp8_integers(hip, M, K, N):
    """fg_gemm_fp8_bf16_s on the same integers cast to e4m3 (exact), scale_a rows in {1, 2, 4} passed directly: scale_a * acc + bias."""
    a, w, bias, scale, res, table = _gemm_operands(M, K, N, "cuda", fp8=True)
    rows, first = _gemm_rows(M), _class_change(M)
    what = f"fp8 gemm {M}x{K}x{N}"
    y16, gated16, plain16 = (_exact_int(t, what) for t in _gemm_expected(a, w, bias, scale, res, table, first, rows))
    a8, w8 = a.to(F8), w.to(F8)
    assert torch.equal(a8.to(BF16), a) and torch.equal(w8.to(BF16), w)
    _assert_same(hip.gemm_fp8(a8, scale, w8, bias)[rows], y16, what)
    if K >= 12288:
        _assert_same(hip.gemm_fp8(a8, scale, w8, bias, workspace=False)[rows], y16, what + ", no workspace")
    got = hip.gemm_fp8(a8, scale, w8, bias, out=res.clone(), residual=True, mod=hip.ModTable(table, first), gate_idx=5)
    _assert_same(got[rows], gated16, what + ", mode 2")
    got = hip.gemm_fp8(a8, scale, w8, bias, out=res.clone(), residual=True)
    _assert_same(got[rows], plain16, what + ", mode 3")
    assert_gelu_of(hip.gemm_fp8(a8, scale, w8, bias, act="gelu_tanh")[rows], y16, what + " + gelu")
    wide = torch.zeros((M, K + 128), dtype=torch.uint8, device="cuda").fill_(0x7F).view(F8)          # 0x7F: NaN in e4m3fn
    wide[:, 64:64 + K] = a8
    _assert_same(hip.gemm_fp8(wide[:, 64:64 + K], scale, w8, bias)[rows], y16, what + ", lda = K + 128")


# ------------------------------------------------------------------------------------------------------ 3. convolutions
CONV_CASES = [      # name, tile, hand-scheduled, Cin, Cout, kt, ks, T, H, W (output), history frames, resample, interleave, residual
    ("48-64-3x3x3", 128, False, 48, 64, 3, 3, 1, 6, 10, False, 0, False, False),                  # the rows of test_conv3d_cl
    ("64-128-3x3x3-prev", 128, False, 64, 128, 3, 3, 2, 9, 7, True, 0, False, False),
    ("128-256-3x1x1-prev", 128, True, 128, 256, 3, 1, 1, 5, 6, True, 0, False, False),
    ("96-48-1x1x1", 128, False, 96, 48, 1, 1, 3, 4, 4, False, 0, False, False),
    ("256-12-3x3x3-prev", 128, False, 256, 12, 3, 3, 4, 8, 8, True, 0, False, False),
    ("1024-1024-3x3x3-prev", 128, True, 1024, 1024, 3, 3, 1, 4, 6, True, 0, False, False),
    ("w4-64-512-3x3x3-prev-res", 256, True, 64, 512, 3, 3, 8, 33, 31, True, 0, False, True),    # 8 184 pixels = 31 tiles + 248: 64 workgroups
    ("256p-96-512-1x3x3", 256, False, 96, 512, 1, 3, 8, 33, 31, False, 0, False, False),         # Cin % 64 != 0: the compiler-scheduled 256 tile
    ("upsample2x-res", 128, False, 64, 64, 1, 3, 2, 10, 12, False, 1, False, True),              # test_conv_upsample_interleave_residual
    ("interleave-res", 128, False, 64, 128, 3, 1, 2, 5, 6, True, 0, True, True),
    ("downsample2x", 128, False, 64, 64, 1, 3, 2, 5, 6, False, 2, False, False),                 # test_encoder_kernels
]
CONV_CPU = [c for c in CONV_CASES if c[1] == 128]


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    _, _, _, cin, cout, kt, ks, T, H, W, history, resample, interleave, residual = next(c for c in CONV_CASES if c[0] == name)
    g = torch.Generator("cpu").manual_seed(6000 + cin + cout + 3 * kt + 5 * ks + resample)
    hin, win = (H // 2, W // 2) if resample == 1 else ((2 * H, 2 * W) if resample == 2 else (H, W))
    density = min(1.0, 200.0 / (cin * kt * ks * ks))

    def sparse(shape):
        return _signs(shape, g) * (torch.rand(shape, generator=g) < density).to(BF16)
    x = sparse((1, cin, T, hin, win))
    prev = sparse((1, cin, 2, hin, win)) if history else None
    w, b = _signs((cout, cin, kt, ks, ks), g), _ints((cout,), -8, 8, g)
    cout2 = cout // 2 if interleave else cout
    res = _ints((1, cout2, 2 * T if interleave else T, H, W), -64, 64, g) if residual else None
    ref64 = _conv_ref(x, w, b, prev, res, kt, ks, resample, interleave, torch.float64)
    return x, prev, w, b, res, _exact_int(ref64, f"conv {name}")


@pytest.mark.parametrize("name", [c[0] for c in CONV_CPU])
def test_integer_conv_construction(name):
    """The fp64 expectation is an integer tensor within the bound, and the oracle's bf16 convolution gives the same bits."""
    _, _, _, cin, cout, kt, ks, T, H, W, history, resample, interleave, residual = next(c for c in CONV_CASES if c[0] == name)
    x, prev, w, b, res, want = _conv_case(name)
    assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(w.unique().tolist()) == {-1.0, 1.0}
    active = (x != 0).float().mean().item() * cin * kt * ks * ks
    assert active <= 260 and (cin * kt * ks * ks < 200 or active >= 140), active
    assert want.abs().max().item() > 16, "the outputs are not trivially small"
    assert torch.equal(_conv_ref(x, w, b, prev, res, kt, ks, resample, interleave, BF16), want), "bf16 oracle"


@gpu
@pytest.mark.parametrize("name,tile,w4,cin,cout,kt,ks,T,H,W,history,resample,interleave,residual", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3d_integers(hip, name, tile, w4, cin, cout, kt, ks, T, H, W, history, resample, interleave, residual):
    """fg_conv3d_cl_bf16 on its three kernels and in its resample / interleave / residual forms: torch.equal to the fp64 convolution."""
    lib = hip.load()
    cout2 = cout // 2 if interleave else cout
    assert lib.fg_conv_tile_choice(T, H, W, cout) == tile and (cin % 64 == 0 and cout2 % 256 == 0) == w4, name
    x, prev, w, b, res, want = _conv_case(name)
    xin = x if kt == 1 else torch.cat([prev if prev is not None else x.new_zeros(x.shape[:2] + (2,) + x.shape[3:]), x], dim=2)
    got = hip.conv3d_cl(dev(_cl(xin)), hip.conv_pack_weight(dev(w)), dev(b), cout, kt, ks, residual=None if res is None else dev(_cl(res)),
                        upsample2x=resample == 1, downsample2x=resample == 2, time_interleave=interleave)
    _assert_same(_ncthw(got.cpu()), want, f"conv {name}  [index: (1, channel, frame, y, x)]")


# ------------------------------------------------------------------------------------------------------ 4. hot-LoRA kernels
LORA_APPLY = [(333, 3072, 3072, 16, "add"), (333, 3072, 3072, 128, "add"), (333, 3072, 3072, 16, "gate"), (333, 3072, 3072, 128, "gate")]
LORA_FUSE = [(192, 320, 16, 2.0), (192, 320, 128, 2.0), (192, 320, 128, 0.5)]


@functools.lru_cache(maxsize=None)
def _lora_apply_case(m, k, n, rank, mode):
    """x: 32 non-zeros +-1 per row; alpha * A = +-2 (alpha = 2 folded in, as the product stacks it); B: two +-1 per row; out0 and the
    gate as the GEMM cases.  Reference: plain torch with a rounding at each point the header names."""
    g = torch.Generator("cpu").manual_seed(7000 + m + rank)
    x, a, b = _sparse_signs(m, k, 32, g), 2 * _signs((rank, k), g), _sparse_signs(n, rank, 2, g)
    out0, table, first = _ints((m, n), -64, 64, g), _ints((2, 6, n), -2, 2, g), 77          # first_rows inside the second row tile
    t = _exact_int(x.float() @ a.float().T, "bf16(x A^T)")
    low = _exact_int(t.float() @ b.float().T, "bf16(t B^T)")
    gate = table[(torch.arange(m) >= first).long(), 2]
    add = _exact_int(gate.float() * low.float(), "bf16(gate * l)") if mode == "gate" else low
    want = _exact_int(out0.float() + add.float(), "out")
    assert low.abs().max().item() > 16 and not torch.equal(want, out0)
    return x, a, b, out0, table, first, want, (t, low)


@pytest.mark.parametrize("m,k,n,rank,mode", LORA_APPLY)
def test_integer_lora_apply_construction(m, k, n, rank, mode):
    x, a, b, out0, table, first, want, (t, low) = _lora_apply_case(m, k, n, rank, mode)
    t64 = x.double() @ a.double().T
    assert torch.equal(t.double(), t64) and torch.equal(low.double(), t64 @ b.double().T), "fp32 == fp64 at both rounding points"
    assert torch.equal((b != 0).sum(1), torch.full((n,), 2)) and torch.equal((x != 0).sum(1), torch.full((m,), 32))


@gpu
@pytest.mark.parametrize("m,k,n,rank,mode", LORA_APPLY)
def test_lora_apply_integers(hip, m, k, n, rank, mode):
    from fairygen_amd.wan_video_dit import stack_hot_loras
    x, a, b, out0, table, first, want, _ = _lora_apply_case(m, k, n, rank, mode)
    a_st, b_st = stack_hot_loras([[(a, b)]], [(k, n)], torch.device("cuda"), BF16)
    assert a_st.shape == (max(32, rank), k) and b_st.shape == (n, max(32, rank))
    out = dev(out0).clone()
    hip.lora_apply(dev(x), a_st, b_st, out, mode=mode, mod=hip.ModTable(dev(table), first) if mode == "gate" else None, gate_idx=2)
    _assert_same(out, want, f"lora_apply rank {rank} {mode}")


@functools.lru_cache(maxsize=None)
def _lora_fuse_case(n, k, rank, alpha):
    g = torch.Generator("cpu").manual_seed(8000 + rank)
    a, b, w = _signs((rank, k), g), _signs((n, rank), g), _ints((n, k), -64, 64, g)
    if alpha < 1:
        b = 2 * b          # alpha * d stays an integer
    d = _exact_int(b.float() @ a.float(), "bf16(B A)")
    d = _exact_int(alpha * d.float(), "bf16(alpha * d)")
    want = _exact_int(w.float() + d.float(), "w'")
    assert torch.equal(d.double(), alpha * (b.double() @ a.double())) and d.abs().max().item() > 8
    return w, a, b, want


@pytest.mark.parametrize("n,k,rank,alpha", LORA_FUSE)
def test_integer_lora_fuse_construction(n, k, rank, alpha):
    """The integers equal what the reference's own code (GeneralLoRALoader.fuse_lora_to_base_model on the CPU, in bf16) gives."""
    from test_lora_fuse_kernel import _cpu_reference
    w, a, b, want = _lora_fuse_case(n, k, rank, alpha)
    assert torch.equal(_cpu_reference(w, a, b, alpha), want)


@gpu
@pytest.mark.parametrize("n,k,rank,alpha", LORA_FUSE)
def test_lora_fuse_integers(hip, n, k, rank, alpha):
    from test_lora_fuse_kernel import _padded
    w, a, b, want = _lora_fuse_case(n, k, rank, alpha)
    a_t, b_p = _padded(a, b, max(32, rank))
    out8 = torch.zeros((n, k), dtype=torch.uint8, device="cuda")
    got = hip.lora_fuse(dev(w), a_t, b_p, alpha, out_fp8=out8.view(F8))
    _assert_same(got, want, f"lora_fuse rank {rank} alpha {alpha}")
    _assert_same(out8, want.to(F8).view(torch.uint8), f"lora_fuse rank {rank} alpha {alpha}, e4m3 copy")

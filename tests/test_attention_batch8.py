"""The e4m3 attention chain on batches: the C ABI extension include/fairygen_hip_batch8.h and its binding in fairygen_amd.hip.  (The DiT
forward does not use it yet: a merged CFG call is still evaluated element by element, so there is no model switch and no model test.)

THE CONTRACT, checked with torch.equal everywhere: for every batch element b, the bytes a batched entry point writes for b — operands,
scales, attention output — are those the single-element entry point writes when it is called on element b alone.  The elements of a
test batch differ on purpose (N(0,1); scaled by 37 with a per-channel offset of 3; scaled by 1/64), so a statistic that leaked from one
element into another would change bytes.

Split-KV: the batched self-attention plans every element as the single-element call on a 1/B share of the workspace
(fairygen_hip_batch8.h), so the per-element reference of a call with B * fg_attn_workspace_bytes(1, ..) bytes is the single-element call
with fg_attn_workspace_bytes(1, ..) bytes; SPLIT_SHAPE below is a shape at which that is non-zero on 256 CUs.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from fairygen_amd import hip as _hip

gpu = pytest.mark.gpu
BF16, F8, U8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.float32
NAMES = ("fg_attn_quant_qk_bf16_b", "fg_rmsnorm_rope_q8_bf16_b", "fg_rmsnorm_rope_kstats_bf16_b", "fg_attn_quant_k_bf16_b",
         "fg_attn_quant_vt_bf16_b", "fg_attn_fwd_qk8_bf16_b", "fg_attn_fwd_pv8_bf16_b", "fg_attn_fwd_cross8_bf16_b")
QUERIES = ("fg_attn_batch8_version",)
EPS = 1e-6
# 2 heads, 2 q-blocks of 3 072 keys: 4 workgroups on 256 CUs, every q-block is split over the keys (fg_attn_workspace_bytes(1, ..) > 0,
# asserted where it is used)
SPLIT_SHAPE = (2, 512, 3072)


# ------------------------------------------------------------------------------------------------------------------ CPU: ABI and argument checks
def test_extension_abi():
    lib = _hip.load()
    main = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    ext = open(os.path.join(REPO, "include", "fairygen_hip_batch8.h")).read()
    # the main table and the earlier extensions are what they were
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55
    assert len(_hip.PV8_SYMBOLS) == 4 and len(_hip.SHARD8_SYMBOLS) == 6 and len(_hip.CROSS8_SYMBOLS) == 3
    assert (_hip.QK8_ABI_VERSION, _hip.QK8F_ABI_VERSION, _hip.PV8_ABI_VERSION, _hip.SHARD8_ABI_VERSION, _hip.CROSS8_ABI_VERSION) == (1,) * 5
    others = _hip.EXPORTED_SYMBOLS + _hip.PV8_SYMBOLS + _hip.SHARD8_SYMBOLS + _hip.CROSS8_SYMBOLS
    assert not any(name in others or name in main for name in NAMES + QUERIES)
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.BATCH8_SYMBOLS == sorted(NAMES + QUERIES)
    assert _hip.BATCH8_ABI_VERSION == 1 and lib.fg_attn_batch8_version() == 1
    assert sorted(_hip._BATCH8_SIGNATURES) == sorted(NAMES) and _hip._BATCH8_QUERIES == {QUERIES[0]: (ctypes.c_int, [])}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has as many arguments as its declaration
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_hip._BATCH8_SIGNATURES[name]) == len(getattr(lib, name).argtypes), name


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1): B = 0, a batch stride smaller than the
    element, misaligned pointers, Nkv above max_kv, a short scratch."""
    lib, a = _hip.load(), 4096
    n, h, hd = 100, 2, 256
    err = lambda: lib.fg_last_error()      # noqa: E731
    # fg_attn_quant_qk_bf16_b(q, ldq, bs_q, k, ldk, bs_k, q8, bs_q8, k8, bs_k8, sq, bs_sq, sk, bs_sk, scratch, bytes, bs_scratch, B, N, H, D)
    def qk(B=2, bs_q=n * 768, bs_q8=n * hd, bs_sk=h, scr=hd * 4, bs_scr=hd * 4, q=a, sq=a):
        return lib.fg_attn_quant_qk_bf16_b(q, 768, bs_q, a, 768, n * 768, a, bs_q8, a, n * hd, sq, n * h, a, bs_sk, a, scr, bs_scr, B, n, h, 128, None)
    assert qk(B=0) == -1 and b"B must be in 1..65535" in err()
    assert qk(B=65536) == -1 and b"B must be" in err()
    assert qk(bs_q=(n - 1) * 768 + hd - 8) == -1 and b"batch stride" in err()
    assert qk(bs_q8=n * hd - 8) == -1 and b"batch stride" in err()
    assert qk(bs_sk=h - 1) == -1 and b"batch stride" in err()
    assert qk(scr=hd * 4 - 1) == -1 and b"scratch" in err()
    assert qk(bs_scr=hd * 4 + 8) == -1 and b"alignment" in err()
    assert qk(q=a + 8) == -1 and b"aligned" in err()
    assert qk(sq=a + 2) == -1 and b"aligned" in err()
    # fg_rmsnorm_rope_q8_bf16_b / fg_rmsnorm_rope_kstats_bf16_b
    assert lib.fg_rmsnorm_rope_q8_bf16_b(a, 768, a, None, None, 0, a, a, 0, n, hd, h, EPS, None) == -1 and b"B must be" in err()
    assert lib.fg_rmsnorm_rope_q8_bf16_b(a + 8, 768, a, None, None, 0, a, a, 2, n, hd, h, EPS, None) == -1 and b"aligned" in err()
    need = lib.fg_attn_qk8_fused_scratch_bytes(n, hd)
    ks = lambda B=2, pb=need, bs=need, x=a: lib.fg_rmsnorm_rope_kstats_bf16_b(x, 768, a, None, None, 0, a, a, pb, bs, B, n, hd, h, EPS, None)      # noqa: E731
    assert ks(B=0) == -1 and b"B must be" in err()
    assert ks(pb=need - 1) == -1 and b"partials must hold" in err()
    assert ks(bs=need - 16) == -1 and b"batch stride" in err()
    assert ks(x=a + 8) == -1 and b"aligned" in err()
    # fg_attn_quant_k_bf16_b(k, ldk, bs_k, partials, bytes, bs_partials, k8, bs_k8, sk, bs_sk, kbar, bs_kbar, B, N, H, D)
    qkk = lambda B=2, bs_k=n * 768, pb=need, bs_kbar=hd, k8=a: lib.fg_attn_quant_k_bf16_b(      # noqa: E731
        a, 768, bs_k, a, pb, need, k8, n * hd, a, h, a, bs_kbar, B, n, h, 128, None)
    assert qkk(B=0) == -1 and b"B must be" in err()
    assert qkk(bs_k=n * 768 - 1024) == -1 and b"batch stride" in err()
    assert qkk(pb=need - 1) == -1 and b"partials must hold" in err()
    assert qkk(bs_kbar=hd - 4) == -1 and b"batch stride" in err()
    assert qkk(k8=a + 4) == -1 and b"aligned" in err()
    # fg_attn_quant_vt_bf16_b(v, ldv, bs_v, v8t, bs_v8t, sv, bs_sv, scratch, bytes, bs_scratch, B, N, H, D)
    vneed, nkp = lib.fg_attn_pv8_scratch_bytes(n, h), 128
    vt = lambda B=2, bs_v8t=hd * nkp, scr=vneed, bs_sv=hd, v=a: lib.fg_attn_quant_vt_bf16_b(      # noqa: E731
        v, 768, n * 768, a, bs_v8t, a, bs_sv, a, scr, vneed, B, n, h, 128, None)
    assert vt(B=0) == -1 and b"B must be" in err()
    assert vt(bs_v8t=hd * nkp - 64) == -1 and b"batch stride" in err()
    assert vt(scr=vneed - 1) == -1 and b"scratch must hold" in err()
    assert vt(bs_sv=hd + 2) == -1 and b"alignment" in err()
    assert vt(v=a + 8) == -1 and b"aligned" in err()
    # the three attention kernels
    def fq(B=2, bs_q8=n * hd, bs_v=n * 768, ws=None, wsb=0, out=a):
        return lib.fg_attn_fwd_qk8_bf16_b(a, bs_q8, a, n * hd, a, n * h, a, h, a, 768, bs_v, out, n * hd, B, n, n, h, 128, 0.1, ws, wsb, None)
    assert fq(B=0) == -1 and b"B must be" in err()
    assert fq(bs_q8=n * hd - 16) == -1 and b"batch stride" in err()
    assert fq(bs_v=(n - 1) * 768) == -1 and b"batch stride" in err()
    assert fq(ws=None, wsb=1024) == -1 and b"bad workspace" in err()
    assert fq(ws=a + 8, wsb=1024) == -1 and b"aligned" in err()
    assert fq(out=a + 8) == -1 and b"aligned" in err()
    def fp(B=2, bs_v8t=hd * nkp, bs_sv=hd, wsb=0, ws=None, nkv=n):
        return lib.fg_attn_fwd_pv8_bf16_b(a, n * hd, a, n * hd, a, n * h, a, h, a, bs_v8t, a, bs_sv, a, n * hd, B, n, nkv, h, 128, 0.1, ws, wsb, None)
    assert fp(B=0) == -1 and b"B must be" in err()
    assert fp(bs_v8t=hd * nkp - 16) == -1 and b"batch stride" in err()
    assert fp(bs_sv=hd - 4) == -1 and b"batch stride" in err()
    assert fp(wsb=-1) == -1 and b"bad workspace" in err()
    max_kv = lib.fg_attn_cross8_max_kv()
    def fc(B=2, nkv=n, bs_k8=n * hd, bs_out=n * hd, sv=a, scale=0.1):
        return lib.fg_attn_fwd_cross8_bf16_b(a, n * hd, a, bs_k8, a, n * h, a, h, a, hd * 704, sv, hd, a, bs_out, B, n, nkv, h, 128, scale, None)
    assert fc(B=0) == -1 and b"B must be" in err()
    assert fc(nkv=max_kv + 1, bs_k8=(max_kv + 1) * hd) == -1 and b"Nkv must be in 1..640" in err()
    assert fc(bs_k8=n * hd - 16) == -1 and b"batch stride" in err()
    assert fc(bs_out=n * hd + 4) == -1 and b"alignment" in err()
    assert fc(sv=a + 8) == -1 and b"aligned" in err()
    assert fc(scale=0.0) == -1 and b"scale" in err()


# ------------------------------------------------------------------------------------------------------------------ GPU: inputs
def make_qkv(b, n, h, seed, contiguous=False):
    """(q, k, v), each (B, N, H*128) bf16: column slices of one (B, N, 3C) buffer (ld = 3C, batch stride N * 3C), or contiguous.  Element
    0 is N(0,1), element 1 is scaled by 37 and offset by 3 per channel, element 2 is scaled by 1/64."""
    c = h * 128
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, n, 3 * c), generator=g, dtype=F32)
    if b > 1:
        x[1] = x[1] * 37.0 + 3.0 * torch.linspace(-1.0, 1.0, 3 * c)
    if b > 2:
        x[2] = x[2] / 64.0
    x = x.to(BF16).cuda()
    q, k, v = x[..., :c], x[..., c:2 * c], x[..., 2 * c:]
    return tuple(t.contiguous() for t in (q, k, v)) if contiguous else (q, k, v)


def rope_table(n, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand((n, 64), generator=g, dtype=torch.float64) * 6.283185307179586
    return torch.stack([ang.cos(), ang.sin()], dim=-1).to(F32).contiguous().cuda()      # (rows, head_dim / 2, {cos, sin})


def same(a, b):
    a, b = (t.view(U8) if t.dtype == F8 else t for t in (a, b))
    return a.shape == b.shape and torch.equal(a, b)


def operands(q, k, v, h):
    """The batched operands (q8, k8, sq, sk, v8t, sv) of a (B, ..) batch."""
    q8, k8, sq, sk, _ = _hip.attn_quant_qk(q, k, h)
    v8t, sv, _ = _hip.attn_quant_vt(v, h)
    return q8, k8, sq, sk, v8t, sv


# ------------------------------------------------------------------------------------------------------------------ GPU: producers
@gpu
@pytest.mark.parametrize("n", [1, 15, 64, 65, 200, 1100])
@pytest.mark.parametrize("b,h", [(2, 1), (3, 3), (2, 3), (3, 1)])
def test_producers_match_per_element(b, h, n):
    """The two-step producer, the fused producers and the V producer on a batch against the single-element entry points per element:
    q8, sq, k8, sk, the key mean, bf16 k, v8t (padding included) and sv."""
    q, k, v = make_qkv(b, n, h, seed=100 * n + 10 * b + h)
    w = (torch.randn(h * 128, generator=torch.Generator().manual_seed(7)) * 0.5 + 1.0).to(BF16).cuda()
    tab = rope_table(n, seed=n)
    bq8, bk8, bsq, bsk, bkbar = _hip.attn_quant_qk(q, k, h)
    bv8t, bsv, _ = _hip.attn_quant_vt(v, h)
    fq8, fsq = _hip.rmsnorm_rope_q8(q, w, h, EPS, tab)
    fk, parts = _hip.rmsnorm_rope_kstats(k, w, h, EPS, tab)
    fk8, fsk, fkbar = _hip.attn_quant_k(fk, parts, h)
    nq8, nsq = _hip.rmsnorm_rope_q8(q, w, h, EPS)      # without a table: the cross-attention q norm
    assert bq8.shape == (b, n, h * 128) and bsk.shape == (b, h) and bv8t.shape == (b, h, 128, (n + 63) // 64 * 64) and bsv.shape == (b, h, 128)
    for e in range(b):
        qe, ke, ve = q[e:e + 1], k[e:e + 1], v[e:e + 1]
        q8, k8, sq, sk, kbar = _hip.attn_quant_qk(qe, ke, h)
        assert same(bq8[e], q8) and same(bk8[e], k8) and same(bsq[e], sq) and same(bsk[e], sk) and same(bkbar[e], kbar), ("two-step", e)
        v8t, sv, _ = _hip.attn_quant_vt(ve, h)
        assert same(bv8t[e], v8t) and same(bsv[e], sv), ("v", e)
        q8, sq = _hip.rmsnorm_rope_q8(qe, w, h, EPS, tab)
        assert same(fq8[e], q8) and same(fsq[e], sq), ("fused q", e)
        ko, pe = _hip.rmsnorm_rope_kstats(ke, w, h, EPS, tab)
        assert same(fk[e], ko[0]), ("fused k rows", e)
        k8, sk, kbar = _hip.attn_quant_k(ko, pe, h)
        assert same(fk8[e], k8) and same(fsk[e], sk) and same(fkbar[e], kbar), ("fused k", e)
        q8, sq = _hip.rmsnorm_rope_q8(qe, w, h, EPS)
        assert same(nq8[e], q8) and same(nsq[e], sq), ("plain q", e)
    # the elements do differ: the scales of element 1 are not those of element 0 (one key is its own mean: sk is the floor for both)
    assert not torch.equal(bsv[0], bsv[1]) and (n == 1 or not torch.equal(bsk[0], bsk[1]))


@gpu
def test_producers_contiguous_inputs():
    """The additional contiguous case (ld = C, batch stride N * C)."""
    b, n, h = 3, 200, 3
    q, k, v = make_qkv(b, n, h, seed=5, contiguous=True)
    bq8, bk8, bsq, bsk, _ = _hip.attn_quant_qk(q, k, h)
    bv8t, bsv, _ = _hip.attn_quant_vt(v, h)
    for e in range(b):
        q8, k8, sq, sk, _ = _hip.attn_quant_qk(q[e:e + 1], k[e:e + 1], h)
        v8t, sv, _ = _hip.attn_quant_vt(v[e:e + 1], h)
        assert same(bq8[e], q8) and same(bk8[e], k8) and same(bsq[e], sq) and same(bsk[e], sk) and same(bv8t[e], v8t) and same(bsv[e], sv), e


# ------------------------------------------------------------------------------------------------------------------ GPU: self-attention
def self_attention_case(b, h, nq, nkv, seed, with_ws):
    q, _, _ = make_qkv(b, nq, h, seed)
    _, k, v = make_qkv(b, nkv, h, seed + 1)
    q8, _, sq, _, _ = _hip.attn_quant_qk(q, q, h)
    _, k8, _, sk, _ = _hip.attn_quant_qk(k, k, h)
    v8t, sv, _ = _hip.attn_quant_vt(v, h)
    lib = _hip.load()
    need1 = lib.fg_attn_workspace_bytes(1, nq, nkv, h)
    ws = None if with_ws else []      # None: the binding's scratch, B shares of the single-element need; []: kept empty below
    scale = 0.11
    c = h * 128

    def run_b(pv8):
        out = torch.empty((b, nq, c), dtype=BF16, device="cuda")
        wsb = torch.empty(b * need1 if with_ws else 0, dtype=U8, device="cuda")
        args = (_hip._ptr(q8), nq * c, _hip._ptr(k8), nkv * c, _hip._ptr(sq), nq * h, _hip._ptr(sk), h)
        tail = (_hip._ptr(out), nq * c, b, nq, nkv, h, 128, scale, _hip._ptr(wsb) if wsb.numel() else None, wsb.numel(), _hip._stream(out))
        if pv8:
            _hip._call("fg_attn_fwd_pv8_bf16_b", *args, _hip._ptr(v8t), v8t.stride(0), _hip._ptr(sv), c, *tail)
        else:
            _hip._call("fg_attn_fwd_qk8_bf16_b", *args, _hip._ptr(v), v.stride(1), v.stride(0), *tail)
        return out

    def run_1(e, pv8):
        out = torch.empty((1, nq, c), dtype=BF16, device="cuda")
        ws1 = torch.empty(need1 if with_ws else 0, dtype=U8, device="cuda")
        tail = (_hip._ptr(out), nq, nkv, h, 128, scale, _hip._ptr(ws1) if ws1.numel() else None, ws1.numel(), _hip._stream(out))
        if pv8:
            _hip._call("fg_attn_fwd_pv8_bf16", _hip._ptr(q8[e]), _hip._ptr(k8[e]), _hip._ptr(sq[e]), _hip._ptr(sk[e]), _hip._ptr(v8t[e]),
                       _hip._ptr(sv[e]), *tail)
        else:
            _hip._call("fg_attn_fwd_qk8_bf16", _hip._ptr(q8[e]), _hip._ptr(k8[e]), _hip._ptr(sq[e]), _hip._ptr(sk[e]), _hip._ptr(v[e]),
                       v.stride(1), *tail)
        return out
    del ws
    for pv8 in (False, True):
        got = run_b(pv8)
        assert torch.isfinite(got.float()).all()
        for e in range(b):
            assert torch.equal(got[e], run_1(e, pv8)[0]), (pv8, e)
    return need1


@gpu
@pytest.mark.parametrize("nq,nkv", [(65, 65), (200, 1100), (300, 77)])
@pytest.mark.parametrize("b,h", [(2, 3), (3, 1)])
def test_self_attention_matches_per_element(b, h, nq, nkv):
    """fg_attn_fwd_qk8_bf16_b and fg_attn_fwd_pv8_bf16_b against per-element calls, with and without a workspace."""
    for with_ws in (False, True):
        self_attention_case(b, h, nq, nkv, seed=nq + nkv + b, with_ws=with_ws)


@gpu
def test_self_attention_split_kv():
    """A shape whose single-element plan splits the keys (fg_attn_workspace_bytes(1, ..) > 0): the batched forward kernel writes each
    element's partials into its share of the workspace and the batched merge reads them; without a workspace the direct path runs."""
    h, nq, nkv = SPLIT_SHAPE
    need1 = self_attention_case(2, h, nq, nkv, seed=9, with_ws=True)
    assert need1 > 0, "SPLIT_SHAPE no longer splits on this device: pick another shape at or below 4 096 keys"
    self_attention_case(2, h, nq, nkv, seed=9, with_ws=False)
    # the binding's own path: B shares of the single-element need
    q, k, v = make_qkv(2, nkv, h, seed=11)
    got = _hip.attention_qk8(q, k, v, h, pv8=True)
    for e in range(2):
        assert torch.equal(got[e], _hip.attention_qk8(q[e:e + 1], k[e:e + 1], v[e:e + 1], h, pv8=True)[0]), e


# ------------------------------------------------------------------------------------------------------------------ GPU: cross-attention
@gpu
@pytest.mark.parametrize("nkv", [1, 77, 512, 640])
@pytest.mark.parametrize("nq", [5, 300, 700])
@pytest.mark.parametrize("b,h", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_cross8_matches_per_element(b, h, nq, nkv):
    """fg_attn_fwd_cross8_bf16_b per element equals fg_attn_fwd_cross8_bf16 and fg_attn_fwd_pv8_bf16 without a workspace."""
    assert _hip.attention_cross8_max_kv() == 640
    q, _, _ = make_qkv(b, nq, h, seed=nq + nkv)
    _, k, v = make_qkv(b, nkv, h, seed=nq + nkv + 1)
    q8, _, sq, _, _ = _hip.attn_quant_qk(q, q, h)
    _, k8, _, sk, _ = _hip.attn_quant_qk(k, k, h)
    v8t, sv, _ = _hip.attn_quant_vt(v, h)
    got = _hip.attention_cross8_pre(q8, k8, sq, sk, v8t, sv, h)
    assert got.shape == (b, nq, h * 128) and torch.isfinite(got.float()).all()
    for e in range(b):
        ops = (q8[e], k8[e], sq[e], sk[e], v8t[e], sv[e])
        assert torch.equal(got[e], _hip.attention_cross8_pre(*ops, h)[0]), ("cross8", e)
        assert torch.equal(got[e], _hip.attention_pv8_pre(*ops, h, workspace=[])[0]), ("pv8 without workspace", e)


# ------------------------------------------------------------------------------------------------------------------ GPU: stream and capture
@gpu
def test_capture_and_replay():
    """One batched self-attention chain and one batched cross chain recorded under torch.cuda.graph on a side stream and replayed twice
    on refilled inputs: both replays reproduce the eager bytes."""
    b, h, n, l = 2, 2, 1100, 77
    c = h * 128
    w = torch.ones(c, dtype=BF16, device="cuda")
    tab = rope_table(n, seed=3)
    fills = [make_qkv(b, n, h, seed=s) for s in (21, 22)]
    ctxs = [make_qkv(b, l, h, seed=s) for s in (31, 32)]
    qkv = torch.empty((b, n, 3 * c), dtype=BF16, device="cuda")
    kvc = torch.empty((b, l, 2 * c), dtype=BF16, device="cuda")

    def load(i):
        for j in range(3):
            qkv[..., j * c:(j + 1) * c].copy_(fills[i][j])
        kvc[..., :c].copy_(ctxs[i][1])
        kvc[..., c:].copy_(ctxs[i][2])

    bufs = _hip.attention_qk8_fused_scratch(n, h, 128, "cuda", b)
    pvb = _hip.attention_pv8_scratch(n, h, 128, "cuda", b)
    cvb = _hip.attention_pv8_scratch(l, h, 128, "cuda", b)
    out_s = torch.empty((b, n, c), dtype=BF16, device="cuda")
    out_c = torch.empty((b, n, c), dtype=BF16, device="cuda")
    kout = torch.empty((b, n, c), dtype=BF16, device="cuda")
    kc = torch.empty((b, l, c), dtype=BF16, device="cuda")
    cparts = torch.empty((b, _hip.load().fg_attn_qk8_fused_scratch_bytes(l, c)), dtype=U8, device="cuda")
    ck8, csk, ckbar = torch.empty((b, l, c), dtype=F8, device="cuda"), torch.empty((b, h), dtype=F32, device="cuda"), \
        torch.empty((b, c), dtype=F32, device="cuda")
    ws = []

    def chain():
        q8, k8, sq, sk, kbar, parts = bufs
        _hip.rmsnorm_rope_kstats(qkv[..., c:2 * c], w, h, EPS, tab, out=kout, partials=parts)
        _hip.rmsnorm_rope_q8(qkv[..., :c], w, h, EPS, tab, q8=q8, sq=sq)
        _hip.attn_quant_k(kout, parts, h, k8, sk, kbar)
        _hip.attention_qk8_pre(q8, k8, sq, sk, qkv[..., 2 * c:], h, out=out_s, workspace=ws, pv8=True, pv8_bufs=pvb)
        # cross: the queries are the self-attention's q8 / sq, the context its own k | v rows
        _hip.rmsnorm_rope_kstats(kvc[..., :c], w, h, EPS, out=kc, partials=cparts)
        _hip.attn_quant_k(kc, cparts, h, ck8, csk, ckbar)
        v8t, sv, _ = _hip.attn_quant_vt(kvc[..., c:], h, cvb)
        _hip.attention_cross8_pre(q8, ck8, sq, csk, v8t, sv, h, out=out_c)

    eager = []
    for i in range(2):
        load(i)
        chain()      # also warms the batched cross8 kernel's hipFuncSetAttribute and grows ws before the capture
        eager.append((out_s.clone(), out_c.clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            chain()
    for i in (1, 0):
        load(i)
        out_s.zero_()
        out_c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, eager[i][0]) and torch.equal(out_c, eager[i][1]), i

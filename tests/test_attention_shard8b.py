"""The batched producers of a token shard (include/fairygen_hip_shard8b.h): fg_attn_shard8_stats_b / _quant_b / _vt_b and
fg_attn_shard8s_stats_b / _quant_b, what the stacked CFG forward runs on a rank of the K / V all-gather layout
(WanModel.enable_stacked_cfg(sharded=True); the model is tests/test_stacked_cfg_sharded.py).

  1. (no GPU) the ABI extension: declared once, exported, bound, version-checked; the argument checks.
  2. per element the bytes of the single-element entry point on that element alone — every output, nothing has a tolerance; distinct
     data per element, so a kernel that reads element 0 twice fails; local rows below one 16-row quantise group, across one, many; the
     gathered records of W = 3 ranks, one of them empty (the neutral record); fg_attn_shard8_vt_b on a contiguous input and on one whose
     elements lie further apart than N rows.
  3. the sharded chain on B = 2 against the existing batched UNSHARDED producers (include/fairygen_hip_batch8.h, the smoothing form
     included), byte for byte, on inputs whose fp64 sums are exact (asserted).
  4. stream capture: the entry points only enqueue, a replay gives the eager bytes.
No multi-GPU hardware run exists: the ranks are emulated on one GPU."""
import ctypes
import functools
import os
import re

import pytest
import torch

import test_attention_qk8_fused as fused
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from test_attention_qk8 import guarded, guards_intact, hip  # noqa: F401  (hip: the module fixture)
from test_attention_shard8 import local_ranges, u8

gpu = pytest.mark.gpu
BF16, F8, U8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.float32
EPS = fused.EPS
NAMES = ("fg_attn_shard8_stats_b", "fg_attn_shard8_quant_b", "fg_attn_shard8_vt_b", "fg_attn_shard8s_stats_b", "fg_attn_shard8s_quant_b")
QUERIES = ("fg_attn_shard8b_version",)


# ------------------------------------------------------------------------------------------------------------------ 1. ABI, checks
def test_extension_abi():
    """Fails on the parent commit: the symbols, the header and the binding's tables are this extension's."""
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_shard8b.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55      # the main table is what it was
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_shard8b.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.SHARD8B_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 6
    assert _hip.SHARD8B_ABI_VERSION == 1 and lib.fg_attn_shard8b_version() == 1
    raw = ctypes.CDLL(_hip.library_path())
    assert all(hasattr(raw, name) for name in NAMES + QUERIES)
    V, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    ctype = {"const void*": V, "void*": V, "float*": V, "fg_stream_t": V, "int64_t": I64, "int": I32}
    for name in NAMES:
        args = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        types = [ctype[a.strip().rsplit(" ", 1)[0]] for a in args.replace("\n", " ").split(",")]
        assert types == _hip._SHARD8B_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is I32
    # the smoothing forms are the plain ones, mu behind sv
    assert _hip._SHARD8B_SIGNATURES[NAMES[3]] == _hip._SHARD8B_SIGNATURES[NAMES[0]]
    base = _hip._SHARD8B_SIGNATURES[NAMES[1]]
    assert _hip._SHARD8B_SIGNATURES[NAMES[4]] == base[:15] + [V] + base[15:]
    real = _hip._lib
    try:          # load() checks the version: a library that answers another one is refused
        _hip._lib = None
        _hip.SHARD8B_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="token shard on batches"):
            _hip.load()
    finally:
        _hip.SHARD8B_ABI_VERSION, _hip._lib = 1, real


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1)."""
    lib, a = _hip.load(), 4096
    c, b = 256, 2
    pb = lib.fg_attn_qk8_fused_scratch_bytes(10, c)
    big = 1 << 24
    for smooth, stats_fn, unit, sunit in ((False, lib.fg_attn_shard8_stats_b, 20, 4), (True, lib.fg_attn_shard8s_stats_b, 32, 16)):
        def stats(partials=a, pbytes=pb, bsp=pb, v=a, ldv=c, bsv=10 * c, rec=a, rbytes=b * unit * c, scr=a, sbytes=big, bss=big, nb=b, rows=10,
                  h=2, d=128):
            return stats_fn(partials, pbytes, bsp, v, ldv, bsv, rec, rbytes, scr, sbytes, bss, nb, rows, h, d, None)
        assert stats(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
        assert stats(nb=0) == -1 and b"B in 1.." in lib.fg_last_error() and stats(nb=-1) == -1 and stats(nb=65536) == -1
        assert stats(ldv=c - 8) == -1 and stats(ldv=c + 4) == -1
        assert stats(bsv=10 * c - 8) == -1 and b"element stride of v" in lib.fg_last_error() and stats(bsv=10 * c + 4) == -1
        assert stats(rbytes=b * unit * c - 1) == -1 and b"records" in lib.fg_last_error()          # room for one record short of B
        assert stats(pbytes=pb - 1) == -1 and b"partials" in lib.fg_last_error()
        assert stats(bsp=pb - 16) == -1 and stats(bsp=pb + 8) == -1
        assert stats(sbytes=c * sunit - 1) == -1 and b"scratch" in lib.fg_last_error()
        assert stats(bss=c * sunit - 16) == -1 and stats(bss=big + 8) == -1
        assert stats(rows=0) == -1 and stats(h=0) == -1 and stats(h=33) == -1
        assert stats(partials=a + 8) == -1 and stats(rec=a + 8) == -1 and stats(v=a + 8) == -1 and stats(scr=a + 8) == -1
        assert stats(partials=None) == -1 and stats(rec=None) == -1 and stats(scr=None) == -1
        if smooth:      # v is required by the smoothing form (the plain form without v is a valid call: not made here, nothing may launch)
            assert stats(v=None) == -1 and b"null pointer" in lib.fg_last_error()

        def quant(rec=a, rbytes=4 * b * unit * c, w=4, n=40, k=a, ldk=c, bsk=10 * c, v=a, ldv=c, bsv=10 * c, k8=a, v8=a, sk=a, kbar=a, sv=a, mu=a,
                  nb=b, rows=10, h=2, d=128):
            if smooth:
                return lib.fg_attn_shard8s_quant_b(rec, rbytes, w, n, k, ldk, bsk, v, ldv, bsv, k8, v8, sk, kbar, sv, mu, nb, rows, h, d, None)
            return lib.fg_attn_shard8_quant_b(rec, rbytes, w, n, k, ldk, bsk, v, ldv, bsv, k8, v8, sk, kbar, sv, nb, rows, h, d, None)
        assert quant(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
        assert quant(nb=0) == -1 and b"B in 1.." in lib.fg_last_error() and quant(nb=65536) == -1
        assert quant(ldk=c - 8) == -1 and quant(ldv=c - 8) == -1 and quant(bsk=10 * c - 8) == -1 and quant(bsv=10 * c - 8) == -1 and quant(bsk=10 * c + 4) == -1
        assert quant(rbytes=4 * b * unit * c - 1) == -1 and b"records" in lib.fg_last_error()
        assert quant(w=0) == -1 and quant(n=0) == -1 and quant(rows=0) == -1 and quant(h=0) == -1 and quant(h=33) == -1
        assert quant(rows=41) == -1 and b"rows" in lib.fg_last_error()
        assert quant(rec=a + 8) == -1 and quant(k=a + 8) == -1 and quant(v=a + 8) == -1 and quant(kbar=a + 8) == -1 and quant(sv=a + 8) == -1
        assert quant(k8=a + 4) == -1 and quant(v8=a + 4) == -1 and quant(sk=a + 2) == -1
        assert quant(rec=None) == -1 and quant(k=None) == -1 and quant(k8=None) == -1 and quant(sk=None) == -1 and quant(kbar=None) == -1
        assert quant(v8=None) == -1 and quant(sv=None) == -1
        if smooth:
            assert quant(mu=None) == -1 and quant(mu=a + 8) == -1 and quant(v=None) == -1

    def vt(v8=a, bs=10 * c, v8t=a, nb=b, n=10, h=2, d=128):
        return lib.fg_attn_shard8_vt_b(v8, bs, v8t, nb, n, h, d, None)
    assert vt(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert vt(nb=0) == -1 and vt(n=0) == -1 and vt(h=0) == -1 and vt(h=33) == -1
    assert vt(bs=10 * c - 16) == -1 and b"element stride" in lib.fg_last_error() and vt(bs=10 * c + 8) == -1      # a short buffer; misaligned
    assert vt(v8=a + 8) == -1 and vt(v8t=a + 8) == -1 and vt(v8=None) == -1 and vt(v8t=None) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. per element
OTHER_ROWS = 23      # the rows of the second rank of the gathered records; the third rank is empty
VARIANTS = ("qk8", "pv8", "smooth")


@functools.lru_cache(maxsize=None)
def element_case(b, rows, heads):
    """B elements of distinct data: this rank's q | k | v buffer (B, rows, 3 C) and another rank's (B, OTHER_ROWS, 3 C), one norm weight, the
    rope angles of both (one element's, shared by the batch).  One v channel of element 1 carries an offset: a mean worth taking out."""
    c = heads * 128
    mine, other = seeded((b, rows, 3 * c), 7000 + 10 * rows + heads + b), seeded((b, OTHER_ROWS, 3 * c), 7500 + heads + b)
    mine[1, :, 2 * c + 3] += 2.0
    other[1, :, 2 * c + 3] += 2.0
    wk = (1 + 0.1 * seeded((c,), 7100 + heads).float()).to(BF16)
    ang = torch.rand((rows + OTHER_ROWS, 64), generator=torch.Generator("cpu").manual_seed(7200 + rows), dtype=torch.float64) * 6.283
    return mine, other, wk, ang


def _rank_records(hip, variant, d, wk, cs, heads):  # noqa: F811
    """(k, records) of one rank from its (B, rows, 3 C) buffer, through the wrappers: B > 1 takes the _b entry points, B = 1 the single ones."""
    c, rows = heads * 128, d.shape[1]
    k, parts = hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk, heads, EPS, *cs)
    v = d[..., 2 * c:]
    rec = hip.attn_shard8s_stats(parts, rows, heads, v) if variant == "smooth" else hip.attn_shard8_stats(parts, rows, heads, v if variant == "pv8" else None)
    return k, rec


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows", [1, 17, 200])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("b", [2, 3])
def test_batched_entry_points_equal_single_per_element(hip, b, heads, rows, variant):  # noqa: F811
    """record, k8, v8, sk, kbar, sv, mu of the _b entry points against the single-element entry points on each element alone, torch.equal
    on the bytes.  W = 3: this rank, a rank with 23 other rows, an empty rank (neutral records for every element).  The calls are counted
    by name: the batch runs one _b call per step and no single-element one."""
    c, smooth = heads * 128, variant == "smooth"
    mine, other, wk, ang = element_case(b, rows, heads)
    d, d2, wk = mine.cuda(), other.cuda(), wk.cuda()
    cs, cs2 = fused.tables(ang[:rows], "f32", "cuda"), fused.tables(ang[rows:], "f32", "cuda")
    n = rows + OTHER_ROWS
    neutral = (hip.attn_shard8s_neutral_record if smooth else hip.attn_shard8_neutral_record)
    quant = hip.attn_shard8s_quant if smooth else hip.attn_shard8_quant
    names, real = [], _hip._call
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(_hip, "_call", lambda name, *args: (names.append(name), real(name, *args))[1])
        k, rec = _rank_records(hip, variant, d, wk, cs, heads)
        _, rec2 = _rank_records(hip, variant, d2, wk, cs2, heads)
        empty = neutral(c, "cuda", b)
        assert rec.shape == rec2.shape == empty.shape == (b, (32 if smooth else 20) * c)
        records = torch.stack([rec, rec2, empty])      # (W, B, bytes)
        full8, k8 = guarded((b, rows, c), F8)
        fullv, v8 = guarded((b, rows, c), F8)
        v = d[..., 2 * c:] if variant != "qk8" else None
        outs = quant(records, n, k, heads, v, k8=k8, v8=v8 if v is not None else None)
    torch.cuda.synchronize()
    s = "s" if smooth else ""
    assert names.count(f"fg_attn_shard8{s}_stats_b") == 2 and names.count(f"fg_attn_shard8{s}_quant_b") == 1
    assert not any(nm in ("fg_attn_shard8_stats", "fg_attn_shard8_quant", "fg_attn_shard8s_stats", "fg_attn_shard8s_quant") for nm in names)
    assert guards_intact(full8) and guards_intact(fullv), "a guard element of k8 / v8 was written"
    if variant == "qk8":
        assert (fullv == 0x5A).all() and outs[1] is None and outs[4] is None, "the qk8-only form wrote a v output"
        assert not records[0].view(b, 5, c, 4)[:, 4].any(), "the |v| maxima of the qk8-only form are not 0"
    labels = ("k8", "v8", "sk", "kbar", "sv", "mu")
    for e in range(b):
        k1, rec1 = _rank_records(hip, variant, d[e:e + 1], wk, cs, heads)
        _, rec21 = _rank_records(hip, variant, d2[e:e + 1], wk, cs2, heads)
        assert torch.equal(k1[0], k[e]), "the batched key pass is not per element"
        assert torch.equal(rec1, rec[e]) and torch.equal(rec21, rec2[e]), f"element {e}: record differs from the single-element entry point"
        single = quant(torch.stack([rec1, rec21, neutral(c, "cuda")]), n, k1, heads, d[e:e + 1, :, 2 * c:] if variant != "qk8" else None)
        for name, got, want in zip(labels, outs, single):
            if want is None:
                assert got is None
                continue
            assert got[e].shape == want.shape and torch.equal(u8(got[e]), u8(want)), \
                f"B={b} H={heads} rows={rows} {variant}, element {e}: {name} differs from the single-element entry point"
    for e in range(1, b):      # the elements are told apart
        assert not torch.equal(u8(outs[0][e]), u8(outs[0][0])) and not torch.equal(rec[e], rec[0])


@gpu
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("n", [63, 64, 200])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("b", [2, 3])
def test_vt_batched_equals_single_per_element(hip, b, heads, n, strided):  # noqa: F811
    """fg_attn_shard8_vt_b: N = 63, 64, 200 (padding to 64: one key short of a tile, a whole tile, 8 keys into the fourth), on a contiguous
    (B, N, C) and on the rows [:N] of a slab whose elements lie N + 37 rows apart — the gathered buffer of W * chunk != N — with the rows
    behind N filled with 0xFF, which must not show up in the padding."""
    c = heads * 128
    g = torch.Generator().manual_seed(900 + n + heads + b)
    slab = torch.full((b, n + 37, c), 0xFF, dtype=U8)
    slab[:, :n] = torch.randint(0, 255, (b, n, c), dtype=U8, generator=g)
    slab = slab.cuda()
    v8 = slab[:, :n] if strided else slab[:, :n].contiguous()
    assert (v8.stride(0) == (n + 37) * c) == strided
    nkp = (n + 63) // 64 * 64
    full, v8t = guarded((b, heads, 128, nkp), F8)
    names, real = [], _hip._call
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(_hip, "_call", lambda name, *args: (names.append(name), real(name, *args))[1])
        hip.attn_shard8_vt(v8, heads, v8t=v8t)
    torch.cuda.synchronize()
    assert names == ["fg_attn_shard8_vt_b"] and guards_intact(full)
    for e in range(b):
        want = hip.attn_shard8_vt(slab[e, :n].contiguous(), heads)
        assert torch.equal(u8(v8t[e]), u8(want)), f"B={b} H={heads} N={n} strided={strided}: element {e} differs from the single-element entry point"
    assert not torch.equal(u8(v8t[0]), u8(v8t[1]))


# ------------------------------------------------------------------------------------------------------------------ 3. the chain
@functools.lru_cache(maxsize=None)
def chain_case(n, heads):
    """B = 2: element 0 is tests/test_attention_shard8.py's recipe (fused.case), element 1 the same rows in reverse order — other bytes in
    every row once the (shared) rotation is applied, the same exactness of the sums."""
    qkv, _, wk, ang = fused.case(n, heads, "normal")
    return torch.cat([qkv, qkv.flip(1)], 0).contiguous(), wk, ang


CHAIN = [(333, 2), (333, 3), (200, 3), (4, 3)]


@gpu
@pytest.mark.parametrize("smooth", [False, True], ids=["pv8", "smooth"])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("n,world", CHAIN, ids=[f"N{n}-W{w}" for n, w in CHAIN])
def test_sharded_chain_equals_unsharded_batched(hip, n, world, heads, smooth):  # noqa: F811
    """For W in (2, 3) and B = 2 the gathered k8, v8t, sk, sv (and mu) of the sharded chain are byte for byte those of the batched unsharded
    producers.  N = 333: chunks 167 and 111, no multiple of 16 or 64; N = 200, W = 3: the last rank one row short; N = 4, W = 3: the last
    rank is empty and sends B neutral records."""
    c = heads * 128
    qkv, wk, ang = chain_case(n, heads)
    d, wk = qkv.cuda(), wk.cuda()
    k_ref, parts = hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk, heads, EPS, *fused.tables(ang, "f32", "cuda"))
    k8_ref, sk_ref, kbar_ref = hip.attn_quant_k(k_ref, parts, heads)
    vref = hip.attn_quant_vt(d[..., 2 * c:], heads, smooth=smooth)
    torch.cuda.synchronize()
    for e in range(2):
        assert fused.exact_sum_bits(k_ref[e].cpu(), n) <= 52 and fused.exact_sum_bits(qkv[e, :, 2 * c:], n) <= 52, "an fp64 sum is not exact"
    ranges = local_ranges(n, world)
    assert (n, world) != (4, 3) or ranges[-1] == (4, 4), "the case of an empty last rank"
    neutral = hip.attn_shard8s_neutral_record if smooth else hip.attn_shard8_neutral_record
    ks, recs = [], []
    for lo, hi in ranges:
        if hi == lo:
            ks.append(None)
            recs.append(neutral(c, "cuda", 2))
            continue
        k, rec = _rank_records(hip, "smooth" if smooth else "pv8", d[:, lo:hi].contiguous(), wk, fused.tables(ang[lo:hi], "f32", "cuda"), heads)
        ks.append(k)
        recs.append(rec)
    records = torch.stack(recs)
    assert records.shape == (world, 2, (32 if smooth else 20) * c)
    outs = [None if k is None else (hip.attn_shard8s_quant if smooth else hip.attn_shard8_quant)(records, n, k, heads, d[:, lo:hi, 2 * c:].contiguous())
            for k, (lo, hi) in zip(ks, ranges)]
    live = [o for o in outs if o is not None]
    what = f"N = {n}, W = {world}, {heads} heads, {'smooth' if smooth else 'pv8'}: "
    for r, o in enumerate(live):
        for name, got, want in (("sk", o[2], sk_ref), ("kbar", o[3], kbar_ref), ("sv", o[4], vref[1])) + ((("mu", o[5], vref[3]),) if smooth else ()):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what + f"rank {r}: {name} differs from the unsharded batched producer's"
    k8 = torch.cat([u8(o[0]) for o in live], dim=1)
    assert torch.equal(k8, u8(k8_ref)), what + f"{(k8 != u8(k8_ref)).sum().item()} of {k8.numel()} bytes of the gathered k8 differ"
    # the gathered v8 in a slab of W * chunk rows per element, as the exchange leaves it: read where it lies
    chunk = -(-n // world)
    slab = torch.full((2, world * chunk, c), 0xFF, dtype=U8, device="cuda")
    slab[:, :n] = torch.cat([u8(o[1]) for o in live], dim=1)
    v8t = hip.attn_shard8_vt(slab[:, :n], heads)
    torch.cuda.synchronize()
    assert torch.equal(u8(v8t), u8(vref[0])), what + f"{(u8(v8t) != u8(vref[0])).sum().item()} of {v8t.numel()} bytes of v8t differ"


# ------------------------------------------------------------------------------------------------------------------ 4. capture
@gpu
@pytest.mark.parametrize("smooth", [False, True], ids=["pv8", "smooth"])
def test_entry_points_only_enqueue_and_capture(hip, smooth):  # noqa: F811
    """The batched entry points recorded on a side stream into a graph: nothing runs at capture (the outputs keep their fill), a replay
    gives the bytes of the eager calls."""
    b, heads, rows = 2, 2, 84
    c = heads * 128
    unit = 32 if smooth else 20
    mine, _, wk, ang = element_case(b, rows, heads)
    d = mine.cuda()
    k, parts = hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk.cuda(), heads, EPS, *fused.tables(ang[:rows], "f32", "cuda"))
    v = d[..., 2 * c:]
    others = (hip.attn_shard8s_neutral_record if smooth else hip.attn_shard8_neutral_record)(c, "cuda", b)
    want_rec = (hip.attn_shard8s_stats if smooth else hip.attn_shard8_stats)(parts, rows, heads, v)
    want = (hip.attn_shard8s_quant if smooth else hip.attn_shard8_quant)(torch.stack([want_rec, others]), rows, k, heads, v)
    want_t = hip.attn_shard8_vt(want[1], heads)
    torch.cuda.synchronize()
    recs = torch.stack([torch.full_like(want_rec, 0x7F), others])
    k8, v8 = (torch.full((b, rows, c), 0x7F, dtype=U8, device="cuda").view(F8) for _ in range(2))
    v8t = torch.full((b, heads, 128, 128), 0x7F, dtype=U8, device="cuda").view(F8)
    need = (hip.load().fg_attn_shard8s_scratch_bytes if smooth else hip.load().fg_attn_shard8_scratch_bytes)(rows, c)
    scratch = torch.empty((b, need), dtype=U8, device="cuda")
    sk, kbar, sv, mu = (torch.full((b, m), -1.0, device="cuda") for m in (heads, c, c, c))
    s_ = "s" if smooth else ""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        s = hip._stream(k)
        hip._call(f"fg_attn_shard8{s_}_stats_b", hip._ptr(parts), parts.shape[1], parts.stride(0), hip._ptr(v), 3 * c, rows * 3 * c, hip._ptr(recs),
                  b * unit * c, hip._ptr(scratch), need, need, b, rows, heads, 128, s)
        hip._call(f"fg_attn_shard8{s_}_quant_b", hip._ptr(recs), recs.numel(), 2, rows, hip._ptr(k), c, rows * c, hip._ptr(v), 3 * c, rows * 3 * c,
                  hip._ptr(k8), hip._ptr(v8), hip._ptr(sk), hip._ptr(kbar), hip._ptr(sv), *((hip._ptr(mu),) if smooth else ()), b, rows, heads, 128, s)
        hip._call("fg_attn_shard8_vt_b", hip._ptr(v8), rows * c, hip._ptr(v8t), b, rows, heads, 128, s)
    torch.cuda.synchronize()
    assert all((u8(t) == 0x7F).all() for t in (recs[0], k8, v8, v8t)) and all((t == -1.0).all() for t in (sk, kbar, sv, mu)), "a capture launched work"
    graph.replay()
    first = [u8(t).clone() for t in (recs[0], k8, v8, v8t)]
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, u8(t)) for a, t in zip(first, (recs[0], k8, v8, v8t))), "two replays differ"
    for name, got, ref in (("record", recs[0], want_rec), ("k8", k8, want[0]), ("v8", v8, want[1]), ("sk", sk, want[2]), ("kbar", kbar, want[3]),
                           ("sv", sv, want[4].view(b, -1)), ("v8t", v8t, want_t)) + ((("mu", mu, want[5].view(b, -1)),) if smooth else ()):
        assert torch.equal(u8(got), u8(ref)), name

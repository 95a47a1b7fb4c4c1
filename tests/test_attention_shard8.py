"""The opt-in e4m3 self-attention on token-sharded layouts (WanModel.enable_qk8_attention(sharded=True), include/fairygen_hip_shard8.h).

The property everything rests on: for any partition of the rows [0, N) into W contiguous shards, some possibly empty, the gathered k8 and
v8t and every rank's sk, key mean and sv are byte for byte what fg_rmsnorm_rope_kstats_bf16 + fg_attn_quant_k_bf16 and
fg_attn_quant_vt_bf16 write on the unsharded rows, where the fp64 key sum is exact (asserted on the CPU for the inputs used).  Nothing in
the operand comparisons has a tolerance.

  1. (no GPU) the ABI extension: declared once, exported, bound; the argument checks; the routing switch; the record exchange of the
     mailbox double on CPU tensors and of the real TokenShard over gloo.
  2. the kernels: the sharded chain against the unsharded entry points on guarded, sentinel-filled buffers; attention on a shard's queries
     against the torch recipes of tests/test_attention_qk8.py and tests/test_attention_pv8.py and against the unsharded call; the Ulysses
     head groups; stream capture.
  3. the dim-3072 model of tests/test_token_shard_invariance.py with emulated ranks, both exchange modes, both forms.
No multi-GPU hardware run exists: the ranks are emulated on one GPU."""
import ctypes
import functools
import math
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_attention_pv8 as pv8t
import test_attention_qk8 as qk8t
import test_attention_qk8_fused as fused
import test_token_shard_invariance as tsi
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic
from fairygen_amd.sequence_parallel import TokenShard
from test_attention_qk8 import guarded, guards_intact, hip  # noqa: F401  (hip: the module fixture)
from test_token_shard_invariance import medium  # noqa: F401  (the module fixture)

gpu = pytest.mark.gpu
BF16, F8, U8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.float32
EPS = fused.EPS
NAMES = ("fg_attn_shard8_stats", "fg_attn_shard8_quant", "fg_attn_shard8_vt")
QUERIES = ("fg_attn_shard8_version", "fg_attn_shard8_record_bytes", "fg_attn_shard8_scratch_bytes")


# ------------------------------------------------------------------------------------------------------------------ 1. ABI, checks, routing
def test_extension_abi():
    lib = _hip.load()
    main = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    ext = open(os.path.join(REPO, "include", "fairygen_hip_shard8.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55 and len(_hip.PV8_SYMBOLS) == 4
    assert not any(name in _hip.EXPORTED_SYMBOLS or name in _hip.PV8_SYMBOLS or name in main for name in NAMES + QUERIES)
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.SHARD8_SYMBOLS == sorted(NAMES + QUERIES)
    assert _hip.SHARD8_ABI_VERSION == 1 and lib.fg_attn_shard8_version() == 1
    V, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _hip._SHARD8_SIGNATURES == {NAMES[0]: [V, I64, V, I64, V, I64, V, I64, I64, I32, I32, V],
                                       NAMES[1]: [V, I64, I32, I64, V, I64, V, I64, V, V, V, V, V, I64, I32, I32, V],
                                       NAMES[2]: [V, V, I64, I32, I32, V]}
    assert _hip._SHARD8_QUERIES == {QUERIES[0]: (I32, []), QUERIES[1]: (I64, [I32]), QUERIES[2]: (I64, [I64, I32])}
    # the argument lists of the header, type by type, are the bound ones
    ctype = {"const void*": V, "void*": V, "float*": V, "fg_stream_t": V, "int64_t": I64, "int": I32}
    for name in NAMES:
        args = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        types = [ctype[a.strip().rsplit(" ", 1)[0]] for a in args.replace("\n", " ").split(",")]
        assert types == _hip._SHARD8_SIGNATURES[name] == getattr(lib, name).argtypes, name
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    assert "20 * C" in ext and "PV8_KEY_ORDER" in ext


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1)."""
    lib, a = _hip.load(), 4096
    c = 256
    assert lib.fg_attn_shard8_record_bytes(c) == 20 * c and lib.fg_attn_shard8_record_bytes(3072) == 61440
    assert lib.fg_attn_shard8_record_bytes(0) == -1 and lib.fg_attn_shard8_record_bytes(200) == -1 and lib.fg_attn_shard8_record_bytes(4224) == -1
    assert lib.fg_attn_shard8_scratch_bytes(84, c) == 6 * c * 4 and lib.fg_attn_shard8_scratch_bytes(10 ** 6, 3072) == 256 * 3072 * 4
    assert lib.fg_attn_shard8_scratch_bytes(0, c) == -1 and lib.fg_attn_shard8_scratch_bytes(5, 100) == -1
    pb = lib.fg_attn_qk8_fused_scratch_bytes(10, c)
    big = 1 << 24

    def stats(partials=a, pbytes=pb, v=a, ldv=c, rec=a, rbytes=20 * c, scr=a, sbytes=big, rows=10, h=2, d=128):
        return lib.fg_attn_shard8_stats(partials, pbytes, v, ldv, rec, rbytes, scr, sbytes, rows, h, d, None)
    assert stats(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert stats(ldv=c - 8) == -1 and stats(ldv=c + 4) == -1                       # ldv < C; not a multiple of 8
    assert stats(rbytes=20 * c - 1) == -1 and b"record" in lib.fg_last_error()     # a record buffer that is too small
    assert stats(pbytes=pb - 1) == -1 and b"partials" in lib.fg_last_error()
    assert stats(sbytes=c * 4 - 1) == -1 and b"scratch" in lib.fg_last_error()
    assert stats(scr=None) == -1                                                   # v without scratch
    assert stats(rows=0) == -1 and stats(h=0) == -1 and stats(h=33) == -1
    assert stats(partials=a + 8) == -1 and stats(rec=a + 8) == -1 and stats(v=a + 8) == -1 and stats(scr=a + 8) == -1
    assert stats(partials=None) == -1 and stats(rec=None) == -1

    def quant(rec=a, rbytes=4 * 20 * c, w=4, n=40, k=a, ldk=c, v=a, ldv=c, k8=a, v8=a, sk=a, kbar=a, sv=a, rows=10, h=2, d=128):
        return lib.fg_attn_shard8_quant(rec, rbytes, w, n, k, ldk, v, ldv, k8, v8, sk, kbar, sv, rows, h, d, None)
    assert quant(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert quant(ldk=c - 8) == -1 and quant(ldv=c - 8) == -1
    assert quant(rbytes=4 * 20 * c - 1) == -1 and b"records" in lib.fg_last_error()
    assert quant(w=0) == -1 and quant(n=0) == -1 and quant(rows=0) == -1
    assert quant(rows=41) == -1 and b"rows" in lib.fg_last_error()                  # more local rows than keys in all
    assert quant(rec=a + 8) == -1 and quant(k=a + 8) == -1 and quant(v=a + 8) == -1 and quant(kbar=a + 8) == -1 and quant(sv=a + 8) == -1
    assert quant(k8=a + 4) == -1 and quant(v8=a + 4) == -1 and quant(sk=a + 2) == -1
    assert quant(v8=None) == -1 and quant(sv=None) == -1 and quant(k8=None) == -1   # v needs v8 and sv
    assert lib.fg_attn_shard8_vt(a, a, 10, 2, 64, None) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert lib.fg_attn_shard8_vt(a, a, 0, 2, 128, None) == -1 and lib.fg_attn_shard8_vt(a, a, 10, 0, 128, None) == -1
    assert lib.fg_attn_shard8_vt(a + 8, a, 10, 2, 128, None) == -1 and lib.fg_attn_shard8_vt(a, a + 8, 10, 2, 128, None) == -1
    assert lib.fg_attn_shard8_vt(None, a, 10, 2, 128, None) == -1


def test_enable_sets_the_routing():
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)

    class Shard:
        active = True
    assert m.qk8_sharded is False
    for kw in ({}, {"pv8": True}, {"fused_producer": True}):
        m.enable_qk8_attention(**kw)
        assert m.qk8_sharded is False, "off by default"
        with pytest.raises(NotImplementedError, match="token-sharded"):
            m.check_qk8_layout(Shard())
        assert m.enable_qk8_attention(sharded=True, **kw) is m and m.qk8_sharded is True and m.pv8_attention is bool(kw.get("pv8"))
        m.check_qk8_layout(Shard())
        m.check_qk8_layout(None)
    with pytest.raises(ValueError, match="sharded"):
        m.enable_qk8_attention(False, sharded=True)
    m.enable_qk8_attention(sharded=True)
    m.enable_qk8_attention()
    assert m.qk8_sharded is False, "a plain enable switches the sharded form off again"
    m.enable_qk8_attention(sharded=True)
    m.enable_qk8_attention(False)
    assert m.qk8_sharded is False and m.qk8_attention is False
    m.check_qk8_layout(Shard())
    # the predicate is takes_qk8_attention on the TOTAL key count: a shard of 200 rows of 1 600 keys takes the mode, one of 1 000 does not
    # (that the forward asks it about the total: test_emulated_ranks_equal_unsharded_forward counts the kernels)
    attn = m.blocks[0].self_attn.attn
    m.enable_qk8_attention(sharded=True)
    assert dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV + 1, 1) and not dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV, 1)


class RecordShard(tsi.LoopbackShard):
    """tsi.LoopbackShard with the record exchange of the e4m3 mode."""

    def all_gather_records_async(self, record):
        return _LoopRecords(self, self._post("rec", record.contiguous().view(-1)))


class _LoopRecords:
    def __init__(self, shard, key):
        self.shard, self.key = shard, key

    def wait(self):
        items = self.shard.box.collect(self.key)
        assert len({(t.numel(), t.dtype) for t in items}) == 1
        return torch.stack(items)


@pytest.mark.parametrize("world", [3, 4, 8])
def test_loopback_record_exchange(world):
    """The mailbox double on random CPU tensors: every rank receives the W records in rank order; N = 43 leaves the last rank short, and
    the uint8 k8 gathered through all_gather_kv_async beside a bf16 v comes back as the concatenation."""
    n, c = 43, 256
    box = tsi.Mailbox(world)
    shards = [RecordShard(box, r, "allgather") for r in range(world)]
    ranges = [s.local_range(n) for s in shards]
    assert 0 < ranges[-1][1] - ranges[-1][0] < ranges[0][1] - ranges[0][0]
    recs = [torch.randint(0, 256, (20 * c,), dtype=U8, generator=torch.Generator().manual_seed(r)) for r in range(world)]
    pend = [s.all_gather_records_async(rec) for s, rec in zip(shards, recs)]
    for p in pend:
        got = p.wait()
        assert got.shape == (world, 20 * c) and torch.equal(got, torch.stack(recs))
    assert box.completed == 1 and not box.slots
    k8 = torch.randint(0, 256, (1, n, c), dtype=U8, generator=torch.Generator().manual_seed(99))
    v = seeded((1, n, 3 * c), 3)[..., 2 * c:]
    pend = [s.all_gather_kv_async(k8[:, lo:hi], v[:, lo:hi], n) for s, (lo, hi) in zip(shards, ranges)]
    for p in pend:
        kf, vf = p.wait()
        assert kf.dtype == U8 and torch.equal(kf, k8) and torch.equal(vf, v)
    assert box.completed == 2
    with pytest.raises(RuntimeError, match="no deposit"):
        shards[0].all_gather_records_async(recs[0]).wait()


def _gloo_worker(rank, world, port, result_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = TokenShard()
        c, n = 256, 43
        recs = [torch.randint(0, 256, (20 * c,), dtype=U8, generator=torch.Generator().manual_seed(r)) for r in range(world)]
        pend_a = shard.all_gather_records_async(recs[rank])
        pend_b = shard.all_gather_records_async(recs[rank].flip(0))      # two in flight, as the interleaved CFG branches have
        assert torch.equal(pend_a.wait(), torch.stack(recs)) and torch.equal(pend_b.wait(), torch.stack(recs).flip(1))
        k8 = torch.randint(0, 256, (1, n, c), dtype=U8, generator=torch.Generator().manual_seed(7))
        v = seeded((1, n, 3 * c), 3)[..., 2 * c:]
        lo, hi = shard.local_range(n)
        kf, vf = shard.all_gather_kv_async(k8[:, lo:hi], v[:, lo:hi], n).wait()
        assert kf.dtype == U8 and torch.equal(kf, k8) and torch.equal(vf, v)
        open(os.path.join(result_dir, f"ok{rank}"), "w").close()
    finally:
        dist.destroy_process_group()


def test_record_exchange_gloo(tmp_path):
    """The real TokenShard.all_gather_records_async (and a uint8 K gather beside a bf16 V) on CPU tensors, two gloo ranks."""
    mp.spawn(_gloo_worker, args=(2, 29661, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / f"ok{r}") for r in range(2))


def test_inactive_shard_records_are_identity():
    rec = torch.arange(40, dtype=U8)
    assert torch.equal(TokenShard().all_gather_records_async(rec).wait(), rec.unsqueeze(0))


# ------------------------------------------------------------------------------------------------------------------ 2. the kernels
def local_ranges(n, world):
    s = TokenShard()
    s.world_size = world
    return [s.local_range(n, r) for r in range(world)]


SPIKE_K_CH, SPIKE_V_CH = 5, 130      # channel 5 of head 0 of k, channel 2 of head 1 of v


@functools.lru_cache(maxsize=None)
def chain_case(n, heads, world, variant):
    """fused.case(n, heads, "normal" / "offset"), or "spiked": one key channel far out in a row of rank 1 and one v channel far out in a
    row of the last rank that has rows, so that the extremes that decide sk and sv come from different ranks."""
    qkv, wq, wk, ang = fused.case(n, heads, "offset" if variant == "offset" else "normal")
    if variant == "spiked":
        qkv, c = qkv.clone(), heads * 128
        ranges = [r for r in local_ranges(n, world) if r[1] > r[0]]
        qkv[0, ranges[1][0], c + SPIKE_K_CH] = 60.0
        qkv[0, ranges[-1][1] - 1, 2 * c + SPIKE_V_CH] = -40.0
        ang = ang.clone()
        ang[:, SPIKE_K_CH // 2] = 0      # not rotated away
    return qkv, wq, wk, ang


@functools.lru_cache(maxsize=None)
def unsharded(n, heads, world, variant):
    """The unsharded entry points on the device, once: (k bf16, k8, sk, kbar, v8t, sv, q8, sq)."""
    qkv, wq, wk, ang = chain_case(n, heads, world, variant)
    c = heads * 128
    d, cs = qkv.cuda(), fused.tables(ang, "f32", "cuda")
    k, parts = _hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    k8, sk, kbar = _hip.attn_quant_k(k, parts, heads)
    v8t, sv, _ = _hip.attn_quant_vt(d[..., 2 * c:], heads)
    q8, sq = _hip.rmsnorm_rope_q8(d[..., :c], wq.cuda(), heads, EPS, *cs)
    torch.cuda.synchronize()
    assert fused.exact_sum_bits(k[0].cpu(), n) <= 52, "the fp64 sum of these keys is not exact: the comparison of the mean would not be one"
    return k[0], k8, sk, kbar, v8t, sv, q8, sq


def sharded_chain(hip, n, heads, world, variant, with_v):  # noqa: F811
    """Every rank's launches on guarded, sentinel-filled outputs.  Returns (records, per-rank (k8, v8, sk, kbar, sv), ranges)."""
    qkv, wq, wk, ang = chain_case(n, heads, world, variant)
    c = heads * 128
    d, wk_d = qkv.cuda(), wk.cuda()
    ranges = local_ranges(n, world)
    ks, records, fulls = [], [], []
    for lo, hi in ranges:
        if hi == lo:      # a rank without rows launches nothing
            ks.append(None)
            records.append(hip.attn_shard8_neutral_record(c, "cuda"))
            continue
        cs = fused.tables(ang[lo:hi], "f32", "cuda")
        k, parts = hip.rmsnorm_rope_kstats(d[:, lo:hi, c:2 * c], wk_d, heads, EPS, *cs)
        full, rec = guarded((1, 20 * c), U8)
        hip.attn_shard8_stats(parts, hi - lo, heads, d[:, lo:hi, 2 * c:] if with_v else None, record=rec.view(-1))
        fulls.append(full)
        ks.append(k)
        records.append(rec.view(-1))
    records = torch.stack(records)
    outs = []
    for (lo, hi), k in zip(ranges, ks):
        if k is None:
            outs.append(None)
            continue
        rows = hi - lo
        f, b = zip(*[guarded(s, t) for s, t in (((rows, c), F8), ((rows, c), F8), ((1, heads), F32), ((1, c), F32), ((1, c), F32))])
        v = d[:, lo:hi, 2 * c:] if with_v else None
        hip._call("fg_attn_shard8_quant", hip._ptr(records), records.numel(), world, n, hip._ptr(k), c, hip._ptr(v), 3 * c if with_v else 0,
                  hip._ptr(b[0]), hip._ptr(b[1]) if with_v else None, hip._ptr(b[2]), hip._ptr(b[3]), hip._ptr(b[4]) if with_v else None,
                  rows, heads, 128, hip._stream(k))
        fulls.extend(f)
        outs.append((b[0], b[1], b[2].view(heads), b[3].view(c), b[4].view(heads, 128), f))
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in fulls), "a guard row of an output was written"
    return records, outs, ranges


def u8(t):
    return t.contiguous().view(U8)


PARTITIONS = [(333, 4), (43, 8), (9, 4), (128, 2), (1100, 3)]
CHAIN = [(n, w, h, "normal") for n, w in PARTITIONS for h in (2, 3)] + [(333, 4, 24, "normal"), (333, 4, 2, "offset"), (333, 4, 3, "spiked"),
                                                                         (1100, 3, 2, "spiked")]


@gpu
@pytest.mark.parametrize("with_v", [False, True], ids=["qk8", "pv8"])
@pytest.mark.parametrize("n,world,heads,variant", CHAIN, ids=[f"N{n}-W{w}-H{h}-{v}" for n, w, h, v in CHAIN])
def test_sharded_chain_equals_unsharded(hip, n, world, heads, variant, with_v):  # noqa: F811
    """N = 333, W = 4: chunk 84, no multiple of 64 or 16, the 64-key tiles straddle every boundary.  N = 43, W = 8: chunk 6, the last rank
    holds 1 row.  N = 9, W = 4: the last rank is empty.  N = 128, W = 2: boundaries on tiles, no padding.  N = 1 100, W = 3: above
    QK8_MIN_KV.  2 and 3 heads: one and two key-statistics vector slots per lane; 24 heads once."""
    c = heads * 128
    k_ref, k8_ref, sk_ref, kbar_ref, v8t_ref, sv_ref, _, _ = unsharded(n, heads, world, variant)
    records, outs, ranges = sharded_chain(hip, n, heads, world, variant, with_v)
    what = f"N = {n}, W = {world}, {heads} heads, {variant}, {'pv8' if with_v else 'qk8'}: "
    assert (n, world) != (9, 4) or ranges[-1] == (9, 9), "the case of an empty last rank"
    assert (n, world) != (43, 8) or ranges[-1] == (42, 43)
    for r, (out, (lo, hi)) in enumerate(zip(outs, ranges)):
        if out is None:
            continue
        k8, v8, sk, kbar, sv, fulls = out
        for name, got, want in (("sk", sk, sk_ref), ("kbar", kbar, kbar_ref)) + ((("sv", sv, sv_ref),) if with_v else ()):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what + f"rank {r}: {name} differs from the unsharded one"
        if not with_v:      # nothing of v8 / sv was written
            assert (fulls[1] == qk8t.POISON).all() and (fulls[4] == qk8t.POISON).all(), what + "the qk8-only form wrote a v output"
            assert not records.view(world, 5, c, 4)[:, 4].any(), what + "the |v| maxima of the qk8-only form are not 0"
        assert not (u8(k8) == qk8t.POISON).all(dim=1).any(), what + f"rank {r}: rows of k8 were not written"
    k8 = torch.cat([u8(o[0]) for o in outs if o is not None])
    assert torch.equal(k8, u8(k8_ref)), what + f"{(k8 != u8(k8_ref)).sum().item()} of {k8.numel()} bytes of the gathered k8 differ"
    if with_v:
        v8 = torch.cat([u8(o[1]) for o in outs if o is not None])
        nkp = (n + 63) // 64 * 64
        full, v8t = guarded((heads, 128, nkp), F8)
        hip.attn_shard8_vt(v8, heads, v8t=v8t)
        torch.cuda.synchronize()
        assert guards_intact(full), "a guard row of v8t was written"
        assert torch.equal(u8(v8t), u8(v8t_ref)), what + f"{(u8(v8t) != u8(v8t_ref)).sum().item()} of {v8t.numel()} bytes of v8t differ"
        nat, pad = pv8t.from_tiles(u8(v8t).cpu(), n)
        assert (pad == 0).all() and torch.equal(nat, v8.cpu()), what + "v8t is not the tile order of the gathered v8 with zero padding"
    if variant == "spiked":      # the maxima really cross ranks: sk's comes from rank 1, sv's from the last rank with rows
        live = [r for r, (lo, hi) in enumerate(ranges) if hi > lo]
        rec = records.cpu().view(world, 5, c, 4)      # the arithmetic of the check on the CPU: IEEE division
        kmax = rec[:, 3].contiguous().view(F32).squeeze(-1)[:, SPIKE_K_CH]
        assert kmax.argmax().item() == live[1] and (kmax[live[1]] - kbar_ref.cpu()[SPIKE_K_CH]) / 448 == sk_ref.cpu()[0], what + "the key spike does not set sk"
        if with_v:
            vmax = rec[:, 4].contiguous().view(F32).squeeze(-1)[:, SPIKE_V_CH]
            assert vmax.argmax().item() == live[-1] and vmax[live[-1]].item() == 40.0
            assert sv_ref.cpu().view(-1)[SPIKE_V_CH].item() == (torch.tensor(40.0) / 448).item()


def fwd(hip, form, q8, k8, sq, sk, v, sv, heads):  # noqa: F811
    """One direct launch (no workspace: every q-block one workgroup) of the qk8 (v: (Nkv, C) bf16) or pv8 (v: v8t) attention."""
    nq, nkv, c = q8.shape[0], k8.shape[0], heads * 128
    out = torch.empty((nq, c), dtype=BF16, device="cuda")
    if form == "pv8":
        hip._call("fg_attn_fwd_pv8_bf16", *[hip._ptr(t) for t in (q8, k8, sq, sk, v, sv)], hip._ptr(out), nq, nkv, heads, 128, 128 ** -0.5,
                  None, 0, hip._stream(out))
    else:
        hip._call("fg_attn_fwd_qk8_bf16", *[hip._ptr(t) for t in (q8, k8, sq, sk, v)], v.stride(0), hip._ptr(out), nq, nkv, heads, 128,
                  128 ** -0.5, None, 0, hip._stream(out))
    return out


@functools.lru_cache(maxsize=None)
def small_logit_case():
    """N = 1 100, 3 heads, W = 3 with the q norm weight scaled by 1/8 (exact in bf16): the logits stay small enough that no wave of the
    attention kernels takes its deferred rescale, whichever rows share it."""
    n, heads, world = 1100, 3, 3
    qkv, wq, wk, ang = fused.case(n, heads, "normal")
    return n, heads, world, qkv, (wq.float() / 8).to(BF16), wk, ang


@gpu
@pytest.mark.parametrize("form", ["qk8", "pv8"])
def test_attention_on_a_shards_queries(hip, form):  # noqa: F811
    """Nq = n_local against Nkv = N with operands from the sharded chain: against the fp64 recipes under the criteria of
    test_attention_qk8.py / test_attention_pv8.py; and the concatenated shard outputs equal the unsharded call bit for bit, under the
    condition of test_token_shard_invariance.py on the logits — with the threshold of the form: a maximum that cannot move by more than
    2^6 (qk8) or 2^3 (pv8, PV8_DEFER_LOG2) after the first tile, i.e. max |scale log2(e) logit| <= 3 or 1.5."""
    n, heads, world, qkv, wq, wk, ang = small_logit_case()
    c = heads * 128
    d, wq_d, wk_d = qkv.cuda(), wq.cuda(), wk.cuda()
    ranges = local_ranges(n, world)
    v = d[0, :, 2 * c:]
    ks, recs, q8s, sqs = [], [], [], []
    for lo, hi in ranges:
        cs = fused.tables(ang[lo:hi], "f32", "cuda")
        k, parts = hip.rmsnorm_rope_kstats(d[:, lo:hi, c:2 * c], wk_d, heads, EPS, *cs)
        recs.append(hip.attn_shard8_stats(parts, hi - lo, heads, d[:, lo:hi, 2 * c:] if form == "pv8" else None))
        q8, sq = hip.rmsnorm_rope_q8(d[:, lo:hi, :c], wq_d, heads, EPS, *cs)
        ks.append(k), q8s.append(q8), sqs.append(sq)
    recs = torch.stack(recs)
    assert fused.exact_sum_bits(torch.cat([k[0] for k in ks]).cpu(), n) <= 52, "the fp64 sum of these keys is not exact"
    quant = [hip.attn_shard8_quant(recs, n, k, heads, d[:, lo:hi, 2 * c:] if form == "pv8" else None) for k, (lo, hi) in zip(ks, ranges)]
    k8 = torch.cat([u8(x[0]) for x in quant]).view(F8)
    sk, sv = quant[0][2], quant[0][4]
    vop = hip.attn_shard8_vt(torch.cat([u8(x[1]) for x in quant]), heads) if form == "pv8" else v
    q8_full, sq_full = torch.cat(q8s), torch.cat(sqs)
    whole = fwd(hip, form, q8_full, k8, sq_full, sk, vop, sv, heads)
    parts = [fwd(hip, form, q8, k8, sq, sk, vop, sv, heads) for q8, sq in zip(q8s, sqs)]
    torch.cuda.synchronize()
    # the recipes, on the CPU, on the same operands
    q8c, k8c, sqc, skc, vc = q8_full.cpu(), k8.cpu(), sq_full.cpu(), sk.cpu(), v.cpu()
    ref = qk8t.attn_emu(q8c, k8c, sqc, skc, vc, heads)
    got = torch.cat(parts).cpu()
    err = (got.double() - ref).abs()
    if form == "qk8":
        err_ref = (ref.to(BF16).double() - ref).abs().max().item()
        print(f"qk8 on shard queries: err {err.max().item():.3e}, bf16(emu) err {err_ref:.3e}")
        assert err.max().item() <= 2 * err_ref + qk8t.ATTN_FLOOR
    else:
        v8c = pv8t.from_tiles(u8(vop).cpu(), n)[0].view(F8)
        e = (pv8t.attn_pv8_emu(q8c, k8c, sqc, skc, v8c, sv.cpu(), heads) - ref).abs()
        print(f"pv8 on shard queries: max {err.max().item():.3e} (recipe {e.max().item():.3e}), mean {err.mean().item():.3e} (recipe "
              f"{e.mean().item():.3e})")
        assert err.max().item() <= 2 * e.max().item() + qk8t.ATTN_FLOOR and err.mean().item() <= 2 * e.mean().item() + qk8t.ATTN_FLOOR
    # the condition for bit-equality, on the dequantised logits
    s2 = 128 ** -0.5 * math.log2(math.e)
    a = (q8c.float().view(n, heads, 128) * sqc.unsqueeze(-1)).double()
    b = (k8c.float().view(n, heads, 128) * skc.view(1, heads, 1)).double()
    peak = (s2 * torch.einsum("qhd,khd->hqk", a, b)).abs().max().item()
    limit = 3.0 if form == "qk8" else _hip.PV8_DEFER_LOG2 / 2
    print(f"{form}: max |scaled base-2 logit| = {peak:.3f} (limit {limit})")
    assert peak <= limit
    for (lo, hi), p in zip(ranges, parts):
        tsi.assert_same_rows(p, whole, lo, hi, f"{form} attention on the queries of shard [{lo}, {hi})")


@gpu
@pytest.mark.parametrize("pv8", [False, True], ids=["qk8", "pv8"])
def test_ulysses_head_groups_equal_unsharded_columns(hip, pv8):  # noqa: F811
    """W = 3, one head per rank, N = 1 100: behind the first all-to-all a rank holds all tokens of its head as strided views of the
    receive buffer; the operands written from them are the unsharded operands' columns, byte for byte."""
    n, heads, world, qkv, wq, wk, ang = small_logit_case()
    c, g = heads * 128, 128
    d, cs = qkv.cuda(), fused.tables(ang, "f32", "cuda")
    q = hip.rmsnorm_rope(d[..., :c], wq.cuda(), heads, EPS, *cs)
    k = hip.rmsnorm_rope(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    v = d[..., 2 * c:]
    q8, k8, sq, sk, kbar = hip.attn_quant_qk(q, k, heads)
    v8t, sv, _ = hip.attn_quant_vt(v, heads)
    box = tsi.Mailbox(world)
    shards = [RecordShard(box, r, "ulysses") for r in range(world)]
    pend = []
    for s, (lo, hi) in zip(shards, local_ranges(n, world)):      # the send layout sequence_parallel.ulysses_qkv_async fills
        send = s.ulysses_send_buffer(n, c, q, hi - lo)
        for j, t in enumerate((q, k, v)):
            send[:, :hi - lo, j].copy_(t[0, lo:hi].unflatten(-1, (world, g)).transpose(0, 1))
        pend.append(s.ulysses_exchange_async(send, n))
    for r, p in enumerate(pend):
        qg, kg, vg = p.wait()
        assert qg.shape == (1, n, g) and qg.stride(1) == 3 * g
        bufs = hip.attn_quant_qk(qg, kg, 1)
        cols = slice(r * g, (r + 1) * g)
        for name, got, want in (("q8", bufs[0], q8[:, cols]), ("k8", bufs[1], k8[:, cols]), ("sq", bufs[2], sq[:, r:r + 1]),
                                ("sk", bufs[3], sk[r:r + 1]), ("kbar", bufs[4], kbar[cols])):
            assert torch.equal(u8(got), u8(want)), f"head group {r}: {name}"
        if pv8:
            t, s, _ = hip.attn_quant_vt(vg, 1)
            assert torch.equal(u8(t), u8(v8t[r:r + 1])) and torch.equal(s, sv[r:r + 1]), f"head group {r}: v8t / sv"
        want = hip.attention_qk8(q[..., cols], k[..., cols], v[..., cols], 1, pv8=pv8)
        assert torch.equal(hip.attention_qk8(qg, kg, vg, 1, pv8=pv8), want), f"head group {r}: the attention output"


@gpu
def test_entry_points_only_enqueue_and_capture(hip):  # noqa: F811
    """The three entry points (five launches) recorded on a side stream into a graph: nothing runs at capture (the outputs keep their
    fill), a replay gives the bytes of the eager calls."""
    n, heads, rows = 333, 2, 84
    c = heads * 128
    qkv, _, wk, ang = fused.case(n, heads, "normal")
    d = qkv.cuda()
    k, parts = hip.rmsnorm_rope_kstats(d[:, :rows, c:2 * c], wk.cuda(), heads, EPS, *fused.tables(ang[:rows], "f32", "cuda"))
    v = d[:, :rows, 2 * c:]
    others = hip.attn_shard8_neutral_record(c, "cuda")
    want_rec = hip.attn_shard8_stats(parts, rows, heads, v)
    want = hip.attn_shard8_quant(torch.stack([want_rec, others]), rows, k, heads, v)
    want_t = hip.attn_shard8_vt(want[1], heads)
    torch.cuda.synchronize()
    recs = torch.stack([torch.full_like(want_rec, 0x7F), others])
    k8, v8 = torch.full((rows, c), 0x7F, dtype=U8, device="cuda").view(F8), torch.full((rows, c), 0x7F, dtype=U8, device="cuda").view(F8)
    v8t = torch.full((heads, 128, 128), 0x7F, dtype=U8, device="cuda").view(F8)
    scratch = torch.empty(hip.load().fg_attn_shard8_scratch_bytes(rows, c), dtype=U8, device="cuda")
    sk, kbar, sv = (torch.full((m,), -1.0, device="cuda") for m in (heads, c, c))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        s = hip._stream(k)
        hip._call("fg_attn_shard8_stats", hip._ptr(parts), parts.numel(), hip._ptr(v), 3 * c, hip._ptr(recs), 20 * c, hip._ptr(scratch),
                  scratch.numel(), rows, heads, 128, s)
        hip._call("fg_attn_shard8_quant", hip._ptr(recs), recs.numel(), 2, rows, hip._ptr(k), c, hip._ptr(v), 3 * c, hip._ptr(k8), hip._ptr(v8),
                  hip._ptr(sk), hip._ptr(kbar), hip._ptr(sv), rows, heads, 128, s)
        hip._call("fg_attn_shard8_vt", hip._ptr(v8), hip._ptr(v8t), rows, heads, 128, s)
    torch.cuda.synchronize()
    assert all((u8(t) == 0x7F).all() for t in (recs[0], k8, v8, v8t)) and all((t == -1.0).all() for t in (sk, kbar, sv)), "a capture launched work"
    graph.replay()
    torch.cuda.synchronize()
    for name, got, ref in (("record", recs[0], want_rec), ("k8", k8, want[0]), ("v8", v8, want[1]), ("sk", sk, want[2]), ("kbar", kbar, want[3]),
                           ("sv", sv, want[4].view(-1)), ("v8t", v8t, want_t)):
        assert torch.equal(u8(got), u8(ref)), name


# ------------------------------------------------------------------------------------------------------------------ 3. the model
def run_ranks(dit, world, attn_mode, **call):
    """tsi.run_emulated_ranks with shards that have the record exchange."""
    from fairygen_amd.wan_video import model_fn_wan_video_steps, run_interleaved
    box = tsi.Mailbox(world)
    shards = [RecordShard(box, r, attn_mode) for r in range(world)]
    results = run_interleaved([model_fn_wan_video_steps(dit, sequence_shard=s, gather_output=False, **call) for s in shards])
    return dit.unpatchify(torch.cat([out for out, _ in results], dim=1), results[0][1]), box


_whole = {}
MODEL = [("allgather", w) for w in (3, 4, 8)] + [("ulysses", w) for w in (4, 8)]


@gpu
@pytest.mark.parametrize("pv8", [False, True], ids=["qk8", "pv8"])
@pytest.mark.parametrize("attn_mode,world", MODEL, ids=[f"{m}-P{w}" for m, w in MODEL])
def test_emulated_ranks_equal_unsharded_forward(medium, attn_mode, world, pv8):  # noqa: F811
    """The dim-3072, 2-layer model over N = 1 950 tokens, P emulated ranks against the unsharded forward OF THE SAME MODE.  The operand
    bytes are identical, so as in the bf16 case only the k-split and split-KV grouping can differ: the bound is
    tests/test_token_shard_invariance.py's own 2 err_ref + 1e-2.  Every exchange of every block ran: 2 per block in either mode (allgather:
    the records, then k8 with v or v8; ulysses: the two all-to-alls).  No comparison against the fp32 oracle: the accuracy of the mode is
    pinned by tests/test_attention_qk8.py and tests/test_attention_pv8.py.

    Measured on an MI355X: err_ref = 0.03223, bound 0.07446; max|emulated - unsharded| = 0.03125 (one bf16 ulp of a value in [4, 8)) in
    all ten cases of either form.

    The routing goes by the TOTAL key count: every rank holds at most 650 rows, below QK8_MIN_KV, of 1 950 keys, above it, so in both
    exchange modes every rank's self-attention of every block must run the e4m3 forward kernel and fg_attn_fwd_bf16 is left with
    cross-attention alone.  A branch that asked takes_qk8_attention about its local rows fails the counts."""
    from fairygen_amd import wan_video_dit
    from fairygen_amd.wan_video import model_fn_wan_video
    dit = medium.dit
    medium.setting(False, True)
    names, real = [], _hip._call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    try:
        with torch.no_grad():
            if pv8 not in _whole:
                dit.enable_qk8_attention(pv8=pv8)
                _whole[pv8] = model_fn_wan_video(dit, **medium.call).float().cpu()
            dit.enable_qk8_attention(pv8=pv8, sharded=True)
            with pytest.MonkeyPatch.context() as patch:
                patch.setattr(_hip, "_call", call)
                out, box = run_ranks(dit, world, attn_mode, **medium.call)
    finally:
        dit.enable_qk8_attention(False)
    out, want = out.float().cpu(), _whole[pv8]
    assert box.completed == 2 * len(dit.blocks) and not box.slots, "not every exchange of every block ran"
    assert -(-1950 // world) <= wan_video_dit.QK8_MIN_KV < 1950
    assert names.count("fg_attn_fwd_pv8_bf16" if pv8 else "fg_attn_fwd_qk8_bf16") == world * len(dit.blocks), "self-attention routed by the local rows"
    assert names.count("fg_attn_fwd_bf16") == world * len(dit.blocks), "fg_attn_fwd_bf16 ran for more than cross-attention"
    bound = 2 * medium.err_ref + 1e-2
    diff = (out - want).abs().max().item()
    print(f"emulated {attn_mode} P={world} {'pv8' if pv8 else 'qk8'}: max|emulated - unsharded| = {diff:.5f}, err_ref = {medium.err_ref:.5f}, "
          f"bound = {bound:.5f}, max|unsharded| = {want.abs().max().item():.3f}")
    assert torch.isfinite(out).all() and out.shape == want.shape
    assert diff <= bound, f"emulated ranks differ from the unsharded forward of the mode by {diff} (bound {bound})"

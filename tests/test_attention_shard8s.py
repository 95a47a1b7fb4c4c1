"""The e4m3 modes with smoothed V, and the e4m3 cross-attention, on token-sharded layouts (WanModel.enable_qk8_attention(sharded="all"),
include/fairygen_hip_shard8s.h): the kernels and the switch.  The model is tests/test_shard8s_forward.py.

The property: for any partition of the rows [0, N) into W contiguous shards, some empty, in any rank order of the records, the gathered
v8t and every rank's mu and sv are byte for byte what fg_attn_quant_vt_smooth_bf16 writes on the unsharded rows, and k8, sk and the key
mean are the bytes of include/fairygen_hip_shard8.h, where the fp64 sums are exact — asserted on the CPU for the inputs used, per channel:
(largest - smallest exponent of the non-zero |v|) + 8 + ceil(log2 N) <= 52.  Nothing here has a tolerance.

  1. (no GPU) the ABI extension, the argument checks, the routing switch, the exchange of 32 C byte records through the mailbox double.
  2. the kernels: the sharded chain against the unsharded producers on guarded buffers with leading dimensions above C; constant V;
     attention on a shard's queries; the Ulysses head groups; the cross-attention rows; stream capture.
No multi-GPU hardware run exists: the ranks are emulated on one GPU."""
import ctypes
import functools
import itertools
import math
import os
import re

import pytest
import torch

import test_attention_cross8s as cross8s
import test_attention_pv8 as pv8t
import test_attention_qk8 as qk8t
import test_attention_qk8_fused as fused
import test_attention_shard8 as shard8
import test_token_shard_invariance as tsi
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic
from test_attention_qk8 import guarded, guards_intact, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8, U8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.float32
EPS = fused.EPS
NAMES = ("fg_attn_shard8s_stats", "fg_attn_shard8s_quant")
QUERIES = ("fg_attn_shard8s_version", "fg_attn_shard8s_record_bytes", "fg_attn_shard8s_scratch_bytes")
u8 = shard8.u8


# ------------------------------------------------------------------------------------------------------------------ 1. ABI, checks, routing
def test_extension_abi():
    """Fails on the parent commit: the symbols, the header and the binding's tables are this extension's."""
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_shard8s.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55      # the main table is what it was
    tables = (_hip.PV8_SYMBOLS, _hip.SHARD8_SYMBOLS, _hip.CROSS8_SYMBOLS, _hip.BATCH8_SYMBOLS, _hip.ROWBATCH_SYMBOLS, _hip.ROWBATCH8_SYMBOLS,
              _hip.LORABATCH_SYMBOLS, _hip.UP2PHASE_SYMBOLS, _hip.GATEGEMM_SYMBOLS, _hip.SMOOTHV_SYMBOLS, _hip.CROSS8S_SYMBOLS)
    assert [len(t) for t in tables] == [4, 6, 3, 9, 5, 3, 3, 4, 3, 6, 3]
    others = _hip.EXPORTED_SYMBOLS + [s for t in tables for s in t]
    assert not any(name in others for name in NAMES + QUERIES)
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_shard8s.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.SHARD8S_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 5
    assert _hip.SHARD8S_ABI_VERSION == 1 and lib.fg_attn_shard8s_version() == 1
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    V, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    ctype = {"const void*": V, "void*": V, "float*": V, "fg_stream_t": V, "int64_t": I64, "int": I32}
    for name in NAMES:
        args = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        types = [ctype[a.strip().rsplit(" ", 1)[0]] for a in args.replace("\n", " ").split(",")]
        assert types == _hip._SHARD8S_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is I32
    # the shard8 signatures, mu behind sv
    assert _hip._SHARD8S_SIGNATURES[NAMES[0]] == _hip._SHARD8_SIGNATURES["fg_attn_shard8_stats"]
    base = _hip._SHARD8_SIGNATURES["fg_attn_shard8_quant"]
    assert _hip._SHARD8S_SIGNATURES[NAMES[1]] == base[:13] + [V] + base[13:]
    assert _hip._SHARD8S_QUERIES == {QUERIES[0]: (I32, []), QUERIES[1]: (I64, [I32]), QUERIES[2]: (I64, [I64, I32])}
    assert "32 * C" in ext and "fairygen_hip_smoothv.h" in ext and "binades" in ext and "neutral record" in ext
    real = _hip._lib
    try:          # load() checks the version: a library that answers another one is refused
        _hip._lib = None
        _hip.SHARD8S_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="ABI mismatch"):
            _hip.load()
    finally:
        _hip.SHARD8S_ABI_VERSION = 1
        _hip._lib = real


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1)."""
    lib, a = _hip.load(), 4096
    c = 256
    assert lib.fg_attn_shard8s_record_bytes(c) == 32 * c and lib.fg_attn_shard8s_record_bytes(3072) == 98304
    for bad in (0, 200, 4224, -128):
        assert lib.fg_attn_shard8s_record_bytes(bad) == -1 and b"multiple of 128" in lib.fg_last_error()
    assert lib.fg_attn_shard8s_scratch_bytes(84, c) == 6 * c * 16 and lib.fg_attn_shard8s_scratch_bytes(10 ** 6, 3072) == 256 * 3072 * 16
    assert lib.fg_attn_shard8s_scratch_bytes(0, c) == -1 and lib.fg_attn_shard8s_scratch_bytes(5, 100) == -1
    pb = lib.fg_attn_qk8_fused_scratch_bytes(10, c)
    big = 1 << 24

    def stats(partials=a, pbytes=pb, v=a, ldv=c, rec=a, rbytes=32 * c, scr=a, sbytes=big, rows=10, h=2, d=128):
        return lib.fg_attn_shard8s_stats(partials, pbytes, v, ldv, rec, rbytes, scr, sbytes, rows, h, d, None)
    assert stats(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert stats(ldv=c - 8) == -1 and stats(ldv=c + 4) == -1
    assert stats(rbytes=32 * c - 1) == -1 and b"record" in lib.fg_last_error()
    assert stats(pbytes=pb - 1) == -1 and b"partials" in lib.fg_last_error()
    assert stats(sbytes=c * 16 - 1) == -1 and b"scratch" in lib.fg_last_error()
    assert stats(rows=0) == -1 and stats(h=0) == -1 and stats(h=33) == -1
    assert stats(partials=a + 8) == -1 and stats(rec=a + 8) == -1 and stats(v=a + 8) == -1 and stats(scr=a + 8) == -1
    assert stats(partials=None) == -1 and stats(rec=None) == -1
    assert stats(v=None) == -1 and stats(scr=None) == -1                            # v is required: the record is the smoothing form's

    def quant(rec=a, rbytes=4 * 32 * c, w=4, n=40, k=a, ldk=c, v=a, ldv=c, k8=a, v8=a, sk=a, kbar=a, sv=a, mu=a, rows=10, h=2, d=128):
        return lib.fg_attn_shard8s_quant(rec, rbytes, w, n, k, ldk, v, ldv, k8, v8, sk, kbar, sv, mu, rows, h, d, None)
    assert quant(d=64) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert quant(ldk=c - 8) == -1 and quant(ldv=c - 8) == -1 and quant(ldk=c + 4) == -1
    assert quant(rbytes=4 * 32 * c - 1) == -1 and b"records" in lib.fg_last_error()
    assert quant(w=0) == -1 and quant(n=0) == -1 and quant(rows=0) == -1 and quant(h=0) == -1 and quant(h=33) == -1
    assert quant(rows=41) == -1 and b"rows" in lib.fg_last_error()
    for name in ("rec", "k", "v", "kbar", "sv", "mu"):
        assert quant(**{name: a + 8}) == -1, name
    assert quant(k8=a + 4) == -1 and quant(v8=a + 4) == -1 and quant(sk=a + 2) == -1
    for name in ("rec", "k", "v", "k8", "v8", "sk", "kbar", "sv", "mu"):
        assert quant(**{name: None}) == -1 and b"null pointer" in lib.fg_last_error(), name


class Shard:
    active = True


SWITCHES = [dict(zip(("smooth_v", "cross", "smooth_v_cross"), s)) for s in itertools.product((False, True), repeat=3) if s[1] or not s[2]]


def test_sharded_all_sets_the_routing():
    """sharded="all": every e4m3 form that is switched on also runs on an active token shard; True keeps its meaning and its refusals
    (pinned by the existing tests of the three forms); any other value raises; a refused call changes no switch."""
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)
    x = torch.empty((1, 8, 256), device="meta")
    assert len(SWITCHES) == 6
    for kw in SWITCHES:
        assert m.enable_qk8_attention(pv8=True, sharded="all", **kw) is m and m.qk8_sharded == "all"
        assert (m.smoothv_attention, m.cross8_attention, m.smoothv_cross_attention) == (kw["smooth_v"], kw["cross"], kw["smooth_v_cross"])
        m.check_qk8_layout(Shard())
        m.check_qk8_layout(None)
        if not any(kw.values()):
            continue
        m.enable_qk8_attention(pv8=True, **kw)      # without it an active shard raises, as before
        assert m.qk8_sharded is False
        with pytest.raises(NotImplementedError, match="smooth_v=True.*no V sum" if kw["smooth_v"] else "cross=True"):
            m.check_qk8_layout(Shard())
        with pytest.raises(NotImplementedError):
            next(m.forward_tokens_steps(x, x, torch.empty((1, 6, 256), device="meta"), x, 0, (x, x), Shard(), 16))
        if kw["smooth_v"]:
            with pytest.raises(ValueError, match="no V sum"):
                m.enable_qk8_attention(pv8=True, sharded=True, **kw)
        else:
            m.enable_qk8_attention(pv8=True, sharded=True, **kw)
            assert m.qk8_sharded is True
            with pytest.raises(NotImplementedError, match="cross=True"):
                m.check_qk8_layout(Shard())
    # plain qk8 with "all" is the sharded mode
    m.enable_qk8_attention(sharded="all")
    assert m.qk8_sharded == "all" and not m.pv8_attention
    m.check_qk8_layout(Shard())
    full = dict(pv8=True, fused_producer=True, cross=True, smooth_v=True, smooth_v_cross=True, sharded="all")
    m.enable_qk8_attention(**full)
    state = (m.qk8_attention, m.qk8_fused_producer, m.pv8_attention, m.qk8_sharded, m.cross8_attention, m.smoothv_attention, m.smoothv_cross_attention)
    assert state == (True, True, True, "all", True, True, True)
    for bad in ("ALL", "yes", 1, 0, None, 2.0):
        with pytest.raises(ValueError, match="sharded"):
            m.enable_qk8_attention(pv8=True, sharded=bad)
    with pytest.raises(ValueError, match="sharded"):
        m.enable_qk8_attention(False, sharded="all")
    for kw in ({"smooth_v": True}, {"cross": True, "pv8": False}, {"smooth_v_cross": True, "pv8": True}):
        with pytest.raises(ValueError):
            m.enable_qk8_attention(sharded="all", **kw)
    assert state == (m.qk8_attention, m.qk8_fused_producer, m.pv8_attention, m.qk8_sharded, m.cross8_attention, m.smoothv_attention,
                     m.smoothv_cross_attention), "a refused call changes no switch"
    m.enable_qk8_attention(pv8=True)
    assert m.qk8_sharded is False, "an enable without sharded= switches it off"
    m.enable_qk8_attention(**full)
    m.enable_qk8_attention(False)
    assert m.qk8_sharded is False and not m.qk8_attention
    m.check_qk8_layout(Shard())


def test_example_passes_sharded_all():
    """examples/inference.py on a parallel layout: sharded="all" with any of --smooth-v, --cross8-attention, --smooth-v-cross, True without."""
    from examples import inference
    for pv8, cross8, sv, svc in itertools.product((False, True), repeat=4):
        kw = inference.sharded_attention_switches(True, pv8 or cross8 or sv, cross8 or svc, sv, svc)
        assert kw["sharded"] == ("all" if (cross8 or sv or svc) else True), (pv8, cross8, sv, svc)
        assert kw["fused_producer"] is True and kw["cross"] is (cross8 or svc) and kw["smooth_v"] is sv and kw["smooth_v_cross"] is svc


def neutral_cpu(c):
    return _hip.attn_shard8s_neutral_record(c, "cpu")


def test_neutral_record():
    c = 256
    rec = neutral_cpu(c)
    assert rec.shape == (32 * c,) and rec.dtype == U8
    for at in (0, 16 * c):
        assert (rec[at:at + 8 * c].view(torch.float64) == 0).all()
        assert (rec[at + 8 * c:at + 12 * c].view(F32) == float("inf")).all() and (rec[at + 12 * c:at + 16 * c].view(F32) == float("-inf")).all()


@pytest.mark.parametrize("world", [3, 4, 8])
def test_loopback_record_exchange(world):
    """The mailbox double on 32 C byte records, neutral ones among them: every rank receives the W records in rank order."""
    c = 256
    box = tsi.Mailbox(world)
    shards = [shard8.RecordShard(box, r, "allgather") for r in range(world)]
    recs = [torch.randint(0, 256, (32 * c,), dtype=U8, generator=torch.Generator().manual_seed(r)) for r in range(world)]
    recs[1], recs[-1] = neutral_cpu(c), neutral_cpu(c)
    pend = [s.all_gather_records_async(rec) for s, rec in zip(shards, recs)]
    for p in pend:
        got = p.wait()
        assert got.shape == (world, 32 * c) and torch.equal(got, torch.stack(recs))
    assert box.completed == 1 and not box.slots


# ------------------------------------------------------------------------------------------------------------------ 2. the kernels
def sum_bits(v, n):
    """Per channel of the (n, C) bf16 tensor v the bits an exact sum of its rows needs; the largest over the channels."""
    e = torch.frexp(v.float().abs())[1].double()
    zero = v.float() == 0
    spread = e.masked_fill(zero, float("-inf")).amax(0) - e.masked_fill(zero, float("inf")).amin(0)
    spread = torch.nan_to_num(spread, nan=0.0, neginf=0.0)      # a channel of zeros
    return int(spread.max().item()) + 8 + (math.ceil(math.log2(n)) if n > 1 else 0)


def splits(n, world):
    """Uneven contiguous shards of [0, n): a single-row rank, an empty rank, shards that start off the 16-row grid."""
    if world == 3:
        cuts = [0, 1, 1, n]
    else:
        cuts = [0, 1, 1, n // 7 + 3, n // 3 + 5, n // 2 + 1, n // 2 + 1, n - 1, n]
    assert len(cuts) == world + 1 and cuts == sorted(cuts)
    ranges = list(zip(cuts, cuts[1:]))
    assert any(hi == lo for lo, hi in ranges) and any(hi - lo == 1 for lo, hi in ranges) and any(lo % 16 and hi - lo > 16 for lo, hi in ranges)
    return ranges


@functools.lru_cache(maxsize=None)
def chain_case(n, heads, constant=False):
    """fused.case's q | k | v buffer with v = mu_c + eps, mu_c ~ 8 N(0, 1), eps ~ N(0, 1) (constant: v = mu_c for all keys), in bf16."""
    qkv, wq, wk, ang = fused.case(n, heads, "normal")
    c = heads * 128
    qkv = qkv.clone()
    m = 8.0 * seeded((1, c), 7100 + heads, dtype=F32)
    qkv[0, :, 2 * c:] = (m + (0 if constant else seeded((n, c), 7200 + n + heads, dtype=F32))).to(BF16)
    assert sum_bits(qkv[0, :, 2 * c:], n) <= 52, "the fp64 sum of a v channel is not exact: the comparison of mu would not be one"
    return qkv, wq, wk, ang


@functools.lru_cache(maxsize=None)
def unsharded(n, heads, constant=False):
    """The unsharded producers on the device, once: (k8, sk, kbar, v8t, sv, mu, q8, sq)."""
    qkv, wq, wk, ang = chain_case(n, heads, constant)
    c = heads * 128
    d, cs = qkv.cuda(), fused.tables(ang, "f32", "cuda")
    k, parts = _hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    k8, sk, kbar = _hip.attn_quant_k(k, parts, heads)
    v8t, sv, _, mu = _hip.attn_quant_vt(d[..., 2 * c:], heads, smooth=True)
    q8, sq = _hip.rmsnorm_rope_q8(d[..., :c], wq.cuda(), heads, EPS, *cs)
    torch.cuda.synchronize()
    assert fused.exact_sum_bits(k[0].cpu(), n) <= 52, "the fp64 sum of these keys is not exact"
    return k8, sk, kbar, v8t, sv, mu, q8, sq


def sharded_chain(hip, n, heads, ranges, constant=False):  # noqa: F811
    """Every rank's launches on guarded, sentinel-filled outputs, k in a buffer wider than C (ldk = C + 64; ldv = 3 C).  Returns
    (records (W, 32 C), per rank None or (k8, v8, sk, kbar, sv, mu), per rank None or the rank's k and key partials)."""
    qkv, wq, wk, ang = chain_case(n, heads, constant)
    c = heads * 128
    d, wk_d = qkv.cuda(), wk.cuda()
    ks, records, fulls = [], [], []
    for lo, hi in ranges:
        if hi == lo:      # a rank without rows launches nothing
            ks.append(None)
            records.append(hip.attn_shard8s_neutral_record(c, "cuda"))
            continue
        k, parts = hip.rmsnorm_rope_kstats(d[:, lo:hi, c:2 * c], wk_d, heads, EPS, *fused.tables(ang[lo:hi], "f32", "cuda"))
        wide = torch.full((1, hi - lo, c + 64), float("nan"), dtype=BF16, device="cuda")
        wide[..., :c] = k
        full, rec = guarded((1, 32 * c), U8)
        hip.attn_shard8s_stats(parts, hi - lo, heads, d[:, lo:hi, 2 * c:], record=rec.view(-1))
        fulls.append(full)
        ks.append((wide[..., :c], parts))
        records.append(rec.view(-1))
    records = torch.stack(records)
    outs = []
    for (lo, hi), kp in zip(ranges, ks):
        if kp is None:
            outs.append(None)
            continue
        rows = hi - lo
        f, b = zip(*[guarded(s, t) for s, t in (((rows, c), F8), ((rows, c), F8), ((1, heads), F32), ((1, c), F32), ((1, c), F32), ((1, c), F32))])
        v = d[:, lo:hi, 2 * c:]
        hip._call("fg_attn_shard8s_quant", hip._ptr(records), records.numel(), len(ranges), n, hip._ptr(kp[0]), c + 64, hip._ptr(v), 3 * c,
                  *[hip._ptr(t) for t in b], rows, heads, 128, hip._stream(v))
        fulls.extend(f)
        outs.append((b[0], b[1], b[2].view(heads), b[3].view(c), b[4].view(heads, 128), b[5].view(heads, 128)))
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in fulls), "a guard row of an output was written"
    for out in outs:
        assert out is None or not any((u8(t) == qk8t.POISON).all() for t in out), "an output was not written"
    return records, outs, ks


def gathered_vt(hip, outs, heads, n):  # noqa: F811
    v8 = torch.cat([u8(o[1]) for o in outs if o is not None])
    full, v8t = guarded((heads, 128, (n + 63) // 64 * 64), F8)
    hip.attn_shard8_vt(v8, heads, v8t=v8t)
    torch.cuda.synchronize()
    assert guards_intact(full), "a guard row of v8t was written"
    return v8, v8t


CHAIN = [(n, h, w) for n, h in ((1100, 2), (2049, 2), (333, 3)) for w in (3, 8)]


@gpu
@pytest.mark.parametrize("n,heads,world", CHAIN, ids=[f"N{n}-H{h}-W{w}" for n, h, w in CHAIN])
def test_sharded_chain_equals_unsharded(hip, n, heads, world):  # noqa: F811
    """stats per rank -> gather the records -> quant per rank -> concatenate k8, v8 -> attn_shard8_vt, against the unsharded producers and
    against the chain of include/fairygen_hip_shard8.h on the same split; then the records in another rank order."""
    c = heads * 128
    k8_ref, sk_ref, kbar_ref, v8t_ref, sv_ref, mu_ref, _, _ = unsharded(n, heads)
    ranges = splits(n, world)
    records, outs, ks = sharded_chain(hip, n, heads, ranges)
    what = f"N = {n}, W = {world}, {heads} heads: "
    live = [r for r, o in enumerate(outs) if o is not None]
    # the existing chain on the same rows (its record has no V sum: the key half only)
    old_recs = torch.stack([hip.attn_shard8_neutral_record(c, "cuda") if kp is None else hip.attn_shard8_stats(kp[1], hi - lo, heads)
                            for kp, (lo, hi) in zip(ks, ranges)])
    for r in live:
        k8, v8, sk, kbar, sv, mu = outs[r]
        for name, got, want in (("sk", sk, sk_ref), ("kbar", kbar, kbar_ref), ("sv", sv, sv_ref), ("mu", mu, mu_ref)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what + f"rank {r}: {name} differs from the unsharded one"
        for name, i in (("sk", 2), ("kbar", 3), ("sv", 4), ("mu", 5)):
            assert torch.equal(u8(outs[r][i]), u8(outs[live[0]][i])), what + f"ranks {live[0]} and {r} derive different {name} bytes"
        o8, _, osk, okbar, _ = hip.attn_shard8_quant(old_recs, n, ks[r][0], heads)
        assert torch.equal(u8(k8), u8(o8)) and torch.equal(sk, osk) and torch.equal(kbar, okbar), what + f"rank {r}: k8 / sk / kbar differ from attn_shard8_quant's"
    k8 = torch.cat([u8(outs[r][0]) for r in live])
    assert torch.equal(k8, u8(k8_ref)), what + f"{(k8 != u8(k8_ref)).sum().item()} of {k8.numel()} bytes of the gathered k8 differ"
    v8, v8t = gathered_vt(hip, outs, heads, n)
    assert torch.equal(u8(v8t), u8(v8t_ref)), what + f"{(u8(v8t) != u8(v8t_ref)).sum().item()} of {v8t.numel()} bytes of v8t differ"
    nat, pad = pv8t.from_tiles(u8(v8t).cpu(), n)
    assert (pad == 0).all() and torch.equal(nat, v8.cpu()), what + "v8t is not the tile order of the gathered v8 with zero padding"
    # the key half of the record is the existing record's
    assert torch.equal(records[:, :16 * c], old_recs[:, :16 * c]), what + "the key fields differ from attn_shard8_stats's"
    # another rank order of the records: the same scales and bytes
    perm = list(reversed(range(world)))
    r = live[-1]
    lo, hi = ranges[r]
    again = hip.attn_shard8s_quant(records[perm].contiguous(), n, ks[r][0], heads, chain_case(n, heads)[0].cuda()[:, lo:hi, 2 * c:])
    for name, got, want in zip(("k8", "v8", "sk", "kbar", "sv", "mu"), again, outs[r]):
        assert torch.equal(u8(got), u8(want)), what + f"{name} depends on the rank order of the records"


@gpu
def test_outputs_stay_inside_their_buffers(hip):  # noqa: F811
    """record, k8, v8, sk, kbar, sv and mu between poisoned guard rows, ldk = C + 64 and ldv = 3 C: sharded_chain asserts the guards; here
    additionally the columns of the wide k buffer behind C are still what they were, and v was not written."""
    n, heads = 333, 3
    c = heads * 128
    before = chain_case(n, heads)[0].clone()
    _, outs, ks = sharded_chain(hip, n, heads, splits(n, 8))
    for kp in ks:
        assert kp is None or kp[0]._base is not None and torch.isnan(kp[0]._base[..., c:]).all()
    assert torch.equal(chain_case(n, heads)[0], before)


def fwd_s(hip, q8, k8, sq, sk, v8t, sv, mu, heads, split=False):  # noqa: F811
    """fg_attn_fwd_pv8s_bf16 through the C ABI: without a workspace (every q-block one workgroup over all keys), or with the one the
    planner wants for this shape, which must then cut KV ranges."""
    nq, nkv, c = q8.shape[0], k8.shape[0], heads * 128
    out = torch.empty((nq, c), dtype=BF16, device="cuda")
    ws, need = None, 0
    if split:
        need = hip.load().fg_attn_workspace_bytes(1, nq, nkv, heads)
        R, S = ctypes.c_int(), ctypes.c_int()
        assert hip.load().fg_attn_split_choice(1, nq, nkv, heads, need, ctypes.byref(R), ctypes.byref(S)) == 0
        assert need > 0 and S.value > 1, "with a workspace this shape is meant to take the split-KV path"
        ws = torch.empty(need, dtype=U8, device="cuda")
    hip._call("fg_attn_fwd_pv8s_bf16", *[hip._ptr(t) for t in (q8, k8, sq, sk, v8t, sv, mu)], hip._ptr(out), nq, nkv, heads, 128, 128 ** -0.5,
              hip._ptr(ws), need, hip._stream(out))
    return out


@gpu
@pytest.mark.parametrize("n,split", [(1100, False), (2049, True)], ids=["1100-direct", "2049-split-kv"])
def test_constant_v_comes_back_bit_for_bit(hip, n, split):  # noqa: F811
    """v[j][c] = m_c for all keys through the sharded chain: every rank's mu is m_c, v8 is zero, sv the floor, and attention on one
    shard's queries returns m_c bit for bit."""
    heads, world = 2, 3
    c = heads * 128
    ranges = [(0, n // 3 + 5), (n // 3 + 5, n // 3 + 5), (n // 3 + 5, n)]
    _, outs, _ = sharded_chain(hip, n, heads, ranges, constant=True)
    m = chain_case(n, heads, True)[0][0, :1, 2 * c:]
    for out in outs:
        assert out is None or (torch.equal(out[5].cpu().view(1, c), m.float()) and (u8(out[1]) == 0).all() and (out[4] == qk8t.FLOOR_SCALE).all())
    _, v8t = gathered_vt(hip, outs, heads, n)
    assert (u8(v8t) == 0).all()
    k8 = torch.cat([u8(o[0]) for o in outs if o is not None]).view(F8)
    q8, sq = unsharded(n, heads, True)[6:]
    lo, hi = ranges[2]
    got = fwd_s(hip, q8[lo:hi], k8, sq[lo:hi], outs[0][2], v8t, outs[0][4], outs[0][5], heads, split)
    torch.cuda.synchronize()
    bad = (got.cpu() != m).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {hi - lo} rows differ from m_c, first {bad[:8].tolist()}"


@gpu
def test_attention_on_a_shards_queries(hip):  # noqa: F811
    """attention_pv8_pre(q8[lo:hi], ..., mu=mu) on the gathered operands of the sharded chain equals rows [lo, hi) of the unsharded
    attention_qk8(pv8=True, smooth=True), both without a workspace, under the condition test_attention_shard8.py holds the pv8 form to: no
    wave takes its deferred rescale (max |scaled base-2 logit| <= PV8_DEFER_LOG2 / 2).  The shards: off the 64-row q-block grid, and one
    row."""
    n, heads, world, qkv, wq, wk, ang = shard8.small_logit_case()
    c = heads * 128
    qkv = qkv.clone()
    qkv[0, :, 2 * c:] = (8.0 * seeded((1, c), 7300, dtype=F32) + seeded((n, c), 7301, dtype=F32)).to(BF16)
    assert sum_bits(qkv[0, :, 2 * c:], n) <= 52
    d, wq_d, wk_d = qkv.cuda(), wq.cuda(), wk.cuda()
    ranges = [(0, 367), (367, 368), (368, 368), (368, n)]
    recs, ks, q8s, sqs = [], [], [], []
    for lo, hi in ranges:
        if hi == lo:
            recs.append(hip.attn_shard8s_neutral_record(c, "cuda"))
            continue
        cs = fused.tables(ang[lo:hi], "f32", "cuda")
        k, parts = hip.rmsnorm_rope_kstats(d[:, lo:hi, c:2 * c], wk_d, heads, EPS, *cs)
        recs.append(hip.attn_shard8s_stats(parts, hi - lo, heads, d[:, lo:hi, 2 * c:]))
        q8, sq = hip.rmsnorm_rope_q8(d[:, lo:hi, :c], wq_d, heads, EPS, *cs)
        ks.append(k), q8s.append(q8), sqs.append(sq)
    recs = torch.stack(recs)
    live = [r for r in ranges if r[1] > r[0]]
    assert fused.exact_sum_bits(torch.cat([k[0] for k in ks]).cpu(), n) <= 52, "the fp64 sum of these keys is not exact"
    quant = [hip.attn_shard8s_quant(recs, n, k, heads, d[:, lo:hi, 2 * c:]) for k, (lo, hi) in zip(ks, live)]
    k8 = torch.cat([u8(x[0]) for x in quant]).view(F8)
    v8t = hip.attn_shard8_vt(torch.cat([u8(x[1]) for x in quant]), heads)
    sk, sv, mu = quant[0][2], quant[0][4], quant[0][5]
    # the unsharded call: the fused producers' operands (the bytes of the two-step form), the smoothing V producer, no workspace
    cs = fused.tables(ang, "f32", "cuda")
    kf, parts = hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk_d, heads, EPS, *cs)
    k8_u, sk_u, _ = hip.attn_quant_k(kf, parts, heads)
    q8_u, sq_u = hip.rmsnorm_rope_q8(d[..., :c], wq_d, heads, EPS, *cs)
    v8t_u, sv_u, _, mu_u = hip.attn_quant_vt(d[..., 2 * c:], heads, smooth=True)
    whole = fwd_s(hip, q8_u, k8_u, sq_u, sk_u, v8t_u, sv_u, mu_u, heads)
    parts_out = [fwd_s(hip, q8, k8, sq, sk, v8t, sv, mu, heads) for q8, sq in zip(q8s, sqs)]
    torch.cuda.synchronize()
    s2 = 128 ** -0.5 * math.log2(math.e)
    a = (q8_u.cpu().float().view(n, heads, 128) * sq_u.cpu().unsqueeze(-1)).double()
    b = (k8_u.cpu().float().view(n, heads, 128) * sk_u.cpu().view(1, heads, 1)).double()
    peak = (s2 * torch.einsum("qhd,khd->hqk", a, b)).abs().max().item()
    print(f"pv8 smoothed: max |scaled base-2 logit| = {peak:.3f} (limit {_hip.PV8_DEFER_LOG2 / 2})")
    assert peak <= _hip.PV8_DEFER_LOG2 / 2
    assert torch.isfinite(whole.float()).all()
    for (lo, hi), p in zip(live, parts_out):
        tsi.assert_same_rows(p, whole, lo, hi, f"smoothed pv8 attention on the queries of shard [{lo}, {hi})")


@gpu
def test_ulysses_head_groups_equal_unsharded_columns(hip):  # noqa: F811
    """W = 3, one head per rank, N = 1 100: the smoothing twin of test_attention_shard8.py's test — a head group's operands and output are
    the columns of the all-heads call, every statistic being per head and channel."""
    n, heads, world, qkv, wq, wk, ang = shard8.small_logit_case()
    c, g = heads * 128, 128
    qkv = qkv.clone()
    qkv[0, :, 2 * c:] = (8.0 * seeded((1, c), 7300, dtype=F32) + seeded((n, c), 7301, dtype=F32)).to(BF16)
    d, cs = qkv.cuda(), fused.tables(ang, "f32", "cuda")
    q = hip.rmsnorm_rope(d[..., :c], wq.cuda(), heads, EPS, *cs)
    k = hip.rmsnorm_rope(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    v = d[..., 2 * c:]
    v8t, sv, _, mu = hip.attn_quant_vt(v, heads, smooth=True)
    want = hip.attention_qk8(q, k, v, heads, pv8=True, smooth=True)
    for r in range(world):
        cols = slice(r * g, (r + 1) * g)
        t, s, _, m = hip.attn_quant_vt(v[..., cols], 1, smooth=True)
        assert torch.equal(u8(t), u8(v8t[r:r + 1])) and torch.equal(s, sv[r:r + 1]) and torch.equal(m, mu[r:r + 1]), f"head group {r}: v8t / sv / mu"
        got = hip.attention_qk8(q[..., cols], k[..., cols], v[..., cols], 1, pv8=True, smooth=True)
        assert torch.equal(got, want[..., cols]), f"head group {r}: the attention output"


CROSS_SHARDS = [(0, 100), (97, 103), (99, 100), (1, 333)]


@gpu
@pytest.mark.parametrize("smooth", [False, True], ids=["cross8", "cross8s"])
@pytest.mark.parametrize("nkv,data", [(512, "normal"), (77, "normal"), (512, "padded")], ids=["512", "77", "512-padded"])
def test_cross_attention_rows(hip, nkv, data, smooth):  # noqa: F811
    """The context is whole on every rank and the kernel is row-wise in the queries: a shard's queries give that shard's rows.  padded:
    40 text rows and one repeated row behind them (tests/test_attention_cross8s.py).  Bit-equality of a row with the same row of another
    launch holds under the condition of test_attention_on_a_shards_queries, asserted here on the dequantised logits: no wave takes its
    deferred rescale, whichever rows share it (q ~ N(0, 1) / 8, exact in bf16; with q ~ N(0, 1) the rows 96 .. 99 of the shard [0, 100)
    differ from the full call's, which rescales them together with the rows behind them — either is a valid evaluation, and the
    model-level test holds such logits to the forward's bound)."""
    heads, nq = cross8s.ACC_HEADS, 333
    q, k = (seeded((nq, heads * 128), 7400, dtype=F32) / 8).to(BF16), seeded((nkv, heads * 128), 7401)
    v = cross8s.padded_context_v(40, nkv, heads) if data == "padded" else seeded((nkv, heads * 128), 7402)
    q8, k8, sq, sk, v8t, sv, *mu = cross8s.quantise(hip, q, k, v, heads, smooth=smooth)
    mu = mu[0] if smooth else None
    a = (q8.cpu().float().view(nq, heads, 128) * sq.cpu().view(nq, heads, 1)).double()
    b = (k8.cpu().float().view(nkv, heads, 128) * sk.cpu().view(1, heads, 1)).double()
    peak = (128 ** -0.5 * math.log2(math.e) * torch.einsum("qhd,khd->hqk", a, b)).abs().max().item()
    assert peak <= _hip.PV8_DEFER_LOG2 / 2, f"max |scaled base-2 logit| = {peak:.3f}: a wave may take its deferred rescale"
    whole = hip.attention_cross8_pre(q8, k8, sq, sk, v8t, sv, heads, mu=mu)
    assert torch.isfinite(whole.float()).all()
    for lo, hi in CROSS_SHARDS:
        got = hip.attention_cross8_pre(q8[lo:hi], k8, sq[lo:hi], sk, v8t, sv, heads, mu=mu)
        tsi.assert_same_rows(got, whole, lo, hi, f"e4m3 cross-attention ({nkv} keys, {data}, mu {smooth}) on the queries [{lo}, {hi})")


@gpu
def test_entry_points_only_enqueue_and_capture(hip):  # noqa: F811
    """The two entry points (four launches) recorded on a side stream into a graph: nothing runs at capture (the outputs keep their
    fill), a replay gives the bytes of the eager calls."""
    n, heads, rows = 333, 2, 84
    c = heads * 128
    qkv, _, wk, ang = chain_case(n, heads)
    d = qkv.cuda()
    k, parts = hip.rmsnorm_rope_kstats(d[:, :rows, c:2 * c], wk.cuda(), heads, EPS, *fused.tables(ang[:rows], "f32", "cuda"))
    v = d[:, :rows, 2 * c:]
    others = hip.attn_shard8s_neutral_record(c, "cuda")
    want_rec = hip.attn_shard8s_stats(parts, rows, heads, v)
    want = hip.attn_shard8s_quant(torch.stack([want_rec, others]), rows, k, heads, v)
    torch.cuda.synchronize()
    recs = torch.stack([torch.full_like(want_rec, 0x7F), others])
    k8, v8 = (torch.full((rows, c), 0x7F, dtype=U8, device="cuda").view(F8) for _ in range(2))
    scratch = torch.empty(hip.load().fg_attn_shard8s_scratch_bytes(rows, c), dtype=U8, device="cuda")
    sk, kbar, sv, mu = (torch.full((m,), -1.0, device="cuda") for m in (heads, c, c, c))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        s = hip._stream(k)
        hip._call("fg_attn_shard8s_stats", hip._ptr(parts), parts.numel(), hip._ptr(v), 3 * c, hip._ptr(recs), 32 * c, hip._ptr(scratch),
                  scratch.numel(), rows, heads, 128, s)
        hip._call("fg_attn_shard8s_quant", hip._ptr(recs), recs.numel(), 2, rows, hip._ptr(k), c, hip._ptr(v), 3 * c, hip._ptr(k8), hip._ptr(v8),
                  hip._ptr(sk), hip._ptr(kbar), hip._ptr(sv), hip._ptr(mu), rows, heads, 128, s)
    torch.cuda.synchronize()
    assert all((u8(t) == 0x7F).all() for t in (recs[0], k8, v8)) and all((t == -1.0).all() for t in (sk, kbar, sv, mu)), "a capture launched work"
    graph.replay()
    torch.cuda.synchronize()
    for name, got, ref in (("record", recs[0], want_rec), ("k8", k8, want[0]), ("v8", v8, want[1]), ("sk", sk, want[2]), ("kbar", kbar, want[3]),
                           ("sv", sv, want[4].view(-1)), ("mu", mu, want[5].view(-1))):
        assert torch.equal(u8(got), u8(ref)), name

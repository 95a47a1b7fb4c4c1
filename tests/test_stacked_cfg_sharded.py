"""The stacked CFG forward on token shards of the K / V all-gather layout (WanModel.enable_stacked_cfg(sharded=True)): a merged CFG call
on an active shard with cfg_parallel=1 runs ONE stacked forward on the rank's rows, every exchange of a stacked block carrying both
elements.  The kernels are tests/test_attention_shard8b.py.

  CPU: the refusal matrix of check_stacked_cfg; the batched exchanges of the real TokenShard over gloo (worlds 2 and 3, a short rank and an
       empty one) against the B = 1 exchange of each element; an inactive shard is the identity on batched inputs.
  GPU: the dim-3072 model of tests/test_token_shard_invariance.py with emulated ranks on one GPU — against the unsharded stacked forward
       with the same switches, with the launches counted; and, with the calls whose plan depends on the row count made per element,
       bit for bit against the element-by-element merged call on the same emulated ranks.
No multi-GPU hardware run exists."""
import os
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_stacked_cfg_forward as scf
import test_token_shard_invariance as tsi
from conftest import seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic
from fairygen_amd.sequence_parallel import TokenShard
from test_attention_shard8 import RecordShard
from test_token_shard_invariance import medium  # noqa: F401  (the module fixture)

gpu = pytest.mark.gpu
U8 = torch.uint8


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def _shard(mode, active=True):
    return types.SimpleNamespace(active=active, attn_mode=mode)


def test_refusal_matrix():
    from fairygen_amd import ModelConfig
    from fairygen_amd.wan_video_dit import WanModel
    with torch.device("meta"):
        m = WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.stacked_cfg_sharded is False
    m.enable_stacked_cfg()
    with pytest.raises(NotImplementedError, match="stacked_cfg with an active token shard: the stacked forward has no exchange"):
        m.check_stacked_cfg(2, _shard("allgather"))
    with pytest.raises(NotImplementedError, match="active token shard"):      # the shard of the existing test: no attn_mode is looked at
        m.check_stacked_cfg(2, types.SimpleNamespace(active=True))
    assert m.enable_stacked_cfg(sharded=True) is m and m.stacked_cfg_sharded is True and m.stacked_cfg is True
    m.check_stacked_cfg(2, _shard("allgather"))
    m.check_stacked_cfg(2, _shard("ulysses", active=False))
    m.check_stacked_cfg(2, None)
    with pytest.raises(NotImplementedError, match="attn_mode='ulysses'.*no batched form"):
        m.check_stacked_cfg(2, _shard("ulysses"))
    with pytest.raises(NotImplementedError, match="attn_mode='windows'"):
        m.check_stacked_cfg(2, _shard("windows"))
    with pytest.raises(NotImplementedError, match="sliding windows"):
        m.check_stacked_cfg(2, _shard("allgather"), sliding_window=True)
    for batch in (1, 3):
        with pytest.raises(NotImplementedError, match=f"context batch of 2, not {batch}"):
            m.check_stacked_cfg(batch, _shard("allgather"))
    # stated with every call: a call that does not restate it clears it, like fp8_linear, hot_lora and periodic_gate
    m.enable_stacked_cfg(periodic_gate=True)
    assert m.stacked_cfg_sharded is False and m.stacked_cfg_periodic_gate is True
    with pytest.raises(NotImplementedError, match="active token shard"):
        m.check_stacked_cfg(2, _shard("allgather"))
    m.enable_stacked_cfg(fp8_linear=True, hot_lora=True, periodic_gate=True, sharded=True)
    assert (m.stacked_cfg_fp8, m.stacked_cfg_hot_lora, m.stacked_cfg_periodic_gate, m.stacked_cfg_sharded) == (True,) * 4
    m.enable_stacked_cfg(False, sharded=True)
    assert m.stacked_cfg_sharded is False and m.stacked_cfg is False
    # the composition that is not carried: unfused adapters on a shard
    m.enable_stacked_cfg(hot_lora=True, sharded=True)
    m.hot_lora_backend, m.hot_loras = "hip", {"blocks.0.self_attn.q": [None]}
    m.check_stacked_cfg(2, None)
    with pytest.raises(NotImplementedError, match="sharded=True.*hot-loaded adapters"):
        m.check_stacked_cfg(2, _shard("allgather"))
    m.hot_loras = {}
    # ... and the fp8 Linears together with any e4m3 attention form on a shard; each of the two alone passes, and so do both unsharded
    m.enable_stacked_cfg(fp8_linear=True, sharded=True)
    m.fp8_dtype = torch.float8_e4m3fn
    m.check_stacked_cfg(2, _shard("allgather"))
    for kw in (dict(sharded=True), dict(pv8=True, sharded=True), dict(pv8=True, cross=True, smooth_v=True, smooth_v_cross=True, sharded="all")):
        m.enable_qk8_attention(**kw)
        m.check_stacked_cfg(2, None)
        with pytest.raises(NotImplementedError, match="enable_fp8_linear AND enable_qk8_attention.*not carried on token shards"):
            m.check_stacked_cfg(2, _shard("allgather"))
        m.fp8_dtype = None
        m.check_stacked_cfg(2, _shard("allgather"))
        m.fp8_dtype = torch.float8_e4m3fn
    m.enable_qk8_attention(False)
    m.fp8_dtype = None
    # the loader's switch
    assert ModelConfig(path="x").stacked_cfg_sharded is False
    assert ModelConfig(path="x", stacked_cfg=True, stacked_cfg_sharded=True).vram_config()["stacked_cfg_sharded"] is True
    with pytest.raises(ValueError, match="stacked_cfg_sharded=True.*needs stacked_cfg=True"):
        ModelConfig(path="x", stacked_cfg_sharded=True).check_input()


def test_merged_call_on_a_shard_raises_as_before_without_the_switch():
    """Host tensors: every refusal is decided before anything touches a device.  cfg_parallel=2 with cfg_merge, graph=True with a shard
    and TeaCache raise where they always did, with the switch on."""
    from fairygen_amd.wan_video import TeaCache, model_fn_wan_video
    m, _ = scf._model(synthetic.TINY_DIT_KWARGS, 1234, "cpu")
    lat, ctx_p, ctx_n, _, ts = scf._tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    call = lambda **kw: model_fn_wan_video(m, **{**dict(latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=True), **kw})      # noqa: E731
    m.enable_stacked_cfg(sharded=True)
    with pytest.raises(NotImplementedError, match="ulysses"):
        call(sequence_shard=_shard("ulysses"))
    with pytest.raises(NotImplementedError, match="TeaCache is per CFG branch"):
        call(sequence_shard=_shard("allgather"), tea_cache=TeaCache(3, 0.1, "Wan2.1-T2V-1.3B"))
    with pytest.raises(NotImplementedError, match="not recorded into a graph"):
        call(sequence_shard=_shard("allgather"), owned=object())
    m.enable_stacked_cfg()
    with pytest.raises(NotImplementedError, match="active token shard"):
        call(sequence_shard=_shard("allgather"))


# ------------------------------------------------------------------------------------------------------------------ CPU: the exchanges
def _gloo_worker(rank, world, port, result_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = TokenShard()
        b, c = 2, 16
        for n in (7, 2) if world == 3 else (7,):      # 7: a short last rank (4 | 3, or 3 | 3 | 1); 2 at W = 3: the last rank is empty
            lo, hi = shard.local_range(n)
            assert (n, world, rank) != (2, 3, 2) or hi == lo
            k = torch.randint(0, 256, (b, n, c), dtype=U8, generator=torch.Generator().manual_seed(7))
            v = seeded((b, n, 3 * c), 3)[..., 2 * c:]      # a strided slice, like the fused qkv buffer
            want = [shard.all_gather_kv(k[e:e + 1, lo:hi], v[e:e + 1, lo:hi], n) for e in range(b)]
            for kf, vf in (shard.all_gather_kv(k[:, lo:hi], v[:, lo:hi], n), shard.all_gather_kv_async(k[:, lo:hi], v[:, lo:hi], n).wait()):
                assert kf.shape == (b, n, c) and vf.shape == (b, n, c) and kf.dtype == U8
                for e in range(b):
                    assert torch.equal(kf[e:e + 1], want[e][0]) and torch.equal(vf[e:e + 1], want[e][1])
                assert torch.equal(kf, k) and torch.equal(vf, v)
            kf, _ = shard.all_gather_kv_async(k[:, lo:hi], v[:, lo:hi], n).wait()
            assert kf.stride(0) == world * shard.chunk(n) * c, "the views of the slab: elements world * chunk rows apart"
            dense = shard.tokens_of(kf._base if kf._base is not None else kf, n)
            assert dense.is_contiguous() and torch.equal(dense, k)
            x = seeded((b, n, c), 5)
            got = shard.all_gather_tokens(x[:, lo:hi], n)
            assert got.is_contiguous() and torch.equal(got, x)
            assert all(torch.equal(got[e:e + 1], shard.all_gather_tokens(x[e:e + 1, lo:hi], n)) for e in range(b))
        recs = [torch.randint(0, 256, (b, 40), dtype=U8, generator=torch.Generator().manual_seed(r)) for r in range(world)]
        pend_a = shard.all_gather_records_async(recs[rank])
        pend_b = shard.all_gather_records_async(recs[rank].flip(1))      # two in flight
        got = pend_a.wait()
        assert got.shape == (world, b, 40) and torch.equal(got, torch.stack(recs)) and torch.equal(pend_b.wait(), torch.stack(recs).flip(2))
        for e in range(b):
            assert torch.equal(got[:, e], shard.all_gather_records_async(recs[rank][e]).wait())
        open(os.path.join(result_dir, f"ok{rank}"), "w").close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,port", [(2, 29671), (3, 29673)])
def test_batched_exchanges_gloo(tmp_path, world, port):
    """The real TokenShard on CPU tensors: the batched all_gather_kv / all_gather_kv_async / all_gather_records_async /
    all_gather_tokens return, per element, exactly what the B = 1 exchange returns for that element."""
    mp.spawn(_gloo_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / f"ok{r}") for r in range(world))


def test_inactive_shard_is_the_identity_on_batched_inputs():
    s = TokenShard()
    assert not s.active
    k, v, rec = seeded((2, 5, 8), 1), seeded((2, 5, 24), 2)[..., 16:], torch.arange(80, dtype=U8).view(2, 40)
    for kf, vf in (s.all_gather_kv(k, v, 5), s.all_gather_kv_async(k, v, 5).wait()):
        assert kf.shape == (2, 5, 8) and torch.equal(kf, k) and torch.equal(vf, v)
    assert torch.equal(s.all_gather_records_async(rec).wait(), rec.unsqueeze(0))
    assert torch.equal(s.all_gather_records_async(rec[0]).wait(), rec[0].unsqueeze(0))
    assert s.all_gather_tokens(k, 5) is k


# ------------------------------------------------------------------------------------------------------------------ GPU: emulated ranks
class BatchShard(RecordShard):
    """RecordShard whose exchanges also take the batched deposits of a stacked forward: (B, rows, C) rows and (B, bytes) records.  The rows
    come back as the product's exchange hands them back — views [:, :N] of a slab whose elements lie world * chunk rows apart — unless
    `cuts` gives the ranks other row ranges than the ceil split (an empty rank in the middle), where they are concatenated."""

    def __init__(self, box, rank, attn_mode, cuts=None):
        super().__init__(box, rank, attn_mode)
        self.cuts = cuts

    def local_range(self, n, rank=None):
        rank = self.rank if rank is None else rank
        return (self.cuts[rank], self.cuts[rank + 1]) if self.cuts else super().local_range(n, rank)

    def all_gather_kv_async(self, k, v, n):
        if k.shape[0] == 1:
            return super().all_gather_kv_async(k, v, n)
        return _LoopBatchKV(self, self._post("kv", (k, v)), n)

    def all_gather_records_async(self, record):
        if record.dim() == 1:
            return super().all_gather_records_async(record)
        return _LoopBatchRecords(self, self._post("rec", record.contiguous()))


class _LoopBatchKV:
    def __init__(self, shard, key, n):
        self.shard, self.key, self.n = shard, key, n

    def wait(self):
        items, n = self.shard.box.collect(self.key), self.n
        assert sum(k.shape[1] for k, _ in items) == n and len({k.shape[0] for k, _ in items}) == 1
        out = []
        for j in (0, 1):
            rows = torch.cat([it[j] for it in items], dim=1)
            if self.shard.cuts:
                out.append(rows)
                continue
            slab = rows.new_zeros((rows.shape[0], self.shard.world_size * self.shard.chunk(n), rows.shape[2]))
            slab[:, :n] = rows
            out.append(slab[:, :n])
        return tuple(out)


class _LoopBatchRecords:
    def __init__(self, shard, key):
        self.shard, self.key = shard, key

    def wait(self):
        items = self.shard.box.collect(self.key)
        assert len({(tuple(t.shape), t.dtype) for t in items}) == 1
        return torch.stack(items)      # (W, B, bytes)


def run_stacked_ranks(dit, world, cuts=None, shard_cls=BatchShard, **call):
    """P generators of the merged call, one per emulated rank, advanced in turns; the (2, ...) prediction from the ranks' head outputs."""
    from fairygen_amd.wan_video import model_fn_wan_video_steps, run_interleaved
    box = tsi.Mailbox(world)
    shards = [shard_cls(box, r, "allgather", cuts) if shard_cls is BatchShard else shard_cls(box, r, "allgather") for r in range(world)]
    results = run_interleaved([model_fn_wan_video_steps(dit, sequence_shard=s, gather_output=False, **call) for s in shards])
    grid = results[0][1]
    n = grid[0] * grid[1] * grid[2]
    for s, (out, g) in zip(shards, results):
        lo, hi = s.local_range(n)
        assert g == grid and out.shape[:2] == (2, hi - lo), (s.rank, out.shape, (lo, hi))
    return dit.unpatchify(torch.cat([out for out, _ in results], dim=1), grid), box


FORMS = {
    "bf16": None,
    "pv8": dict(pv8=True, fused_producer=True, sharded=True),
    "full": dict(pv8=True, fused_producer=True, cross=True, smooth_v=True, smooth_v_cross=True, sharded="all"),
}
N = 1950
CUTS = (0, 975, 975, N)      # the middle rank is empty
# (attention form, world, cuts, fp8_linear, periodic_gate)
CASES = [(form, 3, cuts, False, False) for form in FORMS for cuts in (None, CUTS)] + [
    ("pv8", 4, None, False, False),       # chunk 488, 4 * 488 = 1 952 != N: the gathered slab has padding rows (k8 compacted, v8 read strided)
    ("bf16", 4, None, False, False),
    ("bf16", 3, None, True, False),       # the compositions the implementation takes: the fp8 Linear mode ...
    ("bf16", 3, None, False, True)]       # ... and the periodic gate (rows_per_element = n_local = 650); fp8 Linears without adapters have
#                                           no gated GEMM store, so periodic_gate has nothing to replace there
# Not a case, because the forward refuses it (check_stacked_cfg; test_refusal_matrix asserts the raise): the fp8 Linears TOGETHER with an
# e4m3 attention form on a shard.  With the full stack it measured max|emulated - unsharded stacked| = 0.11914 on an MI355X (P = 3) against
# this bound of 0.07446; the cause has not been established, and fp8 Linears with qk8 / pv8 alone were never run.
_whole = {}


def _settings(dit, form, fp8, periodic, sharded):
    dit.enable_fp8_linear(torch.float8_e4m3fn if fp8 else None)
    if FORMS[form] is None:
        dit.enable_qk8_attention(False)
    else:
        dit.enable_qk8_attention(**FORMS[form])
    dit.enable_stacked_cfg(fp8_linear=fp8, periodic_gate=periodic, sharded=sharded)


@gpu
@pytest.mark.parametrize("form,world,cuts,fp8,periodic", CASES,
                         ids=[f"{f}-P{w}" + ("-emptyrank" if c else "") + ("-fp8" if f8 else "") + ("-periodic" if p else "") for f, w, c, f8, p in CASES])
def test_emulated_ranks_equal_unsharded_stacked_forward(medium, form, world, cuts, fp8, periodic):  # noqa: F811
    """The dim-3072, 2-layer model over N = 1 950 tokens, TI2V: the merged call with enable_stacked_cfg(sharded=True) on P emulated ranks of
    the K / V all-gather layout against the unsharded stacked forward with the same switches; bound 2 err_ref + 1e-2, that of
    tests/test_token_shard_invariance.py.  Fails without the feature (the parent commit refuses the call).

    The structure, from the calls by name.  Exchanges: one per block in bf16, two with the e4m3 forms, each carrying both elements.
    Block 0's shared self-attention half runs once per rank with B = 1; in every later block a rank with rows runs ONE batched
    self-attention launch and no single-element one, the _b shard producers once each, and its q | k | v Linear as ONE GEMM on
    2 n_local rows.  A rank without rows launches no kernel at all.

    Measured on an MI355X: err_ref = 0.03223, bound 0.07446; max|emulated - unsharded stacked| = 0.03125 (one bf16 ulp of a value in
    [4, 8)) in the bf16 and pv8 cases (P = 3, P = 4, the empty rank, the periodic gate), 0.06250 / 0.05469 in the full stack (P = 3 / the
    empty rank), 0.07422 with the fp8 Linears (a one-ulp flip that crosses an e4m3 rounding boundary of a later Linear's input, as in
    tests/test_token_shard_invariance.py's fp8 case)."""
    from fairygen_amd import wan_video_dit as D
    from fairygen_amd.wan_video import model_fn_wan_video
    dit, layers = medium.dit, len(medium.dit.blocks)
    call = dict(medium.call, context=torch.cat([medium.call["context"], seeded((1, 24, 256), 8).cuda()], 0))
    calls, gemms, real = [], [], _hip._call
    try:
        with torch.no_grad():
            key = (form, fp8, periodic)
            if key not in _whole:
                _settings(dit, form, fp8, periodic, False)
                _whole[key] = model_fn_wan_video(dit, **call).float().cpu()
            _settings(dit, form, fp8, periodic, True)
            with pytest.MonkeyPatch.context() as patch:
                patch.setattr(_hip, "_call", lambda name, *args: (calls.append((name, args)), real(name, *args))[1])
                for seam in ("gemm_bias", "gemm_bias_own"):
                    patch.setattr(D, seam, (lambda inner: lambda x, w, b, **kw: (gemms.append((x.numel() // x.shape[-1], w.shape[0])), inner(x, w, b, **kw))[1])(getattr(D, seam)))
                patch.setattr(D, "gemm_fp8_own", (lambda inner: lambda xq, sa, w8, b, **kw: (gemms.append((xq.shape[0], w8.shape[0])), inner(xq, sa, w8, b, **kw))[1])(D.gemm_fp8_own))
                out, box = run_stacked_ranks(dit, world, cuts, **call)
    finally:
        dit.enable_stacked_cfg(False)
        dit.enable_qk8_attention(False)
        medium.setting(False, True)
    out, want = out.float().cpu(), _whole[key]
    assert want.shape[0] == 2 and not torch.equal(want[0], want[1])
    e4m3 = form != "bf16"
    assert box.completed == layers * (2 if e4m3 else 1) and not box.slots, "the exchanges per block grew, or one did not run"
    probe = BatchShard(tsi.Mailbox(world), 0, "allgather", cuts)
    locals_ = [hi - lo for lo, hi in (probe.local_range(N, r) for r in range(world))]
    working = sum(1 for r in locals_ if r)
    assert working == (2 if cuts else world)
    names = [nm for nm, _ in calls]
    later = working * (layers - 1)      # (rank with rows, block behind block 0)
    if not e4m3:
        batches = [a[7] for nm, a in calls if nm == "fg_attn_fwd_bf16"]      # self- and cross-attention: the batch argument
        assert batches.count(1) == working and batches.count(2) == later + working * layers, "one batched attention launch per block and rank"
    else:
        s = "s" if form == "full" else ""
        assert names.count(f"fg_attn_fwd_pv8{s}_bf16") == working and names.count(f"fg_attn_fwd_pv8{s}_bf16_b") == later
        assert not any(nm in names for nm in ("fg_attn_fwd_qk8_bf16", "fg_attn_fwd_qk8_bf16_b", "fg_attn_fwd_pv8" + ("" if s else "s") + "_bf16_b"))
        for stem in (f"fg_attn_shard8{s}_stats", f"fg_attn_shard8{s}_quant", "fg_attn_shard8_vt"):
            assert names.count(stem) == working and names.count(stem + "_b") == later, f"{stem}: the _b producer once per working rank and block"
        if form == "full":      # cross-attention in the e4m3 form too, batched in every block; the bf16 kernel is not launched
            assert names.count("fg_attn_fwd_cross8s_bf16_b") == working * layers and "fg_attn_fwd_bf16" not in names
        else:
            assert [a[7] for nm, a in calls if nm == "fg_attn_fwd_bf16"] == [2] * (working * layers)
    qkv = [rows for rows, n_out in gemms if n_out == 3 * 3072]
    assert sorted(qkv) == sorted([r for r in locals_ if r] + [2 * r for r in locals_ if r] * (layers - 1)), \
        f"the q | k | v Linear is not one GEMM on 2 n_local rows behind block 0: {qkv}"
    if periodic:      # self_attn.o and ffn.2 of every stacked block as ONE launch on 2 n_local rows; block 0's shared o on n_local rows
        assert names.count("fg_gemm_epilogue_bf16_sp") == working * (2 * layers - 1), "the periodic gate did not run once per gated Linear"
    bound = 2 * medium.err_ref + 1e-2
    diff = (out - want).abs().max().item()
    print(f"stacked on shards {form} P={world} cuts={cuts} fp8={fp8} periodic={periodic}: max|emulated - unsharded stacked| = {diff:.5f}, "
          f"err_ref = {medium.err_ref:.5f}, bound = {bound:.5f}, max|unsharded| = {want.abs().max().item():.3f}")
    assert torch.isfinite(out).all() and out.shape == want.shape
    assert diff <= bound, f"the sharded stacked forward differs from the unsharded stacked forward by {diff} (bound {bound})"


@pytest.fixture(scope="module")
def medium1200():
    return scf._model(scf.MEDIUM, 99, "cuda")


@gpu
def test_sharded_stacked_equals_element_by_element_on_the_same_ranks(monkeypatch, medium1200):
    """Bit for bit, bf16 attention, P = 2, N = 1 200 (600 rows a rank): with the calls whose plan depends on the row count or the batch made
    per element — the GEMM seams, the own GEMM's residual store and hip.attention, as tests/test_stacked_cfg_forward.py wraps them for the
    unsharded forward — the stacked merged call on the emulated ranks equals the element-by-element merged call on the same ranks (the
    parent commit's path: two batch-1 sharded forwards that share block 0's self-attention half).  The stacked call runs one exchange
    per block, the element-by-element one a second in every block behind block 0."""
    from fairygen_amd import wan_video_dit as D
    m, _ = medium1200
    monkeypatch.setattr(D, "GEMM_MIN_TILES", 0)
    scf._wrap_plans(monkeypatch, residual_store=True)
    lat, both, ts = scf._medium_inputs(1200)
    call = dict(latents=lat.cuda(), timestep=ts, context=both.cuda(), fuse_vae_embedding_in_latents=True)
    layers = len(m.blocks)
    try:
        with torch.no_grad():
            m.enable_stacked_cfg(False)
            want, box = run_stacked_ranks(m, 2, shard_cls=tsi.LoopbackShard, **call)
            assert box.completed == 1 + 2 * (layers - 1)
            m.enable_stacked_cfg(sharded=True)
            got, box = run_stacked_ranks(m, 2, **call)
            assert box.completed == layers
    finally:
        m.enable_stacked_cfg(False)
    assert got.shape == want.shape and got.shape[0] == 2
    assert torch.equal(got, want)
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------------------------ GPU: the host-staged path
def _staged_gloo_worker(rank, port, result_dir):
    """One gloo rank with FAIRYGEN_FORCE_COLLECTIVES=1 and DEVICE tensors: sequence_parallel._staged() is True, so the batched exchanges
    take their host-staged branches (TokenShard._gather_batch, _PendingKV, _PendingRecords), which the CPU test above cannot reach."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", FAIRYGEN_FORCE_COLLECTIVES="1")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        from fairygen_amd import sequence_parallel as sp
        from fairygen_amd.wan_video import model_fn_wan_video
        shard = TokenShard()
        assert shard.active and shard.world_size == 1
        b, n, c = 2, 7, 16
        k = torch.randint(0, 256, (b, n, c), dtype=U8, generator=torch.Generator().manual_seed(7)).cuda()
        v = seeded((b, n, 3 * c), 3).cuda()[..., 2 * c:]
        assert sp._staged(k, shard.group) and sp._staged(v, shard.group)
        for kf, vf in (shard.all_gather_kv(k, v, n), shard.all_gather_kv_async(k, v, n).wait()):
            assert kf.is_cuda and kf.data_ptr() != k.data_ptr() and torch.equal(kf, k) and torch.equal(vf, v)      # a real exchange made a copy
            for e in range(b):
                k1, v1 = shard.all_gather_kv(k[e:e + 1], v[e:e + 1], n)
                assert torch.equal(kf[e:e + 1], k1) and torch.equal(vf[e:e + 1], v1)
        x = seeded((b, n, c), 5).cuda()
        got = shard.all_gather_tokens(x, n)
        assert got.data_ptr() != x.data_ptr() and got.is_contiguous() and torch.equal(got, x)
        rec = torch.randint(0, 256, (b, 40), dtype=U8, generator=torch.Generator().manual_seed(1)).cuda()
        full = shard.all_gather_records_async(rec).wait()
        assert full.is_cuda and full.shape == (1, b, 40) and torch.equal(full[0], rec)
        assert all(torch.equal(full[:, e], shard.all_gather_records_async(rec[e]).wait()) for e in range(b))
        # the merged call through the product's own exchanges: one rank holds all rows, so the stacked forward on the shard runs the
        # kernels of the unsharded stacked forward on the same rows — the same bits
        m, _ = scf._model(synthetic.TINY_DIT_KWARGS, 1234, "cuda")
        lat, ctx_p, ctx_n, _, ts = scf._tiny_inputs()
        call = dict(latents=lat.cuda(), timestep=ts, context=torch.cat([ctx_p, ctx_n], 0).cuda(), fuse_vae_embedding_in_latents=True)
        with torch.no_grad():
            want = model_fn_wan_video(m.enable_stacked_cfg(), **call)
            got = model_fn_wan_video(m.enable_stacked_cfg(sharded=True), sequence_shard=shard, **call)
        torch.cuda.synchronize()
        assert got.shape == want.shape and got.shape[0] == 2 and torch.equal(got, want) and not torch.equal(got[0], got[1])
        open(os.path.join(result_dir, "ok0"), "w").close()
    finally:
        dist.destroy_process_group()


@gpu
def test_batched_exchanges_host_staged_one_rank(tmp_path):
    """The host-staged gloo path of the batched exchanges on device tensors, and the merged stacked call through the real TokenShard (not
    a test double) against the unsharded stacked forward, bit for bit.  A process of its own: the process group is the test's subject."""
    mp.spawn(_staged_gloo_worker, args=(29675, str(tmp_path)), nprocs=1, join=True)
    assert os.path.exists(tmp_path / "ok0")

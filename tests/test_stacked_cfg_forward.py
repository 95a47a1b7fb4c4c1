"""The stacked CFG forward (WanModel.enable_stacked_cfg, ModelConfig(stacked_cfg=True)): with the switch on, a merged CFG call
(cfg_merge=True, a context batch of 2) runs ONE forward on the residual stream (2, N, dim) in place of two batch-1 forwards.

Three kinds of test.  EXACT: everything the stacked forward adds — the batched row kernels of include/fairygen_hip_rowbatch.h, the
routing of the per-element gated stores, the batched e4m3 attention chain of include/fairygen_hip_batch8.h, the shared tables — gives the
bits of the element-by-element merged call once the calls whose PLAN depends on the row count or the batch are made per element.  ORACLE:
nothing wrapped, each element of the stacked prediction against oracle.wan_dit.model_fn on its context, with the criterion and the
floor of tests/test_hip_models.py::test_medium_dit_block_stack_vs_oracle.  PIPELINE: the call of test_cfg_merge_and_reference_default_kwargs.
"""
import types

import pytest
import torch

from conftest import seeded
from fairygen_amd import synthetic
from oracle import wan_dit

gpu = pytest.mark.gpu
MEDIUM = dict(synthetic.TINY_DIT_KWARGS, dim=3072, num_heads=24, ffn_dim=1024, text_dim=256, num_layers=2)
GEMM_SEAMS = ("gemm_bias", "gemm_bias_gelu", "gemm_bias_tuned", "gemm_bias_own", "gemm_bias_gelu_own")


def cos(a, b):
    a, b = a.float().flatten().cpu(), b.float().flatten().cpu()
    return torch.nn.functional.cosine_similarity(a, b, dim=0).item()


def _tiny_inputs():      # those of tests/test_hip_models.py
    lat = seeded((1, 48, 3, 8, 8), 1)
    ctx_p = seeded((1, 16, 128), 2); ctx_p[:, 10:] = 0
    ctx_n = seeded((1, 16, 128), 3); ctx_n[:, 12:] = 0
    return lat, ctx_p, ctx_n, seeded((1, 48, 1, 8, 8), 4), torch.tensor([995.9]).to(torch.bfloat16)


def _model(cfg, seed, device):
    from fairygen_amd.wan_video_dit import WanModel
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=seed)
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    return m.to(device=device, dtype=torch.bfloat16).eval(), sd


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def test_switch_exists_and_is_off_by_default():
    from fairygen_amd import ModelConfig
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.stacked_cfg is False
    assert m.enable_stacked_cfg() is m and m.stacked_cfg is True
    assert m.enable_stacked_cfg(False).stacked_cfg is False
    assert ModelConfig(path="x").stacked_cfg is False and ModelConfig(path="x").vram_config()["stacked_cfg"] is False
    assert ModelConfig(path="x", stacked_cfg=True).vram_config()["stacked_cfg"] is True


def test_unsupported_combinations_raise_before_any_launch():
    """Host tensors throughout: each refusal is decided before anything touches a device (a launch on a host tensor would raise
    HipLibraryError, not NotImplementedError)."""
    from fairygen_amd.wan_video import TeaCache, model_fn_wan_video
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cpu")
    m.enable_stacked_cfg()
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    call = lambda **kw: model_fn_wan_video(m, **{**dict(latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=True), **kw})      # noqa: E731
    with pytest.raises(NotImplementedError, match="context batch of 2, not 3"):
        call(context=torch.cat([both, ctx_p], 0))
    with pytest.raises(NotImplementedError, match="sliding windows"):
        call(sliding_window_size=2, sliding_window_stride=1)
    with pytest.raises(NotImplementedError, match="active token shard"):
        call(sequence_shard=types.SimpleNamespace(active=True))
    with pytest.raises(NotImplementedError, match="TeaCache is per CFG branch"):      # raises as it did
        call(tea_cache=TeaCache(3, 0.1, "Wan2.1-T2V-1.3B"))
    m.enable_fp8_linear()
    with pytest.raises(NotImplementedError, match="enable_fp8_linear"):
        call()
    m.enable_fp8_linear(None)
    for backend in ("torch", "hip"):
        m.hot_lora_backend = backend
        m.add_hot_lora("blocks.0.self_attn.q", torch.zeros(4, 256), torch.zeros(256, 4))
        with pytest.raises(NotImplementedError, match=f"hot_backend='{backend}'"):
            call()
        m.clear_hot_loras()
    # one context is no merged call: the switch does not concern it (it gets as far as the first kernel, which refuses host tensors)
    from fairygen_amd.hip import HipLibraryError
    with pytest.raises(HipLibraryError):
        call(context=ctx_p)


# ------------------------------------------------------------------------------------------------------------------ GPU: exactness
def _per_element(fn):
    """fn(x, ...) on a stacked x (B, n, K) as B calls on (1, n, K): the call of the batch-1 forward, whatever plan fn picks by row count."""
    def wrapped(x, *args, **kw):
        if x.dim() == 3 and x.shape[0] > 1:
            return torch.cat([fn(x[e:e + 1], *args, **kw) for e in range(x.shape[0])], dim=0)
        return fn(x, *args, **kw)
    return wrapped


def _wrap_plans(monkeypatch, residual_store=False):
    from fairygen_amd import hip, wan_video_dit as D
    for name in GEMM_SEAMS:
        monkeypatch.setattr(D, name, _per_element(getattr(D, name)))
    if residual_store:
        inner = D.gemm_residual

        def store(x, a, *args, **kw):
            if a.shape[0] > 1:
                for e in range(a.shape[0]):
                    inner(x[e:e + 1], a[e:e + 1], *args, **kw)
                return x
            return inner(x, a, *args, **kw)
        monkeypatch.setattr(D, "gemm_residual", store)
    attn = hip.attention

    def attention(q, k, v, num_heads, out=None, **kw):
        if q.shape[0] > 1:
            return torch.cat([attn(q[e:e + 1], k[e:e + 1], v[e:e + 1], num_heads, **kw) for e in range(q.shape[0])], dim=0)
        return attn(q, k, v, num_heads, out=out, **kw)
    monkeypatch.setattr(hip, "attention", attention)


def _merged(m, stacked, lat, ts, both, ti2v=True, kv_cache=None):
    from fairygen_amd.wan_video import model_fn_wan_video
    m.enable_stacked_cfg(stacked)
    try:
        with torch.no_grad():
            return model_fn_wan_video(m, latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=ti2v, kv_cache=kv_cache)
    finally:
        m.enable_stacked_cfg(False)


@gpu
@pytest.mark.parametrize("share", (True, False))
def test_stacked_equals_element_by_element_tiny(monkeypatch, share):
    """Tiny DiT, TI2V (two modulation rows), every block Linear on the library (GEMM_BACKEND "lib": both forwards take the same GEMM path,
    the residual adds run on the batched row kernels).  Wrapped to run per element: the five GEMM seams of wan_video_dit.py (a library
    GEMM may pick another solution for 2 N rows) and hip.attention (the bf16 kernel plans its split-KV by the batch).  Then the stacked
    merged call equals the element-by-element one bit for bit, with block 0's self-attention half shared and not, and over two steps
    of one kv_cache (the second step reads the stacked cross-attention K / V back)."""
    from fairygen_amd import wan_video, wan_video_dit as D
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cuda")
    monkeypatch.setattr(D, "GEMM_BACKEND", "lib")
    monkeypatch.setattr(wan_video, "CFG_SHARE_PREFIX", share)
    _wrap_plans(monkeypatch)
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0).cuda()
    steps = [(lat.cuda(), ts), (seeded((1, 48, 3, 8, 8), 11).cuda(), torch.tensor([700.0]).to(torch.bfloat16))]
    kv_s, kv_e = {}, {}
    for lat_i, ts_i in steps:
        want = _merged(m, False, lat_i, ts_i, both, kv_cache=kv_e)
        got = _merged(m, True, lat_i, ts_i, both, kv_cache=kv_s)
        assert got.shape == want.shape == (2, 48, 3, 8, 8)
        assert torch.equal(got, want)
        assert not torch.equal(got[0], got[1])
    assert kv_s["entries"][0]["kv"][0][0].shape[0] == 2      # block 0's cross-attention keys of the pair, stacked
    # T2V (one modulation row) and no kv_cache
    assert torch.equal(_merged(m, True, lat.cuda(), ts, both, ti2v=False), _merged(m, False, lat.cuda(), ts, both, ti2v=False))


@pytest.fixture(scope="module")
def medium():
    return _model(MEDIUM, 99, "cuda")


def _medium_inputs(n):
    lat = seeded((1, 48, 3, 10, 14), 5) if n == 105 else seeded((1, 48, 3, 40, 40), 7)      # N = 3 * 5 * 7 = 105, 3 * 20 * 20 = 1 200
    return lat, torch.cat([seeded((1, 24, 256), 6), seeded((1, 24, 256), 8)], 0), torch.tensor([500.0]).to(torch.bfloat16)


@gpu
@pytest.mark.parametrize("qk8", (False, True))
def test_stacked_equals_element_by_element_medium(monkeypatch, medium, qk8):
    """dim 3072 / 24 heads, 2 layers, N = 1 200, TI2V, GEMM_MIN_TILES 0: every block Linear on the own persistent GEMM, so the gated
    stores (self-attention o, ffn.2) run once per element, and with qk8 the batched e4m3 producers and attention kernels of
    include/fairygen_hip_batch8.h run as they are (self-attention over 1 200 keys, cross-attention over 24).
    Wrapped to run per element: the five GEMM seams — the own GEMM splits the k loop of its last round's tiles where
    hip.gemm_workspace_need says so, a choice of the tile count and so of the row count (1 200 vs 2 400 rows); gemm_residual, the own
    GEMM's residual store, for the same reason (the ungated cross-attention o store takes 2 400 rows in the stacked forward); and, in
    the bf16 leg, hip.attention, whose split-KV plan depends on the batch.  Nothing of the e4m3 chain and no row kernel is wrapped."""
    from fairygen_amd import wan_video_dit as D
    m, _ = medium
    monkeypatch.setattr(D, "GEMM_MIN_TILES", 0)
    _wrap_plans(monkeypatch, residual_store=True)
    launches = []
    inner = D.gemm_residual
    monkeypatch.setattr(D, "gemm_residual", lambda x, a, *args, **kw: (launches.append((a.shape[0], args[2] is not None)), inner(x, a, *args, **kw))[1])
    lat, both, ts = _medium_inputs(1200)
    m.enable_qk8_attention(qk8, pv8=qk8, cross=qk8, fused_producer=qk8)
    try:
        want = _merged(m, False, lat.cuda(), ts, both.cuda())
        launches.clear()
        got = _merged(m, True, lat.cuda(), ts, both.cuda())
    finally:
        m.enable_qk8_attention(False)
    # the stacked forward's own stores: block 0's shared o on one element, then per block 2 gated stores per element (never a gated
    # store on the batch: the table has two rows) and the ungated cross-attention o on the batch
    assert (2, True) not in launches and launches.count((1, True)) == 1 + 2 + 2 * 2 + 0 and launches.count((2, False)) == 2
    assert torch.equal(got, want)
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------------------------ GPU: against the oracle
_REFS = {}


def _oracle(sd, n, ti2v):
    """(ref_bf16, ref_f32) per element, computed once per shape and mode and shared."""
    if (n, ti2v) not in _REFS:
        lat, both, ts = _medium_inputs(n)
        sd32 = {k: v.float() for k, v in sd.items()}
        _REFS[(n, ti2v)] = [(wan_dit.model_fn(sd, MEDIUM, lat, ts, both[e:e + 1], ti2v),
                             wan_dit.model_fn(sd32, MEDIUM, lat.float(), ts.float(), both[e:e + 1].float(), ti2v)) for e in range(2)]
    return _REFS[(n, ti2v)]


@gpu
@pytest.mark.parametrize("n,ti2v", [(105, True), (1200, True), (1200, False)])
def test_stacked_vs_oracle(medium, n, ti2v):
    """Nothing wrapped.  N = 105: every Linear on the library, the gates on the batched row kernels.  N = 1 200: the plain Linears on the own
    GEMM with 2 400 rows; TI2V: the gated adds on the batched row kernels behind library GEMMs (1 200 rows are under the own GEMM's
    tile floor); T2V (one gate row): the single 2 N-row gated store.  Criterion of test_medium_dit_block_stack_vs_oracle, per element."""
    m, sd = medium
    lat, both, ts = _medium_inputs(n)
    got = _merged(m, True, lat.cuda(), ts, both.cuda(), ti2v=ti2v)
    assert got.shape[0] == 2
    for e, (ref16, ref32) in enumerate(_oracle(sd, n, ti2v)):
        err_ref = (ref16.float() - ref32).abs().max().item()
        err = (got[e:e + 1].float().cpu() - ref32).abs().max().item()
        print(f"stacked vs oracle: N={n} ti2v={ti2v} element {e}: err {err:.5f} err_ref {err_ref:.5f} cos {cos(got[e:e + 1], ref32):.6f}")
        assert err <= 2 * err_ref + 1e-2, (e, err, err_ref)
        assert cos(got[e:e + 1], ref32) > 0.9995, e


# ------------------------------------------------------------------------------------------------------------------ GPU: the pipeline
@gpu
def test_pipeline_cfg_merge_with_the_switch():
    """The call of tests/test_hip_models.py::test_cfg_merge_and_reference_default_kwargs.  Switch on: one batched model call per step and
    a clip close to the two-call clip — not bit-equal: the library GEMMs of the stacked forward run on 2 N rows, where hipBLASLt may take
    another solution.  Switch off: the merged call is still the two-call clip bit for bit."""
    from fairygen_amd.wan_video import WanVideoPipeline, model_fn_wan_video
    from fairygen_amd.wan_video_vae import WanVideoVAE38
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cuda")
    vae = WanVideoVAE38(dim=32, dec_dim=32)
    vae.load_state_dict(synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=32, dim=32), seed=1234))
    pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
    pipe.dit, pipe.vae = m, vae.to(device="cuda", dtype=torch.bfloat16).eval()
    pipe.height_division_factor = pipe.width_division_factor = 32
    ctx_p = seeded((1, 16, 128), 2); ctx_p[:, 10:] = 0
    ctx_n = seeded((1, 16, 128), 3); ctx_n[:, 12:] = 0
    z0 = seeded((1, 48, 1, 4, 4), 4)
    kw = dict(prompt=ctx_p, negative_prompt=ctx_n, first_frame_latents=z0, seed=1, height=64, width=64, num_frames=9,
              num_inference_steps=3, tiled=False, output_type="floatpoint", progress_bar_cmd=lambda x: x)
    calls = []
    pipe.model_fn = lambda *a, **k: (calls.append(k["context"].shape[0]), model_fn_wan_video(*a, **k))[1]
    two = pipe(**kw)
    assert calls == [1] * 6
    calls.clear()
    merged = pipe(**kw, cfg_merge=True)
    assert calls == [2] * 3 and torch.equal(two, merged)
    calls.clear()
    m.enable_stacked_cfg()
    stacked = pipe(**kw, cfg_merge=True)
    assert calls == [2] * 3, "the stacked forward is the merged call: one batched call per step"
    assert stacked.shape == two.shape and cos(stacked, two) > 0.999
    with pytest.raises(NotImplementedError, match="graph=True with cfg_merge"):
        pipe.model_fn = model_fn_wan_video
        pipe(**kw, cfg_merge=True, graph=True)

"""The stacked CFG forward in the fp8 Linear mode (WanModel.enable_stacked_cfg(fp8_linear=True), ModelConfig(computation_dtype=
torch.float8_e4m3fn, stacked_cfg=True)): tests/test_stacked_cfg_forward.py for the forward whose norms hand (e4m3 rows, row scales) to
fp8 Linears — the batched fp8-output norms of include/fairygen_hip_rowbatch8.h, one fp8 GEMM per Linear on the 2 N rows of the pair.

The kinds of test.  EXACT: the stacked merged call gives the bits of the element-by-element merged call once the calls whose PLAN
depends on the row count or the batch are made per element — in the fp8 mode that is WanModel._scaled_linear, the one seam in front of
both fp8 GEMMs (gemm_fp8_own: hip.gemm_workspace_need makes its k-split a function of the row count; torch._scaled_mm: the library
may pick another solution for 2 N rows), and hip.attention (the bf16 kernel plans its split-KV by the batch).  No row kernel, no
quantisation pass and nothing of the e4m3 attention chain is wrapped.  FOLD: nothing wrapped, the stacked forward with the fp8-output
norms against the stacked forward with bf16 norms and the quantisation pass (FAIRYGEN_FP8_FOLD=0) — the same GEMM plans on 2 N rows in
both, so bit for bit.  ORACLE: nothing wrapped, each element against oracle.wan_dit.model_fn(Fp8Blocks) with the criterion of
tests/test_hip_models.py::test_fp8_linear_mode_vs_oracle.  PIPELINE: the call of test_pipeline_cfg_merge_with_the_switch in the fp8 mode.
"""
import types

import pytest
import torch

from conftest import seeded
from fairygen_amd import synthetic
from oracle import wan_dit

gpu = pytest.mark.gpu
F8 = torch.float8_e4m3fn
MEDIUM = dict(synthetic.TINY_DIT_KWARGS, dim=3072, num_heads=24, ffn_dim=1024, text_dim=256, num_layers=2)
NORMS_B = ("fg_ln_modulate_fp8_bf16_b", "fg_residual_ln_fp8_bf16_b")
NORMS_1 = ("fg_ln_modulate_fp8_bf16", "fg_residual_ln_fp8_bf16")


def cos(a, b):
    a, b = a.float().flatten().cpu(), b.float().flatten().cpu()
    return torch.nn.functional.cosine_similarity(a, b, dim=0).item()


def _tiny_inputs():      # those of tests/test_hip_models.py and tests/test_stacked_cfg_forward.py
    lat = seeded((1, 48, 3, 8, 8), 1)
    ctx_p = seeded((1, 16, 128), 2); ctx_p[:, 10:] = 0
    ctx_n = seeded((1, 16, 128), 3); ctx_n[:, 12:] = 0
    return lat, ctx_p, ctx_n, seeded((1, 48, 1, 8, 8), 4), torch.tensor([995.9]).to(torch.bfloat16)


def _model(cfg, seed, device, fp8=True):
    from fairygen_amd.wan_video_dit import WanModel
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=seed)
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(device=device, dtype=torch.bfloat16).eval()
    return (m.enable_fp8_linear() if fp8 else m), sd


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def test_fp8_opt_in_is_off_by_default_and_cleared_with_the_switch():
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.stacked_cfg is False and m.stacked_cfg_fp8 is False
    assert m.enable_stacked_cfg() is m and m.stacked_cfg is True and m.stacked_cfg_fp8 is False
    assert m.enable_stacked_cfg(fp8_linear=True) is m and m.stacked_cfg is True and m.stacked_cfg_fp8 is True
    assert m.enable_stacked_cfg(True).stacked_cfg_fp8 is False      # the opt-in is stated with every call, like enable_qk8_attention's
    m.enable_stacked_cfg(fp8_linear=True)
    assert m.enable_stacked_cfg(False).stacked_cfg is False and m.stacked_cfg_fp8 is False
    assert m.enable_stacked_cfg(False, fp8_linear=True).stacked_cfg_fp8 is False      # nothing to opt into with the switch off


def test_refusals_with_the_fp8_opt_in():
    """Host tensors throughout: each refusal is decided before anything touches a device (a launch on a host tensor would raise
    HipLibraryError, not NotImplementedError).  Without the opt-in an fp8 model still raises; with it the fp8 mode passes the check
    and gets as far as the first kernel, and everything else the stacked forward does not take raises as before."""
    from fairygen_amd.hip import HipLibraryError
    from fairygen_amd.wan_video import TeaCache, model_fn_wan_video
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cpu")
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    call = lambda **kw: model_fn_wan_video(m, **{**dict(latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=True), **kw})      # noqa: E731
    m.enable_stacked_cfg()
    with pytest.raises(NotImplementedError, match="enable_fp8_linear"):
        call()
    m.enable_stacked_cfg(fp8_linear=True)
    with pytest.raises(HipLibraryError):
        call()
    with pytest.raises(NotImplementedError, match="context batch of 2, not 3"):
        call(context=torch.cat([both, ctx_p], 0))
    with pytest.raises(NotImplementedError, match="sliding windows"):
        call(sliding_window_size=2, sliding_window_stride=1)
    with pytest.raises(NotImplementedError, match="active token shard"):
        call(sequence_shard=types.SimpleNamespace(active=True))
    with pytest.raises(NotImplementedError, match="TeaCache is per CFG branch"):
        call(tea_cache=TeaCache(3, 0.1, "Wan2.1-T2V-1.3B"))
    with pytest.raises(NotImplementedError, match="not recorded into a graph"):
        call(owned=types.SimpleNamespace())
    for backend in ("torch", "hip"):
        m.hot_lora_backend = backend
        m.add_hot_lora("blocks.0.self_attn.q", torch.zeros(4, 256), torch.zeros(256, 4))
        with pytest.raises(NotImplementedError, match=f"hot_backend='{backend}'"):
            call()
        m.clear_hot_loras()
    m.enable_stacked_cfg(False)
    assert m.stacked_cfg_fp8 is False
    m.enable_stacked_cfg()
    with pytest.raises(NotImplementedError, match="enable_fp8_linear"):      # cleared: the refusal is back
        call()


def test_model_config_states_both_wishes(tmp_path):
    """ModelConfig(computation_dtype=e4m3, stacked_cfg=True) through ModelPool on a saved tiny DiT: the loader opts the stacked forward
    into the fp8 mode; stacked_cfg with bf16 Linears leaves the opt-in off, fp8 alone leaves the switch off."""
    from fairygen_amd import ModelConfig, loader
    assert ModelConfig(path="x", computation_dtype=F8, stacked_cfg=True).vram_config()["stacked_cfg"] is True
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        got = []
        for comp, stacked in ((F8, True), (torch.bfloat16, True), (F8, False)):
            pool = loader.ModelPool()      # a pool per load: every registered config with this file's hash loads one model
            pool.auto_load_model(path, vram_config={"computation_dtype": comp, "computation_device": "cpu", "stacked_cfg": stacked})
            got.append({(m.fp8_dtype, m.stacked_cfg, m.stacked_cfg_fp8) for m in pool.model})
        assert got == [{(F8, True, True)}, {(None, True, False)}, {(F8, False, False)}]
    finally:
        loader.MODEL_CONFIGS.remove(entry)


# ------------------------------------------------------------------------------------------------------------------ GPU: exactness
def _wrap_plans(monkeypatch, attention=True):
    """Per element: WanModel._scaled_linear (both fp8 GEMMs behind it) on the rows of a stacked call (batch=B > 1), and hip.attention."""
    from fairygen_amd import hip, wan_video_dit as D
    inner = D.WanModel._scaled_linear

    def scaled_linear(self, xq, scale_a, w8, bias, batch=1, **state):
        if batch > 1:
            r = xq.shape[0] // batch
            return torch.cat([inner(self, xq[e * r:(e + 1) * r], scale_a[e * r:(e + 1) * r], w8, bias, **state) for e in range(batch)], dim=0)
        return inner(self, xq, scale_a, w8, bias, **state)
    monkeypatch.setattr(D.WanModel, "_scaled_linear", scaled_linear)
    if attention:
        attn = hip.attention

        def attention_fn(q, k, v, num_heads, out=None, **kw):
            if q.shape[0] > 1:
                return torch.cat([attn(q[e:e + 1], k[e:e + 1], v[e:e + 1], num_heads, **kw) for e in range(q.shape[0])], dim=0)
            return attn(q, k, v, num_heads, out=out, **kw)
        monkeypatch.setattr(hip, "attention", attention_fn)


def _merged(m, stacked, lat, ts, both, ti2v=True, kv_cache=None):
    from fairygen_amd.wan_video import model_fn_wan_video
    m.enable_stacked_cfg(stacked, fp8_linear=True)
    try:
        with torch.no_grad():
            return model_fn_wan_video(m, latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=ti2v, kv_cache=kv_cache)
    finally:
        m.enable_stacked_cfg(False)


@gpu
@pytest.mark.parametrize("fp8_gemm", ("own", "lib"))
@pytest.mark.parametrize("share", (True, False))
def test_stacked_equals_element_by_element_tiny(monkeypatch, share, fp8_gemm):
    """Tiny DiT in the fp8 mode, every fp8 Linear on fg_gemm_fp8_bf16 ("own") or on torch._scaled_mm ("lib"), the gates and the fp8-output
    norms on the batched row kernels.  TI2V over two steps of one kv_cache (the second step reads the stacked cross-attention K / V
    back) and T2V, with block 0's self-attention half shared and not."""
    from fairygen_amd import wan_video, wan_video_dit as D
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cuda")
    monkeypatch.setattr(D, "FP8_GEMM", fp8_gemm)
    monkeypatch.setattr(wan_video, "CFG_SHARE_PREFIX", share)
    _wrap_plans(monkeypatch)
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0).cuda()
    steps = [(lat.cuda(), ts), (seeded((1, 48, 3, 8, 8), 11).cuda(), torch.tensor([700.0]).to(torch.bfloat16))]
    kv_s, kv_e, outs = {}, {}, []
    for lat_i, ts_i in steps:
        want = _merged(m, False, lat_i, ts_i, both, kv_cache=kv_e)
        got = _merged(m, True, lat_i, ts_i, both, kv_cache=kv_s)
        assert got.shape == want.shape == (2, 48, 3, 8, 8)
        assert torch.equal(got, want)
        assert not torch.equal(got[0], got[1])
        outs.append(got)
    assert kv_s["entries"][0]["kv"][0][0].shape[0] == 2      # block 0's cross-attention keys of the pair, stacked
    got_t2v = _merged(m, True, lat.cuda(), ts, both, ti2v=False)
    assert torch.equal(got_t2v, _merged(m, False, lat.cuda(), ts, both, ti2v=False)) and not torch.equal(got_t2v[0], got_t2v[1])
    # the fp8 mode is what ran: the bf16 stacked forward gives other numbers
    m.enable_fp8_linear(None)
    assert not torch.equal(_merged(m, True, lat.cuda(), ts, both), outs[0])


@pytest.fixture(scope="module")
def medium():
    return _model(MEDIUM, 99, "cuda")


def _medium_inputs():      # N = 3 * 20 * 20 = 1 200
    return seeded((1, 48, 3, 40, 40), 7), torch.cat([seeded((1, 24, 256), 6), seeded((1, 24, 256), 8)], 0), torch.tensor([500.0]).to(torch.bfloat16)


def _count_norms(monkeypatch):
    """Record (name, B or None, rows) of every fp8-output norm launch that reaches hip._call."""
    from fairygen_amd import hip
    seen, inner = [], hip._call

    def call(name, *args):
        if name == NORMS_B[0]:
            seen.append((name, args[5], args[6]))
        elif name == NORMS_B[1]:
            seen.append((name, args[9], args[10]))
        elif name in NORMS_1:
            seen.append((name, None, args[5] if name == NORMS_1[0] else args[9]))
        return inner(name, *args)
    monkeypatch.setattr(hip, "_call", call)
    return seen


@gpu
@pytest.mark.parametrize("qk8", (False, True))
def test_stacked_equals_element_by_element_medium(monkeypatch, medium, qk8):
    """dim 3072 / 24 heads / ffn 1024, 2 layers, N = 1 200, TI2V, fp8 Linears on fg_gemm_fp8_bf16; bf16 attention, or with qk8 the batched
    e4m3 producers and attention kernels as they are (self-attention over 1 200 keys, cross-attention over 24).  Wrapped per element:
    the fp8 GEMM seam and, in the bf16 leg, hip.attention.  The fp8-output norms that reach the library are counted: with block 0's
    self-attention half shared, the first norm runs once on one element (fg_ln_modulate_fp8_bf16) and four fused residual + norm
    launches take B = 2 (block 0: cross-attention o, ffn.2; block 1: self-attention o, cross-attention o); without the share the
    first norm takes B = 2 as well and block 0's self-attention o adds a fifth.  No single-element fp8-output norm runs besides."""
    from fairygen_amd import wan_video
    m, _ = medium
    _wrap_plans(monkeypatch, attention=not qk8)
    seen = _count_norms(monkeypatch)
    lat, both, ts = _medium_inputs()
    m.enable_qk8_attention(qk8, pv8=qk8, cross=qk8, fused_producer=qk8)
    try:
        for share in (True, False):
            monkeypatch.setattr(wan_video, "CFG_SHARE_PREFIX", share)
            want = _merged(m, False, lat.cuda(), ts, both.cuda())
            seen.clear()
            got = _merged(m, True, lat.cuda(), ts, both.cuda())
            batched = [s for s in seen if s[0] in NORMS_B]
            assert all(s[1:] == (2, 1200) for s in batched), seen
            assert [s[0] for s in batched].count(NORMS_B[0]) == (0 if share else 1), seen
            assert [s[0] for s in batched].count(NORMS_B[1]) == (4 if share else 5), seen
            assert [s for s in seen if s[0] in NORMS_1] == ([(NORMS_1[0], None, 1200)] if share else []), seen
            assert torch.equal(got, want), share
            assert not torch.equal(got[0], got[1])
    finally:
        m.enable_qk8_attention(False)


@gpu
@pytest.mark.parametrize("qk8", (False, True))
def test_stacked_fold_equals_unfolded(monkeypatch, medium, qk8):
    """Nothing wrapped.  FP8_FOLD True (the batched fp8-output norms) against False (the batched bf16 norms, then fg_fp8_quant_rows_bf16 on
    the 2 N rows): both legs run the same GEMM and attention plans on the pair, and an fp8-output norm is by contract the row
    quantisation of the bf16 norm — so the predictions are equal bit for bit.  The one exact test on the stacked GEMMs as they are."""
    from fairygen_amd import wan_video, wan_video_dit as D
    m, _ = medium
    monkeypatch.setattr(wan_video, "CFG_SHARE_PREFIX", True)
    seen = _count_norms(monkeypatch)
    lat, both, ts = _medium_inputs()
    m.enable_qk8_attention(qk8, pv8=qk8, cross=qk8, fused_producer=qk8)
    try:
        monkeypatch.setattr(D, "FP8_FOLD", True)
        folded = _merged(m, True, lat.cuda(), ts, both.cuda())
        assert len([s for s in seen if s[0] in NORMS_B]) == 4, seen
        seen.clear()
        monkeypatch.setattr(D, "FP8_FOLD", False)
        unfolded = _merged(m, True, lat.cuda(), ts, both.cuda())
        assert seen == []
    finally:
        m.enable_qk8_attention(False)
    assert torch.equal(folded, unfolded)
    assert not torch.equal(folded[0], folded[1])


# ------------------------------------------------------------------------------------------------------------------ GPU: against the oracle
@gpu
def test_stacked_fp8_vs_oracle_tiny():
    """Nothing wrapped.  Each element of the stacked fp8 prediction against oracle.wan_dit.model_fn(Fp8Blocks(sd), ...) on its context, with
    the criterion of tests/test_hip_models.py::test_fp8_linear_mode_vs_oracle (cos > 0.999, err < 0.5 * drift + 0.05, drift = the
    oracle's own fp8-to-bf16 distance), and the batch-1 fp8 forward on the same context under the same bound."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, sd = _model(synthetic.TINY_DIT_KWARGS, 1234, "cuda")
    cfg = synthetic.TINY_DIT_KWARGS
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    got = _merged(m, True, lat.cuda(), ts, both.cuda())
    assert got.shape[0] == 2
    for e in range(2):
        ctx = both[e:e + 1]
        want = wan_dit.model_fn(wan_dit.Fp8Blocks(sd), cfg, lat, ts, ctx, True)
        drift = (want.float() - wan_dit.model_fn(sd, cfg, lat, ts, ctx, True).float()).abs().max().item()
        with torch.no_grad():
            one = model_fn_wan_video(m, latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
        err = (got[e:e + 1].float().cpu() - want.float()).abs().max().item()
        err_one = (one.float().cpu() - want.float()).abs().max().item()
        print(f"stacked fp8 vs oracle: element {e}: err {err:.5f} (batch-1 forward: {err_one:.5f}) drift {drift:.5f} "
              f"cos {cos(got[e:e + 1], want):.6f} (batch-1: {cos(one, want):.6f})")
        assert cos(one, want) > 0.999 and err_one < 0.5 * drift + 0.05, (e, err_one, drift)
        assert cos(got[e:e + 1], want) > 0.999 and err < 0.5 * drift + 0.05, (e, err, drift)


# ------------------------------------------------------------------------------------------------------------------ GPU: a fused adapter
@gpu
def test_stacked_fp8_with_fused_adapter(monkeypatch):
    """hot_backend="fused": the adapters are folded into the weights, the e4m3 copies rewritten along, so the stacked fp8 forward takes
    them as plain weights: stacked equals element by element (wrapped as in the tiny exact test), the adapters change the prediction,
    and after clear_hot_loras() the stacked prediction is the adapter-free one bit for bit."""
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cuda")
    _wrap_plans(monkeypatch)
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0).cuda()
    base = _merged(m, True, lat.cuda(), ts, both)      # also builds the blocks' e4m3 copies, which the fuse then rewrites in place
    m.hot_lora_backend = "fused"
    m.add_hot_lora("blocks.0.self_attn.q", seeded((4, 256), 31, scale=0.3).cuda(), seeded((256, 4), 32, scale=0.3).cuda(), alpha=1.0)
    m.add_hot_lora("blocks.1.ffn.2", seeded((4, 512), 33, scale=0.3).cuda(), seeded((256, 4), 34, scale=0.3).cuda(), alpha=1.0)
    assert not m.hot_loras and len(m._fused_stash) == 2
    want = _merged(m, False, lat.cuda(), ts, both)
    got = _merged(m, True, lat.cuda(), ts, both)
    assert torch.equal(got, want) and not torch.equal(got, base)
    assert m.clear_hot_loras() == 2
    assert torch.equal(_merged(m, True, lat.cuda(), ts, both), base)


# ------------------------------------------------------------------------------------------------------------------ GPU: the pipeline
@gpu
def test_pipeline_cfg_merge_with_the_switch_fp8():
    """The call of tests/test_stacked_cfg_forward.py::test_pipeline_cfg_merge_with_the_switch with the DiT in the fp8 mode: one batched
    model call per step and a clip close to the fp8 two-call clip (that test's criterion); graph=True with cfg_merge still raises."""
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
    m.enable_stacked_cfg()
    with pytest.raises(NotImplementedError, match="enable_fp8_linear"):      # without the opt-in the fp8 model still refuses
        pipe(**kw, cfg_merge=True)
    calls.clear()
    m.enable_stacked_cfg(fp8_linear=True)
    stacked = pipe(**kw, cfg_merge=True)
    assert calls == [2] * 3, "the stacked forward is the merged call: one batched call per step"
    assert stacked.shape == two.shape and cos(stacked, two) > 0.999
    with pytest.raises(NotImplementedError, match="graph=True with cfg_merge"):
        pipe.model_fn = model_fn_wan_video
        pipe(**kw, cfg_merge=True, graph=True)

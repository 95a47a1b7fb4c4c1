"""The stacked CFG forward with unfused hot-loaded adapters on the project's own kernels (WanModel.enable_stacked_cfg(hot_lora=True),
ModelConfig(stacked_cfg=True, stacked_cfg_hot_lora=True), load_lora(..., hotload=True, hot_backend="hip")): the adapter kernel and the
two-output modulate norm take the batch through include/fairygen_hip_lorabatch.h (tests/test_lora_apply_batched.py holds the kernels'
contract), in the bf16 and the fp8 Linear modes.

The kinds of test, those of tests/test_stacked_cfg_forward.py and tests/test_stacked_cfg_fp8.py.  EXACT: the stacked merged call gives the
bits of the element-by-element merged call with the same "hip" adapters once the calls whose PLAN depends on the row count or the batch
are made per element — the GEMM seams (the five of wan_video_dit.py, gemm_residual, WanModel._scaled_linear, hip.gemm_fp8) and
hip.attention.  Nothing of lora_apply, the dual norm or the row kernels is wrapped.  ORACLE: nothing wrapped, each element against the
oracle forward with the adapters applied by the reference's arithmetic (lora_forward), criterion of
tests/test_hot_lora_kernel.py::test_tiny_dit_hot_backend_hip and tests/test_fp8_hot_lora.py: max|hip - f32| <= 2 * max|torch - f32| + 1e-2
with the "torch" backend's batch-1 forward as yardstick.  PIPELINE: load_lora / clear_lora around two stacked denoise steps.
"""
import types

import pytest
import torch

from conftest import seeded
from fairygen_amd import synthetic
from oracle import wan_dit

gpu = pytest.mark.gpu
F8 = torch.float8_e4m3fn
MEDIUM = dict(synthetic.TINY_DIT_KWARGS, dim=3072, num_heads=24, ffn_dim=1024, text_dim=256, num_layers=2)      # that of the stacked tests
GEMM_SEAMS = ("gemm_bias", "gemm_bias_gelu", "gemm_bias_tuned", "gemm_bias_own", "gemm_bias_gelu_own")
ADAPTED = ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "cross_attn.q", "ffn.0", "ffn.2")
LORA_B, LORA_1 = "fg_lora_apply_bf16_b", "fg_lora_apply_bf16"
DUAL_B, DUAL_1 = "fg_ln_modulate_dual_bf16_b", "fg_ln_modulate_dual_bf16"


def _tiny_inputs():      # those of tests/test_hip_models.py and the stacked tests
    lat = seeded((1, 48, 3, 8, 8), 1)
    ctx_p = seeded((1, 16, 128), 2); ctx_p[:, 10:] = 0
    ctx_n = seeded((1, 16, 128), 3); ctx_n[:, 12:] = 0
    return lat, ctx_p, ctx_n, torch.tensor([995.9]).to(torch.bfloat16)


def _medium_inputs():      # N = 3 * 20 * 20 = 1 200, the first latent frame's 400 tokens on the first time row
    return seeded((1, 48, 3, 40, 40), 7), torch.cat([seeded((1, 24, 256), 6), seeded((1, 24, 256), 8)], 0), torch.tensor([500.0]).to(torch.bfloat16)


def _model(cfg, seed, device, fp8):
    from fairygen_amd.wan_video_dit import WanModel
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=seed)
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(device=device, dtype=torch.bfloat16).eval()
    return (m.enable_fp8_linear() if fp8 else m), sd


def _adapters(cfg, ranks=(4, 8)):
    """name -> [(alpha * A (r, in), B (out, r)), ...]: adapters of rank 4 and 8 stacked on ADAPTED of every block, x A^T B^T of O(0.3)."""
    shapes, out = synthetic.dit_shapes(cfg), {}
    for i in range(cfg["num_layers"]):
        for j, nm in enumerate(ADAPTED):
            name = f"blocks.{i}.{nm}"
            n, k = shapes[name + ".weight"]
            out[name] = [(seeded((r, k), 1000 + 100 * i + 10 * j + s, scale=k ** -0.5), seeded((n, r), 2000 + 100 * i + 10 * j + s, scale=0.3 * r ** -0.5))
                         for s, r in enumerate(ranks)]
    return out


def _attach(m, adapters, backend="hip"):
    m.hot_lora_backend = backend
    for name, ads in adapters.items():
        for a, b in ads:
            m.add_hot_lora(name, a, b)
    return m


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def test_hot_lora_opt_in_is_off_by_default_and_stated_with_every_call():
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.stacked_cfg is False and m.stacked_cfg_hot_lora is False
    assert m.enable_stacked_cfg() is m and m.stacked_cfg is True and m.stacked_cfg_hot_lora is False
    assert m.enable_stacked_cfg(hot_lora=True) is m and m.stacked_cfg is True and m.stacked_cfg_hot_lora is True and m.stacked_cfg_fp8 is False
    assert m.enable_stacked_cfg(True).stacked_cfg_hot_lora is False      # cleared by a call that does not restate it
    assert m.enable_stacked_cfg(fp8_linear=True).stacked_cfg_hot_lora is False and m.stacked_cfg_fp8 is True      # independent of fp8_linear
    assert m.enable_stacked_cfg(hot_lora=True).stacked_cfg_fp8 is False and m.stacked_cfg_hot_lora is True
    m.enable_stacked_cfg(fp8_linear=True, hot_lora=True)
    assert m.stacked_cfg_fp8 is True and m.stacked_cfg_hot_lora is True
    assert m.enable_stacked_cfg(False).stacked_cfg is False and m.stacked_cfg_hot_lora is False and m.stacked_cfg_fp8 is False
    assert m.enable_stacked_cfg(False, hot_lora=True).stacked_cfg_hot_lora is False      # nothing to opt into with the switch off


@pytest.mark.parametrize("fp8", (False, True))
def test_refusals_with_the_hot_lora_opt_in(fp8):
    """Host tensors throughout: each refusal is decided before anything touches a device.  With the opt-in a "hip" adapter passes the
    check and gets as far as the first kernel, which refuses host tensors; a "torch" adapter and everything else the stacked forward
    does not take raise as before; without the opt-in the "hip" adapter raises with the message it has always had."""
    from fairygen_amd.hip import HipLibraryError
    from fairygen_amd.wan_video import TeaCache, model_fn_wan_video
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cpu", fp8)
    lat, ctx_p, ctx_n, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    call = lambda **kw: model_fn_wan_video(m, **{**dict(latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=True), **kw})      # noqa: E731
    on = lambda: m.enable_stacked_cfg(fp8_linear=fp8, hot_lora=True)      # noqa: E731
    m.hot_lora_backend = "hip"
    m.add_hot_lora("blocks.0.self_attn.q", torch.zeros(4, 256), torch.zeros(256, 4))
    m.enable_stacked_cfg(fp8_linear=fp8)
    with pytest.raises(NotImplementedError, match="hot_backend='hip'.*has no batched form"):
        call()
    on()
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
    if fp8:      # the fp8 refusal does not depend on the adapters' opt-in
        m.enable_stacked_cfg(hot_lora=True)
        with pytest.raises(NotImplementedError, match="enable_fp8_linear"):
            call()
    m.clear_hot_loras()
    m.hot_lora_backend = "torch"
    m.add_hot_lora("blocks.0.self_attn.q", torch.zeros(4, 256), torch.zeros(256, 4))
    on()
    with pytest.raises(NotImplementedError, match="hot_backend='torch'"):
        call()
    m.enable_stacked_cfg(fp8_linear=fp8)      # not restated: cleared, and today's message is back
    with pytest.raises(NotImplementedError, match="hot_backend='torch'.*has no batched form"):
        call()


def test_model_config_carries_the_opt_in(tmp_path):
    """ModelConfig(stacked_cfg=True, stacked_cfg_hot_lora=True) through ModelPool on a saved tiny DiT, in bf16 and with an fp8
    computation_dtype; without stacked_cfg the wish has nothing to ride on and ModelConfig.check_input raises."""
    from fairygen_amd import ModelConfig, loader
    assert ModelConfig(path="x").stacked_cfg_hot_lora is False and ModelConfig(path="x").vram_config()["stacked_cfg_hot_lora"] is False
    assert ModelConfig(path="x", stacked_cfg=True, stacked_cfg_hot_lora=True).vram_config()["stacked_cfg_hot_lora"] is True
    ModelConfig(path="x", stacked_cfg=True, stacked_cfg_hot_lora=True).check_input()
    with pytest.raises(ValueError, match="needs stacked_cfg=True"):      # the wish has nothing to ride on
        ModelConfig(path="x", stacked_cfg_hot_lora=True).check_input()
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        got = []
        for comp, hot in ((torch.bfloat16, True), (F8, True), (F8, False)):
            pool = loader.ModelPool()
            cfg = ModelConfig(path=path, computation_dtype=comp, computation_device="cpu", stacked_cfg=True, stacked_cfg_hot_lora=hot).vram_config()
            pool.auto_load_model(path, vram_config={k: cfg[k] for k in ("computation_dtype", "computation_device", "stacked_cfg", "stacked_cfg_hot_lora")})
            got.append({(m.fp8_dtype, m.stacked_cfg, m.stacked_cfg_fp8, m.stacked_cfg_hot_lora) for m in pool.model})
        assert got == [{(None, True, False, True)}, {(F8, True, True, True)}, {(F8, True, True, False)}]
    finally:
        loader.MODEL_CONFIGS.remove(entry)


# ------------------------------------------------------------------------------------------------------------------ GPU: exactness
def _wrap_plans(monkeypatch):
    """Per element: the GEMM seams — the five of wan_video_dit.py and gemm_residual (bf16), WanModel._scaled_linear and hip.gemm_fp8 (fp8:
    the plain form by its lead_shape, the residual store by its `out`) — and hip.attention.  A library GEMM may pick another solution
    for 2 N rows, the own GEMMs split k by the row count, the bf16 attention kernel plans its split-KV by the batch."""
    from fairygen_amd import hip, wan_video_dit as D

    def per_element(fn):
        def wrapped(x, *args, **kw):
            if x.dim() == 3 and x.shape[0] > 1:
                return torch.cat([fn(x[e:e + 1], *args, **kw) for e in range(x.shape[0])], dim=0)
            return fn(x, *args, **kw)
        return wrapped
    for name in GEMM_SEAMS:
        monkeypatch.setattr(D, name, per_element(getattr(D, name)))
    store = D.gemm_residual

    def gemm_residual(x, a, *args, **kw):
        if a.shape[0] > 1:
            for e in range(a.shape[0]):
                store(x[e:e + 1], a[e:e + 1], *args, **kw)
            return x
        return store(x, a, *args, **kw)
    monkeypatch.setattr(D, "gemm_residual", gemm_residual)
    scaled = D.WanModel._scaled_linear

    def scaled_linear(self, xq, scale_a, w8, bias, batch=1, **state):
        if batch > 1:
            r = xq.shape[0] // batch
            return torch.cat([scaled(self, xq[e * r:(e + 1) * r], scale_a[e * r:(e + 1) * r], w8, bias, **state) for e in range(batch)], dim=0)
        return scaled(self, xq, scale_a, w8, bias, **state)
    monkeypatch.setattr(D.WanModel, "_scaled_linear", scaled_linear)
    gemm8 = hip.gemm_fp8

    def gemm_fp8(xq, scale_a, w8, bias, out=None, residual=False, lead_shape=None, **kw):
        nb = out.shape[0] if residual and out is not None and out.dim() == 3 else lead_shape[0] if lead_shape is not None and len(lead_shape) == 2 else 1
        if nb > 1:
            r = xq.shape[0] // nb
            parts = [gemm8(xq[e * r:(e + 1) * r], scale_a[e * r:(e + 1) * r], w8, bias, out=out[e:e + 1] if residual else None, residual=residual,
                           lead_shape=None if residual else (1, r), **kw) for e in range(nb)]
            return out if residual else torch.cat(parts, dim=0)
        return gemm8(xq, scale_a, w8, bias, out=out, residual=residual, lead_shape=lead_shape, **kw)
    monkeypatch.setattr(hip, "gemm_fp8", gemm_fp8)
    attn = hip.attention

    def attention(q, k, v, num_heads, out=None, **kw):
        if q.shape[0] > 1:
            return torch.cat([attn(q[e:e + 1], k[e:e + 1], v[e:e + 1], num_heads, **kw) for e in range(q.shape[0])], dim=0)
        return attn(q, k, v, num_heads, out=out, **kw)
    monkeypatch.setattr(hip, "attention", attention)


def _count_calls(monkeypatch):
    """The adapter and dual-norm launches that reach hip._call, by entry point."""
    from fairygen_amd import hip
    seen, inner = [], hip._call

    def call(name, *args):
        if name in (LORA_B, LORA_1, DUAL_B, DUAL_1):
            seen.append(name)
        return inner(name, *args)
    monkeypatch.setattr(hip, "_call", call)
    return seen


def _merged(m, stacked, lat, ts, both, ti2v=True, kv_cache=None):
    from fairygen_amd.wan_video import model_fn_wan_video
    m.enable_stacked_cfg(stacked, fp8_linear=m.fp8_dtype is not None, hot_lora=True)
    try:
        with torch.no_grad():
            return model_fn_wan_video(m, latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=ti2v, kv_cache=kv_cache)
    finally:
        m.enable_stacked_cfg(False)


def _expected_launches(seen, layers, share, fp8):
    """Per block five adapter launches (q | k | v, o, cross q, ffn.0, ffn.2), all with B = 2 but block 0's shared self-attention half (q | k | v
    and o on one element); in the fp8 mode the two-output modulate norm: norm2 of every block and norm1 of every block but the first
    with B = 2, block 0's norm1 on one element when its half is shared."""
    assert seen.count(LORA_B) == 5 * layers - (2 if share else 0) and seen.count(LORA_1) == (2 if share else 0), seen
    if fp8:
        assert seen.count(DUAL_B) == 2 * layers - (1 if share else 0) and seen.count(DUAL_1) == (1 if share else 0), seen
    else:
        assert DUAL_B not in seen and DUAL_1 not in seen, seen


@gpu
@pytest.mark.parametrize("share", (True, False))
@pytest.mark.parametrize("fp8", (False, True))
def test_stacked_equals_element_by_element_tiny(monkeypatch, fp8, share):
    """Tiny DiT with the adapters on the "hip" backend.  bf16: library GEMMs (the tiny widths stay below the own GEMM's tile floor), the
    adapters added to their outputs, the gates on the batched row kernels.  fp8: every Linear on fg_gemm_fp8_bf16, so the gated stores
    (two gate rows: TI2V) run per element on the element's quantised rows with ONE gated adapter launch behind them, and the norms are
    the two-output ones.  TI2V over two steps of one kv_cache, and T2V (one gate row: one gated store on 2 N rows)."""
    from fairygen_amd import wan_video
    cfg = synthetic.TINY_DIT_KWARGS
    m, _ = _model(cfg, 1234, "cuda", fp8)
    lat, ctx_p, ctx_n, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0).cuda()
    base = _merged(m, True, lat.cuda(), ts, both)
    _attach(m, _adapters(cfg))
    monkeypatch.setattr(wan_video, "CFG_SHARE_PREFIX", share)
    _wrap_plans(monkeypatch)
    seen = _count_calls(monkeypatch)
    steps = [(lat.cuda(), ts), (seeded((1, 48, 3, 8, 8), 11).cuda(), torch.tensor([700.0]).to(torch.bfloat16))]
    kv_s, kv_e = {}, {}
    for lat_i, ts_i in steps:
        want = _merged(m, False, lat_i, ts_i, both, kv_cache=kv_e)
        del seen[:]
        got = _merged(m, True, lat_i, ts_i, both, kv_cache=kv_s)
        _expected_launches(seen, cfg["num_layers"], share, fp8)
        assert got.shape == want.shape == (2, 48, 3, 8, 8)
        assert torch.equal(got, want)
        assert not torch.equal(got[0], got[1])
    got_t2v = _merged(m, True, lat.cuda(), ts, both, ti2v=False)
    assert torch.equal(got_t2v, _merged(m, False, lat.cuda(), ts, both, ti2v=False)) and not torch.equal(got_t2v[0], got_t2v[1])
    # the adapters are what ran, and without them the stacked forward is what it was
    assert not torch.equal(_merged(m, True, lat.cuda(), ts, both), base)
    m.clear_hot_loras()
    assert torch.equal(_merged(m, True, lat.cuda(), ts, both), base)


@gpu
@pytest.mark.parametrize("fp8", (False, True))
def test_stacked_equals_element_by_element_medium(monkeypatch, fp8):
    """dim 3072 / 24 heads / ffn 1024, 2 layers, N = 1 200, TI2V with first_rows = 400 inside the sequence; bf16 with GEMM_MIN_TILES 0:
    every block Linear on the own persistent GEMM, so in both modes the gated stores (self-attention o, ffn.2) run once per element
    and the gated adapter launch behind them takes B = 2 with the gate rule counted inside the element."""
    from fairygen_amd import wan_video, wan_video_dit as D
    m, _ = _model(MEDIUM, 99, "cuda", fp8)
    _attach(m, _adapters(MEDIUM))
    monkeypatch.setattr(D, "GEMM_MIN_TILES", 0)
    monkeypatch.setattr(wan_video, "CFG_SHARE_PREFIX", True)
    _wrap_plans(monkeypatch)
    seen = _count_calls(monkeypatch)
    lat, both, ts = _medium_inputs()
    want = _merged(m, False, lat.cuda(), ts, both.cuda())
    del seen[:]
    got = _merged(m, True, lat.cuda(), ts, both.cuda())
    _expected_launches(seen, 2, True, fp8)
    assert torch.equal(got, want)
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------------------------ GPU: against the oracle
@gpu
@pytest.mark.parametrize("fp8", (False, True))
def test_stacked_hot_lora_vs_oracle_tiny(monkeypatch, fp8):
    """Nothing wrapped.  Each element of the stacked prediction against the oracle's fp32 forward (fp8: Fp8Blocks) with lora_forward's sum
    behind every adapted Linear; yardstick: the "torch" backend's batch-1 forward on the element's context."""
    from fairygen_amd.wan_video import model_fn_wan_video
    cfg = synthetic.TINY_DIT_KWARGS
    adapters = _adapters(cfg)
    hot_h, sd = _model(cfg, 1234, "cuda", fp8)
    hot_t, _ = _model(cfg, 1234, "cuda", fp8)
    _attach(hot_h, adapters), _attach(hot_t, adapters, "torch")
    lat, ctx_p, ctx_n, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    got = _merged(hot_h, True, lat.cuda(), ts, both.cuda())
    assert got.shape[0] == 2
    sd32 = {k: v.float() for k, v in sd.items()}
    sd32 = wan_dit.Fp8Blocks(sd32) if fp8 else sd32
    real = wan_dit.linear

    def linear(sd_, prefix, x):      # oracle.wan_dit.linear followed by lora_forward's sum on the same input (core/vram/layers.py:417-436)
        out = real(sd_, prefix, x)
        for a, b in adapters.get(prefix, ()):
            out = out + x @ a.to(x.dtype).T @ b.to(x.dtype).T
        return out
    monkeypatch.setattr(wan_dit, "linear", linear)
    for e in range(2):
        ctx = both[e:e + 1]
        want = wan_dit.model_fn(sd32, cfg, lat.float(), ts.float(), ctx.float(), fuse_vae_embedding_in_latents=True)
        with torch.no_grad():
            out_t = model_fn_wan_video(hot_t, latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
        err_h, err_t = (got[e:e + 1].float().cpu() - want).abs().max().item(), (out_t.float().cpu() - want).abs().max().item()
        print(f"stacked hot adapters ({'fp8' if fp8 else 'bf16'}), element {e}: max|hip-f32|={err_h:.4f} max|torch-f32|={err_t:.4f} "
              f"max|f32|={want.abs().max().item():.2f}")
        assert err_h <= 2 * err_t + 1e-2, e


# ------------------------------------------------------------------------------------------------------------------ GPU: the pipeline
@gpu
@pytest.mark.parametrize("fp8", (False, True))
def test_pipeline_load_and_clear_lora_around_stacked_steps(monkeypatch, fp8):
    """pipe.load_lora(..., hotload=True, hot_backend="hip") on a tiny pipeline with stacked_cfg and the opt-in: two denoise steps with
    cfg_merge=True are one batched model call each and launch the batched adapter kernel; the adapters (on all ten Linears of a block:
    those of the 16 context rows take the reference's row-wise torch ops on the stacked context) change the clip; clear_lora() restores
    the adapter-free stacked clip bit for bit."""
    from fairygen_amd.wan_video import WanVideoPipeline, model_fn_wan_video
    from fairygen_amd.wan_video_vae import WanVideoVAE38
    cfg = synthetic.TINY_DIT_KWARGS
    m, _ = _model(cfg, 1234, "cuda", fp8)
    vae = WanVideoVAE38(dim=32, dec_dim=32)
    vae.load_state_dict(synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=32, dim=32), seed=1234))
    pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
    pipe.dit, pipe.vae = m, vae.to(device="cuda", dtype=torch.bfloat16).eval()
    pipe.height_division_factor = pipe.width_division_factor = 32
    _, ctx_p, ctx_n, _ = _tiny_inputs()
    kw = dict(prompt=ctx_p, negative_prompt=ctx_n, first_frame_latents=seeded((1, 48, 1, 4, 4), 4), seed=1, height=64, width=64, num_frames=9,
              num_inference_steps=2, tiled=False, output_type="floatpoint", progress_bar_cmd=lambda x: x, cfg_merge=True)
    calls = []
    pipe.model_fn = lambda *a, **k: (calls.append(k["context"].shape[0]), model_fn_wan_video(*a, **k))[1]
    seen = _count_calls(monkeypatch)
    m.enable_stacked_cfg(fp8_linear=fp8, hot_lora=True)
    base = pipe(**kw)
    assert calls == [2] * 2 and LORA_B not in seen and LORA_1 not in seen
    pipe.load_lora(pipe.dit, state_dict=synthetic.random_lora(synthetic.dit_shapes(cfg), rank=4, seed=4321), alpha=2.0, hotload=True,
                   hot_backend="hip")
    assert m.hot_loras and m.hot_lora_backend == "hip" and m.stacked_cfg_hot_lora is True
    del calls[:], seen[:]
    hot = pipe(**kw)
    assert calls == [2] * 2, "the stacked forward is the merged call: one batched call per step"
    # per step and block six adapter launches (q | k | v, o, cross q, cross o, ffn.0, ffn.2; the context's k | v take the torch ops, once
    # per loop), all with B = 2 but block 0's shared q | k | v and o; fp8: the two-output modulate norms as in _expected_launches
    layers, steps = cfg["num_layers"], 2
    assert seen.count(LORA_B) == steps * (6 * layers - 2) and seen.count(LORA_1) == steps * 2, seen
    assert seen.count(DUAL_B) == (steps * (2 * layers - 1) if fp8 else 0) and seen.count(DUAL_1) == (steps if fp8 else 0), seen
    assert hot.shape == base.shape and not torch.equal(hot, base)
    m.enable_stacked_cfg(fp8_linear=fp8)      # without the opt-in the loaded adapters refuse the merged call, as they always have
    with pytest.raises(NotImplementedError, match="has no batched form"):
        pipe(**kw)
    m.enable_stacked_cfg(fp8_linear=fp8, hot_lora=True)
    pipe.clear_lora()
    assert m.hot_loras == {}
    assert torch.equal(pipe(**kw), base)

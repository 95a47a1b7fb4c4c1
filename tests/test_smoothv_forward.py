"""The model level of the mean-smoothed V (WanModel.enable_qk8_attention(pv8=True, smooth_v=True), ModelConfig(attention_v_smoothing=True),
examples/inference.py --smooth-v; the kernels: tests/test_attention_smoothv.py).

On the CPU: the switch and its refusals (token shards, no e4m3 P V form), the config field, the example's flag.  On the GPU, the tiny DiT
over 1 200 tokens: the launches of a forward and 1 - cos to the fp32 oracle within the bound tests/test_attention_pv8.py holds the e4m3
P V form to; graph=True against the eager loop, bit for bit; the stacked CFG forward against the element-by-element merged call, bit for
bit, with the plans that depend on the batch made per element as tests/test_stacked_cfg_forward.py makes them.
"""
import pytest
import torch

import test_attention_pv8 as pv8
import test_attention_qk8 as qk8
import test_stacked_cfg_forward as stacked
from conftest import seeded
from fairygen_amd import synthetic
from test_attention_qk8 import hip  # noqa: F401  (the module fixture)

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn


class Shard:
    active = True


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def test_enable_sets_the_routing_and_refuses():
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.smoothv_attention is False
    assert m.enable_qk8_attention(pv8=True) is m and m.smoothv_attention is False, "the default is off"
    for fused in (False, True):
        assert m.enable_qk8_attention(fused_producer=fused, pv8=True, smooth_v=True) is m
        assert m.qk8_attention and m.pv8_attention and m.smoothv_attention is True and m.qk8_fused_producer is fused
    m.enable_qk8_attention(pv8=True)
    assert m.smoothv_attention is False, "an enable without smooth_v= switches it off"
    # it is V of the e4m3 P V product that is smoothed
    for kw in ({}, {"pv8": False}, {"flag": False}):
        with pytest.raises(ValueError, match="smooth_v=True.*pv8=True"):
            m.enable_qk8_attention(smooth_v=True, **kw)
    assert m.pv8_attention is True and m.smoothv_attention is False, "a refused call changes nothing"
    # token shards, sharded=True or not: the mean spans every rank's keys and the shard8 record has no V sum
    with pytest.raises(ValueError, match="no V sum"):
        m.enable_qk8_attention(pv8=True, smooth_v=True, sharded=True)
    m.enable_qk8_attention(pv8=True, smooth_v=True)
    m.check_qk8_layout(None)
    with pytest.raises(NotImplementedError, match="smooth_v=True.*no V sum"):
        m.check_qk8_layout(Shard())
    x = torch.empty((1, 8, 256), device="meta")
    with pytest.raises(NotImplementedError, match="smooth_v=True"):
        next(m.forward_tokens_steps(x, x, torch.empty((1, 6, 256), device="meta"), x, 0, (x, x), Shard(), 16))
    # e4m3 cross-attention keeps its unsmoothed V8^T: the two switches are independent
    m.enable_qk8_attention(pv8=True, cross=True, smooth_v=True)
    assert m.cross8_attention is True and m.smoothv_attention is True
    m.enable_qk8_attention(False)
    assert m.smoothv_attention is False


def test_model_config(tmp_path):
    from fairygen_amd import ModelConfig, loader
    assert ModelConfig(path="x").attention_v_smoothing is False and ModelConfig(path="x").vram_config()["attention_v_smoothing"] is False
    good = ModelConfig(path="x", attention_dtype=F8, attention_pv_dtype=F8, attention_v_smoothing=True)
    good.check_input()
    assert good.vram_config()["attention_v_smoothing"] is True
    for kw in ({}, {"attention_dtype": F8}, {"attention_pv_dtype": F8}):
        with pytest.raises(ValueError, match="attention_v_smoothing"):
            ModelConfig(path="x", attention_v_smoothing=True, **kw).check_input()
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        base = {"computation_dtype": BF16, "computation_device": "cpu"}
        def load(**kw):      # a pool of its own per configuration: the last model loaded is this entry's
            pool = loader.ModelPool()
            pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8, attention_pv_dtype=F8, **kw))
            return pool.model[-1]
        m = load(attention_v_smoothing=True)
        assert m.pv8_attention is True and m.smoothv_attention is True and m.qk8_fused_producer is True
        m = load()
        assert m.pv8_attention is True and m.smoothv_attention is False
        m = load(cross_attention_dtype=F8, attention_v_smoothing=True)
        assert m.cross8_attention is True and m.smoothv_attention is True
        for kw in ({}, {"attention_dtype": F8}):
            with pytest.raises(ValueError, match="attention_v_smoothing"):
                loader.ModelPool().auto_load_model(path, vram_config=dict(base, attention_v_smoothing=True, **kw))
    finally:
        loader.MODEL_CONFIGS.remove(entry)


def test_example_flag(monkeypatch):
    """examples/inference.py --smooth-v implies both e4m3 halves and sets the config field; without it the field stays off."""
    from examples import inference

    class Built(Exception):
        pass

    def from_pretrained(**kw):
        raise Built(kw["model_configs"][1])
    monkeypatch.setattr(inference.WanVideoPipeline, "from_pretrained", staticmethod(from_pretrained))
    for flags, want in (([], (None, None, False)), (["--pv8-attention"], (F8, F8, False)), (["--smooth-v"], (F8, F8, True)),
                        (["--pv8-attention", "--smooth-v"], (F8, F8, True))):
        monkeypatch.setattr("sys.argv", ["inference.py", "--weights", "w", "--tokenizer", "t", "--image", "i.png"] + flags)
        with pytest.raises(Built) as e:
            inference.main()
        cfg = e.value.args[0]
        assert (cfg.attention_dtype, cfg.attention_pv_dtype, cfg.attention_v_smoothing) == want, flags


# ------------------------------------------------------------------------------------------------------------------ GPU: the tiny DiT
@gpu
@pytest.mark.parametrize("fused", [False, True], ids=["two-step", "fused-producers"])
def test_tiny_dit_forward(hip, monkeypatch, fused):  # noqa: F811
    """enable_qk8_attention(pv8=True, smooth_v=True) on the tiny DiT over 1 200 tokens, behind either producer path: the launches are the
    smoothed form's, the forward is finite and not the unsmoothed one's, and 1 - cos to the fp32 oracle (and to the bf16 kernel forward)
    stays within the bound tests/test_attention_pv8.py::test_tiny_dit_forward holds the e4m3 P V form to: 2 d_recipe, d_recipe = 1 - cos
    (the oracle's bf16 forward with its self-attention replaced by the emulation of the e4m3 P V recipe, the oracle's fp32 forward)."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, sd, cfg = qk8.tiny_model()
    lat, ctx, ts = seeded(qk8.LATENT, 11), seeded((1, 16, 128), 12), torch.tensor([995.9]).to(BF16)
    args = dict(latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    try:
        with torch.no_grad():
            out_bf16 = model_fn_wan_video(m, **args)
            out_pv8 = model_fn_wan_video(m.enable_qk8_attention(fused_producer=fused, pv8=True), **args)
            monkeypatch.setattr(hip, "_call", call)
            out_s = model_fn_wan_video(m.enable_qk8_attention(fused_producer=fused, pv8=True, smooth_v=True), **args)
            monkeypatch.setattr(hip, "_call", real)
    finally:
        m.enable_qk8_attention(False)
    nb = cfg["num_layers"]
    assert calls.count("fg_attn_fwd_pv8s_bf16") == nb and calls.count("fg_attn_quant_vt_smooth_bf16") == nb
    assert calls.count("fg_attn_fwd_pv8_bf16") == 0 and calls.count("fg_attn_quant_vt_bf16") == 0 and calls.count("fg_attn_fwd_qk8_bf16") == 0
    assert calls.count("fg_attn_fwd_bf16") == nb, "cross-attention stays on the bf16 kernel"
    assert torch.isfinite(out_s.float()).all()
    assert not torch.equal(out_s, out_pv8) and not torch.equal(out_s, out_bf16), "the switch is dead"
    want32, want_emu = pv8.tiny_oracle()
    cos = qk8.cos_distance
    d_recipe = cos(want_emu, want32)
    d_s, d_pv8, d_bf16, d_pair = cos(out_s, want32), cos(out_pv8, want32), cos(out_bf16, want32), cos(out_s, out_bf16)
    print(f"tiny DiT, 1 200 tokens, {'fused' if fused else 'two-step'} producers: 1 - cos to the fp32 oracle: pv8 recipe in the bf16 oracle "
          f"{d_recipe:.3e}, smoothed pv8 kernels {d_s:.3e}, pv8 kernels {d_pv8:.3e}, bf16 kernels {d_bf16:.3e}; smoothed pv8 kernels to bf16 "
          f"kernels {d_pair:.3e}, to pv8 kernels {cos(out_s, out_pv8):.3e}")
    assert d_s <= 2 * d_recipe, (d_s, d_recipe)
    assert d_pair <= 2 * d_recipe, (d_pair, d_recipe)


@gpu
def test_graph_loop_equals_eager(hip):  # noqa: F811
    """graph=True on the tiny loop over 1 200 tokens with the mode on: the captured step owns v8t, sv, mu and the statistics scratch next
    to the e4m3 q / k buffers and replays to the bits of the eager loop."""
    from fairygen_amd.wan_video import WanVideoPipeline
    m, _, _ = qk8.tiny_model()
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.enable_qk8_attention(pv8=True, smooth_v=True)
    lat, ctx_p, ctx_n = seeded(qk8.LATENT, 21), seeded((1, 16, 128), 22), seeded((1, 16, 128), 23)
    z0 = seeded(qk8.LATENT[:2] + (1,) + qk8.LATENT[3:], 24)

    def loop(graph):
        pipe.scheduler.set_timesteps(4, denoising_strength=1.0, shift=5.0)
        latents = lat.clone()
        latents[:, :, 0:1] = z0
        inputs = {"latents": latents.cuda(), "fuse_vae_embedding_in_latents": True, "first_frame_latents": z0.cuda()}
        with torch.no_grad():
            out = pipe.denoise(inputs, {"context": ctx_p.cuda()}, {"context": ctx_n.cuda()}, 5.0, progress_bar_cmd=lambda x: x, graph=graph)
        torch.cuda.synchronize()
        return out.clone()
    try:
        want = loop(False)
        got = loop(True)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} latents differ from the eager loop"
        pipe.dit.enable_qk8_attention(pv8=True)
        assert not torch.equal(loop(False), want), "the loop above ran without the smoothed V"
    finally:
        m.enable_qk8_attention(False)


@gpu
def test_stacked_equals_element_by_element(hip, monkeypatch):  # noqa: F811
    """The stacked CFG forward of the tiny DiT over 1 200 tokens with the mode on (the fused producers, as the loader sets them): the
    e4m3 chain runs on the batched entry points — fg_attn_quant_vt_smooth_bf16_b and fg_attn_fwd_pv8s_bf16_b among them — and the merged
    call equals the element-by-element one bit for bit.  Wrapped to run per element, as in tests/test_stacked_cfg_forward.py: the GEMM
    seams (a library GEMM may pick another solution for 2 N rows) and hip.attention (the bf16 kernel of cross-attention plans by the
    batch).  Nothing of the e4m3 chain is wrapped."""
    from fairygen_amd import wan_video_dit as D
    m, _, _ = qk8.tiny_model()
    monkeypatch.setattr(D, "GEMM_BACKEND", "lib")
    stacked._wrap_plans(monkeypatch)
    lat, ts = seeded(qk8.LATENT, 31).cuda(), torch.tensor([500.0]).to(BF16)
    both = torch.cat([seeded((1, 16, 128), 32), seeded((1, 16, 128), 33)], 0).cuda()
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    m.enable_qk8_attention(pv8=True, smooth_v=True, fused_producer=True)
    try:
        want = stacked._merged(m, False, lat, ts, both)
        monkeypatch.setattr(hip, "_call", call)
        got = stacked._merged(m, True, lat, ts, both)
        monkeypatch.setattr(hip, "_call", real)
    finally:
        m.enable_qk8_attention(False)
    assert calls.count("fg_attn_fwd_pv8s_bf16_b") >= 1 and calls.count("fg_attn_quant_vt_smooth_bf16_b") == calls.count("fg_attn_fwd_pv8s_bf16_b")
    assert calls.count("fg_attn_fwd_pv8_bf16_b") == 0 and calls.count("fg_attn_quant_vt_bf16_b") == 0
    assert got.shape == want.shape and got.shape[0] == 2
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} elements differ"
    assert not torch.equal(got[0], got[1])

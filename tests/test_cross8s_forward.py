"""The model level of the mean-smoothed V of the e4m3 cross-attention (WanModel.enable_qk8_attention(pv8=True, cross=True,
smooth_v_cross=True), ModelConfig(cross_attention_v_smoothing=True), examples/inference.py --smooth-v-cross; the kernel:
tests/test_attention_cross8s.py).

On the CPU: the switch and its refusals (no e4m3 cross-attention, token shards), its independence of smooth_v, the config field, the
example's flag.  On the GPU, the tiny DiT over 1 200 tokens with a context of 512 rows whose tail (rows >= 40) is zero, as the pipeline
leaves a prompt: the launches of a forward and 1 - cos to the fp32 oracle within the bound tests/test_attention_pv8.py holds the e4m3
P V form to; one context quantisation per kv_cache, whose entries have five tensors; graph=True against the eager loop, bit for bit;
the stacked CFG forward against the element-by-element merged call, bit for bit, with the plans that depend on the batch made per
element as tests/test_stacked_cfg_forward.py makes them.
"""
import functools

import pytest
import torch

import test_attention_pv8 as pv8
import test_attention_qk8 as qk8
import test_stacked_cfg_forward as stacked
from conftest import seeded
from fairygen_amd import synthetic
from oracle import wan_dit
from test_attention_qk8 import hip  # noqa: F401  (the module fixture)

gpu = pytest.mark.gpu
BF16, F8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float32
L_CTX, L_TEXT = 512, 40


class Shard:
    active = True


def padded_context(seed, l_text=L_TEXT):
    """(1, 512, 128) bf16 text embeddings with the rows at and beyond the prompt's length zeroed."""
    ctx = seeded((1, L_CTX, 128), seed)
    ctx[:, l_text:] = 0
    return ctx


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def test_enable_sets_the_routing_and_refuses():
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.smoothv_cross_attention is False
    assert m.enable_qk8_attention(pv8=True, cross=True) is m and m.smoothv_cross_attention is False, "the default is off"
    for fused in (False, True):
        assert m.enable_qk8_attention(fused_producer=fused, pv8=True, cross=True, smooth_v_cross=True) is m
        assert m.qk8_attention and m.pv8_attention and m.cross8_attention and m.smoothv_cross_attention is True
        assert m.smoothv_attention is False and m.qk8_fused_producer is fused, "it does not smooth self-attention"
    # it is V of the e4m3 cross-attention that is smoothed: without cross, without pv8, with the mode off
    for kw in ({"pv8": True}, {"cross": False, "pv8": True}, {}, {"pv8": False}, {"flag": False}, {"flag": False, "pv8": True, "cross": True},
               {"pv8": True, "smooth_v": True}):
        with pytest.raises(ValueError):
            m.enable_qk8_attention(smooth_v_cross=True, **kw)
        assert m.cross8_attention is True and m.smoothv_cross_attention is True and m.smoothv_attention is False and m.qk8_fused_producer is True, \
            "a refused call changes nothing"
    with pytest.raises(ValueError, match="smooth_v_cross=True.*cross=True"):
        m.enable_qk8_attention(pv8=True, smooth_v_cross=True)
    # independent of smooth_v, in both directions
    m.enable_qk8_attention(pv8=True, cross=True, smooth_v=True)
    assert m.smoothv_attention is True and m.cross8_attention is True and m.smoothv_cross_attention is False, "smooth_v leaves cross-attention unsmoothed"
    m.enable_qk8_attention(pv8=True, cross=True, smooth_v=True, smooth_v_cross=True)
    assert m.smoothv_attention is True and m.smoothv_cross_attention is True
    m.enable_qk8_attention(pv8=True, cross=True)
    assert m.cross8_attention is True and m.smoothv_cross_attention is False, "an enable without smooth_v_cross= switches it off"
    # token shards are refused as the e4m3 cross-attention is, sharded=True or not
    for sharded in (False, True):
        m.enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True, sharded=sharded)
        m.check_qk8_layout(None)
        with pytest.raises(NotImplementedError, match="cross=True"):
            m.check_qk8_layout(Shard())
        x = torch.empty((1, 8, 256), device="meta")
        with pytest.raises(NotImplementedError, match="cross=True"):
            next(m.forward_tokens_steps(x, x, torch.empty((1, 6, 256), device="meta"), x, 0, (x, x), Shard(), 16))
    m.enable_qk8_attention(False)
    assert m.smoothv_cross_attention is False and m.cross8_attention is False


def test_model_config(tmp_path):
    from fairygen_amd import ModelConfig, loader
    assert ModelConfig(path="x").cross_attention_v_smoothing is False
    assert ModelConfig(path="x").vram_config()["cross_attention_v_smoothing"] is False
    all8 = dict(attention_dtype=F8, attention_pv_dtype=F8, cross_attention_dtype=F8)
    good = ModelConfig(path="x", cross_attention_v_smoothing=True, **all8)
    good.check_input()
    assert good.vram_config()["cross_attention_v_smoothing"] is True and good.vram_config()["attention_v_smoothing"] is False
    for kw in ({}, {"attention_dtype": F8, "attention_pv_dtype": F8}, {"attention_dtype": F8, "attention_pv_dtype": F8, "attention_v_smoothing": True},
               dict(all8, cross_attention_dtype=BF16)):
        with pytest.raises(ValueError, match="cross_attention_v_smoothing"):
            ModelConfig(path="x", cross_attention_v_smoothing=True, **kw).check_input()
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        base = {"computation_dtype": BF16, "computation_device": "cpu"}

        def load(**kw):      # a pool of its own per configuration: the last model loaded is this entry's
            pool = loader.ModelPool()
            pool.auto_load_model(path, vram_config=dict(base, **kw))
            return pool.model[-1]
        m = load(cross_attention_v_smoothing=True, **all8)
        assert m.cross8_attention is True and m.smoothv_cross_attention is True and m.smoothv_attention is False and m.qk8_fused_producer is True
        vram = ModelConfig(path="x", cross_attention_v_smoothing=True, attention_v_smoothing=True, **all8).vram_config()      # the round trip
        m = load(**{k: v for k, v in vram.items() if v is not None})
        assert m.smoothv_cross_attention is True and m.smoothv_attention is True
        m = load(**all8)
        assert m.cross8_attention is True and m.smoothv_cross_attention is False
        m = load(attention_v_smoothing=True, **all8)
        assert m.smoothv_attention is True and m.smoothv_cross_attention is False
        for kw in ({}, {"attention_dtype": F8, "attention_pv_dtype": F8}):
            with pytest.raises(ValueError, match="cross_attention_v_smoothing"):
                load(cross_attention_v_smoothing=True, **kw)
    finally:
        loader.MODEL_CONFIGS.remove(entry)


def test_example_flag(monkeypatch):
    """examples/inference.py --smooth-v-cross implies --cross8-attention (and with it both e4m3 halves) and sets the config field alone;
    without it the field stays off, and build_pipeline is called without the keyword (stubs with the earlier signature keep working)."""
    from examples import inference

    class Built(Exception):
        pass

    def from_pretrained(**kw):
        raise Built(kw["model_configs"][1])
    monkeypatch.setattr(inference.WanVideoPipeline, "from_pretrained", staticmethod(from_pretrained))
    argv = ["inference.py", "--weights", "w", "--tokenizer", "t", "--image", "i.png"]
    for flags, want in (([], (None, None, None, False, False)), (["--cross8-attention"], (F8, F8, F8, False, False)),
                        (["--smooth-v-cross"], (F8, F8, F8, False, True)), (["--cross8-attention", "--smooth-v-cross"], (F8, F8, F8, False, True)),
                        (["--smooth-v", "--cross8-attention"], (F8, F8, F8, True, False)), (["--smooth-v", "--smooth-v-cross"], (F8, F8, F8, True, True))):
        monkeypatch.setattr("sys.argv", argv + flags)
        with pytest.raises(Built) as e:
            inference.main()
        cfg = e.value.args[0]
        assert (cfg.attention_dtype, cfg.attention_pv_dtype, cfg.cross_attention_dtype, cfg.attention_v_smoothing,
                cfg.cross_attention_v_smoothing) == want, flags
        cfg.check_input()
    seen = []

    def old_build_pipeline(weights, tokenizer, lora=None, fp8=False, qk8=False, pv8=False, cross8=False, stacked_cfg=False, periodic_gate=False,
                           smooth_v=False):
        seen.append(cross8)
        raise Built()
    monkeypatch.setattr(inference, "build_pipeline", old_build_pipeline)
    monkeypatch.setattr("sys.argv", argv + ["--cross8-attention"])
    with pytest.raises(Built):
        inference.main()
    assert seen == [True]
    monkeypatch.setattr("sys.argv", argv + ["--smooth-v-cross"])
    with pytest.raises(TypeError, match="smooth_v_cross"):
        inference.main()


# ------------------------------------------------------------------------------------------------------------------ GPU: the tiny DiT
def tiny_args():
    lat, ts = seeded(qk8.LATENT, 11), torch.tensor([995.9]).to(BF16)
    return dict(latents=lat.cuda(), timestep=ts, context=padded_context(12).cuda(), fuse_vae_embedding_in_latents=True)


@functools.lru_cache(maxsize=None)
def tiny_oracle():
    """test_attention_pv8.tiny_oracle on the padded context of this file: (the oracle's fp32 forward, its bf16 forward with self-attention
    replaced by the emulation of both e4m3 halves; cross-attention stays the oracle's)."""
    cfg = synthetic.TINY_DIT_KWARGS
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    lat, ctx, ts = seeded(qk8.LATENT, 11), padded_context(12), torch.tensor([995.9]).to(BF16)
    want32 = wan_dit.model_fn({k_: v_.float() for k_, v_ in sd.items()}, cfg, lat.float(), ts.float(), ctx.float(), True)
    bf16_attention = wan_dit.attention

    def emulated(q, k, v, num_heads):
        if q.shape[1] != k.shape[1]:      # cross-attention
            return bf16_attention(q, k, v, num_heads)
        q8, k8, sq, sk, _, _ = qk8.quant_emu(q[0].to(BF16), k[0].to(BF16), num_heads)
        sv, v8, _ = pv8.quant_v_emu(v[0].to(BF16), num_heads)
        return pv8.attn_pv8_emu(q8, k8, sq, sk, v8, sv, num_heads).to(q.dtype).unsqueeze(0)
    wan_dit.attention = emulated
    try:
        want_emu = wan_dit.model_fn(sd, cfg, lat, ts, ctx, True)
    finally:
        wan_dit.attention = bf16_attention
    return want32, want_emu


@gpu
def test_tiny_dit_forward(hip, monkeypatch):  # noqa: F811
    """enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True) on the tiny DiT (1 200 tokens, 512 context rows, 472 of them zero):
    cross-attention launches the smoothing V producer and fg_attn_fwd_cross8s_bf16 and not the unsmoothed ones, self-attention keeps its
    unsmoothed form; the forward is finite and not the unsmoothed one's; 1 - cos to the fp32 oracle stays within the bound
    tests/test_attention_pv8.py::test_tiny_dit_forward holds the e4m3 P V form to: 2 d_recipe, d_recipe = 1 - cos(the oracle's bf16
    forward with its self-attention replaced by the emulation of the e4m3 recipe, the oracle's fp32 forward)."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, sd, cfg = qk8.tiny_model()
    args = tiny_args()
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    try:
        with torch.no_grad():
            out_bf16 = model_fn_wan_video(m, **args)
            out_cross = model_fn_wan_video(m.enable_qk8_attention(fused_producer=True, pv8=True, cross=True), **args)
            monkeypatch.setattr(hip, "_call", call)
            out_s = model_fn_wan_video(m.enable_qk8_attention(fused_producer=True, pv8=True, cross=True, smooth_v_cross=True), **args)
            monkeypatch.setattr(hip, "_call", real)
    finally:
        m.enable_qk8_attention(False)
    nb = cfg["num_layers"]
    assert calls.count("fg_attn_fwd_cross8s_bf16") == nb and calls.count("fg_attn_quant_vt_smooth_bf16") == nb
    assert calls.count("fg_attn_fwd_cross8_bf16") == 0, "cross-attention still reaches the unsmoothed kernel"
    # self-attention keeps the unsmoothed e4m3 P V form: its V producer and its kernel, once per block
    assert calls.count("fg_attn_quant_vt_bf16") == nb and calls.count("fg_attn_fwd_pv8_bf16") == nb and calls.count("fg_attn_fwd_pv8s_bf16") == 0
    assert calls.count("fg_attn_fwd_bf16") == 0
    assert torch.isfinite(out_s.float()).all()
    assert not torch.equal(out_s, out_cross) and not torch.equal(out_s, out_bf16), "the switch is dead"
    want32, want_emu = tiny_oracle()
    cos = qk8.cos_distance
    d_recipe = cos(want_emu, want32)
    d_s, d_cross, d_bf16 = cos(out_s, want32), cos(out_cross, want32), cos(out_bf16, want32)
    print(f"tiny DiT, 1 200 tokens, 512 context rows ({L_TEXT} live): 1 - cos to the fp32 oracle: pv8 recipe in the bf16 oracle {d_recipe:.3e}, "
          f"cross8s kernels {d_s:.3e}, cross8 kernels {d_cross:.3e}, bf16 kernels {d_bf16:.3e}; cross8s to cross8 kernels {cos(out_s, out_cross):.3e}")
    assert d_s <= 2 * d_recipe, (d_s, d_recipe)


@gpu
def test_kv_cache_quantises_a_context_once(hip, monkeypatch):  # noqa: F811
    """Two forwards with one kv_cache: each block's context is projected and quantised in the first only, the cache holds
    (k8, sk, v8t, sv, mu), and the second forward gives the bits of the first."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, _, cfg = qk8.tiny_model()
    args, nb = tiny_args(), cfg["num_layers"]
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(hip, "_call", call)
    try:
        with torch.no_grad():
            m.enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True)      # two-step producers: self-attention does not use fg_attn_quant_k_bf16
            cache = {}
            first = model_fn_wan_video(m, kv_cache=cache, **args)
            names = ("fg_attn_quant_k_bf16", "fg_rmsnorm_rope_kstats_bf16", "fg_attn_quant_vt_smooth_bf16", "fg_attn_quant_vt_bf16")
            per_forward = {n_: calls.count(n_) for n_ in names}
            second = model_fn_wan_video(m, kv_cache=cache, **args)
    finally:
        m.enable_qk8_attention(False)
    assert per_forward == dict(zip(names, (nb, nb, nb, nb)))
    assert all(calls.count(n_) == nb for n_ in names[:3]), "a context was quantised twice"
    assert calls.count("fg_attn_quant_vt_bf16") == 2 * nb and calls.count("fg_attn_fwd_cross8s_bf16") == 2 * nb
    assert torch.equal(first, second)
    (entry,) = cache["entries"]
    for i in range(nb):
        assert len(entry["kv"][i]) == 5
        k8, sk, v8t, sv, mu = entry["kv"][i]
        assert (k8.dtype, sk.dtype, v8t.dtype, sv.dtype, mu.dtype) == (F8, F32, F8, F32, F32)
        assert k8.shape == (L_CTX, 256) and sk.shape == (2,) and v8t.shape == (2, 128, L_CTX) and sv.shape == mu.shape == (2, 128)


@gpu
def test_graph_loop_equals_eager(hip):  # noqa: F811
    """graph=True on the tiny loop with the mode on: the context is quantised in the eager first step into the loop's kv_cache, mu with
    it, the replayed steps only read it, and they give the bits of the eager loop."""
    from fairygen_amd.wan_video import WanVideoPipeline
    m, _, _ = qk8.tiny_model()
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True)
    lat, ctx_p, ctx_n = seeded(qk8.LATENT, 21), padded_context(22), padded_context(23, 7)
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
        pipe.dit.enable_qk8_attention(pv8=True, cross=True)
        assert not torch.equal(loop(False), want), "the loop above ran without the smoothed V"
    finally:
        m.enable_qk8_attention(False)


@gpu
def test_stacked_equals_element_by_element(hip, monkeypatch):  # noqa: F811
    """The stacked CFG forward of the tiny DiT with the mode on (the fused producers, as the loader sets them), a context batch of 2: the
    context goes through fg_attn_quant_vt_smooth_bf16_b, cross-attention through fg_attn_fwd_cross8s_bf16_b, and the merged call equals
    the element-by-element one bit for bit.  Wrapped to run per element, as in tests/test_stacked_cfg_forward.py: the GEMM seams (a library
    GEMM may pick another solution for 2 N rows) and hip.attention.  Nothing of the e4m3 chain is wrapped."""
    from fairygen_amd import wan_video_dit as D
    m, _, cfg = qk8.tiny_model()
    monkeypatch.setattr(D, "GEMM_BACKEND", "lib")
    stacked._wrap_plans(monkeypatch)
    lat, ts = seeded(qk8.LATENT, 31).cuda(), torch.tensor([500.0]).to(BF16)
    both = torch.cat([padded_context(32), padded_context(33, 7)], 0).cuda()
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    m.enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True, fused_producer=True)
    try:
        want = stacked._merged(m, False, lat, ts, both)
        monkeypatch.setattr(hip, "_call", call)
        got = stacked._merged(m, True, lat, ts, both)
        monkeypatch.setattr(hip, "_call", real)
    finally:
        m.enable_qk8_attention(False)
    nb = cfg["num_layers"]
    assert calls.count("fg_attn_fwd_cross8s_bf16_b") == nb and calls.count("fg_attn_quant_vt_smooth_bf16_b") == nb
    assert calls.count("fg_attn_fwd_cross8_bf16_b") == 0 and calls.count("fg_attn_fwd_cross8s_bf16") == 0
    assert got.shape == want.shape and got.shape[0] == 2
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} elements differ"
    assert not torch.equal(got[0], got[1])

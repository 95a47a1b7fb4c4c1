"""Pins the CPU oracle against vectors produced by the reference's own code (oracle/gen_golden.py).

Same dtype + same op order => the bf16 comparisons are bit-exact; the two places where the oracle's
formulation differs from the reference's module code by a mathematically equal rewrite are given a stated
tolerance of one bf16 ulp.
"""
import pytest
import torch

from conftest import seeded
from oracle import pipeline as opipe
from oracle import wan_dit, wan_text, wan_vae
from fairygen_amd import synthetic


def test_dit_primitives(golden):
    g = golden("dit_primitives.safetensors")
    x = seeded((1, 24, 256), 11)
    table = wan_dit.rope_table_3d(128, 2, 3, 4)
    assert torch.equal(table.real.contiguous(), g["rope_table_real"]) and torch.equal(table.imag.contiguous(), g["rope_table_imag"])
    assert torch.equal(wan_dit.rope_apply(x, table, 2), g["rope_out"])
    assert torch.equal(wan_dit.sinusoid_1d(256, torch.tensor([0.0, 996.0, 92.5], dtype=torch.bfloat16)), g["sinusoid_bf16"])
    assert torch.equal(wan_dit.sinusoid_1d(256, torch.tensor([0.0, 995.9, 92.59])), g["sinusoid_f32"])
    w = (1 + 0.1 * seeded((256,), 12, torch.float32)).to(torch.bfloat16)
    assert torch.equal(wan_dit.rms_norm(x, w, 1e-6), g["rmsnorm_out"])
    mod = wan_dit.layer_norm(x, 1e-6) * (1 + seeded((1, 1, 256), 14)) + seeded((1, 1, 256), 13)
    assert torch.equal(mod, g["modulate_out"])
    q, k, v = seeded((1, 80, 256), 15), seeded((1, 50, 256), 16), seeded((1, 50, 256), 17)
    assert torch.equal(wan_dit.attention(q, k, v, 2), g["attn_out_bf16"])
    assert torch.allclose(wan_dit.attention(q.float(), k.float(), v.float(), 2), g["attn_out_f32"], atol=1e-6)
    assert torch.equal(x + seeded((1, 1, 256), 18) * seeded((1, 24, 256), 19), g["gate_out"])


def _tiny_inputs():
    lat = seeded((1, 48, 3, 8, 8), 1)
    ctx_p = seeded((1, 16, 128), 2); ctx_p[:, 10:] = 0
    ctx_n = seeded((1, 16, 128), 3); ctx_n[:, 12:] = 0
    return lat, ctx_p, ctx_n, seeded((1, 48, 1, 8, 8), 4), torch.tensor([995.9]).to(torch.bfloat16)


def test_dit_tiny_forward_and_loop(golden):
    g = golden("dit_tiny.safetensors")
    cfg = synthetic.TINY_DIT_KWARGS
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    lat, ctx_p, ctx_n, z0, ts = _tiny_inputs()
    assert torch.equal(wan_dit.model_fn(sd, cfg, lat, ts, ctx_p, True), g["ti2v_bf16"])
    assert torch.equal(wan_dit.model_fn(sd, cfg, lat, ts, ctx_p, False), g["t2v_bf16"])
    sd32 = {k: v.float() for k, v in sd.items()}
    assert torch.allclose(wan_dit.model_fn(sd32, cfg, lat.float(), ts.float(), ctx_p.float(), True), g["ti2v_f32"], atol=2e-5, rtol=1e-5)
    rec = []
    opipe.denoise_loop(sd, cfg, lat, ctx_p, ctx_n, 4, 5.0, 5.0, z0, record=rec)
    for i, r in enumerate(rec):
        assert torch.equal(r, g[f"loop_step{i}"]), f"loop step {i}"


def test_teacache_loop(golden):
    """TeaCache (step skipping) restatement == the reference's TeaCache inside its model_fn, step for step: same
    skipped steps (the accumulated distances match) and bit-identical latents, in TI2V and T2V timestep modes."""
    g = golden("serving.safetensors")
    cfg = synthetic.TINY_DIT_KWARGS
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    lat, ctx_p, ctx_n, z0, _ = _tiny_inputs()
    assert g["ti2v_skipped"][:, 0].tolist() == [0, 1, 1, 0, 1, 0, 1, 0] and g["t2v_skipped"].sum().item() == 0
    assert g["t2v_skip_skipped"][:, 0].tolist() == [0, 1, 1, 0, 1, 0, 0, 0]      # T2V mode WITH skipped steps (threshold 100)
    for mode, first, thresh in (("ti2v", z0, 25.0), ("t2v", None, 25.0), ("t2v_skip", None, 100.0)):
        rec = []
        opipe.denoise_loop(sd, cfg, lat, ctx_p, ctx_n, 8, 5.0, 5.0, first, record=rec,
                           tea_cache_l1_thresh=thresh, tea_cache_model_id="Wan2.1-I2V-14B-720P")
        for i, r in enumerate(rec):
            assert torch.equal(r, g[f"{mode}_step{i}"]), f"{mode} step {i}"
    with pytest.raises(ValueError):
        wan_dit.TeaCache(4, 0.1, "Wan2.2-TI2V-5B")


def test_hot_lora_linear(golden):
    g = golden("serving.safetensors")
    x = seeded((1, 40, 256), 91)
    w, b = seeded((384, 256), 92, scale=0.05), seeded((384,), 93, scale=0.1)
    a1, b1 = seeded((4, 256), 94, scale=0.05), seeded((384, 4), 95, scale=0.05)
    a2, b2 = seeded((8, 256), 96, scale=0.05), seeded((384, 8), 97, scale=0.05)
    assert torch.equal(opipe.hot_lora_linear(x, w, b, [(a1 * 0.5, b1), (a2 * 2, b2)]), g["hot_lora_out"])


def test_fp8_linear_restatement():
    """fp8_linear has no golden vector (the reference's row-wise torch._scaled_mm call does not run on this container's
    CPU backend: parity unpinned).  What can be pinned here: the written-out scaled matmul equals the real CPU
    torch._scaled_mm for unit scales, and the quantisation follows the reference's formulae on a case that scales down."""
    x = seeded((1, 12, 64), 101)
    x[0, 3] *= 300.0                                         # one row above the fp8 range: scale_a > 1 there
    w, b = seeded((32, 64), 102, scale=0.05), seeded((32,), 103, scale=0.1)
    out = wan_dit.fp8_linear(x, w, b)
    assert out.dtype == torch.bfloat16 and out.shape == (1, 12, 32)
    x2 = x.reshape(-1, 64)
    scale_a = torch.clamp(x2.abs().amax(-1, keepdim=True) / 448.0, min=1.0).float()
    assert scale_a[3].item() > 1.0 and (scale_a[[0, 1, 2]] == 1.0).all()
    xq, wq = (x2 / (scale_a + 1e-8)).to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn)
    assert xq.float().abs().max().item() <= 448.0
    one = torch.ones(())
    keep = [0, 1, 2] + list(range(4, 12))                    # rows with unit scale: the real op applies
    real = torch._scaled_mm(xq[keep], wq.T, scale_a=one, scale_b=one, bias=b, out_dtype=torch.bfloat16)
    assert torch.equal(out[0, keep], real)
    ref = torch.nn.functional.linear(x, w, b)
    rel = (out.float() - ref.float()).abs().mean() / ref.float().abs().mean()
    assert rel < 0.08                                         # e4m3 weights of magnitude 0.05: ~4 % mean error


def test_fp8_linear_vs_reference_golden(golden):
    """The reference's own AutoWrappedLinear.fp8_linear (core/vram/layers.py:321-357), run by oracle/gen_fp8_linear_1x1.py on the one
    shape this container's CPU torch._scaled_mm accepts with its (rows, 1) / (1, out) scales — one row x one output — for 64 cases
    (K = 3072 and 14336, row maxima below, around and far above fp8_max): the restatement must reproduce every output, calling it
    both one case at a time and with all rows / all weight rows at once (the diagonal: per-row scales do not mix rows)."""
    g = golden("fp8_linear_1x1.safetensors")
    for k in (3072, 14336):
        x, w, b, want = g[f"x_{k}"], g[f"w_{k}"], g[f"b_{k}"], g[f"out_{k}"]
        assert (x.float().abs().amax(-1) > 448).any() and (x.float().abs().amax(-1) < 448).any()
        one = torch.cat([wan_dit.fp8_linear(x[i:i + 1], w[i:i + 1], b[i:i + 1]).reshape(1) for i in range(x.shape[0])])
        assert torch.equal(one, want)
        full = wan_dit.fp8_linear(x, w, b)                      # (cases, cases): entry (i, i) is case i
        assert torch.equal(torch.diagonal(full), want)


def test_sliding_window_model_fn(golden):
    g = golden("serving.safetensors")
    cfg = synthetic.TINY_DIT_KWARGS
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    _, ctx_p, _, _, _ = _tiny_inputs()
    got = wan_dit.model_fn_sliding(sd, cfg, seeded((1, 48, 7, 8, 8), 98), torch.tensor([700.0]).to(torch.bfloat16), ctx_p, 4, 2)
    assert torch.equal(got, g["sliding_window_out"])


def test_oracle_full_width_config1(golden):
    """The oracle at the FULL Wan2.2-TI2V-5B widths (30 blocks, dim 3072) on BASELINE.json configs[0]: the first two denoise
    steps must equal, bit for bit, the latents the reference's own code produced (oracle/gen_config1.py; there all four
    steps and the decoded video were bit-identical, reference 25.0 s vs restatement 24.1 s per clip on 8 cores)."""
    from fairygen_amd.loader import TI2V_5B_DIT_KWARGS
    g = golden("config1.safetensors")
    cfg = dict(TI2V_5B_DIT_KWARGS)
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    noise = seeded((1, 48, 5, 16, 16), 1)
    ctx_p = seeded((1, 512, 4096), 2); ctx_p[:, 64:] = 0
    ctx_n = seeded((1, 512, 4096), 3); ctx_n[:, 128:] = 0
    z0 = seeded((1, 48, 1, 16, 16), 4)
    sig, ts = opipe.wan_sigmas(4, shift=5.0)
    lat = noise.clone()
    lat[:, :, 0:1] = z0
    with torch.no_grad():
        for i in range(2):
            t = ts[i].unsqueeze(0).to(torch.bfloat16)
            posi = wan_dit.model_fn(sd, cfg, lat, t, ctx_p, True)
            nega = wan_dit.model_fn(sd, cfg, lat, t, ctx_n, True)
            lat = opipe.euler_step(nega + 5.0 * (posi - nega), i, lat, sig)
            lat[:, :, 0:1] = z0
            assert torch.equal(lat, g[f"latents_step{i}"]), f"step {i}"


def test_config2_loop_fixture_parts_and_pin(golden):
    """tests/golden/config2_loop.part{0,1,2}.safetensors (oracle/gen_config2_loop.py, cut along the last dimension): the parts join to
    the stored shapes, and frame 0 of every step equals the sampled channels of the TI2V first frame bit for bit in the reference's bf16
    loop and in the fp32 one (the pin after every step, and a check that the parts are joined in order)."""
    g = golden("config2_loop.safetensors")
    assert sorted(g) == sorted(f"{kind}_step{k}" for kind in ("ref_bf16", "f32") for k in range(3))
    z0 = seeded((1, 48, 1, 30, 52), 4)[:, ::8]
    for k in range(3):
        ref, f32 = g[f"ref_bf16_step{k}"], g[f"f32_step{k}"]
        assert ref.dtype == torch.bfloat16 and f32.dtype == torch.float32
        assert ref.shape == f32.shape == (1, 6, 13, 30, 52)
        assert torch.equal(ref[:, :, 0:1], z0) and torch.equal(f32[:, :, 0:1], z0.float()), f"step {k}"
        if k:
            assert not torch.equal(ref[:, :, 1:], g[f"ref_bf16_step{k - 1}"][:, :, 1:])


def test_scheduler(golden):
    g = golden("scheduler.safetensors")
    for n in (4, 30, 50):
        s, t = opipe.wan_sigmas(n, shift=5.0)
        assert torch.equal(s, g[f"sigmas_{n}"]) and torch.equal(t, g[f"timesteps_{n}"])
    s, _ = opipe.wan_sigmas(4, shift=5.0)
    xs, vs = seeded((1, 4, 2, 3, 3), 21), seeded((1, 4, 2, 3, 3), 22)
    for i in range(4):
        assert torch.equal(opipe.euler_step(vs, i, xs, s), g[f"step_{i}"])


def test_lora_fuse_and_merge(golden):
    g = golden("lora.safetensors")
    cfg = synthetic.TINY_DIT_KWARGS
    shapes = synthetic.dit_shapes(cfg)
    sd = synthetic.random_state_dict(shapes, seed=1234)
    lora = synthetic.random_lora(shapes, rank=4, seed=4321)
    assert opipe.fuse_lora(sd, lora, alpha=0.5) == 20
    for k in ("blocks.0.self_attn.q.weight", "blocks.1.cross_attn.v.weight", "blocks.1.ffn.2.weight", "blocks.0.ffn.0.weight",
              "blocks.0.self_attn.q.bias"):
        assert torch.equal(sd[k], g[k]), k
    stage2 = {k.replace(".lora_B.default.weight", ".lora_B2.weight"): seeded(v.shape, 77 + i, scale=0.02)
              for i, (k, v) in enumerate(sorted(lora.items())) if ".lora_B." in k}
    merged = opipe.merge_stage_loras(lora, stage2)
    assert len(merged) == int(g["merged_num_keys"])
    assert torch.equal(merged["blocks.0.self_attn.q.lora_B.default.weight"], g["merged.blocks.0.self_attn.q.lora_B"])
    assert torch.equal(merged["blocks.1.ffn.0.lora_A.default.weight"], g["merged.blocks.1.ffn.0.lora_A"])


def test_vae_tiny_decode(golden):
    g = golden("vae_tiny.safetensors")
    sd = synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=32, dim=32), seed=1234)
    z = seeded((1, 48, 3, 4, 6), 31)
    assert torch.equal(wan_vae.vae_decode(sd, z, tiled=False), g["decode_bf16"])
    assert torch.equal(wan_vae.vae_decode(sd, z, tiled=True, tile_size=(3, 4), tile_stride=(2, 2)), g["tiled_bf16"])
    sd32 = {k: v.float() for k, v in sd.items()}
    assert torch.allclose(wan_vae.vae_decode(sd32, z.float(), tiled=False), g["decode_f32"], atol=1e-5, rtol=1e-5)


def test_vae_tiny_decode_long(golden):
    """11 latent frames (41 video frames): the oracle's one-frame-per-call decode against the reference's (oracle/gen_vae_long.py)."""
    g = golden("vae_long.safetensors")
    sd = synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=32, dim=32), seed=1234)
    z = seeded((1, 48, 11, 2, 2), 36)
    assert torch.equal(wan_vae.vae_decode(sd, z, tiled=False), g["decode_bf16"])
    sd32 = {k: v.float() for k, v in sd.items()}
    assert torch.allclose(wan_vae.vae_decode(sd32, z.float(), tiled=False), g["decode_f32"], atol=1e-5, rtol=1e-5)


def test_vae_tiny_encode(golden):
    g = golden("vae_tiny.safetensors")
    sd = synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=32, dim=32), seed=1234)
    img = seeded((3, 1, 64, 96), 32, scale=0.5).clamp(-1, 1)
    vid = seeded((3, 9, 64, 96), 33, scale=0.5).clamp(-1, 1)
    assert torch.equal(wan_vae.vae_encode(sd, [img]), g["encode_image_bf16"])
    assert torch.equal(wan_vae.vae_encode(sd, [vid]), g["encode_video_bf16"])
    assert torch.equal(wan_vae.vae_encode(sd, [img], True, (3, 4), (2, 2)), g["encode_image_tiled_bf16"])
    sd32 = {k: v.float() for k, v in sd.items()}
    assert torch.allclose(wan_vae.vae_encode(sd32, [img.float()]), g["encode_image_f32"], atol=1e-5, rtol=1e-5)


def _tiny_text_sd():
    tkw = synthetic.TINY_TEXT_KWARGS
    sd = synthetic.random_state_dict(synthetic.text_encoder_shapes(tkw), seed=1234)
    return {k: (v * 3 if v.dim() == 2 else v) for k, v in sd.items()}, tkw


def test_text_encoder_tiny(golden):
    g = golden("text_tiny.safetensors")
    sd, tkw = _tiny_text_sd()
    assert torch.equal(wan_text.text_encoder(sd, g["ids"], g["mask"], tkw["num_heads"]), g["encoder_bf16"])
    assert torch.equal(wan_text.encode_prompt(sd, g["ids"], g["mask"], tkw["num_heads"]), g["prompt_emb_bf16"])
    sd32 = {k: v.float() for k, v in sd.items()}
    assert torch.allclose(wan_text.text_encoder(sd32, g["ids"], g["mask"], tkw["num_heads"]), g["encoder_f32"], atol=1e-5, rtol=1e-5)


def test_pixels_and_noise(golden):
    g = golden("pixels.safetensors")
    assert torch.equal(opipe.generate_noise((1, 48, 2, 4, 4), 1), g["noise_seed1"])
    vid = seeded((1, 3, 2, 8, 8), 41, scale=0.7).clamp(-1.2, 1.2)
    assert torch.equal(opipe.video_to_uint8(vid[0]), g["uint8_frames"])

"""Hot-loaded LoRA adapters on the HIP backend in the fp8 Linear mode (`enable_fp8_linear()` + `hot_backend="hip"`): the dual-output norm
kernels (bf16 row + e4m3 row + scale in one pass), the host path that puts the residual / gate adds into fg_gemm_fp8_bf16's store and the
low-rank term on fg_lora_apply_bf16, and the fp8 mode at model width.

Exact checks: the new kernels against the existing ones byte for byte; zero adapters and clear_lora() against the adapter-free fp8 model;
the launches really taken.  Numeric checks, the criterion of tests/test_hot_lora_kernel.py: max|hip - f32| <= 2 * max|torch - f32| + 1e-2,
`torch` = the same fp8 model with hot_backend="torch" (the reference's ops one by one), `f32` = the oracle with fp32 activations on
oracle.wan_dit.Fp8Blocks weights and the adapters added unfused per Linear (AutoWrappedLinear.forward, core/vram/layers.py:429-436:
fp8_linear(x), then lora_forward on the same x)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import seeded
from fairygen_amd import hip, synthetic
from oracle import pipeline as opipe
from oracle import wan_dit as odit


def dev(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------- kernels
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [77, 80])      # 77: the last workgroup (4 rows) is partly empty
def test_dual_output_norms(rows):
    """fg_ln_modulate_dual_bf16 / fg_ln_affine_dual_bf16 on the inputs of test_fp8_output_norms (shifts / a bias of 900 push row maxima
    above 448): e4m3 bytes and scales equal the fp8-output kernel's (and fg_fp8_quant_rows_bf16's on the bf16 row), the bf16 row equals
    hip.ln_modulate / hip.ln_affine bit for bit, and the rows after each output stay untouched."""
    C, guard = 3072, 3
    x, y = seeded((1, rows, C), 51), seeded((1, rows, C), 52)
    table = seeded((2, 6, C), 53, scale=0.5)
    table[1, 0, 7] = table[0, 3, 9] = 900.0
    mod = hip.ModTable(dev(table), 30)
    w, b = (1 + 0.1 * seeded((C,), 54)).to(torch.bfloat16), (0.1 * seeded((C,), 55)).to(torch.bfloat16)
    b[11] = 900.0
    real_rows_out = hip._fp8_rows_out

    def guarded(call, x_in):
        """Run a dual wrapper with all three outputs carved out of larger buffers filled with a guard pattern."""
        out16 = torch.full((1, rows + guard, C), 7.0, dtype=torch.bfloat16, device="cuda")
        q = torch.full((rows + guard, C), 0x55, dtype=torch.uint8, device="cuda")
        sc = torch.full((rows + guard, 1), -3.0, dtype=torch.float32, device="cuda")
        hip._fp8_rows_out = lambda _x: (q[:rows].view(torch.float8_e4m3fn), sc[:rows])
        try:
            o, (q8, s) = call(x_in, out16[:, :rows])
        finally:
            hip._fp8_rows_out = real_rows_out
        torch.cuda.synchronize()
        assert (out16[:, rows:] == 7.0).all() and (q[rows:] == 0x55).all() and (sc[rows:] == -3.0).all(), "guard rows"
        return o, (q8, s)

    def same(got, bf16_rows, pair):
        o, (q8, s) = got
        assert torch.equal(o.view(torch.int16), bf16_rows.view(torch.int16)), "bf16 row"
        assert torch.equal(q8.view(torch.uint8), pair[0].view(torch.uint8)) and torch.equal(s, pair[1]), "fp8-output kernel"
        qq, ss = hip.fp8_quant_rows(bf16_rows)
        assert torch.equal(q8.view(torch.uint8), qq.view(torch.uint8)) and torch.equal(s, ss), "fp8_quant_rows of the bf16 row"
        assert s.max().item() > 1.0

    for si, ci in ((0, 1), (3, 4)):
        got = guarded(lambda t, o: hip.ln_modulate_dual(t, mod, si, ci, 1e-6, out=o), dev(x))
        same(got, hip.ln_modulate(dev(x), mod, si, ci, 1e-6), hip.ln_modulate_fp8(dev(x), mod, si, ci, 1e-6))
    # norm3 has no fp8-output form without a residual input: the residual kernel's pair on the same residual stream
    xo, pair = hip.residual_ln_affine_fp8(dev(x), dev(y), dev(w), dev(b), 1e-6, mod, 2)
    got = guarded(lambda t, o: hip.ln_affine_dual(t, dev(w), dev(b), 1e-6, out=o), xo)
    same(got, hip.ln_affine(xo, dev(w), dev(b), 1e-6), pair)
    # without `out` the wrappers allocate
    o, (q8, s) = hip.ln_affine_dual(xo, dev(w), dev(b), 1e-6)
    assert o.shape == xo.shape and q8.shape == (rows, C) and q8.dtype == torch.float8_e4m3fn and s.shape == (rows, 1)


def test_dual_norm_argument_checks():
    """The new entry points check their arguments on the host (nothing is launched); the wrappers refuse CPU tensors."""
    lib = hip.load()
    p16, p8 = ctypes.c_void_p(16), ctypes.c_void_p(8)

    def modulate(x=p16, out=p16, out8=p16, scale=p16, fp8_max=448.0, c=256):
        return lib.fg_ln_modulate_dual_bf16(x, p16, p16, out, out8, scale, 64, c, 1e-6, 1, 0, 6 * 256, fp8_max, None)

    def affine(x=p16, out=p16, out8=p16, scale=p16, fp8_max=448.0, c=256):
        return lib.fg_ln_affine_dual_bf16(x, p16, p16, out, out8, scale, 64, c, 1e-6, fp8_max, None)
    for name, call in (("fg_ln_modulate_dual_bf16", modulate), ("fg_ln_affine_dual_bf16", affine)):
        assert call(x=p8) == -1 and b"16-byte aligned" in lib.fg_last_error() and name.encode() in lib.fg_last_error()
        assert call(out=p8) == -1 and b"16-byte aligned" in lib.fg_last_error()
        assert call(out8=ctypes.c_void_p(4)) == -1 and b"16-byte aligned" in lib.fg_last_error()
        assert call(fp8_max=0.0) == -1 and b"fp8_max positive" in lib.fg_last_error()
        assert call(fp8_max=-448.0) == -1 and b"fp8_max positive" in lib.fg_last_error()
        assert call(scale=None) == -1 and b"null pointer" in lib.fg_last_error()
        assert call(c=4100) == -1 and b"C % 8" in lib.fg_last_error()
    q = seeded((1, 8, 256), 1)
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        hip.ln_affine_dual(q, q[0, 0], q[0, 0], 1e-6)
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        hip.ln_modulate_dual(q, None, 0, 1, 1e-6)


@pytest.mark.gpu
def test_gelu_forms_agree_after_e4m3_at_unit_scale():
    """The adapter kernel applies the GEMM epilogue's GELU(tanh), the adapter-free fp8 mode the elementwise one inside
    fg_fp8_quant_rows_bf16; as bf16 values they differ on 164 inputs in [-6, -3] (|GELU| < 4e-3).  What ffn.2's fp8 Linear reads is
    the e4m3 form: for every finite bf16 input below fp8_max (row scale 1) the two e4m3 values are equal (the bytes differ for the
    input -0 alone: +0 against -0), which is what makes a zero adapter on ffn.0 reproduce the adapter-free fp8 model."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    ok = torch.isfinite(bits.float()) & (bits.float().abs() < 448.0)
    pre = torch.where(ok, bits, torch.zeros_like(bits)).view(256, 256).cuda()
    zero_a, zero_b = torch.zeros((32, 256), dtype=torch.bfloat16, device="cuda"), torch.zeros((256, 32), dtype=torch.bfloat16, device="cuda")
    f = hip.lora_apply(seeded((256, 256), 3).cuda(), zero_a, zero_b, pre.clone(), mode="gelu_tanh")
    (q_new, s_new), (q_old, s_old) = hip.fp8_quant_rows(f), hip.fp8_quant_rows(pre, "gelu_tanh")
    assert s_new.max().item() == 1.0 and torch.equal(s_new, s_old)
    assert torch.equal(q_new.float(), q_old.float())
    assert (q_new.view(torch.uint8) != q_old.view(torch.uint8)).sum().item() <= 1


# ------------------------------------------------------------------------------------------- model level: helpers
def _cos(a, b):
    return F.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0).item()


def _zero_b(lora):
    return {k: (torch.zeros_like(v) if ".lora_B" in k else v) for k, v in lora.items()}


def _only(lora, name):
    return {k: v for k, v in lora.items() if k.startswith(name + ".")}


def _oracle_adapters(loras):
    """name -> [(alpha * A, B), ...] in fp32, as base_pipeline.py:258-259 stores hot-loaded adapters."""
    out = {}
    for lo, alpha in loras:
        for name, (kb, ka) in opipe.lora_name_map(lo).items():
            out.setdefault(name, []).append((alpha * lo[ka].float(), lo[kb].float()))
    return out


def _with_lora_forward(monkeypatch, adapters):
    """oracle.wan_dit.linear followed by lora_forward's sum on the same input (core/vram/layers.py:417-436)."""
    real = odit.linear

    def linear(sd, prefix, x):
        out = real(sd, prefix, x)
        for a, b in adapters.get(prefix, ()):
            out = out + x @ a.to(x.dtype).T @ b.to(x.dtype).T
        return out
    monkeypatch.setattr(odit, "linear", linear)


class _Counts:
    """Counts the hip.* calls that tell the code paths apart."""

    def __init__(self, monkeypatch):
        self.lora, self.gemm8, self.quant, self.norm_rows = [], [], [], []      # norm_rows keeps the tensors: no address is reused

        def wrap(name, note):
            real = getattr(hip, name)      # AttributeError where the entry point does not exist

            def fn(*a, **k):
                out = real(*a, **k)
                note(a, k, out)
                return out
            monkeypatch.setattr(hip, name, fn)
        wrap("lora_apply", lambda a, k, out: self.lora.append(k.get("mode", "add")))
        wrap("gemm_fp8", lambda a, k, out: self.gemm8.append(bool(k.get("residual", False))))
        wrap("fp8_quant_rows", lambda a, k, out: self.quant.append((a[0], a[1] if len(a) > 1 else k.get("act"))))
        for name in ("ln_modulate", "ln_affine"):
            wrap(name, lambda a, k, out: self.norm_rows.append(out))
        for name in ("ln_modulate_dual", "ln_affine_dual"):
            wrap(name, lambda a, k, out: self.norm_rows.append(out[0]))
        for name in ("residual_ln_modulate", "residual_ln_affine"):
            wrap(name, lambda a, k, out: self.norm_rows.append(out[1]))

    def reset(self):
        del self.lora[:], self.gemm8[:], self.quant[:], self.norm_rows[:]


# ------------------------------------------------------------------------------------------- tiny DiT
def _tiny_pipe(sd, cfg, fp8=True):
    from fairygen_amd.wan_video import WanVideoPipeline
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
    pipe.dit = m.to(device="cuda", dtype=torch.bfloat16).eval()
    if fp8:
        pipe.dit.enable_fp8_linear()
    return pipe


def _tiny_setup():
    cfg = synthetic.TINY_DIT_KWARGS
    shapes = synthetic.dit_shapes(cfg)
    sd = synthetic.random_state_dict(shapes, seed=1234)
    lat, ctx, ts = seeded((1, 48, 3, 8, 8), 1), seeded((1, 16, 128), 2), torch.tensor([995.9]).to(torch.bfloat16)
    ctx[:, 10:] = 0

    def fwd(pipe):
        from fairygen_amd.wan_video import model_fn_wan_video
        with torch.no_grad():
            return model_fn_wan_video(pipe.dit, latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
    return cfg, shapes, sd, (lat, ctx, ts), fwd


@pytest.mark.gpu
def test_tiny_dit_fp8_zero_adapter_clear_and_mode_switch(monkeypatch):
    """Tiny DiT (dim 256, ffn 512: shapes the own fp8 GEMM takes), fp8 on, hot_backend="hip": rank-32 adapters with B = 0 — on all
    Linears, and on one Linear only (the others take the fused stores without an adapter) — give the adapter-free fp8 output bit for
    bit; so does clear_lora() after real adapters; enable_fp8_linear(None) with the adapters still loaded gives the bf16 hip-backend
    output of a model that never was in the fp8 mode."""
    cfg, shapes, sd, _, fwd = _tiny_setup()
    assert cfg["dim"] % 256 == 0 and cfg["ffn_dim"] % 256 == 0
    counts = _Counts(monkeypatch)
    out_fp8 = fwd(_tiny_pipe(sd, cfg))
    assert counts.lora == [] and not any(counts.gemm8) and len(counts.gemm8) == 7 * cfg["num_layers"]
    lora = synthetic.random_lora(shapes, rank=32, seed=4321)
    for zero, n_apply in ((_zero_b(lora), 6 * cfg["num_layers"]), (_only(_zero_b(lora), "blocks.0.self_attn.q"), 1), (_only(_zero_b(lora), "blocks.1.ffn.2"), 1)):
        pipe = _tiny_pipe(sd, cfg)
        pipe.load_lora(pipe.dit, state_dict=zero, alpha=1.0, hotload=True, hot_backend="hip")
        counts.reset()
        out = fwd(pipe)
        assert counts.gemm8.count(True) == 3 * cfg["num_layers"] and len(counts.lora) == n_apply
        assert torch.equal(out, out_fp8)
    pipe = _tiny_pipe(sd, cfg)
    pipe.load_lora(pipe.dit, state_dict=lora, alpha=2.0, hotload=True, hot_backend="hip")
    out_hot = fwd(pipe)
    assert not torch.equal(out_hot, out_fp8)
    never_fp8 = _tiny_pipe(sd, cfg, fp8=False)
    never_fp8.load_lora(never_fp8.dit, state_dict=lora, alpha=2.0, hotload=True, hot_backend="hip")
    pipe.dit.enable_fp8_linear(None)
    assert torch.equal(fwd(pipe), fwd(never_fp8))
    pipe.dit.enable_fp8_linear()
    assert torch.equal(fwd(pipe), out_hot)
    pipe.clear_lora()
    assert pipe.dit.hot_loras == {} and pipe.dit.hot_lora_backend == "hip" and torch.equal(fwd(pipe), out_fp8)


@pytest.mark.gpu
def test_tiny_dit_fp8_hot_backend_hip_vs_oracle(monkeypatch):
    """The configuration of test_tiny_dit_hot_backend_hip in the fp8 mode: one adapter, two stacked adapters of different alpha, and
    five rank-32 adapters stacked on one Linear (rank 160 > 128: that Linear stays on WanModel._hot, the others take the new path)."""
    cfg, shapes, sd, (lat, ctx, ts), fwd = _tiny_setup()
    layers = cfg["num_layers"]
    lora1, lora2 = synthetic.random_lora(shapes, rank=4, seed=4321), synthetic.random_lora(shapes, rank=8, seed=99)
    wide = "blocks.0.self_attn.o"
    five = [(synthetic.random_lora(shapes, rank=32, seed=200), 1.0)] + \
           [(_only(synthetic.random_lora(shapes, rank=32, seed=201 + j), wide), 0.5 + 0.25 * j) for j in range(4)]
    counts = _Counts(monkeypatch)
    sd32 = odit.Fp8Blocks({k: v.float() for k, v in sd.items()})
    real_linear = odit.linear
    for label, loras, n_apply in (("1 adapter", [(lora1, 2.0)], 6 * layers), ("2 adapters", [(lora1, 2.0), (lora2, 0.5)], 6 * layers),
                                  ("5 x rank 32 on one Linear", five, 6 * layers - 1)):
        hot_t, hot_h = _tiny_pipe(sd, cfg), _tiny_pipe(sd, cfg)
        for lo, alpha in loras:
            hot_t.load_lora(hot_t.dit, state_dict=lo, alpha=alpha, hotload=True, hot_backend="torch")
            hot_h.load_lora(hot_h.dit, state_dict=lo, alpha=alpha, hotload=True, hot_backend="hip")
        counts.reset()
        out_t = fwd(hot_t)
        assert counts.lora == [] and not any(counts.gemm8)
        counts.reset()
        out_h = fwd(hot_h)
        assert len(counts.lora) == n_apply and counts.lora.count("gelu_tanh") == layers, counts.lora
        # the Linear above the kernel's rank keeps its residual add out of the GEMM's store as well
        assert counts.gemm8.count(True) == 3 * layers - (n_apply != 6 * layers)
        monkeypatch.setattr(odit, "linear", real_linear)
        _with_lora_forward(monkeypatch, _oracle_adapters(loras))
        want = odit.model_fn(sd32, cfg, lat.float(), ts.float(), ctx.float(), fuse_vae_embedding_in_latents=True)
        monkeypatch.setattr(odit, "linear", real_linear)
        err_h, err_t = (out_h.float().cpu() - want).abs().max().item(), (out_t.float().cpu() - want).abs().max().item()
        print(f"tiny DiT fp8, {label}: max|hip-f32|={err_h:.4f} max|torch-f32|={err_t:.4f} max|f32|={want.abs().max().item():.2f}")
        assert err_h <= 2 * err_t + 1e-2


# ------------------------------------------------------------------------------------------- one full-width block
class _FullBlock:
    """One block at the model's width (the setup of test_full_width_block_hot_backend_hip: 5 070 tokens, dim 3 072, ffn 14 336)."""

    def __init__(self):
        from fairygen_amd.loader import TI2V_5B_DIT_KWARGS
        self.cfg = dict(TI2V_5B_DIT_KWARGS, num_layers=1)
        self.dim, self.nh, self.eps = self.cfg["dim"], self.cfg["num_heads"], self.cfg["eps"]
        self.shapes = {k: v for k, v in synthetic.dit_shapes(self.cfg).items() if k.startswith("blocks.0.")}
        self.sd = synthetic.random_state_dict(self.shapes, seed=7)
        self.lora = synthetic.random_lora(self.shapes, rank=32, seed=8)
        self.fhw = (3, 26, 65)
        n = 3 * 26 * 65
        self.x0, self.ctx, self.t_mod = seeded((1, n, self.dim), 11), seeded((1, 512, self.dim), 12), seeded((1, 6, self.dim), 13, scale=0.5)

    def run(self, lora=None, backend=None, fp8=True):
        """The residual stream after the block, on the device model."""
        from fairygen_amd import wan_video_dit as wd
        from fairygen_amd.wan_video import WanVideoPipeline
        with torch.device("meta"):
            m = wd.WanModel(**self.cfg)
        full = synthetic.random_state_dict(synthetic.dit_shapes(self.cfg), seed=1, device="cuda")
        full.update({k: v.cuda() for k, v in self.sd.items()})
        m.load_state_dict(full, assign=True)
        pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
        pipe.dit = m.to(device="cuda", dtype=torch.bfloat16).eval()
        if fp8:
            m.enable_fp8_linear()
        if lora is not None:
            pipe.load_lora(pipe.dit, state_dict=lora, alpha=1.0, hotload=True, hot_backend=backend)
        seen = {}

        class Keep:
            def store(self, x):
                seen["x"] = x.clone()
        f, h, w = self.fhw
        with torch.no_grad():
            m.forward_tokens(self.x0.cuda(), self.ctx.cuda(), self.t_mod.cuda(), seeded((1, self.dim), 14).cuda(), 0,
                             m.rope_tables(f, h, w, torch.device("cuda")), tea_cache=Keep())
        torch.cuda.synchronize()
        return seen["x"].cpu()

    def oracle(self, sd, dtype):
        f, h, w = self.fhw
        return odit.dit_block(sd, "blocks.0", self.x0.to(dtype), self.ctx.to(dtype), self.t_mod.to(dtype),
                              odit.rope_table_3d(self.dim // self.nh, f, h, w), self.nh, self.eps)


@functools.lru_cache(maxsize=None)
def _full_block():
    return _FullBlock()


@functools.lru_cache(maxsize=None)
def _full_block_fp8_plain():
    return _full_block().run()


@pytest.mark.gpu
def test_full_width_block_fp8_zero_adapter_is_identity():
    """fg_gemm_fp8_bf16's residual stores (modes 2, 3) + the stand-alone dual norms reproduce fg_residual_ln_fp8_bf16, and a zero
    adapter leaves every output unchanged: bit-equal to the adapter-free fp8 block."""
    fb = _full_block()
    x_zero = fb.run(_zero_b(fb.lora), "hip")
    assert torch.equal(x_zero, _full_block_fp8_plain())


@pytest.mark.gpu
def test_full_width_block_fp8_hot_backend_hip(monkeypatch):
    """Rank 32 on all ten Linears of the full-width block in the fp8 mode: the launches really taken with hot_backend="hip" (six
    fg_lora_apply_bf16 calls; seven fg_gemm_fp8_bf16 calls — qkv, o, cross q, cross k|v, cross o, ffn.0, ffn.2 — three of them with the
    residual store; four quantisation passes — context, a, ac, f — none with an activation, none on a norm output), today's with
    "torch", and the residual stream after the block against the oracle (2x criterion)."""
    fb = _full_block()
    counts = _Counts(monkeypatch)
    x_torch = fb.run(fb.lora, "torch")
    assert counts.lora == [] and counts.gemm8.count(True) == 0 and len(counts.gemm8) == 7
    counts.reset()
    x_hip = fb.run(fb.lora, "hip")
    assert len(counts.lora) == 6 and counts.lora.count("gelu_tanh") == 1 and counts.lora.count("gate") == 2, counts.lora
    assert len(counts.gemm8) == 7 and counts.gemm8.count(True) == 3, counts.gemm8
    assert len(counts.quant) == 4 and all(act is None for _, act in counts.quant), counts.quant
    assert counts.norm_rows and not {t.data_ptr() for t, _ in counts.quant} & {t.data_ptr() for t in counts.norm_rows}, \
        "a norm output went through fg_fp8_quant_rows_bf16"
    _with_lora_forward(monkeypatch, _oracle_adapters([(fb.lora, 1.0)]))
    want = fb.oracle(odit.Fp8Blocks({k: v.float() for k, v in fb.sd.items()}), torch.float32)
    err_h, err_t = (x_hip.float() - want).abs().max().item(), (x_torch.float() - want).abs().max().item()
    print(f"full-width block fp8: max|hip-f32|={err_h:.4f} max|torch-f32|={err_t:.4f} max|f32|={want.abs().max().item():.2f}")
    assert err_h <= 2 * err_t + 1e-2


@pytest.mark.gpu
def test_full_width_block_fp8_vs_oracle():
    """The fp8 Linear mode without adapters at model width, checked like test_fp8_linear_mode_vs_oracle checks the tiny model: against
    the oracle's bf16 block on Fp8Blocks weights, relative to that oracle's distance from its own bf16 block."""
    fb = _full_block()
    got = _full_block_fp8_plain()
    want, want_bf16 = fb.oracle(odit.Fp8Blocks(fb.sd), torch.bfloat16), fb.oracle(fb.sd, torch.bfloat16)
    err, drift = (got.float() - want.float()).abs().max().item(), (want.float() - want_bf16.float()).abs().max().item()
    print(f"full-width block fp8, no adapter: err={err:.4f} drift={drift:.4f} cos={_cos(got, want):.6f} max|want|={want.float().abs().max().item():.2f}")
    assert not torch.equal(got, fb.run(fp8=False))
    assert _cos(got, want) > 0.999 and err < 0.5 * drift + 0.05, (err, drift)

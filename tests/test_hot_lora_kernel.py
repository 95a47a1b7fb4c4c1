"""Hot-loaded LoRA adapters on fg_lora_apply_bf16 (`hot_backend="hip"`): the kernel against the oracle's lora_forward arithmetic, its
argument checks, the DiT forward with the backend switched on (tiny model and one full-width block), and the shot scheduler's
adapter switching.

Criterion of the numeric checks, the project's own: max|hip - f32| <= 2 * max|bf16 - f32| + 1e-2, where bf16 is the reference's
arithmetic in bf16 (oracle.pipeline.hot_lora_linear / the "torch" backend) and f32 the same formula in fp32."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import seeded
from fairygen_amd import hip, synthetic
from oracle import pipeline as opipe
from oracle import wan_dit as odit


def _adapters(k, n, ranks, seed, scale_b=1.0):
    """[(alpha * A (r, k), B (n, r)), ...] with x @ A^T @ B^T of O(1) for x ~ N(0, 1)."""
    return [(seeded((r, k), seed + 2 * i, scale=k ** -0.5) * (1.0 + i), seeded((n, r), seed + 2 * i + 1, scale=scale_b * r ** -0.5))
            for i, r in enumerate(ranks)]


def _epilogue(mode, lin, resid, gate):
    """What the reference makes of the Linear's (adapter-carrying) output at the site the mode stands for."""
    if mode == "gate":
        return resid + gate * lin
    if mode == "gelu_tanh":
        return F.gelu(lin, approximate="tanh")
    return lin


def _run_case(m, k, n, ranks, mode, groups=1, gate_rows=1, first_rows=0, zero_b=False, seed=100):
    from fairygen_amd.wan_video_dit import stack_hot_loras
    ng = n // groups
    x = seeded((m, k), seed)
    w, bias = seeded((n, k), seed + 1, scale=k ** -0.5), seeded((n,), seed + 2, scale=0.1)
    per_group = [_adapters(k, ng, ranks, seed + 10 + 20 * g, scale_b=0.0 if zero_b else 1.0) for g in range(groups)]
    resid = seeded((m, n), seed + 3)
    table = seeded((gate_rows, 6, n), seed + 4)
    gate_full = table[0, 2].expand(m, n) if gate_rows == 1 else torch.where(torch.arange(m).unsqueeze(1) < first_rows, table[0, 2], table[1, 2])
    if mode == "write":
        w, bias = torch.zeros_like(w), torch.zeros_like(bias)

    def reference(dt):
        cols = [opipe.hot_lora_linear(x.to(dt), w[g * ng:(g + 1) * ng].to(dt), bias[g * ng:(g + 1) * ng].to(dt), [(a.to(dt), b.to(dt)) for a, b in per_group[g]])
                for g in range(groups)]
        return _epilogue(mode, torch.cat(cols, dim=1), resid.to(dt), gate_full.to(dt))
    ref16, ref32 = reference(torch.bfloat16), reference(torch.float32)
    # the kernel's input `out`: what the GEMM's fused store leaves at that site (the bf16 Linear output, or residual + gate * it)
    lin16 = F.linear(x, w, bias)
    out0 = resid + gate_full * lin16 if mode == "gate" else lin16
    # strided buffers with guard values: 8 columns left and right of x and out, 3 rows below
    guard = 7.0
    xbuf = torch.full((m + 3, k + 16), guard, dtype=torch.bfloat16)
    obuf = torch.full((m + 3, n + 16), guard, dtype=torch.bfloat16)
    xbuf[:m, 8:8 + k], obuf[:m, 8:8 + n] = x, (torch.full_like(out0, guard) if mode == "write" else out0)
    xbuf, obuf = xbuf.cuda(), obuf.cuda()
    a_st, b_st = stack_hot_loras(per_group, [(k, ng)] * groups, torch.device("cuda"), torch.bfloat16)
    assert a_st.shape[0] % (32 * groups) == 0 and a_st.shape[0] // groups >= sum(ranks)
    mod = hip.ModTable(table.cuda().contiguous(), first_rows) if mode == "gate" else None
    before = obuf.clone()
    hip.lora_apply(xbuf[:m, 8:8 + k], a_st, b_st, obuf[:m, 8:8 + n], groups=groups, mode=mode, mod=mod, gate_idx=2)
    torch.cuda.synchronize()
    got = obuf[:m, 8:8 + n].cpu()
    assert torch.equal(obuf[m:], before[m:]) and torch.equal(obuf[:, :8], before[:, :8]) and torch.equal(obuf[:, 8 + n:], before[:, 8 + n:]), "guards"
    if zero_b and mode in ("add", "gate"):
        assert torch.equal(got, out0), "a zero adapter must leave out unchanged"
    err_hip = (got.float() - ref32).abs().max().item()
    err_16 = (ref16.float() - ref32).abs().max().item()
    print(f"lora_apply m={m} k={k} n={n} ranks={ranks} groups={groups} mode={mode}: max|hip-f32|={err_hip:.4f} max|bf16-f32|={err_16:.4f} "
          f"max|f32|={ref32.abs().max().item():.2f}")
    assert err_hip <= 2 * err_16 + 1e-2
    return got


KERNEL_CASES = [
    # m, k, n, ranks, mode, groups, gate_rows, first_rows
    (333, 3072, 3072, (32,), "write", 1, 1, 0),
    (333, 3072, 3072, (32,), "add", 1, 1, 0),
    (333, 3072, 3072, (32,), "gate", 1, 1, 0),
    (333, 3072, 3072, (32,), "gate", 1, 2, 77),            # first_rows inside the second row tile
    (333, 3072, 3072, (32,), "gelu_tanh", 1, 1, 0),
    (5070, 3072, 9216, (32,), "add", 3, 1, 0),             # q | k | v in one pass over x
    (200, 3072, 9216, (64,), "add", 3, 1, 0),              # one pass per group
    (130, 3072, 3072, (64,), "add", 1, 1, 0),
    (130, 3072, 3072, (128,), "gate", 1, 2, 64),
    (130, 3072, 3072, (96,), "write", 1, 1, 0),
    (130, 3072, 3072, (4, 8), "add", 1, 1, 0),             # two stacked adapters, zero-padded to 32
    (1, 3072, 3072, (32,), "add", 1, 1, 0),
    (5070, 14336, 3072, (32,), "gate", 1, 2, 1690),        # ffn.2
    (5070, 3072, 14336, (32,), "gelu_tanh", 1, 1, 0),      # ffn.0
]


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n,ranks,mode,groups,gate_rows,first_rows", KERNEL_CASES)
def test_lora_apply_vs_oracle(m, k, n, ranks, mode, groups, gate_rows, first_rows):
    _run_case(m, k, n, ranks, mode, groups, gate_rows, first_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,gate_rows", [("add", 1), ("gate", 1), ("gate", 2)])
def test_lora_apply_zero_adapter_is_identity(mode, gate_rows):
    _run_case(200, 3072, 3072, (32,), mode, 1, gate_rows, 50, zero_b=True)


def test_lora_apply_argument_checks():
    """fg_lora_apply_bf16 checks its arguments on the host; nothing is launched."""
    lib = hip.load()
    p16 = ctypes.c_void_p(16)

    def call(x=p16, m=512, k=256, ng=256, r=32, g=1, mode=1, gate=None, rows=1):
        return lib.fg_lora_apply_bf16(x, k, p16, p16, p16, g * ng, m, k, ng, r, g, mode, gate, rows, g * ng, 0, None)
    assert call(x=ctypes.c_void_p(8)) == -1 and b"16-byte aligned" in lib.fg_last_error()
    assert call(x=None) == -1 and b"null pointer" in lib.fg_last_error()
    assert call(r=48) == -1 and b"rank" in lib.fg_last_error()
    assert call(r=160) == -1 and b"rank" in lib.fg_last_error()
    assert call(k=288) == -1 and b"K % 64" in lib.fg_last_error()
    assert call(ng=96) == -1 and b"Ng % 64" in lib.fg_last_error()
    assert call(mode=3) == -1 and b"mode must be" in lib.fg_last_error()
    assert call(mode=2) == -1 and b"gate table" in lib.fg_last_error()
    assert call(g=5) == -1 and b"groups" in lib.fg_last_error()
    q = seeded((8, 256), 1)
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        hip.lora_apply(q, q, q, q)


# ------------------------------------------------------------------------------------------- model level
def _cos(a, b):
    return F.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0).item()


def _tiny_pipe(sd, cfg):
    from fairygen_amd.wan_video import WanVideoPipeline
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
    pipe.dit = m.to(device="cuda", dtype=torch.bfloat16).eval()
    return pipe


@pytest.mark.gpu
def test_tiny_dit_hot_backend_hip(monkeypatch):
    """The configuration of test_lora_hotload_and_clear with hot_backend="hip": against the fused weights (that test's bounds), against
    the "torch" backend (2x criterion, the oracle's fp32 forward of the fp32-fused weights as yardstick), with two stacked adapters
    of different alpha, after clear_lora(), and the default backend against itself.  The tiny widths stay below the own GEMM's
    64-tile threshold, so here the adapters run on fg_lora_apply_bf16 behind library GEMMs (counted); the own GEMM next to the
    kernel is the full-width test's."""
    from fairygen_amd.wan_video import model_fn_wan_video
    cfg = synthetic.TINY_DIT_KWARGS
    shapes = synthetic.dit_shapes(cfg)
    sd = synthetic.random_state_dict(shapes, seed=1234)
    lora1, lora2 = synthetic.random_lora(shapes, rank=4, seed=4321), synthetic.random_lora(shapes, rank=8, seed=99)
    lat, ctx, ts = seeded((1, 48, 3, 8, 8), 1), seeded((1, 16, 128), 2), torch.tensor([995.9]).to(torch.bfloat16)
    ctx[:, 10:] = 0

    def fwd(pipe):
        with torch.no_grad():
            return model_fn_wan_video(pipe.dit, latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)

    def ref32(loras):
        sd32 = {k: v.float() for k, v in sd.items()}
        for lo, alpha in loras:
            opipe.fuse_lora(sd32, {k: v.float() for k, v in lo.items()}, alpha=alpha)
        return odit.model_fn(sd32, cfg, lat.float(), ts.float(), ctx.float(), fuse_vae_embedding_in_latents=True)

    calls = []
    real = hip.lora_apply
    monkeypatch.setattr(hip, "lora_apply", lambda *a, **k: (calls.append(k.get("mode")), real(*a, **k))[1])
    out_base = fwd(_tiny_pipe(sd, cfg))
    for loras in ([(lora1, 2.0)], [(lora1, 2.0), (lora2, 0.5)]):
        fused, hot_t, hot_h, hot_d = (_tiny_pipe(sd, cfg) for _ in range(4))
        for lo, alpha in loras:
            fused.load_lora(fused.dit, state_dict=lo, alpha=alpha)
            hot_d.load_lora(hot_d.dit, state_dict=lo, alpha=alpha, hotload=True)
            hot_t.load_lora(hot_t.dit, state_dict=lo, alpha=alpha, hotload=True, hot_backend="torch")
            hot_h.load_lora(hot_h.dit, state_dict=lo, alpha=alpha, hotload=True, hot_backend="hip")
        assert hot_d.dit.hot_lora_backend == "torch" and hot_h.dit.hot_lora_backend == "hip"
        del calls[:]
        out_fused, out_d, out_t = fwd(fused), fwd(hot_d), fwd(hot_t)
        assert calls == [] and torch.equal(out_d, out_t)
        out_h = fwd(hot_h)
        assert len(calls) == 6 * cfg["num_layers"] and calls.count("gelu_tanh") == cfg["num_layers"]      # qkv, o, cross q, cross o, ffn.0, ffn.2
        assert not torch.equal(out_h, out_base)
        assert _cos(out_h, out_fused) > 0.9995 and (out_h.float() - out_fused.float()).abs().max().item() < 0.1
        want = ref32(loras)
        err_h = (out_h.float().cpu() - want).abs().max().item()
        err_t = (out_t.float().cpu() - want).abs().max().item()
        print(f"tiny DiT, {len(loras)} adapter(s): max|hip-f32|={err_h:.4f} max|torch-f32|={err_t:.4f} max|f32|={want.abs().max().item():.2f}")
        assert err_h <= 2 * err_t + 1e-2
        hot_h.clear_lora()
        assert hot_h.dit.hot_loras == {} and hot_h.dit.hot_lora_backend == "hip" and torch.equal(fwd(hot_h), out_base)
    with pytest.raises(ValueError, match="hot_backend"):
        hot_h.load_lora(hot_h.dit, state_dict=lora1, hotload=True, hot_backend="triton")


@pytest.mark.gpu
def test_full_width_block_hot_backend_hip(monkeypatch):
    """One block at the model's width (5 070 tokens, dim 3 072, ffn 14 336), rank 32 on its ten Linears: the residual stream after the
    block with hot_backend="hip" against "torch" (2x criterion; yardstick: the oracle's dit_block in fp32 on the fp32-fused weights),
    and the launches really taken: six fg_lora_apply_bf16 calls next to six own GEMMs, none of them on the library."""
    from fairygen_amd import wan_video_dit as wd
    from fairygen_amd.loader import TI2V_5B_DIT_KWARGS
    from fairygen_amd.wan_video import WanVideoPipeline
    cfg = dict(TI2V_5B_DIT_KWARGS, num_layers=1)
    dim, nh, eps = cfg["dim"], cfg["num_heads"], cfg["eps"]
    shapes = {k: v for k, v in synthetic.dit_shapes(cfg).items() if k.startswith("blocks.0.")}
    sd = synthetic.random_state_dict(shapes, seed=7)
    lora = synthetic.random_lora(shapes, rank=32, seed=8)
    f, h, w = 3, 26, 65
    n = f * h * w
    x0, ctx, t_mod = seeded((1, n, dim), 11), seeded((1, 512, dim), 12), seeded((1, 6, dim), 13, scale=0.5)

    def run(backend):
        with torch.device("meta"):
            m = wd.WanModel(**cfg)
        full = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1, device="cuda")
        full.update({k: v.cuda() for k, v in sd.items()})
        m.load_state_dict(full, assign=True)
        pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
        pipe.dit = m.to(device="cuda", dtype=torch.bfloat16).eval()
        pipe.load_lora(pipe.dit, state_dict=lora, alpha=1.0, hotload=True, hot_backend=backend)
        seen = {}

        class Keep:
            def store(self, x):
                seen["x"] = x.clone()
        with torch.no_grad():
            m.forward_tokens(x0.cuda(), ctx.cuda(), t_mod.cuda(), seeded((1, dim), 14).cuda(), 0, m.rope_tables(f, h, w, torch.device("cuda")),
                             tea_cache=Keep())
        torch.cuda.synchronize()
        return seen["x"].float().cpu()

    counts = {"lora_apply": 0, "gemm_bias_own": 0, "gemm_bias_gelu_own": 0, "gemm_residual": 0, "gemm_bias": 0}

    def counted(mod, name):
        real = getattr(mod, name)

        def fn(*a, **k):
            counts[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(mod, name, fn)
    counted(hip, "lora_apply")
    for name in ("gemm_bias_own", "gemm_bias_gelu_own", "gemm_residual", "gemm_bias"):
        counted(wd, name)
    x_torch = run("torch")
    assert counts["lora_apply"] == 0 and counts["gemm_residual"] == 0
    counts.update({k: 0 for k in counts})
    x_hip = run("hip")
    # own GEMMs: qkv, cross q, ffn.0 (plain store) and o, cross o, ffn.2 (residual store); the library keeps cross k | v (512 context rows)
    assert counts == {"lora_apply": 6, "gemm_bias_own": 3, "gemm_bias_gelu_own": 0, "gemm_residual": 3, "gemm_bias": 1}, counts
    sd32 = {k: v.float() for k, v in sd.items()}
    opipe.fuse_lora(sd32, {k: v.float() for k, v in lora.items()}, alpha=1.0)
    want = odit.dit_block(sd32, "blocks.0", x0.float(), ctx.float(), t_mod.float(), odit.rope_table_3d(dim // nh, f, h, w), nh, eps)
    err_h, err_t = (x_hip - want).abs().max().item(), (x_torch - want).abs().max().item()
    print(f"full-width block: max|hip-f32|={err_h:.4f} max|torch-f32|={err_t:.4f} max|f32|={want.abs().max().item():.2f}")
    assert err_h <= 2 * err_t + 1e-2


# ------------------------------------------------------------------------------------------- scheduler (no GPU)
def test_run_folder_switches_adapters_between_shots(tmp_path, monkeypatch):
    from PIL import Image
    from fairygen_amd import data
    from fairygen_amd.batch import ShotScheduler
    src = tmp_path / "in"
    src.mkdir()
    for name in ("s1_a", "s2_a", "s3_b", "s4_none"):
        Image.new("RGB", (8, 8)).save(src / f"{name}.png")
        (src / f"{name}.txt").write_text("a prompt")
    log = []

    class Pipe:
        dit = object()

        def __call__(self, **kw):
            log.append("run")
            return None

        def clear_lora(self):
            log.append("clear")

        def load_lora(self, module, path, **kw):
            assert module is self.dit and kw == {"hotload": True, "hot_backend": "hip"}
            log.append(f"load {path}")
    monkeypatch.setattr(data, "save_video", lambda video, path, **kw: path)
    paths = {"a": "/adapters/a.safetensors", "b": "/adapters/b.safetensors"}
    done = ShotScheduler(replica_size=1).run_folder(Pipe(), str(src), str(tmp_path / "out"), size=(8, 8),
                                                    lora_for_shot=lambda name: paths.get(name.split("_")[1]))
    assert [d[0] for d in done] == ["s1_a", "s2_a", "s3_b", "s4_none"]
    assert log == ["load /adapters/a.safetensors", "run", "run", "clear", "load /adapters/b.safetensors", "run", "clear", "run"]
    del log[:]
    ShotScheduler(replica_size=1).run_folder(Pipe(), str(src), str(tmp_path / "out"), size=(8, 8))
    assert log == ["run"] * 4

"""`hot_backend="fused"`: hot-loaded adapters folded into the weights (fg_lora_fuse_bf16, or torch ops on the device), the originals kept so `clear_lora()` puts
them back.  The weights against a permanent fuse (`hotload=False`, the reference's arithmetic on library GEMMs), the forward against the
oracle, the restore in bf16 and in the fp8 Linear mode (where a stale e4m3 or QKV copy would show), one full-width block against a model
that got the same weights through load_state_dict, the mixing rules, and the host logic that needs no GPU."""
import pytest
import torch

from conftest import seeded
from fairygen_amd import hip, synthetic
from oracle import pipeline as opipe
from oracle import wan_dit as odit

CFG = synthetic.TINY_DIT_KWARGS
# two adapters of different rank and alpha, stacked in this order
ADAPTERS = ((dict(rank=4, seed=4321), 2.0), (dict(rank=8, seed=99), 0.5))


def _ulp_distance(x, y):
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(x) - line(y)).abs()


def _tiny():
    shapes = synthetic.dit_shapes(CFG)
    sd = synthetic.random_state_dict(shapes, seed=1234)
    loras = [(synthetic.random_lora(shapes, **kw), alpha) for kw, alpha in ADAPTERS]
    return sd, loras


def _pipe(sd, cfg=CFG, device="cuda"):
    from fairygen_amd.wan_video import WanVideoPipeline
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    pipe = WanVideoPipeline(device=device, torch_dtype=torch.bfloat16)
    pipe.dit = m.to(device=device, dtype=torch.bfloat16).eval()
    return pipe


def _fwd(pipe):
    from fairygen_amd.wan_video import model_fn_wan_video
    lat, ctx, ts = seeded((1, 48, 3, 8, 8), 1), seeded((1, 16, 128), 2), torch.tensor([995.9]).to(torch.bfloat16)
    ctx[:, 10:] = 0
    with torch.no_grad():
        return model_fn_wan_video(pipe.dit, latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)


def _adapted(sd):
    return sorted(k for k in sd if k.startswith("blocks.") and k.endswith(".weight") and sd[k].dim() == 2)


# ------------------------------------------------------------------------------------------- GPU: tiny DiT
# Share of weight elements that must be identical to the permanent fuse's.  The yardstick is the reference's own arithmetic under another
# summation order — fp32 accumulation over the rank in reversed order, test_share_of_identical_weights_under_another_summation_order
# below — which leaves every element of these inputs identical, so the issue's 99 % stands.
IDENTICAL_SHARE = 0.99


def test_share_of_identical_weights_under_another_summation_order():
    """CPU check behind IDENTICAL_SHARE: fuse the two adapters with the reference's code, and again with the product accumulated in fp32 in
    reversed order over the rank; the share of identical elements and the largest distance must be within what the GPU test asks."""
    from fairygen_amd.lora import GeneralLoRALoader
    from fairygen_amd.wan_video_dit import WanModel
    sd, loras = _tiny()
    m = WanModel(**CFG)
    m.load_state_dict(sd)
    m = m.to(torch.bfloat16)
    loader = GeneralLoRALoader(device="cpu", torch_dtype=torch.bfloat16)
    other = {k: sd[k].clone() for k in _adapted(sd)}
    for lora, alpha in loras:
        loader.fuse_lora_to_base_model(m, lora, alpha=alpha)
        conv = loader.convert_state_dict(lora)
        for k in other:
            a, b = conv[k[:-len(".weight")] + ".lora_A.weight"].float(), conv[k[:-len(".weight")] + ".lora_B.weight"].float()
            acc = torch.zeros(other[k].shape)
            for r in reversed(range(a.shape[0])):
                acc = acc + b[:, r:r + 1] * a[r:r + 1]
            other[k] = other[k] + alpha * acc.to(torch.bfloat16)
    ref = m.state_dict()
    same = sum((other[k] == ref[k]).sum().item() for k in other) / sum(v.numel() for v in other.values())
    worst = max(_ulp_distance(other[k], ref[k]).max().item() for k in other)
    print(f"reversed-order fp32 accumulation: {same:.6f} of the elements identical, max {worst} ulp")
    assert same >= IDENTICAL_SHARE and worst <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["kernel", "torch_ops"])
def test_two_stacked_adapters_match_permanent_fuse(path, monkeypatch):
    """Weights: within 1 bf16 ulp of a model fused twice with hotload=False, >= 99 % identical, on fg_lora_fuse_bf16 (the default)
    and on the torch ops (FAIRYGEN_LORA_FUSE=torch; the permanent fuse's own ops: bit-equal).  Forward: the 2x criterion of test_hot_lora_kernel.py against the oracle's
    fp32 evaluation on the fp32-fused weights."""
    from fairygen_amd import wan_video_dit as wd
    sd, loras = _tiny()
    monkeypatch.setattr(wd, "LORA_FUSE", "hip" if path == "kernel" else "torch")
    calls = []
    real = hip.lora_fuse
    monkeypatch.setattr(hip, "lora_fuse", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    perm, hot = _pipe(sd), _pipe(sd)
    for lora, alpha in loras:
        perm.load_lora(perm.dit, state_dict=lora, alpha=alpha)
        hot.load_lora(hot.dit, state_dict=lora, alpha=alpha, hotload=True, hot_backend="fused")
    names = _adapted(sd)
    assert len(calls) == (2 * len(names) if path == "kernel" else 0)
    assert hot.dit.hot_loras == {} and sorted(hot.dit._fused_stash) == [k[:-len(".weight")] for k in names]
    wp, wh = perm.dit.state_dict(), hot.dit.state_dict()
    same = sum((wp[k] == wh[k]).sum().item() for k in names) / sum(wp[k].numel() for k in names)
    worst = max(_ulp_distance(wp[k], wh[k]).max().item() for k in names)
    print(f"{path}: {same:.6f} of the adapted weight elements identical to the permanent fuse, max {worst} ulp")
    assert all(not torch.equal(wh[k].cpu(), sd[k]) for k in names)
    assert worst <= 1 and same >= (1.0 if path == "torch_ops" else IDENTICAL_SHARE)
    assert all(torch.equal(wp[k], wh[k]) for k in wp if k not in names)
    sd32 = {k: v.float() for k, v in sd.items()}
    for lora, alpha in loras:
        opipe.fuse_lora(sd32, {k: v.float() for k, v in lora.items()}, alpha=alpha)
    lat, ctx, ts = seeded((1, 48, 3, 8, 8), 1), seeded((1, 16, 128), 2), torch.tensor([995.9]).to(torch.bfloat16)
    ctx[:, 10:] = 0
    want = odit.model_fn(sd32, CFG, lat.float(), ts.float(), ctx.float(), fuse_vae_embedding_in_latents=True)
    err_h, err_p = (_fwd(hot).float().cpu() - want).abs().max().item(), (_fwd(perm).float().cpu() - want).abs().max().item()
    print(f"tiny DiT, 2 adapters: max|fused hot-f32|={err_h:.4f} max|permanent-f32|={err_p:.4f} max|f32|={want.abs().max().item():.2f}")
    assert err_h <= 2 * err_p + 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", ["hip", "torch"])
@pytest.mark.parametrize("fp8", [False, True])
def test_clear_lora_restores_weights_and_forward(fp8, fuse, monkeypatch):
    """After clear_lora() every parameter is bit-equal to its value before the first adapter and so is the forward — also in the fp8 mode,
    where the forward reads the e4m3 and the fused QKV copies: both exist before the adapters arrive, so a stale one would show, with the
    adapters in place (against a model given the same weights by load_state_dict) and after the restore."""
    from fairygen_amd import wan_video_dit as wd
    monkeypatch.setattr(wd, "LORA_FUSE", fuse)
    sd, loras = _tiny()
    pipe = _pipe(sd)
    if fp8:
        pipe.dit.enable_fp8_linear()
    snap = {k: v.clone() for k, v in pipe.dit.state_dict().items()}
    out_base = _fwd(pipe)
    assert pipe.dit.blocks[0]._fused is not None and (pipe.dit.blocks[0]._fp8 is not None) == fp8
    for lora, alpha in loras:
        pipe.load_lora(pipe.dit, state_dict=lora, alpha=alpha, hotload=True, hot_backend="fused")
    out_hot = _fwd(pipe)
    assert not torch.equal(out_hot, out_base)
    twin = _pipe({k: v.cpu() for k, v in pipe.dit.state_dict().items()})
    if fp8:
        twin.dit.enable_fp8_linear()
    assert torch.equal(_fwd(twin), out_hot), "a derived copy (fused QKV / e4m3) is out of step with the rewritten weights"
    pipe.clear_lora()
    assert pipe.dit._fused_stash == {} and pipe.dit.hot_lora_backend == "fused"
    now = pipe.dit.state_dict()
    assert all(torch.equal(now[k], snap[k]) for k in snap)
    assert torch.equal(_fwd(pipe), out_base)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", ["hip", "torch"])
@pytest.mark.parametrize("fp8", [False, True])
def test_full_width_block_gemms_get_current_weights(fp8, fuse, monkeypatch):
    """One block at the model's width (dim 3 072, ffn 14 336, 256 tokens), rank 32 on its ten Linears, adapters attached after a first
    forward has built the derived copies.  Every GEMM of the forward, own or library, bf16 or e4m3, is handed the same weight values as in
    a model that got the rewritten weights through load_state_dict, and the two forwards are bit-equal."""
    from fairygen_amd import wan_video_dit as wd
    from fairygen_amd.loader import TI2V_5B_DIT_KWARGS
    from fairygen_amd.wan_video import WanVideoPipeline
    monkeypatch.setattr(wd, "LORA_FUSE", fuse)
    cfg = dict(TI2V_5B_DIT_KWARGS, num_layers=1)
    dim = cfg["dim"]
    shapes = synthetic.dit_shapes(cfg)
    lora = synthetic.random_lora({k: v for k, v in shapes.items() if k.startswith("blocks.0.")}, rank=32, seed=8)
    f, h, w = 1, 16, 16
    x0, ctx, t_mod, t_row = seeded((1, f * h * w, dim), 11), seeded((1, 512, dim), 12), seeded((1, 6, dim), 13, scale=0.5), seeded((1, dim), 14)
    seen = []

    def recorded(mod, name, at):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, **k: (seen.append(a[at]), real(*a, **k))[1])
    for name in ("gemm_bias", "gemm_bias_gelu", "gemm_bias_tuned", "gemm_bias_own", "gemm_bias_gelu_own"):
        recorded(wd, name, 1)
    recorded(wd, "gemm_residual", 2)
    recorded(hip, "gemm_fp8", 2)

    def model(sd):
        with torch.device("meta"):
            m = wd.WanModel(**cfg)
        m.load_state_dict(sd, assign=True)
        pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
        pipe.dit = m.to(device="cuda", dtype=torch.bfloat16).eval()
        if fp8:
            pipe.dit.enable_fp8_linear()
        return pipe

    def run(pipe):
        del seen[:]
        kept = {}

        class Keep:
            def store(self, x):
                kept["x"] = x.clone()
        with torch.no_grad():
            pipe.dit.forward_tokens(x0.cuda(), ctx.cuda(), t_mod.cuda(), t_row.cuda(), 0, pipe.dit.rope_tables(f, h, w, torch.device("cuda")),
                                    tea_cache=Keep())
        torch.cuda.synchronize()
        return kept["x"], list(seen)

    hot = model(synthetic.random_state_dict(shapes, seed=1, device="cuda"))
    x_base, _ = run(hot)
    hot.load_lora(hot.dit, state_dict=lora, alpha=1.0, hotload=True, hot_backend="fused")
    assert len(hot.dit._fused_stash) == 10
    x_hot, w_hot = run(hot)
    twin = model({k: v.clone() for k, v in hot.dit.state_dict().items()})
    x_twin, w_twin = run(twin)
    assert len(w_hot) == len(w_twin) >= 7      # qkv, o, cross q, cross k | v, cross o, ffn.0, ffn.2
    for a, b in zip(w_hot, w_twin):
        assert a.shape == b.shape and a.dtype == b.dtype == (torch.float8_e4m3fn if fp8 else torch.bfloat16)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert not torch.equal(x_hot, x_base) and torch.equal(x_hot, x_twin)


@pytest.mark.gpu
def test_mixing_rules_and_load_state_dict():
    sd, loras = _tiny()
    (lora1, _), (lora2, _) = loras
    pipe = _pipe(sd)
    pipe.load_lora(pipe.dit, state_dict=lora1, hotload=True, hot_backend="hip")
    with pytest.raises(ValueError, match="clear_lora"):
        pipe.load_lora(pipe.dit, state_dict=lora2, hotload=True, hot_backend="fused")
    assert pipe.dit.hot_lora_backend == "hip" and pipe.dit._fused_stash == {}
    pipe.clear_lora()
    pipe.load_lora(pipe.dit, state_dict=lora1, hotload=True, hot_backend="fused")
    for backend in ("hip", "torch"):
        with pytest.raises(ValueError, match="clear_lora"):
            pipe.load_lora(pipe.dit, state_dict=lora2, hotload=True, hot_backend=backend)
    before = {k: v.clone() for k, v in pipe.dit.state_dict().items()}
    with pytest.raises(ValueError, match="clear_lora"):      # a permanent fuse with the stash alive
        pipe.load_lora(pipe.dit, state_dict=lora2)
    assert pipe.dit.hot_lora_backend == "fused" and pipe.dit.hot_loras == {} and len(pipe.dit._fused_stash) == len(_adapted(sd))
    assert all(torch.equal(v, before[k]) for k, v in pipe.dit.state_dict().items())
    # .to() takes the stash along; load_state_dict makes the new weights the originals: the stash goes and clear_lora() restores nothing
    pipe.dit.to("cuda")
    assert all(v.device.type == "cuda" for v in pipe.dit._fused_stash.values())
    pipe.dit.load_state_dict(before)
    assert pipe.dit._fused_stash == {}
    pipe.clear_lora()
    assert all(torch.equal(v, before[k]) for k, v in pipe.dit.state_dict().items())
    pipe.load_lora(pipe.dit, state_dict=lora2)      # and a permanent fuse is allowed again


# ------------------------------------------------------------------------------------------- host logic (no GPU)
def test_fused_backend_has_no_cpu_fallback():
    sd, loras = _tiny()
    pipe = _pipe(sd, device="cpu")
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        pipe.load_lora(pipe.dit, state_dict=loras[0][0], hotload=True, hot_backend="fused")
    assert pipe.dit._fused_stash == {} and all(torch.equal(v, sd[k]) for k, v in pipe.dit.state_dict().items())


def test_fused_backend_is_accepted_by_the_argument_check():
    sd, _ = _tiny()
    pipe = _pipe(sd, device="cpu")
    pipe.load_lora(pipe.dit, state_dict={}, hotload=True, hot_backend="fused")      # an adapter file without a target: nothing to rewrite
    assert pipe.dit.hot_lora_backend == "fused"
    with pytest.raises(ValueError, match="'torch', 'hip' or 'fused'"):
        pipe.load_lora(pipe.dit, state_dict={}, hotload=True, hot_backend="triton")


def test_run_folder_passes_hot_backend_through(tmp_path, monkeypatch):
    from PIL import Image
    from fairygen_amd import data
    from fairygen_amd.batch import ShotScheduler
    src = tmp_path / "in"
    src.mkdir()
    for name in ("s1_a", "s2_b"):
        Image.new("RGB", (8, 8)).save(src / f"{name}.png")
        (src / f"{name}.txt").write_text("a prompt")
    log = []

    class Pipe:
        dit = object()

        def __call__(self, **kw):
            log.append("run")

        def clear_lora(self):
            log.append("clear")

        def load_lora(self, module, path, **kw):
            assert module is self.dit
            log.append((path, kw))
    monkeypatch.setattr(data, "save_video", lambda video, path, **kw: path)
    for given, want in (({}, "hip"), ({"hot_backend": "fused"}, "fused")):
        del log[:]
        ShotScheduler(replica_size=1).run_folder(Pipe(), str(src), str(tmp_path / "out"), size=(8, 8), lora_for_shot=lambda n: n.split("_")[1], **given)
        kw = {"hotload": True, "hot_backend": want}
        assert log == [("a", kw), "run", "clear", ("b", kw), "run"]

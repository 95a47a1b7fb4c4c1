"""The denoise step as one captured graph (WanVideoPipeline.denoise(graph=True), wan_video.GraphedStep) and its kernel
fg_cfg_euler_dev_bf16 (ABI 8).

The property everywhere is "the same bits as the eager loop": a replayed step issues the launches of an eager step on the same values,
only its per-step inputs come from device tables (time-embedding rows, sigma' - sigma) indexed by a step counter on the device.  So the
comparisons are torch.equal, and the reference is the eager loop of the same pipeline, whose arithmetic the other modules pin
(test_hip_models.py, test_oracle_golden.py).

  1. the tiny DiT loop of test_hip_models.py::test_tiny_denoise_loop_vs_golden, graph against eager and against the golden latents;
  2. a two-block DiT of the production width (dim 3072, 24 heads, 1 440 tokens): every block Linear on the persistent GEMM with its
     k-split scratch, self-attention on the 4-wave kernel, cfg_prefix and kv_cache on; bf16 and the fp8 Linear mode;
  3. replay safety: two graph loops and an eager loop on one pipeline, and no per-(device, stream) state of hip left behind by a capture;
  4. fg_cfg_euler_dev_bf16 alone: against hip.cfg_euler + the torch re-pin for every step index, guard bands, capture and replay,
     argument checks;
  5. the combinations graph=True refuses;
  6. (no GPU) the ABI: version, header, and the signatures of ABI 7 in hip._SIGNATURES unchanged.
"""
import ctypes
import hashlib
import os
import re

import pytest
import torch

from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
NAME = "fg_cfg_euler_dev_bf16"
# the stream-taking entry points of ABI 7; SIGNATURES_SHA256 is the sha256 of their sorted "name:argtypes" lines
SIGNATURES_ABI7 = (
    "fg_ln_modulate_bf16", "fg_ln_affine_bf16", "fg_ln_modulate_fp8_bf16", "fg_residual_ln_fp8_bf16", "fg_ln_modulate_dual_bf16",
    "fg_ln_affine_dual_bf16", "fg_gate_residual_bf16", "fg_residual_ln_bf16", "fg_rmsnorm_rope_bf16", "fg_rmsnorm_rope_grouped_bf16",
    "fg_copy_groups_bf16", "fg_fp8_quant_rows_bf16", "fg_act_bf16", "fg_gemm_epilogue_bf16", "fg_gemm_fp8_bf16", "fg_gemm_sched_reset",
    "fg_gemm_epilogue_bf16_s", "fg_gemm_fp8_bf16_s", "fg_lora_apply_bf16", "fg_attn_fwd_bf16", "fg_cfg_euler_bf16", "fg_vae_rmsnorm_silu_bf16",
    "fg_conv_pack_weight_bf16", "fg_conv3d_cl_bf16", "fg_dupup3d_add_bf16", "fg_softmax_rows_f32_bf16", "fg_vae_latent_to_cl_bf16",
    "fg_vae_unpatchify_bf16", "fg_vae_tile_accumulate_bf16", "fg_vae_tile_finalize_bf16", "fg_vae_patchify_bf16", "fg_avgdown3d_add_bf16",
    "fg_vae_latent_from_cl_bf16", "fg_video_to_uint8", "fg_softmax_bias_bf16", "fg_gated_gelu_bf16")


def cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().flatten().cpu(), b.float().flatten().cpu(), dim=0).item()


@pytest.fixture(scope="module")
def hip():
    _hip.load()
    return _hip


def make_pipe(cfg, seed=1234):
    from fairygen_amd.wan_video import WanVideoPipeline
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**cfg)
    m.load_state_dict(synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=seed))
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.to(device="cuda", dtype=BF16).eval()
    return pipe


@pytest.fixture(scope="module")
def tiny_pipe():
    return make_pipe(synthetic.TINY_DIT_KWARGS)


WIDE_DIT_KWARGS = dict(synthetic.TINY_DIT_KWARGS, dim=3072, num_heads=24, num_layers=2, ffn_dim=3072, text_dim=256)
WIDE_LATENT = (1, 48, 5, 32, 36)      # 5 x 16 x 18 = 1 440 tokens


@pytest.fixture(scope="module")
def wide_pipe():
    return make_pipe(WIDE_DIT_KWARGS)


def loop(pipe, lat, ctx_p, ctx_n, z0, steps, cfg_scale=5.0, fuse=True, graph=False, **shared):
    """pipe.denoise on fresh device copies of the inputs, as WanVideoPipeline.__call__ prepares them."""
    pipe.scheduler.set_timesteps(steps, denoising_strength=1.0, shift=5.0)
    latents = lat.clone()
    inputs = {"latents": None, "fuse_vae_embedding_in_latents": fuse, **shared}
    if z0 is not None:
        latents[:, :, 0:1] = z0
        inputs["first_frame_latents"] = z0.cuda()
    inputs["latents"] = latents.cuda()
    with torch.no_grad():
        out = pipe.denoise(inputs, {"context": ctx_p.cuda()}, {"context": ctx_n.cuda()}, cfg_scale, progress_bar_cmd=lambda x: x, graph=graph)
    torch.cuda.synchronize()
    return out.clone()


def tiny_inputs():      # test_hip_models.py::_tiny_inputs
    ctx_p, ctx_n = seeded((1, 16, 128), 2), seeded((1, 16, 128), 3)
    ctx_p[:, 10:] = 0
    ctx_n[:, 12:] = 0
    return seeded((1, 48, 3, 8, 8), 1), ctx_p, ctx_n, seeded((1, 48, 1, 8, 8), 4)


def wide_inputs(seed):
    return (seeded(WIDE_LATENT, seed), seeded((1, 32, 256), seed + 1), seeded((1, 32, 256), seed + 2),
            seeded(WIDE_LATENT[:2] + (1,) + WIDE_LATENT[3:], seed + 3))


def hip_tables(hip):  # noqa: F811
    return {name: set(getattr(hip, name)) for name in ("_gemm_sched", "_gemm_workspace", "_attn_workspace")}


# ------------------------------------------------------------------------------------------------------------------ 1. the tiny loop
@gpu
@pytest.mark.parametrize("mode", ["ti2v-cfg5", "ti2v-cfg1", "t2v-time-repin", "t2v"])
def test_tiny_loop_bit_for_bit(tiny_pipe, golden, mode):
    lat, ctx_p, ctx_n, z0 = tiny_inputs()
    kw = {"ti2v-cfg5": {}, "ti2v-cfg1": {"cfg_scale": 1.0}, "t2v-time-repin": {"fuse": False}, "t2v": {"fuse": False, "z0": None}}[mode]
    z0 = kw.pop("z0", z0)
    want = loop(tiny_pipe, lat, ctx_p, ctx_n, z0, 4, **kw)
    got = loop(tiny_pipe, lat, ctx_p, ctx_n, z0, 4, graph=True, **kw)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want), f"{mode}: {(got != want).sum().item()} of {got.numel()} latents differ from the eager loop"
    if z0 is not None:
        assert torch.equal(got[:, :, 0:1].cpu(), z0)
    if mode == "ti2v-cfg5":
        assert cos(got, golden("dit_tiny.safetensors")["loop_step3"]) > 0.999


def test_call_takes_graph():
    """pipe(..., graph=True) hands the keyword to denoise; the default is the eager loop."""
    class Seen(Exception):
        pass

    def denoise(inputs_shared, inputs_posi, inputs_nega, cfg_scale, progress_bar_cmd, graph=False):
        raise Seen(graph)
    pipe = _refusal_pipe()
    pipe.denoise, pipe.units = denoise, []
    for kw, want in (({}, False), ({"graph": True}, True)):
        with pytest.raises(Seen) as e:
            pipe(prompt=None, num_inference_steps=2, **kw)
        assert e.value.args == (want,)


# ------------------------------------------------------------------------------------------------------------------ 2. the production mix
@gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_wide_loop_bit_for_bit(hip, wide_pipe, fp8, monkeypatch):  # noqa: F811
    """Every own GEMM, with its k-split pieces, and the 4-wave attention under capture: the launches are counted on the way."""
    from fairygen_amd import wan_video, wan_video_dit
    assert wan_video.CFG_SHARE_PREFIX and wan_video.CROSS_KV_CACHE
    n, dim = 1440, WIDE_DIT_KWARGS["dim"]
    assert wan_video_dit.own_gemm_ok(n, dim, dim) and n > 1024 and hip.gemm_workspace_need(n, dim, 2 * dim) > 0
    wide_pipe.dit.enable_fp8_linear(torch.float8_e4m3fn if fp8 else None)
    calls, real = [], hip._call

    def call(name, *args):
        calls.append((name, torch.cuda.is_current_stream_capturing(), args))
        return real(name, *args)
    try:
        ins = wide_inputs(700)
        want = loop(wide_pipe, *ins, 3)
        monkeypatch.setattr(hip, "_call", call)
        got = loop(wide_pipe, *ins, 3, graph=True)
    finally:
        wide_pipe.dit.enable_fp8_linear(None)
    assert torch.isfinite(got.float()).all() and torch.equal(got[:, :, 0:1].cpu(), ins[3])
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} latents differ from the eager loop"
    captured = [(name, args) for name, cap, args in calls if cap]
    gemm = "fg_gemm_fp8_bf16_s" if fp8 else "fg_gemm_epilogue_bf16_s"
    gemms = [args for name, args in captured if name == gemm]
    # per block and forward: qkv, o, cross q, cross o, ffn.0, ffn.2; block 0's first two once for both CFG forwards
    assert len(gemms) == 2 * 2 * 6 - 2, len(gemms)
    ws_at = 15 if fp8 else 14      # workspace, sched in the argument lists of hip.gemm_fp8 / hip.gemm_epilogue
    assert all(a[ws_at].value for a in gemms), "a captured GEMM ran without k-split scratch"
    assert len({a[ws_at].value for a in gemms}) == 1 and len({a[ws_at + 1].value for a in gemms}) == 1, "the captured GEMMs must share the step's own state"
    assert sum(name == "fg_attn_fwd_bf16" for name, _ in captured) == 2 * 2 * 2 - 1
    assert sum(name == NAME for name, _ in captured) == 1 and not any(name == "fg_cfg_euler_bf16" for name, _ in captured)
    assert not any(name == "fg_gemm_sched_reset" for name, _ in captured), "a scheduler reset was recorded into the graph"


# ------------------------------------------------------------------------------------------------------------------ 3. replay safety
@gpu
def test_graph_loops_leave_nothing_behind(hip, wide_pipe):  # noqa: F811
    a, b = wide_inputs(800), wide_inputs(900)
    want_a, want_b = loop(wide_pipe, *a, 3), loop(wide_pipe, *b, 3)
    assert not torch.equal(want_a, want_b)
    before = hip_tables(hip)
    got_a = loop(wide_pipe, *a, 3, graph=True)
    got_b = loop(wide_pipe, *b, 3, graph=True)
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    assert hip_tables(hip) == before, "a captured step left per-(device, stream) state in hip's tables"
    assert torch.equal(loop(wide_pipe, *a, 3), want_a), "the eager loop after the graph loops"
    assert torch.equal(loop(wide_pipe, *b, 3, graph=True), want_b)


# ------------------------------------------------------------------------------------------------------------------ 4. the kernel
SHAPES = {"tiny-latent": (1, 48, 3, 8, 8), "odd": (1, 5, 3, 3, 7)}      # 9 216 = 1 152 vectors; 315 = 39 vectors + 3, frames of 21: no vector is all frame 0
DSIGMA = [-0.0712890625, -0.1337, -0.25, 0.3]


def euler_operands(shape, seed):
    return [seeded(shape, seed + i) for i in range(3)] + [seeded(shape[:2] + (1,) + shape[3:], seed + 3)]


def euler_want(hip, lat, posi, nega, first, cfg, ds):  # noqa: F811
    want = hip.cfg_euler(lat, posi, nega, cfg, ds)
    if first is not None:
        want[:, :, 0:1] = first
    return want


@gpu
@pytest.mark.parametrize("with_first", [False, True], ids=["nofirst", "first"])
@pytest.mark.parametrize("with_nega", [False, True], ids=["nonega", "nega"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cfg_euler_dev_equals_scalar_form(hip, shape, with_nega, with_first):  # noqa: F811
    from test_buffer_contract import Guards
    lat, posi, nega, first = (t.cuda() for t in euler_operands(SHAPES[shape], 40))
    nega, first = nega if with_nega else None, first if with_first else None
    cfg = 5.0 if with_nega else 1.0
    table = torch.tensor(DSIGMA, dtype=torch.float32, device="cuda")
    for i, ds in enumerate(DSIGMA):
        want = euler_want(hip, lat, posi, nega, first, cfg, ds)
        step = torch.tensor([i], dtype=torch.int32, device="cuda")
        g = Guards()
        ops = [g.embed(t) if t is not None else None for t in (lat, posi, nega, first)]
        out = g.embed(torch.empty_like(lat))
        assert hip.cfg_euler_dev(ops[0], ops[1], ops[2], cfg, table, step, first=ops[3], out=out) is out
        g.check(f"cfg_euler_dev {shape} step {i}")
        assert torch.equal(out, want), f"step {i}: {(out != want).sum().item()} elements differ"
        assert torch.equal(hip.cfg_euler_dev(ops[0], ops[1], ops[2], cfg, table, step, first=ops[3], out=ops[0]), want), f"step {i}, out = latents"
        g.check(f"cfg_euler_dev {shape} step {i} in place")
        assert step.item() == i and torch.equal(table.cpu(), torch.tensor(DSIGMA, dtype=torch.float32)), "the kernel only reads step and the table"
    # element-aligned operands (2 bytes past a 16-byte boundary): the single-element path, same bits
    flat = [torch.empty(lat.numel() + 1, dtype=BF16, device="cuda")[1:] for _ in range(4)]
    for f, t in zip(flat, (lat, posi, nega if with_nega else posi)):
        f.copy_(t.reshape(-1))
    off = [f.view(lat.shape) for f in flat]
    got = hip.cfg_euler_dev(off[0], off[1], off[2] if with_nega else None, cfg, table, step, first=first, out=off[3])
    assert got.data_ptr() % 16 == 2 and torch.equal(got, want)


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cfg_euler_dev_capture_and_replay(hip, shape):  # noqa: F811
    """Captured once on a side stream with the loop's in-place form and a captured step.add_(1): each replay takes the next table entry."""
    lat, posi, nega, first = (t.cuda() for t in euler_operands(SHAPES[shape], 50))
    table = torch.tensor(DSIGMA, dtype=torch.float32, device="cuda")
    want, cur = [], lat
    for ds in DSIGMA:
        cur = euler_want(hip, cur, posi, nega, first, 5.0, ds)
        want.append(cur)
    static, step = lat.clone(), torch.zeros(1, dtype=torch.int32, device="cuda")
    names, real = [], hip._call
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, "_call", lambda name, *args: (names.append(name), real(name, *args))[1])
        with torch.cuda.graph(graph, stream=side):      # strict mode: an allocation by the runtime, a synchronisation or a blocking copy aborts it
            hip.cfg_euler_dev(static, posi, nega, 5.0, table, step, first=first, out=static)
            step.add_(1)
    torch.cuda.synchronize()
    assert names == [NAME] and torch.equal(static, lat) and step.item() == 0, "a capture records, it does not run"
    for i in range(len(DSIGMA)):
        graph.replay()
        torch.cuda.synchronize()
        assert step.item() == i + 1 and torch.equal(static, want[i]), f"replay {i}"
    del graph


def test_cfg_euler_dev_argument_checks():
    """FG_EINVAL with a message that names the function for every precondition the header states, before any launch (fake pointers without
    a device; with one, real buffers and the unbroken call first) — what test_buffer_contract.py::test_argument_checks does per entry point."""
    lib = _hip.load()
    have_dev = torch.cuda.is_available()
    keep = []

    def P():
        if not have_dev:
            keep.append(None)
            return 0x100000 * len(keep)
        keep.append(torch.zeros(1 << 16, dtype=torch.uint8, device="cuda"))
        return keep[-1].data_ptr()
    good = [P(), P(), P(), P(), 48 * 3 * 64, 5.0, P(), P(), P(), 64, 3 * 64, None]
    if have_dev:
        assert lib.fg_cfg_euler_dev_bf16(*good) == 0, lib.fg_last_error().decode()
        torch.cuda.synchronize()
    broken = {"null latents": {0: None}, "null posi": {1: None}, "null out": {3: None}, "n < 0": {4: -1}, "null dsigma_table": {6: None},
              "null step": {7: None}, "dsigma_table off by 2 bytes": {6: good[6] + 2}, "step off by 2 bytes": {7: good[7] + 2},
              "first_n == 0": {9: 0}, "first_n > frame_stride": {9: 3 * 64 + 1}, "n not a multiple of frame_stride": {4: 48 * 3 * 64 + 8}}
    for what, change in broken.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert lib.fg_cfg_euler_dev_bf16(*args) == -1, what
        assert NAME in lib.fg_last_error().decode(), what
    if have_dev:
        torch.cuda.synchronize()
        assert all(not t.any() for t in keep[3:4]), "a rejected call wrote to out"
    # the wrapper: wrong dtypes / shapes raise before the library is reached
    with pytest.raises(_hip.HipLibraryError):
        _hip.cfg_euler_dev(torch.zeros(8, dtype=BF16), torch.zeros(8, dtype=BF16), None, 1.0, torch.zeros(1), torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
class _Active:
    active, cfg_parallel, world = True, 1, None


def _refusal_pipe():
    """A pipeline on meta tensors: the refusals come before anything touches a device."""
    from fairygen_amd.wan_video import WanVideoPipeline
    from fairygen_amd.wan_video_dit import WanModel
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    with torch.device("meta"):
        pipe.dit = WanModel(**synthetic.TINY_DIT_KWARGS)
    pipe.scheduler.set_timesteps(2, shift=5.0)
    return pipe


def _refused(pipe, shared=None, posi=None, nega=None, match=""):
    lat = torch.zeros((1, 48, 3, 8, 8), dtype=BF16, device="meta")
    ctx = torch.zeros((1, 16, 128), dtype=BF16, device="meta")
    with pytest.raises(NotImplementedError, match=match) as e:
        pipe.denoise({"latents": lat, **(shared or {})}, {"context": ctx, **(posi or {})}, {"context": ctx, **(nega or {})}, 5.0,
                     progress_bar_cmd=lambda x: x, graph=True)
    assert "\n" not in str(e.value)


def test_graph_refuses_what_it_does_not_record():
    from fairygen_amd.wan_video import TeaCache, model_fn_wan_video
    tea = TeaCache(2, 0.05, "Wan2.1-T2V-1.3B")
    _refused(_refusal_pipe(), posi={"tea_cache": tea}, nega={"tea_cache": tea}, match="TeaCache")
    _refused(_refusal_pipe(), shared={"sliding_window_size": 2, "sliding_window_stride": 1}, match="sliding windows")
    _refused(_refusal_pipe(), shared={"cfg_merge": True}, match="cfg_merge")
    pipe = _refusal_pipe()
    pipe.sequence_shard = _Active()
    _refused(pipe, match="sequence_shard")
    pipe = _refusal_pipe()
    pipe.parallel = _Active()
    pipe.parallel.cfg_parallel = 2
    _refused(pipe, match="parallel")
    pipe = _refusal_pipe()
    pipe.dit.hot_loras = {"blocks.0.self_attn.q": [(None, None)]}
    assert pipe.dit.hot_lora_backend == "torch"
    _refused(pipe, match="'torch' backend")
    pipe = _refusal_pipe()
    pipe.model_fn = lambda *a, **k: model_fn_wan_video(*a, **k)
    _refused(pipe, match="model_fn")
    pipe = _refusal_pipe()
    pipe.dit.blocks[1].cross_attn.attn = torch.nn.Identity()
    _refused(pipe, match="AttentionModule")


@gpu
def test_graph_takes_hip_and_fused_adapters(tiny_pipe):
    """The adapter backends graph=True supports, on the tiny DiT: 'hip' (fg_lora_apply_bf16 under capture) and 'fused' (plain weights)."""
    lat, ctx_p, ctx_n, z0 = tiny_inputs()
    lora = synthetic.random_lora(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), rank=32)
    base = loop(tiny_pipe, lat, ctx_p, ctx_n, z0, 3)
    try:
        for backend in ("hip", "fused"):
            tiny_pipe.load_lora(tiny_pipe.dit, state_dict=dict(lora), alpha=4.0, hotload=True, hot_backend=backend)
            want = loop(tiny_pipe, lat, ctx_p, ctx_n, z0, 3)
            assert not torch.equal(want, base), backend
            assert torch.equal(loop(tiny_pipe, lat, ctx_p, ctx_n, z0, 3, graph=True), want), backend
            tiny_pipe.clear_lora()
    finally:
        tiny_pipe.clear_lora()
        tiny_pipe.dit.hot_lora_backend = "torch"
    assert torch.equal(loop(tiny_pipe, lat, ctx_p, ctx_n, z0, 3), base)


def test_eager_forward_calls_the_seams_as_before():
    """The eager forward hands the seams that tools replace (hip.attention; wan_video_dit.gemm_bias_own, gemm_bias_gelu_own, gemm_residual,
    gemm_fp8_own) exactly the arguments it handed them before the graph mode: no sched= / workspace= unless a recorded step owns them."""
    import inspect
    from fairygen_amd import wan_video_dit as wd
    seen = []
    real = _hip.attention
    try:
        _hip.attention = lambda q, k, v, num_heads, out=None, scale=None: seen.append((num_heads, out, scale))      # a wrapper of the old signature
        wd.AttentionModule(3)("q", "k", "v")
        wd.AttentionModule(3)("q", "k", "v", scale=0.5)
    finally:
        _hip.attention = real
    assert seen == [(3, None, None), (3, None, 0.5)]

    class Model:
        eps, fp8_dtype, hot_loras, hot_lora_backend = 1e-6, None, {}, "torch"
        qk8_fused_producer = pv8_attention = smoothv_attention = smoothv_cross_attention = False
    lin = wd._BlockLinears(Model(), 2)
    assert lin.owned is None and lin.state(1440, 3072, 6144) == {}
    att = wd._BlockAttention(Model(), lin)
    assert att.owned is None and att.workspace() == {}
    called = []
    att.attention(lambda *a, **kw: called.append((a, kw)), "q", "k", "v")
    att.attention(lambda *a, **kw: called.append((a, kw)), "q", "k", "v", 0.25)
    assert called == [(("q", "k", "v"), {}), (("q", "k", "v"), {"scale": 0.25})]
    for name in ("gemm_bias_own", "gemm_bias_gelu_own", "gemm_fp8_own", "gemm_residual"):
        params = list(inspect.signature(getattr(wd, name)).parameters.values())
        assert params[-1].kind is inspect.Parameter.VAR_KEYWORD and all(p.kind is not inspect.Parameter.KEYWORD_ONLY for p in params), name


# ------------------------------------------------------------------------------------------------------------------ 6. the ABI
def test_abi_8():
    lib = _hip.load()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == _hip.ABI_VERSION
    header = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    assert re.search(r"^int fg_cfg_euler_dev_bf16\(const void\* latents, const void\* posi, const void\* nega, void\* out,\s*int64_t n, float cfg_scale, "
                     r"const float\* dsigma_table, const int\* step,\s*const void\* first, int64_t first_n, int64_t frame_stride, fg_stream_t stream\);",
                     header, re.M), "include/fairygen_hip.h does not declare fg_cfg_euler_dev_bf16 with the agreed argument list"
    assert "ABI version, currently 8" in header
    assert NAME in _hip.EXPORTED_SYMBOLS and len(_hip.EXPORTED_SYMBOLS) == 55 and getattr(lib, NAME).argtypes == _hip._SIGNATURES[NAME]
    V, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert _hip._SIGNATURES[NAME] == [V, V, V, V, I64, F, V, V, V, I64, I64, V]


def test_older_signature_tables_unchanged():
    """The 36 entry points of ABI 7 are in hip._SIGNATURES with the argument types they had; entry points added since sit next to them."""
    assert len(set(SIGNATURES_ABI7)) == 36 and NAME not in SIGNATURES_ABI7
    lines = "\n".join(f"{n}:{','.join(t.__name__ for t in _hip._SIGNATURES[n])}" for n in sorted(SIGNATURES_ABI7))
    assert hashlib.sha256(lines.encode()).hexdigest() == SIGNATURES_SHA256, "hip._SIGNATURES differs from the table of ABI 7"


SIGNATURES_SHA256 = "f176879e9cbcd66f1073f9b5ac3b84525bda597f7ef32fd05aab596ae0d05a2a"

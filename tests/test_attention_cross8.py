"""The opt-in e4m3 cross-attention with a head's K8 and V8^T resident in LDS (WanModel.enable_qk8_attention(pv8=True, cross=True),
fg_attn_fwd_cross8_bf16, include/fairygen_hip_cross8.h).

The parity criterion is exact: a query row's arithmetic does not depend on the workgroup that holds it, so on the same operands the
output must be BIT FOR BIT that of fg_attn_fwd_pv8_bf16 launched without a workspace (hip.attention_pv8_pre(..., workspace=None): no
KV length this kernel takes has enough tiles for a split) — the kernel that tests/test_attention_pv8.py pins to the fp64 emulation of the
recipe.  No tolerance is written here; the one case that goes against the emulation itself uses that file's criterion and helpers.
  1. (no GPU) the extension's ABI, the argument checks, the switch and its raises, the config, the example flag;
  2. the kernel against fg_attn_fwd_pv8_bf16 with torch.equal, on operands from the library's own quantisers: every (Nq, Nkv) below, four
     kinds of data; 24 and 32 heads where every workgroup walks three query blocks, the last ragged; the exact construction;
  3. memory and stream hygiene: NaN bands around every operand, sentinels around out, refused arguments launch nothing, capture;
  4. the tiny DiT: the launches of a forward, the distance to the fp32 oracle, one context quantisation per kv_cache, graph=True.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import test_attention_pv8 as pv8
import test_attention_qk8 as qk8
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic
from test_attention_qk8 import ATTN_FLOOR, guarded, guards_intact, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8, U8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.float32
NAMES = ("fg_attn_fwd_cross8_bf16",)
QUERIES = ("fg_attn_cross8_version", "fg_attn_cross8_max_kv")
MAX_KV = 640      # 160 KiB / (128 B of K8 + 128 B of V8^T per key); asserted against the library below
DATA = ("normal", "peaked", "spiked", "peaked+spiked")
# (heads, Nq, Nkv): one row and one key; sizes below a tile; whole tiles; one past them; the context length of tiny prompts; the DiT's 512
# keys; the longest context with few and with many rows (several workgroups per head), its last tile ragged by one key
SHAPES = [(3, 1, 1), (3, 31, 5), (3, 256, 64), (3, 257, 65), (3, 300, 77), (3, 513, 512), (3, 70, MAX_KV), (3, 1300, MAX_KV - 63)]
# G = 10 and G = 8 on 256 CUs: every workgroup walks three query blocks (21 and 17 blocks of 256 rows), the last of the walk ragged
WALKS = [(24, 5157, 512), (32, 4133, 512)]


# ------------------------------------------------------------------------------------------------------------------ 1. the ABI and the switch
def test_extension_abi():
    lib = _hip.load()
    main = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    ext = open(os.path.join(REPO, "include", "fairygen_hip_cross8.h")).read()
    # the main table and the earlier extensions are what they were
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55
    assert len(_hip.PV8_SYMBOLS) == 4 and len(_hip.SHARD8_SYMBOLS) == 6
    others = _hip.EXPORTED_SYMBOLS + _hip.PV8_SYMBOLS + _hip.SHARD8_SYMBOLS
    assert not any(name in others or name in main for name in NAMES + QUERIES)
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.CROSS8_SYMBOLS == sorted(NAMES + QUERIES)
    assert _hip.CROSS8_ABI_VERSION == 1 and lib.fg_attn_cross8_version() == 1
    assert re.search(r"^int fg_attn_fwd_cross8_bf16\(const void\* q8, const void\* k8, const float\* sq, const float\* sk, const void\* v8t, "
                     r"const float\* sv, void\* out,\s*int64_t Nq, int64_t Nkv, int H, int D, float scale, fg_stream_t stream\);", ext, re.M)
    assert re.search(r"^int64_t fg_attn_cross8_max_kv\(void\);", ext, re.M)
    V, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert _hip._CROSS8_SIGNATURES == {NAMES[0]: [V, V, V, V, V, V, V, I64, I64, I32, I32, F, V]}
    assert _hip._CROSS8_QUERIES == {QUERIES[0]: (I32, []), QUERIES[1]: (I64, [])}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    assert getattr(lib, NAMES[0]).argtypes == _hip._CROSS8_SIGNATURES[NAMES[0]]
    max_kv = lib.fg_attn_cross8_max_kv()
    assert max_kv >= 512 and max_kv % 64 == 0 and max_kv == MAX_KV == _hip.attention_cross8_max_kv()
    assert 256 * max_kv <= 160 * 1024 < 256 * (max_kv + 64), "max_kv is what the 160 KiB budget holds, K8 and V8^T and nothing besides"
    assert "models/wan_video_dit.py:48-52" in ext and "PV8_KEY_ORDER" in ext


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1)."""
    lib, a = _hip.load(), 4096
    call = lib.fg_attn_fwd_cross8_bf16
    assert call(a, a, a, a, a, a, a, 10, 10, 2, 64, 0.1, None) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert call(a, a, a, a, a, a, a, 10, MAX_KV + 1, 2, 128, 0.1, None) == -1 and b"Nkv must be in 1..640" in lib.fg_last_error()
    assert call(a, a, a, a, a, a, a, 10, 0, 2, 128, 0.1, None) == -1 and b"Nkv" in lib.fg_last_error()
    assert call(a, a, a, a, a, a, a, 0, 10, 2, 128, 0.1, None) == -1 and call(a, a, a, a, a, a, a, 10, 10, 0, 128, 0.1, None) == -1
    assert call(a, a, a, a, a, a, a, 10, 10, 2, 128, 0.0, None) == -1 and b"scale" in lib.fg_last_error()
    for i in (0, 1, 4, 5, 6):      # q8, k8, v8t, sv, out: 16-byte aligned
        args = [a] * 7
        args[i] = a + 8
        assert call(*args, 10, 10, 2, 128, 0.1, None) == -1 and b"aligned" in lib.fg_last_error(), i
    for i in (2, 3):               # sq, sk: 4
        args = [a] * 7
        args[i] = a + 2
        assert call(*args, 10, 10, 2, 128, 0.1, None) == -1 and b"aligned" in lib.fg_last_error(), i
    for i in range(7):
        args = [a] * 7
        args[i] = None
        assert call(*args, 10, 10, 2, 128, 0.1, None) == -1 and b"null" in lib.fg_last_error(), i
    assert call(a, a, a, a, a, a, a, 1 << 24, 10, 2, 128, 0.1, None) == -1 and b"4 GiB" in lib.fg_last_error()


def test_enable_sets_the_routing():
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)
    attn = m.blocks[0].cross_attn.attn
    assert m.cross8_attention is False
    assert m.enable_qk8_attention(pv8=True) is m and m.cross8_attention is False, "the default is off"
    assert not dit.takes_cross8_attention(m, attn, 512, 1)
    for fused in (False, True):
        assert m.enable_qk8_attention(fused_producer=fused, pv8=True, cross=True) is m
        assert m.qk8_attention is True and m.pv8_attention is True and m.cross8_attention is True and m.qk8_fused_producer is fused
    # routing: the stock module, one batch element, a context that fits the LDS
    assert dit.takes_cross8_attention(m, attn, 512, 1) and dit.takes_cross8_attention(m, attn, 1, 1) and dit.takes_cross8_attention(m, attn, MAX_KV, 1)
    assert not dit.takes_cross8_attention(m, attn, MAX_KV + 1, 1) and not dit.takes_cross8_attention(m, attn, 512, 2)
    other = type("Other", (dit.AttentionModule,), {})
    assert not dit.takes_cross8_attention(m, other.__new__(other), 512, 1)
    assert m.attn_scale() == (128 ** -0.5, 1.0)
    for kw in ({}, {"pv8": False}, {"flag": False, "pv8": True}):
        with pytest.raises(ValueError, match="cross=True|pv8=True"):
            m.enable_qk8_attention(cross=True, **kw)
    assert m.cross8_attention is True, "a refused call leaves the switches alone"
    m.enable_qk8_attention(pv8=True)
    assert m.cross8_attention is False and m.pv8_attention is True, "an enable without cross= switches cross-attention back to bf16"
    m.enable_qk8_attention(pv8=True, cross=True)
    m.enable_qk8_attention(False)
    assert m.qk8_attention is False and m.pv8_attention is False and m.cross8_attention is False


def test_sharded_layout_raises():
    """An active token shard raises with cross=True, with or without sharded=True: no sharded run of it is tested."""
    from fairygen_amd.wan_video_dit import WanModel
    with torch.device("meta"):
        m = WanModel(**synthetic.TINY_DIT_KWARGS)

    class Shard:
        active = True
    for sharded in (False, True):
        m.enable_qk8_attention(pv8=True, cross=True, sharded=sharded)
        m.check_qk8_layout(None)
        with pytest.raises(NotImplementedError, match="cross=True"):
            m.check_qk8_layout(Shard())
        x = torch.empty((1, 8, 256), device="meta")
        with pytest.raises(NotImplementedError, match="cross=True"):
            next(m.forward_tokens_steps(x, x, torch.empty((1, 6, 256), device="meta"), x, 0, (x, x), Shard(), 16))
    m.enable_qk8_attention(pv8=True, sharded=True)
    m.check_qk8_layout(Shard())      # without cross= the sharded mode is what it was


def test_model_config(tmp_path):
    """ModelConfig(attention_dtype, attention_pv_dtype, cross_attention_dtype all e4m3) through ModelPool on a saved tiny DiT switches the
    three on; any other dtype, or one without the other two, raises; without it nothing changes."""
    from fairygen_amd import ModelConfig, loader
    assert ModelConfig(path="x").vram_config()["cross_attention_dtype"] is None
    assert ModelConfig(path="x", attention_dtype=F8, attention_pv_dtype=F8, cross_attention_dtype=F8).vram_config()["cross_attention_dtype"] == F8
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        base = {"computation_dtype": BF16, "computation_device": "cpu"}
        pool = loader.ModelPool()
        pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8, attention_pv_dtype=F8, cross_attention_dtype=F8))
        pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8, attention_pv_dtype=F8))
        pool.auto_load_model(path, vram_config=dict(base))
        m = pool.model[0]
        assert m.qk8_attention is True and m.pv8_attention is True and m.cross8_attention is True and m.qk8_fused_producer is True
        assert pool.model[1].pv8_attention is True and pool.model[1].cross8_attention is False
        assert pool.model[2].qk8_attention is False and pool.model[2].cross8_attention is False
        for bad in (torch.float8_e5m2, torch.float8_e4m3fnuz, torch.int8, BF16):
            with pytest.raises(NotImplementedError, match="cross_attention_dtype"):
                loader.ModelPool().auto_load_model(path, vram_config=dict(base, attention_dtype=F8, attention_pv_dtype=F8, cross_attention_dtype=bad))
        for partial in ({}, {"attention_dtype": F8}):
            with pytest.raises(NotImplementedError, match="without attention_dtype and attention_pv_dtype"):
                loader.ModelPool().auto_load_model(path, vram_config=dict(base, cross_attention_dtype=F8, **partial))
    finally:
        loader.MODEL_CONFIGS.remove(entry)


def test_example_flag_implies_pv8(monkeypatch):
    """examples/inference.py --cross8-attention alone: the DiT's ModelConfig gets all three dtypes; the other flags give what they gave."""
    from examples import inference

    class Built(Exception):
        pass

    def from_pretrained(**kw):
        raise Built(kw["model_configs"][1])
    monkeypatch.setattr(inference.WanVideoPipeline, "from_pretrained", staticmethod(from_pretrained))
    for flags, want in (([], (None, None, None)), (["--qk8-attention"], (F8, None, None)), (["--pv8-attention"], (F8, F8, None)),
                        (["--cross8-attention"], (F8, F8, F8)), (["--qk8-attention", "--cross8-attention"], (F8, F8, F8))):
        monkeypatch.setattr("sys.argv", ["inference.py", "--weights", "w", "--tokenizer", "t", "--image", "i.png"] + flags)
        with pytest.raises(Built) as e:
            inference.main()
        cfg = e.value.args[0]
        assert (cfg.attention_dtype, cfg.attention_pv_dtype, cfg.cross_attention_dtype) == want, flags


# ------------------------------------------------------------------------------------------------------------------ 2. the kernel
def cross_inputs(heads, nq, nkv, data):
    """q (nq, C), k and v (nkv, C) bf16 on the CPU, in the kinds of test_attention_qk8.attn_case: N(0, 1); peaked rows (q x 8); keys that
    move the running max by far more than 2^3 in the first tile, a middle one, the last full one and at the end of the ragged one."""
    c = heads * 128
    q, k, v = seeded((nq, c), 130, scale=8.0 if "peaked" in data else 1.0), seeded((nkv, c), 131), seeded((nkv, c), 132)
    if "spiked" in data:
        rows = [r % nq for r in (5, 17, 150, 255, 299, 5)]
        keys = [min(6, nkv - 1), nkv // 3, nkv // 2, max((nkv // 64) * 64 - 3, 0), max(nkv - 2, 0), nkv - 1]
        k = qk8._spiked_keys(q, k, list(zip(keys, rows)))
    return q, k, v


def quantise(hip, q, k, v, heads):  # noqa: F811
    """The operands of both kernels from the library's own quantisers, on the GPU: (q8, k8, sq, sk, v8t, sv)."""
    qd, kd, vd = q.cuda()[None], k.cuda()[None], v.cuda()[None]
    q8, _, sq, _, _ = hip.attn_quant_qk(qd, torch.zeros_like(qd), heads)
    _, k8, _, sk, _ = hip.attn_quant_qk(torch.zeros_like(kd), kd, heads)
    v8t, sv, _ = hip.attn_quant_vt(vd, heads)
    return q8, k8, sq, sk, v8t, sv


def assert_cross8_equals_pv8(hip, ops, heads, label):  # noqa: F811
    want = hip.attention_pv8_pre(*ops, heads, workspace=None)
    got = hip.attention_cross8_pre(*ops, heads)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all(), "the comparator itself"
    bad = (got != want).any(-1).flatten().nonzero().flatten()
    assert torch.equal(got, want), f"{label}: {bad.numel()} of {got.shape[1]} rows differ from fg_attn_fwd_pv8_bf16, first {bad[:8].tolist()}"
    return got


@gpu
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("heads,nq,nkv", SHAPES + WALKS, ids=[f"{h}x{a}x{b}" for h, a, b in SHAPES + WALKS])
def test_cross8_equals_pv8(hip, heads, nq, nkv, data):  # noqa: F811
    """torch.equal with the direct launch of fg_attn_fwd_pv8_bf16 on the same operands."""
    lib = hip.load()
    assert lib.fg_attn_cross8_max_kv() == MAX_KV and lib.fg_attn_workspace_bytes(1, nq, nkv, heads) == 0, "the comparator must be the direct launch"
    ops = quantise(hip, *cross_inputs(heads, nq, nkv, data), heads)
    assert_cross8_equals_pv8(hip, ops, heads, f"{heads} heads, Nq {nq}, Nkv {nkv}, {data}")


@gpu
def test_cross8_against_the_recipe(hip):  # noqa: F811
    """One case against the fp64 emulation of the recipe, under the criterion of test_attention_pv8_against_the_recipe (its operands, its
    yardstick, its factors): 600 queries and keys, peaked and spiked."""
    n, data = 600, "peaked+spiked"
    q8, k8, sq, sk, v8t, sv, ref, (e_max, e_spiked, e_mean) = pv8.attn_case(n, data)
    ops = [t.cuda().contiguous() for t in (q8, k8, sq, sk, v8t.view(F8), sv)]
    got = assert_cross8_equals_pv8(hip, ops, pv8.HEADS, "the recipe case")[0].cpu()
    err = (got.double() - ref).abs()
    g_max, g_spiked, g_mean = err.max().item(), err[list(pv8.SPIKED_ROWS)].max().item(), err.mean().item()
    print(f"cross8 attention N = {n}, {data}: max {g_max:.3e} (recipe {e_max:.3e}), spiked rows {g_spiked:.3e} (recipe {e_spiked:.3e}), "
          f"mean {g_mean:.3e} (recipe {e_mean:.3e})")
    assert g_max <= 2 * e_max + ATTN_FLOOR, f"max {g_max} vs {e_max}"
    assert g_spiked <= 2 * e_spiked + ATTN_FLOOR, f"spiked rows {g_spiked} vs {e_spiked}"
    assert g_mean <= 2 * e_mean + ATTN_FLOOR, f"mean {g_mean} vs {e_mean}"


@gpu
@pytest.mark.parametrize("n", (577, MAX_KV))
def test_cross8_exact(hip, n):  # noqa: F811
    """The exact construction of test_attention_pv8_exact through the quantisers and this kernel: the selected v row, bit for bit."""
    qk8.check_exact_case(n)
    q, k, v, want, _ = qk8.exact_case(n)
    got = assert_cross8_equals_pv8(hip, quantise(hip, q, k, v, qk8.HEADS), qk8.HEADS, f"exact, N {n}")
    bad = (got[0].cpu() != want).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {n} rows differ from the selected v row, first {bad[:8].tolist()}"


@gpu
@pytest.mark.parametrize("nkv", (512, 77))
def test_cross8_exact_last_key(hip, nkv):  # noqa: F811
    """300 queries, query 0 selects the last key: of the last full tile (512) and of a ragged tile with 13 of 64 keys live (77)."""
    nq, heads = 300, qk8.HEADS
    qk8.check_exact_case(nq, nkv, heads, (nkv - 1,))
    q, k, v, want, _ = qk8.exact_case(nq, nkv, heads, (nkv - 1,))
    got = assert_cross8_equals_pv8(hip, quantise(hip, q, k, v, heads), heads, f"exact, Nkv {nkv}")
    assert want[0].view(heads, 128).argmax(1).tolist() == [(nkv - 1) % 128] * heads
    bad = (got[0].cpu() != want).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {nq} rows differ from the selected v row, first {bad[:8].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ 3. memory and streams
BAND = 4096      # bytes on either side of an operand


def banded(t, fill):
    """A copy of t between two bands of `fill` bytes in one buffer (0x7F: the e4m3 NaN; four 0xFF: an fp32 NaN): (the buffer, the view)."""
    nbytes = t.numel() * t.element_size()
    full = torch.full((2 * BAND + nbytes,), fill, dtype=U8, device="cuda")
    view = full[BAND:BAND + nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return full, view


@gpu
@pytest.mark.parametrize("heads,nq,nkv", [(3, 300, 77), (3, 257, 512)])
def test_cross8_reads_and_writes_inside_its_buffers(hip, heads, nq, nkv):  # noqa: F811
    """Every operand between NaN bands and out between sentinel rows: the result is that of the plain buffers, so nothing past an operand
    (the key rows of a ragged tile's padding among them) reached it, and the guard rows of out are intact."""
    ops = quantise(hip, *cross_inputs(heads, nq, nkv, "spiked"), heads)
    want = hip.attention_cross8_pre(*ops, heads)
    held = [banded(t, 0x7F if t.dtype == F8 else 0xFF) for t in ops]
    full, out = guarded((nq, heads * 128), BF16)
    hip.attention_cross8_pre(*[v for _, v in held], heads, out=out.unsqueeze(0))
    torch.cuda.synchronize()
    assert guards_intact(full), "a guard row of out was written"
    assert torch.equal(out, want[0])
    for (buf, view), t in zip(held, ops):
        assert torch.equal(view.view(U8), t.view(U8)) and (buf[:BAND] == buf[0]).all() and (buf[-BAND:] == buf[0]).all(), "an operand was written"


@gpu
def test_refused_arguments_launch_nothing(hip):  # noqa: F811
    """Nkv = max_kv + 1, D = 64 and a misaligned pointer: the argument error, and out keeps its sentinel."""
    heads, nq, nkv = 2, 40, MAX_KV + 1
    c = heads * 128
    q8, k8 = torch.zeros((nq, c), dtype=F8, device="cuda"), torch.zeros((nkv, c), dtype=F8, device="cuda")
    sq, sk = torch.ones((nq, heads), device="cuda"), torch.ones(heads, device="cuda")
    v8t, sv = torch.zeros((heads, 128, 704), dtype=F8, device="cuda"), torch.ones((heads, 128), device="cuda")
    full, out = guarded((nq, c), BF16)
    lib, p, s = hip.load(), hip._ptr, hip._stream(out)
    ptrs = [p(t) for t in (q8, k8, sq, sk, v8t, sv, out)]
    assert lib.fg_attn_fwd_cross8_bf16(*ptrs, nq, nkv, heads, 128, 0.1, s) == -1 and b"Nkv must be in 1..640" in lib.fg_last_error()
    assert lib.fg_attn_fwd_cross8_bf16(*ptrs, nq, 64, 2 * heads, 64, 0.1, s) == -1 and b"head_dim 128" in lib.fg_last_error()
    odd = list(ptrs)
    odd[0] = ctypes.c_void_p(q8.data_ptr() + 8)
    assert lib.fg_attn_fwd_cross8_bf16(*odd, nq, 64, heads, 128, 0.1, s) == -1 and b"aligned" in lib.fg_last_error()
    with pytest.raises(hip.HipLibraryError, match="Nkv must be in"):
        hip.attention_cross8_pre(q8, k8, sq, sk, v8t, sv, heads, out=out.unsqueeze(0))
    torch.cuda.synchronize()
    assert (full == qk8.POISON).all(), "a refused call wrote to out"


@gpu
def test_entry_point_only_enqueues_and_captures(hip):  # noqa: F811
    """The entry point recorded on a side stream into a graph: nothing runs at capture (out keeps its fill), two replays give the bits of
    the eager call."""
    heads, nq, nkv = 3, 700, 512
    ops = quantise(hip, *cross_inputs(heads, nq, nkv, "normal"), heads)
    want = hip.attention_cross8_pre(*ops, heads)
    torch.cuda.synchronize()
    out = torch.zeros_like(want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        hip.attention_cross8_pre(*ops, heads, out=out)
    torch.cuda.synchronize()
    assert (out == 0).all(), "a capture launched work"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        out.zero_()


# ------------------------------------------------------------------------------------------------------------------ 4. the tiny DiT
def tiny_args():
    lat, ctx, ts = seeded(qk8.LATENT, 11), seeded((1, 16, 128), 12), torch.tensor([995.9]).to(BF16)
    return dict(latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)


@gpu
def test_tiny_dit_forward(hip, monkeypatch):  # noqa: F811
    """enable_qk8_attention(pv8=True, cross=True) on the tiny DiT of test_attention_pv8.test_tiny_dit_forward (1 200 tokens, 16 context
    rows): the launches of a forward, and 1 - cos to the fp32 oracle next to the bf16 and pv8 figures, held to that test's bound for pv8
    (2 d_recipe).  Mode off: the forward is the default path's, bit for bit."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, sd, cfg = qk8.tiny_model()
    args = tiny_args()
    calls, real = [], hip._call

    def call(name, *a):
        calls.append((name, a))
        return real(name, *a)
    with torch.no_grad():
        out_bf16 = model_fn_wan_video(m, **args)
        out_pv8 = model_fn_wan_video(m.enable_qk8_attention(fused_producer=True, pv8=True), **args)
        monkeypatch.setattr(hip, "_call", call)
        out_cross = model_fn_wan_video(m.enable_qk8_attention(fused_producer=True, pv8=True, cross=True), **args)
        monkeypatch.setattr(hip, "_call", real)
        out_back = model_fn_wan_video(m.enable_qk8_attention(False), **args)
    nb = cfg["num_layers"]
    count = lambda name: sum(1 for n_, _ in calls if n_ == name)      # noqa: E731
    assert count("fg_attn_fwd_cross8_bf16") == nb and count("fg_attn_fwd_pv8_bf16") == nb
    # fg_attn_fwd_bf16(q, ldq, k, ldk, v, ldv, out, B, Nq, Nkv, ..): no launch over a text-sized context is left
    assert not [a for n_, a in calls if n_ == "fg_attn_fwd_bf16" and a[9] <= 1024], "cross-attention still reaches the bf16 kernel"
    # with the fused producers no bf16 q (or k) norm is left anywhere: the q norms write e4m3 rows (self and cross: 2 per block), the k
    # norms write bf16 k with its statistics (self and cross)
    assert count("fg_rmsnorm_rope_bf16") == 0 and count("fg_rmsnorm_rope_q8_bf16") == 2 * nb and count("fg_rmsnorm_rope_kstats_bf16") == 2 * nb
    assert count("fg_attn_quant_k_bf16") == 2 * nb and count("fg_attn_quant_vt_bf16") == 2 * nb
    assert torch.isfinite(out_cross.float()).all()
    assert torch.equal(out_back, out_bf16), "mode off is not the default path"
    assert not torch.equal(out_cross, out_pv8) and not torch.equal(out_cross, out_bf16), "the switch is dead"

    want32, want_emu = pv8.tiny_oracle()
    cos = qk8.cos_distance
    d_recipe = cos(want_emu, want32)
    d_cross, d_pv8, d_bf16 = cos(out_cross, want32), cos(out_pv8, want32), cos(out_bf16, want32)
    print(f"tiny DiT, 1 200 tokens, 16 context rows: 1 - cos to the fp32 oracle: cross8 kernels {d_cross:.3e}, pv8 kernels {d_pv8:.3e}, bf16 "
          f"kernels {d_bf16:.3e}, the pv8 recipe in the bf16 oracle {d_recipe:.3e}; cross8 to pv8 kernels {cos(out_cross, out_pv8):.3e}")
    assert d_cross <= 2 * d_recipe, (d_cross, d_recipe)


@gpu
def test_kv_cache_quantises_a_context_once(hip, monkeypatch):  # noqa: F811
    """Two forwards with one kv_cache: each block's context is projected and quantised in the first only, the cache holds
    (k8, sk, v8t, sv), and the second forward gives the bits of the first.  Mode off: the entries are the bf16 (k, v) pairs."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, _, cfg = qk8.tiny_model()
    args, nb = tiny_args(), cfg["num_layers"]
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(hip, "_call", call)
    with torch.no_grad():
        m.enable_qk8_attention(pv8=True, cross=True)      # two-step producers: self-attention does not use fg_attn_quant_k_bf16
        cache = {}
        first = model_fn_wan_video(m, kv_cache=cache, **args)
        per_forward = {n_: calls.count(n_) for n_ in ("fg_attn_quant_k_bf16", "fg_rmsnorm_rope_kstats_bf16", "fg_attn_quant_vt_bf16")}
        second = model_fn_wan_video(m, kv_cache=cache, **args)
        assert per_forward == {"fg_attn_quant_k_bf16": nb, "fg_rmsnorm_rope_kstats_bf16": nb, "fg_attn_quant_vt_bf16": 2 * nb}
        assert calls.count("fg_attn_quant_k_bf16") == nb and calls.count("fg_rmsnorm_rope_kstats_bf16") == nb, "a context was quantised twice"
        assert calls.count("fg_attn_quant_vt_bf16") == 3 * nb and calls.count("fg_attn_fwd_cross8_bf16") == 2 * nb
        assert torch.equal(first, second)
        (entry,) = cache["entries"]
        for i in range(nb):
            k8, sk, v8t, sv = entry["kv"][i]
            assert (k8.dtype, sk.dtype, v8t.dtype, sv.dtype) == (F8, F32, F8, F32)
            assert k8.shape == (16, 256) and sk.shape == (2,) and v8t.shape == (2, 128, 64) and sv.shape == (2, 128)
        m.enable_qk8_attention(False)
        cache = {}
        model_fn_wan_video(m, kv_cache=cache, **args)
        (entry,) = cache["entries"]
        for i in range(nb):
            kc, vc = entry["kv"][i]
            assert kc.dtype == BF16 and vc.dtype == BF16 and kc.shape == vc.shape == (1, 16, 256)


@gpu
def test_graph_loop_equals_eager(hip):  # noqa: F811
    """graph=True on the tiny loop with the mode on: the captured step owns the q8 / sq buffers of cross-attention, the context operands
    live in the loop's kv_cache, and the replays give the bits of the eager loop."""
    from fairygen_amd.wan_video import WanVideoPipeline
    m, _, _ = qk8.tiny_model()
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.enable_qk8_attention(pv8=True, cross=True)
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
    want = loop(False)
    got = loop(True)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} latents differ from the eager loop"
    pipe.dit.enable_qk8_attention(pv8=True)
    assert not torch.equal(loop(False), want), "the loop above ran without the e4m3 cross-attention"

"""The opt-in e4m3 P V product of the e4m3 Q K^T self-attention (WanModel.enable_qk8_attention(pv8=True), fg_attn_quant_vt_bf16 +
fg_attn_fwd_pv8_bf16, include/fairygen_hip_pv8.h): both MFMAs of self-attention 8-bit, what the reference's sageattn call
(models/wan_video_dit.py:48-52) resolves to on current parts.

The recipe (DESIGN §5 "e4m3 P V") is written out below in torch (`quant_v_emu`, `attn_pv8_emu`) next to the Q K^T half of
tests/test_attention_qk8.py, whose helpers and generators this file imports, and is what the kernels are held to:
  1. (no GPU) the recipe's own properties: sv never overflows, an all-zero channel gives the floor and zeros, c 2^T <= 448 with c a power of
     two, PV8_KEY_ORDER is a permutation, and the tie exemption of the V-quantise test is rare;
  2. (no GPU) the extension's ABI: its own header, its own tables, the main table and its version untouched; the switch, the config, the
     raises;
  3. fg_attn_quant_vt_bf16: sv bit for bit, bytes (PV8_KEY_ORDER undone) bit for bit outside rounding ties, padding zero, guards intact;
  4. fg_attn_fwd_pv8_bf16 against the yardstick ref = the fp64 attn_emu on the same q8 / k8 with the bf16 v:
     max|gpu - ref| <= 2 max|attn_pv8_emu - ref| + floor, the same for the spiked rows alone and for the mean absolute error; and the
     exact case through the whole chain;
  5. the tiny DiT, eager and graph=True; both entry points captured on a side stream.

Measured on the MI355X (2 heads, direct launch; max and mean |gpu - ref| against max and mean |attn_pv8_emu - ref|; the split-KV launch
within 5 % of these except peaked at 2 049, 1.51e-1): N = 1 100: normal 1.33e-2, 1.46e-3 against 1.28e-2, 1.43e-3; peaked 1.64e-1, 1.46e-2
against 1.41e-1, 1.46e-2; spiked 1.25e-1, 5.39e-3 against 1.18e-1, 5.39e-3; peaked+spiked 1.36e-1, 1.77e-2 against 1.30e-1, 1.77e-2.
N = 2 049: normal 9.99e-3, 1.06e-3 against 9.41e-3, 1.04e-3; peaked 1.97e-1, 1.46e-2 against 1.49e-1, 1.44e-2; spiked 1.25e-1, 4.45e-3
against 1.21e-1, 4.46e-3; peaked+spiked 1.41e-1, 1.81e-2 against 1.34e-1, 1.82e-2.  The producer: 0 bytes differ from the emulation at
every N (its division is IEEE's).  The 28 GPU tests take 5.5 s of pytest time.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import test_attention_qk8 as qk8
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic
from oracle import wan_dit
from test_attention_qk8 import ATTN_FLOOR, FLOOR_SCALE, guarded, guards_intact, hip, near_tie  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
HEADS = qk8.HEADS
QUANT_N = (1, 63, 64, 65, 1100)
TIE_N = (1, 63, 1100)
ATTN_N = qk8.ATTN_N            # 1 100 and 2 049: the kernel, a ragged last tile, and with a workspace the split-KV path
C_P = 2.0 ** _hip.PV8_LOG2_C   # the library's c
ORDER = torch.tensor(_hip.PV8_KEY_ORDER)


# ------------------------------------------------------------------------------------------------------------------ the recipe
def quant_v_emu(v, heads):
    """v (N, heads*128) bf16 -> sv (heads, 128) fp32, v8 (N, heads*128) e4m3, and the fp32 quotients that were rounded."""
    n = v.shape[0]
    vf = v.float().view(n, heads, 128)
    sv = torch.clamp(vf.abs().amax(0) / 448.0, min=FLOOR_SCALE)
    x = vf / sv
    return sv, x.clamp(-448, 448).to(F8).view(n, -1), x.view(n, -1)


def attn_pv8_emu(q8, k8, sq, sk, v8, sv, heads, scale=128 ** -0.5):
    """The recipe on given operands: an fp64 softmax relative to the final row maximum, P8 = e4m3(c p), an fp64 product with v8, the row
    sum of the unrounded p: out = (P8 v8) sv / (c sum p), (Nq, heads*128) fp64."""
    nq, nkv = q8.shape[0], k8.shape[0]
    a, b, vv = q8.double().view(nq, heads, 128), k8.double().view(nkv, heads, 128), v8.double().view(nkv, heads, 128)
    out = torch.empty((nq, heads, 128), dtype=torch.float64)
    for h in range(heads):
        s = (a[:, h] @ b[:, h].T) * (scale * sq[:, h].double().unsqueeze(1) * sk[h].double())
        p = torch.exp(s - s.amax(1, keepdim=True))
        p8 = (C_P * p).float().to(F8).double()
        out[:, h] = (p8 @ vv[:, h]) * sv[h].double() / (C_P * p.sum(1, keepdim=True))
    return out.view(nq, -1)


def to_tiles(v8, heads):
    """v8 (N, heads*128) e4m3 -> the v8t layout (heads, 128, Nkp) as uint8: transposed, zero padding, PV8_KEY_ORDER inside each tile."""
    n = v8.shape[0]
    nkp = (n + 63) // 64 * 64
    nat = torch.zeros((heads, 128, nkp), dtype=torch.uint8)
    nat[:, :, :n] = v8.view(torch.uint8).view(n, heads, 128).permute(1, 2, 0)
    return nat.view(heads, 128, nkp // 64, 64)[..., ORDER].reshape(heads, 128, nkp).contiguous()


def from_tiles(v8t, n):
    """The inverse of to_tiles: (heads, 128, Nkp) uint8 -> (the natural (n, heads*128) uint8, the padding bytes)."""
    heads, _, nkp = v8t.shape
    nat = v8t.view(heads, 128, nkp // 64, 64)[..., torch.argsort(ORDER)].reshape(heads, 128, nkp)
    return nat[:, :, :n].permute(2, 0, 1).reshape(n, heads * 128), nat[:, :, n:]


@functools.lru_cache(maxsize=None)
def quant_case(n):
    """The v column slice of test_attention_qk8's q | k | v buffer and its emulation."""
    qkv, _ = qk8.quant_case(n)
    return qkv, quant_v_emu(qkv[:, 2 * HEADS * 128:], HEADS)


# ------------------------------------------------------------------------------------------------------------------ 1. the recipe's properties
@pytest.mark.parametrize("n", QUANT_N)
def test_recipe_sv_never_overflows(n):
    _, (sv, v8, x) = quant_case(n)
    assert torch.isfinite(v8.float()).all() and v8.float().abs().max() <= 448
    assert x.abs().max() <= 448 * (1 + 2.0 ** -22) and (sv >= FLOOR_SCALE).all()
    # every channel reaches the top of the range: its own maximum maps to +-448
    assert (v8.float().view(n, HEADS, 128).abs().amax(0) == 448).all()


def test_recipe_zero_channel():
    v = seeded((70, 256), 6)
    v[:, 130] = 0
    sv, v8, _ = quant_v_emu(v, 2)
    assert sv[1, 2] == FLOOR_SCALE and (v8.float()[:, 130] == 0).all() and (sv.flatten()[torch.arange(256) != 130] > FLOOR_SCALE).all()
    q8, k8, sq, sk, _, _ = qk8.quant_emu(seeded((70, 256), 3), seeded((70, 256), 4), 2)
    out = attn_pv8_emu(q8, k8, sq, sk, v8, sv, 2)
    assert torch.isfinite(out).all() and (out[:, 130] == 0).all()


def test_recipe_constants():
    """c is a power of two and c 2^T <= 448: the deferred rescale bounds p by 2^T, so P8 never saturates; and the table is a permutation
    whose 4-aligned key groups stay together (the producer writes them as one dword)."""
    assert _hip.PV8_LOG2_C == 5 and _hip.PV8_DEFER_LOG2 == 3 and C_P == 32.0
    assert C_P * 2.0 ** _hip.PV8_DEFER_LOG2 <= 448 and C_P * 2.0 ** (_hip.PV8_DEFER_LOG2 + 1) > 448
    assert len(_hip.PV8_KEY_ORDER) == 64 and sorted(_hip.PV8_KEY_ORDER) == list(range(64))
    # lane half hh = p >> 5 of the S^T accumulators holds the keys 32 sub + 8 i + 4 hh + j (j < 4) of a tile: register 4 i + j of sub
    for p, key in enumerate(_hip.PV8_KEY_ORDER):
        hh, sub, reg = p >> 5, (p >> 4) & 1, p & 15
        assert key == 32 * sub + 8 * (reg >> 2) + 4 * hh + (reg & 3)
    x = torch.arange(5 * 64 * 256, dtype=torch.int64).remainder(251).to(torch.uint8).view(5 * 64, 256)[:300]
    nat, pad = from_tiles(to_tiles(x.view(F8), 2), 300)
    assert torch.equal(nat, x) and (pad == 0).all()


def test_recipe_tie_exemption_is_rare():
    """test_attention_qk8's test of that name for v: the recipe with the quotient formed as x * (1 / s) moves fewer than 0.1 % of the bytes
    and only where the quotient lies within one fp32 ulp of an e4m3 tie.  Bytes that differ / elements on these seeds: N = 1: 0 / 256,
    N = 63: 8 / 16 128 (0.050 %), N = 1 100: 142 / 281 600 (0.050 %), of 0, 86 and 913 quotients within an ulp of a tie (printed below)."""
    for n in TIE_N:
        qkv, (sv, v8, x) = quant_case(n)
        vf = qkv[:, 2 * HEADS * 128:].float().view(n, HEADS, 128)
        alt = (vf * (1.0 / sv)).clamp(-448, 448).to(F8).view(n, -1)
        diff = alt.view(torch.uint8) != v8.view(torch.uint8)
        assert not (diff & ~near_tie(x)).any(), "a one-ulp change of the quotient moved a byte away from a tie"
        print(f"N = {n}: {diff.sum().item()} of {x.numel()} bytes differ under x * (1 / s); {near_tie(x).sum().item()} quotients within one "
              f"ulp of an e4m3 tie")
        assert diff.sum().item() < 1e-3 * x.numel()


# ------------------------------------------------------------------------------------------------------------------ 2. the ABI and the switch
NAMES = ("fg_attn_quant_vt_bf16", "fg_attn_fwd_pv8_bf16")
QUERIES = ("fg_attn_pv8_version", "fg_attn_pv8_scratch_bytes")


def test_extension_abi():
    lib = _hip.load()
    main = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    ext = open(os.path.join(REPO, "include", "fairygen_hip_pv8.h")).read()
    # the main table is what it was
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55
    assert not any(name in _hip.EXPORTED_SYMBOLS or name in main for name in NAMES + QUERIES)
    # the extension: its header includes the main one and declares each symbol once; the second tables match it; the versions agree
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.PV8_SYMBOLS == sorted(NAMES + QUERIES)
    assert _hip.PV8_ABI_VERSION == 1 and lib.fg_attn_pv8_version() == 1
    assert re.search(r"^int fg_attn_quant_vt_bf16\(const void\* v, int64_t ldv, void\* v8t, float\* sv, void\* scratch, int64_t scratch_bytes, "
                     r"int64_t N, int H,\s*int D, fg_stream_t stream\);", ext, re.M)
    assert re.search(r"^int fg_attn_fwd_pv8_bf16\(const void\* q8, const void\* k8, const float\* sq, const float\* sk, const void\* v8t, "
                     r"const float\* sv, void\* out,\s*int64_t Nq, int64_t Nkv, int H, int D, float scale, void\* workspace, "
                     r"int64_t workspace_bytes,\s*fg_stream_t stream\);", ext, re.M)
    assert re.search(r"^int64_t fg_attn_pv8_scratch_bytes\(int64_t N, int H\);", ext, re.M)
    V, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert _hip._PV8_SIGNATURES == {NAMES[0]: [V, I64, V, V, V, I64, I64, I32, I32, V],
                                    NAMES[1]: [V, V, V, V, V, V, V, I64, I64, I32, I32, F, V, I64, V]}
    assert _hip._PV8_QUERIES == {QUERIES[0]: (I32, []), QUERIES[1]: (I64, [I64, I32])}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    for name in NAMES:
        assert getattr(lib, name).argtypes == _hip._PV8_SIGNATURES[name]
    assert "models/wan_video_dit.py:48-52" in ext and "PV8_KEY_ORDER" in ext


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1)."""
    lib, a = _hip.load(), 4096
    assert lib.fg_attn_pv8_scratch_bytes(1100, 2) == 69 * 256 * 4 and lib.fg_attn_pv8_scratch_bytes(10 ** 6, 24) == 256 * 24 * 128 * 4
    assert lib.fg_attn_pv8_scratch_bytes(0, 2) == -1 and lib.fg_attn_pv8_scratch_bytes(5, 0) == -1
    assert lib.fg_attn_quant_vt_bf16(a, 256, a, a, a, 1024, 10, 2, 64, None) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert lib.fg_attn_quant_vt_bf16(a, 255, a, a, a, 1024, 10, 2, 128, None) == -1                      # ldv < H*D
    assert lib.fg_attn_quant_vt_bf16(a, 256, a, a, a, 1023, 10, 2, 128, None) == -1 and b"scratch" in lib.fg_last_error()
    assert lib.fg_attn_quant_vt_bf16(a, 256, a + 8, a, a, 1024, 10, 2, 128, None) == -1                  # v8t not 16-byte aligned
    assert lib.fg_attn_quant_vt_bf16(a, 256, a, None, a, 1024, 10, 2, 128, None) == -1
    assert lib.fg_attn_fwd_pv8_bf16(a, a, a, a, a, a, a, 10, 10, 2, 64, 0.1, None, 0, None) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert lib.fg_attn_fwd_pv8_bf16(a, a, a, a, a, a, a, 10, 10, 2, 128, 0.0, None, 0, None) == -1      # scale
    assert lib.fg_attn_fwd_pv8_bf16(a, a, a, a, a + 8, a, a, 10, 10, 2, 128, 0.1, None, 0, None) == -1  # v8t not 16-byte aligned
    assert lib.fg_attn_fwd_pv8_bf16(a, a, a, a, a, None, a, 10, 10, 2, 128, 0.1, None, 0, None) == -1
    assert lib.fg_attn_fwd_pv8_bf16(a, a, a, a, a, a, a, 10, 10, 2, 128, 0.1, None, 64, None) == -1     # workspace bytes without a workspace
    assert lib.fg_attn_fwd_pv8_bf16(a, a, a, a, a, a, a, 10, 1 << 25, 2, 128, 0.1, None, 0, None) == -1 and b"4 GiB" in lib.fg_last_error()


def test_enable_sets_the_routing():
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)
    attn = m.blocks[0].self_attn.attn
    assert m.pv8_attention is False
    assert m.enable_qk8_attention() is m and m.qk8_attention is True and m.pv8_attention is False, "the default is off"
    for fused in (False, True):      # either producer path
        assert m.enable_qk8_attention(fused_producer=fused, pv8=True) is m
        assert m.qk8_attention is True and m.pv8_attention is True and m.qk8_fused_producer is fused
    # routing is the e4m3 Q K^T mode's: the stock module, more than QK8_MIN_KV keys, one batch element
    assert dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV + 1, 1) and not dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV, 1)
    other = type("Other", (dit.AttentionModule,), {})
    assert not dit.takes_qk8_attention(m, other.__new__(other), 4096, 1) and not dit.takes_qk8_attention(m, attn, 4096, 2)
    assert m.attn_scale() == (128 ** -0.5, 1.0)
    with pytest.raises(ValueError, match="pv8"):
        m.enable_qk8_attention(False, pv8=True)
    m.enable_qk8_attention(False)
    assert m.qk8_attention is False and m.pv8_attention is False
    m.enable_qk8_attention(pv8=True)
    m.enable_qk8_attention()
    assert m.pv8_attention is False, "a plain enable switches the P V half back to bf16"


def test_sharded_layout_raises():
    from fairygen_amd.wan_video_dit import WanModel
    with torch.device("meta"):
        m = WanModel(**synthetic.TINY_DIT_KWARGS)

    class Shard:
        active = True
    m.enable_qk8_attention(pv8=True)
    m.check_qk8_layout(None)
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.check_qk8_layout(Shard())
    x = torch.empty((1, 8, 256), device="meta")
    with pytest.raises(NotImplementedError, match="token-sharded"):
        next(m.forward_tokens_steps(x, x, torch.empty((1, 6, 256), device="meta"), x, 0, (x, x), Shard(), 16))


def test_model_config(tmp_path):
    """ModelConfig(attention_dtype=e4m3, attention_pv_dtype=e4m3) through ModelPool on a saved tiny DiT switches both halves on; any other
    P V dtype, or one without attention_dtype, raises."""
    from fairygen_amd import ModelConfig, loader
    assert ModelConfig(path="x").vram_config()["attention_pv_dtype"] is None
    assert ModelConfig(path="x", attention_dtype=F8, attention_pv_dtype=F8).vram_config()["attention_pv_dtype"] == F8
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        base = {"computation_dtype": BF16, "computation_device": "cpu"}
        pool = loader.ModelPool()
        pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8, attention_pv_dtype=F8))
        pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8))
        assert pool.model[0].qk8_attention is True and pool.model[0].pv8_attention is True and pool.model[0].qk8_fused_producer is True
        assert pool.model[1].qk8_attention is True and pool.model[1].pv8_attention is False
        for bad in (torch.float8_e5m2, torch.float8_e4m3fnuz, torch.int8, BF16):
            with pytest.raises(NotImplementedError, match="attention_pv_dtype"):
                loader.ModelPool().auto_load_model(path, vram_config=dict(base, attention_dtype=F8, attention_pv_dtype=bad))
        with pytest.raises(NotImplementedError, match="without attention_dtype"):
            loader.ModelPool().auto_load_model(path, vram_config=dict(base, attention_pv_dtype=F8))
    finally:
        loader.MODEL_CONFIGS.remove(entry)


def test_example_flag_implies_qk8(monkeypatch):
    """examples/inference.py --pv8-attention alone: main() asks build_pipeline for both halves, and build_pipeline hands the DiT's
    ModelConfig both dtypes (and neither without a flag; --qk8-attention alone: the Q K^T half only)."""
    from examples import inference

    class Built(Exception):
        pass

    def from_pretrained(**kw):
        raise Built(kw["model_configs"][1])
    monkeypatch.setattr(inference.WanVideoPipeline, "from_pretrained", staticmethod(from_pretrained))
    for flags, want in (([], (None, None)), (["--qk8-attention"], (F8, None)), (["--pv8-attention"], (F8, F8)),
                        (["--qk8-attention", "--pv8-attention"], (F8, F8))):
        monkeypatch.setattr("sys.argv", ["inference.py", "--weights", "w", "--tokenizer", "t", "--image", "i.png"] + flags)
        with pytest.raises(Built) as e:
            inference.main()
        cfg = e.value.args[0]
        assert (cfg.attention_dtype, cfg.attention_pv_dtype) == want, flags


# ------------------------------------------------------------------------------------------------------------------ 3. fg_attn_quant_vt_bf16
@gpu
@pytest.mark.parametrize("n", QUANT_N)
def test_quant_vt_against_the_recipe(hip, n):  # noqa: F811
    qkv, (sv, v8, x) = quant_case(n)
    c, nkp = HEADS * 128, (n + 63) // 64 * 64
    # the rows live between guard rows of NaN, and the q | k slices (inside the leading dimension, never read) are NaN too
    src = torch.full((n + 2, 3 * c), float("nan"), dtype=BF16)
    src[1:-1, 2 * c:] = qkv[:, 2 * c:]
    d = src.cuda()[1:-1].unsqueeze(0)
    need = hip.load().fg_attn_pv8_scratch_bytes(n, HEADS)
    fulls, bufs = zip(*[guarded(s, t) for s, t in (((HEADS, 128, nkp), F8), ((HEADS, 128), torch.float32), ((1, need), torch.uint8))])
    got = hip.attn_quant_vt(d[..., 2 * c:], HEADS, (bufs[0], bufs[1], bufs[2].view(need)))
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in fulls), "a guard row of an output was written"
    g_sv, g_t = got[1].cpu(), got[0].cpu().view(torch.uint8)
    assert torch.equal(g_sv, sv), f"sv: {(g_sv != sv).sum().item()} of {sv.numel()} differ"
    g8, pad = from_tiles(g_t, n)
    assert (pad == 0).all(), f"{(pad != 0).sum().item()} of {pad.numel()} padding bytes are not zero"
    w8 = v8.view(torch.uint8)
    diff, tie = g8 != w8, near_tie(x)
    print(f"N = {n}, v8: {diff.sum().item()} bytes differ, {tie.sum().item()} quotients within one ulp of a tie")
    assert not (diff & ~tie).any(), f"{(diff & ~tie).sum().item()} bytes differ away from a rounding tie"
    # a byte that differs at a tie is the other neighbour: within one e4m3 step
    assert (g8.view(F8).float()[diff] - v8.float()[diff]).abs().le((x[diff].abs() / 8).clamp(min=2.0 ** -9)).all()
    assert diff.sum().item() <= 1e-3 * n * c, f"{diff.sum().item()} of {n * c} elements used the tie exemption"


# ------------------------------------------------------------------------------------------------------------------ 4. fg_attn_fwd_pv8_bf16
SPIKED_ROWS = (5, 17, 150, 255, 299)


@functools.lru_cache(maxsize=None)
def attn_case(n, data):
    """test_attention_qk8's attn_case with the V half of the recipe: the operands, the yardstick ref (fp64 attn_emu on the same q8 / k8
    with the bf16 v) and the recipe's own distance from it, as a maximum (all rows, the spiked rows) and as a mean."""
    q8, k8, sq, sk, v, ref, _ = qk8.attn_case(n, data)
    sv, v8, _ = quant_v_emu(v, HEADS)
    e = (attn_pv8_emu(q8, k8, sq, sk, v8, sv, HEADS) - ref).abs()
    return q8, k8, sq, sk, to_tiles(v8, HEADS), sv, ref, (e.max().item(), e[list(SPIKED_ROWS)].max().item(), e.mean().item())


def run_fwd(hip, q8, k8, sq, sk, v8t, sv, n, split):  # noqa: F811
    lib = hip.load()
    need = lib.fg_attn_workspace_bytes(1, n, n, HEADS) if split else 0
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, HEADS * 128), dtype=BF16, device="cuda")
    ops = [t.cuda().contiguous() for t in (q8, k8, sq, sk, v8t, sv)]
    hip._call("fg_attn_fwd_pv8_bf16", *[hip._ptr(t) for t in ops], hip._ptr(out), n, n, HEADS, 128, 128 ** -0.5,
              hip._ptr(ws) if need > 0 else None, need, hip._stream(out))
    torch.cuda.synchronize()
    return out.cpu()


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["direct", "split-kv"])
@pytest.mark.parametrize("data", ["normal", "peaked", "spiked", "peaked+spiked"])
@pytest.mark.parametrize("n", ATTN_N)
def test_attention_pv8_against_the_recipe(hip, n, data, split):  # noqa: F811
    """The yardstick is not the kernel: err_recipe is how far the recipe in fp64 sits from the same attention with the bf16 v.  The kernel
    may sit twice as far plus the floor: it rounds P relative to a running maximum that is smaller than or equal to the final one the
    emulation uses — so its P is resolved at least as finely — accumulates in fp32 and rounds the result to bf16."""
    q8, k8, sq, sk, v8t, sv, ref, (e_max, e_spiked, e_mean) = attn_case(n, data)
    if split:
        R, S = qk8.split_choice(hip, n, hip.load().fg_attn_workspace_bytes(1, n, n, HEADS))
        assert R > 0 and S > 1, "with a workspace this shape is meant to take the split-KV path"
    got = run_fwd(hip, q8, k8, sq, sk, v8t, sv, n, split)
    assert torch.isfinite(got.float()).all()
    err = (got.double() - ref).abs()
    g_max, g_spiked, g_mean = err.max().item(), err[list(SPIKED_ROWS)].max().item(), err.mean().item()
    print(f"pv8 attention N = {n}, {data}, {'split-KV' if split else 'direct'}: max {g_max:.3e} (recipe {e_max:.3e}), spiked rows "
          f"{g_spiked:.3e} (recipe {e_spiked:.3e}), mean {g_mean:.3e} (recipe {e_mean:.3e})")
    assert g_max <= 2 * e_max + ATTN_FLOOR, f"max {g_max} vs {e_max}"
    assert g_spiked <= 2 * e_spiked + ATTN_FLOOR, f"spiked rows {g_spiked} vs {e_spiked}"
    assert g_mean <= 2 * e_mean + ATTN_FLOOR, f"mean {g_mean} vs {e_mean}"


def test_exact_case_is_exact_in_the_recipe():
    """exact_case under the V half: the one-hot v gives sv = 1 / 448 and v8 = 448 in every live channel, p = 1 gives P8 = c, and
    c 448 sv / (c l) rounds to bf16 1.0 — the emulation equals the selected v row."""
    for n, nkv, must in ((1100, None, ()), (300, 1100, (1099,))):
        q, k, v, want, _ = qk8.exact_case(n, nkv, HEADS, must)
        q8, k8, sq, sk, _, _ = qk8.quant_emu(q, k, HEADS)
        sv, v8, _ = quant_v_emu(v, HEADS)
        assert (sv == torch.tensor(1.0) / 448).all() and set(v8.float().unique().tolist()) == {0.0, 448.0}
        assert torch.equal(attn_pv8_emu(q8, k8, sq, sk, v8, sv, HEADS).to(BF16), want)


@gpu
@pytest.mark.parametrize("n", ATTN_N)
def test_attention_pv8_exact(hip, n):  # noqa: F811
    """All three launches of hip.attention_qk8(pv8=True) on strided q | k | v column slices: the selected v row, bit for bit."""
    q, k, v, want, _ = qk8.exact_case(n)
    d = torch.cat([q, k, v], dim=-1).cuda().unsqueeze(0)
    c = HEADS * 128
    got = hip.attention_qk8(d[..., :c], d[..., c:2 * c], d[..., 2 * c:], HEADS, pv8=True)
    torch.cuda.synchronize()
    bad = (got[0].cpu() != want).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {n} rows differ from the selected v row, first {bad[:8].tolist()}"


@gpu
def test_attention_pv8_exact_last_key_of_a_ragged_tile(hip):  # noqa: F811
    """Nkv != Nq: 300 queries over 1 100 keys, query 0 selects key 1 099, the last key of the ragged last tile (12 of 64 keys live)."""
    nq, nkv = 300, 1100
    q, k, v, want, _ = qk8.exact_case(nq, nkv, HEADS, (nkv - 1,))
    qkv = torch.cat([k, k, v], dim=-1).cuda().unsqueeze(0)      # k | v as column slices of one buffer
    c = HEADS * 128
    qd = q.cuda()
    q8, _, sq, _, _ = hip.attn_quant_qk(qd[None], torch.zeros_like(qd)[None], HEADS)
    _, k8, _, sk, _ = hip.attn_quant_qk(torch.zeros_like(qkv[..., c:2 * c]), qkv[..., c:2 * c], HEADS)
    got = hip.attention_qk8_pre(q8, k8, sq, sk, qkv[..., 2 * c:], HEADS, pv8=True)
    torch.cuda.synchronize()
    assert want[0].view(HEADS, 128).argmax(1).tolist() == [(nkv - 1) % 128] * HEADS
    bad = (got[0].cpu() != want).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {nq} rows differ from the selected v row, first {bad[:8].tolist()}"


@gpu
def test_entry_points_only_enqueue_and_capture(hip):  # noqa: F811
    """Both entry points recorded on a side stream into a graph: nothing runs at capture (the outputs keep their fill), a replay gives
    the bits of the eager call."""
    n, c = 1100, HEADS * 128
    qkv = seeded((1, n, 3 * c), 78).cuda()
    q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    want = hip.attention_qk8(q, k, v, HEADS, pv8=True)
    torch.cuda.synchronize()
    bufs, pv_bufs = hip.attention_qk8_scratch(n, HEADS, 128, q.device), hip.attention_pv8_scratch(n, HEADS, 128, q.device)
    ws, out = [], torch.zeros_like(want)
    need = hip.load().fg_attn_workspace_bytes(1, n, n, HEADS)
    if need > 0:
        ws.append(torch.empty(need, dtype=torch.uint8, device="cuda"))
    pv_bufs[1].fill_(-1.0)
    pv_bufs[0].view(torch.uint8).fill_(0x5A)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        hip.attention_qk8(q, k, v, HEADS, out=out, workspace=ws, bufs=bufs, pv8=True, pv8_bufs=pv_bufs)
    torch.cuda.synchronize()
    assert (out == 0).all() and (pv_bufs[1] == -1.0).all() and (pv_bufs[0].view(torch.uint8) == 0x5A).all(), "a capture launched work"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------------------------ 5. the tiny DiT
@functools.lru_cache(maxsize=None)
def tiny_oracle():
    """(the oracle's fp32 forward, its bf16 forward with self-attention replaced by the emulation of both halves) on the inputs of
    test_tiny_dit_forward; computed once for both of its cases."""
    cfg = synthetic.TINY_DIT_KWARGS
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    lat, ctx, ts = seeded(qk8.LATENT, 11), seeded((1, 16, 128), 12), torch.tensor([995.9]).to(BF16)
    want32 = wan_dit.model_fn({k_: v_.float() for k_, v_ in sd.items()}, cfg, lat.float(), ts.float(), ctx.float(), True)
    bf16_attention = wan_dit.attention

    def emulated(q, k, v, num_heads):
        if q.shape[1] != k.shape[1]:      # cross-attention
            return bf16_attention(q, k, v, num_heads)
        q8, k8, sq, sk, _, _ = qk8.quant_emu(q[0].to(BF16), k[0].to(BF16), num_heads)
        sv, v8, _ = quant_v_emu(v[0].to(BF16), num_heads)
        return attn_pv8_emu(q8, k8, sq, sk, v8, sv, num_heads).to(q.dtype).unsqueeze(0)
    wan_dit.attention = emulated
    try:
        want_emu = wan_dit.model_fn(sd, cfg, lat, ts, ctx, True)
    finally:
        wan_dit.attention = bf16_attention
    return want32, want_emu


@gpu
@pytest.mark.parametrize("fused", [False, True], ids=["two-step", "fused-producers"])
def test_tiny_dit_forward(hip, monkeypatch, fused):  # noqa: F811
    """enable_qk8_attention(pv8=True) on the tiny DiT over 1 200 tokens, behind either producer path: finite, not the e4m3 Q K^T forward,
    and no further from the fp32 oracle, or from the bf16 kernel forward, than 2 d_recipe: d_recipe = 1 - cos(the oracle's bf16 forward
    with its self-attention replaced by the emulation of both halves, the oracle's fp32 forward)."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, sd, cfg = qk8.tiny_model()
    lat, ctx, ts = seeded(qk8.LATENT, 11), seeded((1, 16, 128), 12), torch.tensor([995.9]).to(BF16)
    args = dict(latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    with torch.no_grad():
        out_bf16 = model_fn_wan_video(m, **args)
        out_qk8 = model_fn_wan_video(m.enable_qk8_attention(fused_producer=fused), **args)
        monkeypatch.setattr(hip, "_call", call)
        out_pv8 = model_fn_wan_video(m.enable_qk8_attention(fused_producer=fused, pv8=True), **args)
        monkeypatch.setattr(hip, "_call", real)
        out_back = model_fn_wan_video(m.enable_qk8_attention(False), **args)
    nb = cfg["num_layers"]
    assert calls.count("fg_attn_fwd_pv8_bf16") == nb and calls.count("fg_attn_quant_vt_bf16") == nb and calls.count("fg_attn_fwd_qk8_bf16") == 0
    assert calls.count("fg_attn_quant_qk_bf16") == (0 if fused else nb) and calls.count("fg_attn_quant_k_bf16") == (nb if fused else 0)
    assert calls.count("fg_attn_fwd_bf16") == nb, "cross-attention stays on the bf16 kernel"
    assert torch.isfinite(out_pv8.float()).all()
    assert torch.equal(out_back, out_bf16) and not torch.equal(out_pv8, out_qk8) and not torch.equal(out_pv8, out_bf16), "the switch is dead"

    want32, want_emu = tiny_oracle()
    cos = qk8.cos_distance
    d_recipe = cos(want_emu, want32)
    d_pv8, d_bf16, d_pair = cos(out_pv8, want32), cos(out_bf16, want32), cos(out_pv8, out_bf16)
    print(f"tiny DiT, 1 200 tokens, {'fused' if fused else 'two-step'} producers: 1 - cos to the fp32 oracle: recipe in the bf16 oracle "
          f"{d_recipe:.3e}, pv8 kernels {d_pv8:.3e}, bf16 kernels {d_bf16:.3e}; pv8 kernels to bf16 kernels {d_pair:.3e}, to qk8 kernels "
          f"{cos(out_pv8, out_qk8):.3e}")
    assert d_pv8 <= 2 * d_recipe, (d_pv8, d_recipe)
    assert d_pair <= 2 * d_recipe, (d_pair, d_recipe)


@gpu
def test_graph_loop_equals_eager(hip):  # noqa: F811
    """graph=True on the tiny loop over 1 200 tokens with the mode on: the captured step owns v8t, sv and the statistics scratch next to
    the e4m3 q / k buffers and replays to the bits of the eager loop."""
    from fairygen_amd.wan_video import WanVideoPipeline
    m, _, _ = qk8.tiny_model()
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.enable_qk8_attention(pv8=True)
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
    pipe.dit.enable_qk8_attention()
    assert not torch.equal(loop(False), want), "the loop above ran without the P V half of the mode"

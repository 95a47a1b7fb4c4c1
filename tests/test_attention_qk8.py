"""The opt-in e4m3 Q K^T self-attention (WanModel.enable_qk8_attention, fg_attn_quant_qk_bf16 + fg_attn_fwd_qk8_bf16, include/fairygen_hip.h): the form
the reference's flash_attention takes when the sageattention package is present (models/wan_video_dit.py:48-52).

The recipe is written out below in fp32 / fp64 torch (`quant_emu`, `attn_emu`) and is what the kernels are held to:
  1. (no GPU) the recipe's own properties: dropping kbar leaves the fp64 softmax unchanged, the scales never overflow e4m3, an all-zero
     q row gives a finite result, and few quotients sit within an fp32 ulp of an e4m3 rounding tie;
  2. (no GPU) the ABI: declared, exported, bound; enable_qk8_attention / ModelConfig(attention_dtype=...) set the routing, a token-sharded
     layout raises;
  3. fg_attn_quant_qk_bf16: scales bit for bit, bytes bit for bit outside rounding ties, guard bands untouched;
  4. fg_attn_fwd_qk8_bf16 against the fp64 emulation on the same operands: N(0, 1), peaked rows, spiked keys, with and without split-KV,
     and one case whose result is exact;
  5. the tiny DiT: finite, different from bf16, no further from it than the recipe itself moves the oracle; graph=True == eager.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic
from oracle import wan_dit

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
ATTN_FLOOR = 2e-3            # the floor of tests/test_hip_kernels.py's attention criterion
FLOOR_SCALE = 2.0 ** -20     # the recipe's floor of sq and sk
QUANT_N = (1, 63, 1100)
ATTN_N = (1100, 2049)
HEADS = 2


# ------------------------------------------------------------------------------------------------------------------ the recipe
def quant_emu(q, k, heads):
    """q (Nq, heads*128), k (N, heads*128) bf16 -> q8, k8 e4m3 of those shapes, sq (Nq, heads), sk (heads) fp32, and the fp32 quotients
    that were rounded.  (Nq = N in self-attention; the two halves of the recipe do not meet before the attention kernel.)"""
    nq, n = q.shape[0], k.shape[0]
    qf, kf = q.float().view(nq, heads, 128), k.float().view(n, heads, 128)
    kbar = (k.double().view(n, heads, 128).sum(0) / n).float()               # the fp64 sum, divided by N, rounded once to fp32
    kp = kf - kbar
    sk = torch.clamp(kp.abs().amax((0, 2)) / 448.0, min=FLOOR_SCALE)
    sq = torch.clamp(qf.abs().amax(2) / 448.0, min=FLOOR_SCALE)
    xq, xk = qf / sq.unsqueeze(-1), kp / sk.view(1, heads, 1)
    q8, k8 = xq.clamp(-448, 448).to(F8), xk.clamp(-448, 448).to(F8)           # round-to-nearest-even, saturating
    return q8.view(nq, -1), k8.view(n, -1), sq, sk, xq.view(nq, -1), xk.view(n, -1)


def attn_emu(q8, k8, sq, sk, v, heads, scale=128 ** -0.5):
    """softmax(scale * sq[r] * sk * (q8 k8^T)) v in fp64: (N, heads*128)."""
    nq, nkv = q8.shape[0], k8.shape[0]
    a, b, vv = q8.double().view(nq, heads, 128), k8.double().view(nkv, heads, 128), v.double().view(nkv, heads, 128)
    out = torch.empty((nq, heads, 128), dtype=torch.float64)
    for h in range(heads):
        s = (a[:, h] @ b[:, h].T) * (scale * sq[:, h].double().unsqueeze(1) * sk[h].double())
        out[:, h] = torch.softmax(s, dim=-1) @ vv[:, h]
    return out.view(nq, -1)


E4M3_VALUES = torch.arange(256, dtype=torch.uint8).view(F8).float()
E4M3_VALUES = torch.unique(E4M3_VALUES[torch.isfinite(E4M3_VALUES)])         # sorted, -448 .. 448


def near_tie(x):
    """Elements of the fp32 tensor x (|x| <= 448 up to rounding) that lie within one fp32 ulp of the midpoint of two adjacent e4m3 values."""
    x = x.clamp(-448, 448)
    hi = torch.bucketize(x, E4M3_VALUES).clamp(1, E4M3_VALUES.numel() - 1)
    mid = (E4M3_VALUES[hi - 1] + E4M3_VALUES[hi]) / 2
    ulp = torch.nextafter(x.abs(), torch.full_like(x, float("inf"))) - x.abs()
    return (x - mid).abs() <= ulp


@functools.lru_cache(maxsize=None)
def quant_case(n, heads=HEADS):
    """q | k | v column slices of one (n, 3*H*128) row-major buffer, as the qkv GEMM leaves them."""
    qkv = seeded((n, 3 * heads * 128), 900 + n + 1000 * (heads - HEADS))
    c = heads * 128
    return qkv, quant_emu(qkv[:, :c], qkv[:, c:2 * c], heads)


# ------------------------------------------------------------------------------------------------------------------ 1. the recipe's properties
def test_recipe_kbar_leaves_softmax_unchanged():
    q, k = seeded((77, 128), 1).double(), (seeded((90, 128), 2).double() + 3.0)
    s = q @ k.T * 128 ** -0.5
    s_smooth = q @ (k - k.mean(0)).T * 128 ** -0.5
    assert (torch.softmax(s, -1) - torch.softmax(s_smooth, -1)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("n", QUANT_N)
def test_recipe_scales_never_overflow(n):
    _, (q8, k8, sq, sk, xq, xk) = quant_case(n)
    assert torch.isfinite(q8.float()).all() and torch.isfinite(k8.float()).all()
    assert q8.float().abs().max() <= 448 and k8.float().abs().max() <= 448
    # the quotients themselves stay within one rounding of 448: the clamp of the recipe never moves a value by more than that
    assert xq.abs().max() <= 448 * (1 + 2.0 ** -22) and xk.abs().max() <= 448 * (1 + 2.0 ** -22)
    assert (sq >= FLOOR_SCALE).all() and (sk >= FLOOR_SCALE).all()
    # every row of q reaches the top of the range (its own maximum maps to +-448), and so does every head of k
    assert (q8.float().view(n, HEADS, 128).abs().amax(2) == 448).all()
    assert n == 1 or (k8.float().view(n, HEADS, 128).abs().amax((0, 2)) == 448).all()      # one key: k' = 0


def test_recipe_zero_rows_are_finite():
    q, k, v = seeded((70, 256), 3), seeded((70, 256), 4), seeded((70, 256), 5)
    q[7] = 0
    q8, k8, sq, sk, _, _ = quant_emu(q, k, 2)
    assert (sq[7] == FLOOR_SCALE).all() and (q8[7].float() == 0).all()
    out = attn_emu(q8, k8, sq, sk, v, 2)
    assert torch.isfinite(out).all()
    assert torch.allclose(out[7].view(2, 128), v.double().view(70, 2, 128).mean(0), atol=1e-12), "a zero query row attends uniformly"
    # all keys equal: k' = 0 exactly, sk sits at its floor, no 0 / 0
    k[:] = k[0]
    q8, k8, sq, sk, _, _ = quant_emu(q, k, 2)
    assert (sk == FLOOR_SCALE).all() and (k8.float() == 0).all() and torch.isfinite(attn_emu(q8, k8, sq, sk, v, 2)).all()


def test_recipe_tie_exemption_is_rare():
    """The GPU test lets a byte differ from the emulation where the quotient lies within one fp32 ulp of a rounding tie, for at most 0.1 %
    of the elements.  What uses that exemption is an evaluation whose quotient is one ulp off, so the emulation is held to it alone: the
    same recipe with the quotient formed as x * (1 / s) — within an ulp of x / s, the difference the exemption is for — must differ from
    the emulation only at such ties and in fewer than 0.1 % of the elements.  Measured on these seeds (bytes that differ / elements):
    N = 1: 0 / 512; N = 63: 16 / 32 256 (0.050 %); N = 1 100: 149 / 563 200 (0.026 %).  The quotients that lie within an ulp of a tie
    at all are more (0, 107 and 1 509: bf16 inputs over a bf16 maximum / 448 hit ties exactly, e.g. every 16th element of a row whose
    maximum is 448 * 2^k / 128); IEEE division rounds those the same way everywhere, and the GPU run reports how many bytes differed."""
    for n in QUANT_N:
        check_tie_exemption(n)


def check_tie_exemption(n, heads=HEADS):
    """test_recipe_tie_exemption_is_rare for one quant_case; returns the bytes that differ."""
    qkv, (q8, k8, sq, sk, xq, xk) = quant_case(n, heads)
    c = heads * 128
    qf = qkv[:, :c].float().view(n, heads, 128)
    kp = qkv[:, c:2 * c].float().view(n, heads, 128) - (qkv[:, c:2 * c].double().view(n, heads, 128).sum(0) / n).float()
    alt_q = (qf * (1.0 / sq).unsqueeze(-1)).clamp(-448, 448).to(F8).view(n, -1)
    alt_k = (kp * (1.0 / sk).view(1, heads, 1)).clamp(-448, 448).to(F8).view(n, -1)
    used = 0
    for alt, w8, x in ((alt_q, q8, xq), (alt_k, k8, xk)):
        diff = alt.view(torch.uint8) != w8.view(torch.uint8)
        assert not (diff & ~near_tie(x)).any(), "a one-ulp change of the quotient moved a byte away from a tie"
        used += diff.sum().item()
    near = near_tie(xq).sum().item() + near_tie(xk).sum().item()
    print(f"N = {n}, {heads} heads: {used} of {xq.numel() + xk.numel()} bytes differ under x * (1 / s); {near} quotients within one ulp of "
          f"an e4m3 tie")
    assert used < 1e-3 * (xq.numel() + xk.numel())
    return used


# ------------------------------------------------------------------------------------------------------------------ 2. the ABI and the switch
NAMES = ("fg_attn_quant_qk_bf16", "fg_attn_fwd_qk8_bf16")


def test_abi_declared_exported_bound():
    lib = _hip.load()
    header = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    assert lib.fg_version() == _hip.ABI_VERSION and _hip.QK8_ABI_VERSION == 1 and lib.fg_attn_qk8_version() == 1
    assert "version of this extension, currently 1" in header
    # the entry points and their version function: declared in the header, each exactly once, and in EXPORTED_SYMBOLS
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", header, re.M)
    for name in NAMES + ("fg_attn_qk8_version",):
        assert declared.count(name) == 1 and name in _hip.EXPORTED_SYMBOLS, name
    assert re.search(r"^int fg_attn_quant_qk_bf16\(const void\* q, int64_t ldq, const void\* k, int64_t ldk, void\* q8, void\* k8, float\* sq, "
                     r"float\* sk,\s*void\* scratch, int64_t scratch_bytes, int64_t N, int H, int D, fg_stream_t stream\);", header, re.M)
    assert re.search(r"^int fg_attn_fwd_qk8_bf16\(const void\* q8, const void\* k8, const float\* sq, const float\* sk, const void\* v, int64_t ldv, "
                     r"void\* out,\s*int64_t Nq, int64_t Nkv, int H, int D, float scale, void\* workspace, int64_t workspace_bytes,\s*"
                     r"fg_stream_t stream\);", header, re.M)
    assert "models/wan_video_dit.py:48-52" in header
    V, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert {n: _hip._SIGNATURES[n] for n in NAMES} == {NAMES[0]: [V, I64, V, I64, V, V, V, V, V, I64, I64, I32, I32, V],
                                                       NAMES[1]: [V, V, V, V, V, I64, V, I64, I64, I32, I32, F, V, I64, V]}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _hip._SIGNATURES[name]
    assert hasattr(raw, "fg_attn_qk8_version") and "fg_attn_qk8_version" in _hip._QUERIES


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1)."""
    lib, a = _hip.load(), 4096
    assert lib.fg_attn_quant_qk_bf16(a, 256, a, 256, a, a, a, a, a, 1024, 10, 2, 64, None) == -1 and b"head_dim 128" in lib.fg_last_error()
    assert lib.fg_attn_quant_qk_bf16(a, 255, a, 256, a, a, a, a, a, 1024, 10, 2, 128, None) == -1      # ldq < H*D
    assert lib.fg_attn_quant_qk_bf16(a, 256, a, 256, a, a, a, a, a, 1023, 10, 2, 128, None) == -1 and b"scratch" in lib.fg_last_error()
    assert lib.fg_attn_quant_qk_bf16(a, 256, a, 256, a + 4, a, a, a, a, 1024, 10, 2, 128, None) == -1  # q8 not 8-byte aligned
    assert lib.fg_attn_quant_qk_bf16(a, 256, None, 256, a, a, a, a, a, 1024, 10, 2, 128, None) == -1
    assert lib.fg_attn_fwd_qk8_bf16(a, a, a, a, a, 256, a, 10, 10, 2, 64, 0.1, None, 0, None) == -1
    assert lib.fg_attn_fwd_qk8_bf16(a, a, a, a, a, 248, a, 10, 10, 2, 128, 0.1, None, 0, None) == -1   # ldv < H*D
    assert lib.fg_attn_fwd_qk8_bf16(a, a, a, a, a, 256, a, 10, 10, 2, 128, 0.0, None, 0, None) == -1   # scale
    assert lib.fg_attn_fwd_qk8_bf16(a + 8, a, a, a, a, 256, a, 10, 10, 2, 128, 0.1, None, 0, None) == -1
    assert lib.fg_attn_fwd_qk8_bf16(a, a, a, a, a, 256, a, 10, 10, 2, 128, 0.1, None, 64, None) == -1   # workspace bytes without a workspace


def test_enable_sets_the_routing():
    from fairygen_amd.wan_video_dit import QK8_MIN_KV, AttentionModule, WanModel
    with torch.device("meta"):
        m = WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.qk8_attention is False and m.attn_scale() == _hip.pow2_softmax_scale(128)
    assert m.enable_qk8_attention() is m and m.qk8_attention is True
    assert m.attn_scale() == (128 ** -0.5, 1.0), "q takes the unfolded RoPE table and attention 1/sqrt(d)"
    assert QK8_MIN_KV == 1024 and all(type(b.self_attn.attn) is AttentionModule for b in m.blocks)
    m.enable_qk8_attention(False)
    assert m.qk8_attention is False and m.attn_scale() == _hip.pow2_softmax_scale(128)


def test_sharded_layout_raises():
    from fairygen_amd.wan_video_dit import WanModel
    with torch.device("meta"):
        m = WanModel(**synthetic.TINY_DIT_KWARGS)

    class Shard:
        active = True
    m.check_qk8_layout(Shard())      # mode off: any layout
    m.enable_qk8_attention()
    m.check_qk8_layout(None)
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.check_qk8_layout(Shard())
    x = torch.empty((1, 8, 256), device="meta")
    with pytest.raises(NotImplementedError, match="token-sharded"):
        next(m.forward_tokens_steps(x, x, torch.empty((1, 6, 256), device="meta"), x, 0, (x, x), Shard(), 16))


def test_model_config_attention_dtype():
    from fairygen_amd import ModelConfig
    from fairygen_amd.loader import ModelPool
    assert ModelConfig(path="x").vram_config()["attention_dtype"] is None
    assert ModelConfig(path="x", attention_dtype=F8).vram_config()["attention_dtype"] == F8
    src = open(os.path.join(REPO, "fairygen_amd", "loader.py")).read()
    assert "model.enable_qk8_attention()" in src and ModelPool is not None


def test_model_config_other_dtypes_raise(tmp_path):
    """ModelConfig(attention_dtype=...) through ModelPool on a saved tiny DiT: e4m3 switches the mode on, other dtypes raise."""
    from fairygen_amd import loader
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        base = {"computation_dtype": BF16, "computation_device": "cpu"}
        pool = loader.ModelPool()
        pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8))
        assert pool.model[0].qk8_attention is True
        pool.auto_load_model(path, vram_config=base)
        assert pool.model[1].qk8_attention is False
        for bad in (torch.float8_e5m2, torch.float8_e4m3fnuz, torch.int8):
            with pytest.raises(NotImplementedError, match="attention_dtype"):
                loader.ModelPool().auto_load_model(path, vram_config=dict(base, attention_dtype=bad))
    finally:
        loader.MODEL_CONFIGS.remove(entry)


# ------------------------------------------------------------------------------------------------------------------ 3. fg_attn_quant_qk_bf16
@pytest.fixture(scope="module")
def hip():
    _hip.load()
    assert torch.cuda.is_available()
    return _hip


POISON = 0x5A


def guarded(shape, dtype, fill=POISON):
    """A tensor of `shape` between two guard rows of one larger buffer, every byte of which is `fill`."""
    rows = shape[0] + 2
    full = torch.full((rows,) + tuple(shape[1:]), fill, dtype=torch.uint8, device="cuda") if dtype in (F8, torch.uint8) else None
    if full is None:
        size = torch.empty((), dtype=dtype).element_size()
        full = torch.full((rows,) + tuple(shape[1:-1]) + (shape[-1] * size,), fill, dtype=torch.uint8, device="cuda")
    return full, full[1:-1].view(dtype)


def guards_intact(full):
    return bool((full[0] == POISON).all() and (full[-1] == POISON).all())


@gpu
@pytest.mark.parametrize("n", QUANT_N)
def test_quant_qk_against_the_recipe(hip, n):
    check_quant_qk(hip, n)


def check_quant_qk(hip, n, heads=HEADS):
    """fg_attn_quant_qk_bf16 on quant_case(n, heads) against quant_emu; returns the bytes that used the tie exemption."""
    qkv, (q8, k8, sq, sk, xq, xk) = quant_case(n, heads)
    c = heads * 128
    # the rows live between guard rows of NaN, and the v slice (inside the leading dimension, never read) is NaN too
    src = torch.full((n + 2, 3 * c), float("nan"), dtype=BF16)
    src[1:-1, :2 * c] = qkv[:, :2 * c]
    d = src.cuda()[1:-1].unsqueeze(0)
    fulls, bufs = zip(*[guarded(s, t) for s, t in (((n, c), F8), ((n, c), F8), ((n, heads), torch.float32), ((1, heads), torch.float32),
                                                   ((1, c), torch.float32))])
    bufs = (bufs[0], bufs[1], bufs[2], bufs[3].view(heads), bufs[4].view(c))
    got = hip.attn_quant_qk(d[..., :c], d[..., c:2 * c], heads, bufs)
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in fulls), "a guard row of an output was written"
    g_q8, g_k8, g_sq, g_sk = (t.cpu() for t in got[:4])
    assert torch.equal(g_sq, sq), f"sq: {(g_sq != sq).sum().item()} of {sq.numel()} differ"
    assert torch.equal(g_sk, sk), f"sk: {g_sk.tolist()} != {sk.tolist()}"
    kbar = (qkv[:, c:2 * c].double().sum(0) / n).float()
    assert torch.equal(got[4].cpu(), kbar), "the column means in the scratch"
    exempt = 0
    for name, g8, w8, x in (("q8", g_q8, q8, xq), ("k8", g_k8, k8, xk)):
        diff = g8.view(torch.uint8) != w8.view(torch.uint8)
        tie = near_tie(x)
        print(f"N = {n}, {heads} heads, {name}: {diff.sum().item()} bytes differ, {tie.sum().item()} quotients within one ulp of a tie")
        assert not (diff & ~tie).any(), f"{name}: {(diff & ~tie).sum().item()} bytes differ away from a rounding tie"
        # a byte that differs at a tie is the other neighbour, not anything else
        assert (g8.float()[diff] - w8.float()[diff]).abs().le((x[diff].abs() / 8).clamp(min=2.0 ** -9)).all()
        exempt += diff.sum().item()
    assert exempt <= 1e-3 * 2 * n * c, f"{exempt} of {2 * n * c} elements used the tie exemption"
    return exempt


# ------------------------------------------------------------------------------------------------------------------ 4. fg_attn_fwd_qk8_bf16
def _spiked_keys(q, k, picks):      # tests/test_hip_kernels.py::_spiked_keys for 2-D tensors
    k = k.clone()
    for i, (pos, row) in enumerate(picks):
        k[pos] = (q[row].float() * (1.5 + i)).to(BF16)
    return k


@functools.lru_cache(maxsize=None)
def attn_case(n, data):
    """Inputs of test_attention_w4_deferred_rescale at Nq = Nkv = n: N(0, 1), peaked rows (q x 8), keys that move the running max by far
    more than 2^6 in the first, a middle, the last full and the ragged tile.  The operands are the recipe's; the reference is fp64."""
    c = HEADS * 128
    q, k, v = seeded((n, c), 130, scale=8.0 if "peaked" in data else 1.0), seeded((n, c), 131), seeded((n, c), 132)
    if "spiked" in data:
        last_full = (n // 64) * 64 - 3
        k = _spiked_keys(q, k, [(70, 5), (n // 3, 17), (n // 2, 150), (last_full, 255), (n - 2, 299), (n - 1, 5)])
    q8, k8, sq, sk, _, _ = quant_emu(q, k, HEADS)
    ref = attn_emu(q8, k8, sq, sk, v, HEADS)
    err_ref = (ref.to(BF16).double() - ref).abs().max().item()
    return q8, k8, sq, sk, v, ref, err_ref


def split_choice(hip, n, ws_bytes):
    R, S = ctypes.c_int(), ctypes.c_int()
    assert hip.load().fg_attn_split_choice(1, n, n, HEADS, ws_bytes, ctypes.byref(R), ctypes.byref(S)) == 0
    return R.value, S.value


def run_fwd(hip, q8, k8, sq, sk, v, n, split):
    lib = hip.load()
    need = lib.fg_attn_workspace_bytes(1, n, n, HEADS) if split else 0
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, HEADS * 128), dtype=BF16, device="cuda")
    ops = [t.cuda().contiguous() for t in (q8, k8, sq, sk, v)]
    hip._call("fg_attn_fwd_qk8_bf16", *[hip._ptr(t) for t in ops[:4]], hip._ptr(ops[4]), HEADS * 128, hip._ptr(out), n, n, HEADS, 128,
              128 ** -0.5, hip._ptr(ws) if need > 0 else None, need, hip._stream(out))
    torch.cuda.synchronize()
    return out.cpu()


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["direct", "split-kv"])
@pytest.mark.parametrize("data", ["normal", "peaked", "spiked", "peaked+spiked"])
@pytest.mark.parametrize("n", ATTN_N)
def test_attention_qk8_against_the_recipe(hip, n, data, split):
    """max|hip - emu_f64| <= 2 max|bf16(emu) - emu_f64| + floor, the emulation on the same q8, k8 and scales with an fp64 softmax and the
    bf16 v; the spiked rows once more on their own, so that a wrong rescale cannot hide in a maximum elsewhere."""
    q8, k8, sq, sk, v, ref, err_ref = attn_case(n, data)
    if split:
        R, S = split_choice(hip, n, hip.load().fg_attn_workspace_bytes(1, n, n, HEADS))
        assert R > 0 and S > 1, "with a workspace this shape is meant to take the split-KV path"
    got = run_fwd(hip, q8, k8, sq, sk, v, n, split)
    assert torch.isfinite(got.float()).all()
    err = (got.double() - ref).abs().max().item()
    print(f"qk8 attention N = {n}, {data}, {'split-KV' if split else 'direct'}: err {err:.3e}, bf16(emu) err {err_ref:.3e}")
    assert err <= 2 * err_ref + ATTN_FLOOR, f"err {err} vs {err_ref}"
    for row in (5, 17, 150, 255, 299):
        e = (got[row].double() - ref[row]).abs().max().item()
        assert e <= 2 * err_ref + ATTN_FLOOR, f"row {row}: {e}"


@functools.lru_cache(maxsize=None)
def exact_case(n, nkv=None, heads=HEADS, must=()):
    """Small-integer q and k and one-hot v for which every step of the recipe and of the kernel is exact.  Keys are +-4 in every channel
    and come in (k, -k) pairs (an odd n ends on a zero row), so every column sums to 0: kbar = 0, sk = 4 / 448 and k8 = +-448 exactly.
    Query r is 16 x sign(key sel(r)): sq = 16 / 448, q8 = +-448.  Every score is 448^2 x an integer below 2^15 — exact in fp32 in any
    summation order.  The logit of the selected key is 16 * 4 * 128 / sqrt(128) = 724 nats; the gap to every other key is asserted
    to be > 150 nats, so every other probability underflows to 0 in fp32 and out[r] = v[sel(r)] = e_(sel(r) mod 128), exactly.
    nkv: the number of keys where it is not n (the n queries then draw from them); must: keys that queries 0, 1, .. select in every head
    whatever the draw — when the last key of an odd nkv is among them, the zero row is key nkv // 2 instead."""
    nkv = n if nkv is None else nkv
    g = torch.Generator("cpu").manual_seed(8000 + n + (0 if nkv == n else 3 * nkv))
    half = nkv // 2
    signs = (torch.randint(0, 2, (half, heads, 128), generator=g) * 2 - 1).float()
    zero = nkv - 1 if nkv - 1 not in must else nkv // 2                  # of an odd nkv
    assert nkv % 2 == 0 or zero not in must
    rows = torch.tensor([i for i in range(nkv) if nkv % 2 == 0 or i != zero])
    k = torch.zeros((nkv, heads, 128))
    k[rows[0::2]], k[rows[1::2]] = 4 * signs, -4 * signs
    live = 2 * half                                                      # the zero row of an odd n is selected by nobody
    sel = torch.stack([rows[torch.randperm(live, generator=g)[torch.arange(n) % live]] for _ in range(heads)], 1)      # (n, H)
    for i, key in enumerate(must):
        sel[i] = key
    q = 4 * k[sel, torch.arange(heads)]                                  # 16 x sign
    v = torch.zeros((nkv, heads, 128))
    v[torch.arange(nkv), :, torch.arange(nkv) % 128] = 1.0
    want = v[sel, torch.arange(heads)]
    gap = float("inf")
    for h in range(heads):
        logits = (q[:, h].double() @ k[:, h].double().T) * 128 ** -0.5
        top = logits.gather(1, sel[:, h:h + 1])
        assert (top == 16 * 4 * 128 * 128 ** -0.5).all()
        gap = min(gap, (top - logits.scatter(1, sel[:, h:h + 1], float("-inf")).amax(1, keepdim=True)).min().item())
    return q.view(n, -1).to(BF16), k.view(nkv, -1).to(BF16), v.view(nkv, -1).to(BF16), want.view(n, -1).to(BF16), gap


@pytest.mark.parametrize("n", ATTN_N)
def test_exact_case_construction(n):
    check_exact_case(n)


def check_exact_case(n, nkv=None, heads=HEADS, must=()):
    """The conditions exact_case rests on, for one of its cases (nkv None: n keys, the zero row of an odd n the last)."""
    q, k, v, want, gap = exact_case(n, nkv, heads, must)
    nkv = n if nkv is None else nkv
    print(f"exact case Nq = {n}, Nkv = {nkv}, {heads} heads: smallest logit gap {gap:.1f} nats")
    assert gap > 150
    q8, k8, sq, sk, _, _ = quant_emu(q, k, heads)
    assert (sk == 4 / 448).all() and (sq == 16 / 448).all() and (q8.float().abs() == 448).all()
    zero = [] if nkv % 2 == 0 else [nkv - 1 if nkv - 1 not in must else nkv // 2]
    live = [i for i in range(nkv) if i not in zero]
    assert (k8.float().abs()[live] == 448).all() and (k8.float()[zero] == 0).all()
    emu = attn_emu(q8, k8, sq, sk, v, heads)      # fp64 does not underflow where fp32 does: e^-150 is what is left of the other keys
    assert torch.equal(emu.to(BF16), want) and (emu - want.double()).abs().max().item() < 1e-60
    for i, key in enumerate(must):                # the keys a case names are selected, in every head
        assert (want[i].view(heads, 128).argmax(1) == key % 128).all() and (want[i].view(heads, 128).sum(1) == 1).all()


@gpu
@pytest.mark.parametrize("n", ATTN_N)
def test_attention_qk8_exact(hip, n):
    """Both launches of hip.attention_qk8 on strided q | k | v column slices: the result is the index expectation bit for bit."""
    q, k, v, want, _ = exact_case(n)
    d = torch.cat([q, k, v], dim=-1).cuda().unsqueeze(0)
    c = HEADS * 128
    got = hip.attention_qk8(d[..., :c], d[..., c:2 * c], d[..., 2 * c:], HEADS)
    torch.cuda.synchronize()
    bad = (got[0].cpu() != want).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {n} rows differ from the selected v row, first {bad[:8].tolist()}"


@gpu
def test_entry_points_only_enqueue_and_capture(hip):
    """Both entry points recorded on a side stream into a graph: nothing runs at capture (the outputs keep their fill), a replay gives
    the bits of the eager call."""
    n, c = 1100, HEADS * 128
    qkv = seeded((1, n, 3 * c), 77).cuda()
    q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    want = hip.attention_qk8(q, k, v, HEADS)
    torch.cuda.synchronize()
    bufs, ws, out = hip.attention_qk8_scratch(n, HEADS, 128, q.device), [], torch.zeros_like(want)
    need = hip.load().fg_attn_workspace_bytes(1, n, n, HEADS)
    if need > 0:
        ws.append(torch.empty(need, dtype=torch.uint8, device="cuda"))
    bufs[2].fill_(-1.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        hip.attention_qk8(q, k, v, HEADS, out=out, workspace=ws, bufs=bufs)
    torch.cuda.synchronize()
    assert (out == 0).all() and (bufs[2] == -1.0).all(), "a capture launched work"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------------------------ 5. the tiny DiT
LATENT = (1, 48, 3, 40, 40)      # 3 x 20 x 20 = 1 200 tokens: above QK8_MIN_KV, so the tiny model's self-attention takes the new kernel


def cos_distance(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return 1.0 - (a @ b / (a.norm() * b.norm())).item()


def tiny_model():
    from fairygen_amd.wan_video_dit import WanModel
    cfg = synthetic.TINY_DIT_KWARGS
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    m = WanModel(**cfg)
    m.load_state_dict(sd)
    return m.to(device="cuda", dtype=BF16).eval(), sd, cfg


@gpu
def test_tiny_dit_forward(hip, monkeypatch):
    """enable_qk8_attention() on the tiny DiT over 1 200 tokens: finite, not the bf16 forward, and close to it.  How close is measured, not
    chosen: d_recipe = 1 - cos(the oracle's bf16 forward with its self-attention replaced by the emulation above, the oracle's fp32
    forward) is how far the recipe, inside the oracle's own bf16 arithmetic, sits from fp32.  The kernel path may sit no further from
    fp32 than 2 d_recipe, and no further than that from the bf16 kernel forward either."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, sd, cfg = tiny_model()
    lat, ctx, ts = seeded(LATENT, 11), seeded((1, 16, 128), 12), torch.tensor([995.9]).to(BF16)
    args = dict(latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    with torch.no_grad():
        out_bf16 = model_fn_wan_video(m, **args)
        monkeypatch.setattr(hip, "_call", call)
        out_qk8 = model_fn_wan_video(m.enable_qk8_attention(), **args)
        monkeypatch.setattr(hip, "_call", real)
        out_back = model_fn_wan_video(m.enable_qk8_attention(False), **args)
    nb = cfg["num_layers"]
    assert calls.count("fg_attn_fwd_qk8_bf16") == nb and calls.count("fg_attn_quant_qk_bf16") == nb
    assert calls.count("fg_attn_fwd_bf16") == nb, "cross-attention stays on the bf16 kernel"
    assert torch.isfinite(out_qk8.float()).all()
    assert torch.equal(out_back, out_bf16) and not torch.equal(out_qk8, out_bf16), "the switch is dead"

    want32 = wan_dit.model_fn({k_: v_.float() for k_, v_ in sd.items()}, cfg, lat.float(), ts.float(), ctx.float(), True)
    bf16_attention = wan_dit.attention

    def emulated(q, k, v, num_heads):
        if q.shape[1] != k.shape[1]:      # cross-attention
            return bf16_attention(q, k, v, num_heads)
        q8, k8, sq, sk, _, _ = quant_emu(q[0].to(BF16), k[0].to(BF16), num_heads)
        return attn_emu(q8, k8, sq, sk, v[0].to(BF16), num_heads).to(q.dtype).unsqueeze(0)
    monkeypatch.setattr(wan_dit, "attention", emulated)
    want_emu = wan_dit.model_fn(sd, cfg, lat, ts, ctx, True)
    monkeypatch.setattr(wan_dit, "attention", bf16_attention)
    d_recipe = cos_distance(want_emu, want32)
    d_qk8, d_bf16, d_pair = cos_distance(out_qk8, want32), cos_distance(out_bf16, want32), cos_distance(out_qk8, out_bf16)
    print(f"tiny DiT, 1 200 tokens: 1 - cos to the fp32 oracle: recipe in the bf16 oracle {d_recipe:.3e}, qk8 kernels {d_qk8:.3e}, "
          f"bf16 kernels {d_bf16:.3e}; qk8 kernels to bf16 kernels {d_pair:.3e}")
    assert d_qk8 <= 2 * d_recipe, (d_qk8, d_recipe)
    assert d_pair <= 2 * d_recipe, (d_pair, d_recipe)


@gpu
def test_graph_loop_equals_eager(hip):
    """graph=True on the tiny loop over 1 200 tokens with the mode on: the captured step owns the quantised operands' buffers and
    replays to the bits of the eager loop."""
    from fairygen_amd.wan_video import WanVideoPipeline
    m, _, _ = tiny_model()
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.enable_qk8_attention()
    lat, ctx_p, ctx_n = seeded(LATENT, 21), seeded((1, 16, 128), 22), seeded((1, 16, 128), 23)
    z0 = seeded(LATENT[:2] + (1,) + LATENT[3:], 24)

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
    pipe.dit.enable_qk8_attention(False)
    assert not torch.equal(loop(False), want), "the loop above ran without the mode"

"""The opt-in mean-smoothed V of the e4m3 P V self-attention (WanModel.enable_qk8_attention(pv8=True, smooth_v=True),
fg_attn_quant_vt_smooth_bf16 + fg_attn_fwd_pv8s_bf16 and their batched forms, include/fairygen_hip_smoothv.h): what the reference's
sageattn package ships as smooth_v.

The recipe (DESIGN §5 "e4m3 P V with smoothed V") is written out below (`quant_vs_emu`, `attn_pv8s_emu`) on top of the two halves
tests/test_attention_qk8.py and tests/test_attention_pv8.py hold:
  1. the ABI: the extension header, the binding's tables, the exported symbols, the version;
  2. the producer against the emulation — mu and sv bit for bit, v8t byte for byte with NO tie exemption, padding zero — twice into
     poisoned buffers between guard rows, at every Nkv of QUANT_N and at 2 049;
  3. an input whose correct result is exact: v[j][c] = m_c for all keys gives mu = m_c, v8t = 0, sv = the floor, and out = m_c bit for bit
     on the direct path, the split-KV path and per element of a batch (what fg_attn_fwd_pv8_bf16 makes of it is printed, not asserted);
  4. accuracy, neither yardstick being the code under test: (a) the bound of test_attention_pv8_against_the_recipe against the emulation
     of THIS recipe; (b) on V with per-channel offsets the mean |error| below that of fg_attn_fwd_pv8_bf16 on the same tensors;
  5. the batched forms per element against the single-element entry points, with batch strides that leave gaps;
  6. the argument checks, the stream-only and capture checks.
The model level is tests/test_smoothv_forward.py.

Measured on the MI355X (2 heads).  The producer: 0 bytes, 0 scales and 0 means differ from the emulation at every N.  Offset V, peaked
rows, mean |gpu - ref|: N = 1 100 direct 1.095e-1 (fg_attn_fwd_pv8_bf16) against 1.762e-2 (smoothed), ratio 6.21; N = 2 049 split-KV
1.049e-1 against 1.710e-2, ratio 6.13 (the fp64 emulations: 7.47 and 7.49).  Constant V through fg_attn_fwd_pv8_bf16 at N = 2 049, direct:
max |out - m_c| 6.25e-2 with 2.5 % of the elements off on normal rows, 3.13e-1 (4.3 % of |m_c|) with 41 % off on peaked rows; the
smoothed form: 0.  Yardstick (a), N = 2 049 direct, max / mean against the emulation's: normal 1.02e-2, 1.09e-3 against 1.04e-2, 1.07e-3;
peaked 2.04e-1, 1.46e-2 against 1.55e-1, 1.43e-2; spiked 1.29e-1, 4.41e-3 against 1.24e-1, 4.42e-3; peaked+spiked 1.52e-1, 1.79e-2 against
1.36e-1, 1.78e-2.  The 36 GPU tests of this file take about 4 s of pytest time.
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
from test_attention_qk8 import ATTN_FLOOR, FLOOR_SCALE, guarded, guards_intact, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float32
HEADS = qk8.HEADS
C = HEADS * 128
QUANT_N = (1, 63, 64, 65, 1100, 2049)
ATTN_N = qk8.ATTN_N            # 1 100 (direct) and 2 049 (with the workspace the planner cuts KV ranges)
NAMES = ("fg_attn_quant_vt_smooth_bf16", "fg_attn_quant_vt_smooth_bf16_b", "fg_attn_fwd_pv8s_bf16", "fg_attn_fwd_pv8s_bf16_b")
QUERIES = ("fg_attn_smoothv_version", "fg_attn_smoothv_scratch_bytes")


# ------------------------------------------------------------------------------------------------------------------ the recipe
def ordered_sum(v64):
    """The fp64 sum over the rows of v64 (N, C) in the order include/fairygen_hip_smoothv.h states: parts = min(ceil(N / 16), 256) row
    strides, stride p = (w0 + w1) + (w2 + w3) with w_i the rows 4 p + i + 4 parts n added in that order, then the even strides added
    in order plus the odd strides added in order."""
    n = v64.shape[0]
    parts = min((n + 15) // 16, 256)
    rec = torch.zeros((parts, v64.shape[1]), dtype=torch.float64)
    for p in range(parts):
        w = []
        for i in range(4):
            s = torch.zeros(v64.shape[1], dtype=torch.float64)
            for r in range(4 * p + i, n, 4 * parts):
                s = s + v64[r]
            w.append(s)
        rec[p] = (w[0] + w[1]) + (w[2] + w[3])
    halves = []
    for g in range(2):
        s = torch.zeros(v64.shape[1], dtype=torch.float64)
        for p in range(g, parts, 2):
            s = s + rec[p]
        halves.append(s)
    return halves[0] + halves[1]


def quant_vs_emu(v, heads):
    """v (N, heads*128) bf16 -> mu, sv (heads, 128) fp32 and v8 (N, heads*128) e4m3: the mean from the fp64 sum, rounded once to fp32;
    d = fl32(v - mu); sv = max(max |d| / 448, 2^-20) with the maximum taken over d itself (the library takes it from the minimum and
    maximum of v); v8 = e4m3(fl32(d / sv)), round-to-nearest-even."""
    n = v.shape[0]
    mu = (ordered_sum(v.double()) / n).float()
    d = v.float() - mu
    sv = torch.clamp(d.abs().amax(0) / 448.0, min=FLOOR_SCALE)
    x = d / sv
    return mu.view(heads, 128), sv.view(heads, 128), x.clamp(-448, 448).to(F8)


def attn_pv8s_emu(q8, k8, sq, sk, v8, sv, mu, heads):
    """The recipe in fp64: that of the e4m3 P V form on the centred v8, plus the key mean."""
    return pv8.attn_pv8_emu(q8, k8, sq, sk, v8, sv, heads) + mu.double().view(1, -1)


def offset_v(n, seed=140):
    """V as trained projections leave it: per channel an offset mu_c ~ 8 N(0, 1) under a spread eps ~ N(0, 1)."""
    return (seeded((n, C), seed, dtype=F32) + 8.0 * seeded((1, C), seed + 1, dtype=F32)).to(BF16)


@functools.lru_cache(maxsize=None)
def quant_case(n):
    """The v of tests/test_attention_pv8.py's producer test at n keys with a per-channel offset added (so that mu is not ~0), and its
    emulation."""
    v = offset_v(n, 900 + n)
    return v, quant_vs_emu(v, HEADS)


# ------------------------------------------------------------------------------------------------------------------ 1. the ABI
def test_extension_abi():
    """Fails on the parent commit: the symbols, the header and the binding's tables are this extension's."""
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_smoothv.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55      # the main table is what it was
    tables = (_hip.PV8_SYMBOLS, _hip.SHARD8_SYMBOLS, _hip.CROSS8_SYMBOLS, _hip.BATCH8_SYMBOLS, _hip.ROWBATCH_SYMBOLS, _hip.ROWBATCH8_SYMBOLS,
              _hip.LORABATCH_SYMBOLS, _hip.UP2PHASE_SYMBOLS, _hip.GATEGEMM_SYMBOLS)
    assert [len(t) for t in tables] == [4, 6, 3, 9, 5, 3, 3, 4, 3]
    others = _hip.EXPORTED_SYMBOLS + [s for t in tables for s in t]
    assert not any(name in others for name in NAMES + QUERIES)
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_smoothv.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.SMOOTHV_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 6
    assert _hip.SMOOTHV_ABI_VERSION == 1 and lib.fg_attn_smoothv_version() == 1
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has the arguments of its declaration, and the attention entry points those of the pv8 ones plus mu behind sv
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
             "fg_stream_t": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    args = {}
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        args[name] = [a.split() for a in decl.split(",")]
        want = [kinds[" ".join(a[:-1])] for a in args[name]]
        assert want == _hip._SMOOTHV_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is ctypes.c_int
    for name, base, width in ((NAMES[0], _hip._PV8_SIGNATURES["fg_attn_quant_vt_bf16"], 1),
                              (NAMES[1], _hip._BATCH8_SIGNATURES["fg_attn_quant_vt_bf16_b"], 2),
                              (NAMES[2], _hip._PV8_SIGNATURES["fg_attn_fwd_pv8_bf16"], 1),
                              (NAMES[3], _hip._BATCH8_SIGNATURES["fg_attn_fwd_pv8_bf16_b"], 2)):
        at = [a[-1] for a in args[name]].index("mu")
        assert args[name][at - width][-1] == "sv" and " ".join(args[name][at][:-1]) in ("float*", "const float*"), name
        sig = _hip._SMOOTHV_SIGNATURES[name]
        assert sig[:at] + sig[at + width:] == list(base), name
    assert _hip._SMOOTHV_QUERIES == {QUERIES[0]: (ctypes.c_int, []), QUERIES[1]: (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int])}
    assert "smooth_v" in ext and "2^-20" in ext
    real = _hip._lib
    try:          # load() checks the version: a library that answers another one is refused
        _hip._lib = None
        _hip.SMOOTHV_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="ABI mismatch"):
            _hip.load()
    finally:
        _hip.SMOOTHV_ABI_VERSION = 1
        _hip._lib = real


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1), and fg_last_error names the argument."""
    lib, a = _hip.load(), 4096
    err = lib.fg_last_error
    assert lib.fg_attn_smoothv_scratch_bytes(1100, 2) == 69 * 256 * 16 and lib.fg_attn_smoothv_scratch_bytes(10 ** 6, 24) == 256 * 24 * 128 * 16
    assert lib.fg_attn_smoothv_scratch_bytes(0, 2) == -1 and lib.fg_attn_smoothv_scratch_bytes(5, 0) == -1
    need = lib.fg_attn_smoothv_scratch_bytes(10, 2)
    quant = lib.fg_attn_quant_vt_smooth_bf16
    assert quant(a, 256, a, a, None, a, need, 10, 2, 128, None) == -1 and b"mu" in err()
    assert quant(a, 256, a, a, a + 8, a, need, 10, 2, 128, None) == -1 and b"mu" in err()
    assert quant(a, 256, a, a, a, a, need - 1, 10, 2, 128, None) == -1 and b"scratch" in err()
    assert quant(a, 256, a, a, a, a, need, 10, 2, 64, None) == -1 and b"head_dim 128" in err()
    assert quant(a, 255, a, a, a, a, need, 10, 2, 128, None) == -1 and b"ldv" in err()
    assert quant(a, 256, a + 8, a, a, a, need, 10, 2, 128, None) == -1 and b"aligned" in err()
    assert quant(a, 256, a, None, a, a, need, 10, 2, 128, None) == -1 and b"null" in err()

    def quant_b(mu=a, bs_mu=256, sb=need, bs_s=need, d=128, b=2):
        return lib.fg_attn_quant_vt_smooth_bf16_b(a, 256, 10 * 256, a, 256 * 64, a, 256, mu, bs_mu, a, sb, bs_s, b, 10, 2, d, None)
    assert quant_b(mu=None) == -1 and b"mu" in err()
    assert quant_b(mu=a + 4) == -1 and b"mu" in err()
    assert quant_b(sb=need - 16) == -1 and b"scratch" in err()
    assert quant_b(d=64) == -1 and b"head_dim 128" in err()
    assert quant_b(bs_mu=255) == -1 and b"batch stride" in err()
    assert quant_b(bs_mu=258) == -1 and b"mu" in err()
    assert quant_b(bs_s=need - 16) == -1 and b"batch stride" in err()
    assert quant_b(b=0) == -1 and b"B must be" in err()

    def fwd(mu=a, d=128, scale=0.1, v8t=a, nkv=10, ws=0):
        return lib.fg_attn_fwd_pv8s_bf16(a, a, a, a, v8t, a, mu, a, 10, nkv, 2, d, scale, None, ws, None)
    assert fwd(mu=None) == -1 and b"mu" in err()
    assert fwd(mu=a + 8) == -1 and b"mu" in err()
    assert fwd(d=64) == -1 and b"head_dim 128" in err()
    assert fwd(scale=0.0) == -1 and b"scale" in err()
    assert fwd(v8t=a + 8) == -1 and b"aligned" in err()
    assert fwd(ws=64) == -1 and b"workspace" in err()
    assert fwd(nkv=1 << 25) == -1 and b"4 GiB" in err()

    def fwd_b(mu=a, bs_mu=256, d=128, b=2):
        return lib.fg_attn_fwd_pv8s_bf16_b(a, 10 * 256, a, 10 * 256, a, 20, a, 2, a, 256 * 64, a, 256, mu, bs_mu, a, 10 * 256, b, 10, 10, 2, d,
                                           0.1, None, 0, None)
    assert fwd_b(mu=None) == -1 and b"mu" in err()
    assert fwd_b(mu=a + 12) == -1 and b"mu" in err()
    assert fwd_b(d=64) == -1 and b"head_dim 128" in err()
    assert fwd_b(bs_mu=128) == -1 and b"batch stride" in err()
    assert fwd_b(bs_mu=257) == -1 and b"mu" in err()
    assert fwd_b(b=0) == -1 and b"B must be" in err()


def test_binding_refuses_mismatched_buffers():
    """The host wrappers decide on shapes alone, before any pointer is read."""
    v = torch.empty((1, 10, C), dtype=BF16, device="meta")
    three = tuple(torch.empty(s, dtype=t, device="meta") for s, t in (((HEADS, 128, 64), F8), ((HEADS, 128), F32), ((64,), torch.uint8)))
    with pytest.raises(_hip.HipLibraryError, match="smooth=True"):
        _hip.attn_quant_vt(v, HEADS, three, smooth=True)
    with pytest.raises(_hip.HipLibraryError, match="smooth=False"):
        _hip.attn_quant_vt(v, HEADS, three + (three[1],))
    with pytest.raises(_hip.HipLibraryError, match="pv8=True"):
        _hip.attention_qk8_pre(None, None, None, None, v, HEADS, smooth=True)
    with pytest.raises(_hip.HipLibraryError, match="mu must be"):
        _hip.attention_pv8_pre(None, None, None, None, three[0], three[1], HEADS, mu=torch.empty((HEADS, 64), dtype=F32, device="meta"))


# ------------------------------------------------------------------------------------------------------------------ the recipe's properties
def test_recipe_ordered_sum_is_the_sum_and_constant_channels_are_exact():
    """On bf16 data of a few binades the fp64 sum is exact, so the stated order gives THE sum; and a channel that is the same for all keys
    has mu = that value, d = 0 and the floor as its scale."""
    for n in (1, 63, 65, 1100):
        v = offset_v(n, 50 + n)
        assert torch.equal(ordered_sum(v.double()), v.double().sum(0)), n
    m = seeded((1, C), 7, scale=3.0)
    mu, sv, v8 = quant_vs_emu(m.expand(300, C).contiguous(), HEADS)
    assert torch.equal(mu.view(1, C), m.float()) and (sv == FLOOR_SCALE).all() and (v8.view(torch.uint8) == 0).all()


def test_recipes_separate_on_offset_v():
    """Yardstick (b) before any device is involved: on V with per-channel offsets (offset_v: mu_c ~ 8 N(0, 1), eps ~ N(0, 1)) and peaked
    rows the two recipes, both emulated in fp64, separate by a clear factor — mean |pv8 emulation - ref| is 7.47 x (N = 1 100: 1.087e-1
    against 1.456e-2) and 7.49 x (N = 2 049: 1.080e-1 against 1.442e-2) mean |smoothed emulation - ref| (printed below; asserted here as at least 3 x).  That is what makes "smaller" in
    test_offset_v_error_is_below_pv8 a statement about the recipe and not about noise."""
    for n in ATTN_N:
        q8, k8, sq, sk, v, ref, e_pv8, e_s = offset_case(n)[:8]
        print(f"offset V, peaked rows, N = {n}: mean |emulation - ref| pv8 {e_pv8:.3e}, smoothed {e_s:.3e}, ratio {e_pv8 / e_s:.2f}")
        assert e_pv8 >= 3 * e_s


@functools.lru_cache(maxsize=None)
def offset_case(n):
    """(q8, k8, sq, sk, v, ref, mean error of the pv8 emulation, of the smoothed emulation): peaked rows over offset_v."""
    q, k = seeded((n, C), 130, scale=8.0), seeded((n, C), 131)
    v = offset_v(n)
    q8, k8, sq, sk, _, _ = qk8.quant_emu(q, k, HEADS)
    ref = qk8.attn_emu(q8, k8, sq, sk, v, HEADS)
    sv0, v80, _ = pv8.quant_v_emu(v, HEADS)
    e_pv8 = (pv8.attn_pv8_emu(q8, k8, sq, sk, v80, sv0, HEADS) - ref).abs().mean().item()
    mu, sv, v8 = quant_vs_emu(v, HEADS)
    e_s = (attn_pv8s_emu(q8, k8, sq, sk, v8, sv, mu, HEADS) - ref).abs().mean().item()
    return q8, k8, sq, sk, v, ref, e_pv8, e_s


# ------------------------------------------------------------------------------------------------------------------ 2. the producer
def run_quant(hip, v, n):  # noqa: F811
    """fg_attn_quant_vt_smooth_bf16 on v (n, C) as the v column slice of a q | k | v buffer between NaN guard rows, into poisoned outputs
    between guard rows: (v8t bytes, sv, mu) on the host."""
    src = torch.full((n + 2, 3 * C), float("nan"), dtype=BF16)
    src[1:-1, 2 * C:] = v
    d = src.cuda()[1:-1].unsqueeze(0)
    nkp = (n + 63) // 64 * 64
    need = hip.load().fg_attn_smoothv_scratch_bytes(n, HEADS)
    fulls, bufs = zip(*[guarded(s, t) for s, t in (((HEADS, 128, nkp), F8), ((HEADS, 128), F32), ((1, need), torch.uint8), ((HEADS, 128), F32))])
    got = hip.attn_quant_vt(d[..., 2 * C:], HEADS, (bufs[0], bufs[1], bufs[2].view(need), bufs[3]), smooth=True)
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in fulls), "a guard row of an output was written"
    return got[0].cpu().view(torch.uint8), got[1].cpu(), got[3].cpu()


@gpu
@pytest.mark.parametrize("n", QUANT_N)
def test_quant_vt_smooth_against_the_recipe(hip, n):  # noqa: F811
    v, (mu, sv, v8) = quant_case(n)
    first = run_quant(hip, v, n)
    g_t, g_sv, g_mu = first
    assert torch.equal(g_mu, mu), f"mu: {(g_mu != mu).sum().item()} of {mu.numel()} differ"
    assert torch.equal(g_sv, sv), f"sv: {(g_sv != sv).sum().item()} of {sv.numel()} differ"
    g8, pad = pv8.from_tiles(g_t, n)
    assert (pad == 0).all(), f"{(pad != 0).sum().item()} of {pad.numel()} padding bytes are not zero"
    diff = g8 != v8.view(torch.uint8)
    assert not diff.any(), f"N = {n}: {diff.sum().item()} of {diff.numel()} bytes differ from the emulation"
    again = run_quant(hip, v, n)
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "a second run into fresh poisoned buffers wrote other bytes"


# ------------------------------------------------------------------------------------------------------------------ 3. exact
def quantise(hip, q, k, v, smooth):  # noqa: F811
    """The library's own operands of q, k, v (n, C) bf16 on the host: (q8, k8, sq, sk, v8t, sv[, mu]) on the device."""
    qd, kd, vd = (t.cuda().unsqueeze(0) for t in (q, k, v))
    q8, k8, sq, sk, _ = hip.attn_quant_qk(qd, kd, HEADS)
    v8t, sv, _, *mu = hip.attn_quant_vt(vd, HEADS, smooth=smooth)
    return (q8, k8, sq, sk, v8t, sv) + tuple(mu)


def workspace(hip, n, split, batch=1):  # noqa: F811
    """The caller's workspace list of the wrappers for the split-KV plan of n keys (they size one themselves when it is empty)."""
    need = batch * hip.load().fg_attn_workspace_bytes(1, n, n, HEADS) if split else 0
    if split:
        R, S = qk8.split_choice(hip, n, need // batch)
        assert R > 0 and S > 1, "with a workspace this shape is meant to take the split-KV path"
    return [torch.empty(need, dtype=torch.uint8, device="cuda")] if need > 0 else []


def run_fwd(hip, ops, n, split):  # noqa: F811
    """fg_attn_fwd_pv8s_bf16 on (q8, k8, sq, sk, v8t, sv, mu) — fg_attn_fwd_pv8_bf16 without mu — straight through the C ABI: with the
    workspace of the split-KV plan, or with none (every q-block one workgroup over all keys).  (n, C) bf16 on the device."""
    ws = workspace(hip, n, split)
    out = torch.empty((n, C), dtype=BF16, device="cuda")
    dev = [t.cuda().contiguous() for t in ops]
    hip._call("fg_attn_fwd_pv8s_bf16" if len(ops) == 7 else "fg_attn_fwd_pv8_bf16", *[hip._ptr(t) for t in dev], hip._ptr(out), n, n, HEADS, 128,
              128 ** -0.5, hip._ptr(ws[0]) if ws else None, ws[0].numel() if ws else 0, hip._stream(out))
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("peak", [1.0, 8.0], ids=["normal", "peaked"])
@pytest.mark.parametrize("n,split", [(1100, False), (2049, False), (2049, True)], ids=["1100-direct", "2049-direct", "2049-split-kv"])
def test_constant_v_is_exact(hip, n, split, peak):  # noqa: F811
    """v[j][c] = m_c for all keys: softmax . m_c is m_c, and the smoothed form returns it bit for bit — mu = m_c, every byte of v8t zero,
    sv the floor, acc = 0, out = bf16(0 + m_c).  fg_attn_fwd_pv8_bf16 on the same input carries m_c times the rounding defect of its P
    row; what it makes of it is printed for DESIGN.md and not asserted (that kernel is unchanged)."""
    q, k = seeded((n, C), 150, scale=peak), seeded((n, C), 151)
    m = seeded((1, C), 152, scale=3.0)
    v = m.expand(n, C).contiguous()
    ops = quantise(hip, q, k, v, True)
    assert torch.equal(ops[6].cpu().view(1, C), m.float()) and (ops[4].view(torch.uint8) == 0).all() and (ops[5] == FLOOR_SCALE).all()
    got = run_fwd(hip, ops, n, split)
    bad = (got.cpu() != m).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {n} rows differ from m_c, first {bad[:8].tolist()}"
    plain = run_fwd(hip, quantise(hip, q, k, v, False), n, split)
    e = (plain.cpu().float() - m.float()).abs()
    print(f"constant V, N = {n}, {'split-KV' if split else 'direct'}, q x {peak:g}: fg_attn_fwd_pv8_bf16 max |out - m_c| = {e.max().item():.3e}, "
          f"mean {e.mean().item():.3e}, {(e != 0).float().mean().item():.1%} of the elements off; relative to |m_c| max "
          f"{(e / m.float().abs().clamp(min=1e-30)).max().item():.3e}; the smoothed form: 0")


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["direct", "split-kv"])
def test_constant_v_is_exact_per_batch_element(hip, split):  # noqa: F811
    """The same through the batched entry points, B = 2, every element with its own m_c."""
    n = 2049
    q, k = seeded((2, n, C), 160, scale=8.0).cuda(), seeded((2, n, C), 161).cuda()
    m = seeded((2, 1, C), 162, scale=3.0)
    v = m.expand(2, n, C).contiguous().cuda()
    q8, k8, sq, sk, _ = hip.attn_quant_qk(q, k, HEADS)
    v8t, sv, _, mu = hip.attn_quant_vt(v, HEADS, smooth=True)
    ws = workspace(hip, n, split, 2)
    got = torch.empty((2, n, C), dtype=BF16, device="cuda")
    hip._call("fg_attn_fwd_pv8s_bf16_b", hip._ptr(q8), n * C, hip._ptr(k8), n * C, hip._ptr(sq), n * HEADS, hip._ptr(sk), HEADS, hip._ptr(v8t),
              v8t.stride(0), hip._ptr(sv), C, hip._ptr(mu), C, hip._ptr(got), n * C, 2, n, n, HEADS, 128, 128 ** -0.5,
              hip._ptr(ws[0]) if ws else None, ws[0].numel() if ws else 0, hip._stream(got))
    torch.cuda.synchronize()
    assert torch.equal(mu.cpu().view(2, 1, C), m.float()) and (v8t.view(torch.uint8) == 0).all()
    for e in range(2):
        bad = (got[e].cpu() != m[e]).any(-1).nonzero().flatten()
        assert bad.numel() == 0, f"element {e}: {bad.numel()} of {n} rows differ from m_c, first {bad[:8].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ 4. accuracy
@functools.lru_cache(maxsize=None)
def attn_case(n, data):
    """tests/test_attention_pv8.py's attn_case under this recipe: the operands, the yardstick ref (fp64 softmax . V of the dequantised
    qk8 operands with the bf16 v) and the emulation's own distance from it (max, spiked rows, mean)."""
    q8, k8, sq, sk, v, ref, _ = qk8.attn_case(n, data)
    mu, sv, v8 = quant_vs_emu(v, HEADS)
    e = (attn_pv8s_emu(q8, k8, sq, sk, v8, sv, mu, HEADS) - ref).abs()
    return q8, k8, sq, sk, pv8.to_tiles(v8, HEADS), sv, mu, ref, (e.max().item(), e[list(pv8.SPIKED_ROWS)].max().item(), e.mean().item())


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["direct", "split-kv"])
@pytest.mark.parametrize("data", ["normal", "peaked", "spiked", "peaked+spiked"])
@pytest.mark.parametrize("n", ATTN_N)
def test_attention_pv8s_against_the_recipe(hip, n, data, split):  # noqa: F811
    """Yardstick (a), the bound of test_attention_pv8_against_the_recipe: max and mean |gpu - ref| <= 2 x the same statistic of the fp64
    emulation of the recipe + 2e-3, for all rows and for the spiked rows alone."""
    q8, k8, sq, sk, v8t, sv, mu, ref, (e_max, e_spiked, e_mean) = attn_case(n, data)
    got = run_fwd(hip, (q8, k8, sq, sk, v8t.view(F8), sv, mu), n, split).cpu()
    assert torch.isfinite(got.float()).all()
    err = (got.double() - ref).abs()
    g_max, g_spiked, g_mean = err.max().item(), err[list(pv8.SPIKED_ROWS)].max().item(), err.mean().item()
    print(f"smoothed pv8 attention N = {n}, {data}, {'split-KV' if split else 'direct'}: max {g_max:.3e} (recipe {e_max:.3e}), spiked rows "
          f"{g_spiked:.3e} (recipe {e_spiked:.3e}), mean {g_mean:.3e} (recipe {e_mean:.3e})")
    assert g_max <= 2 * e_max + ATTN_FLOOR, f"max {g_max} vs {e_max}"
    assert g_spiked <= 2 * e_spiked + ATTN_FLOOR, f"spiked rows {g_spiked} vs {e_spiked}"
    assert g_mean <= 2 * e_mean + ATTN_FLOOR, f"mean {g_mean} vs {e_mean}"


@gpu
@pytest.mark.parametrize("n,split", [(1100, False), (2049, True)], ids=["1100-direct", "2049-split-kv"])
def test_offset_v_error_is_below_pv8(hip, n, split):  # noqa: F811
    """Yardstick (b): on offset_case (the recipes themselves separate there by 7.5 x: test_recipes_separate_on_offset_v) the mean
    |error| of fg_attn_fwd_pv8s_bf16 is below that of fg_attn_fwd_pv8_bf16 on the same tensors, both on the library's own operands."""
    q8, k8, sq, sk, v, ref, e_pv8, e_s = offset_case(n)
    vd = v.cuda().unsqueeze(0)
    outs = {}
    for smooth in (False, True):
        v8t, sv, _, *mu = hip.attn_quant_vt(vd, HEADS, smooth=smooth)
        got = run_fwd(hip, (q8, k8, sq, sk, v8t, sv) + tuple(mu), n, split)
        outs[smooth] = (got.cpu().double() - ref).abs().mean().item()
    print(f"offset V, peaked rows, N = {n}, {'split-KV' if split else 'direct'}: mean |gpu - ref| pv8 {outs[False]:.3e} (recipe {e_pv8:.3e}), "
          f"smoothed {outs[True]:.3e} (recipe {e_s:.3e}), ratio {outs[False] / outs[True]:.2f}")
    assert outs[True] < outs[False]


# ------------------------------------------------------------------------------------------------------------------ 5. the batched forms
def spread(shape, dtype, gap):
    """(B, ...) whose elements lie `gap` elements further apart than they are long, every byte poisoned: (the strided view, the buffer)."""
    one = 1
    for s in shape[1:]:
        one *= s
    full = torch.full((shape[0], one + gap), qk8.POISON, dtype=torch.uint8, device="cuda") if dtype in (F8, torch.uint8) else \
        torch.full((shape[0], one + gap), float("nan"), dtype=dtype, device="cuda")
    return full[:, :one].view(dtype).view(shape), full


@gpu
@pytest.mark.parametrize("n", [65, 2049])
def test_batched_forms_equal_single_calls(hip, n):  # noqa: F811
    """fg_attn_quant_vt_smooth_bf16_b and fg_attn_fwd_pv8s_bf16_b (B = 2, every batch stride with a gap, v a column slice of a wider
    buffer) per element against the single-element entry points on that element alone: torch.equal, with and without a workspace."""
    b, nkp, lib = 2, (n + 63) // 64 * 64, hip.load()
    qkv = torch.stack([torch.cat([seeded((n, C), 170 + e, scale=8.0), seeded((n, C), 172 + e), offset_v(n, 174 + 2 * e)], dim=-1) for e in range(b)])
    wide = torch.full((b, n + 3, 3 * C), float("nan"), dtype=BF16, device="cuda")
    wide[:, :n] = qkv.cuda()
    v = wide[:, :n, 2 * C:]
    need = lib.fg_attn_smoothv_scratch_bytes(n, HEADS)
    (v8t, _), (sv, _), (mu, _), (scr, _) = spread((b, HEADS, 128, nkp), F8, 64), spread((b, HEADS, 128), F32, 12), \
        spread((b, HEADS, 128), F32, 4), spread((b, need), torch.uint8, 48)
    hip._call("fg_attn_quant_vt_smooth_bf16_b", hip._ptr(v), 3 * C, v.stride(0), hip._ptr(v8t), v8t.stride(0), hip._ptr(sv), sv.stride(0),
              hip._ptr(mu), mu.stride(0), hip._ptr(scr), need, scr.stride(0), b, n, HEADS, 128, hip._stream(v))
    torch.cuda.synchronize()
    singles = [hip.attn_quant_vt(v[e:e + 1], HEADS, smooth=True) for e in range(b)]
    for e in range(b):
        one = singles[e]
        assert torch.equal(v8t[e].view(torch.uint8), one[0].view(torch.uint8)) and torch.equal(sv[e], one[1]) and torch.equal(mu[e], one[3]), e

    q8, k8, sq, sk = (torch.stack(t) for t in zip(*[hip.attn_quant_qk(wide[e:e + 1, :n, :C], wide[e:e + 1, :n, C:2 * C], HEADS)[:4]
                                                    for e in range(b)]))
    (q8s, _), (k8s, _), (sqs, _), (sks, _), (out, _) = spread((b, n, C), F8, 32), spread((b, n, C), F8, 16), spread((b, n, HEADS), F32, 3), \
        spread((b, HEADS), F32, 5), spread((b, n, C), BF16, 8)
    for dst, src in ((q8s, q8), (k8s, k8), (sqs, sq), (sks, sk)):
        dst.view(torch.uint8 if dst.dtype == F8 else dst.dtype).copy_(src.view(torch.uint8 if src.dtype == F8 else src.dtype))
    for split in (False, True):
        share = lib.fg_attn_workspace_bytes(1, n, n, HEADS) if split else 0
        ws = torch.empty(max(b * share, 16), dtype=torch.uint8, device="cuda")
        out.fill_(float("nan"))
        hip._call("fg_attn_fwd_pv8s_bf16_b", hip._ptr(q8s), q8s.stride(0), hip._ptr(k8s), k8s.stride(0), hip._ptr(sqs), sqs.stride(0),
                  hip._ptr(sks), sks.stride(0), hip._ptr(v8t), v8t.stride(0), hip._ptr(sv), sv.stride(0), hip._ptr(mu), mu.stride(0),
                  hip._ptr(out), out.stride(0), b, n, n, HEADS, 128, 128 ** -0.5, hip._ptr(ws) if share > 0 else None, b * share,
                  hip._stream(out))
        torch.cuda.synchronize()
        for e in range(b):
            one = singles[e]
            want = run_fwd(hip, (q8[e], k8[e], sq[e], sk[e], one[0], one[1], one[3]), n, split and share > 0)
            assert torch.isfinite(want.float()).all()
            assert torch.equal(out[e], want), (split, e, (out[e] != want).sum().item())
    # and the wrappers pick the batched forms by the leading dimension (they take a batch stride of N rows)
    d = qkv.cuda()
    got = hip.attention_qk8(d[..., :C], d[..., C:2 * C], d[..., 2 * C:], HEADS, pv8=True, smooth=True)
    for e in range(b):
        one = d[e:e + 1]
        assert torch.equal(got[e], hip.attention_qk8(one[..., :C], one[..., C:2 * C], one[..., 2 * C:], HEADS, pv8=True, smooth=True)[0])


# ------------------------------------------------------------------------------------------------------------------ 6. stream and capture
@gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_entry_points_only_enqueue_and_capture(hip, batch):  # noqa: F811
    """The entry points (batch 2: their _b forms) recorded on a side stream into a graph: nothing runs at capture (the outputs keep their
    fill), a replay gives the bits of the eager call — and a second replay the same."""
    n = 2049
    qkv = torch.cat([seeded((batch, n, 2 * C), 78), offset_v(batch * n, 79).view(batch, n, C)], dim=-1).cuda()
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    want = hip.attention_qk8(q, k, v, HEADS, pv8=True, smooth=True)
    torch.cuda.synchronize()
    bufs = hip.attention_qk8_scratch(n, HEADS, 128, q.device, batch)
    pv_bufs = hip.attention_pv8_scratch(n, HEADS, 128, q.device, batch, smooth=True)
    ws, out = workspace(hip, n, True, batch), torch.zeros_like(want)      # (the eager call above sized its own: the same plan)
    pv_bufs[1].fill_(-1.0)
    pv_bufs[3].fill_(-2.0)
    pv_bufs[0].view(torch.uint8).fill_(0x5A)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        hip.attention_qk8(q, k, v, HEADS, out=out, workspace=ws, bufs=bufs, pv8=True, pv8_bufs=pv_bufs, smooth=True)
    torch.cuda.synchronize()
    assert (out == 0).all() and (pv_bufs[1] == -1.0).all() and (pv_bufs[3] == -2.0).all() and (pv_bufs[0].view(torch.uint8) == 0x5A).all(), \
        "a capture launched work"
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)

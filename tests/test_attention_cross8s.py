"""The opt-in mean-smoothed V of the e4m3 cross-attention (WanModel.enable_qk8_attention(pv8=True, cross=True, smooth_v_cross=True),
fg_attn_fwd_cross8s_bf16 and its batched form, include/fairygen_hip_cross8s.h): the kernel of tests/test_attention_cross8.py on the
operands of the smoothing V producer of tests/test_attention_smoothv.py, with the key mean added where an output row is rounded.

The parity criterion is exact, as in tests/test_attention_cross8.py: on the same operands the output must be BIT FOR BIT that of
fg_attn_fwd_pv8s_bf16 launched without a workspace (hip.attention_pv8_pre(..., workspace=None, mu=mu)), the kernel that
tests/test_attention_smoothv.py pins to the fp64 emulation of the recipe.
  1. (no GPU) the extension's ABI and the argument checks; the recipes, emulated in fp64, on a padded context;
  2. the kernel against fg_attn_fwd_pv8s_bf16 with torch.equal: every (Nq, Nkv) edge of the cross8 test, one walk shape, three kinds of data;
  3. a V that is the same for all keys comes back bit for bit, and fg_attn_fwd_cross8_bf16 does not return it;
  4. the batched form per element against the single-element entry point;
  5. accuracy on a padded context: the device error of the two kernels against the separation of the two emulated recipes;
  6. guard bands around every operand, refused arguments, stream and capture.
The model level is tests/test_cross8s_forward.py.

The padded context (padded_context_v: 512 keys, L_text = 40 rows ~ N(0, 1), 472 rows that are one common row ~ 4 N(0, 1); peaked query
rows, 3 heads, Nq = 300).  The two recipes emulated in fp64, mean |emulation - ref|: 2.139e-2 (pv8) against 9.669e-3 (smoothed), ratio
2.21 (above the 2 below which the criterion would say nothing, so L_text stays at 40), and the criterion of
test_padded_context_error_falls asks the device for at least 1.11 x.  The factor is this small because a peaked row puts most of its
weight on a few keys, and where those are text rows the error is that of e4m3 on v - mu, whose range (|text - pad|) is no smaller than
that of v.  Measured on the MI355X: mean |gpu - ref| 1.950e-2 (fg_attn_fwd_cross8_bf16) against 8.690e-3 (fg_attn_fwd_cross8s_bf16), device
factor 2.24.  Constant V, peaked rows, through fg_attn_fwd_cross8_bf16: max |out - m_c| 1.875e-1 at 77 and at 512 keys, 33.0 % and
33.7 % of the elements off, up to 2.9 % of |m_c|; the smoothed form: 0.  The 37 GPU tests of this file take about 3 s of pytest time.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import test_attention_pv8 as pv8
import test_attention_qk8 as qk8
import test_attention_smoothv as smv
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from test_attention_cross8 import BAND, MAX_KV, banded
from test_attention_qk8 import guarded, guards_intact, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8, U8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.float32
NAMES = ("fg_attn_fwd_cross8s_bf16", "fg_attn_fwd_cross8s_bf16_b")
QUERIES = ("fg_attn_cross8s_version",)
DATA = ("normal", "peaked", "padded")
# (heads, Nq, Nkv): the edges of tests/test_attention_cross8.py — one row and one key, a ragged query block, one tile and one past it, a
# ragged last tile, the DiT's 512 keys, the LDS limit with few rows and, one tile short and ragged, with many
SHAPES = [(3, 1, 1), (3, 31, 5), (3, 256, 64), (3, 257, 65), (3, 300, 77), (3, 513, 512), (3, 70, MAX_KV), (3, 1300, MAX_KV - 63)]
WALK = (24, 5157, 512)      # G = 10 on 256 CUs: every workgroup walks three query blocks, the last of the walk ragged
L_TEXT, L_CTX, ACC_HEADS, ACC_NQ = 40, 512, 3, 300


def padded_context_v(l_text, l=512, heads=ACC_HEADS, seed=180):
    """V of a text context as the pipeline leaves it (the context rows behind the prompt are zeroed and the v Linear acts row by row):
    l_text rows ~ N(0, 1), the other l - l_text rows ONE common row ~ 4 N(0, 1) per channel.  (l, heads * 128) bf16.  The generator
    of tools/attn_ab.py --cross8 --smooth-v-cross."""
    c = heads * 128
    pad = (4.0 * seeded((1, c), seed + 1, dtype=F32)).to(BF16)
    return torch.cat([seeded((l_text, c), seed), pad.expand(l - l_text, c)], dim=0).contiguous()


# ------------------------------------------------------------------------------------------------------------------ 1. the ABI
def test_extension_abi():
    """Fails on the parent commit: the symbols, the header and the binding's tables are this extension's."""
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_cross8s.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55      # the main table is what it was
    tables = (_hip.PV8_SYMBOLS, _hip.SHARD8_SYMBOLS, _hip.CROSS8_SYMBOLS, _hip.BATCH8_SYMBOLS, _hip.ROWBATCH_SYMBOLS, _hip.ROWBATCH8_SYMBOLS,
              _hip.LORABATCH_SYMBOLS, _hip.UP2PHASE_SYMBOLS, _hip.GATEGEMM_SYMBOLS, _hip.SMOOTHV_SYMBOLS)
    assert [len(t) for t in tables] == [4, 6, 3, 9, 5, 3, 3, 4, 3, 6]
    others = _hip.EXPORTED_SYMBOLS + [s for t in tables for s in t]
    assert not any(name in others for name in NAMES + QUERIES)
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_cross8s.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert not any(s in ext for s in others), "the header refers to other extensions by file name"
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.CROSS8S_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 3
    assert _hip.CROSS8S_ABI_VERSION == 1 and lib.fg_attn_cross8s_version() == 1
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has the arguments of its declaration, and those are the cross8 ones plus mu (and bs_mu) behind sv (and bs_sv)
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "fg_stream_t": ctypes.c_void_p,
             "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    args = {}
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        args[name] = [a.split() for a in decl.split(",")]
        want = [kinds[" ".join(a[:-1])] for a in args[name]]
        assert want == _hip._CROSS8S_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is ctypes.c_int
    for name, base, width in ((NAMES[0], _hip._CROSS8_SIGNATURES["fg_attn_fwd_cross8_bf16"], 1),
                              (NAMES[1], _hip._BATCH8_SIGNATURES["fg_attn_fwd_cross8_bf16_b"], 2)):
        at = [a[-1] for a in args[name]].index("mu")
        assert args[name][at - width][-1] == "sv" and " ".join(args[name][at][:-1]) == "const float*", name
        if width == 2:
            assert [a[-1] for a in args[name]][at - 1:at + 2] == ["bs_sv", "mu", "bs_mu"]
        sig = _hip._CROSS8S_SIGNATURES[name]
        assert sig[:at] + sig[at + width:] == list(base), name
    assert _hip._CROSS8S_QUERIES == {QUERIES[0]: (ctypes.c_int, [])}
    assert "smooth_v" in ext and "BIT FOR BIT" in ext and "fairygen_hip_smoothv.h" in ext and "hipFuncSetAttribute" in ext
    real = _hip._lib
    try:          # load() checks the version: a library that answers another one is refused
        _hip._lib = None
        _hip.CROSS8S_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="ABI mismatch"):
            _hip.load()
    finally:
        _hip.CROSS8S_ABI_VERSION = 1
        _hip._lib = real


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1): the checks of the unsmoothed entry points,
    plus mu non-null and 16-byte aligned, bs_mu a multiple of 4 and at least one element."""
    lib, a = _hip.load(), 4096
    err = lib.fg_last_error

    def fwd(mu=a, d=128, scale=0.1, nq=10, nkv=10, h=2, ptrs=None):
        p = ptrs or [a] * 6
        return lib.fg_attn_fwd_cross8s_bf16(*p[:6], mu, a, nq, nkv, h, d, scale, None)
    assert fwd(mu=None) == -1 and b"mu" in err()
    for off in (4, 8, 12):
        assert fwd(mu=a + off) == -1 and b"mu" in err()
    assert fwd(d=64) == -1 and b"head_dim 128" in err()
    assert fwd(nkv=MAX_KV + 1) == -1 and b"Nkv must be in 1..640" in err()
    assert fwd(nkv=0) == -1 and b"Nkv" in err()
    assert fwd(nq=0) == -1 and fwd(h=0) == -1
    assert fwd(scale=0.0) == -1 and b"scale" in err()
    assert fwd(nq=1 << 24) == -1 and b"4 GiB" in err()
    for i, off in ((0, 8), (1, 8), (4, 8), (5, 8), (2, 2), (3, 2)):      # q8, k8, v8t, sv: 16-byte aligned; sq, sk: 4
        p = [a] * 6
        p[i] = a + off
        assert fwd(ptrs=p) == -1 and b"aligned" in err(), i
    for i in range(6):
        p = [a] * 6
        p[i] = None
        assert fwd(ptrs=p) == -1 and b"null" in err(), i
    assert lib.fg_attn_fwd_cross8s_bf16(a, a, a, a, a, a, a, None, 10, 10, 2, 128, 0.1, None) == -1 and b"null" in err()
    assert lib.fg_attn_fwd_cross8s_bf16(a, a, a, a, a, a, a, a + 8, 10, 10, 2, 128, 0.1, None) == -1 and b"aligned" in err()

    def fwd_b(mu=a, bs_mu=256, d=128, b=2, nkv=10, bs_sv=256):
        return lib.fg_attn_fwd_cross8s_bf16_b(a, 10 * 256, a, 10 * 256, a, 20, a, 2, a, 256 * 64, a, bs_sv, mu, bs_mu, a, 10 * 256, b, 10, nkv, 2,
                                              d, 0.1, None)
    assert fwd_b(mu=None) == -1 and b"mu" in err()
    assert fwd_b(mu=a + 12) == -1 and b"mu" in err()
    assert fwd_b(d=64) == -1 and b"head_dim 128" in err()
    assert fwd_b(nkv=MAX_KV + 1) == -1 and b"Nkv must be in 1..640" in err()
    assert fwd_b(bs_mu=128) == -1 and b"batch stride" in err()
    for bad in (257, 258, 259):
        assert fwd_b(bs_mu=bad) == -1 and b"mu" in err()
    assert fwd_b(bs_sv=258) == -1 and b"batch strides" in err()
    assert fwd_b(b=0) == -1 and b"B must be" in err()


def test_binding_refuses_a_mismatched_mu():
    """The host wrapper decides on shapes alone, before any pointer is read."""
    v8t, sv = torch.empty((3, 128, 64), dtype=F8, device="meta"), torch.empty((3, 128), dtype=F32, device="meta")
    for mu in (torch.empty((3, 64), dtype=F32, device="meta"), torch.empty((3, 128), dtype=BF16, device="meta"),
               torch.empty((3, 256), dtype=F32, device="meta")[:, ::2]):
        with pytest.raises(_hip.HipLibraryError, match="mu must be"):
            _hip.attention_cross8_pre(None, None, None, None, v8t, sv, 3, mu=mu)


# ------------------------------------------------------------------------------------------------------------------ the recipes on a padded context
@functools.lru_cache(maxsize=None)
def padded_case():
    """The accuracy case: (q, k, v bf16; the emulated q8, k8, sq, sk; ref; mean error of the pv8 emulation, of the smoothed emulation).
    ref is attention in fp64 on the dequantised q8 / k8 scores and the bf16 v: only the P V recipe differs between the two legs."""
    c = ACC_HEADS * 128
    q, k = seeded((ACC_NQ, c), 130, scale=8.0), seeded((L_CTX, c), 131)
    v = padded_context_v(L_TEXT, L_CTX, ACC_HEADS)
    q8, k8, sq, sk, _, _ = qk8.quant_emu(q, k, ACC_HEADS)
    ref = qk8.attn_emu(q8, k8, sq, sk, v, ACC_HEADS)
    sv0, v80, _ = pv8.quant_v_emu(v, ACC_HEADS)
    e_pv8 = (pv8.attn_pv8_emu(q8, k8, sq, sk, v80, sv0, ACC_HEADS) - ref).abs().mean().item()
    mu, sv, v8 = smv.quant_vs_emu(v, ACC_HEADS)
    e_s = (smv.attn_pv8s_emu(q8, k8, sq, sk, v8, sv, mu, ACC_HEADS) - ref).abs().mean().item()
    return q, k, v, (q8, k8, sq, sk), ref, e_pv8, e_s


def test_recipes_separate_on_a_padded_context():
    """Before any device is involved: on the padded context the two recipes, both emulated in fp64, separate by more than the factor
    2 below which the criterion of test_padded_context_error_falls would say nothing (2.21 x: 2.139e-2 against 9.669e-3)."""
    v = padded_case()[2]
    assert v.shape == (L_CTX, ACC_HEADS * 128) and torch.equal(v[L_TEXT:], v[L_TEXT:L_TEXT + 1].expand(L_CTX - L_TEXT, -1))
    assert not torch.equal(v[L_TEXT - 1], v[L_TEXT]) and 3.0 < v[L_TEXT].float().std().item() < 5.0 and 0.9 < v[:L_TEXT].float().std().item() < 1.1
    e_pv8, e_s = padded_case()[5:]
    print(f"padded context, {L_CTX} keys, L_text {L_TEXT}, peaked rows: mean |emulation - ref| pv8 {e_pv8:.3e}, smoothed {e_s:.3e}, "
          f"ratio {e_pv8 / e_s:.2f}")
    assert e_pv8 >= 2 * e_s


# ------------------------------------------------------------------------------------------------------------------ 2. the kernel
def cross_inputs(heads, nq, nkv, data):
    """q (nq, C), k and v (nkv, C) bf16 on the CPU: N(0, 1); peaked rows (q x 8); peaked rows over a padded-context v."""
    c = heads * 128
    q, k = seeded((nq, c), 130, scale=1.0 if data == "normal" else 8.0), seeded((nkv, c), 131)
    v = padded_context_v(max(1, nkv * L_TEXT // L_CTX), nkv, heads) if data == "padded" else seeded((nkv, c), 132)
    return q, k, v


def quantise(hip, q, k, v, heads, smooth=True):  # noqa: F811
    """The operands from the library's own quantisers, on the GPU: (q8, k8, sq, sk, v8t, sv[, mu]); a leading batch dimension is kept."""
    qd, kd, vd = (t.cuda() if t.dim() == 3 else t.cuda()[None] for t in (q, k, v))
    q8, _, sq, _, _ = hip.attn_quant_qk(qd, torch.zeros_like(qd), heads)
    _, k8, _, sk, _ = hip.attn_quant_qk(torch.zeros_like(kd), kd, heads)
    v8t, sv, _, *mu = hip.attn_quant_vt(vd, heads, smooth=smooth)
    return (q8, k8, sq, sk, v8t, sv) + tuple(mu)


def assert_cross8s_equals_pv8s(hip, ops, heads, label):  # noqa: F811
    want = hip.attention_pv8_pre(*ops[:6], heads, workspace=None, mu=ops[6])
    got = hip.attention_cross8_pre(*ops[:6], heads, mu=ops[6])
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all(), "the comparator itself"
    bad = (got != want).any(-1).flatten().nonzero().flatten()
    assert torch.equal(got, want), f"{label}: {bad.numel()} of {got.shape[1]} rows differ from fg_attn_fwd_pv8s_bf16, first {bad[:8].tolist()}"
    return got


@gpu
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("heads,nq,nkv", SHAPES + [WALK], ids=[f"{h}x{a}x{b}" for h, a, b in SHAPES + [WALK]])
def test_cross8s_equals_pv8s(hip, heads, nq, nkv, data):  # noqa: F811
    """torch.equal with the direct launch of fg_attn_fwd_pv8s_bf16 on the same operands."""
    assert hip.load().fg_attn_workspace_bytes(1, nq, nkv, heads) == 0, "the comparator must be the direct launch"
    ops = quantise(hip, *cross_inputs(heads, nq, nkv, data), heads)
    got = assert_cross8s_equals_pv8s(hip, ops, heads, f"{heads} heads, Nq {nq}, Nkv {nkv}, {data}")
    if nkv > 1:
        assert not torch.equal(got, hip.attention_cross8_pre(*ops[:6], heads)), "mu was not added"


# ------------------------------------------------------------------------------------------------------------------ 3. exact
@gpu
@pytest.mark.parametrize("nkv", (77, 512))
def test_constant_v_is_exact(hip, nkv):  # noqa: F811
    """v[j][c] = m_c for all keys: softmax . m_c is m_c and the smoothed form returns it bit for bit (mu = m_c, every byte of v8t zero, sv
    the floor).  fg_attn_fwd_cross8_bf16 on the same input carries m_c times the rounding defect of its P row and does NOT return it."""
    heads, nq = 3, 300
    c = heads * 128
    q, k = seeded((nq, c), 150, scale=8.0), seeded((nkv, c), 151)
    m = seeded((1, c), 152, scale=3.0)
    v = m.expand(nkv, c).contiguous()
    ops = quantise(hip, q, k, v, heads)
    assert torch.equal(ops[6].cpu().view(1, c), m.float()) and (ops[4].view(U8) == 0).all() and (ops[5] == qk8.FLOOR_SCALE).all()
    got = hip.attention_cross8_pre(*ops[:6], heads, mu=ops[6])[0].cpu()
    bad = (got != m).any(-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {nq} rows differ from m_c, first {bad[:8].tolist()}"
    plain = hip.attention_cross8_pre(*quantise(hip, q, k, v, heads, smooth=False), heads)[0].cpu()
    e = (plain.float() - m.float()).abs()
    print(f"constant V, Nkv = {nkv}, q x 8: fg_attn_fwd_cross8_bf16 max |out - m_c| = {e.max().item():.3e}, {(e != 0).float().mean().item():.1%} "
          f"of the elements off, relative to |m_c| max {(e / m.float().abs().clamp(min=1e-30)).max().item():.3e}; the smoothed form: 0")
    assert not torch.equal(plain, m.expand(nq, c)), "the unsmoothed kernel returns a constant V too: the input shows nothing"


# ------------------------------------------------------------------------------------------------------------------ 4. the batched form
@gpu
@pytest.mark.parametrize("heads,nq,nkv", [(3, 300, 77), (3, 257, 512)])
def test_batched_form_equals_single_calls(hip, heads, nq, nkv):  # noqa: F811
    """B = 2 with a context of its own per element (one padded, one N(0, 1)): each element's bytes are those of the single-element call
    on that element's operands."""
    c = heads * 128
    q = torch.stack([seeded((nq, c), 170, scale=8.0), seeded((nq, c), 171)])
    k = torch.stack([seeded((nkv, c), 172), seeded((nkv, c), 173)])
    v = torch.stack([padded_context_v(max(1, nkv * L_TEXT // L_CTX), nkv, heads, 174), seeded((nkv, c), 176)])
    ops = quantise(hip, q, k, v, heads)
    assert ops[0].dim() == 3 and ops[6].shape == (2, heads, 128) and not torch.equal(ops[6][0], ops[6][1])
    got = hip.attention_cross8_pre(*ops[:6], heads, mu=ops[6])
    torch.cuda.synchronize()
    assert got.shape == (2, nq, c)
    for e in range(2):
        one = [t[e] for t in ops]
        want = hip.attention_cross8_pre(*one[:6], heads, mu=one[6])
        assert torch.isfinite(want.float()).all()
        assert torch.equal(got[e], want[0]), (e, (got[e] != want[0]).sum().item())
    # batch strides with gaps, mu's included, straight through the C ABI
    (q8s, _), (k8s, _), (sqs, _), (sks, _), (v8s, _), (svs, _), (mus, _), (out, _) = (
        smv.spread(t.shape, t.dtype, g) for t, g in zip(ops + (got,), (32, 16, 3, 5, 64, 12, 4, 8)))
    for dst, src in zip((q8s, k8s, sqs, sks, v8s, svs, mus), ops):
        dst.view(U8 if dst.dtype == F8 else dst.dtype).copy_(src.view(U8 if src.dtype == F8 else src.dtype))
    hip._call("fg_attn_fwd_cross8s_bf16_b", hip._ptr(q8s), q8s.stride(0), hip._ptr(k8s), k8s.stride(0), hip._ptr(sqs), sqs.stride(0),
              hip._ptr(sks), sks.stride(0), hip._ptr(v8s), v8s.stride(0), hip._ptr(svs), svs.stride(0), hip._ptr(mus), mus.stride(0),
              hip._ptr(out), out.stride(0), 2, nq, nkv, heads, 128, 128 ** -0.5, hip._stream(out))
    torch.cuda.synchronize()
    assert torch.equal(out, got)


# ------------------------------------------------------------------------------------------------------------------ 5. accuracy
@gpu
def test_padded_context_error_falls(hip):  # noqa: F811
    """On the padded context (512 keys, L_text = 40, peaked rows, 3 heads, Nq = 300) the mean |error| of fg_attn_fwd_cross8s_bf16 against
    the fp64 reference is at most that of fg_attn_fwd_cross8_bf16 divided by half the ratio by which the two recipes, emulated in fp64,
    separate on this input (2.21: test_recipes_separate_on_a_padded_context; the half because the emulation models neither the fp32
    accumulation order nor the deferred rescale).  q8 / k8 / sq / sk are the emulation's for both legs, V goes through the library's two
    producers."""
    q, k, v, qk, ref, e_pv8, e_s = padded_case()
    assert e_pv8 >= 2 * e_s, "below 2 the criterion says nothing"
    dev = [t.cuda().contiguous() for t in qk]
    errs = {}
    for smooth in (False, True):
        v8t, sv, _, *mu = hip.attn_quant_vt(v.cuda()[None], ACC_HEADS, smooth=smooth)
        got = hip.attention_cross8_pre(*dev, v8t, sv, ACC_HEADS, mu=mu[0] if smooth else None)
        torch.cuda.synchronize()
        assert torch.isfinite(got.float()).all()
        errs[smooth] = (got[0].cpu().double() - ref).abs().mean().item()
    print(f"padded context, {L_CTX} keys, L_text {L_TEXT}, peaked rows: mean |gpu - ref| cross8 {errs[False]:.3e} (recipe {e_pv8:.3e}), "
          f"cross8s {errs[True]:.3e} (recipe {e_s:.3e}), device factor {errs[False] / errs[True]:.2f}, emulated {e_pv8 / e_s:.2f}")
    assert errs[True] <= errs[False] / (0.5 * e_pv8 / e_s), (errs, e_pv8 / e_s)


# ------------------------------------------------------------------------------------------------------------------ 6. memory and streams
@gpu
@pytest.mark.parametrize("heads,nq,nkv", [(3, 300, 77), (3, 257, 512)])
def test_cross8s_reads_and_writes_inside_its_buffers(hip, heads, nq, nkv):  # noqa: F811
    """Every operand, mu included, between NaN bands of 4096 bytes and out between sentinel rows: the result is that of the plain
    buffers, so nothing past an operand reached it; the bands, the operands and the guard rows of out are intact."""
    ops = quantise(hip, *cross_inputs(heads, nq, nkv, "padded"), heads)
    want = hip.attention_cross8_pre(*ops[:6], heads, mu=ops[6])
    held = [banded(t, 0x7F if t.dtype == F8 else 0xFF) for t in ops]
    full, out = guarded((nq, heads * 128), BF16)
    views = [v for _, v in held]
    hip.attention_cross8_pre(*views[:6], heads, out=out.unsqueeze(0), mu=views[6])
    torch.cuda.synchronize()
    assert guards_intact(full), "a guard row of out was written"
    assert torch.equal(out, want[0])
    for (buf, view), t in zip(held, ops):
        assert torch.equal(view.view(U8), t.view(U8)) and (buf[:BAND] == buf[0]).all() and (buf[-BAND:] == buf[0]).all(), "an operand was written"


@gpu
def test_refused_arguments_launch_nothing(hip):  # noqa: F811
    """A null and a misaligned mu, Nkv = 641, bs_mu not a multiple of 4: the argument error, and out keeps its sentinel."""
    heads, nq = 2, 40
    c = heads * 128
    q8, k8 = torch.zeros((2, nq, c), dtype=F8, device="cuda"), torch.zeros((2, MAX_KV + 1, c), dtype=F8, device="cuda")
    sq, sk = torch.ones((2, nq, heads), device="cuda"), torch.ones((2, heads), device="cuda")
    v8t, sv = torch.zeros((2, heads, 128, 704), dtype=F8, device="cuda"), torch.ones((2, heads, 128), device="cuda")
    mu = torch.ones((2, heads, 128 + 1), device="cuda")
    full, out = guarded((2 * nq, c), BF16)
    lib, p, s = hip.load(), hip._ptr, hip._stream(out)
    ptrs = [p(t) for t in (q8, k8, sq, sk, v8t, sv)]
    one, err = lib.fg_attn_fwd_cross8s_bf16, lib.fg_last_error
    assert one(*ptrs, None, p(out), nq, 64, heads, 128, 0.1, s) == -1 and b"mu" in err()
    assert one(*ptrs, ctypes.c_void_p(mu.data_ptr() + 4), p(out), nq, 64, heads, 128, 0.1, s) == -1 and b"mu" in err()
    assert one(*ptrs, p(mu), p(out), nq, MAX_KV + 1, heads, 128, 0.1, s) == -1 and b"Nkv must be in 1..640" in err()

    def batched(mu_ptr, bs_mu, nkv=64):
        return lib.fg_attn_fwd_cross8s_bf16_b(ptrs[0], nq * c, ptrs[1], (MAX_KV + 1) * c, ptrs[2], nq * heads, ptrs[3], heads, ptrs[4],
                                              v8t.stride(0), ptrs[5], c, mu_ptr, bs_mu, p(out), nq * c, 2, nq, nkv, heads, 128, 0.1, s)
    assert batched(p(mu), mu.stride(0)) == -1 and b"mu" in err()      # 258 floats: not a multiple of 4
    assert batched(p(mu), c + 2) == -1 and b"mu" in err()
    assert batched(None, c) == -1 and b"mu" in err()
    assert batched(ctypes.c_void_p(mu.data_ptr() + 8), c) == -1 and b"mu" in err()
    assert batched(p(mu), c, MAX_KV + 1) == -1 and b"Nkv must be in 1..640" in err()
    with pytest.raises(hip.HipLibraryError, match="Nkv must be in"):
        hip.attention_cross8_pre(q8[0], k8[0], sq[0], sk[0], v8t[0], sv[0], heads, out=out[:nq].unsqueeze(0), mu=sv[0])
    torch.cuda.synchronize()
    assert (full == qk8.POISON).all(), "a refused call wrote to out"


@gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_entry_point_only_enqueues_and_captures(hip, batch):  # noqa: F811
    """The entry point (batch 2: its _b form) recorded on a side stream into a graph: nothing runs at capture (out keeps its fill), two
    replays give the bits of the eager call."""
    heads, nq, nkv = 3, 700, 512
    q, k, v = cross_inputs(heads, nq, nkv, "padded")
    if batch == 2:
        q, k, v = (torch.stack([t, u]) for t, u in zip((q, k, v), cross_inputs(heads, nq, nkv, "normal")))
    ops = quantise(hip, q, k, v, heads)
    want = hip.attention_cross8_pre(*ops[:6], heads, mu=ops[6])
    torch.cuda.synchronize()
    assert want.shape[0] == batch
    out = torch.zeros_like(want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        hip.attention_cross8_pre(*ops[:6], heads, out=out, mu=ops[6])
    torch.cuda.synchronize()
    assert (out == 0).all(), "a capture launched work"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        out.zero_()

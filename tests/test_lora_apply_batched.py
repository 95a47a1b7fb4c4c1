"""What unfused hot-loaded adapters need on batches that share their gate / modulation table: the C ABI extension
include/fairygen_hip_lorabatch.h and its binding in fairygen_amd.hip (fg_lora_apply_bf16_b, fg_ln_modulate_dual_bf16_b; lora_apply and
ln_modulate_dual with batch=).

THE CONTRACT, checked with torch.equal everywhere: for every batch element b, the bytes a batched entry point writes for b are those the
entry point without `_b` writes when it is called on element b alone, with the same (one element's) table and the same A and B.  The
elements of a test batch differ, the two gate rows differ, and the rows of an element (1, 63, 70, 130) are no multiples of the 64 rows a
workgroup of the adapter kernel holds: a flat launch over B * M rows would put an element boundary inside a tile and would pick the gate
row of every element but the first by the row number of the whole matrix — both change bytes.

The contract cases call fg_lora_apply_bf16_b itself through ctypes for every B, 1 included (hip.lora_apply sends batch=1 to the
single-element entry point); the binding's batch= is compared with the entry point in a test of its own.

x and out of the adapter kernel lie in strided buffers with guard columns left and right and guard rows below; the reference buffers
carry ANOTHER guard value and, for the write mode, another fill: all rows must be written, the guards must survive.
"""
import ctypes
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, seeded
from fairygen_amd import hip as _hip

gpu = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("fg_lora_apply_bf16_b", "fg_ln_modulate_dual_bf16_b")
QUERIES = ("fg_dit_lorabatch_version",)
EPS, FP8_MAX = 1e-6, 448.0
K, NG = 256, 128                       # the smallest K and group width the kernel's callers use: four k-chunks (one per wave), two column blocks
ROWS, BATCHES = (1, 63, 70, 130), (1, 2, 3)
GUARD_ROWS, GUARD_COLS = 3, 8
GUARD, GUARD_REF = 7.0, -3.0


# ------------------------------------------------------------------------------------------------------------------ CPU: ABI and argument checks
def test_extension_abi():
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_lorabatch.h")).read()
    # the main table and the seven earlier extensions are what they were
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55
    tables = (_hip.PV8_SYMBOLS, _hip.SHARD8_SYMBOLS, _hip.CROSS8_SYMBOLS, _hip.BATCH8_SYMBOLS, _hip.ROWBATCH_SYMBOLS, _hip.ROWBATCH8_SYMBOLS)
    assert [len(t) for t in tables] == [4, 6, 3, 9, 5, 3]
    assert lib.fg_dit_rowbatch_version() == 1 and lib.fg_dit_rowbatch8_version() == 1
    others = _hip.EXPORTED_SYMBOLS + [s for t in tables for s in t]
    assert not any(name in others for name in NAMES + QUERIES)
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_lorabatch.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.LORABATCH_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 3
    assert _hip.LORABATCH_ABI_VERSION == 1 and lib.fg_dit_lorabatch_version() == 1
    assert sorted(_hip._LORABATCH_SIGNATURES) == sorted(NAMES) and _hip._LORABATCH_QUERIES == {QUERIES[0]: (ctypes.c_int, [])}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has the arguments of its declaration, and they are the single-element entry point's with a c_int (B) in front of the rows
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "fg_stream_t": ctypes.c_void_p,
             "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name, rows_arg in zip(NAMES, ("M", "rows")):
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        args = [a.split() for a in decl.split(",")]
        want = [kinds[" ".join(a[:-1])] for a in args]
        assert want == _hip._LORABATCH_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is ctypes.c_int
        at = [a[-1] for a in args].index("B")
        assert args[at] == ["int", "B"] and args[at + 1] == ["int64_t", rows_arg], name
        assert want[:at] + want[at + 1:] == list(_hip._SIGNATURES[name[:-2]]), name
    # load() checks the version: a library that answers another one is refused
    real = _hip._lib
    try:
        _hip._lib = None
        _hip.LORABATCH_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="ABI mismatch"):
            _hip.load()
    finally:
        _hip.LORABATCH_ABI_VERSION = 1
        _hip._lib = real


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1; the pointers here are not device memory, a
    launch would fault — so every call below carries exactly one bad argument and none is valid)."""
    lib = _hip.load()
    p16 = ctypes.c_void_p(16)
    err = lambda: lib.fg_last_error()      # noqa: E731

    def la(B=2, x=p16, m=512, k=256, ng=256, r=32, g=1, mode=1, gate=None, rows=1):
        return lib.fg_lora_apply_bf16_b(x, k, p16, p16, p16, g * ng, B, m, k, ng, r, g, mode, gate, rows, g * ng, 0, None)
    for bad in (0, 65536, -1):
        assert la(B=bad) == -1 and b"B must be in 1..65535" in err() and b"fg_lora_apply_bf16_b" in err(), bad
    # the single-element refusals, through _b (tests/test_hot_lora_kernel.py::test_lora_apply_argument_checks)
    assert la(x=ctypes.c_void_p(8)) == -1 and b"16-byte aligned" in err()
    assert la(x=None) == -1 and b"null pointer" in err()
    assert la(r=48) == -1 and b"rank" in err()
    assert la(r=160) == -1 and b"rank" in err()
    assert la(k=288) == -1 and b"K % 64" in err()
    assert la(ng=96) == -1 and b"Ng % 64" in err()
    assert la(mode=3) == -1 and b"mode must be" in err()
    assert la(mode=2) == -1 and b"gate table" in err()
    assert la(g=5) == -1 and b"groups" in err()
    assert la(m=0) == -1
    assert la(B=1, m=1 << 31) == -1 and b"31 bits" in err()
    # the rows of the whole matrix: B * M at and above 2^31, each factor fine on its own
    assert la(B=2048, m=1 << 20) == -1 and b"B * M must fit 31 bits" in err()
    assert la(B=65535, m=1 << 16) == -1 and b"B * M must fit 31 bits" in err()

    a = 4096
    rows, c = 6, 64

    def dn(B=2, mod_rows=2, first=3, x=a, out=a, q=a, sc=a, ld=6 * c, C=c, mx=FP8_MAX):
        return lib.fg_ln_modulate_dual_bf16_b(x, a, a, out, q, sc, B, rows, C, EPS, mod_rows, first, ld, mx, None)
    for bad in (0, 65536, -1):
        assert dn(B=bad) == -1 and b"B must be in 1..65535" in err(), bad
    assert dn(first=rows + 1) == -1 and b"first_rows out of range" in err()
    assert dn(first=-1) == -1 and b"first_rows out of range" in err()
    for bad in (0, 3, rows - 1, rows + 1, 2 * rows):      # 2 * rows: the rows of the whole matrix are NOT a table size
        assert dn(mod_rows=bad) == -1 and b"mod_rows must be 1, 2 or rows" in err(), bad
    for key in ("x", "out", "q", "sc"):
        assert dn(**{key: None}) == -1 and b"null pointer" in err(), key
    assert dn(x=a + 8) == -1 and b"aligned" in err()
    assert dn(out=a + 8) == -1 and b"aligned" in err()
    assert dn(q=a + 4) == -1 and b"aligned" in err()
    assert dn(ld=6 * c + 4) == -1 and b"aligned" in err()
    assert dn(mx=0.0) == -1 and b"fp8_max positive" in err()
    assert dn(C=4104) == -1 and b"need C" in err()

    # the binding decides what a batch means on the host, before it looks at anything else
    x, w = torch.zeros((2, 3, 256), dtype=BF16), torch.zeros((32, 256), dtype=BF16)
    with pytest.raises(_hip.HipLibraryError, match="does not divide"):
        _hip.lora_apply(x, w, w.T.contiguous(), x.clone(), batch=4)
    ragged = torch.zeros((2, 5, 256), dtype=BF16)[:, :3]      # a row slice of a batch: two row strides, no one strided matrix
    with pytest.raises(_hip.HipLibraryError, match="one row stride"):
        _hip.lora_apply(ragged, w, w.T.contiguous(), x.clone(), batch=2)
    with pytest.raises(_hip.HipLibraryError, match="one row stride"):
        _hip.lora_apply(x, w, w.T.contiguous(), ragged, batch=2)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):      # a layout that fits gets as far as the device check
        _hip.lora_apply(x, w, w.T.contiguous(), x.clone(), batch=2)
    with pytest.raises(_hip.HipLibraryError):
        _hip.ln_modulate_dual(torch.zeros((2, 3, 8), dtype=BF16), None, 0, 1, EPS, batch=2)


# ------------------------------------------------------------------------------------------------------------------ GPU: helpers
def _p(t, offset_elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    assert rc == 0, (name, rc, lib.fg_last_error())


def banded(rows, cols, guard):
    """A (rows + GUARD_ROWS, cols + 2 * GUARD_COLS) bf16 buffer full of `guard` and the (rows, cols) view inside its guard bands."""
    buf = torch.full((rows + GUARD_ROWS, cols + 2 * GUARD_COLS), guard, dtype=BF16, device="cuda")
    return buf, buf[:rows, GUARD_COLS:GUARD_COLS + cols]


def bands_ok(buf, rows, cols, guard):
    return bool((buf[rows:] == guard).all() and (buf[:, :GUARD_COLS] == guard).all() and (buf[:, GUARD_COLS + cols:] == guard).all())


def operands(k, ng, groups, r, seed):
    """(A (G * R, K), B (G * Ng, R)) with x A^T B^T of O(1) for x ~ N(0, 1)."""
    return (seeded((groups * r, k), seed, scale=k ** -0.5).cuda(), seeded((groups * ng, r), seed + 1, scale=r ** -0.5).cuda())


def mode_cases(m):
    """(mode, gate rows, first_rows): the five modes, the two-row gate split at 0, 5, 64 and M (inside the first tile, on the tile edge,
    all rows on row 0), each capped at the element's rows."""
    return [("write", 1, 0), ("add", 1, 0), ("gate", 1, 0), ("gelu_tanh", 1, 0)] + [("gate", 2, f) for f in sorted({0, min(5, m), min(64, m), m})]


def contract_case(b, m, k, ng, groups, r, mode, gate_rows, first, seed):
    """One launch of fg_lora_apply_bf16_b itself (ctypes: the binding sends batch=1 to the single-element entry point, so B = 1 would
    otherwise never reach the batched kernel) against b single-element launches, everything in guard bands."""
    lib = _hip.load()
    n = groups * ng
    a, bm = operands(k, ng, groups, r, seed)
    x = seeded((b * m, k), seed + 2).cuda()
    out0 = seeded((b * m, n), seed + 3).cuda()
    mod = _hip.ModTable(seeded((gate_rows, 6, n), seed + 4).cuda().contiguous(), first) if mode == "gate" else None
    xbuf, xv = banded(b * m, k, GUARD)
    obuf, ov = banded(b * m, n, GUARD)
    xv.copy_(x)
    if mode != "write":
        ov.copy_(out0)
    assert xv.stride(0) == k + 2 * GUARD_COLS and ov.stride(0) == n + 2 * GUARD_COLS      # strided: the leading dimensions are not K and N
    call(lib, "fg_lora_apply_bf16_b", _p(xv), xv.stride(0), _p(a), _p(bm), _p(ov), ov.stride(0), b, m, k, ng, r, groups, _hip._LORA_MODES[mode],
         mod.vec(2) if mod is not None else None, gate_rows, mod.ld if mod is not None else n, first, _s())
    where = (b, m, r, mode, gate_rows, first)
    for e in range(b):
        xrbuf, xr = banded(m, k, GUARD_REF)
        rbuf, rv = banded(m, n, GUARD_REF)
        xr.copy_(x[e * m:(e + 1) * m])
        if mode != "write":
            rv.copy_(out0[e * m:(e + 1) * m])
        _hip.lora_apply(xr, a, bm, rv, groups=groups, mode=mode, mod=mod, gate_idx=2)
        assert torch.equal(ov[e * m:(e + 1) * m], rv), where + (e,)
        assert bands_ok(rbuf, m, n, GUARD_REF) and bands_ok(xrbuf, m, k, GUARD_REF), where + (e,)
    assert bands_ok(obuf, b * m, n, GUARD) and bands_ok(xbuf, b * m, k, GUARD) and torch.equal(xv, x), where
    if mode != "write":
        assert not torch.equal(ov, out0), where      # the adapters did something
    return ov


# ------------------------------------------------------------------------------------------------------------------ GPU: the contract
@gpu
@pytest.mark.parametrize("r", (32, 64, 96, 128))
def test_lora_apply_contract(r):
    """The four one-pass-per-group instantiations (rank tiles 1 to 4) at K = 256, Ng = 128, every mode and gate split, M in
    (1, 63, 70, 130) x B in (1, 2, 3)."""
    for (m, b) in itertools.product(ROWS, BATCHES):
        for mode, gate_rows, first in mode_cases(m):
            contract_case(b, m, K, NG, 1, r, mode, gate_rows, first, seed=10 * m + b)


@gpu
def test_lora_apply_contract_two_gate_rows_differ_from_a_flat_launch():
    """The premise of the gate cases: on B = 2 elements of 70 rows with first_rows = 5, the single-element entry point on all 140 rows —
    what the stacked forward would have launched without the batched form — writes other bytes into element 1."""
    b, m, r, first = 2, 70, 32, 5
    got = contract_case(b, m, K, NG, 1, r, "gate", 2, first, seed=777).clone()
    a, bm = operands(K, NG, 1, r, 777)
    x, flat = seeded((b * m, K), 779).cuda(), seeded((b * m, NG), 780).cuda()
    mod = _hip.ModTable(seeded((2, 6, NG), 781).cuda().contiguous(), first)
    _hip.lora_apply(x, a, bm, flat, mode="gate", mod=mod, gate_idx=2)
    assert torch.equal(got[:m], flat[:m]) and not torch.equal(got[m:], flat[m:])


@gpu
@pytest.mark.parametrize("mode,gate_rows,first", [("add", 1, 0), ("gate", 2, 5), ("gelu_tanh", 1, 0)])
def test_lora_apply_binding_batch_equals_entry_point(mode, gate_rows, first):
    """hip.lora_apply(batch=B) on (B, M, .) views of guard-banded buffers writes what the entry point writes (contract_case), so the
    binding's view of the layout — leading dimensions, rows per element, the table's arguments — is the entry point's."""
    b, m, r = 3, 70, 64
    want = contract_case(b, m, K, NG, 1, r, mode, gate_rows, first, seed=900)
    a, bm = operands(K, NG, 1, r, 900)
    mod = _hip.ModTable(seeded((gate_rows, 6, NG), 904).cuda().contiguous(), first) if mode == "gate" else None
    xbuf, xv = banded(b * m, K, GUARD)
    obuf, ov = banded(b * m, NG, GUARD)
    xv.copy_(seeded((b * m, K), 902).cuda()), ov.copy_(seeded((b * m, NG), 903).cuda())
    _hip.lora_apply(xv.view(b, m, K), a, bm, ov.view(b, m, NG), mode=mode, mod=mod, gate_idx=2, batch=b)
    assert torch.equal(ov, want) and bands_ok(obuf, b * m, NG, GUARD) and bands_ok(xbuf, b * m, K, GUARD)


@gpu
def test_lora_apply_contract_qkv_single_pass():
    """q | k | v at rank 32 — the three-group single-pass instantiation — at the model's width: K = 3072, three groups of 3072 columns,
    M = 200, B = 2."""
    contract_case(2, 200, 3072, 3072, 3, 32, "add", 1, 0, seed=31)


@gpu
@pytest.mark.parametrize("mode,gate_rows,first", [("add", 1, 0), ("gate", 2, 64)])
def test_lora_apply_contract_column_slices(mode, gate_rows, first):
    """x and out as column slices of wider contiguous (B, M, .) buffers — 3-D views with one row stride across the elements, the layout
    of a q | k | v buffer's parts: the columns outside the slices keep their bytes."""
    b, m, r, n, wide = 3, 70, 64, NG, 64
    a, bm = operands(K, NG, 1, r, 50)
    xw, ow = seeded((b, m, K + 2 * wide), 51).cuda(), seeded((b, m, n + 2 * wide), 52).cuda()
    x, out = xw[..., wide:wide + K], ow[..., wide:wide + n]
    assert not x.is_contiguous() and not out.is_contiguous()
    before = ow.clone()
    mod = _hip.ModTable(seeded((gate_rows, 6, n), 53).cuda().contiguous(), first) if mode == "gate" else None
    _hip.lora_apply(x, a, bm, out, mode=mode, mod=mod, gate_idx=2, batch=b)
    for e in range(b):
        want = before[e, :, wide:wide + n].contiguous()
        _hip.lora_apply(x[e].contiguous(), a, bm, want, mode=mode, mod=mod, gate_idx=2)
        assert torch.equal(out[e], want), e
    assert torch.equal(ow[..., :wide], before[..., :wide]) and torch.equal(ow[..., wide + n:], before[..., wide + n:])
    assert not torch.equal(ow, before)


@gpu
def test_binding_routes_by_batch(monkeypatch):
    """batch=B > 1 goes to fg_lora_apply_bf16_b in every mode and to fg_ln_modulate_dual_bf16_b; batch None and 1 are the calls they
    have always been."""
    names, inner = [], _hip._call
    monkeypatch.setattr(_hip, "_call", lambda name, *args: (names.append(name), inner(name, *args))[1])
    a, bm = operands(K, NG, 1, 32, 5)
    x, out = seeded((2, 70, K), 6).cuda(), seeded((2, 70, NG), 7).cuda()
    mod = _hip.ModTable(seeded((2, 6, NG), 8).cuda().contiguous(), 5)
    for mode in ("write", "add", "gate", "gelu_tanh"):
        _hip.lora_apply(x, a, bm, out, mode=mode, mod=mod if mode == "gate" else None, gate_idx=2, batch=2)
    assert names == ["fg_lora_apply_bf16_b"] * 4
    del names[:]
    _hip.lora_apply(x, a, bm, out)
    _hip.lora_apply(x, a, bm, out, batch=1)
    assert names == ["fg_lora_apply_bf16"] * 2
    del names[:]
    xn, modn = seeded((2, 5, 256), 9).cuda(), _hip.ModTable(seeded((2, 6, 256), 10).cuda().contiguous(), 2)
    o2, (q2, s2) = _hip.ln_modulate_dual(xn, modn, 0, 1, EPS, batch=2)
    _hip.ln_modulate_dual(xn, modn, 0, 1, EPS)
    assert names == ["fg_ln_modulate_dual_bf16_b", "fg_ln_modulate_dual_bf16"]
    assert o2.shape == xn.shape and q2.shape == (10, 256) and q2.dtype == torch.float8_e4m3fn and s2.shape == (10, 1)
    with pytest.raises(_hip.HipLibraryError, match="does not divide"):
        _hip.ln_modulate_dual(xn, modn, 0, 1, EPS, batch=3)


# ------------------------------------------------------------------------------------------------------------------ GPU: numeric
@gpu
def test_lora_apply_batched_vs_oracle():
    """gate, two gate rows, M = 333, K = N = 3072, B = 2 against the oracle's lora_forward arithmetic per element.  Criterion of
    tests/test_hot_lora_kernel.py: max|hip - f32| <= 2 * max|bf16 - f32| + 1e-2."""
    from fairygen_amd.wan_video_dit import stack_hot_loras
    from oracle import pipeline as opipe
    b, m, k, n, first = 2, 333, 3072, 3072, 77
    x = seeded((b, m, k), 100)
    w, bias = seeded((n, k), 101, scale=k ** -0.5), seeded((n,), 102, scale=0.1)
    adapters = [(seeded((32, k), 110, scale=k ** -0.5), seeded((n, 32), 111, scale=32 ** -0.5))]
    resid, table = seeded((b, m, n), 103), seeded((2, 6, n), 104)
    gate_full = torch.where(torch.arange(m).unsqueeze(1) < first, table[0, 2], table[1, 2])      # by the row INSIDE the element

    def reference(e, dt):
        lin = opipe.hot_lora_linear(x[e].to(dt), w.to(dt), bias.to(dt), [(a.to(dt), bb.to(dt)) for a, bb in adapters])
        return resid[e].to(dt) + gate_full.to(dt) * lin
    out = torch.stack([resid[e] + gate_full * F.linear(x[e], w, bias) for e in range(b)]).cuda()      # what the gated GEMM store leaves
    a_st, b_st = stack_hot_loras([adapters], [(k, n)], torch.device("cuda"), BF16)
    _hip.lora_apply(x.cuda(), a_st, b_st, out, mode="gate", mod=_hip.ModTable(table.cuda().contiguous(), first), gate_idx=2, batch=b)
    for e in range(b):
        ref16, ref32 = reference(e, BF16), reference(e, F32)
        err_hip, err_16 = (out[e].float().cpu() - ref32).abs().max().item(), (ref16.float() - ref32).abs().max().item()
        print(f"lora_apply batched, element {e}: max|hip-f32|={err_hip:.4f} max|bf16-f32|={err_16:.4f} max|f32|={ref32.abs().max().item():.2f}")
        assert err_hip <= 2 * err_16 + 1e-2, e


# ------------------------------------------------------------------------------------------------------------------ GPU: the dual norm
def rows_in(b, rows, c, seed):
    """(b * rows, c) bf16 whose elements differ in scale and offset."""
    g = torch.Generator("cpu").manual_seed(seed)
    x = torch.randn((b, rows, c), generator=g, dtype=F32)
    x = x * torch.tensor([1.0, 5.0, 0.125])[:b].view(b, 1, 1) + torch.tensor([0.0, -1.5, 0.25])[:b].view(b, 1, 1)
    return x.reshape(b * rows, c).to(BF16).cuda()


def table(mod_rows, c, seed):
    """(mod_rows, 6, c) bf16 modulation rows, each its own values; the scale vector (1) 400 x wider, so that rows pass 448 and the row
    scales differ from 1 and from each other (tests/test_row_kernels_batched_fp8.py)."""
    g = torch.Generator("cpu").manual_seed(seed)
    t = torch.randn((mod_rows, 6, c), generator=g, dtype=F32) * 0.5
    t[:, 1] *= 400.0
    return t.to(BF16).cuda()


def poisoned(rows, c, dtype, poison):
    buf = torch.empty((rows + GUARD_ROWS, c), dtype=dtype, device="cuda")
    buf.view(torch.uint8).fill_(poison)
    return buf


@gpu
@pytest.mark.parametrize("c", (256, 3072))
def test_ln_modulate_dual_contract(c):
    lib = _hip.load()
    for b, rows in itertools.product((2, 3), (1, 5, 70)):
        x = rows_in(b, rows, c, seed=rows + b)
        for mod_rows, first in itertools.product(sorted({1, 2, rows}), sorted({0, min(2, rows), rows})):
            tab, ld = table(mod_rows, c, seed=7 + mod_rows), 6 * c
            got = [poisoned(b * rows, c, BF16, 0x7A), poisoned(b * rows, c, torch.uint8, 0x7A), poisoned(b * rows, 1, F32, 0x7A)]
            call(lib, "fg_ln_modulate_dual_bf16_b", _p(x), _p(tab), _p(tab, c), *(_p(t) for t in got), b, rows, c, EPS, mod_rows, first, ld,
                 FP8_MAX, _s())
            for e in range(b):
                want = [poisoned(rows, c, BF16, 0x55), poisoned(rows, c, torch.uint8, 0x55), poisoned(rows, 1, F32, 0x55)]
                call(lib, "fg_ln_modulate_dual_bf16", _p(x, e * rows * c), _p(tab), _p(tab, c), *(_p(t) for t in want), rows, c, EPS, mod_rows,
                     first, ld, FP8_MAX, _s())
                for g, w in zip(got, want):
                    assert torch.equal(g[e * rows:(e + 1) * rows].view(torch.uint8), w[:rows].view(torch.uint8)), (b, rows, mod_rows, first, e)
                    assert bool((w[rows:].view(torch.uint8) == 0x55).all())
            assert all(bool((g[b * rows:].view(torch.uint8) == 0x7A).all()) for g in got), (b, rows, mod_rows, first)
            sc = got[2][:b * rows].view(b, rows)
            assert rows < 5 or (sc.unique().numel() > 1 and not torch.equal(sc[0], sc[1])), (b, rows, mod_rows, first)


# ------------------------------------------------------------------------------------------------------------------ GPU: stream and capture
def _capture_and_replay(fill, chain, outs):
    """chain(), handed a side stream, is recorded under torch.cuda.graph on that stream — a launch on any other stream would end the
    capture with an error — runs nothing while it is recorded, and replays the eager bytes on refilled inputs."""
    eager = []
    for i in range(2):
        fill(i)
        chain()
        eager.append([o.clone() for o in outs])
    assert not torch.equal(eager[0][0], eager[1][0])
    fill(0)
    torch.cuda.synchronize()
    before = [o.clone() for o in outs]
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            chain()
    torch.cuda.synchronize()
    assert all(torch.equal(o, p) for o, p in zip(outs, before))      # recorded, not run
    for i in (1, 0):
        fill(i)
        graph.replay()
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            assert torch.equal(o.view(torch.uint8), eager[i][j].view(torch.uint8)), (i, j)


@gpu
def test_lora_apply_b_capture_and_replay():
    lib = _hip.load()
    b, m, r, first = 3, 70, 32, 5
    a, bm = operands(K, NG, 1, r, 60)
    fills = [(seeded((b * m, K), s).cuda(), seeded((b * m, NG), s + 1).cuda()) for s in (61, 71)]
    x, out = torch.empty_like(fills[0][0]), torch.empty_like(fills[0][1])
    tab = seeded((2, 6, NG), 63).cuda().contiguous()

    def fill(i):
        x.copy_(fills[i][0]), out.copy_(fills[i][1])

    def chain():
        call(lib, "fg_lora_apply_bf16_b", _p(x), K, _p(a), _p(bm), _p(out), NG, b, m, K, NG, r, 1, 2, _p(tab, 2 * NG), 2, 6 * NG, first, _s())
    _capture_and_replay(fill, chain, [out])


@gpu
def test_ln_modulate_dual_b_capture_and_replay():
    lib = _hip.load()
    b, rows, c = 3, 70, 3072
    fills = [rows_in(b, rows, c, s) for s in (21, 31)]
    x, tab = torch.empty_like(fills[0]), table(2, c, 3)
    outs = [torch.zeros((b * rows, c), dtype=BF16, device="cuda"), torch.zeros((b * rows, c), dtype=torch.uint8, device="cuda"),
            torch.zeros((b * rows, 1), dtype=F32, device="cuda")]

    def chain():
        call(lib, "fg_ln_modulate_dual_bf16_b", _p(x), _p(tab), _p(tab, c), *(_p(t) for t in outs), b, rows, c, EPS, 2, 40, 6 * c, FP8_MAX, _s())
    _capture_and_replay(lambda i: x.copy_(fills[i]), chain, outs)

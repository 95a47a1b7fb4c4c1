"""The persistent GEMM's gated store with a PERIODIC gate rule: include/fairygen_hip_gategemm.h (fg_gemm_epilogue_bf16_sp,
fg_gemm_fp8_bf16_sp) and its binding (hip.gemm_epilogue / hip.gemm_fp8 with rows_per_element=P): row r of a batch of elements of P rows
each takes gate row 0 iff r % P < first_rows.

On the CPU: the extension's ABI tables, the refusals (FG_EINVAL before anything is launched), and the two pieces of generated code the
rule consists of, interpreted — the scalar program that turns a tile's first row into its place inside the element (one reciprocal
multiplication and one correction, no division) against m0 % P, and the four instructions per 4-row store group against (m0 + row) % P
>= first_rows for every row of a tile, in both operand types and both bodies (whole tiles / k-range pieces, 64-column pieces).

On the GPU every comparison is torch.equal.  The expectation of a case is the SAME launch shape in mode 0 (bias only; mode 0 and mode 2
of one shape share their unit plan, so this holds on every store path), followed by torch's bf16 ops: x + gate[class(row)] * y, one
rounding per op, as test_hip_kernels.test_gemm_epilogue does for the rule of the launch's rows.

Paths (asserted from the Python plan of test_gemm_unit_plan where the device has 8 x 32 CUs, never assumed):
  whole    N = 9216, K = 128 (e4m3: 256), no scratch: 72 .. 216 tiles, 9 .. 27 per XCD, too many to cut: whole tiles of the first body
  rounds   N = 11008, 3 x 512 rows: 258 tiles, a whole round per XCD and two left-over tiles (column pieces): the cursor walk over rounds
  kpieces  N = 256, K = 512 and K = 6144 with scratch: at most one tile per XCD, cut along K: first body raw stores + the reduce kernel
  columns  N = 512, K = 128 (e4m3: 256), no scratch: 64-column pieces of the second body
The issue behind this file names N = 320 among its sizes; the kernel takes N % 256 == 0 only (the header's contract, which the new entry
points keep), so the sizes here are multiples of 256 and N = 320 is one of the refusals.
"""
import ctypes
import functools
import importlib.util
import os
import re
import struct

import pytest
import torch

import test_gemm_unit_plan as U
from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from test_buffer_contract import Guards
from test_gemm_shapes import describe_plan, device_layout, paths_of

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
NAMES = ("fg_gemm_epilogue_bf16_sp", "fg_gemm_fp8_bf16_sp")
QUERIES = ("fg_gemm_gate_period_version",)
M32 = 0xFFFFFFFF

PERIODS = (256, 512, 257, 511, 301, 390, 300)      # on a tile edge | one row either side | inside a 4-row group / a 32-row block | see FIRSTS
GATE_IDX = 5


def firsts_of(P):
    """first_rows of a period: around a store group (4 rows), a 32-row block and the tile edge, the ends — and at P = 300 the value
    whose class-0 run in the second element (rows 300 .. 549) crosses the tile edge at 512."""
    vals = {0, 1, 3, 4, 5, 31, 32, 33, 255, 256, P - 1, P} | ({250} if P == 300 else set())
    return sorted(v for v in vals if 0 <= v <= P)


def batches_of(P):
    return ((2, 2 * P), (3, 3 * P), (2, 2 * P - 37))      # (elements, M): the last one with a short last element


# ------------------------------------------------------------------------------------------------------ CPU: ABI and refusals
def test_extension_abi():
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_gategemm.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55      # the main table is what it was
    tables = (_hip.PV8_SYMBOLS, _hip.SHARD8_SYMBOLS, _hip.CROSS8_SYMBOLS, _hip.BATCH8_SYMBOLS, _hip.ROWBATCH_SYMBOLS, _hip.ROWBATCH8_SYMBOLS,
              _hip.LORABATCH_SYMBOLS, _hip.UP2PHASE_SYMBOLS)
    assert [len(t) for t in tables] == [4, 6, 3, 9, 5, 3, 3, 4]
    others = _hip.EXPORTED_SYMBOLS + [s for t in tables for s in t]
    assert not any(name in others for name in NAMES + QUERIES)
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_gategemm.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.GATEGEMM_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 3
    assert _hip.GATEGEMM_ABI_VERSION == 1 and lib.fg_gemm_gate_period_version() == 1
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has the arguments of its declaration: the _s entry point's with an int64_t rows_per_element behind first_rows
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "fg_stream_t": ctypes.c_void_p,
             "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        args = [a.split() for a in decl.split(",")]
        want = [kinds[" ".join(a[:-1])] for a in args]
        assert want == _hip._GATEGEMM_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is ctypes.c_int
        at = [a[-1] for a in args].index("rows_per_element")
        assert args[at] == ["int64_t", "rows_per_element"] and args[at - 1] == ["int64_t", "first_rows"], name
        assert want[:at] + want[at + 1:] == list(_hip._SIGNATURES[name[:-1]]), name
    assert lib.fg_gemm_sched_bytes() == 256 and lib.fg_gemm_workspace_bytes(512, 256, 256) == lib.fg_gemm_workspace_bytes(1, 256, 256)
    real = _hip._lib
    try:          # load() checks the version: a library that answers another one is refused
        _hip._lib = None
        _hip.GATEGEMM_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="ABI mismatch"):
            _hip.load()
    finally:
        _hip.GATEGEMM_ABI_VERSION = 1
        _hip._lib = real


def test_refusals():
    """FG_EINVAL (-1) on the host, before anything is launched: the pointers are not device memory, a launch would fault — every call
    below carries exactly one bad argument."""
    lib, p16 = _hip.load(), ctypes.c_void_p(16)

    def bf16(mode=2, gate_rows=2, P=256, M=512, N=256, gate=p16):
        return lib.fg_gemm_epilogue_bf16_sp(p16, 256, p16, p16, p16, N, M, N, 256, mode, gate, gate_rows, 6 * N, 3, P, None, p16, 0, None)

    def fp8(mode=2, gate_rows=2, P=256, M=512, N=256, gate=p16):
        return lib.fg_gemm_fp8_bf16_sp(p16, 256, p16, p16, p16, p16, N, M, N, 256, mode, gate, gate_rows, 6 * N, 3, P, None, p16, 0, None)

    for call, name in ((bf16, b"fg_gemm_epilogue_bf16_sp"), (fp8, b"fg_gemm_fp8_bf16_sp")):
        for mode in (0, 3, 4, 1, 5):
            assert call(mode=mode) == -1 and b"mode must be 2" in lib.fg_last_error() and name in lib.fg_last_error(), mode
        assert call(gate_rows=1) == -1 and b"gate table of 2 rows" in lib.fg_last_error()
        for P in (0, -1, -256):
            assert call(P=P) == -1 and b"rows_per_element must be positive" in lib.fg_last_error(), P
        for P in (1, 37, 255):          # below the tile height and below M: a tile could meet two element boundaries
            assert call(P=P) == -1 and b"at least 256" in lib.fg_last_error(), P
        assert call(N=320) == -1 and b"N % 256" in lib.fg_last_error()          # the checks of the _s forms behind them
        assert call(gate=None) == -1 and b"gate table" in lib.fg_last_error()
    x = torch.zeros(4, 256, dtype=BF16)          # the binding: a CPU tensor never reaches the library
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.gemm_epilogue(x, x, x[0], rows_per_element=256)


# ------------------------------------------------------------------------------------------------------ CPU: the generated rule, interpreted
@functools.lru_cache(maxsize=None)
def generator(fp8):
    """gen_gemm_p.py under a name of its own (its configuration lives in module globals), in the form the Makefile builds."""
    spec = importlib.util.spec_from_file_location("gen_gemm_p_gate_%d" % fp8, os.path.join(REPO, "fairygen_amd", "csrc", "gen_gemm_p.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    if fp8:
        G.configure_fp8()
    G.GATEP = True
    return G


def sreg(tok):
    m = re.fullmatch(r"s(\d+)", tok.strip())
    return int(m.group(1)) if m else None


def run_place_program(G, m0, period):
    """emit_load_record_b of the periodic form on a fake record and kernel-argument block -> the SGPR file."""
    E = G.Emitter()
    G.emit_load_record_b(E)
    magic = ((1 << 32) + period - 1) // period if period > 1 else 0
    mem = bytearray(256)
    struct.pack_into("<Q", mem, G.K_GATE, 0x7000_0000_1000)
    struct.pack_into("<II", mem, G.K_PERIOD, period, magic)
    s, scc = {G.S["KARG"]: 0, G.S["KARG"] + 1: 0}, 0
    for i in range(16):
        s[G.S["REC"] + i] = 0x100 + i
    s[G.S["REC"] + 11] = m0

    def val(tok):
        r = sreg(tok)
        return s[r] if r is not None else int(tok, 0) & M32

    for ln in E.lines:
        if ln.startswith("s_waitcnt"):
            continue
        op, rest = ln.split(None, 1)
        a = [t.strip() for t in rest.split(",")]
        if op == "s_mov_b64":
            (d, _), (b, _) = [map(int, re.fullmatch(r"s\[(\d+):(\d+)\]", t).groups()) for t in a]
            s[d], s[d + 1] = s[b], s[b + 1]
        elif op == "s_load_dwordx2":
            d = int(re.fullmatch(r"s\[(\d+):\d+\]", a[0]).group(1))
            s[d], s[d + 1] = struct.unpack_from("<II", mem, val(a[2]))
        elif op == "s_mov_b32":
            s[sreg(a[0])] = val(a[1])
        elif op in ("s_add_u32", "s_addc_u32"):
            r = val(a[1]) + val(a[2]) + (scc if op == "s_addc_u32" else 0)
            s[sreg(a[0])], scc = r & M32, int(r > M32)
        elif op == "s_sub_u32":
            r = val(a[1]) - val(a[2])
            s[sreg(a[0])], scc = r & M32, int(r < 0)
        elif op == "s_mul_i32":
            s[sreg(a[0])] = (val(a[1]) * val(a[2])) & M32
        elif op == "s_mul_hi_u32":
            s[sreg(a[0])] = (val(a[1]) * val(a[2])) >> 32
        elif op == "s_cmp_lt_i32":
            x, y = val(a[0]), val(a[1])
            scc = int((x - (1 << 32) if x >> 31 else x) < (y - (1 << 32) if y >> 31 else y))
        elif op == "s_cselect_b32":
            s[sreg(a[0])] = val(a[1]) if scc else val(a[2])
        else:
            raise AssertionError(f"instruction outside the interpreted subset: {ln}")
    return s


@pytest.mark.parametrize("fp8", (False, True))
def test_tile_place_program_is_m0_mod_period(fp8):
    """S_E0 = m0 % PERIOD for every tile start the header admits (m0 a multiple of 256 below 2^31) at the periods of this file, the
    smallest, a few that make the reciprocal's estimate one too large, and the largest; the tile's descriptors are what they were."""
    G = generator(fp8)
    assert G.GATEP and G.S_E0 == 99, "s100 / s101 are not the body's to take"
    tiles = sorted(set(list(range(0, 64)) + [2 ** k + d for k in range(6, 23) for d in (-1, 0, 1)] + [(1 << 23) - 1]))
    periods = PERIODS + (1, 2, 3, 255, 258, 65535, 65537, 1000003, (1 << 30) + 1, (1 << 31) - 1)
    for period in periods:
        for t in tiles if period > 1 else (0,):          # a period of one row is admitted for M = 1 only (period >= M)
            m0 = 256 * t
            s = run_place_program(G, m0, period)
            assert s[G.S_E0] == m0 % period, (period, m0, s[G.S_E0])
            assert s[G.S["M0ROW"]] == m0 and s[G.S["KIND"]] == 0x100 + 10 and s[G.S["CD"]] == 0x100 + 4
            assert s[G.S["GD"]] == (0x1000 + 0x100 + 12) and s[G.S["GD"] + 1] == 0x7000


@functools.lru_cache(maxsize=None)
def epilogue_lines(G, nb):
    E = G.Emitter()
    G.emit_epilogue(E, G.Cfg(nb), 0)
    return E.lines


def gate_classes(G, nb, e0, period, first):
    """The gated branch of emit_epilogue for the NB x 64-column body -> {row of the tile: 1 if the store group's v_cndmask took gate row
    1}: the rule's instructions are executed per lane, every other write to its registers poisons them."""
    lines = epilogue_lines(G, nb)
    start = next(i for i, ln in enumerate(lines) if ln == f"s_mov_b32 s{G.S['T']}, s{G.S_E0}")
    assert lines[start - 1].startswith(f"s_load_dword s{G.S['UNIT']},") and lines[start - 1].endswith(str(G.K_PERIOD))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("s_branch"))
    tb, rrow = G.V_TB, G.V_RROW
    lanes = [(wave, lane) for wave in range(2) for lane in range(0, 64, 16)]      # one lane per value of V_RROW (wave & 1, lane >> 4)
    v = {rrow: [128 * (w & 1) + (ln >> 4) for w, ln in lanes], tb: None, tb + 1: None}
    s = {G.S["T"]: e0, G.S["UNIT"]: period, G.S["FIRST"]: first}
    vcc, classes, group, waited = None, {}, 0, False

    def vreg(tok):
        m = re.fullmatch(r"v(\d+)", tok)
        return int(m.group(1))

    for ln in lines[start + 1:end]:
        op, _, rest = ln.partition(" ")
        a = [t.strip() for t in rest.split(",")]
        if op == "s_waitcnt" and "lgkmcnt(0)" in rest:
            waited = True          # the period's scalar load has landed before the first group
        if op == "v_add_u32" and a[0] == f"v{tb}":
            assert waited and a[1] == f"s{G.S['T']}" and a[2] == f"v{rrow}"
            v[tb] = [(s[G.S["T"]] + r) & M32 for r in v[rrow]]
        elif op == "v_subrev_u32" and a[0] == f"v{tb + 1}":
            v[tb + 1] = [(x - s[sreg(a[1])]) & M32 for x in v[vreg(a[2])]]
        elif op == "v_min_u32" and a[0] == f"v{tb}":
            v[tb] = [min(x, y) for x, y in zip(v[vreg(a[1])], v[vreg(a[2])])]
        elif op == "v_cmp_le_u32":
            assert a[0] == "vcc" and v[vreg(a[2])] is not None
            vcc = [int(s[sreg(a[1])] <= x) for x in v[vreg(a[2])]]
        elif op == "s_add_u32" and a[0] == f"s{G.S['T']}":
            assert a[1] == f"s{G.S['T']}" and a[2] == "4"
            s[G.S["T"]] += 4
        elif op == "v_cndmask_b32":
            assert a[3] == "vcc" and vcc is not None and int(a[1][1:]) - G.V_G0 == int(a[2][1:]) - G.V_G1 == int(a[0][1:]) - (tb + 6)
            if a[1] == f"v{G.V_G0}":          # the first of the group's four
                for r, c in zip(v[rrow], vcc):
                    assert classes.setdefault(r + 4 * group, c) == c
                group += 1
        else:          # any other write to the rule's registers
            dst = re.match(r"v\[?(\d+)(?::(\d+))?", a[0]) if op.startswith(("v_", "ds_read", "buffer_load")) else None
            if dst:
                lo, hi = int(dst.group(1)), int(dst.group(2) or dst.group(1))
                for r in (tb, tb + 1):
                    if lo <= r <= hi:
                        v[r] = None
            if op.startswith("v_cmp") or "vcc" in a[0]:
                vcc = None
    assert group == 32 and sorted(classes) == list(range(256))
    return classes


@pytest.mark.parametrize("fp8", (False, True))
def test_store_group_rule_is_the_periodic_class(fp8):
    """Every row of a tile, both bodies: the class the generated store groups select is (m0 + row) % P >= first_rows, for the tiles of
    three elements of every period and first_rows of this file."""
    G = generator(fp8)
    for nb in (4, 1):
        for P in PERIODS:
            for first in firsts_of(P):
                for m0 in range(0, 3 * P, 256):
                    got = gate_classes(G, nb, m0 % P, P, first)
                    want = {r: int((m0 + r) % P >= first) for r in range(256)}
                    assert got == want, (nb, P, first, m0, [r for r in range(256) if got[r] != want[r]][:8])


def test_existing_bodies_do_not_change():
    """The flag is a second instantiation: without it the generator emits what it emitted (the record program and the gated branch)."""
    plain, gate = U.G, generator(False)
    assert not getattr(plain, "GATEP", False)
    for fn, args in (("emit_load_record_b", ()), ("emit_epilogue", (plain.Cfg(4), 0))):
        a, b = plain.Emitter(), gate.Emitter()
        getattr(plain, fn)(a, *args)
        getattr(gate, fn)(b, *((gate.Cfg(4), 0) if args else ()))
        assert a.lines != b.lines and not any("224" in ln and ln.startswith("s_load") for ln in a.lines)
        assert [ln for ln in a.lines if "v_min_u32" in ln or f"s{gate.S_E0}" in ln] == []


# ------------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def hip():
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


@pytest.fixture(scope="module")
def state(hip):
    """One scheduler block and scratch for the module: every launch here is on it, and it is never reset."""
    return hip.gemm_state("cuda")


M_MAX = 3 * max(PERIODS)
# name -> (N, K of bf16, K of e4m3, scratch, the path names (test_gemm_shapes.paths_of) a launch must / must not reach)
CONFIGS = {
    "whole": (9216, 128, 256, False, ("main: whole", "left-over tiles whole"), ("second:", "reduce:")),
    "kpieces": (256, 512, 512, True, ("reduce: split",), ("main: whole", "second:")),
    "kpieces-k6144": (256, 6144, 6144, True, ("reduce: split",), ("main: whole", "second:")),
    "columns": (512, 128, 256, False, ("second:",), ("main: whole", "reduce:")),
}


@functools.lru_cache(maxsize=None)
def operands(fp8, N, K):
    """(a, scale, w, bias, res, table) on the device for M_MAX rows; a case takes the first M rows."""
    a = seeded((M_MAX, K), 901, scale=0.5).cuda()
    w, bias = seeded((N, K), 902, scale=0.05).cuda(), seeded((N,), 903, scale=0.2).cuda()
    res, table = seeded((M_MAX, N), 904).cuda(), seeded((2, 6, N), 905).cuda()
    if fp8:
        aq, sc = _hip.fp8_quant_rows(a)
        return aq, sc, w.to(F8), bias, res, table
    return a, None, w, bias, res, table


def launch(hip, fp8, ops, M, state, ws, **kw):
    a, sc, w, bias, _, _ = ops
    sched, scratch = state
    kw = dict(sched=sched, workspace=scratch if ws else False, **kw)
    return hip.gemm_fp8(a[:M], sc[:M], w, bias, **kw) if fp8 else hip.gemm_epilogue(a[:M], w, bias, **kw)


def expected(y, res, table, M, P, first):
    """x + bf16(gate[class] * y) in bf16 tensor ops, class = row % P >= first."""
    cls = (torch.arange(M, device=y.device) % P >= first).long()
    return res[:M] + table[cls, GATE_IDX] * y


def assert_paths(name, M, N, k_bytes, ws):
    must, never = CONFIGS[name][4:]
    nxcd, per = device_layout()
    print(f"{name} {M}x{N}, {k_bytes} k bytes: " + describe_plan(M, N, k_bytes, ws, nxcd, per))
    if (nxcd, per) == (8, 32):
        names = paths_of(M, N, k_bytes, ws)
        assert all(any(n.startswith(m) for n in names) for m in must[:1]) and not [n for n in names if n.startswith(never)], (name, M, names)
        if len(must) > 1:
            assert any(n.startswith(must[1]) for n in names), (name, M, names)


@gpu
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_periodic_gate(hip, state, fp8, name, P):
    """One (type, store path, period): 2 and 3 elements and a short last element, every first_rows of the period."""
    N, k16, k8, ws = CONFIGS[name][:4]
    K = k8 if fp8 else k16
    ops = operands(fp8, N, K)
    res, table = ops[4], ops[5]
    for B, M in batches_of(P):
        assert_paths(name, M, N, K * (1 if fp8 else 2), ws)
        y = launch(hip, fp8, ops, M, state, ws)
        for first in firsts_of(P):
            got = launch(hip, fp8, ops, M, state, ws, out=res[:M].clone(), residual=True, mod=hip.ModTable(table, first), gate_idx=GATE_IDX,
                         rows_per_element=P)
            want = expected(y, res, table, M, P, first)
            if not torch.equal(got, want):
                bad = (got != want).any(1).nonzero().flatten()
                raise AssertionError(f"{name} {'e4m3' if fp8 else 'bf16'} P {P} B {B} M {M} first_rows {first}: {bad.numel()} rows differ, "
                                     f"first {bad[:6].tolist()}, last {bad[-1].item()} (row % P: {(bad[:6] % P).tolist()})")
    assert not state[0].any(), "the cursors were not cleared"


@gpu
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_whole_rounds_and_one_workgroup_per_xcd(hip, state, fp8):
    """3 x 512 rows at N = 11008: 258 tiles — a whole round of every XCD's CUs, then two XCDs' left-over tile as column pieces — with one
    workgroup per CU and with one per XCD (workgroups = 8: each walks its XCD's whole list in order); and the three paths of CONFIGS with
    8 workgroups at a period inside a store group."""
    N, K, P, M = 11008, 256 if fp8 else 128, 512, 3 * 512
    ops = operands(fp8, N, K)
    res, table = ops[4], ops[5]
    nxcd, per = device_layout()
    print(describe_plan(M, N, K * (1 if fp8 else 2), False, nxcd, per))
    if (nxcd, per) == (8, 32):
        assert "whole tiles, then column pieces" in paths_of(M, N, K * (1 if fp8 else 2), False)
    for wg in (0, 8):
        y = launch(hip, fp8, ops, M, state, False, workgroups=wg)
        for first in (0, 33, 256, 511):
            got = launch(hip, fp8, ops, M, state, False, workgroups=wg, out=res[:M].clone(), residual=True, mod=hip.ModTable(table, first),
                         gate_idx=GATE_IDX, rows_per_element=P)
            assert torch.equal(got, expected(y, res, table, M, P, first)), (wg, first)
    for name in ("whole", "kpieces", "columns"):
        N, k16, k8, ws = CONFIGS[name][:4]
        ops = operands(fp8, N, k8 if fp8 else k16)
        y = launch(hip, fp8, ops, 3 * 301, state, ws, workgroups=8)
        got = launch(hip, fp8, ops, 3 * 301, state, ws, workgroups=8, out=ops[4][:903].clone(), residual=True, mod=hip.ModTable(ops[5], 33),
                     gate_idx=GATE_IDX, rows_per_element=301)
        assert torch.equal(got, expected(y, ops[4], ops[5], 903, 301, 33)), name
    assert not state[0].any()


@gpu
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_one_element_is_the_s_entry_point(hip, state, fp8, name):
    """rows_per_element >= M: the bytes of fg_gemm_*_s with the same first_rows — also below the tile height, where only a period that
    covers all rows is admitted, and for a first_rows outside [0, M]."""
    N, k16, k8, ws = CONFIGS[name][:4]
    ops = operands(fp8, N, k8 if fp8 else k16)
    res, table = ops[4], ops[5]
    for M, periods in ((100, (100, 256, 1 << 40)), (777, (777, 778, 1 << 31, 1 << 40))):
        for first in (0, 1, 99, 300, M, M + 5, -3):
            mod = hip.ModTable(table, first)
            want = launch(hip, fp8, ops, M, state, ws, out=res[:M].clone(), residual=True, mod=mod, gate_idx=GATE_IDX)
            for P in periods:
                got = launch(hip, fp8, ops, M, state, ws, out=res[:M].clone(), residual=True, mod=mod, gate_idx=GATE_IDX, rows_per_element=P)
                assert torch.equal(got, want), (name, M, first, P)
    with pytest.raises(hip.HipLibraryError, match="at least 256"):
        launch(hip, fp8, ops, 777, state, ws, out=res[:777].clone(), residual=True, mod=hip.ModTable(table, 3), gate_idx=GATE_IDX, rows_per_element=255)
    with pytest.raises(hip.HipLibraryError, match="mode must be 2"):
        launch(hip, fp8, ops, 777, state, ws, out=res[:777].clone(), residual=True, rows_per_element=777)
    assert not state[0].any()


@gpu
@pytest.mark.parametrize("name", ("whole", "kpieces", "columns"))
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_rows_behind_m_and_guard_bands(hip, state, fp8, name):
    """The raw entry point on a c with ldc = N + 32 between sentinel columns and bands: nothing outside the M x N view is written (rows
    >= M of the last tile, the columns beside it, the band behind c), and the view holds the expectation."""
    N, k16, k8, ws = CONFIGS[name][:4]
    K = k8 if fp8 else k16
    a, sc, w, bias, res, table = operands(fp8, N, K)
    P, M, first = 301, 2 * 301 - 37, 33
    sched, scratch = state
    y = launch(hip, fp8, (a, sc, w, bias, res, table), M, state, ws)
    g = Guards()
    c = g.embed(res[:M], 16, 256, 8, 24)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    mod = hip.ModTable(table, first)
    tail = (p(bias), p(c), c.stride(0), M, N, K, 2, mod.vec(GATE_IDX), 2, mod.ld, first, P, p(scratch if ws else None), p(sched), 0,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if fp8:
        hip._call("fg_gemm_fp8_bf16_sp", p(a), a.stride(0), p(sc), p(w), *tail)
    else:
        hip._call("fg_gemm_epilogue_bf16_sp", p(a), a.stride(0), p(w), *tail)
    g.check(f"{name}: periodic gate, ldc = N + 32")
    assert torch.equal(c, expected(y, res, table, M, P, first))
    assert not sched.any()

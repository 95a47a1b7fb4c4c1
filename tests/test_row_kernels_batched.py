"""The DiT row kernels on batches that share their table: the C ABI extension include/fairygen_hip_rowbatch.h and its binding in
fairygen_amd.hip (fg_ln_modulate_bf16_b, fg_gate_residual_bf16_b, fg_residual_ln_bf16_b, fg_rmsnorm_rope_bf16_b).

THE CONTRACT, checked with torch.equal everywhere: for every batch element b, the bytes a batched entry point writes for b are those the
entry point without `_b` writes when it is called on element b alone, with the same (one element's) modulation / RoPE table.  The
elements of a test batch differ on purpose (N(0,1) scaled by 1, 5 and 1/8 with an offset), and the table rows differ from each other, so
a row that read the table by its row number in the whole matrix, or a workgroup that straddled two elements, would change bytes: the
rows per element (1, 5, 130) are no multiples of the 4 rows a workgroup holds.

Every output lies in a buffer that is poisoned as a whole before the launch and carries guard rows behind the B * rows rows: the rows
must all be written (they equal the reference) and the guard must survive (the pattern of tests/test_buffer_contract.py).

The batched kernels launch (ceil(rows / 4), B) workgroups: there is no capped grid-stride loop in them, so no case beyond a cap.
"""
import ctypes
import itertools
import os
import re

import pytest
import torch

from conftest import REPO
from fairygen_amd import hip as _hip

gpu = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAMES = ("fg_ln_modulate_bf16_b", "fg_gate_residual_bf16_b", "fg_residual_ln_bf16_b", "fg_rmsnorm_rope_bf16_b")
QUERIES = ("fg_dit_rowbatch_version",)
EPS = 1e-6
BATCHES, ROWS = (1, 2, 3), (1, 5, 130)
WIDTHS = (8, 3072, 4096)      # the smallest and the largest width of tests/test_row_kernel_shapes.py (W8), and the model's
GUARD, POISON = 3, 0x7ABC     # guard rows behind every output; the bf16 bit pattern (2.6e35) every output buffer is filled with


# ------------------------------------------------------------------------------------------------------------------ CPU: ABI and argument checks
def test_extension_abi():
    lib = _hip.load()
    main = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    ext = open(os.path.join(REPO, "include", "fairygen_hip_rowbatch.h")).read()
    # the main table and the earlier extensions are what they were
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55
    assert len(_hip.PV8_SYMBOLS) == 4 and len(_hip.SHARD8_SYMBOLS) == 6 and len(_hip.CROSS8_SYMBOLS) == 3 and len(_hip.BATCH8_SYMBOLS) == 9
    others = _hip.EXPORTED_SYMBOLS + _hip.PV8_SYMBOLS + _hip.SHARD8_SYMBOLS + _hip.CROSS8_SYMBOLS + _hip.BATCH8_SYMBOLS
    assert not any(name in others or name in main for name in NAMES + QUERIES)
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.ROWBATCH_SYMBOLS == sorted(NAMES + QUERIES)
    assert _hip.ROWBATCH_ABI_VERSION == 1 and lib.fg_dit_rowbatch_version() == 1
    assert sorted(_hip._ROWBATCH_SIGNATURES) == sorted(NAMES) and _hip._ROWBATCH_QUERIES == {QUERIES[0]: (ctypes.c_int, [])}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has the arguments of its declaration: as many, and of the declared kinds
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "fg_stream_t": ctypes.c_void_p, "int": ctypes.c_int,
             "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        want = [kinds[" ".join(a.split()[:-1])] for a in decl.split(",")]
        assert want == _hip._ROWBATCH_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is ctypes.c_int
        # the single-element entry point's arguments with B in front of rows
        single = list(_hip._SIGNATURES[name[:-2]])
        at = want.index(ctypes.c_int64, 4)
        assert want[:at - 1] + want[at:] == single and want[at - 1] is ctypes.c_int, name


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1; the pointers here are not device memory, a
    launch would fault): B = 0 and B above 65535, first_rows > rows, mod_rows outside {1, 2, rows}, and the single-element checks."""
    lib, a = _hip.load(), 4096
    rows, c = 6, 64
    err = lambda: lib.fg_last_error()      # noqa: E731

    def lm(B=2, mod_rows=2, first=3, x=a, ld=6 * c, C=c):
        return lib.fg_ln_modulate_bf16_b(x, a, a, a, B, rows, C, EPS, mod_rows, first, ld, None)

    def gr(B=2, mod_rows=2, first=3, gate=a, y=a):
        return lib.fg_gate_residual_bf16_b(a, y, gate, a, B, rows, c, mod_rows, first, 6 * c, None)

    def rl(B=2, mod_rows=2, first=3, gate=a, mode=0, norm=a):
        return lib.fg_residual_ln_bf16_b(a, a, gate, a, a, a, norm, mode, B, rows, c, EPS, mod_rows, first, 6 * c, None)

    def rr(B=2, ldx=3 * c, heads=2, tab=a, f32=1, sin=None):
        return lib.fg_rmsnorm_rope_bf16_b(a, ldx, a, tab, sin, f32, a, B, rows, c, heads, EPS, None)

    for fn in (lm, gr, rl):
        assert fn(B=0) == -1 and b"B must be in 1..65535" in err()
        assert fn(B=65536) == -1 and b"B must be" in err()
        assert fn(B=-1) == -1 and b"B must be" in err()
        assert fn(first=rows + 1) == -1 and b"first_rows out of range" in err()
        assert fn(first=-1) == -1 and b"first_rows out of range" in err()
        for bad in (0, 3, rows - 1, rows + 1, 2 * rows):      # 2 * rows: the rows of the whole matrix are NOT a table size
            assert fn(mod_rows=bad) == -1 and b"mod_rows must be 1, 2 or rows" in err(), bad
    assert rr(B=0) == -1 and b"B must be" in err()
    assert rr(B=65536) == -1 and b"B must be" in err()
    # the single-element entry points' own checks hold as well
    assert lm(x=a + 8) == -1 and b"aligned" in err()
    assert lm(ld=6 * c + 4) == -1 and b"aligned" in err()
    assert lm(C=4104) == -1 and b"need C" in err()
    assert gr(y=None) == -1 and b"null pointer" in err()
    assert rl(mode=2) == -1 and b"mode must be" in err()
    assert rl(norm=None) == -1 and b"null pointer" in err()
    assert rr(ldx=c - 8) == -1 and b"aligned" in err()
    assert rr(heads=3) == -1 and b"head_dim" in err()
    assert rr(f32=1, sin=a) == -1 and b"fp32 mode ONE interleaved table" in err()
    assert rr(f32=0, tab=a, sin=None) == -1 and b"both tables or neither" in err()
    # without a gate the table arguments are not read (fg_gate_residual_bf16, and fg_residual_ln_bf16 in mode 1)
    assert gr(B=0, gate=None, mod_rows=7) == -1 and b"B must be" in err()
    assert rl(B=0, gate=None, mode=1, mod_rows=7) == -1 and b"B must be" in err()


# ------------------------------------------------------------------------------------------------------------------ GPU: helpers
def _p(t, offset_elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rows_in(b, rows, c, seed):
    """(b * rows, c) bf16 whose elements differ in scale and offset."""
    g = torch.Generator("cpu").manual_seed(seed)
    x = torch.randn((b, rows, c), generator=g, dtype=F32)
    x = x * torch.tensor([1.0, 5.0, 0.125])[:b].view(b, 1, 1) + torch.tensor([0.0, -1.5, 0.25])[:b].view(b, 1, 1)
    return x.reshape(b * rows, c).to(BF16).cuda()


def table(mod_rows, c, seed):
    """(mod_rows, 6, c) bf16 modulation rows, each row its own values."""
    g = torch.Generator("cpu").manual_seed(seed)
    return (torch.randn((mod_rows, 6, c), generator=g, dtype=F32) * 0.5).to(BF16).cuda()


def poisoned(rows, c):
    buf = torch.empty((rows + GUARD, c), dtype=BF16, device="cuda")
    buf.view(torch.int16).fill_(POISON)
    return buf


def guard_ok(buf, rows):
    return bool((buf[rows:].view(torch.int16) == POISON).all())


def table_cases(rows):
    mods = sorted({1, 2, rows})
    firsts = sorted({0, min(1, rows), max(rows - 1, 0), rows})
    return list(itertools.product(mods, firsts))


def call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    assert rc == 0, (name, rc, lib.fg_last_error())


# ------------------------------------------------------------------------------------------------------------------ GPU: the contract
@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_ln_modulate_contract(c):
    lib = _hip.load()
    for b, rows in itertools.product(BATCHES, ROWS):
        x = rows_in(b, rows, c, seed=rows + b)
        for mod_rows, first in table_cases(rows):
            tab = table(mod_rows, c, seed=7 + mod_rows)
            ld = 6 * c
            got = poisoned(b * rows, c)
            call(lib, "fg_ln_modulate_bf16_b", _p(x), _p(tab), _p(tab, c), _p(got), b, rows, c, EPS, mod_rows, first, ld, _s())
            for e in range(b):
                want = poisoned(rows, c)
                call(lib, "fg_ln_modulate_bf16", _p(x, e * rows * c), _p(tab), _p(tab, c), _p(want), rows, c, EPS, mod_rows, first, ld, _s())
                assert torch.equal(got[e * rows:(e + 1) * rows], want[:rows]), (b, rows, mod_rows, first, e)
            assert guard_ok(got, b * rows), (b, rows, mod_rows, first)


@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_gate_residual_contract(c):
    lib = _hip.load()
    for b, rows in itertools.product(BATCHES, ROWS):
        x, y = rows_in(b, rows, c, seed=rows + b), rows_in(b, rows, c, seed=50 + rows + b)
        for (mod_rows, first), gated in itertools.product(table_cases(rows), (True, False)):
            tab = table(mod_rows, c, seed=7 + mod_rows)
            gate, ld = (_p(tab, 2 * c) if gated else None), 6 * c
            got = poisoned(b * rows, c)
            call(lib, "fg_gate_residual_bf16_b", _p(x), _p(y), gate, _p(got), b, rows, c, mod_rows, first, ld, _s())
            for e in range(b):
                want = poisoned(rows, c)
                call(lib, "fg_gate_residual_bf16", _p(x, e * rows * c), _p(y, e * rows * c), gate, _p(want), rows, c, mod_rows, first, ld, _s())
                assert torch.equal(got[e * rows:(e + 1) * rows], want[:rows]), (b, rows, mod_rows, first, gated, e)
            assert guard_ok(got, b * rows), (b, rows, mod_rows, first, gated)


@gpu
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("c", WIDTHS)
def test_residual_ln_contract(c, mode):
    """mode 0: p0 / p1 are the shift / scale vectors of the table; mode 1: a weight and a bias of C values."""
    lib = _hip.load()
    wb = table(1, c, seed=99)
    for b, rows in itertools.product(BATCHES, ROWS):
        x, y = rows_in(b, rows, c, seed=rows + b), rows_in(b, rows, c, seed=50 + rows + b)
        for (mod_rows, first), gated in itertools.product(table_cases(rows), (True, False)):
            tab = table(mod_rows, c, seed=7 + mod_rows)
            gate, ld = (_p(tab, 2 * c) if gated else None), 6 * c
            p0, p1 = (_p(tab, 3 * c), _p(tab, 4 * c)) if mode == 0 else (_p(wb), _p(wb, c))
            got_x, got_n = poisoned(b * rows, c), poisoned(b * rows, c)
            call(lib, "fg_residual_ln_bf16_b", _p(x), _p(y), gate, _p(got_x), p0, p1, _p(got_n), mode, b, rows, c, EPS, mod_rows, first, ld, _s())
            for e in range(b):
                want_x, want_n, o = poisoned(rows, c), poisoned(rows, c), e * rows * c
                call(lib, "fg_residual_ln_bf16", _p(x, o), _p(y, o), gate, _p(want_x), p0, p1, _p(want_n), mode, rows, c, EPS, mod_rows, first,
                     ld, _s())
                where = (b, rows, mod_rows, first, gated, e)
                assert torch.equal(got_x[e * rows:(e + 1) * rows], want_x[:rows]), where
                assert torch.equal(got_n[e * rows:(e + 1) * rows], want_n[:rows]), where
            assert guard_ok(got_x, b * rows) and guard_ok(got_n, b * rows), (b, rows, mod_rows, first, gated)


@gpu
@pytest.mark.parametrize("c,heads", [(8, 1), (3072, 24), (3072, 32), (4096, 4)])      # head_dim 8, 128, 96 (no power of two), 1024
def test_rmsnorm_rope_contract(c, heads):
    """x is the middle column block of a 3 C wide buffer (ldx = 3 C); the RoPE table is the fp32 interleaved one, the fp64 pair, or none."""
    lib = _hip.load()
    half = c // heads // 2
    w = (1.0 + 0.25 * torch.randn(c, generator=torch.Generator("cpu").manual_seed(5))).to(BF16).cuda()
    for b, rows in itertools.product(BATCHES, ROWS):
        buf = rows_in(b, rows, 3 * c, seed=rows + b)
        ang = torch.rand((rows, half), generator=torch.Generator("cpu").manual_seed(rows), dtype=F64) * 6.0
        cos64, sin64 = ang.cos().cuda(), ang.sin().cuda()
        tab32 = torch.stack([cos64, sin64], dim=-1).to(F32).contiguous()
        for tabs in ((tab32, None, 1), (cos64, sin64, 0), (None, None, 0)):
            got = poisoned(b * rows, c)
            call(lib, "fg_rmsnorm_rope_bf16_b", _p(buf, c), 3 * c, _p(w), _p(tabs[0]), _p(tabs[1]), tabs[2], _p(got), b, rows, c, heads, EPS, _s())
            for e in range(b):
                want = poisoned(rows, c)
                call(lib, "fg_rmsnorm_rope_bf16", _p(buf, e * rows * 3 * c + c), 3 * c, _p(w), _p(tabs[0]), _p(tabs[1]), tabs[2], _p(want), rows,
                     c, heads, EPS, _s())
                assert torch.equal(got[e * rows:(e + 1) * rows], want[:rows]), (b, rows, tabs[2], tabs[0] is None, e)
            assert guard_ok(got, b * rows), (b, rows, tabs[2])


@gpu
def test_binding_batch_argument():
    """fairygen_amd.hip: batch=B routes ln_modulate, gate_residual, residual_ln_modulate, residual_ln_affine and rmsnorm_rope to the _b
    entry points; per element the result of the call without batch= on that element."""
    b, rows, c, heads = 2, 37, 256, 2
    x, y = rows_in(b, rows, c, 1).view(b, rows, c), rows_in(b, rows, c, 2).view(b, rows, c)
    mod = _hip.ModTable(table(2, c, 3), first_rows=9)
    w, bias = table(1, c, 4)[0, 0], table(1, c, 4)[0, 1]
    qkv = rows_in(b, rows, 3 * c, 5).view(b, rows, 3 * c)
    ang = torch.rand((rows, c // heads // 2), generator=torch.Generator("cpu").manual_seed(6), dtype=F64)
    tab32 = torch.stack([ang.cos(), ang.sin()], dim=-1).to(F32).contiguous().cuda()
    got = {
        "ln": _hip.ln_modulate(x, mod, 0, 1, EPS, batch=b),
        "gate": _hip.gate_residual(x, y, mod, 2, batch=b),
        "plain": _hip.gate_residual(x, y, batch=b),
        "rm": _hip.residual_ln_modulate(x, y, mod, 2, 3, 4, EPS, batch=b),
        "ra": _hip.residual_ln_affine(x, y, w, bias, EPS, mod, 2, batch=b),
        "rope": _hip.rmsnorm_rope(qkv[..., c:2 * c], w, heads, EPS, tab32, batch=b),
    }
    for e in range(b):
        xe, ye = x[e:e + 1].contiguous(), y[e:e + 1].contiguous()
        assert torch.equal(got["ln"][e:e + 1], _hip.ln_modulate(xe, mod, 0, 1, EPS))
        assert torch.equal(got["gate"][e:e + 1], _hip.gate_residual(xe, ye, mod, 2))
        assert torch.equal(got["plain"][e:e + 1], _hip.gate_residual(xe, ye))
        for key, want in (("rm", _hip.residual_ln_modulate(xe, ye, mod, 2, 3, 4, EPS)), ("ra", _hip.residual_ln_affine(xe, ye, w, bias, EPS, mod, 2))):
            assert torch.equal(got[key][0][e:e + 1], want[0]) and torch.equal(got[key][1][e:e + 1], want[1]), key
        assert torch.equal(got["rope"][e:e + 1], _hip.rmsnorm_rope(qkv[e:e + 1, :, c:2 * c], w, heads, EPS, tab32))
    with pytest.raises(_hip.HipLibraryError, match="does not divide"):
        _hip.ln_modulate(x, mod, 0, 1, EPS, batch=3)


# ------------------------------------------------------------------------------------------------------------------ GPU: stream and capture
@gpu
def test_capture_and_replay():
    """Every entry point, handed a side stream, is recorded under torch.cuda.graph on that stream — a launch on any other stream would end
    the capture with an error — runs nothing while it is recorded (the zeroed outputs stay zero), and replays the eager bytes twice on
    refilled inputs."""
    lib = _hip.load()
    b, rows, c, heads = 3, 130, 3072, 24
    fills = [(rows_in(b, rows, c, s), rows_in(b, rows, c, s + 1), rows_in(b, rows, 3 * c, s + 2)) for s in (21, 31)]
    x, y, qkv = (torch.empty_like(t) for t in fills[0])
    tab, wb = table(2, c, 3), table(1, c, 4)
    ang = torch.rand((rows, 64), generator=torch.Generator("cpu").manual_seed(6), dtype=F64)
    tab32 = torch.stack([ang.cos(), ang.sin()], dim=-1).to(F32).contiguous().cuda()
    outs = [torch.empty((b * rows, c), dtype=BF16, device="cuda") for _ in range(7)]
    ld, first = 6 * c, 40

    def load(i):
        for dst, src in zip((x, y, qkv), fills[i]):
            dst.copy_(src)

    def chain():
        s = _s()
        call(lib, "fg_ln_modulate_bf16_b", _p(x), _p(tab), _p(tab, c), _p(outs[0]), b, rows, c, EPS, 2, first, ld, s)
        call(lib, "fg_gate_residual_bf16_b", _p(x), _p(y), _p(tab, 2 * c), _p(outs[1]), b, rows, c, 2, first, ld, s)
        call(lib, "fg_residual_ln_bf16_b", _p(x), _p(y), _p(tab, 2 * c), _p(outs[2]), _p(tab, 3 * c), _p(tab, 4 * c), _p(outs[3]), 0, b, rows, c, EPS,
             2, first, ld, s)
        call(lib, "fg_residual_ln_bf16_b", _p(x), _p(y), None, _p(outs[4]), _p(wb), _p(wb, c), _p(outs[5]), 1, b, rows, c, EPS, 1, 0, 0, s)
        call(lib, "fg_rmsnorm_rope_bf16_b", _p(qkv, c), 3 * c, _p(wb), _p(tab32), None, 1, _p(outs[6]), b, rows, c, heads, EPS, s)

    eager = []
    for i in range(2):
        load(i)
        chain()
        eager.append([o.clone() for o in outs])
    assert not torch.equal(eager[0][0], eager[1][0])
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            chain()
    torch.cuda.synchronize()
    assert all(not bool(o.any()) for o in outs)      # recorded, not run: nothing was enqueued outside the capture
    for i in (1, 0):
        load(i)
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            assert torch.equal(o, eager[i][j]), (i, j)

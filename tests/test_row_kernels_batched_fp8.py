"""The fp8-output norms of the DiT on batches that share their modulation table: the C ABI extension include/fairygen_hip_rowbatch8.h and
its binding in fairygen_amd.hip (fg_ln_modulate_fp8_bf16_b, fg_residual_ln_fp8_bf16_b) — tests/test_row_kernels_batched.py for the two
norms that hand their row to an fp8 Linear as e4m3 bytes and one fp32 scale per row.

THE CONTRACT, checked with torch.equal everywhere (the e4m3 bytes as uint8, the scales as int32, x_out as it is): for every batch element
b, the bytes a batched entry point writes for b are those the entry point without `_b` writes when it is called on element b alone,
with the same (one element's) table.  The elements of a test batch differ on purpose (N(0,1) scaled by 1, 5 and 1/8 with an offset), so
their row scales differ, and the table rows differ from each other: a kernel that indexed the scale output or the table by the row
number of the whole matrix, or a workgroup that straddled two elements, would change bytes — the rows per element (1, 5, 130) are no
multiples of the 4 rows a workgroup holds.

Every output lies in a buffer that is poisoned as a whole before the launch and carries guard rows behind the B * rows rows.  The
reference buffers carry ANOTHER poison, so a row that neither launch wrote differs as well: all rows must be written, the guard must
survive.
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
BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("fg_ln_modulate_fp8_bf16_b", "fg_residual_ln_fp8_bf16_b")
QUERIES = ("fg_dit_rowbatch8_version",)
EPS, FP8_MAX = 1e-6, 448.0
BATCHES, ROWS = (1, 2, 3), (1, 5, 130)
WIDTHS = (8, 3072, 4096)      # the smallest and the largest width of tests/test_row_kernel_shapes.py::test_fp8_and_dual_norm_widths, and the model's
GUARD = 3                     # guard rows behind every output
POISON, POISON_REF = 0x7A, 0x55      # the byte every output buffer / every reference buffer is filled with


# ------------------------------------------------------------------------------------------------------------------ CPU: ABI and argument checks
def test_extension_abi():
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_rowbatch8.h")).read()
    # the main table and the six earlier extensions are what they were
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55
    assert [len(t) for t in (_hip.PV8_SYMBOLS, _hip.SHARD8_SYMBOLS, _hip.CROSS8_SYMBOLS, _hip.BATCH8_SYMBOLS, _hip.ROWBATCH_SYMBOLS)] == [4, 6, 3, 9, 5]
    assert _hip.ROWBATCH_ABI_VERSION == 1 and lib.fg_dit_rowbatch_version() == 1
    others = _hip.EXPORTED_SYMBOLS + _hip.PV8_SYMBOLS + _hip.SHARD8_SYMBOLS + _hip.CROSS8_SYMBOLS + _hip.BATCH8_SYMBOLS + _hip.ROWBATCH_SYMBOLS
    assert not any(name in others for name in NAMES + QUERIES)
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_rowbatch8.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.ROWBATCH8_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 3
    assert _hip.ROWBATCH8_ABI_VERSION == 1 and lib.fg_dit_rowbatch8_version() == 1
    assert sorted(_hip._ROWBATCH8_SIGNATURES) == sorted(NAMES) and _hip._ROWBATCH8_QUERIES == {QUERIES[0]: (ctypes.c_int, [])}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES + QUERIES:
        assert hasattr(raw, name)
    # every binding has the arguments of its declaration: as many, and of the declared kinds
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "fg_stream_t": ctypes.c_void_p,
             "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        want = [kinds[" ".join(a.split()[:-1])] for a in decl.split(",")]
        assert want == _hip._ROWBATCH8_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
        assert getattr(lib, name).restype is ctypes.c_int
        # the single-element entry point's arguments with a c_int (B) in front of rows
        single = list(_hip._SIGNATURES[name[:-2]])
        at = want.index(ctypes.c_int64)
        assert want[:at - 1] + want[at:] == single and want[at - 1] is ctypes.c_int, name
        assert re.search(r"int B,\s*int64_t rows", decl), name


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1; the pointers here are not device memory, a
    launch would fault — so every call below carries exactly one bad argument and none is valid)."""
    lib, a = _hip.load(), 4096
    rows, c = 6, 64
    err = lambda: lib.fg_last_error()      # noqa: E731

    def lm(B=2, mod_rows=2, first=3, x=a, q=a, sc=a, ld=6 * c, C=c, mx=FP8_MAX):
        return lib.fg_ln_modulate_fp8_bf16_b(x, a, a, q, sc, B, rows, C, EPS, mod_rows, first, ld, mx, None)

    def rl(B=2, mod_rows=2, first=3, gate=a, mode=0, y=a, q=a, sc=a, ld=6 * c, mx=FP8_MAX):
        return lib.fg_residual_ln_fp8_bf16_b(a, y, gate, a, a, a, q, sc, mode, B, rows, c, EPS, mod_rows, first, ld, mx, None)

    for fn in (lm, rl):
        assert fn(B=0) == -1 and b"B must be in 1..65535" in err()
        assert fn(B=65536) == -1 and b"B must be" in err()
        assert fn(B=-1) == -1 and b"B must be" in err()
        assert fn(first=rows + 1) == -1 and b"first_rows out of range" in err()
        assert fn(first=-1) == -1 and b"first_rows out of range" in err()
        for bad in (0, 3, rows - 1, rows + 1, 2 * rows):      # 2 * rows: the rows of the whole matrix are NOT a table size
            assert fn(mod_rows=bad) == -1 and b"mod_rows must be 1, 2 or rows" in err(), bad
        assert fn(q=None) == -1 and b"null pointer" in err()
        assert fn(sc=None) == -1 and b"null pointer" in err()
        assert fn(q=a + 4) == -1 and b"aligned" in err()          # the e4m3 rows are written as 8-byte vectors
        assert fn(ld=6 * c + 4) == -1 and b"aligned" in err()
        assert fn(mx=0.0) == -1 and b"fp8_max positive" in err()
        assert fn(mx=-448.0) == -1 and b"fp8_max positive" in err()
    for bad in (-1, 2):
        assert rl(mode=bad) == -1 and b"mode must be" in err()
    assert lm(x=None) == -1 and b"null pointer" in err()
    assert lm(x=a + 8) == -1 and b"aligned" in err()
    assert lm(C=4104) == -1 and b"need C" in err()
    assert rl(y=None) == -1 and b"null pointer" in err()
    # without a gate, mode 1 does not read the table arguments (fg_residual_ln_fp8_bf16): the batch is still checked
    assert rl(B=0, gate=None, mode=1, mod_rows=7) == -1 and b"B must be" in err()
    # the binding refuses a batch that does not divide the rows, and host tensors, before it calls anything
    with pytest.raises(_hip.HipLibraryError):
        _hip.ln_modulate_fp8(torch.zeros((2, 3, 8), dtype=BF16), None, 0, 1, EPS, batch=2)
    with pytest.raises(_hip.HipLibraryError):
        _hip.residual_ln_affine_fp8(torch.zeros((2, 3, 8), dtype=BF16), None, None, None, EPS, batch=2)


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


def table(mod_rows, c, seed, big=(1, 4)):
    """(mod_rows, 6, c) bf16 modulation rows, each row its own values.  The vectors `big` (the two scale vectors of the table; the
    weight of the affine form) are 400 x wider: a LayerNorm output is of order 1 whatever its input's scale, and a row scale is
    max(bf16(amax / 448), 1), so only a wide multiplier takes rows above 448 and makes their scales differ from 1 and from each other."""
    g = torch.Generator("cpu").manual_seed(seed)
    t = torch.randn((mod_rows, 6, c), generator=g, dtype=F32) * 0.5
    t[:, list(big)] *= 400.0
    return t.to(BF16).cuda()


def scales_differ(sc, b, rows, c):
    """The premise of the scale checks, where the shape can carry it: the rows' scales are not all one value, and two elements' differ."""
    if c == 8 or b * rows < 2:
        return True
    s = sc[:b * rows].view(b, rows)
    return s.unique().numel() > 1 and (b == 1 or not torch.equal(s[0], s[1]))


def poisoned(rows, c, dtype, poison=POISON):
    """(rows + GUARD, c) of dtype, every byte `poison`."""
    buf = torch.empty((rows + GUARD, c), dtype=dtype, device="cuda")
    buf.view(torch.uint8).fill_(poison)
    return buf


def guard_ok(buf, rows, poison=POISON):
    return bool((buf[rows:].view(torch.uint8) == poison).all())


class Outs:
    """The outputs of one launch on `rows` rows: e4m3 rows, row scales and (the residual form) x_out, each poisoned and guarded."""

    def __init__(self, rows, c, poison, x_out=True):
        self.rows, self.poison = rows, poison
        self.q, self.sc = poisoned(rows, c, torch.uint8, poison), poisoned(rows, 1, F32, poison)
        self.x = poisoned(rows, c, BF16, poison) if x_out else None

    def parts(self, lo, hi):
        return [self.q[lo:hi], self.sc[lo:hi].view(torch.int32)] + ([self.x[lo:hi].view(torch.int16)] if self.x is not None else [])

    def guards_ok(self):
        return all(guard_ok(t, self.rows, self.poison) for t in (self.q, self.sc, self.x) if t is not None)


def table_cases(rows):
    """(mod_rows, first_rows): one table row, two rows split at 0, 2 and rows (all rows on row 1, a split, all on row 0), one row per token."""
    return list(itertools.product(sorted({1, 2, rows}), sorted({0, min(2, rows), rows})))


def call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    assert rc == 0, (name, rc, lib.fg_last_error())


# ------------------------------------------------------------------------------------------------------------------ GPU: the contract
@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_ln_modulate_fp8_contract(c):
    lib = _hip.load()
    for b, rows in itertools.product(BATCHES, ROWS):
        x = rows_in(b, rows, c, seed=rows + b)
        for mod_rows, first in table_cases(rows):
            tab, ld = table(mod_rows, c, seed=7 + mod_rows), 6 * c
            got = Outs(b * rows, c, POISON, x_out=False)
            call(lib, "fg_ln_modulate_fp8_bf16_b", _p(x), _p(tab), _p(tab, c), _p(got.q), _p(got.sc), b, rows, c, EPS, mod_rows, first, ld,
                 FP8_MAX, _s())
            for e in range(b):
                want = Outs(rows, c, POISON_REF, x_out=False)
                call(lib, "fg_ln_modulate_fp8_bf16", _p(x, e * rows * c), _p(tab), _p(tab, c), _p(want.q), _p(want.sc), rows, c, EPS, mod_rows,
                     first, ld, FP8_MAX, _s())
                for g, w in zip(got.parts(e * rows, (e + 1) * rows), want.parts(0, rows)):
                    assert torch.equal(g, w), (b, rows, mod_rows, first, e)
                assert want.guards_ok()
            assert got.guards_ok(), (b, rows, mod_rows, first)
            assert scales_differ(got.sc, b, rows, c), (b, rows, mod_rows, first)


@gpu
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("c", WIDTHS)
def test_residual_ln_fp8_contract(c, mode):
    """mode 0: p0 / p1 are the shift / scale vectors of the table; mode 1: a weight and a bias of C values.  Gate given and NULL; x_out
    a buffer of its own, and x_out aliasing x (the forward's use: the residual stream is updated in place)."""
    lib = _hip.load()
    wb = table(1, c, seed=99, big=(0,))
    for b, rows in itertools.product(BATCHES, ROWS):
        x, y = rows_in(b, rows, c, seed=rows + b), rows_in(b, rows, c, seed=50 + rows + b)
        for (mod_rows, first), gated in itertools.product(table_cases(rows), (True, False)):
            tab, ld = table(mod_rows, c, seed=7 + mod_rows), 6 * c
            gate = _p(tab, 2 * c) if gated else None
            p0, p1 = (_p(tab, 3 * c), _p(tab, 4 * c)) if mode == 0 else (_p(wb), _p(wb, c))
            where = (b, rows, mod_rows, first, gated)
            got = Outs(b * rows, c, POISON)
            call(lib, "fg_residual_ln_fp8_bf16_b", _p(x), _p(y), gate, _p(got.x), p0, p1, _p(got.q), _p(got.sc), mode, b, rows, c, EPS,
                 mod_rows, first, ld, FP8_MAX, _s())
            for e in range(b):
                want, o = Outs(rows, c, POISON_REF), e * rows * c
                call(lib, "fg_residual_ln_fp8_bf16", _p(x, o), _p(y, o), gate, _p(want.x), p0, p1, _p(want.q), _p(want.sc), mode, rows, c, EPS,
                     mod_rows, first, ld, FP8_MAX, _s())
                for g, w in zip(got.parts(e * rows, (e + 1) * rows), want.parts(0, rows)):
                    assert torch.equal(g, w), where + (e,)
                assert want.guards_ok()
            assert got.guards_ok(), where
            assert scales_differ(got.sc, b, rows, c), where
            # x_out = x: the same bytes, and the guard behind the stream survives
            inplace = Outs(b * rows, c, POISON)
            inplace.x[:b * rows].copy_(x)
            call(lib, "fg_residual_ln_fp8_bf16_b", _p(inplace.x), _p(y), gate, _p(inplace.x), p0, p1, _p(inplace.q), _p(inplace.sc), mode, b,
                 rows, c, EPS, mod_rows, first, ld, FP8_MAX, _s())
            for g, w in zip(inplace.parts(0, b * rows), got.parts(0, b * rows)):
                assert torch.equal(g, w), where + ("x_out = x",)
            assert inplace.guards_ok(), where


@gpu
def test_binding_batch_argument():
    """fairygen_amd.hip: batch=B routes ln_modulate_fp8, residual_ln_modulate_fp8 and residual_ln_affine_fp8 to the _b entry points —
    counted at hip._call — and returns the pair of ALL rows, (B * rows, C) e4m3 and (B * rows, 1) fp32: per element the result of the
    call without batch= on that element."""
    b, rows, c = 2, 37, 256
    x, y = rows_in(b, rows, c, 1).view(b, rows, c), rows_in(b, rows, c, 2).view(b, rows, c)
    mod = _hip.ModTable(table(2, c, 3), first_rows=9)
    w, bias = table(1, c, 4)[0, 0], table(1, c, 4)[0, 1]
    names, inner = [], _hip._call
    _hip._call = lambda name, *args: (names.append(name), inner(name, *args))[1]
    try:
        got = {
            "ln": (None, _hip.ln_modulate_fp8(x, mod, 0, 1, EPS, batch=b)),
            "rm": _hip.residual_ln_modulate_fp8(x, y, mod, 2, 3, 4, EPS, batch=b),
            "ra": _hip.residual_ln_affine_fp8(x, y, w, bias, EPS, mod, 2, batch=b),
            "ra0": _hip.residual_ln_affine_fp8(x, y, w, bias, EPS, batch=b),
        }
    finally:
        _hip._call = inner
    assert names == ["fg_ln_modulate_fp8_bf16_b"] + ["fg_residual_ln_fp8_bf16_b"] * 3
    for key, (xo, (q, sc)) in got.items():
        assert q.shape == (b * rows, c) and q.dtype == torch.float8_e4m3fn and sc.shape == (b * rows, 1) and sc.dtype == F32, key
        assert xo is None or xo.shape == x.shape
    for e in range(b):
        xe, ye, sl = x[e:e + 1].contiguous(), y[e:e + 1].contiguous(), slice(e * rows, (e + 1) * rows)
        wants = {"ln": (None, _hip.ln_modulate_fp8(xe, mod, 0, 1, EPS)), "rm": _hip.residual_ln_modulate_fp8(xe, ye, mod, 2, 3, 4, EPS),
                 "ra": _hip.residual_ln_affine_fp8(xe, ye, w, bias, EPS, mod, 2), "ra0": _hip.residual_ln_affine_fp8(xe, ye, w, bias, EPS)}
        for key, (xo, (q, sc)) in wants.items():
            assert torch.equal(got[key][1][0][sl].view(torch.uint8), q.view(torch.uint8)), (key, e)
            assert torch.equal(got[key][1][1][sl].view(torch.int32), sc.view(torch.int32)), (key, e)
            assert xo is None or torch.equal(got[key][0][e:e + 1], xo), (key, e)
    with pytest.raises(_hip.HipLibraryError, match="does not divide"):
        _hip.ln_modulate_fp8(x, mod, 0, 1, EPS, batch=3)


# ------------------------------------------------------------------------------------------------------------------ GPU: stream and capture
@gpu
def test_capture_and_replay():
    """Both entry points, handed a side stream, are recorded under torch.cuda.graph on that stream — a launch on any other stream would end
    the capture with an error — run nothing while they are recorded (the zeroed outputs stay zero), and replay the eager bytes twice on
    refilled inputs."""
    lib = _hip.load()
    b, rows, c = 3, 130, 3072
    fills = [(rows_in(b, rows, c, s), rows_in(b, rows, c, s + 1)) for s in (21, 31)]
    x, y = (torch.empty_like(t) for t in fills[0])
    tab, wb = table(2, c, 3), table(1, c, 4)
    q8 = [torch.empty((b * rows, c), dtype=torch.uint8, device="cuda") for _ in range(3)]
    sc = [torch.empty((b * rows, 1), dtype=F32, device="cuda") for _ in range(3)]
    xo = [torch.empty((b * rows, c), dtype=BF16, device="cuda") for _ in range(2)]
    outs = q8 + sc + xo
    ld, first = 6 * c, 40

    def load(i):
        for dst, src in zip((x, y), fills[i]):
            dst.copy_(src)

    def chain():
        s = _s()
        call(lib, "fg_ln_modulate_fp8_bf16_b", _p(x), _p(tab), _p(tab, c), _p(q8[0]), _p(sc[0]), b, rows, c, EPS, 2, first, ld, FP8_MAX, s)
        call(lib, "fg_residual_ln_fp8_bf16_b", _p(x), _p(y), _p(tab, 2 * c), _p(xo[0]), _p(tab, 3 * c), _p(tab, 4 * c), _p(q8[1]), _p(sc[1]), 0, b,
             rows, c, EPS, 2, first, ld, FP8_MAX, s)
        call(lib, "fg_residual_ln_fp8_bf16_b", _p(x), _p(y), None, _p(xo[1]), _p(wb), _p(wb, c), _p(q8[2]), _p(sc[2]), 1, b, rows, c, EPS, 1, 0, 0,
             FP8_MAX, s)

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
    assert all(not bool(o.view(torch.uint8).any()) for o in outs)      # recorded, not run: nothing was enqueued outside the capture
    for i in (1, 0):
        load(i)
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            assert torch.equal(o.view(torch.uint8), eager[i][j].view(torch.uint8)), (i, j)

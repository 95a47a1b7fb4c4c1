"""The persistent GEMMs (fg_gemm_epilogue_bf16(_s), fg_gemm_fp8_bf16(_s)) at every k-step count, small M and unit plan they accept.

The other GEMM tests run the DiT's own shapes and a few ragged ones: M >= 600, at least 9 tiles, and of the short reductions only K = 128,
256 and 512.  Here: M from 1 row on, launches of 1 and 2 tiles (six or seven XCDs without a unit), every short K the header accepts, and
each of them with and without the k-split scratch, so that both asm bodies, the k-range pieces and gemm_reduce_kernel run at the small
k-step counts where the k-loop (gen_gemm_p.py emit_kloop) leaves through another branch and emit_dma_k0 fetches past the end of K.
Helpers, operands and criteria are those of test_exact_arithmetic.py (imported): integer operands, the expectation the fp64 product,
the comparison torch.equal — no tolerance.

K and k-steps.  A k-step is 128 operand BYTES of a row: nk = K * esz / 128.  The header asks K % 128 == 0 of bf16 and K % 256 == 0 of
e4m3, i.e. K * esz % 256 == 0 in both: EVERY launch has an even nk >= 2 (test_header_shapes_have_even_k_step_counts holds the rejection
of the others).  The K list of the module, K = 128 u, therefore gives nk = 2 u in bf16 (2 .. 22 and 128) and nk = u in e4m3 (2 .. 10).  So
three exits of the generated k-loop are not reachable through the ABI by a whole tile or a column piece: the main body's nk = 1 and odd
nk >= 3, and the second body's nk = 1 and odd nk.  Odd lengths do run in the main body, as k-range pieces (3, 5, 7 steps: base + 1 of an
uneven split); a length of 1 never does (split <= nk / 2).  The scalar record program is swept over odd and even nk alike on the CPU.

Layouts (8 XCDs of 32 CUs; on another device the plan is computed from its CU count and printed, the path assertions are skipped —
hip.gemm_workspace_need assumes 256 CUs as well and then only allocates scratch that is not needed):
  L1  N = 256, M in {1, 8, 255, 256, 257}: 1 or 2 tiles, qd = 0, plan[1] all zeros: six or seven XCDs leave both bodies at once
  L2  M = 700, N = 768: 9 tiles, XCD 0 has two
  L3  M = 2309, N = 2048: 80 tiles, 10 per XCD: whole without scratch (10 * 4 > 32), split = min(3, nk / 2) with it
  L4  M = 8198, N = 2048: 264 tiles, 33 per XCD: a round of whole tiles + one left-over tile: k-range pieces, or 4 column pieces

Entry point -> path -> how it was confirmed (test_every_path_is_named holds the list against the Python plan at 256 CUs, the GPU cases
assert their own path where the device has 256 CUs and print split / cut / n_whole / n_main / n_tail per XCD population):
  first asm body, whole tiles      nk = 2 (L3 without scratch, L3 u = 1), even nk >= 4 (L3 / L4 without scratch)
  first asm body, k-range pieces   of 2 (L1: split = nk / 2), of 3 = the odd exit (L3: nk = 8 -> 3 + 3 + 2, nk = 10 -> 4 + 3 + 3), extra != 0
  gemm_reduce_kernel               splits 2, 3, 4, 5 (L1 u = 2 .. 5: the remainder loop alone, and one unrolled group of four + 0 / 1 more),
                                   6 .. 11, 32 (L1 u = 64: 7 groups of four + 3), 3 with nk % 3 != 0 (L3)
  second asm body (ring of 3)      nk = 2 (fetches one slice past K before the loop), nk = 0, 1, 2 mod 3 (4 .. 22, 128) — L1 / L2
                                   without scratch
  whole tiles, then pieces / then column pieces in one XCD's list   L4 with / without scratch, also walked by ONE workgroup per XCD
                                   (workgroups = 8), as L3's
  total < nxcd                     L1; every launch is repeated on the same scheduler block without a reset, and the block must be
                                   all zeros after each case: the last workgroup clears the cursors although most XCDs had no unit
  a slice fetched past K           L1 / L2: A inside a (M, K + 128) buffer of NaN (0x7F bytes in e4m3): same integers
  stores outside [M, N]            every M < 3000 case: `out` with ldc = N + 32 between sentinel columns and bands (Guards), both bodies
                                   and the reduce kernel

Sensitivity: with the sense of ONE exit branch of the second body's k-loop swapped (the one taken for nk = 0 mod 3) in a scratch build,
the first no-scratch case with nk = 4 fails (245 of 256 elements of the M = 1 output differ); the nk = 2 cases before it pass, as they
must (their exit is another branch).  Tried on an MI355X against the scratch library, which is not part of the tree.

Cost: the unmarked tests take 8 s of pytest time on a 16-thread host (11 s with the imports).  The 112 GPU cases, CPU references
included, take 5.3 s of pytest time on an MI355X; the slowest test 0.6 s (the first to touch the device), an L4 case 0.25 s.
"""
import ctypes

import pytest
import torch

import test_gemm_unit_plan as U
from test_buffer_contract import Guards
from test_exact_arithmetic import _assert_same, _class_change, _exact_int, _gemm_expected, _gemm_operands
from test_hip_kernels import assert_gelu_of, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn

# K = 128 u.  bf16: nk = 2 u k-steps of 128 bytes, e4m3: nk = u.
U_BF16 = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11)
U_FP8 = (2, 4, 6, 8, 10)
U_L1_LONG = 64                                   # bf16 on L1 only: split 32
L1_M, L1_N = (1, 8, 255, 256, 257), 256
L2, L3, L4 = (700, 768), (2309, 2048), (8198, 2048)
U_L3 = {False: (1, 2, 4, 5, 7, 11), True: (2, 8, 10)}          # [fp8]: whole | split 2 | 3 + 3 + 2 | 4 + 3 + 3 | 5 + 5 + 4 | 8 + 7 + 7
U_L4 = {False: (1, 2, 3, 5, 10), True: (2, 4, 10)}
U_ONE_WORKGROUP_PER_XCD = {False: (1, 2, 5), True: (2, 10)}    # of L3 and L4: also with workgroups = 8
LARGE = 3000                                     # rows from which the expectation is the device's fp32 product, cross-checked on 900 rows


def gpu_cases():
    for fp8 in (False, True):
        for u in (U_FP8 if fp8 else U_BF16 + (U_L1_LONG,)):
            for m in L1_M:
                yield "L1", fp8, m, L1_N, u
        for u in (U_FP8 if fp8 else U_BF16):
            yield ("L2", fp8) + L2 + (u,)
        for u in U_L3[fp8]:
            yield ("L3", fp8) + L3 + (u,)
        for u in U_L4[fp8]:
            yield ("L4", fp8) + L4 + (u,)


def k_bytes_of(fp8, u):
    return 128 * u * (1 if fp8 else 2)


# ------------------------------------------------------------------------------------------------------ A. the plan, on the CPU
def xcd_plans(M, N, k_bytes, have_ws, nxcd=8, per=32):
    """[(number of XCDs, TailPlan fields)] of the two XCD populations of a launch, from the Python plan of test_gemm_unit_plan."""
    s, _ = U.build_sched(M, N, k_bytes, k_bytes, nxcd=nxcd, per=per, have_ws=have_ws)
    out = []
    for count, xcd in ((s["rm"], 0), (nxcd - s["rm"], s["rm"])):
        if count:
            out.append((count, U.tail_plan(s["total"], xcd, nxcd, per, s["nk"], s["have_ws"], 4)))
    return s, out


def describe_plan(M, N, k_bytes, have_ws, nxcd=8, per=32):
    s, pops = xcd_plans(M, N, k_bytes, have_ws, nxcd, per)
    parts = []
    for (count, tp), pl in zip(pops, s["plans"] if s["rm"] else s["plans"][1:]):
        parts.append(f"{count} XCDs x {tp['len']} tiles: split {tp['split']} cut {tp['cut']} n_whole {pl['n_whole']} n_main {pl['n_main']} n_tail {pl['n_tail']}")
    return f"{s['total']} tiles, nk {s['nk']}, {nxcd} x {per} CUs, scratch {'taken' if s['have_ws'] else 'not taken'}: " + "; ".join(parts)


def paths_of(M, N, k_bytes, have_ws, nxcd=8, per=32):
    """The named paths a launch reaches."""
    s, pops = xcd_plans(M, N, k_bytes, have_ws, nxcd, per)
    nk, names = s["nk"], set()
    if s["total"] < nxcd:
        names.add("total < nxcd")
    for _, tp in pops:
        n_whole = tp["full"] * per + (tp["rem"] if tp["split"] == 1 and tp["cut"] == 1 else 0)
        if n_whole:
            names.add("main: whole, nk = 1" if nk == 1 else "main: whole, nk = 2" if nk == 2 else f"main: whole, nk {'even' if nk % 2 == 0 else 'odd'} >= 3")
        if tp["split"] > 1:
            base, extra = divmod(nk, tp["split"])
            names.add(f"reduce: split {tp['split']}")
            names.update(f"piece of {n}" for n in ({base, base + 1} if extra else {base}) if n <= 3)
            names.update({"extra != 0"} if extra else set())
            names.update({"whole tiles, then k-range pieces"} if tp["full"] else set())
        if tp["cut"] > 1:
            names.add(f"second: nk = {nk}" if nk < 3 else f"second: nk = {nk % 3} mod 3")
            names.update({"whole tiles, then column pieces"} if tp["full"] else set())
        if not have_ws and tp["rem"] and tp["rem"] * 4 > per:
            assert tp["split"] == 1 and tp["cut"] == 1
            names.add("left-over tiles whole: rem * 4 > per")
    return names


def meant_path(layout, nk, have_ws):
    """What a case is there for (from the layout table of the docstring, not from the plan code)."""
    if layout in ("L1", "L2"):          # one left-over tile per XCD (L2: two on XCD 0): nk / 2 pieces of 2 while they fit its 32 CUs
        if have_ws and nk >= 4:
            return {f"reduce: split {min(32 if layout == 'L1' else 16, nk // 2)}"} | ({"piece of 2"} if nk <= 32 else set())
        return {f"second: nk = {nk}" if nk < 3 else f"second: nk = {nk % 3} mod 3"}
    if layout == "L3":
        return {f"reduce: split {min(3, nk // 2)}"} if have_ws and nk >= 4 else {"main: whole, nk = 2" if nk == 2 else "main: whole, nk even >= 3"}
    return {"whole tiles, then k-range pieces"} if have_ws and nk >= 4 else {"whole tiles, then column pieces"}


REACHABLE = ["main: whole, nk = 2", "main: whole, nk even >= 3",
             "piece of 2", "piece of 3", "extra != 0",
             "reduce: split 2", "reduce: split 3", "reduce: split 4", "reduce: split 5", "reduce: split 32",
             "second: nk = 2", "second: nk = 0 mod 3", "second: nk = 1 mod 3", "second: nk = 2 mod 3",
             "total < nxcd", "whole tiles, then k-range pieces", "whole tiles, then column pieces", "left-over tiles whole: rem * 4 > per"]
# the issue's list also names these; K * esz % 256 == 0 keeps every launch from them (module docstring)
UNREACHABLE = ["main: whole, nk = 1", "main: whole, nk odd >= 3", "second: nk = 1"]


def reached(cases):
    names = set()
    for _, fp8, m, n, u in cases:
        for have_ws in (True, False):
            names |= paths_of(m, n, k_bytes_of(fp8, u), have_ws)
    return names


def test_every_path_is_named():
    """The GPU case list reaches every path a launch can take (256 CUs), in bf16; in e4m3 all but split 32; and a case list without the
    carrier of a path does not (so that an edit of the lists cannot drop one silently)."""
    cases = list(gpu_cases())
    bf16, fp8 = [c for c in cases if not c[1]], [c for c in cases if c[1]]
    got = reached(bf16)
    assert not [n for n in REACHABLE if n not in got], [n for n in REACHABLE if n not in got]
    got8 = reached(fp8)
    assert not [n for n in REACHABLE if n not in got8 and n != "reduce: split 32"]
    assert not (got | got8) & set(UNREACHABLE), "an odd or single k-step in a whole tile: K * esz % 256 != 0 ?"
    for layout, fp8_, m, n, u in cases:          # each case is meant for a path: it reaches it
        for have_ws in (True, False):
            assert meant_path(layout, k_bytes_of(fp8_, u) // 128, have_ws) <= paths_of(m, n, k_bytes_of(fp8_, u), have_ws), (layout, fp8_, m, u, have_ws)
    # the carriers: without them the list fails
    without = {"L1": {"total < nxcd", "reduce: split 32"},
               "L3": {"left-over tiles whole: rem * 4 > per", "piece of 3", "extra != 0"},
               "L4": {"whole tiles, then k-range pieces", "whole tiles, then column pieces"}}
    for layout, names in without.items():
        assert names.isdisjoint(reached([c for c in bf16 if c[0] != layout])), layout
    assert "reduce: split 32" not in reached([c for c in bf16 if c[4] != U_L1_LONG])
    assert "second: nk = 2" not in reached([c for c in cases if k_bytes_of(c[1], c[4]) != 256])
    assert "second: nk = 0 mod 3" not in reached([c for c in bf16 if c[4] % 3])


def test_header_shapes_have_even_k_step_counts():
    """K * esz % 256 == 0 is checked on the host before any launch: a whole tile never has 1 or an odd number of k-steps."""
    from fairygen_amd import hip as h
    lib, p16 = h.load(), ctypes.c_void_p(16)
    for k in (64, 192, 320):          # 1, 3, 5 k-steps of bf16
        assert lib.fg_gemm_epilogue_bf16_s(p16, 512, p16, p16, p16, 256, 8, 256, k, 0, None, 1, 0, 0, None, p16, 0, None) == -1
        assert b"K %" in lib.fg_last_error()
    for k in (128, 384, 640):         # ... of e4m3
        assert lib.fg_gemm_fp8_bf16_s(p16, 1024, p16, p16, p16, p16, 256, 8, 256, k, 0, None, 1, 0, 0, None, p16, 0, None) == -1
        assert b"K %" in lib.fg_last_error()
    for fp8 in (False, True):
        for u in (U_FP8 if fp8 else U_BF16 + (U_L1_LONG,)):
            assert k_bytes_of(fp8, u) % 256 == 0


SWEEP_NK = tuple(range(1, 12)) + (64,)
SWEEP = [(1, 1, 1), (1, 1, 3), (1, 1, 8), (2, 257, 1), (2, 257, 3), (2, 257, 8), (3, 700, 1), (3, 700, 3), (3, 700, 8),
         (10, 2309, 1), (10, 2309, 8), (33, 8198, 8)]          # tiles_m, M, tiles_n (the two largest row counts: not at every width)


@pytest.mark.parametrize("tiles_m,M,tiles_n", SWEEP)
def test_scalar_record_program_on_small_plans(tiles_m, M, tiles_n):
    """emit_make_record, interpreted, against the Python plan for every unit of every XCD, and every tile covered exactly once: 1 .. 11
    and 64 k-steps (odd ones too: the record program does not know what the header rejects), with and without scratch; short launches
    take the scratch, so these are the record programs of k-range pieces with base 2 or 3 and extra != 0."""
    assert (M + 255) // 256 == tiles_m and M % 256
    seen = set()
    for nk in SWEEP_NK:
        for have_ws in (True, False):
            s = U.check_records(M, tiles_n * 256, 128 * nk, 8, 32, have_ws)
            assert s["have_ws"] == have_ws and s["m_last"] == M - 1
            seen |= {(pl["split"], pl["base"], pl["extra"] != 0) for pl in s["plans"] if pl["split"] > 1}
    assert any(base == 2 for _, base, _ in seen) and all(base >= 2 for _, base, _ in seen), seen
    if (tiles_m, tiles_n) == (1, 1):          # split = min(32, nk / 2): 2 + 2 + 1 extra at nk = 5
        assert (2, 2, True) in seen and (32, 2, False) in seen, seen
    if (tiles_m, tiles_n) == (10, 8):         # split = min(3, nk / 2): 3 + 3 + 3 at nk = 9, 4 + 3 + 3 at nk = 10
        assert (3, 3, False) in seen and (3, 3, True) in seen, seen


def test_scalar_record_program_on_one_xcd():
    for M, N in ((1, 256), (257, 768), (2309, 2048)):
        for nk in SWEEP_NK:
            for have_ws in (True, False):
                U.check_records(M, N, 128 * nk, 1, 40, have_ws)


# ------------------------------------------------------------------------------------------------------ B. on the GPU
@pytest.fixture(scope="module")
def state(hip):
    """One scheduler block and scratch for the module: every launch here is an _s launch on it, and it is never reset."""
    return hip.gemm_state("cuda")


def device_layout():
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    nxcd = 8 if cus >= 64 and cus % 8 == 0 else 1          # device_grid() of csrc/dit_gemm.hip
    return nxcd, cus // nxcd


def _same(got, want, what):
    """torch.equal (on the device where both are there); on a difference _assert_same names the places."""
    if got.device == want.device and got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want):
        return
    _assert_same(got, want, what)


def _expected(a, w, bias, scale, res, table, first, what):
    """(y, x + gate y, x + y) as bf16 integers (asserted <= 256).  M < LARGE: the fp64 product on the CPU, all rows.  Larger: torch's fp32
    matmul of the same integers on the device — exact on these operands in any summation order — cross-checked against the CPU's fp64
    product on the first, middle and last 300 rows."""
    M = a.shape[0]
    if M < LARGE:
        return tuple(_exact_int(t, what).cuda() for t in _gemm_expected(a, w, bias, scale, res, table, first, torch.arange(M), torch.float64))
    y = a.float() @ w.float().T
    y = (y if scale is None else scale * y) + bias.float()
    gate = table[(torch.arange(M, device=a.device) >= first).long(), 5].float()
    dev32 = (y, res.float() + gate * y, res.float() + y)
    rows = torch.cat([torch.arange(0, 300), torch.arange(M // 2 - 150, M // 2 + 150), torch.arange(M - 300, M)])
    for t32, t64 in zip(dev32, _gemm_expected(a, w, bias, scale, res, table, first, rows, torch.float64)):
        assert torch.equal(t32[rows.cuda()].double().cpu(), t64), what + ": the device's fp32 product is not the fp64 product on the sampled rows"
    return tuple(_exact_int(t, what) for t in dev32)


def _gelu_check(got, y16, what):
    if got.numel() <= 1 << 22:
        return assert_gelu_of(got, y16, what)
    # large outputs: GELU of an integer in [-256, 256] is one of 513 values — the output is a function of y alone (every element, on the
    # device), and the criterion itself is held on the first, middle and last 300 rows
    idx = (y16.float() + 256).long().view(-1)
    table = torch.zeros(513, dtype=BF16, device=got.device).scatter_(0, idx, got.reshape(-1))
    assert torch.equal(table[idx].view_as(got), got), what + ": equal y, different GELU outputs"
    M = got.shape[0]
    rows = torch.cat([torch.arange(0, 300), torch.arange(M // 2 - 150, M // 2 + 150), torch.arange(M - 300, M)]).cuda()
    assert_gelu_of(got[rows], y16[rows], what)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@gpu
@pytest.mark.parametrize("layout,fp8,M,N,u", list(gpu_cases()), ids=lambda v: str(v))
def test_gemm_shape(hip, state, layout, fp8, M, N, u):
    """One (layout, type, K) with and without the k-split scratch: modes 0 (twice on the block, no reset between), 2 (the gate class
    changing inside the last row tile; M = 1: first_rows 0 and 1), 3, 4; L1 / L2: A inside a NaN buffer; M < 3000: out with ldc > N
    between guard columns and bands (modes 0, 3, raw entry point); L3 / L4 at some K: one workgroup per XCD.  All torch.equal."""
    sched, scratch = state
    K, k_bytes = 128 * u, k_bytes_of(fp8, u)
    nk = k_bytes // 128
    nxcd, per = device_layout()
    a, w, bias, scale, res, table = _gemm_operands(M, K, N, "cuda", fp8)
    firsts = (0, 1) if M == 1 else (_class_change(M),)
    what = f"{layout} {'e4m3' if fp8 else 'bf16'} gemm {M}x{K}x{N} (nk {nk})"
    want = {first: _expected(a, w, bias, scale, res, table, first, what) for first in firsts}
    y16, _, plain16 = want[firsts[0]]
    if fp8:
        a, w = a.to(F8), w.to(F8)
        assert torch.equal(a.to(BF16).to(F8).view(torch.uint8), a.view(torch.uint8))

    def gemm(x, **kw):
        return hip.gemm_fp8(x, scale, w, bias, sched=sched, **kw) if fp8 else hip.gemm_epilogue(x, w, bias, sched=sched, **kw)

    for have_ws in (True, False):
        tag = what + (", scratch" if have_ws else ", no scratch")
        print(tag + ": " + describe_plan(M, N, k_bytes, have_ws, nxcd, per))
        if (nxcd, per) == (8, 32):
            assert meant_path(layout, nk, have_ws) <= paths_of(M, N, k_bytes, have_ws), tag
        ws = scratch if have_ws else False
        for launch in range(2):
            _same(gemm(a, workspace=ws), y16, f"{tag}, mode 0, launch {launch}")
        for first in firsts:
            got = gemm(a, workspace=ws, out=res.clone(), residual=True, mod=hip.ModTable(table, first), gate_idx=5)
            _same(got, want[first][1], f"{tag}, mode 2, first_rows {first}")
        _same(gemm(a, workspace=ws, out=res.clone(), residual=True), plain16, tag + ", mode 3")
        _gelu_check(gemm(a, workspace=ws, act="gelu_tanh"), y16, tag + ", mode 4")
        if layout in ("L1", "L2"):          # the slices behind K are NaN: one that reaches an MFMA shows
            wide = torch.full((M, K + 128), 0x7F, dtype=torch.uint8, device="cuda").view(F8) if fp8 else \
                torch.full((M, K + 128), float("nan"), dtype=BF16, device="cuda")
            wide[:, 64:64 + K] = a
            got = gemm(wide[:, 64:64 + K], workspace=ws)
            assert torch.isfinite(got.float()).all(), tag + ": NaN from behind K"
            _same(got, y16, tag + ", lda = K + 128 over NaN")
        if M < LARGE:
            for mode, start, expect in ((0, torch.empty_like(res), y16), (3, res, plain16)):
                g = Guards()
                c = g.embed(start, 16, 256, 8, 24)
                tail = (_ptr(bias), _ptr(c), c.stride(0), M, N, K, mode, None, 1, N, 0, _ptr(scratch if have_ws else None), _ptr(sched), 0,
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                if fp8:
                    hip._call("fg_gemm_fp8_bf16_s", _ptr(a), a.stride(0), _ptr(scale), _ptr(w), *tail)
                else:
                    hip._call("fg_gemm_epilogue_bf16_s", _ptr(a), a.stride(0), _ptr(w), *tail)
                g.check(f"{tag}, mode {mode}, ldc = N + 32")
                _same(c, expect, f"{tag}, mode {mode}, ldc = N + 32")
        if layout in ("L3", "L4") and u in U_ONE_WORKGROUP_PER_XCD[fp8]:          # one workgroup walks an XCD's whole list, in order
            for launch in range(2):
                _same(gemm(a, workspace=ws, workgroups=8), y16, f"{tag}, workgroups 8, launch {launch}")
                got = gemm(a, workspace=ws, workgroups=8, out=res.clone(), residual=True, mod=hip.ModTable(table, firsts[0]), gate_idx=5)
                _same(got, want[firsts[0]][1], f"{tag}, workgroups 8, mode 2, launch {launch}")
        assert not sched.any(), tag + ": the cursors were not cleared"

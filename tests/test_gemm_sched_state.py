"""Caller-owned scheduler state of the persistent GEMM (fg_gemm_sched_bytes / fg_gemm_sched_reset / fg_gemm_epilogue_bf16_s /
fg_gemm_fp8_bf16_s, include/fairygen_hip.h): the launch whose only state is a block the caller passed in — stream-ordered from the
first call on a stream on, and therefore capturable into a graph.

Every GPU comparison here is torch.equal against the entry points without the block argument (fg_gemm_epilogue_bf16,
fg_gemm_fp8_bf16) on the same inputs: those are checked against the oracle by tests/test_hip_kernels.py (test_gemm_epilogue*,
test_gemm_fp8), and the two forms run the same kernel on the same unit plan, so no tolerance is involved.  Shapes are the ones of
those tests."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO, seeded
from fairygen_amd import hip

NEW_SYMBOLS = ["fg_gemm_sched_bytes", "fg_gemm_sched_reset", "fg_gemm_epilogue_bf16_s", "fg_gemm_fp8_bf16_s"]


# ------------------------------------------------------------------------------------------------ host side (no device)
def test_sched_block_size():
    n = hip.load().fg_gemm_sched_bytes()
    assert n > 0 and n % 16 == 0 and n >= 17 * 4          # 16 unit cursors + the done counter


def test_new_entry_points_declared_listed_and_exported():
    header = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    declared = set(re.findall(r"\b(fg_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(hip.library_path())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fairygen_hip.h"
        assert name in hip.EXPORTED_SYMBOLS, f"{name} is not in hip.EXPORTED_SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert hip.ABI_VERSION >= 6 and hip.load().fg_version() == hip.ABI_VERSION


def test_s_entry_points_validate_sched_and_workgroups():
    """The argument checks of the _s forms run on the host before any launch (every call below has exactly one bad argument)."""
    lib = hip.load()
    p16 = ctypes.c_void_p(16)
    bf16 = lambda sched, wg=0, N=256: lib.fg_gemm_epilogue_bf16_s(      # noqa: E731
        p16, 256, p16, p16, p16, N, 512, N, 256, 0, None, 1, 0, 0, None, sched, wg, None)
    fp8 = lambda sched, wg=0, N=256: lib.fg_gemm_fp8_bf16_s(      # noqa: E731
        p16, 256, p16, p16, p16, p16, N, 512, N, 256, 0, None, 1, 0, 0, None, sched, wg, None)
    for call in (bf16, fp8):
        assert call(None) == -1 and b"sched" in lib.fg_last_error()
        assert call(ctypes.c_void_p(24)) == -1 and b"sched" in lib.fg_last_error()          # 8-byte aligned only
        assert call(ctypes.c_void_p(4)) == -1 and b"sched" in lib.fg_last_error()
        for wg in (7, 12, -8, 264, 1 << 20):          # not a multiple of the XCD count / negative / more than one per CU
            assert call(p16, wg) == -1 and b"workgroups" in lib.fg_last_error(), wg
        assert call(p16, 0, N=250) == -1 and b"N % 256" in lib.fg_last_error()          # the checks of the forms without a block, as before
    assert b"fg_gemm_fp8_bf16_s" in lib.fg_last_error()
    assert lib.fg_gemm_sched_reset(None, None) == -1 and b"sched" in lib.fg_last_error()
    assert lib.fg_gemm_sched_reset(ctypes.c_void_p(8), None) == -1 and b"sched" in lib.fg_last_error()
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        hip.gemm_state("cpu")
    with pytest.raises(hip.HipLibraryError):
        hip.gemm_sched_reset(torch.zeros(256, dtype=torch.uint8))


def test_s_launch_path_source_has_no_hidden_state():
    """csrc/dit_gemm.hip marks what a fg_gemm_*_s call runs (FG-GEMM-S-PATH-BEGIN / -END): nothing in there allocates, synchronises
    the host, takes a lock or keeps a table; the per-stream table of the two older entry points lives outside."""
    src = open(os.path.join(REPO, "fairygen_amd", "csrc", "dit_gemm.hip")).read()
    regions = re.findall(r"FG-GEMM-S-PATH-BEGIN(.*?)FG-GEMM-S-PATH-END", src, flags=re.S)
    assert regions and src.count("FG-GEMM-S-PATH-BEGIN") == src.count("FG-GEMM-S-PATH-END") == len(regions)
    path = "\n".join(regions)
    for needed in ("GemmCall::check", "GemmCall::enqueue", "fg_gemm_sched_reset", "fg_gemm_epilogue_bf16_s", "fg_gemm_fp8_bf16_s", "hipLaunchKernelGGL"):
        assert needed in path, f"{needed} is not inside the marked path"
    for pattern in (r"hipMalloc", r"hipFree", r"hipMemset\s*\(", r"hipMemcpy\s*\(", r"hipDeviceSynchronize", r"hipStreamSynchronize", r"hipEventSynchronize",
                    r"std::mutex", r"lock_guard", r"unique_lock", r"\bstatic\b[^;=()]*\[", r"stream_cursors"):
        found = re.search(pattern, path)
        assert found is None, f"the _s launch path contains {found.group(0)!r}"
    outside = src
    for r in regions:
        outside = outside.replace(r, "")
    assert "stream_cursors" in outside and "hipMalloc" in outside          # the documented exception is still there, outside the path


# ------------------------------------------------------------------------------------------------------------ on the GPU
def dev(t):
    return t.to("cuda")


def old_form(fp8, x2, sc, w, b, out, mode, mod=None, gate_idx=None, ws=None):
    """fg_gemm_epilogue_bf16 / fg_gemm_fp8_bf16 (the library's own per-stream block), in place on `out`."""
    (m, k), n = x2.shape, w.shape[0]
    gate, rows, ld, first = (mod.vec(gate_idx), mod.mod_rows, mod.ld, mod.first_rows) if mode == 2 else (None, 1, n, 0)
    tail = (hip._ptr(b), hip._ptr(out), n, m, n, k, mode, gate, rows, ld, first, hip._ptr(ws), hip._stream(x2))
    if fp8:
        hip._call("fg_gemm_fp8_bf16", hip._ptr(x2), x2.stride(0), hip._ptr(sc), hip._ptr(w), *tail)
    else:
        hip._call("fg_gemm_epilogue_bf16", hip._ptr(x2), x2.stride(0), hip._ptr(w), *tail)
    return out


def operands(M, K, N, seed, fp8=False):
    x, w, b = dev(seeded((M, K), seed, scale=0.5)), dev(seeded((N, K), seed + 1, scale=0.05)), dev(seeded((N,), seed + 2, scale=0.2))
    if not fp8:
        return x, None, w, b
    xq, sc = hip.fp8_quant_rows(x)
    return xq, sc, w.to(torch.float8_e4m3fn), b


def new_form(fp8, x, sc, w, b, **kw):
    return hip.gemm_fp8(x, sc, w, b, **kw) if fp8 else hip.gemm_epilogue(x, w, b, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,fp8,use_ws", [
    (600, 14336, 3072, False, True),       # ffn.2's reduction length: the left-over tiles as k-range pieces + the reduce kernel
    (4200, 512, 4096, False, True),        # a full round + left-over tiles, short launch: k-split as well
    (4200, 512, 4096, False, False),       # ... and without scratch: 64-column pieces (second body)
    (10500, 128, 2048, False, False),      # left-over tiles not cut at all, 4 rows in the last row tile
    (600, 14336, 3072, True, True),        # e4m3, k-range pieces
    (4200, 1024, 4096, True, False)])      # e4m3, column pieces
def test_s_forms_equal_the_forms_without_a_block(M, K, N, fp8, use_ws):
    """Modes 0, 2 (one- and two-row gate table, the row class changing inside a tile), 3, 4: same bits from both forms."""
    x, sc, w, b = operands(M, K, N, 301, fp8)
    res = dev(seeded((M, N), 304))
    table = dev(seeded((2, 6, N), 305))
    mod2, mod1 = hip.ModTable(table, 130), hip.ModTable(table[:1].contiguous())
    ws = torch.empty(hip.load().fg_gemm_workspace_bytes(M, N, K), dtype=torch.uint8, device="cuda") if use_ws else None
    cases = [(0, None, None, {}), (2, mod1, 2, dict(residual=True, mod=mod1, gate_idx=2)), (2, mod2, 5, dict(residual=True, mod=mod2, gate_idx=5)),
             (3, None, None, dict(residual=True)), (4, None, None, dict(act="gelu_tanh"))]
    for mode, mod, gate_idx, kw in cases:
        want = old_form(fp8, x, sc, w, b, res.clone() if mode in (2, 3) else torch.empty_like(res), mode, mod, gate_idx, ws)
        got = new_form(fp8, x, sc, w, b, out=res.clone() if mode in (2, 3) else None, workspace=use_ws, **kw)
        assert torch.isfinite(want.float()).all()
        assert torch.equal(got, want), f"mode {mode}, gate rows {mod.mod_rows if mod else 0}"
    if use_ws:          # the scratch really took part: the k-split result is another summation order than the single accumulation
        y_ws, y_nows = new_form(fp8, x, sc, w, b), new_form(fp8, x, sc, w, b, workspace=False)
        assert fp8 or K < 6144 or not torch.equal(y_ws, y_nows)          # (asserted where test_gemm_epilogue_ksplit asserts it)
        assert torch.equal(y_nows, old_form(fp8, x, sc, w, b, torch.empty_like(res), 0, ws=None))


@pytest.mark.gpu
def test_first_call_on_a_fresh_stream_is_capturable():
    """A stream nothing was ever launched on; on it, inside a stream capture: reset + the three dependent GEMMs of a block (qkv-shaped
    mode 0; o-shaped mode 2 from a column slice of the qkv buffer into the residual stream; ffn.2-shaped mode 2, K = 14 336 with the
    k-split scratch, into the same residual stream), block and scratch from hip.gemm_state.  One linear chain; three replays with fresh
    inputs copied into the static buffers, each equal to the eager result bit for bit."""
    M, C, F = 600, 3072, 14336
    wqkv, bqkv = dev(seeded((3 * C, C), 311, scale=0.05)), dev(seeded((3 * C,), 312, scale=0.2))
    wo, bo = dev(seeded((C, C), 313, scale=0.05)), dev(seeded((C,), 314, scale=0.2))
    w2, b2 = dev(seeded((C, F), 315, scale=0.02)), dev(seeded((C,), 316, scale=0.2))
    mod = hip.ModTable(dev(seeded((2, 6, C), 317)), 130)

    def block(x, h, res, qkv, **state):
        hip.gemm_epilogue(x, wqkv, bqkv, out=qkv, **state)
        hip.gemm_epilogue(qkv[:, :C], wo, bo, out=res, residual=True, mod=mod, gate_idx=2, **state)
        hip.gemm_epilogue(h, w2, b2, out=res, residual=True, mod=mod, gate_idx=5, **state)

    inputs = [(dev(seeded((M, C), 320 + 3 * i, scale=0.5)), dev(seeded((M, F), 321 + 3 * i, scale=0.5)), dev(seeded((M, C), 322 + 3 * i))) for i in range(4)]
    eager = []
    for x, h, res in inputs:
        res, qkv = res.clone(), torch.empty((M, 3 * C), dtype=torch.bfloat16, device="cuda")
        block(x, h, res, qkv)
        eager.append((qkv, res))
    assert not torch.equal(eager[0][1], eager[1][1])
    sx, sh, sres = (torch.empty_like(t) for t in inputs[0])
    sqkv = torch.empty((M, 3 * C), dtype=torch.bfloat16, device="cuda")
    sched, ws = hip.gemm_state("cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()          # never launched on eagerly
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        hip.gemm_sched_reset(sched)
        block(sx, sh, sres, sqkv, sched=sched, workspace=ws)
    for i in (1, 2, 3):
        for static, fresh in zip((sx, sh, sres), inputs[i]):
            static.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sqkv, eager[i][0]), f"replay {i}: qkv"
        assert torch.equal(sres, eager[i][1]), f"replay {i}: residual stream"
    assert not sched.any()          # every launch leaves the block in its initial state


@pytest.mark.gpu
def test_reset_repairs_a_block_left_dirty():
    """What a launch that died leaves behind is produced from the host (a non-initial pattern); fg_gemm_sched_reset makes the block
    usable again.  Nothing is launched on the dirty block."""
    M, K, N = 4200, 512, 4096
    x, _, w, b = operands(M, K, N, 331)
    want = old_form(False, x, None, w, b, torch.empty((M, N), dtype=torch.bfloat16, device="cuda"), 0)
    sched, ws = hip.gemm_state("cuda")
    assert sched.numel() == hip.load().fg_gemm_sched_bytes() and not sched.any()
    sched.fill_(0xA5)
    hip.gemm_sched_reset(sched)
    assert not sched.any()
    for rep in range(2):
        assert torch.equal(hip.gemm_epilogue(x, w, b, sched=sched, workspace=ws), old_form(False, x, None, w, b, torch.empty_like(want), 0, ws=ws)), rep
        assert torch.equal(hip.gemm_epilogue(x, w, b, sched=sched, workspace=False), want), rep
    assert not sched.any()
    # the host's own block of a (device, stream): a launch that raised marks it, the next use resets it first
    key = hip._gemm_key(x)
    hip.gemm_epilogue(x, w, b)
    with pytest.raises(hip.HipLibraryError, match="workgroups"):
        hip.gemm_epilogue(x, w, b, workgroups=7)
    assert key in hip._gemm_sched_dirty
    hip._gemm_sched[key].fill_(0x5A)
    assert torch.equal(hip.gemm_epilogue(x, w, b, workspace=False), want)
    assert key not in hip._gemm_sched_dirty and not hip._gemm_sched[key].any()


@pytest.mark.gpu
def test_seventy_streams_in_sequence(monkeypatch):
    """70 short-lived streams, one after the other, one small GEMM each: same bits everywhere; every launch is the _s entry point
    (counted at hip._call: the library allocates nothing), and device memory grows by no more than the blocks and scratch the host
    keeps per (device, stream)."""
    M, K, N = 700, 256, 768
    x, _, w, b = operands(M, K, N, 341)
    want = hip.gemm_epilogue(x, w, b)
    names = []
    real_call = hip._call

    def counting_call(name, *args):
        names.append(name)
        return real_call(name, *args)
    monkeypatch.setattr(hip, "_call", counting_call)

    def held():          # bytes as the caching allocator counts them (512-byte granules)
        return sum((t.numel() * t.element_size() + 511) // 512 * 512 for d in (hip._gemm_workspace, hip._gemm_sched) for t in d.values())
    keys_before = set(hip._gemm_workspace) | set(hip._gemm_sched)
    torch.cuda.synchronize()
    held0, allocated0 = held(), torch.cuda.memory_allocated()
    try:
        for i in range(70):
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                y = hip.gemm_epilogue(x, w, b)
            stream.synchronize()
            assert torch.equal(y, want), f"stream {i}"
            del y, stream
        torch.cuda.synchronize()
        grown, kept = torch.cuda.memory_allocated() - allocated0, held() - held0
        print(f"70 streams: memory_allocated grew by {grown} bytes, the host keeps {kept} bytes more in {len(hip._gemm_sched)} blocks")
        assert grown <= kept
        assert names.count("fg_gemm_epilogue_bf16_s") == 70 and "fg_gemm_epilogue_bf16" not in names
        assert set(names) <= {"fg_gemm_epilogue_bf16_s", "fg_gemm_sched_reset"} and names.count("fg_gemm_sched_reset") <= 70
    finally:          # what this test made the host keep goes again
        for d in (hip._gemm_workspace, hip._gemm_sched):
            for key in set(d) - keys_before:
                del d[key]


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(4200, 512, 4096), (600, 14336, 3072), (700, 256, 768), (27280, 256, 3072)])
def test_workgroups_per_call(M, K, N):
    """workgroups = 8, 64, 248 per call give the bits of 0 (one per CU), the process-wide fg_gemm_debug_grid staying at 0: the units
    are fixed by the shape, fewer workgroups only take more of them each."""
    lib = hip.load()
    assert lib.fg_gemm_debug_grid(0) == 0
    x, _, w, b = operands(M, K, N, 351)
    res = dev(seeded((M, N), 354))
    mod = hip.ModTable(dev(seeded((2, 6, N), 355)), 130)
    xq, sc = hip.fp8_quant_rows(x)
    w8 = w.to(torch.float8_e4m3fn)

    def run(wg):
        return (hip.gemm_epilogue(x, w, b, workgroups=wg), hip.gemm_epilogue(x, w, b, out=res.clone(), residual=True, mod=mod, gate_idx=2, workgroups=wg),
                hip.gemm_epilogue(x, w, b, act="gelu_tanh", workgroups=wg), hip.gemm_fp8(xq, sc, w8, b, workgroups=wg) if K % 256 == 0 else None)
    want = run(0)
    assert torch.isfinite(want[0].float()).all()
    assert torch.equal(want[0], old_form(False, x, None, w, b, torch.empty_like(res), 0, ws=hip._gemm_ws(x, M, N, 2 * K, True)))
    for wg in (8, 64, 248):
        for rep in range(2):
            for i, (g, wnt) in enumerate(zip(run(wg), want)):
                assert wnt is None or torch.equal(g, wnt), f"workgroups {wg}, launch {rep}, output {i}"
    assert all(wnt is None or torch.equal(g, wnt) for g, wnt in zip(run(0), want))

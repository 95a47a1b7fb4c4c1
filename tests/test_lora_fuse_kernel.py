"""fg_lora_fuse_bf16 (one adapter folded into one Linear's weight, `hot_backend="fused"`) through the C ABI, against
GeneralLoRALoader.fuse_lora_to_base_model run on the CPU in bf16 on a one-Linear module: w' = bf16(w + bf16(alpha * bf16(B A))).

Exact case: operands for which every product, every partial sum over the rank and alpha * d are exactly representable, so no summation
order can change a bit and the kernel must be bit-equal to the reference.  Random case: against an fp64 evaluation with the three
roundings applied, max|hip - f64| <= 2 * max|cpu_bf16 - f64|, and every element within 1 bf16 ulp of the CPU reference's.  Layout:
in place, into a row range of a wider and taller buffer whose guard rows and columns keep their poison, and the e4m3 copy byte for byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch import nn

from conftest import seeded
from fairygen_amd import hip
from fairygen_amd.lora import GeneralLoRALoader

BF16 = torch.bfloat16


class _OneLinear(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.lin = nn.Linear(w.shape[1], w.shape[0], bias=False, dtype=w.dtype)
        with torch.no_grad():
            self.lin.weight.copy_(w)


def _cpu_reference(w, a, b, alpha):
    """The reference's own code path on the CPU, in bf16."""
    m = _OneLinear(w)
    GeneralLoRALoader(device="cpu", torch_dtype=BF16).fuse_lora_to_base_model(m, {"lin.lora_A.weight": a, "lin.lora_B.weight": b}, alpha=alpha)
    return m.lin.weight.detach().clone()


def _f64_reference(w, a, b, alpha):
    """fp64 arithmetic, rounded to bf16 at the reference's three points; alpha as the fp32 value a bf16 tensor op multiplies by."""
    def rb(t):
        return t.to(torch.float32).to(BF16).double()
    d = rb(b.double() @ a.double())
    d = rb(float(np.float32(alpha)) * d)
    return rb(w.double() + d)


def _ulp_distance(x, y):
    """Distance in representable bf16 values (sign-magnitude bits mapped to one ordered integer line)."""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(x) - line(y)).abs()


def _padded(a, b, r_pad):
    """The kernel's operands: A^T (K, R) and B (N, R) with zero columns up to the padded rank."""
    rank, k = a.shape
    a_t, b_p = torch.zeros((k, r_pad), dtype=BF16), torch.zeros((b.shape[0], r_pad), dtype=BF16)
    a_t[:, :rank], b_p[:, :rank] = a.T, b
    return a_t.cuda(), b_p.cuda()


@functools.lru_cache(maxsize=None)
def _exact_case(n, k, r, alpha):
    """A in {-1, 0, 1} * 2^-3, B in {-2 .. 2} * 2^-2: products are integers in [-2, 2] times 2^-5, and the sum of their magnitudes over the
    rank stays <= 256 quanta, so every partial sum in any order is an integer of at most 9 bits times 2^-5: exact in bf16 and fp32."""
    g = torch.Generator("cpu").manual_seed(1000 + n + k + r)
    a = (torch.randint(-1, 2, (r, k), generator=g).float() * 2.0 ** -3).to(BF16)
    b = (torch.randint(-2, 3, (n, r), generator=g).float() * 2.0 ** -2).to(BF16)
    w = seeded((n, k), 7 + n, scale=2.0)
    return w, a, b, _cpu_reference(w, a, b, alpha)


@functools.lru_cache(maxsize=None)
def _random_case(n, k, rank, alpha):
    a, b, w = seeded((rank, k), 31 + rank, scale=0.02), seeded((n, rank), 32 + rank, scale=0.02), seeded((n, k), 33, scale=0.02)
    return w, a, b, _cpu_reference(w, a, b, alpha), _f64_reference(w, a, b, alpha)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.5, 1])
@pytest.mark.parametrize("n,k,r", [(128, 192, 32), (64, 64, 128)])
def test_exact_operands_bit_equal_to_reference(n, k, r, alpha):
    w, a, b, want = _exact_case(n, k, r, alpha)
    # the property the case rests on, in fp64: no rounding anywhere before the final add
    quantum = 2.0 ** -5
    mags = (b.double().abs() @ a.double().abs()) / quantum
    assert mags.max().item() <= 256 and torch.equal(mags, mags.round()), "partial sums must stay exact 9-bit integers of 2^-5"
    d = b.double() @ a.double()
    assert torch.equal(d.float().to(BF16).double(), d) and torch.equal((alpha * d).float().to(BF16).double(), alpha * d)
    assert torch.equal(want.double(), _f64_reference(w, a, b, alpha)), "the CPU reference itself must be exact on these operands"
    a_t, b_p = _padded(a, b, r)
    got = hip.lora_fuse(w.cuda(), a_t, b_p, alpha)
    torch.cuda.synchronize()
    assert not torch.equal(got.cpu(), w) and torch.equal(got.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("rank,r_pad", [(24, 32), (96, 96)])
def test_random_operands_against_f64(rank, r_pad):
    n, k, alpha = 192, 320, 0.7
    w, a, b, cpu, f64 = _random_case(n, k, rank, alpha)
    a_t, b_p = _padded(a, b, r_pad)
    got = hip.lora_fuse(w.cuda(), a_t, b_p, alpha).cpu()
    err_hip, err_cpu = (got.double() - f64).abs().max().item(), (cpu.double() - f64).abs().max().item()
    ulps = _ulp_distance(got, cpu)
    print(f"lora_fuse n={n} k={k} rank={rank} R={r_pad}: max|hip-f64|={err_hip:.3e} max|cpu-f64|={err_cpu:.3e} "
          f"differ from cpu: {(ulps > 0).sum().item()} of {ulps.numel()}, max {ulps.max().item()} ulp")
    assert err_hip <= 2 * err_cpu
    assert ulps.max().item() <= 1


@pytest.mark.gpu
def test_layouts_alias_row_range_and_e4m3_copy():
    n, k, rank, alpha = 192, 320, 24, 0.7
    w, a, b, cpu, _ = _random_case(n, k, rank, alpha)
    a_t, b_p = _padded(a, b, 32)
    first = hip.lora_fuse(w.cuda(), a_t, b_p, alpha, out=torch.empty((n, k), dtype=BF16, device="cuda")).cpu()
    assert _ulp_distance(first, cpu).max().item() <= 1
    # w_dst aliasing w_src: the default of the binding
    wd = w.cuda()
    assert hip.lora_fuse(wd, a_t, b_p, alpha) is wd and torch.equal(wd.cpu(), first)
    # a row range of a larger buffer with ld > K, bf16 and e4m3, guard rows above and below and guard columns to the right
    ld, top, rows = k + 64, 5, n + 11
    poison16 = torch.full((rows, ld), 0x7FC1, dtype=torch.int16).view(BF16)      # a NaN with a payload: compared as bits
    buf16 = poison16.cuda()
    poison8 = torch.full((rows, ld), 0xA5, dtype=torch.uint8)
    buf8 = poison8.cuda()
    src = w.cuda()
    hip.lora_fuse(src, a_t, b_p, alpha, out=buf16[top:top + n, :k], out_fp8=buf8.view(torch.float8_e4m3fn)[top:top + n, :k])
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), w), "w_src is only read when w_dst is another buffer"
    got16, got8 = buf16.cpu(), buf8.cpu()
    assert torch.equal(got16[top:top + n, :k], first)
    assert torch.equal(got8[top:top + n, :k], first.to(torch.float8_e4m3fn).view(torch.uint8))
    for got, poison in ((got16.view(torch.int16), poison16.view(torch.int16)), (got8, poison8)):
        assert torch.equal(got[:top], poison[:top]) and torch.equal(got[top + n:], poison[top + n:]) and torch.equal(got[:, k:], poison[:, k:]), "guards"


@pytest.mark.gpu
def test_e4m3_copy_outside_the_finite_range():
    """torch's cast to float8_e4m3fn does not saturate: up to 464 rounds to 448, above it the NaN byte with the sign.  A zero adapter leaves
    w as it is, so w' holds exactly these values."""
    w = seeded((64, 64), 5)
    w[0, :9] = torch.tensor([448.0, 450.0, 464.0, 466.0, -464.0, -466.0, 1000.0, -3.0e38, float("inf")]).to(BF16)
    a_t, b_p = torch.zeros((64, 32), dtype=BF16, device="cuda"), torch.zeros((64, 32), dtype=BF16, device="cuda")
    out8 = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    got = hip.lora_fuse(w.cuda(), a_t, b_p, 1.0, out_fp8=out8.view(torch.float8_e4m3fn)).cpu()
    assert torch.equal(got.view(torch.int16), w.view(torch.int16))
    want8 = w.to(torch.float8_e4m3fn).view(torch.uint8)
    assert want8[0, :9].tolist() == [0x7E, 0x7E, 0x7E, 0x7F, 0xFE, 0xFF, 0x7F, 0xFF, 0x7F]      # what the cast is documented to do
    assert torch.equal(out8.cpu(), want8)


def test_argument_checks():
    """fg_lora_fuse_bf16 checks its arguments on the host: FG_EINVAL with a message, nothing is launched."""
    lib = hip.load()
    p16 = ctypes.c_void_p(4096)

    def call(src=p16, dst=p16, dst8=None, a_t=p16, b=p16, n=128, k=192, r=32, ld_src=None, ld_dst=None):
        return lib.fg_lora_fuse_bf16(src, ld_src or k, dst, ld_dst or k, dst8, k, a_t, b, n, k, r, 1.0, None)
    assert call(src=ctypes.c_void_p(4104)) == -1 and b"16-byte aligned" in lib.fg_last_error()
    assert call(dst8=ctypes.c_void_p(4104)) == -1 and b"e4m3" in lib.fg_last_error()
    assert call(k=96) == -1 and b"K % 64" in lib.fg_last_error()
    assert call(n=96) == -1 and b"N % 64" in lib.fg_last_error()
    assert call(r=160) == -1 and b"rank" in lib.fg_last_error()
    assert call(r=48) == -1 and b"rank" in lib.fg_last_error()
    assert call(dst=ctypes.c_void_p(1 << 20), dst8=ctypes.c_void_p(4096 + 1024)) == -1 and b"e4m3 copy must not overlap" in lib.fg_last_error()
    assert call(a_t=None) == -1 and b"null pointer" in lib.fg_last_error()
    assert call(ld_dst=200) == -1 and b"overlap" in lib.fg_last_error()
    assert call(dst=ctypes.c_void_p(4096 + 64)) == -1 and b"overlap" in lib.fg_last_error()
    q = seeded((64, 64), 1)
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        hip.lora_fuse(q, q[:, :32].contiguous(), q[:, :32].contiguous())

"""fg_conv3d_cl_bf16 on its three kernels at every tap form, channel tail, pixel count and tile edge its index arithmetic distinguishes,
and fg_conv_pack_weight_bf16 on its own.

The older tests meet the convolution at a handful of hand-picked shapes (test_hip_kernels.py, test_exact_arithmetic.py,
test_buffer_contract.py) and inside whole-model goldens.  A wrong index in its addressing modes (causal history frames, spatial zero
padding, nearest-2x upsample, stride-2 downsample, channel-to-time interleave, residual add) gives a plausible picture, not a fault.

Data: dyadic operands, so that the criterion is torch.equal and both roundings of the epilogue are real.  x and the history frames in
{0, +-1} at the density min(1, 200 / (Cin kt ks ks)) of test_exact_arithmetic._conv_case; weights k / 16, k uniform in [-16, 16];
bias bf16(k / 64) in [-8, 8], k uniform on the even channels and, on the odd ones, odd with 3 < |k / 64| < 4: just below the binade at
4, from which on a 2^-6 step is no bf16 number, so that the short reductions too (Cin = 8 at 1x1x1, a 3x3 tap on one pixel, where |acc|
stays below 4) leave the bf16 grid at the first rounding; residual bf16(k / 64) in [-64, 64] (both multiples of 2^-6 and bf16 numbers,
asserted).  Every product and
partial sum is a multiple of 2^-4 below 2^10, so the fp32 accumulation is exact in any order, on any tile and with any k-step split;
acc + bias is a multiple of 2^-6 that often is no bf16 number, and bf16(acc + bias) + residual mostly is none either.  Expectation (the
header's formula): test_buffer_contract._conv_ref with bias in fp64, one rounding to bf16, + residual in fp64, one rounding to bf16.
The output buffer is passed as out=, pre-filled with NaN: a tile that is never written fails.

  kernel (csrc/vae_conv.hip)    swept (the lists are the constants below)                                    criterion
  conv3d_cl_kernel              TAPS: the four (kt, ks) forms x BORDER_THW (H = 1, W = 1, H = W = 1: every     torch.equal to the
  (128 x 128 tile)              neighbour of a 3x3 tap is padding) x history frames given / zero;              expectation, every
                                CIN_TAILS (Cin < 64, Cin % 64 in 8..56, several k-steps + a tail) x 3x3x3 and   element, padding
                                1x1x1; COUT_TAILS with a residual (cout_pad = 128 .. 640, a part-filled last    columns never written
                                cout tile, 384 and 640: multiples of 128 and not of 256);                       (the output is dense:
                                PIXELS_128: M = T H W in {1, 127, 128, 129, 255, 256, 257, 385}, tile           a column past Cout
                                boundaries inside an image row, exactly at a frame boundary, a tile over        would land in the next
                                three and more frames; upsample at UP_HW x T in {1, 3} x residual on / off;     pixel)
                                stride-2 at DOWN_HW x T in {1, 3} and (5, 5, 6); interleave at INTER_COUT
                                (halves of 96 and 192 fall inside a cout tile) x T in {1, 3} x INTER_TAPS x
                                residual on / off, at T = 3 two pixel tiles; the 63-workgroup side of the
                                dispatch edge
  conv3d_cl_256p_kernel         Cout = 2048: CIN_256P (every Cin % 64 in 8..56, one and two and three           the same
  (256 x 256, LDS-DMA)          k-steps) x 3x3x3 with history and 1x1x1; the four tap forms with history at
                                Cin = 72; PIXELS_256: M in {1793, 2047, 2048, 2049} and (15, 11, 11) whose
                                tiles span three frames; upsample + residual and stride-2 at Cin = 72 on
                                (2, 30, 30); interleave at Cout = 768 (half 384 inside the second cout tile)
                                with a residual and at Cout = 256 (half 128); band map, below
  conv3d_cl_w4_kernel           Cout = 2048: the four tap forms with history x Cin in {64, 128}; Cin = 192      the same
  (256 x 256, gen_conv_w4.py,   at (1, 3) and (3, 1); PIXELS_256; upsample with and without residual and
  LDS offset table)             stride-2 on (2, 30, 30); interleave at Cout = 512 (a whole tile is the odd
                                frame) and at Cout = 1024 (two tiles per half) with residual on / off; the
                                64-workgroup side of the dispatch edge (same operands as the 63-workgroup
                                one plus one image row: both must equal their expectation); band map
  conv_logical_block            Cout = 256, 1x1x1, M = 256 (64 + j) - 3, j = 0..7: grids of 64..71 workgroups,  the same: a map that
  (XCD band map of the 256      every gridDim.x % 8, Cin = 64 on w4 and Cin = 72 on 256p; j = 1 also at 1x3x3   is no permutation
  tiles)                        as (1, 127, 131).  A wrong map that still is a permutation of the tiles only    leaves NaN tiles
                                moves work between XCDs: no result test can see it.
  fg_conv_pack_weight_bf16      PACK_COUT x PACK_CIN x PACK_TAPS (1, 3, 9, 27 taps), a 4-d weight through       torch.equal to the
                                hip.conv_pack_weight, kh != kw through the C entry point; the packed buffer     zero-padded
                                pre-filled with a sentinel and 64 guard elements behind it                      [tap][Cout_pad][Cin_pad]

The unmarked tests are construction checks and run without a GPU.  Over every case of the tables: the operand value sets are as
stated; the fp32 reference equals the fp64 one bit for bit (the GPU tests use the fp32 one); max |conv + bias| <= 2^10; the oracle's
own bf16 path (bf16 F.conv3d, then the residual add) gives the expected bits (no case had to be excepted); at least 10 % of the outputs
change at the first rounding and, with a residual, at least 10 % at the second (conditions on the inputs: a case that misses one takes
its next seed, the share stays); the kernel a case is meant for is the one the launcher picks (fg_conv_tile_choice plus the launcher's
Cin % 64 / cout2 % 256 rule; asserted again in the GPU test).
test_tables_cover_what_the_text_claims holds the tables to the lists and geometry above.

That the tests bite: four mutants of vae_conv.hip that change only what is read or computed (never a store address or a store's bounds
check), each run once against this file on an MI355X (296 GPU cases; the committed kernels pass all of them):
  (a) border test `yy < p.H * sstride` -> `<=` in all three kernels: 102 cases fail, every ks = 3 case in which some frame is
      followed by another (T + kt - 1 >= 2: row H of a frame is row 0 of the next; behind the last frame the buffer load returns the
      same zeros as the padding).  128 tile: 12 of taps_and_borders, the 12 3x3x3 of cin_tails, all 15 cout_tails, all 9 pixel_counts,
      32 of modes; 13 of conv256p; 9 of conv_w4 (among them its upsample and stride-2 cases).
  (b) residual added before the first bf16 rounding (the epilogues of the 128 tile and of 256p; that of w4 is generated assembly and
      was left alone): 59 cases fail, every residual case of those two kernels: all 15 cout_tails, the 41 residual cases of modes
      (8 upsample, 3 stride-2, 30 interleave), 256p upsample-res and 256p interleave-768-res, and the 63-workgroup edge case.
  (c) conv_logical_block without its `+ (xcd < rm ? xcd : rm)` term: 17 cases fail, the 16 band_map cases with gridDim.x % 8 != 0
      (j = 1..7 on both kernels and the two 1x3x3 ones) and 256p-64-768-3x1x1-3x43x42-prev-inter-res (66 workgroups); j = 0 passes, as
      it must (rm = 0: the term is 0).
  (d) the w4 wrapper fills off_tab with dy and dx swapped: 14 cases fail, every ks = 3 case of w4: the 1x3x3 and 3x3x3 forms at
      Cin = 64 / 128 / 192, the four w4-pix cases, upsample with and without residual, stride-2, the 64-workgroup edge case and
      band-64-256-1x3x3-1x127x131.

Cost: the 229 construction checks (three CPU convolutions per case, the largest 136 -> 2048 channels, 27 taps, 1 793 pixels) take ~7 s
of pytest time on a 16-thread host (20 s on 8 threads); the 296 GPU cases, their fp32 CPU references included, 4.6 s of pytest time
on an MI355X, the slowest case 0.2 s.
"""
import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch

from conftest import seeded
from test_buffer_contract import _conv_ref
from test_exact_arithmetic import _assert_same, _signs
from test_hip_kernels import _cl, _ncthw, dev, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
PEAK = 2.0 ** 10          # |conv + bias| stays below: every partial sum is a multiple of 2^-4 with at most 14 significant bits
MIN_SHARE = 0.10          # of the outputs changed by each rounding point

Case = namedtuple("Case", "name kernel cin cout kt ks T H W history resample interleave residual seed_key draw_h")


def _c(family, kernel, cin, cout, kt, ks, thw, history=False, resample=0, interleave=False, residual=False, seed_key=None, draw_h=0):
    T, H, W = thw
    flags = ("-prev" if history else "") + ("", "-up", "-down")[resample] + ("-inter" if interleave else "") + ("-res" if residual else "")
    return Case(f"{family}-{cin}-{cout}-{kt}x{ks}x{ks}-{T}x{H}x{W}{flags}", kernel, cin, cout, kt, ks, T, H, W, history, resample, interleave,
                residual, seed_key, draw_h)


# ------------------------------------------------------------------------------------------------------------------- the case tables
TAPS = [(1, 1), (1, 3), (3, 1), (3, 3)]
BORDER_THW = [(2, 5, 7), (1, 9, 1), (1, 1, 9), (1, 1, 1), (3, 1, 1)]
CIN_TAILS = [8, 16, 24, 48, 56, 64, 72, 120, 128, 136, 160, 320]
COUT_TAILS = [4, 8, 12, 20, 60, 68, 124, 128, 132, 160, 252, 260, 320, 384, 640]
PIXELS_128 = [(1, 1, 1), (127, 1, 1), (2, 8, 8), (3, 43, 1), (1, 3, 43), (5, 3, 17), (2, 8, 16), (1, 257, 1), (7, 5, 11)]
UP_HW = [(2, 2), (2, 14), (14, 2), (10, 12)]
DOWN_HW = [(1, 1), (1, 7), (5, 6)]
INTER_COUT = [8, 24, 192, 256, 384]
INTER_TAPS = [(3, 1), (3, 3), (1, 1)]
CIN_256P = [8, 24, 56, 72, 120, 136]
PIXELS_256 = [(1, 11, 163), (1, 23, 89), (2, 32, 32), (3, 1, 683), (15, 11, 11)]      # M = 1793, 2047, 2048, 2049, 1815
BAND_J = list(range(8))

TAPS_128 = [_c("taps", "128", 64, 128, kt, ks, thw, history=h) for kt, ks in TAPS for thw in BORDER_THW for h in ((False, True) if kt == 3 else (False,))]
CIN_128 = [_c("cin", "128", cin, 64, kt, ks, (2, 5, 7), history=kt == 3) for cin in CIN_TAILS for kt, ks in ((3, 3), (1, 1))]
COUT_128 = [_c("cout", "128", 64, cout, 1, 3, (2, 5, 7), residual=True) for cout in COUT_TAILS]
PIX_128 = [_c("pix", "128", 64, 128, 3, 3, thw, history=True) for thw in PIXELS_128]
UP_128 = [_c("up", "128", 64, 64, 1, 3, (T, H, W), resample=1, residual=r) for H, W in UP_HW for T in (1, 3) for r in (False, True)]
DOWN_128 = [_c("down", "128", 64, 64, 1, 3, (T, H, W), resample=2, residual=T == 3) for H, W in DOWN_HW for T in (1, 3)] + \
    [_c("down", "128", 64, 64, 1, 3, (5, 5, 6), resample=2)]
INTER_128 = [_c("inter", "128", 64, cout, kt, ks, (T, 5, 9), history=kt == 3, interleave=True, residual=r)
             for cout in INTER_COUT for T in (1, 3) for kt, ks in INTER_TAPS for r in (False, True)]
MODES_128 = UP_128 + DOWN_128 + INTER_128

P256 = [_c("256p", "256p", cin, 2048, kt, ks, (1, 11, 163), history=kt == 3) for cin in CIN_256P for kt, ks in ((3, 3), (1, 1))] + \
    [_c("256p", "256p", 72, 2048, kt, ks, (1, 11, 163), history=kt == 3) for kt, ks in ((1, 3), (3, 1))] + \
    [_c("256p-pix", "256p", 24, 2048, 3, 3, thw, history=True) for thw in PIXELS_256] + \
    [_c("256p", "256p", 72, 2048, 1, 3, (2, 30, 30), resample=1, residual=True),
     _c("256p", "256p", 72, 2048, 1, 3, (2, 30, 30), resample=2),
     _c("256p", "256p", 64, 768, 3, 1, (3, 43, 42), history=True, interleave=True, residual=True),
     _c("256p", "256p", 64, 256, 3, 1, (3, 74, 73), history=True, interleave=True)]

W4 = [_c("w4", "w4", cin, 2048, kt, ks, (1, 11, 163), history=kt == 3) for cin in (64, 128) for kt, ks in TAPS] + \
    [_c("w4", "w4", 192, 2048, kt, ks, (1, 11, 163), history=kt == 3) for kt, ks in ((1, 3), (3, 1))] + \
    [_c("w4-pix", "w4", 64, 2048, 3, 3, thw, history=True) for thw in PIXELS_256 if thw != (1, 11, 163)] + \
    [_c("w4", "w4", 64, 2048, 1, 3, (2, 30, 30), resample=1, residual=r) for r in (False, True)] + \
    [_c("w4", "w4", 64, 2048, 1, 3, (2, 30, 30), resample=2),
     _c("w4", "w4", 64, 512, 3, 1, (3, 52, 51), history=True, interleave=True),
     _c("w4", "w4", 64, 1024, 3, 1, (3, 36, 36), history=True, interleave=True),
     _c("w4", "w4", 64, 1024, 3, 1, (3, 36, 36), history=True, interleave=True, residual=True)]
# the dispatch edge: blocks256 = 63 -> 128 tile, 64 -> w4; the smaller case is the larger one without its last image row
EDGE = [_c("edge", "128", 64, 256, 1, 3, (1, 126, 128), residual=True, seed_key="edge", draw_h=127),
        _c("edge", "w4", 64, 256, 1, 3, (1, 127, 128), residual=True, seed_key="edge", draw_h=127)]

BAND = [_c("band", kernel, cin, 256, 1, 1, (1, 1, 256 * (64 + j) - 3)) for kernel, cin in (("w4", 64), ("256p", 72)) for j in BAND_J] + \
    [_c("band", kernel, cin, 256, 1, 3, (1, 127, 131)) for kernel, cin in (("w4", 64), ("256p", 72))]

ALL = TAPS_128 + CIN_128 + COUT_128 + PIX_128 + MODES_128 + P256 + W4 + EDGE + BAND
BY_NAME = {c.name: c for c in ALL}

PACK_COUT, PACK_CIN, PACK_TAPS = [4, 12, 128, 132], [8, 64, 72], [(1, 1, 1), (3, 1, 1), (1, 3, 3), (3, 3, 3)]


def _names(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------------------ operands and expectation
def _cout2(c):
    return c.cout // 2 if c.interleave else c.cout


def _draw(c, salt):
    """The operands of a case in NCTHW: x, prev (or None), w, b, res (or None)."""
    g = torch.Generator("cpu").manual_seed(zlib.crc32((c.seed_key or c.name).encode()) + 1000003 * salt)
    H = c.draw_h or c.H
    hin, win = (H // 2, c.W // 2) if c.resample == 1 else ((2 * H, 2 * c.W) if c.resample == 2 else (H, c.W))
    density = min(1.0, 200.0 / (c.cin * c.kt * c.ks * c.ks))

    def sparse(shape):
        return _signs(shape, g) * (torch.rand(shape, generator=g) < density).to(BF16)

    def dyadic(shape, bound, denom):          # bf16(k / denom) with k uniform in [-bound denom, bound denom]
        return (torch.randint(-bound * denom, bound * denom + 1, shape, generator=g).double() / denom).to(BF16)
    x = sparse((1, c.cin, c.T, hin, win))
    prev = sparse((1, c.cin, 2, hin, win)) if c.history else None
    w, b = dyadic((c.cout, c.cin, c.kt, c.ks, c.ks), 1, 16), dyadic((c.cout,), 8, 64)
    # odd channels: an odd k with 3 < |k / 64| < 4, just below the binade in which a 2^-6 step stops being a bf16 number
    edge = (256 - (2 * torch.randint(0, 32, (c.cout,), generator=g) + 1)) * (2 * torch.randint(0, 2, (c.cout,), generator=g) - 1)
    b[1::2] = (edge.double() / 64).to(BF16)[1::2]
    res = dyadic((1, _cout2(c), 2 * c.T if c.interleave else c.T, H, c.W), 64, 64) if c.residual else None
    if H != c.H:          # the crop of a taller draw (resample 0 only): the same operands minus the last image rows
        assert c.resample == 0
        x, prev, res = (t if t is None else t[:, :, :, :c.H].contiguous() for t in (x, prev, res))
    return x, prev, w, b, res


def _expect(c, x, prev, w, b, res, dtype):
    """(conv + bias in dtype, bf16 of it, bf16 of that + residual): the two rounding points of the header."""
    acc = _conv_ref(x, w, b, prev, None, c.kt, c.ks, c.resample, c.interleave, dtype)
    first = acc.to(BF16)
    want = first if res is None else (first.to(dtype) + res.to(dtype)).to(BF16)
    return acc, first, want


def _shares(acc, first, want, res):
    s1 = (acc != first.to(acc.dtype)).float().mean().item()
    s2 = None if res is None else ((first.to(acc.dtype) + res.to(acc.dtype)) != want.to(acc.dtype)).float().mean().item()
    return s1, s2


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands and the fp32 expectation of a case, at the first seed whose inputs meet the rounding shares and the peak."""
    c = BY_NAME[name]
    for salt in range(8):
        x, prev, w, b, res = _draw(c, salt)
        acc, first, want = _expect(c, x, prev, w, b, res, torch.float32)
        s1, s2 = _shares(acc, first, want, res)
        peak = acc.abs().max().item()
        if peak <= PEAK and s1 >= MIN_SHARE and (s2 is None or s2 >= MIN_SHARE):
            return SimpleNamespace(c=c, x=x, prev=prev, w=w, b=b, res=res, acc=acc, first=first, want=want, s1=s1, s2=s2, peak=peak, salt=salt)
    raise AssertionError(f"{name}: no seed of 8 meets the rounding shares (last: first {s1:.3f}, second {s2}, peak {peak})")


def _kernel(lib, c):
    """The kernel the launcher picks: fg_conv_tile_choice, then its Cin % 64 / cout2 % 256 rule between the two 256 tiles."""
    if lib.fg_conv_tile_choice(c.T, c.H, c.W, c.cout) == 128:
        return "128"
    return "w4" if c.cin % 64 == 0 and _cout2(c) % 256 == 0 else "256p"


def _geometry(c):
    """How the pixel tiles of a case lie in the image: M % tile, gridDim.x % 8, a tile boundary inside an image row, one exactly at
    a frame boundary, and the largest number of frames one tile touches."""
    tile = 128 if c.kernel == "128" else 256
    M, hw = c.T * c.H * c.W, c.H * c.W
    grid = -(-M // tile) * (-(-c.cout // 128) * 128 // tile)
    cuts = range(tile, M, tile)
    frames = max((min(m + tile, M) - 1) // hw - m // hw + 1 for m in range(0, M, tile))
    return SimpleNamespace(rem=M % tile, grid8=grid % 8, in_row=any(m % c.W for m in cuts), at_frame=any(m % hw == 0 for m in cuts), frames=frames)


# ------------------------------------------------------------------------------------------------------------ construction checks
def test_names_are_unique():
    assert len(BY_NAME) == len(ALL)


@pytest.mark.parametrize("name", _names(ALL))
def test_case_construction(name):
    from fairygen_amd import hip as h
    k = _case(name)
    c = k.c
    print(f"{name}: seed {k.salt}, first rounding changes {k.s1:.3f}, second {k.s2}, max |conv + bias| {k.peak}")
    assert _kernel(h.load(), c) == c.kernel, "the launcher picks another kernel"
    for t in (k.x, k.prev):
        assert t is None or set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
    w16, b64 = 16 * k.w.double(), 64 * k.b.double()
    assert torch.equal(w16, w16.round()) and w16.abs().max().item() <= 16 and w16.unique().numel() > min(16, k.w.numel() // 4)
    assert torch.equal(b64, b64.round()) and k.b.abs().max().item() <= 8 and k.b.dtype == BF16
    if c.residual:
        r64 = 64 * k.res.double()
        assert torch.equal(r64, r64.round()) and k.res.abs().max().item() <= 64 and k.res.dtype == BF16 and k.res.abs().max().item() > 32
    acc64, first64, want64 = _expect(c, k.x, k.prev, k.w, k.b, k.res, torch.float64)
    assert torch.equal(k.acc.double(), acc64), "fp32 and fp64 convolutions differ"
    assert torch.equal(k.first, first64) and torch.equal(k.want, want64)
    assert torch.equal(16 * 4 * acc64, (16 * 4 * acc64).round()) and k.peak <= PEAK
    assert torch.equal(_conv_ref(k.x, k.w, k.b, k.prev, k.res, c.kt, c.ks, c.resample, c.interleave, BF16), k.want), "the oracle's bf16 path"
    assert k.s1 >= MIN_SHARE and (k.s2 is None or k.s2 >= MIN_SHARE)
    assert not k.want.isnan().any() and tuple(k.want.shape) == (1, _cout2(c), (2 if c.interleave else 1) * c.T, c.H, c.W)


def test_dispatch_edge_pair_shares_its_operands():
    lo, hi = (_case(c.name) for c in EDGE)
    assert torch.equal(lo.x, hi.x[:, :, :, :126]) and torch.equal(lo.res, hi.res[:, :, :, :126]) and torch.equal(lo.w, hi.w) and torch.equal(lo.b, hi.b)
    assert torch.equal(lo.want[:, :, :, :125], hi.want[:, :, :, :125]) and not torch.equal(lo.want[:, :, :, 125], hi.want[:, :, :, 125])
    blocks = [-(-c.T * c.H * c.W // 256) * (c.cout // 256) for c in EDGE]
    assert blocks == [63, 64]


def test_thresholds_of_the_256_tile():
    """The smallest M on the 256 tile for each Cout the tables use, through fg_conv_tile_choice."""
    from fairygen_amd import hip as h
    lib = h.load()
    for cout, m in ((2048, 1793), (1024, 3841), (768, 5377), (512, 7937), (256, 16129)):
        assert lib.fg_conv_tile_choice(1, 1, m, cout) == 256 and lib.fg_conv_tile_choice(1, 1, m - 1, cout) == 128, (cout, m)
    assert all(lib.fg_conv_tile_choice(1, 1, 1 << 20, cout) == 128 for cout in (384, 640, 132))


def test_tables_cover_what_the_text_claims():
    def values(cases, field):
        return sorted({getattr(c, field) for c in cases})

    def thw(cases):
        return {(c.T, c.H, c.W) for c in cases}
    assert {(c.kt, c.ks, (c.T, c.H, c.W), c.history) for c in TAPS_128} == \
        {(kt, ks, s, h) for kt, ks in TAPS for s in BORDER_THW for h in (False, True) if kt == 3 or not h}
    assert {(c.cin, c.kt, c.ks) for c in CIN_128} == {(cin, kt, ks) for cin in CIN_TAILS for kt, ks in ((3, 3), (1, 1))}
    assert values(CIN_128, "cin") == CIN_TAILS and {c % 64 for c in CIN_TAILS} >= {8, 16, 24, 48, 56, 0} and {c // 64 for c in CIN_TAILS} >= {0, 1, 2, 5}
    assert values(COUT_128, "cout") == COUT_TAILS and {-(-c // 128) * 128 for c in COUT_TAILS} == {128, 256, 384, 640}
    assert sorted(c.T * c.H * c.W for c in PIX_128) == [1, 127, 128, 129, 129, 255, 256, 257, 385]
    assert {(c.H, c.W, c.T, c.residual) for c in UP_128} == {(H, W, T, r) for H, W in UP_HW for T in (1, 3) for r in (False, True)}
    assert {(c.H, c.W) for c in DOWN_128} == set(DOWN_HW) and values(DOWN_128, "T") == [1, 3, 5]
    assert {(c.cout, c.T, c.kt, c.ks, c.residual) for c in INTER_128} == \
        {(co, T, kt, ks, r) for co in INTER_COUT for T in (1, 3) for kt, ks in INTER_TAPS for r in (False, True)}
    assert {co // 2 % 128 for co in INTER_COUT} >= {96, 64, 0}, "halves inside a cout tile and on its edge"
    wide = [c for c in P256 if c.cout == 2048 and c.resample == 0]
    assert {c.cin for c in wide if (c.kt, c.ks) in ((3, 3), (1, 1))} >= set(CIN_256P) and {c.cin % 64 for c in wide} >= {8, 24, 56}
    assert {(c.kt, c.ks) for c in wide if c.cin == 72 and (c.history or c.kt == 1)} == set(TAPS)
    assert thw(P256) >= set(PIXELS_256) and thw(W4) >= set(PIXELS_256)
    assert {(c.resample, c.residual) for c in P256 if c.resample} == {(1, True), (2, False)} and all(c.cin == 72 for c in P256 if c.resample)
    assert {(c.cout, c.residual) for c in P256 if c.interleave} == {(768, True), (256, False)}
    for cin in (64, 128):
        assert {(c.kt, c.ks) for c in W4 if c.cin == cin and c.cout == 2048 and (c.history or c.kt == 1) and c.resample == 0} == set(TAPS)
    assert {(c.kt, c.ks) for c in W4 if c.cin == 192} == {(1, 3), (3, 1)}
    assert {(c.resample, c.residual) for c in W4 if c.resample} == {(1, False), (1, True), (2, False)}
    assert {(c.cout, c.residual) for c in W4 if c.interleave} == {(512, False), (1024, False), (1024, True)}
    assert all(c.cin <= 192 for c in P256 + W4 + BAND)
    # pixel-tile geometry, per kernel
    for kernel, tile in (("128", 128), ("256p", 256), ("w4", 256)):
        geo = [_geometry(c) for c in ALL if c.kernel == kernel]
        assert {g.rem for g in geo} >= {0, 1, tile - 1}, kernel
        assert any(g.in_row for g in geo) and any(g.at_frame for g in geo) and any(g.frames >= 3 for g in geo), kernel
        if tile == 256:
            assert {g.grid8 for g in geo} == set(range(8)), kernel
            band = [_geometry(c) for c in BAND if c.kernel == kernel and c.ks == 1]
            assert sorted(g.grid8 for g in band) == BAND_J and all(g.rem == 253 for g in band)
        # ... and in the upsample, downsample and interleave forms: a tile boundary inside an image row, a tile over two frames
        for form in (lambda c: c.resample == 1, lambda c: c.resample == 2, lambda c: c.interleave):
            geo = [_geometry(c) for c in ALL if c.kernel == kernel and form(c)]
            assert any(g.in_row for g in geo) and any(g.frames >= 2 for g in geo), kernel


def _packed_expectation(w):
    """(Cout, Cin, kt, kh, kw) -> the zero-padded [tap][Cout_pad][Cin_pad] the kernels read."""
    cout, cin = w.shape[:2]
    taps = w[0, 0].numel()
    e = torch.zeros((taps, -(-cout // 128) * 128, -(-cin // 64) * 64), dtype=w.dtype)
    e[:, :cout, :cin] = w.reshape(cout, cin, taps).permute(2, 0, 1)
    return e


def test_packed_bytes_and_expectation():
    from fairygen_amd import hip as h
    lib = h.load()
    for cout in PACK_COUT:
        for cin in PACK_CIN:
            for kt, kh, kw in PACK_TAPS + [(1, 3, 1), (1, 2, 3)]:
                e = _packed_expectation(torch.zeros((cout, cin, kt, kh, kw)))
                assert lib.fg_conv_packed_bytes(cout, cin, kt, kh, kw) == 2 * e.numel()
    w = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 1, 2, 2)
    e = _packed_expectation(w)
    assert e.shape == (4, 128, 64) and e[3, 1, 2] == w[1, 2, 0, 1, 1] and e[:, 2:].abs().sum() == 0 and e[:, :, 3:].abs().sum() == 0


# ------------------------------------------------------------------------------------------------------------------------ GPU tests
def _run(hip, name):
    k = _case(name)
    c = k.c
    assert _kernel(hip.load(), c) == c.kernel, name
    xin = k.x if c.kt == 1 else torch.cat([k.prev if k.prev is not None else k.x.new_zeros(k.x.shape[:2] + (2,) + k.x.shape[3:]), k.x], dim=2)
    out = torch.full(((2 if c.interleave else 1) * c.T, c.H, c.W, _cout2(c)), float("nan"), dtype=BF16, device="cuda")
    got = hip.conv3d_cl(dev(_cl(xin)), hip.conv_pack_weight(dev(k.w)), dev(k.b), c.cout, c.kt, c.ks, residual=None if k.res is None else dev(_cl(k.res)),
                        upsample2x=c.resample == 1, downsample2x=c.resample == 2, time_interleave=c.interleave, out=out)
    assert got.data_ptr() == out.data_ptr()
    _assert_same(_ncthw(got.cpu()), k.want, f"conv {name} on the {c.kernel} kernel  [index: (1, channel, frame, y, x)]")


@gpu
@pytest.mark.parametrize("name", _names(TAPS_128))
def test_conv128_taps_and_borders(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(CIN_128))
def test_conv128_cin_tails(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(COUT_128))
def test_conv128_cout_tails(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(PIX_128))
def test_conv128_pixel_counts(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(MODES_128))
def test_conv128_modes(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(P256))
def test_conv256p(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(W4))
def test_conv_w4(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(EDGE))
def test_conv_dispatch_edge(hip, name):
    _run(hip, name)


@gpu
@pytest.mark.parametrize("name", _names(BAND))
def test_conv_band_map(hip, name):
    _run(hip, name)


SENTINEL, GUARD = -77.0, 64


def _pack_raw(hip, w, kt, kh, kw):
    """fg_conv_pack_weight_bf16 through the C entry point into a buffer pre-filled with SENTINEL, GUARD elements longer than needed."""
    cout, cin = w.shape[:2]
    n = hip.load().fg_conv_packed_bytes(cout, cin, kt, kh, kw) // 2
    buf = torch.full((n + GUARD,), SENTINEL, dtype=BF16, device="cuda")
    hip._call("fg_conv_pack_weight_bf16", hip._ptr(w), hip._ptr(buf), cout, cin, kt, kh, kw, hip._stream(w))
    torch.cuda.synchronize()
    assert (buf[n:] == SENTINEL).all(), "written past the packed size"
    return buf[:n].cpu()


@gpu
@pytest.mark.parametrize("kt,kh,kw", PACK_TAPS + [(1, 3, 1), (1, 2, 3)])
@pytest.mark.parametrize("cin", PACK_CIN)
@pytest.mark.parametrize("cout", PACK_COUT)
def test_pack_weight(hip, cout, cin, kt, kh, kw):
    w = seeded((cout, cin, kt, kh, kw), 400 + cout + 3 * cin + kt * kh * kw)
    assert (w != 0).all() and (w != SENTINEL).all()
    want = _packed_expectation(w)
    _assert_same(_pack_raw(hip, dev(w), kt, kh, kw).view(want.shape), want, f"pack {cout} x {cin} x ({kt}, {kh}, {kw})  [index: (tap, cout, cin)]")
    if (kt, kh, kw) == (1, 3, 3):          # the 4-d weight of a Conv2d through the wrapper
        _assert_same(hip.conv_pack_weight(dev(w[:, :, 0])).cpu().view(want.shape), want, f"conv_pack_weight of a 4-d weight {cout} x {cin}")

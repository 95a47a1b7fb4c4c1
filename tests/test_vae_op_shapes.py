"""The helper kernels of csrc/vae_ops.hip at every width, factor and tile geometry their index arithmetic distinguishes.

The older tests meet each of them at one or two hand-picked shapes (test_hip_kernels.py), above their grid caps (test_grid_stride.py) and
inside whole-model goldens at the stock geometry.  A wrong index in any of them gives a plausible picture, not a fault, so every kernel is
compared here with the oracle's expression of the same operation (oracle/wan_vae.py, oracle/pipeline.py) on small tensors.

  kernel                          swept                                                                     criterion
  fg_vae_rmsnorm_silu_bf16        C in NORM_C (32-lane form up to 256, 64-lane form up to 2048: one lane,     assert_close_bf16(got, R16, 1.0): every element
                                  both sides of the switch, part-filled vector slots 520 / 1032 / 2040, the    within 1 bf16 ulp of max(|R16|, 1e-3) and at
                                  encoder widths 160 / 320 / 640) x pixels in NORM_PIXELS (whole and ragged    most 2e-3 of the elements different (the
                                  blocks of 8 resp. 4 pixels, a dead upper half-wave) x SiLU on / off; rows    project's own numbers); R16 = rms_norm_c
                                  of all zeros (the 1e-12 clamp), scaled by 1e-4 and 1e4, one channel at       (+ F.silu) in bf16
                                  +-256 over 0.01 noise; gamma = 40 on 8 channels (y < -80: the exp clamp)
  fg_dupup3d_add_bf16             the older list + Wo * Cout / 8 in {257, 320, 330, 525, 532, 546} (two and    torch.equal(main + dup_up3d)
                                  three workgroups in x, the last one partial) on every source form (vector
                                  loads of stride 1 / 2 / 4, gathers with a shift at stride 8 and at
                                  Cin % 8 != 0, gathers with a division at repeats = 6), (ft, fs) = (1, 1)
                                  and (2, 1), T in {1, 2, 3} with first_chunk on and off (T = 1, ft = 2,
                                  first: one output frame)
  fg_vae_tile_accumulate_bf16     one tile inside a larger, pre-filled canvas at odd y0 / x0: all 16           torch.equal(values += tile * m),
                                  bound_bits x 12 (border_h, border_w) pairs from {1, 2, 3, 5, 6, 7, 12},      torch.equal(weight += m), m = tile_mask in bf16;
                                  tile = border, border < tile < 2 border (the second ramp overwrites the      refused: return code FG_EINVAL and an unchanged
                                  first), tile >= 2 border, tile < border on an axis bound on both sides;      canvas
                                  F in {1, 5}, C in {1, 3, 48}; refused: border > tile with a free side
  ... + fg_vae_tile_finalize_bf16 a walk over four tiles with borders (48, 80) and (80, 48) = (size -          torch.equal(values / weight [.clamp(-1, 1)])
                                  stride) * 16, every canvas pixel covered; clamp on and off
  fg_avgdown3d_add_bf16           the encoder's channel pairs and two with a group of 3 / 6 / 12 x every       (a) integers: torch.equal to the fp64 evaluation
                                  (ft, fs) the launcher accepts x T in {1, 2, 3, 5} (front padding with and    rounded as the header says; (b) N(0, 1): the
                                  without real frames)                                                         criterion of test_encoder_kernels, unchanged
  fg_vae_latent_to_cl_bf16,       C / Z in {16, 48}, Cx in {2 Z, 2 Z + 8}, odd T, H, W, random mean and         torch.equal
  fg_vae_latent_from_cl_bf16      positive inv_std, and the VAE38 constants
  fg_vae_unpatchify_bf16          odd H, W; T in {1, 3}; t0 in {0, middle, F - T}; clamp on / off on inputs    torch.equal; frames outside [t0, t0 + T) keep
                                  beyond +-1                                                                   the sentinel
  fg_vae_patchify_bf16            odd half sizes; T in {1, 3}; output pre-filled with a sentinel               torch.equal; channels 12..15 zero
  fg_video_to_uint8               every finite bf16 bit pattern (65 280 values) in one launch                  torch.equal(pipeline.video_to_uint8)

The unmarked tests are construction checks and run without a GPU.  For the RMS_norm they hold the inputs to what the criterion assumes:
R64, an fp64 evaluation of the header's formula with a bf16 rounding at each point it names (the norm included), meets the same
criterion against R16 on every (C, pixels) used; no row's fp64 norm is within 2^-20 relative of a bf16 rounding tie (a flipped norm moves
a whole row by an ulp); and in the cases below NORM_SMALL elements, where the 2e-3 share allows only a handful of elements or none, no
more elements than that lie on a knife edge of their own: a rounding point of R64 within 2^-21 relative of a tie (2^-19 for the SiLU
quotient).  The kernel's reciprocal + one correction quotient is within 1 fp32 ulp (2^-23) of the exact one and its exp2-based exponential
within ~|y| 2^-23 + 2^-22 of exp, so an element further from every tie than that rounds as R64 does.  A case that misses any of this
takes its next inputs (`first_robust` of test_row_kernel_shapes.py: a property of inputs and oracle, decided on the CPU); the bound and
the cap stay.  The other construction checks hold the case tables to the coverage claimed above and the exact-arithmetic inputs of
avgdown to what makes them exact.

Cost: the construction checks take ~4 s of pytest time on a 16-thread host; the GPU tests (CPU references included) a few seconds in
all on an MI355X, the largest tensor 35 x 2048 elements.
"""
import functools
import math
import random
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import seeded
from oracle import pipeline as opipe
from oracle import wan_vae
from test_hip_kernels import _cl, _ncthw, assert_close_bf16, dev, hip  # noqa: F401  (hip: the module fixture)
from test_row_kernel_shapes import first_robust

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
SHARE = 2e-3                                   # assert_close_bf16's default mismatch share
FG_EINVAL = -1


def rbf64(t):
    """fp64 -> bf16 -> fp64: one rounding."""
    return t.to(BF16).double()


def seeded_int(shape, seed, bound=64):
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).to(BF16)


def tie_distance(v):
    """Relative distance of every |v| (fp64) from the nearest midpoint between two bf16 values of its binade; inf for 0."""
    a = v.abs()
    safe = torch.where(a > 0, a, torch.ones_like(a))
    ulp = torch.exp2(torch.floor(torch.log2(safe)) - 7.0)
    t = safe / ulp
    d = ((t - torch.floor(t)) - 0.5).abs() * ulp / safe
    return torch.where(a > 0, d, torch.full_like(a, math.inf))


# ------------------------------------------------------------------------------------------------------------ 1. RMS_norm (+ SiLU)
NORM_C = [8, 16, 160, 248, 256, 264, 320, 504, 512, 520, 640, 1016, 1024, 1032, 1536, 2040, 2048]
NORM_PIXELS = [1, 3, 4, 5, 7, 8, 9, 35]
NORM_HOT_C = [256, 512]                         # gamma = 40 on HOT_CHANNELS, both lane forms
HOT_CHANNELS = [3, 9, 64, 65, 130, 199, 200, 255]
SPECIALS = ("zero", "small", "big", "spike+", "spike-")
NORM_TIE, KNIFE, KNIFE_SILU = 2.0 ** -20, 2.0 ** -21, 2.0 ** -19
NORM_SMALL = 4096                               # below: the knife-edge elements count against the share too


def special_rows(C, pixels):
    """{row: kind}: up to five special rows, spread over the tensor, at least one ordinary row left; fewer rows take a rotating subset."""
    n = min(len(SPECIALS), pixels - 1)
    start = (C // 8) % len(SPECIALS)
    return {(k * pixels) // n: SPECIALS[(start + k) % len(SPECIALS)] for k in range(n)}


def r64_norm(x, g, silu):
    """The header's formula in fp64, rounded to bf16 where it says: silu(bf16(bf16(bf16(x / max(bf16(||x||), 1e-12)) * sqrt(C)) * gamma)).
    Returns (result bf16, fp64 norms, knife mask, y before the SiLU)."""
    xd, gd = x.double(), g.double()
    norm = torch.sqrt((xd * xd).sum(-1, keepdim=True))
    sqrt_c = float(torch.tensor(float(x.shape[-1]), dtype=torch.float32).sqrt())        # the launcher's sqrtf((float)C)
    q = xd / rbf64(norm).clamp_min(1e-12)
    s = rbf64(q) * sqrt_c
    y = rbf64(s) * gd
    knife = (tie_distance(q) < KNIFE) | (tie_distance(s) < KNIFE)
    y = rbf64(y)                                 # a product of two bf16 is exact in fp32: its ties are exact ties, rounded to even by everyone
    out = y
    if silu:
        out = y / (1.0 + torch.exp(torch.clamp(-y, max=80.0)))
        knife = knife | (tie_distance(out) < KNIFE_SILU)
    return out.to(BF16), norm, knife, y


def _norm_build(C, pixels, hot, salt):
    c = SimpleNamespace(C=C, pixels=pixels, hot=hot)
    x = seeded((pixels, C), 20000 + 64 * C + pixels + 1000003 * salt, scale=2.0)
    c.rows = special_rows(C, pixels)
    for r, kind in c.rows.items():
        if kind == "zero":
            x[r] = 0
        elif kind == "small":
            x[r] = (x[r].float() * 1e-4).to(BF16)
        elif kind == "big":
            x[r] = (x[r].float() * 1e4).to(BF16)
        else:
            x[r] = (x[r].float() * 0.005).to(BF16)
            x[r, (7 * r + 3) % C] = 256.0 if kind == "spike+" else -256.0
    c.x = x
    c.g = (1 + 0.1 * seeded((C,), 21000 + C)).to(BF16)
    if hot:
        c.g[HOT_CHANNELS] = 40.0
    x5 = x.t().reshape(1, C, 1, 1, pixels)
    r16 = wan_vae.rms_norm_c({"n.gamma": c.g.view(C, 1, 1, 1)}, "n", x5)
    c.r16 = {False: _cl(r16).reshape(pixels, C), True: _cl(F.silu(r16)).reshape(pixels, C)}
    return c


def _norm_check(c):
    """What the criterion assumes of the inputs (module docstring)."""
    allowed = int(SHARE * c.pixels * c.C)
    for silu in (False, True):
        r64, norm, knife, y = r64_norm(c.x, c.g, silu)
        what = f"R64 against R16, C={c.C} pixels={c.pixels} silu={silu}"
        assert_close_bf16(r64, c.r16[silu], 1.0, what)
        assert (tie_distance(norm) >= NORM_TIE).all(), f"{what}: a row norm on a bf16 rounding tie"
        if c.pixels * c.C < NORM_SMALL:
            differ = (r64.float() != c.r16[silu].float()).sum().item()
            assert differ + knife.sum().item() <= allowed, f"{what}: {differ} different + {knife.sum().item()} knife-edge elements, {allowed} allowed"
        if c.hot:
            assert (y < -80.0).any() and (y > 80.0).any(), f"{what}: the exponent clamp is not reached"
    for r, kind in c.rows.items():
        if kind == "zero":
            assert not c.x[r].any() and not c.r16[False][r].any() and not c.r16[True][r].any()


@functools.lru_cache(maxsize=None)
def norm_case(C, pixels, hot=False):
    return first_robust(functools.partial(_norm_build, C, pixels, hot), _norm_check)


@pytest.mark.parametrize("C", NORM_C)
def test_norm_inputs_leave_the_criterion_to_the_kernel(C):
    for pixels in NORM_PIXELS:
        c = norm_case(C, pixels)
        print(f"vae rmsnorm C={C} pixels={pixels}: inputs of salt {c.salt}, special rows {c.rows}")
        _norm_check(c)


@pytest.mark.parametrize("C", NORM_HOT_C)
def test_norm_hot_gamma_reaches_the_exponent_clamp(C):
    c = norm_case(C, 35, True)
    print(f"vae rmsnorm C={C}, gamma 40: inputs of salt {c.salt}")
    _norm_check(c)
    assert (c.g[HOT_CHANNELS] == 40.0).all() and max(HOT_CHANNELS) < min(NORM_HOT_C)


def test_norm_case_table():
    """Both lane forms meet every special row next to an ordinary one, in an odd and an even pixel count, and every width class is there."""
    for form in (lambda C: C <= 256, lambda C: C > 256):
        for parity in (0, 1):
            kinds = set()
            for C in filter(form, NORM_C):
                for p in NORM_PIXELS:
                    if p % 2 == parity:
                        rows = special_rows(C, p)
                        assert len(rows) == min(5, p - 1) and len(rows) < p and all(0 <= r < p for r in rows)
                        kinds |= set(rows.values())
            assert kinds == set(SPECIALS)
    assert {248, 256, 264, 2040, 2048} <= set(NORM_C) and {160, 320, 640} <= set(NORM_C)         # switch, limit, encoder widths
    assert {520, 1032, 2040} <= {C for C in NORM_C if C > 256 and (C // 8) % 64}                  # a part-filled vector slot of the 64-lane form
    assert {p % 8 for p in NORM_PIXELS} >= {0, 1, 3, 4, 5, 7} and {p % 4 for p in NORM_PIXELS} == {0, 1, 3}


@gpu
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C", NORM_C)
def test_vae_rmsnorm_silu_shapes(hip, C, silu):
    for pixels in NORM_PIXELS:
        c = norm_case(C, pixels)
        got = hip.vae_rmsnorm_silu(dev(c.x), dev(c.g), silu).cpu()
        assert_close_bf16(got, c.r16[silu], 1.0, f"vae rmsnorm C={C} pixels={pixels} silu={silu}")
        for r, kind in c.rows.items():
            if kind == "zero":
                assert not got[r].any(), f"C={C} pixels={pixels}: the all-zero pixel {r} must come back as zeros"


@gpu
@pytest.mark.parametrize("C", NORM_HOT_C)
def test_vae_rmsnorm_silu_exponent_clamp(hip, C):
    c = norm_case(C, 35, True)
    for silu in (True, False):
        got = hip.vae_rmsnorm_silu(dev(c.x), dev(c.g), silu).cpu()
        assert torch.isfinite(got.float()).all()
        assert_close_bf16(got, c.r16[silu], 1.0, f"vae rmsnorm C={C}, gamma 40, silu={silu}")


# ------------------------------------------------------------------------------------------------------------ 2. DupUp3D + add
# (cin, cout, ft, fs, first_chunk, T, H, W)
DUPUP_OLD = [(cin, cout, ft, fs, first, 2, 3, 4) for cin, cout, ft, fs, first in [
    (64, 64, 2, 2, True), (64, 64, 2, 2, False), (64, 32, 1, 2, False), (128, 64, 1, 2, True), (256, 64, 1, 2, False),
    (256, 32, 2, 2, True), (256, 32, 2, 2, False), (32, 48, 1, 2, False), (12, 24, 1, 2, False), (12, 24, 2, 2, True), (12, 24, 2, 2, False)]]
DUPUP_WIDE = [                                               # Wo * Cout / 8 > 256: more than one workgroup in x, the last one partial
    (256, 256, 1, 2, False, 2, 2, 5),                        # 320, vector loads of stride 1
    (512, 256, 1, 2, False, 1, 2, 5),                        # 320, stride 2
    (1024, 256, 1, 2, True, 2, 2, 5),                        # 320, stride 4
    (2048, 256, 2, 2, False, 1, 2, 5), (2048, 256, 2, 2, True, 2, 2, 5),      # 320, stride 8: gathers, shift 0
    (208, 312, 1, 2, False, 2, 2, 7),                        # 546 = 513 + 33, repeats = 6: gathers with a division
    (132, 264, 1, 2, False, 2, 2, 5), (132, 264, 2, 2, True, 1, 2, 5),        # 330, Cin % 8 != 0: gathers, shift 3 / 4
    (16, 8, 2, 1, False, 2, 2, 257), (8, 8, 1, 1, False, 2, 3, 257),          # 257: one live thread in the second workgroup
    (304, 304, 2, 2, False, 1, 2, 7),                        # 532 = 513 + 19: three workgroups
    (120, 120, 1, 1, True, 3, 2, 35)]                        # 525: odd
DUPUP_FACTORS = [(64, 64, 1, 1, False, 2, 3, 4), (32, 64, 1, 1, False, 2, 3, 4), (64, 64, 2, 1, True, 2, 3, 4), (64, 64, 2, 1, False, 2, 3, 4),
                 (128, 64, 2, 1, False, 2, 3, 4), (64, 128, 2, 1, True, 3, 3, 4)]
DUPUP_FRAMES = [(cin, cout, ft, fs, first, T, 3, 4) for cin, cout, ft, fs in [(64, 64, 2, 2), (256, 32, 2, 2), (64, 64, 2, 1), (64, 32, 1, 2)]
                for T in (1, 3) for first in (True, False)]
DUPUP_CASES = DUPUP_OLD + DUPUP_WIDE + DUPUP_FACTORS + DUPUP_FRAMES


def dupup_form(cin, cout, ft, fs):
    """The source form dupup3d_add_kernel takes, by its own rule."""
    factor = ft * fs * fs
    repeats = cout * factor // cin
    stride = factor // repeats
    if stride * repeats == factor and stride <= 4 and cin % 8 == 0:
        return f"vec{stride}"
    return "shift" if repeats & (repeats - 1) == 0 else "div"


def test_dupup_case_table():
    assert len(set(DUPUP_CASES)) == len(DUPUP_CASES)
    wide = {}
    for cin, cout, ft, fs, first, T, H, W in DUPUP_CASES:
        assert (cout * ft * fs * fs) % cin == 0 and cout % 8 == 0 and T * ft - (ft - 1 if first else 0) > 0
        n = W * fs * (cout // 8)
        if n > 256:
            assert n % 256 != 0
            form = dupup_form(cin, cout, ft, fs)
            key = form if form.startswith("vec") else (form, "stride 8" if cin == 8 * cout else ("ragged" if cin % 8 else "wide repeats"))
            wide.setdefault(key, set()).add(n)
    assert set(wide) == {"vec1", "vec2", "vec4", ("shift", "stride 8"), ("shift", "ragged"), ("div", "wide repeats")}, wide
    sizes = set().union(*wide.values())
    assert {257, 320} <= sizes and any(n > 513 and n % 2 for n in sizes) and any(n > 513 and (n - 513) % 2 for n in sizes) and max(sizes) > 512
    assert {(ft, fs) for _, _, ft, fs, *_ in DUPUP_CASES} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {(T, first) for *_, first, T, _, _ in DUPUP_CASES} == {(T, f) for T in (1, 2, 3) for f in (True, False)}
    assert any(ft == 2 and first and T == 1 for _, _, ft, _, first, T, _, _ in DUPUP_CASES)
    assert set(DUPUP_OLD) <= set(DUPUP_CASES)


@gpu
@pytest.mark.parametrize("cin,cout,ft,fs,first,T,H,W", DUPUP_CASES)
def test_dupup3d_add_shapes(hip, cin, cout, ft, fs, first, T, H, W):
    x = seeded((1, cin, T, H, W), 300 + cin)
    sc = wan_vae.dup_up3d(x, cout, ft, fs, first)
    assert sc.shape[2] == T * ft - (ft - 1 if first else 0)
    main = seeded(tuple(sc.shape), 301 + cout)
    got = hip.dupup3d_add(dev(_cl(x)), dev(_cl(main)), cout, ft, fs, first)
    assert torch.equal(_ncthw(got.cpu()), main + sc)


# ------------------------------------------------------------------------------------------------------------ 3. tile feathering
BORDER_PAIRS = [(1, 1), (2, 3), (3, 2), (5, 7), (7, 5), (6, 12), (12, 6), (3, 3), (5, 12), (12, 1), (1, 6), (7, 7)]
TILE_F, TILE_C = (1, 5), (1, 3, 48)


def tile_len(kind, border, both_bound):
    """Tile length of a kind: equal to the border; between one and two borders (the ramps overlap, the later assignment wins); two clear
    ramps; shorter than the border, which only an axis bound on both sides accepts (no ramp at all)."""
    if kind == "short" and both_bound and border > 1:
        return border - 1
    if kind == "overlap" and border > 1:
        return border + border // 2
    return 2 * border + 3 if kind == "wide" else border


@functools.lru_cache(maxsize=None)
def tile_cases(bits):
    """Twelve single-tile cases of one bound_bits value: every border pair, the rest drawn from a fixed generator (test_tile_case_table
    holds the whole table to its coverage)."""
    rng = random.Random(4000 + bits)
    cases = []
    for bh, bw in BORDER_PAIRS:
        kh, kw = (rng.choice(("eq", "overlap", "wide", "short")) for _ in range(2))
        th, tw = tile_len(kh, bh, bits & 3 == 3), tile_len(kw, bw, bits & 12 == 12)
        cases.append(SimpleNamespace(bits=bits, bh=bh, bw=bw, th=th, tw=tw, F=rng.choice(TILE_F), C=rng.choice(TILE_C),
                                     y0=rng.choice((1, 3)), x0=rng.choice((3, 5))))
    return cases


def tile_bounds(bits):
    return tuple(bool(bits & (1 << i)) for i in range(4))


def tile_reference(c, seed):
    """Seeded tile and canvas of a case, and the canvas after `values[...] += tile * m; weight[...] += m` in torch bf16."""
    Hv, Wv = c.y0 + c.th + 2, c.x0 + c.tw + 1
    tile = seeded((c.C, c.F, c.th, c.tw), seed)
    values, weight = seeded((c.C, c.F, Hv, Wv), seed + 1), seeded((c.F, Hv, Wv), seed + 2).abs() + 0.5
    assert values.count_nonzero() > 0.99 * values.numel() and (weight > 0).all()
    m = wan_vae.tile_mask(c.th, c.tw, tile_bounds(c.bits), (c.bh, c.bw)).to(BF16)[0, 0]
    want_v, want_w = values.clone(), weight.clone()
    want_v[:, :, c.y0:c.y0 + c.th, c.x0:c.x0 + c.tw] += tile * m
    want_w[:, c.y0:c.y0 + c.th, c.x0:c.x0 + c.tw] += m[0]
    return tile, values, weight, want_v, want_w


def test_tile_case_table():
    cases = [c for bits in range(16) for c in tile_cases(bits)]
    assert {c.bits for c in cases} == set(range(16)) and all({(c.bh, c.bw) for c in tile_cases(b)} == set(BORDER_PAIRS) for b in range(16))
    assert {b for pair in BORDER_PAIRS for b in pair} == {1, 2, 3, 5, 6, 7, 12} and any(bh != bw for bh, bw in BORDER_PAIRS)
    assert {c.F for c in cases} == set(TILE_F) and {c.C for c in cases} == set(TILE_C)
    assert all(c.y0 % 2 and c.x0 % 2 for c in cases)
    for length, border, free in ((lambda c: c.th, lambda c: c.bh, lambda c: c.bits & 3 != 3), (lambda c: c.tw, lambda c: c.bw, lambda c: c.bits & 12 != 12)):
        live = [c for c in cases if free(c)]                           # an axis with at least one ramp
        assert all(length(c) >= border(c) for c in live)               # what the reference and the launcher accept
        assert any(length(c) == border(c) and border(c) not in (1, 2, 4, 8) for c in live)                   # border == tile, not a power of two
        assert any(border(c) < length(c) < 2 * border(c) for c in live)                                      # overlapping ramps
        assert any(length(c) >= 2 * border(c) for c in live)
        assert any(length(c) < border(c) for c in cases if not free(c))                                      # no ramp: any border goes
    two_ramps_h = [c for c in cases if c.bits & 3 == 0 and c.bh < c.th < 2 * c.bh]
    two_ramps_w = [c for c in cases if c.bits & 12 == 0 and c.bw < c.tw < 2 * c.bw]
    assert two_ramps_h and two_ramps_w                                 # both ramps present AND overlapping
    # the reference builds every accepted case, and the ramps of a border that is no power of two are inexact in fp32: the quotient matters
    for c in cases:
        m = wan_vae.tile_mask(c.th, c.tw, tile_bounds(c.bits), (c.bh, c.bw))
        assert m.shape == (1, 1, 1, c.th, c.tw) and (m > 0).all() and (m <= 1).all()
    assert any(float(torch.tensor(k / b, dtype=torch.float32)) != k / b for b in (3, 5, 6, 7, 12) for k in range(1, b))


@gpu
@pytest.mark.parametrize("bits", range(16))
def test_tile_accumulate_single_tile(hip, bits):
    for i, c in enumerate(tile_cases(bits)):
        tile, values, weight, want_v, want_w = tile_reference(c, 5000 + 100 * bits + 3 * i)
        dv, dw = dev(values), dev(weight)
        hip.vae_tile_accumulate(dev(tile), dv, dw, c.y0, c.x0, c.bh, c.bw, tile_bounds(bits))
        assert torch.equal(dw.cpu(), want_w), f"weight: {vars(c)}"
        assert torch.equal(dv.cpu(), want_v), f"values: {vars(c)}"


@gpu
@pytest.mark.parametrize("bits", range(15))
def test_tile_accumulate_refuses_a_border_wider_than_the_tile(hip, bits):
    """A ramp needs `border` pixels of the tile: with a free side on an axis and border > tile the reference's slice assignment raises,
    and the launcher returns FG_EINVAL without touching the canvas."""
    lib = hip.load()
    for axis, free in (("h", bits & 3 != 3), ("w", bits & 12 != 12)):
        if not free:
            continue
        for border in (2, 7):
            th, tw = (border - 1, 9) if axis == "h" else (9, border - 1)
            bh, bw = (border, 2) if axis == "h" else (2, border)
            with pytest.raises(RuntimeError):
                wan_vae.tile_mask(th, tw, tile_bounds(bits), (bh, bw))
            tile = dev(seeded((3, 1, th, tw), 6000))
            values, weight = seeded((3, 1, 12, 13), 6001), seeded((1, 12, 13), 6002)
            dv, dw = dev(values), dev(weight)
            rc = lib.fg_vae_tile_accumulate_bf16(hip._ptr(tile), hip._ptr(dv), hip._ptr(dw), 3, 1, 12, 13, th, tw, 1, 3, bh, bw, bits,
                                                 hip._stream(tile))
            torch.cuda.synchronize()
            assert rc == FG_EINVAL, f"bound_bits {bits}, border_{axis} {border} on a tile of {th} x {tw}: accepted"
            assert torch.equal(dv.cpu(), values) and torch.equal(dw.cpu(), weight)


# (latent H, W, tile_size, tile_stride): (size - stride) * 16 = (48, 80) and (80, 48)
WALKS = [(7, 9, (5, 7), (2, 2)), (9, 7, (7, 5), (2, 2))]
WALK_UP, WALK_F = 16, 2


@functools.lru_cache(maxsize=None)
def walk_reference(i):
    H, W, size, stride = WALKS[i]
    up = WALK_UP
    border = ((size[0] - stride[0]) * up, (size[1] - stride[1]) * up)
    values = torch.zeros((3, WALK_F, H * up, W * up), dtype=BF16)
    weight = torch.zeros((WALK_F, H * up, W * up), dtype=BF16)
    steps = []
    for k, (h, h_, w, w_) in enumerate(wan_vae.tile_tasks(H, W, size, stride)):
        th, tw = (min(h_, H) - h) * up, (min(w_, W) - w) * up
        tile = seeded((3, WALK_F, th, tw), 7000 + 10 * i + k)
        bounds = (h == 0, h_ >= H, w == 0, w_ >= W)
        m = wan_vae.tile_mask(th, tw, bounds, border).to(BF16)[0, 0]
        values[:, :, h * up:h * up + th, w * up:w * up + tw] += tile * m
        weight[:, h * up:h * up + th, w * up:w * up + tw] += m[0]
        steps.append((tile, h * up, w * up, bounds))
    return border, steps, values, weight


@pytest.mark.parametrize("i", range(len(WALKS)))
def test_tile_walk_geometry(i):
    border, steps, values, weight = walk_reference(i)
    assert border == ((48, 80), (80, 48))[i] and len(steps) == 4
    assert (weight > 0).all()                                           # every pixel under a tile: no 0 / 0 in the reference
    assert (values.abs() > 1).any()                                     # the clamp has something to do after the division
    assert ((values / weight).abs() > 1).any()


@gpu
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("i", range(len(WALKS)))
def test_tile_walk_and_finalize(hip, i, clamp):
    border, steps, values, weight = walk_reference(i)
    dv, dw = dev(torch.zeros_like(values)), dev(torch.zeros_like(weight))
    for tile, y0, x0, bounds in steps:
        hip.vae_tile_accumulate(dev(tile), dv, dw, y0, x0, border[0], border[1], bounds)
    assert torch.equal(dv.cpu(), values) and torch.equal(dw.cpu(), weight)
    assert (dw > 0).all()
    hip.vae_tile_finalize(dv, dw, clamp)
    want = values / weight
    assert torch.equal(dv.cpu(), want.clamp(-1, 1) if clamp else want)
    assert torch.equal(dw.cpu(), weight)


# ------------------------------------------------------------------------------------------------------------ 4. AvgDown3D + add
AVG_PAIRS = [(160, 160), (160, 320), (320, 640), (640, 640), (96, 64), (32, 64)]
AVG_T, AVG_H, AVG_W = (1, 2, 3, 5), 6, 10
AVG_CASES = [(cin, cout, ft, fs) for cin, cout in AVG_PAIRS for ft in (1, 2) for fs in (1, 2) if (cin * ft * fs * fs) % cout == 0]


def avg_group(cin, cout, ft, fs):
    return cin * ft * fs * fs // cout


@functools.lru_cache(maxsize=None)
def avg_exact_case(cin, cout, ft, fs, T):
    """Integer-valued x and main: every fp32 partial sum is an integer below 2^24, so the kernel's sum is exact in any order.
    Expectation: bf16(main + bf16(mean)) with the mean in fp64."""
    x = seeded_int((1, cin, T, AVG_H, AVG_W), 8000 + cin + T)
    mean = wan_vae.avg_down3d(x.double(), cout, ft, fs)
    main = seeded_int(tuple(mean.shape), 8001 + cout + T)
    return x, main, mean, (main.double() + rbf64(mean)).to(BF16)


def test_avgdown_case_table():
    assert len(AVG_CASES) == 20 and all((2, 1) in {(ft, fs) for ci, co, ft, fs in AVG_CASES if (ci, co) == pair} for pair in AVG_PAIRS)
    groups = {avg_group(*c) for c in AVG_CASES}
    assert groups == {1, 2, 3, 4, 6, 8, 12}


@pytest.mark.parametrize("cin,cout,ft,fs", AVG_CASES)
def test_avgdown_exact_inputs(cin, cout, ft, fs):
    group = avg_group(cin, cout, ft, fs)
    for T in AVG_T:
        x, main, mean, want = avg_exact_case(cin, cout, ft, fs, T)
        assert torch.equal(x.double(), x.double().round()) and x.abs().max() <= 64 and torch.equal(main.double(), main.double().round())
        total = mean * group                                    # the integer sums the kernel accumulates in fp32
        assert torch.equal(total, total.round()) and total.abs().max() < 2 ** 24
        if group & (group - 1) == 0:                            # the quotient is exact in fp32: nothing but the two bf16 roundings is left
            assert torch.equal(mean.float().double(), mean)
        else:                                                   # fp32 and fp64 quotients round to the same bf16
            assert torch.equal((total.float() / float(group)).to(BF16), mean.to(BF16))
        assert torch.equal((main.float() + rbf64(mean).float()).to(BF16), want)         # the fp32 sum of two bf16 rounds like the fp64 one
        if T % ft:
            assert (T + ft - 1) // ft == mean.shape[2]          # a padded leading frame


@gpu
@pytest.mark.parametrize("cin,cout,ft,fs", AVG_CASES)
def test_avgdown3d_add_shapes(hip, cin, cout, ft, fs):
    for T in AVG_T:
        what = f"avgdown {cin}->{cout} ft{ft} fs{fs} T{T}"
        x, main, _, want = avg_exact_case(cin, cout, ft, fs, T)
        got = hip.avgdown3d_add(dev(_cl(x)), dev(_cl(main)), ft, fs)
        assert torch.equal(_ncthw(got.cpu()), want), what + ": integer inputs"
        xs = seeded((1, cin, T, AVG_H, AVG_W), 8100 + cin + T)
        sc = wan_vae.avg_down3d(xs, cout, ft, fs)
        main = seeded(tuple(sc.shape), 8101 + cout + T)
        got = hip.avgdown3d_add(dev(_cl(xs)), dev(_cl(main)), ft, fs)
        assert_close_bf16(_ncthw(got.cpu()), main + sc, 1.0, what, mag=main, max_mismatch=0.02)


# ------------------------------------------------------------------------------------------------------------ 5. layout kernels
LAYOUT_THW = (3, 5, 7)
SENTINEL = 7.5


def latent_stats(Z, stock):
    if stock:
        return torch.tensor(wan_vae.VAE38_MEAN[:Z]).to(BF16), (1.0 / torch.tensor(wan_vae.VAE38_STD[:Z])).to(BF16)
    return seeded((Z,), 9000 + Z, scale=0.3), (seeded((Z,), 9001 + Z).abs() + 0.5).to(BF16)


@gpu
@pytest.mark.parametrize("stock", [False, True])
@pytest.mark.parametrize("Z", [16, 48])
def test_latent_layout_shapes(hip, Z, stock):
    T, H, W = LAYOUT_THW
    mean, inv_std = latent_stats(Z, stock)
    assert (inv_std > 0).all()
    mv, sv = mean.view(1, Z, 1, 1, 1), inv_std.view(1, Z, 1, 1, 1)
    z = seeded((1, Z, T, H, W), 9100 + Z)
    got = hip.vae_latent_to_cl(dev(z[0].contiguous()), dev(mean), dev(inv_std))
    assert got.shape == (T, H, W, Z) and torch.equal(_ncthw(got.cpu()), z / sv + mv)
    for Cx in (2 * Z, 2 * Z + 8):
        h = seeded((1, Cx, T, H, W), 9200 + Cx)
        got = hip.vae_latent_from_cl(dev(_cl(h)), dev(mean), dev(inv_std), Z)
        assert got.shape == (Z, T, H, W) and torch.equal(got.cpu().unsqueeze(0), (h[:, :Z] - mv) * sv), f"Z={Z} Cx={Cx}"


@gpu
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("T", [1, 3])
def test_unpatchify_frame_windows(hip, T, clamp):
    H, W, F_ = 5, 7, T + 4
    x = seeded((1, 12, T, H, W), 9300 + T, scale=0.8)
    assert (x.abs() > 1).any()
    want = wan_vae.unpatchify2(x)[0]
    want = want.clamp(-1, 1) if clamp else want
    for t0 in (0, 2, F_ - T):
        video = torch.full((3, F_, 2 * H, 2 * W), SENTINEL, dtype=BF16, device="cuda")
        hip.vae_unpatchify(dev(_cl(x)), video, t0, clamp)
        video = video.cpu()
        assert torch.equal(video[:, t0:t0 + T], want), f"t0={t0}"
        assert (video[:, :t0] == SENTINEL).all() and (video[:, t0 + T:] == SENTINEL).all(), f"t0={t0}: frames outside the window written"


@gpu
@pytest.mark.parametrize("T", [1, 3])
def test_patchify_shapes(hip, T):
    h, w = 5, 7
    vid = seeded((1, 3, T, 2 * h, 2 * w), 9400 + T, scale=0.5)
    video = dev(vid[0].contiguous())
    out = torch.full((T, h, w, 16), SENTINEL, dtype=BF16, device="cuda")
    hip._call("fg_vae_patchify_bf16", hip._ptr(video), hip._ptr(out), T, 2 * h, 2 * w, hip._stream(video))
    out = out.cpu()
    assert torch.equal(_ncthw(out[..., :12]), wan_vae.patchify2(vid))
    assert not out[..., 12:].any()
    assert torch.equal(hip.vae_patchify(video).cpu(), out)


# ------------------------------------------------------------------------------------------------------------ 6. uint8 frames
def all_finite_bf16():
    """Every finite bf16 value once, as (3, 1, 160, 136): bit patterns 0x0000..0x7F7F and 0x8000..0xFF7F."""
    bits = torch.cat([torch.arange(0x0000, 0x7F80), torch.arange(0x8000, 0xFF80)])
    return (bits - ((bits >= 0x8000) * 0x10000)).to(torch.int16).view(BF16).reshape(3, 1, 160, 136)


def test_uint8_domain():
    v = all_finite_bf16()
    assert v.numel() == 65280 and torch.isfinite(v.float()).all()
    assert torch.unique(v.view(torch.int16)).numel() == 65280
    want = opipe.video_to_uint8(v)
    assert want.shape == (1, 160, 136, 3) and torch.unique(want).numel() == 256          # every level is reached


@gpu
def test_video_to_uint8_every_finite_bf16(hip):
    """(x + 1) * 127.5 in bf16 steps, the clip and the truncation on the kernel's whole finite domain.  NaNs and infinities are left out:
    the pipeline hands over decoded frames, and a cast of NaN to uint8 has no defined value to compare."""
    v = all_finite_bf16()
    assert torch.equal(hip.video_to_uint8(dev(v)).cpu(), opipe.video_to_uint8(v))

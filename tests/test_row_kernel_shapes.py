"""The one-wave-per-row kernels at every width, head size and modulation-table layout their dispatch distinguishes.

A lane of these kernels owns the 8-element vectors lane + i * 64 (lane + i * 32 in the narrow VAE form) of a row, `vi < nvec` guards
the ragged end, and the launcher changes kernel or template at a width boundary.  The older tests meet them at C in {3072, 1536,
256}, head_dim 128 and table splits in the interior only.  Here every width list holds a row that fits in one lane, one that ends
inside the first lane step, exactly on a step, one vector past a step, mid-way through the steps, one vector short of the limit and
at the limit; data is `seeded` N(0, 1) at the scales of the older tests, every case of a sweep has >= 16 384 elements (one flipped
rounding is 6e-5 of a case, far below the 2e-3 mismatch cap) and a row count that is no multiple of the 4 rows of a workgroup.

Criteria (the project's own, none new): norm kernels within 1 bf16 ulp of the oracle's bf16 result (mag = the shift / bias) with at
most 2e-3 of the elements different; gate_residual and every x_out torch.equal to the bf16 expression; fp8 / dual outputs
torch.equal to fp8_quant_rows of the plain kernel's row, the dual bf16 row torch.equal to the plain kernel's; fp8_quant_rows
torch.equal to the reference's torch expression (with GELU: test_fp8_quant_rows' allowances).

Covered per entry point, and how each form was confirmed:
  fg_ln_modulate_bf16, fg_ln_affine_bf16, fg_gate_residual_bf16 (gated, plain), fg_residual_ln_bf16 (modulate with gate + norm_mod,
  modulate without gate, affine), fg_ln_modulate_fp8_bf16, fg_ln_modulate_dual_bf16, fg_ln_affine_dual_bf16, fg_residual_ln_fp8_bf16
  (modulate, affine), fg_rmsnorm_rope_bf16 without a table
                     C in {8, 64, 504, 512, 520, 1544, 4088, 4096} (64 lanes x 8 vectors: limit 4096); refused: 4104 and C % 8 != 0.
                     One kernel each, no switch: the width only moves the `vi < nvec` guard.
  fg_fp8_quant_rows_bf16   the same widths on fp8_quant_rows_kernel<8>, and {4104, 14328, 14336} on <28> (the launcher's
                     `C <= 4096` rule, csrc/fp8_linear.hip; the last two are one vector short of / at its limit); with and without
                     gelu_tanh, on a column slice (ld = C + 64); refused: 14344 and C % 8 != 0.
  fg_vae_rmsnorm_silu_bf16   C in {8, 160, 248, 256} on the 32-lane form (two pixels per wave; odd pixel counts: the last wave's
                     second half is dead and still shuffles) and {264, 320, 512, 520, 640, 2040, 2048} on the 64-lane form (4 vectors: limit
                     2048), by the launcher's `C <= 256` rule (csrc/vae_ops.hip); SiLU on and off; one call with a single pixel per
                     form; refused: 2056 and C % 8 != 0.
  fg_rmsnorm_rope_bf16 with tables   head_dim in {8, 16, 64, 128, 256, 512, 1024, 24, 48, 96, 192, 1000}, one head and several, x a
                     column slice with ld = 3C, tables from random angles (fp64 cos / sin, and the same values rounded once to the
                     interleaved fp32 table).  The form of a case is computed in the test from the launcher's rule (plain =
                     head_dim a power of two; hoist = fp32 table and 512 % head_dim == 0) and asserted before the call:
                     fp32 table: plain + hoist (8 .. 512), plain + no hoist (1024), non-plain + no hoist (24, 48, 96, 192, 1000);
                     fp64 tables: plain and non-plain; the hoist exists only with the fp32 table (rope_begin), so fp64 has no
                     hoisted form to hit.  Non-plain + hoist cannot come from this entry point (512 % head_dim == 0 makes head_dim
                     a power of two); the grouped entry point, always non-plain, runs it at head_dim 128.
  fg_rmsnorm_rope_grouped_bf16   head_dim in {128, 96, 48}, 4 heads, group_cols in {head_dim, 2 head_dim, C}, both table modes:
                     equal to the plain call's columns bit for bit, in a destination pre-filled with a sentinel whose padding
                     (group_cols .. out_ld) and rows past the shard stay untouched.
  Modulation tables  C = 520, rows in {1, 2, 3, 4, 5, 9}, mod_rows in {1, 2, rows}, first_rows in {0, 1, rows - 1, rows} on
                     ln_modulate, gate_residual, residual_ln_modulate (distinct gate and norm tables), ln_modulate_fp8,
                     ln_modulate_dual; the GEMM epilogue's gate (mode 2) at M = 9.  The expectation indexes the table on the host.
                     mod_rows == rows == 2 is pinned as the TI2V split (hip.ModTable, include/fairygen_hip.h); a per-token table
                     of two rows goes through ModTable(per_token=True).

The unmarked self-checks run on a CPU-only machine: an emulation of each kernel's chain (fp64 row statistics, then the rounding
points of norm_store, rope_vec and vae_rmsnorm_kernel in fp32) meets the same criterion against the oracle on every case, so the
inputs leave the 2e-3 cap to the kernel; the form rule covers the forms claimed above; every sweep case has >= 16 384 elements.
The emulation also runs with its statistic moved by +-4e-7, and a case whose chain leaves the 1-ulp bound there takes its next
inputs (STAT_ERRORS below says why: such an element fails every correct kernel, and one did on the GPU); the rounding points of the
affine form count `n * w + b` as one FMA, which is how the compiler contracts it.  Where a wrapper takes no output tensor
(ln_modulate_fp8, fp8_quant_rows, the fp8 pair of the residual forms) the refusal test can only hold the error, not an untouched output.

Cost: the self-checks take 2 s of pytest time on a 16-thread host, the GPU cases (CPU references included, shared with the
self-checks through the case cache) 3 s on an MI355X, none above 0.3 s; the largest tensor is 5 rows of 14 336 + 64 columns.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import seeded
from oracle import wan_dit, wan_vae
from test_hip_kernels import _cl, _ncthw, assert_close_bf16, dev, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
EPS = 1e-6
MIN_ELEMS = 16384

W8 = [8, 64, 504, 512, 520, 1544, 4088, 4096]                     # 64 lanes x 8 vectors: limit 4096
W_FP8 = W8 + [4104, 14328, 14336]                                  # <8> up to 4096, <28> up to 14336
W_VAE = [8, 160, 248, 256, 264, 320, 512, 520, 640, 2040, 2048]              # 32 lanes x 1 vector up to 256, 64 lanes x 4 vectors up to 2048
LIMIT8, LIMIT_FP8, LIMIT_VAE = 4096, 14336, 2048
# (head_dim, heads): every head size alone and with several heads; C = 40, 48, 320, 384, 768, 120, 336, 576, 1344, 4000 end inside a lane step
ROPE_CASES = [(8, 1), (8, 5), (16, 1), (16, 3), (64, 1), (64, 5), (128, 1), (128, 3), (256, 1), (256, 3), (512, 1), (512, 3),
              (1024, 1), (1024, 4), (24, 1), (24, 5), (48, 1), (48, 7), (96, 1), (96, 6), (192, 1), (192, 7), (1000, 1), (1000, 4)]
GROUPED_HD = [128, 96, 48]
TABLE_C, TABLE_ROWS = 520, [1, 2, 3, 4, 5, 9]


def rows_for(C):
    """Smallest row count >= 5 (a second workgroup) that is no multiple of 4 and gives the case MIN_ELEMS elements."""
    r = max(5, -(-MIN_ELEMS // C))
    return r + 1 if r % 4 == 0 else r


def pixels_for(C):
    """rows_for, and odd on the 32-lane form (C <= 256): the last wave holds one live pixel next to a dead half."""
    p = rows_for(C)
    return p + 1 if C <= 256 and p % 2 == 0 else p


def rbf(t):
    return t.to(BF16).float()


def rope_form(hd, f32tab):
    """The launcher's rule (fg_rmsnorm_rope_bf16, rope_begin): (plain, hoist)."""
    return (hd & (hd - 1)) == 0, bool(f32tab) and 512 % hd == 0


def mod_index(rows, mod_rows, first):
    """Table row of every token row, by the convention of include/fairygen_hip.h (two rows: always the split)."""
    if mod_rows == 1:
        return torch.zeros(rows, dtype=torch.long)
    if mod_rows == 2:
        return (torch.arange(rows) >= first).long()
    assert mod_rows == rows
    return torch.arange(rows)


# --------------------------------------------------------------------------- CPU emulations of the kernels' chains (fp64 row statistics)
# `rel`: relative error put on the row statistic (1 / std, 1 / rms, the sum of squares).  A correct kernel differs from the oracle
# there: an fp32 statistic summed in lane order and reduced by a butterfly is within ~1 fp32 ulp (1.2e-7) of the exact one, the
# two fp32 roundings of (x - mean) * rstd add 6e-8 each, and so does the emulation's own rounding of the fp64 value: 3e-7 between the
# two normalised values, 4e-7 with a margin.  Where that value lies so close to a bf16
# rounding boundary, the FIRST rounding of the chain flips, and under a factor below 1 (|1 + scale| < 1, a weight below 1, a rotation
# that cancels) one ulp of the larger intermediate is two of the smaller result: beyond the criterion for every correct implementation
# (met on the GPU at C = 1544, row 6: an fp32 replay of the kernel's summation order on the CPU gives the same two elements).
# About one element in 40 000 is such a knife edge.  The inputs of a case are therefore drawn again (salt 0, 1, 2, ...) until every
# chain of the case meets the criterion at rel = 0 and +-4e-7: a property of the inputs and the oracle, decided on the CPU.
STAT_ERRORS = (0.0, 4e-7, -4e-7)
MAX_SALT = 40


def first_robust(build, check):
    """build(salt) for the first salt whose case passes check (the emulated chains against the oracle at every STAT_ERRORS)."""
    for salt in range(MAX_SALT):
        c = build(salt)
        try:
            check(c)
        except AssertionError:
            continue
        c.salt = salt
        return c
    raise RuntimeError("no robust inputs found")


def emu_ln(x, p0, p1, mode, rel=0.0):
    """norm_store: MODE 0 (p0 = shift, p1 = scale) / MODE 1 (p0 = weight, p1 = bias) on rows x (..., C); p0, p1 broadcast to x."""
    xf, xd = x.float(), x.double()
    mean = xd.mean(-1, keepdim=True)
    rstd = (1.0 + rel) / torch.sqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + EPS)
    n = (xf - mean.float()) * rstd.float()
    if mode == 0:
        return (rbf(rbf(n) * rbf(1.0 + p1.float())) + p0.float()).to(BF16)
    return (n.double() * p0.double() + p1.double()).float().to(BF16)          # n * w + b contracts to one FMA


def emu_rmsnorm_rope(x, w, heads, cos=None, sin=None, f32tab=False, rel=0.0):
    """rope_begin + rope_vec on x (1, rows, C); cos, sin (rows, head_dim / 2) fp64 (rounded once to fp32 with f32tab)."""
    xf = x.float()
    rinv = ((1.0 + rel) / torch.sqrt((x.double() ** 2).mean(-1, keepdim=True) + EPS)).float()
    o = rbf(rbf(xf * rinv) * w.float())
    if cos is None:
        return o.to(BF16)
    b, s, _ = x.shape
    o = o.reshape(b, s, heads, -1, 2)
    a, bb = o[..., 0], o[..., 1]
    cc, sn = cos.view(s, 1, -1), sin.view(s, 1, -1)
    if f32tab:
        cc, sn = cc.float(), sn.float()
        r0 = (a.double() * cc.double() - (bb * sn).double()).float()          # fmaf(a, c, -(b * s))
        r1 = (a.double() * sn.double() + (bb * cc).double()).float()          # fmaf(a, s, b * c)
    else:
        r0, r1 = a.double() * cc - bb.double() * sn, a.double() * sn + bb.double() * cc
    return torch.stack([r0, r1], dim=-1).flatten(2).to(BF16)


def emu_vae(x, gamma, silu, rel=0.0):
    """vae_rmsnorm_kernel on x (pixels, C), gamma (C,)."""
    xf = x.float()
    denom = rbf(torch.sqrt((x.double() ** 2).sum(-1, keepdim=True) * (1.0 + rel)).float()).clamp_min(1e-12)
    sqrt_c = torch.tensor(float(x.shape[-1]), dtype=torch.float32).sqrt()
    y = rbf(rbf(rbf(xf / denom) * sqrt_c) * gamma.float())
    if silu:
        y = y / (1.0 + torch.exp(torch.clamp(-y, max=80.0)))
    return y.to(BF16)


# --------------------------------------------------------------------------------------------- cases (inputs and references, built once)
def _ln_build(C, salt):
    """Inputs of the LayerNorm family at width C and the oracle's results: a two-row table split at rows // 3, an affine pair, and
    `planted` copies (one shift / bias of 900) for the fp8 and dual outputs."""
    rows = rows_for(C)
    c = SimpleNamespace(C=C, rows=rows, first=rows // 3)
    c.x, c.y = seeded((1, rows, C), 1000 + C + 100000 * salt), seeded((1, rows, C), 2000 + C)
    c.table, c.table2 = seeded((2, 6, C), 3000 + C, scale=0.5), seeded((2, 6, C), 4000 + C, scale=0.5)
    c.w, c.b = (1 + 0.1 * seeded((C,), 5000 + C)).to(BF16), (0.1 * seeded((C,), 6000 + C)).to(BF16)
    c.planted, c.b_planted = c.table.clone(), c.b.clone()
    c.planted[1, 0, min(7, C - 1)] = c.planted[0, 3, min(9, C - 1)] = 900.0
    c.b_planted[min(11, C - 1)] = 900.0
    c.idx = mod_index(rows, 2, c.first)
    row = lambda t, j: t[c.idx, j].unsqueeze(0)      # noqa: E731
    c.shift, c.scale = row(c.table, 0), row(c.table, 1)
    c.want_mod = wan_dit.layer_norm(c.x, EPS) * (1 + c.scale) + c.shift
    c.want_aff = wan_dit.layer_norm(c.x, EPS, c.w, c.b)
    c.x_gated, c.x_plain, c.x_gated2 = c.x + row(c.table, 5) * c.y, c.x + c.y, c.x + row(c.table, 2) * c.y
    c.shift2, c.scale2 = row(c.table2, 0), row(c.table2, 1)
    c.want_res_mod = wan_dit.layer_norm(c.x_gated, EPS) * (1 + c.scale2) + c.shift2
    c.shift3, c.scale3 = row(c.table, 3), row(c.table, 4)
    c.want_res_plain = wan_dit.layer_norm(c.x_plain, EPS) * (1 + c.scale3) + c.shift3
    c.want_res_aff = wan_dit.layer_norm(c.x_gated2, EPS, c.w, c.b)
    c.want_rms = wan_dit.rms_norm(c.x, c.w, EPS)
    return c


def _ln_check(c):
    for rel in STAT_ERRORS:
        assert_close_bf16(emu_ln(c.x, c.shift, c.scale, 0, rel), c.want_mod, 1.0, f"ln_modulate {rel}", mag=c.shift)
        assert_close_bf16(emu_ln(c.x, c.w, c.b, 1, rel), c.want_aff, 1.0, f"ln_affine {rel}", mag=c.b)
        assert_close_bf16(emu_ln(c.x_gated, c.shift2, c.scale2, 0, rel), c.want_res_mod, 1.0, f"res+modulate {rel}", mag=c.shift2)
        assert_close_bf16(emu_ln(c.x_plain, c.shift3, c.scale3, 0, rel), c.want_res_plain, 1.0, f"res+modulate (no gate) {rel}", mag=c.shift3)
        assert_close_bf16(emu_ln(c.x_gated2, c.w, c.b, 1, rel), c.want_res_aff, 1.0, f"res+affine {rel}", mag=c.b)
        assert_close_bf16(emu_rmsnorm_rope(c.x, c.w, 1, rel=rel), c.want_rms, 1.0, f"rmsnorm {rel}")


@functools.lru_cache(maxsize=None)
def ln_case(C):
    return first_robust(functools.partial(_ln_build, C), _ln_check)


def _rope_build(hd, heads, salt):
    C = hd * heads
    rows = rows_for(C)
    c = SimpleNamespace(hd=hd, heads=heads, C=C, rows=rows)
    c.wide = seeded((1, rows, 3 * C), 7000 + C + 100000 * salt)
    c.wt = (1 + 0.1 * seeded((C,), 8000 + C)).to(BF16)
    g = torch.Generator("cpu").manual_seed(9000 + C)
    angle = (torch.rand((rows, 1, hd // 2), generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    table = torch.polar(torch.ones_like(angle), angle)
    c.cos, c.sin = table.real.reshape(rows, -1).contiguous(), table.imag.reshape(rows, -1).contiguous()
    c.cs = torch.stack([c.cos, c.sin], dim=-1).to(torch.float32).contiguous()
    c.xq = c.wide[..., C:2 * C]
    c.want = wan_dit.rope_apply(wan_dit.rms_norm(c.xq, c.wt, EPS), table, heads)
    return c


def _rope_check(c):
    for rel in STAT_ERRORS:
        assert_close_bf16(emu_rmsnorm_rope(c.xq, c.wt, c.heads, c.cos, c.sin, rel=rel), c.want, 1.0, f"rmsnorm+rope (fp64) {rel}")
        assert_close_bf16(emu_rmsnorm_rope(c.xq, c.wt, c.heads, c.cos, c.sin, f32tab=True, rel=rel), c.want, 1.0, f"rmsnorm+rope (fp32 table) {rel}")


@functools.lru_cache(maxsize=None)
def rope_case(hd, heads):
    return first_robust(functools.partial(_rope_build, hd, heads), _rope_check)


def _vae_build(C, pixels, salt):
    c = SimpleNamespace(C=C, pixels=pixels)
    c.x = seeded((1, C, 1, 1, pixels), 10000 + C + 100000 * salt, scale=2.0)
    c.g = (1 + 0.1 * seeded((C, 1, 1, 1), 11000 + C)).to(BF16)
    c.want = wan_vae.rms_norm_c({"n.gamma": c.g}, "n", c.x)
    c.want_silu = F.silu(c.want)
    return c


def _vae_check(c):
    x2 = _cl(c.x).reshape(-1, c.C)
    for silu, want, rel in ((s, w, r) for s, w in ((False, c.want), (True, c.want_silu)) for r in STAT_ERRORS):
        got = emu_vae(x2, c.g.view(-1), silu, rel).view(1, 1, c.pixels, c.C)
        assert_close_bf16(_ncthw(got), want, 1.0, f"vae rmsnorm C={c.C} pixels={c.pixels} silu={silu} {rel}")


@functools.lru_cache(maxsize=None)
def vae_case(C, pixels=None):
    return first_robust(functools.partial(_vae_build, C, pixels_for(C) if pixels is None else pixels), _vae_check)


def table_cases():
    """(rows, mod_rows, first_rows) of the layout sweep, duplicates removed."""
    out = []
    for rows in TABLE_ROWS:
        for mod_rows in sorted({1, 2, rows}):
            for first in sorted({0, 1, rows - 1, rows}):
                if 0 <= first <= rows:
                    out.append((rows, mod_rows, first))
    return out


def _table_build(rows, mod_rows, first, salt):
    C = TABLE_C
    c = SimpleNamespace(C=C, rows=rows, mod_rows=mod_rows, first=first)
    c.x, c.y = seeded((1, rows, C), 12000 + rows + 100000 * salt), seeded((1, rows, C), 12100 + rows)
    c.table, c.table2 = seeded((mod_rows, 6, C), 12200 + mod_rows, scale=0.5), seeded((mod_rows, 6, C), 12300 + mod_rows, scale=0.5)
    for t in (c.table, c.table2):              # every table row differs visibly: row r sits r + 1 above / below in all six vectors
        t += (torch.arange(mod_rows, dtype=torch.float32).view(-1, 1, 1) + 1).to(BF16) * (1 if t is c.table else -1)
    c.idx = mod_index(rows, mod_rows, first)
    row = lambda t, j: t[c.idx, j].unsqueeze(0)      # noqa: E731
    c.shift, c.scale = row(c.table, 0), row(c.table, 1)
    c.want_mod = wan_dit.layer_norm(c.x, EPS) * (1 + c.scale) + c.shift
    c.x_gated = c.x + row(c.table, 5) * c.y
    c.shift2, c.scale2 = row(c.table2, 0), row(c.table2, 1)
    c.want_res_mod = wan_dit.layer_norm(c.x_gated, EPS) * (1 + c.scale2) + c.shift2
    return c


def _table_check(c):
    for rel in STAT_ERRORS:
        assert_close_bf16(emu_ln(c.x, c.shift, c.scale, 0, rel), c.want_mod, 1.0, f"ln_modulate {rel}", mag=c.shift)
        assert_close_bf16(emu_ln(c.x_gated, c.shift2, c.scale2, 0, rel), c.want_res_mod, 1.0, f"res+modulate {rel}", mag=c.shift2)


@functools.lru_cache(maxsize=None)
def table_case(rows, mod_rows, first):
    return first_robust(functools.partial(_table_build, rows, mod_rows, first), _table_check)


# ----------------------------------------------------------------------------------------------------------------- host self-checks
def test_case_sizes_and_lists():
    """Every sweep case has >= 16 384 elements and a row count that is no multiple of 4; the width lists hold the seven conditions
    of their kernels (derived from the lane count, the vectors per lane and the limit, not copied)."""
    for C in W8 + W_FP8:
        assert rows_for(C) * C >= MIN_ELEMS and rows_for(C) % 4 and rows_for(C) >= 5
    for C in W_VAE:
        assert pixels_for(C) * C >= MIN_ELEMS and pixels_for(C) % 4 and (C > 256 or pixels_for(C) % 2)
    for hd, heads in ROPE_CASES:
        assert rows_for(hd * heads) * hd * heads >= MIN_ELEMS and hd * heads <= LIMIT8

    def conditions(widths, lanes, nvec, lo=0):
        step, limit = lanes * 8, lanes * 8 * nvec
        ws = [w for w in widths if w > lo]
        assert all(w % 8 == 0 and w <= limit for w in ws)
        return {"one lane": any(w == 8 for w in widths), "inside first step": any(8 < w < step for w in widths),
                "on a step": any(w % step == 0 and w < limit for w in ws), "one past a step": any(w % step == 8 and w > step for w in ws),
                "mid-way": any(step + 8 < w < limit - step for w in ws),
                "one short of the limit": limit - 8 in ws, "limit": limit in ws}
    assert all(conditions(W8, 64, 8).values()), conditions(W8, 64, 8)
    assert all(conditions(W_VAE, 64, 4, lo=256).values()), conditions(W_VAE, 64, 4, lo=256)
    big = conditions(W_FP8, 64, 28, lo=LIMIT8)          # the <28> kernel starts one vector past the <8> limit
    assert big["one past a step"] and big["one short of the limit"] and big["limit"], big
    narrow = [w for w in W_VAE if w <= 256]            # 32 lanes x 1 vector: one lane, inside the step, one short, the limit = the switch
    assert 8 in narrow and 248 in narrow and 256 in narrow and 264 in W_VAE and any(8 < w < 248 for w in narrow)
    assert LIMIT8 in W_FP8 and LIMIT8 + 8 in W_FP8      # the <8> / <28> switch


def test_rope_form_rule_covers_the_forms():
    hds = sorted({hd for hd, _ in ROPE_CASES})
    assert hds == sorted([8, 16, 64, 128, 256, 512, 1024, 24, 48, 96, 192, 1000])
    for hd in hds:
        assert any(h == hd and n == 1 for h, n in ROPE_CASES) and any(h == hd and n > 1 for h, n in ROPE_CASES)
    f32 = {rope_form(hd, True) for hd in hds}
    f64 = {rope_form(hd, False) for hd in hds}
    assert f32 == {(True, True), (True, False), (False, False)}          # non-plain + hoist cannot exist: 512 % hd == 0 => power of two
    assert f64 == {(True, False), (False, False)}                        # the hoist is a property of the fp32 table
    assert sum(1 for C in {hd * n for hd, n in ROPE_CASES} if C % 512) >= 2          # widths that end inside a lane step
    assert all(rope_form(hd, True)[1] for hd in GROUPED_HD if 512 % hd == 0) and 128 in GROUPED_HD


def test_table_rows_differ_and_rows2_rule():
    """Any two rows of a layout-sweep table differ, in more than 80 % of their elements, by more than 3 bf16 ulps of the table's largest
    value (the cap on differing elements is 0.2 %: a wrong row index cannot pass), and hip._mod_args resolves the rows == mod_rows == 2 case: the split by default, first_rows = 1 per token."""
    for rows, mod_rows, first in table_cases():
        c = table_case(rows, mod_rows, first)
        for t in (c.table, c.table2):
            assert t.float().abs().max().item() < 16
            for i in range(mod_rows):
                for j in range(i):
                    d = (t[i].float() - t[j].float()).abs()
                    assert (d > 3 * 2.0 ** -7 * 16).float().mean().item() > 0.8 and d.mean().item() > 0.9
    from fairygen_amd import hip as h
    mod = SimpleNamespace(mod_rows=2, first_rows=0, ld=6 * TABLE_C, per_token=False)
    assert h._mod_args(mod, 2) == (2, 0, mod.ld) and h._mod_args(mod, 9) == (2, 0, mod.ld)
    mod.per_token = True
    assert h._mod_args(mod, 2) == (2, 1, mod.ld)
    with pytest.raises(h.HipLibraryError):
        h._mod_args(mod, 9)
    assert h._mod_args(SimpleNamespace(mod_rows=9, first_rows=4, ld=8, per_token=True), 9) == (9, 0, 8)
    assert h._mod_args(SimpleNamespace(mod_rows=1, first_rows=0, ld=8, per_token=True), 1) == (1, 0, 8)
    with pytest.raises(h.HipLibraryError):
        h._mod_args(SimpleNamespace(mod_rows=3, first_rows=0, ld=8, per_token=False), 9)


@pytest.mark.parametrize("C", W8)
def test_emulated_ln_chain_meets_the_criterion(C):
    c = ln_case(C)
    print(f"LayerNorm family C={C}: rows {c.rows}, inputs of salt {c.salt}")
    _ln_check(c)


@pytest.mark.parametrize("hd,heads", ROPE_CASES)
def test_emulated_rope_chain_meets_the_criterion(hd, heads):
    c = rope_case(hd, heads)
    print(f"rmsnorm+rope {hd} x {heads}: rows {c.rows}, inputs of salt {c.salt}")
    _rope_check(c)


@pytest.mark.parametrize("C", W_VAE)
def test_emulated_vae_chain_meets_the_criterion(C):
    for c in (vae_case(C), vae_case(C, 1)):
        print(f"vae rmsnorm C={C}: pixels {c.pixels}, inputs of salt {c.salt}")
        _vae_check(c)


def test_emulated_table_layouts_meet_the_criterion():
    salts = []
    for key in table_cases():
        c = table_case(*key)
        salts.append(c.salt)
        _table_check(c)
    print("table layouts: salts", salts)


# ------------------------------------------------------------------------------------------------------------------ 1. widths (GPU)
def _same_fp8(hip, pair, bf16_rows, what):
    q, sc = hip.fp8_quant_rows(bf16_rows)
    assert torch.equal(pair[0].view(torch.uint8).cpu(), q.view(torch.uint8).cpu()), f"{what}: e4m3 bytes"
    assert torch.equal(pair[1].cpu(), sc.cpu()), f"{what}: scales"
    assert pair[1].max().item() > 1.0, f"{what}: the planted 900 must give a scale above 1"


@gpu
@pytest.mark.parametrize("C", W8)
def test_layernorm_family_widths(hip, C):
    c = ln_case(C)
    x, y, w, b = dev(c.x), dev(c.y), dev(c.w), dev(c.b)
    mod, mod2 = hip.ModTable(dev(c.table), c.first), hip.ModTable(dev(c.table2), c.first)
    assert_close_bf16(hip.ln_modulate(x, mod, 0, 1, EPS), c.want_mod, 1.0, "ln_modulate", mag=c.shift)
    assert_close_bf16(hip.ln_affine(x, w, b, EPS), c.want_aff, 1.0, "ln_affine", mag=c.b)
    assert torch.equal(hip.gate_residual(x, y, mod, 5).cpu(), c.x_gated)
    assert torch.equal(hip.gate_residual(x, y).cpu(), c.x_plain)
    xo, no = hip.residual_ln_modulate(x, y, mod, 5, 0, 1, EPS, norm_mod=mod2)
    assert torch.equal(xo.cpu(), c.x_gated)
    assert_close_bf16(no, c.want_res_mod, 1.0, "res+modulate", mag=c.shift2)
    xo, no = hip.residual_ln_modulate(x, y, mod, None, 3, 4, EPS)
    assert torch.equal(xo.cpu(), c.x_plain)
    assert_close_bf16(no, c.want_res_plain, 1.0, "res+modulate (no gate)", mag=c.shift3)
    xo, no = hip.residual_ln_affine(x, y, w, b, EPS, mod, 2)
    assert torch.equal(xo.cpu(), c.x_gated2)
    assert_close_bf16(no, c.want_res_aff, 1.0, "res+affine", mag=c.b)
    assert_close_bf16(hip.rmsnorm_rope(x, w, 1, EPS), c.want_rms, 1.0, "rmsnorm (no table)")


@gpu
@pytest.mark.parametrize("C", W8)
def test_fp8_and_dual_norm_widths(hip, C):
    c = ln_case(C)
    x, y, w, b = dev(c.x), dev(c.y), dev(c.w), dev(c.b_planted)
    mod = hip.ModTable(dev(c.planted), c.first)
    plain = hip.ln_modulate(x, mod, 0, 1, EPS)
    _same_fp8(hip, hip.ln_modulate_fp8(x, mod, 0, 1, EPS), plain, "ln_modulate_fp8")
    out, pair = hip.ln_modulate_dual(x, mod, 0, 1, EPS)
    assert torch.equal(out, plain)
    _same_fp8(hip, pair, plain, "ln_modulate_dual")
    plain = hip.ln_affine(x, w, b, EPS)
    out, pair = hip.ln_affine_dual(x, w, b, EPS)
    assert torch.equal(out, plain)
    _same_fp8(hip, pair, plain, "ln_affine_dual")
    for gate_idx, si, ci, what in ((5, 0, 1, "gated"), (None, 3, 4, "no gate")):
        xo, no = hip.residual_ln_modulate(x, y, mod, gate_idx, si, ci, EPS)
        xo8, pair = hip.residual_ln_modulate_fp8(x, y, mod, gate_idx, si, ci, EPS)
        assert torch.equal(xo8, xo)
        _same_fp8(hip, pair, no, f"residual_ln_modulate_fp8 ({what})")
    xo, no = hip.residual_ln_affine(x, y, w, b, EPS, mod, 2)
    xo8, pair = hip.residual_ln_affine_fp8(x, y, w, b, EPS, mod, 2)
    assert torch.equal(xo8, xo)
    _same_fp8(hip, pair, no, "residual_ln_affine_fp8")


@gpu
@pytest.mark.parametrize("act", [None, "gelu_tanh"])
@pytest.mark.parametrize("C", W_FP8)
def test_fp8_quant_rows_widths(hip, C, act):
    rows = rows_for(C)
    wide = seeded((1, rows, C + 64), 13000 + C, scale=2.0)
    wide[0, 1] *= 400.0                                   # a row above the fp8 range: scale > 1
    wide[0, 3] *= 1e-3                                    # a tiny row: the subnormal roundings
    x = wide[..., 32:32 + C]
    x2 = (F.gelu(x, approximate="tanh") if act else x).reshape(-1, C)
    want_scale = torch.clamp(x2.abs().amax(-1, keepdim=True) / 448.0, min=1.0).float()
    want = (x2 / (want_scale + 1e-8)).to(torch.float8_e4m3fn)
    got, scale = hip.fp8_quant_rows(dev(wide)[..., 32:32 + C], act)
    assert got.dtype == torch.float8_e4m3fn and got.shape == (rows, C) and scale.shape == (rows, 1)
    assert torch.equal(scale.cpu(), want_scale)
    assert want_scale[1].item() > 1.0 and want_scale[0].item() == 1.0
    same = got.cpu().view(torch.uint8) == want.view(torch.uint8)
    if act is None:
        assert same.all(), f"{(~same).sum().item()} fp8 bytes differ"
    else:
        assert same.float().mean().item() > 0.95
        assert (got.cpu().float() - want.float()).abs().max().item() <= 0.07 * want.float().abs().max().item()


@gpu
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("C", W_VAE)
def test_vae_rmsnorm_silu_widths(hip, C, silu):
    c = vae_case(C)
    got = hip.vae_rmsnorm_silu(dev(_cl(c.x)), dev(c.g.view(-1)), silu)
    assert_close_bf16(_ncthw(got.cpu()), c.want_silu if silu else c.want, 1.0, f"vae rmsnorm C={C} pixels={c.pixels}")


@gpu
@pytest.mark.parametrize("C", [248, 256, 264, 2048])
def test_vae_rmsnorm_silu_single_pixel(hip, C):
    """One pixel: on the 32-lane form 7 of the 8 pixel slots of the workgroup are dead; the output sits in a sentinel-filled buffer of
    three pixels whose other two must stay untouched."""
    c = vae_case(C, 1)
    for silu, want in ((True, c.want_silu), (False, c.want)):
        buf = torch.full((3, C), 7.0, dtype=BF16, device="cuda")
        hip.vae_rmsnorm_silu(dev(_cl(c.x)), dev(c.g.view(-1)), silu, out=buf[1:2].view(1, 1, 1, C))
        assert (buf[0] == 7.0).all() and (buf[2] == 7.0).all(), "pixels next to the only live one were written"
        assert_close_bf16(_ncthw(buf[1:2].view(1, 1, 1, C).cpu()), want, 1.0, f"vae rmsnorm single pixel C={C}")


@gpu
def test_row_kernels_refuse_bad_widths(hip):
    """limit + 8 and C % 8 != 0 are refused by every entry point, and an output handed in stays as it was."""
    E = hip.HipLibraryError

    def refused(call, *outs):
        with pytest.raises(E):
            call()
        torch.cuda.synchronize()
        for o in outs:
            assert (o == 7.0).all(), "a refused call wrote to its output"

    for C in (LIMIT8 + 8, 12):
        x, y = dev(seeded((1, 5, C), 1)), dev(seeded((1, 5, C), 2))
        w, b = dev(seeded((C,), 3)), dev(seeded((C,), 4))
        mod = hip.ModTable(dev(seeded((2, 6, C), 5)), 2)
        o1, o2 = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
        refused(lambda: hip.ln_modulate(x, mod, 0, 1, EPS, out=o1), o1)
        refused(lambda: hip.ln_affine(x, w, b, EPS, out=o1), o1)
        refused(lambda: hip.gate_residual(x, y, mod, 2, out=o1), o1)
        refused(lambda: hip.gate_residual(x, y, out=o1), o1)
        refused(lambda: hip.residual_ln_modulate(x, y, mod, 5, 0, 1, EPS, x_out=o1, norm_out=o2, norm_mod=mod), o1, o2)
        refused(lambda: hip.residual_ln_modulate(x, y, mod, None, 0, 1, EPS, x_out=o1, norm_out=o2), o1, o2)
        refused(lambda: hip.residual_ln_affine(x, y, w, b, EPS, mod, 2, x_out=o1, norm_out=o2), o1, o2)
        refused(lambda: hip.ln_modulate_fp8(x, mod, 0, 1, EPS))
        refused(lambda: hip.ln_modulate_dual(x, mod, 0, 1, EPS, out=o1), o1)
        refused(lambda: hip.ln_affine_dual(x, w, b, EPS, out=o1), o1)
        refused(lambda: hip.residual_ln_modulate_fp8(x, y, mod, 5, 0, 1, EPS, x_out=o1), o1)
        refused(lambda: hip.residual_ln_affine_fp8(x, y, w, b, EPS, mod, 2, x_out=o1), o1)
        refused(lambda: hip.rmsnorm_rope(x, w, 1, EPS, out=o1), o1)
    for C in (LIMIT_FP8 + 8, 12):
        x = dev(seeded((1, 5, C), 6))
        refused(lambda: hip.fp8_quant_rows(x))
        refused(lambda: hip.fp8_quant_rows(x, "gelu_tanh"))
    for C in (LIMIT_VAE + 8, 12):
        x, g = dev(seeded((1, 1, 5, C), 7)), dev(seeded((C,), 8))
        o1 = torch.full_like(x, 7.0)
        refused(lambda: hip.vae_rmsnorm_silu(x, g, True, out=o1), o1)
        refused(lambda: hip.vae_rmsnorm_silu(x, g, False, out=o1), o1)


# ----------------------------------------------------------------------------------------------- 2. head sizes of RMSNorm+RoPE (GPU)
@gpu
@pytest.mark.parametrize("hd,heads", ROPE_CASES)
def test_rmsnorm_rope_head_sizes(hip, hd, heads):
    c = rope_case(hd, heads)
    C = c.C
    wide = dev(c.wide)
    assert wide[..., C:2 * C].stride(-2) == 3 * C
    plain64, hoist64 = rope_form(hd, False)
    plain32, hoist32 = rope_form(hd, True)
    assert plain64 == plain32 == (hd in (8, 16, 64, 128, 256, 512, 1024)) and not hoist64
    assert hoist32 == (hd in (8, 16, 64, 128, 256, 512)) and (plain32 or not hoist32)
    got = hip.rmsnorm_rope(wide[..., C:2 * C], dev(c.wt), heads, EPS, dev(c.cos), dev(c.sin))
    got32 = hip.rmsnorm_rope(wide[..., C:2 * C], dev(c.wt), heads, EPS, dev(c.cs))
    same = (got32 == got).float().mean().item()
    print(f"rmsnorm+rope head_dim {hd} x {heads}: plain={plain32} hoist(fp32)={hoist32}; fp32-table == fp64-table on {same:.5f} of the elements")
    assert_close_bf16(got, c.want, 1.0, f"rmsnorm+rope head_dim {hd} x {heads} (fp64 tables)")
    assert_close_bf16(got32, c.want, 1.0, f"rmsnorm+rope head_dim {hd} x {heads} (fp32 table)")


@gpu
@pytest.mark.parametrize("hd", GROUPED_HD)
def test_rmsnorm_rope_grouped_head_sizes(hip, hd):
    heads = 4
    c = rope_case(hd, heads)
    C, rows = c.C, c.rows
    x, wt = dev(c.wide)[..., C:2 * C], dev(c.wt)
    size = rows + 2                                        # a token shard shorter than its chunk: two rows past it
    for tables in ((dev(c.cos), dev(c.sin)), (dev(c.cs),)):
        plain = hip.rmsnorm_rope(x, wt, heads, EPS, *tables)[0]
        for group_cols in (hd, 2 * hd, C):
            G, out_ld = C // group_cols, group_cols + 16
            dst = torch.full((G, size, out_ld), 7.0, dtype=BF16, device="cuda")
            hip.rmsnorm_rope(x, wt, heads, EPS, *tables, grouped=(dst.view(-1), group_cols, size * out_ld, out_ld))
            what = f"head_dim {hd}, group_cols {group_cols}, {'fp32 table' if len(tables) == 1 else 'fp64 tables'}"
            assert torch.equal(dst[:, :rows, :group_cols], plain.unflatten(-1, (G, group_cols)).transpose(0, 1)), what
            assert (dst[:, rows:] == 7.0).all(), f"{what}: rows past the shard were written"
            assert (dst[:, :, group_cols:] == 7.0).all(), f"{what}: the padding between group_cols and out_ld was written"


# -------------------------------------------------------------------------------------------------------- 3. table layouts (GPU)
@gpu
@pytest.mark.parametrize("rows,mod_rows,first", table_cases())
def test_table_layouts(hip, rows, mod_rows, first):
    c = table_case(rows, mod_rows, first)
    x, y = dev(c.x), dev(c.y)
    mod, mod2 = hip.ModTable(dev(c.table), first), hip.ModTable(dev(c.table2), first)
    what = f"rows={rows} mod_rows={mod_rows} first_rows={first}"
    plain = hip.ln_modulate(x, mod, 0, 1, EPS)
    assert_close_bf16(plain, c.want_mod, 1.0, f"ln_modulate {what}", mag=c.shift)
    assert torch.equal(hip.gate_residual(x, y, mod, 5).cpu(), c.x_gated), what
    xo, no = hip.residual_ln_modulate(x, y, mod, 5, 0, 1, EPS, norm_mod=mod2)
    assert torch.equal(xo.cpu(), c.x_gated), what
    assert_close_bf16(no, c.want_res_mod, 1.0, f"res+modulate {what}", mag=c.shift2)
    q, sc = hip.fp8_quant_rows(plain)
    for pair in (hip.ln_modulate_fp8(x, mod, 0, 1, EPS), hip.ln_modulate_dual(x, mod, 0, 1, EPS)[1]):
        assert torch.equal(pair[0].view(torch.uint8), q.view(torch.uint8)) and torch.equal(pair[1], sc), what
    assert torch.equal(hip.ln_modulate_dual(x, mod, 0, 1, EPS)[0], plain), what


@gpu
def test_two_rows_two_row_table(hip):
    """rows == mod_rows == 2.  Default: the TI2V split, so first_rows = 0 sends BOTH rows to table row 1 (a token shard behind the first
    latent frame).  ModTable(per_token=True): row r reads table row r (= the split at first_rows 1); a per-token table must have
    the call's row count."""
    c = table_case(2, 2, 0)
    x, y, table = dev(c.x), dev(c.y), dev(c.table)
    assert torch.equal(c.idx, torch.tensor([1, 1]))
    assert torch.equal(hip.gate_residual(x, y, hip.ModTable(table), 5).cpu(), c.x + c.table[1, 5] * c.y)
    per = c.x + c.table[:, 5].unsqueeze(0) * c.y
    assert not torch.equal(per, c.x_gated)
    assert torch.equal(hip.gate_residual(x, y, hip.ModTable(table, per_token=True), 5).cpu(), per)
    assert torch.equal(hip.gate_residual(x, y, hip.ModTable(table, 1), 5).cpu(), per)
    got = hip.ln_modulate(x, hip.ModTable(table, per_token=True), 0, 1, EPS)
    shift, scale = c.table[:, 0].unsqueeze(0), c.table[:, 1].unsqueeze(0)
    assert_close_bf16(got, wan_dit.layer_norm(c.x, EPS) * (1 + scale) + shift, 1.0, "ln_modulate, per-token table of two rows", mag=shift)
    c9 = table_case(9, 2, 0)
    with pytest.raises(hip.HipLibraryError):
        hip.ln_modulate(dev(c9.x), hip.ModTable(dev(c9.table), per_token=True), 0, 1, EPS)
    c9 = table_case(9, 9, 0)              # first_rows is not used with nine rows, per token or not
    for mod in (hip.ModTable(dev(c9.table), per_token=True), hip.ModTable(dev(c9.table), 4)):
        assert torch.equal(hip.gate_residual(dev(c9.x), dev(c9.y), mod, 5).cpu(), c9.x_gated)


@gpu
def test_gemm_gate_table_layouts(hip):
    """The GEMM epilogue's gate (mode 2) reads the same table convention: M = 9 output rows, one or two table rows, first_rows at
    0, 1, M - 1 and M; the expectation indexes the table on the host and uses the kernel's own y."""
    M, K, N = 9, 128, 256
    x, w, b = dev(seeded((1, M, K), 14001)), dev(seeded((N, K), 14002, scale=0.05)), dev(seeded((N,), 14003, scale=0.2))
    res = seeded((1, M, N), 14004)
    y = hip.gemm_epilogue(x, w, b).cpu()
    for mod_rows in (1, 2):
        table = seeded((mod_rows, 6, N), 14005 + mod_rows) + (torch.arange(mod_rows, dtype=torch.float32).view(-1, 1, 1) + 1).to(BF16)
        for first in (0, 1, M - 1, M):
            got = hip.gemm_epilogue(x, w, b, out=dev(res).clone(), residual=True, mod=hip.ModTable(dev(table), first), gate_idx=5)
            idx = mod_index(M, mod_rows, first)
            assert torch.equal(got.cpu(), res + table[idx, 5].unsqueeze(0) * y), f"mod_rows={mod_rows} first_rows={first}"
    with pytest.raises(hip.HipLibraryError):
        hip.gemm_epilogue(x, w, b, out=dev(res).clone(), residual=True, mod=hip.ModTable(dev(table), per_token=True), gate_idx=5)

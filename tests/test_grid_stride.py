"""The grid-stride kernels beyond the cap of their launch grids.

Thirteen entry points launch at most `cap` workgroups of 256 threads and cover the rest of the tensor with a grid-stride loop
(`for (i = tid; i < total; i += gridDim.x * blockDim.x)`).  A call "wraps" when its loop total exceeds cap x 256 loop indices, i.e.
cap x 256 x (elements per thread) elements: some threads then run the loop body a second time ("second pass"), with an index one whole grid
further on, and the last pass ends somewhere inside a workgroup.  The unit tests of these kernels (test_hip_kernels.py, test_graph_step.py)
stay far below the caps, where the loop is an `if`; the product is always above them (a 5.2 M-element latent, 327 M video samples).

  entry point                                   source               cap     elements / thread   first size that wraps
  fg_act_bf16 (both kinds)                      dit_elementwise.hip   8 192  8                   n > 16 777 216
  fg_gated_gelu_bf16                            text_encoder.hip      8 192  8                   n > 16 777 216
  fg_cfg_euler_bf16                             dit_elementwise.hip   4 096  1                   n > 1 048 576
  fg_cfg_euler_dev_bf16, vector path            dit_elementwise.hip   4 096  8                   n > 8 388 608
  fg_cfg_euler_dev_bf16, element path           dit_elementwise.hip   4 096  1                   n > 1 048 576  (a pointer not 16-byte aligned)
  fg_copy_groups_bf16                           dit_elementwise.hip  16 384  8 (one vector)      groups * rows * cols / 8 > 4 194 304
  fg_vae_latent_to_cl_bf16, _latent_from_cl,    vae_ops.hip          16 384  1                   loop total > 4 194 304
  _unpatchify, _patchify, _tile_accumulate,     (grid_for's default)
  _tile_finalize, fg_avgdown3d_add_bf16,
  fg_video_to_uint8

CAPS below holds this table.  test_caps_are_what_the_table_says (no GPU) reads the three sources and fails when a launcher no longer
carries its cap, its 256 threads, its kernel or its loop total; every GPU test asserts from CAPS (past_cap) that its shape needs a second
pass of at least one whole workgroup and that the last pass ends inside a workgroup (inside a wave for the shapes of the vector kernels).
A changed cap therefore fails here instead of turning the GPU tests into single-pass tests.

Each GPU test takes the oracle function, the criterion and the input distribution of the kernel's small test: nothing here has a
tolerance of its own.  The comparisons run in the order of the kernel's loop index, so a failure names the flat index of the first differing
element and its pass (index // (cap * 256 * elements per thread)): "pass 1" reads as "second pass wrong".

Left to other modules on purpose: widths at lane-group boundaries, ragged row counts and guard bands (test_buffer_contract.py), offsets above
2^31 (test_full_size_properties.py), and fg_conv_pack_weight_bf16, whose fixed 2048-block grid already wraps in
test_hip_kernels.py::test_conv3d_cl[1024-1024-...] and is checked through the convolution's result.
"""
import collections
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from oracle import pipeline as opipe
from oracle import wan_text, wan_vae
from test_hip_kernels import _cl, assert_close_bf16, dev

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
THREADS = 256
SENTINEL = 768.0      # exact in bf16, far outside what seeded() or a clamp to [-1, 1] produces

# kernels: what the launcher hands to hipLaunchKernelGGL; count: the loop total the grid is sized from, as the source writes it
Cap = collections.namedtuple("Cap", "entry source cap per_thread kernels count")
CAPS = {c.entry + ("/" + path if path else ""): c for path, c in [
    ("", Cap("fg_act_bf16", "dit_elementwise.hip", 8192, 8, ("act_kernel<0>", "act_kernel<1>"), "const int64_t nvec = n / 8;")),
    ("", Cap("fg_gated_gelu_bf16", "text_encoder.hip", 8192, 8, ("gated_gelu_kernel",), "const int64_t nvec = n / 8;")),
    ("", Cap("fg_cfg_euler_bf16", "dit_elementwise.hip", 4096, 1, ("cfg_euler_kernel",), "n")),
    ("vector", Cap("fg_cfg_euler_dev_bf16", "dit_elementwise.hip", 4096, 8, ("cfg_euler_dev_kernel",),
                   "const int64_t nvec = vec ? n / 8 : 0;\n    const int64_t work = nvec > n - nvec * 8 ? nvec : n - nvec * 8;")),
    ("element", Cap("fg_cfg_euler_dev_bf16", "dit_elementwise.hip", 4096, 1, ("cfg_euler_dev_kernel",),
                    "const int64_t nvec = vec ? n / 8 : 0;\n    const int64_t work = nvec > n - nvec * 8 ? nvec : n - nvec * 8;")),
    ("", Cap("fg_copy_groups_bf16", "dit_elementwise.hip", 16384, 8, ("copy_groups_kernel",),
             "const int64_t total = (int64_t)groups * rows * (cols / 8);")),
    ("", Cap("fg_vae_latent_to_cl_bf16", "vae_ops.hip", 16384, 1, ("latent_to_cl_kernel",), "thw * C")),
    ("", Cap("fg_vae_latent_from_cl_bf16", "vae_ops.hip", 16384, 1, ("latent_from_cl_kernel",), "thw * Z")),
    ("", Cap("fg_vae_unpatchify_bf16", "vae_ops.hip", 16384, 1, ("unpatchify_kernel",), "total")),
    ("", Cap("fg_vae_patchify_bf16", "vae_ops.hip", 16384, 1, ("patchify_kernel",), "(int64_t)T * H * W * 4")),
    ("", Cap("fg_vae_tile_accumulate_bf16", "vae_ops.hip", 16384, 1, ("tile_accumulate_kernel",), "(int64_t)F * th * tw")),
    ("", Cap("fg_vae_tile_finalize_bf16", "vae_ops.hip", 16384, 1, ("tile_finalize_kernel",), "C * fhw")),
    ("", Cap("fg_avgdown3d_add_bf16", "vae_ops.hip", 16384, 1, ("avgdown3d_add_kernel",), "total")),
    ("", Cap("fg_video_to_uint8", "vae_ops.hip", 16384, 1, ("video_to_uint8_kernel",), "3 * fhw")),
]}


def span(key):
    """Elements one pass of the whole grid covers."""
    return CAPS[key].cap * THREADS * CAPS[key].per_thread


def past_cap(key, total):
    """`total` elements need a second pass of >= one whole workgroup, and the last pass ends inside a workgroup.  Returns span(key)."""
    c = CAPS[key]
    extra = total // c.per_thread - c.cap * THREADS           # loop indices behind the first pass
    assert extra >= THREADS, f"{key}: {total} elements do not wrap a grid of {c.cap} x {THREADS} threads x {c.per_thread} by a whole workgroup"
    assert extra % THREADS, f"{key}: the last pass of {total} elements ends on a workgroup boundary"
    return span(key)


# ------------------------------------------------------------------------------------------------ 1. the caps (no GPU)
_INLINE_CAP = re.compile(r"const unsigned grid = \(unsigned\)\(\((\w+) \+ 255\) / 256 < (\d+) \? \(\1 \+ 255\) / 256 : (\d+)\);")
_INLINE_LAUNCH = re.compile(r"hipLaunchKernelGGL\((\w+(?:<\d>)?), dim3\(grid\), dim3\((\d+)\),")
_GRID_FOR = re.compile(r"inline unsigned grid_for\(int64_t n, int per_block = (\d+), int cap = (\d+)\) \{\s*"
                       r"const int64_t g = \(n \+ per_block - 1\) / per_block;\s*"
                       r"return \(unsigned\)\(g < cap \? \(g > 0 \? g : 1\) : cap\);\s*\}")
_GRID_FOR_LAUNCH = re.compile(r"hipLaunchKernelGGL\((\w+), dim3\(grid_for\(([^,;]+?)\)\), dim3\((\d+)\),")


def test_caps_are_what_the_table_says():
    """Every launcher of CAPS still sizes its grid as the table says: min(ceil(count / 256), cap) workgroups of 256 threads on the kernel(s)
    named, `count` being the loop total the source derives (n / 8 where a thread owns one 16-byte vector)."""
    assert len({c.entry for c in CAPS.values()}) == 13 and len(CAPS) == 14
    src = {name: open(os.path.join(REPO, "fairygen_amd", "csrc", name)).read() for name in {c.source for c in CAPS.values()}}
    m = _GRID_FOR.search(src["vae_ops.hip"])
    assert m, "vae_ops.hip: grid_for is not the function this module knows"
    grid_for_default = (int(m.group(1)), int(m.group(2)))
    for key, c in CAPS.items():
        body = re.search(rf"^int {c.entry}\(.*?^}}", src[c.source], re.M | re.S)
        assert body, f"{c.source}: no definition of {c.entry}"
        body = body.group(0)
        if c.source == "vae_ops.hip":
            launches = _GRID_FOR_LAUNCH.findall(body)      # one argument: the defaults of grid_for hold
            assert launches == [(c.kernels[0], c.count, str(THREADS))], f"{key}: {launches}"
            assert grid_for_default == (THREADS, c.cap), f"{key}: grid_for defaults to {grid_for_default}"
            assert c.count != "total" or re.search(r"const int64_t total = [^;]+;", body), key
        else:
            m = _INLINE_CAP.search(body)
            assert m and len(_INLINE_CAP.findall(body)) == 1, f"{key}: grid expression not found"
            assert int(m.group(2)) == int(m.group(3)) == c.cap, f"{key}: cap {m.group(2)} / {m.group(3)} in the source, {c.cap} in the table"
            launches = _INLINE_LAUNCH.findall(body)
            assert launches == [(k, str(THREADS)) for k in c.kernels], f"{key}: {launches}"
            if c.count == "n":
                assert m.group(1) == "n", key
            else:      # the counted variable is the last one c.count defines
                assert c.count in body and re.findall(r"const int64_t (\w+) =", c.count)[-1] == m.group(1), key
    # the vector path of fg_cfg_euler_dev_bf16 is taken when every pointer is 16-byte aligned, else nvec = 0: one element per thread
    assert "const bool vec = FG_ALIGNED16(latents) && FG_ALIGNED16(posi) && FG_ALIGNED16(out) && (nega == nullptr || FG_ALIGNED16(nega));" in \
        src["dit_elementwise.hip"]


def test_past_cap_rejects_single_pass_and_even_shapes():
    """past_cap is what keeps the GPU tests two-pass: it refuses a shape at the cap, one short of a whole workgroup, and an even last pass."""
    full = span("fg_cfg_euler_bf16")
    assert past_cap("fg_cfg_euler_bf16", full + THREADS + 1) == full == 4096 * 256
    for total in (full, full + THREADS - 1, full + 2 * THREADS):
        with pytest.raises(AssertionError):
            past_cap("fg_cfg_euler_bf16", total)
    assert past_cap("fg_act_bf16", span("fg_act_bf16") + 8 * (THREADS + 1)) == 8192 * 256 * 8
    with pytest.raises(AssertionError):
        past_cap("fg_act_bf16", span("fg_act_bf16") + 8 * THREADS)


# ------------------------------------------------------------------------------------------------ failure messages
def _where(diff, key, base=0, per_index=None):
    """'first at flat index i = pass p' for a boolean tensor laid out in the order of the kernel's loop index (per_index elements per
    index: default the table's elements per thread; base: the flat index of diff's first element in the whole tensor)."""
    c = CAPS[key]
    one_pass = c.cap * THREADS * (c.per_thread if per_index is None else per_index)
    at = diff.reshape(-1).nonzero().reshape(-1) + base
    per_pass = torch.bincount(at // one_pass).tolist()
    return (f"first at flat index {at[0].item()} = pass {at[0].item() // one_pass} of {c.entry} ({c.cap} workgroups x {THREADS} threads x "
            f"{one_pass // (c.cap * THREADS)}); differing elements per pass {per_pass}")


def assert_same(got, want, key, what, base=0, per_index=None):
    """torch.equal, both tensors in the order of the kernel's loop index."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.device != want.device:
        got, want = got.cpu(), want.cpu()
    if torch.equal(got, want):
        return
    diff = (got != want) | (got != got)
    raise AssertionError(f"{what}: {diff.sum().item()} of {diff.numel()} elements differ, {_where(diff, key, base, per_index)}")


def assert_close_by_pass(got, want, key, what, mag=None, max_mismatch=2e-3):
    """assert_close_bf16 (1 bf16 ulp, at most max_mismatch of the elements not identical) with the pass named on failure."""
    got, want = got.float().cpu(), want.float().cpu()
    diff = got != want
    print(f"{what}: {diff.float().mean().item():.3e} of {diff.numel()} elements differ from the oracle (allowed {max_mismatch:.0e}), "
          f"max abs {(got - want).abs().max().item():.3e}")
    try:
        assert_close_bf16(got, want, 1.0, what, mag=mag, max_mismatch=max_mismatch)
    except AssertionError as e:
        # (for the message only) the elements beyond assert_close_bf16's 1 ulp, if that is what failed; else the ones not identical
        ref = want.abs() if mag is None else torch.maximum(want.abs(), mag.float().cpu().abs().expand_as(want))
        beyond = ~((got - want).abs() <= ref.clamp_min(1e-3) * 2.0 ** -7)
        where = f"beyond 1 ulp: {_where(beyond, key)}" if beyond.any() else f"not identical: {_where(diff, key)}"
        raise AssertionError(f"{str(e).splitlines()[0]}; {where}") from None


@pytest.fixture(scope="module")
def hip():
    _hip.load()
    assert torch.cuda.is_available()
    return _hip


def sentinel_like(t):
    return torch.full_like(t, SENTINEL)


# ------------------------------------------------------------------------------------------------ 2. DiT / text-encoder elementwise
N_ACT = 16777216 + 6440      # 805 vectors behind the first pass: three workgroups and 37 lanes


@pytest.fixture(scope="module")
def act_input():
    return seeded((N_ACT,), 14, scale=3.0)      # test_hip_kernels.py::test_activations_and_cfg_euler's distribution, shared by both kinds


@gpu
@pytest.mark.parametrize("kind", ["silu", "gelu_tanh"])
def test_act_two_passes(hip, act_input, kind):
    """fg_act_bf16 against F.silu / F.gelu(approximate="tanh"): <= 1 bf16 ulp, <= 5 % not identical (the criterion of
    test_activations_and_cfg_euler), out of place into a sentinel-filled tensor; the in-place call gives the same bits; the second-pass
    region equals a call on that region alone (one pass), bit for bit."""
    one_pass = past_cap("fg_act_bf16", N_ACT)
    x = act_input
    want = F.silu(x) if kind == "silu" else F.gelu(x, approximate="tanh")
    xd = dev(x)
    out = sentinel_like(xd)
    assert hip.activation(xd, kind, out=out) is out and torch.equal(xd.cpu(), x)
    assert_close_by_pass(out, want, "fg_act_bf16", f"{kind}, {N_ACT} elements", max_mismatch=0.05)
    assert_same(hip.activation(xd[one_pass:].clone(), kind), out[one_pass:], "fg_act_bf16", f"{kind}: second pass vs a call on its region", base=one_pass)
    inplace = xd.clone()
    assert hip.activation(inplace, kind) is inplace
    assert_same(inplace, out, "fg_act_bf16", f"{kind} in place vs out of place")
    del xd, out, inplace


@gpu
def test_gated_gelu_two_passes(hip):
    """fg_gated_gelu_bf16 against fc1 * gelu_tanh_explicit(gate) on the whole tensor (criterion of test_text_encoder_kernels), and the
    second-pass region against a call on that region alone."""
    key = "fg_gated_gelu_bf16"
    one_pass = past_cap(key, N_ACT)
    fc1, gate = seeded((N_ACT,), 122), seeded((N_ACT,), 123, scale=2.0)
    want = fc1 * wan_text.gelu_tanh_explicit(gate)
    d1, dg = dev(fc1), dev(gate)
    got = hip.gated_gelu(d1, dg)
    assert_close_by_pass(got, want, key, f"gated gelu, {N_ACT} elements", max_mismatch=0.02)
    assert_same(hip.gated_gelu(d1[one_pass:].clone(), dg[one_pass:].clone()), got[one_pass:], key, "gated gelu: second pass vs a call on its region",
                base=one_pass)
    del d1, dg, got


EULER_SHAPE = (1, 48, 7, 56, 57)             # 1 072 512 elements: 93 workgroups and 128 threads behind the first pass
EULER_DEV_SHAPE = (1, 49, 7, 161, 157)       # 8 670 011 = 1 083 751 vectors + 3; frame_stride 176 939 and first_n 25 277 are odd: vectors
#                                              straddle channel blocks and the edge of frame 0 all through the second pass
EULER_STEP = 2


@pytest.fixture(scope="module")
def euler_operands():
    """shape -> (lat, posi, nega, first) on the CPU, generated once per shape and never written."""
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = tuple(seeded(shape, 15 + i) for i in range(3)) + (seeded(shape[:2] + (1,) + shape[3:], 18),)
        return cache[shape]
    yield get
    cache.clear()


def _euler_case(operands, with_nega, with_first):
    """(lat, posi, nega, first, cfg, want) on the CPU: opipe.euler_step on the CFG combine, then the re-pin of frame 0."""
    lat, posi, nega, first = operands
    first = first if with_first else None
    sig, _ = opipe.wan_sigmas(4)
    want = opipe.euler_step(nega + 5.0 * (posi - nega) if with_nega else posi, EULER_STEP, lat, sig)
    if with_first:
        want[:, :, 0:1] = first
    return lat, posi, nega if with_nega else None, first, 5.0 if with_nega else 1.0, want


def _dsigma():
    sig, _ = opipe.wan_sigmas(4)
    return [float((0 if i == 3 else sig[i + 1]) - sig[i]) for i in range(4)]


@gpu
@pytest.mark.parametrize("with_nega", [False, True], ids=["nonega", "nega"])
def test_cfg_euler_two_passes(hip, euler_operands, with_nega):
    key = "fg_cfg_euler_bf16"
    lat, posi, nega, _, cfg, want = _euler_case(euler_operands(EULER_SHAPE), with_nega, False)
    past_cap(key, lat.numel())
    dl, dp, dn = dev(lat), dev(posi), None if nega is None else dev(nega)
    out = sentinel_like(dl)
    assert hip.cfg_euler(dl, dp, dn, cfg, _dsigma()[EULER_STEP], out=out) is out
    assert_same(out.cpu(), want, key, "cfg+euler")
    assert hip.cfg_euler(dl, dp, dn, cfg, _dsigma()[EULER_STEP], out=dl) is dl
    assert_same(dl.cpu(), want, key, "cfg+euler, out = latents")
    del dl, dp, dn, out


def _check_euler_dev(got, want, key, what):
    frame_stride = want.shape[2] * want.shape[3] * want.shape[4]
    last = want.shape[1] - 1      # the last channel block alone: a wrong ch * first_n at large i is named
    assert_same(got[0, last].cpu(), want[0, last], key, f"{what}, channel {last}", base=last * frame_stride)
    assert_same(got.cpu(), want, key, what)


@gpu
@pytest.mark.parametrize("with_first", [False, True], ids=["nofirst", "first"])
@pytest.mark.parametrize("with_nega", [False, True], ids=["nonega", "nega"])
def test_cfg_euler_dev_vector_path_two_passes(hip, euler_operands, with_nega, with_first):
    key = "fg_cfg_euler_dev_bf16/vector"
    lat, posi, nega, first, cfg, want = _euler_case(euler_operands(EULER_DEV_SHAPE), with_nega, with_first)
    n = lat.numel()
    past_cap(key, n)
    assert n == 8670011 and n % 8 == 3 and want.shape[1] == 49
    dl, dp = dev(lat), dev(posi)
    dn, df = None if nega is None else dev(nega), None if first is None else dev(first)
    assert all(t is None or t.data_ptr() % 16 == 0 for t in (dl, dp, dn))
    table = torch.tensor(_dsigma(), dtype=torch.float32, device="cuda")
    step = torch.tensor([EULER_STEP], dtype=torch.int32, device="cuda")
    out = sentinel_like(dl)
    assert hip.cfg_euler_dev(dl, dp, dn, cfg, table, step, first=df, out=out) is out
    _check_euler_dev(out, want, key, "cfg_euler_dev")
    assert hip.cfg_euler_dev(dl, dp, dn, cfg, table, step, first=df, out=dl) is dl
    _check_euler_dev(dl, want, key, "cfg_euler_dev, out = latents")
    del dl, dp, dn, df, out


@gpu
def test_cfg_euler_dev_element_path_two_passes(hip, euler_operands):
    """Operands 2 bytes past a 16-byte boundary (as test_graph_step.py::test_cfg_euler_dev_equals_scalar_form builds them): no vectors,
    one element per thread."""
    key = "fg_cfg_euler_dev_bf16/element"
    lat, posi, nega, first, cfg, want = _euler_case(euler_operands(EULER_SHAPE), True, True)
    past_cap(key, lat.numel())
    flat = [torch.full((lat.numel() + 1,), SENTINEL, dtype=BF16, device="cuda")[1:] for _ in range(4)]
    for f, t in zip(flat, (lat, posi, nega)):
        f.copy_(t.reshape(-1))
    off = [f.view(lat.shape) for f in flat]
    assert all(t.data_ptr() % 16 == 2 for t in off)
    table = torch.tensor(_dsigma(), dtype=torch.float32, device="cuda")
    step = torch.tensor([EULER_STEP], dtype=torch.int32, device="cuda")
    df = dev(first)
    assert hip.cfg_euler_dev(off[0], off[1], off[2], cfg, table, step, first=df, out=off[3]) is off[3]
    _check_euler_dev(off[3], want, key, "cfg_euler_dev, element path")
    assert hip.cfg_euler_dev(off[0], off[1], off[2], cfg, table, step, first=df, out=off[0]) is off[0]
    _check_euler_dev(off[0], want, key, "cfg_euler_dev, element path, out = latents")
    del flat, off, df


@gpu
def test_copy_groups_two_passes(hip):
    """3 groups x 5 500 rows x 257 vectors, both sides strided (rows wider than cols, group strides larger than rows * ld), into a
    sentinel-filled destination: the block equals torch's strided copy on the device and nothing outside it is written."""
    key = "fg_copy_groups_bf16"
    groups, rows, cols = 3, 5500, 2056
    past_cap(key, groups * rows * cols)
    sld, dld = cols + 8, cols + 24
    sgs, dgs = rows * sld + 64, rows * dld + 128
    s0, d0 = 8, 16                                         # the views start 16 / 32 bytes into their buffers
    src = dev(seeded((s0 + (groups - 1) * sgs + (rows - 1) * sld + cols + 8,), 33))
    dst = torch.full((d0 + (groups - 1) * dgs + (rows - 1) * dld + cols + 16,), SENTINEL, dtype=BF16, device="cuda")
    want = dst.clone()
    want[d0:].as_strided((groups, rows, cols), (dgs, dld, 1)).copy_(src[s0:].as_strided((groups, rows, cols), (sgs, sld, 1)))
    hip.copy_groups(src[s0:], sgs, sld, dst[d0:], dgs, dld, groups, rows, cols)
    loop_order = ((rows, groups, cols), (dld, dgs, 1))     # the kernel's index runs over (row, group, vector)
    assert_same(dst[d0:].as_strided(*loop_order), want[d0:].as_strided(*loop_order), key, "copied block")
    assert torch.equal(dst, want), "elements outside the copied block were written"
    outside = torch.ones_like(want, dtype=torch.bool)
    outside[d0:].as_strided((groups, rows, cols), (dgs, dld, 1)).fill_(False)
    assert outside.sum().item() == want.numel() - groups * rows * cols and (dst[outside] == SENTINEL).all()
    del src, dst, want, outside


# ------------------------------------------------------------------------------------------------ 3. VAE kernels (grid_for)
def _vae_stats():
    return torch.tensor(wan_vae.VAE38_MEAN).to(BF16), (1.0 / torch.tensor(wan_vae.VAE38_STD)).to(BF16)


@gpu
def test_latent_to_cl_two_passes(hip):
    key = "fg_vae_latent_to_cl_bf16"
    z = seeded((1, 48, 3, 172, 170), 91)
    past_cap(key, z.numel())
    mean, inv_std = _vae_stats()
    want = z / inv_std.view(1, 48, 1, 1, 1) + mean.view(1, 48, 1, 1, 1)      # test_softmax_latent_unpatchify_uint8's expression
    got = hip.vae_latent_to_cl(dev(z[0].contiguous()), dev(mean), dev(inv_std))
    assert_same(got.cpu(), _cl(want), key, "latent_to_cl")
    del got


@gpu
def test_latent_from_cl_two_passes(hip):
    key = "fg_vae_latent_from_cl_bf16"
    h96 = seeded((1, 96, 3, 172, 170), 116)
    past_cap(key, h96.numel() // 2)
    mean, inv_std = _vae_stats()
    want = (h96[:, :48] - mean.view(1, 48, 1, 1, 1)) * inv_std.view(1, 48, 1, 1, 1)      # test_encoder_kernels' expression
    got = hip.vae_latent_from_cl(dev(_cl(h96)), dev(mean), dev(inv_std), 48)
    assert_same(got.cpu().unsqueeze(0), want, key, "latent_from_cl")
    del got


@gpu
def test_unpatchify_two_passes(hip):
    key = "fg_vae_unpatchify_bf16"
    x = seeded((1, 12, 2, 420, 420), 92, scale=0.8)
    video = torch.full((3, 3, 840, 840), SENTINEL, dtype=BF16, device="cuda")
    past_cap(key, 3 * 2 * 840 * 840)
    hip.vae_unpatchify(dev(_cl(x)), video, 1, True)
    assert_same(video[:, 1:3].cpu().contiguous(), wan_vae.unpatchify2(x)[0].clamp(-1, 1), key, "unpatchify into frames [1, 3)")
    assert (video[:, 0] == SENTINEL).all(), "frame 0 was written"
    del video


@gpu
def test_patchify_two_passes(hip):
    key = "fg_vae_patchify_bf16"
    vid = seeded((1, 3, 2, 730, 722), 113, scale=0.5)
    past_cap(key, 2 * 365 * 361 * 16)
    p = hip.vae_patchify(dev(vid[0].contiguous())).cpu()
    assert p.shape == (2, 365, 361, 16)
    want = torch.cat([_cl(wan_vae.patchify2(vid)), torch.zeros((2, 365, 361, 4), dtype=BF16)], dim=-1)
    assert_same(p, want, key, "patchify (12 patch channels + 4 zero channels)")
    assert not p[..., 12:].any()


@gpu
def test_tile_blend_two_passes(hip):
    """The four tiles wan_vae.tile_tasks gives for a 930 x 930 canvas with tiles of (920, 916) at stride (10, 14) — two of them at (0, 0)
    and (10, 14) — with its masks, borders and bound bits: values and weight after every accumulate, then finalize with clamp, as in
    test_tile_blend."""
    C, F_, H, W = 3, 5, 930, 930
    tile_size, tile_stride = (920, 916), (10, 14)
    tasks = wan_vae.tile_tasks(H, W, tile_size, tile_stride)
    assert tasks == [(0, 920, 0, 916), (0, 920, 14, 930), (10, 930, 0, 916), (10, 930, 14, 930)]
    acc, fin = "fg_vae_tile_accumulate_bf16", "fg_vae_tile_finalize_bf16"
    past_cap(acc, F_ * 920 * 916)
    past_cap(fin, C * F_ * H * W)
    border = (tile_size[0] - tile_stride[0], tile_size[1] - tile_stride[1])
    values, weight = torch.zeros((C, F_, H, W), dtype=BF16), torch.zeros((F_, H, W), dtype=BF16)
    dv, dw = dev(values), dev(weight)
    for i, (h, h_, w, w_) in enumerate(tasks):
        th, tw = h_ - h, w_ - w
        tile = seeded((C, F_, th, tw), 100 + i)
        bounds = (h == 0, h_ >= H, w == 0, w_ >= W)
        m = wan_vae.tile_mask(th, tw, bounds, border).to(BF16)[0, 0]
        values[:, :, h:h_, w:w_] += tile * m
        weight[:, h:h_, w:w_] += m[0]
        hip.vae_tile_accumulate(dev(tile), dv, dw, h, w, border[0], border[1], bounds)
        gv, gw = dv.cpu(), dw.cpu()
        # the kernel's index runs over the tile's (frame, row, column); it writes the C channels of that pixel
        assert_same(gv[:, :, h:h_, w:w_].permute(1, 2, 3, 0), values[:, :, h:h_, w:w_].permute(1, 2, 3, 0), acc, f"values under tile {i}", per_index=C)
        assert_same(gw[:, h:h_, w:w_], weight[:, h:h_, w:w_], acc, f"weight under tile {i}")
        assert torch.equal(gv, values) and torch.equal(gw, weight), f"tile {i}: the canvas outside the tile changed"
    assert (weight > 0).all()
    hip.vae_tile_finalize(dv, dw)
    assert_same(dv.cpu(), (values / weight).clamp_(-1, 1), fin, "finalize")
    del dv, dw


@gpu
def test_avgdown3d_add_two_passes(hip):
    """T = 3 is odd: the zero frame in front of the first pair is in play.  Criterion of test_encoder_kernels."""
    key = "fg_avgdown3d_add_bf16"
    xs = seeded((1, 32, 3, 366, 362), 114)
    sc = wan_vae.avg_down3d(xs, 64, 2, 2)
    assert sc.shape == (1, 64, 2, 183, 181)
    past_cap(key, sc.numel())
    main = seeded(tuple(sc.shape), 115)
    got = hip.avgdown3d_add(dev(_cl(xs)), dev(_cl(main)), 2, 2)
    assert_close_by_pass(got, _cl(main + sc), key, "avgdown 32->64 ft2 fs2", mag=_cl(main), max_mismatch=0.02)
    del got


@gpu
def test_video_to_uint8_two_passes(hip):
    key = "fg_video_to_uint8"
    vid = seeded((3, 2, 840, 836), 93, scale=0.7).clamp(-1.2, 1.2)
    past_cap(key, vid.numel())
    got = hip.video_to_uint8(dev(vid))
    assert_same(got.cpu(), opipe.video_to_uint8(vid), key, "video_to_uint8")
    del got

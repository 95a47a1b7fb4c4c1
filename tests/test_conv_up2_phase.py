"""The nearest-2x upsample + 3x3 conv of the VAE decoder as four 2x2 phase convs (include/fairygen_hip_up2phase.h:
fg_conv_up2phase_pack_bf16, fg_conv3d_up2_phase_bf16; hip.conv_up2_phase_pack_weight, conv3d_up2_phase, conv3d_up2).

Output pixel (2y + a, 2x + b) of the 9-tap conv over the upsampled image reads only the low-resolution pixels (y + i - 1 + a,
x + j - 1 + b), i, j in {0, 1}, so its taps can be summed first: W_ab[i][j] = sum of W[dy][dx] over dy in R_a(i), dx in R_b(j) with
R_0 = ({0}, {1, 2}), R_1 = ({0, 1}, {2}).  Checked here:

  the packer          the 16 summed matrices against that formula in torch (fp32 sum, one round-to-nearest-even), bit for bit
  exactness           small-integer weights and inputs (every summed weight a bf16 number, every fp32 sum exact): torch.equal to the
                      existing resample == 1 kernel
  error               N(0,1) data against an fp64 reference (upsample, then the conv with the ORIGINAL bf16 weights):
                      e4 <= 2 e9 + 1e-2 rms(out), e9 / e4 the largest error of the 9-tap kernel / of the phase form
  launch invariance   a call on T frames equals T calls on one frame, bit for bit
  guard bands         input and output inside larger poisoned allocations: nothing outside the output is written, NaN outside the
                      input does not reach the result
  capture             the call is captured into a graph and replayed (it only enqueues on the caller's stream)
  arguments           odd H / W, kt = 3, ks = 1, Cin = 48 refused on the host; hip.conv3d_up2 takes the old path where there is no
                      phase form, and the decoder takes the phase form where there is one

Shapes: the smallest at which the form can go wrong — a 3 x 5 image (every pixel on or next to a border, all four phases at all
four edges), 9 x 17 (612 output pixels: ragged tiles, phases across tile edges), a cout tail (96), two cout tiles (320), T = 3, two
k-steps per tap (Cin = 128); and two shapes of 64 workgroups, the fewest that run the hand-scheduled 256-tile kernel (one with a
ragged last pixel tile, one with two cout tiles, two k-steps per tap and frames that cross tiles).

What the emulation of both forms on the CPU (bf16 operands, fp32 accumulation, one bf16 rounding) gives on the four small shapes, in
the order of SMALL: e4 / e9 = 1.21, 1.32, 1.07, 1.37 (test_emulated_error_bound); the kernels measure the same four figures, and 1.53 /
1.21 on the two 256-tile shapes — the bound allows 2 + 1e-2 rms / e9 = 2.7 to 2.9.
"""
import ctypes
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, seeded
from fairygen_amd import hip as _hip

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
NAMES = ("fg_conv_up2phase_pack_bf16", "fg_conv3d_up2_phase_bf16")
QUERIES = ("fg_conv_up2phase_version", "fg_conv_up2phase_packed_bytes")
RANGES = {0: ((0, 1), (1, 3)), 1: ((0, 2), (2, 3))}      # R_a(i) as [lo, hi)

# (cin, cout, T, low-resolution H, W)
SMALL = {"3x5": (64, 64, 1, 3, 5), "9x17": (64, 64, 1, 9, 17), "cin128-cout96-t3": (128, 96, 3, 9, 17), "cout320": (64, 320, 1, 9, 17)}
W4 = {"w4-ragged": (64, 256, 1, 63, 65), "w4-cout512-t2": (128, 512, 2, 33, 31)}      # 64 workgroups of the 256-tile kernel each
CASES = {**SMALL, **W4}


def phase_weights(w):
    """(Cout, Cin, 3, 3) bf16 -> (4, 4, Cout, Cin) bf16, [2a + b][2i + j]: the formula of the header, fp32 sums rounded once."""
    wf = w.float()
    out = torch.zeros((4, 4) + tuple(w.shape[:2]), dtype=torch.float32, device=w.device)
    for a in (0, 1):
        for b in (0, 1):
            for i in (0, 1):
                for j in (0, 1):
                    (y0, y1), (x0, x1) = RANGES[a][i], RANGES[b][j]
                    s = torch.zeros(w.shape[:2], dtype=torch.float32, device=w.device)
                    for dy in range(y0, y1):
                        for dx in range(x0, x1):
                            s = s + wf[:, :, dy, dx]
                    out[2 * a + b, 2 * i + j] = s
    return out.to(BF16)


def reference_fp64(x_cl, w, bias):
    """x (T, h, w, Cin) channels-last, w (Cout, Cin, 3, 3), bias (Cout,) -> fp64 (T, 2h, 2w, Cout): nearest 2x, then the 3x3 conv with
    the original weights (unfold + matmul, all in fp64)."""
    up = x_cl.double().permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    t, c, hh, ww = up.shape
    cols = F.unfold(up, 3, padding=1)                                    # (T, Cin * 9, H * W)
    out = torch.matmul(w.double().reshape(w.shape[0], -1), cols) + bias.double()[None, :, None]
    return out.reshape(t, -1, hh, ww).permute(0, 2, 3, 1).contiguous()


def make(case, integers, device):
    cin, cout, t, h, w = CASES[case]
    if integers:      # |w| <= 2, |x| <= 3, |bias| <= 4: summed weights <= 8, |out| <= 9 * 128 * 6 + 4 < 2^24
        g = torch.Generator("cpu").manual_seed(11)
        x = torch.randint(-3, 4, (t, h, w, cin), generator=g).to(BF16)
        wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).to(BF16)
        bias = torch.randint(-4, 5, (cout,), generator=g).to(BF16)
    else:
        x, wt, bias = seeded((t, h, w, cin), 1), seeded((cout, cin, 3, 3), 2), seeded((cout,), 3)
    return x.to(device), wt.to(device), bias.to(device)


@functools.lru_cache(maxsize=None)
def computed(case, integers):
    """(x, w, bias, 9-tap output, phase output, packed phase weights) of a case on the GPU, computed once and left unchanged."""
    x, wt, bias = make(case, integers, "cuda:0")
    cout = wt.shape[0]
    out9 = _hip.conv3d_cl(x, _hip.conv_pack_weight(wt), bias, cout, 1, 3, upsample2x=True)
    wph = _hip.conv_up2_phase_pack_weight(wt)
    out4 = _hip.conv3d_up2_phase(x, wph, bias, cout)
    torch.cuda.synchronize()
    return x, wt, bias, out9, out4, wph


# ------------------------------------------------------------------------------------------------------------------ CPU: ABI, arguments, emulation
def test_extension_abi():
    lib = _hip.load()
    inc = os.path.join(REPO, "include")
    ext = open(os.path.join(inc, "fairygen_hip_up2phase.h")).read()
    assert _hip.ABI_VERSION == 8 and lib.fg_version() == 8 and len(_hip.EXPORTED_SYMBOLS) == 55      # the main table is what it was
    for header in sorted(os.listdir(inc)):
        if header != "fairygen_hip_up2phase.h":
            text = open(os.path.join(inc, header)).read()
            assert not any(re.search(r"\b%s\b" % name, text) for name in NAMES + QUERIES), header
    assert '#include "fairygen_hip.h"' in ext and "version of this extension, currently 1" in ext
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", ext, re.M)
    assert sorted(declared) == _hip.UP2PHASE_SYMBOLS == sorted(NAMES + QUERIES) and len(declared) == 4
    assert _hip.UP2PHASE_ABI_VERSION == 1 and lib.fg_conv_up2phase_version() == 1
    kinds = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "fg_stream_t": ctypes.c_void_p, "int": ctypes.c_int}
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, ext, re.M | re.S).group(1)
        want = [kinds[" ".join(a.split()[:-1])] for a in decl.split(",")]
        assert want == _hip._UP2PHASE_SIGNATURES[name] == list(getattr(lib, name).argtypes), name
    real = _hip._lib
    try:
        _hip._lib = None
        _hip.UP2PHASE_ABI_VERSION = 2
        with pytest.raises(_hip.HipLibraryError, match="ABI mismatch"):
            _hip.load()
    finally:
        _hip.UP2PHASE_ABI_VERSION = 1
        _hip._lib = real


def test_argument_checks():
    """Refused on the host before anything is launched (-1 and the FG_CHECK_ARG message); the pointers are not device memory, so every
    call below carries one bad argument and none is valid."""
    lib = _hip.load()
    p16 = ctypes.c_void_p(4096)
    err = lambda: lib.fg_last_error()      # noqa: E731

    def conv(x=p16, w=p16, b=p16, out=p16, t=1, h=6, wd=10, cin=64, cout=64, kt=1, ks=3):
        return lib.fg_conv3d_up2_phase_bf16(x, w, b, out, t, h, wd, cin, cout, kt, ks, None)
    assert conv(h=7) == -1 and b"fg_conv3d_up2_phase_bf16: need even H and W" in err()
    assert conv(wd=11) == -1 and b"need even H and W" in err()
    assert conv(kt=3) == -1 and b"the phase form is that of the 1x3x3 conv" in err()
    assert conv(ks=1) == -1 and b"the phase form is that of the 1x3x3 conv" in err()
    assert conv(cin=48) == -1 and b"need Cin % 64 == 0" in err()
    assert conv(cin=96) == -1 and b"need Cin % 64 == 0" in err()
    assert conv(cout=66) == -1 and b"Cout % 4 == 0" in err()
    assert conv(t=0) == -1 and b"sizes must be positive" in err()
    for key in ("x", "w", "b", "out"):
        assert conv(**{key: None}) == -1 and b"null pointer" in err(), key
    assert conv(x=ctypes.c_void_p(4104)) == -1 and b"misaligned" in err()
    assert conv(out=ctypes.c_void_p(4100)) == -1 and b"misaligned" in err()
    assert conv(t=64, h=2048, wd=2048, cin=64, cout=64) == -1 and b"3.5 GiB" in err()
    assert lib.fg_conv_up2phase_pack_bf16(p16, p16, 64, 48, None) == -1 and b"need Cin % 64 == 0" in err()
    assert lib.fg_conv_up2phase_pack_bf16(None, p16, 64, 64, None) == -1 and b"bad arguments" in err()
    assert lib.fg_conv_up2phase_packed_bytes(64, 48) == 0 and lib.fg_conv_up2phase_packed_bytes(0, 64) == 0
    assert lib.fg_conv_up2phase_packed_bytes(96, 128) == 16 * 128 * 128 * 2 and lib.fg_conv_up2phase_packed_bytes(320, 64) == 16 * 384 * 64 * 2
    assert _hip.conv_up2_phase_ok(64, 1, 3) and not _hip.conv_up2_phase_ok(48, 1, 3) and not _hip.conv_up2_phase_ok(64, 3, 3) \
        and not _hip.conv_up2_phase_ok(64, 1, 1)


@pytest.mark.parametrize("case", sorted(SMALL))
def test_emulated_error_bound(case):
    """Both forms emulated in torch on the CPU — bf16 operands, fp32 accumulation, one bf16 rounding — against the fp64 reference: the
    bound of test_error_against_fp64 holds with room before any kernel runs (and the identity itself is checked: the phase form is
    computed from phase_weights on the low-resolution image)."""
    x, wt, bias = make(case, False, "cpu")
    ref = reference_fp64(x, wt, bias)
    xc = x.float().permute(0, 3, 1, 2)
    up = xc.repeat_interleave(2, 2).repeat_interleave(2, 3)
    out9 = F.conv2d(up, wt.float(), bias.float(), padding=1).to(BF16)
    pw = phase_weights(wt).float()
    out4 = torch.empty_like(out9)
    for a in (0, 1):
        for b in (0, 1):
            k = pw[2 * a + b].reshape(2, 2, *wt.shape[:2]).permute(2, 3, 0, 1)
            out4[:, :, a::2, b::2] = F.conv2d(F.pad(xc, (1 - b, b, 1 - a, a)), k, bias.float()).to(BF16)
    e9 = (out9.double().permute(0, 2, 3, 1) - ref).abs().max().item()
    e4 = (out4.double().permute(0, 2, 3, 1) - ref).abs().max().item()
    rms = ref.pow(2).mean().sqrt().item()
    print(f"{case}: emulated e9 {e9:.4f} e4 {e4:.4f} e4/e9 {e4 / e9:.3f} rms {rms:.2f}")
    assert e4 <= 2 * e9 + 1e-2 * rms


# ------------------------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("case", ["3x5", "cin128-cout96-t3", "cout320"])
def test_packer_matches_formula(case):
    """All 16 matrices, bit for bit; the rows that pad Cout to 128 are zero."""
    _, wt, _, _, _, wph = computed(case, False)
    cout, cin = wt.shape[:2]
    cout_pad = (cout + 127) // 128 * 128
    got = wph.view(4, 4, cout_pad, cin)
    assert torch.equal(got[:, :, :cout], phase_weights(wt))
    assert not got[:, :, cout:].any()


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_on_small_integers(case):
    x, wt, bias, out9, out4, _ = computed(case, True)
    assert out4.shape == out9.shape == (x.shape[0], 2 * x.shape[1], 2 * x.shape[2], wt.shape[0])
    assert torch.equal(out9.float(), reference_fp64(x, wt, bias).to(BF16).float())      # the data is exact for the 9-tap kernel
    assert torch.equal(out4, out9)


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_error_against_fp64(case):
    x, wt, bias, out9, out4, _ = computed(case, False)
    ref = reference_fp64(x, wt, bias)
    e9, e4 = (out9.double() - ref).abs().max().item(), (out4.double() - ref).abs().max().item()
    rms = ref.pow(2).mean().sqrt().item()
    print(f"{case}: e9 {e9:.4f} e4 {e4:.4f} e4/e9 {e4 / e9:.3f} rms {rms:.2f}")
    assert e4 <= 2 * e9 + 1e-2 * rms


@gpu
@pytest.mark.parametrize("case,frames", [("cin128-cout96-t3", 3), ("w4-ragged", 2)])
def test_launch_invariance(case, frames):
    """T frames in one call = T calls on one frame (for w4-ragged both sizes run the 256-tile kernel)."""
    cin, cout, _, h, w = CASES[case]
    x = seeded((frames, h, w, cin), 5).to("cuda:0")
    _, _, bias, _, _, wph = computed(case, False)
    full = _hip.conv3d_up2_phase(x, wph, bias, cout)
    for f in range(frames):
        assert torch.equal(_hip.conv3d_up2_phase(x[f:f + 1].contiguous(), wph, bias, cout), full[f:f + 1]), f


@gpu
@pytest.mark.parametrize("case", ["3x5", "cout320", "w4-ragged"])
def test_guard_bands(case):
    """x, the packed weights, the bias and out each sit inside a larger allocation: NaN around the three inputs, a sentinel around out."""
    x, _, bias, _, out4, wph = computed(case, False)
    guard = 4096      # elements; keeps the 16-byte alignment

    def embed(t, fill):
        big = torch.full((t.numel() + 2 * guard,), fill, dtype=BF16, device=t.device)
        big[guard:guard + t.numel()] = t.reshape(-1)
        return big, big[guard:guard + t.numel()].view(t.shape)
    _, xe = embed(x, float("nan"))
    _, we = embed(wph, float("nan"))
    _, be = embed(bias, float("nan"))
    big_out, oe = embed(torch.zeros_like(out4), 7.0)
    got = _hip.conv3d_up2_phase(xe, we, be, out4.shape[-1], out=oe)
    torch.cuda.synchronize()
    assert got.data_ptr() == oe.data_ptr() and torch.equal(oe, out4)
    assert bool((big_out[:guard] == 7.0).all()) and bool((big_out[guard + out4.numel():] == 7.0).all())


@gpu
@pytest.mark.parametrize("case", ["9x17", "w4-ragged"])
def test_captured_and_replayed(case):
    """The entry point only enqueues on the caller's stream: it is captured into a graph (a synchronisation or an allocation of its
    own would end the capture with an error) and the replay writes the eager call's bytes."""
    x, _, bias, _, out4, wph = computed(case, False)
    out = torch.zeros_like(out4)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.conv3d_up2_phase(x, wph, bias, out4.shape[-1], out=out)
    assert not out.any()      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, out4)


@gpu
def test_host_wrapper_takes_the_old_path_without_a_phase_form():
    """Cin = 48: hip.conv3d_up2 calls the 9-tap upsample conv, bit for bit, whatever is passed as phase weights.  kt = 3: there is no
    upsample conv of that size in either form — the old path's own refusal comes back.  (An odd output size cannot reach the wrapper:
    it doubles the input's.)"""
    x, wt, bias = seeded((1, 5, 7, 48), 1).to("cuda:0"), seeded((64, 48, 3, 3), 2).to("cuda:0"), seeded((64,), 3).to("cuda:0")
    packed = _hip.conv_pack_weight(wt)
    want = _hip.conv3d_cl(x, packed, bias, 64, 1, 3, upsample2x=True)
    assert torch.equal(_hip.conv3d_up2(x, packed, None, bias, 64, 1, 3), want)
    assert torch.equal(_hip.conv3d_up2(x, packed, packed, bias, 64, 1, 3), want)
    with pytest.raises(_hip.HipLibraryError, match="no phase form"):
        _hip.conv_up2_phase_pack_weight(wt)
    x3, w3 = seeded((3, 5, 7, 64), 4).to("cuda:0"), seeded((64, 64, 3, 3, 3), 5).to("cuda:0")
    with pytest.raises(_hip.HipLibraryError, match="upsample2x needs even H, W and kt==1"):
        _hip.conv3d_up2(x3, _hip.conv_pack_weight(w3), None, bias, 64, 3, 3)
    # and with a phase form the wrapper is the phase call
    x, _, bias, _, out4, wph = computed("9x17", False)
    assert torch.equal(_hip.conv3d_up2(x, None, wph, bias, 64, 1, 3), out4)


@gpu
def test_decoder_takes_the_phase_form(monkeypatch):
    """A tiny decoder (upsample convs of 128, 128 and 64 input channels): every upsample conv runs in the phase form, on weights packed
    once, and none as the 9-tap upsample conv."""
    from fairygen_amd import synthetic
    from fairygen_amd.wan_video_vae import WanVideoVAE38
    vae = WanVideoVAE38(dim=32, dec_dim=32)
    vae.load_state_dict(synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=32, dim=32), seed=1234))
    vae = vae.to(device="cuda:0", dtype=BF16).eval()
    calls = {"phase": 0, "up9": 0, "pack": 0}
    real_phase, real_cl, real_pack = _hip.conv3d_up2_phase, _hip.conv3d_cl, _hip.conv_up2_phase_pack_weight

    def phase(*a, **kw):
        calls["phase"] += 1
        return real_phase(*a, **kw)

    def cl(*a, **kw):
        calls["up9"] += bool(kw.get("upsample2x"))
        return real_cl(*a, **kw)

    def pack(*a, **kw):
        calls["pack"] += 1
        return real_pack(*a, **kw)
    monkeypatch.setattr(_hip, "conv3d_up2_phase", phase)
    monkeypatch.setattr(_hip, "conv3d_cl", cl)
    monkeypatch.setattr(_hip, "conv_up2_phase_pack_weight", pack)
    z = seeded((1, 48, 3, 4, 4), 4).to("cuda:0")
    with torch.no_grad():
        vae.model.decode(z, vae.scale)
        first = dict(calls)
        vae.model.decode(z, vae.scale)
    assert first["phase"] > 0 and first["up9"] == 0 and first["pack"] == 3
    assert calls["pack"] == 3 and calls["phase"] == 2 * first["phase"]

"""BASELINE.json full sizes (704x1280x121: N = 27 280 tokens, 24 heads; VAE layers at 480x832 tiles) on the GPU, checked
through size-independent properties and through the CPU oracle on SAMPLED outputs (the oracle cannot finish the full
tensors in seconds, but any output row / pixel depends on the full key set / receptive field only)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N, H, D = 27280, 24, 128


def _rand(shape, seed, scale=1.0):
    g = torch.Generator("cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)


@pytest.fixture(scope="module")
def hip():
    from fairygen_amd import hip as h
    h.load()
    return h


def test_attention_full_size_sampled_rows_and_properties(hip):
    q, k, v = _rand((1, N, H * D), 1), _rand((1, N, H * D), 2), _rand((1, N, H * D), 3)
    out = hip.attention(q, k, v, H)
    # (1) sampled query rows (first / last / block edges / ragged tail) against an fp32 softmax over ALL 27 280 keys
    rows = torch.tensor([0, 1, 255, 256, 257, 13639, 27135, 27136, 27263, 27279], device="cuda")
    qs = q[0, rows].view(-1, H, D).transpose(0, 1).float()                   # (H, R, D)
    kf = k[0].view(N, H, D).transpose(0, 1).float()
    vf = v[0].view(N, H, D).transpose(0, 1).float()
    ref = torch.softmax(qs @ kf.transpose(1, 2) * D ** -0.5, dim=-1) @ vf      # (H, R, D)
    got = out[0, rows].view(-1, H, D).transpose(0, 1).float()
    assert (got - ref).abs().max().item() < 6e-3, (got - ref).abs().max().item()
    # (2) rows of softmax sum to one: constant V comes back unchanged (up to bf16 rounding of P)
    vc = torch.full_like(v, 0.75)
    oc = hip.attention(q, k, vc, H).float()
    assert (oc - 0.75).abs().max().item() < 4e-3
    # (3) permuting the keys (with their values) does not change the result beyond summation order
    perm = torch.randperm(N, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    op = hip.attention(q, k[:, perm].contiguous(), v[:, perm].contiguous(), H).float()
    assert (op - out.float()).abs().max().item() < 4e-3
    # (4) a token shard (1/8 of the queries, the split-every-q-block decomposition) equals the same rows of the full call
    lo, hi = 3 * 3410, 4 * 3410
    os_ = hip.attention(q[:, lo:hi].contiguous(), k, v, H).float()
    assert (os_ - out[:, lo:hi].float()).abs().max().item() < 4e-3


def test_attention_head_shard_equals_full_call(hip):
    """The Ulysses head shard at P = 8 (3 of 24 heads over ALL 27 280 tokens, q | k | v as column slices of one
    (N, 1152) buffer, i.e. what the all-to-all delivers) gives the same numbers as those heads' columns of the full call."""
    q, k, v = _rand((1, N, H * D), 11), _rand((1, N, H * D), 12), _rand((1, N, H * D), 13)
    full = hip.attention(q, k, v, H)
    g = 3 * D
    for rank in (0, 5):
        cols = slice(rank * g, (rank + 1) * g)
        buf = torch.cat([q[..., cols], k[..., cols], v[..., cols]], dim=-1).contiguous()      # (1, N, 1152)
        part = hip.attention(buf[..., :g], buf[..., g:2 * g], buf[..., 2 * g:], 3)
        assert (part.float() - full[..., cols].float()).abs().max().item() < 4e-3


def test_fp8_quant_full_size_round_trip(hip):
    """fg_fp8_quant_rows_bf16 on the full ffn.2 input (27 280 x 14 336): scale >= 1, |q| <= 448, and q * scale recovers x to
    e4m3 precision (relative 2^-4 per element above the subnormal range)."""
    x = _rand((1, N, 14336), 14, scale=3.0)
    x[0, 7] *= 200.0
    q8, scale = hip.fp8_quant_rows(x)
    assert q8.shape == (N, 14336) and scale.shape == (N, 1) and scale.min().item() == 1.0 and scale[7].item() > 1.0
    deq = q8.float() * (scale + 1e-8)
    xf = x[0].float()
    assert q8.float().abs().max().item() <= 448.0
    err = (deq - xf).abs()
    assert bool((err <= 2.0 ** -4 * xf.abs() + 2.0 ** -9 * scale).all())


@pytest.mark.parametrize("cin,cout,T,Hh,Ww", [(256, 256, 4, 240, 416), (1024, 1024, 2, 60, 104)])
def test_conv_full_size_sampled_pixels(hip, cin, cout, T, Hh, Ww):
    """A last-stage and a second-stage decoder layer of a 480x832 tile (256x256 LDS-DMA tile variant), checked on sampled
    output pixels against F.conv3d over their receptive fields, plus linearity in the input."""
    x = _rand((T + 2, Hh, Ww, cin), 5)
    w = _rand((cout, cin, 3, 3, 3), 6, scale=(cin * 27) ** -0.5)
    b = _rand((cout,), 7, scale=0.1)
    wp = hip.conv_pack_weight(w)
    y = hip.conv3d_cl(x, wp, b, cout, 3, 3)
    assert y.shape == (T, Hh, Ww, cout)
    xp = F.pad(x.float().permute(3, 0, 1, 2).unsqueeze(0), (1, 1, 1, 1, 0, 0))        # (1,C,T+2,H+2,W+2), zero spatial pad
    for (t, yy, xx) in [(0, 0, 0), (T - 1, Hh - 1, Ww - 1), (1, 17, 255 % Ww), (T - 1, Hh // 2, 0), (0, Hh - 1, Ww // 3)]:
        patch = xp[:, :, t:t + 3, yy:yy + 3, xx:xx + 3]
        ref = F.conv3d(patch, w.float(), b.float())[0, :, 0, 0, 0]
        assert (y[t, yy, xx].float() - ref).abs().max().item() < 3e-2
    y2 = hip.conv3d_cl((x.float() * 0.5).to(torch.bfloat16), wp, torch.zeros_like(b), cout, 3, 3).float()
    y1 = hip.conv3d_cl(x, wp, torch.zeros_like(b), cout, 3, 3).float()
    assert (y2 - 0.5 * y1).abs().max().item() < 3e-2


# ---------------------------------------------------------------------------------- VAE kernels on tensors above 2 GiB
# The (30, 52) latent tile of the bench decoded in groups of 8 latent frames: 32 frames at 240x416 on the last two stages.  One
# 512-channel frame there is 102 236 160 bytes, so byte offsets pass 2^31 in frame 21; the checks sample frame 0, the last frames and
# the spatial borders.
T8, H8, W8 = 32, 240, 416
TOP = (0, 21, T8 - 1)               # first frame, the frame where offsets pass 2^31, last frame


def _rand_frames(shape, seed, scale=1.0):
    """_rand without the fp32 copy of the whole tensor: filled one frame at a time."""
    g = torch.Generator("cuda").manual_seed(seed)
    x = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    for t in range(shape[0]):
        x[t] = (torch.randn(shape[1:], generator=g, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)
    return x


def _window(x, t, y, xx, kt, ks, up=False):
    """fp32 (1, C, kt, ks, ks) receptive field of output pixel (t, y, xx) in the channels-last input x: frames t .. t+kt-1, zeros outside
    the image, read through the nearest-2x upsample when `up`."""
    hin, win, c = x.shape[1:]
    h, w, p = hin << up, win << up, ks // 2
    out = torch.zeros((kt, ks, ks, c), device=x.device)
    for dy in range(ks):
        for dx in range(ks):
            yy, xc = y + dy - p, xx + dx - p
            if 0 <= yy < h and 0 <= xc < w:
                out[:, dy, dx] = x[t:t + kt, yy >> up, xc >> up].float()
    return out.permute(3, 0, 1, 2).unsqueeze(0)


PIXELS = [(t, y, xx) for t in TOP for (y, xx) in ((0, 0), (H8 - 1, W8 - 1), (0, W8 - 1), (H8 - 1, 0), (H8 // 2, W8 // 2 + 1))] + \
         [(T8 - 2, 1, 207), (22, 239, 3)]


def test_vae_conv_input_above_2gib(hip):
    """The first 240x416 conv of a group-8 chunk: a (34, 240, 416, 512) ring (3.48 GB, under the kernel's 0xF0000000-byte limit of
    32-bit offsets) -> 256 couts, 3x3x3, on the hand-scheduled 256x256 kernel; sampled pixels against F.conv3d in fp32."""
    cin, cout = 512, 256
    lib = hip.load()
    assert lib.fg_conv_tile_choice(T8, H8, W8, cout) == 256 and cin % 64 == 0 and cout % 256 == 0      # conv3d_cl_w4_kernel
    x = _rand_frames((T8 + 2, H8, W8, cin), 21)
    assert x.numel() * 2 > 3.4e9
    w = _rand((cout, cin, 3, 3, 3), 22, scale=(cin * 27) ** -0.5)
    b = _rand((cout,), 23, scale=0.1)
    y = hip.conv3d_cl(x, hip.conv_pack_weight(w), b, cout, 3, 3)
    assert y.shape == (T8, H8, W8, cout)
    for (t, yy, xx) in PIXELS:
        ref = F.conv3d(_window(x, t, yy, xx, 3, 3), w.float(), b.float())[0, :, 0, 0, 0]
        assert (y[t, yy, xx].float() - ref).abs().max().item() < 3e-2, (t, yy, xx)
    del x, y
    torch.cuda.empty_cache()


def test_vae_conv_output_above_2gib(hip):
    """The 3x3 Conv2d of Resample38 after the nearest-2x upsample, 512 channels, 120x208 -> 240x416 with a residual: the output
    (32, 240, 416, 512) is 3.27 GB.  Sampled pixels: bf16(conv + bias) + residual against fp32 on the upsampled window."""
    c = 512
    lib = hip.load()
    assert lib.fg_conv_tile_choice(T8, H8, W8, c) == 256
    x = _rand_frames((T8, H8 // 2, W8 // 2, c), 24)
    res = _rand_frames((T8, H8, W8, c), 25)
    w = _rand((c, c, 3, 3), 26, scale=(c * 9) ** -0.5)
    b = _rand((c,), 27, scale=0.1)
    y = hip.conv3d_cl(x, hip.conv_pack_weight(w), b, c, 1, 3, upsample2x=True, residual=res)
    assert y.shape == (T8, H8, W8, c) and y.numel() * 2 > 3.2e9
    for (t, yy, xx) in PIXELS:
        conv = F.conv3d(_window(x, t, yy, xx, 1, 3, up=True), w.float().unsqueeze(2), b.float())[0, :, 0, 0, 0]
        ref = conv.to(torch.bfloat16).float() + res[t, yy, xx].float()
        assert (y[t, yy, xx].float() - ref).abs().max().item() < 3e-2, (t, yy, xx)
    del x, res, y
    torch.cuda.empty_cache()


def test_vae_rmsnorm_silu_above_2gib(hip):
    """RMS_norm * SiLU over the (32, 240, 416, 512) activation (3.27 GB): whole image rows at frame 0, across the 2^31-byte mark and at
    the last frame, against the oracle's rms_norm_c + SiLU to 1 bf16 ulp."""
    from oracle import wan_vae
    from test_hip_kernels import assert_close_bf16
    c = 512
    x = _rand_frames((T8, H8, W8, c), 28, scale=2.0)
    g = (1 + 0.1 * _rand((c,), 29).float()).to(torch.bfloat16)
    y = hip.vae_rmsnorm_silu(x, g, True)
    for (t, yy) in ((0, 0), (0, H8 - 1), (21, 1), (T8 - 1, 0), (T8 - 1, H8 - 1)):
        xs = x[t, yy].cpu().t().reshape(1, c, W8, 1, 1)          # (1, C, pixels, 1, 1)
        want = F.silu(wan_vae.rms_norm_c({"n.gamma": g.cpu().view(c, 1, 1, 1)}, "n", xs))
        assert_close_bf16(y[t, yy].cpu(), want.reshape(c, W8).t(), 1.0, f"rmsnorm_silu frame {t} row {yy}")
    del x, y
    torch.cuda.empty_cache()


def test_vae_dupup3d_above_2gib(hip):
    """The 1024 -> 512 DupUp3D shortcut of the third up block (ft = 1, fs = 2) from (32, 120, 208, 1024) onto a (32, 240, 416, 512) main
    path (3.27 GB): aligned crops of x and main through the oracle's dup_up3d + add equal the kernel's output crops bit for bit."""
    from oracle import wan_vae
    cin, cout, hc, wc = 1024, 512, 3, 4
    x = _rand_frames((T8, H8 // 2, W8 // 2, cin), 30)
    main = _rand_frames((T8, H8, W8, cout), 31)
    out = hip.dupup3d_add(x, main, cout, 1, 2, False)
    assert out.shape == main.shape
    for t in TOP + (T8 - 2,):
        for (y0, x0) in ((0, 0), (H8 // 2 - hc, W8 // 2 - wc), (0, W8 // 2 - wc), (H8 // 2 - hc, 0), (57, 101)):
            xs = x[t:t + 1, y0:y0 + hc, x0:x0 + wc].cpu().permute(3, 0, 1, 2).unsqueeze(0)      # (1, Cin, 1, hc, wc)
            ms = main[t:t + 1, 2 * y0:2 * (y0 + hc), 2 * x0:2 * (x0 + wc)].cpu().permute(3, 0, 1, 2).unsqueeze(0)
            want = ms + wan_vae.dup_up3d(xs, cout, 1, 2, False)
            got = out[t:t + 1, 2 * y0:2 * (y0 + hc), 2 * x0:2 * (x0 + wc)].cpu().permute(3, 0, 1, 2).unsqueeze(0)
            assert torch.equal(got, want), (t, y0, x0)
    del x, main, out
    torch.cuda.empty_cache()


def test_token_kernels_full_size_statistics(hip):
    """LN+modulate / RMSNorm+RoPE on the full (27 280, 3072) token tensor: row statistics and norm preservation."""
    from fairygen_amd.wan_video_dit import precompute_freqs_cis_3d
    x = _rand((1, N, 3072), 8, scale=2.0)
    mod = hip.ModTable(torch.zeros((2, 6, 3072), dtype=torch.bfloat16, device="cuda"), 880)
    y = hip.ln_modulate(x, mod, 0, 1, 1e-6).float()                                   # zero shift/scale: plain LayerNorm
    assert y.mean(-1).abs().max().item() < 2e-2 and (y.var(-1, unbiased=False) - 1).abs().max().item() < 2e-2
    f, h, w = 31, 22, 40
    fr = precompute_freqs_cis_3d(128)
    tab = torch.cat([fr[0][:f].view(f, 1, 1, -1).expand(f, h, w, -1), fr[1][:h].view(1, h, 1, -1).expand(f, h, w, -1),
                     fr[2][:w].view(1, 1, w, -1).expand(f, h, w, -1)], dim=-1).reshape(N, -1)
    ones = torch.ones(3072, dtype=torch.bfloat16, device="cuda")
    r0 = hip.rmsnorm_rope(x, ones, 24, 1e-6).float()
    r1 = hip.rmsnorm_rope(x, ones, 24, 1e-6, tab.real.contiguous().cuda(), tab.imag.contiguous().cuda()).float()
    assert (r0.pow(2).mean(-1) - 1).abs().max().item() < 2e-2                         # unit RMS
    n0 = r0.view(N, 24, 64, 2).pow(2).sum(-1)
    n1 = r1.view(N, 24, 64, 2).pow(2).sum(-1)
    assert bool(((n0 - n1).abs() <= 0.02 * n0 + 0.01).all())                           # rotations preserve each pair's norm
    assert torch.equal(r0[0, :1], r1[0, :1])                                           # token (0,0,0): angle 0 -> identity

"""The two attention paths that are assembled on the host from library GEMMs and the project's row-softmax kernels, against the oracle:
the VAE mid AttentionBlock (VideoVAE38_._attn around fg_softmax_rows_f32_bf16) and the umT5 layer (WanTextEncoder.forward around
fg_softmax_bias_bf16 and fg_gated_gelu_bf16).

1. fg_softmax_rows_f32_bf16 against an fp64 softmax with the relative criterion of assert_probs_close (1 bf16 ulp of each probability,
   no floor, row sums), at every column count where the 256-thread row walk changes (one trip, a full trip, a ragged second trip, the
   (30, 52) tile's 1560 keys, the untiled 704 x 1280 latent's 3520) and on rows whose exact result is known.
2. fg_softmax_bias_bf16 at the encoder's geometry (L up to 512, 64 heads) against the oracle's formula, with every mask form the kernel
   can be given; the empty negative prompt (one valid key) must give exactly [1, 0, 0, ...].
3. _attn at decoder width (1024 channels) with weights that make the softmax peaked, and frame by frame, bit for bit.
4. WanTextEncoder at full width, two layers, on one, 300 and "no mask" valid tokens; valid rows must not see the pad tokens.

Cost: the CPU references of the module take about 20 s on an 8-thread host: 3 to 4 s for each of the three full-width umT5 cases (the
oracle in bf16 and in fp32), 1 to 2 s for the (2, 30, 52) mid block, 5 s for the twenty softmax_bias cases; the device time is negligible.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import seeded
from fairygen_amd import synthetic
from oracle import wan_text, wan_vae
from test_hip_kernels import ATTN_FLOOR, _cl, _ncthw, assert_probs_close, dev, hip  # noqa: F401  (hip: the module fixture)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
BF16_MIN = torch.finfo(BF16).min
LOGIT_STD = 5.0          # standard deviation of the scaled logits of a random row, as test_softmax_latent_unpatchify_uint8 has it (20 * 0.25)


# ------------------------------------------------------------------------------------------------ 1. fg_softmax_rows_f32_bf16
def _mid_width():
    """Channels of the decoder's mid AttentionBlock at the shipped configuration (its softmax scale is C ** -0.5), read from the module."""
    from fairygen_amd.wan_video_vae import WanVideoVAE38
    with torch.device("meta"):
        return WanVideoVAE38().model.decoder.middle[1].dim


def _in_checked_range(want):
    """Fraction of each row of `want` in [2^-100, 2^-9): large enough for the relative criterion, too small for an absolute one."""
    return ((want >= 2.0 ** -100) & (want < 2.0 ** -9)).double().mean(dim=-1)


def softmax_rows_input(cols, scale, seed=90):
    """(rows, cols) fp32 logits of mixed row kinds and {kind: row indices}.  `random` rows are N(0, (LOGIT_STD / scale)^2), the first of a
    seeded pool of 128 that meet the condition check_softmax_rows_input asserts (a row of 63 to 65 columns meets it only when its maximum
    stands out: 35 to 50 of the 128 do; 119 or more from 255 columns on, all from 1024 on).  The other kinds are built from further such rows:
      constant   one value in every column: every exp is exp(0) = 1, the sum is `cols`, every output is bf16(1 / cols);
      dominant   the row's maximum raised to 30 / scale, or 60 / scale, above the runner-up: the others sum to < cols * e^-30 < 2^-25,
                 so the fp32 sum is 1.0 and that output is exactly 1.0; with 60 the smallest others are below 2^-100;
      negative   the row minus 1e4: without the subtraction of the maximum every exp underflows, and the subtraction has to come before
                 the multiplication by scale (both scales here are powers of two, so only the former can show);
      last, c256 the maximum moved into the last column / into column 256, the first one of the second trip of the 256-thread walk,
                 at offset 0 and at offset -1e4."""
    sigma = LOGIT_STD / scale
    pool = seeded((128, cols), seed + cols, F32, scale=sigma)
    good = _in_checked_range(torch.softmax(pool.double() * scale, dim=-1)) >= 0.9
    r = pool[good] if cols > 1 else pool
    assert r.shape[0] >= 12, (cols, r.shape[0])
    rows, kinds = [], {}

    def add(kind, row):
        kinds.setdefault(kind, []).append(len(rows))
        rows.append(row)

    for i in range(6):
        add("random", r[i])
    add("constant", torch.full((cols,), 0.37 * sigma))
    add("constant", torch.full((cols,), -1e4))
    for i, margin in ((6, 30.0), (7, 60.0)):
        row = r[i].clone()
        j = row.argmax()
        row[j] = float("-inf")
        top = row.max() if cols > 1 else torch.tensor(0.0)
        row[j] = top + margin / scale
        add("dominant", row)
    for i in (8, 9):
        add("negative", r[i] - 1e4)
    for kind, col, i in (("last", cols - 1, 10), ("c256", 256, 11)):
        if 0 < col < cols:
            row = r[i].clone()
            row[col] = row.max() + 2.0 / scale
            add(kind, row)
            add(kind, row - 1e4)
    return torch.stack(rows).contiguous(), kinds


SOFTMAX_COLS = [1, 63, 64, 65, 255, 256, 257, 301, 1024, 1025, 1560, 3520]


def check_softmax_rows_input(s, kinds, scale):
    """The fp64 reference of one input, and the condition under which the relative criterion is what decides: in every row that is not
    degenerate by construction (constant, dominant, a single column) at least 90 % of the reference lies in [2^-100, 2^-9)."""
    want = torch.softmax(s.double() * scale, dim=-1)
    assert 5 <= s.shape[0] <= 40
    if s.shape[1] > 1:
        frac = _in_checked_range(want)
        for kind in ("random", "negative", "last", "c256"):
            for i in kinds.get(kind, []):
                assert frac[i] >= 0.9, f"cols {s.shape[1]} scale {scale}: row {i} ({kind}) has {frac[i].item():.3f} of its reference in range"
    return want


@pytest.mark.parametrize("scale", ["0.25", "mid"])
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows_vs_fp64(hip, cols, scale):
    scale = 0.25 if scale == "0.25" else _mid_width() ** -0.5
    s, kinds = softmax_rows_input(cols, scale)
    want = check_softmax_rows_input(s, kinds, scale)
    got = hip.softmax_rows(dev(s), scale)
    assert got.dtype == BF16 and got.shape == s.shape
    assert_probs_close(got, want, f"softmax_rows cols {cols} scale {scale:.5f}")
    got = got.float().cpu()
    for i in kinds["constant"]:
        assert (got[i] == torch.tensor(1.0 / cols, dtype=torch.float64).to(BF16).float()).all(), (cols, i, got[i].unique())
    for i in kinds["dominant"]:
        assert got[i, s[i].argmax()] == 1.0, (cols, i, got[i].max().item())
    for kind, col in (("last", cols - 1), ("c256", 256)):
        for i in kinds.get(kind, []):
            assert got[i].argmax() == col, (cols, kind, i)


# ------------------------------------------------------------------------------------------------ 2. fg_softmax_bias_bf16
SPIKE_HEAD, SPIKE = 1, 60.0


def softmax_bias_reference(scores, bias, mask, heads):
    """The lines of oracle.wan_text.t5_attention between the projections and the value product: the mask goes into the bf16 bias as
    finfo(bf16).min, the sum is rounded to bf16, the softmax runs in fp32 and is cast back."""
    L = scores.shape[-1]
    b = bias.view(1, heads, L, L).clone()
    if mask is not None:
        b.masked_fill_(mask.view(1, 1, 1, -1) == 0, BF16_MIN)
    attn = scores.view(1, heads, L, L) + b
    return F.softmax(attn.float(), dim=-1).type_as(attn).view(heads * L, L)


def key_mask(kind, L):
    if kind == "none":
        return None
    if kind == "holes":          # every third key off, the first one among them on
        return (torch.arange(L) % 3 != 1).to(torch.int32)
    keep = {"one": 1, "all_but_one": L - 1, "all": L}[kind]
    mask = torch.zeros(L, dtype=torch.int32)
    mask[:keep] = 1
    return mask


_bias_inputs = {}


def softmax_bias_input(L, heads):
    if L not in _bias_inputs:
        _bias_inputs.clear()          # one geometry at a time: 64 heads of 512 x 512 are 32 MiB each
        _bias_inputs[L] = (seeded((heads * L, L), 120 + L, scale=4.0), seeded((heads * L, L), 121 + L))
    return _bias_inputs[L]


@pytest.mark.parametrize("kind", ["none", "one", "all_but_one", "all", "holes"])
@pytest.mark.parametrize("L,heads", [(255, 4), (256, 4), (257, 4), (512, 64)])
def test_softmax_bias_real_geometry(hip, L, heads, kind):
    """Scores N(0, 4^2) and bias N(0, 1) as test_text_encoder_kernels has them, at the widths around the 256-thread stride and at the
    encoder's own (512 keys, 64 heads); head 1 carries a spike of +60 on the first masked key of every row, which must not win."""
    scores, bias = softmax_bias_input(L, heads)
    mask = key_mask(kind, L)
    off = None if mask is None else (mask == 0).nonzero().flatten()
    if off is not None and len(off):
        scores = scores.clone()
        scores[SPIKE_HEAD * L:(SPIKE_HEAD + 1) * L, off[0]] = SPIKE
    want = softmax_bias_reference(scores, bias, mask, heads)
    got = hip.softmax_bias(dev(scores), dev(bias), None if mask is None else dev(mask)).cpu()
    what = f"softmax_bias L {L} heads {heads} mask {kind}"
    assert_probs_close(got, want, what)
    frac = (got != want).float().mean().item()
    assert frac <= 0.02, f"{what}: {frac:.2e} of the elements differ from the oracle (allowed 2e-2)"
    if off is not None and len(off):
        assert not got[:, off].any(), f"{what}: a masked key has weight"
    if kind == "one":          # the empty negative prompt: EOS is the only valid token
        assert (got[:, 0] == 1).all() and not got[:, 1:].any()


# ------------------------------------------------------------------------------------------------ 3. the VAE mid AttentionBlock
MID = "model.decoder.middle.1"
QKV_WEIGHT_SCALE = 3.5          # chosen on the CPU: scaled logits of the oracle get a standard deviation of 4.5 to 5.2 per frame on the inputs below
DEVICE = "cuda"


@pytest.fixture(scope="module")
def mid_block():
    """The VAE at full decoder width (mid AttentionBlock of 1024 channels) with synthetic weights; only the block under test is
    materialised, _attn touches nothing else."""
    from fairygen_amd.wan_video_vae import WanVideoVAE38
    shapes = {k: v for k, v in synthetic.vae_shapes(dec_dim=256, dim=32).items() if k.startswith(MID + ".")}
    sd = synthetic.random_state_dict(shapes, seed=7)
    sd[MID + ".to_qkv.weight"] = (sd[MID + ".to_qkv.weight"].float() * QKV_WEIGHT_SCALE).to(BF16)
    with torch.device("meta"):
        vae = WanVideoVAE38(dim=32, dec_dim=256)
    blk = vae.model.decoder.middle[1]
    assert blk.dim == _mid_width()
    blk.to_empty(device=DEVICE).to(BF16)
    blk.load_state_dict({k[len(MID) + 1:]: v for k, v in sd.items()})
    return vae.model, blk.eval(), sd


def mid_input(t, h, w, c):
    """Channels-last (t, h, w, c) activations whose frames differ in scale and offset (the offset survives the RMS norm as a direction
    shared by the frame's pixels), small next to the attention branch (|.| up to 7) so that the residual does not cover it."""
    x = seeded((t, h, w, c), 300 + h).float()
    scale = torch.tensor([0.5, 0.05, 0.2])[:t].view(t, 1, 1, 1)
    offset = torch.tensor([0.0, 0.04, -0.1])[:t].view(t, 1, 1, 1)
    return (x * scale + offset).to(BF16)


def oracle_scaled_logits(sd, x):
    """(t, hw, hw) fp32: q k^T * C^-0.5 as oracle.wan_vae.attention_block forms them inside its SDPA."""
    t, h, w, c = x.shape
    f32 = {k: v.float() for k, v in sd.items()}
    y = wan_vae.rms_norm_c(f32, MID + ".norm", x.permute(0, 3, 1, 2).float())
    qkv = F.conv2d(y, f32[MID + ".to_qkv.weight"], f32[MID + ".to_qkv.bias"]).reshape(t, 3 * c, h * w)
    return torch.einsum("tci,tcj->tij", qkv[:, :c], qkv[:, c:2 * c]) * c ** -0.5


@pytest.mark.parametrize("t,h,w", [(1, 5, 7), (3, 13, 20), (2, 30, 52)])
def test_vae_mid_attention_vs_oracle(hip, mid_block, t, h, w):
    """VideoVAE38_._attn (RMS norm kernel, qkv GEMM, fp32 q k^T, fg_softmax_rows_f32_bf16, probs @ v, proj GEMM, residual kernel) against
    oracle.wan_vae.attention_block on the same weights: 35 keys, 260 keys (past the softmax kernel's 256 stride) and the bench tile's
    1560; error to the oracle's fp32 evaluation <= 2x that of the oracle's own bf16 evaluation + ATTN_FLOOR, at the maximum and on
    average.  to_qkv.weight is 3.5x the synthetic default, which makes the softmax peaked (asserted: standard deviation of the scaled
    logits between 3 and 8 in every frame; with the default it is 0.4 and the rows are near uniform).
    Measured on the CPU (oracle bf16 vs fp32, max / mean): 0.104 / 0.0081 at (1, 5, 7), 0.151 / 0.0083 at (3, 13, 20), 0.229 / 0.0100
    at (2, 30, 52), on outputs of |.| up to 7.5, so ATTN_FLOOR (2e-3) is a small addition and stays as it is.  A frame reading the
    previous frame's keys is off by 7 to 8 at the maximum."""
    model, blk, sd = mid_block
    x = mid_input(t, h, w, blk.dim)
    for f, std in enumerate(oracle_scaled_logits(sd, x).flatten(1).std(dim=1).tolist()):
        assert 3.0 <= std <= 8.0, f"frame {f}: the scaled logits have standard deviation {std:.2f}"
    xc = _ncthw(x)
    ref16 = wan_vae.attention_block(sd, MID, xc).float()
    ref32 = wan_vae.attention_block({k: v.float() for k, v in sd.items()}, MID, xc.float())
    with torch.no_grad():
        got = _ncthw(model._attn(blk, dev(x)).cpu()).float()
    assert got.shape == ref32.shape
    err_ref, err = (ref16 - ref32).abs(), (got - ref32).abs()
    print(f"mid attention {(t, h, w)}: max {err.max().item():.4f} (oracle bf16 {err_ref.max().item():.4f}), mean {err.mean().item():.5f} ({err_ref.mean().item():.5f})")
    assert err.max().item() <= 2 * err_ref.max().item() + ATTN_FLOOR, (err.max().item(), err_ref.max().item())
    assert err.mean().item() <= 2 * err_ref.mean().item() + ATTN_FLOOR, (err.mean().item(), err_ref.mean().item())


def test_vae_mid_attention_frames_are_independent(hip, mid_block):
    """Attention runs per frame: frame f of a 3-frame call equals, bit for bit, the 1-frame call on that frame alone (the frames differ
    in scale and offset, so a q, k or v slice taken from a neighbour cannot go unnoticed)."""
    model, blk, _ = mid_block
    x = dev(mid_input(3, 13, 20, blk.dim))
    with torch.no_grad():
        full = model._attn(blk, x)
        for f in range(3):
            one = model._attn(blk, x[f:f + 1].contiguous())
            assert torch.equal(one[0], full[f]), (f, (one[0].float() - full[f].float()).abs().max().item())
    assert not torch.equal(full[0], full[1]) and not torch.equal(full[1], full[2])


# ------------------------------------------------------------------------------------------------ 4. the umT5 layer
TEXT_KWARGS = dict(vocab=64, num_layers=2)          # every other dimension at its default: dim 4096, 64 heads of 64, ffn 10240, 32 buckets
TEXT_CASES = {"one_valid": (512, 1), "300_valid": (512, 300), "no_mask": (257, None)}


def _text_state_dict():
    """Synthetic weights, scaled as oracle/gen_text_full.py scales them and for its reason (N(0, 0.02^2) everywhere is chaotic in bf16):
    token embeddings of unit scale (x50), projections x0.5; the relative-position embeddings also x50, so that the attention bias is
    of order 1 like a trained T5's and not lost next to the scores."""
    sd = synthetic.random_state_dict(synthetic.text_encoder_shapes(TEXT_KWARGS), seed=1234, device=DEVICE)      # 380 M values: drawn on the device
    return {k: (v * (50.0 if "embedding" in k else 0.5) if v.dim() == 2 else v).cpu() for k, v in sd.items()}


def _text_ids(L, valid, seed=61):
    """(ids, mask): `valid` real tokens in front, the pad id 0 behind; mask None means every token is real."""
    ids = torch.randint(1, TEXT_KWARGS["vocab"], (1, L), generator=torch.Generator("cpu").manual_seed(seed))
    if valid is None:
        return ids, None
    mask = torch.zeros((1, L), dtype=torch.long)
    mask[:, :valid] = 1
    return ids * mask, mask


@pytest.fixture(scope="module")
def text_encoder():
    from fairygen_amd.wan_video_text_encoder import WanTextEncoder
    sd = _text_state_dict()
    with torch.device("meta"):
        enc = WanTextEncoder(**TEXT_KWARGS)
    assert (enc.dim, enc.num_heads, enc.dim_ffn, enc.num_buckets) == (4096, 64, 10240, 32)
    enc.load_state_dict(sd, assign=True)
    return enc.to(device=DEVICE, dtype=BF16).eval(), sd


@pytest.mark.parametrize("case", list(TEXT_CASES))
def test_text_encoder_layers_full_width_vs_oracle(hip, text_encoder, case):
    """WanTextEncoder.forward (two full-width layers: T5LayerNorm kernel, q / k / v GEMMs, bmm, fg_softmax_bias_bf16 with the relative
    position bias and the key mask, bmm, o GEMM, fg_gated_gelu_bf16 FFN) against oracle.wan_text.text_encoder: error to the oracle's fp32
    evaluation <= 2x that of its bf16 evaluation + 1e-2 (the floor of test_text_encoder_full_width_vs_reference_golden), on every row,
    the pad tokens' included.  One valid token is the empty negative prompt (EOS only).
    Measured on an MI355X (16 host threads), error of the encoder / of the oracle's bf16 evaluation: 0.0289 / 0.0299 with one valid token,
    0.0573 / 0.0573 with 300, 0.0508 / 0.0508 without a mask, on outputs of |.| up to 5.3."""
    enc, sd = text_encoder
    L, valid = TEXT_CASES[case]
    ids, mask = _text_ids(L, valid)
    ref16 = wan_text.text_encoder(sd, ids, mask, enc.num_heads).float()
    ref32 = wan_text.text_encoder({k: v.float() for k, v in sd.items()}, ids, mask, enc.num_heads)
    with torch.no_grad():
        got = enc(dev(ids), None if mask is None else dev(mask)).float().cpu()
    assert got.shape == ref32.shape == (1, L, enc.dim)
    err_ref, err = (ref16 - ref32).abs().max().item(), (got - ref32).abs().max().item()
    print(f"umT5 layers {case}: max error {err:.4f} (oracle bf16 {err_ref:.4f}), |fp32 output| up to {ref32.abs().max().item():.2f}")
    assert err <= 2 * err_ref + 1e-2, (case, err, err_ref)


def test_text_encoder_valid_rows_ignore_pad_tokens(hip, text_encoder):
    """The key mask keeps every pad token out of every valid token's attention, and nothing else mixes rows: with 300 valid tokens the
    first 300 output rows are the same bits whatever ids stand in the padded positions."""
    enc, _ = text_encoder
    L, valid = TEXT_CASES["300_valid"]
    ids, mask = _text_ids(L, valid)
    other = ids.clone()
    other[:, valid:] = torch.randint(1, TEXT_KWARGS["vocab"], (1, L - valid), generator=torch.Generator("cpu").manual_seed(62))
    assert not (other[:, valid:] == ids[:, valid:]).any()
    with torch.no_grad():
        a, b = enc(dev(ids), dev(mask)), enc(dev(other), dev(mask))
    assert torch.equal(a[:, :valid], b[:, :valid]), (a[:, :valid].float() - b[:, :valid].float()).abs().max().item()
    assert not torch.equal(a[:, valid:], b[:, valid:])

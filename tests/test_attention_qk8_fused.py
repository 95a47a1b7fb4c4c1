"""The e4m3 operands of the opt-in 8-bit Q K^T self-attention written by the RMSNorm+RoPE pass itself (include/fairygen_hip.h:
fg_rmsnorm_rope_q8_bf16, fg_rmsnorm_rope_kstats_bf16, fg_attn_quant_k_bf16; WanModel.enable_qk8_attention(fused_producer=True)).  The recipe
is tests/test_attention_qk8.py's, unchanged, and the yardstick is the path that file pins to it: hip.rmsnorm_rope -> hip.attn_quant_qk.  The
fused producers must write the same q8, sq, k, k8, sk and key mean byte for byte, so nothing here has a tolerance.

  1. (no GPU) the two identities the one-pass key statistics rest on, in torch: an exact fp64 column sum does not depend on its order, and
     max_rows |fl(v - m)| = max(fl(vmax - m), fl(m - vmin)); and that the inputs of the GPU tests lie where the fp64 sum is exact.
  2. (no GPU) the ABI: declared once, exported, bound; the argument checks; the routing switch.
  3. the producers against the two-step path on strided, poisoned, guarded buffers; the composed attention; stream and capture.
  4. the tiny DiT forward and the captured loop: fused_producer=True equals fused_producer=False bit for bit."""
import ctypes
import functools
import math
import os
import re

import pytest
import torch

from conftest import REPO, seeded
from fairygen_amd import hip as _hip
from fairygen_amd import synthetic

gpu = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
EPS = 1e-6
# (N, heads): row counts that are no multiple of 4 (the rows of a workgroup's pass) nor of a workgroup's walk, fewer rows than partial
# records (1, 15, 17: neutral records), more than one row per wave (4 099 > 4 x 256), and the production vector count (24 heads)
SHAPES = ((1, 2), (15, 2), (17, 2), (1030, 2), (4099, 2), (1030, 24))
TABLES = ("f32", "f64", "none")
VARIANTS = ("normal", "flat-head", "offset", "zero-row")


# ------------------------------------------------------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def case(n, heads, variant):
    """The (1, n, 3C) q | k | v buffer of the qkv GEMM, the two norm weights and the rope angles (n, 64)."""
    c = heads * 128
    qkv = seeded((1, n, 3 * c), 4000 + n + heads)
    if variant == "flat-head":        # head 1's keys are all equal (zero in, zero after the norm and any rotation): sk at its floor
        qkv[..., c + 128:c + 256] = 0
    elif variant == "offset":         # one key channel (of head 0) far from 0: the mean matters
        qkv[..., c + 5] += 3.0
    elif variant == "zero-row":       # a zero query row: sq at its floor
        qkv[0, min(7, n - 1), :c] = 0
    wq, wk = (1 + 0.1 * seeded((c,), 4100 + heads).float()).to(BF16), (1 + 0.1 * seeded((c,), 4200 + heads).float()).to(BF16)
    ang = torch.rand((n, 64), generator=torch.Generator("cpu").manual_seed(4300 + n), dtype=torch.float64) * (2 * math.pi)
    if variant == "offset":
        ang[:, 2] = 0                 # channels 4 | 5 are not rotated, so the offset is not averaged away over the rows
    return qkv, wq, wk, ang


def tables(ang, mode, device=None):
    """The rope arguments (cos, sin) of hip.rmsnorm_rope for a table mode."""
    if mode == "none":
        return None, None
    if mode == "f64":
        return ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)
    return torch.stack([ang.cos(), ang.sin()], -1).float().contiguous().to(device), None


def norm_rope_emu(x, w, ang):
    """RMSNorm * weight, then the rotation, in fp32 on the CPU with the kernel's bf16 rounding points: close to the kernel's bf16 row (not
    pinned to it: used for the range of the values only)."""
    xf = x.float()
    y = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)).to(BF16).float() * w.float()
    y = y.to(BF16).float().view(x.shape[0], -1, 64, 2)
    if ang is None:
        return y.reshape(x.shape).to(BF16)
    cs, sn = ang.cos().float().view(-1, 1, 64), ang.sin().float().view(-1, 1, 64)
    return torch.stack([y[..., 0] * cs - y[..., 1] * sn, y[..., 0] * sn + y[..., 1] * cs], -1).reshape(x.shape).to(BF16)


def exact_sum_bits(k, n):
    """Bits an exact sum of the n rows of the bf16 tensor k needs: the exponent spread of its non-zero values + 8 + ceil(log2 n)."""
    a = k.float().abs()
    a = a[a > 0]
    if a.numel() == 0:
        return 0
    spread = int(torch.frexp(a.max())[1]) - int(torch.frexp(a.min())[1])
    return spread + 8 + math.ceil(math.log2(n)) if n > 1 else spread + 8


# ------------------------------------------------------------------------------------------------------------------ 1. the identities
def identity_cases():
    g = torch.Generator("cpu").manual_seed(77)
    for i in range(40):
        n = 1 if i < 3 else int(torch.randint(2, 3000, (1,), generator=g))
        k = torch.randn((n, 32), generator=g)
        if i % 4 == 1:
            k[:, :8] += 3.0                       # offset columns
        if i % 4 == 2:
            k[:, 8:16] = k[0, 8:16].clone()       # constant columns
        if i % 4 == 3:
            k[:, 16:24] *= 2.0 ** -12
        yield k.to(BF16), g


def test_exact_fp64_sum_does_not_depend_on_its_order():
    for k, g in identity_cases():
        n = k.shape[0]
        assert exact_sum_bits(k, n) <= 52
        straight = k.double().sum(0)
        perm = torch.randperm(n, generator=g)
        parts = [k[perm[i::7]].double().sum(0) for i in range(7)]            # strided partial sums, as the workgroups take them
        order = torch.randperm(7, generator=g).tolist()
        shuffled = torch.zeros(k.shape[1], dtype=torch.float64)
        for i in order:
            shuffled += parts[i]
        seq = torch.zeros(k.shape[1], dtype=torch.float64)
        for r in range(min(n, 64)):                                           # one row at a time, where that is quick
            seq += k[r].double()
        assert torch.equal(shuffled, straight), f"n = {n}"
        assert n > 64 or torch.equal(seq, straight)
        assert torch.equal((shuffled / n).float(), (straight / n).float())


def test_scale_from_the_column_extremes():
    for k, _ in identity_cases():
        n = k.shape[0]
        m = (k.double().sum(0) / n).float()
        kf = k.float()
        want = (kf - m).abs().amax(0)                                         # the rounded differences of the two-pass kernel
        got = torch.maximum(kf.amax(0) - m, m - kf.amin(0))
        assert torch.equal(got, want), f"n = {n}"
        assert (got >= 0).all()


def test_gpu_inputs_lie_where_the_sum_is_exact():
    """exponent spread + 8 + ceil(log2 N) <= 52 for the keys of every case below — on the CPU emulation of the norm, with 2 bits in hand
    for where its rounding is not the kernel's (the GPU test repeats the count on the kernel's own bf16 keys)."""
    for (n, heads) in SHAPES:
        for variant in VARIANTS:
            check_sum_is_exact(n, heads, variant)


def check_sum_is_exact(n, heads, variant):
    qkv, _, wk, ang = case(n, heads, variant)
    c = heads * 128
    for a in (ang, None):
        bits = exact_sum_bits(norm_rope_emu(qkv[0, :, c:2 * c], wk, a), n)
        assert bits <= 50, f"N = {n}, {heads} heads, {variant}: an exact sum needs {bits} bits"


# ------------------------------------------------------------------------------------------------------------------ 2. the ABI and the switch
NAMES = ("fg_rmsnorm_rope_q8_bf16", "fg_rmsnorm_rope_kstats_bf16", "fg_attn_quant_k_bf16")
QUERIES = ("fg_attn_qk8_fused_version", "fg_attn_qk8_fused_scratch_bytes")


def test_abi_declared_exported_bound():
    lib = _hip.load()
    header = open(os.path.join(REPO, "include", "fairygen_hip.h")).read()
    assert _hip.QK8F_ABI_VERSION == 1 and lib.fg_attn_qk8_fused_version() == 1
    assert header.count("version of this extension, currently 1") == 2
    # the entry points and their two query functions: declared in the header, each exactly once, and in EXPORTED_SYMBOLS
    declared = re.findall(r"^(?:int|int64_t) (fg_[a-z0-9_]+)\s*\(", header, re.M)
    for name in NAMES + QUERIES:
        assert declared.count(name) == 1 and name in _hip.EXPORTED_SYMBOLS, name
    assert set(QUERIES) <= set(_hip._QUERIES)
    assert lib.fg_version() == _hip.ABI_VERSION and lib.fg_attn_qk8_version() == 1
    assert re.search(r"^int fg_rmsnorm_rope_q8_bf16\(const void\* x, int64_t ldx, const void\* weight, const void\* cos_tab, const void\* sin_tab, "
                     r"int table_f32,\s*void\* q8, float\* sq, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream\);", header, re.M)
    assert re.search(r"^int fg_rmsnorm_rope_kstats_bf16\(const void\* x, int64_t ldx, const void\* weight, const void\* cos_tab, const void\* sin_tab, "
                     r"int table_f32,\s*void\* k_out, void\* partials, int64_t partials_bytes, int64_t rows, int C, int num_heads, float eps,\s*"
                     r"fg_stream_t stream\);", header, re.M)
    assert re.search(r"^int fg_attn_quant_k_bf16\(const void\* k, int64_t ldk, const void\* partials, int64_t partials_bytes, void\* k8, float\* sk, "
                     r"float\* kbar,\s*int64_t N, int H, int D, fg_stream_t stream\);", header, re.M)
    assert re.search(r"^int64_t fg_attn_qk8_fused_scratch_bytes\(int64_t rows, int C\);", header, re.M)
    V, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert {n: _hip._SIGNATURES[n] for n in NAMES} == {NAMES[0]: [V, I64, V, V, V, I32, V, V, I64, I32, I32, F, V],
                                                       NAMES[1]: [V, I64, V, V, V, I32, V, V, I64, I64, I32, I32, F, V],
                                                       NAMES[2]: [V, I64, V, I64, V, V, V, I64, I32, I32, V]}
    raw = ctypes.CDLL(_hip.library_path())
    for name in NAMES:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _hip._SIGNATURES[name]
    assert hasattr(raw, "fg_attn_qk8_fused_version") and hasattr(raw, "fg_attn_qk8_fused_scratch_bytes")


def test_scratch_bytes():
    lib = _hip.load()
    size = lib.fg_attn_qk8_fused_scratch_bytes
    for c in (256, 3072):
        got = [size(n, c) for n in (1, 15, 17, 1030, 4099, 27280, 10 ** 6)]
        assert all(b > 0 and b % (16 * c) == 0 for b in got)
        parts = [b // (16 * c) for b in got]
        assert parts == sorted(parts) and parts[-1] == parts[-2] <= 512, "a few hundred workgroups at most, whatever the row count"
        assert parts[0] > 1, "fewer rows than records: the neutral record is reached"
    assert [size(n, 256) // 256 for n in (15, 4099)] == [size(n, 3072) // 3072 for n in (15, 4099)], "the count depends on the rows alone"
    for bad in ((0, 256), (10, 0), (10, 192), (10, 8192)):
        assert size(*bad) == -1 and b"fg_attn_qk8_fused_scratch_bytes" in lib.fg_last_error()


def test_argument_checks():
    """Bad arguments are refused on the host, before anything is launched (FG_EINVAL = -1), with a message."""
    lib, a, big = _hip.load(), 4096, 1 << 40
    need = lib.fg_attn_qk8_fused_scratch_bytes(10, 256)

    def refused(fn, args, word=None):
        rc = getattr(lib, fn)(*args)
        msg = lib.fg_last_error()
        assert rc == -1 and fn.encode() in msg, (fn, args, rc, msg)
        assert word is None or word in msg, (fn, msg)

    def q8(x=a, ldx=768, w=a, cos=a, sin=None, f32=1, o=a, sq=a, rows=10, c=256, h=2):
        return (x, ldx, w, cos, sin, f32, o, sq, rows, c, h, EPS, None)

    def ks(x=a, ldx=768, w=a, cos=a, sin=None, f32=1, o=a, parts=a, nbytes=big, rows=10, c=256, h=2):
        return (x, ldx, w, cos, sin, f32, o, parts, nbytes, rows, c, h, EPS, None)

    def qk(k=a, ldk=256, parts=a, nbytes=big, k8=a, sk=a, kbar=a, n=10, h=2, d=128):
        return (k, ldk, parts, nbytes, k8, sk, kbar, n, h, d, None)
    for fn, mk in ((NAMES[0], q8), (NAMES[1], ks)):
        refused(fn, mk(x=None), b"null")
        refused(fn, mk(w=None), b"null")
        refused(fn, mk(o=None), b"null")
        refused(fn, mk(c=256, h=4), b"head_dim 128")          # C != H * 128
        refused(fn, mk(c=192, h=3), b"head_dim 128")
        refused(fn, mk(x=a + 8), b"aligned")
        refused(fn, mk(ldx=248), b"ldx")                      # below C
        refused(fn, mk(ldx=772), b"ldx")                      # no multiple of 8
        refused(fn, mk(rows=0))
        refused(fn, mk(cos=None), b"table")                   # fp32 mode without its table
        refused(fn, mk(f32=0, cos=a, sin=None), b"table")     # fp64 mode with one table
    refused(NAMES[0], q8(sq=None), b"null")
    refused(NAMES[0], q8(o=a + 4), b"aligned")                # q8: 8 bytes
    refused(NAMES[0], q8(sq=a + 2), b"aligned")               # the scales: 4
    refused(NAMES[1], ks(parts=None), b"null")
    refused(NAMES[1], ks(o=a + 8), b"aligned")                # k_out: 16
    refused(NAMES[1], ks(parts=a + 8), b"aligned")            # partials: 16
    refused(NAMES[1], ks(nbytes=need - 1), b"partials")
    refused(NAMES[2], qk(d=64), b"head_dim 128")
    for null in ("k", "parts", "k8", "sk", "kbar"):
        refused(NAMES[2], qk(**{null: None}), b"null")
    refused(NAMES[2], qk(ldk=248), b"ldk")
    refused(NAMES[2], qk(ldk=260), b"ldk")
    refused(NAMES[2], qk(k=a + 8), b"aligned")
    refused(NAMES[2], qk(parts=a + 8), b"aligned")
    refused(NAMES[2], qk(k8=a + 4), b"aligned")
    refused(NAMES[2], qk(sk=a + 2), b"aligned")
    refused(NAMES[2], qk(nbytes=need - 1), b"partials")
    refused(NAMES[2], qk(n=0))


def test_enable_sets_the_routing():
    """The switch, and the one predicate that routes a block's self-attention to the e4m3 kernel.  A plain enable_qk8_attention() keeps the
    two-step producers — tests/test_attention_qk8.py::test_tiny_dit_forward counts their launches — and ModelConfig(attention_dtype=...)
    takes the fused ones."""
    from fairygen_amd import wan_video_dit as dit
    with torch.device("meta"):
        m = dit.WanModel(**synthetic.TINY_DIT_KWARGS)
    attn = m.blocks[0].self_attn.attn
    assert m.qk8_attention is False and m.qk8_fused_producer is False
    assert not dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV + 1, 1), "the mode is off"
    assert m.enable_qk8_attention(fused_producer=True) is m and m.qk8_attention is True and m.qk8_fused_producer is True
    assert dit.QK8_MIN_KV == 1024
    assert dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV + 1, 1) and not dit.takes_qk8_attention(m, attn, dit.QK8_MIN_KV, 1)
    assert not dit.takes_qk8_attention(m, attn, 4 * dit.QK8_MIN_KV, 2), "one batch element"

    class Other(dit.AttentionModule):
        pass
    assert not dit.takes_qk8_attention(m, Other(attn.num_heads), 4 * dit.QK8_MIN_KV, 1), "the stock AttentionModule only"
    m.enable_qk8_attention(fused_producer=False)
    assert m.qk8_attention is True and m.qk8_fused_producer is False
    m.enable_qk8_attention(True, True)
    m.enable_qk8_attention(False)
    assert m.qk8_attention is False and m.qk8_fused_producer is False
    m.enable_qk8_attention(False, fused_producer=True)
    assert m.qk8_fused_producer is False, "no fused producer without the mode"
    m.enable_qk8_attention()
    assert m.qk8_attention is True and m.qk8_fused_producer is False


def test_model_config_takes_the_fused_producer(tmp_path):
    from fairygen_amd import loader
    sd = synthetic.random_state_dict(synthetic.dit_shapes(synthetic.TINY_DIT_KWARGS), seed=1)
    path = synthetic.save_checkpoint(sd, str(tmp_path / "tiny_dit.safetensors"))
    entry = {"model_hash": loader.hash_model_file(path), "model_name": "wan_video_dit", "model_class": "fairygen_amd.wan_video_dit.WanModel",
             "extra_kwargs": synthetic.TINY_DIT_KWARGS}
    loader.MODEL_CONFIGS.append(entry)
    try:
        base = {"computation_dtype": BF16, "computation_device": "cpu"}
        pool = loader.ModelPool()
        pool.auto_load_model(path, vram_config=dict(base, attention_dtype=F8))
        pool.auto_load_model(path, vram_config=base)
        assert pool.model[0].qk8_attention is True and pool.model[0].qk8_fused_producer is True
        assert pool.model[1].qk8_attention is False and pool.model[1].qk8_fused_producer is False
    finally:
        loader.MODEL_CONFIGS.remove(entry)


# ------------------------------------------------------------------------------------------------------------------ 3. the producers
@pytest.fixture(scope="module")
def hip():
    _hip.load()
    assert torch.cuda.is_available()
    return _hip


@functools.lru_cache(maxsize=None)
def reference(n, heads, variant, mode):
    """The two-step path on the device: (k bf16, q8, k8, sq, sk, key mean) of hip.rmsnorm_rope x 2 -> hip.attn_quant_qk.  Computed once."""
    qkv, wq, wk, ang = case(n, heads, variant)
    c = heads * 128
    d, cs = qkv.cuda(), tables(ang, mode, "cuda")
    q = _hip.rmsnorm_rope(d[..., :c], wq.cuda(), heads, EPS, *cs)
    k = _hip.rmsnorm_rope(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    q8, k8, sq, sk, kbar = _hip.attn_quant_qk(q, k, heads)
    torch.cuda.synchronize()
    return k[0], q8, k8, sq, sk, kbar


def poisoned(g, shape, dtype):
    """An output of `shape` inside guard rows, every byte of the output itself a NaN of its type (0x7F: e4m3 NaN; no kernel here writes one)."""
    fill = {F8: 0x7F, BF16: 0x7FA5, torch.float32: 0x7FC5A5A5}[dtype]
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[torch.empty((), dtype=dtype).element_size()]
    return g.embed(torch.full(shape, fill, dtype=bits).view(dtype))


@gpu
@pytest.mark.parametrize("mode", TABLES)
@pytest.mark.parametrize("n,heads", SHAPES)
def test_producers_equal_the_two_step_path(hip, n, heads, mode):
    check_producers(hip, n, heads, mode)


def check_producers(hip, n, heads, mode, variants=VARIANTS):
    """The three producers on case(n, heads, variant) against reference(...), byte for byte, on poisoned and guarded buffers."""
    from test_buffer_contract import Guards
    c = heads * 128
    for variant in variants:
        qkv, wq, wk, ang = case(n, heads, variant)
        k_ref, q8_ref, k8_ref, sq_ref, sk_ref, kbar_ref = reference(n, heads, variant, mode)
        bits = exact_sum_bits(k_ref.cpu(), n)
        assert bits <= 52, f"{variant}: the fp64 sum of these keys is not exact ({bits} bits): the comparison of the mean would not be one"
        d, cs = qkv.cuda(), tables(ang, mode, "cuda")                       # x: a column slice, ldx = 3C
        g = Guards()
        q8, k8 = poisoned(g, (n, c), F8), poisoned(g, (n, c), F8)
        sq, sk, kbar = poisoned(g, (n, heads), torch.float32), poisoned(g, (1, heads), torch.float32), poisoned(g, (1, c), torch.float32)
        k = poisoned(g, (n, c), BF16)
        need = hip.load().fg_attn_qk8_fused_scratch_bytes(n, c)
        parts = g.embed(torch.full((need // (16 * c), 16 * c), 0xFF, dtype=torch.uint8)).view(-1)
        hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs, out=k.view(1, n, c), partials=parts)
        hip.rmsnorm_rope_q8(d[..., :c], wq.cuda(), heads, EPS, *cs, q8=q8, sq=sq)
        hip.attn_quant_k(k.view(1, n, c), parts, heads, k8, sk.view(heads), kbar.view(c))
        g.check(f"N = {n}, {heads} heads, {mode}, {variant}")
        what = f"N = {n}, {heads} heads, {mode}, {variant}: "
        # every record of the partials was written: P x C sums, then minima, then maxima, none the 0xFF.. NaN of the fill
        pc = need // 16
        assert not torch.isnan(parts[:8 * pc].view(torch.float64)).any() and not torch.isnan(parts[8 * pc:].view(torch.float32)).any(), what
        for name, got, want in (("k", k, k_ref), ("sq", sq, sq_ref), ("sk", sk.view(heads), sk_ref), ("kbar", kbar.view(c), kbar_ref)):
            assert not torch.isnan(got.float()).any(), what + name + ": poison survived"
            assert torch.equal(got, want), what + f"{name}: {(got != want).sum().item()} of {want.numel()} differ"
        for name, got, want in (("q8", q8, q8_ref), ("k8", k8, k8_ref)):
            gb, wb = got.view(torch.uint8), want.view(torch.uint8)
            assert not ((gb & 0x7F) == 0x7F).any(), what + name + ": poison survived"
            assert torch.equal(gb, wb), what + f"{name}: {(gb != wb).sum().item()} of {wb.numel()} bytes differ"
        if variant == "flat-head":
            assert sk[0, 1].item() == 2.0 ** -20 and (n == 1 or sk[0, 0].item() > 2.0 ** -20)
        if variant == "zero-row":
            assert (sq[min(7, n - 1)] == 2.0 ** -20).all()
        if variant == "offset":
            assert kbar[0, 5].abs().item() > 1.0


@gpu
def test_composed_attention_equals_the_two_step_path(hip):
    check_composed_attention(hip, 1030, 2)


def check_composed_attention(hip, n, heads):
    c = heads * 128
    qkv, wq, wk, ang = case(n, heads, "normal")
    d, cs = qkv.cuda(), tables(ang, "f32", "cuda")
    q = hip.rmsnorm_rope(d[..., :c], wq.cuda(), heads, EPS, *cs)
    k = hip.rmsnorm_rope(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    want = hip.attention_qk8(q, k, d[..., 2 * c:], heads)
    k2, parts = hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk.cuda(), heads, EPS, *cs)
    q8, sq = hip.rmsnorm_rope_q8(d[..., :c], wq.cuda(), heads, EPS, *cs)
    k8, sk, _ = hip.attn_quant_k(k2, parts, heads)
    got = hip.attention_qk8_pre(q8, k8, sq, sk, d[..., 2 * c:], heads)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)


@gpu
def test_entry_points_only_enqueue_and_capture(hip):
    """The four launches recorded on a side stream into a graph (one stream, no parallel branch): nothing runs at capture (the outputs
    keep their fill), a replay gives the bytes of the eager calls."""
    n, heads, c = 1030, 2, 256
    qkv, wq, wk, ang = case(n, heads, "normal")
    d, cs, wq, wk = qkv.cuda(), tables(ang, "f32", "cuda"), wq.cuda(), wk.cuda()
    k_ref, q8_ref, k8_ref, sq_ref, sk_ref, kbar_ref = reference(n, heads, "normal", "f32")
    q8, k8, sq, sk, kbar, parts = hip.attention_qk8_fused_scratch(n, heads, 128, d.device)
    k = torch.zeros((1, n, c), dtype=BF16, device="cuda")
    for t in (q8, k8, parts):
        t.view(torch.uint8).fill_(0x7F)
    for t in (sq, sk, kbar):
        t.fill_(-1.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        hip.rmsnorm_rope_kstats(d[..., c:2 * c], wk, heads, EPS, *cs, out=k, partials=parts)
        hip.rmsnorm_rope_q8(d[..., :c], wq, heads, EPS, *cs, q8=q8, sq=sq)
        hip.attn_quant_k(k, parts, heads, k8, sk, kbar)
    torch.cuda.synchronize()
    assert (k == 0).all() and (sq == -1.0).all() and (sk == -1.0).all() and (kbar == -1.0).all(), "a capture launched work"
    assert all((t.view(torch.uint8) == 0x7F).all() for t in (q8, k8, parts)), "a capture launched work"
    graph.replay()
    torch.cuda.synchronize()
    for name, got, want in (("k", k[0], k_ref), ("q8", q8.view(torch.uint8), q8_ref.view(torch.uint8)), ("k8", k8.view(torch.uint8), k8_ref.view(torch.uint8)),
                            ("sq", sq, sq_ref), ("sk", sk, sk_ref), ("kbar", kbar, kbar_ref)):
        assert torch.equal(got, want), name


# ------------------------------------------------------------------------------------------------------------------ 4. the tiny DiT
LATENT = (1, 48, 3, 40, 40)      # tests/test_attention_qk8.py's 1 200-token case: above QK8_MIN_KV


def tiny_model():
    from fairygen_amd.wan_video_dit import WanModel
    cfg = synthetic.TINY_DIT_KWARGS
    m = WanModel(**cfg)
    m.load_state_dict(synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234))
    return m.to(device="cuda", dtype=BF16).eval(), cfg


@gpu
def test_tiny_dit_forward(hip, monkeypatch):
    """fused_producer=True equals fused_producer=False (which tests/test_attention_qk8.py::test_tiny_dit_forward pins to the oracle) with
    torch.equal, through the new entry points and none of the quantise pass's."""
    from fairygen_amd.wan_video import model_fn_wan_video
    m, cfg = tiny_model()
    lat, ctx, ts = seeded(LATENT, 11), seeded((1, 16, 128), 12), torch.tensor([995.9]).to(BF16)
    args = dict(latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
    calls, real = [], hip._call

    def call(name, *a):
        calls.append(name)
        return real(name, *a)
    with torch.no_grad():
        want = model_fn_wan_video(m.enable_qk8_attention(fused_producer=False), **args)
        monkeypatch.setattr(hip, "_call", call)
        got = model_fn_wan_video(m.enable_qk8_attention(fused_producer=True), **args)
        monkeypatch.setattr(hip, "_call", real)
        off = model_fn_wan_video(m.enable_qk8_attention(False), **args)
    nb = cfg["num_layers"]
    assert all(calls.count(name) == nb for name in NAMES + ("fg_attn_fwd_qk8_bf16",)), {name: calls.count(name) for name in set(calls)}
    assert calls.count("fg_attn_quant_qk_bf16") == 0, "q and k went through the quantise pass too"
    assert calls.count("fg_rmsnorm_rope_bf16") == 2 * nb, "only cross-attention's two norms are left on the bf16 norm kernel"
    assert calls.count("fg_attn_fwd_bf16") == nb, "cross-attention stays on the bf16 kernel"
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} differ"
    assert not torch.equal(off, want), "the switch is dead"


@gpu
def test_graph_loop_equals_eager(hip):
    """graph=True with the mode and the fused producers: the captured step owns the operands' buffers and the partials, and replays to
    the bits of the eager loop — which are the bits of the loop with the two-step producers."""
    from fairygen_amd.wan_video import WanVideoPipeline
    m, _ = tiny_model()
    pipe = WanVideoPipeline(device="cuda", torch_dtype=BF16)
    pipe.dit = m.enable_qk8_attention(fused_producer=True)
    lat, ctx_p, ctx_n = seeded(LATENT, 21), seeded((1, 16, 128), 22), seeded((1, 16, 128), 23)
    z0 = seeded(LATENT[:2] + (1,) + LATENT[3:], 24)

    def loop(graph):
        pipe.scheduler.set_timesteps(4, denoising_strength=1.0, shift=5.0)
        latents = lat.clone()
        latents[:, :, 0:1] = z0
        inputs = {"latents": latents.cuda(), "fuse_vae_embedding_in_latents": True, "first_frame_latents": z0.cuda()}
        with torch.no_grad():
            out = pipe.denoise(inputs, {"context": ctx_p.cuda()}, {"context": ctx_n.cuda()}, 5.0, progress_bar_cmd=lambda x: x, graph=graph)
        torch.cuda.synchronize()
        return out.clone()
    want = loop(False)
    got = loop(True)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} latents differ from the eager loop"
    pipe.dit.enable_qk8_attention(fused_producer=False)
    assert torch.equal(loop(False), want), "the two-step producers give another loop"
    pipe.dit.enable_qk8_attention(False)
    assert not torch.equal(loop(False), want), "the loops above ran without the mode"

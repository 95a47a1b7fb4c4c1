"""Token shards reproduce the unsharded DiT rows.

Sequence parallelism (K/V all-gather, Ulysses, cfg_parallel) rests on one property: a rank that holds the tokens [lo, hi) computes, for
those rows, what the unsharded forward computes.  The launch plan may depend on the row count in two places only, the k-split pieces
of the GEMM and the split-KV of attention; a third, data-dependent exception is the per-wave deferred rescale of the 4-wave attention
kernel (below).

Part 1, kernel level, `torch.equal` on the bit patterns: every kernel of the token forward is called once on all rows and once per
shard, with row-sliced operands, the same tables and first_rows' = clamp(first_rows - lo, 0, hi - lo), the value
model_fn_wan_video_steps hands to a shard.  The shards put first_rows' at both ends (0: every rank after the first frame; rows: a rank
inside it), start off the 4-rows-per-workgroup grid of the row kernels and off the 256-row tiles of the GEMMs, and include single rows.
GEMMs run without a workspace (every element one k-ordered accumulation), attention without one (every q-block one direct workgroup).

The attention cases hold under a condition on the inputs, asserted on the CPU: gen_attn_w4.py decides per WAVE whether a tile's new
row maxima are applied (the deferred rescale, taken when any row of the wave moved by more than 2^6), and then rescales every row of
that wave, so a row's bits may depend on its wave-mates.  With max |scale * log2(e) * logit| <= 3 no maximum can move by more than 6
after the first tile, the branch is never taken, and a query row's bits do not depend on which rows share its wave.

Part 2, model level: P emulated ranks in ONE process.  forward_tokens_steps yields right after it has started each exchange, so P
generators advanced in turns can exchange through a mailbox (LoopbackShard) with no process group; the concatenated rank outputs are
held against the oracle and against the unsharded HIP forward on a dim-3072 model with N = 1950 tokens (4-wave self-attention, GEMMs
with real tile counts).  The mailbox logic has a CPU self-check on random tensors.
"""
import functools
import math
import types

import pytest
import torch

from conftest import seeded
from fairygen_amd import synthetic
from fairygen_amd.sequence_parallel import TokenShard
from oracle import wan_dit
from test_buffer_contract import _attn
from test_hip_kernels import assert_close_bf16, dev, hip  # noqa: F401  (hip: the module fixture)

gpu = pytest.mark.gpu

EPS = 1e-6
ROWS, FIRST = 333, 100
ROW_SHARDS = [(0, 100),        # first' == rows
              (100, 233),      # first' == 0, the shard starts on the boundary
              (97, 103),       # straddles; lo is no multiple of the 4 rows per workgroup
              (99, 100), (100, 101),      # single rows on either side
              (1, 333)]
WIDTHS = [3072, 264]           # 24 heads x 128; 3 heads x 88 (no power of two: the other rmsnorm_rope instantiation)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def shard_first(first, lo, hi):
    """first_rows of the shard [lo, hi), as model_fn_wan_video_steps computes it."""
    return min(max(first - lo, 0), hi - lo)


def gemm_shards(m):
    return [(0, 300),          # first' == M
            (300, m),          # first' == 0
            (257, m),          # the rows sit at other positions of their 256-row tile
            (511, 513)]


def _flat(outs):
    """The tensors of a (nested) result as 2-D (rows, cols) bit patterns."""
    if isinstance(outs, torch.Tensor):
        return [outs.reshape(-1, outs.shape[-1]).view(_INT[outs.element_size()])]
    return [t for o in outs for t in _flat(o)]


def assert_same_rows(got, full, lo, hi, what):
    got, full = _flat(got), _flat(full)
    assert len(got) == len(full)
    for i, (g, f) in enumerate(zip(got, full)):
        assert g.shape[0] == hi - lo and g.shape[1] == f.shape[1], (what, g.shape, f.shape)
        if not torch.equal(g, f[lo:hi]):
            bad = (g != f[lo:hi]).any(dim=1).nonzero().flatten()
            raise AssertionError(f"{what}: output {i} of the shard [{lo}, {hi}) differs from the same rows of the full call in "
                                 f"{bad.numel()} of {hi - lo} rows; first at local row {bad[0].item()}, last at {bad[-1].item()}")


def assert_shards(run, rows, first, shards, what):
    """run(lo, hi, first') on [0, rows) once, then on every shard: the same bits in the shard's rows."""
    full = run(0, rows, first)
    assert all(t.shape[0] == rows for t in _flat(full)), what
    for lo, hi in shards:
        assert_same_rows(run(lo, hi, shard_first(first, lo, hi)), full, lo, hi, what)


# ------------------------------------------------------------------------------------------------------------------ row kernels
@functools.lru_cache(maxsize=None)
def _row_data(c):
    d = dict(x=seeded((ROWS, c), 11), y=seeded((ROWS, c), 12), qkv=seeded((ROWS, 3 * c), 13),
             w=(1 + 0.1 * seeded((c,), 14).float()).to(torch.bfloat16), b=seeded((c,), 15, scale=0.1))
    for r in (1, 2, ROWS):
        d[f"t{r}"] = seeded((r, 6, c), 16 + r % 7, scale=0.5)
    return {k: dev(v) for k, v in d.items()}


def _mod(hip, d, mod_rows, lo, hi, first):
    """The table of the call on [lo, hi): the same one or two rows, or the rows of the shard's tokens."""
    t = d[f"t{mod_rows}"]
    return hip.ModTable(t[lo:hi] if mod_rows == ROWS else t, first)


@gpu
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("mod_rows", [1, 2, ROWS])
def test_ln_modulate_row_shards(hip, c, mod_rows):
    d = _row_data(c)
    for fn in (hip.ln_modulate, hip.ln_modulate_fp8, hip.ln_modulate_dual):
        assert_shards(lambda lo, hi, first: fn(d["x"][lo:hi], _mod(hip, d, mod_rows, lo, hi, first), 0, 1, EPS),
                      ROWS, FIRST, ROW_SHARDS, f"{fn.__name__} C={c} mod_rows={mod_rows}")
    if mod_rows == 2:      # the two table rows are told apart at all: another first_rows changes exactly the rows in between
        a, b = (hip.ln_modulate(d["x"], hip.ModTable(d["t2"], f), 0, 1, EPS) for f in (FIRST, 0))
        assert torch.equal(a[FIRST:], b[FIRST:]) and (a[:FIRST] != b[:FIRST]).any(dim=1).all()


@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_ln_affine_row_shards(hip, c):
    d = _row_data(c)
    for fn in (hip.ln_affine, hip.ln_affine_dual):
        assert_shards(lambda lo, hi, first: fn(d["x"][lo:hi], d["w"], d["b"], EPS), ROWS, FIRST, ROW_SHARDS, f"{fn.__name__} C={c}")


@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_gate_residual_row_shards(hip, c):
    d = _row_data(c)
    assert_shards(lambda lo, hi, first: hip.gate_residual(d["x"][lo:hi], d["y"][lo:hi]), ROWS, FIRST, ROW_SHARDS, f"gate_residual, no gate, C={c}")
    for mod_rows in (1, 2):
        assert_shards(lambda lo, hi, first: hip.gate_residual(d["x"][lo:hi], d["y"][lo:hi], _mod(hip, d, mod_rows, lo, hi, first), 2),
                      ROWS, FIRST, ROW_SHARDS, f"gate_residual C={c} mod_rows={mod_rows}")


@gpu
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("mod_rows", [1, 2])
def test_residual_ln_row_shards(hip, c, mod_rows):
    """fg_residual_ln_bf16 / fg_residual_ln_fp8_bf16: modulate and affine, gated and not; x_out and the norm output (bf16 row, or e4m3 row
    and scale) are all compared."""
    d = _row_data(c)
    for fp8 in (False, True):
        modulate = hip.residual_ln_modulate_fp8 if fp8 else hip.residual_ln_modulate
        affine = hip.residual_ln_affine_fp8 if fp8 else hip.residual_ln_affine
        for gate_idx in (2, None):
            what = f"C={c} mod_rows={mod_rows} fp8={fp8} gate={gate_idx}"
            assert_shards(lambda lo, hi, first: modulate(d["x"][lo:hi], d["y"][lo:hi], _mod(hip, d, mod_rows, lo, hi, first), gate_idx, 3, 4, EPS),
                          ROWS, FIRST, ROW_SHARDS, "residual_ln_modulate " + what)
            assert_shards(lambda lo, hi, first: affine(d["x"][lo:hi], d["y"][lo:hi], d["w"], d["b"], EPS,
                                                       mod=_mod(hip, d, mod_rows, lo, hi, first) if gate_idx is not None else None, gate_idx=gate_idx),
                          ROWS, FIRST, ROW_SHARDS, "residual_ln_affine " + what)


@functools.lru_cache(maxsize=None)
def _rope_tables(half):
    """Per-row angles: fp64 (cos, sin), the fp32 interleaved {cos, sin} table, and none."""
    ang = seeded((ROWS, half), 21, dtype=torch.float64) * math.pi
    cos, sin = dev(torch.cos(ang)), dev(torch.sin(ang))
    return {"f64": (cos, sin), "f32": (torch.stack([cos, sin], dim=-1).to(torch.float32).contiguous(), None), "none": (None, None)}


@gpu
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("tables", ["f64", "f32", "none"])
def test_rmsnorm_rope_row_shards(hip, c, tables):
    """x is the k column block of a (rows, 3C) buffer (the fused qkv output) or a contiguous tensor; the tables are sliced and made
    contiguous the way model_fn_wan_video_steps does it; the grouped form writes the k slot of a Ulysses send buffer for 3 ranks."""
    d = _row_data(c)
    heads = 24 if c == 3072 else 3
    cos, sin = _rope_tables(c // heads // 2)[tables]
    g = c // 3

    def local(t, lo, hi):
        return t[lo:hi].contiguous() if t is not None else None

    for src in ("qkv slice", "contiguous"):
        def x_of(lo, hi):
            return d["qkv"][lo:hi, c:2 * c] if src == "qkv slice" else d["x"][lo:hi]

        def plain(lo, hi, first):
            return hip.rmsnorm_rope(x_of(lo, hi), d["w"], heads, EPS, local(cos, lo, hi), local(sin, lo, hi))

        def grouped(lo, hi, first):
            n = hi - lo
            send = torch.zeros((3, n, 3, g), dtype=torch.bfloat16, device="cuda")
            hip.rmsnorm_rope(x_of(lo, hi), d["w"], heads, EPS, local(cos, lo, hi), local(sin, lo, hi),
                             grouped=(send.view(-1)[g:], g, n * 3 * g, 3 * g))
            assert not send[:, :, 0].any() and not send[:, :, 2].any()
            return send[:, :, 1].transpose(0, 1).reshape(n, c)
        assert_shards(plain, ROWS, FIRST, ROW_SHARDS, f"rmsnorm_rope C={c} tables={tables} x={src}")
        assert_shards(grouped, ROWS, FIRST, ROW_SHARDS, f"rmsnorm_rope grouped C={c} tables={tables} x={src}")
        assert torch.equal(plain(0, ROWS, FIRST), grouped(0, ROWS, FIRST))
    if tables != "none":      # the table rows are told apart: the table of the next row gives other bits in every row
        shifted = hip.rmsnorm_rope(d["x"][:-1], d["w"], heads, EPS, local(cos, 1, ROWS), local(sin, 1, ROWS))
        assert (shifted != hip.rmsnorm_rope(d["x"], d["w"], heads, EPS, cos, sin)[:-1]).any(dim=1).all()


@gpu
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("act", [None, "gelu_tanh"])
def test_fp8_quant_rows_row_shards(hip, c, act):
    d = _row_data(c)
    assert_shards(lambda lo, hi, first: hip.fp8_quant_rows(d["x"][lo:hi], act), ROWS, FIRST, ROW_SHARDS, f"fp8_quant_rows C={c} act={act}")
    assert_shards(lambda lo, hi, first: hip.fp8_quant_rows(d["qkv"][lo:hi, c:2 * c], act), ROWS, FIRST, ROW_SHARDS,
                  f"fp8_quant_rows on a column slice, C={c} act={act}")


# ------------------------------------------------------------------------------------------------------------------ GEMMs
def _gemm_kwargs(hip, mode, c, table, lo, hi, first):
    if mode == 2:
        return dict(out=c[lo:hi].clone(), residual=True, mod=hip.ModTable(table, first), gate_idx=2)
    if mode == 3:
        return dict(out=c[lo:hi].clone(), residual=True)
    return dict(act="gelu_tanh") if mode == 4 else {}


@gpu
@pytest.mark.parametrize("m,k,n", [(700, 256, 768), (4200, 512, 4096)])
@pytest.mark.parametrize("mode", [0, 2, 3, 4])
def test_gemm_bf16_row_shards(hip, m, k, n, mode):
    """fg_gemm_epilogue_bf16_s without a workspace: bias, x + gate * y with a two-row gate table (first_rows 300), x + y, GELU.  The last
    shard list entry repeats (257, M) with A as a column slice of a wider buffer."""
    wide = dev(seeded((m, k + 128), 31, scale=0.5))
    x, w, b = wide[:, 64:64 + k].contiguous(), dev(seeded((n, k), 32, scale=k ** -0.5)), dev(seeded((n,), 33, scale=0.2))
    c, table = dev(seeded((m, n), 34)), dev(seeded((2, 6, n), 35))

    def run(lo, hi, first, a=x):
        return hip.gemm_epilogue(a[lo:hi], w, b, workspace=False, **_gemm_kwargs(hip, mode, c, table, lo, hi, first))
    assert_shards(run, m, 300, gemm_shards(m), f"gemm_epilogue {m}x{k}x{n} mode {mode}")
    assert_same_rows(run(257, m, 43, wide[:, 64:64 + k]), run(0, m, 300), 257, m, f"gemm_epilogue {m}x{k}x{n} mode {mode}, strided A")


@gpu
@pytest.mark.parametrize("mode", [0, 2])
def test_gemm_fp8_row_shards(hip, mode):
    m, k, n = 700, 3072, 768
    xq, sc = hip.fp8_quant_rows(dev(seeded((m, k), 36)))
    wide = torch.zeros((m, k + 128), dtype=torch.uint8, device="cuda")
    wide[:, 64:64 + k] = xq.view(torch.uint8)
    wide = wide.view(torch.float8_e4m3fn)
    w8, b = dev(seeded((n, k), 37, scale=k ** -0.5)).to(torch.float8_e4m3fn), dev(seeded((n,), 38, scale=0.2))
    c, table = dev(seeded((m, n), 39)), dev(seeded((2, 6, n), 40))

    def run(lo, hi, first, a=xq):
        return hip.gemm_fp8(a[lo:hi], sc[lo:hi], w8, b, workspace=False, **_gemm_kwargs(hip, mode, c, table, lo, hi, first))
    assert_shards(run, m, 300, gemm_shards(m), f"gemm_fp8 mode {mode}")
    assert_same_rows(run(257, m, 43, wide[:, 64:64 + k]), run(0, m, 300), 257, m, f"gemm_fp8 mode {mode}, strided A")


@gpu
def test_gemm_ksplit_row_shards(hip):
    """With the default workspace the plan depends on M (which tiles are left over and cut into k-range pieces), so a shard and the full
    call are two plans of the same product: the criterion test_gemm_epilogue_ksplit uses between two plans, 1 bf16 ulp and <= 2 % of the
    elements different at all."""
    m, k, n = 600, 14336, 3072
    x, w, b = dev(seeded((m, k), 141, scale=0.5)), dev(seeded((n, k), 142, scale=0.02)), dev(seeded((n,), 143, scale=0.2))
    full = hip.gemm_epilogue(x, w, b)
    assert not torch.equal(full, hip.gemm_epilogue(x, w, b, workspace=False)), "the k-split path did not run"
    for lo, hi in gemm_shards(m):
        assert_close_bf16(hip.gemm_epilogue(x[lo:hi], w, b), full[lo:hi], 1.0, f"k-split gemm, shard [{lo}, {hi})", max_mismatch=0.02)


@gpu
@pytest.mark.parametrize("groups", [3, 1])
@pytest.mark.parametrize("mode", ["write", "add", "gate", "gelu_tanh"])
def test_lora_apply_row_shards(hip, groups, mode):
    m, k, ng, r = 700, 512, 256, 32
    n = groups * ng
    xw, ow = dev(seeded((m, k + 16), 51)), dev(seeded((m, n + 16), 52))
    x, out0 = xw[:, 8:8 + k].contiguous(), ow[:, 8:8 + n].contiguous()
    a, b = dev(seeded((groups * r, k), 53, scale=k ** -0.5)), dev(seeded((n, r), 54, scale=r ** -0.5))
    table = dev(seeded((2, 6, n), 55))

    def run(lo, hi, first, strided=False):
        xs, out = (xw[lo:hi, 8:8 + k], ow.clone()[lo:hi, 8:8 + n]) if strided else (x[lo:hi], out0[lo:hi].clone())
        hip.lora_apply(xs, a, b, out, groups=groups, mode=mode, mod=hip.ModTable(table, first) if mode == "gate" else None, gate_idx=2)
        return out.contiguous()
    assert_shards(run, m, 300, gemm_shards(m), f"lora_apply G={groups} mode={mode}")
    assert_same_rows(run(257, m, 43, strided=True), run(0, m, 300), 257, m, f"lora_apply G={groups} mode={mode}, strided x and out")


# ------------------------------------------------------------------------------------------------------------------ attention
ATTN_SHARDS = [(0, 256), (256, 700), (300, 556), (13, 269), (699, 700)]


@gpu
@pytest.mark.parametrize("name,nkv,form", [("short-kv", 512, "plain"), ("w4", 1500, "plain"), ("w4-pow2", 1500, "pow2")])
def test_attention_query_row_shards(hip, name, nkv, form):
    """Query rows [lo, hi) against the full K / V, every q-block one direct workgroup: the bits of the same rows of the full call.  lo = 13
    and 300 put a row into another wave and another 256-row q-block than it has in the full call."""
    nq, heads = 700, 2
    c = heads * 128
    wide = seeded((1, nq, c + 128), 61, scale=0.25)
    q, k, v = wide[..., 64:64 + c].contiguous(), seeded((1, nkv, c), 62), seeded((1, nkv, c), 63)
    scale = None if form == "plain" else hip.pow2_softmax_scale(128)[0]
    # the condition under which no wave takes the deferred rescale (module docstring): the scaled base-2 logits stay within +-3
    s2 = (128 ** -0.5 if scale is None else scale) * math.log2(math.e)
    logits = torch.einsum("qhd,khd->hqk", q[0].float().view(nq, heads, 128), k[0].float().view(nkv, heads, 128))
    assert (s2 * logits).abs().max().item() <= 3.0
    dwide, dk, dv = dev(wide), dev(k), dev(v)
    dq = dwide[..., 64:64 + c].contiguous()
    full = _attn(hip, dq, dk, dv, heads, torch.empty_like(dq), scale, ws=False)
    assert torch.isfinite(full.float()).all()
    for lo, hi in ATTN_SHARDS:
        got = _attn(hip, dq[:, lo:hi], dk, dv, heads, torch.empty((1, hi - lo, c), dtype=dq.dtype, device="cuda"), scale, ws=False)
        assert_same_rows(got, full, lo, hi, f"attention {name}")
    got = _attn(hip, dwide[:, 300:556, 64:64 + c], dk, dv, heads, torch.empty((1, 256, c), dtype=dq.dtype, device="cuda"), scale, ws=False)
    assert_same_rows(got, full, 300, 556, f"attention {name}, strided q")


# ------------------------------------------------------------------------------------------------------------------ emulated ranks
class Mailbox:
    """What P LoopbackShards of one process exchange through: one slot per exchange (its kind and running number), filled by every
    rank before any rank reads it, dropped once every rank has read it."""

    def __init__(self, world):
        self.world, self.slots, self.taken, self.completed = world, {}, {}, 0

    def deposit(self, key, rank, item):
        slot = self.slots.setdefault(key, {})
        assert rank not in slot, f"rank {rank} deposited twice for {key}"
        slot[rank] = item

    def collect(self, key):
        """The deposits of all ranks, in rank order."""
        slot = self.slots.get(key, {})
        missing = [r for r in range(self.world) if r not in slot]
        if missing:
            raise RuntimeError(f"exchange {key}: no deposit from rank(s) {missing} (every rank must start an exchange before any waits for it)")
        self.taken[key] = self.taken.get(key, 0) + 1
        if self.taken[key] == self.world:
            del self.slots[key], self.taken[key]
            self.completed += 1
        return [slot[r] for r in range(self.world)]


class LoopbackShard(TokenShard):
    """A TokenShard of rank `rank` of `box.world` whose exchanges go through a Mailbox in the same process: no torch.distributed.
    chunk, local_range, heads_local and the send / out buffers are the product's own."""

    def __init__(self, box, rank, attn_mode):
        super().__init__(None, attn_mode)
        self.box, self.world_size, self.rank, self.active = box, box.world, rank, True
        self._count = 0

    def _post(self, kind, item):
        key = (kind, self._count)      # every rank runs the same exchanges in the same order
        self._count += 1
        self.box.deposit(key, self.rank, item)
        return key

    def all_gather_kv_async(self, k, v, n):
        return _LoopKV(self, self._post("kv", (k[0], v[0])), n)

    def ulysses_exchange_async(self, send, n):
        assert send.shape[:3] == (self.world_size, self.chunk(n), 3) and send.is_contiguous()
        return _LoopQKV(self, self._post("qkv", send), n)

    def ulysses_out_async(self, o_full, n, n_local):
        assert o_full.shape[0] == self.world_size * self.chunk(n) and o_full.is_contiguous()
        return _LoopOut(self, self._post("out", o_full), n, n_local)


class _LoopKV:
    def __init__(self, shard, key, n):
        self.shard, self.key, self.n = shard, key, n

    def wait(self):
        items = self.shard.box.collect(self.key)
        assert sum(k.shape[0] for k, _ in items) == self.n
        return tuple(torch.cat([it[j] for it in items])[: self.n].unsqueeze(0) for j in (0, 1))


class _LoopQKV:
    """Receive layout of sequence_parallel._PendingQKV: block p = what rank p sent to this rank, (P * chunk tokens in global order, 3g)."""

    def __init__(self, shard, key, n):
        self.shard, self.key, self.n = shard, key, n

    def wait(self):
        sends = self.shard.box.collect(self.key)
        p, size, _, g = sends[0].shape
        recv = torch.stack([s[self.shard.rank] for s in sends]).view(p * size, 3 * g)
        r = recv[: self.n].unsqueeze(0)
        return r[..., :g], r[..., g:2 * g], r[..., 2 * g:]


class _LoopOut:
    def __init__(self, shard, key, n, n_local):
        self.shard, self.key, self.size, self.n_local = shard, key, shard.chunk(n), n_local

    def wait_blocks(self):
        """-> (P, chunk, g): block p = head group p of this rank's tokens, as sequence_parallel._PendingOut."""
        outs, r = self.shard.box.collect(self.key), self.shard.rank
        return torch.stack([o[r * self.size:(r + 1) * self.size] for o in outs])

    def wait(self):
        return self.wait_blocks()[:, : self.n_local].transpose(0, 1).reshape(1, self.n_local, -1)


@pytest.mark.parametrize("world", [3, 4, 8])
def test_loopback_shard_self_check(world):
    """The test double on random CPU tensors, no model: n = 43 tokens is not divisible by P and leaves the last rank short (13, 10 and 1
    rows).  Gathered K / V = the concatenation; the Ulysses receive layout = the head-group columns of the full q, k, v; the reverse
    exchange returns each rank's rows with all heads; a missing deposit raises."""
    n, heads, d = 43, 24, 8
    c = heads * d
    q, k, o = seeded((1, n, c), 1), seeded((1, n, c), 2), seeded((1, n, c), 4)
    v = seeded((1, n, 3 * c), 3)[..., 2 * c:]      # a strided slice, like the fused qkv buffer
    for mode in ("allgather", "ulysses"):
        box = Mailbox(world)
        shards = [LoopbackShard(box, r, mode) for r in range(world)]
        ranges = [s.local_range(n) for s in shards]
        assert [s.rank for s in shards] == list(range(world)) and all(s.active and s.world_size == world for s in shards)
        assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert 0 < ranges[-1][1] - ranges[-1][0] < ranges[0][1] - ranges[0][0]
        if mode == "allgather":
            pend = [s.all_gather_kv_async(k[:, lo:hi], v[:, lo:hi], n) for s, (lo, hi) in zip(shards, ranges)]
            for p in pend:
                kf, vf = p.wait()
                assert kf.shape == k.shape and torch.equal(kf, k) and torch.equal(vf, v)
            assert box.completed == 1 and not box.slots
            continue
        g = c // world
        pend = []
        for s, (lo, hi) in zip(shards, ranges):      # the send layout sequence_parallel.ulysses_qkv_async fills
            send = s.ulysses_send_buffer(n, c, q, hi - lo)
            for j, t in enumerate((q, k, v)):
                send[:, :hi - lo, j].copy_(t[0, lo:hi].unflatten(-1, (world, g)).transpose(0, 1))
            pend.append(s.ulysses_exchange_async(send, n))
        back = []
        for s, p in zip(shards, pend):
            qg, kg, vg = p.wait()
            cols = slice(s.rank * g, (s.rank + 1) * g)
            assert qg.shape == (1, n, g) and qg.stride(1) == 3 * g
            assert torch.equal(qg, q[..., cols]) and torch.equal(kg, k[..., cols]) and torch.equal(vg, v[..., cols])
            o_full = s.ulysses_out_buffer(n, g, q)
            o_full[:n] = o[0, :, cols]
            back.append(o_full)
        pend = [s.ulysses_out_async(b, n, hi - lo) for s, b, (lo, hi) in zip(shards, back, ranges)]
        for s, p, (lo, hi) in zip(shards, pend, ranges):
            assert torch.equal(p.wait(), o[:, lo:hi])
        assert box.completed == 2 and not box.slots
        with pytest.raises(RuntimeError, match="no deposit"):      # read a second time: the slot is gone, nothing stale is returned
            pend[0].wait()
    box = Mailbox(world)
    shards = [LoopbackShard(box, r, "allgather") for r in range(world)]
    pend = [s.all_gather_kv_async(k[:, lo:hi], v[:, lo:hi], n) for s, (lo, hi) in list(zip(shards, [s.local_range(n) for s in shards]))[:-1]]
    with pytest.raises(RuntimeError, match=f"no deposit from rank\\(s\\) \\[{world - 1}\\]"):
        pend[0].wait()


def run_emulated_ranks(dit, world, attn_mode, **call):
    """P generators of the sharded forward, one per emulated rank, advanced in turns: every rank has started (deposited) an exchange
    before any rank waits for it.  Returns the prediction assembled from the ranks' head outputs, and the mailbox."""
    from fairygen_amd.wan_video import model_fn_wan_video_steps, run_interleaved
    box = Mailbox(world)
    shards = [LoopbackShard(box, r, attn_mode) for r in range(world)]
    gens = [model_fn_wan_video_steps(dit, sequence_shard=s, gather_output=False, **call) for s in shards]
    results = run_interleaved(gens)
    grid = results[0][1]
    n = grid[0] * grid[1] * grid[2]
    for s, (out, g) in zip(shards, results):
        lo, hi = s.local_range(n)
        assert g == grid and out.shape[:2] == (1, hi - lo), (s.rank, out.shape, (lo, hi))
    return dit.unpatchify(torch.cat([out for out, _ in results], dim=1), grid), box


@pytest.fixture(scope="module")
def medium():
    """The dim-3072, 2-layer model of test_medium_dit_block_stack_vs_oracle on a (5, 15, 26) grid: N = 1950 tokens, first_rows = 390,
    TI2V mode, t = 500.  The oracle in bf16 and fp32 (once), and the unsharded HIP forward per model setting (once each)."""
    from fairygen_amd.wan_video import model_fn_wan_video
    from fairygen_amd.wan_video_dit import WanModel
    cfg = dict(synthetic.TINY_DIT_KWARGS, dim=3072, num_heads=24, ffn_dim=1024, text_dim=256, num_layers=2)
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=99)
    dit = WanModel(**cfg)
    dit.load_state_dict(sd)
    dit = dit.to(device="cuda", dtype=torch.bfloat16).eval()
    lat, ctx, ts = seeded((1, 48, 5, 30, 52), 5), seeded((1, 24, 256), 6), torch.tensor([500.0]).to(torch.bfloat16)
    ref16 = wan_dit.model_fn(sd, cfg, lat, ts, ctx, True)
    ref32 = wan_dit.model_fn({k: v.float() for k, v in sd.items()}, cfg, lat.float(), ts.float(), ctx.float(), True)
    call = dict(latents=lat.cuda(), timestep=ts, context=ctx.cuda(), fuse_vae_embedding_in_latents=True)
    unsharded = {}

    def setting(fp8, fold):
        if (dit.fp8_dtype is not None) != fp8:
            dit.enable_fp8_linear(torch.float8_e4m3fn if fp8 else None)
        dit.fold_attn_scale = fold

    def whole(fp8, fold):
        if (fp8, fold) not in unsharded:
            setting(fp8, fold)
            with torch.no_grad():
                unsharded[fp8, fold] = model_fn_wan_video(dit, **call).float().cpu()
        return unsharded[fp8, fold]
    yield types.SimpleNamespace(dit=dit, call=call, ref32=ref32, err_ref=(ref16.float() - ref32).abs().max().item(), whole=whole, setting=setting)
    setting(False, True)


EMULATED = [(mode, world, False, True) for mode in ("allgather", "ulysses") for world in (3, 4, 8)] + [
    ("allgather", 4, True, True),        # the fp8 Linear mode
    ("ulysses", 4, False, False)]        # fold_attn_scale off: the plain 4-wave body, 1 / sqrt(d) as the scale


@gpu
@pytest.mark.parametrize("attn_mode,world,fp8,fold", EMULATED,
                         ids=[f"{m}-P{w}" + ("-fp8" if f8 else "") + ("" if fo else "-nofold") for m, w, f8, fo in EMULATED])
def test_emulated_ranks_equal_unsharded_forward(medium, attn_mode, world, fp8, fold):
    """P ranks in one process against the unsharded forward.  N = 1950, first_rows = 390: with P = 3 (650 rows each) and P = 4 (488, the
    last rank 486) rank 0 straddles the first frame; with P = 8 (244, the last rank 242) rank 0 lies inside it and rank 1 straddles.

    Yardstick err_ref = max|oracle bf16 - oracle fp32|; the emulated output must be within 2 * err_ref + 1e-2 of the fp32 oracle (the
    unsharded test's own bound) and within the same bound of the unsharded HIP output (both are valid bf16 evaluations, apart in the
    k-split and split-KV grouping only).  The fp8 case is held against the unsharded fp8 forward only, with the bf16 oracle's err_ref.

    Measured on an MI355X: err_ref = 0.03223, bound 0.07446 (max|oracle fp32| = 5.44, max|unsharded - oracle fp32| = 0.03394).
    max|emulated - unsharded| = 0.03125 (one bf16 ulp of a value in [4, 8)) in every bf16 case, both modes, P = 3, 4, 8 and with the fold
    off; max|emulated - oracle fp32| = 0.03510 / 0.03247 / 0.03394 (allgather P = 3 / 4 / 8), 0.03510 / 0.03347 / 0.03394 (ulysses),
    0.03412 (ulysses P = 4, fold off).  fp8, allgather P = 4: max|emulated - unsharded fp8| = 0.06793 (a one-ulp flip that crosses an
    e4m3 rounding boundary of a later Linear's input is 2^-4 of that element).  The bound is not tightened to these figures: the
    bit-exact kernel checks above carry the discriminating power."""
    want = medium.whole(fp8, fold)
    medium.setting(fp8, fold)
    with torch.no_grad():
        out, box = run_emulated_ranks(medium.dit, world, attn_mode, **medium.call)
    out = out.float().cpu()
    layers = len(medium.dit.blocks)
    assert box.completed == layers * (1 if attn_mode == "allgather" else 2) and not box.slots, "not every exchange of every block ran"
    bound = 2 * medium.err_ref + 1e-2
    d_hip, d_ref = (out - want).abs().max().item(), (out - medium.ref32).abs().max().item()
    print(f"emulated {attn_mode} P={world} fp8={fp8} fold={fold}: max|emulated - unsharded| = {d_hip:.5f}, max|emulated - oracle fp32| = {d_ref:.5f}, "
          f"max|unsharded - oracle fp32| = {(want - medium.ref32).abs().max().item():.5f}, err_ref = {medium.err_ref:.5f}, bound = {bound:.5f}")
    assert torch.isfinite(out).all() and out.shape == medium.ref32.shape
    assert d_hip <= bound, f"emulated ranks differ from the unsharded HIP forward by {d_hip} (bound {bound}, err_ref {medium.err_ref})"
    if not fp8:
        assert d_ref <= bound, f"emulated ranks differ from the fp32 oracle by {d_ref} (bound {bound}, err_ref {medium.err_ref})"

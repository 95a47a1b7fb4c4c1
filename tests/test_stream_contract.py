"""The stream contract of the C ABI (include/fairygen_hip.h): an entry point does nothing but enqueue work on the stream it is given — no
allocation, no host synchronisation, no blocking copy, no launch on another stream, nothing that is special about the first call of a
process — so a host may call it on any stream and capture it into a graph.

The older tests launch everything on the default stream and then synchronise, where a kernel on the wrong stream is ordered anyway and a
hidden synchronisation costs nothing; only the persistent GEMM was ever captured (test_gemm_sched_state.py).  Here:

  1. CASES: one call through a fairygen_amd.hip wrapper per case, with its inputs built from a seed on the CPU, the buffers it reads and
     writes, and the fg_* names it is declared to reach.  test_case_table_covers_the_abi (no GPU) holds the union of those names equal to
     the entry points of hip._SIGNATURES less the two GEMM forms without a block — the documented exception — and less ELSEWHERE, the
     ones whose stream and capture checks have a named home in another module (the host queries are hip._QUERIES); on the GPU every
     case must launch exactly what it declares (recorded at hip._call), and the
     cases of a launcher that picks between kernels assert the pick (fg_attn_split_choice, fg_conv_tile_choice, the scratch of a k-split).
  2. test_capture_and_replay: the call is captured on a fresh side stream in the default (strict) capture mode and replayed on two input
     sets; every output, overwritten with a byte sentinel before each replay, must equal the eager call on the default stream.
  3. test_side_stream_ordering: on a side stream, behind a ~1 ms producer: NaN into the inputs, the real inputs, the call, clones of the
     outputs, one host wait at the end.  test_two_streams_keep_their_own_scratch: the cases with scratch (split attention, k-split GEMM)
     on two streams in turns, equal to eager, with distinct scratch tensors per stream in hip's tables.
  4. test_first_launch_of_a_process_inside_a_capture: a child process (stream_contract_child.py) whose FIRST use of the entry points with
     per-process setup (hipFuncSetAttribute statics, device / CU caches, getenv statics) is inside a capture.
  5. test_tiny_dit_forward_capture: WanModel.forward_tokens of the tiny DiT of test_dit_launch_plan.py in six modes, captured after one
     eager warm-up (rope tables, weight copies and adapter packs are built there) and replayed on fresh tokens, context and time rows.

The comparator everywhere is the same call, eager, on the default stream, and the comparison is exact (bytes): the property is independence
from the stream; the arithmetic of these shapes is pinned by test_hip_kernels.py, test_buffer_contract.py and test_exact_arithmetic.py.
tea_cache, cfg_prefix, kv_cache and token shards stay out of 5: they carry host decisions from call to call by design.

Cost: the 143 GPU tests of the module take about 9 s of pytest time on an MI355X — the child process 2.6 s, the first model case 2 s (it
builds the tiny weights), every other case at most 0.3 s; the CPU inputs of all 66 cases are built in 1.4 s.
A capture that aborts leaves torch's capture state behind: the tests that follow it in the same process then fail as well, so the first
failure of a run is the one to read.
"""
import contextlib
import functools
import os
import subprocess
import sys

import pytest
import torch

from conftest import seeded
from fairygen_amd import hip as _hip
from test_buffer_contract import _split_choice
from test_dit_launch_plan import CASES as DIT_CASES
from test_dit_launch_plan import built_model
from test_hip_kernels import hip  # noqa: F401  (the module fixture)

gpu = pytest.mark.gpu
BF16, F8, F32, F64 = torch.bfloat16, torch.float8_e4m3fn, torch.float32, torch.float64
SENTINEL = 0xA5
SEEDS = (9100, 9200)
EPS = 1e-6
RESET = "fg_gemm_sched_reset"
# the two GEMM forms whose first call per stream allocates and synchronises: the header's documented exception (the host queries,
# hip._QUERIES, launch nothing)
LEGACY_GEMMS = {"fg_gemm_epilogue_bf16", "fg_gemm_fp8_bf16"}
# entry point -> "file::test" that holds its stream and capture checks, for the ones that have no case here
ELSEWHERE = {
    "fg_cfg_euler_dev_bf16": "test_graph_step.py::test_cfg_euler_dev_capture_and_replay",
    "fg_attn_quant_qk_bf16": "test_attention_qk8.py::test_entry_points_only_enqueue_and_capture",
    "fg_attn_fwd_qk8_bf16": "test_attention_qk8.py::test_entry_points_only_enqueue_and_capture",
    "fg_rmsnorm_rope_q8_bf16": "test_attention_qk8_fused.py::test_entry_points_only_enqueue_and_capture",
    "fg_rmsnorm_rope_kstats_bf16": "test_attention_qk8_fused.py::test_entry_points_only_enqueue_and_capture",
    "fg_attn_quant_k_bf16": "test_attention_qk8_fused.py::test_entry_points_only_enqueue_and_capture",
}
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_contract_child.py")


class Case:
    """One call.  build(seed) -> {name: CPU tensor}; `inputs`: the keys the call reads (in-place operands included), `inplace`: those of
    them it also writes, `outs`: caller-allocated buffers it only writes; run(hip, t, **kw) -> the output tensors (t[...] for in-place and
    caller-allocated ones, else what the wrapper allocated); derive(hip, t): device-made inputs (packed conv weights), eager;
    check(hip, t): the kernel choice; scratch: "attn" / "gemm" for the cases that use per-stream scratch."""

    def __init__(self, name, reaches, build, run, inputs, inplace=(), outs=(), derive=None, check=None, scratch=None):
        self.name, self.reaches, self.build, self.run = name, frozenset(reaches), build, run
        self.inputs, self.inplace, self.outs = tuple(inputs), tuple(inplace), tuple(outs)
        self.derive, self.check, self.scratch = derive, check, scratch
        assert set(self.inplace) <= set(self.inputs) and not set(self.outs) & set(self.inputs), name


# ------------------------------------------------------------------------------------------------------------------ the case table
def _row_cases():
    rows, c = 13, 520
    cs = []

    def xy(seed):
        return {"x": seeded((1, rows, c), seed), "y": seeded((1, rows, c), seed + 1), "table": seeded((2, 6, c), seed + 2, scale=0.5),
                "w": (1 + 0.1 * seeded((c,), seed + 3)).to(BF16), "b": (0.1 * seeded((c,), seed + 4)).to(BF16)}

    def mod(t):
        return _hip.ModTable(t["table"], 4)

    def add(name, reaches, run, inputs, inplace=()):
        cs.append(Case(name, reaches, xy, run, inputs, inplace))

    add("ln_modulate", ["fg_ln_modulate_bf16"], lambda h, t, **_: [h.ln_modulate(t["x"], mod(t), 0, 1, EPS)], ["x", "table"])
    add("ln_affine", ["fg_ln_affine_bf16"], lambda h, t, **_: [h.ln_affine(t["x"], t["w"], t["b"], EPS)], ["x", "w", "b"])
    add("ln_modulate_fp8", ["fg_ln_modulate_fp8_bf16"], lambda h, t, **_: list(h.ln_modulate_fp8(t["x"], mod(t), 0, 1, EPS)), ["x", "table"])

    def dual(out):
        return [out[0], *out[1]]
    add("ln_modulate_dual", ["fg_ln_modulate_dual_bf16"], lambda h, t, **_: dual(h.ln_modulate_dual(t["x"], mod(t), 0, 1, EPS)), ["x", "table"])
    add("ln_affine_dual", ["fg_ln_affine_dual_bf16"], lambda h, t, **_: dual(h.ln_affine_dual(t["x"], t["w"], t["b"], EPS)), ["x", "w", "b"])
    add("gate_residual-inplace", ["fg_gate_residual_bf16"], lambda h, t, **_: [h.gate_residual(t["x"], t["y"], mod(t), 2, out=t["x"])],
        ["x", "y", "table"], ["x"])
    for fp8 in (False, True):
        for affine in (False, True):
            for gate in (True, False):
                def run(h, t, fp8=fp8, affine=affine, gate=gate, **_):
                    if affine:
                        fn = h.residual_ln_affine_fp8 if fp8 else h.residual_ln_affine
                        x_out, norm = fn(t["x"], t["y"], t["w"], t["b"], EPS, mod(t) if gate else None, 2 if gate else None, x_out=t["x"])
                    else:
                        fn = h.residual_ln_modulate_fp8 if fp8 else h.residual_ln_modulate
                        x_out, norm = fn(t["x"], t["y"], mod(t), 2 if gate else None, 0, 1, EPS, x_out=t["x"])
                    return [x_out, *norm] if fp8 else [x_out, norm]
                inputs = ["x", "y"] + (["w", "b"] if affine else []) + (["table"] if gate or not affine else [])
                add(f"residual_ln{'_fp8' if fp8 else ''}-mode{int(affine)}-{'gate' if gate else 'nogate'}",
                    ["fg_residual_ln_fp8_bf16" if fp8 else "fg_residual_ln_bf16"], run, inputs, ["x"])
    # RMSNorm + RoPE: no table, fp64 tables, the fp32 table; the grouped form (Ulysses send buffer) in both table modes
    heads, groups = 5, 5
    half, g, size = c // heads // 2, c // groups, rows + 3
    ld = g + 8

    def rope(seed):
        return {"x": seeded((1, rows, c), seed), "w": (1 + 0.1 * seeded((c,), seed + 1)).to(BF16), "cos": seeded((rows, half), seed + 2, F64),
                "sin": seeded((rows, half), seed + 3, F64), "cs": seeded((rows, half, 2), seed + 4, F32), "dst": torch.empty(groups * size * ld, dtype=BF16),
                "src": seeded((rows * (c + 16),), seed + 5)}

    def tabs(t, mode):
        return tuple(t[k] for k in tab_keys[mode])
    tab_keys = {"none": [], "f64": ["cos", "sin"], "f32": ["cs"]}
    for mode in ("none", "f64", "f32"):
        cs.append(Case(f"rmsnorm_rope-{mode}", ["fg_rmsnorm_rope_bf16"], rope,
                       lambda h, t, mode=mode, **_: [h.rmsnorm_rope(t["x"], t["w"], heads, EPS, *tabs(t, mode))], ["x", "w"] + tab_keys[mode]))
    for mode in ("f64", "f32"):
        cs.append(Case(f"rmsnorm_rope_grouped-{mode}", ["fg_rmsnorm_rope_grouped_bf16"], rope,
                       lambda h, t, mode=mode, **_: [h.rmsnorm_rope(t["x"], t["w"], heads, EPS, *tabs(t, mode), grouped=(t["dst"], g, size * ld, ld))],
                       ["x", "w"] + tab_keys[mode], outs=["dst"]))
    cs.append(Case("copy_groups", ["fg_copy_groups_bf16"], rope,
                   lambda h, t, **_: [h.copy_groups(t["src"], g, c + 16, t["dst"], size * ld, ld, groups, rows, g)], ["src"], outs=["dst"]))
    # fp8 row quantisation: its two template widths; act 0, act 1, act 1 with the activated bf16 row as a second output (raw: the wrapper passes none)
    for width in (256, 14336):
        def quant(seed, width=width):
            x = seeded((5, width), seed, scale=2.0)
            x[seed // 100 % 5] *= 300.0      # a scale above 1, in another row per seed
            return {"x": x, "q": torch.empty((5, width), dtype=F8), "sc": torch.empty((5, 1), dtype=F32), "ao": torch.empty((5, width), dtype=BF16)}

        def raw(h, t, width=width, **_):
            h._call("fg_fp8_quant_rows_bf16", h._ptr(t["x"]), width, h._ptr(t["q"]), h._ptr(t["sc"]), h._ptr(t["ao"]), 5, width, 1, h.FP8_E4M3FN_MAX,
                    h._stream(t["x"]))
            return [t["q"], t["sc"], t["ao"]]
        cs.append(Case(f"fp8_quant_rows-{width}-act0", ["fg_fp8_quant_rows_bf16"], quant, lambda h, t, **_: list(h.fp8_quant_rows(t["x"])), ["x"]))
        cs.append(Case(f"fp8_quant_rows-{width}-act1", ["fg_fp8_quant_rows_bf16"], quant, lambda h, t, **_: list(h.fp8_quant_rows(t["x"], "gelu_tanh")), ["x"]))
        cs.append(Case(f"fp8_quant_rows-{width}-act_out", ["fg_fp8_quant_rows_bf16"], quant, raw, ["x"], outs=["q", "sc", "ao"]))
    for kind in ("silu", "gelu_tanh"):
        cs.append(Case(f"act-{kind}-inplace", ["fg_act_bf16"], lambda seed: {"x": seeded((5, 1000, 8), seed, scale=3.0)},
                       lambda h, t, kind=kind, **_: [h.activation(t["x"], kind)], ["x"], ["x"]))
    cs.append(Case("cfg_euler-inplace", ["fg_cfg_euler_bf16"], lambda seed: {k: seeded((1, 48, 3, 7, 9), seed + i) for i, k in enumerate(("lat", "posi", "nega"))},
                   lambda h, t, **_: [h.cfg_euler(t["lat"], t["posi"], t["nega"], 5.0, -0.125, out=t["lat"])], ["lat", "posi", "nega"], ["lat"]))
    return cs


GEMM_SMOKE = {"gemm_bf16_s-ksplit": (False, 4200, 512, 4096), "gemm_fp8_s-ksplit": (True, 4200, 1024, 4096)}      # a full round + left-over tiles: k-split (test_gemm_sched_state.py)


def _gemm_cases():
    cs = []
    for name, (fp8, m, k, n) in GEMM_SMOKE.items():
        def build(seed, fp8=fp8, m=m, k=k, n=n):
            d = {"x": seeded((m, k), seed, scale=0.5), "w": seeded((n, k), seed + 1, scale=0.05), "b": seeded((n,), seed + 2, scale=0.2)}
            if fp8:
                d["x"], d["w"], d["sc"] = d["x"].to(F8), d["w"].to(F8), seeded((m, 1), seed + 3, F32).abs() + 0.5
            else:
                d["res"], d["table"] = seeded((m, n), seed + 3), seeded((2, 6, n), seed + 4)
            return d

        def run(h, t, state=None, owned=True, fp8=fp8, **_):
            """bf16: mode 2 in place on the residual stream; fp8: mode 4.  owned: on a caller-owned block + scratch (hip.gemm_state), the
            reset first; else on what hip keeps for the current (device, stream)."""
            kw = {}
            if owned:
                sched, ws = h.gemm_state() if state is None else state
                kw = dict(sched=h.gemm_sched_reset(sched), workspace=ws)
            if fp8:
                return [h.gemm_fp8(t["x"], t["sc"], t["w"], t["b"], act="gelu_tanh", **kw)]
            return [h.gemm_epilogue(t["x"], t["w"], t["b"], out=t["res"], residual=True, mod=h.ModTable(t["table"], 130), gate_idx=2, **kw)]

        def check(h, t, run=run):
            """The shape is a k-split one: the scratch is written (the reduce kernel is the entry point's second launch)."""
            sched, ws = h.gemm_state()
            ws.fill_(0x5A)
            run(h, {k_: v.clone() for k_, v in t.items()}, state=(sched, ws))
            torch.cuda.synchronize()
            assert (ws != 0x5A).any(), "no k-split piece was written: the reduce kernel did not run at this shape"
        cs.append(Case(name, ["fg_gemm_fp8_bf16_s" if fp8 else "fg_gemm_epilogue_bf16_s", RESET], build, run,
                       ["x", "sc", "w", "b"] if fp8 else ["x", "w", "b", "res", "table"], [] if fp8 else ["res"], check=check, scratch="gemm"))
    return cs


# name -> (Nq, Nkv, heads, B, form, workspace, fused qkv, split expected)
ATTN = {
    "attn-short-kv-31x5": (31, 5, 1, 1, "plain", True, False, False),
    "attn-short-kv-300x77": (300, 77, 2, 1, "plain", True, False, False),
    "attn-8wave-direct": (513, 512, 3, 1, "plain", True, False, False),
    "attn-split-combine": (300, 1000, 24, 1, "plain", True, False, True),
    "attn-w4-plain": (300, 1500, 2, 1, "plain", False, False, False),
    "attn-w4-pow2": (300, 1500, 2, 1, "pow2", False, False, False),
    "attn-w4-split": (700, 2700, 24, 1, "pow2", True, False, True),      # test_exact_arithmetic.py::test_attention_gather_w4
    "attn-batch2-fused-qkv": (300, 300, 2, 2, "pow2", True, True, None),
}


def _attn_cases():
    cs = []
    for name, (nq, nkv, heads, b, form, ws, fused, split) in ATTN.items():
        c = heads * 128
        scale = None if form == "plain" else _hip.pow2_softmax_scale(128)[0]

        def build(seed, nq=nq, nkv=nkv, b=b, c=c, fused=fused):
            if fused:
                return {"qkv": seeded((b, nq, 3 * c), seed)}
            return {"q": seeded((b, nq, c), seed), "k": seeded((b, nkv, c), seed + 1), "v": seeded((b, nkv, c), seed + 2)}

        def run(h, t, c=c, heads=heads, scale=scale, ws=ws, fused=fused, **_):
            q, k, v = (t["qkv"][..., :c], t["qkv"][..., c:2 * c], t["qkv"][..., 2 * c:]) if fused else (t["q"], t["k"], t["v"])
            if ws:
                return [h.attention(q, k, v, heads, scale=scale)]
            out = torch.empty(q.shape, dtype=BF16, device=q.device)      # no workspace: every q-block one direct workgroup
            h._call("fg_attn_fwd_bf16", h._ptr(q), q.stride(1), h._ptr(k), k.stride(1), h._ptr(v), v.stride(1), h._ptr(out), q.shape[0], q.shape[1], k.shape[1],
                    heads, 128, 128 ** -0.5 if scale is None else scale, None, 0, h._stream(q))
            return [out]

        def check(h, t, nq=nq, nkv=nkv, heads=heads, b=b, ws=ws, split=split, name=name):
            r, s, _ = _split_choice(h, b, nq, nkv, heads, ws)
            assert split is None or (r > 0 and s > 1) == split, f"{name}: fg_attn_split_choice gives (R, S) = ({r}, {s})"
            assert (nkv > 1024) == ("w4" in name), name      # the launcher's rule between the 8-wave and the 4-wave kernel
        cs.append(Case(name, ["fg_attn_fwd_bf16"], build, run, ["qkv"] if fused else ["q", "k", "v"], check=check, scratch="attn" if split else None))
    return cs


# name -> (kernel, Cin, Cout, kt, ks, T, H, W (output), resample, interleave, residual): rows of test_exact_arithmetic.CONV_CASES
CONV = {
    "conv-128": ("128", 48, 64, 3, 3, 1, 6, 10, 0, False, False),
    "conv-256p": ("256p", 96, 512, 1, 3, 8, 33, 31, 0, False, False),
    "conv-w4-res": ("w4", 64, 512, 3, 3, 8, 33, 31, 0, False, True),
    "conv-upsample-res": ("128", 64, 64, 1, 3, 2, 10, 12, 1, False, True),
    "conv-downsample": ("128", 64, 64, 1, 3, 2, 5, 6, 2, False, False),
    "conv-interleave-res": ("128", 64, 128, 3, 1, 2, 5, 6, 0, True, True),
}


def _conv_cases():
    cs = []
    for name, (kernel, cin, cout, kt, ks, T, H, W, resample, interleave, residual) in CONV.items():
        hin, win = (H // 2, W // 2) if resample == 1 else ((2 * H, 2 * W) if resample == 2 else (H, W))
        oshape = (2 * T, H, W, cout // 2) if interleave else (T, H, W, cout)

        def build(seed, shape=(T + kt - 1, hin, win, cin), wshape=(cout, cin, kt, ks, ks), oshape=oshape, residual=residual):
            d = {"x": seeded(shape, seed), "w": seeded(wshape, seed + 1, scale=(wshape[1] * wshape[2] * wshape[3] * wshape[4]) ** -0.5),
                 "b": seeded((wshape[0],), seed + 2, scale=0.1)}
            if residual:
                d["res"] = seeded(oshape, seed + 3)
            return d

        def derive(h, t):
            t["packed"] = h.conv_pack_weight(t["w"])

        def run(h, t, cout=cout, kt=kt, ks=ks, resample=resample, interleave=interleave, **_):
            return [h.conv3d_cl(t["x"], t["packed"], t["b"], cout, kt, ks, residual=t.get("res"), upsample2x=resample == 1, downsample2x=resample == 2,
                                time_interleave=interleave)]

        def check(h, t, kernel=kernel, cin=cin, cout=cout, T=T, H=H, W=W, interleave=interleave):
            tile = h.load().fg_conv_tile_choice(T, H, W, cout)
            takes_w4 = cin % 64 == 0 and (cout // 2 if interleave else cout) % 256 == 0
            assert (tile, takes_w4 and tile == 256) == {"w4": (256, True), "256p": (256, False), "128": (128, False)}[kernel], (tile, takes_w4)
        cs.append(Case(name, ["fg_conv3d_cl_bf16"], build, run, ["x", "packed", "b"] + (["res"] if residual else []), derive=derive, check=check))
    cs.append(Case("conv_pack_weight", ["fg_conv_pack_weight_bf16"], lambda seed: {"w": seeded((64, 48, 3, 3, 3), seed)},
                   lambda h, t, **_: [h.conv_pack_weight(t["w"])], ["w"]))
    return cs


def _lora_cases():
    cs = []
    m, k, ng = 333, 256, 192
    for groups, rank, mode in ((1, 32, "add"), (3, 32, "add"), (1, 128, "gate"), (3, 128, "gelu_tanh")):
        n = groups * ng

        def build(seed, groups=groups, rank=rank, n=n):
            return {"x": seeded((m, k), seed), "a": seeded((groups * rank, k), seed + 1, scale=k ** -0.5), "b": seeded((n, rank), seed + 2, scale=rank ** -0.5),
                    "out": seeded((m, n), seed + 3), "table": seeded((2, 6, n), seed + 4)}

        def run(h, t, groups=groups, mode=mode, **_):
            return [h.lora_apply(t["x"], t["a"], t["b"], t["out"], groups=groups, mode=mode, mod=h.ModTable(t["table"], 100) if mode == "gate" else None, gate_idx=2)]
        cs.append(Case(f"lora_apply-g{groups}-r{rank}", ["fg_lora_apply_bf16"], build, run, ["x", "a", "b", "out"] + (["table"] if mode == "gate" else []), ["out"]))
    for with_fp8 in (False, True):
        def build(seed):
            return {"w": seeded((192, 320), seed, scale=0.05), "a_t": seeded((320, 32), seed + 1, scale=0.1), "b": seeded((192, 32), seed + 2, scale=0.1),
                    "w8": torch.empty((192, 320), dtype=F8)}

        def run(h, t, with_fp8=with_fp8, **_):
            out = h.lora_fuse(t["w"], t["a_t"], t["b"], 2.0, out_fp8=t["w8"] if with_fp8 else None)
            return [out, t["w8"]] if with_fp8 else [out]
        cs.append(Case(f"lora_fuse{'-fp8' if with_fp8 else ''}", ["fg_lora_fuse_bf16"], build, run, ["w", "a_t", "b"], ["w"], outs=["w8"] if with_fp8 else []))
    return cs


def _vae_text_cases():
    cs = []

    def add(name, reach, build, run, inputs, inplace=()):
        cs.append(Case(name, [reach], build, run, inputs, inplace))

    for c in (32, 1024):      # the 32-lane and the 64-lane instantiation
        add(f"vae_rmsnorm_silu-{c}", "fg_vae_rmsnorm_silu_bf16", lambda seed, c=c: {"x": seeded((17, c), seed, scale=2.0), "g": (1 + 0.1 * seeded((c,), seed + 1)).to(BF16)},
            lambda h, t, **_: [h.vae_rmsnorm_silu(t["x"], t["g"], True)], ["x", "g"])
    add("dupup3d_add", "fg_dupup3d_add_bf16", lambda seed: {"x": seeded((2, 3, 5, 64), seed), "main": seeded((3, 6, 10, 64), seed + 1)},
        lambda h, t, **_: [h.dupup3d_add(t["x"], t["main"], 64, 2, 2, True)], ["x", "main"])
    add("avgdown3d_add", "fg_avgdown3d_add_bf16", lambda seed: {"x": seeded((5, 6, 10, 32), seed), "main": seeded((3, 3, 5, 64), seed + 1)},
        lambda h, t, **_: [h.avgdown3d_add(t["x"], t["main"], 2, 2)], ["x", "main"])
    add("softmax_rows", "fg_softmax_rows_f32_bf16", lambda seed: {"s": seeded((5, 257), seed, F32, scale=20.0)}, lambda h, t, **_: [h.softmax_rows(t["s"], 0.25)], ["s"])

    def stats(seed, shape):
        return {"x": seeded(shape, seed), "mean": seeded((48,), seed + 1, scale=0.3), "inv_std": (1 + 0.2 * seeded((48,), seed + 2)).to(BF16)}
    add("vae_latent_to_cl", "fg_vae_latent_to_cl_bf16", lambda seed: stats(seed, (48, 2, 3, 5)), lambda h, t, **_: [h.vae_latent_to_cl(t["x"], t["mean"], t["inv_std"])],
        ["x", "mean", "inv_std"])
    add("vae_latent_from_cl", "fg_vae_latent_from_cl_bf16", lambda seed: stats(seed, (1, 3, 5, 96)),
        lambda h, t, **_: [h.vae_latent_from_cl(t["x"], t["mean"], t["inv_std"], 48)], ["x", "mean", "inv_std"])
    add("vae_unpatchify-window", "fg_vae_unpatchify_bf16", lambda seed: {"x": seeded((3, 5, 7, 12), seed, scale=0.8), "video": seeded((3, 6, 10, 14), seed + 1)},
        lambda h, t, **_: [h.vae_unpatchify(t["x"], t["video"], 2, True)], ["x", "video"], ["video"])
    add("vae_patchify", "fg_vae_patchify_bf16", lambda seed: {"video": seeded((3, 2, 6, 10), seed, scale=0.5)}, lambda h, t, **_: [h.vae_patchify(t["video"])], ["video"])
    add("video_to_uint8", "fg_video_to_uint8", lambda seed: {"video": seeded((3, 2, 5, 7), seed, scale=0.7)}, lambda h, t, **_: [h.video_to_uint8(t["video"])], ["video"])

    def tiles(seed):
        return {"tile": seeded((3, 5, 6, 8), seed), "values": seeded((3, 5, 10, 14), seed + 1), "weight": (seeded((5, 10, 14), seed + 2).abs() + 0.5).to(BF16)}

    def accumulate(h, t, **_):
        h.vae_tile_accumulate(t["tile"], t["values"], t["weight"], 2, 4, 2, 2, (False, False, True, False))
        return [t["values"], t["weight"]]
    add("vae_tile_accumulate", "fg_vae_tile_accumulate_bf16", tiles, accumulate, ["tile", "values", "weight"], ["values", "weight"])
    add("vae_tile_finalize", "fg_vae_tile_finalize_bf16", tiles, lambda h, t, **_: [h.vae_tile_finalize(t["values"], t["weight"])], ["values", "weight"], ["values"])

    def scores(seed):
        mask = torch.zeros(257, dtype=torch.int32)
        mask[:150 + seed // 100 % 100] = 1
        return {"s": seeded((5, 257), seed, scale=4.0), "bias": seeded((5, 257), seed + 1), "mask": mask}
    add("softmax_bias", "fg_softmax_bias_bf16", scores, lambda h, t, **_: [h.softmax_bias(t["s"], t["bias"], t["mask"])], ["s", "bias", "mask"])
    add("gated_gelu", "fg_gated_gelu_bf16", lambda seed: {"fc1": seeded((5, 1000, 8), seed, scale=2.0), "gate": seeded((5, 1000, 8), seed + 1)},
        lambda h, t, **_: [h.gated_gelu(t["fc1"], t["gate"])], ["fc1", "gate"])
    return cs


CASES = {c.name: c for c in _row_cases() + _gemm_cases() + _attn_cases() + _conv_cases() + _lora_cases() + _vae_text_cases()}
SCRATCH_CASES = [n for n, c in CASES.items() if c.scratch]
# what the child process captures before anything else of the library has run: one case per entry point with per-process launch setup
CHILD_CASES = ["lora_apply-g1-r32", "conv-w4-res", "conv-256p", "attn-w4-plain", "attn-w4-pow2", "attn-8wave-direct", "attn-split-combine",
               "gemm_bf16_s-ksplit", "gemm_fp8_s-ksplit"]


def test_case_table_covers_the_abi():
    """Every launching entry point has a case, or a named test elsewhere: a new one cannot be added without either."""
    declared = set().union(*(c.reaches for c in CASES.values()))
    assert set(ELSEWHERE) <= set(_hip._SIGNATURES)
    launching = set(_hip._SIGNATURES) - LEGACY_GEMMS - set(ELSEWHERE)
    assert declared == launching, f"without a case: {sorted(launching - declared)}; unknown: {sorted(declared - launching)}"
    for name, home in ELSEWHERE.items():
        path, test = home.split("::")
        assert f"\ndef {test}(" in open(os.path.join(os.path.dirname(CHILD), path)).read(), f"{name}: {home} does not exist"
    assert not declared & set(_hip._QUERIES)
    assert set(CHILD_CASES) <= set(CASES) and set(SCRATCH_CASES) == {n for n, (*_, split) in ATTN.items() if split} | set(GEMM_SMOKE)
    assert os.path.exists(CHILD) and not os.path.basename(CHILD).startswith("test_")


# ------------------------------------------------------------------------------------------------------------------ the harness
@functools.lru_cache(maxsize=None)
def cpu_set(name, seed):
    """The inputs of a case, built once per (case, seed) and never written."""
    return CASES[name].build(seed)


def fill_sentinel(t):
    assert t.is_contiguous()
    t.view(torch.uint8).fill_(SENTINEL)


def poison(t):
    """NaN in every floating type (e4m3: 0x7F), zeros in the integer ones."""
    if t.dtype in (BF16, F32, F64):
        t.fill_(float("nan"))
    else:
        t.view(torch.uint8).fill_(0x7F if t.dtype == F8 else 0)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def device_set(hip, case, seed, derive=True):  # noqa: F811
    """The operands of a case on the device: inputs, caller-allocated outputs (sentinel), derived inputs."""
    t = {k: v.cuda() for k, v in cpu_set(case.name, seed).items()}
    for k in case.outs:
        fill_sentinel(t[k])
    if derive and case.derive is not None:
        case.derive(hip, t)
    return t


def static_like(case, t):
    """Fresh buffers for the operands the call touches."""
    return {k: torch.empty_like(t[k]) for k in case.inputs + case.outs}


def load_static(case, static, t):
    for k in case.outs:
        fill_sentinel(static[k])
    for k in case.inputs:
        static[k].copy_(t[k])


def eager(hip, case, t, names=None):  # noqa: F811
    """The call on the current stream on copies of the operands; returns copies of its outputs.  names: a list that receives the fg_*
    names that went through hip._call."""
    work = {k: v.clone() for k, v in t.items()}
    with pytest.MonkeyPatch.context() as mp:
        if names is not None:
            real = hip._call

            def call(name, *args):
                names.append(name)
                return real(name, *args)
            mp.setattr(hip, "_call", call)
        outs = case.run(hip, work)
    for k in case.inplace + case.outs:
        assert any(o.data_ptr() == work[k].data_ptr() for o in outs), f"{case.name}: operand {k} is declared as written but is not among the outputs"
    return [o.clone() for o in outs]


@contextlib.contextmanager
def scratch_restored(hip):  # noqa: F811
    """Whatever the block makes hip keep per (device, stream) goes again."""
    tables = (hip._attn_workspace, hip._gemm_workspace, hip._gemm_sched)
    before, dirty = [dict(d) for d in tables], set(hip._gemm_sched_dirty)
    try:
        yield
    finally:
        for d, b in zip(tables, before):
            d.clear()
            d.update(b)
        hip._gemm_sched_dirty.clear()
        hip._gemm_sched_dirty.update(dirty)


def assert_outputs(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        if not same(g, w):
            written = bool((g.contiguous().view(torch.uint8) != SENTINEL).any())
            raise AssertionError(f"{what}: output {j} {tuple(g.shape)} {g.dtype} differs from the eager call on the default stream"
                                 + ("" if written else " (nothing was written: it still holds the sentinel)"))


# ------------------------------------------------------------------------------------------------------------------ 2. capture and replay
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_capture_and_replay(hip, name):  # noqa: F811
    case = CASES[name]
    with scratch_restored(hip):
        sets = [device_set(hip, case, seed) for seed in SEEDS]
        names = []
        want = [eager(hip, case, t, names) for t in sets]
        assert set(names) - {RESET} == case.reaches - {RESET}, f"{name} launched {sorted(set(names))}, declared {sorted(case.reaches)}"
        if case.check is not None:
            case.check(hip, sets[0])
        assert any(not same(a, b) for a, b in zip(*want)), f"{name}: both input sets give the same outputs"
        static = static_like(case, sets[0])
        load_static(case, static, sets[0])
        state = hip.gemm_state() if case.scratch == "gemm" else None
        torch.cuda.synchronize()
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):      # the default error mode: a synchronisation, an allocation by the runtime or a blocking copy aborts it
            outs = case.run(hip, static, state=state)
        torch.cuda.synchronize()
        for i in (1, 0):
            for o in outs:
                fill_sentinel(o)
            load_static(case, static, sets[i])
            graph.replay()
            torch.cuda.synchronize()
            assert_outputs(outs, want[i], f"{name}, replay on input set {i + 1}")
        del graph


# ------------------------------------------------------------------------------------------------------------------ 3. side streams
@pytest.fixture(scope="module")
def producer():
    """Operand and result of the ~1 ms kernel that runs in front of the call under test (the result is never read)."""
    a = torch.zeros((8192, 8192), dtype=BF16, device="cuda")
    return a, torch.empty_like(a)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_side_stream_ordering(hip, producer, name):  # noqa: F811
    case = CASES[name]
    with scratch_restored(hip):
        src = device_set(hip, case, SEEDS[0])
        want = eager(hip, case, src)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            static = static_like(case, src)
            for k in case.inputs:
                poison(static[k])
            for k in case.outs:
                fill_sentinel(static[k])
            # what a wrapper allocates for its outputs on this stream comes from blocks that hold the sentinel
            spare = [torch.empty_like(w) for w in want]
            for s in spare:
                fill_sentinel(s)
            del spare, s
            torch.matmul(producer[0], producer[0], out=producer[1])
            for k in case.inputs:
                static[k].copy_(src[k])
            outs = case.run(hip, static)
            got = [o.clone() for o in outs]
        side.synchronize()      # the only host wait
        assert_outputs(got, want, f"{name} on a side stream behind a producer")


@gpu
@pytest.mark.parametrize("name", SCRATCH_CASES)
def test_two_streams_keep_their_own_scratch(hip, name):  # noqa: F811
    """Two streams with operands of their own, the calls issued in turns, three rounds each, on the scratch hip keeps per (device, stream)."""
    case = CASES[name]
    with scratch_restored(hip):
        srcs = [device_set(hip, case, seed) for seed in SEEDS]
        want = [eager(hip, case, t) for t in srcs]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        assert streams[0].cuda_stream != streams[1].cuda_stream
        statics, got = [], [None, None]
        for s, t in zip(streams, srcs):
            with torch.cuda.stream(s):
                statics.append(static_like(case, t))
        for _ in range(3):
            for i, s in enumerate(streams):
                with torch.cuda.stream(s):
                    load_static(case, statics[i], srcs[i])
                    got[i] = [o.clone() for o in case.run(hip, statics[i], owned=False)]
        for s in streams:
            s.synchronize()
        for i in range(2):
            assert_outputs(got[i], want[i], f"{name}, stream {i}")
        device = srcs[0][case.inputs[0]].device
        tables = {"attn": ["_attn_workspace"], "gemm": ["_gemm_workspace", "_gemm_sched"]}[case.scratch]
        for table in tables:
            a, b = (getattr(hip, table).get((device, s.cuda_stream)) for s in streams)
            assert a is not None and b is not None, f"hip.{table} has no entry for one of the streams"
            assert a is not b and a.data_ptr() != b.data_ptr(), f"hip.{table}: the two streams share their scratch"


# ------------------------------------------------------------------------------------------------------------------ 4. first launch in a process
@gpu
def test_first_launch_of_a_process_inside_a_capture():
    """stream_contract_child.py: a fresh process that captures CHILD_CASES before the library has launched anything, replays each graph
    and compares with the eager call.  It stops at its first error."""
    done = subprocess.run([sys.executable, CHILD], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert done.returncode == 0, f"the child exited with {done.returncode}:\n{done.stdout[-6000:]}"
    assert f"{len(CHILD_CASES)} captures equal eager" in done.stdout, done.stdout[-2000:]


# ------------------------------------------------------------------------------------------------------------------ 5. the tiny DiT
MODEL_CASES = ["bf16-all", "bf16-default-gelu-epilogue", "bf16-hip-adapters-own", "fp8", "fp8-hip-adapters", "fp8-hip-ti2v"]


@gpu
@pytest.mark.parametrize("name", MODEL_CASES)
def test_tiny_dit_forward_capture(hip, name):  # noqa: F811
    """WanModel.forward_tokens (2 layers, 48 tokens, 16 context rows) as one captured chain: every fg_* launch, library GEMM and torch op
    of the block stack between the token embedding and the head output."""
    case = DIT_CASES[name]
    rows, first = (2, 16) if case["ti2v"] else (1, 0)
    with scratch_restored(hip), built_model(case) as m, torch.no_grad():
        rope = m.rope_tables(3, 4, 4, torch.device("cuda", torch.cuda.current_device()))

        def args(seed):
            return [seeded((1, 48, m.dim), seed).cuda(), seeded((1, 16, m.dim), seed + 1).cuda(), seeded((rows, 6, m.dim), seed + 2, scale=0.5).cuda(),
                    seeded((rows, m.dim), seed + 3).cuda()]

        def forward(a):      # the residual stream is updated in place: x is an in-place operand
            return m.forward_tokens(a[0], a[1], a[2], a[3], first, rope)
        sets = [args(seed) for seed in (9300, 9400, 9500)]
        want = [forward([t.clone() for t in a]).clone() for a in sets]      # the first one is the warm-up: tables, weight copies, adapter packs
        assert torch.isfinite(want[1].float()).all() and not torch.equal(want[1], want[2])
        static = [t.clone() for t in sets[0]]
        torch.cuda.synchronize()
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = forward(static)
        torch.cuda.synchronize()
        for i in (1, 2):
            fill_sentinel(out)
            for s, t in zip(static, sets[i]):
                s.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[i]), f"{name}: replay {i} differs from the eager forward"
        del graph

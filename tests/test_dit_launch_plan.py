"""Which kernels a DiT forward launches, per mode: the ordered trace of one `model_fn_wan_video` call on the tiny DiT (dim 256, ffn 512,
2 layers, 48 tokens) against tests/golden/dit_launch_plan.json.

A trace is the list, in call order, of
  - every `hip._call`: the fg_* name and its integer / float arguments (pointers dropped);
  - every call of the library seams `gemm_bias`, `gemm_bias_gelu`, `gemm_bias_tuned` of wan_video_dit (operand shapes);
  - every `torch._scaled_mm` (operand shapes);
  - every `WanModel._hot` (Linear name and shapes).
fg_gemm_sched_reset is left out: it runs once per (device, stream) of the process, so whether it shows depends on what ran before.

The fixture was recorded from the commit before the block forward was rewritten around one activation type and two Linear primitives
(`python tests/test_dit_launch_plan.py --record` on the MI355X) and pins that the rewrite launches what the five mode forks launched.
Re-record it only for a change that is meant to move a launch."""
import contextlib
import functools
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN, seeded
from fairygen_amd import hip, synthetic
from fairygen_amd import wan_video_dit as dit_module

FIXTURE = os.path.join(GOLDEN, "dit_launch_plan.json")
WIDE = "blocks.0.self_attn.o"


def _case(**kw):
    return dict(dict(fp8=False, backend="all", min_tiles=None, gelu_epilogue=True, fold=True, fp8_gemm="own", lora=None, hot=None,
                     ti2v=False, variant="single"), **kw)


_OWN = dict(min_tiles=1)                                # bf16 on the own GEMM at tiny width
_HIP8 = dict(fp8=True, lora="all", hot="hip")           # fp8 Linears + adapters on the HIP backend
CASES = {
    "bf16-all": _case(**_OWN),
    "bf16-fused": _case(backend="fused", **_OWN),
    "bf16-fused-ffn2": _case(backend="fused-ffn2", **_OWN),
    "bf16-lib": _case(backend="lib", **_OWN),
    "bf16-default-gelu-epilogue": _case(),
    "bf16-default-gelu-separate": _case(gelu_epilogue=False),
    "bf16-torch-adapters": _case(lora="all", hot="torch"),
    "bf16-torch-adapters-own": _case(lora="all", hot="torch", **_OWN),
    "bf16-hip-adapters-own": _case(lora="all", hot="hip", **_OWN),
    "bf16-hip-adapters-default": _case(lora="all", hot="hip"),
    "bf16-hip-adapters-fused-ffn2": _case(lora="all", hot="hip", backend="fused-ffn2", **_OWN),
    "bf16-hip-rank160": _case(lora="five", hot="hip", **_OWN),
    "bf16-hip-only-ffn0": _case(lora="blocks.1.ffn.0", hot="hip", **_OWN),
    "bf16-hip-only-ffn2": _case(lora="blocks.1.ffn.2", hot="hip", **_OWN),
    "fp8": _case(fp8=True),
    "fp8-nofold": _case(fp8=True, fold=False),
    "fp8-lib-gemm": _case(fp8=True, fp8_gemm="lib"),
    "fp8-torch-adapters": _case(fp8=True, lora="all", hot="torch"),
    "fp8-hip-adapters": _case(**_HIP8),
    "fp8-hip-adapters-lib-gemm": _case(fp8_gemm="lib", **_HIP8),
    "fp8-hip-rank160": _case(fp8=True, lora="five", hot="hip"),
    "fp8-hip-only-ffn0": _case(fp8=True, lora="blocks.1.ffn.0", hot="hip"),
    "fp8-hip-only-ffn2": _case(fp8=True, lora="blocks.1.ffn.2", hot="hip"),
    "bf16-own-ti2v": _case(ti2v=True, **_OWN),
    "bf16-own-kv-cache": _case(variant="kv_cache", **_OWN),
    "bf16-own-cfg-prefix": _case(variant="cfg_prefix", **_OWN),
    "fp8-hip-ti2v": _case(ti2v=True, **_HIP8),
    "fp8-hip-kv-cache": _case(variant="kv_cache", **_HIP8),
    "fp8-hip-cfg-prefix": _case(variant="cfg_prefix", **_HIP8),
}


@functools.lru_cache(maxsize=None)
def _tiny():
    """The setup of tests/test_fp8_hot_lora.py::_tiny_setup: weights, adapters and inputs, made once."""
    cfg = synthetic.TINY_DIT_KWARGS
    shapes = synthetic.dit_shapes(cfg)
    full = synthetic.random_lora(shapes, rank=32, seed=4321)

    def only(lora, name):
        return {k: v for k, v in lora.items() if k.startswith(name + ".")}
    loras = {"all": [(full, 2.0)],
             # five rank-32 adapters on one Linear: stacked rank 160 > 128, so its pack is False
             "five": [(synthetic.random_lora(shapes, rank=32, seed=200), 1.0)] +
                     [(only(synthetic.random_lora(shapes, rank=32, seed=201 + j), WIDE), 0.5 + 0.25 * j) for j in range(4)],
             "blocks.1.ffn.0": [(only(full, "blocks.1.ffn.0"), 2.0)], "blocks.1.ffn.2": [(only(full, "blocks.1.ffn.2"), 2.0)]}
    ctx, ctx2 = seeded((1, 16, 128), 2), seeded((1, 16, 128), 3)
    ctx[:, 10:] = 0
    inputs = dict(lat=seeded((1, 48, 3, 8, 8), 1).cuda(), ts=torch.tensor([995.9]).to(torch.bfloat16), ctx=ctx.cuda(), ctx2=ctx2.cuda())
    return cfg, synthetic.random_state_dict(shapes, seed=1234), loras, inputs


def _ev(name, *args):
    return " ".join([name] + [repr(a) for a in args])


@contextlib.contextmanager
def _recording(wd, trace):
    """Put the recorders around hip._call, the library seams of `wd`, torch._scaled_mm and wd.WanModel._hot."""
    with pytest.MonkeyPatch.context() as mp:
        real_call = hip._call

        def call(name, *args):
            if name != "fg_gemm_sched_reset":
                trace.append(_ev(name, *[a for a in args if isinstance(a, (int, float))]))
            return real_call(name, *args)
        mp.setattr(hip, "_call", call)

        def seam(name):
            real = getattr(wd, name)

            def fn(x, weight, bias):
                trace.append(_ev(name, tuple(x.shape), tuple(weight.shape)))
                return real(x, weight, bias)
            mp.setattr(wd, name, fn)
        for name in ("gemm_bias", "gemm_bias_gelu", "gemm_bias_tuned"):
            seam(name)
        real_mm = torch._scaled_mm

        def scaled_mm(a, b, *args, **kw):
            trace.append(_ev("torch._scaled_mm", tuple(a.shape), tuple(b.shape)))
            return real_mm(a, b, *args, **kw)
        mp.setattr(torch, "_scaled_mm", scaled_mm)
        real_hot = wd.WanModel._hot

        def hot(self, name, x, out):
            trace.append(_ev("_hot", name, tuple(x.shape), tuple(out.shape)))
            return real_hot(self, name, x, out)
        mp.setattr(wd.WanModel, "_hot", hot)
        yield


@contextlib.contextmanager
def built_model(case, wd=dit_module):
    """The tiny WanModel of module `wd` in the mode of `case` (weights, fp8 Linears, adapters), on the GPU; the module switches of the case
    hold inside the block."""
    from fairygen_amd.wan_video import WanVideoPipeline
    cfg, sd, loras, _ = _tiny()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(wd, "GEMM_BACKEND", case["backend"])
        mp.setattr(wd, "FP8_FOLD", case["fold"])
        mp.setattr(wd, "FP8_GEMM", case["fp8_gemm"])
        if case["min_tiles"] is not None:
            mp.setattr(wd, "GEMM_MIN_TILES", case["min_tiles"])
        m = wd.WanModel(**cfg)
        m.load_state_dict(sd)
        pipe = WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
        pipe.dit = m.to(device="cuda", dtype=torch.bfloat16).eval()
        m.gelu_epilogue = case["gelu_epilogue"]
        if case["fp8"]:
            m.enable_fp8_linear()
        for lo, alpha in loras.get(case["lora"], ()):
            pipe.load_lora(m, state_dict=lo, alpha=alpha, hotload=True, hot_backend=case["hot"])
        yield m


def run_case(case, wd=dit_module):
    """(trace, outputs) of one case on the WanModel of module `wd`."""
    from fairygen_amd.wan_video import model_fn_wan_video
    inp = _tiny()[3]
    with built_model(case, wd) as m:
        # the TI2V layout: two time rows, the 16 tokens of the first latent frame on row 0; else one row
        kw = dict(latents=inp["lat"], timestep=inp["ts"], fuse_vae_embedding_in_latents=case["ti2v"])
        if case["variant"] == "kv_cache":        # the second call finds every block's cross-attention K / V
            shared = {}
            calls = [dict(kw, context=inp["ctx"], kv_cache=shared)] * 2
        elif case["variant"] == "cfg_prefix":    # the first forward leaves block 0's self-attention half, the second takes it
            shared = {}
            calls = [dict(kw, context=inp["ctx"], cfg_prefix=shared), dict(kw, context=inp["ctx2"], cfg_prefix=shared)]
        else:
            calls = [dict(kw, context=inp["ctx"])]
        trace, outs = [], []
        with torch.no_grad(), _recording(wd, trace):
            for j, call in enumerate(calls):
                trace.append(f"forward {j}")
                outs.append(model_fn_wan_video(m, **call))
        torch.cuda.synchronize()
    return trace, outs


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_every_case():
    assert sorted(_fixture()) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_plan(name):
    trace, outs = run_case(CASES[name])
    assert all(torch.isfinite(o.float()).all() for o in outs)
    want = _fixture()[name]
    first = next((j for j, (a, b) in enumerate(zip(trace, want)) if a != b), min(len(trace), len(want)))
    assert trace == want, f"{name}: first difference at event {first}: got {trace[first:first + 3]}, recorded {want[first:first + 3]}"


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_dit_launch_plan.py --record [path]   (on the GPU; rewrites the fixture)")
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump({name: run_case(case)[0] for name, case in sorted(CASES.items())}, f, indent=0)
        f.write("\n")
    print(f"recorded {len(CASES)} cases to {path}")

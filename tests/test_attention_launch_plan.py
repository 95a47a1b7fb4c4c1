"""Which kernels a DiT forward launches, per attention mode, and what it computes: tests/test_dit_launch_plan.py's trace (every `hip._call`
with its integer / float arguments, the library seams) for the attention modes, which that module leaves off, against
tests/golden/dit_attention_launch_plan.json.

The tiny DiT (dim 256, 2 heads of 128, 2 layers) on the input of tests/test_attention_qk8.py: 1 200 tokens, above QK8_MIN_KV, a context of
16 rows with the tail zeroed, fuse_vae_embedding_in_latents=True (two gate rows).  Next to a case's trace the fixture holds the sha256 of
every output tensor's bytes — for the cases whose outputs two recordings reproduced; None for the others.

The fixture was recorded from the commit before the attention of a forward moved into `_BlockAttention` and the single / batched bodies
of the hip.py wrappers were folded (`python tests/test_attention_launch_plan.py --record A`, then `--record B A` in a second process, on
the MI355X) and pins that the rewrite launches and computes what the mode forks did.  Re-record it only for a change that is meant to
move a launch or a bit."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

import test_dit_launch_plan as plan
from conftest import GOLDEN, seeded
from fairygen_amd import hip
from fairygen_amd import wan_video_dit as wd

FIXTURE = os.path.join(GOLDEN, "dit_attention_launch_plan.json")
LATENT = (1, 48, 3, 40, 40)      # tests/test_attention_qk8.py::LATENT: 3 x 20 x 20 = 1 200 tokens
SHORT = (1, 48, 3, 8, 8)         # 48 tokens: below QK8_MIN_KV


def _case(qk8=None, **kw):
    """qk8: the keywords of enable_qk8_attention (None: the modes off); latent / ctx_rows ("max+1": one more than the e4m3 cross-attention
    takes): the input; variant: one call, two calls on one kv_cache, the merged CFG call of the stacked forward (with and without the
    shared block-0 prefix), or the launches recorded into a GraphedStep."""
    return dict(dict(qk8=qk8, fp8=False, latent=LATENT, ctx_rows=16, variant="single"), **kw)


_PV8 = dict(pv8=True)
_CROSS = dict(pv8=True, cross=True)
_CROSS_S = dict(pv8=True, cross=True, smooth_v_cross=True)
_ALL = dict(pv8=True, smooth_v=True, cross=True, smooth_v_cross=True)
CASES = {
    "off-1200": _case(),
    "qk8-twostep": _case({}),
    "qk8-fused": _case(dict(fused_producer=True)),
    "pv8-twostep": _case(_PV8),
    "pv8-fused": _case(dict(_PV8, fused_producer=True)),
    "pv8s-fused": _case(dict(_PV8, smooth_v=True, fused_producer=True)),
    "cross8": _case(_CROSS),
    "cross8s": _case(_CROSS_S),
    "cross8s-smoothv": _case(_ALL),
    "cross8-kvcache": _case(_CROSS, variant="kv_cache"),
    "cross8s-kvcache": _case(_CROSS_S, variant="kv_cache"),
    "short-48": _case(_CROSS, latent=SHORT),
    "ctx-641": _case(_CROSS, ctx_rows="max+1"),
    "fp8-pv8-cross": _case(dict(_CROSS, fused_producer=True), fp8=True),
    "stacked-prefix": _case(_ALL, variant="stacked"),
    "stacked-noprefix": _case(_ALL, variant="stacked-noprefix"),
    "owned": _case(dict(pv8=True, smooth_v=True, cross=True, fused_producer=True), variant="owned"),
}


class _WhileCapturing(list):
    """A trace that keeps only what is issued while the current stream is being captured."""

    def append(self, ev):
        if torch.cuda.is_current_stream_capturing():
            super().append(ev)


def _context(rows, seed, keep):
    ctx = seeded((1, rows, 128), seed)
    ctx[:, keep:] = 0
    return ctx.cuda()


def run_case(case):
    """(trace, outputs) of one case."""
    from fairygen_amd import wan_video
    cfg, sd, _, _ = plan._tiny()
    m = wd.WanModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(device="cuda", dtype=torch.bfloat16).eval()
    if case["fp8"]:
        m.enable_fp8_linear()
    if case["qk8"] is not None:
        m.enable_qk8_attention(**case["qk8"])
    rows = hip.attention_cross8_max_kv() + 1 if case["ctx_rows"] == "max+1" else case["ctx_rows"]
    lat, ts = seeded(case["latent"], 11).cuda(), torch.tensor([995.9]).to(torch.bfloat16)
    kw = dict(latents=lat, timestep=ts, fuse_vae_embedding_in_latents=True)
    variant = case["variant"]
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        if variant == "owned":      # tests/test_graph_step.py::loop over two steps: step 0 eager, step 1 recorded
            pipe = wan_video.WanVideoPipeline(device="cuda", torch_dtype=torch.bfloat16)
            pipe.dit = m
            pipe.scheduler.set_timesteps(2, denoising_strength=1.0, shift=5.0)
            z0 = seeded(LATENT[:2] + (1,) + LATENT[3:], 14).cuda()
            lat[:, :, 0:1] = z0
            inputs = {"latents": lat, "fuse_vae_embedding_in_latents": True, "first_frame_latents": z0}
            trace = _WhileCapturing()
            with plan._recording(wd, trace):
                outs = [pipe.denoise(inputs, {"context": _context(rows, 12, 10)}, {"context": _context(rows, 13, 12)}, 5.0,
                                     progress_bar_cmd=lambda x: x, graph=True).clone()]
            torch.cuda.synchronize()
            return list(trace), outs
        if variant.startswith("stacked"):      # the merged CFG call of tests/test_stacked_cfg_forward.py::_merged
            m.enable_stacked_cfg()
            mp.setattr(wan_video, "CFG_SHARE_PREFIX", variant == "stacked")
            calls = [dict(kw, context=torch.cat([_context(rows, 12, 10), _context(rows, 13, 12)], 0))]
        elif variant == "kv_cache":      # the second call finds every block's cross-attention operands
            shared = {}
            calls = [dict(kw, context=_context(rows, 12, 10), kv_cache=shared)] * 2
        else:
            calls = [dict(kw, context=_context(rows, 12, 10))]
        trace, outs = [], []
        with plan._recording(wd, trace):
            for j, call in enumerate(calls):
                trace.append(f"forward {j}")
                outs.append(wan_video.model_fn_wan_video(m, **call))
        torch.cuda.synchronize()
    return trace, outs


def digests(outs):
    return [hashlib.sha256(o.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() for o in outs]


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_every_case():
    assert sorted(_fixture()) == sorted(CASES)
    assert all(sorted(rec) == ["sha256", "trace"] and rec["trace"] for rec in _fixture().values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_attention_launch_plan(name):
    trace, outs = run_case(CASES[name])
    assert all(torch.isfinite(o.float()).all() for o in outs)
    want = _fixture()[name]
    first = next((j for j, (a, b) in enumerate(zip(trace, want["trace"])) if a != b), min(len(trace), len(want["trace"])))
    assert trace == want["trace"], \
        f"{name}: first difference at event {first}: got {trace[first:first + 3]}, recorded {want['trace'][first:first + 3]}"
    if want["sha256"] is not None:
        assert digests(outs) == want["sha256"], f"{name}: the outputs are not the recorded bytes"


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) < 3:
        sys.exit("usage: python tests/test_attention_launch_plan.py --record path [earlier recording]   (on the GPU)\n"
                 "with an earlier recording: the traces must equal its traces, and a digest is kept only where both agree")
    earlier = json.load(open(sys.argv[3])) if len(sys.argv) > 3 else None
    out = {}
    for name, case in sorted(CASES.items()):
        trace, outs = run_case(case)
        out[name] = {"trace": trace, "sha256": digests(outs)}
        if earlier is not None:
            assert earlier[name]["trace"] == trace, f"{name}: two recordings of one commit launch differently"
            if earlier[name]["sha256"] != out[name]["sha256"]:
                print(f"{name}: outputs differ between the recordings, no digest kept")
                out[name]["sha256"] = None
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"recorded {len(CASES)} cases to {sys.argv[2]}; digests kept for {sorted(n for n, r in out.items() if r['sha256'] is not None)}")

"""The CFG step three ways over the same denoise loop (WanVideoPipeline.denoise): ms per step, event-timed, legs interleaved in one process.

    python tools/stacked_step.py                                  # N = 8 190 and N = 27 280, bf16 attention and pv8 + cross + fused producers
    python tools/stacked_step.py --sizes n8190 --attn bf16 --layers 4      # a short look
    python tools/stacked_step.py --linear fp8                     # the same legs in the fp8 Linear mode (enable_fp8_linear)

Legs: "two-call" (the default loop: two batch-1 forwards that share block 0's self-attention half), "merged" (cfg_merge=True with the
switch off: the merged call evaluated element by element — the same launches as two-call) and "stacked" (cfg_merge=True with
WanModel.enable_stacked_cfg(): one forward on (2, N, dim)).  Sizes: "n8190" (latent (1,48,13,42,60)) and "headline" (704x1280x121, latent
(1,48,31,44,80), N = 27 280).  Full width, 30 blocks, synthetic weights, TI2V with CFG 5, kv_cache on — the loop the pipeline runs.
--linear fp8: the blocks' Linears in the fp8 mode in all three legs, the stacked leg with enable_stacked_cfg(fp8_linear=True).
--hot-lora hip: rank-32 adapters on self_attn.q / k / v / o, ffn.0 and ffn.2 of every block, unfused on hot_backend="hip" in the three legs
(the stacked one with enable_stacked_cfg(hot_lora=True): fg_lora_apply_bf16_b), and a fourth leg "stacked-fused": the stacked forward with
the same adapters on hot_backend="fused" (folded into the weights before the leg, outside the timed steps) — the price of not fusing.
--periodic-gate: two legs, "stacked" and "stacked-periodic" — the stacked forward as it is, and with enable_stacked_cfg(periodic_gate=True):
the two-row gated stores (self_attn.o, ffn.2) as ONE fg_gemm_*_sp launch on 2 N rows instead of one _s launch per element.  Combines with
--linear fp8 --hot-lora hip (the fp8 form has gated stores only with adapters on the HIP backend).  The cosine is then to "stacked".

A round runs every leg once, in order; `--rounds` rounds follow each other, so a leg's samples are spread over the run and drift hits all
legs alike.  A leg is ONE denoise call of `1 + --warmup + --steps` steps; step 0 (tables, kv_cache) and the warm-up steps are not timed,
every later step lies between two HIP events on the loop's stream, read after one host wait at the end.  Per leg: median and standard
deviation of its step times over all rounds.  "cos_vs_two_call": cosine of the leg's final latents to the two-call leg's of the same form
(merged is bit-equal by construction; stacked is not: its library GEMMs run on 2 N rows).  Prints a line per leg and one JSON line."""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fairygen_amd import hip, synthetic  # noqa: E402
from fairygen_amd.loader import TI2V_5B_DIT_KWARGS  # noqa: E402
from fairygen_amd.wan_video import WanVideoPipeline  # noqa: E402
from fairygen_amd.wan_video_dit import WanModel  # noqa: E402

SIZES = {"n8190": (1, 48, 13, 42, 60), "headline": (1, 48, 31, 44, 80)}
LEGS = ("two-call", "merged", "stacked")
HOT_LEGS = LEGS + ("stacked-fused",)
PERIODIC_LEGS = ("stacked", "stacked-periodic")
HOT_TARGETS = ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "ffn.0", "ffn.2")


def hot_adapters(dit, rank, dev):
    """[(name, A (rank, in), B (out, rank))] for HOT_TARGETS of every block, x A^T B^T of O(0.1)."""
    g = torch.Generator("cpu").manual_seed(4321)
    out = []
    for i in range(len(dit.blocks)):
        for nm in HOT_TARGETS:
            n, k = dit.get_submodule(f"blocks.{i}.{nm}").weight.shape
            out.append((f"blocks.{i}.{nm}", (torch.randn((rank, k), generator=g) * k ** -0.5).to(torch.bfloat16).to(dev),
                        (torch.randn((n, rank), generator=g) * 0.1 * rank ** -0.5).to(torch.bfloat16).to(dev)))
    return out


def build(layers, dev):
    cfg = dict(TI2V_5B_DIT_KWARGS)
    if layers:
        cfg["num_layers"] = layers
    with torch.device("meta"):
        dit = WanModel(**cfg)
    dit.load_state_dict(synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234, device=dev), assign=True)
    pipe = WanVideoPipeline(device=dev, torch_dtype=torch.bfloat16)
    pipe.dit = dit.to(device=dev, dtype=torch.bfloat16).eval()
    return pipe


class Timed:
    """The loop's progress bar: an event in front of every step from `skip` on, and one behind the last."""

    def __init__(self, skip):
        self.skip, self.events = skip, []

    def mark(self):
        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record()

    def __call__(self, timesteps):
        for i, t in enumerate(timesteps):
            if i >= self.skip:
                self.mark()
            yield t
        self.mark()

    def step_ms(self):
        return [a.elapsed_time(b) for a, b in zip(self.events, self.events[1:])]


def leg(pipe, shape, mode, warmup, steps, dev, fp8=False, adapters=None):
    fused, periodic = mode == "stacked-fused", mode == "stacked-periodic"
    mode = "stacked" if periodic else mode
    if adapters is not None:
        pipe.dit.clear_hot_loras()
        pipe.dit.hot_lora_backend = "fused" if fused else "hip"
        for name, a, b in adapters:
            pipe.dit.add_hot_lora(name, a, b)
        mode = "stacked" if fused else mode
    g = torch.Generator("cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g).to(torch.bfloat16).to(dev)      # noqa: E731
    lat, ctx_p, ctx_n, z0 = rnd(*shape), rnd(1, 512, 4096), rnd(1, 512, 4096), rnd(*shape[:2], 1, *shape[3:])
    lat[:, :, 0:1] = z0
    pipe.scheduler.set_timesteps(1 + warmup + steps, denoising_strength=1.0, shift=5.0)
    shared = {"latents": lat, "fuse_vae_embedding_in_latents": True, "first_frame_latents": z0}
    posi, nega = {"context": ctx_p}, {"context": ctx_n}
    if mode != "two-call":      # what WanVideoUnit_CfgMerger leaves: the contexts batched in the shared inputs
        shared.update(cfg_merge=True, context=torch.cat([ctx_p, ctx_n], 0))
        posi, nega = {}, {}
    pipe.dit.enable_stacked_cfg(mode == "stacked", fp8_linear=fp8, hot_lora=adapters is not None and not fused,
                                periodic_gate=periodic)
    bar = Timed(1 + warmup)
    try:
        with torch.no_grad():
            out = pipe.denoise(shared, posi, nega, 5.0, progress_bar_cmd=bar)
        torch.cuda.synchronize()
    finally:
        pipe.dit.enable_stacked_cfg(False)
        if adapters is not None:
            pipe.dit.clear_hot_loras()
    return bar.step_ms(), out.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="n8190,headline")
    ap.add_argument("--attn", default="bf16,e4m3", help="bf16, and e4m3 = enable_qk8_attention(pv8=True, cross=True, fused_producer=True)")
    ap.add_argument("--legs", default=None, help="default: %s; with --hot-lora: %s" % (",".join(LEGS), ",".join(HOT_LEGS)))
    ap.add_argument("--hot-lora", default=None, choices=("hip",), help="rank-32 unfused adapters on six Linears of every block (hot_backend='hip')")
    ap.add_argument("--periodic-gate", action="store_true", help="legs stacked and stacked-periodic (enable_stacked_cfg(periodic_gate=True))")
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer DiT layers")
    ap.add_argument("--linear", default="bf16", choices=("bf16", "fp8"), help="the blocks' Linears: bf16, or the fp8 Linear mode in every leg")
    a = ap.parse_args()
    hip.load()
    dev = "cuda"
    pipe = build(a.layers, dev)
    fp8 = a.linear == "fp8"
    if fp8:
        pipe.dit.enable_fp8_linear()
    adapters = hot_adapters(pipe.dit, a.rank, dev) if a.hot_lora else None
    a.legs = a.legs or ",".join(PERIODIC_LEGS if a.periodic_gate else HOT_LEGS if adapters else LEGS)
    rows = []
    for size in a.sizes.split(","):
        n = SIZES[size][2] * (SIZES[size][3] // 2) * (SIZES[size][4] // 2)
        for attn in a.attn.split(","):
            e4m3 = attn == "e4m3"
            pipe.dit.enable_qk8_attention(e4m3, fused_producer=e4m3, pv8=e4m3, cross=e4m3)
            samples, outs = {m: [] for m in a.legs.split(",")}, {}
            for _ in range(a.rounds):
                for mode in samples:
                    ms, out = leg(pipe, SIZES[size], mode, a.warmup, a.steps, dev, fp8, adapters)
                    samples[mode] += ms
                    outs[mode] = out
            ref_leg = "two-call" if "two-call" in outs else "stacked" if a.periodic_gate and "stacked" in outs else None
            ref = outs.get(ref_leg)
            for mode, ms in samples.items():
                cos = None if ref is None else torch.nn.functional.cosine_similarity(outs[mode].float().flatten(), ref.float().flatten(), dim=0).item()
                rows.append({"size": size, "tokens": n, "attn": attn, "leg": mode, "median_ms": round(statistics.median(ms), 3),
                             "sd_ms": round(statistics.pstdev(ms), 3), "samples": len(ms), "cos_vs_two_call": cos,
                             **({"cos_is_to": ref_leg} if ref_leg not in (None, "two-call") else {}),
                             "same_bits": None if ref is None else bool(torch.equal(outs[mode], ref))})
                print(f"{size:9s} N={n:6d} {attn:5s} {mode:16s}: median {rows[-1]['median_ms']:9.3f} ms/step, sd {rows[-1]['sd_ms']:7.3f} over {len(ms)} steps "
                      f"in {a.rounds} rounds; cos to {ref_leg} {cos if cos is None else round(cos, 6)}, same bits {rows[-1]['same_bits']}", flush=True)
            pipe.dit.enable_qk8_attention(False)
            del outs, ref
            gc.collect()
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "stacked_step", **({"linear": "fp8"} if fp8 else {}), **({"hot_lora": a.hot_lora, "rank": a.rank} if adapters else {}), "layers": a.layers or 30, "rounds": a.rounds, "warmup": a.warmup, "steps": a.steps,
                      "device": torch.cuda.get_device_name(0), "legs": rows}))


if __name__ == "__main__":
    main()

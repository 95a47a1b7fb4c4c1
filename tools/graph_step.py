"""Eager against graph=True over the same denoise loop (WanVideoPipeline.denoise, wan_video.GraphedStep): ms per step, event-timed.

    python tools/graph_step.py                                   # the four sizes below, bf16 and fp8, eager and graph
    python tools/graph_step.py --sizes config1 --dtypes bf16 --modes eager      # one leg (this form also runs on a tree without graph=)

Sizes: "config1" (256x256x17, latent (1,48,5,16,16), N = 320 tokens), "config2" (480x832x49, N = 5 070), "shard8" (latent (1,48,5,44,62),
N = 3 410 tokens: the row count of one rank of the 8-rank layout of tools/shard_dryrun.py, as an unsharded single-GPU loop — the GEMMs, row
kernels and the launch count of that rank, but self-attention over 3 410 keys where the rank's attends to all 27 280: comm-free, and
cheaper in attention than the real shard) and "headline" (704x1280x121, N = 27 280).  Full width, 30 blocks, synthetic weights, TI2V with
CFG 5, cfg_prefix and kv_cache on — the loop the pipeline runs.

A leg is ONE denoise call of `--warmup + --steps + 1` steps.  Step 0 is never timed (eager in both modes: tables, kv_cache), the next
`--warmup` steps neither (in graph mode the first of them records the graph); the remaining steps lie between two HIP events on the loop's
stream, recorded from the progress-bar iterator the loop already takes, with one host wait at the end.  ms/step = elapsed / steps.  Prints
a line per leg and one JSON line; "same_bits" tells whether the graph leg's latents equal the eager leg's."""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fairygen_amd import hip, synthetic  # noqa: E402
from fairygen_amd.loader import TI2V_5B_DIT_KWARGS  # noqa: E402
from fairygen_amd.wan_video import WanVideoPipeline  # noqa: E402
from fairygen_amd.wan_video_dit import WanModel  # noqa: E402

SIZES = {"config1": (1, 48, 5, 16, 16), "config2": (1, 48, 13, 30, 52), "shard8": (1, 48, 5, 44, 62), "headline": (1, 48, 31, 44, 80)}


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
    """The loop's progress bar: events in front of the first timed step and behind the last one."""

    def __init__(self, skip):
        self.skip, self.start, self.stop = skip, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __call__(self, timesteps):
        for i, t in enumerate(timesteps):
            if i == self.skip:
                self.start.record()
            yield t
        self.stop.record()


def leg(pipe, shape, mode, warmup, steps, dev):
    g = torch.Generator("cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g).to(torch.bfloat16).to(dev)      # noqa: E731
    lat, ctx_p, ctx_n, z0 = rnd(*shape), rnd(1, 512, 4096), rnd(1, 512, 4096), rnd(*shape[:2], 1, *shape[3:])
    lat[:, :, 0:1] = z0
    pipe.scheduler.set_timesteps(1 + warmup + steps, denoising_strength=1.0, shift=5.0)
    shared = {"latents": lat, "fuse_vae_embedding_in_latents": True, "first_frame_latents": z0}
    bar = Timed(1 + warmup)
    with torch.no_grad():
        out = pipe.denoise(shared, {"context": ctx_p}, {"context": ctx_n}, 5.0, progress_bar_cmd=bar, **({"graph": True} if mode == "graph" else {}))
    torch.cuda.synchronize()
    return bar.start.elapsed_time(bar.stop) / steps, out.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="config1,config2,shard8,headline")
    ap.add_argument("--dtypes", default="bf16,fp8")
    ap.add_argument("--modes", default="eager,graph,eager,graph", help="legs per size and dtype, in this order (repeats show the run-to-run spread)")
    ap.add_argument("--attn", default="bf16", help="self-attention forms, legs in this order: bf16, qk8 (enable_qk8_attention(), the two-step "
                    "producers), qk8-fused (fused_producer=True), pv8 and pv8-fused (the same with pv8=True: e4m3 P V too), cross8 and "
                    "cross8-fused (pv8 with cross=True: cross-attention in the e4m3 form too), pv8s and pv8s-fused (pv8 with smooth_v=True: V "
                    "mean-smoothed), cross8s and cross8s-fused (cross8 with smooth_v_cross=True: V of the context mean-smoothed); the latents of a -fused leg are compared with "
                    "the first leg's of its form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer DiT layers")
    a = ap.parse_args()
    if a.steps < 10 and not a.layers:
        ap.error("--steps: at least 10 timed steps")
    hip.load()
    dev = "cuda"
    pipe = build(a.layers, dev)
    rows = []
    for dtype in a.dtypes.split(","):
        pipe.dit.enable_fp8_linear(torch.float8_e4m3fn if dtype == "fp8" else None)
        for size in a.sizes.split(","):
            first = {}
            for attn, mode in ((at, md) for at in a.attn.split(",") for md in a.modes.split(",")):
                pipe.dit.enable_qk8_attention(attn != "bf16", fused_producer=attn.endswith("-fused"), pv8=attn.startswith(("pv8", "cross8")),
                                              cross=attn.startswith("cross8"), smooth_v=attn.split("-")[0] == "pv8s",
                                              smooth_v_cross=attn.split("-")[0] == "cross8s")
                ms, out = leg(pipe, SIZES[size], mode, a.warmup, a.steps, dev)
                ref = first.setdefault(attn.split("-")[0], out)
                n = SIZES[size][2] * (SIZES[size][3] // 2) * (SIZES[size][4] // 2)
                rows.append({"size": size, "tokens": n, "dtype": dtype, "attn": attn, "mode": mode, "ms_per_step": round(ms, 3),
                             "same_bits": bool(torch.equal(out, ref))})
                print(f"{size:9s} N={n:6d} {dtype:4s} {attn:9s} {mode:6s}: {ms:9.3f} ms/step over {a.steps} steps; latents equal the first "
                      f"{attn.split('-')[0]} leg's: {rows[-1]['same_bits']}", flush=True)
                del out
            pipe.dit.enable_qk8_attention(False)
            del first, ref
            gc.collect()
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "graph_step", "layers": a.layers or 30, "warmup": a.warmup, "steps": a.steps, "device": torch.cuda.get_device_name(0), "legs": rows}))


if __name__ == "__main__":
    main()

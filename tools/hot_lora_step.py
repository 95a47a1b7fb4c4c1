"""Time the DiT part of one denoise step (both CFG forwards) of the headline configuration with a rank-32 adapter on every block Linear:
hot-loaded on each backend of WanModel.hot_lora_backend ("fused_hot" is hot_backend="fused": folded into the weights, originals kept), and
fused into the weights for good (the floor).  With --swap N, a "fused_hot" leg also times the per-shot adapter switch of that backend.

    python tools/hot_lora_step.py --steps 3 --order torch,hip,torch,fused
    python tools/hot_lora_step.py --linear-dtype fp8 --steps 3 --order torch,hip,torch,fused      # the same legs in the fp8 Linear mode
    python tools/hot_lora_step.py --steps 3 --swap 5 --order fused,fused_hot,fused,fused_hot      # restorable against permanent fuse, and the swap

Every leg builds the 30-block model from the same seeds, warms up one step and reports the median of `--steps` timed steps (host clock
around a device synchronise).  "torch" is the code path of hotload=True before the backend existed.  Prints one line per leg and a
JSON line at the end.  The swap: clear_lora() + load_lora(hot_backend="fused") of an adapter already on the device over all 300 Linears,
then the derived copies the next forward would build (fused QKV / cross KV weights, e4m3 weights in the fp8 mode), each part closed by a
device synchronise; once with fg_lora_fuse_bf16 and once with the torch ops for every Linear (FAIRYGEN_LORA_FUSE=torch)."""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fairygen_amd import hip, synthetic  # noqa: E402
from fairygen_amd.loader import TI2V_5B_DIT_KWARGS  # noqa: E402
from fairygen_amd.wan_video import WanVideoPipeline, model_fn_wan_video  # noqa: E402
from fairygen_amd.wan_video_dit import WanModel  # noqa: E402


def build(leg, layers, dev, linear_dtype="bf16"):
    cfg = dict(TI2V_5B_DIT_KWARGS)
    if layers:
        cfg["num_layers"] = layers
    shapes = synthetic.dit_shapes(cfg)
    with torch.device("meta"):
        dit = WanModel(**cfg)
    dit.load_state_dict(synthetic.random_state_dict(shapes, seed=1234, device=dev), assign=True)
    pipe = WanVideoPipeline(device=dev, torch_dtype=torch.bfloat16)
    pipe.dit = dit.to(device=dev, dtype=torch.bfloat16).eval()
    if linear_dtype == "fp8":
        pipe.dit.enable_fp8_linear()
    lora = synthetic.random_lora(shapes, rank=32, seed=4321)
    if leg == "fused":
        pipe.load_lora(pipe.dit, state_dict=lora, alpha=1)
    else:
        pipe.load_lora(pipe.dit, state_dict=lora, alpha=1, hotload=True, hot_backend="fused" if leg == "fused_hot" else leg)
    return pipe


def time_swaps(pipe, count, dev):
    """[{path, swap_ms, rebuild_ms}]: medians over `count` switches between two adapters, on the kernel and on the torch-op fallback."""
    shapes = synthetic.dit_shapes(dict(TI2V_5B_DIT_KWARGS, num_layers=len(pipe.dit.blocks)))
    adapters = [{k: v.to(dev) for k, v in synthetic.random_lora(shapes, rank=32, seed=s).items()} for s in (4321, 99)]
    from fairygen_amd import wan_video_dit as wd
    default, rows = wd.LORA_FUSE, []
    try:
        for path in ("kernel", "torch_ops"):
            wd.LORA_FUSE = "hip" if path == "kernel" else "torch"
            swaps, rebuilds = [], []
            for i in range(count + 1):      # the first switch is the warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.clear_lora()
                pipe.load_lora(pipe.dit, state_dict=adapters[i % 2], alpha=1, hotload=True, hot_backend="fused")
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for blk in pipe.dit.blocks:
                    blk.fused_weights()
                    if pipe.dit.fp8_dtype is not None:
                        blk.fp8_weights(pipe.dit.fp8_dtype)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if i:
                    swaps.append(t1 - t0), rebuilds.append(t2 - t1)
            swaps.sort(), rebuilds.sort()
            rows.append({"path": path, "swap_ms": round(swaps[len(swaps) // 2] * 1e3, 2), "rebuild_ms": round(rebuilds[len(rebuilds) // 2] * 1e3, 2)})
            print(f"swap ({path:9s}): clear_lora + load_lora median {rows[-1]['swap_ms']:8.1f} ms, derived copies {rows[-1]['rebuild_ms']:8.1f} ms "
                  f"over {len(pipe.dit._fused_stash)} Linears, {count} switches", flush=True)
    finally:
        wd.LORA_FUSE = default
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer DiT layers")
    ap.add_argument("--height", type=int, default=704)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=121)
    ap.add_argument("--order", default="torch,hip,torch,fused")
    ap.add_argument("--swap", type=int, default=0, help="after the first fused_hot leg: time this many adapter switches per path")
    ap.add_argument("--linear-dtype", choices=("bf16", "fp8"), default="bf16", help="fp8: every leg calls enable_fp8_linear() before the adapters are loaded")
    a = ap.parse_args()
    hip.load()
    dev = "cuda"
    g = torch.Generator("cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g).to(torch.bfloat16).to(dev)      # noqa: E731
    lat = rnd(1, 48, (a.frames - 1) // 4 + 1, a.height // 16, a.width // 16)
    ctx_p, ctx_n = rnd(1, 512, 4096), rnd(1, 512, 4096)
    ts = torch.tensor([900.0]).to(torch.bfloat16)
    results, outs, swaps = [], {}, None
    for leg in a.order.split(","):
        pipe = build(leg, a.layers, dev, a.linear_dtype)

        def step():
            with torch.no_grad():
                p = model_fn_wan_video(pipe.dit, latents=lat, timestep=ts, context=ctx_p, fuse_vae_embedding_in_latents=True)
                n = model_fn_wan_video(pipe.dit, latents=lat, timestep=ts, context=ctx_n, fuse_vae_embedding_in_latents=True)
            return n + 5.0 * (p - n)
        out = step()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        times.sort()
        med = times[len(times) // 2]
        ref = outs.setdefault("first", out.float())
        diff = (out.float() - ref).abs().max().item()
        print(f"{leg:6s}: DiT step (2 CFG forwards) median {med * 1e3:8.1f} ms, min {times[0] * 1e3:8.1f} ms; max|out - first leg's| = {diff:.4f} "
              f"(max|out| = {out.float().abs().max().item():.2f})", flush=True)
        results.append({"leg": leg, "step_ms": round(med * 1e3, 2), "min_ms": round(times[0] * 1e3, 2), "max_abs_diff_vs_first_leg": diff})
        if leg == "fused_hot" and a.swap and swaps is None:
            swaps = time_swaps(pipe, a.swap, dev)
        del pipe, out
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "hot_lora_step", "height": a.height, "width": a.width, "frames": a.frames, "layers": a.layers or 30, "steps": a.steps, "linear_dtype": a.linear_dtype,
                      "legs": results, "swap": swaps}))


if __name__ == "__main__":
    main()

"""Per-rank compute of every multi-GPU layout, measured on ONE GPU: the collectives are replaced by local copies of the
same size (no xGMI), so a step's time is what rank 0 of a P-rank job computes plus its launch overhead — the
communication-free upper bound of the scaling the driver's 8-GPU run can reach, and the place to see which layout
loses how much to small shapes.

    python tools/shard_dryrun.py [--steps 2] [--worlds 2,4,8] [--attention {bf16,qk8,pv8,pv8-cross,full}] [--stacked-cfg [--repeats 5]]

--attention qk8 / pv8: the e4m3 self-attention on the sharded layouts (enable_qk8_attention(sharded=True)), the single-GPU line in the
same mode; the record exchange is a local copy like the others.  pv8-cross: with the e4m3 cross-attention as well; full: that with both
V smoothings (enable_qk8_attention(pv8=True, cross=True, smooth_v=True, smooth_v_cross=True, sharded="all")).

--stacked-cfg (composable with --attention): on the K / V all-gather cfg_parallel=1 layouts only, two legs of the denoise step in ONE
process, run in turns --repeats times each: the two-call leg (the CFG branches as two interleaved batch-1 forwards) and the stacked leg
(cfg_merge with enable_stacked_cfg(sharded=True): one forward on (2, n_local, dim)); --periodic-gate adds that form to the stacked leg.
Per leg the median and the standard deviation over the repeats, and the stacked leg against the two-call leg of the same run.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fairygen_amd import sequence_parallel as sp  # noqa: E402


class DryShard(sp.TokenShard):
    def __init__(self, world_size, rank, attn_mode):
        self.group, self.attn_mode, self.world_size, self.rank = None, attn_mode, world_size, rank
        self.active = world_size > 1

    def _gather_rows(self, local, size):
        # every "peer" contributes a copy of the local rows: same statistics as real data (all-zero peers would let the
        # MFMA kernels run cooler and faster than they do in a real job)
        full = torch.empty((self.world_size, size, local.shape[-1]), dtype=local.dtype, device=local.device)
        full[:, : local.shape[0]] = local
        if local.shape[0] < size:
            full[:, local.shape[0]:] = 0
        return full.view(self.world_size * size, -1)

    def _gather_batch(self, local, size):
        # the stacked forward's slab (B, world * size, C), every "peer" a copy of the local rows of the element
        full = torch.empty((local.shape[0], self.world_size, size, local.shape[-1]), dtype=local.dtype, device=local.device)
        full[:, :, : local.shape[1]] = local.unsqueeze(1)
        if local.shape[1] < size:
            full[:, :, local.shape[1]:] = 0
        return full.view(local.shape[0], self.world_size * size, -1)

    def broadcast(self, tensor, src):
        return tensor

    def all_gather_records_async(self, record):
        if record.dim() == 2 and record.shape[0] > 1:      # one record per element of a stacked forward: (world, B, bytes)
            return _DryRecords(record.unsqueeze(0).repeat(self.world_size, 1, 1))
        return _DryRecords(record.view(1, -1).repeat(self.world_size, 1))      # every "peer" sends this rank's record


class _DryRecords:
    def __init__(self, full):
        self.full = full

    def wait(self):
        return self.full


class DryLayout:
    def __init__(self, world, cfg_parallel, attn_mode):
        self.cfg_parallel, self.attn_mode = cfg_parallel, attn_mode
        self.world = DryShard(world, 0, attn_mode)
        self.branch = 0 if cfg_parallel == 2 else None
        self.shard = DryShard(world // cfg_parallel, 0, attn_mode)

    describe = sp.ParallelLayout.describe
    sp = property(lambda self: self.shard.world_size)

    def gather_branches(self, out_local, n):
        size = self.shard.chunk(n)
        full = self.world._gather_rows(out_local[0], size)
        return full.view(2, self.sp * size, -1)[:, :n]


def _copy_rows(shard, send, recv):
    recv.copy_(send)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--only", default="", help="substring filter on the layout name (profiling one layout)")
    ap.add_argument("--no-vae", action="store_true")
    ap.add_argument("--height", type=int, default=704)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=121)
    ap.add_argument("--attention", choices=("bf16", "qk8", "pv8", "pv8-cross", "full"), default="bf16",
                    help="attention form of every line (default: bf16)")
    ap.add_argument("--stacked-cfg", action="store_true",
                    help="on the all-gather cfg_parallel=1 layouts: the stacked CFG forward next to the two-call leg, in turns in one process")
    ap.add_argument("--periodic-gate", action="store_true", help="with --stacked-cfg: enable_stacked_cfg(periodic_gate=True) in the stacked leg")
    ap.add_argument("--repeats", type=int, default=5, help="with --stacked-cfg: timed repeats per leg (median and sd are printed)")
    a = ap.parse_args()
    args = argparse.Namespace(layers=0, no_lora=True, height=a.height, width=a.width, frames=a.frames)
    device = "cuda:0"
    sp._staged = lambda t, group: True                       # take the synchronous branch of the pending objects ...
    sp._all_to_all_rows = _copy_rows                         # ... and copy instead of exchanging
    pipe, cfg = bench.build_pipeline(args, device)
    if a.attention in ("qk8", "pv8"):
        pipe.dit.enable_qk8_attention(pv8=a.attention == "pv8", sharded=True)
    elif a.attention != "bf16":
        full = a.attention == "full"
        pipe.dit.enable_qk8_attention(pv8=True, fused_producer=True, cross=True, smooth_v=full, smooth_v_cross=full, sharded="all")
    print(f"attention: {a.attention}")
    lat_shape = (1, 48, (a.frames - 1) // 4 + 1, a.height // 16, a.width // 16)
    noise = bench.seeded(lat_shape, 1).to(device)
    ctx_p, ctx_n = bench.seeded((1, 512, 4096), 2).to(device), bench.seeded((1, 512, 4096), 3).to(device)
    z0 = bench.seeded((1, 48, 1, lat_shape[3], lat_shape[4]), 4).to(device)

    def run(steps, merge=False):
        pipe.scheduler.set_timesteps(steps, denoising_strength=1.0, shift=5.0)
        lat = noise.clone()
        shared = {"latents": lat, "fuse_vae_embedding_in_latents": True, "first_frame_latents": z0}
        if merge:      # the merged call: the batched context is shared, the branches carry none
            shared.update(cfg_merge=True, context=torch.cat([ctx_p, ctx_n], 0))
            return pipe.denoise(shared, {}, {}, 5.0, progress_bar_cmd=lambda x: x)
        return pipe.denoise(shared, {"context": ctx_p}, {"context": ctx_n}, 5.0, progress_bar_cmd=lambda x: x)

    def timed(steps, merge=False, warm=True):
        if warm:
            run(1, merge)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps, merge)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def legs(world):
        """The two-call leg and the stacked leg of one layout in turns: [two-call times], [stacked times], seconds per step."""
        times = ([], [])
        for rep_ in range(a.repeats + 1):      # round 0 warms both legs up and is dropped
            for leg in (0, 1):
                pipe.dit.enable_stacked_cfg(bool(leg), periodic_gate=bool(leg) and a.periodic_gate, sharded=bool(leg))
                t = timed(a.steps, merge=bool(leg), warm=False)
                if rep_:
                    times[leg].append(t)
        pipe.dit.enable_stacked_cfg(False)
        return times

    with torch.no_grad():
        base = timed(a.steps)
        print(f"single: {base * 1e3:.1f} ms/step")
        for world in [int(w) for w in a.worlds.split(",")]:
            for cfgp, mode in bench.candidate_layouts(world, cfg["num_heads"]):
                if a.only and a.only not in DryLayout(world, cfgp, mode).describe():
                    continue
                if a.stacked_cfg and (cfgp != 1 or mode != "allgather"):
                    continue
                pipe.parallel = DryLayout(world, cfgp, mode)
                pipe.sequence_shard = pipe.parallel.shard
                if a.stacked_cfg:
                    two, stk = legs(world)
                    m2, ms = statistics.median(two), statistics.median(stk)
                    print(f"world {world} {pipe.parallel.describe()} [{a.attention}{' periodic-gate' if a.periodic_gate else ''}] "
                          f"{a.repeats} x {a.steps} steps, legs in turns: two-call {m2 * 1e3:.1f} ms/step (sd {statistics.pstdev(two) * 1e3:.2f}), "
                          f"stacked {ms * 1e3:.1f} ms/step (sd {statistics.pstdev(stk) * 1e3:.2f}) per rank, no comm -> stacked / two-call "
                          f"{ms / m2:.3f}; against single x{base / m2:.2f} -> x{base / ms:.2f} of {world}", flush=True)
                    continue
                t = timed(a.steps)
                print(f"world {world} {pipe.parallel.describe()}: {t * 1e3:.1f} ms/step per rank, no comm -> "
                      f"x{base / t:.2f} of {world} ({base / t / world * 100:.0f}%)", flush=True)
        if a.no_vae or a.stacked_cfg:
            return
        # VAE: the largest tile alone is the decode critical path at >= 6 ranks
        pipe.parallel = None
        lat = noise
        pipe.vae.decode(lat[:, :, :2, :8, :8].contiguous(), device=device, tiled=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.vae.model.decode(lat[:, :, :, :30, :52].contiguous(), pipe.vae.scale)
        torch.cuda.synchronize()
        print(f"VAE largest tile (30x52 latent): {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()

"""Three denoise steps of BASELINE.json configs[1] (480x832x49: latent (1,48,13,30,52), N = 5 070 tokens) at the full model width,
with the REFERENCE's own model_fn_wan_video and FlowMatchScheduler on the CPU, next to the oracle's loop in bf16 and fp32.

    python oracle/gen_config2_loop.py          # build container only (needs /root/reference); ~20-30 min on 8 cores, < 35 GB

Wan2.2-TI2V-5B (30 blocks, dim 3072, synthetic weights), config 2's latent with the TI2V first frame, config 1's two prompts,
3 steps (the last one to sigma 0), CFG 5, shift 5, frame 0 re-pinned after every step.  The oracle (oracle.pipeline.denoise_loop)
must reproduce the reference's latents of every step bit for bit; the same loop evaluated in fp32 is the yardstick of the GPU test
(tests/test_hip_models.py::test_config2_loop_full_width_vs_reference_golden), which runs it on the production kernel mix: the w4
attention kernel with the folded softmax scale, the own GEMMs, the shared CFG prefix and the cross-attention K/V cache.

Writes tests/golden/config2_loop.part{0,1,2}.safetensors: every 8th channel of the reference's bf16 latents and of the fp32 ones after
every step, each tensor cut along its last dimension into three parts (each file < 1 MiB); the same bytes on every run.
"""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import gen_golden  # noqa: E402

STEPS = 3
CH = 8          # channels 0, 8, ..., 40 are stored
PARTS = 3


def save_parts(name, tensors, meta, parts, limit=1 << 20):
    """gen_golden.save() of a fixture above the 1 MiB limit for a committed file: <stem>.part0.safetensors, .part1, ..., every tensor cut
    along its last dimension into `parts` pieces in part order (what the tests' `golden` fixture joins back)."""
    stem = name[: -len(".safetensors")]
    pieces = {k: v.tensor_split(parts, dim=-1) for k, v in tensors.items()}
    for i in range(parts):
        part = f"{stem}.part{i}.safetensors"
        gen_golden.save(part, {k: p[i] for k, p in pieces.items()}, meta)
        size = os.path.getsize(os.path.join(gen_golden.OUT, part))
        assert size < limit, f"{part}: {size} bytes >= {limit}"


def config2_loop_inputs():
    s = gen_golden.seeded
    noise = s((1, 48, 13, 30, 52), 1)
    z0 = s((1, 48, 1, 30, 52), 4)
    ctx_p = s((1, 512, 4096), 2); ctx_p[:, 64:] = 0
    ctx_n = s((1, 512, 4096), 3); ctx_n[:, 128:] = 0
    return noise, ctx_p, ctx_n, z0


def main():
    torch.set_num_threads(8)
    R = gen_golden.import_reference()
    from fairygen_amd import synthetic
    from fairygen_amd.loader import TI2V_5B_DIT_KWARGS
    from oracle import pipeline as opipe
    cfg = dict(TI2V_5B_DIT_KWARGS)
    sd = synthetic.random_state_dict(synthetic.dit_shapes(cfg), seed=1234)
    with torch.device("meta"):
        model = R["dit"].WanModel(**cfg)
    model.load_state_dict(sd, assign=True)
    model.freqs = R["dit"].precompute_freqs_cis_3d(cfg["dim"] // cfg["num_heads"])
    model.eval()
    noise, ctx_p, ctx_n, z0 = config2_loop_inputs()
    fn = R["pipe"].model_fn_wan_video
    ref, timing = [], {}
    with torch.no_grad():
        # the loop of WanVideoPipeline.__call__ (pipelines/wan_video.py:283-309)
        sched = R["sched"]("Wan")
        sched.set_timesteps(STEPS, denoising_strength=1.0, shift=5.0)
        latents = noise.clone()
        latents[:, :, 0:1] = z0
        t0 = time.perf_counter()
        for pid, timestep in enumerate(sched.timesteps):
            t = timestep.unsqueeze(0).to(dtype=torch.bfloat16)
            posi = fn(dit=model, latents=latents, timestep=t, context=ctx_p, fuse_vae_embedding_in_latents=True)
            nega = fn(dit=model, latents=latents, timestep=t, context=ctx_n, fuse_vae_embedding_in_latents=True)
            latents = sched.step(nega + 5.0 * (posi - nega), sched.timesteps[pid], latents)
            latents[:, :, 0:1] = z0
            ref.append(latents.clone())
            print(f"reference step {pid}: {time.perf_counter() - t0:.0f} s", flush=True)
        timing["reference_loop_s"] = time.perf_counter() - t0
        del model, posi, nega
        rec = []
        t0 = time.perf_counter()
        opipe.denoise_loop(sd, cfg, noise, ctx_p, ctx_n, STEPS, 5.0, 5.0, z0, record=rec)
        timing["oracle_loop_s"] = time.perf_counter() - t0
        same = [torch.equal(a, b) for a, b in zip(rec, ref)]
        for i, ok in enumerate(same):
            print(f"step {i}: oracle {'equals' if ok else 'DIFFERS FROM'} reference", flush=True)
        assert len(same) == STEPS and all(same), "the oracle restatement differs from the reference's loop at N = 5070"
        del rec
        # the same loop in fp32 (the restatement; it equals the reference in bf16 above): how far a correct bf16 evaluation of this
        # random-weight network may sit from the fp32-ideal one, step by step
        sd32 = {k: v.float() for k, v in sd.items()}
        del sd
        rec32 = []
        t0 = time.perf_counter()
        opipe.denoise_loop(sd32, cfg, noise.float(), ctx_p.float(), ctx_n.float(), STEPS, 5.0, 5.0, z0.float(), dtype=torch.float32,
                           record=rec32)
        timing["fp32_loop_s"] = time.perf_counter() - t0
        del sd32
    out = {}
    for i in range(STEPS):
        b, f = ref[i][:, ::CH].contiguous(), rec32[i][:, ::CH].contiguous()
        out[f"ref_bf16_step{i}"], out[f"f32_step{i}"] = b, f
        d = (b.float() - f).abs()
        cos = torch.nn.functional.cosine_similarity(b.float().flatten(), f.flatten(), dim=0).item()
        timing[f"step{i}_bf16_vs_f32"] = {"cos": round(cos, 6), "mean_abs": round(d.mean().item(), 6), "max_abs": round(d.max().item(), 5)}
    timing.update(oracle_equals_reference=all(same), cores=torch.get_num_threads())
    print(json.dumps(timing, indent=1), flush=True)
    # one metadata entry: safetensors stores the metadata as a hash map, whose order (and so the file's bytes) varies between runs
    # when it has several entries; the timings are printed, not stored
    save_parts("config2_loop.safetensors", out, {"provenance": "; ".join([
        "config: TI2V_5B_DIT_KWARGS (30 blocks, dim 3072)",
        "weights: synthetic.random_state_dict(dit_shapes(), seed=1234), CPU generator",
        "inputs: noise=seeded((1,48,13,30,52),1); z0=seeded((1,48,1,30,52),4); ctx+=seeded((1,512,4096),2) rows>=64 zero; "
        "ctx-=seed 3 rows>=128 zero; 3 steps cfg 5 shift 5 denoising_strength 1, frame 0 re-pinned after every step",
        f"stored: latents after every step, channels 0,{CH},...,{48 - CH}; ref_bf16 = the reference's loop (the oracle equalled it "
        f"bit for bit), f32 = oracle.pipeline.denoise_loop(dtype=float32); every tensor cut along its last dim into {PARTS} parts",
        "source: diffsynth/pipelines/wan_video.py model_fn_wan_video + __call__ loop :283-309; diffusion/flow_match.py"])}, PARTS)


if __name__ == "__main__":
    main()

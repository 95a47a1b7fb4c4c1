"""animation/inference.py of the reference, on fairygen_amd (same calls; local checkpoint paths instead of downloads).

    python examples/inference.py --weights /path/to/Wan2.2-TI2V-5B --tokenizer /path/to/google/umt5-xxl \\
        --lora ./lora-libraries/pig_walk/merged/200_400.safetensors --image ./data/pig_walk/shot/1.png --out ./outputs/1.mp4
"""
import argparse
import glob
import os
import sys
from pathlib import Path

import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the repo root: run from anywhere, no install
from fairygen_amd import ModelConfig, WanVideoPipeline, save_video

NEGATIVE = ("色调艳丽，过曝，静态，细节模糊不清，字幕，风格，作品，画作，画面，静止，整体发灰，最差质量，低质量，JPEG压缩残留，丑陋的，残缺的，多余的手指，"
            "画得不好的手部，画得不好的脸部，畸形的，毁容的，形态畸形的肢体，手指融合，静止不动的画面，杂乱的背景，三条腿，背景人很多，倒着走")


def build_pipeline(weights, tokenizer, lora=None, fp8=False, qk8=False, pv8=False, cross8=False, stacked_cfg=False, periodic_gate=False,
                   smooth_v=False, smooth_v_cross=False):
    dit_cfg = dict(computation_dtype=torch.float8_e4m3fn) if fp8 else {}
    if stacked_cfg:
        dit_cfg["stacked_cfg"] = True
    if periodic_gate:
        dit_cfg["stacked_cfg_periodic_gate"] = True
    if qk8 or pv8:
        dit_cfg["attention_dtype"] = torch.float8_e4m3fn
    if pv8:
        dit_cfg["attention_pv_dtype"] = torch.float8_e4m3fn
    if cross8:
        dit_cfg["cross_attention_dtype"] = torch.float8_e4m3fn
    if smooth_v:
        dit_cfg["attention_v_smoothing"] = True
    if smooth_v_cross:
        dit_cfg["cross_attention_v_smoothing"] = True
    pipe = WanVideoPipeline.from_pretrained(
        torch_dtype=torch.bfloat16, device="cuda",
        model_configs=[
            ModelConfig(path=os.path.join(weights, "models_t5_umt5-xxl-enc-bf16.pth")),
            ModelConfig(path=sorted(glob.glob(os.path.join(weights, "diffusion_pytorch_model*.safetensors"))), **dit_cfg),
            ModelConfig(path=os.path.join(weights, "Wan2.2_VAE.pth")),
        ],
        tokenizer_config=ModelConfig(path=tokenizer))
    if lora:
        pipe.load_lora(pipe.dit, lora, alpha=1)
    if (qk8 or pv8) and getattr(pipe, "parallel", None) is not None:
        pipe.dit.enable_qk8_attention(**sharded_attention_switches(pipe.dit.qk8_fused_producer, pv8, cross8, smooth_v, smooth_v_cross))
    if stacked_cfg and stacked_cfg_on_layout(getattr(pipe, "parallel", None)):
        if fp8 and (qk8 or pv8):
            raise SystemExit("--stacked-cfg on a parallel layout with --fp8 AND an e4m3 attention form: that composition is not carried on "
                             "token shards (WanModel.check_stacked_cfg); drop --fp8 or the e4m3 attention switches, or drop --stacked-cfg")
        d = pipe.dit      # restate what the loader switched on: a call that does not restate a form clears it
        d.enable_stacked_cfg(fp8_linear=d.stacked_cfg_fp8, hot_lora=d.stacked_cfg_hot_lora, periodic_gate=d.stacked_cfg_periodic_gate, sharded=True)
    return pipe


def stacked_cfg_on_layout(layout):
    """Whether --stacked-cfg needs enable_stacked_cfg(sharded=True): False on a single GPU; True on a parallel layout that the stacked
    forward takes, the K / V all-gather exchange with cfg_parallel=1; any other parallel layout is an error said here, before anything runs."""
    if layout is None or layout.shard is None or not layout.shard.active:
        return False
    if layout.cfg_parallel != 1 or layout.attn_mode != "allgather":
        raise SystemExit(f"--stacked-cfg on the parallel layout {layout.describe()}: the stacked CFG forward runs on token shards of the K / V "
                         "all-gather layout with cfg_parallel=1 only (attn_mode='allgather'); use that layout, or drop --stacked-cfg")
    return True


def sharded_attention_switches(fused_producer, pv8, cross8, smooth_v, smooth_v_cross):
    """The enable_qk8_attention arguments of a token-sharded layout: the e4m3 mode with its statistics exchange (off by default; no
    multi-GPU hardware run exists).  sharded=True, self-attention qk8 / pv8 alone, unless one of the forms that want sharded="all" is
    asked for: V smoothing (the statistics record with a V sum), the e4m3 cross-attention, its V smoothing."""
    every = bool(smooth_v or cross8 or smooth_v_cross)
    return dict(fused_producer=fused_producer, pv8=pv8, cross=bool(cross8), smooth_v=bool(smooth_v), smooth_v_cross=bool(smooth_v_cross),
                sharded="all" if every else True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", required=True)
    ap.add_argument("--tokenizer", required=True)
    ap.add_argument("--lora")
    ap.add_argument("--image", required=True)
    ap.add_argument("--prompt", default="[p]_character_[w]_motion [p] walks towards the camera, filling the frame with a sense of movement.")
    ap.add_argument("--out", default="./outputs/1.mp4")
    ap.add_argument("--fp8", action="store_true", help="the reference's fp8 Linear mode for the DiT blocks")
    ap.add_argument("--qk8-attention", action="store_true",
                    help="e4m3 Q K^T in the DiT's self-attention (the reference's sageattn branch); P V and cross-attention stay bf16")
    ap.add_argument("--pv8-attention", action="store_true",
                    help="... and e4m3 P V as well (both MFMAs of self-attention 8-bit); implies --qk8-attention")
    ap.add_argument("--cross8-attention", action="store_true",
                    help="... and cross-attention over the text context in the same e4m3 form; implies --pv8-attention")
    ap.add_argument("--smooth-v", action="store_true",
                    help="with e4m3 P V: the key mean of every V channel leaves V before it is quantised and joins the output row (sageattn's "
                         "smooth_v; ModelConfig(attention_v_smoothing=True)); self-attention only; implies --pv8-attention")
    ap.add_argument("--smooth-v-cross", action="store_true",
                    help="with e4m3 cross-attention: the same smoothing for V of the text context, most of whose 512 keys carry one padding "
                         "row (ModelConfig(cross_attention_v_smoothing=True)); independent of --smooth-v; implies --cross8-attention")
    ap.add_argument("--stacked-cfg", action="store_true",
                    help="both CFG branches in ONE stacked forward of the DiT per step (implies cfg_merge=True); single GPU, or a parallel layout "
                         "with the K / V all-gather exchange and cfg_parallel=1 (enable_stacked_cfg(sharded=True)); bf16 Linears or, "
                         "with --fp8, the fp8 Linear mode (the loader then calls enable_stacked_cfg(fp8_linear=True)); --lora here is fused into the weights and works; unfused hot-loaded "
                         "adapters need hot_backend='hip' and ModelConfig(stacked_cfg_hot_lora=True)")
    ap.add_argument("--stacked-cfg-periodic-gate", action="store_true",
                    help="with --stacked-cfg: the gated Linears of a block (self_attn.o, ffn.2) as ONE GEMM launch on the rows of both CFG "
                         "branches instead of one per branch (ModelConfig(stacked_cfg_periodic_gate=True))")
    a = ap.parse_args()
    if a.stacked_cfg_periodic_gate and not a.stacked_cfg:
        ap.error("--stacked-cfg-periodic-gate is a form of --stacked-cfg")
    cross8 = a.cross8_attention or a.smooth_v_cross
    pv8 = a.pv8_attention or cross8 or a.smooth_v
    pipe = build_pipeline(a.weights, a.tokenizer, a.lora, a.fp8, a.qk8_attention or pv8, pv8, cross8, a.stacked_cfg,
                          a.stacked_cfg_periodic_gate, **({"smooth_v": True} if a.smooth_v else {}),
                          **({"smooth_v_cross": True} if a.smooth_v_cross else {}))
    image = Image.open(a.image).convert("RGB").resize((832, 480))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    video = pipe(prompt=a.prompt, negative_prompt=NEGATIVE, input_image=image, num_frames=81, seed=1, tiled=True, cfg_merge=a.stacked_cfg)
    print("wrote", save_video(video, a.out, fps=15, quality=5))


if __name__ == "__main__":
    main()

"""The reference's untiled VAE38 decode of a latent long enough for the decoder groups of 8: (1,48,11,2,2) -> (1,3,41,32,32) on the
tiny decoder (dim = dec_dim = 32, the weights and hand-assembled wrapper of gen_golden.py section 5).  The reference decodes one
latent frame per decoder call; the HIP decode runs chunks 1 + 8 + 2, so this pins the group of 8 against the reference's order.

    python oracle/gen_vae_long.py          # needs the reference checkout (gen_golden.import_reference); a few seconds

Writes tests/golden/vae_long.safetensors: the clamped bf16 decode of the reference, the clamped fp32 decode (the yardstick) and a
provenance string; the same bytes on every run.
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import gen_golden  # noqa: E402

LIMIT = 1 << 20        # committed files stay within 1 MiB


def main():
    torch.set_num_threads(8)
    R = gen_golden.import_reference()
    from fairygen_amd import synthetic
    from oracle.wan_vae import VAE38_MEAN, VAE38_STD
    ref_vae = R["vae"]
    dim, dec_dim = 32, 32
    vsd = synthetic.random_state_dict(synthetic.vae_shapes(dec_dim=dec_dim, dim=dim), seed=1234)
    inner = ref_vae.VideoVAE38_(dim=dim, z_dim=48, dec_dim=dec_dim).eval().requires_grad_(False)
    wrap = ref_vae.WanVideoVAE38.__new__(ref_vae.WanVideoVAE38)
    torch.nn.Module.__init__(wrap)
    wrap.mean, wrap.std = torch.tensor(VAE38_MEAN), torch.tensor(VAE38_STD)
    wrap.scale = [wrap.mean, 1.0 / wrap.std]
    wrap.model, wrap.upsampling_factor, wrap.z_dim = inner, 16, 48
    wrap = wrap.to(torch.bfloat16)
    wrap.load_state_dict(vsd)
    z = gen_golden.seeded((1, 48, 11, 2, 2), 36)
    with torch.no_grad():
        out = {"decode_bf16": wrap.decode(z, device="cpu", tiled=False)}
        out["decode_f32"] = wrap.float().decode(z.float(), device="cpu", tiled=False)
    assert tuple(out["decode_bf16"].shape) == (1, 3, 41, 32, 32)
    name = "vae_long.safetensors"
    # one metadata entry: safetensors stores the metadata as a hash map, whose order (and so the file's bytes) varies between runs
    # when it has several entries
    gen_golden.save(name, out, {"provenance": "; ".join([
        f"config: VideoVAE38_(dim={dim}, z_dim=48, dec_dim={dec_dim}) in a hand-assembled WanVideoVAE38 wrapper (gen_golden.py section 5)",
        f"weights: synthetic.random_state_dict(vae_shapes(dec_dim={dec_dim}, dim={dim}), seed=1234)",
        "inputs: z=seeded((1,48,11,2,2),36); decode(tiled=False), one latent frame per decoder call, output clamped to [-1, 1]",
        "source: diffsynth/models/wan_video_vae.py WanVideoVAE.decode / single_decode :1212-1215,1235-1247; VideoVAE38_.decode :1326-1351"])})
    size = os.path.getsize(os.path.join(gen_golden.OUT, name))
    assert size <= LIMIT, f"{name}: {size} bytes > {LIMIT}"


if __name__ == "__main__":
    main()

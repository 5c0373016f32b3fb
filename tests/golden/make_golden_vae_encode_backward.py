"""Writes tests/golden/vae_encode_backward.npz by RUNNING the reference's own GeneralVAESeg (only where the reference checkout
exists): its encoder under CPU autograd at B = 2, H = 16 with this repository's deterministic weights, `backward()` from a seeded
gradient of the moments, and its DiagonalGaussianDistribution.sample under `backward()` from a seeded gradient of the latents on
moments whose logvar lies inside, outside and on the bounds of the clamp.  Nothing of the reference is copied: the fixture holds
the inputs and the gradients its modules returned - x, grad_moments, the noise, grad_z -> grad_moments, the small parameter
gradients whole and, for the large weight gradients, every 97th element plus their fp64 sum and absolute sum.

    python tests/golden/make_golden_vae_encode_backward.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, ROOT, stub_modules  # noqa: E402

OUT = os.path.join(HERE, "vae_encode_backward.npz")
STRIDE, WHOLE_BELOW = 97, 4096
NOISE_SEED = 77


def main():
    if not os.path.isdir(os.path.join(REF, "ldmseg")):
        print("reference checkout not found; nothing to do")
        return
    stub_modules()
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))
    from ldmseg.models.vae import DiagonalGaussianDistribution, GeneralVAESeg
    import vae_encode_backward_ref as R
    kw = dict(in_channels=7, int_channels=256, out_channels=128, block_out_channels=[32, 64, 128, 256],
              latent_channels=4, num_latents=2, num_upscalers=2, upscale_channels=256, norm_num_groups=32,
              scaling_factor=0.2, parametrization="gaussian", act_fn="none", clamp_output=False,
              freeze_codebook=False, num_mid_blocks=0, fuse_rgb=False, resize_input=False, skip_encoder=False)
    ref = GeneralVAESeg(**kw)
    ref.load_state_dict(R.state_dict("seg"), strict=True)
    B, H = 2, 16
    x, gm = R.inputs("seg", B, H)
    moments = ref.encode(x * R.IN_MUL + R.IN_ADD).latent_dist.parameters
    moments.backward(gm)
    out = {"B": np.int64(B), "H": np.int64(H), "stride": np.int64(STRIDE), "x": x.numpy(), "grad_moments": gm.numpy(),
           "moments": moments.detach().numpy()}
    for k, p in ref.named_parameters():
        if not k.startswith("encoder."):
            continue
        g = p.grad.detach()
        if g.numel() < WHOLE_BELOW:
            out["grad/" + k] = g.numpy()
        else:
            flat = g.reshape(-1)
            out["sample/" + k] = flat[::STRIDE].numpy()
            out["sum/" + k] = np.float64(flat.double().sum())
            out["abssum/" + k] = np.float64(flat.double().abs().sum())
            out["max/" + k] = np.float64(flat.double().abs().max())
    # the posterior: sample() on crafted moments; the noise is what its generator draws
    mom, _, gz = R.posterior_case()
    m = mom.clone().requires_grad_(True)
    z = DiagonalGaussianDistribution(m).sample(generator=torch.Generator().manual_seed(NOISE_SEED))
    noise = torch.randn(z.shape, generator=torch.Generator().manual_seed(NOISE_SEED))
    z.backward(gz)
    out.update({"post/moments": mom.numpy(), "post/noise": noise.numpy(), "post/grad_z": gz.numpy(), "post/z": z.detach().numpy(),
                "post/grad_moments": m.grad.numpy()})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()

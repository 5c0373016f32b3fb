"""Writes tests/golden/clip_vision.npz: the small CLIP vision configuration's weights, one input and the three outputs
**as transformers computes them** (CLIPVisionModelWithProjection).  Needs `transformers`; the fixture it writes is what
pins tests/clip_vision_ref.py where transformers is not installed.

Weights: ldmseg_amd.weights.generate() of clip_vision_schema(**SMALL), quantised per tensor to 255 levels and stored as
int8 `q::<key>` with the fp32 step `s::<key>` (the weight is q * s in fp32), which keeps the file inside the repository's
size limit for committed files; the model is loaded with exactly those dequantised values.

    python tests/golden/make_golden_clip.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "latent-diffusion-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def quantise(t):
    step = np.float32(float(t.abs().max()) / 127.0)
    q = torch.round(t / float(step)).clamp(-127, 127).to(torch.int8).numpy()
    return q, step


def dequantise(q, step):
    return torch.from_numpy(q.astype(np.float32) * np.float32(step))


def load_weights(z):
    """{key: fp32 tensor} from the fixture (used by the tests as well)"""
    return {k[3:]: dequantise(z[k], z["s::" + k[3:]]) for k in z.files if k.startswith("q::")}


def main():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    import clip_vision_ref as R
    from ldmseg_amd import weights
    c = R.SMALL
    schema = weights.clip_vision_schema(**c)
    sd = weights.generate(schema, seed=11, norm_keys=weights.clip_vision_norm_keys(schema))
    out = {}
    for k, v in sd.items():
        out["q::" + k], out["s::" + k] = quantise(v)
    sd = load_weights(type("Z", (), {"files": list(out), "__getitem__": lambda self, k: out[k]})())
    cfg = CLIPVisionConfig(hidden_size=c["hidden"], intermediate_size=c["intermediate"], num_hidden_layers=c["layers"],
                           num_attention_heads=c["heads"], image_size=c["image"], patch_size=c["patch"],
                           projection_dim=c["projection_dim"])
    model = CLIPVisionModelWithProjection(cfg).eval()
    full = {(k if k.startswith("visual_projection") else "vision_model." + k): v for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    x = torch.randn(2, 3, c["image"], c["image"], generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        o = model(pixel_values=x)
        v = model.vision_model(pixel_values=x)
    out.update(pixel_values=x.numpy(), last_hidden_state=v.last_hidden_state.numpy(), pooler_output=v.pooler_output.numpy(),
               image_embeds=o.image_embeds.numpy())
    path = os.path.join(HERE, "clip_vision.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

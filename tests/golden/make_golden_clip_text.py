"""Writes tests/golden/clip_text.npz: the small CLIP text configuration's weights, one batch of ids and the
last_hidden_state **as transformers computes it** (CLIPTextModel, hidden_act="quick_gelu").  Needs `transformers`; the
fixture it writes is what pins tests/clip_text_ref.py where transformers is not installed.

Weights: ldmseg_amd.weights.generate() of clip_text_schema(**SMALL), quantised per tensor to 255 levels and stored as int8
`q::<key>` with the fp32 step `s::<key>` as in make_golden_clip.py; the model is loaded with exactly those dequantised
values.

    python tests/golden/make_golden_clip_text.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "latent-diffusion-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden_clip import quantise, load_weights   # noqa: E402


def text_model(tf, c):
    """transformers' CLIPTextModel of a configuration dict (used by the CPU test as well)"""
    cfg = tf.CLIPTextConfig(vocab_size=c["vocab"], hidden_size=c["hidden"], intermediate_size=c["intermediate"],
                            num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                            max_position_embeddings=c["positions"], hidden_act="quick_gelu", projection_dim=c["hidden"],
                            bos_token_id=c["vocab"] - 2, eos_token_id=c["vocab"] - 1, pad_token_id=c["vocab"] - 1)
    return tf.CLIPTextModel(cfg).eval()


def load_into(model, sd):
    """loads a prefix-less state dict under whichever key layout this transformers release uses"""
    keys = [k for k in model.state_dict() if "position_ids" not in k]
    full = {k: sd[k[len("text_model."):] if k.startswith("text_model.") else k] for k in keys}
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    return full


def main():
    import transformers as tf
    import clip_text_ref as R
    from ldmseg_amd import weights
    c = R.SMALL
    schema = weights.clip_text_schema(**c)
    sd = weights.generate(schema, seed=13, norm_keys=weights.clip_text_norm_keys(schema))
    out = {}
    for k, v in sd.items():
        out["q::" + k], out["s::" + k] = quantise(v)
    sd = load_weights(type("Z", (), {"files": list(out), "__getitem__": lambda self, k: out[k]})())
    model = text_model(tf, c)
    load_into(model, sd)
    ids = R.prompt_ids([5, 40, 76], c["positions"], c["vocab"], seed=5)
    with torch.no_grad():
        o = model(input_ids=ids)
    out.update(input_ids=ids.numpy(), last_hidden_state=o.last_hidden_state.numpy())
    path = os.path.join(HERE, "clip_text.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

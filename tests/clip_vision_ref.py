"""Torch-only restatement of transformers' CLIPVisionModel / CLIPVisionModelWithProjection forward (the image
descriptor of the clip_image / clip_image_proj modes) on a prefix-less state dict, as the reference for the library's
CLIP vision executor.  tests/test_clip_vision_cpu.py pins it against transformers itself (where installed) and against
outputs transformers produced (tests/golden/clip_vision.npz); GPU tests import nothing but this file.

`rnd`: a rounding hook applied to every GEMM / attention operand and every stored activation; `bf16_round` makes the
forward a simulation of bf16 storage with fp32 accumulation (it leaves the accumulation order out)."""
import torch
import torch.nn.functional as F

PIXEL_MEAN_CLIP = (0.48145466, 0.4578275, 0.40821073)
PIXEL_STD_CLIP = (0.26862954, 0.26130258, 0.27577711)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def strip_prefix(sd):
    return {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}


def norm_resize(rgb, size=224, mean=PIXEL_MEAN_CLIP, std=PIXEL_STD_CLIP):
    """norm_resize_images of the reference trainer for a CLIP descriptor: bilinear (no antialias) + CLIP statistics."""
    x = F.interpolate(rgb, size=(size, size), mode='bilinear', align_corners=False)
    m = torch.tensor(mean, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - m) / s


def forward(sd, pixel_values, heads, eps=1e-5, rnd=None):
    """-> dict(last_hidden_state [B,T,C], pooler_output [B,C], image_embeds [B,P] or None)."""
    sd = strip_prefix(sd)
    r = (lambda t: t) if rnd is None else rnd
    dt = pixel_values.dtype
    W = {k: v.to(dt) for k, v in sd.items() if torch.is_floating_point(v)}
    wp = W["embeddings.patch_embedding.weight"]
    C, patch = wp.shape[0], wp.shape[-1]
    B = pixel_values.shape[0]
    h = r(F.conv2d(r(pixel_values), r(wp), stride=patch)).flatten(2).transpose(1, 2)
    cls = W["embeddings.class_embedding"].view(1, 1, C).expand(B, 1, C)
    h = torch.cat([cls, h], 1) + W["embeddings.position_embedding.weight"].unsqueeze(0)
    h = r(F.layer_norm(h, (C,), W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], eps))
    T = h.shape[1]
    d = C // heads
    layers = 1 + max(int(k.split(".")[2]) for k in W if k.startswith("encoder.layers."))
    for i in range(layers):
        p = f"encoder.layers.{i}."
        y = r(F.layer_norm(h, (C,), W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], eps))
        q, k, v = (r(F.linear(y, r(W[p + f"self_attn.{n}_proj.weight"]), W[p + f"self_attn.{n}_proj.bias"]))
                   .view(B, T, heads, d).transpose(1, 2) for n in ("q", "k", "v"))
        a = torch.softmax((q @ k.transpose(-1, -2)) * d ** -0.5, dim=-1)
        a = r(r(a) @ v).transpose(1, 2).reshape(B, T, C)
        h = r(h + F.linear(a, r(W[p + "self_attn.out_proj.weight"]), W[p + "self_attn.out_proj.bias"]))
        y = r(F.layer_norm(h, (C,), W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], eps))
        y = F.linear(y, r(W[p + "mlp.fc1.weight"]), W[p + "mlp.fc1.bias"])
        y = r(y * torch.sigmoid(1.702 * y))
        h = r(h + F.linear(y, r(W[p + "mlp.fc2.weight"]), W[p + "mlp.fc2.bias"]))
    pooled = F.layer_norm(h[:, 0], (C,), W["post_layernorm.weight"], W["post_layernorm.bias"], eps)
    emb = F.linear(pooled, W["visual_projection.weight"]) if "visual_projection.weight" in W else None
    return dict(last_hidden_state=h, pooler_output=pooled, image_embeds=emb)


def last_feat(out, projection):
    """What the reference's wrappers return (descriptors.py:26-37, 48-56)."""
    return out["image_embeds"].unsqueeze(-1) if projection else out["last_hidden_state"].permute(0, 2, 1)


def rel_err(a, b):
    """max-norm relative error, the suite's parity figure"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


SMALL = dict(hidden=128, intermediate=512, layers=2, heads=2, image=42, patch=14, projection_dim=96)

"""Cost of the CLIP ViT-L/14 image descriptor: ms per `describe` call from 512 x 512 images on the library in its three
compute modes, against what a user had to run before the library had the encoder - the same weights in a torch module
on the same GPU (fp32, under bf16 autocast, and converted to bf16 once), F.interpolate + normalise included.

  python tools/clip_cost.py [--B 8 16] [--size 512] [--warmup 3] [--iters 20] [--projection]

The torch module is transformers' CLIPVisionModel(/WithProjection) where transformers is installed, else the same
arithmetic as a plain torch module.  Timing: one HIP-event pair per call after `warmup` calls, median of `iters` calls.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def median_ms(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def torch_module(sd, projection, half=False):
    """(module on the GPU returning the descriptor output, its name); half: parameters converted to bf16 once"""
    import torch
    import torch.nn.functional as F
    try:
        import transformers as tf
        cfg = tf.CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                                  image_size=224, patch_size=14, projection_dim=768)
        if projection:
            m = tf.CLIPVisionModelWithProjection(cfg)
            full = {(k if k.startswith("visual_projection") else "vision_model." + k): v for k, v in sd.items()}
        else:
            m = tf.CLIPVisionModel(cfg)
            pref = any(k.startswith("vision_model.") for k in m.state_dict())
            full = {("vision_model." + k if pref else k): v for k, v in sd.items()}
        m.load_state_dict(full, strict=False)
        m = m.eval().to(DEV)
        if half:
            m = m.to(torch.bfloat16)
        return (lambda x: m(pixel_values=x).image_embeds if projection else m(pixel_values=x).last_hidden_state), "transformers"
    except ImportError:
        pass
    W = {k: v.to(DEV, torch.bfloat16 if half else torch.float32) for k, v in sd.items()}

    def fwd(x):
        C, heads, d = 1024, 16, 64
        B = x.shape[0]
        h = F.conv2d(x, W["embeddings.patch_embedding.weight"].to(x.dtype), stride=14).flatten(2).transpose(1, 2)
        h = torch.cat([W["embeddings.class_embedding"].view(1, 1, C).expand(B, 1, C).to(h.dtype), h], 1)
        h = h + W["embeddings.position_embedding.weight"]
        h = F.layer_norm(h, (C,), W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], 1e-5)
        for i in range(24):
            p = f"encoder.layers.{i}."
            y = F.layer_norm(h, (C,), W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], 1e-5)
            q, k, v = (F.linear(y, W[p + f"self_attn.{n}_proj.weight"], W[p + f"self_attn.{n}_proj.bias"])
                       .view(B, -1, heads, d).transpose(1, 2) for n in ("q", "k", "v"))
            a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, -1, C)
            h = h + F.linear(a, W[p + "self_attn.out_proj.weight"], W[p + "self_attn.out_proj.bias"])
            y = F.layer_norm(h, (C,), W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], 1e-5)
            y = F.linear(y, W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"])
            y = y * torch.sigmoid(1.702 * y)
            h = h + F.linear(y, W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"])
        if not projection:
            return h
        pooled = F.layer_norm(h[:, 0], (C,), W["post_layernorm.weight"], W["post_layernorm.bias"], 1e-5)
        return F.linear(pooled, W["visual_projection.weight"])
    return fwd, "torch module"


def main():
    import torch
    import torch.nn.functional as F
    from ldmseg_amd import weights
    from ldmseg_amd.models import CLIPVisionDescriptor
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--projection", action="store_true", help="clip_image_proj (image_embeds) instead of clip_image")
    args = ap.parse_args()
    schema = weights.clip_vision_schema(projection_dim=768 if args.projection else 0)
    sd = weights.generate(schema, seed=13, norm_keys=weights.clip_vision_norm_keys(schema))
    mean = torch.tensor(MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=DEV).view(1, 3, 1, 1)
    fwd, name = torch_module(sd, args.projection)
    fwd16, _ = torch_module(sd, args.projection, half=True)

    def torch_describe(rgb, autocast, half=False):
        x = (F.interpolate(rgb, size=(224, 224), mode="bilinear", align_corners=False) - mean) / std
        if half:                                   # the module converted to bf16 once: no per-call casts of the weights
            with torch.no_grad():
                return fwd16(x.to(torch.bfloat16)).float()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return fwd(x)

    images = {B: torch.rand(B, 3, args.size, args.size, generator=torch.Generator().manual_seed(B)).to(DEV) for B in args.B}
    for B in args.B:
        for autocast in (False, True):
            ms = median_ms(lambda: torch_describe(images[B], autocast), args.warmup, args.iters)
            print(json.dumps({"what": "describe", "impl": name + (" bf16 autocast" if autocast else " fp32"), "B": B,
                              "size": args.size, "projection": args.projection, "ms": round(ms, 3)}), flush=True)
        ms = median_ms(lambda: torch_describe(images[B], False, half=True), args.warmup, args.iters)
        print(json.dumps({"what": "describe", "impl": name + " bf16 module (.to(bfloat16))", "B": B, "size": args.size,
                          "projection": args.projection, "ms": round(ms, 3)}), flush=True)
    for mode in ("bf16", "bf16x3", "fp32"):
        m = CLIPVisionDescriptor(sd, projection=args.projection, device=DEV, compute_dtype=mode)
        for B in args.B:
            ms = median_ms(lambda: m.describe(images[B]), args.warmup, args.iters)
            print(json.dumps({"what": "describe", "impl": "ldmseg_hip " + mode, "B": B, "size": args.size,
                              "projection": args.projection, "ms": round(ms, 3)}), flush=True)
        del m


if __name__ == "__main__":
    main()

"""Test support: the forward of a UNet with a separate image encoder, restated on the oracle's blocks.

What ``modify_encoder(separate_encoder=True[, add_adaptor=True])`` of the reference builds and its forward runs
(ldmseg/models/unet.py:42-63, 301-385), written from that description on ``oracle.unet``'s resnet / transformer /
timestep_embedding:

* the 8-channel sample is split into a segmentation half and an image half;
* the image half goes through ``conv_in_img`` and ``down_blocks_additional`` with the time embedding of ``timestep_img``
  (zeros when None), through the SAME time_embedding MLP as the main path; the outputs of block i pass
  ``adaptor_layers[i]`` (3x3, C -> C) where the state dict has them - conv_in_img's own output does not - and the
  un-adapted tensor feeds the next layer;
* the segmentation half goes through ``conv_in`` and ``down_blocks`` as always;
* every skip connection becomes itself plus its image residual; the mid block takes the un-summed running tensor.

``reference_loop`` is the four-step sampling loop in the reference's order (trainers_ldm_cond.py:1121-1160, no
self-conditioning, no timestep_img) on ``oracle.ddim``.
"""
import torch
import torch.nn.functional as F

from oracle import ddim as o_ddim
from oracle.unet import resnet, timestep_embedding, transformer

GROUPS = 32


def _embed(sd, t, B):
    t = torch.as_tensor(t).reshape(-1).expand(B)
    e = timestep_embedding(t).to(sd["time_embedding.linear_1.weight"].dtype)
    e = F.linear(e, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    return F.linear(F.silu(e), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])


def _down(sd, prefix, h, emb, each_block=None):
    """The four down blocks under ``prefix``: the running tensor and the 11 outputs, per block through ``each_block(i, outs)``."""
    res = []
    for i in range(4):
        outs = []
        for j in range(2):
            h = resnet(sd, f"{prefix}.{i}.resnets.{j}.", h, emb)
            if i < 3:
                h = transformer(sd, f"{prefix}.{i}.attentions.{j}.", h)
            outs.append(h)
        if i < 3:
            h = F.conv2d(h, sd[f"{prefix}.{i}.downsamplers.0.conv.weight"], sd[f"{prefix}.{i}.downsamplers.0.conv.bias"],
                         stride=2, padding=1)
            outs.append(h)
        res += each_block(i, outs) if each_block else outs
    return h, res


def image_residuals(sd, image_half, timestep_img=None):
    """The 12 tensors the image branch adds to the skip connections."""
    emb_img = _embed(sd, 0 if timestep_img is None else timestep_img, image_half.shape[0])
    h = F.conv2d(image_half, sd["conv_in_img.weight"], sd["conv_in_img.bias"], padding=1)

    def adapt(i, outs):
        if f"adaptor_layers.{i}.weight" not in sd:
            return outs
        return [F.conv2d(o, sd[f"adaptor_layers.{i}.weight"], sd[f"adaptor_layers.{i}.bias"], padding=1) for o in outs]
    _, res = _down(sd, "down_blocks_additional", h, emb_img, adapt)
    return [h] + res


def sepenc_forward(sd, sample, timestep, timestep_img=None):
    """sample [B, 8, L, L] fp32 = [segmentation | image], timestep / timestep_img 0-d or [B] -> [B, 4, L, L]."""
    B = sample.shape[0]
    seg, img = sample.chunk(2, dim=1)
    extra = image_residuals(sd, img, timestep_img)
    emb = _embed(sd, timestep, B)
    h0 = F.conv2d(seg, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    h, res = _down(sd, "down_blocks", h0, emb)
    skips = [s + e for s, e in zip([h0] + res, extra)]
    assert len(skips) == 12

    h = resnet(sd, "mid_block.resnets.0.", h, emb)                 # (the un-summed running tensor)
    h = transformer(sd, "mid_block.attentions.0.", h)
    h = resnet(sd, "mid_block.resnets.1.", h, emb)
    for i in range(4):
        for j in range(3):
            h = resnet(sd, f"up_blocks.{i}.resnets.{j}.", torch.cat([h, skips.pop()], dim=1), emb)
            if i > 0:
                h = transformer(sd, f"up_blocks.{i}.attentions.{j}.", h)
        if i < 3:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    h = F.silu(F.group_norm(h, GROUPS, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], eps=1e-5))
    return F.conv2d(h, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def reference_loop(sd, sched_kw, noise, rgb, n=4):
    """latents after n DDIM steps from ``noise``; every step runs the whole forward, image branch included."""
    so = o_ddim.OracleDDIM(**sched_kw)
    so.set_timesteps_inference(n)
    latents = noise * so.init_noise_sigma
    for idx, t in enumerate(so.timesteps):
        eps = sepenc_forward(sd, torch.cat([latents, rgb], dim=1), t)
        prev, x0 = so.step(eps, t, latents)
        latents = x0 if idx == len(so.timesteps) - 1 else prev
    return latents


def plain_equivalent(sd):
    """The plain 8-channel state dict a separate-encoder one equals when its image branch adds zeros: the extra tensors
    dropped, conv_in zero-extended over the image half."""
    out = {k: v for k, v in sd.items()
           if not k.startswith(("conv_in_img.", "down_blocks_additional.", "adaptor_layers."))}
    w = sd["conv_in.weight"]
    out["conv_in.weight"] = torch.cat([w, torch.zeros_like(w)], dim=1)
    return out

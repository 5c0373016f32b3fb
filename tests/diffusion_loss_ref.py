"""Torch restatement of the forward half of the training step, in this project's own words: what csrc/loss.hip computes behind
the UNet output and what TrainerDiffusion.compute_loss / predict_sample / get_loss_weight_mask return.  Pinned to the reference's
own functions by tests/golden/diffusion_loss.npz (tests/golden/make_golden_loss.py runs them); the GPU tests compare the library
with this file and with that fixture.

Everything here is a chain of single torch elementwise ops (each rounded once, no fused multiply-add), so that CPU and GPU
give the same bits.  Square roots of the alpha table come from the caller (`sqrt_a`, `sqrt_b`: [T] fp32): torch's CPU `** 0.5`
may differ in the last bit between hosts, so the fixture carries the values it was made with.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

LOSS_KINDS = ("l1", "l2", "smooth_l1")


class StandIn(object):
    """The fixed stand-in for the epsilon network: a 1x1 channel mix plus t / 1000, written as separately rounded products and
    sums in a fixed order (a matmul would round differently on CPU and GPU).  `w` [4, Cin] fp32; `table` = arange(T) / 1000 is
    made once on the host and looked up, so that no device division is involved."""

    def __init__(self, w, n_train=1000, device="cpu"):
        self.w = [[float(v) for v in row] for row in torch.as_tensor(w, dtype=torch.float32)]
        self.table = (torch.arange(n_train, dtype=torch.float32) / 1000).to(device)
        self.calls = []

    def __call__(self, inputs, timesteps, encoder_hidden_states=None, timestep_img=None):
        self.calls.append((inputs, timesteps, encoder_hidden_states, timestep_img))
        x = inputs.float()
        outs = []
        for row in self.w:
            assert len(row) == x.shape[1], (len(row), x.shape)
            acc = x[:, 0] * row[0]
            for c in range(1, len(row)):
                acc = acc + x[:, c] * row[c]
            outs.append(acc)
        bias = self.table[torch.as_tensor(timesteps).to(self.table.device).long().reshape(-1)]
        out = torch.stack(outs, dim=1) + bias[:, None, None, None]
        return SimpleNamespace(sample=out.contiguous())


def per_sample(v, like):
    """[B] coefficients -> broadcastable against `like`"""
    return v.reshape(-1, *([1] * (like.dim() - 1)))


def add_noise(x0, noise, t, sqrt_a, sqrt_b):
    return per_sample(sqrt_a[t], x0) * x0 + per_sample(sqrt_b[t], x0) * noise


def remove_noise(noisy, eps, t, sqrt_a, sqrt_b):
    return (noisy - per_sample(sqrt_b[t], noisy) * eps) / per_sample(sqrt_a[t], noisy)


def element_loss(x, y, kind):
    d = x - y
    if kind == "l1":
        return d.abs()
    if kind == "l2":
        return d * d
    if kind == "smooth_l1":                      # beta = 1
        z = d.abs()
        return torch.where(z < 1, (z * 0.5) * z, z - 0.5)
    raise ValueError(kind)


def weighted_element_loss(prediction, target, kind, loss_mask=None, weights=None, t=None):
    """the element loss as the loss tail writes it: loss_fn, then * mask[:, None], then * weights[t]"""
    loss = element_loss(prediction.float(), target.float(), kind)
    if loss_mask is not None:
        loss = loss * loss_mask[:, None]
    if weights is not None:
        loss = loss * per_sample(weights[t], loss)
    return loss


def reduce_loss(elem, ohem_ratio=1.0):
    """fp64 value of the mean / of the mean of the k largest; (value, k)"""
    flat = elem.reshape(-1).double()
    if ohem_ratio < 1.0:
        k = int(ohem_ratio * flat.numel())
        return float(torch.topk(flat, k)[0].sum() / k), k
    return float(flat.sum() / flat.numel()), flat.numel()


def exact_sample_sums(elem):
    """[B] fp32: the exact sum of every sample's element losses, rounded once"""
    e = elem.detach().cpu().numpy().astype(np.float64)
    return np.asarray([np.float32(math.fsum(row.ravel().tolist())) for row in e], dtype=np.float32)


def pred_latents(prediction, noisy, t, sqrt_a, sqrt_b, prediction_type, paste_mask=None, paste_src=None, clamp=None):
    if prediction_type == "epsilon":
        out = remove_noise(noisy, prediction, t, sqrt_a, sqrt_b)
    elif prediction_type == "sample":
        out = prediction.clone()
    else:
        raise ValueError(prediction_type)
    if paste_mask is not None:
        out = torch.where(paste_mask, paste_src, out)
    if clamp is not None:
        out = torch.clamp(out, clamp[0], clamp[1])
    return out


def compute_loss(network, noise, t, noisy, rgb, loss_mask, kind, prediction_type, sqrt_a, sqrt_b, weights=None, latents=None,
                 original=None, paste_mask=None, condition=None, ohem_ratio=1.0, encoder_hidden_states=None, timestep_img=None):
    """(loss as a python float (fp64 reduction), element loss, pred_latents, prediction) - `network(inputs, t, ctx,
    timestep_img=...)` returns an object with `.sample`"""
    parts = [noisy, rgb] + ([condition] if condition is not None else [])
    prediction = network(torch.cat(parts, dim=1), t, encoder_hidden_states, timestep_img=timestep_img).sample
    target = noise if prediction_type == "epsilon" else (original if original is not None else latents)
    elem = weighted_element_loss(prediction, target, kind, loss_mask, weights, t)
    loss, _ = reduce_loss(elem, ohem_ratio)
    pl = pred_latents(prediction, noisy, t, sqrt_a, sqrt_b, prediction_type, paste_mask, original)
    return loss, elem, pl, prediction


def predict_sample(network, latents, rgb, noise, t, sqrt_a, sqrt_b, prediction_type):
    noisy = add_noise(latents, noise, t, sqrt_a, sqrt_b)
    inputs = noisy if rgb is None else torch.cat([noisy, rgb], dim=1)
    prediction = network(inputs, t, None).sample
    return pred_latents(prediction, noisy, t, sqrt_a, sqrt_b, prediction_type, clamp=(latents.min(), latents.max()))


def nearest_index(in_size, out_size):
    """source index of every output index of a nearest resize: fp32 scale, fp32 product, floor, clipped to the last pixel"""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, in_size - 1)


def loss_weight_mask(src, size, type_mask, ignore_label=0):
    """src [B,Hi,Wi] (targets, or the padding mask for 'padding') -> [B,h,w] fp32"""
    B, Hi, Wi = src.shape
    iy = torch.from_numpy(nearest_index(Hi, size[0]))
    ix = torch.from_numpy(nearest_index(Wi, size[1]))
    small = src.float()[:, iy][:, :, ix]
    if type_mask == "padding":
        return small
    if type_mask == "ignore":
        return (small != ignore_label).float()
    if type_mask == "counts":
        out = torch.zeros_like(small)
        for b in range(B):
            ids = small[b].long()
            counts = torch.bincount(ids.reshape(-1), minlength=256)
            w = 1.0 / counts[ids].float()
            out[b] = torch.where(small[b] == ignore_label, torch.zeros_like(w), w)
        return out
    return None

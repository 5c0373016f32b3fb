"""Shared by the tests of the seg-VAE encoder's backward: the configurations and shapes they run, seeded inputs, and the
reference - oracle.vae.encode_moments (which reads its channel counts from the state dict, so it serves the reduced configuration
too) under torch-CPU autograd in fp64, computed once per case and shared.  No GPU and no library here.

Metric and gate are vae_backward_ref's: per gradient tensor max|g - g64| / max|g64| <= 1e-3, in "fp32" and in "bf16x3"."""
import functools
from collections import OrderedDict

import torch

import vae_backward_ref as R
import vae_cases as V

BOUND = R.BOUND
MODES = R.MODES
metric = R.metric
CUS = R.CUS
# the real encoder and a reduced one: every level 32 or 64 channels wide, so the narrow tiles serve all of its layers
CONFIGS = {
    "seg": dict(V.SEG),
    "reduced": dict(V.SEG, block_out_channels=(32, 32, 64, 64), int_channels=64),
}
# (configuration, B, H): full-resolution maps 16^2 .. 40^2; the lowest level is 2^2 .. 5^2, off the power-of-two grid at 24 and 40
SHAPES = [("seg", 1, 16), ("seg", 2, 24), ("seg", 3, 40), ("seg", 2, 32), ("reduced", 2, 24)]
IN_MUL, IN_ADD = 2.0, -1.0                          # encode_inputs' 2 x - 1 on the bit planes


def schema(cfg):
    return R.schema(cfg)


@functools.lru_cache(maxsize=None)
def state_dict(name):
    from ldmseg_amd import weights
    cfg = CONFIGS[name]
    return weights.generate(schema(cfg), seed=11, norm_keys=("encoder.13.weight", "encoder.13.bias") + R.norm_keys(cfg))


def encoder_keys(cfg):
    return [k for k in schema(cfg) if k.startswith("encoder.")]


def conv_layers(cfg):
    """the nine convs in model order: (state-dict index, Ci, Co, stride, level) - level l runs on maps H / 2^l (its INPUT)"""
    boc = cfg["block_out_channels"]
    out = [(0, cfg["in_channels"], boc[0], 1, 0)]
    idx = 2
    for i in range(3):
        out.append((idx, boc[i], boc[i], 1, i))
        out.append((idx + 1, boc[i], boc[i + 1], 2, i))
        idx += 3
    out.append((idx, boc[3], cfg["int_channels"], 1, 3))
    out.append((idx + 4, cfg["int_channels"], 2 * cfg["latent_channels"], 1, 3))
    return out


def wgrad_descs(name, B, H):
    """every weight-gradient launch of one encode_backward call: (P of the OUTPUT map, N, C, taps, stride), storage widths"""
    up = lambda c: (c + 31) // 32 * 32
    out = []
    for _, ci, co, stride, level in conv_layers(CONFIGS[name]):
        side = H >> level
        so = (side - 1) // 2 + 1 if stride == 2 else side
        out.append((B * so * so, up(co), up(ci), 9, stride))
    return out


def inputs(name, B, H, seed=0):
    """(bit planes x [B,7,H,H] in {0, 1}, grad_moments [B,8,H/8,H/8]) seeded; the images of a batch differ"""
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(1000 * seed + 131 * B + H)
    x = (torch.rand(B, cfg["in_channels"], H, H, generator=g) < 0.5).float()
    gm = torch.randn(B, 2 * cfg["latent_channels"], H // 8, H // 8, generator=g)
    return x, gm


def autograd_grads(name, x, gm, dtype):
    """{key: gradient} of sum(encode_moments(2 x - 1) * gm) under torch-CPU autograd in `dtype`"""
    from oracle import vae as o_vae
    sd = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in state_dict(name).items() if k.startswith("encoder."))
    out = o_vae.encode_moments(sd, x.to(dtype) * IN_MUL + IN_ADD)
    keys = list(sd)
    gs = torch.autograd.grad(out, [sd[k] for k in keys], grad_outputs=gm.to(dtype))
    return {k: g.detach() for k, g in zip(keys, gs)}


@functools.lru_cache(maxsize=None)
def reference(name, B, H, seed=0):
    """fp64 gradients of the case, computed once and shared (do not modify)"""
    x, gm = inputs(name, B, H, seed)
    return autograd_grads(name, x, gm, torch.float64)


@functools.lru_cache(maxsize=None)
def reference_fp32(name, B, H, seed=0):
    """torch's own fp32 CPU autograd on the same inputs: its error against fp64 is the reference's own error"""
    x, gm = inputs(name, B, H, seed)
    return autograd_grads(name, x, gm, torch.float32)


def tensor_class(key):
    if key.startswith("encoder.13."):
        return "norm"
    return "weight" if key.endswith("weight") else "bias"


def wgrad_plan_ex(lib, P, N, C, taps, stride, x3=0, cus=CUS):
    """(code, line, fields, executed MACs per pixel) of ldmseg_op_wgrad_plan_ex"""
    import ctypes
    buf = ctypes.create_string_buffer(256)
    macs = ctypes.c_int64(0)
    code = lib.ldmseg_op_wgrad_plan_ex(P, N, C, taps, x3, stride, cus, buf, 256, ctypes.byref(macs))
    line = buf.value.decode()
    fields = {}
    if code == 0:
        for tok in line.split()[1:]:
            k, v = tok.split("=")
            fields[k] = v
    return code, line, fields, macs.value


def conv_case(B, Ci, Co, H, W, stride):
    """(x, w, dy, and the fp64 gradients of x, w, b) of F.conv2d(x, w, b, stride, padding=1) under torch-CPU autograd, seeded"""
    import zlib
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(zlib.crc32(repr(("enc-conv", B, Ci, Co, H, W, stride)).encode()) & 0xffffff)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    b = torch.randn(Co, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xd, wd, bd, stride=stride, padding=1)
    dy = torch.randn(y.shape, generator=g)
    rx, rw, rb = torch.autograd.grad(y, [xd, wd, bd], dy.double())
    return x, w, dy, rx, rw, rb


def posterior_case(B=2, l=6, seed=5):
    """moments whose logvar half holds values inside, outside and exactly on the clamp bounds [-30, 20]; noise; grad_z"""
    g = torch.Generator().manual_seed(seed)
    mom = torch.randn(B, 8, l, l, generator=g)
    lv = mom[:, 4:] * 4.0
    flat = lv.reshape(-1)
    flat[0::7] = -30.0
    flat[1::7] = 20.0
    flat[2::7] = -31.5
    flat[3::7] = 20.5
    flat[4::7] = 12.0                                # a large std
    mom[:, 4:] = flat.view_as(lv)
    noise = torch.randn(B, 4, l, l, generator=g)
    gz = torch.randn(B, 4, l, l, generator=g)
    return mom, noise, gz


def posterior_reference(mom, noise, gz, scale=1.0):
    m = mom.double().clone().requires_grad_(True)
    mean, logvar = m[:, :4], m[:, 4:]
    z = mean + (torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise.double() if noise is not None else 0.0)
    g, = torch.autograd.grad(z * scale, [m], gz.double())
    return g

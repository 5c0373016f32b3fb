"""Shared by the tests of the seg-VAE decoder's backward: the configurations and shapes they run, seeded inputs, and the
reference - the decoder restated with torch-CPU ops (for the real configuration: oracle.vae.decode itself) under torch autograd in
fp64, computed once per case and shared.  No GPU and no library here.

Metric, per gradient tensor: max|g - g64| / max|g64|; the gate is the project's bound for its fp32-storage modes, 1e-3, in "fp32"
and in "bf16x3"."""
import functools
from collections import OrderedDict

import torch
import torch.nn.functional as F

import vae_cases as V

BOUND = 1e-3
MODES = ("fp32", "bf16x3")
# the real decoder (vae_cases.SEG) and a reduced one: three upscalers, Ci != Co in the first transposed conv, 16 logit channels (below a
# K tile of the data gradient and below a 16-row MFMA tile border of the weight gradient's 32-column storage)
CONFIGS = {
    "seg": dict(V.SEG),
    "reduced": dict(V.SEG, num_upscalers=3, int_channels=64, upscale_channels=128, out_channels=16),
}
# (configuration, B, L): logits maps 8^2, 12^2, 20^2 - pixel counts 64, 288, 1200 leave a partial pixel tile in every kernel, odd rows
# and columns come off the power-of-two grid, B >= 2 with different images, borders a large share of the map
SHAPES = [("seg", 1, 2), ("seg", 2, 3), ("seg", 3, 5), ("reduced", 2, 3)]
# the smallest (B <= 3, L) whose last conv's weight gradient the chooser cuts into more than one pixel slice
# (tests/test_wgrad_plan_cpu.py::test_multi_slice_case_is_the_smallest keeps this true)
MULTI_SLICE = ("seg", 2, 4)
ALL_SHAPES = SHAPES + [MULTI_SLICE]
CUS = 256                                           # an MI355X


def schema(cfg):
    from ldmseg_amd import weights
    return weights.vae_schema(cfg["in_channels"], cfg["int_channels"], cfg["out_channels"], cfg["block_out_channels"],
                              cfg["latent_channels"], 2, cfg["num_upscalers"], cfg["upscale_channels"])


def norm_keys(cfg):
    """LayerNorm2d and GroupNorm keys of the decoder (+ the encoder's GroupNorm): gamma = 1 + noise, beta = noise"""
    U = cfg["num_upscalers"]
    idx = [3 + 3 * i for i in range(U)] + [2 + 3 * U]
    return tuple(f"decoder.{i}.{p}" for i in idx for p in ("weight", "bias")) + ("encoder.13.weight", "encoder.13.bias")


@functools.lru_cache(maxsize=None)
def state_dict(name):
    from ldmseg_amd import weights
    cfg = CONFIGS[name]
    return weights.generate(schema(cfg), seed=7, norm_keys=norm_keys(cfg))


def decoder_keys(cfg):
    return [k for k in schema(cfg) if k.startswith("decoder.")]


def layer_plan(cfg):
    """decoder indices: (conv_in, [(convT, LayerNorm)], GroupNorm, conv_out)"""
    U = cfg["num_upscalers"]
    return 0, [(2 + 3 * i, 3 + 3 * i) for i in range(U)], 2 + 3 * U, 4 + 3 * U


def decode(sd, z, cfg):
    """vae.py:123-172 + :267-271 with interpolate=False, for any num_upscalers (oracle.vae.decode restates the two-upscaler one;
    tests/test_vae_backward_cpu.py holds the two equal)"""
    from oracle.vae import layernorm2d
    c_in, ups, gn, c_out = layer_plan(cfg)
    h = F.conv2d(z, sd[f"decoder.{c_in}.weight"], sd[f"decoder.{c_in}.bias"], padding=1)
    for ct, ln in ups:
        h = F.conv_transpose2d(h, sd[f"decoder.{ct}.weight"], sd[f"decoder.{ct}.bias"], stride=2)
        h = F.silu(layernorm2d(h, sd[f"decoder.{ln}.weight"], sd[f"decoder.{ln}.bias"]))
    h = F.silu(F.group_norm(h, 32, sd[f"decoder.{gn}.weight"], sd[f"decoder.{gn}.bias"], eps=1e-5))
    return F.conv2d(h, sd[f"decoder.{c_out}.weight"], sd[f"decoder.{c_out}.bias"], padding=1)


def inputs(name, B, L, seed=0):
    """(z [B,4,L,L], grad_logits [B,Co,4L * 2^(U-2)...]) seeded; the images of a batch differ"""
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + L)
    z = torch.randn(B, cfg["latent_channels"], L, L, generator=g) * 1.5
    up = 2 ** cfg["num_upscalers"] * L
    gl = torch.randn(B, cfg["out_channels"], up, up, generator=g)
    return z, gl


def autograd_grads(name, z, gl, dtype, z_scale=1.0):
    """{key: gradient, "z": gradient} of sum(decode(z * z_scale) * gl) under torch-CPU autograd in `dtype`"""
    cfg = CONFIGS[name]
    sd = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in state_dict(name).items() if k.startswith("decoder."))
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    if name == "seg" and z_scale == 1.0:
        from oracle import vae as o_vae
        out = o_vae.decode(sd, zz, interpolate=False)
    else:
        out = decode(sd, zz * z_scale, cfg)
    keys = list(sd)
    gs = torch.autograd.grad(out, [zz] + [sd[k] for k in keys], grad_outputs=gl.to(dtype))
    res = {"z": gs[0].detach()}
    res.update({k: g.detach() for k, g in zip(keys, gs[1:])})
    return res


@functools.lru_cache(maxsize=None)
def reference(name, B, L, seed=0):
    """fp64 gradients of the case, computed once and shared (do not modify)"""
    z, gl = inputs(name, B, L, seed)
    return autograd_grads(name, z, gl, torch.float64)


@functools.lru_cache(maxsize=None)
def reference_fp32(name, B, L, seed=0):
    """torch's own fp32 CPU autograd on the same inputs: its error against fp64 is the reference's own error"""
    z, gl = inputs(name, B, L, seed)
    return autograd_grads(name, z, gl, torch.float32)


def metric(g, g64):
    g = torch.as_tensor(g).detach().double().cpu()
    g64 = g64.double()
    return float((g - g64).abs().max() / g64.abs().max().clamp_min(1e-300))


def tensor_class(key):
    """class of a gradient tensor for the tables of DESIGN 8.6"""
    if key == "z":
        return "latents"
    return "weight" if key.endswith("weight") and key not in _NORM else ("norm" if key in _NORM else "bias")


_NORM = set()
for _c in CONFIGS.values():
    _NORM |= set(k for k in norm_keys(_c) if k.startswith("decoder."))


def last_conv_wgrad_desc(name, B, L):
    """(P, N, C, taps) of the last conv's weight-gradient launch: dY stored on rup(Co, 32) columns, X = the GroupNorm output"""
    cfg = CONFIGS[name]
    side = 2 ** cfg["num_upscalers"] * L
    return B * side * side, (cfg["out_channels"] + 31) // 32 * 32, cfg["upscale_channels"], 9


def wgrad_descs(name, B, L):
    """every weight-gradient launch of one decode_backward call: (P, N, C, taps)"""
    cfg = CONFIGS[name]
    out = [(B * L * L, cfg["int_channels"], 32, 9)]
    side, cin = L, cfg["int_channels"]
    for _ in range(cfg["num_upscalers"]):
        out.append((B * side * side, 4 * cfg["upscale_channels"], cin, 1))
        side, cin = 2 * side, cfg["upscale_channels"]
    out.append(last_conv_wgrad_desc(name, B, L))
    return out


def wgrad_plan(lib, P, N, C, taps, x3=0, cus=CUS):
    import ctypes
    buf = ctypes.create_string_buffer(256)
    code = lib.ldmseg_op_wgrad_plan(P, N, C, taps, x3, cus, buf, 256)
    line = buf.value.decode()
    fields = {}
    if code == 0:
        for tok in line.split()[1:]:
            k, v = tok.split("=")
            fields[k] = v
    return code, line, fields


# ---- three SGD steps on a fixed batch with a smooth loss, F.cross_entropy(decode(z), targets): the fp64 restatement's losses
SGD_SHAPE = ("seg", 2, 3)
SGD_LR = 0.2                                       # tests/test_vae_backward_cpu.py: the restatement's loss falls at each step
SGD_STEPS = 3


def sgd_inputs():
    name, B, L = SGD_SHAPE
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(4242)
    z = torch.randn(B, cfg["latent_channels"], L, L, generator=g) * 1.5
    side = 2 ** cfg["num_upscalers"] * L
    targets = torch.randint(0, cfg["out_channels"], (B, side, side), generator=g)
    return z, targets


@functools.lru_cache(maxsize=None)
def sgd_reference():
    """losses before each of the SGD_STEPS steps and after the last, fp64 restatement with torch.optim.SGD"""
    name, _, _ = SGD_SHAPE
    cfg = CONFIGS[name]
    z, targets = sgd_inputs()
    sd = OrderedDict((k, v.detach().double().clone().requires_grad_(True)) for k, v in state_dict(name).items() if k.startswith("decoder."))
    opt = torch.optim.SGD(list(sd.values()), lr=SGD_LR)
    losses = []
    for _ in range(SGD_STEPS):
        opt.zero_grad()
        loss = F.cross_entropy(decode(sd, z.double(), cfg), targets)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(F.cross_entropy(decode(sd, z.double(), cfg), targets)))
    return losses

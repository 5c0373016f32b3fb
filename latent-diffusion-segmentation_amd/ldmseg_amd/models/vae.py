"""Segmentation VAE with the reference's call surface, executed by the gfx950 library.

Stands behind /root/reference/ldmseg/models/vae.py::GeneralVAESeg for the
default (gaussian, num_mid_blocks=0) configuration of base.yaml:14-33:

    logits = vae_semseg.decode(z)                           # trainers_ldm_cond.py:422
    z = vae_semseg.encode(x).latent_dist.mode() / .sample() # trainers_ldm_cond.py:371-375
"""
import ctypes as C
from collections import OrderedDict
from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..utils import EncoderOutput, VAEOutput
from ..weights import vae_schema


class DiagonalGaussianDistribution(object):
    """vae.py:370-424 on device moments [B, 8, l, l] (mean | logvar)."""

    def __init__(self, parameters: torch.Tensor, clamp_output: bool = False, act_fn: str = 'none'):
        if clamp_output or act_fn != 'none':
            raise NotImplementedError("only clamp_output=False / act_fn='none' (base.yaml:25-26)")
        self.parameters = parameters
        self.clamp_output = clamp_output
        self.act_fn = act_fn

    def _posterior(self, noise):
        p = self.parameters
        B, _, l, _ = p.shape
        out = torch.empty((B, 4, l, l), device=p.device, dtype=torch.float32)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().ldmseg_vae_posterior(_lib.ptr(p), _lib.ptr(noise), 1.0, B, l, _lib.ptr(out),
                                                       _lib.stream_ptr(p.device)), "ldmseg_vae_posterior")
        return out

    @property
    def mean(self):
        return self.parameters[:, :4]

    @property
    def logvar(self):
        return torch.clamp(self.parameters[:, 4:], -30.0, 20.0)

    def _draw(self, noise):
        """mode() (noise None) / sample(): with grad mode on and `parameters` requiring grad the latents are differentiable with
        respect to them (once: ldmseg_vae_posterior_backward; the noise is saved), the values are those of the no-grad path"""
        p = self.parameters
        if torch.is_grad_enabled() and isinstance(p, torch.Tensor) and p.requires_grad:
            return _PosteriorFunction.apply(self, _lib.require_cuda_f32(p, "moments"), noise)
        return self._posterior(noise)

    def mode(self):
        return self._draw(None)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        p = self.parameters
        shape = (p.shape[0], 4, p.shape[2], p.shape[3])
        noise = torch.randn(shape, generator=generator, device=p.device, dtype=p.dtype)
        return self._draw(noise)

    def kl(self, return_mean: bool = False):
        """:416-417: 0.5 * sum(mean^2 + var - 1 - logvar) per image, [B] on the device (ldmseg_gaussian_kl; fp64 sums).  With
        return_mean the pair (per image [B], batch mean 0-d) of the same call.  With grad mode on and `parameters` requiring
        grad the results are differentiable with respect to them (once: ldmseg_gaussian_kl_backward)."""
        if torch.is_grad_enabled() and isinstance(self.parameters, torch.Tensor) and self.parameters.requires_grad:
            per, mean = _GaussianKLFunction.apply(_lib.require_cuda_f32(self.parameters, "moments"))
            return (per, mean) if return_mean else per
        with torch.no_grad():
            return self._kl_forward(_lib.require_cuda_f32(self.parameters, "moments"), return_mean)

    @staticmethod
    def _kl_forward(p: torch.Tensor, return_mean: bool):
        B, C2 = p.shape[0], p.shape[1]
        per = torch.empty(B, device=p.device, dtype=torch.float32)
        mean = torch.empty(1, device=p.device, dtype=torch.float32) if return_mean else None
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().ldmseg_gaussian_kl(_lib.ptr(p), B, C2 // 2, p[0, 0].numel(), _lib.ptr(per), _lib.ptr(mean),
                                                     _lib.stream_ptr(p.device)), "ldmseg_gaussian_kl")
        return (per, mean[0]) if return_mean else per


class _GaussianKLFunction(torch.autograd.Function):
    """(kl per image [B], batch mean) of fp32 contiguous moments with a backward to them: d kl_b / d mean = mean,
    d kl_b / d logvar = 0.5 * (exp(logvar) - 1) where the clamp passes gradient; the batch mean adds grad / B per image."""

    @staticmethod
    def forward(ctx, p):
        per, mean = DiagonalGaussianDistribution._kl_forward(p, True)
        ctx.save_for_backward(p)
        ctx.set_materialize_grads(False)
        return per, mean.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_per, grad_mean):
        p, = ctx.saved_tensors
        if grad_per is None and grad_mean is None:
            return None
        B, C2 = p.shape[0], p.shape[1]
        g = torch.zeros(B, device=p.device, dtype=torch.float32)
        if grad_per is not None:
            g = g + grad_per.to(device=p.device, dtype=torch.float32)
        if grad_mean is not None:
            g = g + grad_mean.to(device=p.device, dtype=torch.float32) / B
        g = g.contiguous()
        grad = torch.empty_like(p)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().ldmseg_gaussian_kl_backward(_lib.ptr(p), B, C2 // 2, p[0, 0].numel(), _lib.ptr(g), _lib.ptr(grad),
                                                              _lib.stream_ptr(p.device)), "ldmseg_gaussian_kl_backward")
        return grad


class _PosteriorFunction(torch.autograd.Function):
    """z = mean + exp(0.5 clamp(logvar, -30, 20)) noise of fp32 contiguous moments with a backward to them: d mean = dz,
    d logvar = dz noise std / 2 where the clamp passes gradient (bounds included), zeros elsewhere and for mode()."""

    @staticmethod
    def forward(ctx, dist, p, noise):
        with torch.no_grad():
            out = DiagonalGaussianDistribution(p)._posterior(noise)
        ctx.noise = noise
        ctx.save_for_backward(p)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_z):
        p, = ctx.saved_tensors
        if grad_z is None:
            return None, None, None
        g = grad_z.to(device=p.device, dtype=torch.float32).contiguous()
        B, _, l, _ = p.shape
        grad = torch.empty_like(p)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().ldmseg_vae_posterior_backward(_lib.ptr(p), _lib.ptr(ctx.noise), 1.0, B, l, _lib.ptr(g), _lib.ptr(grad),
                                                                _lib.stream_ptr(p.device)), "ldmseg_vae_posterior_backward")
        return None, grad, None


def _name_arrays(tensors):
    """(n, names, ptrs, numels) of a {key: tensor} dict as the C ABI takes them (arrays of one dummy element when empty)"""
    n = len(tensors)
    names = (C.c_char_p * max(n, 1))(*[k.encode() for k in tensors])
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in tensors.values()])
    numels = (C.c_int64 * max(n, 1))(*[t.numel() for t in tensors.values()])
    return n, names, ptrs, numels


class _EncodeFunction(torch.autograd.Function):
    """encode_moments(x, in_mul, in_add) with a backward to the encoder parameters: forward is the no-grad path's own
    ldmseg_vae_encode call, backward one ldmseg_vae_encode_backward call (stateless: the library runs the encoder forward again
    inside it) that returns the parameter gradients autograd asks for.  The input is data: it gets no gradient."""

    @staticmethod
    def forward(ctx, vae, in_mul, in_add, x, *params):
        out = vae._encode_call(x, in_mul, in_add)
        ctx.vae, ctx.in_mul, ctx.in_add = vae, in_mul, in_add
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        vae = ctx.vae
        x, = ctx.saved_tensors
        need = ctx.needs_input_grad
        keys = list(vae._enc_params)
        if grad is None:
            return (None,) * len(need)
        vae._check_encoder_fresh()
        g = grad.to(device=x.device, dtype=torch.float32).contiguous()
        B, _, H, _ = x.shape
        grads = {k: torch.empty_like(vae._enc_params[k]) for i, k in enumerate(keys) if need[4 + i]}
        n, names, ptrs, numels = _name_arrays(grads)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_vae_encode_backward(vae._h, _lib.ptr(x), float(ctx.in_mul), float(ctx.in_add), B, H, _lib.ptr(g),
                                                             n, names, ptrs, numels, _lib.stream_ptr(x.device)),
                       "ldmseg_vae_encode_backward")
        return (None, None, None, None) + tuple(grads.get(k) for k in keys)


class _DecodeFunction(torch.autograd.Function):
    """decode(z, interpolate=False, z_scale) with a backward to the latents and the decoder parameters: forward is the no-grad
    path's own ldmseg_vae_decode call, backward one ldmseg_vae_decode_backward call (stateless: the library runs the decoder
    forward again inside it) that returns grad_z and the parameter gradients autograd asks for."""

    @staticmethod
    def forward(ctx, vae, z_scale, z, *params):
        out = vae._decode_call(z, 0, z_scale)
        ctx.vae, ctx.z_scale = vae, z_scale
        ctx.save_for_backward(z)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        vae = ctx.vae
        z, = ctx.saved_tensors
        need = ctx.needs_input_grad
        keys = list(vae._dec_params) if len(need) > 3 else []
        if grad is None:
            return (None,) * len(need)
        vae._check_decoder_fresh()
        g = grad.to(device=z.device, dtype=torch.float32).contiguous()
        B, _, L, _ = z.shape
        grad_z = torch.empty_like(z) if need[2] else None
        grads = {k: torch.empty_like(vae._dec_params[k]) for i, k in enumerate(keys) if need[3 + i]}
        n = len(grads)
        names = (C.c_char_p * max(n, 1))(*[k.encode() for k in grads])
        ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in grads.values()])
        numels = (C.c_int64 * max(n, 1))(*[t.numel() for t in grads.values()])
        with torch.cuda.device(z.device):
            _lib.check(_lib.lib().ldmseg_vae_decode_backward(vae._h, _lib.ptr(z), float(ctx.z_scale), B, L, _lib.ptr(g), _lib.ptr(grad_z),
                                                             n, names, ptrs, numels, _lib.stream_ptr(z.device)),
                       "ldmseg_vae_decode_backward")
        return (None, None, grad_z) + tuple(grads.get(k) for k in keys)


class GeneralVAESeg(object):
    def __init__(self, state_dict, in_channels: int = 7, int_channels: int = 256, out_channels: int = 128,
                 block_out_channels: Tuple[int] = (32, 64, 128, 256), latent_channels: int = 4,
                 norm_num_groups: int = 32, scaling_factor: float = 0.18215, num_mid_blocks: int = 0,
                 num_latents: int = 2, num_upscalers: int = 2, upscale_channels: int = 256,
                 parametrization: str = 'gaussian', act_fn: str = 'none', clamp_output: bool = False,
                 device: Union[str, torch.device] = "cuda:0", compute_dtype="bf16", **unused):
        if parametrization != 'gaussian' or num_mid_blocks != 0 or len(block_out_channels) != 4:
            raise NotImplementedError("only the default gaussian seg-VAE without mid blocks is built")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GeneralVAESeg needs an MI355X device (no CPU fallback)")
        self.scaling_factor = scaling_factor
        self.downsample_factor = 2 ** (len(block_out_channels) - 1)
        self.interpolation_factor = self.downsample_factor // (2 ** num_upscalers)
        if self.interpolation_factor not in (1, 2):
            raise NotImplementedError("interpolation factor must be 1 or 2")
        self.parametrization = parametrization
        self.num_latents = num_latents
        self.act_fn = act_fn
        self.clamp_output = clamp_output
        self.out_channels = out_channels
        self.dtype = torch.float32
        schema = vae_schema(in_channels, int_channels, out_channels, block_out_channels, latent_channels,
                            num_latents, num_upscalers, upscale_channels)
        state_dict = {k.replace('module.', ''): v for k, v in state_dict.items()}   # vae.py:119
        missing = [k for k in schema if k not in state_dict]
        if missing:
            raise KeyError(f"state dict lacks seg-VAE tensors, e.g. {missing[:3]}")
        cd = {"bf16": _lib.BF16, torch.bfloat16: _lib.BF16, "fp32": _lib.F32, torch.float32: _lib.F32,
              "float32": _lib.F32, "bfloat16": _lib.BF16, "bf16x3": _lib.BF16X3}[compute_dtype]
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cfg = _lib.VAECfg(in_channels, int_channels, out_channels, latent_channels, num_latents, num_upscalers,
                          upscale_channels, norm_num_groups, (C.c_int32 * 4)(*block_out_channels), cd, idx)
        n, names, ptrs, numels, keep = _lib.weight_arrays(state_dict, self.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.lib().ldmseg_vae_create(C.byref(cfg), n, names, ptrs, numels, C.byref(handle)),
                       "ldmseg_vae_create")
        del keep
        self._h = handle
        self._in_channels = in_channels
        self._upscale = 2 ** num_upscalers
        self._bf16 = cd == _lib.BF16
        # the decoder tensors the object was built from, kept on the device (decoder_parameters() makes leaves of them)
        self._dec_sd = OrderedDict((k, state_dict[k].detach().to(device=self.device, dtype=torch.float32).clone().contiguous())
                                   for k in schema if k.startswith("decoder."))
        self._dec_params = None
        self._dec_versions = None
        # ... and the encoder's (encoder_parameters())
        self._enc_sd = OrderedDict((k, state_dict[k].detach().to(device=self.device, dtype=torch.float32).clone().contiguous())
                                   for k in schema if k.startswith("encoder."))
        self._enc_params = None
        self._enc_versions = None

    @property
    def num_parameters(self) -> int:
        return int(_lib.lib().ldmseg_vae_num_params(self._h))

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().ldmseg_vae_destroy(h)
            except Exception:
                pass
            self._h = None

    def encode_moments(self, semseg: torch.Tensor, in_mul: float = 1.0, in_add: float = 0.0) -> torch.Tensor:
        """Moments [B,8,H/8,H/8] of semseg * in_mul + in_add.  With grad mode on, once `encoder_parameters()` has been called and a
        tensor of it requires grad, the result carries a graph to them (once differentiable): the values are bitwise those of the
        no-grad path, the backward is one ldmseg_vae_encode_backward call.  bf16 objects raise NotImplementedError then."""
        x = _lib.require_cuda_f32(semseg, "semseg")
        B, Cin, H, W = x.shape
        if Cin != self._in_channels or H != W:
            raise ValueError(f"expected [B,{self._in_channels},H,H], got {tuple(x.shape)}")
        if torch.is_grad_enabled() and self._enc_params is not None:
            params = list(self._enc_params.values())
            if any(p.requires_grad for p in params):
                if self._bf16:
                    raise NotImplementedError("the encoder backward needs an fp32-storage object (compute_dtype 'fp32' or 'bf16x3')")
                self._check_encoder_fresh()
                return _EncodeFunction.apply(self, float(in_mul), float(in_add), x, *params)
        return self._encode_call(x, in_mul, in_add)

    def _encode_call(self, x, in_mul, in_add):
        B, _, H, _ = x.shape
        l = H // self.downsample_factor
        mom = torch.empty((B, 8, l, l), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_vae_encode(self._h, _lib.ptr(x), in_mul, in_add, B, H, _lib.ptr(mom),
                                                    _lib.stream_ptr(x.device)), "ldmseg_vae_encode")
        return mom

    def encode(self, semseg: torch.Tensor) -> EncoderOutput:
        return EncoderOutput(latent_dist=DiagonalGaussianDistribution(self.encode_moments(semseg)))

    def encoder_parameters(self):
        """Ordered dict: reference key (encoder.0.weight ...) -> fp32 leaf tensor on the device with requires_grad=True, holding
        the encoder tensors of the state dict the object was built from.  Once this has been called, `encode_moments` / `encode` /
        `forward` under grad mode carry the encoder's graph to these tensors; after changing them in place (an optimiser step) call
        `refresh_encoder()` (or `refresh()`) so that the handle computes with the new values."""
        if self._enc_params is None:
            self._enc_params = OrderedDict((k, v.requires_grad_(True)) for k, v in self._enc_sd.items())
            self._enc_versions = {k: v._version for k, v in self._enc_params.items()}
        return self._enc_params

    def refresh_encoder(self):
        """`refresh_decoder()` for the encoder's tensors (ldmseg_vae_load_encoder: nothing is allocated)."""
        params = self.encoder_parameters()
        ts = OrderedDict((k, p.detach()) for k, p in params.items())
        n, names, ptrs, numels = _name_arrays(ts)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ldmseg_vae_load_encoder(self._h, n, names, ptrs, numels, _lib.stream_ptr(self.device)),
                       "ldmseg_vae_load_encoder")
        self._enc_versions = {k: v._version for k, v in params.items()}

    def _check_encoder_fresh(self):
        if self._enc_params is None:
            return
        stale = [k for k, v in self._enc_params.items() if v._version != self._enc_versions[k]]
        if stale:
            raise RuntimeError(f"encoder parameter {stale[0]} was modified in place since the last refresh_encoder(): the handle "
                               "would compute with stale weights; call refresh_encoder() after the optimiser step")

    def parameters(self):
        """The 34 leaves of `encoder_parameters()` then `decoder_parameters()`, for `clip_grad_norm_` and an optimiser."""
        return list(self.encoder_parameters().values()) + list(self.decoder_parameters().values())

    def refresh(self):
        """`refresh_encoder()` and `refresh_decoder()`: after an optimiser step on `parameters()`."""
        self.refresh_encoder()
        self.refresh_decoder()

    def state_dict(self):
        """Ordered dict of every schema key (encoder.0.weight ... decoder.N.bias, the reference's names without `module.`) -> a CPU
        fp32 clone of the tensor's CURRENT values: those of `parameters()`, optimiser steps included.  What `TrainerAE.save` writes
        as 'vae' and `GeneralVAESeg(state_dict)` / `load_state_dict` take back."""
        both = list(self._enc_sd.items()) + list(self._dec_sd.items())
        return OrderedDict((k, v.detach().to("cpu", copy=True)) for k, v in both)

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Copies `state_dict` (every schema key, `module.` prefixes allowed, shapes as built) into the object's own tensors - the
        leaves of `parameters()` stay the same objects, so an optimiser over them stays valid - and repacks them into the handle as `refresh()`
        does: every entry then computes with the new values, bitwise as an object built from that state dict."""
        sd = {k.replace('module.', ''): v for k, v in state_dict.items()}
        both = list(self._enc_sd.items()) + list(self._dec_sd.items())
        missing = [k for k, _ in both if k not in sd]
        if missing:
            raise KeyError(f"state dict lacks seg-VAE tensors, e.g. {missing[:3]}")
        for k, t in both:
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != expected {tuple(t.shape)}")
        for k, t in both:
            t.copy_(sd[k].detach().to(device=self.device, dtype=torch.float32))
        # refresh() without making leaves of the tensors (an object that never asked for its parameters keeps none)
        for entry, part in (("ldmseg_vae_load_encoder", self._enc_sd), ("ldmseg_vae_load_decoder", self._dec_sd)):
            n, names, ptrs, numels = _name_arrays(OrderedDict((k, v.detach()) for k, v in part.items()))
            with torch.cuda.device(self.device):
                _lib.check(getattr(_lib.lib(), entry)(self._h, n, names, ptrs, numels, _lib.stream_ptr(self.device)), entry)
        if self._enc_params is not None:
            self._enc_versions = {k: v._version for k, v in self._enc_params.items()}
        if self._dec_params is not None:
            self._dec_versions = {k: v._version for k, v in self._dec_params.items()}

    def decoder_parameters(self):
        """Ordered dict: reference key (decoder.0.weight ...) -> fp32 leaf tensor on the device with requires_grad=True, holding
        the decoder tensors of the state dict the object was built from.  Once this has been called, `decode` / `forward` under
        grad mode carry the decoder's graph to these tensors; after changing them in place (an optimiser step) call
        `refresh_decoder()` so that the handle computes with the new values."""
        if self._dec_params is None:
            self._dec_params = OrderedDict((k, v.requires_grad_(True)) for k, v in self._dec_sd.items())
            self._dec_versions = {k: v._version for k, v in self._dec_params.items()}
        return self._dec_params

    def refresh_decoder(self):
        """Repacks the current values of `decoder_parameters()` into the handle (ldmseg_vae_load_decoder: nothing is allocated):
        afterwards every entry of the object computes with them, bitwise as an object built from the updated state dict."""
        params = self.decoder_parameters()
        n = len(params)
        ts = [p.detach() for p in params.values()]
        names = (C.c_char_p * n)(*[k.encode() for k in params])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        numels = (C.c_int64 * n)(*[t.numel() for t in ts])
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ldmseg_vae_load_decoder(self._h, n, names, ptrs, numels, _lib.stream_ptr(self.device)),
                       "ldmseg_vae_load_decoder")
        self._dec_versions = {k: v._version for k, v in params.items()}

    def _check_decoder_fresh(self):
        if self._dec_params is None:
            return
        stale = [k for k, v in self._dec_params.items() if v._version != self._dec_versions[k]]
        if stale:
            raise RuntimeError(f"decoder parameter {stale[0]} was modified in place since the last refresh_decoder(): the handle "
                               "would compute with stale weights; call refresh_decoder() after the optimiser step")

    def _decode_call(self, z, interp, z_scale):
        B, _, L, _ = z.shape
        up = self._upscale * L * (2 if interp else 1)
        out = torch.empty((B, self.out_channels, up, up), device=z.device, dtype=torch.float32)
        with torch.cuda.device(z.device):
            _lib.check(_lib.lib().ldmseg_vae_decode(self._h, _lib.ptr(z), float(z_scale), B, L, interp, _lib.ptr(out),
                                                    _lib.stream_ptr(z.device)), "ldmseg_vae_decode")
        return out

    def decode(self, z: torch.Tensor, interpolate: bool = True, z_scale: float = 1.0) -> torch.Tensor:
        """vae.py:267-271.  With grad mode on and `z` or a tensor of `decoder_parameters()` requiring grad, the result carries a
        graph (once differentiable): the values are bitwise those of the no-grad path, the backward is one
        ldmseg_vae_decode_backward call.  The graph covers decode(interpolate=False); with interpolate=True torch's own
        F.interpolate (bilinear, align_corners=False) is applied on top, so torch differentiates the resize.  bf16 objects raise
        NotImplementedError when a graph is requested (the backward needs fp32 storage: "fp32" or "bf16x3")."""
        z = _lib.require_cuda_f32(z, "z")
        if torch.is_grad_enabled():
            params = [] if self._dec_params is None else list(self._dec_params.values())
            if z.requires_grad or any(p.requires_grad for p in params):
                if self._bf16:
                    raise NotImplementedError("the decoder backward needs an fp32-storage object (compute_dtype 'fp32' or 'bf16x3')")
                self._check_decoder_fresh()
                out = _DecodeFunction.apply(self, float(z_scale), z, *params)
                if interpolate and self.interpolation_factor == 2:
                    out = torch.nn.functional.interpolate(out, scale_factor=2, mode="bilinear", align_corners=False)
                return out
        B, _, L, _ = z.shape
        up = self._upscale * L * (self.interpolation_factor if interpolate else 1)
        interp = 1 if (interpolate and self.interpolation_factor == 2) else 0
        out = torch.empty((B, self.out_channels, up, up), device=z.device, dtype=torch.float32)
        with torch.cuda.device(z.device):
            _lib.check(_lib.lib().ldmseg_vae_decode(self._h, _lib.ptr(z), float(z_scale), B, L, interp, _lib.ptr(out),
                                                    _lib.stream_ptr(z.device)), "ldmseg_vae_decode")
        return out

    def decode_argmax(self, z: torch.Tensor, z_scale: float = 1.0, mask_th: Optional[float] = None,
                      ignore_label: int = 0, return_prob: bool = False):
        """Fused decode -> bilinear x2 -> argmax (+ max-softmax threshold): predictions [B,8L,8L] int64."""
        z = _lib.require_cuda_f32(z, "z")
        B, _, L, _ = z.shape
        up = self._upscale * L * self.interpolation_factor
        ids = torch.empty((B, up, up), device=z.device, dtype=torch.int64)
        prob = torch.empty((B, up, up), device=z.device, dtype=torch.float32) if return_prob else None
        with torch.cuda.device(z.device):
            _lib.check(_lib.lib().ldmseg_vae_decode_argmax(self._h, _lib.ptr(z), float(z_scale), B, L,
                                                           -1.0 if mask_th is None else float(mask_th), int(ignore_label),
                                                           _lib.ptr(ids), _lib.ptr(prob), _lib.stream_ptr(z.device)),
                       "ldmseg_vae_decode_argmax")
        return (ids, prob) if return_prob else ids

    def decode_panoptic(self, z: torch.Tensor, in_size, out_sizes, crop_boxes=None, z_scale: float = 1.0,
                        threshold_output: bool = True, threshold_mode: str = "max", mask_th: float = 0.5,
                        count_th: int = 512, overlap_th: float = 0.5, ignore_label: int = 0, return_stats: bool = False,
                        packed: bool = False):
        """The evaluation tail of `compute_pq` (trainers_ldm_cond.py:1243-1313) fused behind the decoder: decode ->
        bilinear x2 -> bilinear to `in_size` (H, W) -> crop to `crop_boxes[b]` = (y0, x0, height, width) -> bilinear to
        `out_sizes[b]` = (h, w) -> argmax / thresholds / segment filtering, without the [B,128,H,W] logits.
        Returns a list of (panoptic [h,w] int32 tensor on the GPU (label + 1, 0 = void), kept label list) - or, with
        `packed=True`, the device form without the copy of the keep table to the host: {"pan": the flat int32 buffer of all
        maps, "offsets": int64 [B] first element of image b, "sizes": int32 [B,2], "keep": uint8 [B,C] on the GPU}
        (what `PanopticEvaluatorAgnostic.process_device` takes)."""
        z = _lib.require_cuda_f32(z, "z")
        if threshold_mode not in ("max", "topk_diff"):
            raise ValueError(f"unknown threshold_mode {threshold_mode!r}")
        B, _, L, _ = z.shape

        def call(boxes, sizes, offs, labels, pan, keep, counts, mcounts):
            _lib.check(_lib.lib().ldmseg_vae_decode_panoptic(
                self._h, _lib.ptr(z), float(z_scale), B, L, int(in_size[0]), int(in_size[1]), boxes, sizes, offs,
                int(bool(threshold_output)), 1 if threshold_mode == "topk_diff" else 0, float(mask_th), int(count_th),
                float(overlap_th), int(ignore_label), _lib.ptr(labels), _lib.ptr(pan), _lib.ptr(keep), _lib.ptr(counts),
                _lib.ptr(mcounts), _lib.stream_ptr(z.device)), "ldmseg_vae_decode_panoptic")
        return self._panoptic_tail(call, B, z.device, out_sizes, crop_boxes, return_stats, packed)

    def _panoptic_tail(self, call, B, dev, out_sizes, crop_boxes, return_stats, packed=False):
        """Host geometry arrays and device outputs of the fused panoptic tail; `call` makes the library call on them."""
        import numpy as np
        Cn = self.out_channels
        sizes = np.ascontiguousarray(np.asarray(out_sizes, dtype=np.int32).reshape(B, 2))
        boxes = None if crop_boxes is None else np.ascontiguousarray(np.asarray(crop_boxes, dtype=np.int32).reshape(B, 4))
        npix = sizes[:, 0].astype(np.int64) * sizes[:, 1].astype(np.int64)
        offs = np.ascontiguousarray(np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64))
        total = int(npix.sum())
        labels = torch.empty(total, dtype=torch.int32, device=dev)
        pan = torch.empty(total, dtype=torch.int32, device=dev)
        keep = torch.empty(B, Cn, dtype=torch.uint8, device=dev)
        counts = torch.empty(B, Cn, dtype=torch.int32, device=dev)
        mcounts = torch.empty(B, Cn, dtype=torch.int32, device=dev)
        vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        with torch.cuda.device(dev):
            call(vp(boxes), vp(sizes), vp(offs), labels, pan, keep, counts, mcounts)
        if packed:
            out = {"pan": pan, "offsets": offs, "sizes": sizes, "keep": keep}
        else:
            keep_h = keep.cpu()
            out = []
            for b in range(B):
                o, n = int(offs[b]), int(npix[b])
                out.append((pan[o:o + n].view(int(sizes[b, 0]), int(sizes[b, 1])), torch.nonzero(keep_h[b]).flatten().tolist()))
        if return_stats:
            lab = [labels[int(offs[b]):int(offs[b]) + int(npix[b])].view(int(sizes[b, 0]), int(sizes[b, 1])) for b in range(B)]
            return out, {"labels": lab, "counts": counts, "mask_counts": mcounts, "keep": keep}
        return out

    def reconstruct_panoptic(self, x: torch.Tensor, in_size, out_sizes, crop_boxes=None, in_mul: float = 1.0,
                             in_add: float = 0.0, threshold_output: bool = True, mask_th: float = 0.5, count_th: int = 512,
                             overlap_th: float = 0.5, ignore_label: int = 0, return_stats: bool = False, packed: bool = False):
        """One batch of `TrainerAE.compute_pq` (trainers_ae.py:611-668) in one call: encode(x * in_mul + in_add) -> posterior
        mode -> decode -> the tail of `decode_panoptic`, with the overlap mask `logit >= mask_th` of :656 (not the sigmoid).
        x [B,7,H,H]; returns what `decode_panoptic` returns (`packed` as there)."""
        x = _lib.require_cuda_f32(x, "x")
        B, H = self._check_bitmaps(x)

        def call(boxes, sizes, offs, labels, pan, keep, counts, mcounts):
            _lib.check(_lib.lib().ldmseg_vae_reconstruct_panoptic(
                self._h, _lib.ptr(x), float(in_mul), float(in_add), B, H, int(in_size[0]), int(in_size[1]), boxes, sizes, offs,
                int(bool(threshold_output)), float(mask_th), int(count_th), float(overlap_th), int(ignore_label),
                _lib.ptr(labels), _lib.ptr(pan), _lib.ptr(keep), _lib.ptr(counts), _lib.ptr(mcounts),
                _lib.stream_ptr(x.device)), "ldmseg_vae_reconstruct_panoptic")
        return self._panoptic_tail(call, B, x.device, out_sizes, crop_boxes, return_stats, packed)

    def _check_bitmaps(self, x):
        B, Cin, H, W = x.shape
        if Cin != self._in_channels or H != W or H % self.downsample_factor:
            raise ValueError(f"expected [B,{self._in_channels},H,H] with H a multiple of {self.downsample_factor}, got {tuple(x.shape)}")
        return B, H

    def _semseg_tail(self, B, dev, out_size, targets, counts, num_classes, return_preds):
        """Arguments of the fused mIoU tail: (out_h, out_w, targets, K, preds, counts) with the tensors checked."""
        oh, ow = int(out_size[0]), int(out_size[1])
        if (targets is None) != (counts is None):
            raise ValueError("targets and counts go together")
        K = 0
        if targets is not None:
            if not targets.is_cuda or not counts.is_cuda:
                raise RuntimeError("targets and counts must live on the MI355X (no CPU fallback)")
            targets = targets.to(torch.int64).contiguous()
            if tuple(targets.shape) != (B, oh, ow):
                raise ValueError(f"targets must be [{B},{oh},{ow}], got {tuple(targets.shape)}")
            K = int(num_classes) if num_classes is not None else int(counts.shape[-1])
            if counts.dtype != torch.int64 or not counts.is_contiguous() or tuple(counts.shape) != (3, K):
                raise ValueError(f"counts must be a contiguous int64 [3,{K}] tensor")
        preds = torch.empty((B, oh, ow), device=dev, dtype=torch.int64) if return_preds else None
        return oh, ow, targets, K, preds

    def decode_semseg(self, z: torch.Tensor, out_size, targets: Optional[torch.Tensor] = None,
                      counts: Optional[torch.Tensor] = None, z_scale: float = 1.0, mask_th: Optional[float] = None,
                      ignore_label: int = 0, ignore_index: int = 255, num_classes: Optional[int] = None,
                      return_preds: bool = True):
        """The tail of `TrainerAE.compute_miou` (trainers_ae.py:754-761) fused behind the decoder: decode(interpolate=False) ->
        bilinear to `out_size` with align_corners=True -> argmax (+ max-softmax threshold -> `ignore_label`) -> the
        `SemsegMeter.update` rule against `targets` [B,h,w], ADDED to `counts` (int64 [3,K] on the GPU, e.g.
        `SemsegMeter.device_counts`).  Returns predictions [B,h,w] int64 (None with return_preds=False)."""
        z = _lib.require_cuda_f32(z, "z")
        B, _, L, _ = z.shape
        oh, ow, targets, K, preds = self._semseg_tail(B, z.device, out_size, targets, counts, num_classes, return_preds)
        with torch.cuda.device(z.device):
            _lib.check(_lib.lib().ldmseg_vae_decode_semseg(
                self._h, _lib.ptr(z), float(z_scale), B, L, oh, ow, -1.0 if mask_th is None else float(mask_th),
                int(ignore_label), _lib.ptr(targets), int(ignore_index), K, _lib.ptr(preds), _lib.ptr(counts),
                _lib.stream_ptr(z.device)), "ldmseg_vae_decode_semseg")
        return preds

    def reconstruct_semseg(self, x: torch.Tensor, out_size, targets: Optional[torch.Tensor] = None,
                           counts: Optional[torch.Tensor] = None, in_mul: float = 1.0, in_add: float = 0.0,
                           mask_th: Optional[float] = None, ignore_label: int = 0, ignore_index: int = 255,
                           num_classes: Optional[int] = None, return_preds: bool = True):
        """`vae_model(x, sample_posterior=False).sample` (vae.py:273-307) plus the tail of `decode_semseg` in one library call:
        encode(x * in_mul + in_add) -> posterior mode -> decode, no scaling factor; moments and latents never leave the
        handle's workspace and nothing synchronises with the host.  x [B,7,H,H]."""
        x = _lib.require_cuda_f32(x, "x")
        B, H = self._check_bitmaps(x)
        oh, ow, targets, K, preds = self._semseg_tail(B, x.device, out_size, targets, counts, num_classes, return_preds)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_vae_reconstruct_semseg(
                self._h, _lib.ptr(x), float(in_mul), float(in_add), B, H, oh, ow, -1.0 if mask_th is None else float(mask_th),
                int(ignore_label), _lib.ptr(targets), int(ignore_index), K, _lib.ptr(preds), _lib.ptr(counts),
                _lib.stream_ptr(x.device)), "ldmseg_vae_reconstruct_semseg")
        return preds

    def forward(self, sample, sample_posterior: bool = True, return_dict: bool = True,
                generator: Optional[torch.Generator] = None, rgb_sample=None, valid_mask=None):
        """vae.py:273-307.  Under grad mode `.sample` carries the decoder's graph (see `decode`) and, once `encoder_parameters()`
        has been called, the posterior's and the encoder's behind it (see `encode_moments`): one graph from a loss on the output to
        every tensor of `parameters()`."""
        if rgb_sample is not None:
            raise NotImplementedError("fuse_rgb is off in base.yaml:30")
        posterior = self.encode(sample).latent_dist
        z = posterior.sample(generator=generator) if sample_posterior else posterior.mode()
        if valid_mask is not None:
            z = z * valid_mask[:, None]
        dec = self.decode(z, interpolate=False)
        if not return_dict:
            return (dec,)
        return VAEOutput(sample=dec, posterior=posterior)

    __call__ = forward



class GeneralVAEImage(object):
    """ldmseg/models/vae.py:36-39 `GeneralVAEImage(AutoencoderKL)` with the decoder removed (tools/main_ldm.py:137-139):
    the RGB encoder used as `encode_func` in `TrainerDiffusion.encode_inputs` (trainers_ldm_cond.py:360-375).

    state_dict: `AutoencoderKL.state_dict()` / the 'vae_image' entry of ldmseg.pt (decoder keys are ignored).
    """

    def __init__(self, state_dict, scaling_factor: float = 0.18215, device: Union[str, torch.device] = "cuda:0",
                 compute_dtype="bf16", **unused):
        from ..weights import vae_image_schema
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GeneralVAEImage needs an MI355X device (no CPU fallback)")
        self.scaling_factor = scaling_factor
        self.dtype = torch.float32
        old = "encoder.mid_block.attentions.0.query.weight" in state_dict
        schema = vae_image_schema(old_attention_names=old)
        missing = [k for k in schema if k not in state_dict]
        if missing:
            raise KeyError(f"state dict lacks AutoencoderKL encoder tensors, e.g. {missing[:3]}")
        sd = {}
        for k in schema:
            t = state_dict[k]
            # newer diffusers store the attention projections as 1x1 convs or Linear; both flatten to [512, 512]
            sd[k] = t.reshape(schema[k]) if tuple(t.shape) != tuple(schema[k]) else t
        cd = {"bf16": _lib.BF16, torch.bfloat16: _lib.BF16, "fp32": _lib.F32, torch.float32: _lib.F32,
              "float32": _lib.F32, "bfloat16": _lib.BF16, "bf16x3": _lib.BF16X3}[compute_dtype]
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cfg = _lib.VAEImageCfg(cd, idx)
        n, names, ptrs, numels, keep = _lib.weight_arrays(sd, self.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.lib().ldmseg_vae_image_create(C.byref(cfg), n, names, ptrs, numels, C.byref(handle)),
                       "ldmseg_vae_image_create")
        del keep
        self._h = handle

    def set_scaling_factor(self, scaling_factor):          # vae.py:38-39
        self.scaling_factor = scaling_factor

    @property
    def num_parameters(self) -> int:
        return int(_lib.lib().ldmseg_vae_image_num_params(self._h))

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def requires_grad_(self, *_a, **_k):
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().ldmseg_vae_image_destroy(h)
            except Exception:
                pass
            self._h = None

    def encode_moments(self, images: torch.Tensor, in_mul: float = 1.0, in_add: float = 0.0) -> torch.Tensor:
        x = _lib.require_cuda_f32(images, "images")
        B, Cin, H, W = x.shape
        if Cin != 3 or H % 8 or W % 8:
            raise ValueError(f"expected [B,3,H,W] with H, W multiples of 8, got {tuple(x.shape)}")
        mom = torch.empty((B, 8, H // 8, W // 8), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_vae_image_encode(self._h, _lib.ptr(x), in_mul, in_add, B, H, W, _lib.ptr(mom),
                                                          _lib.stream_ptr(x.device)), "ldmseg_vae_image_encode")
        return mom

    def encode(self, x: torch.Tensor) -> EncoderOutput:
        """AutoencoderKL.encode(x).latent_dist (.mode() / .sample())."""
        return EncoderOutput(latent_dist=DiagonalGaussianDistribution(self.encode_moments(x)))

"""Sampling entry points with the reference's call surface.

Stands behind the hot-path methods of
/root/reference/ldmseg/trainers/trainers_ldm_cond.py::TrainerDiffusion:

    sample(prompts, num_inference_steps, guidance_scale, seed, rgb_latents, ...)   # :1045-1170
    decode_latents(latents, return_logits=True)                                   # :397-442
    encode_inputs(images, encode_func=vae_semseg.encode, scaling_factor=...)      # :335-394 (seg side)

plus two things the reference does elsewhere or not at all:
  * ``sample_sharded`` - the data-parallel eval decomposition the reference gets from
    DistributedSampler (:245): independent images are split over ranks, each rank runs
    the whole loop locally and ONE RCCL all-gather of the final latents replaces the
    detectron2 ``comm.gather`` of PNGs (evaluations/panoptic_evaluation_agnostic.py:129-131);
  * ``sample_inpaint`` - the build-defined mask-inpainting sampler.

The forward half of the training step is in scope (the loss of a checkpoint needs no backward pass):
``process_inputs`` (:677-765), ``compute_loss`` (:528-617), ``loss_fn`` (:495-526), ``predict_sample`` (:445-493) and
``get_loss_weight_mask`` (:620-661) with the reference's signatures, plus the build-defined driver ``validation_loss``.
Everything behind the UNet output runs in csrc/loss.hip (ldmseg_diffusion_loss / ldmseg_loss_weight_mask /
ldmseg_tensor_minmax) without a host synchronisation.  Backward, optimiser, EMA, logging and data loading stay out of scope.
"""
import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from .. import _lib
from ..utils import OutputDict

LOSS_TYPES = {"l1": 0, "l2": 1, "smooth_l1": 2}                  # LDMSEG_LOSS_*
MASK_MODES = {"ignore": 0, "padding": 1, "counts": 2}            # LDMSEG_MASK_*


class ModelInputs(OutputDict):
    """What `process_inputs` returns (trainers_ldm_cond.py:40-50): text, rgb_images, latents, rgb_latents,
    encoder_hidden_states, original_latents, loss_mask, inpainting_masks, dropout."""


class TrainerDiffusion(object):
    def __init__(self, vae_semseg, unet, noise_scheduler, self_condition: Optional[bool] = None,
                 device=None, latent_size: int = 64, vae_image=None, image_descriptor_model=None, textencoder=None,
                 tokenizer=None, training_loss_type: str = 'l2', rgb_noise_level: int = 0, cond_noise_level: int = 0,
                 ohem_ratio: float = 1.0, type_mask: str = 'ignore', prob_train_on_pred: float = 0.0,
                 prob_inpainting: float = 0.0, min_noise_level: int = 0, sample_posterior: bool = False,
                 ignore_label: int = 0):
        # the loss side of the training step (base.yaml's defaults; trainers_ldm_cond.py:129-160)
        self.training_loss_type = training_loss_type
        self.rgb_noise_level = rgb_noise_level
        self.cond_noise_level = cond_noise_level
        self.ohem_ratio = ohem_ratio
        self.type_mask = type_mask
        self.prob_train_on_pred = prob_train_on_pred
        self.prob_inpainting = prob_inpainting
        self.min_noise_level = min_noise_level
        self.sample_posterior = sample_posterior
        self.sample_posterior_rgb = False
        self.rgb_size = None
        self.dropout = 0.
        self.ignore_label = ignore_label
        self.loss_mask_flag = None            # device int32 [1] of the last get_loss_weight_mask call (bit 0: an id outside [0, 256))
        self._loss_tables = {}
        self.vae_image = vae_image            # RGB encoder (trainers_ldm_cond.py:58,111); optional here
        self.vae_semseg = vae_semseg
        self.unet_model = unet
        self.noise_scheduler = noise_scheduler
        self.self_condition = (unet.in_channels == 12) if self_condition is None else bool(self_condition)
        self.device = torch.device(device) if device is not None else unet.device
        self.args = {'gpu': self.device}
        self.latent_size = latent_size
        self.unet_dtype = torch.float32
        self.weight_dtype = torch.float32
        # Conditioning models of the cross-attention UNets (:55-127, descriptors.py:66-102), run once per batch: an image
        # descriptor model (clip_image / clip_image_proj: models.CLIPVisionDescriptor on the library, or any caller-supplied
        # torch module that returns {'last_feat': [B, D, ...]}) or a caller-supplied text encoder with its tokenizer
        # (image_descriptors none).  None of them: the UNet runs without a context.
        if textencoder is not None and image_descriptor_model is not None:
            raise ValueError("pass either a text encoder or an image descriptor model, not both (:126-127)")
        if textencoder is not None and tokenizer is None:
            raise ValueError("a text encoder needs its tokenizer")
        self.image_descriptor_model = image_descriptor_model
        self.textencoder = textencoder
        self.tokenizer = tokenizer
        for m in (image_descriptor_model, textencoder):
            if m is not None and hasattr(m, "eval"):
                m.eval()
        # imagenet / CLIP pixel statistics (utils.py:355-362, :303-308)
        self.pixel_mean_in = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        self.pixel_std_in = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        self.pixel_mean_clip = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float32,
                                            device=self.device).view(1, 3, 1, 1)
        self.pixel_std_clip = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float32,
                                           device=self.device).view(1, 3, 1, 1)

    # ------------------------------------------------------------------ noise
    @staticmethod
    def draw_noise(batch_size: int, latent_size: int, seed: Optional[int]) -> torch.Tensor:
        """CPU generator draw, identical for every batch of a given size (:1088-1091)."""
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        return torch.randn((batch_size, 4, latent_size, latent_size), generator=g)

    # ------------------------------------------------------------------ sample
    @torch.no_grad()
    def sample(self, prompts: List[str], num_inference_steps: int = 50, guidance_scale: float = 7.5,
               seed: Optional[int] = None, rgb_latents: Optional[torch.Tensor] = None,
               return_all_latents: bool = False, disable_progress_bar: bool = False,
               rgb_images: Optional[torch.Tensor] = None, scheduler=None, repeat_noise: Optional[bool] = None,
               python_loop: bool = False, latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """DDIM sampling loop.  ``python_loop=True`` walks ``scheduler.timesteps`` in Python calling
        ``unet(...)`` and ``scheduler.step(...)`` exactly like the reference; the default hands the
        whole loop to ldmseg_sample_loop (same kernels, no per-step Python)."""
        if rgb_latents is None:
            raise ValueError("rgb_latents is required (the reference dereferences it at :1126)")
        if scheduler is None:
            scheduler = self.noise_scheduler
            scheduler.set_timesteps_inference(num_inference_steps)
        repeat_noise = bool(repeat_noise)
        batch_size = len(prompts)
        rgb = _lib.require_cuda_f32(rgb_latents, "rgb_latents")
        L = rgb.shape[-1]
        if latents is None:
            latents = self.draw_noise(batch_size, L, seed)
        latents = latents.to(device=rgb.device, dtype=torch.float32)
        if repeat_noise:
            latents = latents[0:1].repeat(batch_size, 1, 1, 1)
            original_noise = latents.clone()
        encoder_hidden_states, multiplier = self.encoder_hidden_states(prompts, rgb_images)
        latents = (latents * scheduler.init_noise_sigma).contiguous()

        if encoder_hidden_states is not None:
            if self.self_condition and multiplier > 1:
                # (the reference concatenates the B-row condition with 2B-row tensors and fails at step 2, :1126-1150)
                raise ValueError("self-conditioning cannot be combined with classifier-free guidance (multiplier 2)")
            if python_loop:
                out = self._sample_python_guided(scheduler, latents, rgb, encoder_hidden_states, multiplier, guidance_scale,
                                                 return_all_latents)
            else:
                out = self._sample_native_guided(scheduler, latents, rgb, encoder_hidden_states, multiplier, guidance_scale,
                                                 return_all_latents)
        elif python_loop:
            out = self._sample_python(scheduler, latents, rgb, return_all_latents)
        else:
            out = self._sample_native(scheduler, latents, rgb, return_all_latents)
        if return_all_latents:
            return out
        if repeat_noise:
            return out, original_noise
        return out

    def _sample_python(self, scheduler, latents, rgb, return_all):
        all_latents = []
        condition = torch.zeros_like(rgb)
        n = len(scheduler.timesteps)
        for idx, t in enumerate(scheduler.timesteps):
            parts = [latents, rgb] + ([condition] if self.self_condition else [])
            inputs = torch.cat(parts, dim=1).to(self.unet_dtype)
            noise_pred = self.unet_model(inputs, t, encoder_hidden_states=None).sample
            if self.self_condition:
                condition = scheduler.step(noise_pred, t, latents).pred_original_sample
            if idx == n - 1:
                latents = scheduler.step(noise_pred, t, latents).pred_original_sample
            else:
                latents = scheduler.step(noise_pred, t, latents).prev_sample
            if return_all:
                all_latents.append(latents)
        return torch.cat(all_latents, dim=0) if return_all else latents

    # ------------------------------------------------------------------ conditioning (cross-attention UNets)
    def norm_resize_images(self, x, mode='imagenet'):
        """:663-675: the descriptor model's input - CLIP: 224x224 bilinear + CLIP statistics; DINO: 518x518 + imagenet."""
        import torch.nn.functional as F
        identifier = self.image_descriptor_model.__class__.__name__.lower()
        if 'clip' in identifier:
            x = F.interpolate(x, size=(224, 224), mode='bilinear', align_corners=False)
            x = (x - self.pixel_mean_clip) / self.pixel_std_clip
        elif 'dino' in identifier:
            x = F.interpolate(x, size=(518, 518), mode='bilinear', align_corners=False)
            x = (x - self.pixel_mean_in) / self.pixel_std_in
        else:
            x = (x - self.pixel_mean_in) / self.pixel_std_in
        return x

    @torch.no_grad()
    def encoder_hidden_states(self, prompts: List[str], rgb_images: Optional[torch.Tensor] = None):
        """(encoder_hidden_states, multiplier) as sample() builds them (:1098-1119): descriptors [B, S, D] of the images
        repeated for both halves, or [uncond | text] CLIP embeddings; (None, 1) without a conditioning model."""
        multiplier = 1
        ehs = None
        if self.image_descriptor_model is not None:
            if rgb_images is None:
                raise ValueError("an image descriptor model needs rgb_images")
            if hasattr(self.image_descriptor_model, "describe"):
                # the library's own encoder (models/clip_vision.py): resize + normalise run in its front kernel and the
                # context comes back as [B, S, D]
                d = self.image_descriptor_model.describe(rgb_images.to(self.device))
            else:
                x = self.norm_resize_images(rgb_images.to(self.device))
                d = self.image_descriptor_model(x.to(self.weight_dtype))['last_feat']
                d = d.view(d.shape[0], d.shape[1], -1).permute(0, 2, 1)
            ehs = torch.cat([d] * 2).to(torch.float)
            multiplier = 2
        if self.textencoder is not None:
            batch_size = len(prompts)
            text_input = self.tokenizer(prompts, padding="max_length", max_length=self.tokenizer.model_max_length,
                                        truncation=True, return_tensors="pt")
            text_embeddings = self.textencoder(text_input.input_ids.to(device=self.device))[0]
            max_length = text_input.input_ids.shape[-1]
            uncond_input = self.tokenizer([""] * batch_size, padding="max_length", max_length=max_length, return_tensors="pt")
            uncond_embeddings = self.textencoder(uncond_input.input_ids.to(device=self.device))[0]
            ehs = torch.cat([uncond_embeddings, text_embeddings]).to(torch.float)
            multiplier = 2
        return ehs, multiplier

    def _sample_python_guided(self, scheduler, latents, rgb, encoder_hidden_states, multiplier, guidance_scale, return_all):
        """:1121-1160 step for step: the UNet on multiplier * B images, guidance combine, DDIM step on B."""
        all_latents = []
        rgb_latents = torch.cat([rgb] * multiplier)
        condition = torch.zeros_like(rgb_latents)
        n = len(scheduler.timesteps)
        for idx, t in enumerate(scheduler.timesteps):
            latent_model_input = torch.cat([latents] * multiplier)
            if self.self_condition:
                inputs = torch.cat([latent_model_input, rgb_latents, condition], dim=1)
            else:
                inputs = torch.cat([latent_model_input, rgb_latents], dim=1)
            inputs = inputs.to(self.unet_dtype)
            noise_pred = self.unet_model(inputs, t, encoder_hidden_states=encoder_hidden_states).sample
            if multiplier > 1:
                noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
                noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
            if self.self_condition:
                condition = scheduler.step(noise_pred, t, latents).pred_original_sample
            if idx == n - 1:
                latents = scheduler.step(noise_pred, t, latents).pred_original_sample
            else:
                latents = scheduler.step(noise_pred, t, latents).prev_sample
            if return_all:
                all_latents.append(latents)
        return torch.cat(all_latents, dim=0) if return_all else latents

    def _sample_native_guided(self, scheduler, latents, rgb, encoder_hidden_states, multiplier, guidance_scale, return_all):
        if scheduler.thresholding:
            raise NotImplementedError
        cfg, keep = self._loop_cfg(scheduler)
        B, _, L, _ = rgb.shape
        lat = latents.clone()
        ctx = self.unet_model._context(encoder_hidden_states, multiplier * B)
        allv = torch.empty((cfg.n_steps * B, 4, L, L), device=rgb.device) if return_all else None
        with torch.cuda.device(rgb.device):
            _lib.check(_lib.lib().ldmseg_sample_loop_guided(
                self.unet_model._h, C.byref(cfg), _lib.ptr(lat), _lib.ptr(rgb), B, L, _lib.ptr(ctx), ctx.shape[1], ctx.shape[2],
                int(multiplier), float(guidance_scale), _lib.ptr(allv), _lib.stream_ptr(rgb.device)), "ldmseg_sample_loop_guided")
        del keep
        return allv if return_all else lat

    def _loop_cfg(self, scheduler):
        ts = scheduler.timesteps_host()
        n = len(ts)
        coef = np.ascontiguousarray(scheduler.coefficient_table(), dtype=np.float32)
        c_ts = (C.c_int64 * n)(*ts)
        cfg = _lib.SampleCfg()
        cfg.n_steps = n
        cfg.timesteps = c_ts
        cfg.coef = coef.ctypes.data_as(C.POINTER(C.c_float))
        cfg.prediction_type = _lib.PRED[scheduler.prediction_type]
        cfg.clip_sample = int(bool(scheduler.clip_sample))
        cfg.clip_sample_range = float(scheduler.clip_sample_range)
        cfg.self_condition = int(self.self_condition)
        return cfg, (c_ts, coef)

    def _sample_native(self, scheduler, latents, rgb, return_all, inpaint=None):
        if scheduler.thresholding:
            raise NotImplementedError
        cfg, keep = self._loop_cfg(scheduler)
        B, _, L, _ = rgb.shape
        lat = latents.clone()
        allv = torch.empty((cfg.n_steps * B, 4, L, L), device=rgb.device) if return_all else None
        if inpaint is not None:
            known, z0, noise, paste = inpaint
            cfg.known_dev = known.data_ptr()
            cfg.z0_dev = z0.data_ptr()
            cfg.noise_dev = noise.data_ptr()
            cfg.paste_coef = paste.ctypes.data_as(C.POINTER(C.c_float))
        with torch.cuda.device(rgb.device):
            _lib.check(_lib.lib().ldmseg_sample_loop(self.unet_model._h, C.byref(cfg), _lib.ptr(lat), _lib.ptr(rgb), B, L,
                                                     _lib.ptr(allv), _lib.stream_ptr(rgb.device)), "ldmseg_sample_loop")
        del keep
        return allv if return_all else lat

    # ------------------------------------------------------------------ inpainting (build-defined)
    @torch.no_grad()
    def sample_inpaint(self, prompts, known_mask: torch.Tensor, known_latents: torch.Tensor,
                       num_inference_steps: int = 50, seed: Optional[int] = None,
                       rgb_latents: Optional[torch.Tensor] = None, scheduler=None) -> torch.Tensor:
        """Mask-inpainting DDIM sampling (absent from the reference).  ``known_mask``
        bool [B,1,L,L], True = latent given (convention of trainers_ldm_cond.py:613-615);
        ``known_latents`` = scaling_factor * vae_semseg.encode(partial).mode().  After every step
        the known region is replaced by the known latents re-noised to the next timestep with the
        same fixed noise; the final step pastes them clean."""
        if scheduler is None:
            scheduler = self.noise_scheduler
            scheduler.set_timesteps_inference(num_inference_steps)
        rgb = _lib.require_cuda_f32(rgb_latents, "rgb_latents")
        B, _, L, _ = rgb.shape
        noise = self.draw_noise(len(prompts), L, seed).to(rgb.device).contiguous()
        z0 = _lib.require_cuda_f32(known_latents, "known_latents")
        known = known_mask.to(device=rgb.device).reshape(B, 1, L, L).to(torch.uint8).contiguous()
        ts = scheduler.timesteps_host()
        paste = np.zeros((len(ts), 2), dtype=np.float32)
        for i in range(len(ts)):
            if i == len(ts) - 1:
                paste[i] = (1.0, 0.0)
            else:
                a = scheduler.alphas_cumprod[ts[i + 1]]
                paste[i] = (float(a ** 0.5), float((1 - a) ** 0.5))
        latents = (noise * scheduler.init_noise_sigma).contiguous()
        return self._sample_native(scheduler, latents, rgb, False, inpaint=(known, z0, noise, paste))

    # ------------------------------------------------------------------ multi-GPU
    @torch.no_grad()
    def sample_sharded(self, prompts, num_inference_steps: int = 50, seed: Optional[int] = None,
                       rgb_latents: Optional[torch.Tensor] = None, scheduler=None, noise_mode: str = "reference",
                       group=None) -> torch.Tensor:
        """Data-parallel sampling of a GLOBAL batch: rank r owns images [r*B/W, (r+1)*B/W).
        ``rgb_latents`` is this rank's shard [B/W,4,L,L] (or the global batch on any device, from
        which the shard is sliced).  noise_mode 'reference': every rank seeds identically and draws
        randn(B/W) (what the reference's per-rank sample() does); 'global': one randn(B) draw,
        sliced.  Returns the all-gathered latents [B,4,L,L] on every rank (RCCL over xGMI)."""
        import torch.distributed as dist
        W = dist.get_world_size(group) if dist.is_initialized() else 1
        r = dist.get_rank(group) if dist.is_initialized() else 0
        B = len(prompts)
        if B % W:
            raise ValueError("global batch must divide by world size")
        per = B // W
        if rgb_latents.shape[0] == B and W > 1:
            rgb_latents = rgb_latents[r * per:(r + 1) * per]
        L = rgb_latents.shape[-1]
        if noise_mode == "reference":
            noise = self.draw_noise(per, L, seed)
        elif noise_mode == "global":
            noise = self.draw_noise(B, L, seed)[r * per:(r + 1) * per]
        else:
            raise ValueError(noise_mode)
        local = self.sample(prompts[r * per:(r + 1) * per], num_inference_steps, seed=seed,
                            rgb_latents=rgb_latents.to(self.device), scheduler=scheduler, latents=noise)
        if W == 1:
            return local
        out = torch.empty((B,) + tuple(local.shape[1:]), device=local.device, dtype=local.dtype)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out

    # ------------------------------------------------------------------ VAE side
    @torch.no_grad()
    def decode_latents(self, latents: torch.Tensor, return_logits: bool = False, threshold_output: bool = False,
                       rgb_latents=None, weight_dtype: torch.dtype = torch.float32, mask_th: float = 0.5,
                       ignore_label: int = 0, return_ids: bool = False):
        """:397-442.  return_logits=True -> fp32 logits [B,128,8L,8L] on the GPU; otherwise, like the reference, the
        colour-encoded uint8 numpy image [B,8L,8L,3] of the argmax ids (`encode_seg`, :436).  `return_ids=True`
        (extension) returns the int64 id map on the GPU instead of painting it.  The 1/scaling_factor multiply is
        fused into the decoder's input packing, and argmax (+ max-softmax threshold) with the decoder tail: the
        logits are never materialised on that path."""
        zs = 1.0 / self.vae_semseg.scaling_factor
        if return_logits:
            return self.vae_semseg.decode(latents, z_scale=zs).float()
        ids = self.vae_semseg.decode_argmax(latents, z_scale=zs, mask_th=mask_th if threshold_output else None,
                                            ignore_label=ignore_label)
        if return_ids:
            return ids
        from ..utils import encode_seg
        return encode_seg(ids.cpu().numpy()).astype(np.uint8)

    @torch.no_grad()
    def postprocess_panoptic(self, masks_logits: torch.Tensor, threshold_output: bool = False,
                             threshold_mode: str = "max", mask_th: float = 0.5, count_th: int = 512,
                             overlap_th: float = 0.5, ignore_label: int = 0, return_stats: bool = False):
        """The per-image post-processing loop of the evaluation (:1277-1313) in one pass on the GPU.

        masks_logits [B,C,H,W] fp32 on the GPU, already at the output size.  Returns `processed_results`
        like the reference: a list of {"panoptic_seg": (panoptic [H,W] int32 tensor (label+1, 0 = void),
        segments_info)} with segments_info = [{"id": label+1, "category_id": 1, "isthing": True}, ...] in
        ascending label order (np.unique order).  Only the [B,C] keep table is copied to the host.
        """
        from .. import _lib
        import ctypes as C
        x = _lib.require_cuda_f32(masks_logits, "masks_logits")
        if x.dim() != 4:
            raise ValueError("masks_logits must be [B,C,H,W]")
        if threshold_mode not in ("max", "topk_diff"):
            raise ValueError(f"unknown threshold_mode {threshold_mode!r}")
        B, Cn, H, W = x.shape
        dev = x.device
        labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        pan = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        keep = torch.empty(B, Cn, dtype=torch.uint8, device=dev)
        counts = torch.empty(B, Cn, dtype=torch.int32, device=dev)
        mcounts = torch.empty(B, Cn, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ldmseg_panoptic_postprocess(
                _lib.ptr(x), B, Cn, H, W, int(bool(threshold_output)), 1 if threshold_mode == "topk_diff" else 0,
                float(mask_th), int(count_th), float(overlap_th), int(ignore_label), _lib.ptr(labels), _lib.ptr(pan),
                _lib.ptr(keep), _lib.ptr(counts), _lib.ptr(mcounts), _lib.stream_ptr(dev)), "panoptic_postprocess")
        keep_h = keep.cpu()
        results = []
        for b in range(B):
            info = [{"id": int(c) + 1, "category_id": 1, "isthing": True} for c in torch.nonzero(keep_h[b]).flatten().tolist()]
            results.append({"panoptic_seg": (pan[b], info)})
        if return_stats:
            return results, {"labels": labels, "counts": counts, "mask_counts": mcounts, "keep": keep}
        return results

    # ------------------------------------------------------------------ evaluation loop body (compute_pq)
    @staticmethod
    def crop_padding(prediction: torch.Tensor, padding_mask: torch.Tensor) -> torch.Tensor:
        """:1172-1178 - bounding box of the non-padded region."""
        co = padding_mask.nonzero()
        y0, y1 = int(co[:, 0].min()), int(co[:, 0].max())
        x0, x1 = int(co[:, 1].min()), int(co[:, 1].max())
        return prediction[:, y0:y1 + 1, x0:x1 + 1]

    @staticmethod
    def padding_boxes(padding_masks: torch.Tensor):
        """The crop boxes of `crop_padding` for a whole batch, one D2H copy: [B,4] int32 numpy (y0, x0, height, width)."""
        m = padding_masks != 0
        rows, cols = m.any(dim=2), m.any(dim=1)                                   # [B,H], [B,W]
        if not bool(rows.any(dim=1).all()):
            raise ValueError("a padding mask without a single valid pixel")        # (the reference's .min() raises too)
        H, W = rows.shape[1], cols.shape[1]
        y0 = rows.int().argmax(dim=1)
        y1 = H - 1 - rows.flip(1).int().argmax(dim=1)
        x0 = cols.int().argmax(dim=1)
        x1 = W - 1 - cols.flip(1).int().argmax(dim=1)
        return torch.stack([y0, x0, y1 - y0 + 1, x1 - x0 + 1], dim=1).to(torch.int32).cpu().numpy()

    @torch.no_grad()
    def predict_panoptic(self, rgb_images: torch.Tensor, im_sizes, padding_masks: Optional[torch.Tensor] = None,
                         num_inference_steps: int = 50, guidance_scale: float = 7.5, seed: Optional[int] = None,
                         threshold_output: bool = True, threshold_mode: str = "max", scheduler=None, rgb_size: Optional[int] = None,
                         mask_th: float = 0.5, count_th: int = 512, overlap_th: float = 0.5, ignore_label: int = 0,
                         return_intermediates: bool = False, fused: bool = True, prompts: Optional[List[str]] = None,
                         packed: bool = False):
        """One batch of `compute_pq` (:1218-1313): RGB images [B,3,S,S] in [0,1] on the GPU -> `processed_results`
        (per image {"panoptic_seg": (panoptic map at the original size (h, w), segments_info)}).
        Pixels -> image-VAE latents -> DDIM sampling -> seg-VAE decoder -> [bilinear x2 -> bilinear to the input size ->
        crop the padding -> bilinear to (h, w) -> argmax / thresholds / segment filtering].  The bracket runs as ONE fused
        tail behind the decoder (`ldmseg_vae_decode_panoptic`: no [B,128,H,W] logits, no per-image torch interpolation);
        `fused=False` (and `return_intermediates`) materialises the logits and walks the reference's steps one by one.
        `packed=True` (fused tail only) returns the device form of `GeneralVAESeg.decode_panoptic` instead: nothing is copied
        to the host."""
        import torch.nn.functional as F
        if self.vae_image is None:
            raise ValueError("predict_panoptic needs the image VAE (TrainerDiffusion(..., vae_image=...))")
        rgb_images = _lib.require_cuda_f32(rgb_images, "rgb_images")
        B = rgb_images.shape[0]
        if scheduler is None:
            scheduler = self.noise_scheduler
            scheduler.set_timesteps_inference(num_inference_steps)
        rgb_latents, _ = self.encode_inputs(rgb_images, encode_func=self.vae_image.encode,
                                            scaling_factor=self.vae_image.scaling_factor, resize=rgb_size)
        # (prompts: data['text'] of the batch, read by a text encoder only; the images feed a descriptor model, :1222-1242)
        latents = self.sample(list(prompts) if prompts is not None else [""] * B, num_inference_steps, guidance_scale, seed,
                              rgb_latents=rgb_latents, scheduler=scheduler, disable_progress_bar=True, rgb_images=rgb_images)
        sizes = [(int(s[0]), int(s[1])) for s in im_sizes]
        if packed and (not fused or return_intermediates):
            raise ValueError("packed=True needs the fused tail")
        if fused and not return_intermediates:
            boxes = self.padding_boxes(padding_masks) if padding_masks is not None else None
            outs = self.vae_semseg.decode_panoptic(
                latents, (rgb_images.shape[-2], rgb_images.shape[-1]), sizes, boxes, z_scale=1.0 / self.vae_semseg.scaling_factor,
                threshold_output=threshold_output, threshold_mode=threshold_mode, mask_th=mask_th, count_th=count_th,
                overlap_th=overlap_th, ignore_label=ignore_label, packed=packed)
            if packed:
                return outs
            return [{"panoptic_seg": (pan, [{"id": int(c) + 1, "category_id": 1, "isthing": True} for c in kept])}
                    for pan, kept in outs]
        logits = self.decode_latents(latents, return_logits=True)
        logits = F.interpolate(logits, size=(rgb_images.shape[-2], rgb_images.shape[-1]), mode="bilinear",
                               align_corners=False)                                           # :1252-1257
        results = []
        for i in range(B):
            m = logits[i]
            if padding_masks is not None:
                m = self.crop_padding(m, padding_masks[i])                                    # :1263
            h, w = sizes[i]
            m = F.interpolate(m[None].float(), size=(h, w), mode="bilinear", align_corners=False)   # :1266-1271
            results += self.postprocess_panoptic(m.contiguous(), threshold_output=threshold_output,
                                                 threshold_mode=threshold_mode, mask_th=mask_th, count_th=count_th,
                                                 overlap_th=overlap_th, ignore_label=ignore_label)
        if return_intermediates:
            return results, {"rgb_latents": rgb_latents, "latents": latents, "logits": logits}
        return results

    @torch.no_grad()
    def compute_pq(self, dataloader, evaluator, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                   seed: Optional[int] = None, threshold_output: bool = True, max_iter: Optional[int] = None,
                   threshold_mode: str = "max", **post_kw):
        """`compute_pq` (:1181-1346) over an iterable of batches shaped like the reference's `collate_fn` output:
        {'image': [B,3,S,S] in [0,1], 'mask': [B,S,S] padding masks or None, 'meta': [{'image_file', 'image_id',
        'im_size': (h, w)}, ...]}.  `evaluator` is a PanopticEvaluatorAgnostic; all ranks must call this (the
        evaluator gathers).  Returns evaluator.evaluate() (rank 0) / None.  An evaluator built with `on_device=True` is fed
        through `process_device` (maps and keep table stay on the GPU; a batch may bring its ground truth as 'panoptic_gt')."""
        evaluator.reset()
        on_device = getattr(evaluator, "on_device", False)
        scheduler = self.noise_scheduler
        scheduler.set_timesteps_inference(num_inference_steps=num_inference_steps)
        scheduler.move_timesteps_to(self.device)                                              # :1211-1212
        for batch_idx, data in enumerate(dataloader):
            meta = data["meta"]
            file_names = [x["image_file"] for x in meta]
            image_ids = [x["image_id"] for x in meta]
            sizes = [x["im_size"] for x in meta]
            rgb = data["image"].to(self.device, non_blocking=True)
            masks = data.get("mask")
            masks = masks.to(self.device) if masks is not None else None
            processed = self.predict_panoptic(rgb, sizes, masks, num_inference_steps, guidance_scale, seed,
                                              threshold_output, threshold_mode, scheduler=scheduler, prompts=data.get("text"),
                                              **post_kw, **({"packed": True} if on_device else {}))
            if on_device:
                evaluator.process_device(file_names, image_ids, processed, gt_maps=data.get("panoptic_gt"))
            else:
                evaluator.process(file_names, image_ids, processed)
            if max_iter is not None and batch_idx > max_iter:                                 # (sic, :1332)
                break
        return evaluator.evaluate()

    @torch.no_grad()
    def encode_inputs(self, images: torch.Tensor, sample_posterior: bool = False, encode_func=None,
                      scaling_factor: Optional[float] = None, resize: Optional[int] = None, weight_dtype=None,
                      generator=None):
        """:335-394.  images in [0,1] (RGB, or bit maps for the segmentation VAE) -> 2x-1 -> encoder ->
        (latents, latents_mean) * scaling_factor.  As in the reference the default encoder is the image VAE
        (`self.vae_image.encode`); pass `encode_func=self.vae_semseg.encode` with its scaling factor for
        segmentation maps.  The 2x-1 is fused into the encoder's input packing."""
        import torch.nn.functional as F
        from ..models.vae import DiagonalGaussianDistribution
        if encode_func is None:
            if self.vae_image is None:
                raise ValueError("no encode_func given and the trainer was built without vae_image")
            encode_func = self.vae_image.encode
        owner = getattr(encode_func, "__self__", None)
        if scaling_factor is None:
            scaling_factor = (self.vae_image if self.vae_image is not None else owner).scaling_factor
        if resize is not None:
            images = F.interpolate(images, size=(resize, resize), mode='bilinear', align_corners=False)
        if owner is not None and hasattr(owner, "encode_moments"):
            dist_ = DiagonalGaussianDistribution(owner.encode_moments(images, in_mul=2.0, in_add=-1.0))   # :369 fused
        else:
            dist_ = encode_func(2. * images - 1.).latent_dist
        mean = dist_.mode()
        latents = dist_.sample(generator) if sample_posterior else mean.clone()
        if resize is not None:
            size = (self.latent_size, self.latent_size)
            latents = F.interpolate(latents, size=size, mode='bilinear', align_corners=False)
            mean = F.interpolate(mean, size=size, mode='bilinear', align_corners=False)
        return latents * scaling_factor, mean * scaling_factor

    # ------------------------------------------------------------------ denoising loss (forward half of the training step)
    def _scheduler_tables(self, device):
        """(alphas_cumprod, weights or None) of the scheduler as fp32 device tensors, cached per device and table."""
        sch = self.noise_scheduler
        w = getattr(sch, "weights", None)
        key = (str(device), id(sch.alphas_cumprod), id(w))
        if key not in self._loss_tables:
            ac = sch.alphas_cumprod.to(device=device, dtype=torch.float32).contiguous()
            wd = w.to(device=device, dtype=torch.float32).contiguous() if w is not None else None
            self._loss_tables = {key: (ac, wd, sch.alphas_cumprod, w)}        # (the host tables are kept so that the ids stay theirs)
        return self._loss_tables[key][:2]

    def _loss_type(self):
        if self.training_loss_type not in LOSS_TYPES:
            raise ValueError('Unknown loss type: {}'.format(self.training_loss_type))
        return LOSS_TYPES[self.training_loss_type]

    def _loss_tail(self, prediction, timesteps, target=None, noisy=None, loss_mask=None, paste_mask=None, paste_src=None,
                   minmax=None, prediction_type='sample', use_weights=False, ohem_ratio=1.0, want_pred=False, want_elem=False):
        """ldmseg_diffusion_loss on [B,C,...] tensors; returns (mean [1] or None, elem or None, pred_latents or None,
        sample_sums [B] or None).  Nothing is read back."""
        pred = _lib.require_cuda_f32(prediction, "prediction")
        dev = pred.device
        B, Cn = pred.shape[0], pred.shape[1]
        HW = pred.numel() // (B * Cn)

        def same(t, name):
            if t is None:
                return None
            t = _lib.require_cuda_f32(t.to(dev) if isinstance(t, torch.Tensor) else t, name)
            if t.shape != pred.shape:
                raise ValueError(f"{name} must have the prediction's shape {tuple(pred.shape)}, got {tuple(t.shape)}")
            return t
        target, noisy, paste_src = same(target, "target"), same(noisy, "noisy_latents"), same(paste_src, "original_latents")
        if loss_mask is not None:
            loss_mask = _lib.require_cuda_f32(loss_mask.to(dev), "loss_mask")
            if loss_mask.numel() != B * HW or loss_mask.shape[0] != B:
                raise ValueError(f"loss_mask must be [B,H,W] = [{B}, ...] with {HW} pixels per sample, got {tuple(loss_mask.shape)}")
        if paste_mask is not None:
            if paste_mask.dtype != torch.bool or paste_mask.shape != pred.shape:
                raise ValueError("inpainting_masks must be a bool mask of the latents' shape "
                                 f"{tuple(pred.shape)} (True = paste the original latents)")
            if paste_src is None:
                raise ValueError("inpainting_masks needs original_latents")
            paste_mask = paste_mask.to(dev).contiguous()
        k = None
        if target is not None and ohem_ratio < 1.:
            k = int(ohem_ratio * pred.numel())
            if k == 0:
                raise ValueError(f"ohem_ratio {ohem_ratio} selects none of the {pred.numel()} elements")
            want_elem = True
        ac, wd = self._scheduler_tables(dev)
        if timesteps is None:                                 # no timestep-dependent term is asked for (loss_fn): any valid index
            t = torch.zeros(B, dtype=torch.int64, device=dev)
        else:
            t = torch.as_tensor(timesteps).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if t.numel() == 1 and B > 1:
            t = t.expand(B).contiguous()
        if t.numel() != B:
            raise ValueError("timesteps must hold one entry per sample")
        lib = _lib.lib()
        mean = torch.empty(1, device=dev) if target is not None else None
        sums = torch.empty(B, device=dev) if target is not None else None
        elem = torch.empty_like(pred) if (want_elem and target is not None) else None
        out = torch.empty_like(pred) if want_pred else None
        scratch = torch.empty(int(lib.ldmseg_diffusion_loss_scratch_bytes(B, Cn, HW)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ldmseg_diffusion_loss(
                _lib.ptr(pred), _lib.ptr(target), _lib.ptr(noisy), _lib.ptr(t), _lib.ptr(ac), int(ac.numel()),
                _lib.ptr(wd if use_weights else None), _lib.ptr(loss_mask), _lib.ptr(paste_mask),
                _lib.ptr(paste_src if paste_mask is not None else None), _lib.ptr(minmax), self._loss_type(),
                _lib.PRED[prediction_type], float(ohem_ratio if k is not None else 1.0), B, Cn, HW, _lib.ptr(elem), _lib.ptr(out),
                _lib.ptr(mean), _lib.ptr(sums), _lib.ptr(scratch), _lib.stream_ptr(dev)), "ldmseg_diffusion_loss")
        return mean, elem, out, sums

    def loss_fn(self, x: torch.Tensor, y: torch.Tensor, reduction: str = 'none', mask: Optional[torch.Tensor] = None):
        """:495-526 - l1 / l2 / smooth_l1 element loss of x and y [B,C,...], times mask[:, None] if given, on the device.
        reduction 'none' (what compute_loss uses) returns the element losses, 'mean' / 'sum' the reduced scalar (a mask
        together with a reduction is refused: the reference would multiply the scalar by the mask)."""
        self._loss_type()
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"unknown reduction {reduction!r}")
        if reduction != 'none' and mask is not None:
            raise ValueError("a mask needs reduction='none'")
        mean, elem, _, sums = self._loss_tail(x, None, target=y, loss_mask=mask, want_elem=reduction == 'none')
        if reduction == 'mean':
            return mean[0]
        if reduction == 'sum':
            return sums.double().sum().float()                # the kernel's per-sample sums (fp64 sums rounded once), added in fp64
        return elem.view(x.shape)

    def _predict(self, noisy_latents, rgb_latents, condition, timesteps, encoder_hidden_states, timesteps_img=None):
        """The UNet on [noisy | rgb | condition]: through forward_parts (nothing concatenated in torch) when the handle takes the
        parts; with a context or an image timestep the concatenated input goes to forward (forward_ctx / forward_img)."""
        u = self.unet_model
        if (encoder_hidden_states is None and timesteps_img is None and hasattr(u, "forward_parts")
                and not getattr(u, "cross_attention", False) and rgb_latents is not None):
            return u.forward_parts(noisy_latents, rgb_latents, condition, timesteps).sample
        parts = [noisy_latents] + ([rgb_latents] if rgb_latents is not None else []) + ([condition] if condition is not None else [])
        inputs = torch.cat(parts, dim=1) if len(parts) > 1 else noisy_latents
        if timesteps_img is not None:
            return u(inputs, timesteps, encoder_hidden_states, timestep_img=timesteps_img).sample
        return u(inputs, timesteps, encoder_hidden_states).sample

    @staticmethod
    def _gen(generator, device):
        """`generator` if it lives on `device`'s kind of device, else None (the default generator of that device)."""
        if generator is not None and generator.device.type == torch.device(device).type:
            return generator
        return None

    @torch.no_grad()
    def compute_loss(self, noise: torch.Tensor, timesteps: torch.Tensor, noisy_latents: torch.Tensor,
                     rgb_latents: Optional[torch.Tensor], encoder_hidden_states: Optional[torch.Tensor],
                     loss_mask: Optional[torch.Tensor], latents: Optional[torch.Tensor] = None,
                     original_latents: Optional[torch.Tensor] = None, inpainting_masks: Optional[torch.Tensor] = None,
                     condition: Optional[torch.Tensor] = None, generator=None):
        """:528-617 without the graph: (loss, noisy_latents, pred_latents, timesteps), all on the device, nothing read back.
        One UNet forward, then ONE loss-tail launch (+ a finishing launch; + the radix select when ohem_ratio < 1) computes the
        element loss, its mask and timestep weight, the mean and pred_latents.  `inpainting_masks`: bool [B,4,H,W], True = paste
        original_latents (the only form the reference's `pred[m] = orig[m]` accepts).  `generator=` (extension) seeds the RGB /
        condition noise draws.  ohem_ratio * numel < 1 raises ValueError (the reference would return the mean of an empty
        tensor, NaN)."""
        assert rgb_latents is not None
        sch = self.noise_scheduler
        noisy = _lib.require_cuda_f32(noisy_latents, "noisy_latents")
        dev = noisy.device
        rgb = _lib.require_cuda_f32(rgb_latents, "rgb_latents")
        B = noisy.shape[0]
        gen = self._gen(generator, dev)
        if self.self_condition and condition is None:
            condition = torch.zeros_like(noisy)
        timesteps_img = None
        if self.rgb_noise_level > 0:                                                          # :568-572
            rgb_noise = torch.randn(rgb.shape, device=dev, dtype=rgb.dtype, generator=gen)
            timesteps_img = torch.randint(0, self.rgb_noise_level, (B,), device=dev, dtype=torch.long, generator=gen)
            rgb = sch.add_noise(rgb, rgb_noise, timesteps_img)
        if condition is not None and self.cond_noise_level > 0:                               # :577-581
            condition = _lib.require_cuda_f32(condition, "condition")
            cond_noise = torch.randn(condition.shape, device=dev, dtype=condition.dtype, generator=gen)
            timesteps_cond = torch.randint(0, self.cond_noise_level, (B,), device=dev, dtype=torch.long, generator=gen)
            condition = sch.add_noise(condition, cond_noise, timesteps_cond)
        if sch.prediction_type == "epsilon":
            target = noise
        elif sch.prediction_type == "sample":
            target = original_latents if original_latents is not None else latents
        else:
            raise ValueError(f"Unknown prediction type: {sch.prediction_type}")
        self._loss_type()
        timesteps = torch.as_tensor(timesteps).to(device=dev, dtype=torch.long)
        prediction = self._predict(noisy, rgb, condition, timesteps, encoder_hidden_states, timesteps_img)
        mean, _, pred_latents, sums = self._loss_tail(
            prediction, timesteps, target=target, noisy=noisy, loss_mask=loss_mask, paste_mask=inpainting_masks,
            paste_src=original_latents, prediction_type=sch.prediction_type, use_weights=hasattr(sch, 'weights'),
            ohem_ratio=self.ohem_ratio, want_pred=True)
        self.last_sample_loss_sums = sums
        return mean[0], noisy, pred_latents, timesteps

    def tensor_minmax(self, x: torch.Tensor) -> torch.Tensor:
        """Device pair [x.min(), x.max()] (ldmseg_tensor_minmax; what the loss tail's clamp reads through a pointer)."""
        x = _lib.require_cuda_f32(x, "x")
        out = torch.empty(2, device=x.device)
        scratch = torch.empty(3072, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_tensor_minmax(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.ptr(scratch),
                                                       _lib.stream_ptr(x.device)), "ldmseg_tensor_minmax")
        return out

    @torch.no_grad()
    def predict_sample(self, latents: torch.Tensor, rgb_latents: Optional[torch.Tensor] = None,
                       encoder_hidden_states: Optional[torch.Tensor] = None, tmax: Optional[int] = None, generator=None,
                       noise: Optional[torch.Tensor] = None, timesteps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """:445-493 - one-step prediction of the clean latents from a random noise level below `tmax`, clamped to the range
        of `latents`.  The clamp bounds never leave the device: ldmseg_tensor_minmax writes the pair the loss tail reads.
        `generator=`, `noise=` and `timesteps=` (extensions) make the draws reproducible."""
        sch = self.noise_scheduler
        if sch.prediction_type not in ('epsilon', 'sample'):
            raise ValueError('Unknown prediction type: {}'.format(sch.prediction_type))
        if tmax is None:
            tmax = sch.num_train_timesteps
        lat = _lib.require_cuda_f32(latents, "latents")
        dev = lat.device
        gen = self._gen(generator, dev)
        if noise is None:
            noise = torch.randn(lat.shape, device=dev, dtype=lat.dtype, generator=gen)
        if timesteps is None:
            timesteps = torch.randint(0, tmax, (lat.shape[0],), device=dev, dtype=torch.long, generator=gen)
        timesteps = torch.as_tensor(timesteps).to(device=dev, dtype=torch.long)
        noisy = sch.add_noise(lat, noise.to(dev), timesteps)
        prediction = self._predict(noisy, rgb_latents, None, timesteps, encoder_hidden_states)
        _, _, pred_latents, _ = self._loss_tail(prediction, timesteps, noisy=noisy, minmax=self.tensor_minmax(lat),
                                                prediction_type=sch.prediction_type, want_pred=True)
        return pred_latents

    @torch.no_grad()
    def get_loss_weight_mask(self, targets: torch.Tensor, ignore_label: int = 0, mode: str = 'nearest', size=(64, 64),
                             device=None, type_mask: str = 'ignore', padding_mask: Optional[torch.Tensor] = None):
        """:620-661 - the loss weight mask [B,h,w] fp32 in one launch: the nearest resize picks F.interpolate's source pixel;
        'ignore': target != ignore_label (the reference reads its dataset's ignore label there; this takes the argument),
        'padding': the resized padding mask, 'counts': 1 / (pixels of the id in the resized map), 0 on ignore_label, from a
        256-entry table per image in LDS instead of the torch.unique loop.  Any other type_mask: None, as in the reference.
        'counts' serves ids in [0, 256) (the bit codec's range): another id gets the weight NaN and sets `self.loss_mask_flag`
        (device int32 [1], bit 0), which stays on the device for the caller to read together with the loss."""
        if type_mask not in MASK_MODES:
            return None
        if mode != 'nearest':
            raise ValueError("only mode='nearest' is served")
        device = torch.device(device) if device is not None else self.device
        src = padding_mask if type_mask == 'padding' else targets
        if src is None:
            raise ValueError(f"type_mask={type_mask!r} needs its input map")
        src = src.to(device)
        if src.dim() != 3:
            raise ValueError("expected a [B,H,W] map")
        if src.dtype in (torch.bool, torch.uint8):
            code, src = 1, src.contiguous().view(torch.uint8) if src.dtype == torch.bool else src.contiguous()
        elif src.dtype.is_floating_point:
            code, src = 2, src.float().contiguous()
        else:
            code, src = 0, src.long().contiguous()
        B, Hi, Wi = src.shape
        h, w = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size), int(size))
        out = torch.empty((B, h, w), dtype=torch.float32, device=device)
        flag = torch.empty(1, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().ldmseg_loss_weight_mask(_lib.ptr(src), code, B, Hi, Wi, h, w, MASK_MODES[type_mask],
                                                          int(ignore_label), _lib.ptr(out), _lib.ptr(flag),
                                                          _lib.stream_ptr(device)), "ldmseg_loss_weight_mask")
        self.loss_mask_flag = flag
        return out

    @torch.no_grad()
    def process_inputs(self, data: dict, generator=None) -> ModelInputs:
        """:677-765 - a batch of the training loader ({'image', 'image_semseg', 'text', 'semseg', 'mask'} + 'inpainting_mask'
        / 'tokens' where used) -> ModelInputs.  `generator=` (extension) seeds the per-batch Bernoulli draws (made on the host
        like the reference's) when it is a CPU generator, and the device draws below it otherwise.

        With `prob_inpainting > 0` the returned `inpainting_masks` is, as in the reference, the resized fp32 map [B,h,w]
        (zeroed for the samples the draw left out).  `compute_loss` takes a bool [B,4,H,W] paste mask only - the one form the
        reference's `pred[m] = orig[m]` accepts - so the two cannot be chained on that path without the caller turning the map
        into such a mask (e.g. `(m > 0)[:, None].expand(-1, 4, -1, -1)`); the reference has the same gap."""
        dev = self.device
        rgb_images = data['image'].to(dev, non_blocking=True)
        bit_maps = data['image_semseg'].to(dev, non_blocking=True)
        B = bit_maps.shape[0]
        gen_dev, gen_cpu = self._gen(generator, dev), self._gen(generator, 'cpu')

        # both VAEs: segmentation bit maps -> latents (+ their posterior mean, the 'original' latents), RGB -> rgb_latents
        seg, img = self.vae_semseg, self.vae_image
        latents, original = self.encode_inputs(bit_maps, encode_func=seg.encode, scaling_factor=seg.scaling_factor,
                                               sample_posterior=self.sample_posterior, generator=gen_dev)
        rgb_latents = self.encode_inputs(rgb_images, encode_func=img.encode if img is not None else None,
                                         scaling_factor=img.scaling_factor if img is not None else None,
                                         sample_posterior=self.sample_posterior_rgb, resize=self.rgb_size, generator=gen_dev)[0]
        latents, original, rgb_latents = latents.float(), original.float(), rgb_latents.float()
        fields = ModelInputs()
        fields['text'] = data.get('text')
        fields['rgb_images'] = rgb_images

        # inpainting (:712-717): one Bernoulli draw per sample on the host; the nearest resize is the mask kernel's 'padding' mode
        paste_map = None
        if self.prob_inpainting > 0.:
            drawn = torch.rand(B, generator=gen_cpu) < self.prob_inpainting
            paste_map = self.get_loss_weight_mask(None, size=tuple(latents.shape[-2:]), device=dev, type_mask='padding',
                                                  padding_mask=data['inpainting_mask'])
            paste_map[~drawn] = 0.

        # conditioning (:721-733): image descriptors [B,S,D], or the text encoder's embeddings of the batch's tokens
        context = None
        desc = self.image_descriptor_model
        if desc is not None:
            if hasattr(desc, "describe"):
                context = desc.describe(rgb_images).to(torch.float32)
            else:
                feat = desc(self.norm_resize_images(rgb_images).to(self.weight_dtype))['last_feat']
                context = feat.flatten(2).transpose(1, 2).to(torch.float32)
        if self.textencoder is not None:
            context = self.textencoder(data['tokens'].to(dev, non_blocking=True))[0].to(torch.float32)

        # train on the model's own one-step prediction (:736-742): the drawn samples' latents are replaced, tmax = T // 2
        if self.prob_train_on_pred > 0.:
            drawn = torch.rand(B, generator=gen_cpu) < self.prob_train_on_pred
            if bool(drawn.any()):
                latents[drawn] = self.predict_sample(latents[drawn], rgb_latents[drawn], None if context is None else context[drawn],
                                                     tmax=self.noise_scheduler.num_train_timesteps // 2, generator=gen_dev)

        fields['latents'] = latents
        fields['rgb_latents'] = rgb_latents
        fields['encoder_hidden_states'] = context
        fields['original_latents'] = original
        fields['loss_mask'] = self.get_loss_weight_mask(data.get('semseg'), ignore_label=self.ignore_label, device=dev,
                                                        size=(self.latent_size, self.latent_size), type_mask=self.type_mask,
                                                        padding_mask=data.get('mask'))
        fields['inpainting_masks'] = paste_map
        fields['dropout'] = self.dropout if self.dropout > 0 else None
        return fields

    @torch.no_grad()
    def validation_loss(self, dataloader, timesteps=tuple(range(50, 1000, 100)), seed: Optional[int] = None,
                        max_iter: Optional[int] = None):
        """The denoising loss of a checkpoint over a loader, per timestep.  NOT in the reference (its loss is only ever logged
        from inside the training loop): for every batch `process_inputs`, then for every t of the grid all samples are noised to
        t with the `draw_noise(seed)` draw (the same for every batch, like `sample`), a self-conditioned handle runs the no-grad
        pre-pass of train_single_epoch (:822-831), and `compute_loss` gives the batch's loss.  The sums stay on the device; one
        read at the end returns {'loss': mean over the grid, 'per_timestep': {t: image-weighted mean loss}, 'images': n}."""
        sch = self.noise_scheduler
        grid = [int(t) for t in timesteps]
        sums = torch.zeros(len(grid), dtype=torch.float64, device=self.device)
        images = 0
        for batch_idx, data in enumerate(dataloader):
            if max_iter is not None and batch_idx >= max_iter:
                break
            mi = self.process_inputs(data)
            B, L = mi.latents.shape[0], mi.latents.shape[-1]
            noise = self.draw_noise(B, L, seed).to(self.device)
            for j, t in enumerate(grid):
                tt = torch.full((B,), t, dtype=torch.long, device=self.device)
                noisy = sch.add_noise(mi.latents, noise, tt)
                condition = None
                if self.self_condition:
                    pred = self._predict(noisy, mi.rgb_latents, torch.zeros_like(noisy), tt, mi.encoder_hidden_states)
                    condition = sch.remove_noise(noisy, pred, tt)
                loss, _, _, _ = self.compute_loss(noise, tt, noisy, mi.rgb_latents, mi.encoder_hidden_states, mi.loss_mask,
                                                  latents=mi.latents, original_latents=mi.original_latents, condition=condition)
                sums[j] += loss.double() * B
            images += B
        if images == 0:
            raise ValueError("validation_loss: the loader gave no batch")
        per = (sums / images).cpu().tolist()
        return {'loss': float(np.mean(per)), 'per_timestep': {t: v for t, v in zip(grid, per)}, 'images': images}

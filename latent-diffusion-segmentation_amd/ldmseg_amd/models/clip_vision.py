"""The CLIP ViT image encoder of the image-conditioned modes on the HIP library.

`CLIPVisionDescriptor` stands where the reference puts `MyCLIPVisionModel` / `MyCLIPVisionModelWithProjection`
(ldmseg/models/descriptors.py:15-56, 67-76): transformers' CLIPVisionModel(/WithProjection) over
openai/clip-vit-large-patch14, called once per batch at trainers_ldm_cond.py:1102-1103.
"""
import ctypes as C
from typing import Optional, Union

import torch

from .. import _lib
from ..weights import clip_vision_schema

PIXEL_MEAN_CLIP = (0.48145466, 0.4578275, 0.40821073)      # utils.py:303-308
PIXEL_STD_CLIP = (0.26862954, 0.26130258, 0.27577711)


def strip_vision_prefix(state_dict):
    """CLIPVisionModelWithProjection.state_dict() - and CLIPVisionModel.state_dict() of the transformers 4.x releases -
    prefix the encoder's keys with ``vision_model.``; transformers 5.x's CLIPVisionModel does not.  Both load."""
    return {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state_dict.items()}


def config_from_state_dict(sd):
    """Shape-derived configuration; the head count is hidden / 64 (every CLIP ViT has head dim 64) and the image size
    follows from the position table."""
    pe = sd["embeddings.patch_embedding.weight"]
    hidden, patch = int(pe.shape[0]), int(pe.shape[-1])
    tokens = int(sd["embeddings.position_embedding.weight"].shape[0])
    grid = int(round((tokens - 1) ** 0.5))
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
    proj = sd.get("visual_projection.weight")
    return dict(hidden=hidden, intermediate=int(sd["encoder.layers.0.mlp.fc1.weight"].shape[0]), layers=layers,
                heads=hidden // 64, image=grid * patch, patch=patch, projection_dim=int(proj.shape[0]) if proj is not None else 0)


class CLIPVisionDescriptor(object):
    """state_dict: `CLIPVisionModel.state_dict()` or `CLIPVisionModelWithProjection.state_dict()`, with or without the
    ``vision_model.`` prefix.  projection=True: the `clip_image_proj` descriptor (needs `visual_projection.weight`).

    config: dict(hidden, intermediate, layers, heads, image, patch, projection_dim) - by default read off the tensors."""

    def __init__(self, state_dict, projection: bool = False, device: Union[str, torch.device] = "cuda:0",
                 compute_dtype="bf16", config: Optional[dict] = None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CLIPVisionDescriptor needs an MI355X device (no CPU fallback)")
        sd = strip_vision_prefix(state_dict)
        cfg = dict(config_from_state_dict(sd) if config is None else config)
        if not projection:
            cfg["projection_dim"] = 0
        elif not cfg.get("projection_dim"):
            raise KeyError("projection=True needs visual_projection.weight (CLIPVisionModelWithProjection.state_dict())")
        schema = clip_vision_schema(**cfg)
        missing = [k for k in schema if k not in sd]
        if missing:
            raise KeyError(f"state dict lacks CLIP vision tensors, e.g. {missing[:3]}")
        self.config = cfg
        self.projection = bool(projection)
        self.dtype = torch.float32
        self.tokens = (cfg["image"] // cfg["patch"]) ** 2 + 1
        cd = {"bf16": _lib.BF16, torch.bfloat16: _lib.BF16, "fp32": _lib.F32, torch.float32: _lib.F32,
              "float32": _lib.F32, "bfloat16": _lib.BF16, "bf16x3": _lib.BF16X3}[compute_dtype]
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        ccfg = _lib.ClipVisionCfg(cfg["hidden"], cfg["intermediate"], cfg["layers"], cfg["heads"], cfg["image"], cfg["patch"],
                                  cfg["projection_dim"], cd, idx)
        n, names, ptrs, numels, keep = _lib.weight_arrays({k: sd[k] for k in schema}, self.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.lib().ldmseg_clip_vision_create(C.byref(ccfg), n, names, ptrs, numels, C.byref(handle)),
                       "ldmseg_clip_vision_create")
        del keep
        self._h = handle

    @property
    def num_parameters(self) -> int:
        return int(_lib.lib().ldmseg_clip_vision_num_params(self._h))

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
                _lib.lib().ldmseg_clip_vision_destroy(h)
            except Exception:
                pass
            self._h = None

    def _outputs(self, B, device, hidden=True, embeds=True):
        hid = torch.empty((B, self.tokens, self.config["hidden"]), device=device, dtype=torch.float32) if hidden else None
        emb = (torch.empty((B, self.config["projection_dim"]), device=device, dtype=torch.float32)
               if embeds and self.projection else None)
        return hid, emb

    def encode(self, pixel_values: torch.Tensor, hidden: bool = True):
        """(last_hidden_state [B, T, hidden] - None with hidden=False -, image_embeds [B, projection_dim] or None without
        projection) of resized, normalised images."""
        x = _lib.require_cuda_f32(pixel_values, "pixel_values")
        S = self.config["image"]
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != S or x.shape[3] != S:
            raise ValueError(f"expected pixel_values [B,3,{S},{S}], got {tuple(x.shape)}")
        B = x.shape[0]
        hid, emb = self._outputs(B, x.device, hidden=hidden or not self.projection)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_clip_vision_forward(self._h, _lib.ptr(x), B, _lib.ptr(hid), _lib.ptr(emb),
                                                             _lib.stream_ptr(x.device)), "ldmseg_clip_vision_forward")
        return hid, emb

    def forward(self, pixel_values: torch.Tensor):
        """{'last_feat': last_hidden_state.permute(0, 2, 1)} [B, hidden, T] (descriptors.py:26-37), or with projection=True
        {'last_feat': image_embeds.unsqueeze(-1)} [B, projection_dim, 1] (:48-56)."""
        hid, emb = self.encode(pixel_values, hidden=not self.projection)
        return {'last_feat': emb.unsqueeze(-1) if self.projection else hid.permute(0, 2, 1)}

    __call__ = forward

    def describe(self, rgb_images: torch.Tensor, mean=PIXEL_MEAN_CLIP, std=PIXEL_STD_CLIP) -> torch.Tensor:
        """The UNet's context [B, S, D] from raw images [B,3,H,W] in [0,1] of any size: norm_resize_images
        (trainers_ldm_cond.py:663-675) runs inside the library's front kernel.  [B, T, hidden], or [B, 1, projection_dim]."""
        x = _lib.require_cuda_f32(rgb_images, "rgb_images")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected rgb_images [B,3,H,W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        hid, emb = self._outputs(B, x.device, hidden=not self.projection)
        cm, cs = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldmseg_clip_vision_describe(self._h, _lib.ptr(x), B, H, W, cm, cs, _lib.ptr(hid), _lib.ptr(emb),
                                                              _lib.stream_ptr(x.device)), "ldmseg_clip_vision_describe")
        return emb.unsqueeze(1) if self.projection else hid

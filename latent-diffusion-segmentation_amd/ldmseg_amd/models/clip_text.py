"""The CLIP text encoder of the text-conditioned mode on the HIP library.

`CLIPTextEncoder` stands where the reference puts transformers' `CLIPTextModel` (SD-1.x's text_encoder, loaded at
ldmseg/models/descriptors.py:98-103): called on the tokenised prompts and on the empty prompts at
trainers_ldm_cond.py:1108-1119, which read ``[0]``, the last_hidden_state.  The tokenizer stays the caller's.
"""
import ctypes as C
from typing import Optional, Union

import torch

from .. import _lib
from ..utils import OutputDict
from ..weights import clip_text_schema


def strip_text_prefix(state_dict):
    """CLIPTextModel.state_dict() of the transformers 4.x releases prefixes the encoder's keys with ``text_model.``;
    transformers 5.x does not.  Both load."""
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()}


def config_from_state_dict(sd):
    """Shape-derived configuration; the head count is hidden / 64 (every CLIP text tower has head dim 64), vocabulary and
    positions follow from the two embedding tables."""
    tok = sd["embeddings.token_embedding.weight"]
    vocab, hidden = int(tok.shape[0]), int(tok.shape[1])
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
    return dict(vocab=vocab, hidden=hidden, intermediate=int(sd["encoder.layers.0.mlp.fc1.weight"].shape[0]), layers=layers,
                heads=hidden // 64, positions=int(sd["embeddings.position_embedding.weight"].shape[0]))


class CLIPTextOutput(OutputDict):
    """``out[0]`` is the first field, as on transformers' ModelOutput (trainers_ldm_cond.py:1111 reads ``textencoder(ids)[0]``)."""

    def __getitem__(self, key):
        if isinstance(key, int):
            return list(self.values())[key]
        return super().__getitem__(key)


class CLIPTextEncoder(object):
    """state_dict: `CLIPTextModel.state_dict()`, with or without the ``text_model.`` prefix.

    config: dict(vocab, hidden, intermediate, layers, heads, positions) - by default read off the tensors."""

    def __init__(self, state_dict, device: Union[str, torch.device] = "cuda:0", compute_dtype="bf16",
                 config: Optional[dict] = None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CLIPTextEncoder needs an MI355X device (no CPU fallback)")
        sd = strip_text_prefix(state_dict)
        cfg = dict(config_from_state_dict(sd) if config is None else config)
        schema = clip_text_schema(**cfg)
        missing = [k for k in schema if k not in sd]
        if missing:
            raise KeyError(f"state dict lacks CLIP text tensors, e.g. {missing[:3]}")
        self.config = cfg
        self.dtype = torch.float32
        cd = {"bf16": _lib.BF16, torch.bfloat16: _lib.BF16, "fp32": _lib.F32, torch.float32: _lib.F32,
              "float32": _lib.F32, "bfloat16": _lib.BF16, "bf16x3": _lib.BF16X3}[compute_dtype]
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        ccfg = _lib.ClipTextCfg(cfg["vocab"], cfg["positions"], cfg["hidden"], cfg["intermediate"], cfg["layers"], cfg["heads"],
                                cd, idx)
        n, names, ptrs, numels, keep = _lib.weight_arrays({k: sd[k] for k in schema}, self.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.lib().ldmseg_clip_text_create(C.byref(ccfg), n, names, ptrs, numels, C.byref(handle)),
                       "ldmseg_clip_text_create")
        del keep
        self._h = handle

    @property
    def num_parameters(self) -> int:
        return int(_lib.lib().ldmseg_clip_text_num_params(self._h))

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
                _lib.lib().ldmseg_clip_text_destroy(h)
            except Exception:
                pass
            self._h = None

    def forward(self, input_ids: torch.Tensor):
        """CLIPTextOutput(last_hidden_state=[R, T, hidden] fp32 on the device); ``[0]`` is that tensor, as the sampler reads it.
        input_ids: int32 / int64 [R, T] on any device, 1 <= T <= positions, every id in [0, vocab)."""
        if not isinstance(input_ids, torch.Tensor) or input_ids.dtype not in (torch.int32, torch.int64):
            raise ValueError("input_ids must be an int32 or int64 tensor")
        if input_ids.dim() != 2:
            raise ValueError(f"expected input_ids [R, T], got {tuple(input_ids.shape)}")
        R, T = int(input_ids.shape[0]), int(input_ids.shape[1])
        if R < 1 or T < 1 or T > self.config["positions"]:
            raise ValueError(f"expected 1 <= T <= {self.config['positions']} and R >= 1, got {tuple(input_ids.shape)}")
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        lo, hi = torch.stack(torch.aminmax(ids)).tolist()           # (one host round trip for both)
        if lo < 0 or hi >= self.config["vocab"]:
            raise IndexError(f"input_ids out of range: [{lo}, {hi}] against a vocabulary of {self.config['vocab']}")
        out = torch.empty((R, T, self.config["hidden"]), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ldmseg_clip_text_forward(self._h, _lib.ptr(ids), R, T, _lib.ptr(out),
                                                           _lib.stream_ptr(self.device)), "ldmseg_clip_text_forward")
        return CLIPTextOutput(last_hidden_state=out)

    __call__ = forward

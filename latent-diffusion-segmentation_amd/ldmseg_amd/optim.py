"""The weight update of the training loops on the gfx950 library: gradient-norm clipping and AdamW over a list of tensors.

Stands behind the reference's ldmseg/trainers/optim.py (`torch.optim.AdamW`, base.yaml: optimizer_name adamw) and the
`clip_grad_norm_(..., clip_grad)` of its training steps (trainers_ae.py:305-325): one `ldmseg_adamw_step` call does both for every
parameter (two launches for the seg-VAE's 34 tensors), nothing is copied to or read back from the device.

    opt = AdamW(vae.parameters(), lr=1e-4, weight_decay=0.0)
    norm = opt.step(max_norm=3.0)             # 0-d device tensor: the norm before clipping; .grad holds the clipped gradients

`state_dict()` / `load_state_dict()` speak torch.optim.AdamW's layout, so the 'opt' entry of a reference checkpoint loads here and
ours loads into torch's optimiser.  No amsgrad, no maximize, no gradient scaler, no CPU tensors.
"""
import ctypes as C
from typing import Iterable, Optional

import torch

from . import _lib

HYPER_KEYS = ("lr", "betas", "eps", "weight_decay")
# what torch.optim.AdamW keeps per group besides HYPER_KEYS (its defaults: the only values this optimiser implements)
TORCH_GROUP_EXTRAS = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                      "fused": None, "decoupled_weight_decay": True}


def state_to_torch(packed: dict) -> dict:
    """{'state': {index: {'step': int, 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [{lr, betas, eps, weight_decay, 'params':
    [indices]}]} -> what `torch.optim.AdamW.state_dict()` returns for the same optimiser: the step as a 0-d fp32 tensor, the groups
    with torch's remaining keys at their defaults.  Tensors are shared, not copied."""
    state = {int(i): {"step": torch.tensor(float(s["step"]), dtype=torch.float32), "exp_avg": s["exp_avg"],
                      "exp_avg_sq": s["exp_avg_sq"]} for i, s in packed["state"].items()}
    groups = []
    for g in packed["param_groups"]:
        out = {k: (tuple(g[k]) if k == "betas" else g[k]) for k in HYPER_KEYS}
        out.update(TORCH_GROUP_EXTRAS)
        out["params"] = [int(i) for i in g["params"]]
        groups.append(out)
    return {"state": state, "param_groups": groups}


def state_from_torch(sd: dict) -> dict:
    """The inverse: a `torch.optim.AdamW.state_dict()` (e.g. the 'opt' entry of a reference model.pt) -> the packed form above, the
    step as an int.  A group with amsgrad or maximize, or Adam's coupled weight decay, raises NotImplementedError."""
    groups = []
    for g in sd["param_groups"]:
        for k in ("amsgrad", "maximize"):
            if g.get(k):
                raise NotImplementedError(f"an optimiser state with {k}=True is not supported")
        if g.get("decoupled_weight_decay", True) is False:
            raise NotImplementedError("Adam's coupled weight decay (decoupled_weight_decay=False) is not supported")
        out = {k: (tuple(float(b) for b in g[k]) if k == "betas" else float(g[k])) for k in HYPER_KEYS}
        out["params"] = [int(i) for i in g["params"]]
        groups.append(out)
    state = {}
    for i, s in sd["state"].items():
        if "max_exp_avg_sq" in s:
            raise NotImplementedError("an optimiser state with amsgrad=True is not supported")
        step = s["step"]
        state[int(i)] = {"step": int(round(float(step))), "exp_avg": s["exp_avg"], "exp_avg_sq": s["exp_avg_sq"]}
    return {"state": state, "param_groups": groups}


def _arrays(tensors):
    """(n, pointers) of a list of tensors / None as the C ABI takes them (an array of one dummy element when empty)"""
    n = len(tensors)
    ptrs = (C.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in tensors])
    return n, ptrs


def _written(tensors):
    """the kernels wrote these through raw pointers: tell autograd (GeneralVAESeg's stale-handle check reads the version counters)"""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


def _check(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous fp32 tensor on the MI355X (the HIP path has no CPU fallback)")
    return t


def _grads_call(params, max_norm):
    """ldmseg_grad_norm (max_norm None) / ldmseg_grad_clip over the .grad of `params`"""
    params = [params] if isinstance(params, torch.Tensor) else list(params)
    grads = [_check(p.grad, "a gradient") for p in params if p.grad is not None]
    if not grads:
        raise ValueError("no tensor of the list has a gradient")
    dev = grads[0].device
    n, ptrs = _arrays(grads)
    numels = (C.c_int64 * n)(*[g.numel() for g in grads])
    lib = _lib.lib()
    scratch = torch.empty(max(int(lib.ldmseg_multi_tensor_scratch_bytes(n, numels)), 8), dtype=torch.uint8, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if max_norm is None:
            _lib.check(lib.ldmseg_grad_norm(n, ptrs, numels, _lib.ptr(total), _lib.ptr(scratch), _lib.stream_ptr(dev)), "ldmseg_grad_norm")
        else:
            _lib.check(lib.ldmseg_grad_clip(n, ptrs, numels, float(max_norm), _lib.ptr(total), _lib.ptr(scratch), _lib.stream_ptr(dev)),
                       "ldmseg_grad_clip")
            _written(grads)
    return total


def grad_norm(params: Iterable[torch.Tensor]) -> torch.Tensor:
    """The L2 norm of all `.grad` of `params` (fp64 sums, one rounding) as a 0-d device tensor; nothing is read back."""
    return _grads_call(params, None)


def clip_grad_norm_(params: Iterable[torch.Tensor], max_norm: float) -> torch.Tensor:
    """`torch.nn.utils.clip_grad_norm_(params, max_norm)` (norm_type 2) in two launches: returns the norm before clipping as a 0-d
    device tensor and scales every `.grad` in place by min(1, max_norm / (norm + 1e-6))."""
    return _grads_call(params, max_norm)


class AdamW(object):
    """torch.optim.AdamW (decoupled weight decay; no amsgrad / maximize) over fp32 tensors on the device, or over param-group dicts
    {'params': [...], 'lr': ..., ...}.  `param_groups` is a list of plain dicts that may be changed between steps (the reference's
    loop writes param_group['lr'] every iteration); `state[p]` = {'step': int, 'exp_avg', 'exp_avg_sq'}, made at p's first step."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        self.defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay))
        self.param_groups = []
        self.state = {}
        params = list(params)
        if not params:
            raise ValueError("optimizer got an empty parameter list")
        if not isinstance(params[0], dict):
            params = [{"params": params}]
        seen = set()
        for g in params:
            g = dict(g)
            ps = g["params"]
            g["params"] = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            unknown = set(g) - set(HYPER_KEYS) - {"params"}
            if unknown:
                raise ValueError(f"unknown param-group keys {sorted(unknown)}")
            for p in g["params"]:
                if not isinstance(p, torch.Tensor) or not p.is_leaf:
                    raise ValueError("can only optimise leaf tensors")
                if id(p) in seen:
                    raise ValueError("a parameter appears in more than one group")
                seen.add(id(p))
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            self._validate(g)
            self.param_groups.append(g)

    @staticmethod
    def _validate(g):
        if not g["lr"] >= 0.0 or not g["eps"] >= 0.0 or not g["weight_decay"] >= 0.0:
            raise ValueError(f"lr, eps and weight_decay must not be negative: {g['lr']}, {g['eps']}, {g['weight_decay']}")
        if not (0.0 <= g["betas"][0] < 1.0 and 0.0 <= g["betas"][1] < 1.0):
            raise ValueError(f"betas must lie in [0, 1): {g['betas']}")

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    @torch.no_grad()
    def step(self, max_norm: float = 0.0) -> Optional[torch.Tensor]:
        """One update of every parameter that has a `.grad`, in ONE ldmseg_adamw_step call.  max_norm > 0: the gradients of all groups
        are clipped to that total L2 norm first (`clip_grad_norm_` fused in: `.grad` holds the clipped values afterwards) and the norm
        before clipping is returned as a 0-d device tensor; otherwise None.  The parameters change in place: a model that packs
        them (GeneralVAESeg) needs its `refresh()` afterwards."""
        ps, gs, ms, vs, hyper = [], [], [], [], []
        for g in self.param_groups:
            self._validate(g)
            for p in g["params"]:
                _check(p, "a parameter")
                grad = p.grad
                st = self.state.get(p)
                if grad is not None:
                    if not grad.is_contiguous():
                        grad = p.grad = grad.contiguous()
                    _check(grad, "a gradient")
                    if grad.device != p.device or grad.shape != p.shape:
                        raise RuntimeError("a gradient does not match its parameter")
                    if st is None:
                        st = self.state[p] = {"step": 0, "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                                              "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
                    st["step"] += 1
                ps.append(p); gs.append(grad)
                ms.append(st["exp_avg"] if st else None); vs.append(st["exp_avg_sq"] if st else None)
                hyper.append((g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], st["step"] if st else 0))
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise RuntimeError("all parameters of one optimiser must live on one device")
        n, c_p = _arrays(ps)
        _, c_g = _arrays(gs)
        _, c_m = _arrays(ms)
        _, c_v = _arrays(vs)
        numels = (C.c_int64 * n)(*[p.numel() for p in ps])
        c_h = (_lib.AdamWHyper * n)(*hyper)
        lib = _lib.lib()
        clip = max_norm is not None and max_norm > 0
        total = scratch = None
        if clip:
            scratch = torch.empty(max(int(lib.ldmseg_multi_tensor_scratch_bytes(n, numels)), 8), dtype=torch.uint8, device=dev)
            total = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ldmseg_adamw_step(n, c_p, c_g, c_m, c_v, numels, c_h, float(max_norm) if clip else 0.0, _lib.ptr(total),
                                             _lib.ptr(scratch), _lib.stream_ptr(dev)), "ldmseg_adamw_step")
        _written([p for p, g in zip(ps, gs) if g is not None] + ([g for g in gs if g is not None] if clip else []))
        return total

    def _packed(self):
        index = {}
        groups = []
        for g in self.param_groups:
            out = {k: g[k] for k in HYPER_KEYS}
            out["params"] = []
            for p in g["params"]:
                index[p] = len(index)
                out["params"].append(index[p])
            groups.append(out)
        state = {index[p]: s for p, s in self.state.items() if p in index}
        return {"state": dict(sorted(state.items())), "param_groups": groups}

    def state_dict(self) -> dict:
        """torch.optim.AdamW's layout: {'state': {index: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [{..., 'params':
        [indices]}]} (the moments are the optimiser's own tensors, not copies - `torch.save` writes them out)."""
        return state_to_torch(self._packed())

    def load_state_dict(self, sd: dict):
        """From this class's or torch.optim.AdamW's `state_dict()`: the hyper-parameters of every group and the state of every
        parameter, matched by position; moments are copied to the parameter's device as fp32."""
        packed = state_from_torch(sd)
        if len(packed["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        flat = []
        for g, lg in zip(self.param_groups, packed["param_groups"]):
            if len(g["params"]) != len(lg["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            flat += list(zip(lg["params"], g["params"]))
        new_groups = []
        for g, lg in zip(self.param_groups, packed["param_groups"]):
            ng = {k: lg[k] for k in HYPER_KEYS}
            ng["params"] = g["params"]
            self._validate(ng)
            new_groups.append(ng)
        by_index = dict(flat)
        state = {}
        for i, s in packed["state"].items():
            if i not in by_index:
                raise ValueError(f"loaded state refers to parameter {i}, which no group lists")
            p = by_index[i]
            m, v = (s[k].detach().to(device=p.device, dtype=torch.float32).contiguous().clone() for k in ("exp_avg", "exp_avg_sq"))
            if m.shape != p.shape or v.shape != p.shape:
                raise ValueError(f"loaded moments of parameter {i} have shape {tuple(m.shape)}, the parameter {tuple(p.shape)}")
            state[p] = {"step": s["step"], "exp_avg": m, "exp_avg_sq": v}
        self.param_groups[:] = new_groups          # in place: a caller's reference to the list stays valid
        self.state = state

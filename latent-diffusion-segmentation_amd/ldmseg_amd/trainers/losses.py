"""The seg-VAE's stage-1 losses: the reference's ldmseg/trainers/losses.py::SegmentationLosses.point_loss
(:364-394) - the PointRend cross entropy on uncertain points (`loss_ce`, :303-362) and the per-object BCE + Dice on uncertain
points (`loss_masks`, :117-185, with `prepare_targets`, :397-439) - computed by csrc/point_loss.hip, and their gradient with
respect to the logits, computed by csrc/point_loss_bwd.hip when the logits require grad (what `loss.backward()` of the
reference's stage-1 step, trainers_ae.py:286-296, needs of the loss; no network backward or optimiser is built).

The library draws nothing: the uniform draws are made here with `torch.rand`, in the reference's order and shapes
(`draw_plan`), so a CPU generator seeded s reproduces what the reference draws on the CPU after `torch.manual_seed(s)`.
One host read per call in one process: the class-presence table, whose count N of object masks fixes the shape of the mask
draws (the reference's `prepare_targets` synchronises once per image); under torch.distributed the all-reduced number of masks
is a second one.  The matcher (:45-101, "not used by default") is not built.
"""
from typing import Dict, List, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib

MAX_CLASSES = 128          # LDMSEG_POINT_LOSS_MAX_C


def draw_plan(batch: int, num_masks: int, num_points: int, oversample_ratio, importance_sample_ratio) -> List[Tuple[str, Tuple[int, ...]]]:
    """The `torch.rand` calls of one `point_loss`, in order: [(name, shape)].  S = int(P * oversample_ratio) oversampled points
    and kR = P - int(importance_sample_ratio * P) fresh ones per row (detectron2_utils.py:43-67); first the B cross-entropy rows
    (:331-339), then the N mask rows (:157-165), which draw nothing when N == 0 (:141-142).  oversample_ratio 0: one draw of P."""
    P = int(num_points)
    if oversample_ratio > 0:
        if oversample_ratio < 1 or not 0 <= importance_sample_ratio <= 1:
            raise ValueError("oversample_ratio must be 0 or >= 1, importance_sample_ratio in [0, 1]")
        S = int(P * oversample_ratio)
        kR = P - int(importance_sample_ratio * P)
    else:
        S, kR = 0, P
    plan = []
    for name, rows in (("ce", batch), ("mask", num_masks)):
        if rows == 0:
            continue
        if S > 0:
            plan.append((name + "_over", (rows, S, 2)))
        if kR > 0:
            plan.append((name + "_fresh", (rows, kR, 2)))
    return plan


class SegmentationLosses(object):
    def __init__(self, num_points: int = 12544, oversample_ratio=3, importance_sample_ratio: float = 0.75, ignore_label: int = 0,
                 cost_mask: float = 1.0, cost_class: float = 1.0, temperature: float = 1.0):
        self.num_points = int(num_points)
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        self.ignore_label = int(ignore_label)
        self.temperature = float(temperature)
        self.cost_mask = cost_mask
        self.cost_class = cost_class
        draw_plan(1, 1, self.num_points, oversample_ratio, importance_sample_ratio)      # checks the ratios

    @property
    def world_size(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def _num_masks(self, N: int, device) -> float:
        """:143-146: the number of object masks averaged over the ranks, at least 1.  In one process this is host arithmetic;
        under torch.distributed the all-reduced count is read back, a second host read of the call."""
        world = self.world_size
        if world == 1:
            return float(max(N, 1))
        import torch.distributed as dist
        count = torch.tensor([float(N)], device=device)
        dist.all_reduce(count)
        return max(float((count / world).item()), 1.0)                   # (the quotient in fp32, as there)

    @torch.no_grad()
    def class_presence(self, targets: torch.Tensor, masks: Optional[torch.Tensor], num_classes: int):
        """-> (targets int64 contiguous, valid uint8 [B,Ht,Wt] or None, rows int32 [N] on the host holding b * C + c).  The one
        host read of `point_loss`.  ValueError on an id outside [0, num_classes) other than ignore_label."""
        dev = targets.device
        B, Ht, Wt = targets.shape
        tg = targets.to(torch.int64).contiguous()
        valid = None
        if masks is not None:
            if not masks.is_cuda or tuple(masks.shape) != (B, 1, Ht, Wt):
                raise RuntimeError(f"masks must be a [{B},1,{Ht},{Wt}] tensor on the MI355X, got {tuple(masks.shape)} on {masks.device}")
            valid = (masks[:, 0] != 0).to(torch.uint8).contiguous()
        present = torch.empty((B, num_classes), dtype=torch.uint8, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ldmseg_class_presence(_lib.ptr(tg), _lib.ptr(valid), B, Ht, Wt, num_classes, self.ignore_label,
                                                        _lib.ptr(present), _lib.ptr(flag), _lib.stream_ptr(dev)),
                       "ldmseg_class_presence")
        table = torch.cat([present.view(-1), flag.view(torch.uint8)]).cpu()               # the host read
        if table[B * num_classes:].any():
            raise ValueError(f"targets hold an id outside [0, {num_classes}) other than ignore_label {self.ignore_label}")
        rows = torch.nonzero(table[:B * num_classes]).flatten().to(torch.int32)
        return tg, valid, rows

    def point_loss(self, outputs: torch.Tensor, targets: torch.Tensor, do_matching: bool = False,
                   masks: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                   return_points: bool = False) -> Dict[str, torch.Tensor]:
        """:364-394 on logits [B,C,H,W] and int64 targets [B,Ht,Wt] (masks: validity [B,1,Ht,Wt], nonzero = valid; `targets` is
        not modified).  Returns {'ce', 'mask'} as 0-d device tensors; with return_points also 'selected' (int32 [B+N,kU], the
        oversampled points chosen per row, ascending), 'rows' (int32 [N], b * C + c) and 'bce' / 'dice' (the two mask terms).
        With grad mode on and `outputs` requiring grad, 'ce' and 'mask' are differentiable with respect to `outputs` (once:
        `_PointLossFunction`; 'bce' / 'dice' stay plain values); otherwise nothing is recorded."""
        if do_matching:
            raise NotImplementedError("the Hungarian matcher (losses.py:45-101, not used by default) is not built")
        for name, t in (("outputs", outputs), ("targets", targets)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{name} must be a tensor on the MI355X: the HIP path has no CPU fallback")
        if torch.is_grad_enabled() and outputs.requires_grad:
            # the cast and the copy are torch ops outside the Function: torch carries the gradient back to a producer that is
            # not fp32 or not contiguous
            x = _lib.require_cuda_f32(outputs, "outputs")
            extras = {}
            ce, mask = _PointLossFunction.apply(x, self, targets, masks, generator, extras)
            losses = {'ce': ce, 'mask': mask}
            if return_points:
                losses.update(selected=extras['selected'], rows=extras['rows'], bce=extras['out'][1], dice=extras['out'][2])
            return losses
        with torch.no_grad():
            out, state = self._point_loss_forward(_lib.require_cuda_f32(outputs, "outputs"), targets, masks, generator, return_points)
        losses = {'ce': out[0], 'mask': out[1] + out[2]}
        if return_points:
            losses.update(selected=state['selected'], rows=state['rows'], bce=out[1], dice=out[2])
        return losses

    def _point_loss_forward(self, x: torch.Tensor, targets: torch.Tensor, masks, generator, keep_selected: bool):
        """The one library call on fp32 contiguous logits, grad mode off: -> (out [3] = ce, bce, dice; what a backward needs)."""
        if x.dim() != 4 or targets.dim() != 3 or targets.shape[0] != x.shape[0]:
            raise ValueError(f"expected logits [B,C,H,W] and targets [B,Ht,Wt], got {tuple(x.shape)} and {tuple(targets.shape)}")
        B, C, H, W = x.shape
        if C > MAX_CLASSES:
            raise ValueError(f"at most {MAX_CLASSES} classes, got {C}")
        dev = x.device
        Ht, Wt = targets.shape[-2:]
        tg, valid, rows = self.class_presence(targets, masks, C)
        N = int(rows.numel())
        plan = draw_plan(B, N, self.num_points, self.oversample_ratio, self.importance_sample_ratio)
        rdev = generator.device if generator is not None else dev
        draws = {name: torch.rand(shape, generator=generator, device=rdev).to(dev) for name, shape in plan}
        P = self.num_points
        S = int(P * self.oversample_ratio) if self.oversample_ratio > 0 else 0
        kU = int(self.importance_sample_ratio * P) if self.oversample_ratio > 0 else 0
        num_masks = self._num_masks(N, dev) if N > 0 else 1.0
        rows_dev = rows.to(dev) if N > 0 else None
        out = torch.empty(3, dtype=torch.float32, device=dev)
        selected = torch.empty((B + N, kU), dtype=torch.int32, device=dev) if keep_selected and kU > 0 else None
        lib = _lib.lib()
        scratch = torch.empty(int(lib.ldmseg_point_loss_scratch_bytes(B + N, S, kU, P)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ldmseg_point_loss(
                _lib.ptr(x), B, C, H, W, _lib.ptr(tg), _lib.ptr(valid), Ht, Wt, _lib.ptr(rows_dev), N,
                _lib.ptr(draws.get("ce_over")), _lib.ptr(draws.get("ce_fresh")), _lib.ptr(draws.get("mask_over")),
                _lib.ptr(draws.get("mask_fresh")), S, kU, P, self.ignore_label, self.temperature, num_masks,
                _lib.ptr(out), _lib.ptr(selected), _lib.ptr(scratch), _lib.stream_ptr(dev)), "ldmseg_point_loss")
        state = dict(tg=tg, valid=valid, rows=rows, rows_dev=rows_dev, draws=draws, selected=selected, num_masks=num_masks,
                     S=S, kU=kU, P=P, ignore_label=self.ignore_label, temperature=self.temperature)
        return out, state


class _PointLossFunction(torch.autograd.Function):
    """(ce, mask) of `SegmentationLosses.point_loss` with a backward to the logits (ldmseg_point_loss_backward, csrc/
    point_loss_bwd.hip).  Saved for it: the logits, the draws, the forward's `selected`, the rows, targets / valid and num_masks
    - no sampled logits.  Once differentiable: a second backward through it is refused by torch."""

    @staticmethod
    def forward(ctx, x, crit, targets, masks, generator, extras):
        out, state = crit._point_loss_forward(x, targets, masks, generator, True)
        ctx.save_for_backward(x)
        ctx.state = state
        ctx.set_materialize_grads(False)
        extras.update(selected=state['selected'], rows=state['rows'], out=out)
        return out[0].clone(), out[1] + out[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_ce, grad_mask):
        x, = ctx.saved_tensors
        st = ctx.state
        if grad_ce is None and grad_mask is None:
            return (None,) * 6
        B, C, H, W = x.shape
        dev = x.device
        N = int(st['rows'].numel())
        Ht, Wt = st['tg'].shape[-2:]
        g_ce = None if grad_ce is None else grad_ce.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        g_mask = None if grad_mask is None else grad_mask.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        grad_x = torch.empty_like(x)
        lib = _lib.lib()
        nbytes = int(lib.ldmseg_point_loss_backward_scratch_bytes(B, C, H, W, N, st['kU'], st['P']))
        if nbytes == 0:
            raise RuntimeError("ldmseg_point_loss_backward: sizes out of range")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d = st['draws']
        with torch.cuda.device(dev):
            _lib.check(lib.ldmseg_point_loss_backward(
                _lib.ptr(x), B, C, H, W, _lib.ptr(st['tg']), _lib.ptr(st['valid']), Ht, Wt, _lib.ptr(st['rows_dev']), N,
                _lib.ptr(d.get("ce_over")), _lib.ptr(d.get("ce_fresh")), _lib.ptr(d.get("mask_over")), _lib.ptr(d.get("mask_fresh")),
                _lib.ptr(st['selected']), st['S'], st['kU'], st['P'], st['ignore_label'], st['temperature'], st['num_masks'],
                _lib.ptr(g_ce), _lib.ptr(g_mask), _lib.ptr(grad_x), _lib.ptr(scratch), _lib.stream_ptr(dev)),
                "ldmseg_point_loss_backward")
        return grad_x, None, None, None, None, None

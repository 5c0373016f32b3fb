"""Readers of tests/golden/point_loss_grad.npz (written by tests/golden/make_golden_point_loss_grad.py): the reference's own
gradients of the stage-1 loss, per case d ce / d logits and d mask / d logits, and d mean(kl) / d moments.  Shared by
tests/test_point_loss_grad_cpu.py and tests/test_point_loss_grad_gpu.py."""
import numpy as np
import torch

import point_loss_ref as R

OLD_CASES = ["base", "odd_points", "c128", "ratio0", "valid_mask", "one_empty", "no_segment", "temperature", "all_uncertain", "ignore3"]
NEW_CASES = ["tiny_map", "one_channel_wide", "saturated"]
CASES = OLD_CASES + NEW_CASES


def _grad(grad, key):
    if key in grad:
        return torch.from_numpy(grad[key])
    shape = tuple(int(v) for v in grad[key + "/shape"])
    flat = np.zeros(int(np.prod(shape)), dtype=np.float32)
    flat[np.cumsum(grad[key + "/index_delta"].astype(np.int64))] = grad[key + "/value"]
    return torch.from_numpy(flat.reshape(shape))


def load_case(gold, grad, name, device="cpu"):
    """-> the dict of point_loss_ref.load_case (inputs of point_loss.npz, or the case's own) plus grad_ce / grad_mask (CPU)."""
    k = name + "/"
    if int(grad[k + "own_inputs"]) == 0:
        case = R.load_case(gold, name, device)
    else:
        P, ratio, isr, temp, ignore = grad[k + "params"].tolist()
        q = gold[str(gold[str(grad[k + "x_of"]) + "/logits"])] if k + "x_of" in grad else grad[k + "x"]
        x = torch.from_numpy(q.astype(np.float32) * float(grad[k + "x_scale"])).to(device)
        case = dict(x=x, targets=torch.from_numpy(grad[k + "targets"].astype(np.int64)).to(device), masks=None, P=int(P),
                    ratio=int(ratio), isr=isr, temperature=temp, ignore=int(ignore), seed=int(grad[k + "seed"]),
                    num_masks=int(grad[k + "num_masks"]), ce=grad[k + "ce"], mask=grad[k + "mask"])
    case["grad_ce"] = _grad(grad, k + "grad_ce")
    case["grad_mask"] = _grad(grad, k + "grad_mask")
    return case


def draws_for(case, device="cpu"):
    """the draws of SegmentationLosses.point_loss for this case: a CPU generator at the case's seed, the plan's order"""
    from ldmseg_amd.trainers.losses import draw_plan
    g = torch.Generator().manual_seed(case["seed"])
    plan = draw_plan(case["x"].shape[0], case["num_masks"], case["P"], case["ratio"], case["isr"])
    return {name: torch.rand(shape, generator=g).to(device) for name, shape in plan}


def restatement_grads(case, x=None):
    """tests/point_loss_ref.py under CPU autograd -> (ce, mask, d ce / d x, d mask / d x); zeros where a term has no graph"""
    x = (case["x"].detach().cpu() if x is None else x).clone().requires_grad_(True)
    cpu = lambda t: None if t is None else t.cpu()
    out = R.point_loss(x, cpu(case["targets"]), cpu(case["masks"]), draws_for(case), case["P"], case["ratio"], case["isr"],
                       case["temperature"], case["ignore"])
    grads = []
    for tag in ("ce", "mask"):
        g = torch.autograd.grad(out[tag], x, retain_graph=True, allow_unused=True)[0] if out[tag].requires_grad else None
        grads.append(torch.zeros_like(x) if g is None else g)
    return out["ce"].detach(), out["mask"].detach(), grads[0], grads[1]


def rel_dev(got, want):
    """max|got - want| / max|want|; both all zero: 0"""
    scale = float(want.abs().max())
    diff = float((got - want).abs().max())
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / scale

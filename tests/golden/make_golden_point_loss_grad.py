"""Writes tests/golden/point_loss_grad.npz by RUNNING the reference's own stage-1 loss functions under CPU autograd (only where
the reference checkout exists): SegmentationLosses.point_loss on logits that require grad, torch.autograd.grad of its 'ce' and of
its 'mask' separately, and the gradient of DiagonalGaussianDistribution(moments).kl().mean() with respect to the moments.
Nothing of the reference is copied: the fixture holds inputs, seeds and the gradients its functions returned.

Cases: the ten of point_loss.npz (inputs and seeds are read from that file, only the gradients are stored here) and three with
inputs of their own, their seeds found by the same search for the selection gap (make_golden_point_loss.py):
    tiny_map          logits [2,16,4,4], targets 16 x 16, P = 64: dozens of taps per pixel, every border tap falls outside the
                      map, the CE row and the mask rows of an image write the same planes
    one_channel_wide  logits [1,3,5,37], targets 10 x 74, P = 33: H != W, neither a power of two, P odd
    saturated         'base' with logits * 8: sigmoid and softmax at their ends
Gradients of 128-channel cases are stored as (flat index, value) pairs of their nonzeros, the indices as first differences;
the others dense.  'saturated' stores no logits of its own: it names the case of point_loss.npz whose logits it scales.

    python tests/golden/make_golden_point_loss_grad.py [path of the reference checkout]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_point_loss import LOGIT_SCALE, gaps_ok, import_reference, make_logits, make_targets, run_case  # noqa: E402
import point_loss_ref as R  # noqa: E402

SRC = os.path.join(HERE, "point_loss.npz")
OUT = os.path.join(HERE, "point_loss_grad.npz")

# name: logits shape, (Ht, Wt), P, oversample_ratio, importance_sample_ratio, temperature, ignore_label, start seed
NEW_CASES = {
    "tiny_map":         ((2, 16, 4, 4), (16, 16), 64, 3, 0.75, 1.0, 0, 2100),
    "one_channel_wide": ((1, 3, 5, 37), (10, 74), 33, 3, 0.75, 1.0, 0, 2200),
}


def grads_of(SL, x, targets, masks, P, ratio, isr, temperature, ignore, seed):
    """The reference's point_loss under autograd at `seed` -> (losses, d ce / d x, d mask / d x)."""
    crit = SL(num_points=P, oversample_ratio=ratio, importance_sample_ratio=isr, ignore_label=ignore, temperature=temperature)
    x = x.clone().requires_grad_(True)
    torch.manual_seed(seed)
    losses = crit.point_loss(x, targets.clone(), False, None if masks is None else masks.clone())
    out = []
    for tag in ("ce", "mask"):
        if losses[tag].requires_grad:
            out.append(torch.autograd.grad(losses[tag], x, retain_graph=True, allow_unused=True)[0])
        else:
            out.append(None)
    return losses, [torch.zeros_like(x) if g is None else g.detach() for g in out]


def store(out, key, g, sparse):
    g = g.numpy().astype(np.float32)
    if not sparse:
        out[key] = g
        return
    flat = g.reshape(-1)
    idx = np.flatnonzero(flat)
    out[key + "/index_delta"] = np.diff(idx, prepend=0).astype(np.int32)     # flat indices = cumsum; the steps compress well
    out[key + "/value"] = flat[idx]
    out[key + "/shape"] = np.asarray(g.shape, dtype=np.int64)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LDMSEG_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "ldmseg")):
        print("reference checkout not given (argument or LDMSEG_REFERENCE); nothing to do")
        return
    SL, DGD = import_reference(ref)
    gold = np.load(SRC)
    out = {"logit_scale": np.float32(LOGIT_SCALE)}
    names = []

    def add(name, case, own_inputs):
        losses, (g_ce, g_mask) = grads_of(SL, case["x"], case["targets"], case["masks"], case["P"], case["ratio"], case["isr"],
                                          case["temperature"], case["ignore"], case["seed"])
        k = name + "/"
        for tag in ("ce", "mask"):
            want, got = float(case[tag]), float(losses[tag])
            assert (np.isnan(want) and np.isnan(got)) or want == got, (name, tag, want, got)   # the same draws as the forward fixture
        sparse = case["x"].shape[1] > 64
        store(out, k + "grad_ce", g_ce, sparse)
        store(out, k + "grad_mask", g_mask, sparse)
        out[k + "own_inputs"] = np.int64(own_inputs)
        names.append(name)
        print(f"{name}: seed {case['seed']} ce {float(losses['ce'])!r} mask {float(losses['mask'])!r} "
              f"max|g_ce| {float(g_ce.abs().max()):.3e} max|g_mask| {float(g_mask.abs().max()):.3e} "
              f"nonzero {int((g_ce != 0).sum())} / {int((g_mask != 0).sum())} of {g_ce.numel()}")

    for name in gold["cases"]:
        add(str(name), R.load_case(gold, str(name)), 0)

    def add_new(name, q, targets, P, ratio, isr, temp, ignore, seed, scale, x_of=None):
        """q: int8 logits in units of `scale`, stored with the case unless they are those of case `x_of` of point_loss.npz"""
        x = q.float() * scale
        kU = int(isr * P)
        while True:
            losses, shapes, picks = run_case(SL, x, targets, None, P, ratio, isr, temp, ignore, seed)
            if gaps_ok(picks, kU):
                break
            seed += 1
        eff = targets
        n_masks = sum(int((torch.unique(t) != ignore).sum()) for t in eff)
        k = name + "/"
        if x_of is None:
            out[k + "x"] = q.numpy()
        else:
            out[k + "x_of"] = np.asarray(x_of)
        out[k + "x_scale"] = np.float32(scale)
        out[k + "targets"] = targets.numpy().astype(np.uint8)
        out[k + "params"] = np.asarray([P, ratio, isr, temp, ignore], dtype=np.float64)
        out[k + "seed"] = np.int64(seed)
        out[k + "num_masks"] = np.int64(n_masks)
        out[k + "ce"] = np.float32(losses["ce"])
        out[k + "mask"] = np.float32(losses["mask"])
        case = dict(x=x, targets=targets, masks=None, P=P, ratio=ratio, isr=isr, temperature=temp, ignore=ignore, seed=seed,
                    ce=out[k + "ce"], mask=out[k + "mask"])
        add(name, case, 1)

    g = torch.Generator().manual_seed(47)
    for name, (shape, (Ht, Wt), P, ratio, isr, temp, ignore, seed) in NEW_CASES.items():
        q = make_logits(shape, g)
        targets = make_targets(shape[0], shape[1], Ht, Wt, "blocks", ignore, g)
        add_new(name, q, targets, P, ratio, isr, temp, ignore, seed, LOGIT_SCALE)
    base = R.load_case(gold, "base")
    q = torch.from_numpy(gold[str(gold["base/logits"])])
    add_new("saturated", q, base["targets"], base["P"], base["ratio"], base["isr"], base["temperature"], base["ignore"], 2300,
            8.0 * LOGIT_SCALE, x_of="base")
    out["cases"] = np.asarray(names)

    for name in gold["kl_cases"]:
        mom = torch.from_numpy(gold[f"kl/{name}/moments"]).clone().requires_grad_(True)
        kl = DGD(mom).kl().mean()
        out[f"kl/{name}/grad_moments"] = torch.autograd.grad(kl, mom)[0].numpy()
    out["kl_cases"] = np.asarray([str(n) for n in gold["kl_cases"]])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()

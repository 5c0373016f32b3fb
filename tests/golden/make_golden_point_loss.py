"""Writes tests/golden/point_loss.npz by RUNNING the reference's own stage-1 loss functions on the CPU (only where the
reference checkout exists): SegmentationLosses.point_loss (ldmseg/trainers/losses.py) and DiagonalGaussianDistribution.kl
(ldmseg/models/vae.py).  Packages the reference imports at module level but that are not installed are handed out as MagicMock
packages by a sys.meta_path finder (make_golden_loss.py).  Nothing of the reference is copied: the fixture holds the inputs,
the seeds, the values its functions returned, the shapes it drew and the index sets its torch.topk calls selected.

Per case the seed is the first one from the case's start seed on at which EVERY row passes the threshold-gap condition: the
kU-th and (kU+1)-th largest uncertainty differ by more than 1e-4 * max(1, |u|).  A few ulps of difference in another
implementation's interpolation then cannot change the selected set, which is what lets the sets be compared exactly.

Logits are multiples of 1/16 in [-8, 8) stored as int8 (the fixture stays small; the value is exact in fp32).

    python tests/golden/make_golden_point_loss.py [path of the reference checkout]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_loss import StubFinder, STUBS  # noqa: E402

OUT = os.path.join(HERE, "point_loss.npz")
GAP = 1e-4
LOGIT_SCALE = 1.0 / 16.0

# name: logits, (Ht, Wt), P, oversample_ratio, importance_sample_ratio, temperature, ignore_label, validity mask, target kind
#   target kinds: 'blocks' every image has segments; 'one_empty' image 1 is all ignore_label; 'empty' no segment at all
CASES = {
    "base":        ("x16", (64, 48), 64, 3, 0.75, 1.0, 0, False, "blocks"),
    "odd_points":  ("x16", (32, 32), 257, 3, 0.75, 1.0, 0, False, "blocks"),
    "c128":        ("x128", (48, 80), 64, 3, 0.75, 1.0, 0, False, "blocks"),
    "ratio0":      ("x16", (64, 48), 64, 0, 0.75, 1.0, 0, False, "blocks"),
    "valid_mask":  ("x16", (64, 48), 64, 3, 0.75, 1.0, 0, True, "blocks"),
    "one_empty":   ("x16", (64, 48), 64, 3, 0.75, 1.0, 0, False, "one_empty"),
    "no_segment":  ("x16", (64, 48), 64, 3, 0.75, 1.0, 0, False, "empty"),
    "temperature": ("x16", (64, 48), 64, 3, 0.75, 0.5, 0, False, "blocks"),
    "all_uncertain": ("x16", (64, 48), 64, 3, 1.0, 1.0, 0, False, "blocks"),
    "ignore3":     ("x16", (64, 48), 64, 3, 0.75, 1.0, 3, True, "blocks"),
}
LOGITS = {"x16": (2, 16, 32, 32), "x128": (3, 128, 24, 40)}


def import_reference(ref):
    import importlib.util
    absent = [n for n in STUBS + ("scipy",) if n not in sys.modules and importlib.util.find_spec(n) is None]
    # ldmseg/models/__init__.py pulls in the CLIP descriptors; an installed transformers does not import beside a stubbed
    # torchvision, and neither function run here touches it
    sys.meta_path.insert(0, StubFinder(absent + ["transformers"]))
    sys.path.insert(0, ref)
    from ldmseg.trainers.losses import SegmentationLosses
    from ldmseg.models.vae import DiagonalGaussianDistribution
    return SegmentationLosses, DiagonalGaussianDistribution


def make_logits(shape, g):
    q = torch.clamp(torch.round(torch.randn(shape, generator=g) * 2.0 / LOGIT_SCALE), -128, 127).to(torch.int8)
    return q


def make_targets(B, C, Ht, Wt, kind, ignore, g):
    """Blocky maps: 8 x 8 blocks of ids from [0, C), so that sampled points fall on both sides of label edges."""
    coarse = torch.randint(0, min(C, 12), (B, (Ht + 7) // 8, (Wt + 7) // 8), generator=g)
    t = coarse.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)[:, :Ht, :Wt].contiguous()
    if kind == "one_empty":
        t[1] = ignore
    elif kind == "empty":
        t[:] = ignore
    return t.to(torch.int64)


def run_case(SL, x, targets, masks, P, ratio, isr, temperature, ignore, seed):
    """-> (losses, draw shapes, [(uncertainties [rows,S], indices [rows,kU])] of the selection calls, in call order)."""
    crit = SL(num_points=P, oversample_ratio=ratio, importance_sample_ratio=isr, ignore_label=ignore, temperature=temperature)
    real_topk, real_rand = torch.topk, torch.rand
    picks, shapes = [], []

    def topk(inp, k, dim=-1, **kw):
        r = real_topk(inp, k, dim=dim, **kw)
        if inp.dim() == 2:                                  # the selection (detectron2_utils.py:56), not the top two of :300
            picks.append((inp.clone(), r[1].clone()))
        return r

    def rand(*size, **kw):
        shapes.append(tuple(int(s) for s in (size[0] if len(size) == 1 and not isinstance(size[0], int) else size)))
        return real_rand(*size, **kw)
    torch.topk, torch.rand = topk, rand
    try:
        torch.manual_seed(seed)
        with torch.no_grad():
            losses = crit.point_loss(x, targets.clone(), False, None if masks is None else masks.clone())
    finally:
        torch.topk, torch.rand = real_topk, real_rand
    return losses, shapes, picks


def gaps_ok(picks, kU):
    for unc, _ in picks:
        if kU >= unc.shape[1]:
            continue
        v = torch.sort(unc, dim=1, descending=True)[0]
        a, b = v[:, kU - 1], v[:, kU]
        if not bool(((a - b) > GAP * torch.clamp(torch.maximum(a.abs(), b.abs()), min=1.0)).all()):
            return False
    return True


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LDMSEG_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "ldmseg")):
        print("reference checkout not given (argument or LDMSEG_REFERENCE); nothing to do")
        return
    SL, DGD = import_reference(ref)
    g = torch.Generator().manual_seed(31)
    out = {"logit_scale": np.float32(LOGIT_SCALE)}
    logits = {}
    for name, shape in LOGITS.items():
        q = make_logits(shape, g)
        out[name] = q.numpy()
        logits[name] = q.float() * LOGIT_SCALE
    names = []
    for i, (name, (xn, (Ht, Wt), P, ratio, isr, temp, ignore, with_mask, kind)) in enumerate(CASES.items()):
        x = logits[xn]
        B, C = x.shape[:2]
        targets = make_targets(B, C, Ht, Wt, kind, ignore, g)
        masks = None
        if with_mask:
            m = torch.rand(B, 1, (Ht + 15) // 16, (Wt + 15) // 16, generator=g) < 0.7
            masks = m.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)[:, :, :Ht, :Wt].float().contiguous()
        kU = int(isr * P)
        seed = 100 * (i + 1)
        while True:
            losses, shapes, picks = run_case(SL, x, targets, masks, P, ratio, isr, temp, ignore, seed)
            if gaps_ok(picks, kU):
                break
            seed += 1
        eff = targets.clone()
        if masks is not None:
            eff[~masks[:, 0].bool()] = ignore
        n_masks = sum(int((torch.unique(t) != ignore).sum()) for t in eff)
        names.append(name)
        k = f"{name}/"
        out[k + "logits"] = np.asarray(xn)
        out[k + "targets"] = targets.numpy().astype(np.uint8)
        if masks is not None:
            out[k + "masks"] = masks.numpy().astype(np.uint8)
        out[k + "params"] = np.asarray([P, ratio, isr, temp, ignore], dtype=np.float64)
        out[k + "seed"] = np.int64(seed)
        out[k + "num_masks"] = np.int64(n_masks)
        out[k + "ce"] = np.float32(losses["ce"])
        out[k + "mask"] = np.float32(losses["mask"])
        out[k + "draw_shapes"] = np.asarray([s + (0,) * (3 - len(s)) for s in shapes], dtype=np.int64).reshape(-1, 3)
        assert len(picks) == (0 if ratio == 0 else (2 if n_masks else 1)), (name, len(picks))
        for tag, (_, idx) in zip(("ce", "mask"), picks):
            out[k + f"selected_{tag}"] = torch.sort(idx, dim=1)[0].numpy().astype(np.int32)
        print(f"{name}: seed {seed} masks {n_masks} ce {float(losses['ce'])!r} mask {float(losses['mask'])!r} draws {shapes}")
    out["cases"] = np.asarray(names)
    # KL: moments [B, 8, l, l]; the second set reaches both clamps of the log-variance
    kl_names = []
    for name, (B, l, scale) in {"small": (2, 8, 1.0), "clamped": (3, 12, 25.0)}.items():
        mom = torch.randn(B, 8, l, l, generator=g)
        mom[:, 4:] *= scale
        kl = DGD(mom).kl()
        out[f"kl/{name}/moments"] = mom.numpy()
        out[f"kl/{name}/per_image"] = kl.numpy()
        out[f"kl/{name}/mean"] = np.float32(torch.mean(kl))
        kl_names.append(name)
    out["kl_cases"] = np.asarray(kl_names)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

"""Torch restatement of the stage-1 loss as csrc/point_loss.hip computes it (this project's code, written from the kernels'
rules): effective targets, class presence, rows by image then class id, uncertainties, an exact top-kU with ties to the lower
index, the point losses.  tests/test_point_loss_cpu.py pins it to the reference's own values (tests/golden/point_loss.npz,
written by tests/golden/make_golden_point_loss.py); tools/ae_loss_cost.py times it on the GPU as the torch-op chain."""
import numpy as np
import torch
import torch.nn.functional as F


def load_case(gold, name, device="cpu"):
    """-> dict(x, targets, masks, P, ratio, isr, temperature, ignore, seed, ...) of one fixture case."""
    k = name + "/"
    P, ratio, isr, temp, ignore = gold[k + "params"].tolist()
    x = torch.from_numpy(gold[str(gold[k + "logits"])].astype(np.float32) * float(gold["logit_scale"])).to(device)
    masks = torch.from_numpy(gold[k + "masks"]).float().to(device) if k + "masks" in gold else None
    sel = {t: gold[k + f"selected_{t}"] for t in ("ce", "mask") if k + f"selected_{t}" in gold}
    return dict(x=x, targets=torch.from_numpy(gold[k + "targets"].astype(np.int64)).to(device), masks=masks, P=int(P),
                ratio=int(ratio) if float(ratio).is_integer() else ratio, isr=isr, temperature=temp, ignore=int(ignore),
                seed=int(gold[k + "seed"]), num_masks=int(gold[k + "num_masks"]), ce=gold[k + "ce"], mask=gold[k + "mask"],
                draw_shapes=[tuple(int(v) for v in s) for s in gold[k + "draw_shapes"]], selected=sel)


def sample(x, u, mode="bilinear"):
    """x [R,C,H,W] at u [R,n,2] in [0,1]^2 -> [R,C,n]"""
    return F.grid_sample(x, 2.0 * u[:, :, None, :] - 1.0, mode=mode, align_corners=False, padding_mode="zeros")[..., 0]


def effective_targets(targets, masks, ignore):
    if masks is None:
        return targets
    return torch.where(masks[:, 0] != 0, targets, torch.full_like(targets, ignore))


def mask_rows(eff, num_classes, ignore):
    """int64 [N]: b * C + c of every id c != ignore present in image b, by image, then class id"""
    B = eff.shape[0]
    present = torch.zeros(B, num_classes + 1, dtype=torch.bool, device=eff.device)
    ids = torch.where(eff != ignore, eff, torch.full_like(eff, num_classes))          # ignored pixels go to a spare column
    present.scatter_(1, ids.view(B, -1), True)
    return torch.nonzero(present[:, :num_classes].reshape(-1)).flatten()


def select(unc, k):
    """ascending indices of the k largest per row; ties to the lower index"""
    order = torch.sort(unc, dim=1, descending=True, stable=True)[1][:, :k]
    return torch.sort(order, dim=1)[0]


def choose_points(unc_fn, over, fresh, kU):
    """(points [R,P,2], selected [R,kU] or None) from the oversampled and the fresh draws"""
    if over is None:
        return fresh, None
    sel = select(unc_fn(over), kU)
    pts = torch.gather(over, 1, sel[:, :, None].expand(-1, -1, 2))
    return (pts if fresh is None else torch.cat([pts, fresh], dim=1)), sel


def point_loss(x, targets, masks, draws, P, ratio, isr, temperature=1.0, ignore=0, num_masks=None):
    """draws: {'ce_over', 'ce_fresh', 'mask_over', 'mask_fresh'} -> tensors (absent: not drawn).  -> dict(ce, mask, bce, dice,
    selected_ce, selected_mask, rows)"""
    B, C = x.shape[:2]
    kU = int(isr * P) if ratio > 0 else 0
    eff = effective_targets(targets, masks, ignore)

    def ce_unc(u):
        top = torch.topk(sample(x, u), 2, dim=1)[0]
        return top[:, 1] - top[:, 0]
    pts, sel_ce = choose_points(ce_unc, draws.get("ce_over"), draws.get("ce_fresh"), kU)
    labels = sample(eff[:, None].float(), pts, mode="nearest")[:, 0].long()
    ce = F.cross_entropy(sample(x, pts) / temperature, labels, reduction="mean", ignore_index=ignore)
    rows = mask_rows(eff, C, ignore)
    N = int(rows.numel())
    out = dict(ce=ce, rows=rows, selected_ce=sel_ce, selected_mask=None)
    if N == 0:
        zero = torch.zeros((), device=x.device)
        out.update(mask=zero, bce=zero, dice=zero)
        return out
    rb, rc = rows // C, rows % C
    xm = x[rb, rc][:, None]                                            # [N,1,H,W]
    tm = (eff[rb] == rc[:, None, None]).float()[:, None]               # [N,1,Ht,Wt]
    pts, sel_m = choose_points(lambda u: -sample(xm, u)[:, 0].abs(), draws.get("mask_over"), draws.get("mask_fresh"), kU)
    logit, t = sample(xm, pts)[:, 0], sample(tm, pts)[:, 0]
    nm = float(max(N, 1)) if num_masks is None else float(num_masks)
    bce = F.binary_cross_entropy_with_logits(logit, t, reduction="none").mean(1).sum() / nm
    s = logit.sigmoid()
    dice = (1 - (2 * (s * t).sum(-1) + 1) / (s.sum(-1) + t.sum(-1) + 1)).sum() / nm
    out.update(mask=bce + dice, bce=bce, dice=dice, selected_mask=sel_m)
    return out


def gaussian_kl(moments):
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = logvar.clamp(-30.0, 20.0)
    return 0.5 * (mean * mean + logvar.exp() - 1.0 - logvar).sum(dim=[1, 2, 3])

"""TEST INFRASTRUCTURE ONLY - CPU restatements of the reference arithmetic behind the stage-1 (seg-VAE reconstruction)
evaluation: the SemsegMeter rule (ldmseg/evaluations/semseg_evaluation.py:24-47), the `compute_miou` tail
(ldmseg/trainers/trainers_ae.py:754-760) and the per-image post-processing of `TrainerAE.compute_pq` (:637-668).
Written from those lines, in the style of oracle/postprocess.py; product code must not import this.
"""
import numpy as np
import torch
import torch.nn.functional as F


def meter_counts(pred, gt, num_classes, ignore_index):
    """semseg_evaluation.py:26-33, one class at a time: int64 [3][K] = (tp | fp | fn)."""
    pred = np.asarray(pred).reshape(-1)
    gt = np.asarray(gt).reshape(-1)
    counted = gt != ignore_index
    out = np.zeros((3, num_classes), np.int64)
    for k in range(num_classes):
        is_t, is_p = (gt == k) & counted, (pred == k) & counted
        out[:, k] = int((is_t & is_p).sum()), int((is_p & ~is_t).sum()), int((is_t & ~is_p).sum())
    return out


def meter_scores(counts):
    """semseg_evaluation.py:41-47 as an explicit loop."""
    tp, fp, fn = counts
    jac = []
    for i in range(len(tp)):
        den = float(tp[i] + fp[i] + fn[i])
        jac.append(float(tp[i]) / (den if den > 1e-8 else 1e-8))
    return {"jaccards_all_categs": jac, "mIoU": sum(jac) / len(jac)}


def resize_align_corners(x, size):
    """trainers_ae.py:754 on [B,C,H,W] fp32."""
    return F.interpolate(x.float(), size=tuple(int(s) for s in size), mode="bilinear", align_corners=True)


def semseg_labels(volume, mask_th, ignore_label):
    """trainers_ae.py:755-760 on logits [B,C,h,w] that are already at the target size.  mask_th None / < 0: no threshold.
    Returns (preds int64 [B,h,w], max softmax probability, top-2 logit gap)."""
    volume = volume.float()
    preds = torch.argmax(volume, dim=1)
    probs = F.softmax(volume, dim=1).max(dim=1)[0]
    if mask_th is not None and mask_th >= 0:
        preds[probs < mask_th] = ignore_label
    top2 = volume.topk(2, dim=1)[0]
    return preds, probs, top2[:, 0] - top2[:, 1]


def ae_panoptic_postprocess(mask_pred_result, threshold_output=True, mask_th=0.5, count_th=512, overlap_th=0.5, ignore_label=0,
                            mask_rule="logit"):
    """One image of trainers_ae.py:637-668.  mask_pred_result [C,h,w] fp32 logits at the original size.  The overlap mask is
    `logit >= mask_th` (:656); mask_rule="sigmoid" gives the LDM trainer's rule instead (to tell the two apart in a test).
    Returns (panoptic_pred + 1 [h,w] int64 numpy, segments_info, raw labels, {"counts", "mask_counts"})."""
    x = mask_pred_result.float()
    panoptic_pred = torch.argmax(x, dim=0)                                       # :637
    if threshold_output:                                                          # :638-641
        probs = F.softmax(x, dim=0).max(dim=0)[0]
        panoptic_pred[probs < mask_th] = -1
    panoptic_pred = panoptic_pred.numpy()                                         # :644
    raw = panoptic_pred.copy()
    m = (torch.sigmoid(x) if mask_rule == "sigmoid" else x).numpy()
    C = x.shape[0]
    counts = np.zeros(C, np.int64)
    mask_counts = np.array([int((m[c] >= np.float32(mask_th)).sum()) for c in range(C)], np.int64)
    segments_info = []
    for label, count_i in zip(*np.unique(panoptic_pred, return_counts=True)):    # :648
        if label >= 0:
            counts[label] = count_i
        if count_i < count_th or label in {-1, ignore_label}:                     # :651-653
            panoptic_pred[panoptic_pred == label] = -1
            continue
        original_mask = m[label] >= np.float32(mask_th)                           # :656
        with np.errstate(divide="ignore"):
            ratio = np.float64((panoptic_pred == label).sum()) / np.float64(original_mask.sum())
        if ratio < overlap_th:                                                    # :657-659
            panoptic_pred[panoptic_pred == label] = -1
            continue
        segments_info.append({"id": int(label) + 1, "category_id": 1, "isthing": True})   # :661-667
    return panoptic_pred + 1, segments_info, raw, {"counts": counts, "mask_counts": mask_counts}


def segment_like_logits(B, C, H, W, seed, sharp=6.0):
    """Smooth class fields plus a little noise: maps with regions and few near-ties."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, C, max(2, H // 16), max(2, W // 16), generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * sharp
    return x + 0.3 * torch.randn(B, C, H, W, generator=g)


def block_targets(B, h, w, num_labels, seed, ignore_label=None, band=None):
    """Coarse random blocks [B,h,w] int64, optionally with a horizontal band of `ignore_label` rows."""
    g = np.random.RandomState(seed)
    out = np.zeros((B, h, w), np.int64)
    for b in range(B):
        out[b] = np.kron(g.randint(0, num_labels, (4, 4)), np.ones((h // 4 + 1, w // 4 + 1), np.int64))[:h, :w]
        if band is not None:
            out[b, band[0]:band[1]] = ignore_label
    return torch.from_numpy(out)


def encode_bits(ids, n=7, fill_value=0.5, ignore_label=0):
    """ldmseg/data/coco.py:377-382 on [B,H,W] int64 ids: n bit planes (LSB first), `fill_value` where id == ignore_label."""
    bits = torch.stack([((ids >> k) & 1).float() for k in range(n)], dim=1)
    bits[(ids == ignore_label)[:, None].expand_as(bits)] = fill_value
    return bits

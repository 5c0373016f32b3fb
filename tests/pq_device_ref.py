"""numpy restatement of the device PQ meter (csrc/pq_meter.hip: pass A contingency table, pass B matching) from the
`np.unique` pair counts - what tests/test_pq_device_cpu.py folds through the evaluator and tests/test_pq_device_gpu.py holds
the kernel's table against.  Plain Python integers and float division, like pq_compute_annotations."""
import numpy as np

from ldmseg_amd.evaluations.panoptic_evaluation_agnostic import OFFSET, pq_slots


def inter_table(gt_ann, gt_ids, pred_ids, P, Gpad=None):
    """int64 [G(pad) + 2][P + 1]: row 0 void, rows 1..G the declared slots (ascending id), row G + 1 painted but undeclared;
    prediction ids outside 0..P are not counted (the kernel flags them)."""
    slots = pq_slots(gt_ann)
    ids = slots["ids"].tolist()
    G = len(ids)
    slot_of = {i: k for k, i in enumerate(ids)}
    tab = np.zeros(((G if Gpad is None else Gpad) + 2, P + 1), dtype=np.int64)
    pair, cnt = np.unique(np.asarray(gt_ids).astype(np.uint64) * np.uint64(OFFSET) + np.asarray(pred_ids).astype(np.uint64),
                          return_counts=True)
    for pr, n in zip(pair.tolist(), cnt.tolist()):
        g, p = pr // OFFSET, pr % OFFSET
        if p > P:
            continue
        row = 0 if g == 0 else slot_of[g] + 1 if g in slot_of else G + 1
        tab[row, p] += n
    return tab


def record(gt_ann, gt_ids, pred_ids, declared, P=None):
    """(tp, fp, fn, [matched IoUs in slot order], flags) of one pair; `declared`: the prediction ids of segments_info."""
    declared = sorted(int(d) for d in declared)
    P = P or max([128] + declared)
    slots = pq_slots(gt_ann)
    G = len(slots["ids"])
    tab = inter_table(gt_ann, gt_ids, pred_ids, P).tolist()
    flags = 4 if int(np.asarray(pred_ids).max()) > P or int(np.asarray(pred_ids).min()) < 0 else 0
    area_pred = [sum(tab[r][p] for r in range(G + 2)) for p in range(P + 1)]
    area_gt = [int(slots["area"][g]) if slots["area"][g] >= 0 else sum(tab[g + 1]) for g in range(G)]
    for p in range(1, P + 1):
        if area_pred[p] > 0 and p not in declared:
            flags |= 1
        if area_pred[p] == 0 and p in declared:
            flags |= 2
    tp, ious, gm, pm = 0, [], set(), set()
    for g in range(G):
        if slots["crowd"][g]:
            continue
        for p in declared:
            n = tab[g + 1][p]
            if n <= 0:
                continue
            union = area_pred[p] + area_gt[g] - n - tab[0][p]
            if union == 0:
                flags |= 8
                continue
            iou = n / union
            if iou > 0.5:
                tp += 1
                if g in gm or p in pm:
                    flags |= 8                  # the slot table holds one IoU per segment
                    continue
                ious.append(iou)
                gm.add(g)
                pm.add(p)
    fn = sum(1 for g in range(G) if not slots["crowd"][g] and g not in gm)
    fp = 0
    for p in declared:
        if p in pm or area_pred[p] == 0:
            continue
        ign = tab[0][p] + (tab[slots["last_crowd"] + 1][p] if slots["last_crowd"] >= 0 else 0)
        if ign / area_pred[p] > 0.5:
            continue
        fp += 1
    return (tp, fp, fn, ious, flags)

"""Class-agnostic panoptic-quality evaluation with the reference's call surface.

Stands behind /root/reference/ldmseg/evaluations/panoptic_evaluation_agnostic.py::PanopticEvaluatorAgnostic
(`reset` :74, `process` :96-126, `evaluate` :128-185, `pq_compute` :188-230) as `compute_pq` drives it
(trainers_ldm_cond.py:1205-1207, 1315, 1335).  This is host-side bookkeeping in the reference too (numpy on the CPU,
run once per evaluation) and stays there; two things differ in mechanism, not in result:

* the reference delegates the metric to **panopticapi** (`pq_compute_multi_core`, pinned only as the git dependency
  `panopticapi @ git+https://github.com/cocodataset/panopticapi.git` in the reference's environment; absent from this
  image and from /root/reference).  `pq_compute_annotations` below restates its published algorithm
  (panopticapi/evaluation.py, `pq_compute_single_core` + `PQStat.pq_average`): segments match when IoU > 0.5 with the
  union reduced by the prediction's overlap with VOID, crowd ground truth is never a false negative, an unmatched
  prediction is no false positive when more than half of it lies on VOID / crowd, PQ = sum IoU / (TP + FP/2 + FN/2).
  PARITY UNPINNED by the reference (no tests, dependency absent); known-answer tests in tests/test_pq_cpu.py.
* the cross-rank gather of per-image predictions (`detectron2.utils.comm.gather` of pickled dicts over a gloo side
  group, :129-131) is `torch.distributed.gather_object` on the default group's CPU/gloo companion; the predictions are
  tiny (one id map per image), so this is not the latents all-gather of the sampling path and needs no RCCL.

Beside that host route stands a device route (`process_device`): the panoptic maps stay on the GPU, one library call
per batch (`ldmseg_pq_match`, csrc/pq_meter.hip) counts the contingency table and does the matching, and `evaluate()` reads a
few numbers per image - (tp, fp, fn, matched IoUs, flags) - instead of decoding PNGs and sorting pixels.  The rule is the same
and so is the result, bit for bit: integer counts, IEEE double divisions, and the IoUs added one by one in the host rule's order.

Ground truth comes in the COCO panoptic format: a JSON with `annotations[*].segments_info` and one PNG per image whose
RGB encodes the segment id (id = R + 256 G + 256^2 B).  As in the reference every segment's category is rewritten to 1
(:59-72).  For data without a JSON (the reference's data/examples) `gt_from_png` derives the annotation from the PNG.
"""
import io
import json
import os
from collections import OrderedDict
from typing import Dict, List, Optional, Union

import numpy as np
import torch

VOID = 0
OFFSET = 256 * 256 * 256
G_MAX = 256          # LDMSEG_PQ_G_MAX (include/ldmseg_hip.h): declared ground-truth segments per image on the device route
P_MAX = 256          # largest prediction id there


def rgb2id(color: np.ndarray) -> np.ndarray:
    """COCO panoptic PNG colour -> segment id (panopticapi/utils.py rgb2id)."""
    color = np.asarray(color)
    if color.ndim == 3:
        c = color.astype(np.int64)
        return c[:, :, 0] + 256 * c[:, :, 1] + 256 * 256 * c[:, :, 2]
    return int(color[0] + 256 * color[1] + 256 * 256 * color[2])


def id2rgb(id_map: np.ndarray) -> np.ndarray:
    """segment id map [H,W] -> uint8 RGB [H,W,3] (panopticapi/utils.py id2rgb)."""
    ids = np.asarray(id_map).astype(np.int64)
    rgb = np.zeros(ids.shape + (3,), dtype=np.uint8)
    for i in range(3):
        rgb[..., i] = ids % 256
        ids = ids // 256
    return rgb


def gt_from_png(id_map: np.ndarray, image_id, file_name: str) -> dict:
    """Class-agnostic ground-truth annotation of one image from its id map (VOID = 0 carries no segment)."""
    ids, cnt = np.unique(id_map, return_counts=True)
    segs = [{"id": int(i), "category_id": 1, "iscrowd": 0, "area": int(c)} for i, c in zip(ids, cnt) if i != VOID]
    return {"image_id": image_id, "file_name": file_name, "segments_info": segs}


class PQStatCat(object):
    def __init__(self):
        self.iou, self.tp, self.fp, self.fn = 0.0, 0, 0, 0


def pq_compute_annotations(pairs, categories: Dict[int, dict], matched: Optional[list] = None):
    """pairs: iterable of (gt_ann, gt_ids [H,W], pred_ann, pred_ids [H,W]).  Returns {category_id: PQStatCat}.
    `matched` (optional list) receives every matched IoU in the order it is added to the running sum."""
    stat = {c: PQStatCat() for c in categories}
    for gt_ann, pan_gt, pred_ann, pan_pred in pairs:
        pan_gt = np.asarray(pan_gt).astype(np.uint64)
        pan_pred = np.asarray(pan_pred).astype(np.uint64)
        if pan_gt.shape != pan_pred.shape:
            raise ValueError(f"image {gt_ann['image_id']}: ground truth {pan_gt.shape} vs prediction {pan_pred.shape}")
        gt_segms = {el["id"]: dict(el) for el in gt_ann["segments_info"]}
        pred_segms = {el["id"]: dict(el) for el in pred_ann["segments_info"]}
        # areas of the predicted segments + sanity checks (every painted id is declared and vice versa)
        declared = set(pred_segms)
        labels, cnt = np.unique(pan_pred, return_counts=True)
        for label, c in zip(labels.tolist(), cnt.tolist()):
            if label not in pred_segms:
                if label == VOID:
                    continue
                raise KeyError(f"image {gt_ann['image_id']}: segment {label} is painted but not in segments_info")
            pred_segms[label]["area"] = c
            declared.discard(label)
            if pred_segms[label]["category_id"] not in categories:
                raise KeyError(f"image {gt_ann['image_id']}: segment {label} has unknown category")
        if declared:
            raise KeyError(f"image {gt_ann['image_id']}: segments {sorted(declared)} are in segments_info but not painted")
        for label, c in zip(*np.unique(pan_gt, return_counts=True)):
            if int(label) in gt_segms:
                gt_segms[int(label)].setdefault("area", int(c))
        # confusion counts
        pair_ids, inter = np.unique(pan_gt * np.uint64(OFFSET) + pan_pred, return_counts=True)
        gt_pred = {(int(p // OFFSET), int(p % OFFSET)): int(n) for p, n in zip(pair_ids.tolist(), inter.tolist())}
        gt_matched, pred_matched = set(), set()
        for (g, p), n in gt_pred.items():
            if g not in gt_segms or p not in pred_segms:
                continue
            if gt_segms[g].get("iscrowd", 0) == 1 or gt_segms[g]["category_id"] != pred_segms[p]["category_id"]:
                continue
            union = pred_segms[p]["area"] + gt_segms[g]["area"] - n - gt_pred.get((VOID, p), 0)
            iou = n / union
            if iou > 0.5:
                st = stat[gt_segms[g]["category_id"]]
                st.tp += 1
                st.iou += iou
                if matched is not None:
                    matched.append(iou)
                gt_matched.add(g)
                pred_matched.add(p)
        crowd_of_cat = {}
        for g, info in gt_segms.items():
            if g in gt_matched:
                continue
            if info.get("iscrowd", 0) == 1:
                crowd_of_cat[info["category_id"]] = g
                continue
            stat[info["category_id"]].fn += 1
        for p, info in pred_segms.items():
            if p in pred_matched:
                continue
            ign = gt_pred.get((VOID, p), 0)
            if info["category_id"] in crowd_of_cat:
                ign += gt_pred.get((crowd_of_cat[info["category_id"]], p), 0)
            if ign / info["area"] > 0.5:
                continue
            stat[info["category_id"]].fp += 1
    return stat


def pq_average(stat: Dict[int, PQStatCat], categories: Dict[int, dict], isthing: Optional[bool]):
    pq = sq = rq = 0.0
    n = 0
    per_class = {}
    for cid, info in categories.items():
        if isthing is not None and (info.get("isthing", 1) == 1) != isthing:
            continue
        st = stat[cid]
        if st.tp + st.fp + st.fn == 0:
            per_class[cid] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
            continue
        n += 1
        c_pq = st.iou / (st.tp + 0.5 * st.fp + 0.5 * st.fn)
        c_sq = st.iou / st.tp if st.tp else 0.0
        c_rq = st.tp / (st.tp + 0.5 * st.fp + 0.5 * st.fn)
        per_class[cid] = {"pq": c_pq, "sq": c_sq, "rq": c_rq}
        pq += c_pq
        sq += c_sq
        rq += c_rq
    if n == 0:
        return {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}, per_class
    return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class


def pq_compute(gt_json: dict, pred_json: dict, gt_maps: Dict, pred_maps: Dict):
    """`pq_compute` (:188-230) on in-memory data: gt_json / pred_json are COCO-panoptic dicts, gt_maps / pred_maps map
    image_id -> id map [H,W] (what the reference reads back from the PNG folders)."""
    categories = {el["id"]: el for el in gt_json["categories"]}
    preds = {el["image_id"]: el for el in pred_json["annotations"]}
    pairs = []
    for gt_ann in gt_json["annotations"]:
        iid = gt_ann["image_id"]
        if iid not in preds:
            continue                                                     # (:216-218: images without a prediction are skipped)
        pairs.append((gt_ann, gt_maps[iid], preds[iid], pred_maps[iid]))
    stat = pq_compute_annotations(pairs, categories)
    return pq_results(stat, categories), stat, len(preds)


def pq_results(stat: Dict[int, PQStatCat], categories: Dict[int, dict]) -> dict:
    results = {}
    for name, isthing in (("All", None), ("Things", True)):
        results[name], per_class = pq_average(stat, categories, isthing)
        if name == "All":
            results["per_class"] = per_class
    return results


def pq_slots(gt_ann: dict):
    """The declared ground-truth segments of one annotation as the device meter takes them: slots in ASCENDING id order.
    Returns {"ids": int32 [G], "crowd": uint8 [G], "area": int64 [G] (-1 = count it: the annotation gives none),
    "last_crowd": slot of the last crowd segment in ANNOTATION order or -1} - or None when the image has to take the host rule:
    more than G_MAX segments, an id of 0 (VOID) or >= 2^24 (beyond an RGB triple), a negative area.
    Follows pq_compute_annotations: a repeated id keeps its first position and its last entry (a dict), `iscrowd` counts when
    it equals 1, `crowd_of_cat` is overwritten in annotation order, and every category is the evaluator's single class."""
    segs = {el["id"]: el for el in gt_ann["segments_info"]}
    if len(segs) > G_MAX:
        return None
    for i, el in segs.items():
        if not isinstance(i, (int, np.integer)) or not 0 < int(i) < OFFSET or ("area" in el and int(el["area"]) < 0):
            return None
    order = sorted(segs)
    slot_of = {i: k for k, i in enumerate(order)}
    last_crowd = -1
    for i, el in segs.items():
        if el.get("iscrowd", 0) == 1:
            last_crowd = slot_of[i]
    return {"ids": np.asarray(order, dtype=np.int32).reshape(-1),
            "crowd": np.asarray([int(segs[i].get("iscrowd", 0) == 1) for i in order], dtype=np.uint8).reshape(-1),
            "area": np.asarray([int(segs[i]["area"]) if "area" in segs[i] else -1 for i in order], dtype=np.int64).reshape(-1),
            "last_crowd": last_crowd}


FLAG_UNDECLARED, FLAG_UNPAINTED, FLAG_RANGE, FLAG_AMBIGUOUS = 1, 2, 4, 8


def raise_for_flags(image_id, flags: int):
    """The host rule's errors for a device record's flags word (include/ldmseg_hip.h, ldmseg_pq_match)."""
    if flags & (FLAG_UNDECLARED | FLAG_RANGE):
        raise KeyError(f"image {image_id}: a segment is painted but not in segments_info")
    if flags & FLAG_UNPAINTED:
        raise KeyError(f"image {image_id}: a segment is in segments_info but not painted")
    if flags & FLAG_AMBIGUOUS:
        raise ValueError(f"image {image_id}: the annotation's areas contradict its map (a segment matched twice or an empty "
                         "union); score this image with process()")


def get_table(pq_res: dict) -> str:
    rows = ["|        |   PQ   |   SQ   |   RQ   | #categories |", "|:------:|:------:|:------:|:------:|:-----------:|"]
    for name in ("All", "Things", "Stuff"):
        if name in pq_res:
            r = pq_res[name]
            rows.append(f"| {name:^6} | {100 * r['pq']:6.3f} | {100 * r['sq']:6.3f} | {100 * r['rq']:6.3f} | {r['n']:^11} |")
    return "\n".join(rows)


class PanopticEvaluatorAgnostic(object):
    """reset() / process(file_names, image_ids, outputs) / evaluate() like the reference class.

    `meta` needs `panoptic_json` (COCO panoptic annotations) and `panoptic_root` (folder of ground-truth PNGs), as in
    the reference's dataset meta data; alternatively pass `gt_maps` / `gt_annotations` in memory (image_id -> id map /
    annotation dict), e.g. from `gt_from_png`.  Every ground-truth category becomes 1 ('object').

    `process_device` is the device route of `process` (same arguments, maps on the GPU, nothing copied to the host); both may
    be used in one evaluation.  `on_device=True` only records the caller's wish: `compute_pq` of the trainers then feeds
    `process_device`.
    """

    def __init__(self, output_dir: Optional[str] = None, meta: Optional[Dict] = None, gt_maps: Optional[Dict] = None,
                 gt_annotations: Optional[List[dict]] = None, group=None, on_device: bool = False):
        self._metadata = meta or {}
        self.on_device = bool(on_device)
        self._ann_by_id = None
        self.class_agnostic = True
        self._output_dir = output_dir
        self._group = group
        self._gt_maps = gt_maps
        self._gt_json = None
        if gt_annotations is not None:
            anns = [dict(a, segments_info=[dict(s, category_id=1) for s in a["segments_info"]]) for a in gt_annotations]
            self._gt_json = {"annotations": anns,
                             "categories": [{"id": 1, "name": "object", "supercategory": "object", "isthing": 1}]}
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        self.reset()

    def reset(self):
        self._predictions = []
        self.last_inter = None
        self._device_batches = []          # (stats [B,4] int32, match_iou [B,Gpad] double, [(entry, b, G)]) per process_device call

    # ------------------------------------------------------------------ device route
    def _annotation(self, image_id):
        if self._ann_by_id is None:
            self._ann_by_id = {a["image_id"]: a for a in self._load_gt()[0]["annotations"]}
        return self._ann_by_id.get(image_id)

    @staticmethod
    def _gt_ids_host(m) -> np.ndarray:
        """One ground-truth map (host or device, RGB bytes or ids) as int64 ids on the host."""
        if isinstance(m, torch.Tensor):
            m = m.cpu().numpy()
        m = np.asarray(m)
        return rgb2id(m) if m.ndim == 3 else m.astype(np.int64)

    def _host_record(self, gt_ann, gt_ids, segs, pred_ids):
        """The host rule on one pair, as a record; its KeyError is kept for evaluate()."""
        ious = []
        try:
            st = pq_compute_annotations([(gt_ann, gt_ids, {"image_id": gt_ann["image_id"], "segments_info": segs}, pred_ids)],
                                        {1: {"id": 1, "isthing": 1}}, matched=ious)[1]
        except KeyError as e:
            return (0, 0, 0, [], FLAG_UNPAINTED if "not painted" in str(e) else FLAG_UNDECLARED)
        return (st.tp, st.fp, st.fn, ious, 0)

    @torch.no_grad()
    def process_device(self, file_names: List[str], image_ids: List, outputs, gt_maps=None):
        """`process` with the maps left on the GPU.  `outputs`: what `process` takes (a list of {"panoptic_seg": (int map [h,w] on
        the GPU, segments_info)}) or the packed form of `GeneralVAESeg.decode_panoptic(..., packed=True)` ({"pan": flat int32
        buffer, "offsets": [B], "sizes": [B,2], "keep": uint8 [B,C] on the GPU}).  `gt_maps`: the batch's ground truth, one uint8
        RGB [h,w,3] or integer id [h,w] array / tensor per image, on the host or the device (a dataloader can prefetch them);
        by default the evaluator's own source.  One library call scores the batch; the results stay on the device until
        `evaluate()`.  An image beyond the device meter's limits (`pq_slots`, prediction ids above P_MAX) takes the host rule
        alone.  With `output_dir` the PNGs are still produced, which costs the copy."""
        import ctypes as C
        from .. import _lib
        B = len(image_ids)
        packed = isinstance(outputs, dict)
        if packed:
            pan, keep = outputs["pan"], outputs["keep"]
            sizes = np.ascontiguousarray(np.asarray(outputs["sizes"], dtype=np.int32).reshape(B, 2))
            offs = np.ascontiguousarray(np.asarray(outputs["offsets"], dtype=np.int64).reshape(B))
            P = int(keep.shape[1])
            if pan.dtype != torch.int32 or keep.dtype != torch.uint8 or not pan.is_cuda or not keep.is_cuda or P > P_MAX:
                raise ValueError("packed outputs: pan int32 and keep uint8 [B, C <= 256] on the GPU")
            pan, keep = pan.contiguous().view(-1), keep.contiguous()
            maps = [pan[int(offs[b]):int(offs[b]) + int(sizes[b, 0]) * int(sizes[b, 1])].view(int(sizes[b, 0]), int(sizes[b, 1]))
                    for b in range(B)]
            seg_lists = [None] * B
        else:
            maps = [o["panoptic_seg"][0] for o in outputs]
            seg_lists = [[dict(s, category_id=1, isthing=True) for s in o["panoptic_seg"][1]] for o in outputs]
            for m in maps:
                if not isinstance(m, torch.Tensor) or not m.is_cuda:
                    raise RuntimeError("process_device takes maps on the MI355X (process() is the host route)")
        dev = maps[0].device
        if self._output_dir and packed:
            keep_h = keep.cpu()
            seg_lists = [[{"id": int(c) + 1, "category_id": 1, "isthing": True} for c in torch.nonzero(keep_h[b]).flatten().tolist()]
                         for b in range(B)]
        gt_src = self._load_gt()[1] if gt_maps is None else None
        entries, dev_rows = [], []                                       # dev_rows: (b, entry, slots, gt map)
        for b in range(B):
            entry = {"image_id": image_ids[b], "file_name": os.path.splitext(os.path.basename(file_names[b]))[0] + ".png",
                     "segments_info": seg_lists[b], "pq_record": None}
            entries.append(entry)
            if self._output_dir:
                from PIL import Image
                with io.BytesIO() as out:
                    Image.fromarray(id2rgb(maps[b].cpu().numpy())).save(out, format="PNG")
                    entry["png_string"] = out.getvalue()
            gt_ann = self._annotation(image_ids[b])
            if gt_ann is None:
                continue                                                 # counted as a prediction, never scored (as in pq_compute)
            g = gt_maps[b] if gt_maps is not None else gt_src[image_ids[b]]
            if tuple(g.shape[:2]) != tuple(maps[b].shape):
                raise ValueError(f"image {image_ids[b]}: ground truth {tuple(g.shape[:2])} vs prediction {tuple(maps[b].shape)}")
            slots = pq_slots(gt_ann)
            ids_ok = packed or all(isinstance(s["id"], (int, np.integer)) and 0 < s["id"] <= P_MAX for s in seg_lists[b])
            if slots is None or not ids_ok:
                segs = seg_lists[b]
                if segs is None:
                    segs = [{"id": int(c) + 1, "category_id": 1} for c in torch.nonzero(keep[b].cpu()).flatten().tolist()]
                entry["pq_record"] = self._host_record(gt_ann, self._gt_ids_host(g), segs, maps[b].cpu().numpy())
                continue
            dev_rows.append((b, entry, slots, g))
        self._predictions += entries
        if not dev_rows:
            return
        n = len(dev_rows)
        # prediction maps: one flat int32 buffer + offsets
        if packed:
            p_off = np.ascontiguousarray(offs[[r[0] for r in dev_rows]])
            p_sizes = np.ascontiguousarray(sizes[[r[0] for r in dev_rows]])
        else:
            P = 128 if all(s["id"] <= 128 for r in dev_rows for s in seg_lists[r[0]]) else P_MAX
            flat = [maps[r[0]].to(torch.int32).contiguous().view(-1) for r in dev_rows]
            p_sizes = np.ascontiguousarray(np.asarray([tuple(maps[r[0]].shape) for r in dev_rows], dtype=np.int32))
            npix = p_sizes[:, 0].astype(np.int64) * p_sizes[:, 1]
            p_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64))
            pan = flat[0] if n == 1 else torch.cat(flat)
            keep_h = np.zeros((n, P), dtype=np.uint8)
            for k, r in enumerate(dev_rows):
                for sg in seg_lists[r[0]]:
                    keep_h[k, int(sg["id"]) - 1] = 1
        npix = p_sizes[:, 0].astype(np.int64) * p_sizes[:, 1]
        g_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64))
        total = int(npix.sum())
        # ground truth: RGB bytes as they are when every map is RGB (rgb2id rides on the load), int32 ids otherwise
        gts = [r[3] for r in dev_rows]
        fmt = 1 if all(x.ndim == 3 and x.dtype == (torch.uint8 if isinstance(x, torch.Tensor) else np.uint8) for x in gts) else 0

        def as_ids(x):
            if x.ndim == 3:
                x = self._gt_ids_host(x) if not isinstance(x, torch.Tensor) else \
                    (x[..., 0].to(torch.int32) + 256 * x[..., 1].to(torch.int32) + 65536 * x[..., 2].to(torch.int32))
            if isinstance(x, torch.Tensor):
                if x.dtype == torch.int32:
                    return x
                x = x.to(torch.int64)
                return torch.where((x < 0) | (x >= 2 ** 31), -1, x).to(torch.int32)          # ids no annotation can declare
            x = np.asarray(x)
            if x.dtype != np.int32:
                x = x.astype(np.int64)
                x = np.where((x < 0) | (x >= 2 ** 31), -1, x).astype(np.int32)
            return x
        if fmt == 0:
            gts = [as_ids(x) for x in gts]
        per = 3 if fmt == 1 else 1
        gdt = torch.uint8 if fmt == 1 else torch.int32
        if all(isinstance(x, torch.Tensor) and x.is_cuda for x in gts):
            flat = [x.contiguous().view(-1) for x in gts]
            gt_dev = flat[0] if n == 1 else torch.cat(flat)
        else:
            stage = torch.empty(total * per, dtype=gdt, pin_memory=True)                      # one upload for the batch
            for k, x in enumerate(gts):
                x = x.cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
                stage[int(g_off[k]) * per:(int(g_off[k]) + int(npix[k])) * per] = x.reshape(-1)
            gt_dev = stage.to(dev, non_blocking=True)
        # slot tables: one pinned byte buffer, one upload:  area int64 [n][Gpad] | ids int32 [n][Gpad] | meta int32 [n][2] | crowd u8 [n][Gpad]
        # (| keep u8 [n][P] when it is built here)
        counts = np.ascontiguousarray(np.asarray([len(r[2]["ids"]) for r in dev_rows], dtype=np.int32))
        Gpad = max(1, int(counts.max()))
        o_area, o_ids, o_meta = 0, 8 * n * Gpad, 12 * n * Gpad
        o_crowd = o_meta + 8 * n
        o_keep = o_crowd + n * Gpad
        nbytes = o_keep + (0 if packed else n * P)
        tab = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)
        tnp = tab.numpy()
        area = tnp[o_area:o_ids].view(np.int64).reshape(n, Gpad)
        ids = tnp[o_ids:o_meta].view(np.int32).reshape(n, Gpad)
        meta = tnp[o_meta:o_crowd].view(np.int32).reshape(n, 2)
        crowd = tnp[o_crowd:o_keep].reshape(n, Gpad)
        for k, r in enumerate(dev_rows):
            G = int(counts[k])
            area[k, :G], ids[k, :G], crowd[k, :G] = r[2]["area"], r[2]["ids"], r[2]["crowd"]
            meta[k] = (G, r[2]["last_crowd"])
        if not packed:
            tnp[o_keep:] = keep_h.reshape(-1)
        tab_dev = tab.to(dev, non_blocking=True)
        base = tab_dev.data_ptr()
        if packed:
            sel = [r[0] for r in dev_rows]
            keep_dev = keep if sel == list(range(B)) else keep[torch.as_tensor(sel, device=dev)].contiguous()
            keep_ptr = keep_dev.data_ptr()
        else:
            keep_ptr = base + o_keep
        inter = torch.empty(n, Gpad + 2, P + 1, dtype=torch.int32, device=dev)
        stats = torch.empty(n, 4, dtype=torch.int32, device=dev)
        miou = torch.empty(n, Gpad, dtype=torch.float64, device=dev)
        hp = lambda a: C.c_void_p(a.ctypes.data)
        vp = C.c_void_p
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ldmseg_pq_match(
                _lib.ptr(pan), _lib.ptr(gt_dev), fmt, n, hp(p_sizes), hp(p_off), hp(g_off), vp(keep_ptr), P, hp(counts), Gpad,
                vp(base + o_ids), vp(base + o_crowd), vp(base + o_area), vp(base + o_meta), _lib.ptr(inter), _lib.ptr(stats),
                _lib.ptr(miou), _lib.stream_ptr(dev)), "ldmseg_pq_match")
        self._device_batches.append((stats, miou, [(r[1], k, int(counts[k])) for k, r in enumerate(dev_rows)]))
        self.last_inter = inter              # the most recent batch's contingency table [n][Gpad + 2][P + 1], device-scored images in order

    def add_records(self, file_names: List[str], image_ids: List, records):
        """Per-image records (tp, fp, fn, [matched IoUs in ascending ground-truth id order], flags) scored elsewhere."""
        for file_name, image_id, r in zip(file_names, image_ids, records):
            tp, fp, fn, ious, flags = r
            self._predictions.append({"image_id": image_id, "file_name": os.path.splitext(os.path.basename(file_name))[0] + ".png",
                                      "segments_info": None,
                                      "pq_record": (int(tp), int(fp), int(fn), [float(v) for v in ious], int(flags))})

    def _materialise(self):
        """The ONE device-to-host read: every pending batch's (stats | matched IoUs) in one buffer -> the entries' records."""
        if not self._device_batches:
            return
        parts = []
        for stats, miou, _ in self._device_batches:
            parts += [stats.view(torch.float64).reshape(-1), miou.reshape(-1)]                # (int32 pairs ride as raw 8-byte words)
        host = torch.cat(parts).cpu()
        o = 0
        for stats, miou, rows in self._device_batches:
            n, Gpad = miou.shape
            st = host[o:o + 2 * n].view(torch.int32).reshape(n, 4).tolist()
            o += 2 * n
            io_ = host[o:o + n * Gpad].reshape(n, Gpad).tolist()
            o += n * Gpad
            for entry, k, G in rows:
                tp, fp, fn, flags = st[k]
                entry["pq_record"] = (tp, fp, fn, [v for v in io_[k][:G] if v != 0.0], flags)
        self._device_batches = []

    def _evaluate_records(self, predictions, gt_json, gt_maps):
        """The fold of per-image records (and, for images that came through `process`, of the host rule on that one pair) into
        one PQStatCat, walking the ground-truth annotations in order and adding every IoU individually: the running sum is built
        in the order pq_compute_annotations builds it."""
        from PIL import Image
        categories = {el["id"]: el for el in gt_json["categories"]}
        preds = {p["image_id"]: p for p in predictions}                   # the last entry of an image id wins
        stat = {c: PQStatCat() for c in categories}
        st = stat[1]
        for gt_ann in gt_json["annotations"]:
            p = preds.get(gt_ann["image_id"])
            if p is None:
                continue
            if "pq_record" in p:
                tp, fp, fn, ious, flags = p["pq_record"]
                raise_for_flags(gt_ann["image_id"], flags)
            else:
                ious = []
                pred_ids = rgb2id(np.asarray(Image.open(io.BytesIO(p["png_string"])).convert("RGB")))
                one = pq_compute_annotations([(gt_ann, gt_maps[gt_ann["image_id"]], p, pred_ids)], categories, matched=ious)[1]
                tp, fp, fn = one.tp, one.fp, one.fn
            st.tp += tp
            st.fp += fp
            st.fn += fn
            for v in ious:
                st.iou += v
        return pq_results(stat, categories), stat, len(preds)

    def process(self, file_names: List[str], image_ids: List, outputs: List[Dict[str, Union[torch.Tensor, np.ndarray, tuple]]]):
        from PIL import Image
        for file_name, image_id, output in zip(file_names, image_ids, outputs):
            panoptic_img, segments_info = output["panoptic_seg"]
            if isinstance(panoptic_img, torch.Tensor):
                panoptic_img = panoptic_img.cpu().numpy()
            segs = [dict(s, category_id=1, isthing=True) for s in segments_info]
            png_name = os.path.splitext(os.path.basename(file_name))[0] + ".png"
            with io.BytesIO() as out:
                Image.fromarray(id2rgb(panoptic_img)).save(out, format="PNG")
                self._predictions.append({"image_id": image_id, "file_name": png_name, "png_string": out.getvalue(),
                                          "segments_info": segs})

    def _gather(self):
        """All ranks' predictions on rank 0 (detectron2 comm.gather, :129-131)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(self._group) == 1:
            return [self._predictions], True
        rank, world = dist.get_rank(self._group), dist.get_world_size(self._group)
        dist.barrier(group=self._group)                                   # comm.synchronize()
        gathered = [None] * world if rank == 0 else None
        dist.gather_object(self._predictions, gathered, dst=0, group=self._group)
        return gathered, rank == 0

    def _load_gt(self):
        from PIL import Image
        if self._gt_json is None:
            with open(self._metadata["panoptic_json"], "r") as f:
                gt = json.load(f)
            for anno in gt["annotations"]:                                # (:65-68) class agnostic ground truth
                for seg in anno["segments_info"]:
                    seg["category_id"] = 1
            gt["categories"] = [{"id": 1, "name": "object", "supercategory": "object", "isthing": 1}]
            self._gt_json = gt
        if self._gt_maps is None:
            root = self._metadata["panoptic_root"]
            self._gt_maps = LazyPngMaps(root, {a["image_id"]: a["file_name"] for a in self._gt_json["annotations"]})
        return self._gt_json, self._gt_maps

    def evaluate(self):
        from PIL import Image
        self._materialise()
        gathered, is_main = self._gather()
        if not is_main:
            return None
        predictions = [p for part in gathered for p in part]
        gt_json, gt_maps = self._load_gt()
        if any("pq_record" in p for p in predictions):
            return self._evaluate_with_records(predictions, gt_json, gt_maps)
        pred_maps = {}
        for p in predictions:
            pred_maps[p["image_id"]] = rgb2id(np.asarray(Image.open(io.BytesIO(p["png_string"])).convert("RGB")))
            if self._output_dir:
                with open(os.path.join(self._output_dir, p["file_name"]), "wb") as f:
                    f.write(p["png_string"])
        pred_json = {"annotations": [{k: v for k, v in p.items() if k != "png_string"} for p in predictions],
                     "categories": gt_json["categories"]}
        if self._output_dir:
            with open(os.path.join(self._output_dir, "predictions.json"), "w") as f:
                json.dump(pred_json, f)
        pq_res, stat, num_preds = pq_compute(gt_json, pred_json, gt_maps, pred_maps)
        return self._result(pq_res, stat, num_preds)

    def _evaluate_with_records(self, predictions, gt_json, gt_maps):
        if self._output_dir:
            for p in predictions:
                if "png_string" in p:
                    with open(os.path.join(self._output_dir, p["file_name"]), "wb") as f:
                        f.write(p["png_string"])
            pred_json = {"annotations": [{k: v for k, v in p.items() if k not in ("png_string", "pq_record")} for p in predictions],
                         "categories": gt_json["categories"]}
            with open(os.path.join(self._output_dir, "predictions.json"), "w") as f:
                json.dump(pred_json, f)
        return self._result(*self._evaluate_records(predictions, gt_json, gt_maps))

    def _result(self, pq_res, stat, num_preds):
        res = {"PQ": 100 * pq_res["All"]["pq"], "SQ": 100 * pq_res["All"]["sq"], "RQ": 100 * pq_res["All"]["rq"],
               "PQ_th": 100 * pq_res["Things"]["pq"], "SQ_th": 100 * pq_res["Things"]["sq"], "RQ_th": 100 * pq_res["Things"]["rq"]}
        st = stat[1]
        res["precision"] = 100 * st.tp / (st.tp + st.fp + 1e-8)
        res["recall"] = 100 * st.tp / (st.tp + st.fn + 1e-8)
        res["num_predictions"] = num_preds
        self.table = get_table(pq_res)
        return OrderedDict({"panoptic_seg": res})


class LazyPngMaps(object):
    """image_id -> id map, read from a folder of COCO panoptic PNGs on access."""

    def __init__(self, root: str, names: Dict):
        self.root, self.names = root, names

    def __getitem__(self, image_id):
        from PIL import Image
        return rgb2id(np.asarray(Image.open(os.path.join(self.root, self.names[image_id])).convert("RGB")))

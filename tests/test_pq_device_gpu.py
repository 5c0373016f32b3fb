"""The device PQ meter on the MI355X: `ldmseg_pq_match` (csrc/pq_meter.hip) through `PanopticEvaluatorAgnostic.process_device`.
The reference throughout is the committed host route on host copies of the same maps: `pq_compute_annotations` for the
per-image records and `process` + `evaluate` for the result dict; the contingency table is held against `np.unique` pair counts
(tests/pq_device_ref.py).  Everything is integers or IEEE double divisions of the same integers, so every comparison is ==."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from ldmseg_amd.evaluations import PanopticEvaluatorAgnostic, id2rgb
from ldmseg_amd.evaluations.panoptic_evaluation_agnostic import G_MAX, gt_from_png

import pq_device_ref as ref
import semseg_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 257), (7, 13), (33, 70), (16, 16), (255, 1), (300, 257)]
GT_COUNTS = [0, 1, 2, 37, G_MAX]


def segs_of(pred, extra=()):
    return [{"id": int(i), "category_id": 1, "isthing": True} for i in sorted(set(np.unique(pred).tolist()) - {0} | set(extra))]


def out_dev(pred, segs=None):
    return {"panoptic_seg": (torch.from_numpy(np.ascontiguousarray(pred)).to(DEV), segs_of(pred) if segs is None else segs)}


def out_host(pred, segs=None):
    return {"panoptic_seg": (np.asarray(pred), segs_of(pred) if segs is None else segs)}


def make_case(h, w, G, big_ids, style, seed, P=128, undeclared=True):
    """-> (gt ids [h,w] int64, annotation, prediction [h,w] int32).  G declared ids (up to 2^24 - 1 or 1..G); the map paints
    declared ids, void and (optionally) two undeclared ids; blocky maps are cells whose prediction mostly follows the ground
    truth, shifted by a pixel (matches exist), random maps draw every pixel on its own (every pair occurs)."""
    rng = np.random.RandomState(seed)
    if big_ids:
        ids = np.unique(np.concatenate([rng.randint(1, 1 << 24, size=2 * G + 2), [(1 << 24) - 1]]))
        ids = np.sort(rng.permutation(ids)[:G]) if G else ids[:0]
        if G:
            ids[-1] = (1 << 24) - 1
    else:
        ids = np.arange(1, G + 1)
    extra = [int(x) for x in ((1 << 24) - 7, G + 5) if x not in set(ids.tolist())] if undeclared else []
    palette = np.asarray([0] + ids.tolist() + extra, dtype=np.int64)                 # choice 0 = void
    if style == "random":
        choice = rng.randint(0, len(palette), size=(h, w))
        pred = rng.randint(0, P + 1, size=(h, w))
    else:
        ny, nx = min(h, 6), min(w, 7)
        cy, cx = np.arange(h) * ny // h, np.arange(w) * nx // w
        cell_choice = rng.randint(0, len(palette), size=(ny, nx))
        cell_pred = np.where(rng.rand(ny, nx) < 0.7, cell_choice % (P + 1), rng.randint(0, P + 1, size=(ny, nx)))
        choice = cell_choice[cy[:, None], cx[None, :]]
        pred = np.roll(cell_pred[cy[:, None], cx[None, :]], (1 if h > 2 else 0, 1 if w > 2 else 0), axis=(0, 1))
    gt = palette[choice]
    order = rng.permutation(G)
    ann = {"image_id": 0, "file_name": "0.png",
           "segments_info": [{"id": int(ids[k]), "category_id": 1, "iscrowd": int(rng.rand() < 0.15)} for k in order]}
    return gt, ann, pred.astype(np.int32)


def host_dict(anns, gts, preds, segs=None):
    ev = PanopticEvaluatorAgnostic(gt_maps={a["image_id"]: g for a, g in zip(anns, gts)}, gt_annotations=anns)
    ev.process([f"{a['image_id']}.jpg" for a in anns], [a["image_id"] for a in anns],
               [out_host(p, None if segs is None else segs[i]) for i, p in enumerate(preds)])
    return ev.evaluate(), ev.table


def check_batch(anns, gts, preds, gt_feed=None, P=128, call_sizes=None):
    """process_device on the pairs (all in one call, or in calls of `call_sizes`), then: table == np.unique counts, every record ==
    the host rule's record, result dict and table == the host route's."""
    anns = [dict(a, image_id=i) for i, a in enumerate(anns)]
    ev = PanopticEvaluatorAgnostic(gt_maps={i: g for i, g in enumerate(gts)}, gt_annotations=anns)
    lo = 0
    for n in call_sizes or [len(anns)]:
        idx = list(range(lo, lo + n))
        ev.process_device([f"{i}.jpg" for i in idx], idx, [out_dev(preds[i]) for i in idx],
                          gt_maps=None if gt_feed is None else [gt_feed[i] for i in idx])
        tab = ev.last_inter.cpu().numpy()
        assert tab.dtype == np.int32 and tab.shape[0] == n and tab.shape[2] == P + 1
        for k, i in enumerate(idx):
            G = len({s["id"] for s in anns[i]["segments_info"]})
            want = ref.inter_table(anns[i], gts[i], preds[i], P)
            assert np.array_equal(tab[k, :G + 2], want), (i, gts[i].shape, G)
            assert not tab[k, G + 2:].any() and int(tab[k].sum()) == gts[i].size
        lo += n
    ev._materialise()
    for i, e in enumerate(ev._predictions):
        want = ev._host_record(ev._annotation(i), gts[i], segs_of(preds[i]), preds[i])
        assert e["pq_record"] == want, (i, e["pq_record"], want)
    got = (ev.evaluate(), ev.table)
    assert got == host_dict(anns, gts, preds)
    return got[0]["panoptic_seg"]


# ------------------------------------------------------------------------------------------------ 1. known answers
def run_one(gt, pred, ann, segs=None):
    ev = PanopticEvaluatorAgnostic(gt_maps={0: gt}, gt_annotations=[ann])
    ev.process_device(["0.jpg"], [0], [out_dev(pred.astype(np.int32), segs)])
    ev._materialise()
    return ev._predictions[0]["pq_record"], ev


def crowd_ann(gt, crowd=()):
    a = gt_from_png(gt, 0, "0.png")
    for s in a["segments_info"]:
        s["iscrowd"] = int(s["id"] in crowd)
    return a


def test_known_answers_through_the_kernel():
    gt = np.zeros((8, 8), np.int64); gt[:4] = 1; gt[4:, :4] = 2
    pr = np.zeros((8, 8), np.int64); pr[:3] = 11; pr[3] = 12; pr[4:, 2:] = 13
    rec, ev = run_one(gt, pr, crowd_ann(gt))
    assert rec == (1, 1, 1, [0.75], 0)                  # P3 against B: IoU exactly 0.5 must NOT match; 16/24 on void: no FP
    tab = ev.last_inter[0].cpu().numpy()
    assert tab[2, 13] == 8 and tab[0, 13] == 16 and tab[1, 11] == 24 and tab[1, 12] == 8
    assert run_one(gt, pr, crowd_ann(gt, crowd=(2,)))[0] == (1, 1, 0, [0.75], 0)
    g2 = np.zeros((8, 8), np.int64); g2[:4] = 5; g2[4:, :4] = 9
    assert run_one(g2, np.where(g2 == 5, 1, np.where(g2 == 9, 2, 0)), crowd_ann(g2))[0] == (2, 0, 0, [1.0, 1.0], 0)


# ------------------------------------------------------------------------------------------------ 2. tables, counts, dicts
@pytest.mark.parametrize("size", SIZES)
def test_one_image_per_call(size):
    h, w = size
    anns, gts, preds = [], [], []
    for k, (G, big) in enumerate((G, big) for G in GT_COUNTS for big in (True, False)):
        gt, ann, pred = make_case(h, w, G, big, "blocky" if k % 2 else "random", seed=100 * h + w + k)
        anns.append(ann); gts.append(gt); preds.append(pred)
    check_batch(anns, gts, preds, call_sizes=[1] * len(anns))


@pytest.mark.parametrize("style", ["blocky", "random"])
@pytest.mark.parametrize("big", [True, False])
def test_mixed_size_batch_in_one_call(style, big):
    spec = [((1, 1), 0), ((7, 13), 2), ((300, 257), 37), ((33, 70), G_MAX), ((16, 16), 1)]
    cases = [make_case(h, w, G, big, style, seed=7 + i) for i, ((h, w), G) in enumerate(spec)]
    res = check_batch([c[1] for c in cases], [c[0] for c in cases], [c[2] for c in cases])
    assert res["num_predictions"] == 5
    if style == "blocky":
        assert res["PQ"] > 0                                 # matches exist: the IoU sum is exercised
    spec = [((1, 257), 1), ((255, 1), 37), ((300, 257), G_MAX), ((33, 70), 2), ((7, 13), 0)]
    cases = [make_case(h, w, G, big, style, seed=70 + i) for i, ((h, w), G) in enumerate(spec)]
    check_batch([c[1] for c in cases], [c[0] for c in cases], [c[2] for c in cases])


@pytest.mark.parametrize("G", [37, G_MAX])
def test_prediction_ids_up_to_256(G):
    cases = [make_case(h, w, G, True, st, seed=900 + i, P=256) for i, (h, w, st) in enumerate([(33, 70, "random"), (300, 257, "blocky")])]
    for c in cases:
        c[2][0, 0] = 256
    check_batch([c[1] for c in cases], [c[0] for c in cases], [c[2] for c in cases], P=256)


@pytest.mark.parametrize("G", [1, G_MAX])                    # table in LDS / in global memory
def test_single_pair_counter(G):
    gt = np.full((512, 512), 5, np.int64)
    ann = {"image_id": 0, "segments_info": [{"id": 5 + 3 * k, "category_id": 1, "iscrowd": 0} for k in range(G)]}
    rec, ev = run_one(gt, np.ones((512, 512), np.int32), ann)
    tab = ev.last_inter[0].cpu().numpy()
    assert tab[1, 1] == 262144 and int(tab.sum()) == 262144
    assert rec == (1, 0, G - 1, [1.0], 0)


def test_special_cases():
    rng = np.random.RandomState(5)
    blocks = np.kron(rng.randint(1, 6, (4, 5)), np.ones((9, 8), np.int64))                 # 36 x 40, ids 1..5
    pred = np.roll(blocks, 1, axis=1).astype(np.int32)
    anns, gts, preds = [], [], []
    # all-void ground truth (declared segments without a pixel: false negatives), all-void prediction
    anns.append({"image_id": 0, "segments_info": [{"id": 3, "category_id": 1}, {"id": 900000, "category_id": 1, "iscrowd": 1}]})
    gts.append(np.zeros_like(blocks)); preds.append(pred)
    anns.append(gt_from_png(blocks * 1000, 0, "0.png")); gts.append(blocks * 1000); preds.append(np.zeros_like(pred))
    # ground-truth ids painted but not declared (ids 4000 / 5000 dropped from the annotation); a declared segment with no pixel
    a = gt_from_png(blocks * 1000, 0, "0.png")
    a["segments_info"] = [s for s in a["segments_info"] if s["id"] < 4000] + [{"id": 777, "category_id": 1, "iscrowd": 0, "area": 50}]
    anns.append(a); gts.append(blocks * 1000); preds.append(pred)
    # annotation areas that differ from the painted counts (larger: the IoUs drop, some below 0.5) and absent areas
    a = gt_from_png(blocks * 1000, 0, "0.png")
    for k, s in enumerate(a["segments_info"]):
        if k % 3 == 0:
            del s["area"]
        elif k % 3 == 1:
            s["area"] = s["area"] * 2 + 3
    anns.append(a); gts.append(blocks * 1000); preds.append(pred)
    check_batch(anns, gts, preds)
    # two crowd segments: A (id 10, upper half) comes first in the annotation, B (id 5, lower half) last.  Prediction 1 lies
    # mostly on B and is forgiven, prediction 2 lies mostly on A and is a false positive (only the LAST crowd counts).
    gt = np.zeros((8, 8), np.int64); gt[:4] = 10; gt[4:] = 5
    pr = np.zeros((8, 8), np.int32); pr[3:, :4] = 1; pr[:5, 4:] = 2
    ann = {"image_id": 0, "segments_info": [{"id": 10, "category_id": 1, "iscrowd": 1}, {"id": 5, "category_id": 1, "iscrowd": 1}]}
    rec, _ = run_one(gt, pr, ann)
    assert rec == (0, 1, 0, [], 0)
    check_batch([ann], [gt], [pr])
    ann["segments_info"].reverse()                                                         # now A is the last crowd
    assert run_one(gt, pr, ann)[0] == (0, 1, 0, [], 0)
    check_batch([ann], [gt], [pr])
    # an area that contradicts the map (a quarter of the painted count: two predictions match one segment) is reported
    gt = np.full((8, 8), 9, np.int64)
    pr = np.ones((8, 8), np.int32); pr[:, 4:] = 2
    rec, ev = run_one(gt, pr, {"image_id": 0, "segments_info": [{"id": 9, "category_id": 1, "area": 16}]})
    assert rec[4] == 8
    with pytest.raises(ValueError):
        ev.evaluate()


# ------------------------------------------------------------------------------------------------ 3. ground truth formats
def test_rgb_ground_truth_equals_id_ground_truth():
    spec = [((7, 13), 2), ((300, 257), 37), ((33, 70), G_MAX)]
    cases = [make_case(h, w, G, True, "blocky", seed=40 + i) for i, ((h, w), G) in enumerate(spec)]
    anns, gts, preds = [c[1] for c in cases], [c[0] for c in cases], [c[2] for c in cases]
    feeds = {"rgb on the device": [torch.from_numpy(id2rgb(g)).to(DEV) for g in gts],
             "rgb on the host": [id2rgb(g) for g in gts],
             "int32 ids on the device": [torch.from_numpy(g.astype(np.int32)).to(DEV) for g in gts],
             "int64 ids on the host": [torch.from_numpy(g) for g in gts],
             "mixed": [id2rgb(gts[0]), torch.from_numpy(gts[1]).to(DEV), gts[2]]}
    got = {name: check_batch(anns, gts, preds, gt_feed=f) for name, f in feeds.items()}
    assert all(v == got["rgb on the device"] for v in got.values())


def test_packed_form_equals_list_form():
    cases = [make_case(h, w, 12, False, "blocky", seed=60 + i, undeclared=False) for i, (h, w) in enumerate([(33, 70), (50, 37)])]
    anns = [dict(c[1], image_id=i) for i, c in enumerate(cases)]
    gts, preds = [c[0] for c in cases], [c[2] for c in cases]
    keep = torch.zeros(2, 128, dtype=torch.uint8)
    for i, p in enumerate(preds):
        keep[i, [s["id"] - 1 for s in segs_of(p)]] = 1
    sizes = np.asarray([p.shape for p in preds], dtype=np.int32)
    packed = {"pan": torch.cat([torch.from_numpy(p).reshape(-1) for p in preds]).to(DEV), "offsets": np.asarray([0, preds[0].size]),
              "sizes": sizes, "keep": keep.to(DEV)}
    ev = PanopticEvaluatorAgnostic(gt_maps=dict(enumerate(gts)), gt_annotations=anns)
    ev.process_device(["0.jpg", "1.jpg"], [0, 1], packed)
    assert (ev.evaluate(), ev.table) == host_dict(anns, gts, preds)


# ------------------------------------------------------------------------------------------------ 4. flags and the host route
def test_flags_and_host_route():
    gt, ann, pred = make_case(33, 70, 5, False, "blocky", seed=3)
    painted = sorted(set(np.unique(pred).tolist()) - {0})
    ev = PanopticEvaluatorAgnostic(gt_maps={0: gt}, gt_annotations=[ann])
    ev.process_device(["0.jpg"], [0], [out_dev(pred, [s for s in segs_of(pred) if s["id"] != painted[0]])])
    with pytest.raises(KeyError, match="painted but not in segments_info"):
        ev.evaluate()
    ev.reset()
    missing = next(i for i in range(1, 129) if i not in painted)
    ev.process_device(["0.jpg"], [0], [out_dev(pred, segs_of(pred, extra=(missing,)))])
    with pytest.raises(KeyError, match="not painted"):
        ev.evaluate()
    # more than G_MAX declared segments, a declared id 0, an id of 2^24: the host rule for that image alone, same results
    big = make_case(33, 70, G_MAX, True, "blocky", seed=4)
    big[1]["segments_info"].append({"id": 12345678, "category_id": 1, "iscrowd": 0})
    zero = make_case(7, 13, 3, False, "blocky", seed=5)
    zero[1]["segments_info"].append({"id": 0, "category_id": 1, "iscrowd": 0})
    wide = make_case(16, 16, 3, False, "blocky", seed=6)
    wide[1]["segments_info"].append({"id": 1 << 24, "category_id": 1, "iscrowd": 0})
    plain = make_case(33, 70, 7, False, "blocky", seed=8)
    cases = [big, plain, zero, wide]
    anns = [dict(c[1], image_id=i) for i, c in enumerate(cases)]
    gts, preds = [c[0] for c in cases], [c[2] for c in cases]
    ev = PanopticEvaluatorAgnostic(gt_maps=dict(enumerate(gts)), gt_annotations=anns)
    ev.process_device([f"{i}.jpg" for i in range(4)], list(range(4)), [out_dev(p) for p in preds])
    assert ev.last_inter.shape[0] == 1                                  # only the plain image went to the device
    assert [e["pq_record"] is not None for e in ev._predictions] == [True, False, True, True]
    assert (ev.evaluate(), ev.table) == host_dict(anns, gts, preds)


# ------------------------------------------------------------------------------------------------ 5. end to end
LOW_TH = 0.018


def test_trainer_ae_compute_pq_on_device(vae_sd):
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.trainers import TrainerAE
    S = 64
    sizes = [(50, 37), (64, 64), (64, 64), (33, 70)]
    ids = semseg_ref.block_targets(4, S, S, 12, seed=5) + 1
    bits = semseg_ref.encode_bits(ids)
    masks = torch.ones(4, S, S, dtype=torch.bool)
    tr = TrainerAE(GeneralVAESeg(vae_sd, device=DEV, compute_dtype="fp32"), num_classes=128, ignore_label=3, mask_th=LOW_TH,
                   count_th=8, overlap_th=0.006)
    own = tr.predict_panoptic(bits[:2].to(DEV), sizes[:2], masks[:2].to(DEV), True)
    g = np.random.RandomState(3)
    gts, anns = {}, []
    for i, hw in enumerate(sizes):
        if i == 0:
            gt = own[0]["panoptic_seg"][0].cpu().numpy().astype(np.int64) * 1000            # its own prediction: true positives exist
        else:
            gt = np.kron(g.randint(0, 4, (4, 4)), np.ones((hw[0] // 4 + 1, hw[1] // 4 + 1), np.int64))[:hw[0], :hw[1]] * 300
        gts[f"img{i}"] = gt
        anns.append(gt_from_png(gt, f"img{i}", f"img{i}.png"))
    loader = [{"image_semseg": bits[a:b], "mask": masks[a:b],
               "meta": [{"image_file": f"/data/img{i}.png", "image_id": f"img{i}", "im_size": sizes[i]} for i in range(a, b)]}
              for a, b in ((0, 2), (2, 4))]
    res = {}
    for on_device in (False, True):
        ev = PanopticEvaluatorAgnostic(gt_maps=gts, gt_annotations=anns, on_device=on_device)
        res[on_device] = (tr.compute_pq(loader, ev, threshold_output=True), ev.table)
        assert (ev.last_inter is not None) == on_device
    assert res[True] == res[False]
    r = res[True][0]["panoptic_seg"]
    assert r["num_predictions"] == 4 and r["PQ"] > 0 and r["RQ"] < 100
    # ground truth handed over by the batch itself, as RGB bytes on the device
    for b in loader:
        b["panoptic_gt"] = [torch.from_numpy(id2rgb(gts[m["image_id"]])).to(DEV) for m in b["meta"]]
    ev = PanopticEvaluatorAgnostic(gt_maps=gts, gt_annotations=anns, on_device=True)
    assert (tr.compute_pq(loader, ev, threshold_output=True), ev.table) == res[False]


def test_trainer_diffusion_compute_pq_on_device(unet_sd, vae_sd, sched_kw):
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet, GeneralVAESeg, GeneralVAEImage
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    from test_compute_pq_gpu import smooth_image
    S, L, STEPS = 64, 8, 2
    post = dict(mask_th=0.01, count_th=8, overlap_th=0.002, ignore_label=3)
    isd = weights.generate(weights.vae_image_schema(), seed=11, norm_keys=weights.VAE_IMAGE_NORM_KEYS)
    tr = TrainerDiffusion(GeneralVAESeg(vae_sd, scaling_factor=0.2, device=DEV, compute_dtype="fp32"),
                          UNet(unet_sd, in_channels=12, device=DEV, compute_dtype="fp32"), DDIMNoiseScheduler(**sched_kw),
                          vae_image=GeneralVAEImage(isd, scaling_factor=0.18215, device=DEV, compute_dtype="fp32"), latent_size=L)
    sizes = [(50, 37), (64, 64), (40, 60)]
    imgs = torch.stack([smooth_image(S, S, 20 + i) for i in range(3)])
    masks = torch.ones(3, S, S, dtype=torch.bool)
    own = tr.predict_panoptic(imgs[:2].to(DEV), sizes[:2], masks[:2].to(DEV), STEPS, seed=42, threshold_output=True, **post)
    g = np.random.RandomState(3)
    gts, anns = {}, []
    for i, hw in enumerate(sizes):
        if i == 0:
            gt = own[0]["panoptic_seg"][0].cpu().numpy().astype(np.int64) * 1000
        else:
            gt = np.kron(g.randint(0, 4, (4, 4)), np.ones((hw[0] // 4 + 1, hw[1] // 4 + 1), np.int64))[:hw[0], :hw[1]] * 300
        gts[f"img{i}"] = gt
        anns.append(gt_from_png(gt, f"img{i}", f"img{i}.png"))

    def loader():
        for a, b in ((0, 2), (2, 3)):
            yield {"image": imgs[a:b], "mask": masks[a:b],
                   "meta": [{"image_file": f"/data/img{i}.jpg", "image_id": f"img{i}", "im_size": sizes[i]} for i in range(a, b)]}
    res = {}
    for on_device in (False, True):
        ev = PanopticEvaluatorAgnostic(gt_maps=gts, gt_annotations=anns, on_device=on_device)
        res[on_device] = (tr.compute_pq(loader(), ev, num_inference_steps=STEPS, seed=42, threshold_output=True, **post), ev.table)
    assert res[True] == res[False]
    r = res[True][0]["panoptic_seg"]
    assert r["num_predictions"] == 3 and r["PQ"] > 0


def test_real_coco_pairs(golden):
    g = golden("real_coco.npz")
    gts = [g[f"resized_ids_{k}"].astype(np.int64) for k in range(2)]
    preds = [np.roll(x, (5, 9), axis=(0, 1)).astype(np.int32) for x in gts]
    anns = [gt_from_png(x, k, f"{k}.png") for k, x in enumerate(gts)]
    res = check_batch(anns, gts, preds)
    assert 0 < res["RQ"] < 100 and res["num_predictions"] == 2          # matched and unmatched segments both occur


def test_main_ae_eval_device_pq_prints_the_same_table(tmp_path):
    from PIL import Image
    gt_dir = tmp_path / "pan"
    gt_dir.mkdir()
    rs = np.random.RandomState(11)
    for i, (h, w) in enumerate([(60, 80), (72, 50), (64, 64)]):
        gt = np.kron(rs.randint(0, 5, (4, 4)), np.ones((h // 4 + 1, w // 4 + 1), np.int64))[:h, :w] * 700
        Image.fromarray(id2rgb(gt)).save(gt_dir / f"{i:03d}.png")
    argv = [sys.executable, os.path.join(ROOT, "tools", "main_ae_eval.py"), "--panoptic", str(gt_dir), "--size", "64", "--batch", "2",
            "--dtype", "bf16", "--count-th", "8", "--mask-th", str(LOW_TH), "--overlap-th", "0.005", "--threshold-output"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "latent-diffusion-segmentation_amd")]))
    procs = [subprocess.Popen(argv + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for extra in ([], ["--device-pq"])]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    assert re.search(r"^PQ (\S+) SQ (\S+) RQ (\S+) num_predictions 3$", outs[0][0], re.M), outs[0][0]
    assert "|  All   |" in outs[0][0] and outs[0][0] == outs[1][0]

"""Stage-1 (seg-VAE reconstruction) evaluation on the MI355X: the meter kernel, the fused mIoU tail (postproc.hip
semseg_scan_kernel) on given maps and behind the decoder, `TrainerAE.compute_miou` / `compute_pq` and the entry
tools/main_ae_eval.py - against the brute-force meter rule, `F.interpolate(align_corners=True)`, the product's own unfused
path and the oracle chain (oracle.vae encode -> mode -> decode) with the restatements of tests/semseg_ref.py."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semseg_ref as ref
from conftest import ROOT
from oracle import vae as o_vae

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC = 128
# random weights give flat class distributions (max softmax probability 0.013 .. 0.11 over 128 classes): a threshold inside
# that range, so that both sides of it occur
LOW_TH = 0.018


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def vaes(vae_sd):
    from ldmseg_amd.models import GeneralVAESeg
    made = {}

    def get(cd):
        if cd not in made:
            made[cd] = GeneralVAESeg(vae_sd, device=DEV, compute_dtype=cd)
        return made[cd]
    return get


def id_maps(B, S, seed, num_labels=12, boxes=None):
    """Coarse block id maps [B,S,S] with labels in [1, num_labels] and a band (or everything outside `boxes`) of 0 = ignore."""
    ids = ref.block_targets(B, S, S, num_labels, seed=seed) + 1
    if boxes is None:
        ids[:, :S // 8] = 0
    else:
        for i, (y0, x0, ch, cw) in enumerate(boxes):
            m = torch.zeros(S, S, dtype=torch.bool)
            m[y0:y0 + ch, x0:x0 + cw] = True
            ids[i][~m] = 0
    return ids


# ------------------------------------------------------------------------------------------------ 1. the meter kernel
@pytest.mark.parametrize("K,ignore_index", [(128, 0), (5, 255)])
@pytest.mark.parametrize("shape", [(1,), (255,), (256,), (257,), (3, 37, 50)])
def test_meter_kernel_against_brute_force(shape, K, ignore_index):
    from ldmseg_amd import _lib
    g = np.random.RandomState(int(np.prod(shape)) + K)
    lo, hi = (0, K) if K == 128 else (-2, K + 4)                   # K = 5: labels outside [0, K), negative ones included
    gt = g.randint(lo, hi, shape)
    gt[g.rand(*shape) < 0.2] = ignore_index
    pred = np.where(g.rand(*shape) < 0.5, gt, g.randint(lo, hi, shape))
    pred[g.rand(*shape) < 0.1] = ignore_index
    want = ref.meter_counts(pred, gt, K, ignore_index)
    dp, dg = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    counts = torch.zeros(3, K, dtype=torch.int64, device=DEV)
    n = int(np.prod(shape))
    assert _lib.lib().ldmseg_semseg_meter_update(P(dp), P(dg), n, K, ignore_index, P(counts), _lib.stream_ptr(DEV)) == 0
    assert np.array_equal(counts.cpu().numpy(), want)
    # a second call accumulates; nothing is reset
    pred2 = np.where(g.rand(*shape) < 0.5, gt, g.randint(lo, hi, shape))
    dp2 = torch.from_numpy(pred2).to(DEV)
    assert _lib.lib().ldmseg_semseg_meter_update(P(dp2), P(dg), n, K, ignore_index, P(counts), _lib.stream_ptr(DEV)) == 0
    assert np.array_equal(counts.cpu().numpy(), want + ref.meter_counts(pred2, gt, K, ignore_index))


def test_meter_class_through_the_kernel():
    from ldmseg_amd.evaluations import SemsegMeter
    g = np.random.RandomState(9)
    gt, pred = g.randint(0, 7, (2, 19, 23)), g.randint(0, 7, (2, 19, 23))
    m = SemsegMeter(6, [str(i) for i in range(7)], has_bg=True, ignore_index=255)      # 7 classes
    m.update(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    m.update(torch.from_numpy(pred[:1]).to(DEV), torch.from_numpy(gt[:1]).to(DEV))
    want = ref.meter_counts(pred, gt, 7, 255) + ref.meter_counts(pred[:1], gt[:1], 7, 255)
    got = m.return_score(verbose=False, suppress_prints=True)
    assert np.array_equal(np.stack([m.tp, m.fp, m.fn]), want)
    assert got["jaccards_all_categs"] == ref.meter_scores(want)["jaccards_all_categs"]
    m.reset()
    assert int(m._dev.sum()) == 0 and m.tp.sum() == 0


# ------------------------------------------------------------------------------------------------ 2. the tail on a given map
# ((H4, W4), (out_h, out_w), seed): seeds chosen on the CPU so that the number of near-ties stays within the cap below
TAIL_GEO = [((16, 16), (32, 32), 203), ((24, 24), (48, 48), 215), ((16, 16), (16, 16), 228), ((16, 16), (37, 50), 230),
            ((8, 8), (1, 5), 200), ((16, 16), (9, 9), 200)]


def run_tail(x4, dt, out, mask_th, ignore_label, targets, ignore_index, K, want_preds=True, want_volume=True, counts=None):
    from ldmseg_amd import _lib
    B, Cn, H4, W4 = x4.shape
    oh, ow = out
    dx = x4.to(DEV)
    preds = torch.full((B, oh, ow), -7, dtype=torch.int64, device=DEV) if want_preds else None
    vol = torch.empty(B, Cn, oh, ow, dtype=torch.float32, device=DEV) if want_volume else None
    if counts is None and targets is not None:
        counts = torch.zeros(3, K, dtype=torch.int64, device=DEV)
    dtg = targets.to(DEV) if targets is not None else None
    r = _lib.lib().ldmseg_op_semseg_from_decoder(P(dx), B, Cn, H4, W4, dt, oh, ow, mask_th, ignore_label, P(dtg), ignore_index, K,
                                                P(preds), P(counts), P(vol), None)
    assert r == 0
    torch.cuda.synchronize()
    return (preds.cpu() if want_preds else None), (vol.cpu() if want_volume else None), (counts.cpu().numpy() if counts is not None else None)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("geo", TAIL_GEO)
def test_semseg_tail_on_a_given_map(geo, dt):
    (H4, W4), (oh, ow), seed = geo
    B, mask_th, ignore_label = 2, 0.3, 0
    x4 = ref.segment_like_logits(B, NC, H4, W4, seed=seed, sharp=5.0)
    if dt == 1:
        x4 = x4.bfloat16().float()
    want_vol = ref.resize_align_corners(x4, (oh, ow))
    # targets: the reference prediction on half of the map (true positives), random labels elsewhere, a band of ignore
    tg = ref.semseg_labels(want_vol, -1.0, ignore_label)[0]
    rnd = torch.from_numpy(np.random.RandomState(seed).randint(0, NC, (B, oh, ow)))
    tg[:, :, : ow // 2] = rnd[:, :, : ow // 2]
    if oh > 1:
        tg[:, : max(1, oh // 6)] = ignore_label
    else:
        tg[:, :, -1] = ignore_label
    tiny = oh * ow <= 5                    # (the degenerate map has too few pixels for every branch to occur)
    preds, vol, counts = run_tail(x4, dt, (oh, ow), mask_th, ignore_label, tg, ignore_label, NC)
    # the resampling itself
    err, scale = float((vol - want_vol).abs().max()), float(want_vol.abs().max())
    print(f"volume max err {err:.3e}, bound {2e-5 * scale:.3e}")
    assert err < 2e-5 * scale
    # labels: exact against argmax / threshold on the kernel's own volume wherever the decision is not within rounding of a tie
    lab, prob, gap = ref.semseg_labels(vol, mask_th, ignore_label)
    clear = (gap > 1e-5) & ((prob - mask_th).abs() > 1e-5)
    for b in range(B):
        nfuzzy = int((~clear[b]).sum())
        print(f"image {b}: {nfuzzy} non-clear pixels, cap {max(3, (oh * ow) // 200)}")
        assert nfuzzy <= max(3, (oh * ow) // 200)
    assert torch.equal(preds[clear], lab[clear])
    assert tiny or (int((preds == ignore_label).sum()) > 0 and len(preds.unique()) > 2)
    # counters: the brute-force rule on the kernel's own predictions, integer-exact
    want_counts = ref.meter_counts(preds.numpy(), tg.numpy(), NC, ignore_label)
    assert np.array_equal(counts, want_counts)
    assert tiny or (want_counts[0].sum() > 0 and want_counts[1].sum() > 0 and want_counts[2].sum() > 0)
    # preds = NULL and targets = NULL each work alone, and accumulate into / leave alone the caller's counters
    _, _, c2 = run_tail(x4, dt, (oh, ow), mask_th, ignore_label, tg, ignore_label, NC, want_preds=False, want_volume=False,
                        counts=torch.from_numpy(counts).to(DEV))
    assert np.array_equal(c2, 2 * want_counts)
    sentinel = torch.full((3, NC), 5, dtype=torch.int64, device=DEV)
    p3, _, c3 = run_tail(x4, dt, (oh, ow), mask_th, ignore_label, None, ignore_label, NC, want_volume=False, counts=sentinel)
    assert torch.equal(p3, preds) and (c3 == 5).all()
    # mask_th < 0 disables the threshold
    p4, _, _ = run_tail(x4, dt, (oh, ow), -1.0, ignore_label, None, ignore_label, 0, want_volume=False)
    arg = vol.argmax(dim=1)
    assert torch.equal(p4[gap > 1e-5], arg[gap > 1e-5])
    assert tiny or int(((p4 != preds) & (prob < mask_th - 1e-5)).sum()) > 0       # the threshold did change pixels above


# ------------------------------------------------------------------------------------------------ 3. fused against unfused
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("L", [6, 16])
def test_reconstruct_semseg_against_the_unfused_path(vaes, L, cd):
    from ldmseg_amd.evaluations import SemsegMeter
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    vae = vaes(cd)
    B, S = 3, 8 * L
    margin = 1e-3 if cd == "fp32" else 1e-2
    ids = id_maps(B, S, seed=L)
    x = ref.encode_bits(ids).to(DEV)
    names = [str(i) for i in range(NC)]
    for mask_th in (None, LOW_TH):
        # the unfused product path
        mom = vae.encode_moments(x, 2.0, -1.0)
        z = DiagonalGaussianDistribution(mom).mode()
        logits = vae.decode(z, interpolate=False)
        up = F.interpolate(logits, size=(S, S), mode="bilinear", align_corners=True)
        lab, prob, gap = ref.semseg_labels(up, mask_th, 0)
        # targets: the encoded maps; for image 0 the unfused prediction itself below the ignore band (true positives)
        tg = ids.to(DEV)
        tg[0, S // 8:] = lab[0, S // 8:]
        fused = SemsegMeter(NC, names, has_bg=False, ignore_index=0)
        preds = vae.reconstruct_semseg(x, (S, S), tg, fused.device_counts(DEV), in_mul=2.0, in_add=-1.0, mask_th=mask_th,
                                       ignore_label=0, ignore_index=0)
        unfused = SemsegMeter(NC, names, has_bg=False, ignore_index=0)
        unfused.update(lab, tg)
        clear = gap > margin
        if mask_th is not None:
            # a logit perturbation d moves the max softmax probability p by at most 2 d p: the logit margin as a relative one
            clear &= (prob - mask_th).abs() > 2 * margin * prob
        share = float(clear.float().mean())
        nonclear = int((~clear).sum())
        mism = int((preds != lab)[clear].sum())
        print(f"{cd} L={L} mask_th={mask_th}: clear share {share:.4f}, mismatches on clear pixels {mism}, "
              f"in all {int((preds != lab).sum())}")
        assert share > 0.9
        assert mism == 0
        fused.return_score(verbose=False, suppress_prints=True)
        unfused.return_score(verbose=False, suppress_prints=True)
        dc = sum(int(np.abs(a - b).sum()) for a, b in ((fused.tp, unfused.tp), (fused.fp, unfused.fp), (fused.fn, unfused.fn)))
        print(f"   summed |dcounts| {dc}, bound {2 * nonclear}")
        assert dc <= 2 * nonclear
        assert fused.tp.sum() > 0 and fused.fp.sum() > 0 and fused.fn.sum() > 0
        # bitwise: the one-call chain against decode_semseg on mode() of encode_moments, same handle
        c2 = torch.zeros(3, NC, dtype=torch.int64, device=DEV)
        p2 = vae.decode_semseg(z, (S, S), tg, c2, mask_th=mask_th, ignore_label=0, ignore_index=0)
        assert torch.equal(p2, preds)
        assert np.array_equal(c2.cpu().numpy(), np.stack([fused.tp, fused.fp, fused.fn]))


# ------------------------------------------------------------------------------------------------ 4. against the oracle chain
def oracle_logits(vae_sd, x):
    with torch.no_grad():
        z = o_vae.encode_mode(vae_sd, 2.0 * x - 1.0)
        return o_vae.decode(vae_sd, z, interpolate=False)


def check_against_oracle_labels(lib_preds, lib_counts, ora_lab, clear, tg, ignore_label):
    """Labels equal where clear; per class the library's and the oracle's counters differ by at most the non-clear pixels that
    involve the class; the Jaccard bound that follows from the counts."""
    assert torch.equal(lib_preds[clear], ora_lab[clear])
    ora_counts = ref.meter_counts(ora_lab.numpy(), tg.numpy(), NC, ignore_label)
    fuzzy = ~clear
    jl, jo = ref.meter_scores(lib_counts)["jaccards_all_categs"], ref.meter_scores(ora_counts)["jaccards_all_categs"]
    bounds = []
    for c in range(NC):
        # a non-clear pixel moves a counter of class c only if c is its target or one of the two predictions, and then by one
        n_c = int((fuzzy & ((tg == c) | (lib_preds == c) | (ora_lab == c))).sum())
        assert np.abs(lib_counts[:, c] - ora_counts[:, c]).max() <= n_c, c
        # J = tp / U with U = tp + fp + fn: every pixel is in at most one of the three, so |dtp| <= n_c and |dU| <= n_c, and
        # |tp'/U' - tp/U| <= |dtp| / U' + (tp / U) |dU| / U' <= 2 n_c / U'
        u = max(int(lib_counts[:, c].sum()), int(ora_counts[:, c].sum()))
        bound = min(1.0, 2.0 * n_c / max(u, 1))
        assert abs(jl[c] - jo[c]) <= bound + 1e-12, (c, jl[c], jo[c], n_c, u)
        bounds.append(bound)
    miou_l, miou_o = float(np.mean(jl)), float(np.mean(jo))
    print(f"mIoU library {miou_l:.6f} oracle {miou_o:.6f} bound {float(np.mean(bounds)):.6f}")
    assert abs(miou_l - miou_o) <= float(np.mean(bounds)) + 1e-12
    return ora_counts


@pytest.mark.parametrize("L", [8, 16])
def test_reconstruct_semseg_against_the_oracle_chain(vaes, vae_sd, L):
    vae = vaes("fp32")
    B, S = 3, 8 * L
    ids = id_maps(B, S, seed=40 + L, num_labels=100)
    x = ref.encode_bits(ids)
    up = ref.resize_align_corners(oracle_logits(vae_sd, x), (S, S))
    for mask_th in (None, LOW_TH):
        lab, prob, gap = ref.semseg_labels(up, mask_th, 0)
        clear = gap > 1e-3
        if mask_th is not None:
            clear &= (prob - mask_th).abs() > 2e-3 * prob          # (the relative form of the logit margin, as in test 3)
        print(f"L={L} mask_th={mask_th}: clear share {float(clear.float().mean()):.4f}")
        assert float(clear.float().mean()) > 0.9
        # targets: the oracle's own prediction for image 0, coarse random blocks with a band of ignore_label for the others
        tg = ref.block_targets(B, S, S, NC, seed=L, ignore_label=0, band=(S // 3, S // 3 + S // 8))
        tg[0] = ref.semseg_labels(up[:1], None, 0)[0][0]
        tg[1, : S // 2] = lab[1, : S // 2]
        counts = torch.zeros(3, NC, dtype=torch.int64, device=DEV)
        preds = vae.reconstruct_semseg(x.to(DEV), (S, S), tg.to(DEV), counts, in_mul=2.0, in_add=-1.0, mask_th=mask_th,
                                       ignore_label=0, ignore_index=0).cpu()
        lib_counts = counts.cpu().numpy()
        assert np.array_equal(lib_counts, ref.meter_counts(preds.numpy(), tg.numpy(), NC, 0))
        check_against_oracle_labels(preds, lib_counts, lab, clear, tg, 0)
        assert int((lib_counts[0] > 0).sum()) >= 2 and lib_counts[1].sum() > 0 and lib_counts[2].sum() > 0


# ------------------------------------------------------------------------------------------------ 5. compute_miou
def test_compute_miou_over_three_batches(vaes, monkeypatch):
    from ldmseg_amd.evaluations import SemsegMeter
    from ldmseg_amd.trainers import TrainerAE
    vae = vaes("fp32")
    S = 64
    ids = id_maps(5, S, seed=77)
    bits = ref.encode_bits(ids)
    parts = [(0, 2), (2, 4), (4, 5)]
    loader = [{"image_semseg": bits[a:b], "semseg": ids[a:b]} for a, b in parts]
    tr = TrainerAE(vae, num_classes=NC, ignore_label=0, mask_th=LOW_TH)
    folds = []
    orig = SemsegMeter.fold_device_counts
    monkeypatch.setattr(SemsegMeter, "fold_device_counts", lambda self: (folds.append(1), orig(self))[1])
    for th_out in (False, True):
        folds.clear()
        res = tr.compute_miou(loader, threshold_output=th_out)
        assert len(folds) == 1                      # one device-to-host copy for the whole loop
        want = np.zeros((3, NC), np.int64)
        for a, b in parts:
            p = vae.reconstruct_semseg(bits[a:b].to(DEV), (S, S), in_mul=2.0, in_add=-1.0, mask_th=LOW_TH if th_out else None,
                                       ignore_label=0)
            want += ref.meter_counts(p.cpu().numpy(), ids[a:b].numpy(), NC, 0)
        sc = ref.meter_scores(want)
        assert res["jaccards_all_categs"] == sc["jaccards_all_categs"]
        assert abs(res["mIoU"] - sc["mIoU"]) <= NC * 2.0 ** -52
        assert want[0].sum() + want[2].sum() == int((ids != 0).sum())        # every non-ignored pixel of a class < K is tp or fn
    out = tr.compute_metrics("miou", loader)
    assert set(out) == {"miou"} and out["miou"]["mIoU"] > 0


# ------------------------------------------------------------------------------------------------ 6. compute_pq
PQ_S = 128
# padding boxes (y0, x0, height, width) in the network grid and original sizes: the geometry of tests/test_compute_pq_gpu.py
PQ_SPECS = [((0, 0, PQ_S, PQ_S), (96, 128)), ((0, 0, 100, PQ_S), (75, 96)), ((9, 4, 111, 86), (150, 117)),
            ((0, 0, PQ_S, 90), (128, 90)), ((0, 0, PQ_S, PQ_S), (64, 64))]
# found on the CPU: with overlap_th 0.006 many segments sit between the two rules' ratios (count / #(logit >= th) is about
# twice count / #(sigmoid(logit) >= th), since the second mask is nearly the whole image)
PQ_POST = dict(mask_th=LOW_TH, count_th=24, overlap_th=0.006, ignore_label=3)


def test_compute_pq_against_oracle_and_brute_force(vaes, vae_sd, tmp_path):
    from PIL import Image
    from ldmseg_amd.evaluations import PanopticEvaluatorAgnostic, id2rgb, rgb2id
    from ldmseg_amd.evaluations.panoptic_evaluation_agnostic import gt_from_png
    from ldmseg_amd.trainers import TrainerAE
    from test_compute_pq_gpu import brute_force_pq
    torch.set_num_threads(16)
    vae = vaes("fp32")
    S, n = PQ_S, len(PQ_SPECS)
    boxes = [sp[0] for sp in PQ_SPECS]
    ids = id_maps(n, S, seed=5, boxes=boxes)
    bits = ref.encode_bits(ids)
    masks = ids != 0
    for i, (y0, x0, ch, cw) in enumerate(boxes):           # (the block maps hold no 0 inside the box: mask = box)
        assert int(masks[i].sum()) == ch * cw
    # the oracle chain and the restatement of trainers_ae.py:613-668, with both overlap rules
    lg = F.interpolate(oracle_logits(vae_sd, bits), size=(S, S), mode="bilinear", align_corners=False)        # :614-619
    ora = []
    for i, ((y0, x0, ch, cw), hw) in enumerate(PQ_SPECS):
        final = F.interpolate(lg[i][:, y0:y0 + ch, x0:x0 + cw][None], size=hw, mode="bilinear", align_corners=False)[0]
        ora.append((final, ref.ae_panoptic_postprocess(final, True, **PQ_POST),
                    ref.ae_panoptic_postprocess(final, True, mask_rule="sigmoid", **PQ_POST)))
    gt_dir, out_dir = tmp_path / "panoptic", tmp_path / "pred"
    gt_dir.mkdir()
    g = np.random.RandomState(3)
    gt_maps, gt_anns = {}, []
    for i, (_, hw) in enumerate(PQ_SPECS):
        if i == 0:
            gt = ora[0][1][0].astype(np.int64) * 1000                  # the oracle's own prediction: true positives exist
        else:
            gt = np.kron(g.randint(0, 4, (4, 4)), np.ones((hw[0] // 4 + 1, hw[1] // 4 + 1), np.int64))[:hw[0], :hw[1]] * 300
        Image.fromarray(id2rgb(gt)).save(gt_dir / f"img{i}.png")
        gt_maps[f"img{i}"] = rgb2id(np.asarray(Image.open(gt_dir / f"img{i}.png").convert("RGB")))
        gt_anns.append(gt_from_png(gt_maps[f"img{i}"], f"img{i}", f"img{i}.png"))
    parts = [(0, 2), (2, 4), (4, 5)]
    loader = [{"image_semseg": bits[a:b], "mask": masks[a:b],
               "meta": [{"image_file": f"/data/img{i}.png", "image_id": f"img{i}", "im_size": PQ_SPECS[i][1]} for i in range(a, b)]}
              for a, b in parts]
    tr = TrainerAE(vae, num_classes=NC, ignore_label=PQ_POST["ignore_label"], mask_th=PQ_POST["mask_th"],
                   count_th=PQ_POST["count_th"], overlap_th=PQ_POST["overlap_th"])
    ev = PanopticEvaluatorAgnostic(output_dir=str(out_dir), gt_maps=gt_maps, gt_annotations=gt_anns)
    res = tr.compute_metrics(["pq"], loader, evaluator=ev, threshold_output=True)["pq"]["panoptic_seg"]
    assert res["num_predictions"] == n
    preds = {i: rgb2id(np.asarray(Image.open(out_dir / f"img{i}.png").convert("RGB"))) for i in range(n)}
    # (b) the metric: brute force on the product's own predictions, exact
    pq, sq, rq, tp, fp, fn = brute_force_pq([gt_maps[f"img{i}"] for i in range(n)], [preds[i] for i in range(n)])
    assert tp >= 1
    assert abs(res["PQ"] - pq) < 1e-9 and abs(res["SQ"] - sq) < 1e-9 and abs(res["RQ"] - rq) < 1e-9
    # (a) against the oracle chain.  Labels: equal where clear.  Segment decisions: equal for every label whose decision cannot
    # be moved by the non-clear pixels (count) or by logits within 1e-4 of the mask threshold (mask count).
    rule_matters = 0
    for a, b in parts:
        processed, st = tr.predict_panoptic(bits[a:b].to(DEV), [PQ_SPECS[i][1] for i in range(a, b)], masks[a:b].to(DEV), True,
                                            return_stats=True)
        for j, i in enumerate(range(a, b)):
            final, (pan_ref, info_ref, raw_ref, st_ref), (_, info_sig, _, st_sig) = ora[i]
            pan = processed[j]["panoptic_seg"][0].cpu().numpy()
            assert pan.shape == PQ_SPECS[i][1] and np.array_equal(pan, preds[i])          # compute_pq wrote exactly this map
            kept = {s["id"] - 1 for s in processed[j]["panoptic_seg"][1]}
            lab = st["labels"][j].cpu().numpy()
            top2 = final.topk(2, dim=0)[0]
            prob = torch.softmax(final, 0).max(0)[0]
            clear = (((top2[0] - top2[1]) > 1e-3) & ((prob - LOW_TH).abs() > 2e-3 * prob)).numpy()
            assert clear.mean() > 0.9
            assert np.array_equal(lab[clear], raw_ref[clear])
            kept_ref, kept_sig = {s["id"] - 1 for s in info_ref}, {s["id"] - 1 for s in info_sig}
            stable_px = clear.copy()
            n_stable = 0
            for c in range(NC):
                n_c = int((~clear & ((raw_ref == c) | (lab == c))).sum())
                m_c = int(((final[c] - LOW_TH).abs() < 1e-4).sum())
                cnt, msk = int(st_ref["counts"][c]), int(st_ref["mask_counts"][c])
                lo_c, hi_c = cnt - n_c, cnt + n_c

                def decide(k, m):
                    return k > 0 and k >= PQ_POST["count_th"] and c != PQ_POST["ignore_label"] and (m == 0 or k / m >= PQ_POST["overlap_th"])
                outcomes = {decide(k, m) for k in (lo_c, hi_c) for m in (max(msk - m_c, 0), msk + m_c)}
                if len(outcomes) == 1:
                    n_stable += 1
                    assert (c in kept) == (c in kept_ref), (i, c, cnt, msk)
                    if (c in kept_ref) != (c in kept_sig):
                        rule_matters += 1
                else:
                    stable_px &= raw_ref != c
            print(f"image {i}: clear share {clear.mean():.4f}, {n_stable} of {NC} labels with a stable decision, kept {len(kept)}")
            assert n_stable > NC // 2 and len(kept) >= 1
            assert np.array_equal(pan[stable_px], pan_ref[stable_px])
    # the sigmoid rule of the LDM tail would have decided these segments differently: it cannot pass for the logit rule
    print(f"{rule_matters} stable decisions differ between the logit and the sigmoid rule")
    assert rule_matters >= 5


# ------------------------------------------------------------------------------------------------ 7. real data
def test_real_coco_pairs_through_compute_miou(vaes, vae_sd, golden):
    """The reference's own example pairs: the remapped real panoptic maps (every 4th pixel of the 512 x 512 validation
    resize: 128 x 128), bit-encoded by the product's codec, through `compute_miou` in fp32, against the oracle chain."""
    from ldmseg_amd.data.bitcodec import encode_bitmap
    from ldmseg_amd.trainers import TrainerAE
    g = golden("real_coco.npz")
    ids = torch.stack([torch.from_numpy(g[f"resized_ids_{k}"][::4, ::4].astype(np.int64)) for k in range(2)])
    S = ids.shape[-1]
    assert S == 128 and int(ids.max()) < NC and len(ids.unique()) > 10
    bits, _ = encode_bitmap(ids.to(DEV), n=7, fill_value=0.5, ignore_label=0)
    assert torch.equal(bits.cpu(), ref.encode_bits(ids))
    vae = vaes("fp32")
    tr = TrainerAE(vae, num_classes=NC, ignore_label=0, mask_th=LOW_TH)
    res = tr.compute_miou([{"image_semseg": bits, "semseg": ids}], threshold_output=False)
    up = ref.resize_align_corners(oracle_logits(vae_sd, bits.cpu()), (S, S))
    lab, prob, gap = ref.semseg_labels(up, None, 0)
    clear = gap > 1e-3
    assert float(clear.float().mean()) > 0.9
    preds = vae.reconstruct_semseg(bits, (S, S), in_mul=2.0, in_add=-1.0, ignore_label=0).cpu()
    lib_counts = ref.meter_counts(preds.numpy(), ids.numpy(), NC, 0)
    assert res["jaccards_all_categs"] == ref.meter_scores(lib_counts)["jaccards_all_categs"]
    check_against_oracle_labels(preds, lib_counts, lab, clear, ids, 0)


# ------------------------------------------------------------------------------------------------ 8. the entry script
def test_main_ae_eval_entry_subprocess(tmp_path):
    from PIL import Image
    from ldmseg_amd.evaluations import id2rgb
    gt_dir, out_dir = tmp_path / "pan", tmp_path / "out"
    gt_dir.mkdir()
    rs = np.random.RandomState(11)
    for i, (h, w) in enumerate([(60, 80), (72, 50), (64, 64)]):
        gt = np.kron(rs.randint(0, 5, (4, 4)), np.ones((h // 4 + 1, w // 4 + 1), np.int64))[:h, :w] * 700
        Image.fromarray(id2rgb(gt)).save(gt_dir / f"{i:03d}.png")
    argv = ["--panoptic", str(gt_dir), "--size", "64", "--batch", "2", "--dtype", "bf16", "--count-th", "8", "--mask-th", str(LOW_TH),
            "--overlap-th", "0.005", "--threshold-output"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "latent-diffusion-segmentation_amd")]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "main_ae_eval.py")] + argv + ["--out", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    m1 = re.search(r"^mIoU (\S+)$", r.stdout, re.M)
    m2 = re.search(r"^PQ (\S+) SQ (\S+) RQ (\S+) num_predictions (\d+)$", r.stdout, re.M)
    assert m1 and m2, r.stdout
    assert sorted(os.listdir(out_dir)) == ["000.png", "001.png", "002.png", "predictions.json"]
    assert np.asarray(Image.open(out_dir / "001.png")).shape[:2] == (72, 50)
    # the same numbers in this process
    spec = importlib.util.spec_from_file_location("main_ae_eval", os.path.join(ROOT, "tools", "main_ae_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import argparse
    args = argparse.Namespace(panoptic=str(gt_dir), ae=None, size=64, batch=2, dtype="bf16", mask_th=LOW_TH, count_th=8,
                              overlap_th=0.005, threshold_output=True, out=None)
    files = sorted(str(p) for p in gt_dir.glob("*.png"))
    miou, pq, _ = mod.evaluate(args, torch.device(DEV), files)
    assert float(m1.group(1)) == float(100 * miou["mIoU"])
    assert (float(m2.group(1)), float(m2.group(2)), float(m2.group(3))) == tuple(float(pq["panoptic_seg"][k]) for k in ("PQ", "SQ", "RQ"))
    assert int(m2.group(4)) == 3

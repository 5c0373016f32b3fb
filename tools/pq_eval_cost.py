"""Cost of the class-agnostic PQ bookkeeping per batch: the device route `PanopticEvaluatorAgnostic.process_device` (one
`ldmseg_pq_match` call per batch: contingency table + matching on the GPU, no map copied to the host) against the host route
`process` (copy to the host + PNG encode per image) - and `evaluate()` of both (one read of a few numbers per image against
PNG decode + four `np.unique` sorts per image).

  python tools/pq_eval_cost.py [--B 8] [--h 480] [--w 640] [--segments 20] [--warmup 3] [--iters 30]

Input: one batch of B panoptic maps (prediction ids 1..segments in blocks, on the GPU, as the fused tails leave them) and ground
truth maps of about `segments` segments each (a shifted copy, so that most segments match and some do not).  The ground truth of
the device route is measured both ways: prefetched on the GPU (`gt_maps=` tensors on the device) and uploaded from the host per
batch.  Timing, the same for all paths: host clock around one batch ending in a device synchronise, median of `iters` batches
after `warmup`, with the fastest and slowest batch as the spread; `evaluate()` is timed apart, per image.  Prints one JSON line
per measurement and checks that all routes give the same result dict.  A record, not a gate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"


def make_maps(B, h, w, segments, seed=0):
    """-> (gt id maps [h,w] int64 with ids beyond 16 bits, prediction maps [h,w] int32 with ids 1..n) as numpy arrays."""
    import numpy as np
    rng = np.random.RandomState(seed)
    gts, preds = [], []
    ny = max(1, int(round(segments ** 0.5)))
    nx = max(1, -(-segments // ny))
    for b in range(B):
        ys = np.minimum(np.arange(h) * ny // h, ny - 1)
        xs = np.minimum(np.arange(w) * nx // w, nx - 1)
        cell = ys[:, None] * nx + xs[None, :]                              # block index 0 .. ny * nx - 1
        pred = (cell + 1).astype(np.int32)
        ids = rng.choice(np.arange(1, 1 << 20), size=ny * nx, replace=False).astype(np.int64) * 7 + 3
        dy, dx = rng.randint(0, h // (3 * ny) + 1), rng.randint(0, w // (3 * nx) + 1)
        gt = np.roll(ids[cell], (dy, dx), axis=(0, 1))
        gt[: h // 20] = 0                                                   # a void band
        gts.append(gt)
        preds.append(pred)
    return gts, preds


def main():
    import numpy as np
    import torch
    from ldmseg_amd.evaluations import PanopticEvaluatorAgnostic, id2rgb
    from ldmseg_amd.evaluations.panoptic_evaluation_agnostic import gt_from_png
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8); ap.add_argument("--h", type=int, default=480); ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    B = args.B
    gts, preds = make_maps(B, args.h, args.w, args.segments)
    anns = [gt_from_png(gts[i], i, f"{i}.png") for i in range(B)]
    gt_maps = {i: gts[i] for i in range(B)}
    names, iids = [f"{i}.jpg" for i in range(B)], list(range(B))
    pred_dev = [torch.from_numpy(p).to(DEV) for p in preds]
    outs = [{"panoptic_seg": (pred_dev[i], [{"id": int(k), "category_id": 1, "isthing": True} for k in np.unique(preds[i])])}
            for i in range(B)]
    gt_rgb_dev = [torch.from_numpy(id2rgb(g)).to(DEV) for g in gts]
    rec = {"what": "pq_batch", "B": B, "h": args.h, "w": args.w, "segments": len(anns[0]["segments_info"])}
    results = {}

    def run(impl, feed):
        ev = PanopticEvaluatorAgnostic(gt_maps=gt_maps, gt_annotations=anns)
        ts, te = [], []
        for it in range(args.warmup + args.iters):
            ev.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feed(ev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = ev.evaluate()
            t2 = time.perf_counter()
            if it >= args.warmup:
                ts.append(1e3 * (t1 - t0))
                te.append(1e3 * (t2 - t1) / B)
        results[impl] = dict(res["panoptic_seg"])
        print(json.dumps(dict(rec, impl=impl, ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                              ms_per_image=round(statistics.median(ts) / B, 3), evaluate_ms_per_image=round(statistics.median(te), 4),
                              evaluate_ms_per_image_min=round(min(te), 4), evaluate_ms_per_image_max=round(max(te), 4))), flush=True)

    run("host process + evaluate", lambda ev: ev.process(names, iids, outs))
    run("device process_device, ground truth on the GPU (RGB bytes)", lambda ev: ev.process_device(names, iids, outs, gt_maps=gt_rgb_dev))
    run("device process_device, ground truth uploaded per batch (ids)", lambda ev: ev.process_device(names, iids, outs))
    same = all(r == results["host process + evaluate"] for r in results.values())
    print(json.dumps(dict(rec, what="pq_check", same_result=same, PQ=results["host process + evaluate"]["PQ"],
                          num_predictions=results["host process + evaluate"]["num_predictions"])), flush=True)
    if not same:
        raise SystemExit("the routes disagree: " + json.dumps(results))


if __name__ == "__main__":
    main()

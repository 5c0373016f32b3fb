"""Cost of the stage-1 (seg-VAE reconstruction) mIoU evaluation per batch: the fused path `GeneralVAESeg.reconstruct_semseg`
(encode -> posterior mode -> decode -> align_corners=True resampling + argmax / threshold + meter counters in one library call,
no host synchronisation) against the same evaluation done the way the reference does it (trainers_ae.py:728-803) with the
calls the library had before: `encode_moments`, `mode`, `decode(interpolate=False)`, then torch `F.interpolate`, `argmax`,
`softmax().max()` on the [B,128,8L,8L] fp32 logits and a torch restatement of the reference meter with its 3 x 128 `.item()`
calls (semseg_evaluation.py:28-33).

  python tools/ae_eval_cost.py [--B 8] [--L 64] [--warmup 3] [--iters 30] [--dtypes bf16 fp32]

Timing, the same for both paths: host clock around one batch ending in a device synchronise (the baseline synchronises 384 times
by itself), median of `iters` batches after `warmup`, with the fastest and slowest batch as the spread.  The fused tail alone comes from the library's per-launch HIP-event profile
(`ldmseg_profile_enable` / `ldmseg_profile_dump`, rows labelled `semseg_tail`) in a pass of its own.  Prints one JSON line per
measurement.  A record, not a gate."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"
NC, IGNORE = 128, 0


def median_ms(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


class ReferenceMeter(object):
    """semseg_evaluation.py:24-33 as written there: per class three masked sums, each read back with .item()"""

    def __init__(self, num_classes, ignore_index):
        self.n, self.ignore_index = num_classes, ignore_index
        self.tp, self.fp, self.fn = [0] * num_classes, [0] * num_classes, [0] * num_classes
        self.syncs = 0

    def update(self, pred, gt):
        import torch
        counted = gt != self.ignore_index
        for k in range(self.n):
            is_t, is_p = (gt == k) & counted, (pred == k) & counted
            # three masked sums per class, each read back on the host: that is the cost being measured
            self.tp[k] += int((is_t & is_p).sum().item())
            self.fp[k] += int((is_p & ~is_t).sum().item())
            self.fn[k] += int((is_t & ~is_p).sum().item())
            self.syncs += 3


def main():
    import torch
    import torch.nn.functional as F
    from ldmseg_amd import _lib, weights
    from ldmseg_amd.evaluations import SemsegMeter
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8); ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--mask-th", type=float, default=0.5)
    args = ap.parse_args()
    B, S = args.B, 8 * args.L
    sd = weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, 40, (B, S // 32, S // 32), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)
    ids[:, : S // 8] = IGNORE
    x = torch.stack([((ids >> k) & 1).float() for k in range(7)], 1)
    x[(ids == IGNORE)[:, None].expand_as(x)] = 0.5
    x, tg = x.to(DEV), ids.to(DEV)
    for cd in args.dtypes:
        vae = GeneralVAESeg(sd, device=DEV, compute_dtype=cd)
        meter = SemsegMeter(NC, [str(i) for i in range(NC)], has_bg=False, ignore_index=IGNORE)

        def fused():
            vae.reconstruct_semseg(x, (S, S), tg, meter.device_counts(DEV), in_mul=2.0, in_add=-1.0, mask_th=args.mask_th,
                                   ignore_label=IGNORE, ignore_index=IGNORE, return_preds=False)
        ref = ReferenceMeter(NC, IGNORE)

        def baseline():
            mom = vae.encode_moments(x, 2.0, -1.0)
            z = DiagonalGaussianDistribution(mom).mode()
            logits = vae.decode(z, interpolate=False)
            logits = F.interpolate(logits, size=(S, S), mode="bilinear", align_corners=True)
            preds = torch.argmax(logits, dim=1)
            probs = F.softmax(logits, dim=1).max(dim=1)[0]
            preds[probs < args.mask_th] = IGNORE
            ref.update(preds, tg)
        rec = {"what": "ae_miou_batch", "dtype": cd, "B": B, "L": args.L}
        ms_f, lo_f, hi_f = median_ms(fused, args.warmup, args.iters)
        print(json.dumps(dict(rec, impl="fused reconstruct_semseg", ms=round(ms_f, 3), ms_min=round(lo_f, 3), ms_max=round(hi_f, 3),
                              host_syncs_per_batch=0)), flush=True)
        ms_b, lo_b, hi_b = median_ms(baseline, args.warmup, args.iters)
        calls = args.warmup + args.iters
        print(json.dumps(dict(rec, impl="unfused torch tail + reference meter", ms=round(ms_b, 3), ms_min=round(lo_b, 3),
                              ms_max=round(hi_b, 3), host_syncs_per_batch=ref.syncs // calls)), flush=True)
        # same counters from both paths (up to near-ties: the fused tail resamples the compute-dtype map)
        fz = meter.return_score(verbose=False, suppress_prints=True)["mIoU"]
        n_f = args.warmup + args.iters
        tot_f = meter.tp.sum() + meter.fn.sum()
        tot_b = sum(ref.tp) + sum(ref.fn)
        print(json.dumps(dict(rec, what="ae_miou_check", fused_mIoU=float(fz), fused_tp_fn_per_batch=int(tot_f) // n_f,
                              baseline_tp_fn_per_batch=int(tot_b) // calls)), flush=True)
        # the tail alone, from the library's per-launch events, in a pass of its own
        lib = _lib.lib()
        lib.ldmseg_profile_reset()
        lib.ldmseg_profile_enable(1)
        for _ in range(args.iters):
            fused()
        torch.cuda.synchronize()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "prof.csv")
            _lib.check(lib.ldmseg_profile_dump(path.encode()), "ldmseg_profile_dump")
            rows = [r for r in csv.DictReader(open(path)) if r["label"].startswith("semseg_tail")]
        lib.ldmseg_profile_enable(0)
        lib.ldmseg_profile_reset()
        tail = statistics.median(float(r["ms"]) for r in rows)
        C4 = (4 * args.L) ** 2 * NC * (2 if cd == "bf16" else 4) * B
        print(json.dumps(dict(rec, what="ae_miou_tail", impl="semseg_scan_kernel", ms=round(tail, 4),
                              bytes_read=C4 + B * S * S * 8, gb_per_s=round((C4 + B * S * S * 8) / tail / 1e6, 1))), flush=True)
        del vae


if __name__ == "__main__":
    main()

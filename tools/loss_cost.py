"""Cost of the denoising loss: `TrainerDiffusion.compute_loss` (one UNet forward + the loss tail of csrc/loss.hip) against the same
arithmetic written with torch ops around the SAME UNet handle, and `get_loss_weight_mask(type_mask='counts')` against a
per-image `torch.unique` loop with its host round trips (the route the reference takes).

  python tools/loss_cost.py [--B 8] [--L 64] [--dtype bf16] [--regions 15] [--reps 5] [--out profiles/loss_cost.json]

Configuration: l2 loss, loss mask on, scheduler weights max_clamp_snr, OHEM off and at 0.7; mask [B,512,512] -> (64,64).
Timing: device events around a region of `reps` calls; regions of the new path and of the torch path alternate in one process after
a warm-up of each; reported: median and min-max of the per-call milliseconds over the regions.  `tail` rows time everything behind
the UNet output alone on a fixed prediction tensor (the share of a call = tail / call).  The mask rows use the host clock around a
synchronised call, since the torch loop synchronises by itself.  A record, not a gate: there is no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"


def torch_tail(prediction, target, noisy, t, loss_mask, weights, ac, ohem_ratio):
    """The torch-op route behind the UNet output, one eager op per step: squared error, pixel mask, timestep weight, optional
    top-k, mean; then the one-step estimate of the clean latents from the per-sample square roots of the alpha table."""
    import torch
    import torch.nn.functional as F
    per_sample = (-1, 1, 1, 1)
    elem = F.mse_loss(prediction.float(), target.float(), reduction='none')
    elem = elem * loss_mask.unsqueeze(1)
    elem = elem * weights[t].view(per_sample)
    flat = elem.reshape(-1)
    if ohem_ratio < 1.:
        flat = torch.topk(flat, int(ohem_ratio * flat.numel())).values
    value = flat.mean()
    alpha = ac[t].view(per_sample)
    root_a, root_b = alpha ** 0.5, (1 - alpha) ** 0.5
    x0 = (noisy - root_b * prediction) / (root_a * 1.0)       # (the scheduler's `scale` argument, 1.0: one more eager op)
    return value, x0


def torch_counts_mask(targets, size, ignore_label=0):
    """The torch-op route of the 'counts' mask: a nearest resize, then per image one `torch.unique(return_counts=True)` and, per
    id found, a comparison with the ignore label on the host (a device-to-host round trip each) and a masked store of 1 / count."""
    import torch
    import torch.nn.functional as F
    small = F.interpolate(targets.unsqueeze(1).float(), size=size, mode='nearest')[:, 0]
    out = torch.zeros_like(small)
    for b in range(small.shape[0]):
        ids, n = torch.unique(small[b], return_counts=True)
        for k in range(ids.numel()):
            if ids[k] == ignore_label:                  # tensor -> bool: the host waits for the device here
                continue
            out[b, small[b] == ids[k]] = 1. / n[k]
    return out


def main():
    import torch
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8); ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, L = args.B, args.L
    kw = dict(prediction_type="epsilon", beta_schedule="scaled_linear", num_train_timesteps=1000, beta_start=0.00085,
              beta_end=0.012, clip_sample=False, set_alpha_to_one=False, weight="max_clamp_snr", verbose=False)
    unet = UNet(weights.generate(weights.unet_schema(12, False), seed=0), in_channels=12, device=DEV, compute_dtype=args.dtype)
    unet.reserve(B, L)
    g = torch.Generator().manual_seed(0)
    latents, rgb, noise = (torch.randn(B, 4, L, L, generator=g).to(DEV) for _ in range(3))
    t = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    loss_mask = (torch.rand(B, L, L, generator=g) < 0.8).float().to(DEV)
    records = []

    def emit(**r):
        records.append(r)
        print(json.dumps(r), flush=True)

    def timed(fns, reps, regions):
        """{name: [ms per call of every region]} - the regions of the paths alternate"""
        out = {k: [] for k in fns}
        for _ in range(regions):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                out[name].append(e0.elapsed_time(e1) / reps)
        return out

    base = dict(B=B, L=L, dtype=args.dtype, loss="l2", weights="max_clamp_snr", loss_mask=True, regions=args.regions, reps=args.reps)
    for ohem in (1.0, 0.7):
        tr = TrainerDiffusion(None, unet, DDIMNoiseScheduler(**kw), ohem_ratio=ohem)
        sch = tr.noise_scheduler
        noisy = sch.add_noise(latents, noise, t)
        ac, wd = tr._scheduler_tables(torch.device(DEV))
        cond = torch.zeros_like(noisy)
        prediction = tr._predict(noisy, rgb, cond, t, None)

        def new_call():
            return tr.compute_loss(noise, t, noisy, rgb, None, loss_mask, latents=latents)

        def torch_call():
            p = tr._predict(noisy, rgb, torch.zeros_like(noisy), t, None)
            return torch_tail(p, noise, noisy, t, loss_mask, wd, ac, ohem)

        def new_tail():
            return tr._loss_tail(prediction, t, target=noise, noisy=noisy, loss_mask=loss_mask, prediction_type="epsilon",
                                 use_weights=True, ohem_ratio=ohem, want_pred=True)

        def torch_tail_only():
            return torch_tail(prediction, noise, noisy, t, loss_mask, wd, ac, ohem)

        a, b = new_call()[0], torch_call()[0]
        torch.cuda.synchronize()
        emit(what="loss_check", ohem_ratio=ohem, new=float(a), torch=float(b), rel_diff=abs(float(a) - float(b)) / abs(float(b)))
        for fns, what in (({"new": new_call, "torch": torch_call}, "compute_loss"), ({"new": new_tail, "torch": torch_tail_only}, "tail")):
            timed(fns, 2, 2)                                                     # warm-up of each path
            for name, ms in timed(fns, args.reps, args.regions).items():
                emit(**dict(base, what=what, ohem_ratio=ohem, impl=name, ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4),
                          ms_max=round(max(ms), 4)))
    # the loss-weight mask
    tr = TrainerDiffusion(None, unet, DDIMNoiseScheduler(**kw))
    targets = torch.randint(0, 24, (B, 64, 64), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).to(DEV)
    fns = {"new": lambda: tr.get_loss_weight_mask(targets, size=(64, 64), type_mask="counts"),
           "torch": lambda: torch_counts_mask(targets, (64, 64))}
    same = bool(torch.equal(fns["new"](), fns["torch"]()))
    res = {k: [] for k in fns}
    for it in range(3 + args.regions):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 3:
                res[name].append(1e3 * (time.perf_counter() - t0))
    for name, ms in res.items():
        emit(**dict(what="loss_weight_mask", type_mask="counts", shape=[B, 512, 512], size=[64, 64], ids=24, impl=name, same_result=same,
                  ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

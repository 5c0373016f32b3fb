"""Cost of the seg-VAE decoder's backward at the workload shape, one process, one device, after warm-up.

  python tools/measure_vae_backward.py [--B 8] [--L 64] [--reps 20] [--points 12544] [--modes fp32,bf16x3]
                                       [--out profiles/vae_backward_cost.json]

Per compute mode, median and min-max of the milliseconds per call over `reps` repetitions (3 warm-up calls of each first):
  (i)   ldmseg_vae_decode_backward alone, on fixed latents and a fixed gradient of the logits (HIP events around the call);
  (ii)  decode under grad + TrainerAE.compute_point_loss + backward() - the library's chain (host clock around a synchronised
        call: the point loss reads the host once);
  (iii) the same chain as torch ops: the oracle decoder (oracle/vae.py) moved to the GPU under torch autograd and the point loss
        of tests/point_loss_ref.py, the yardstick of DESIGN 8.5;
  (iv)  the weight-gradient launch of the last conv by itself (slices + the slab sum), from the library's per-launch profile of one
        decode_backward call, as TFLOP/s of its 2 * Co * 9 Ci * B * (4L)^2 FLOPs against the mode's MFMA peak; and the per-launch
        profile's eight longest launches (which kernel dominates).
(ii) and (iii) alternate in one loop.  A record, not a gate."""
import argparse
import ctypes as C
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
PEAK_TFLOPS = {"fp32": 157.3, "bf16x3": 2516.6 / 3}      # dense MFMA peaks of an MI355X; three bf16 products per fp32 product


def stats(ms):
    return dict(ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), reps=len(ms))


def main():
    import torch
    import point_loss_ref as PR
    from ldmseg_amd import _lib, weights
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.trainers import TrainerAE
    from ldmseg_amd.trainers.losses import draw_plan
    from oracle import vae as o_vae
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8); ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--points", type=int, default=12544)
    ap.add_argument("--segments", type=int, default=20); ap.add_argument("--modes", default="fp32,bf16x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_backward_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_vae_backward.py measures on the GPU; none found")
    B, L, P = args.B, args.L, args.points
    S = 4 * L
    lib = _lib.lib()
    g = torch.Generator().manual_seed(0)
    sd = weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
    z = (torch.randn(B, 4, L, L, generator=g) * 1.5).to(DEV)
    gl = torch.randn(B, 128, S, S, generator=g).to(DEV)
    blocks = max(S // 32, 1)
    ids = torch.stack([torch.randperm(127, generator=g)[:args.segments][torch.randint(0, args.segments, (blocks, blocks), generator=g)]
                       for _ in range(B)])
    targets = ids.repeat_interleave(S // blocks, 1).repeat_interleave(S // blocks, 2).to(DEV)
    records = []

    def emit(**r):
        records.append(r)
        print(json.dumps(r), flush=True)

    # the torch chain's decoder: leaves on the GPU
    tsd = {k: v.to(DEV).requires_grad_(True) for k, v in sd.items() if k.startswith("decoder.")}

    def torch_chain():
        for p in tsd.values():
            p.grad = None
        x = o_vae.decode(tsd, z, interpolate=False)
        rows = PR.mask_rows(targets, x.shape[1], 0)
        gg = torch.Generator(device=DEV).manual_seed(1)
        draws = {n: torch.rand(s, generator=gg, device=DEV) for n, s in draw_plan(B, int(rows.numel()), P, 3, 0.75)}
        r = PR.point_loss(x, targets, None, draws, P, 3, 0.75, 1.0, 0)
        (r["ce"] + r["mask"]).backward()

    for mode in args.modes.split(","):
        vae = GeneralVAESeg(sd, device=DEV, compute_dtype=mode)
        params = vae.decoder_parameters()
        tr = TrainerAE(vae, device=DEV, loss_weights={"mask": 1.0, "ce": 1.0, "kl": 0.0},
                       loss_kwargs=dict(num_points=P, oversample_ratio=3, importance_sample_ratio=0.75))
        base = dict(B=B, L=L, logits=[B, 128, S, S], mode=mode)
        grads = {k: torch.empty_like(p) for k, p in params.items()}
        n = len(grads)
        names = (C.c_char_p * n)(*[k.encode() for k in grads])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in grads.values()])
        numels = (C.c_int64 * n)(*[t.numel() for t in grads.values()])
        gz = torch.empty_like(z)

        def backward_alone():
            _lib.check(lib.ldmseg_vae_decode_backward(vae._h, _lib.ptr(z), 1.0, B, L, _lib.ptr(gl), _lib.ptr(gz), n, names, ptrs, numels,
                                                      _lib.stream_ptr(torch.device(DEV))), "ldmseg_vae_decode_backward")

        ms = []
        for it in range(3 + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            backward_alone()
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        emit(**base, what="(i) decode_backward alone", clock="HIP events", **stats(ms))

        from ldmseg_amd.models.vae import DiagonalGaussianDistribution
        from ldmseg_amd.utils import VAEOutput
        posterior = DiagonalGaussianDistribution(torch.zeros(B, 8, L, L, device=DEV))

        def lib_chain():
            for p in params.values():
                p.grad = None
            out = VAEOutput(sample=vae.decode(z, interpolate=False), posterior=posterior)
            tr.compute_point_loss(out, targets, generator=torch.Generator(device=DEV).manual_seed(1))[0].backward()

        pair = {"(ii) library: decode + point loss + backward": lib_chain, "(iii) torch ops: decode + point loss + backward": torch_chain}
        res = {k: [] for k in pair}
        failed = {}
        for it in range(3 + args.reps):
            for name, fn in pair.items():
                if name in failed:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    fn()
                except RuntimeError as e:          # (the torch chain needs torch's own conv backward on this device)
                    failed[name] = str(e)[:300]
                    continue
                torch.cuda.synchronize()
                if it >= 3:
                    res[name].append(1e3 * (time.perf_counter() - t0))
        for name, v in res.items():
            if name in failed:
                emit(**base, what=name, failed=failed[name])
            else:
                emit(**base, what=name, clock="host, synchronised call", **stats(v))

        # per-launch profile of one decode_backward call
        fd, path = tempfile.mkstemp(suffix=".csv")
        os.close(fd)
        lib.ldmseg_profile_reset(); lib.ldmseg_profile_enable(1)
        backward_alone()
        torch.cuda.synchronize(); lib.ldmseg_profile_enable(0)
        lib.ldmseg_profile_dump(path.encode())
        lib.ldmseg_profile_reset()
        with open(path) as f:
            rows = list(csv.DictReader(f))
        os.remove(path)
        total_ms = sum(float(r["ms"]) for r in rows)
        top = sorted(rows, key=lambda r: -float(r["ms"]))[:8]
        emit(**base, what="per-launch profile of one decode_backward", launches=len(rows), sum_ms=round(total_ms, 4),
             longest=[dict(label=r["label"], ms=round(float(r["ms"]), 4)) for r in top])
        wg = [r for r in rows if r["label"].startswith("wgrad ") and "taps=9" in r["label"]]
        last = max(wg, key=lambda r: float(r["flops"]))
        flops = 2.0 * 128 * 2304 * B * S * S
        tf = flops / (float(last["ms"]) * 1e-3) / 1e12
        emit(**base, what="(iv) weight gradient of the last conv (slices + slab sum)", label=last["label"], ms=round(float(last["ms"]), 4),
             tflops=round(tf, 2), peak_tflops=round(PEAK_TFLOPS[mode], 1), of_peak=round(tf / PEAK_TFLOPS[mode], 4))
        del vae, tr
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

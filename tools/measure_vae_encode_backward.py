"""Cost of the seg-VAE encoder's backward and of the whole stage-1 step at the workload shape, one process, one
device, after warm-up.

  python tools/measure_vae_encode_backward.py [--B 8] [--H 512] [--reps 10] [--points 12544] [--modes fp32,bf16x3]
                                              [--out profiles/vae_encode_backward_cost.json]

Per compute mode, median and min-max of the milliseconds per call over `reps` repetitions (3 warm-up calls of each first):
  (i)   ldmseg_vae_encode_backward alone, on fixed bit planes and a fixed gradient of the moments (HIP events around the call);
  (ii)  the whole step's gradient: forward under grad (sampled posterior) + TrainerAE.compute_point_loss + backward() of both halves
        (host clock around a synchronised call: the point loss reads the host once);
  (iii) the same chain as torch ops: the oracle encoder and decoder (oracle/vae.py) moved to the GPU under torch autograd, the
        posterior and KL in torch, and the point loss of tests/point_loss_ref.py;
  (iv)  every weight-gradient launch of one encode_backward call from the library's per-launch profile (slices + the slab sum), with
        the MACs its tiles execute over the layer's own and the bytes of its two operands; and the eight longest launches.
(ii) and (iii) alternate in one loop.  A record, not a gate."""
import argparse
import ctypes as C
import csv
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"


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
    ap.add_argument("--B", type=int, default=8); ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--points", type=int, default=12544)
    ap.add_argument("--segments", type=int, default=20); ap.add_argument("--modes", default="fp32,bf16x3")
    ap.add_argument("--kl", type=float, default=1e-4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_encode_backward_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_vae_encode_backward.py measures on the GPU; none found")
    B, H, P = args.B, args.H, args.points
    l, S = H // 8, H // 2
    lib = _lib.lib()
    g = torch.Generator().manual_seed(0)
    sd = weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
    blocks = max(S // 32, 1)
    ids = torch.stack([torch.randperm(127, generator=g)[:args.segments][torch.randint(0, args.segments, (blocks, blocks), generator=g)]
                       for _ in range(B)])
    targets = ids.repeat_interleave(S // blocks, 1).repeat_interleave(S // blocks, 2).to(DEV)
    full = ids.repeat_interleave(H // blocks, 1).repeat_interleave(H // blocks, 2)
    x = (2.0 * torch.stack([(full >> i) % 2 for i in range(7)], dim=1).float() - 1.0).to(DEV)
    gm = torch.randn(B, 8, l, l, generator=g).to(DEV)
    records = []

    def emit(**r):
        records.append(r)
        print(json.dumps(r), flush=True)

    tsd = {k: v.to(DEV).requires_grad_(True) for k, v in sd.items()}

    def torch_chain():
        for p in tsd.values():
            p.grad = None
        mom = o_vae.encode_moments(tsd, x)
        mean, logvar = mom[:, :4], torch.clamp(mom[:, 4:], -30.0, 20.0)
        z = mean + torch.exp(0.5 * logvar) * torch.randn(mean.shape, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV)
        kl = 0.5 * torch.sum(mean.pow(2) + logvar.exp() - 1.0 - logvar, dim=[1, 2, 3]).mean()
        y = o_vae.decode(tsd, z, interpolate=False)
        rows = PR.mask_rows(targets, y.shape[1], 0)
        gg = torch.Generator(device=DEV).manual_seed(1)
        draws = {n: torch.rand(s, generator=gg, device=DEV) for n, s in draw_plan(B, int(rows.numel()), P, 3, 0.75)}
        r = PR.point_loss(y, targets, None, draws, P, 3, 0.75, 1.0, 0)
        (r["ce"] + r["mask"] + args.kl * kl).backward()

    for mode in args.modes.split(","):
        vae = GeneralVAESeg(sd, device=DEV, compute_dtype=mode)
        enc = vae.encoder_parameters()
        params = vae.parameters()
        tr = TrainerAE(vae, device=DEV, loss_weights={"mask": 1.0, "ce": 1.0, "kl": args.kl},
                       loss_kwargs=dict(num_points=P, oversample_ratio=3, importance_sample_ratio=0.75))
        base = dict(B=B, H=H, mode=mode)
        grads = {k: torch.empty_like(p) for k, p in enc.items()}
        n = len(grads)
        names = (C.c_char_p * n)(*[k.encode() for k in grads])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in grads.values()])
        numels = (C.c_int64 * n)(*[t.numel() for t in grads.values()])

        def backward_alone():
            _lib.check(lib.ldmseg_vae_encode_backward(vae._h, _lib.ptr(x), 1.0, 0.0, B, H, _lib.ptr(gm), n, names, ptrs, numels,
                                                      _lib.stream_ptr(torch.device(DEV))), "ldmseg_vae_encode_backward")

        ms = []
        for it in range(3 + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            backward_alone()
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        emit(**base, what="(i) encode_backward alone", clock="HIP events", **stats(ms))

        def lib_chain():
            for p in params:
                p.grad = None
            out = vae(x, sample_posterior=True, generator=torch.Generator(device=DEV).manual_seed(2))
            tr.compute_point_loss(out, targets, generator=torch.Generator(device=DEV).manual_seed(1))[0].backward()

        pair = {"(ii) library: forward + point loss + backward of both halves": lib_chain,
                "(iii) torch ops: forward + point loss + backward of both halves": torch_chain}
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

        # per-launch profile of one encode_backward call
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
        emit(**base, what="per-launch profile of one encode_backward", launches=len(rows), sum_ms=round(total_ms, 4),
             longest=[dict(label=r["label"], ms=round(float(r["ms"]), 4)) for r in top])
        for r in rows:
            m = re.match(r"wgrad \w+ P=(\d+) N=(\d+) C=(\d+) taps=(\d+) slices=(\d+) grid=(\d+) tile=(\d+)x(\d+) stride=(\d+)", r["label"])
            if not m:
                continue
            Pp, N, Cc, taps, slices, grid, tn, tc, stride = map(int, m.groups())
            executed = -(-N // tn) * tn * -(-Cc // tc) * tc
            msr = float(r["ms"])
            emit(**base, what="(iv) weight gradient (slices + slab sum)", label=r["label"], ms=round(msr, 4),
                 executed_mac_ratio=round(executed / (N * Cc), 3), operand_bytes=4 * Pp * (N + Cc * stride * stride),
                 tflops_executed=round(2.0 * Pp * executed * taps / (msr * 1e-3) / 1e12, 2))
        del vae, tr
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

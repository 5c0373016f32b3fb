"""Cost of the fused clip + AdamW step (csrc/optim.hip) against torch's optimisers, one process, one device.

  python tools/bench_optim.py [--reps 15] [--inner 20] [--skip-step] [--skip-unet] [--out profiles/optim_cost.json]

Method of DESIGN 6: warm-up, then `reps` repetitions in which the variants ALTERNATE; each repetition times `inner` back-to-back
steps between two device events (one step is tens of microseconds at the seg-VAE's size); median and min-max of the milliseconds
per step.  Every variant owns its tensors (same shapes, same seeded values), clips to max_norm 3.0 (base.yaml: clip_grad) and uses
lr 1e-4, weight decay 0.01.
  (a) the seg-VAE's 34 tensors (about 3 M parameters, launch bound): the library step (two launches) against
      clip_grad_norm_ + torch.optim.AdamW(fused=True) and against foreach=True; `GeneralVAESeg.refresh()` alone; and the whole
      TrainerAE.training_step at B = 8, 512 x 512, 12544 points with either optimiser (host clock around a synchronised call: the
      point loss reads the host once per step).
  (b) a UNet-sized list: the tensor shapes of the default UNet (weights.unet_schema()), about 860 M parameters, a pure HBM stream.
      Milliseconds and achieved bytes per second counting 4 reads + 4 writes of 4 bytes per element (p, g, m, v each read and
      written once; the norm pass's extra read of g is not counted, so it lowers the figure), against torch's fused path.
A record, not a gate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"
MAX_NORM, LR, WD = 3.0, 1e-4, 0.01


def stats(ms):
    return dict(ms=round(statistics.median(ms), 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5), reps=len(ms))


def alternate(variants, inner, reps, warm=3):
    """{name: fn} -> {name: [ms per call]}: the variants take turns; each turn is `inner` calls between two device events"""
    import torch
    out = {k: [] for k in variants}
    for it in range(warm + reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= warm:
                out[name].append(e0.elapsed_time(e1) / inner)
    return out


def tensor_sets(shapes, count, seed=0):
    """`count` lists of leaf tensors of these shapes on the device with a .grad each, the same seeded values in every list"""
    import torch
    sets = []
    for _ in range(count):
        g = torch.Generator(device=DEV).manual_seed(seed)
        ps = []
        for s in shapes:
            p = torch.randn(s, generator=g, device=DEV).requires_grad_(True)
            p.grad = torch.randn(s, generator=g, device=DEV) * 0.01
            ps.append(p)
        sets.append(ps)
    return sets


def optimiser_variants(shapes, which):
    import torch
    from ldmseg_amd.optim import AdamW
    sets = tensor_sets(shapes, len(which))
    out = {}
    for ps, name in zip(sets, which):
        if name == "library":
            opt = AdamW(ps, lr=LR, weight_decay=WD)
            out["library: ldmseg_adamw_step (clip fused in)"] = lambda opt=opt: opt.step(max_norm=MAX_NORM)
        else:
            kw = dict(fused=True) if name == "fused" else dict(foreach=True)
            opt = torch.optim.AdamW(ps, lr=LR, weight_decay=WD, **kw)

            def fn(ps=ps, opt=opt):
                torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
                opt.step()
            out[f"torch: clip_grad_norm_ + AdamW({name}=True)"] = fn
    return out


def main():
    import torch
    from ldmseg_amd import weights
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15); ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="leave out the whole training step of (a)")
    ap.add_argument("--skip-unet", action="store_true", help="leave out (b)")
    ap.add_argument("--B", type=int, default=8); ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU; none found")
    records = []

    def emit(**r):
        records.append(r)
        print(json.dumps(r), flush=True)

    # (a) the seg-VAE's list
    vshapes = list(weights.vae_schema().values())
    nparam = sum(int(torch.Size(s).numel()) for s in vshapes)
    res = alternate(optimiser_variants(vshapes, ["library", "fused", "foreach"]), args.inner, args.reps)
    for name, ms in res.items():
        emit(size="(a) seg-VAE list", tensors=len(vshapes), parameters=nparam, what=name, clock="device events", inner=args.inner, **stats(ms))

    if not args.skip_step:
        from ldmseg_amd.models import GeneralVAESeg
        from ldmseg_amd.optim import AdamW
        from ldmseg_amd.trainers import TrainerAE
        B, H = args.B, args.H
        S = H // 2
        g = torch.Generator().manual_seed(0)
        sd = weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
        blocks = max(S // 32, 1)
        ids = torch.stack([torch.randperm(127, generator=g)[:20][torch.randint(0, 20, (blocks, blocks), generator=g)] for _ in range(B)])
        targets = ids.repeat_interleave(S // blocks, 1).repeat_interleave(S // blocks, 2).to(DEV)
        full = ids.repeat_interleave(H // blocks, 1).repeat_interleave(H // blocks, 2)
        x = (2.0 * torch.stack([(full >> i) % 2 for i in range(7)], dim=1).float() - 1.0).to(DEV)
        for mode in ("fp32", "bf16x3"):
            runs = {}
            for name in ("library AdamW", "torch AdamW(fused=True)"):
                vae = GeneralVAESeg(sd, device=DEV, compute_dtype=mode)
                tr = TrainerAE(vae, device=DEV, loss_weights={"mask": 1.0, "ce": 1.0, "kl": 1e-4})
                opt = AdamW(vae.parameters(), lr=LR, weight_decay=WD) if name.startswith("library") else \
                    torch.optim.AdamW(vae.parameters(), lr=LR, weight_decay=WD, fused=True)
                gd, gp = torch.Generator(device=DEV).manual_seed(2), torch.Generator(device=DEV).manual_seed(1)
                runs[name] = (vae, lambda tr=tr, opt=opt, gd=gd, gp=gp: tr.training_step(x, targets, opt, clip_grad=MAX_NORM, generator=gd,
                                                                                         point_generator=gp))
            ms = {k: [] for k in runs}
            for it in range(3 + args.reps):
                for name, (_, fn) in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it >= 3:
                        ms[name].append(1e3 * (time.perf_counter() - t0))
            for name, v in ms.items():
                emit(size="(a) whole training_step", B=B, H=H, mode=mode, what=name, clock="host, synchronised call", **stats(v))
            vae = runs["library AdamW"][0]
            r = alternate({"refresh()": vae.refresh}, 10, args.reps)
            emit(size="(a) GeneralVAESeg.refresh() alone", mode=mode, what="refresh()", clock="device events", inner=10, **stats(r["refresh()"]))
            del runs, vae

    if not args.skip_unet:
        ushapes = list(weights.unet_schema().values())
        nparam = sum(int(torch.Size(s).numel()) for s in ushapes)
        res = alternate(optimiser_variants(ushapes, ["library", "fused"]), 3, args.reps)
        for name, ms in res.items():
            st = stats(ms)
            emit(size="(b) UNet-sized list", tensors=len(ushapes), parameters=nparam, what=name, clock="device events", inner=3,
                 bytes_counted=32 * nparam, tb_per_s=round(32 * nparam / (st["ms"] * 1e-3) / 1e12, 3), **st)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

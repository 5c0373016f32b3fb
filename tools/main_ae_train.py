#!/usr/bin/env python
"""Stage-1 training entry of the MI355X build - the counterpart of the reference's `tools/main_ae.py` without `eval_only`, over the
folder loader of tools/main_ae_eval.py: the segmentation VAE learns to reconstruct panoptic maps through its 4-channel latent.

    python tools/main_ae_train.py --panoptic DIR [--ae ae.pt | --resume model.pt] [--steps 100] [--batch 8] [--size 512]
                                  [--dtype fp32|bf16x3] [--lr 1e-4] [--clip-grad 3.0] [--warmup-iters 200] [--weight-decay 0.0]
                                  [--print-freq 10] [--out DIR] [--seed 0]

Every step is `TrainerAE.training_step` with the library's fused clip + AdamW (`ldmseg_amd.optim.AdamW`): forward with a sampled
posterior, point CE + mask + KL loss, backward of both halves, one ldmseg_adamw_step call, refresh.  The learning rate follows the
reference's `warmup` schedule (base.yaml: lr 1e-4, 200 warm-up iterations; `ldmseg_amd.trainers.lr_schedules`) and is written into the
param groups at every step.  The four losses and the gradient norm are printed every --print-freq steps, with ONE host read per
print.  --out: `model.pt` in the reference's layout is written there at the end (`TrainerAE.save`); --resume continues from such a
file, optimiser state and step count included.  An epoch is one pass over the folder.  Without --ae / --resume deterministic
random weights of the right architecture are trained.  No EMA, no gradient accumulation, no fp16 scaler.
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from main_ae_eval import IGNORE_LABEL, NUM_CLASSES, batches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panoptic", required=True, help="folder of COCO panoptic PNGs (e.g. data/examples/coco/panoptic_images)")
    ap.add_argument("--ae", default=None, help="AE checkpoint to start from (ae.pt); generated weights without it")
    ap.add_argument("--resume", default=None, help="model.pt written by an earlier run's --out: weights, optimiser state, step")
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--lr", type=float, default=1e-4); ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--clip-grad", type=float, default=3.0); ap.add_argument("--warmup-iters", type=int, default=200)
    ap.add_argument("--kl-weight", type=float, default=0.0)
    ap.add_argument("--print-freq", type=int, default=10)
    ap.add_argument("--out", default=None, help="folder for model.pt")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.size % 8:
        ap.error("--size must be a multiple of 8")
    if not torch.cuda.is_available():
        raise SystemExit("main_ae_train.py trains on the GPU; none found")
    from ldmseg_amd import checkpoint, weights
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.optim import AdamW
    from ldmseg_amd.trainers import TrainerAE
    from ldmseg_amd.trainers.lr_schedules import warmup_scheduler
    device = torch.device("cuda", 0)
    files = sorted(glob.glob(os.path.join(args.panoptic, "*.png")))
    if not files:
        raise SystemExit(f"no PNG under {args.panoptic}")
    vsd = checkpoint.load_ae_checkpoint(args.ae) if args.ae else weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
    vae = GeneralVAESeg(vsd, device=device, compute_dtype=args.dtype)
    trainer = TrainerAE(vae, num_classes=NUM_CLASSES, ignore_label=IGNORE_LABEL, device=device,
                        loss_weights={"mask": 1.0, "ce": 1.0, "kl": args.kl_weight})
    opt = AdamW(vae.parameters(), lr=args.lr, betas=(0.9, 0.999), weight_decay=args.weight_decay)      # base.yaml:135-139
    epoch, step = 0, 0
    if args.resume:
        epoch, step = trainer.resume(args.resume, opt)
    per_epoch = -(-len(files) // args.batch)
    last = step + args.steps
    schedule = warmup_scheduler(args.lr, 0.0, -(-last // per_epoch), per_epoch, warmup_iters=min(args.warmup_iters, last))
    noise = torch.Generator(device=device).manual_seed(args.seed + step)
    points = torch.Generator().manual_seed(args.seed + step)
    while step < last:
        for data in batches(files, args.size, args.batch, device, seed=1 + epoch):
            if step >= last:
                break
            images = 2.0 * data["image_semseg"] - 1.0                                                    # trainers_ae.py:256
            vals = trainer.training_step(images, data["semseg"].to(device), opt, clip_grad=args.clip_grad, generator=noise,
                                         point_generator=points, lr=schedule[step])
            step += 1
            if step % args.print_freq == 0 or step == last:
                norm = trainer.last_grad_norm if trainer.last_grad_norm is not None else torch.zeros((), device=device)
                loss, ce, kl, mask, gn = torch.stack(list(vals) + [norm]).cpu().tolist()                   # the one host read
                print(json.dumps({"step": step, "epoch": epoch, "lr": float(schedule[step - 1]), "loss": loss, "ce": ce, "kl": kl,
                                  "mask": mask, "grad_norm": gn if args.clip_grad > 0 else None}), flush=True)
        else:
            epoch += 1
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        trainer.save(os.path.join(args.out, "model.pt"), opt, epoch=epoch, step=step,
                     p={"optimizer_name": "adamw", "optimizer_kwargs": {"lr": args.lr, "betas": [0.9, 0.999], "weight_decay": args.weight_decay},
                        "clip_grad": args.clip_grad, "lr_scheduler_name": "warmup", "lr_scheduler_kwargs": {"warmup_iters": args.warmup_iters},
                        "train_kwargs": {"batch_size": args.batch}, "size": args.size, "dtype": args.dtype})
        print(f"wrote {os.path.join(args.out, 'model.pt')}")


if __name__ == "__main__":
    main()

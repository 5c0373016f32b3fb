#!/usr/bin/env python
"""Stage-1 evaluation entry of the MI355X build - the counterpart of `tools/main_ae.py` with `eval_only`
(the reference's tools/main_ae.py:189-190: `trainer.compute_metrics(['miou', 'pq'])`): how well the segmentation VAE
reconstructs ground-truth panoptic maps through its 4-channel latent.  This is the upper bound of what the diffusion
sampler can reach, and the check to run after loading `ae.pt`.

    python tools/main_ae_eval.py --panoptic DIR [--ae ae.pt] [--size 512] [--batch 8] [--dtype bf16]
                                 [--mask-th 0.5] [--count-th 512] [--overlap-th 0.5] [--out DIR] [--device-pq]
                                 [--val-loss [--seed 0]]

Per image: COCO panoptic PNG -> segment ids -> remapped to random distinct labels in [1, 128) with the background (0) fixed
(coco.py:320-348, seeded here) -> nearest-neighbour resize of the longer side to --size and zero padding to a square (the
padding is `ignore_label`, the padding mask marks the image) -> 7 bit planes through the library's bit codec.  Then
`TrainerAE.compute_miou` (reconstruction against the remapped map at the network size) and `TrainerAE.compute_pq`
(reconstruction cropped and resized to the original size, class-agnostic PQ against the PNG itself).
With --val-loss also the stage-1 loss the reference's training loop logs (`TrainerAE.validation_loss`: point CE + mask + KL), as
one extra JSON line.
Without --ae deterministic random weights of the right architecture are used: the pipeline runs end to end but the numbers
are meaningless.
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

NUM_CLASSES, IGNORE_LABEL = 128, 0          # tools/configs/base/base.yaml: num_classes 128, ignore_label 0


def remap_labels(ids: np.ndarray, rng: np.random.RandomState) -> np.ndarray:
    """coco.py:320-348 with keep_background_fixed: every segment id gets a distinct random label in [1, NUM_CLASSES)."""
    uniq = [x for x in np.unique(ids) if x != IGNORE_LABEL]
    if len(uniq) >= NUM_CLASSES:
        raise ValueError(f"{len(uniq)} segments do not fit {NUM_CLASSES} labels")
    targets = rng.choice(NUM_CLASSES - 1, size=len(uniq), replace=False) + 1
    out = np.full(ids.shape, IGNORE_LABEL, dtype=np.int64)
    for val, t in zip(uniq, targets):
        out[ids == val] = t
    return out


def load_sample(path: str, size: int, rng: np.random.RandomState):
    """-> (remapped ids [size,size] int64 padded with IGNORE_LABEL, padding mask [size,size] bool, original (h, w))."""
    from PIL import Image
    from ldmseg_amd.evaluations import rgb2id
    ids = rgb2id(np.asarray(Image.open(path).convert("RGB")))
    h, w = ids.shape
    lab = remap_labels(ids, rng)
    s = size / max(h, w)
    nh, nw = max(1, min(size, round(h * s))), max(1, min(size, round(w * s)))
    small = np.asarray(Image.fromarray(lab.astype(np.uint8)).resize((nw, nh), resample=getattr(Image, "Resampling", Image).NEAREST))
    out = np.full((size, size), IGNORE_LABEL, dtype=np.int64)
    out[:nh, :nw] = small
    mask = np.zeros((size, size), dtype=bool)
    mask[:nh, :nw] = True
    return torch.from_numpy(out), torch.from_numpy(mask), (h, w)


def batches(files, size, batch, device, seed=1):
    """Batches shaped like the reference's collate_fn output for the AE trainer: 'image_semseg' [B,7,S,S] bit maps in [0,1] (on
    the GPU: the codec runs there), 'semseg' [B,S,S] int64, 'mask' [B,S,S], 'meta'."""
    from ldmseg_amd.data.bitcodec import encode_bitmap
    for i in range(0, len(files), batch):
        chunk = files[i:i + batch]
        ids, masks, meta = [], [], []
        for j, f in enumerate(chunk):
            lab, m, hw = load_sample(f, size, np.random.RandomState(seed + i + j))
            ids.append(lab); masks.append(m)
            meta.append({"image_file": f, "image_id": os.path.splitext(os.path.basename(f))[0], "im_size": hw})
        semseg = torch.stack(ids)
        bits, _ = encode_bitmap(semseg.to(device), n=7, fill_value=0.5, ignore_label=IGNORE_LABEL)
        yield {"image_semseg": bits, "semseg": semseg, "mask": torch.stack(masks), "meta": meta}


def build_trainer(args, device):
    from ldmseg_amd import checkpoint, weights
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.trainers import TrainerAE
    if args.ae:
        vsd = checkpoint.load_ae_checkpoint(args.ae)
    else:
        vsd = weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
    vae = GeneralVAESeg(vsd, device=device, compute_dtype=args.dtype)
    return TrainerAE(vae, num_classes=NUM_CLASSES, ignore_label=IGNORE_LABEL, mask_th=args.mask_th, count_th=args.count_th,
                     overlap_th=args.overlap_th, device=device)


def evaluate(args, device, files, trainer=None):
    """-> (mIoU result dict, PQ result dict, evaluator)."""
    import torch.distributed as dist
    from ldmseg_amd.evaluations import PanopticEvaluatorAgnostic, rgb2id
    from ldmseg_amd.evaluations.panoptic_evaluation_agnostic import gt_from_png
    from PIL import Image
    trainer = trainer if trainer is not None else build_trainer(args, device)
    gt_maps, gt_anns = {}, []
    for f in sorted(glob.glob(os.path.join(args.panoptic, "*.png"))):
        iid = os.path.splitext(os.path.basename(f))[0]
        gt_maps[iid] = rgb2id(np.asarray(Image.open(f).convert("RGB")))
        gt_anns.append(gt_from_png(gt_maps[iid], iid, os.path.basename(f)))
    world = dist.get_world_size() if dist.is_initialized() else 1
    gloo = dist.new_group(backend="gloo") if world > 1 else None           # object gather side group (detectron2 comm)
    ev = PanopticEvaluatorAgnostic(output_dir=args.out, gt_maps=gt_maps, gt_annotations=gt_anns, group=gloo,
                                   on_device=getattr(args, "device_pq", False))
    out = trainer.compute_metrics(["miou", "pq"], lambda: batches(files, args.size, args.batch, device), evaluator=ev,
                                  threshold_output=args.threshold_output)
    return out["miou"], out["pq"], ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panoptic", required=True, help="folder of COCO panoptic PNGs (e.g. data/examples/coco/panoptic_images)")
    ap.add_argument("--ae", default=None, help="AE checkpoint (ae.pt); generated weights without it")
    ap.add_argument("--size", type=int, default=512); ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--mask-th", type=float, default=0.5); ap.add_argument("--count-th", type=int, default=512)
    ap.add_argument("--overlap-th", type=float, default=0.5)
    ap.add_argument("--threshold-output", action="store_true", help="max-softmax threshold in both metrics (trainers_ae.py:549)")
    ap.add_argument("--out", default=None, help="folder for the prediction PNGs and the evaluator's predictions.json")
    ap.add_argument("--device-pq", action="store_true",
                    help="score PQ on the GPU (PanopticEvaluatorAgnostic.process_device): no map is copied to the host")
    ap.add_argument("--val-loss", action="store_true",
                    help="also print the stage-1 loss (TrainerAE.validation_loss: total / ce / kl / mask) as one JSON line")
    ap.add_argument("--seed", type=int, default=0, help="seed of the point draws of --val-loss")
    args = ap.parse_args()
    if args.size % 8:
        ap.error("--size must be a multiple of 8")
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    files = sorted(glob.glob(os.path.join(args.panoptic, "*.png")))[rank::world]      # images sharded over ranks
    trainer = build_trainer(args, device)
    miou, pq, ev = evaluate(args, device, files, trainer)
    # the stage-1 loss of this rank's images (the point draws are per process; ranks are not averaged)
    val = trainer.validation_loss(batches(files, args.size, args.batch, device), seed=args.seed) if args.val_loss else None
    if rank == 0:
        print(f"mIoU {float(100 * miou['mIoU'])!r}")
        print(ev.table)
        r = pq["panoptic_seg"]
        print(f"PQ {float(r['PQ'])!r} SQ {float(r['SQ'])!r} RQ {float(r['RQ'])!r} num_predictions {r['num_predictions']}")
        if val is not None:
            print(json.dumps({"val_loss": val}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

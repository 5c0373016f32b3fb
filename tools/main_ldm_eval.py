#!/usr/bin/env python
"""Evaluation entry of the MI355X build - the counterpart of `tools/main_ldm.py base.eval_only=True`
(/root/reference/tools/main_ldm.py:130-232; the reference script itself is hard-wired to CUDA, NCCL, hydra, diffusers and
detectron2 and cannot run here).

    python tools/main_ldm_eval.py --images DIR [--panoptic DIR] [--ldm ldmseg.pt --ae ae.pt --vae-image vae.pt]
                                  [--size 512] [--steps 50] [--batch 8] [--dtype bf16]
                                  [--image-descriptors {remove,clip_image,clip_image_proj}] [--clip-vision clip.pt]
                                  [--val-loss]

It assembles what main_worker assembles (image VAE encoder, seg-VAE, UNet with the 12-channel conv_in and cross-attention
removed, DDIM scheduler with base.yaml's noise_scheduler_kwargs), then runs `TrainerDiffusion.compute_pq`:
PIL resize (CropResize) -> 2x-1 -> image VAE -> 50-step DDIM sampling -> seg-VAE decode -> bilinear to the original
size -> argmax / thresholds / segment filtering -> class-agnostic PQ against the COCO panoptic PNGs.
One process per GPU under torch.distributed.run shards the images over ranks (DistributedSampler semantics,
trainers_ldm_cond.py:245); the evaluator gathers the predictions on rank 0.
Without checkpoints (none ship with this repo: the released ones are 3.3 GB downloads) deterministic random weights
of the right architecture are used - the pipeline then runs end to end but the PQ is meaningless.

`--val-loss` (needs `--panoptic`) scores the checkpoint by its denoising loss instead: the panoptic PNGs become 7-plane bit maps
the way tools/main_ae_eval.py makes them (segment ids -> random distinct labels -> bit codec), resized like the RGB image, and
`TrainerDiffusion.validation_loss` prints {'loss', 'per_timestep', 'images'} as one JSON line: one UNet forward per image and
timestep.  One process only (the sums are not reduced across ranks).
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

NOISE_SCHEDULER_KWARGS = dict(prediction_type="epsilon", beta_schedule="scaled_linear", num_train_timesteps=1000,
                              beta_start=0.00085, beta_end=0.012, steps_offset=1, clip_sample=False, set_alpha_to_one=False,
                              thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0,
                              sample_max_value=1.0, weight="none", max_snr=5.0)      # tools/configs/base/base.yaml:48-62


def build_trainer(args, device):
    from ldmseg_amd import checkpoint, weights
    from ldmseg_amd.models import UNet, GeneralVAESeg, GeneralVAEImage
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    if args.ldm:
        ck = checkpoint.load_ldm_checkpoint(args.ldm)
        usd = ck["unet"]
        vsd = checkpoint.load_ae_checkpoint(args.ae) if args.ae else ck["vae_semseg"]
    else:
        usd = weights.generate(weights.unet_schema(12, False), seed=0)
        vsd = weights.generate(weights.vae_schema(), seed=7, norm_keys=weights.VAE_NORM_KEYS)
    if args.vae_image:
        isd = torch.load(args.vae_image, map_location="cpu", weights_only=True)
    else:
        isd = weights.generate(weights.vae_image_schema(), seed=11, norm_keys=weights.VAE_IMAGE_NORM_KEYS)
    # image_descriptors (tools/configs/base/base.yaml, trainers_ldm_cond.py:55-127): remove = the UNet without cross-attention;
    # clip_image = CLIP-L/14 patch features [B, 257, 1024] through encoder_hid_proj; clip_image_proj = the projected image
    # embedding [B, 1, 768].  The descriptor runs on the library (models.CLIPVisionDescriptor).
    cross = args.image_descriptors != "remove"
    desc = None
    if cross:
        from ldmseg_amd.models import CLIPVisionDescriptor
        proj = args.image_descriptors == "clip_image_proj"
        if not args.ldm:
            # the conditioned UNet is the 8-channel one: self-conditioning (12 channels) cannot be combined with the guidance
            # the descriptor modes run under (multiplier 2)
            usd = weights.generate(weights.unet_schema(8, True), seed=0)
            if not proj:
                usd.update(weights.generate(weights.hid_proj_schema(), seed=12))
        if args.clip_vision:
            csd = torch.load(args.clip_vision, map_location="cpu", weights_only=True)
        else:
            schema = weights.clip_vision_schema(projection_dim=768 if proj else 0)
            csd = weights.generate(schema, seed=13, norm_keys=weights.clip_vision_norm_keys(schema))
        desc = CLIPVisionDescriptor(csd, projection=proj, device=device, compute_dtype=args.dtype)
    # (a separate-encoder checkpoint keeps its 4-channel conv_in and takes the 8-channel [segmentation | image] input)
    in_ch = 8 if "conv_in_img.weight" in usd else int(usd["conv_in.weight"].shape[1])
    unet = UNet(usd, in_channels=in_ch, device=device, compute_dtype=args.dtype, cross_attention=cross)
    vae = GeneralVAESeg(vsd, scaling_factor=args.scaling_factor, device=device, compute_dtype=args.dtype)
    enc = GeneralVAEImage(isd, scaling_factor=0.18215, device=device, compute_dtype=args.dtype)
    return TrainerDiffusion(vae, unet, DDIMNoiseScheduler(**NOISE_SCHEDULER_KWARGS), vae_image=enc,
                            latent_size=args.size // 8, image_descriptor_model=desc)


def batches(files, size, batch, panoptic_dir):
    from ldmseg_amd.data.transforms import load_rgb
    for i in range(0, len(files), batch):
        chunk = files[i:i + batch]
        imgs, meta = [], []
        for f in chunk:
            t, (h, w) = load_rgb(f, size)
            imgs.append(t)
            meta.append({"image_file": f, "image_id": os.path.splitext(os.path.basename(f))[0], "im_size": (h, w)})
        # CropResize with the crop_mode=None the reference hard-wires (pil_transforms.py:102) only resizes: nothing is padded,
        # the padding mask of every sample is all ones (compute_pq crops to its bounding box = the whole image)
        yield {"image": torch.stack(imgs), "mask": torch.ones(len(imgs), size, size, dtype=torch.bool), "meta": meta}


def val_batches(files, size, batch, panoptic_dir, device, seed=1):
    """Batches of the training loader's shape for `process_inputs`: the RGB batch of `batches` plus 'image_semseg' [B,7,S,S] bit
    maps, 'semseg' [B,S,S] int64 labels and the all-ones 'mask'.  The label map is resized like the image (nearest)."""
    from PIL import Image
    from main_ae_eval import IGNORE_LABEL, remap_labels            # (tools/ is the script directory)
    from ldmseg_amd.data.bitcodec import encode_bitmap
    from ldmseg_amd.evaluations import rgb2id
    for i, data in enumerate(batches(files, size, batch, panoptic_dir)):
        labs = []
        for j, m in enumerate(data["meta"]):
            ids = rgb2id(np.asarray(Image.open(os.path.join(panoptic_dir, m["image_id"] + ".png")).convert("RGB")))
            lab = remap_labels(ids, np.random.RandomState(seed + i * batch + j))
            small = Image.fromarray(lab.astype(np.uint8)).resize((size, size), resample=getattr(Image, "Resampling", Image).NEAREST)
            labs.append(torch.from_numpy(np.asarray(small).astype(np.int64)))
        semseg = torch.stack(labs)
        bits, _ = encode_bitmap(semseg.to(device), n=7, fill_value=0.5, ignore_label=IGNORE_LABEL)
        yield dict(data, image_semseg=bits, semseg=semseg, text=[""] * len(labs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", required=True, help="folder of RGB images (e.g. data/examples/coco/rgb_images)")
    ap.add_argument("--panoptic", default=None, help="folder of COCO panoptic PNGs with the same stems (ground truth)")
    ap.add_argument("--ldm", default=None); ap.add_argument("--ae", default=None); ap.add_argument("--vae-image", default=None)
    ap.add_argument("--size", type=int, default=512); ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8); ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--scaling-factor", type=float, default=0.18215)      # tools/scripts/eval.sh:11
    ap.add_argument("--seed", type=int, default=42); ap.add_argument("--count-th", type=int, default=512)
    ap.add_argument("--mask-th", type=float, default=0.5); ap.add_argument("--out", default=None)
    ap.add_argument("--image-descriptors", default="remove", choices=["remove", "clip_image", "clip_image_proj"],
                    help="conditioning of the UNet's cross-attention (base.yaml image_descriptors); remove = no cross-attention")
    ap.add_argument("--clip-vision", default=None,
                    help="torch.save'd state dict of CLIPVisionModel / CLIPVisionModelWithProjection (openai/clip-vit-large-patch14); "
                         "generated weights without it")
    ap.add_argument("--device-pq", action="store_true",
                    help="score PQ on the GPU (PanopticEvaluatorAgnostic.process_device): no map is copied to the host")
    ap.add_argument("--val-loss", action="store_true",
                    help="print the denoising loss per timestep (TrainerDiffusion.validation_loss) instead of PQ; needs --panoptic")
    args = ap.parse_args()
    if args.val_loss and not args.panoptic:
        ap.error("--val-loss needs --panoptic (the ground-truth maps are the loss's targets)")
    if args.val_loss and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--val-loss runs on one process: the per-timestep sums are not reduced across ranks")
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    trainer = build_trainer(args, device)
    files = sorted(glob.glob(os.path.join(args.images, "*.jpg")) + glob.glob(os.path.join(args.images, "*.png")))
    files = files[rank::world]                                              # images sharded over ranks
    from ldmseg_amd.evaluations import PanopticEvaluatorAgnostic, rgb2id
    from ldmseg_amd.evaluations.panoptic_evaluation_agnostic import gt_from_png
    gt_maps = gt_anns = None
    if args.panoptic:
        from PIL import Image
        gt_maps, gt_anns = {}, []
        for f in sorted(glob.glob(os.path.join(args.panoptic, "*.png"))):
            iid = os.path.splitext(os.path.basename(f))[0]
            gt_maps[iid] = rgb2id(np.asarray(Image.open(f).convert("RGB")))
            gt_anns.append(gt_from_png(gt_maps[iid], iid, os.path.basename(f)))
    if args.val_loss:
        out = trainer.validation_loss(val_batches(files, args.size, args.batch, args.panoptic, device), seed=args.seed)
        print(json.dumps(out))                                              # one JSON line (per_timestep keyed by str(t))
    elif gt_anns is None:                                                   # no ground truth: predictions only
        from ldmseg_amd.data.transforms import load_rgb
        res = []
        for data in batches(files, args.size, args.batch, None):
            res += trainer.predict_panoptic(data["image"].to(device), [m["im_size"] for m in data["meta"]], None,
                                            args.steps, seed=args.seed, mask_th=args.mask_th, count_th=args.count_th)
        if rank == 0:
            print(f"{len(res)} images, segments per image: {[len(r['panoptic_seg'][1]) for r in res]}")
    else:
        gloo = dist.new_group(backend="gloo") if world > 1 else None       # object gather side group (detectron2 comm)
        ev = PanopticEvaluatorAgnostic(output_dir=args.out, gt_maps=gt_maps, gt_annotations=gt_anns, group=gloo,
                                       on_device=args.device_pq)
        out = trainer.compute_pq(batches(files, args.size, args.batch, args.panoptic), ev, num_inference_steps=args.steps,
                                 seed=args.seed, threshold_output=True, mask_th=args.mask_th, count_th=args.count_th)
        if rank == 0:
            print(ev.table)
            print(dict(out["panoptic_seg"]))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

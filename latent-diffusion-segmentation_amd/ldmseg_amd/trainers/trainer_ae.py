"""Stage-1 evaluation: how well the segmentation VAE reconstructs ground-truth panoptic maps through its latent.

Stands behind the evaluation half of the reference's ldmseg/trainers/trainers_ae.py::TrainerAE
(`compute_metrics` :546-569, `compute_pq` :580-680, `compute_miou` :728-803) - what `tools/main_ae.py` runs with
`eval_only` (:189-190) - and behind the loss of its training step: `compute_point_loss` (:204-224), the number the stage-1
loop logs and selects checkpoints by, differentiable with respect to the logits and the moments it is given (the `loss.backward()`
of :286-296) and behind the step itself: `training_step` (:285-321 without the fp16 scaler) on the library's forward and backward
with a torch optimiser or the library's fused clip + AdamW (ldmseg_amd/optim.py), and `save` / `resume` in the reference's model.pt
layout (:491-530).  The loop around it (tools/main_ae_train.py is a plain one), EMA, gradient accumulation, image dumps and overlays
(`save_images`) are not built.

Per batch ONE library call does encode -> posterior mode -> decode -> the metric's tail
(`GeneralVAESeg.reconstruct_semseg` / `reconstruct_panoptic`); the [B,128,S,S] logits are never materialised and the
mIoU loop does not synchronise with the host until the score is read.
"""
from typing import List, Optional, Union

import torch

from ..evaluations.semseg_evaluation import SemsegMeter
from .losses import SegmentationLosses
from .sampler import TrainerDiffusion

METRICS = ("miou", "pq")
LOSS_WEIGHTS = {"mask": 1.0, "ce": 1.0, "kl": 0.0}                                     # base.yaml:101-104
LOSS_KWARGS = dict(num_points=12544, oversample_ratio=3, importance_sample_ratio=0.75, cost_mask=1.0, cost_class=1.0,
                   temperature=1.0)                                                    # base.yaml:107-113


class TrainerAE(object):
    def __init__(self, vae_model, num_classes: int = 128, ignore_label: int = 0, mask_th: float = 0.5, count_th: int = 512,
                 overlap_th: float = 0.5, class_names: Optional[List[str]] = None, device=None,
                 loss_weights: Optional[dict] = None, loss_kwargs: Optional[dict] = None):
        self.vae_model = vae_model
        self.num_classes = num_classes
        self.ignore_label = ignore_label
        self.mask_th = mask_th
        self.count_th = count_th
        self.overlap_th = overlap_th
        self.class_names = class_names if class_names is not None else [str(i) for i in range(num_classes)]
        self.device = torch.device(device) if device is not None else getattr(vae_model, "device", None)
        self.loss_weights = dict(LOSS_WEIGHTS if loss_weights is None else loss_weights)
        self.last_grad_norm = None                                  # training_step with the library's AdamW and clip_grad > 0
        # :195; the trainer's ignore_label is the one that counts (an 'ignore_label' among loss_kwargs is overridden)
        self.segmentation_losses = SegmentationLosses(**{**(LOSS_KWARGS if loss_kwargs is None else loss_kwargs),
                                                         'ignore_label': ignore_label})

    def compute_metrics(self, names: Union[List[str], str] = ['miou'], dataloader=None, evaluator=None,
                        threshold_output: bool = False) -> dict:
        """:546-569.  `dataloader`: an iterable of batches that can be walked once per metric (a list, a DataLoader) or a
        callable returning one.  Returns {name: result}."""
        if isinstance(names, str):
            names = [names]
        elif not isinstance(names, list):
            raise TypeError(f"names must be a metric name or a list of them, got {type(names).__name__}")
        unknown = [n for n in names if n.lower() not in METRICS]
        if unknown:
            raise NotImplementedError(f'Unknown metric {unknown[0]}')
        out = {}
        for name in names:
            dl = dataloader() if callable(dataloader) else dataloader
            if name.lower() == 'miou':
                out[name] = self.compute_miou(dl, threshold_output=threshold_output)
            else:
                out[name] = self.compute_pq(dl, evaluator, threshold_output=threshold_output)
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                dist.barrier()
        return out

    crop_padding = staticmethod(TrainerDiffusion.crop_padding)          # :571-577

    def compute_point_loss(self, outputs, targets, do_matching: bool = False, masks=None, generator=None):
        """:204-216 on the VAEOutput of `vae_model(...)` (`.sample` logits [B,C,4L,4L], `.posterior`) and targets [B,h,w]:
        (total, ce, kl, mask) as 0-d device tensors; total is the three terms weighted by `loss_weights`, added in the order
        ce, mask, kl.  With grad mode on, the values are differentiable with respect to the logits and the posterior's moments
        where those require grad (`total.backward()`).  The library's own seg-VAE gives `.sample` the decoder's graph once
        `vae_model.decoder_parameters()` has been called (fp32 / bf16x3 objects): `total.backward()` then fills the `.grad` of every
        decoder parameter through ldmseg_point_loss_backward and ldmseg_vae_decode_backward; once `vae_model.encoder_parameters()`
        has been called too, the moments carry the encoder's graph and the `.grad` of every encoder parameter is filled as well
        (ldmseg_vae_posterior_backward, ldmseg_gaussian_kl_backward, ldmseg_vae_encode_backward)."""
        parts = self.segmentation_losses.point_loss(outputs.sample, targets, do_matching, masks, generator=generator)
        ce, mask = parts['ce'], parts['mask']
        kl = outputs.posterior.kl(return_mean=True)[1]
        w = self.loss_weights
        total = w['ce'] * ce + w['mask'] * mask + w['kl'] * kl
        return total, ce, kl, mask

    def training_step(self, images, targets, optimizer, clip_grad: float = 0.0, generator=None, point_generator=None, lr=None):
        """One stage-1 step, :285-321 without the fp16 scaler, on `images` [B,7,S,S] already in [-1, 1] (:256) and `targets` [B,h,w]:
        forward with a sampled posterior, `compute_point_loss`, `backward()`, torch's `clip_grad_norm_` over `vae_model.parameters()`
        when clip_grad > 0, `optimizer.step()`, `vae_model.refresh()`.  `optimizer` is a torch optimiser over
        `vae_model.parameters()`; its gradients are zeroed first (:324-325, moved to the front).  generator: the DEVICE generator
        of the posterior's noise; point_generator: the point sampler's (as `compute_point_loss` takes it).  Returns (loss, ce, kl, mask) as detached 0-d
        device tensors.
        With the library's own `ldmseg_amd.optim.AdamW` as `optimizer`, clipping and update are its one `step(max_norm=clip_grad)`
        (one ldmseg_adamw_step call); the norm before clipping, a 0-d device tensor, is kept in `self.last_grad_norm` (None without
        clipping).  lr: when given, written to every param group first (:305-307, the schedule's entry of this step)."""
        from ..optim import AdamW
        if lr is not None:
            for group in optimizer.param_groups:
                group["lr"] = float(lr)
        if isinstance(optimizer, AdamW):
            optimizer.zero_grad(set_to_none=True)
            with torch.enable_grad():
                output = self.vae_model(images, sample_posterior=True, generator=generator)
                loss, ce, kl, mask = self.compute_point_loss(output, targets, generator=point_generator)
                loss.backward()
            self.last_grad_norm = optimizer.step(max_norm=clip_grad)
            self.vae_model.refresh()
            return loss.detach(), ce.detach(), kl.detach(), mask.detach()
        optimizer.zero_grad(set_to_none=True)
        params = self.vae_model.parameters()
        with torch.enable_grad():
            output = self.vae_model(images, sample_posterior=True, generator=generator)
            loss, ce, kl, mask = self.compute_point_loss(output, targets, generator=point_generator)
            loss.backward()
        if clip_grad > 0:
            torch.nn.utils.clip_grad_norm_(params, clip_grad, norm_type=2)
        optimizer.step()
        self.vae_model.refresh()
        return loss.detach(), ce.detach(), kl.detach(), mask.detach()

    def save(self, path, optimizer=None, epoch: int = 0, step: int = 0, p: Optional[dict] = None) -> None:
        """:491-505: writes the reference's model.pt layout {'step', 'epoch', 'vae', 'opt', 'p', 'scaler': None} - 'vae' the
        seg-VAE's `state_dict()`, 'opt' the optimiser's (torch's AdamW layout with CPU tensors; None without an optimiser), 'p' the
        run's configuration dict.  Tensors and plain containers only: `checkpoint.load_ae_checkpoint(path)` and every
        `weights_only=True` reader take the file."""
        opt = None
        if optimizer is not None:
            opt = optimizer.state_dict()
            opt = {"state": {i: {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
                             for i, s in opt["state"].items()},
                   "param_groups": opt["param_groups"]}
        data = {"step": int(step), "epoch": int(epoch), "vae": self.vae_model.state_dict(), "opt": opt,
                "p": dict(p) if p is not None else {}, "scaler": None}
        torch.save(data, path)

    def resume(self, path, optimizer=None):
        """:507-530: reads a file `save` (or the reference's trainer) wrote: the seg-VAE's tensors into `vae_model`
        (`load_state_dict`: the handle computes with them), the 'opt' entry - if there is one and an optimiser is given - into
        `optimizer`.  Returns (epoch, step) as saved."""
        from ..checkpoint import _load, vae_state_from
        data = _load(path)
        self.vae_model.load_state_dict(vae_state_from(data))
        if optimizer is not None and data.get("opt") is not None:
            optimizer.load_state_dict(data["opt"])
        return int(data.get("epoch", 0)), int(data.get("step", 0))

    @torch.no_grad()
    def validation_loss(self, dataloader, sample_posterior: bool = False, seed: int = 0) -> dict:
        """The stage-1 loss of a checkpoint over a loader.  NOT in the reference (its loss is only ever logged from inside the
        training loop): per batch {'image_semseg': [B,7,S,S] bit maps in [0,1], 'semseg': [B,h,w]} the forward of :253-287
        without corruption, then `compute_point_loss`; every draw comes from one CPU generator seeded `seed`.  The four values
        are averaged over batches (image-weighted) on the device and read once at the end (each batch's `point_loss` reads its
        class-presence table): {'loss', 'ce', 'kl', 'mask', 'images'}."""
        g = torch.Generator().manual_seed(int(seed))
        gd = torch.Generator(device=self.device).manual_seed(int(seed)) if sample_posterior else None
        sums = torch.zeros(4, dtype=torch.float64, device=self.device)
        images = 0
        for data in dataloader:
            x = data['image_semseg'].to(self.device, non_blocking=True)
            targets = data['semseg'].to(self.device, non_blocking=True)
            out = self.vae_model(2. * x - 1., sample_posterior=sample_posterior, generator=gd)
            sums += torch.stack(self.compute_point_loss(out, targets, generator=g)).double() * x.shape[0]
            images += x.shape[0]
        if images == 0:
            raise ValueError("validation_loss: the loader gave no batch")
        total, ce, kl, mask = (sums / images).cpu().tolist()
        return {'loss': total, 'ce': ce, 'kl': kl, 'mask': mask, 'images': images}

    @torch.no_grad()
    def compute_miou(self, dataloader, threshold_output: bool = False) -> dict:
        """:728-803 over batches {'image_semseg': [B,7,S,S] bit maps in [0,1], 'semseg': [B,h,w] int64 targets}.  Like the
        reference, an approximation: predictions are compared at the targets' size, not at the original image size."""
        meter = SemsegMeter(self.num_classes, self.class_names, has_bg=False, ignore_index=self.ignore_label,
                            gpu_idx=self.device)
        for data in dataloader:
            images = data['image_semseg'].to(self.device, non_blocking=True)
            targets = data['semseg'].to(self.device, non_blocking=True)
            # 2 * images - 1 (:747) rides on the encoder's input pack; the tail adds this batch's counters on the device
            self.vae_model.reconstruct_semseg(images, targets.shape[-2:], targets, meter.device_counts(self.device),
                                              in_mul=2.0, in_add=-1.0, mask_th=self.mask_th if threshold_output else None,
                                              ignore_label=self.ignore_label, ignore_index=self.ignore_label,
                                              return_preds=False)
        meter.synchronize_between_processes()                            # :799
        return meter.return_score(verbose=False, name='val set')

    @torch.no_grad()
    def predict_panoptic(self, images: torch.Tensor, im_sizes, padding_masks: Optional[torch.Tensor] = None,
                         threshold_output: bool = True, return_stats: bool = False, packed: bool = False):
        """One batch of `compute_pq` (:604-668): bit maps [B,7,S,S] in [0,1] on the GPU -> `processed_results`; with
        `packed=True` the device form of `GeneralVAESeg.reconstruct_panoptic` (nothing is copied to the host)."""
        sizes = [(int(s[0]), int(s[1])) for s in im_sizes]
        boxes = TrainerDiffusion.padding_boxes(padding_masks) if padding_masks is not None else None
        res = self.vae_model.reconstruct_panoptic(
            images, (images.shape[-2], images.shape[-1]), sizes, boxes, in_mul=2.0, in_add=-1.0,
            threshold_output=threshold_output, mask_th=self.mask_th, count_th=self.count_th, overlap_th=self.overlap_th,
            ignore_label=self.ignore_label, return_stats=return_stats, packed=packed)
        if packed:
            return res
        outs, stats = res if return_stats else (res, None)
        processed = [{"panoptic_seg": (pan, [{"id": int(c) + 1, "category_id": 1, "isthing": True} for c in kept])}
                     for pan, kept in outs]
        return (processed, stats) if return_stats else processed

    @torch.no_grad()
    def compute_pq(self, dataloader, evaluator, threshold_output: bool = True):
        """:580-680 over batches {'image_semseg': [B,7,S,S], 'mask': [B,S,S] padding masks or None, 'meta': [{'image_file',
        'image_id', 'im_size': (h, w)}, ...]}.  `evaluator` is a PanopticEvaluatorAgnostic; all ranks must call this (the
        evaluator gathers).  Returns evaluator.evaluate() (rank 0) / None.  An evaluator built with `on_device=True` is fed
        through `process_device`: the maps and the keep table stay on the GPU (a batch may bring its ground truth as
        'panoptic_gt', one RGB or id map per image)."""
        if evaluator is None:
            raise ValueError("compute_pq needs a PanopticEvaluatorAgnostic")
        evaluator.reset()
        for data in dataloader:
            meta = data['meta']
            images = data['image_semseg'].to(self.device, non_blocking=True)
            masks = data.get('mask')
            masks = masks.to(self.device) if masks is not None else None
            if getattr(evaluator, "on_device", False):
                out = self.predict_panoptic(images, [x['im_size'] for x in meta], masks, threshold_output, packed=True)
                evaluator.process_device([x['image_file'] for x in meta], [x['image_id'] for x in meta], out,
                                         gt_maps=data.get('panoptic_gt'))
                continue
            processed = self.predict_panoptic(images, [x['im_size'] for x in meta], masks, threshold_output)
            evaluator.process([x['image_file'] for x in meta], [x['image_id'] for x in meta], processed)
        return evaluator.evaluate()

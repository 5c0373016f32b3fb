"""Semantic-segmentation meter with the reference's call surface, counted on the MI355X.

Stands behind the reference's ldmseg/evaluations/semseg_evaluation.py::SemsegMeter.  The reference's `update` runs
3 x num_classes masked reductions, each ended by an `.item()`; here one launch (`ldmseg_semseg_meter_update`, or the fused
tails `GeneralVAESeg.decode_semseg` / `reconstruct_semseg`) adds into an int64 [3][K] accumulator that stays on the device.
The accumulator is folded into host totals only by `return_score` / `synchronize_between_processes`.

The host arithmetic (`semseg_scores`, `add_counts`, the all-reduce) needs no GPU.
"""
import numpy as np
import torch

from .. import _lib

MAX_CLASSES = 256      # the kernels keep [3][K] counters in LDS


def semseg_scores(tp, fp, fn) -> dict:
    """semseg_evaluation.py:41-47: per-class Jaccard tp / max(tp + fp + fn, 1e-8) and its mean over ALL classes
    (a class absent from predictions and targets counts as 0)."""
    tp, fp, fn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn))
    jac = [float(t) / max(float(t + p + n), 1e-8) for t, p, n in zip(tp, fp, fn)]
    return {'jaccards_all_categs': jac, 'mIoU': np.mean(jac)}


class SemsegMeter(object):
    def __init__(self, num_classes, class_names, has_bg=True, ignore_index=255, gpu_idx='cuda'):
        self.num_classes = num_classes + (1 if has_bg else 0)
        self.class_names = class_names
        self.ignore_index = ignore_index
        self.gpu_idx = gpu_idx
        self._dev = None          # int64 [3][K] (tp | fp | fn) on the GPU
        self._dirty = False       # the device accumulator may hold counts the host totals lack
        self.reset()

    def reset(self):
        self.tp = np.zeros(self.num_classes, dtype=np.int64)
        self.fp = np.zeros(self.num_classes, dtype=np.int64)
        self.fn = np.zeros(self.num_classes, dtype=np.int64)
        if self._dev is not None:
            self._dev.zero_()
        self._dirty = False

    # ------------------------------------------------------------------ device side
    def device_counts(self, device) -> torch.Tensor:
        """The int64 [3][K] accumulator on `device` (created on first use); a fused tail that is handed this tensor adds to it."""
        if self.num_classes > MAX_CLASSES:
            raise ValueError(f"the device meter supports at most {MAX_CLASSES} classes (got {self.num_classes})")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("SemsegMeter counts on the MI355X (no CPU fallback)")
        if self._dev is None:
            self._dev = torch.zeros(3, self.num_classes, dtype=torch.int64, device=device)
        elif self._dev.device != device and device.index is not None:
            raise RuntimeError(f"meter accumulator lives on {self._dev.device}, got tensors on {device}")
        # fetching it marks it as holding counts the host totals lack: the caller adds to it through launches the meter does not
        # see, and a forgotten mark would lose counts silently, while a fold of zeros costs one small copy
        self._dirty = True
        return self._dev

    @torch.no_grad()
    def update(self, pred, gt):
        for name, t in (("pred", pred), ("gt", gt)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{name} must be a tensor on the MI355X: SemsegMeter.update has no CPU fallback")
        if pred.numel() != gt.numel():
            raise ValueError(f"pred has {pred.numel()} elements, gt {gt.numel()}")
        counts = self.device_counts(pred.device)
        p = pred.to(torch.int64).contiguous()
        g = gt.to(device=pred.device, dtype=torch.int64).contiguous()
        with torch.cuda.device(pred.device):
            _lib.check(_lib.lib().ldmseg_semseg_meter_update(_lib.ptr(p), _lib.ptr(g), p.numel(), self.num_classes,
                                                             int(self.ignore_index), _lib.ptr(counts),
                                                             _lib.stream_ptr(pred.device)), "ldmseg_semseg_meter_update")

    def fold_device_counts(self):
        """The ONE device-to-host copy: adds the device accumulator to the host totals and clears it."""
        c = self._dev.cpu().numpy().copy()
        self._dev.zero_()
        self._dirty = False
        self.add_counts(c[0], c[1], c[2])

    # ------------------------------------------------------------------ host side
    def add_counts(self, tp, fp, fn):
        for mine, theirs in ((self.tp, tp), (self.fp, fp), (self.fn, fn)):
            a = np.asarray(theirs, dtype=np.int64)
            if a.shape != mine.shape:
                raise ValueError(f"expected {mine.shape[0]} counters, got shape {a.shape}")
            mine += a

    def return_score(self, verbose=True, name='dataset', suppress_prints=False):
        """{'jaccards_all_categs', 'mIoU'} of everything counted so far.  Prints the summary (two lines) unless
        `suppress_prints` is set and `verbose` is not; `verbose` adds one line per class."""
        if self._dirty:
            self.fold_device_counts()
        result = semseg_scores(self.tp, self.fp, self.fn)
        lines = []
        if verbose or not suppress_prints:
            lines += ['Evaluation for semantic segmentation - ' + str(name), 'mIoU is {:.2f}'.format(100 * result['mIoU'])]
        if verbose:
            lines += ['IoU class {} is {:.2f}'.format(cls, 100 * j)
                      for cls, j in zip(self.class_names, result['jaccards_all_categs'])]
        if lines:
            print("\n".join(lines))
        return result

    def synchronize_between_processes(self):
        """All-reduce (sum) of the host totals over the default process group; nothing when torch.distributed is not initialised."""
        import torch.distributed as dist
        if self._dirty:
            self.fold_device_counts()
        if not (dist.is_available() and dist.is_initialized()):
            return
        on_gpu = dist.get_backend() == "nccl"
        t = torch.from_numpy(np.stack([self.tp, self.fp, self.fn]))
        if on_gpu:
            t = t.to(self.gpu_idx)
        dist.barrier()
        dist.all_reduce(t)
        t = t.cpu().numpy()
        self.tp, self.fp, self.fn = t[0].copy(), t[1].copy(), t[2].copy()

    def __str__(self):
        score = self.return_score(verbose=False, suppress_prints=True)
        return 'IoU ({:.2f})'.format(100 * score['mIoU'])

"""Per-iteration learning-rate tables of the training loops, restated from the reference's ldmseg/utils/utils.py:84-157
(`cosine_scheduler`, `warmup_scheduler`, `step_scheduler`): same signatures, the same float64 arrays to the bit
(tests/test_lr_schedules_cpu.py compares with arrays the reference's functions returned).  The loop writes entry `step` into every
param group before the update (`TrainerAE.training_step(..., lr=schedule[step])`).

Every table has epochs * niter_per_ep entries: a linear ramp np.linspace(start_warmup_value, base_value, warmup_iters) - its last
entry IS base_value - followed by the schedule proper, which starts again at base_value."""
from typing import Optional

import numpy as np


def _ramp_and_rest(base_value, epochs, niter_per_ep, start_warmup_value, warmup_iters):
    """(the warm-up entries, how many entries follow them)"""
    w = 0 if warmup_iters is None else warmup_iters
    ramp = np.linspace(start_warmup_value, base_value, w) if w > 0 else np.array([])
    return ramp, epochs * niter_per_ep - w


def _joined(ramp, rest, epochs, niter_per_ep):
    out = np.concatenate((ramp, rest))
    if len(out) != epochs * niter_per_ep:
        raise ValueError(f"warm-up of {len(ramp)} iterations does not fit {epochs} x {niter_per_ep} iterations")
    return out


def cosine_scheduler(base_value: float, final_value: float, epochs: int, niter_per_ep: int, start_warmup_value: int = 0,
                     warmup_iters: Optional[int] = None) -> np.ndarray:
    """Half a cosine from base_value down to final_value over the iterations behind the warm-up."""
    ramp, n = _ramp_and_rest(base_value, epochs, niter_per_ep, start_warmup_value, warmup_iters)
    it = np.arange(n)
    rest = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * it / len(it)))
    return _joined(ramp, rest, epochs, niter_per_ep)


def warmup_scheduler(base_value: float, final_value: float, epochs: int, niter_per_ep: int, start_warmup_value: int = 0,
                     warmup_iters: Optional[int] = None) -> np.ndarray:
    """Constant base_value behind the warm-up (final_value is not used: the reference's signature)."""
    ramp, n = _ramp_and_rest(base_value, epochs, niter_per_ep, start_warmup_value, warmup_iters)
    return _joined(ramp, np.ones(n) * base_value, epochs, niter_per_ep)


def step_scheduler(base_value: float, final_value: float, epochs: int, niter_per_ep: int, decay_epochs: list = [20, 40],
                   decay_rate: float = 0.1, start_warmup_value: int = 0, warmup_iters: Optional[int] = None) -> np.ndarray:
    """base_value behind the warm-up, multiplied by decay_rate from every epoch of decay_epochs on (final_value is not used)."""
    if not isinstance(decay_epochs, list):
        raise TypeError("decay_epochs must be a list")
    ramp, n = _ramp_and_rest(base_value, epochs, niter_per_ep, start_warmup_value, warmup_iters)
    w = len(ramp)
    rest = np.ones(n) * base_value
    for e in decay_epochs:
        rest[int(e * niter_per_ep - w):] *= decay_rate
    return _joined(ramp, rest, epochs, niter_per_ep)

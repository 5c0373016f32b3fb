"""Cases and references of the fused clip + AdamW tests (tests/test_optim_gpu.py, tests/test_ae_training_gpu.py).

Reference: torch.optim.AdamW (single-tensor path) + torch.nn.utils.clip_grad_norm_ on float64 CPU copies.  Yardstick: the same pair
on float32 CPU copies - another fp32 evaluation of the same formula, in another operation order.  The metric, per tensor:
    parameters   max|p - p64| / max|p64 - p_initial|        (the error relative to the distance moved)
    moments      max|m - m64| / max|m64|
and the library's worst value over tensors, quantities and steps has to stay within max(2 x the yardstick's worst, 1e-6).
Every run is computed once per process and shared."""
import functools
import math

import torch

CHUNK = 8192                    # csrc/optim.hip: kChunk
PER_LAUNCH = 48                 # include/ldmseg_hip.h: LDMSEG_MULTI_TENSOR_PER_LAUNCH
STEPS = 5
SCALES = (1.0, 1e-2, 1e-6, 1e-1, 1e-4)          # gradient scale of each step
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)

# numels: the list.  none: the tensor without a gradient.  views: tensor -> which of parameter / gradient / the two moments ('pgmv')
# start one element into their storage (4-byte alignment only).  groups: [(first, last + 1, overrides)].  lr_change: (step, lr) written
# into group 0 before that step.
CASES = {
    # a vector tail, chunk edges +- 1, one real layer size (36864 = 64 * 64 * 9), an empty tensor, a skipped one in the middle; tensor
    # 5: parameter and gradient off the 16-byte grid, the moments on it (no common phase: scalar chunk); tensor 7: all four off it
    # by the same element (scalar head of three, vector body); tensor 10: the gradient alone
    "shapes": dict(numels=[1, 3, 8, 31, 257, 4097, 2016, 36864, CHUNK - 1, CHUNK, CHUNK + 1, 0, 5], none=6,
                   views={5: "pg", 7: "pgmv", 10: "g"}),
    # more than one launch's table (5 launches per pass, the partials added by the finish launch), a skipped tensor in the third
    "many": dict(numels=[1 + (7 * i) % 61 for i in range(200)], none=100),
    "single": dict(numels=[1000]),
    "groups": dict(numels=[300, 5000, 17], groups=[(0, 2, dict(lr=1e-3, weight_decay=0.01)), (2, 3, dict(lr=5e-3, weight_decay=0.0))],
                   lr_change=(3, 2.5e-3)),
}


def initial(case):
    g = torch.Generator().manual_seed(sorted(CASES).index(case))
    return [torch.randn(n, generator=g) for n in CASES[case]["numels"]]


def grads(case, step):
    g = torch.Generator().manual_seed(1000 + 10 * sorted(CASES).index(case) + step)
    none = CASES[case].get("none")
    return [None if i == none else torch.randn(n, generator=g) * SCALES[step] for i, n in enumerate(CASES[case]["numels"])]


def true_norm(gs):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs if g is not None))


def max_norm(case, step, above=False):
    """half the step's true norm, so that every step clips; `above`: twice the norm, coef = 1"""
    return (2.0 if above else 0.5) * true_norm(grads(case, step))


def param_groups(case, ps):
    spec = CASES[case].get("groups")
    if spec is None:
        return [{"params": list(ps)}]
    return [dict(over, params=list(ps[a:b])) for a, b, over in spec]


def apply_lr_change(case, step, opt):
    ch = CASES[case].get("lr_change")
    if ch is not None and ch[0] == step:
        opt.param_groups[0]["lr"] = ch[1]


def snapshot(ps, state_of, total):
    """CPU copies: parameters, gradients as the step left them, moments (None where the tensor has no state), the returned norm"""
    cp = lambda t: None if t is None else t.detach().cpu().clone()
    sts = [state_of(p) for p in ps]
    return dict(p=[cp(p) for p in ps], g=[cp(p.grad) for p in ps], m=[cp(s["exp_avg"]) if s else None for s in sts],
                v=[cp(s["exp_avg_sq"]) if s else None for s in sts], total=None if total is None else cp(total))


@functools.lru_cache(maxsize=None)
def torch_run(case, dtype, above=False):
    """STEPS snapshots of clip_grad_norm_ + torch.optim.AdamW on CPU copies of the case in `dtype` ('float64' / 'float32')"""
    dt = getattr(torch, dtype)
    ps = [t.to(dt).clone().requires_grad_(True) for t in initial(case)]
    opt = torch.optim.AdamW(param_groups(case, ps), foreach=False, **HYPER)
    out = []
    for step in range(STEPS):
        for p, g in zip(ps, grads(case, step)):
            p.grad = None if g is None else g.to(dt).clone()
        apply_lr_change(case, step, opt)
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm(case, step, above), foreach=False)
        opt.step()
        out.append(snapshot(ps, lambda p: opt.state.get(p), total))
    return out


def rel(a, ref, scale):
    """max|a - ref| / max|scale| in fp64"""
    return float((a.double() - ref.double()).abs().max() / scale.double().abs().max())


def worst(case, run, run64, init=None):
    """the metric of the module docstring over every step, tensor (with a gradient, not empty) and quantity -> (value, where)"""
    init = initial(case) if init is None else init
    none = CASES[case].get("none") if case in CASES else None
    w, where = 0.0, None
    for step, (a, r) in enumerate(zip(run, run64)):
        for i, p0 in enumerate(init):
            if i == none or p0.numel() == 0:
                continue
            vals = {"p": rel(a["p"][i], r["p"][i], r["p"][i].double() - p0.double()), "m": rel(a["m"][i], r["m"][i], r["m"][i]),
                    "v": rel(a["v"][i], r["v"][i], r["v"][i])}
            for k, x in vals.items():
                if not x <= w:                       # (a NaN is the worst value)
                    w, where = x, (step, i, k)
    return w, where


def clip_coef(total, mn):
    """min(1, max_norm / (total + 1e-6)) in fp32, from the norm a call returned (a 0-d fp32 tensor)"""
    t = total.detach().cpu().float()
    return torch.clamp(torch.tensor(mn, dtype=torch.float32) / (t + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)

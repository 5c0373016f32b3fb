"""The fused clip + AdamW of csrc/optim.hip (ldmseg_adamw_step / ldmseg_grad_clip / ldmseg_grad_norm) and its Python surface
(ldmseg_amd/optim.py) against torch.optim.AdamW + clip_grad_norm_ in float64 on the CPU, with the same pair in float32 as the
yardstick (tests/optim_ref.py states the cases, the metric and the bound)."""
import ctypes as C
import functools
import math
import types

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _place(t, off):
    """a device copy of t; `off`: as a view that starts one element into its storage (4-byte aligned only)"""
    if not off:
        return t.to(DEV).contiguous()
    out = torch.empty(t.numel() + 1, device=DEV)[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    out.copy_(t)
    return out


def build(case):
    """(parameters on the device, the library optimiser over them); the tensor without a gradient gets moments and a step count of its
    own, which no step may touch"""
    from ldmseg_amd.optim import AdamW
    views = R.CASES[case].get("views", {})
    ps = [_place(t, "p" in views.get(i, "")).requires_grad_(True) for i, t in enumerate(R.initial(case))]
    opt = AdamW(R.param_groups(case, ps), **R.HYPER)
    for i, how in views.items():
        if "m" in how or "v" in how:
            z = torch.zeros(ps[i].numel())
            opt.state[ps[i]] = {"step": 0, "exp_avg": _place(z, "m" in how), "exp_avg_sq": _place(z, "v" in how)}
    none = R.CASES[case].get("none")
    if none is not None:
        g = torch.Generator().manual_seed(77)
        opt.state[ps[none]] = {"step": 7, "exp_avg": torch.randn(ps[none].numel(), generator=g).to(DEV),
                               "exp_avg_sq": torch.rand(ps[none].numel(), generator=g).to(DEV)}
    return ps, opt


def set_grads(case, step, ps):
    views = R.CASES[case].get("views", {})
    for i, (p, g) in enumerate(zip(ps, R.grads(case, step))):
        p.grad = None if g is None else _place(g, "g" in views.get(i, ""))


def lib_steps(case, above=False):
    ps, opt = build(case)
    out = []
    for step in range(R.STEPS):
        set_grads(case, step, ps)
        R.apply_lr_change(case, step, opt)
        total = opt.step(max_norm=R.max_norm(case, step, above))
        out.append(R.snapshot(ps, lambda p: opt.state.get(p), total))
    return out, ps, opt


@functools.lru_cache(maxsize=None)
def lib_run(case, above=False):
    return lib_steps(case, above)[0]


def check_against_reference(case, above):
    got, r64, r32 = lib_run(case, above), R.torch_run(case, "float64", above), R.torch_run(case, "float32", above)
    w_lib, at_lib = R.worst(case, got, r64)
    w_32, at_32 = R.worst(case, r32, r64)
    print(f"{case} above={above}: library worst {w_lib:.3e} at (step, tensor, quantity) {at_lib}; fp32 CPU yardstick {w_32:.3e} at {at_32}")
    assert w_lib <= max(2.0 * w_32, 1e-6), (w_lib, at_lib, w_32)
    none = R.CASES[case].get("none")
    for step, (a, r) in enumerate(zip(got, r64)):
        want = float(r["total"])
        assert abs(float(a["total"]) - want) <= 1e-6 * want, (step, float(a["total"]), want)       # fp64 sum, one rounding to fp32
        assert abs(want - R.true_norm(R.grads(case, step))) <= 1e-12 * want
        coef = R.clip_coef(a["total"], R.max_norm(case, step, above))
        assert (float(coef) == 1.0) == above
        for i, g in enumerate(R.grads(case, step)):
            if i == none:
                assert a["g"][i] is None
            else:
                assert torch.equal(a["g"][i], g * coef), (step, i)       # .grad is what clip_grad_norm_ leaves: g * coef, one fp32 product


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_five_clipped_steps_stay_within_twice_the_fp32_yardstick(case):
    check_against_reference(case, False)


def test_max_norm_above_the_norm_leaves_the_gradients_bitwise():
    check_against_reference("shapes", True)                              # coef == 1: g * 1.0f, the same bits


@pytest.mark.parametrize("case", ["shapes", "many"])
def test_skipped_tensor_is_untouched(case):
    _, ps, opt = lib_steps(case)
    none = R.CASES[case]["none"]
    g = torch.Generator().manual_seed(77)
    st = opt.state[ps[none]]
    assert torch.equal(ps[none].detach().cpu(), R.initial(case)[none])
    assert torch.equal(st["exp_avg"].cpu(), torch.randn(ps[none].numel(), generator=g))
    assert torch.equal(st["exp_avg_sq"].cpu(), torch.rand(ps[none].numel(), generator=g))
    assert st["step"] == 7 and opt.state[ps[0]]["step"] == R.STEPS       # its step is not counted either
    # the empty tensor has a state and a count, and nothing else happened to it
    if 0 in R.CASES[case]["numels"]:
        e = R.CASES[case]["numels"].index(0)
        assert opt.state[ps[e]]["step"] == R.STEPS and opt.state[ps[e]]["exp_avg"].numel() == 0


def test_the_same_steps_twice_give_the_same_bits():
    for case in ("shapes", "many"):
        a, b = lib_run(case), lib_steps(case)[0]
        for sa, sb in zip(a, b):
            assert torch.equal(sa["total"], sb["total"])
            for k in "pgmv":
                assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(sa[k], sb[k])), (case, k)


@pytest.mark.parametrize("case", ["shapes", "many", "single"])
def test_norm_and_clip_alone_return_the_fused_steps_norm_bits(case):
    from ldmseg_amd.optim import clip_grad_norm_, grad_norm
    ps, opt = build(case)
    set_grads(case, 0, ps)
    mn = R.max_norm(case, 0)
    fused = lib_run(case)[0]
    n0 = grad_norm(ps)
    assert n0.is_cuda and n0.dim() == 0 and torch.equal(n0.cpu(), fused["total"])
    versions = [p.grad._version for p in ps if p.grad is not None]
    n1 = clip_grad_norm_(ps, mn)
    assert torch.equal(n1.cpu(), fused["total"])
    assert all(p.grad._version > v for p, v in zip([p for p in ps if p.grad is not None], versions))
    for i, p in enumerate(ps):
        assert (p.grad is None and fused["g"][i] is None) or torch.equal(p.grad.cpu(), fused["g"][i]), i
    # clipped once, the norm is max_norm (up to the 1e-6 of the coefficient and fp32 products); a step without clipping returns None and
    # leaves the gradients alone
    assert abs(float(grad_norm(ps)) - mn) <= 1e-5 * mn
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    p0 = [p.detach().clone() for p in ps]
    assert opt.step() is None and opt.step(max_norm=0.0) is None
    assert all((a is None and p.grad is None) or torch.equal(a, p.grad) for a, p in zip(before, ps))
    assert all(p.grad is None or p.numel() == 0 or not torch.equal(a, p.detach()) for a, p in zip(p0, ps))


def test_changed_lr_is_honoured_at_the_next_step():
    """two optimisers in the same state; one gets another lr written into its group, as the reference's loop does every iteration"""
    outs = []
    for lr in (None, 3e-3):
        ps, opt = build("single")
        set_grads("single", 0, ps)
        opt.step(max_norm=1.0)
        set_grads("single", 1, ps)
        if lr is not None:
            opt.param_groups[0]["lr"] = lr
        opt.step(max_norm=1.0)
        outs.append((ps[0].detach().cpu(), opt.state[ps[0]]["exp_avg"].cpu()))
    assert not torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # lr moves the parameter, not the moments


def _call_step(lib, ps, gs, ms, vs, numels, hyper, max_norm=0.0, total=None, scratch=None):
    from ldmseg_amd import _lib
    n = len(hyper) if numels is None else len(numels)
    arr = lambda ts: None if ts is None else (C.c_void_p * n)(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])
    return lib.ldmseg_adamw_step(n, arr(ps), arr(gs), arr(ms), arr(vs), None if numels is None else (C.c_int64 * n)(*numels),
                                 None if hyper is None else (_lib.AdamWHyper * n)(*hyper), max_norm, _lib.ptr(total), _lib.ptr(scratch), None)


def test_bad_arguments_return_e_arg_and_launch_nothing():
    from ldmseg_amd import _lib
    lib = _lib.lib()
    E_ARG = -1
    n = 2
    t = [[torch.full((10,), float(k + 1), device=DEV) for _ in range(n)] for k in range(4)]      # p, g, m, v
    numels = [10, 10]
    ok = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    total, scratch = torch.zeros((), device=DEV), torch.zeros(64, dtype=torch.uint8, device=DEV)
    bad = [
        dict(ps=None), dict(gs=None), dict(ms=None), dict(vs=None), dict(numels_none=True), dict(hyper_none=True),      # null arrays
        dict(numels=[10, -1]),                                                                                           # negative numel
        dict(hyper=[ok, (1e-3, 0.9, 0.999, 1e-8, 0.01, 0)]),                                                             # step < 1
        dict(hyper=[ok, (1e-3, 1.0, 0.999, 1e-8, 0.01, 1)]), dict(hyper=[(1e-3, 0.9, -0.1, 1e-8, 0.01, 1), ok]),         # betas
        dict(hyper=[ok, (1e-3, 0.9, float("nan"), 1e-8, 0.01, 1)]),
        dict(ps=[t[0][0], t[0][1].data_ptr() + 2]), dict(gs=[t[1][0].data_ptr() + 1, t[1][1]]),                          # misaligned
        dict(vs=[t[3][0], t[3][1].data_ptr() + 3]),
        dict(ms=[t[2][0], None]),                                                                                       # a null moment
        dict(max_norm=1.0, no_total=True), dict(max_norm=1.0, no_scratch=True),                                          # clipping needs both
    ]
    for b in bad:
        r = _call_step(lib, b.get("ps", t[0]), b.get("gs", t[1]), b.get("ms", t[2]), b.get("vs", t[3]),
                       None if b.get("numels_none") else b.get("numels", numels), None if b.get("hyper_none") else b.get("hyper", [ok, ok]),
                       b.get("max_norm", 0.0), None if b.get("no_total") else total, None if b.get("no_scratch") else scratch)
        assert r == E_ARG, (b, r)
        assert lib.ldmseg_last_error()
    torch.cuda.synchronize()
    for k in range(4):
        assert all(torch.equal(x, torch.full((10,), float(k + 1), device=DEV)) for x in t[k])      # nothing ran
    # the two gradient entries
    g2 = (C.c_void_p * 2)(t[1][0].data_ptr(), t[1][1].data_ptr())
    nm = (C.c_int64 * 2)(10, 10)
    assert lib.ldmseg_grad_norm(2, None, nm, _lib.ptr(total), _lib.ptr(scratch), None) == E_ARG
    assert lib.ldmseg_grad_norm(2, g2, nm, None, _lib.ptr(scratch), None) == E_ARG
    assert lib.ldmseg_grad_clip(2, g2, nm, 0.0, _lib.ptr(total), _lib.ptr(scratch), None) == E_ARG
    assert lib.ldmseg_grad_clip(2, g2, (C.c_int64 * 2)(10, -3), 1.0, _lib.ptr(total), _lib.ptr(scratch), None) == E_ARG
    assert lib.ldmseg_multi_tensor_scratch_bytes(2, (C.c_int64 * 2)(10, -3)) == 0
    assert lib.ldmseg_multi_tensor_scratch_bytes(3, (C.c_int64 * 3)(0, 1, R.CHUNK + 1)) == 8 * (1 + 0 + 1 + 2)
    # and the good call of the same arguments goes through (a skipped tensor may bring null pointers and any hyper entry)
    assert _call_step(lib, [t[0][0], None], [t[1][0], None], [t[2][0], None], [t[3][0], None], numels, [ok, (0, 5, 5, -1, -1, 0)],
                      1.0, total, scratch) == 0
    torch.cuda.synchronize()
    assert abs(float(total) - 2.0 * math.sqrt(10.0)) < 1e-5 and not torch.equal(t[0][0], torch.full((10,), 1.0, device=DEV))
    assert torch.equal(t[0][1], torch.full((10,), 1.0, device=DEV))


def test_python_surface_refuses_what_the_kernels_do_not_serve():
    from ldmseg_amd.optim import AdamW, grad_norm
    with pytest.raises(ValueError):
        AdamW([torch.zeros(3, device=DEV, requires_grad=True)], betas=(0.9, 1.0))
    p = torch.zeros(3, requires_grad=True)                                  # a CPU tensor: no fallback
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError):
        AdamW([p]).step()
    with pytest.raises(RuntimeError):
        grad_norm([p])
    q = torch.zeros(3, device=DEV, requires_grad=True)
    opt = AdamW([q])
    q.grad = torch.ones(3, device=DEV)
    opt.param_groups[0]["lr"] = -1.0
    with pytest.raises(ValueError):
        opt.step()
    opt.zero_grad(set_to_none=False)
    assert q.grad is not None and float(q.grad.abs().sum()) == 0.0
    opt.zero_grad()
    assert q.grad is None


def test_more_partials_than_the_update_pass_adds_itself():
    """one tensor of 2049 chunks + 5 elements: a single launch whose partials go through the finish launch (the threshold is 2048)"""
    from ldmseg_amd.optim import clip_grad_norm_, grad_norm
    n = 2049 * R.CHUNK + 5
    g = torch.Generator().manual_seed(5)
    g0 = torch.randn(n, generator=g)
    p = torch.zeros(n, device=DEV, requires_grad=True)
    p.grad = g0.to(DEV)
    want = math.sqrt(float(g0.double().pow(2).sum()))
    total = clip_grad_norm_([p], 0.5 * want)
    assert abs(float(total) - want) <= 1e-6 * want
    assert torch.equal(p.grad.cpu(), g0 * R.clip_coef(total, 0.5 * want))
    assert abs(float(grad_norm([p])) - 0.5 * want) <= 1e-5 * want


def test_a_tensor_longer_than_2_to_the_31_elements():
    """2^31 + one chunk + 3 gradient elements: indices past 2^31, and the cut of a tensor into runs of 2^18 chunks (one launch each)"""
    from ldmseg_amd.optim import clip_grad_norm_, grad_norm
    n = 2 ** 31 + R.CHUNK + 3
    grad = torch.full((n,), 0.5, device=DEV)
    marks = {n - 1: 3.0, 2 ** 31: -2.0, 2 ** 31 - 1: 1.5, 0: 0.25}
    for i, v in marks.items():
        grad[i] = v
    p = types.SimpleNamespace(grad=grad)                                    # only the gradient is that long: 8.6 GB, no parameter
    want = math.sqrt((n - len(marks)) * 0.25 + sum(v * v for v in marks.values()))
    total = grad_norm([p])
    assert abs(float(total) - want) <= 1e-6 * want
    t2 = clip_grad_norm_([p], 0.5 * want)
    assert torch.equal(t2, total)
    coef = R.clip_coef(total, 0.5 * want)
    for i, v in marks.items():
        assert float(grad[i]) == float(torch.tensor(v) * coef), i
    half = float(torch.tensor(0.5) * coef)
    count = sum(int((grad[a:min(a + 2 ** 30, n)] == half).sum()) for a in range(0, n, 2 ** 30))
    assert count == n - len(marks)

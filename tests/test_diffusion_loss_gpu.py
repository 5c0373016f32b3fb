"""GPU suite of the denoising loss (csrc/loss.hip, TrainerDiffusion.compute_loss / predict_sample / get_loss_weight_mask /
validation_loss): the loss tail fed the reference's own prediction tensors (tests/golden/diffusion_loss.npz) bit for bit, OHEM
against torch.topk, the masks, min / max + clamp, whole compute_loss calls through the real UNet against the CPU restatement
(tests/diffusion_loss_ref.py driven by oracle/unet.py), and the validation driver with its tool entry.

Bounds.  Tail alone: element losses, pred_latents and per-sample sums are compared bit for bit; the mean within 1e-6 relative of
the fp64 sum (at most four fp32 roundings per element, about 2.4e-7; the fp64 accumulation adds nothing at that scale).  Through
the UNet: `prediction` within the forward tests' own bounds (1e-3 / 1e-3 / 6e-2 max-norm relative for fp32 / bf16x3 / bf16); the
tail adds no error of its own, so with d = bound * max|prediction| the l2 loss mean(w m (p - y)^2) moves by at most
max(w m) * d * (2 mean|p - y| + d), and pred_latents = (noisy - sb p) / sa by at most max_b(sb / sa) * d (+ 4 ulp of its terms).
Measured values: DESIGN.md section 8.3."""
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_loss_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16
SENTINEL = -768.0
KIND = {"l1": 0, "l2": 1, "smooth_l1": 2}
PTYPE = {"epsilon": 0, "sample": 1}
FORWARD_TOL = (("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16", 6e-2))


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def g(golden):
    return golden("diffusion_loss.npz")


def guarded(n, dtype=torch.float32):
    return torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)


def guard_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def dev(t):
    return None if t is None else torch.as_tensor(t).to(DEV).contiguous()


def run_tail(pred, t, ac, target=None, noisy=None, weights=None, mask=None, paste=None, paste_src=None, minmax=None, kind="l2",
             ptype="epsilon", ohem=1.0, want_elem=True, want_pred=True, expect=0):
    """ldmseg_diffusion_loss with guard elements behind every output; returns dict of CPU tensors"""
    B, Cn = pred.shape[0], pred.shape[1]
    HW = pred.numel() // (B * Cn)
    n = pred.numel()
    d = {k: dev(v) for k, v in dict(pred=pred, t=t, ac=ac, target=target, noisy=noisy, weights=weights, mask=mask, paste_src=paste_src,
                                    minmax=minmax).items()}
    pm = dev(paste.to(torch.uint8)) if paste is not None else None
    elem, pl = (guarded(n) if want_elem else None), (guarded(n) if want_pred else None)
    mean, sums = guarded(1), guarded(B)
    nbytes = lib().ldmseg_diffusion_loss_scratch_bytes(B, Cn, HW)
    scratch = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV).fill_(77)
    rc = lib().ldmseg_diffusion_loss(P(d["pred"]), P(d["target"]), P(d["noisy"]), P(d["t"]), P(d["ac"]), int(d["ac"].numel()),
                                     P(d["weights"]), P(d["mask"]), P(pm), P(d["paste_src"]), P(d["minmax"]), KIND[kind], PTYPE[ptype],
                                     float(ohem), B, Cn, HW, P(elem), P(pl), P(mean), P(sums), P(scratch), None)
    assert rc == expect, (rc, lib().ldmseg_last_error())
    torch.cuda.synchronize()
    if expect:
        return None
    assert guard_ok(mean, 1) and guard_ok(sums, B) and bool((scratch[nbytes:] == 77).all())
    out = {"mean": mean[:1].cpu(), "sums": sums[:B].cpu()}
    if want_elem:
        assert guard_ok(elem, n)
        out["elem"] = elem[:n].cpu().view(pred.shape)
    if want_pred:
        assert guard_ok(pl, n)
        out["pred_latents"] = pl[:n].cpu().view(pred.shape)
    return out


def parse_case(key):
    shape, kind, ptype, weight, m, p, o = key.split("/")
    return shape, kind, ptype, weight, int(m[1:]), int(p[1:]), float(o[1:])


# ------------------------------------------------------------------ 1. the tail on the reference's own tensors
@pytest.mark.parametrize("shape", ["a", "b"])
def test_tail_equals_the_reference_bit_for_bit(g, shape):
    x = {k: torch.from_numpy(g[f"{shape}/{k}"]) for k in ("t", "latents", "original", "noise", "loss_mask", "paste", "noisy", "prediction")}
    ac = torch.from_numpy(g["alphas_cumprod"])
    weights = {"none": torch.ones(1000), "max_clamp_snr": torch.from_numpy(g["weights_max_clamp_snr"])}
    for i, key in enumerate(k for k in g["loss_cases"] if k.startswith(shape + "/")):
        _, kind, ptype, weight, mask, paste, ohem = parse_case(key)
        target = x["noise"] if ptype == "epsilon" else x["original"]
        kw = dict(target=target, noisy=x["noisy"], weights=weights[weight], mask=x["loss_mask"] if mask else None,
                  paste=x["paste"] if paste else None, paste_src=x["original"] if paste else None, kind=kind, ptype=ptype, ohem=ohem)
        out = run_tail(x["prediction"], x["t"], ac, **kw)
        ek = f"{shape}/elem/{kind}/{ptype}/{weight}/m{mask}"
        want = torch.from_numpy(g[ek])
        assert torch.equal(out["elem"], want), key
        assert torch.equal(out["pred_latents"], torch.from_numpy(g[f"{shape}/pred_latents/{ptype}/p{paste}"])), key
        assert np.array_equal(out["sums"].numpy(), g[ek + "/sums"]), key
        ref64, _ = R.reduce_loss(want, ohem)
        assert abs(float(out["mean"]) - ref64) <= 1e-6 * abs(ref64), (key, float(out["mean"]), ref64)
        assert abs(float(out["mean"]) - float(g[key + "/loss"])) <= 1e-6 * abs(ref64), key       # and the reference's own fp32 mean
        if i % 7 == 0:
            again = run_tail(x["prediction"], x["t"], ac, **kw)
            assert all(torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)) for k in out), key
    assert float(run_tail(x["prediction"], x["t"], ac, target=x["noise"], noisy=x["noisy"], mask=x["loss_mask"])["sums"][-1]) == 0.0


# (B, C, HW): HW = 25 and C * HW off the vector width; HW = 64 is less than one workgroup; L = 40 leaves a ragged last workgroup
@pytest.mark.parametrize("B,Cn,HW", [(1, 1, 25), (2, 3, 25), (2, 4, 25), (1, 4, 64), (5, 4, 1600), (3, 2, 1023)])
@pytest.mark.parametrize("kind,ptype", [("l2", "epsilon"), ("smooth_l1", "sample"), ("l1", "epsilon")])
def test_tail_operator_shapes(g, B, Cn, HW, kind, ptype):
    gen = torch.Generator().manual_seed(B * 1000 + Cn * 100 + HW)
    shape = (B, Cn, HW)
    pred, target, noisy, src = (torch.randn(shape, generator=gen) for _ in range(4))
    pred = 1.5 * pred
    exact = np.flatnonzero(g["sqrt_exact"])
    t = torch.from_numpy(exact[torch.randint(0, len(exact), (B,), generator=gen).numpy()])
    mask = (torch.rand(B, HW, generator=gen) < 0.6).float() * 0.25
    mask[0] = 0.
    paste = torch.rand(shape, generator=gen) < 0.4
    weights = torch.from_numpy(g["weights_max_clamp_snr"])
    ac = torch.from_numpy(g["alphas_cumprod"])
    sa, sb = torch.from_numpy(g["sqrt_a"]), torch.from_numpy(g["sqrt_b"])
    mm = torch.tensor([-1.25, 0.75])
    out = run_tail(pred, t, ac, target=target, noisy=noisy, weights=weights, mask=mask, paste=paste, paste_src=src, minmax=mm,
                   kind=kind, ptype=ptype)
    elem = R.weighted_element_loss(pred, target, kind, mask.view(B, 1, HW)[:, 0], weights, t)
    want_pl = R.pred_latents(pred, noisy, t, sa, sb, ptype, paste, src, clamp=(mm[0], mm[1]))
    assert torch.equal(out["elem"], elem)
    assert torch.equal(out["pred_latents"], want_pl)
    assert np.array_equal(out["sums"].numpy(), R.exact_sample_sums(elem)) and float(out["sums"][0]) == 0.0
    ref64, _ = R.reduce_loss(elem)
    assert abs(float(out["mean"]) - ref64) <= 1e-6 * abs(ref64)
    # the optional outputs stay optional
    lean = run_tail(pred, t, ac, target=target, weights=weights, mask=mask, kind=kind, ptype=ptype, want_elem=False, want_pred=False)
    assert torch.equal(lean["mean"].view(torch.int32), out["mean"].view(torch.int32))
    assert torch.equal(lean["sums"].view(torch.int32), out["sums"].view(torch.int32))
    only_pred = run_tail(pred, t, ac, noisy=noisy, ptype=ptype, want_elem=False)
    assert torch.equal(only_pred["pred_latents"], R.pred_latents(pred, noisy, t, sa, sb, ptype))
    assert float(only_pred["mean"]) == SENTINEL            # no target: no loss is written


def test_tail_pred_latents_where_the_device_root_differs(g):
    """At about a quarter of the timesteps (tests/golden/device_sqrt_differs.json) the device square root that add_noise /
    remove_noise share is one ulp away from the correctly rounded one, so pred_latents cannot be bitwise there.  Bound: sa and sb
    are each at most 2 ulp (2^-22 relative) from the restatement's; v = (z - sb p) / sa then moves by at most 2^-22 (sb |p| / sa +
    |v|) plus three roundings of half an ulp: |dv| <= 2^-21 (|z| + sb |p|) / sa elementwise.  The element loss has no root in it
    and stays bitwise."""
    with open(os.path.join(ROOT, "tests", "golden", "device_sqrt_differs.json")) as f:
        differs = json.load(f)["device_differs"]
    assert len(differs) > 100
    ts = [differs[0], differs[len(differs) // 2], differs[-1]]
    gen = torch.Generator().manual_seed(77)
    shape = (3, 4, 100)
    pred, target, noisy = (torch.randn(shape, generator=gen) for _ in range(3))
    t = torch.tensor(ts)
    ac = torch.from_numpy(g["alphas_cumprod"])
    sa, sb = torch.from_numpy(g["sqrt_a"]), torch.from_numpy(g["sqrt_b"])
    out = run_tail(pred, t, ac, target=target, noisy=noisy, kind="l2", ptype="epsilon")
    assert torch.equal(out["elem"], R.element_loss(pred, target, "l2"))
    want = R.pred_latents(pred, noisy, t, sa, sb, "epsilon")
    bound = 2.0 ** -21 * (noisy.abs() + R.per_sample(sb[t], pred) * pred.abs()) / R.per_sample(sa[t], pred)
    err = (out["pred_latents"] - want).abs()
    print(f"device-root timesteps {ts}: {int((err > 0).sum())} of {err.numel()} elements differ, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_tail_clamp_propagates_nan_bounds(g):
    """torch.clamp(x, nan, nan) is NaN everywhere: latents that hold a NaN give a NaN {min, max} pair and NaN pred_latents"""
    ac = torch.from_numpy(g["alphas_cumprod"])
    pred, noisy = (torch.randn(2, 4, 16, generator=torch.Generator().manual_seed(i)) for i in range(2))
    nan = float("nan")
    for mm in ([nan, nan], [nan, 1.0], [-1.0, nan]):
        out = run_tail(pred, torch.tensor([10, 20]), ac, noisy=noisy, minmax=torch.tensor(mm), ptype="sample", want_elem=False)
        assert torch.isnan(out["pred_latents"]).all(), mm
        assert torch.isnan(torch.clamp(pred, torch.tensor(mm[0]), torch.tensor(mm[1]))).all()
    out = run_tail(pred, torch.tensor([10, 20]), ac, noisy=noisy, minmax=torch.tensor([-0.5, 0.5]), ptype="sample", want_elem=False)
    assert torch.equal(out["pred_latents"], torch.clamp(pred, -0.5, 0.5))


def test_tail_clamps_timesteps_and_refuses_bad_arguments(g):
    ac = torch.from_numpy(g["alphas_cumprod"])
    pred, target, noisy = (torch.randn(2, 4, 16, generator=torch.Generator().manual_seed(i)) for i in range(3))
    w = torch.from_numpy(g["weights_max_clamp_snr"])
    lo = run_tail(pred, torch.tensor([-5, 2000]), ac, target=target, noisy=noisy, weights=w)
    ok = run_tail(pred, torch.tensor([0, 999]), ac, target=target, noisy=noisy, weights=w)
    assert all(torch.equal(lo[k], ok[k]) for k in ok)
    t = torch.tensor([1, 2])
    run_tail(pred, t, ac, target=target, noisy=noisy, ohem=0.001, expect=-1)                    # k == 0
    run_tail(pred, t, ac, target=target, noisy=noisy, ohem=0.5, want_elem=False, expect=-1)     # OHEM needs the element buffer
    run_tail(pred, t, ac, want_elem=False, want_pred=False, expect=-1)                          # nothing to compute
    run_tail(pred, t, ac, target=target, want_elem=False, expect=-1)                            # epsilon pred_latents without noisy
    assert b"noisy" in lib().ldmseg_last_error()


# ------------------------------------------------------------------ 2. OHEM
def ohem_values(n, flavour, gen):
    v = torch.rand(n, generator=gen) * 3
    if flavour == "half_zero":
        v[torch.randperm(n, generator=gen)[:n // 2]] = 0.
    elif flavour == "levels16":
        v = torch.floor(v * 16 / 3) / 16
    elif flavour == "equal":
        v = torch.full((n,), 0.625)
    return v


@pytest.mark.parametrize("n", [100, 256, 40000])
@pytest.mark.parametrize("flavour", ["random", "half_zero", "levels16", "equal"])
def test_ohem_is_exact(g, n, flavour):
    gen = torch.Generator().manual_seed(n + len(flavour))
    v = ohem_values(n, flavour, gen)
    ac = torch.from_numpy(g["alphas_cumprod"])
    zeros = torch.zeros(1, 1, n)
    for ratio in (0.5, 0.7, 1.5 / n):                      # k = n / 2, int(0.7 n) (reaches into the zeros of half_zero), 1
        k = int(ratio * n)
        out = run_tail(v.view(1, 1, n), torch.tensor([3]), ac, target=zeros, kind="l1", ptype="sample", ohem=ratio, want_pred=False)
        assert torch.equal(out["elem"].view(-1), v)
        want = np.float32(float(torch.topk(v.double(), k)[0].sum()) / k)
        assert np.float32(out["mean"].item()) == want, (ratio, k, out["mean"].item(), want)
        again = run_tail(v.view(1, 1, n), torch.tensor([3]), ac, target=zeros, kind="l1", ptype="sample", ohem=ratio, want_pred=False)
        assert torch.equal(again["mean"].view(torch.int32), out["mean"].view(torch.int32))


def test_ohem_nan_and_l2_values(g):
    ac = torch.from_numpy(g["alphas_cumprod"])
    gen = torch.Generator().manual_seed(9)
    v = torch.rand(1, 1, 1000, generator=gen)
    v[0, 0, 777] = float("nan")
    out = run_tail(v, torch.tensor([3]), ac, target=torch.zeros_like(v), kind="l1", ptype="sample", ohem=0.5, want_pred=False)
    assert torch.isnan(out["mean"]).all()
    plain = run_tail(v, torch.tensor([3]), ac, target=torch.zeros_like(v), kind="l1", ptype="sample", want_pred=False)
    assert torch.isnan(plain["mean"]).all()
    # several samples and channels: the selection runs over the whole flattened buffer
    p, y = torch.randn(3, 4, 100, generator=gen), torch.randn(3, 4, 100, generator=gen)
    out = run_tail(p, torch.tensor([3, 4, 5]), ac, target=y, kind="l2", ptype="sample", ohem=0.7, want_pred=False)
    elem = R.element_loss(p, y, "l2")
    assert torch.equal(out["elem"], elem)
    assert np.float32(out["mean"].item()) == np.float32(R.reduce_loss(elem, 0.7)[0])


# ------------------------------------------------------------------ trainer on a stand-in network
def make_trainer(network, sched_kw, ptype="epsilon", weight="none", **kw):
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    sch = DDIMNoiseScheduler(**{**sched_kw, "prediction_type": ptype, "weight": weight})
    if not hasattr(network, "in_channels"):
        network.in_channels, network.device = 8, torch.device(DEV)
    return TrainerDiffusion(None, network, sch, device=DEV, **kw)


# ------------------------------------------------------------------ 3. masks
def test_masks_equal_the_reference_bit_for_bit(g, sched_kw):
    tr = make_trainer(R.StandIn(g["standin_w"], device=DEV), sched_kw)
    for key in g["mask_cases"]:
        _, name, size, type_mask, ignore = key.split("/")
        targets, padding = torch.from_numpy(g[f"mask/{name}/targets"]), torch.from_numpy(g[f"mask/{name}/padding"])
        want = torch.from_numpy(g[key])
        out = tr.get_loss_weight_mask(targets, ignore_label=int(ignore), size=(int(size), int(size)), type_mask=type_mask,
                                      padding_mask=padding)
        assert out.is_cuda and out.dtype == torch.float32 and torch.equal(out.cpu(), want), key
        assert int(tr.loss_mask_flag.item()) == 0
        if type_mask == "padding":                        # every source dtype reads the same map
            for alt in (padding.to(torch.uint8), padding.float(), padding.long()):
                assert torch.equal(tr.get_loss_weight_mask(None, size=(int(size),) * 2, type_mask="padding", padding_mask=alt).cpu(), want)
    assert tr.get_loss_weight_mask(targets, type_mask="none") is None
    # a non-square output and an int size
    t = torch.from_numpy(g["mask/s37x53/targets"])
    assert torch.equal(tr.get_loss_weight_mask(t, size=(8, 24), type_mask="counts").cpu(), R.loss_weight_mask(t, (8, 24), "counts"))
    assert torch.equal(tr.get_loss_weight_mask(t, size=64, type_mask="ignore").cpu(), R.loss_weight_mask(t, (64, 64), "ignore"))


def test_mask_flags_an_id_outside_the_table(g):
    targets = torch.from_numpy(g["mask/s32/targets"]).clone()
    targets[0, 4:8, 4:8] = 300
    targets[2, 0:4, 0:4] = -7
    B, h, w = 3, 8, 8
    out, flag = guarded(B * h * w), torch.full((1 + GUARD,), 1234, dtype=torch.int32, device=DEV)
    src = targets.to(DEV)
    assert lib().ldmseg_loss_weight_mask(P(src), 0, B, 32, 32, h, w, 2, 0, P(out), P(flag), None) == 0
    torch.cuda.synchronize()
    assert guard_ok(out, B * h * w) and int(flag[0]) == 1 and bool((flag[1:] == 1234).all())
    got = out[:B * h * w].cpu().view(B, h, w)
    small = targets[:, ::4, ::4]
    assert torch.isnan(got[(small == 300) | (small == -7)]).all()                # loud in the loss, never an index
    good = targets.clone()
    good[(targets == 300) | (targets == -7)] = 0
    want = R.loss_weight_mask(good, (h, w), "counts")
    keep = ~torch.isnan(got)
    assert torch.equal(got[keep], want[keep])
    # the same map is fine for 'ignore', which keeps no table
    assert lib().ldmseg_loss_weight_mask(P(src), 0, B, 32, 32, h, w, 0, 0, P(out), P(flag), None) == 0
    torch.cuda.synchronize()
    assert int(flag[0]) == 0 and torch.equal(out[:B * h * w].cpu().view(B, h, w), (small != 0).float())
    assert lib().ldmseg_loss_weight_mask(P(src), 0, B, 32, 32, h, w, 5, 0, P(out), P(flag), None) == -1


# ------------------------------------------------------------------ 4. min / max, clamp, predict_sample
@pytest.mark.parametrize("n", [1, 100, 1024, 300001])
def test_tensor_minmax(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    out, scratch = guarded(2), torch.empty(3072 + GUARD, dtype=torch.uint8, device=DEV).fill_(77)
    assert lib().ldmseg_tensor_minmax(P(x), n, P(out), P(scratch), None) == 0
    torch.cuda.synchronize()
    assert guard_ok(out, 2) and bool((scratch[3072:] == 77).all())
    assert float(out[0]) == float(x.min()) and float(out[1]) == float(x.max())
    x[n // 2] = float("nan")
    assert lib().ldmseg_tensor_minmax(P(x), n, P(out), P(scratch), None) == 0
    assert torch.isnan(out[:2]).all()
    assert lib().ldmseg_tensor_minmax(P(x), 0, P(out), P(scratch), None) == -1


def test_predict_sample_equals_the_reference_bit_for_bit(g, sched_kw):
    net = R.StandIn(g["standin_w"], device=DEV)
    for key in g["predict_cases"]:
        _, shape, ptype = key.split("/")
        tr = make_trainer(net, sched_kw, ptype=ptype)
        lat, rgb = dev(g[f"{shape}/latents"]), dev(g[f"{shape}/rgb"])
        out = tr.predict_sample(lat, rgb, None, noise=dev(g[key + "/noise"]), timesteps=dev(g[key + "/t"]))
        assert torch.equal(out.cpu(), torch.from_numpy(g[key + "/pred"])), key
    # the draws: reproducible with a generator, inside [0, tmax)
    a = tr.predict_sample(lat, rgb, None, tmax=500, generator=torch.Generator(DEV).manual_seed(5))
    b = tr.predict_sample(lat, rgb, None, tmax=500, generator=torch.Generator(DEV).manual_seed(5))
    assert torch.equal(a, b) and int(net.calls[-1][1].max()) < 500
    tr.noise_scheduler.prediction_type = "v_prediction"
    with pytest.raises(ValueError):
        tr.predict_sample(lat, rgb)


# ------------------------------------------------------------------ 5. compute_loss / loss_fn of the trainer on the stand-in
def test_trainer_compute_loss_equals_the_reference(g, sched_kw):
    net = R.StandIn(g["standin_w"], device=DEV)
    for key in g["loss_cases"]:
        shape, kind, ptype, weight, mask, paste, ohem = parse_case(key)
        x = {k: dev(g[f"{shape}/{k}"]) for k in ("t", "latents", "original", "rgb", "noise", "loss_mask", "paste", "noisy")}
        tr = make_trainer(net, sched_kw, ptype=ptype, weight=weight, training_loss_type=kind, ohem_ratio=ohem, self_condition=False)
        loss, noisy, pl, t = tr.compute_loss(x["noise"], x["t"], x["noisy"], x["rgb"], None, x["loss_mask"] if mask else None,
                                             latents=x["latents"], original_latents=x["original"],
                                             inpainting_masks=x["paste"] if paste else None)
        assert loss.is_cuda and loss.dim() == 0 and noisy.is_cuda and t.is_cuda
        ref = float(g[key + "/loss"])
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref), key
        assert torch.equal(pl.cpu(), torch.from_numpy(g[f"{shape}/pred_latents/{ptype}/p{paste}"])), key
        assert torch.equal(noisy, x["noisy"]) and torch.equal(t, x["t"])
        ek = f"{shape}/elem/{kind}/{ptype}/none/m{mask}"
        if ek in g.files and weight == "none":            # loss_fn: the element loss in front of the timestep weights
            got = tr.loss_fn(dev(g[f"{shape}/prediction"]), x["noise"] if ptype == "epsilon" else x["original"],
                             mask=x["loss_mask"] if mask else None)
            assert torch.equal(got.cpu(), torch.from_numpy(g[ek])), key


def test_trainer_refusals_and_noise_levels(g, sched_kw):
    net = R.StandIn(g["standin_w"], device=DEV)
    x = {k: dev(g[f"a/{k}"]) for k in ("t", "latents", "original", "rgb", "noise", "loss_mask", "paste", "noisy")}
    args = (x["noise"], x["t"], x["noisy"], x["rgb"], None, None)
    tr = make_trainer(net, sched_kw, self_condition=False)
    with pytest.raises(AssertionError):
        tr.compute_loss(x["noise"], x["t"], x["noisy"], None, None, None)
    with pytest.raises(ValueError):
        tr.compute_loss(*args, original_latents=x["original"], inpainting_masks=x["paste"][:, :1])
    with pytest.raises(ValueError):
        tr.compute_loss(*args, original_latents=x["original"], inpainting_masks=x["paste"].float())
    with pytest.raises(ValueError):
        make_trainer(net, sched_kw, training_loss_type="huber", self_condition=False).compute_loss(*args)
    with pytest.raises(ValueError):
        make_trainer(net, sched_kw, training_loss_type="huber", self_condition=False).loss_fn(x["noise"], x["noisy"])
    with pytest.raises(ValueError):
        make_trainer(net, sched_kw, ptype="v_prediction", self_condition=False).compute_loss(*args)
    with pytest.raises(ValueError):
        make_trainer(net, sched_kw, ohem_ratio=1e-4, self_condition=False).compute_loss(*args)
    # RGB noise: drawn on the device from `generator`, passed on as timestep_img; the condition noise likewise
    sa, sb = torch.from_numpy(g["sqrt_a"]), torch.from_numpy(g["sqrt_b"])
    net12 = R.StandIn(torch.cat([torch.from_numpy(g["standin_w"]), torch.full((4, 4), 0.125)], dim=1), device=DEV)
    net12.in_channels, net12.device = 12, torch.device(DEV)
    tr = make_trainer(net12, sched_kw, rgb_noise_level=300, cond_noise_level=200)
    assert tr.self_condition
    cond = x["latents"] * 0.5
    loss, _, _, _ = tr.compute_loss(*args, condition=cond, generator=torch.Generator(DEV).manual_seed(11))
    inputs, _, _, t_img = net12.calls[-1]
    gen = torch.Generator(DEV).manual_seed(11)
    rgb_noise = torch.randn(x["rgb"].shape, device=DEV, generator=gen)
    want_t_img = torch.randint(0, 300, (2,), device=DEV, generator=gen)
    cond_noise = torch.randn(cond.shape, device=DEV, generator=gen)
    t_cond = torch.randint(0, 200, (2,), device=DEV, generator=gen)
    assert torch.equal(t_img, want_t_img)
    assert inputs.shape[1] == 12 and torch.equal(inputs[:, :4], x["noisy"])
    # whatever the draws: the device's root and torch's are each within 1 ulp of the exact one, so a coefficient is at most 2 ulp off
    # and sa x + sb n (sa, sb <= 1; two products and a sum, half an ulp each) moves by less than 4 * 2^-23 * (|x| + |n|)
    for got, x0, n0, tt in ((inputs[:, 4:8], x["rgb"], rgb_noise, want_t_img), (inputs[:, 8:], cond, cond_noise, t_cond)):
        want = R.add_noise(x0.cpu(), n0.cpu(), tt.cpu(), sa, sb)
        assert bool(((got.cpu() - want).abs() <= 4 * 2.0 ** -23 * (x0.cpu().abs() + n0.cpu().abs())).all())
        assert not torch.equal(got.cpu(), x0.cpu())
    again, _, _, _ = tr.compute_loss(*args, condition=cond, generator=torch.Generator(DEV).manual_seed(11))
    assert torch.equal(loss, again)
    # a self-conditioned trainer without a condition feeds zeros (:563-564)
    make_trainer(net12, sched_kw).compute_loss(*args)
    assert not net12.calls[-1][0][:, 8:].any() and net12.calls[-1][3] is None


# ------------------------------------------------------------------ 6. whole compute_loss through the real UNet
@pytest.fixture(scope="module")
def unets():
    """(kind, mode) -> (state dict, handle), built when first asked for and kept for the module"""
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet
    sds, made = {}, {}

    def sd_of(kind):
        if kind not in sds:
            if kind == "plain8":
                sds[kind] = weights.generate(weights.unet_schema(8, False), seed=3)
            elif kind == "selfcond12":
                sds[kind] = weights.generate(weights.unet_schema(12, False), seed=0)
            elif kind == "sepenc":
                s = weights.unet_schema(4, False)
                s.update(weights.separate_encoder_schema(True))
                sds[kind] = weights.generate(s, seed=21)
            else:
                sds[kind] = weights.generate(weights.unet_schema(8, True), seed=11)
        return sds[kind]

    def get(kind, mode):
        if (kind, mode) not in made:
            made[(kind, mode)] = UNet(sd_of(kind), in_channels=12 if kind == "selfcond12" else 8, device=DEV, compute_dtype=mode,
                                      cross_attention=kind == "cross")
        return sd_of(kind), made[(kind, mode)]
    yield get
    made.clear()


def oracle_network(kind, sd):
    from oracle import unet as o_unet
    import unet_sepenc_ref

    def net(inputs, t, ctx=None, timestep_img=None):
        if kind == "sepenc":
            return SimpleNamespace(sample=unet_sepenc_ref.sepenc_forward(sd, inputs, t, timestep_img))
        return SimpleNamespace(sample=o_unet.unet_forward(sd, inputs, t, encoder_hidden_states=ctx))
    return net


@pytest.mark.parametrize("B,L,ts", [(2, 8, (999, 120)), (1, 16, (500,))])
@pytest.mark.parametrize("kind", ["plain8", "selfcond12", "sepenc", "cross"])
def test_compute_loss_through_the_unet(g, sched_kw, unets, kind, B, L, ts):
    gen = torch.Generator().manual_seed(B * 100 + L)
    sa, sb = torch.from_numpy(g["sqrt_a"]), torch.from_numpy(g["sqrt_b"])
    t = torch.tensor(ts)
    latents = 0.5 * torch.randn(B, 4, L, L, generator=gen)
    rgb = 0.7 * torch.randn(B, 4, L, L, generator=gen)
    noise = torch.randn(B, 4, L, L, generator=gen)
    ctx = torch.randn(B, 77, 768, generator=gen) if kind == "cross" else None
    loss_mask = (torch.rand(B, L, L, generator=gen) < 0.8).float()
    weights = torch.from_numpy(g["weights_max_clamp_snr"])
    noisy = R.add_noise(latents, noise, t, sa, sb)
    torch.set_num_threads(16)
    sd, _ = unets(kind, "fp32")
    oracle = oracle_network(kind, sd)
    rgb_level = 300 if kind == "sepenc" else 0
    d = {k: dev(v) for k, v in dict(t=t, latents=latents, rgb=rgb, noise=noise, ctx=ctx, loss_mask=loss_mask, noisy=noisy).items()}
    # the call on the CPU, once: restatement + oracle UNet, fed the draws the device will make from the same seed
    seed, rgb_in, t_img = 17, rgb, None
    if rgb_level:
        gd = torch.Generator(DEV).manual_seed(seed)
        rgb_noise = torch.randn(rgb.shape, device=DEV, generator=gd).cpu()
        t_img = torch.randint(0, rgb_level, (B,), device=DEV, generator=gd).cpu()
        rgb_in = R.add_noise(rgb, rgb_noise, t_img, sa, sb)
    with torch.no_grad():
        pre_ref = cond_ref = None
        if kind == "selfcond12":                          # the no-grad pre-pass of train_single_epoch (:822-831)
            pre_ref = oracle(torch.cat([noisy, rgb, torch.zeros_like(noisy)], dim=1), t).sample
            cond_ref = R.remove_noise(noisy, pre_ref, t, sa, sb)
        ref_loss, ref_elem, ref_pl, ref_pred = R.compute_loss(
            oracle, noise, t, noisy, rgb_in, loss_mask, "l2", "epsilon", sa, sb, weights=weights, latents=latents,
            condition=cond_ref, encoder_hidden_states=ctx, timestep_img=t_img)
    for mode, tol in FORWARD_TOL:
        _, unet = unets(kind, mode)
        tr = make_trainer(unet, sched_kw, weight="max_clamp_snr", rgb_noise_level=rgb_level)
        assert tr.self_condition == (kind == "selfcond12")
        condition = None
        if tr.self_condition:
            # the pre-pass runs on the device and is held to the forward bound itself; compute_loss is then fed the oracle's
            # condition, so that `prediction` is one forward away from the reference and the forward bound applies to it
            pre = tr._predict(d["noisy"], d["rgb"], torch.zeros_like(d["noisy"]), d["t"], None)
            assert rel_err(pre, pre_ref) < tol, (mode, rel_err(pre, pre_ref))
            assert tr.noise_scheduler.remove_noise(d["noisy"], pre, d["t"]).shape == noisy.shape
            condition = dev(cond_ref)
        loss, _, pl, _ = tr.compute_loss(d["noise"], d["t"], d["noisy"], d["rgb"], d["ctx"], d["loss_mask"], latents=d["latents"],
                                         condition=condition, generator=torch.Generator(DEV).manual_seed(seed))
        got_pred = tr._predict(d["noisy"], dev(rgb_in), condition, d["t"], d["ctx"], dev(t_img))
        e_pred = rel_err(got_pred, ref_pred)
        delta = tol * float(ref_pred.abs().max())
        wm = float((weights[t].view(B, 1, 1) * loss_mask).max())
        loss_bound = wm * delta * (2 * float((ref_pred - noise).abs().mean()) + delta)
        amp = float((sb[t] / sa[t]).max())
        pl_bound = amp * delta * (1 + 1e-3) + 4 * 2.0 ** -24 * float(noisy.abs().max() + ref_pred.abs().max()) / float(sa[t].min())
        e_loss, e_pl = abs(float(loss) - ref_loss), float((pl.cpu() - ref_pl).abs().max())
        print(f"{kind} B={B} L={L} {mode}: prediction rel err {e_pred:.2e} (bound {tol:.0e}); loss {ref_loss:.5f} abs err {e_loss:.2e} "
              f"(bound {loss_bound:.2e}); pred_latents abs err {e_pl:.2e} (bound {pl_bound:.2e})")
        assert e_pred < tol, (mode, e_pred)
        assert e_loss <= loss_bound, (mode, e_loss, loss_bound)
        assert e_pl <= pl_bound, (mode, e_pl, pl_bound)


# ------------------------------------------------------------------ 7. validation_loss and the tool
@pytest.fixture(scope="module")
def val_trainer(sched_kw, vae_sd):
    from ldmseg_amd import weights
    from ldmseg_amd.models import GeneralVAEImage, GeneralVAESeg, UNet
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    usd = weights.generate(weights.unet_schema(12, False), seed=0)
    isd = weights.generate(weights.vae_image_schema(), seed=11, norm_keys=weights.VAE_IMAGE_NORM_KEYS)
    unet = UNet(usd, in_channels=12, device=DEV, compute_dtype="bf16")
    vae = GeneralVAESeg(vae_sd, scaling_factor=0.18215, device=DEV, compute_dtype="bf16")
    enc = GeneralVAEImage(isd, scaling_factor=0.18215, device=DEV, compute_dtype="bf16")
    return TrainerDiffusion(vae, unet, DDIMNoiseScheduler(**{**sched_kw, "weight": "max_clamp_snr"}), vae_image=enc, latent_size=8,
                            type_mask="counts")


def val_batches(n=2, B=2, S=64):
    from ldmseg_amd.data.bitcodec import encode_bitmap
    gen = torch.Generator().manual_seed(4)
    out = []
    for _ in range(n):
        semseg = torch.randint(0, 6, (B, S // 8, S // 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
        bits, _ = encode_bitmap(semseg.to(DEV), n=7, fill_value=0.5, ignore_label=0)
        out.append({"image": torch.rand(B, 3, S, S, generator=gen), "image_semseg": bits, "semseg": semseg,
                    "mask": torch.ones(B, S, S, dtype=torch.bool), "text": [""] * B})
    return out


def test_validation_loss_is_the_mean_of_compute_loss(val_trainer):
    tr, data, grid, seed = val_trainer, val_batches(), (50, 450, 950), 7
    out = tr.validation_loss(data, timesteps=grid, seed=seed)
    assert out["images"] == 4 and sorted(out["per_timestep"]) == list(grid)
    per = {t: [] for t in grid}
    for batch in data:
        mi = tr.process_inputs(batch)
        assert mi.latents.shape == (2, 4, 8, 8) and mi.loss_mask.shape == (2, 8, 8) and mi.inpainting_masks is None
        assert int(tr.loss_mask_flag.item()) == 0
        noise = tr.draw_noise(2, 8, seed).to(DEV)
        for t in grid:
            tt = torch.full((2,), t, dtype=torch.long, device=DEV)
            noisy = tr.noise_scheduler.add_noise(mi.latents, noise, tt)
            pre = tr._predict(noisy, mi.rgb_latents, torch.zeros_like(noisy), tt, None)
            cond = tr.noise_scheduler.remove_noise(noisy, pre, tt)
            loss, _, _, _ = tr.compute_loss(noise, tt, noisy, mi.rgb_latents, None, mi.loss_mask, latents=mi.latents,
                                            original_latents=mi.original_latents, condition=cond)
            per[t].append(float(loss))
    for t in grid:
        assert abs(out["per_timestep"][t] - np.mean(np.asarray(per[t], dtype=np.float64))) <= 1e-12 * abs(out["per_timestep"][t]), t
    assert abs(out["loss"] - np.mean([out["per_timestep"][t] for t in grid])) <= 1e-12 * abs(out["loss"])
    assert np.isfinite(out["loss"]) and out["loss"] > 0
    again = tr.validation_loss(data, timesteps=grid, seed=seed)
    assert again == out                                                          # bitwise repeatable
    assert tr.validation_loss(data, timesteps=grid, seed=seed, max_iter=1)["images"] == 2


def test_main_ldm_eval_val_loss_on_the_coco_pairs(golden, tmp_path):
    gld = golden("real_coco.npz")
    img_dir, gt_dir = tmp_path / "rgb", tmp_path / "pan"
    img_dir.mkdir(); gt_dir.mkdir()
    for k, n in enumerate(["000000012280", "000000084752"]):
        (img_dir / f"{n}.jpg").write_bytes(gld[f"jpg_{k}"].tobytes())
        (gt_dir / f"{n}.png").write_bytes(gld[f"png_{k}"].tobytes())
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "latent-diffusion-segmentation_amd")]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "main_ldm_eval.py"), "--images", str(img_dir), "--panoptic", str(gt_dir),
                        "--size", "128", "--batch", "2", "--dtype", "bf16", "--val-loss"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"loss"')]
    assert len(line) == 1, r.stdout[-2000:]
    out = json.loads(line[0])
    assert out["images"] == 2 and sorted(map(int, out["per_timestep"])) == list(range(50, 1000, 100)) and np.isfinite(out["loss"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "main_ldm_eval.py"), "--images", str(img_dir), "--val-loss"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 2 and "--val-loss needs --panoptic" in r.stderr

"""The library's fused clip + AdamW through the seg-VAE: TrainerAE.training_step with ldmseg_amd.optim.AdamW against the same steps
with torch.optim.AdamW + clip_grad_norm_ on a second object (identical seeds), the first step's parameters against the float64 CPU
reference under the bound of tests/optim_ref.py, and TrainerAE.save / resume in the reference's model.pt layout.  Shapes and loss
settings are those of tests/test_vae_encode_backward_python_gpu.py (B = 2, H = 24 / 32, 64 points)."""
import pytest
import torch

import optim_ref as O
import vae_backward_run as G
import vae_encode_backward_ref as R

pytestmark = pytest.mark.gpu
NAME = "seg"
LR = 1e-3
LOSS_KW = dict(loss_weights={"ce": 1.0, "mask": 1.0, "kl": 1e-4},
               loss_kwargs=dict(num_points=64, oversample_ratio=3, importance_sample_ratio=0.75, temperature=1.0))


def fresh(mode, sd=None):
    from ldmseg_amd.models import GeneralVAESeg
    return GeneralVAESeg(sd if sd is not None else R.state_dict(NAME), device=G.DEV, compute_dtype=mode, scaling_factor=0.2, **R.CONFIGS[NAME])


def dev_gen(seed):
    return torch.Generator(device=G.DEV).manual_seed(seed)


def batch(B, H, seed=5, classes=12):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, classes, (B, H // 8, H // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    bits = torch.stack([(ids >> i) % 2 for i in range(7)], dim=1).float()
    return G.dev(2.0 * bits - 1.0), ids.to(G.DEV)


def step(tr, x, targets, opt, clip, i):
    return tr.training_step(x, targets, opt, clip_grad=clip, generator=dev_gen(20 + i), point_generator=torch.Generator().manual_seed(i))


def hand_gradient(v, tr, x, targets, i):
    """step i's gradient before any clipping: forward, point loss, backward with the step's seeds (every kernel is bitwise repeatable)"""
    for p in v.parameters():
        p.grad = None
    out = v(x, sample_posterior=True, generator=dev_gen(20 + i))
    tr.compute_point_loss(out, targets, generator=torch.Generator().manual_seed(i))[0].backward()
    return [p.grad.detach().cpu().clone() for p in v.parameters()]


def cpu_step(p0, g0, clip, dtype):
    """one clip_grad_norm_ + torch.optim.AdamW step on CPU copies in `dtype` -> a snapshot as tests/optim_ref.py compares them"""
    ps = [t.to(dtype).clone().requires_grad_(True) for t in p0]
    for p, g in zip(ps, g0):
        p.grad = g.to(dtype).clone()
    opt = torch.optim.AdamW(ps, lr=LR, foreach=False)
    total = torch.nn.utils.clip_grad_norm_(ps, clip, foreach=False)
    opt.step()
    return O.snapshot(ps, lambda p: opt.state.get(p), total)


@pytest.mark.parametrize("mode,H", [("fp32", 32), ("fp32", 24), ("bf16x3", 32), ("bf16x3", 24)])
def test_five_steps_with_the_library_optimiser_follow_torchs(mode, H):
    """Step 1's gradient is the same bits on both objects (the same kernels and seeds); what the two optimisers leave in `.grad` differs
    only by their norms' last bits (fp64 sum here, torch's fp32 one there), so the library's `.grad` is checked bitwise against
    g * coef of ITS returned norm and against torch's within 1e-5."""
    from ldmseg_amd.optim import AdamW
    from ldmseg_amd.trainers import TrainerAE
    torch.set_num_threads(16)
    x, targets = batch(2, H)
    va, vb = fresh(mode), fresh(mode)
    ta, tb = TrainerAE(va, **LOSS_KW), TrainerAE(vb, **LOSS_KW)
    pa, pb = va.parameters(), vb.parameters()
    assert len(pa) == 34
    p0 = [p.detach().cpu().clone() for p in pa]
    g0 = hand_gradient(va, ta, x, targets, 0)
    assert all(torch.equal(a, b) for a, b in zip(g0, hand_gradient(vb, tb, x, targets, 0)))
    norm0 = O.true_norm(g0)
    clip = 0.5 * norm0
    oa, ob = AdamW(pa, lr=LR), torch.optim.AdamW(pb, lr=LR)
    la, lb = [], []
    for i in range(5):
        la.append(float(step(ta, x, targets, oa, clip, i)[0]))
        lb.append(float(step(tb, x, targets, ob, clip, i)[0]))
        assert ta.last_grad_norm.is_cuda and ta.last_grad_norm.dim() == 0
        if i == 0:
            assert abs(float(ta.last_grad_norm) - norm0) <= 1e-6 * norm0
            coef = O.clip_coef(ta.last_grad_norm, clip)
            assert float(coef) < 1.0
            for k, (p, q, g) in enumerate(zip(pa, pb, g0)):
                assert torch.equal(p.grad.cpu(), g * coef), k
                assert R.metric(p.grad, q.grad.cpu()) <= 1e-5, k
            got = O.snapshot(pa, lambda p: oa.state.get(p), ta.last_grad_norm)
            r64, r32 = cpu_step(p0, g0, clip, torch.float64), cpu_step(p0, g0, clip, torch.float32)
            w_lib, at_lib = O.worst(None, [got], [r64], init=p0)
            w_32, at_32 = O.worst(None, [r32], [r64], init=p0)
            print(f"{mode} H={H}: step 1 library worst {w_lib:.3e} at {at_lib}; fp32 CPU yardstick {w_32:.3e} at {at_32}")
            assert w_lib <= max(2.0 * w_32, 1e-6), (w_lib, at_lib, w_32)
    print(f"{mode} H={H}: losses library {la} torch {lb}")
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-3 * abs(b), (la, lb)
    assert all(s["step"] == 5 for s in oa.state.values()) and len(oa.state) == 34
    # the handle is fresh: no stale-weights error, and it computes what an object built from the current state dict computes
    with torch.no_grad():
        mom = va.encode_moments(x)
        w = fresh(mode, va.state_dict())
        assert torch.equal(w.encode_moments(x), mom)
        z = w.encode(x).latent_dist.mode()
        assert torch.equal(w.decode(z, interpolate=False), va.decode(z, interpolate=False))


def test_lr_argument_is_written_to_every_group_first():
    from ldmseg_amd.optim import AdamW
    from ldmseg_amd.trainers import TrainerAE
    x, targets = batch(2, 24)
    outs = []
    for lr in (None, 5e-3):
        v = fresh("fp32")
        tr = TrainerAE(v, **LOSS_KW)
        ps = v.parameters()
        opt = AdamW([{"params": ps[:20]}, {"params": ps[20:], "lr": 7e-4}], lr=LR)
        tr.training_step(x, targets, opt, clip_grad=0.0, generator=dev_gen(20), point_generator=torch.Generator().manual_seed(0), lr=lr)
        assert tr.last_grad_norm is None
        assert [g["lr"] for g in opt.param_groups] == ([LR, 7e-4] if lr is None else [lr, lr])
        outs.append([p.detach().cpu() for p in ps])
    assert all(not torch.equal(a, b) for a, b in zip(*outs))


def test_state_dict_and_load_state_dict_carry_the_current_values():
    v = fresh("fp32")
    sd0 = v.state_dict()
    ref = R.state_dict(NAME)
    assert list(sd0) == list(ref) and all(t.device.type == "cpu" and t.dtype == torch.float32 and torch.equal(t, ref[k]) for k, t in sd0.items())
    x, _ = batch(2, 24)
    plain = v.encode_moments(x)
    other = {("module." + k): t * 1.5 for k, t in sd0.items()}
    params = v.parameters()
    v.load_state_dict(other)
    assert all(a is b for a, b in zip(params, v.parameters()))              # the leaves stay: an optimiser over them stays valid
    assert all(torch.equal(t, sd0[k] * 1.5) for k, t in v.state_dict().items())
    with torch.no_grad():
        assert torch.equal(v.encode_moments(x), fresh("fp32", {k: t * 1.5 for k, t in sd0.items()}).encode_moments(x))
    v.load_state_dict(sd0)
    with torch.no_grad():
        assert torch.equal(v.encode_moments(x), plain)
    with pytest.raises(KeyError):
        v.load_state_dict({k: t for k, t in sd0.items() if k != "decoder.0.bias"})
    with pytest.raises(ValueError):
        v.load_state_dict(dict(sd0, **{"decoder.0.bias": torch.zeros(3)}))


def test_save_and_resume_continue_bitwise(tmp_path):
    from ldmseg_amd.checkpoint import load_ae_checkpoint
    from ldmseg_amd.optim import AdamW
    from ldmseg_amd.trainers import TrainerAE
    x, targets = batch(2, 24)
    path = str(tmp_path / "model.pt")
    va = fresh("fp32")
    ta = TrainerAE(va, **LOSS_KW)
    oa = AdamW(va.parameters(), lr=LR, weight_decay=0.02)
    for i in range(2):
        step(ta, x, targets, oa, 1.0, i)
    ta.save(path, oa, epoch=3, step=2, p={"optimizer_kwargs": {"lr": LR}, "clip_grad": 1.0})
    saved = va.state_dict()
    # a fresh object from the ORIGINAL state dict and a fresh optimiser with other hyper-parameters
    vb = fresh("fp32")
    tb = TrainerAE(vb, **LOSS_KW)
    ob = AdamW(vb.parameters(), lr=0.5, weight_decay=0.0)
    assert tb.resume(path, ob) == (3, 2)
    assert ob.param_groups[0]["lr"] == LR and ob.param_groups[0]["weight_decay"] == 0.02
    vals_a, vals_b = step(ta, x, targets, oa, 1.0, 2), step(tb, x, targets, ob, 1.0, 2)
    assert all(torch.equal(a, b) for a, b in zip(vals_a, vals_b))
    assert torch.equal(ta.last_grad_norm, tb.last_grad_norm)
    for k, (p, q) in enumerate(zip(va.parameters(), vb.parameters())):
        assert torch.equal(p, q), k
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[p][m], ob.state[q][m]), (k, m)
        assert oa.state[p]["step"] == ob.state[q]["step"] == 3
    # the file: the reference's keys, read by the tensors-only loader and by load_ae_checkpoint
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(data) == ["epoch", "opt", "p", "scaler", "step", "vae"] and data["scaler"] is None and data["p"]["clip_grad"] == 1.0
    ck = load_ae_checkpoint(path)
    assert list(ck) == list(saved) and all(torch.equal(ck[k], saved[k]) for k in saved)
    # our 'opt' entry loads into torch's optimiser over same-shaped tensors, and carries on there
    qs = [torch.zeros_like(t).requires_grad_(True) for t in saved.values()]
    topt = torch.optim.AdamW(qs)
    topt.load_state_dict(data["opt"])
    assert topt.param_groups[0]["lr"] == LR and float(topt.state[qs[0]]["step"]) == 2.0
    for q in qs:
        q.grad = torch.ones_like(q)
    topt.step()
    assert float(topt.state[qs[0]]["step"]) == 3.0
    # without an optimiser only the weights come back
    vc = fresh("fp32")
    assert TrainerAE(vc, **LOSS_KW).resume(path) == (3, 2)
    assert all(torch.equal(a, b) for a, b in zip(vc.state_dict().values(), saved.values()))

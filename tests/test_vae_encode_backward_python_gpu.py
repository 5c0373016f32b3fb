"""The Python surface of the encoder's backward (ldmseg_amd/models/vae.py, trainers/trainer_ae.py): encode / forward under grad mode,
encoder_parameters(), parameters(), refresh(), the differentiable posterior, the composition with the stage-1 point loss, three SGD
steps on BOTH halves against the fp64 restatement, and TrainerAE.training_step.

The three SGD steps use cross entropy on the logits plus the KL term, as tests/test_vae_backward_python_gpu.py does for the decoder
half: the point sampler's importance selection reads the logits, so its point sets cannot be pinned between fp32 and fp64."""
import pytest
import torch
import torch.nn.functional as F

import vae_backward_ref as RD
import vae_backward_run as G
import vae_encode_backward_ref as R
import vae_encode_backward_run as E

pytestmark = pytest.mark.gpu
NAME = "seg"


def fresh(mode, sd=None):
    from ldmseg_amd.models import GeneralVAESeg
    return GeneralVAESeg(sd if sd is not None else R.state_dict(NAME), device=G.DEV, compute_dtype=mode, scaling_factor=0.2, **R.CONFIGS[NAME])


def dev_gen(seed):
    return torch.Generator(device=G.DEV).manual_seed(seed)


@pytest.mark.parametrize("mode", R.MODES)
def test_encode_under_grad_is_bitwise_the_no_grad_encode_and_autograd_is_the_entry(mode):
    B, H = 2, 24
    x, gm = R.inputs(NAME, B, H)
    xs = G.dev(x) * 2 - 1
    v = fresh(mode)
    plain = v.encode_moments(xs)
    assert not plain.requires_grad
    assert not v.encode_moments(xs).requires_grad                    # nothing opted in: as before, grad mode or not
    params = v.encoder_parameters()
    assert list(params) == R.encoder_keys(R.CONFIGS[NAME])
    assert all(p.is_leaf and p.requires_grad and p.is_cuda and p.dtype == torch.float32 for p in params.values())
    mom = v.encode_moments(xs)
    assert mom.requires_grad and torch.equal(mom.detach(), plain)
    with torch.no_grad():
        assert not v.encode_moments(xs).requires_grad
    gs = torch.autograd.grad(mom, list(params.values()), G.dev(gm))
    direct = E.encode_backward(v, NAME, x, gm, list(params))
    r64 = R.reference(NAME, B, H)
    for k, g in zip(params, gs):
        assert torch.equal(g, direct[k]), k
        assert R.metric(g, r64[k]) < R.BOUND, k
    assert len(v.parameters()) == 34 and all(a is b for a, b in zip(v.parameters(), params.values()))


def test_bf16_object_refuses_the_encoder_graph():
    v = fresh("bf16")
    x = G.dev(R.inputs(NAME, 1, 16)[0]) * 2 - 1
    assert not v.encode_moments(x).requires_grad
    v.encoder_parameters()
    with pytest.raises(NotImplementedError):
        v.encode_moments(x)


@pytest.mark.parametrize("with_noise", [True, False])
def test_posterior_sample_and_mode_are_differentiable(with_noise):
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    mom, _, gz = R.posterior_case()
    m = G.dev(mom).requires_grad_(True)
    d = DiagonalGaussianDistribution(m)
    plain = DiagonalGaussianDistribution(m.detach())
    if with_noise:
        z, z0 = d.sample(generator=dev_gen(4)), plain.sample(generator=dev_gen(4))
        noise = torch.randn(z.shape, generator=dev_gen(4), device=G.DEV).cpu()
    else:
        z, z0, noise = d.mode(), plain.mode(), None
    assert z.requires_grad and not z0.requires_grad and torch.equal(z.detach(), z0)
    g, = torch.autograd.grad(z, [m], G.dev(gz))
    assert R.metric(g, R.posterior_reference(mom, noise, gz)) < 1e-5


def test_posterior_gradients_match_the_reference_modules_fixture():
    """the saved noise of tests/golden/vae_encode_backward.npz through the autograd function sample() uses: z and the gradient of the
    moments equal what the reference's own DiagonalGaussianDistribution returned; mode(): (grad_z | exact zeros)"""
    import os
    import numpy as np
    from conftest import GOLDEN
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution, _PosteriorFunction
    fx = np.load(os.path.join(GOLDEN, "vae_encode_backward.npz"))
    gz = G.dev(torch.from_numpy(fx["post/grad_z"]))
    m = G.dev(torch.from_numpy(fx["post/moments"])).requires_grad_(True)
    d = DiagonalGaussianDistribution(m)
    z = _PosteriorFunction.apply(d, m, G.dev(torch.from_numpy(fx["post/noise"])))
    assert R.metric(z, torch.from_numpy(fx["post/z"])) < 1e-5
    g, = torch.autograd.grad(z, [m], gz)
    want = torch.from_numpy(fx["post/grad_moments"])
    assert R.metric(g, want) < 1e-5
    assert torch.equal(g.cpu() == 0, want == 0)                  # the clamp's mask, bounds included
    g0, = torch.autograd.grad(d.mode(), [m], gz)
    assert torch.equal(g0[:, :4], gz) and torch.count_nonzero(g0[:, 4:]) == 0


def _batch(B, H, seed=5, classes=12):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, classes, (B, H // 8, H // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    bits = torch.stack([(ids >> i) % 2 for i in range(7)], dim=1).float()
    return bits, ids


def test_point_loss_backward_fills_all_34_gradients_and_equals_the_entries_by_hand():
    """compute_point_loss(vae(x, sample_posterior=True), targets)[0].backward(): the moments' gradient is the posterior's backward of
    grad_z (from the decoder entry) plus the KL term's, one fp32 addition of two terms (commutative: bitwise), and every encoder
    .grad is ldmseg_vae_encode_backward of it, bitwise"""
    from ldmseg_amd import _lib
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    from ldmseg_amd.trainers import TrainerAE
    v = fresh("fp32")
    B, H = 2, 32
    bits, ids = _batch(B, H)
    x, targets = G.dev(2.0 * bits - 1.0), ids.to(G.DEV)
    tr = TrainerAE(v, loss_weights={"ce": 1.0, "mask": 1.0, "kl": 0.01},
                   loss_kwargs=dict(num_points=64, oversample_ratio=3, importance_sample_ratio=0.75, temperature=1.0))
    params = v.parameters()
    enc, dec = v.encoder_parameters(), v.decoder_parameters()
    out = v(x, sample_posterior=True, generator=dev_gen(9))
    mom = out.posterior.parameters
    assert out.sample.requires_grad and mom.requires_grad
    out.sample.retain_grad()
    mom.retain_grad()
    tr.compute_point_loss(out, targets, generator=torch.Generator().manual_seed(3))[0].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and torch.count_nonzero(p.grad) > 0 for p in params)
    # by hand
    noise = torch.randn((B, 4, H // 8, H // 8), generator=dev_gen(9), device=G.DEV)
    z = DiagonalGaussianDistribution(mom.detach()).sample(generator=dev_gen(9))
    d = G.decode_backward(v, z, out.sample.grad, list(dec))
    for k, p in dec.items():
        assert torch.equal(p.grad, d[k]), k
    gm1 = torch.empty_like(mom)
    _lib.check(_lib.lib().ldmseg_vae_posterior_backward(G.P(mom.detach()), G.P(noise), 1.0, B, H // 8, G.P(d["z"]), G.P(gm1), None), "posterior_backward")
    m2 = mom.detach().clone().requires_grad_(True)
    (0.01 * DiagonalGaussianDistribution(m2).kl(return_mean=True)[1]).backward()
    gm = gm1 + m2.grad
    assert torch.equal(mom.grad, gm)
    e = E.encode_backward(v, NAME, bits, gm, list(enc))
    for k, p in enc.items():
        assert torch.equal(p.grad, e[k]), k


def _restatement_losses(sd0, x, targets, noises, lr, kl_w):
    """fp64: three SGD steps on all 34 tensors of loss = CE(decode(sample(encode(x)))) + kl_w * mean KL; the losses before each
    step and after the last"""
    from collections import OrderedDict
    from oracle import vae as o_vae
    cfg = R.CONFIGS[NAME]
    sd = OrderedDict((k, v.detach().double().clone().requires_grad_(True)) for k, v in sd0.items())
    opt = torch.optim.SGD(list(sd.values()), lr=lr)

    def loss_of(noise):
        mom = o_vae.encode_moments(sd, x.double())
        mean, logvar = mom[:, :4], torch.clamp(mom[:, 4:], -30.0, 20.0)
        z = mean + torch.exp(0.5 * logvar) * noise.double()
        kl = 0.5 * torch.sum(mean.pow(2) + logvar.exp() - 1.0 - logvar, dim=[1, 2, 3])
        return F.cross_entropy(RD.decode(sd, z, cfg), targets) + kl_w * kl.mean()
    losses = []
    for i in range(3):
        opt.zero_grad()
        loss = loss_of(noises[i])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(loss_of(noises[3])))
    return losses, sd


SGD_LR, KL_W = 0.01, 0.01                      # at 0.05 the restatement's loss no longer falls at every step


@pytest.mark.parametrize("mode", R.MODES)
def test_three_sgd_steps_on_both_halves_follow_the_fp64_restatement(mode):
    torch.set_num_threads(16)
    B, H = 2, 24
    bits, _ = _batch(B, H, seed=8)
    g = torch.Generator().manual_seed(4243)
    targets = torch.randint(0, R.CONFIGS[NAME]["out_channels"], (B, H // 2, H // 2), generator=g)
    x = 2.0 * bits - 1.0
    xd, td = G.dev(x), targets.to(G.DEV)
    # the same seeded noise at every step (a fixed objective) and on both sides: what sample() draws from a device generator of that seed
    noises = [torch.randn((B, 4, H // 8, H // 8), generator=dev_gen(100), device=G.DEV).cpu()] * 4
    want, _ = _restatement_losses(R.state_dict(NAME), x, targets, noises, SGD_LR, KL_W)
    v = fresh(mode)
    params = v.parameters()
    assert len(params) == 34
    opt = torch.optim.SGD(params, lr=SGD_LR)

    def loss_of(i):
        out = v(xd, sample_posterior=True, generator=dev_gen(100))
        return F.cross_entropy(out.sample, td) + KL_W * out.posterior.kl(return_mean=True)[1]
    losses = []
    for i in range(3):
        opt.zero_grad()
        loss = loss_of(i)
        loss.backward()
        opt.step()
        with pytest.raises(RuntimeError, match="refresh_encoder"):
            v.encode_moments(xd)                                 # modified in place and not refreshed: a stale handle is refused
        v.refresh()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(loss_of(3)))
        last = v.encode_moments(xd)
    print(f"{mode} losses {losses} restatement {want}")
    assert all(b < a for a, b in zip(want, want[1:])), want
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    for a, b in zip(losses, want):
        assert abs(a - b) <= 1e-3 * abs(b), (losses, want)
    # after refresh() the object equals, bitwise, a fresh object built from the updated state dict: forward and backward
    sd = dict(R.state_dict(NAME))
    sd.update({k: p.detach().cpu() for k, p in list(v.encoder_parameters().items()) + list(v.decoder_parameters().items())})
    w = fresh(mode, sd)
    with torch.no_grad():
        assert torch.equal(w.encode_moments(xd), last)
        z = w.encode(xd).latent_dist.mode()
        assert torch.equal(w.decode(z, interpolate=False), v.decode(z, interpolate=False))
    gm = R.inputs(NAME, B, H)[1]
    keys = list(v.encoder_parameters())
    a, b = E.encode_backward(v, NAME, bits, gm, keys), E.encode_backward(w, NAME, bits, gm, keys)
    for k in keys:
        assert torch.equal(a[k], b[k]), k                        # the data-gradient packings were refreshed too


def test_training_step_updates_every_parameter_clips_and_leaves_a_fresh_handle():
    """TrainerAE.training_step on the point loss (its point sets follow the logits, so the values are not compared with a
    restatement here: the gradients behind them are, in the tests above)"""
    from ldmseg_amd.trainers import TrainerAE
    v = fresh("fp32")
    B, H = 2, 32
    bits, ids = _batch(B, H)
    x, targets = G.dev(2.0 * bits - 1.0), ids.to(G.DEV)
    tr = TrainerAE(v, loss_weights={"ce": 1.0, "mask": 1.0, "kl": 1e-4},
                   loss_kwargs=dict(num_points=64, oversample_ratio=3, importance_sample_ratio=0.75, temperature=1.0))
    params = v.parameters()
    before = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=0.05)

    def norm():
        return float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in params)))
    for step in range(3):
        # the step's own gradient by hand (same seeds; every kernel is bitwise repeatable): its norm, before any clipping
        out = v(x, sample_posterior=True, generator=dev_gen(20 + step))
        tr.compute_point_loss(out, targets, generator=torch.Generator().manual_seed(step))[0].backward()
        unclipped = norm()
        assert unclipped > 0
        clip = 0.5 * unclipped                                   # so the step HAS to clip
        vals = tr.training_step(x, targets, opt, clip_grad=clip, generator=dev_gen(20 + step), point_generator=torch.Generator().manual_seed(step))
        assert len(vals) == 4 and all(t.is_cuda and t.dim() == 0 and not t.requires_grad and torch.isfinite(t) for t in vals)
        assert abs(norm() - clip) <= 1e-4 * clip, (norm(), clip)  # clip_grad_norm_ ran before the step: the kept .grad is the clipped one
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params))
    v.encode_moments(x)                                          # refreshed: no stale-handle error
    v.decode(torch.zeros(1, 4, 2, 2, device=G.DEV), interpolate=False)

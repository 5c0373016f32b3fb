"""The Python surface of the decoder's backward (ldmseg_amd/models/vae.py): decode / forward under grad mode, decoder_parameters(),
refresh_decoder(), the composition with the stage-1 point loss and three SGD steps against the fp64 restatement."""
import pytest
import torch
import torch.nn.functional as F

import vae_backward_ref as R
import vae_backward_run as G

pytestmark = pytest.mark.gpu


def fresh(name, mode, sd=None):
    from ldmseg_amd.models import GeneralVAESeg
    return GeneralVAESeg(sd if sd is not None else R.state_dict(name), device=G.DEV, compute_dtype=mode, scaling_factor=0.2,
                         **R.CONFIGS[name])


@pytest.mark.parametrize("mode", R.MODES)
def test_decode_under_grad_is_bitwise_the_no_grad_decode_and_its_gradients_match(mode):
    name, B, L = "seg", 2, 3
    z, gl = R.inputs(name, B, L)
    v = fresh(name, mode)
    with torch.no_grad():
        plain = v.decode(G.dev(z), interpolate=False)
        plain2 = v.decode(G.dev(z), interpolate=True)
    params = v.decoder_parameters()
    assert list(params) == R.decoder_keys(R.CONFIGS[name])
    assert all(p.is_leaf and p.requires_grad and p.is_cuda and p.dtype == torch.float32 for p in params.values())
    zz = G.dev(z).requires_grad_(True)
    out = v.decode(zz, interpolate=False)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    gs = torch.autograd.grad(out, [zz] + list(params.values()), G.dev(gl))
    direct = G.decode_backward(v, z, gl, list(params))
    r64 = R.reference(name, B, L)
    for k, g in zip(["z"] + list(params), gs):
        assert torch.equal(g, direct[k]), k
        assert R.metric(g, r64[k]) < R.BOUND, k
    # interpolate=True under grad: torch's own resize on top, differentiated by torch
    out2 = v.decode(zz, interpolate=True)
    assert out2.shape == plain2.shape and R.metric(out2.detach(), plain2.double().cpu()) < 1e-5
    g2, = torch.autograd.grad(out2.sum(), [zz])
    ref2 = R.autograd_grads(name, z, torch.full_like(gl, 4.0), torch.float64)["z"]     # d sum(x2(y)) / dy = 4: the weights a source pixel gets sum to 4
    assert R.metric(g2, ref2) < R.BOUND
    # only z requires grad and no parameters were asked for: still a graph
    w = fresh(name, mode)
    o = w.decode(zz, interpolate=False)
    assert torch.equal(torch.autograd.grad(o, [zz], G.dev(gl))[0], direct["z"])
    with torch.no_grad():
        assert not v.decode(zz, interpolate=False).requires_grad


def test_bf16_object_refuses_a_graph():
    v = fresh("seg", "bf16")
    z = G.dev(R.inputs("seg", 1, 2)[0])
    assert not v.decode(z, interpolate=False).requires_grad           # no graph asked for: as before
    with pytest.raises(NotImplementedError):
        v.decode(z.clone().requires_grad_(True), interpolate=False)
    v.decoder_parameters()
    with pytest.raises(NotImplementedError):
        v.decode(z, interpolate=False)


def test_point_loss_backward_composes_with_the_decoder_backward():
    """compute_point_loss(vae(x), targets)[0].backward() on an fp32 object: the .grad of every decoder parameter equals, bitwise, the
    point loss's own logits gradient fed to ldmseg_vae_decode_backward directly"""
    from ldmseg_amd.trainers import TrainerAE
    name = "seg"
    v = fresh(name, "fp32")
    params = v.decoder_parameters()
    g = torch.Generator().manual_seed(5)
    B, H = 2, 32
    ids = torch.randint(0, 12, (B, H // 8, H // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    bits = torch.stack([(ids >> i) % 2 for i in range(7)], dim=1).float()
    x = G.dev(2.0 * bits - 1.0)
    targets = ids.to(G.DEV)
    tr = TrainerAE(v, loss_weights={"ce": 1.0, "mask": 1.0, "kl": 0.0},
                   loss_kwargs=dict(num_points=64, oversample_ratio=3, importance_sample_ratio=0.75, temperature=1.0))
    gen = torch.Generator().manual_seed(3)
    out = v(x, sample_posterior=True, generator=torch.Generator(device=G.DEV).manual_seed(9))
    assert out.sample.requires_grad
    out.sample.retain_grad()
    total = tr.compute_point_loss(out, targets, generator=gen)[0]
    total.backward()
    glogits = out.sample.grad
    assert glogits is not None and torch.count_nonzero(glogits) > 0
    # the latents the forward drew: the same generator seed again
    z = v.encode(x).latent_dist.sample(generator=torch.Generator(device=G.DEV).manual_seed(9))
    direct = G.decode_backward(v, z, glogits, list(params), want_z=False)
    for k, p in params.items():
        assert p.grad is not None and torch.equal(p.grad, direct[k]), k


@pytest.mark.parametrize("mode", R.MODES)
def test_three_sgd_steps_follow_the_fp64_restatement(mode):
    name, B, L = R.SGD_SHAPE
    want = R.sgd_reference()
    z, targets = R.sgd_inputs()
    zd, td = G.dev(z), targets.to(G.DEV)
    v = fresh(name, mode)
    params = v.decoder_parameters()
    opt = torch.optim.SGD(list(params.values()), lr=R.SGD_LR)
    losses = []
    for _ in range(R.SGD_STEPS):
        opt.zero_grad()
        loss = F.cross_entropy(v.decode(zd, interpolate=False), td)
        loss.backward()
        opt.step()
        with pytest.raises(RuntimeError, match="refresh_decoder"):
            v.decode(zd, interpolate=False)                   # modified in place and not refreshed: a stale handle is refused
        v.refresh_decoder()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        last = v.decode(zd, interpolate=False)
        losses.append(float(F.cross_entropy(last, td)))
    print(f"{mode} losses {losses} restatement {want}")
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    for a, b in zip(losses, want):
        assert abs(a - b) <= 1e-3 * abs(b), (losses, want)
    # after refresh_decoder() the object equals, bitwise, a fresh object built from the updated state dict
    sd = dict(R.state_dict(name))
    sd.update({k: p.detach().cpu() for k, p in params.items()})
    w = fresh(name, mode, sd)
    with torch.no_grad():
        assert torch.equal(w.decode(zd, interpolate=False), last)
        assert torch.equal(w.decode(zd, interpolate=True), v.decode(zd, interpolate=True))
    gl = R.inputs(name, B, L)[1]
    a, b = G.decode_backward(v, z, gl, list(params)), G.decode_backward(w, z, gl, list(params))
    for k in a:
        assert torch.equal(a[k], b[k]), k                        # the data-gradient packings were refreshed too

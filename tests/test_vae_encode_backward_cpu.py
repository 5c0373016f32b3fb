"""CPU suite of the seg-VAE encoder's backward: the reference the GPU tests compare with (tests/vae_encode_backward_ref.py) is pinned to
gradients the reference's own GeneralVAESeg and DiagonalGaussianDistribution returned (tests/golden/vae_encode_backward.npz, written
by tests/golden/make_golden_vae_encode_backward.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import vae_encode_backward_ref as R

PIN = 1e-5          # of max|g|: the bound the decoder's restatement is pinned with


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "vae_encode_backward.npz"))


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(os.path.join(GOLDEN, "vae_encode_backward.npz")) < 300 * 1024
    keys = R.encoder_keys(R.CONFIGS["seg"])
    assert len(keys) == 20
    for k in keys:
        assert ("grad/" + k in fx.files) != ("sample/" + k in fx.files), k
    assert int(fx["B"]) == 2 and int(fx["H"]) == 16
    lv = fx["post/moments"][:, 4:]
    assert (lv == -30).any() and (lv == 20).any() and (lv < -30).any() and (lv > 20).any() and ((lv > -30) & (lv < 20)).any()


def test_restatement_gradients_equal_the_reference_modules(fx):
    B, H, stride = int(fx["B"]), int(fx["H"]), int(fx["stride"])
    x, gm = R.inputs("seg", B, H)
    assert np.array_equal(x.numpy(), fx["x"]) and np.array_equal(gm.numpy(), fx["grad_moments"])
    for dtype in (torch.float32, torch.float64):
        got = R.autograd_grads("seg", x, gm, dtype)
        assert set(got) == set(R.encoder_keys(R.CONFIGS["seg"]))
        for k, g in got.items():
            g = g.double().reshape(-1).numpy()
            if "grad/" + k in fx.files:
                want = fx["grad/" + k].astype(np.float64).reshape(-1)
                assert np.abs(g - want).max() <= PIN * np.abs(want).max(), (k, dtype)
            else:
                want, peak = fx["sample/" + k].astype(np.float64), float(fx["max/" + k])
                assert np.abs(g[::stride] - want).max() <= PIN * peak, (k, dtype)
                assert abs(g.sum() - float(fx["sum/" + k])) <= PIN * peak * g.size ** 0.5 * 4, (k, dtype)
                assert abs(np.abs(g).sum() - float(fx["abssum/" + k])) <= PIN * float(fx["abssum/" + k]), (k, dtype)


def test_posterior_restatement_equals_the_reference_distribution(fx):
    mom, _, gz = R.posterior_case()
    assert np.array_equal(mom.numpy(), fx["post/moments"]) and np.array_equal(gz.numpy(), fx["post/grad_z"])
    noise = torch.from_numpy(fx["post/noise"])
    got = R.posterior_reference(mom, noise, gz).numpy()
    want = fx["post/grad_moments"].astype(np.float64)
    assert np.abs(got - want).max() <= PIN * np.abs(want).max()
    # the clamp passes gradient on its bounds and nowhere outside (torch.clamp's rule, which the kernel restates)
    lv = fx["post/moments"][:, 4:]
    assert np.all(want[:, 4:][(lv < -30) | (lv > 20)] == 0) and np.all(want[:, 4:][(lv == -30) | (lv == 20)] != 0)
    assert np.array_equal(want[:, :4], fx["post/grad_z"].astype(np.float64))
    assert np.count_nonzero(R.posterior_reference(mom, None, gz)[:, 4:].numpy()) == 0


def test_fp64_reference_is_far_inside_the_bound():
    """torch's fp32 CPU autograd against the fp64 reference - the reference's own error - is orders below the 1e-3 gate"""
    for name, B, H in (("seg", 1, 16), ("reduced", 2, 24)):
        r64, r32 = R.reference(name, B, H), R.reference_fp32(name, B, H)
        for k in r64:
            assert R.metric(r32[k], r64[k]) < 1e-5, (name, B, H, k)

"""CPU suite of the seg-VAE decoder's backward: the reference the GPU tests compare with (tests/vae_backward_ref.py) is pinned to
gradients the reference's own GeneralVAESeg returned (tests/golden/vae_decode_backward.npz, written by
tests/golden/make_golden_vae_decode_backward.py), and the learning rate of the SGD test is checked on the restatement."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import vae_backward_ref as R

PIN = 1e-5          # of max|g|: the bound the CLIP restatements are pinned with


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "vae_decode_backward.npz"))


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(os.path.join(GOLDEN, "vae_decode_backward.npz")) < 300 * 1024
    keys = R.decoder_keys(R.CONFIGS["seg"])
    assert len(keys) == 14
    for k in keys:
        assert ("grad/" + k in fx.files) != ("sample/" + k in fx.files), k
    assert "grad/z" in fx.files and int(fx["B"]) == 2 and int(fx["L"]) == 2


def test_restatement_gradients_equal_the_reference_modules(fx):
    B, L, stride = int(fx["B"]), int(fx["L"]), int(fx["stride"])
    z, gl = R.inputs("seg", B, L)
    assert np.array_equal(z.numpy(), fx["z"]) and np.array_equal(gl.numpy(), fx["grad_logits"])
    for dtype in (torch.float32, torch.float64):
        got = R.autograd_grads("seg", z, gl, dtype)
        for k, g in got.items():
            g = g.double().reshape(-1).numpy()
            if "grad/" + k in fx.files:
                want = fx["grad/" + k].astype(np.float64).reshape(-1)
                assert np.abs(g - want).max() <= PIN * np.abs(want).max(), (k, dtype)
            else:
                want, peak = fx["sample/" + k].astype(np.float64), float(fx["max/" + k])
                assert np.abs(g[::stride] - want).max() <= PIN * peak, (k, dtype)
                # the whole tensor through its sums: n elements, each within PIN * peak
                assert abs(g.sum() - float(fx["sum/" + k])) <= PIN * peak * g.size ** 0.5 * 4, (k, dtype)
                assert abs(np.abs(g).sum() - float(fx["abssum/" + k])) <= PIN * float(fx["abssum/" + k]), (k, dtype)


def test_general_restatement_equals_the_oracle_decoder():
    from oracle import vae as o_vae
    z, _ = R.inputs("seg", 2, 3)
    sd = R.state_dict("seg")
    with torch.no_grad():
        assert torch.equal(R.decode(sd, z, R.CONFIGS["seg"]), o_vae.decode(sd, z, interpolate=False))


def test_fp64_reference_is_far_inside_the_bound():
    """torch's fp32 CPU autograd against the fp64 reference - the reference's own error - is orders below the 1e-3 gate"""
    for name, B, L in R.SHAPES:
        r64, r32 = R.reference(name, B, L), R.reference_fp32(name, B, L)
        assert set(r64) == set(R.decoder_keys(R.CONFIGS[name])) | {"z"}
        for k in r64:
            assert R.metric(r32[k], r64[k]) < 1e-5, (name, B, L, k)


def test_z_scale_enters_the_latent_gradient():
    z, gl = R.inputs("reduced", 2, 3)
    a = R.autograd_grads("reduced", z * 0.5, gl, torch.float64)
    b = R.autograd_grads("reduced", z, gl, torch.float64, z_scale=0.5)
    assert R.metric(b["z"], 0.5 * a["z"]) < 1e-12
    assert R.metric(b["decoder.0.weight"], a["decoder.0.weight"]) < 1e-12


def test_sgd_learning_rate_makes_the_restatements_loss_fall():
    losses = R.sgd_reference()
    assert len(losses) == R.SGD_STEPS + 1
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.5 * losses[0]              # a real descent, not a rounding-level one

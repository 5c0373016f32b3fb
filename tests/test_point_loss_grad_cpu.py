"""CPU suite of the stage-1 loss's backward: (i) the fixture tests/golden/point_loss_grad.npz (the reference's own gradients under
CPU autograd, written by tests/golden/make_golden_point_loss_grad.py) holds the cases; (ii) the torch restatement
tests/point_loss_ref.py under autograd reproduces every fixture gradient - so the fixture and the rules the kernels follow
(rows, tie rule, effective targets, draw order) describe the same function; (iii) the autograd path refuses CPU tensors like the
forward; (iv) the new entries are declared, bound and exported."""
import math
import os
import re

import pytest
import torch

import point_loss_grad_cases as G
import point_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldmseg_point_loss_backward", "ldmseg_point_loss_backward_scratch_bytes", "ldmseg_gaussian_kl_backward")
# fp32 autograd of the same ops in other summation shapes; measured <= 1.33e-7 over the ten cases of point_loss.npz
RESTATEMENT_BOUND = 1e-6


@pytest.fixture(scope="module")
def gold(golden):
    return golden("point_loss.npz")


@pytest.fixture(scope="module")
def grad(golden):
    return golden("point_loss_grad.npz")


def test_grad_fixture_case_list(gold, grad):
    assert [str(n) for n in grad["cases"]] == G.CASES
    assert [str(n) for n in grad["cases"]][:10] == [str(n) for n in gold["cases"]]
    assert [str(n) for n in grad["kl_cases"]] == [str(n) for n in gold["kl_cases"]] == ["small", "clamped"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "point_loss_grad.npz")) < 1_000_000
    by = {n: G.load_case(gold, grad, n) for n in G.CASES}
    for n, case in by.items():
        assert case["grad_ce"].shape == case["x"].shape and case["grad_mask"].shape == case["x"].shape, n
        assert bool(torch.isfinite(case["grad_ce"]).all()) and bool(torch.isfinite(case["grad_mask"]).all()), n
    assert tuple(by["tiny_map"]["x"].shape) == (2, 16, 4, 4) and tuple(by["tiny_map"]["targets"].shape) == (2, 16, 16)
    assert by["tiny_map"]["P"] == 64
    assert tuple(by["one_channel_wide"]["x"].shape) == (1, 3, 5, 37) and by["one_channel_wide"]["P"] == 33
    assert torch.equal(by["saturated"]["x"], by["base"]["x"] * 8) and torch.equal(by["saturated"]["targets"], by["base"]["targets"])
    # no kept point: the forward's ce is NaN, its gradient is all zeros
    assert math.isnan(float(by["no_segment"]["ce"]))
    assert not by["no_segment"]["grad_ce"].any() and not by["no_segment"]["grad_mask"].any()
    # the CE row and the mask rows of an image write the same planes
    both = (by["tiny_map"]["grad_ce"] != 0) & (by["tiny_map"]["grad_mask"] != 0)
    assert int(both.sum()) > 0
    for n in grad["kl_cases"]:
        assert grad[f"kl/{n}/grad_moments"].shape == gold[f"kl/{n}/moments"].shape


@pytest.mark.parametrize("name", G.CASES)
def test_restatement_under_autograd_reproduces_the_reference(gold, grad, name):
    case = G.load_case(gold, grad, name)
    ce, mask, g_ce, g_mask = G.restatement_grads(case)
    for tag, got, want in (("ce", g_ce, case["grad_ce"]), ("mask", g_mask, case["grad_mask"])):
        dev = G.rel_dev(got, want)
        print(f"{name}/{tag}: max|g_ref| {float(want.abs().max()):.3e} rel {dev:.3e}")
        assert dev <= RESTATEMENT_BOUND, (name, tag, dev)
        assert not bool(got[want == 0].any()), (name, tag, "a pixel the reference leaves untouched is not exactly 0")
    if name == "no_segment":
        assert math.isnan(float(ce)) and not g_ce.any() and not g_mask.any()


def test_restatement_kl_gradient(gold, grad):
    for name in grad["kl_cases"]:
        mom = torch.from_numpy(gold[f"kl/{name}/moments"]).clone().requires_grad_(True)
        got = torch.autograd.grad(R.gaussian_kl(mom).mean(), mom)[0]
        want = torch.from_numpy(grad[f"kl/{name}/grad_moments"])
        assert G.rel_dev(got, want) <= RESTATEMENT_BOUND, name
        lv = mom.detach()[:, 4:]
        outside = (lv < -30.0) | (lv > 20.0)
        assert not bool(want[:, 4:][outside].any()), name
    lv = torch.from_numpy(gold["kl/clamped/moments"])[:, 4:]
    assert bool((lv > 20.0).any()) and bool((lv < -30.0).any())                                 # the case reaches both clamps


def test_autograd_path_refuses_cpu_tensors():
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    from ldmseg_amd.trainers import SegmentationLosses
    crit = SegmentationLosses(num_points=8)
    x = torch.zeros(1, 2, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError):
        crit.point_loss(x, torch.zeros(1, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError):
        DiagonalGaussianDistribution(torch.zeros(1, 8, 2, 2, requires_grad=True)).kl()


def test_new_entries_are_declared_bound_and_exported():
    from ldmseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ldmseg_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["ldmseg_point_loss_backward"][1]) == 27
    # sizes the call refuses need no scratch; otherwise room for every tap of every row and two counters per pixel
    assert lib.ldmseg_point_loss_backward_scratch_bytes(0, 16, 8, 8, 0, 48, 64) == 0
    assert lib.ldmseg_point_loss_backward_scratch_bytes(2, 129, 8, 8, 0, 48, 64) == 0
    assert lib.ldmseg_point_loss_backward_scratch_bytes(2, 16, 32, 32, 22, 48, 64) >= 24 * 64 * 4 * 8 + 2 * 32 * 32 * 8
    # argument checks answer before anything touches a device
    args = [None, 1, 16, 8, 8, None, None, 8, 8, None, 0, None, None, None, None, None, 0, 0, 4, 0, 1.0, 1.0, None, None, None, None,
            None]
    assert lib.ldmseg_point_loss_backward(*args) == -1 and b"null" in lib.ldmseg_last_error()
    assert lib.ldmseg_gaussian_kl_backward(None, 1, 4, 64, None, None, None) == -1


def test_the_forward_path_records_nothing_without_requires_grad():
    """`point_loss`, `kl` and `compute_point_loss` carry no blanket no_grad any more: the decision is made per call, inside."""
    import inspect
    from ldmseg_amd.trainers import SegmentationLosses, TrainerAE
    from ldmseg_amd.trainers import losses
    assert hasattr(losses, "_PointLossFunction") and issubclass(losses._PointLossFunction, torch.autograd.Function)
    src = inspect.getsource(SegmentationLosses.point_loss)
    assert "requires_grad" in src and "is_grad_enabled" in src
    assert not inspect.getsource(TrainerAE.compute_point_loss).lstrip().startswith("@torch.no_grad")

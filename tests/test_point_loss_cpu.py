"""CPU suite of the seg-VAE's stage-1 loss: (i) the tap rule of csrc/point_sample.h (through ldmseg_op_point_taps) is
F.grid_sample's, indices exactly and weights to the bit; (ii) the draw plan of SegmentationLosses.point_loss has the reference's
shapes and order (recorded in tests/golden/point_loss.npz by tests/golden/make_golden_point_loss.py); (iii) the torch
restatement tests/point_loss_ref.py, fed the draws of that plan, reproduces the reference's values and selected index sets;
(iv) the new entries are declared, bound and exported."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_loss_ref as R


@pytest.fixture(scope="module")
def gold(golden):
    return golden("point_loss.npz")


def taps(u, H, W, mode):
    from ldmseg_amd import _lib
    u = np.ascontiguousarray(u, dtype=np.float32)
    n = u.shape[0]
    idx = np.full((n, 4) if mode == 0 else (n,), -7, dtype=np.int32)
    w = np.zeros((n, 4), dtype=np.float32)
    rc = _lib.lib().ldmseg_op_point_taps(n, u.ctypes.data_as(C.POINTER(C.c_float)), H, W, mode,
                                         idx.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return idx, w


def tap_points(H, W, seed):
    """random u, u at 0, u at the largest float below 1, pixel centres, half-integer positions (pixel corners)"""
    g = torch.Generator().manual_seed(seed)
    below1 = float(np.nextafter(np.float32(1), np.float32(0)))
    pts = [torch.rand(300, 2, generator=g)]
    edge = torch.tensor([0.0, below1, 0.5])
    pts.append(torch.cartesian_prod(edge, edge))
    cx, cy = (torch.arange(W) + 0.5) / W, (torch.arange(H) + 0.5) / H                # pixel centres: position = integer
    pts.append(torch.cartesian_prod(cx, cy))
    kx, ky = torch.arange(1, W).float() / W, torch.arange(1, H).float() / H          # corners: position = integer + 0.5
    pts.append(torch.cartesian_prod(kx, ky))
    pts.append(torch.stack([torch.rand(40, generator=g), ky[torch.randint(0, H - 1, (40,), generator=g)]], dim=1))
    return torch.cat(pts).float().contiguous()


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8), (24, 40), (33, 31), (64, 48)])
def test_tap_rule_matches_grid_sample(H, W):
    u = tap_points(H, W, H * 100 + W)
    n = u.shape[0]
    # bilinear: a one-hot plane per pixel makes grid_sample return that pixel's weight itself
    eye = torch.eye(H * W).view(1, H * W, H, W)
    want = R.sample(eye, u[None])[0]                                                 # [HW, n]
    idx, w = taps(u.numpy(), H, W, 0)
    got = torch.zeros(H * W, n)
    for k in range(4):
        inside = idx[:, k] >= 0
        cols = torch.arange(n)[torch.from_numpy(inside)]
        got[torch.from_numpy(idx[inside, k].astype(np.int64)), cols] += torch.from_numpy(w[inside, k])
    # (the four taps of a point are distinct pixels, so each entry holds one weight; a zero weight may carry either sign)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert (idx[:, 0] == -1).any() and (idx[:, 3] == -1).any()                       # taps outside the map occur and are dropped
    # nearest: the map of linear indices + 1, so that 0 is 'outside'
    ramp = (torch.arange(H * W, dtype=torch.float32) + 1).view(1, 1, H, W)
    want_n = R.sample(ramp, u[None], mode="nearest")[0, 0].long() - 1
    got_n, _ = taps(u.numpy(), H, W, 1)
    assert np.array_equal(got_n.astype(np.int64), want_n.numpy())


def test_tap_rule_rejects_bad_arguments():
    from ldmseg_amd import _lib
    buf = (C.c_int32 * 4)()
    u = (C.c_float * 2)(0.5, 0.5)
    w = (C.c_float * 4)()
    lib = _lib.lib()
    assert lib.ldmseg_op_point_taps(1, u, 0, 4, 0, buf, w) != 0
    assert lib.ldmseg_op_point_taps(1, u, 4, 4, 2, buf, w) != 0
    assert lib.ldmseg_op_point_taps(1, u, 4, 4, 0, buf, None) != 0
    assert lib.ldmseg_op_point_taps(1, None, 4, 4, 1, buf, None) != 0


def draws_for(case, device="cpu"):
    from ldmseg_amd.trainers.losses import draw_plan
    plan = draw_plan(case["x"].shape[0], case["num_masks"], case["P"], case["ratio"], case["isr"])
    g = torch.Generator().manual_seed(case["seed"])
    return plan, {name: torch.rand(shape, generator=g).to(device) for name, shape in plan}


def test_draw_plan_matches_the_reference_draws(gold):
    for name in gold["cases"]:
        case = R.load_case(gold, str(name))
        plan, _ = draws_for(case)
        assert [shape for _, shape in plan] == case["draw_shapes"], name
    from ldmseg_amd.trainers.losses import draw_plan
    assert draw_plan(2, 0, 64, 3, 0.75) == [("ce_over", (2, 192, 2)), ("ce_fresh", (2, 16, 2))]
    assert draw_plan(2, 5, 64, 0, 0.75) == [("ce_fresh", (2, 64, 2)), ("mask_fresh", (5, 64, 2))]
    with pytest.raises(ValueError):
        draw_plan(2, 5, 64, 0.5, 0.75)


def test_restatement_reproduces_the_reference(gold):
    """The rules the kernels follow (rows, tie rule, draw order, effective targets), in torch ops on the CPU, against the
    reference's own values: the losses to 1e-6 relative (same ops, other summation shapes) and the selected sets exactly."""
    for name in gold["cases"]:
        case = R.load_case(gold, str(name))
        _, draws = draws_for(case)
        out = R.point_loss(case["x"], case["targets"], case["masks"], draws, case["P"], case["ratio"], case["isr"],
                           case["temperature"], case["ignore"])
        assert int(out["rows"].numel()) == case["num_masks"], name
        for tag in ("ce", "mask"):
            want = float(case[tag])
            got = float(out[tag])
            if math.isnan(want):
                assert math.isnan(got), name
            elif want == 0.0:
                assert got == 0.0, name
            else:
                assert abs(got - want) <= 1e-6 * abs(want), (name, tag, got, want)
            if tag in case["selected"]:
                assert np.array_equal(out["selected_" + tag].numpy(), case["selected"][tag]), (name, tag)
            else:
                assert out["selected_" + tag] is None
    for name in gold["kl_cases"]:
        mom = torch.from_numpy(gold[f"kl/{name}/moments"])
        assert torch.allclose(R.gaussian_kl(mom), torch.from_numpy(gold[f"kl/{name}/per_image"]), rtol=1e-6, atol=0)


def test_fixture_holds_the_cases_and_the_gap(gold):
    names = [str(n) for n in gold["cases"]]
    assert len(names) >= 10
    by = {n: R.load_case(gold, n) for n in names}
    assert tuple(by["base"]["x"].shape) == (2, 16, 32, 32) and tuple(by["base"]["targets"].shape) == (2, 64, 48)
    assert by["odd_points"]["P"] == 257 and by["odd_points"]["selected"]["ce"].shape[1] == 192
    assert tuple(by["c128"]["x"].shape) == (3, 128, 24, 40) and tuple(by["c128"]["targets"].shape) == (2 + 1, 48, 80)
    assert by["ratio0"]["ratio"] == 0 and not by["ratio0"]["selected"]
    assert by["valid_mask"]["masks"] is not None and by["temperature"]["temperature"] == 0.5 and by["all_uncertain"]["isr"] == 1.0
    assert math.isnan(float(by["no_segment"]["ce"])) and float(by["no_segment"]["mask"]) == 0.0 and by["no_segment"]["num_masks"] == 0
    assert (by["one_empty"]["targets"][1] == 0).all()
    # the threshold gap, recomputed with the restatement's uncertainties
    for n, case in by.items():
        if not case["selected"]:
            continue
        _, draws = draws_for(case)
        x, kU = case["x"], int(case["isr"] * case["P"])
        top = torch.topk(R.sample(x, draws["ce_over"]), 2, dim=1)[0]
        rows_unc = [top[:, 1] - top[:, 0]]
        if case["num_masks"]:
            rows = R.mask_rows(R.effective_targets(case["targets"], case["masks"], case["ignore"]), x.shape[1], case["ignore"])
            xm = x[rows // x.shape[1], rows % x.shape[1]][:, None]
            rows_unc.append(-R.sample(xm, draws["mask_over"])[:, 0].abs())
        for unc in rows_unc:
            v = torch.sort(unc, dim=1, descending=True)[0]
            a, b = v[:, kU - 1], v[:, kU]
            assert bool(((a - b) > 1e-4 * torch.clamp(torch.maximum(a.abs(), b.abs()), min=1.0)).all()), n


def test_surface_of_the_new_entries():
    from ldmseg_amd import _lib
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    from ldmseg_amd.trainers import SegmentationLosses, TrainerAE
    for name in ("ldmseg_point_loss", "ldmseg_point_loss_scratch_bytes", "ldmseg_class_presence", "ldmseg_gaussian_kl",
                 "ldmseg_op_point_taps"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    lib = _lib.lib()
    assert lib.ldmseg_point_loss_scratch_bytes(0, 192, 48, 64) == 0
    assert lib.ldmseg_point_loss_scratch_bytes(24, 192, 48, 64) >= 24 * (4 * 8 + 192 * 4 + 48 * 4)
    # argument checks answer before anything touches a device
    assert lib.ldmseg_point_loss(None, 1, 16, 8, 8, None, None, 8, 8, None, 0, None, None, None, None, 0, 0, 4, 0, 1.0, 1.0, None,
                                 None, None, None) == -1
    assert b"null" in lib.ldmseg_last_error()
    assert lib.ldmseg_class_presence(None, None, 1, 8, 8, 16, 0, None, None, None) == -1
    assert lib.ldmseg_gaussian_kl(None, 1, 4, 64, None, None, None) == -1
    sig = inspect.signature(SegmentationLosses.point_loss)
    assert list(sig.parameters)[1:] == ["outputs", "targets", "do_matching", "masks", "generator", "return_points"]
    crit = SegmentationLosses()
    assert (crit.num_points, crit.oversample_ratio, crit.importance_sample_ratio, crit.ignore_label, crit.temperature) == \
        (12544, 3, 0.75, 0, 1.0)
    with pytest.raises(NotImplementedError):
        crit.point_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long), do_matching=True)
    with pytest.raises(RuntimeError):
        crit.point_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))        # CPU tensors: no fallback
    assert list(inspect.signature(TrainerAE.compute_point_loss).parameters)[1:] == ["outputs", "targets", "do_matching", "masks",
                                                                                    "generator"]
    assert hasattr(TrainerAE, "validation_loss") and hasattr(DiagonalGaussianDistribution, "kl")
    tr = TrainerAE(None, device="cpu")
    assert tr.loss_weights == {"mask": 1.0, "ce": 1.0, "kl": 0.0}
    assert tr.segmentation_losses.num_points == 12544 and tr.segmentation_losses.ignore_label == 0
    tr = TrainerAE(None, device="cpu", ignore_label=5, loss_kwargs=dict(num_points=8, ignore_label=2))
    assert tr.segmentation_losses.ignore_label == 5 and tr.segmentation_losses.num_points == 8     # the trainer's label counts

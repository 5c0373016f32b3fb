"""CPU suite of the denoising loss: (i) the torch restatement tests/diffusion_loss_ref.py reproduces every array the
reference's own compute_loss / get_loss_weight_mask / predict_sample returned (tests/golden/diffusion_loss.npz, written by
tests/golden/make_golden_loss.py) - element losses, masks and pred_latents bit for bit, scalar losses within 1e-6 relative;
(ii) the nearest-resize source index of csrc/nearest_index.h (through ldmseg_op_nearest_index) is F.interpolate's choice."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diffusion_loss_ref as R


@pytest.fixture(scope="module")
def g(golden):
    return golden("diffusion_loss.npz")


def parse_case(key):
    shape, kind, ptype, weight, m, p, o = key.split("/")
    return shape, kind, ptype, weight, int(m[1:]), int(p[1:]), float(o[1:])


def shape_inputs(g, shape):
    return {k: torch.from_numpy(g[f"{shape}/{k}"]) for k in ("t", "latents", "original", "rgb", "noise", "loss_mask", "paste",
                                                             "noisy", "prediction")}


def test_fixture_covers_the_issue_cases(g):
    cases = [parse_case(k) for k in g["loss_cases"]]
    for col, values in ((1, R.LOSS_KINDS), (2, ("epsilon", "sample")), (3, ("none", "max_clamp_snr")), (4, (0, 1)), (5, (0, 1)),
                        (6, (1.0, 0.5))):
        for shape in ("a", "b"):
            assert {c[col] for c in cases if c[0] == shape} == set(values), (shape, col)
    assert g["a/latents"].shape == (2, 4, 8, 8) and g["b/latents"].shape == (3, 4, 24, 24)
    for shape in ("a", "b"):
        t = g[f"{shape}/t"]
        assert len(set(t.tolist())) == len(t) and 0 in t and 999 in t
        assert not g[f"{shape}/loss_mask"][-1].any() and g[f"{shape}/loss_mask"][0].any()
    assert len(g["mask_cases"]) == 3 * 2 * 4 and len(g["predict_cases"]) == 4


def test_restatement_reproduces_the_reference_losses(g):
    sa, sb = torch.from_numpy(g["sqrt_a"]), torch.from_numpy(g["sqrt_b"])
    net = R.StandIn(g["standin_w"])
    weights = {"none": torch.ones(1000), "max_clamp_snr": torch.from_numpy(g["weights_max_clamp_snr"])}
    for key in g["loss_cases"]:
        shape, kind, ptype, weight, mask, paste, ohem = parse_case(key)
        x = shape_inputs(g, shape)
        assert torch.equal(R.add_noise(x["latents"], x["noise"], x["t"], sa, sb), x["noisy"])
        loss, elem, pl, prediction = R.compute_loss(
            net, x["noise"], x["t"], x["noisy"], x["rgb"], x["loss_mask"] if mask else None, kind, ptype, sa, sb,
            weights=weights[weight], latents=x["latents"], original=x["original"], paste_mask=x["paste"] if paste else None,
            ohem_ratio=ohem)
        assert torch.equal(prediction, x["prediction"]), key
        ek = f"{shape}/elem/{kind}/{ptype}/{weight}/m{mask}"
        assert np.array_equal(elem.numpy(), g[ek]), key
        assert np.array_equal(R.exact_sample_sums(elem), g[ek + "/sums"]), key
        assert np.array_equal(pl.numpy(), g[f"{shape}/pred_latents/{ptype}/p{paste}"]), key
        ref = float(g[key + "/loss"])
        assert abs(loss - ref) <= 1e-6 * abs(ref), (key, loss, ref)


def test_restatement_reproduces_the_reference_masks(g):
    for key in g["mask_cases"]:
        _, name, size, type_mask, ignore = key.split("/")
        src = g[f"mask/{name}/padding"] if type_mask == "padding" else g[f"mask/{name}/targets"]
        out = R.loss_weight_mask(torch.from_numpy(src), (int(size), int(size)), type_mask, int(ignore))
        assert out.dtype == torch.float32 and np.array_equal(out.numpy(), g[key]), key
    assert R.loss_weight_mask(torch.zeros(1, 4, 4), (2, 2), "other") is None
    # the fixture's own edge cases: an image that is all ignore_label, ids up to 255
    assert not g["mask/s32/8/counts/0"][1].any() and g["mask/s32/targets"].max() == 255


def test_restatement_reproduces_the_reference_predict_sample(g):
    sa, sb = torch.from_numpy(g["sqrt_a"]), torch.from_numpy(g["sqrt_b"])
    net = R.StandIn(g["standin_w"])
    for key in g["predict_cases"]:
        _, shape, ptype = key.split("/")
        lat, rgb = torch.from_numpy(g[f"{shape}/latents"]), torch.from_numpy(g[f"{shape}/rgb"])
        out = R.predict_sample(net, lat, rgb, torch.from_numpy(g[key + "/noise"]), torch.from_numpy(g[key + "/t"]), sa, sb, ptype)
        assert np.array_equal(out.numpy(), g[key + "/pred"]), key
        if ptype == "epsilon":      # the clamp is at work: remove_noise at a large t leaves the latents' range
            assert float(out.min()) == float(lat.min()) and float(out.max()) == float(lat.max())


def test_fixture_timesteps_have_correctly_rounded_roots(g):
    """torch's `** 0.5` is not the correctly rounded square root at a few of the 1000 table entries, the device's square root at
    about a quarter of them (tests/golden/device_sqrt_differs.json).  Every timestep of the fixture lies where all three agree,
    so the GPU can meet it bit for bit."""
    exact = g["sqrt_exact"]
    assert exact.sum() > 700
    ac = g["alphas_cumprod"]
    assert np.array_equal(g["sqrt_a"][exact], np.sqrt(ac)[exact])
    ts = [g["a/t"], g["b/t"]] + [g[k + "/t"] for k in g["predict_cases"]]
    assert all(exact[t].all() for t in ts)


def test_nearest_index_header_matches_torch():
    from ldmseg_amd import _lib
    lib = _lib.lib()
    for out_size in (8, 24, 64):
        buf = (C.c_int * out_size)()
        for in_size in range(1, 131):
            assert lib.ldmseg_op_nearest_index(in_size, out_size, buf) == 0
            ramp = torch.arange(in_size, dtype=torch.float32).view(1, 1, in_size, 1)
            want = F.interpolate(ramp, size=(out_size, 1), mode="nearest").view(-1).long().tolist()
            assert list(buf) == want, (in_size, out_size)
            assert R.nearest_index(in_size, out_size).tolist() == want, (in_size, out_size)
    assert lib.ldmseg_op_nearest_index(0, 8, buf) != 0 and lib.ldmseg_op_nearest_index(8, 8, None) != 0


def test_trainer_surface():
    """the reference's method names and the new constructor keywords with base.yaml's defaults"""
    import inspect
    from ldmseg_amd.trainers.sampler import TrainerDiffusion
    sig = inspect.signature(TrainerDiffusion.__init__).parameters
    for name, default in (("training_loss_type", "l2"), ("rgb_noise_level", 0), ("cond_noise_level", 0), ("ohem_ratio", 1.0),
                          ("type_mask", "ignore"), ("prob_train_on_pred", 0.0), ("prob_inpainting", 0.0), ("min_noise_level", 0),
                          ("sample_posterior", False), ("ignore_label", 0)):
        assert sig[name].default == default, name
    want = {"loss_fn": ["x", "y", "reduction", "mask"],
            "compute_loss": ["noise", "timesteps", "noisy_latents", "rgb_latents", "encoder_hidden_states", "loss_mask", "latents",
                             "original_latents", "inpainting_masks", "condition"],
            "predict_sample": ["latents", "rgb_latents", "encoder_hidden_states", "tmax"],
            "get_loss_weight_mask": ["targets", "ignore_label", "mode", "size", "device", "type_mask", "padding_mask"],
            "process_inputs": ["data"], "validation_loss": ["dataloader", "timesteps", "seed", "max_iter"]}
    for name, params in want.items():
        got = list(inspect.signature(getattr(TrainerDiffusion, name)).parameters)[1:]
        assert got[:len(params)] == params, (name, got)

"""GPU suite of the seg-VAE's stage-1 loss (csrc/point_loss.hip, SegmentationLosses.point_loss, DiagonalGaussianDistribution.kl,
TrainerAE.compute_point_loss / validation_loss, tools/main_ae_eval.py --val-loss) against the values the reference's own
functions returned on the CPU (tests/golden/point_loss.npz, written by tests/golden/make_golden_point_loss.py).

Deviation of ce / mask / kl from the reference's values, measured on an MI355X over every fixture case (largest relative
deviation): see REL_BOUND below."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import point_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured on an MI355X, largest relative deviation over the fixture: mask 1.520e-7 (case 'base'), ce 1.397e-7 ('valid_mask'),
# kl 7.767e-8 ('clamped', image 0) - one unit in the last place of the fp32 result each; 15 of the 25 finite values are equal to the
# bit.  The bound is 2x the largest.  The reference's own losses move by under 1e-6 when its logits are perturbed by 1e-5
# relative, so nothing above 1e-5 could pass as rounding.
REL_BOUND = 3.04e-7


@pytest.fixture(scope="module")
def gold(golden):
    return golden("point_loss.npz")


def criterion(case):
    from ldmseg_amd.trainers import SegmentationLosses
    return SegmentationLosses(num_points=case["P"], oversample_ratio=case["ratio"], importance_sample_ratio=case["isr"],
                              ignore_label=case["ignore"], temperature=case["temperature"])


def run(case, seed=None, return_points=True, masks="case"):
    g = torch.Generator().manual_seed(case["seed"] if seed is None else seed)
    m = case["masks"] if isinstance(masks, str) else masks
    return criterion(case).point_loss(case["x"], case["targets"], masks=m, generator=g, return_points=return_points)


def check_value(got, want, what):
    got, want = float(got), float(want)
    if math.isnan(want):
        assert math.isnan(got), what
        return 0.0
    if want == 0.0:
        assert got == 0.0, what
        return 0.0
    dev = abs(got - want) / abs(want)
    print(f"{what}: got {got!r} want {want!r} rel {dev:.3e}")
    assert dev <= REL_BOUND, (what, got, want, dev)
    return dev


CASES = ["base", "odd_points", "c128", "ratio0", "valid_mask", "one_empty", "no_segment", "temperature", "all_uncertain", "ignore3"]


def test_fixture_case_list(gold):
    assert sorted(str(n) for n in gold["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_point_loss_against_the_reference(gold, name):
    case = R.load_case(gold, name, DEV)
    out = run(case)
    B, N = case["x"].shape[0], case["num_masks"]
    assert out["ce"].dim() == 0 and out["mask"].dim() == 0 and out["ce"].is_cuda
    assert int(out["rows"].numel()) == N
    if case["selected"]:
        sel = out["selected"].cpu().numpy()
        assert sel.shape[0] == B + N
        assert np.array_equal(sel[:B], case["selected"]["ce"]), "cross-entropy rows select another set"
        if N:
            assert np.array_equal(sel[B:], case["selected"]["mask"]), "mask rows select another set"
    else:
        assert out["selected"] is None
    check_value(out["ce"], case["ce"], f"{name}/ce")
    check_value(out["mask"], case["mask"], f"{name}/mask")
    # rows follow prepare_targets: by image, then ascending class id
    eff = R.effective_targets(case["targets"], case["masks"], case["ignore"])
    assert torch.equal(out["rows"].long(), R.mask_rows(eff, case["x"].shape[1], case["ignore"]).cpu())


def test_gaussian_kl_against_the_reference(gold):
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    for name in gold["kl_cases"]:
        mom = torch.from_numpy(gold[f"kl/{name}/moments"]).to(DEV)
        per, mean = DiagonalGaussianDistribution(mom).kl(return_mean=True)
        want = gold[f"kl/{name}/per_image"]
        assert per.shape == (mom.shape[0],) and mean.dim() == 0
        for b in range(mom.shape[0]):
            check_value(per[b], want[b], f"kl/{name}/{b}")
        check_value(mean, gold[f"kl/{name}/mean"], f"kl/{name}/mean")
        assert torch.equal(DiagonalGaussianDistribution(mom).kl(), per)


def test_bad_ids_and_cpu_tensors_are_refused(gold):
    case = R.load_case(gold, "base", DEV)
    bad = case["targets"].clone()
    bad[0, 3, 5] = case["x"].shape[1]                                   # an id == C
    with pytest.raises(ValueError):
        criterion(case).point_loss(case["x"], bad)
    bad[0, 3, 5] = -2
    with pytest.raises(ValueError):
        criterion(case).point_loss(case["x"], bad)
    with pytest.raises(RuntimeError):
        criterion(case).point_loss(case["x"].cpu(), case["targets"].cpu())
    with pytest.raises(RuntimeError):
        criterion(case).point_loss(case["x"], case["targets"].cpu())
    with pytest.raises(NotImplementedError):
        criterion(case).point_loss(case["x"], case["targets"], do_matching=True)


def test_targets_are_not_modified_and_calls_repeat_bitwise(gold):
    case = R.load_case(gold, "valid_mask", DEV)
    before = case["targets"].clone()
    a = run(case)
    assert torch.equal(case["targets"], before)
    b = run(case)
    for k in ("ce", "mask", "bce", "dice"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(a["selected"], b["selected"])
    # the mask changes what both terms see: without it the same draws give other values
    c = run(case, masks=None)
    assert float(c["ce"]) != float(a["ce"]) and float(c["mask"]) != float(a["mask"])
    # a device generator is accepted too (another stream of numbers, same shapes)
    g = torch.Generator(device=DEV).manual_seed(3)
    d = criterion(case).point_loss(case["x"], case["targets"], masks=case["masks"], generator=g)
    assert math.isfinite(float(d["ce"])) and math.isfinite(float(d["mask"])) and set(d) == {"ce", "mask"}


@pytest.mark.parametrize("P", [64, 257])
def test_ties_at_the_threshold_go_to_the_lower_index(gold, P):
    """All-zero logits: every sample is 0 (also next to the border, where zero padding enters), so every uncertainty of every
    row is the same value and the whole selection is decided by the tie rule: the kU lowest indices (P = 257: kU = 192 of
    S = 771, several points per thread of the compaction)."""
    from ldmseg_amd.trainers import SegmentationLosses
    case = R.load_case(gold, "base", DEV)
    x = torch.zeros_like(case["x"])
    out = SegmentationLosses(num_points=P).point_loss(x, case["targets"], generator=torch.Generator().manual_seed(1),
                                                      return_points=True)
    kU = int(0.75 * P)
    sel = out["selected"].cpu()
    assert sel.shape == (2 + case["num_masks"], kU)
    assert torch.equal(sel, torch.arange(kU, dtype=torch.int32).expand_as(sel))
    # and the cross entropy of uniform logits over C classes is log C at every kept point
    assert abs(float(out["ce"]) - math.log(x.shape[1])) <= 1e-6 * math.log(x.shape[1])


def test_c_entry_checks_its_arguments(gold):
    from ldmseg_amd import _lib
    case = R.load_case(gold, "base", DEV)
    x, t = case["x"], case["targets"]
    lib, P = _lib.lib(), _lib.ptr
    out = torch.zeros(3, device=DEV)
    scratch = torch.zeros(int(lib.ldmseg_point_loss_scratch_bytes(2, 192, 48, 64)), dtype=torch.uint8, device=DEV)
    over, fresh = torch.rand(2, 192, 2, device=DEV), torch.rand(2, 16, 2, device=DEV)

    def call(S=192, kU=48, Pn=64, temp=1.0, C=16, ce_over=over):
        return lib.ldmseg_point_loss(P(x), 2, C, 32, 32, P(t), None, 64, 48, None, 0, P(ce_over), P(fresh), None, None, S, kU, Pn, 0,
                                     temp, 1.0, P(out), None, P(scratch), None)
    assert call() == 0
    torch.cuda.synchronize()
    assert math.isfinite(float(out[0])) and float(out[1]) == 0.0 and float(out[2]) == 0.0
    assert call(kU=65) == -1 and call(S=40) == -1 and call(temp=0.0) == -1 and call(ce_over=None) == -1
    assert call(C=129) == -2 and b"LDMSEG_POINT_LOSS_MAX_C" in lib.ldmseg_last_error()


@pytest.fixture(scope="module")
def trainer(vae_sd):
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.trainers import TrainerAE
    vae = GeneralVAESeg(vae_sd, device=DEV, compute_dtype="fp32")
    return TrainerAE(vae, device=DEV, loss_weights={"mask": 0.5, "ce": 2.0, "kl": 0.125},
                     loss_kwargs=dict(num_points=96, oversample_ratio=3, importance_sample_ratio=0.75))


def test_compute_point_loss_through_the_vae(trainer):
    """64 x 64 maps through a real GeneralVAESeg: compute_point_loss = point_loss + kl on the model's own outputs, weighted."""
    from ldmseg_amd.data.bitcodec import encode_bitmap
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 9, (2, 8, 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).to(DEV)
    bits, _ = encode_bitmap(ids, n=7, fill_value=0.5, ignore_label=0)
    out = trainer.vae_model(2. * bits - 1., sample_posterior=False)
    assert tuple(out.sample.shape) == (2, 128, 32, 32)
    total, ce, kl, mask = trainer.compute_point_loss(out, ids, generator=torch.Generator().manual_seed(9))
    parts = trainer.segmentation_losses.point_loss(out.sample, ids, generator=torch.Generator().manual_seed(9))
    assert torch.equal(ce, parts["ce"]) and torch.equal(mask, parts["mask"])
    want_kl = R.gaussian_kl(out.posterior.parameters.double()).mean()
    assert abs(float(kl) - float(want_kl)) <= 1e-6 * abs(float(want_kl))
    assert torch.equal(total, 2.0 * ce + 0.125 * kl + 0.5 * mask) or \
        abs(float(total) - (2.0 * float(ce) + 0.125 * float(kl) + 0.5 * float(mask))) <= 1e-6 * abs(float(total))
    # and the restatement on the same logits and draws
    crit = trainer.segmentation_losses
    from ldmseg_amd.trainers.losses import draw_plan
    rows = R.mask_rows(ids, 128, 0)
    gg = torch.Generator().manual_seed(9)
    draws = {n: torch.rand(s, generator=gg).to(DEV) for n, s in draw_plan(2, int(rows.numel()), 96, 3, 0.75)}
    ref = R.point_loss(out.sample, ids, None, draws, 96, 3, 0.75, crit.temperature, 0)
    assert abs(float(ce) - float(ref["ce"])) <= 1e-5 * abs(float(ref["ce"]))
    assert abs(float(mask) - float(ref["mask"])) <= 1e-5 * abs(float(ref["mask"]))
    # validation_loss: image-weighted means of the four values, one read
    batch = {"image_semseg": bits, "semseg": ids}
    val = trainer.validation_loss([batch, batch], seed=9)
    assert val["images"] == 4 and all(math.isfinite(val[k]) for k in ("loss", "ce", "kl", "mask"))
    assert abs(val["kl"] - float(kl)) <= 1e-6 * abs(float(kl))
    assert abs(val["loss"] - (2.0 * val["ce"] + 0.125 * val["kl"] + 0.5 * val["mask"])) <= 1e-6 * abs(val["loss"])
    with pytest.raises(ValueError):
        trainer.validation_loss([])


def test_main_ae_eval_val_loss_subprocess(tmp_path):
    from PIL import Image
    from ldmseg_amd.evaluations import id2rgb
    gt_dir = tmp_path / "pan"
    gt_dir.mkdir()
    rs = np.random.RandomState(12)
    for i, (h, w) in enumerate([(60, 80), (64, 64)]):
        gt = np.kron(rs.randint(0, 5, (4, 4)), np.ones((h // 4 + 1, w // 4 + 1), np.int64))[:h, :w] * 700
        Image.fromarray(id2rgb(gt)).save(gt_dir / f"{i:03d}.png")
    argv = [sys.executable, os.path.join(ROOT, "tools", "main_ae_eval.py"), "--panoptic", str(gt_dir), "--size", "64", "--batch", "2",
            "--dtype", "bf16", "--val-loss"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "latent-diffusion-segmentation_amd")]))
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    val = json.loads(lines[0])["val_loss"]
    assert val["images"] == 2 and all(math.isfinite(val[k]) and val[k] >= 0 for k in ("loss", "ce", "kl", "mask"))
    assert "mIoU" in r.stdout and "PQ " in r.stdout

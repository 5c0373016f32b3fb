"""GPU suite of the stage-1 loss's backward (csrc/point_loss_bwd.hip, ldmseg_point_loss_backward, ldmseg_gaussian_kl_backward,
the autograd path of SegmentationLosses.point_loss, DiagonalGaussianDistribution.kl and TrainerAE.compute_point_loss) against the
gradients the reference's own functions gave under CPU autograd (tests/golden/point_loss_grad.npz, written by
tests/golden/make_golden_point_loss_grad.py).

Deviation from the reference's gradients, max|got - ref| / max|ref| per case and term, measured on an MI355X: see REL_BOUND."""
import math

import pytest
import torch

import point_loss_grad_cases as G
import point_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# measured on an MI355X, largest max|got - ref| / max|ref| over the 13 cases x {ce, mask} and the two kl cases: 2.244e-7
# ('saturated', ce; next 'c128' mask 1.523e-7, 'one_channel_wide' mask 1.511e-7; kl 2.7e-8; 'no_segment' exactly 0).  The bound
# is twice the largest - the margin tests/test_point_loss_gpu.py gives the forward values, for the same reason: the same fp32
# terms added in another order.  Anything above 1e-5 would be a bug, not rounding.
MEASURED_MAX = 2.244e-7
REL_BOUND = 2 * MEASURED_MAX
# conv -> loss -> conv weight gradient on the GPU against the CPU: worst-case relative error of a K-term fp32 dot product is
# K * 2^-24; the conv forward has K = 8 * 9 = 72 (4.3e-6, carried through a loss gradient whose slope in the logits is below 1),
# the weight gradient sums B * H * W = 512 terms (3.1e-5).  Sum of the two worst cases, rounded up.
GRAPH_BOUND = 4e-5


@pytest.fixture(scope="module")
def gold(golden):
    return golden("point_loss.npz")


@pytest.fixture(scope="module")
def grad(golden):
    return golden("point_loss_grad.npz")


@pytest.fixture(scope="module")
def cases(gold, grad):
    """every case on the device, loaded once and left unchanged"""
    return {n: G.load_case(gold, grad, n, DEV) for n in G.CASES}


def criterion(case):
    from ldmseg_amd.trainers import SegmentationLosses
    return SegmentationLosses(num_points=case["P"], oversample_ratio=case["ratio"], importance_sample_ratio=case["isr"],
                              ignore_label=case["ignore"], temperature=case["temperature"])


def run(case, x, **kw):
    return criterion(case).point_loss(x, case["targets"], masks=case["masks"], generator=torch.Generator().manual_seed(case["seed"]),
                                      **kw)


def both_grads(case):
    """-> (losses, d ce / d x, d mask / d x) through autograd; a term without a graph (no mask row) gives zeros"""
    x = case["x"].clone().requires_grad_(True)
    out = run(case, x)
    grads = []
    for tag in ("ce", "mask"):
        assert out[tag].requires_grad and out[tag].grad_fn is not None, tag
        g = torch.autograd.grad(out[tag], x, retain_graph=True, allow_unused=True)[0]
        grads.append(torch.zeros_like(x) if g is None else g)
    return out, grads[0], grads[1]


@pytest.mark.parametrize("name", G.CASES)
def test_gradients_against_the_reference(cases, name):
    case = cases[name]
    out, g_ce, g_mask = both_grads(case)
    plain = run(case, case["x"])
    assert plain["ce"].grad_fn is None and not plain["ce"].requires_grad
    for tag in ("ce", "mask"):                       # the differentiable call returns the plain call's bits
        assert torch.equal(out[tag].detach().view(torch.int32), plain[tag].view(torch.int32)), tag
    for tag, got, want in (("ce", g_ce, case["grad_ce"]), ("mask", g_mask, case["grad_mask"])):
        got = got.cpu()
        assert got.shape == want.shape and got.dtype == torch.float32
        assert bool(torch.isfinite(got).all()), (name, tag)
        dev = G.rel_dev(got, want)
        print(f"{name}/{tag}: max|g_ref| {float(want.abs().max()):.3e} rel {dev:.3e}")
        assert dev <= REL_BOUND, (name, tag, dev)
        assert not bool(got[want == 0].any()), (name, tag, "a pixel the reference leaves untouched is not exactly 0")
    if name == "no_segment":
        assert math.isnan(float(out["ce"].detach())) and not g_ce.any() and not g_mask.any()


def c_backward(case, g_ce, g_mask, grad_x=None, x=None, bad=None):
    """The C entry on the forward's own `selected`: -> (code, grad_x).  g_ce / g_mask: floats or None (a NULL pointer)."""
    from ldmseg_amd import _lib
    crit = criterion(case)
    x = case["x"] if x is None else x
    fwd = run(case, x, return_points=True)
    B, C, H, W = x.shape
    tg, valid, rows = crit.class_presence(case["targets"], case["masks"], C)
    N = int(rows.numel())
    assert torch.equal(rows, fwd["rows"])
    P = case["P"]
    S = int(P * case["ratio"]) if case["ratio"] > 0 else 0
    kU = int(case["isr"] * P) if case["ratio"] > 0 else 0
    draws = G.draws_for(case, DEV)
    assert N == case["num_masks"]
    rows_dev = rows.to(DEV) if N else None
    lib, ptr = _lib.lib(), _lib.ptr
    if grad_x is None:
        grad_x = torch.empty_like(x)
    scratch = torch.empty(int(lib.ldmseg_point_loss_backward_scratch_bytes(B, C, H, W, N, kU, P)), dtype=torch.uint8, device=DEV)
    gc = None if g_ce is None else torch.tensor([g_ce], dtype=torch.float32, device=DEV)
    gm = None if g_mask is None else torch.tensor([g_mask], dtype=torch.float32, device=DEV)
    a = dict(C=C, kU=kU, S=S, P=P, B=B, H=H, grad_x=ptr(grad_x))
    a.update(bad or {})
    code = lib.ldmseg_point_loss_backward(
        ptr(x), a["B"], a["C"], a["H"], W, ptr(tg), ptr(valid), tg.shape[1], tg.shape[2], ptr(rows_dev), N, ptr(draws.get("ce_over")),
        ptr(draws.get("ce_fresh")), ptr(draws.get("mask_over")), ptr(draws.get("mask_fresh")), ptr(fwd["selected"]), a["S"], a["kU"],
        a["P"], case["ignore"], case["temperature"], float(max(N, 1)), ptr(gc), ptr(gm), a["grad_x"], ptr(scratch),
        _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return code, grad_x


@pytest.mark.parametrize("name", ["tiny_map", "one_channel_wide", "base", "no_segment"])
def test_the_call_writes_the_whole_buffer(cases, name):
    """grad_x comes in full of NaN: every element is written, exactly 0.0 where no tap lands."""
    case = cases[name]
    buf = torch.full_like(case["x"], float("nan"))
    code, got = c_backward(case, 1.0, 1.0, grad_x=buf)
    assert code == 0 and got.data_ptr() == buf.data_ptr()
    assert not bool(torch.isnan(got).any())
    untouched = (case["grad_ce"] == 0) & (case["grad_mask"] == 0)
    assert bool((got.cpu()[untouched] == 0.0).all())
    assert int(untouched.sum()) > 0 or name == "tiny_map"
    # and it is what autograd hands out for ce + mask: the same call
    x = case["x"].clone().requires_grad_(True)
    out = run(case, x)
    (out["ce"] + out["mask"]).backward()
    assert torch.equal(x.grad.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("name", ["tiny_map", "c128"])
def test_two_backward_calls_agree_bitwise(cases, name):
    case = cases[name]
    _, a_ce, a_mask = both_grads(case)
    _, b_ce, b_mask = both_grads(case)
    assert torch.equal(a_ce.view(torch.int32), b_ce.view(torch.int32))
    assert torch.equal(a_mask.view(torch.int32), b_mask.view(torch.int32))
    _, c1 = c_backward(case, 2.5, 0.25)
    _, c2 = c_backward(case, 2.5, 0.25)
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))


@pytest.mark.parametrize("name", ["base", "tiny_map"])
def test_upstream_gradients(cases, name):
    case = cases[name]
    _, g_ce, g_mask = both_grads(case)
    x = case["x"].clone().requires_grad_(True)
    out = run(case, x)
    (2.5 * out["ce"] + 0.25 * out["mask"]).backward()
    want = 2.5 * g_ce + 0.25 * g_mask
    dev = G.rel_dev(x.grad, want)
    print(f"{name}: 2.5 ce + 0.25 mask against the weighted sum of the two gradients: rel {dev:.3e}")
    assert dev <= REL_BOUND
    # a NULL upstream pointer leaves that term out: the CE gradient alone, the mask gradient alone
    code, only_ce = c_backward(case, 1.0, None)
    assert code == 0 and torch.equal(only_ce.view(torch.int32), g_ce.view(torch.int32))
    code, only_mask = c_backward(case, None, 1.0)
    assert code == 0 and torch.equal(only_mask.view(torch.int32), g_mask.view(torch.int32))
    code, none = c_backward(case, None, None, grad_x=torch.full_like(case["x"], float("nan")))
    assert code == 0 and not bool(none.any())
    # a second backward through the same graph is refused
    x2 = case["x"].clone().requires_grad_(True)
    g1, = torch.autograd.grad(run(case, x2)["ce"], x2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


def test_backward_through_a_torch_graph():
    """Logits from a conv on the GPU, a non-contiguous slice of its output: .backward() fills conv.weight.grad like CPU autograd
    of the restatement on the same weights.  The seed is the first at which the CPU's selection has the fixture's threshold gap,
    so a few ulps between the two convs cannot change the selected set."""
    from ldmseg_amd.trainers import SegmentationLosses
    from ldmseg_amd.trainers.losses import draw_plan
    g = torch.Generator().manual_seed(77)
    conv = torch.nn.Conv2d(8, 16, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.3)
        conv.bias.copy_(torch.randn(16, generator=g) * 0.1)
    inp = torch.randn(2, 8, 16, 20, generator=g)
    targets = torch.randint(0, 6, (2, 4, 4), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    P, ratio, isr = 48, 3, 0.75
    kU = int(isr * P)
    rows = R.mask_rows(targets, 16, 0)
    N = int(rows.numel())

    def cpu_loss(seed):
        gg = torch.Generator().manual_seed(seed)
        draws = {n: torch.rand(s, generator=gg) for n, s in draw_plan(2, N, P, ratio, isr)}
        x = conv(inp)[:, :, :, 2:18]
        return x, draws, R.point_loss(x, targets, None, draws, P, ratio, isr, 1.0, 0)

    def gap_ok(x, draws):
        top = torch.topk(R.sample(x, draws["ce_over"]), 2, dim=1)[0]
        uncs = [top[:, 1] - top[:, 0], -R.sample(x[rows // 16, rows % 16][:, None], draws["mask_over"])[:, 0].abs()]
        for unc in uncs:
            v = torch.sort(unc.detach(), dim=1, descending=True)[0]
            a, b = v[:, kU - 1], v[:, kU]
            if not bool(((a - b) > 1e-4 * torch.clamp(torch.maximum(a.abs(), b.abs()), min=1.0)).all()):
                return False
        return True
    seed = 300
    while True:
        x, draws, ref = cpu_loss(seed)
        if gap_ok(x, draws):
            break
        seed += 1
    assert not x.is_contiguous()
    conv.zero_grad()
    (2.0 * ref["ce"] + 0.5 * ref["mask"]).backward()
    want_w, want_b = conv.weight.grad.clone(), conv.bias.grad.clone()

    gconv = torch.nn.Conv2d(8, 16, 3, padding=1).to(DEV)
    gconv.load_state_dict(conv.state_dict())
    xg = gconv(inp.to(DEV))[:, :, :, 2:18]
    assert not xg.is_contiguous() and xg.requires_grad
    out = SegmentationLosses(num_points=P, oversample_ratio=ratio, importance_sample_ratio=isr).point_loss(
        xg, targets.to(DEV), generator=torch.Generator().manual_seed(seed), return_points=True)
    assert torch.equal(out["selected"][:2].cpu().long(), ref["selected_ce"]) and torch.equal(out["selected"][2:].cpu().long(), ref["selected_mask"])
    assert not out["bce"].requires_grad and not out["dice"].requires_grad
    (2.0 * out["ce"] + 0.5 * out["mask"]).backward()
    dw, db = G.rel_dev(gconv.weight.grad.cpu(), want_w), G.rel_dev(gconv.bias.grad.cpu(), want_b)
    print(f"conv weight grad rel {dw:.3e}, bias grad rel {db:.3e}")
    assert dw <= GRAPH_BOUND and db <= GRAPH_BOUND


def test_kl_gradients_against_the_reference(gold, grad):
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    for name in grad["kl_cases"]:
        mom = torch.from_numpy(gold[f"kl/{name}/moments"]).to(DEV).requires_grad_(True)
        per, mean = DiagonalGaussianDistribution(mom).kl(return_mean=True)
        plain = DiagonalGaussianDistribution(mom.detach()).kl(return_mean=True)
        assert torch.equal(per.detach(), plain[0]) and torch.equal(mean.detach(), plain[1]) and plain[1].grad_fn is None
        got, = torch.autograd.grad(mean, mom, retain_graph=True)
        want = torch.from_numpy(grad[f"kl/{name}/grad_moments"])
        dev = G.rel_dev(got.cpu(), want)
        print(f"kl/{name}: max|g_ref| {float(want.abs().max()):.3e} rel {dev:.3e}")
        assert dev <= REL_BOUND, (name, dev)
        lv = mom.detach().cpu()[:, 4:]
        outside = (lv < -30.0) | (lv > 20.0)
        assert int(outside.sum()) > 0 or name == "small"
        assert not bool(got.cpu()[:, 4:][outside].any()), name
        # per-image values: image 1 alone, weighted
        one, = torch.autograd.grad(3.0 * per[1], mom)
        assert not bool(one[0].any()) and G.rel_dev(one[1].cpu(), 3.0 * mom.shape[0] * want[1]) <= REL_BOUND


def test_compute_point_loss_is_differentiable(cases, gold, grad):
    from ldmseg_amd.models.vae import DiagonalGaussianDistribution
    from ldmseg_amd.trainers import TrainerAE
    from ldmseg_amd.utils import VAEOutput
    case = cases["base"]
    w = {"ce": 2.0, "mask": 0.5, "kl": 0.125}
    tr = TrainerAE(None, num_classes=16, ignore_label=case["ignore"], device=DEV, loss_weights=w,
                   loss_kwargs=dict(num_points=case["P"], oversample_ratio=case["ratio"], importance_sample_ratio=case["isr"],
                                    temperature=case["temperature"]))
    mom0 = torch.from_numpy(gold["kl/small/moments"]).to(DEV)
    x = case["x"].clone().requires_grad_(True)
    mom = mom0.clone().requires_grad_(True)
    seeded = lambda: torch.Generator().manual_seed(case["seed"])
    vals = tr.compute_point_loss(VAEOutput(sample=x, posterior=DiagonalGaussianDistribution(mom)), case["targets"], generator=seeded())
    with torch.no_grad():
        plain = tr.compute_point_loss(VAEOutput(sample=x, posterior=DiagonalGaussianDistribution(mom)), case["targets"],
                                      generator=seeded())
    for a, b in zip(vals, plain):
        assert b.grad_fn is None and torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
    vals[0].backward()
    _, g_ce, g_mask = both_grads(case)
    m2 =mom0.clone().requires_grad_(True)
    g_kl, = torch.autograd.grad(DiagonalGaussianDistribution(m2).kl(return_mean=True)[1], m2)
    dx, dm = G.rel_dev(x.grad, w["ce"] * g_ce + w["mask"] * g_mask), G.rel_dev(mom.grad, w["kl"] * g_kl)
    print(f"total.backward(): logits rel {dx:.3e}, moments rel {dm:.3e}")
    assert dx <= REL_BOUND and dm <= REL_BOUND


def test_c_entry_checks_its_arguments(cases):
    from ldmseg_amd import _lib
    case = cases["base"]
    lib = _lib.lib()
    code, _ = c_backward(case, 1.0, 1.0)
    assert code == 0
    assert c_backward(case, 1.0, 1.0, bad=dict(grad_x=None))[0] == -1 and b"null" in lib.ldmseg_last_error()
    assert c_backward(case, 1.0, 1.0, bad=dict(C=129))[0] == -2 and b"LDMSEG_POINT_LOSS_MAX_C" in lib.ldmseg_last_error()
    assert c_backward(case, 1.0, 1.0, bad=dict(kU=193, P=256))[0] == -1 and b"kU" in lib.ldmseg_last_error()      # kU > S = 192
    assert c_backward(case, 1.0, 1.0, bad=dict(H=-32))[0] == -2 and b"positive" in lib.ldmseg_last_error()
    assert c_backward(case, 1.0, 1.0, bad=dict(B=-2))[0] < 0 and lib.ldmseg_last_error()
    assert c_backward(case, 1.0, 1.0, bad=dict(P=-64))[0] < 0 and lib.ldmseg_last_error()
    mom = torch.zeros(2, 8, 4, 4, device=DEV)
    g = torch.ones(2, device=DEV)
    out = torch.empty_like(mom)
    P = _lib.ptr
    assert lib.ldmseg_gaussian_kl_backward(P(mom), 2, 4, 16, P(g), P(out), None) == 0
    assert lib.ldmseg_gaussian_kl_backward(P(mom), 2, 4, 16, None, P(out), None) == -1
    assert lib.ldmseg_gaussian_kl_backward(P(mom), 2, -4, 16, P(g), P(out), None) == -2
    torch.cuda.synchronize()

"""Per-kernel tests of what the seg-VAE encoder's backward adds: the by-width and stride-2 weight gradients, the
stride-2 data gradient on igemm, silu_bwd and posterior_backward, each operator entry against torch.autograd.grad of the matching
torch op in fp64.  Metric max|g - g64| / max|g64|, bound 1e-3, in the fp32 and the split-bf16 products.

The stride-2 forward serves odd maps (Ho = (H - 1) / 2 + 1), so the backward entries do too: 5 x 7 -> 3 x 4 is the one place where
the bottom and right padding taps are hit (even maps only ever pad top and left)."""
import pytest
import torch
import torch.nn.functional as F

import vae_backward_run as G
import vae_encode_backward_ref as R
from wgrad_cases import NARROW, STRIDE2      # (B, Ci, Co, H, W); the CPU suite reads them too

pytestmark = pytest.mark.gpu
P, dev, DEV = G.P, G.dev, G.DEV


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


_conv_case = R.conv_case          # (shared with tests/test_wgrad_kernels_gpu.py)




@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", NARROW, ids=lambda s: "x".join(map(str, s)))
def test_narrow_weight_gradient_vs_fp64_autograd(lib, shape, mode):
    B, Ci, Co, H, W = shape
    x, w, dy, rx, rw, rb = _conv_case(B, Ci, Co, H, W, 1)
    gw, gb = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV), torch.full((Co,), float("nan"), device=DEV)
    x_, dy_ = dev(x), dev(dy)                                    # (kept alive: the entry takes raw pointers)
    (_, names) = G.logged(lambda: G._ok(lib, lib.ldmseg_op_conv_wgrad_ex(P(x_), P(dy_), B, Ci, H, W, Co, 1, G.OP_DTYPE[mode], P(gw), P(gb), None)))
    t = 32 if Co <= 32 else 64
    assert f"wgrad9<{'f32' if mode == 'fp32' else 'x3'},{t},{32 if Ci <= 32 else 64}>/taps9" in names, names      # the all-taps tile
    assert G.report(f"narrow wgrad {shape} {mode}", R.metric(gw, rw)) < R.BOUND
    assert G.report(f"narrow bgrad {shape} {mode}", R.metric(gb, rb)) < R.BOUND


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", STRIDE2, ids=lambda s: "x".join(map(str, s)))
def test_stride2_weight_and_data_gradient_vs_fp64_autograd(lib, shape, mode):
    B, Ci, Co, H, W = shape
    x, w, dy, rx, rw, rb = _conv_case(B, Ci, Co, H, W, 2)
    dt = G.OP_DTYPE[mode]
    gw, gb = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV), torch.full((Co,), float("nan"), device=DEV)
    x_, dy_, w_ = dev(x), dev(dy), dev(w)
    G._ok(lib, lib.ldmseg_op_conv_s2_wgrad(P(x_), P(dy_), B, Ci, H, W, Co, dt, P(gw), P(gb), None))
    assert G.report(f"s2 wgrad {shape} {mode}", R.metric(gw, rw)) < R.BOUND
    assert G.report(f"s2 bgrad {shape} {mode}", R.metric(gb, rb)) < R.BOUND
    if Ci % 4:
        return                                                   # (the data-gradient entry takes Ci in fours: no such layer has one)
    gx = torch.full((B, Ci, H, W), float("nan"), device=DEV)
    G._ok(lib, lib.ldmseg_op_conv_s2_dgrad(P(dy_), P(w_), B, Ci, H, W, Co, dt, P(gx), None))
    assert G.report(f"s2 dgrad {shape} {mode}", R.metric(gx, rx)) < R.BOUND


def test_by_width_equals_the_wide_tile_within_rounding_and_repeats_bitwise(lib):
    """the same sum on the all-taps 32 x 32 tile and on the per-tap 128 x 128 tile (ldmseg_op_conv_wgrad); two launches give
    identical bits, one slice (16^2) or several (2 x 24^2)"""
    for B, H in ((1, 16), (2, 24)):
        x, w, dy, rx, rw, rb = _conv_case(B, 32, 32, H, H, 1)
        x_, dy_ = dev(x), dev(dy)
        for dt in (0, 3):
            outs = []
            for rep in range(2):
                gw, gb = torch.empty(32, 32, 3, 3, device=DEV), torch.empty(32, device=DEV)
                G._ok(lib, lib.ldmseg_op_conv_wgrad_ex(P(x_), P(dy_), B, 32, H, H, 32, 1, dt, P(gw), P(gb), None))
                outs.append((gw, gb))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
            wide = torch.empty(32, 32, 3, 3, device=DEV)
            G._ok(lib, lib.ldmseg_op_conv_wgrad(P(x_), P(dy_), B, 32, H, H, 32, dt, P(wide), None, None))
            assert R.metric(outs[0][0], wide.double().cpu()) < R.BOUND


def test_silu_backward_vs_fp64(lib):
    n = 5 * 256 + 77                                             # no multiple of the block
    g = torch.Generator().manual_seed(3)
    u = (torch.rand(n, generator=g) * 2 - 1) * 30.0
    u[:4] = torch.tensor([0.0, -30.0, 30.0, 1e-4])
    # the ends of the range: exp(-u) overflows fp32 below u = -88.7 (and underflows above 88), and tiny arguments
    ends = torch.tensor([88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4])
    u[4:12] = ends
    u[12:76] = torch.logspace(-30, -20, 64)
    da = torch.randn(n, generator=g)
    ud = u.double().requires_grad_(True)
    ref, = torch.autograd.grad(F.silu(ud), [ud], da.double())
    du, u_, da_ = torch.full((n,), float("nan"), device=DEV), dev(u), dev(da)
    G._ok(lib, lib.ldmseg_op_silu_bwd(P(u_), P(da_), n, P(du), None))
    assert G.report("silu_bwd", R.metric(du, ref)) < 1e-5        # elementwise fp32: a few ulp of the largest value
    sig = torch.sigmoid(u.double())
    assert torch.allclose(ref, da.double() * sig * (1 + u.double() * (1 - sig)))
    du = du.cpu()
    assert torch.isfinite(du).all()
    low, high = u <= -100, u >= 100
    assert low.sum() == 2 and high.sum() == 2
    assert torch.equal(du[low], 0 * da[low])                     # a zero as a number (0 * da: either sign), no NaN from 0 * inf
    assert R.metric(du[high], da[high].double()) < 1e-5


@pytest.mark.parametrize("with_noise", [True, False])
def test_posterior_backward_vs_fp64(lib, with_noise):
    from ldmseg_amd import _lib
    mom, noise, gz = R.posterior_case()
    noise = noise if with_noise else None
    B, l = mom.shape[0], mom.shape[2]
    mom_, noise_, gz_ = dev(mom), dev(noise), dev(gz)
    for scale in (1.0, 0.25):
        ref = R.posterior_reference(mom, noise, gz, scale)
        out = torch.full((B, 8, l, l), float("nan"), device=DEV)
        _lib.check(lib.ldmseg_vae_posterior_backward(P(mom_), P(noise_), scale, B, l, P(gz_), P(out), None), "posterior_backward")
        torch.cuda.synchronize()
        assert G.report(f"posterior_bwd noise={with_noise} scale={scale}", R.metric(out, ref)) < 1e-5
        # where the clamp is saturated (and everywhere for mode()) the logvar half is exact zeros; on the bounds it passes
        lv = mom[:, 4:]
        dead = (lv < -30) | (lv > 20) if with_noise else torch.ones_like(lv, dtype=torch.bool)
        assert dead.any() and torch.all(out[:, 4:].cpu()[dead] == 0)
        if with_noise:
            assert torch.all(out[:, 4:].cpu()[(lv == -30) | (lv == 20)] != 0)
        assert torch.equal(out[:, :4].cpu(), (gz * scale))


def test_refusals(lib):
    t = torch.zeros(64, device=DEV)
    p = P(t)
    assert lib.ldmseg_op_conv_wgrad_ex(p, p, 1, 4, 2, 2, 8, 3, 0, p, p, None) == -2           # stride 1 | 2
    assert lib.ldmseg_op_conv_s2_wgrad(p, p, 1, 4, 2, 2, 8, 1, p, p, None) == -2              # bf16 storage: no backward
    assert lib.ldmseg_op_conv_s2_dgrad(p, p, 1, 6, 2, 2, 8, 0, p, None) == -2                 # Ci a multiple of 4
    assert lib.ldmseg_op_silu_bwd(p, p, 0, p, None) == -2

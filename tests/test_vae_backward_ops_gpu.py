"""Per-kernel tests of the seg-VAE decoder's backward (csrc/vae_bwd.hip and the data gradients on igemm): every operator entry at
the layer shapes of the configurations of tests/vae_backward_ref.py against torch.autograd.grad of the matching torch op in fp64.
Metric max|g - g64| / max|g64|, bound 1e-3, in the fp32 and the split-bf16 products.  The shapes carry the padded-channel cases:
the first conv has 4 input channels below a K tile, the reduced configuration 16 logit channels."""
import pytest
import torch

import vae_backward_ref as R
import vae_backward_run as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def _cases():
    seen, out = set(), []
    for name, B, L in R.ALL_SHAPES:
        for kind, q in G.layers(name, B, L):
            key = (kind, tuple(sorted(q.items())))
            if key not in seen:
                seen.add(key)
                # (the norm backwards have no products: one form serves both modes)
                out += [(kind, q, mode) for mode in (R.MODES if kind in ("conv", "convt") else R.MODES[:1])]
    return out


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("kind,q,mode", _cases(), ids=_id)
def test_backward_operator_vs_fp64_autograd(lib, kind, q, mode):
    torch.set_num_threads(16)
    G.CHECK[kind](lib, q, mode)


def test_layernorm_backward_in_row_order(lib):
    G.check_ln(lib, dict(M=2 * 12 * 12, C=256, H2=12), "fp32", pm=0)


# ---- off the configurations' shapes.  GroupNorm + SiLU backward (B, C, HW): gn_silu_bwd_stats_kernel gives a channel PS = 512 / cpg
# threads - cpg 1 with fewer pixels than PS; cpg 3 and 5, which do not divide 512 (510 of 512 threads active, the idle ones inside
# the tree reduction); cpg 16; one pixel per channel
GN_OFF = [(2, 32, 5), (3, 96, 35), (2, 160, 577), (1, 512, 100), (2, 256, 1)]


@pytest.mark.parametrize("shape", GN_OFF, ids=_id)
def test_groupnorm_backward_off_the_configurations(lib, shape):
    B, C, HW = shape
    G.check_gn(lib, dict(B=B, C=C, HW=HW), "fp32")


def test_groupnorm_backward_far_from_zero(lib):
    """every channel mean 1000, deviation 1: the statistics pass takes E[x^2] - E[x]^2 (in fp64); the reference sees the same fp32
    inputs, so the bound is unchanged"""
    G.check_gn(lib, dict(B=2, C=256, HW=144, far=1), "fp32")


# LayerNorm2d + SiLU backward (M, C, pm, H2, W2): 1, 3 and 16 channels per lane; a second block of one row (65 = 64 + 1); the
# phase-major store on maps that are not square - a swapped H2 / W2 in the row index moves rows there
LN_OFF = [(1, 64, 0, 2, 2), (3, 192, 0, 2, 2), (65, 1024, 0, 2, 2), (2 * 4 * 6, 128, 1, 4, 6), (3 * 6 * 2, 256, 1, 6, 2)]


@pytest.mark.parametrize("shape", LN_OFF, ids=_id)
def test_layernorm_backward_off_the_configurations(lib, shape):
    M, C, pm, H2, W2 = shape
    G.check_ln(lib, dict(M=M, C=C, H2=H2, W2=W2), "fp32", pm=pm)


# transposed conv (B, Ci, Co, H, W): weight, bias and data gradient on maps that are not square (stage_phase_major's H and W)
CONVT_OFF = [(3, 64, 32, 3, 5), (2, 256, 256, 2, 6)]
# ldmseg_op_conv_wgrad + ldmseg_op_conv_dgrad (B, Ci, Co, H, W, NCHW epilogue)
CONV_OFF = [(3, 4, 256, 5, 7, 1), (2, 256, 128, 6, 10, 0)]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", CONVT_OFF, ids=_id)
def test_transposed_conv_gradients_on_a_map_that_is_not_square(lib, shape, mode):
    B, Ci, Co, H, W = shape
    G.check_convt(lib, dict(B=B, Ci=Ci, Co=Co, H=H, W=W), mode)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", CONV_OFF, ids=_id)
def test_conv_gradients_on_a_map_that_is_not_square(lib, shape, mode):
    B, Ci, Co, H, W, nchw = shape
    G.check_conv(lib, dict(B=B, Ci=Ci, Co=Co, H=H, W=W, nchw_dx=nchw), mode)


def test_weight_gradient_is_repeatable_and_modes_differ_only_in_rounding(lib):
    """two launches on the same inputs: identical bits, one slice or several; fp32 and split-bf16 products agree to the bound"""
    for B, H in ((2, 12), (2, 16)):
        g = torch.Generator().manual_seed(B * 100 + H)
        x, dy = G.dev(torch.randn(B, 256, H, H, generator=g)), G.dev(torch.randn(B, 128, H, H, generator=g))
        outs = {}
        for dt in (0, 2):
            for rep in range(2):
                w, b = torch.empty(128, 256, 3, 3, device=G.DEV), torch.empty(128, device=G.DEV)
                assert lib.ldmseg_op_conv_wgrad(G.P(x), G.P(dy), B, 256, H, H, 128, dt, G.P(w), G.P(b), None) == 0
                outs[dt, rep] = (w, b)
            assert torch.equal(outs[dt, 0][0], outs[dt, 1][0]) and torch.equal(outs[dt, 0][1], outs[dt, 1][1])
        assert R.metric(outs[2, 0][0], outs[0, 0][0].double().cpu()) < R.BOUND


def test_refusals(lib):
    t = torch.zeros(64, device=G.DEV)
    p = G.P(t)
    assert lib.ldmseg_op_conv_wgrad(p, p, 1, 4, 2, 2, 8, 1, p, p, None) == -2                   # bf16 storage: no backward
    assert lib.ldmseg_op_convt2_wgrad(p, p, 1, 32, 1, 1, 6, 0, p, p, None) == -2
    assert lib.ldmseg_op_layernorm_silu_bwd(p, p, p, p, 4, 96, 1e-6, 0, 2, 2, p, p, p, None) == -2
    assert lib.ldmseg_op_layernorm_silu_bwd(p, p, p, p, 6, 64, 1e-6, 1, 2, 2, p, p, p, None) == -2   # rows are no whole maps
    assert lib.ldmseg_op_groupnorm_silu_bwd(p, p, p, p, 1, 48, 4, 1e-5, p, p, p, None) == -2

"""CPU suite: the layer lists the per-op GPU oracle tests run at every configuration's shapes (tests/test_igemm_shapes_gpu.py)
against the layer walk of oracle/unet.py.  The walk runs on the meta device (shapes only, no arithmetic) at B = 1, L = 64, with
F.group_norm and the attention function of the oracle recorded.  tests/test_offgrid_shapes_gpu.py runs the same lists scaled by
L / 64 at latent sides off the power-of-two grid: the walk at L = 24 and L = 8 checks that scaling."""
import pytest
import torch
import torch.nn.functional as F


def _walk(monkeypatch_module, L):
    from ldmseg_amd import weights
    from oracle import unet as o_unet
    gn, attn = [], []
    real_gn, real_attn = F.group_norm, o_unet.attention

    def group_norm(x, groups, w, b, eps):
        gn.append((x.shape[2], x.shape[1], eps))
        return real_gn(x, groups, w, b, eps)

    def attention(sd, p, x, ctx=None):
        attn.append((x.shape[1], x.shape[2]))
        return real_attn(sd, p, x, ctx)

    monkeypatch_module.setattr(o_unet.F, "group_norm", group_norm)
    monkeypatch_module.setattr(o_unet, "attention", attention)
    sd = {k: torch.empty(shape, device="meta") for k, shape in weights.unet_schema(12, False).items()}
    y = o_unet.unet_forward(sd, torch.empty(1, 12, L, L, device="meta"), 499)
    assert tuple(y.shape) == (1, 4, L, L)
    monkeypatch_module.undo()
    return gn, attn


@pytest.fixture(scope="module")
def walk(monkeypatch_module):
    return _walk(monkeypatch_module, 64)


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def test_gn_shapes_match_the_oracle_walk(walk):
    from test_igemm_shapes_gpu import GN_SHAPES
    gn, _ = walk
    # the oracle normalises torch.cat([h, skip], 1) as one tensor: compare (side, total channels, eps); SiLU follows every eps-1e-5 norm
    assert all((eps == 1e-5) == bool(silu) for _, _, _, eps, silu in GN_SHAPES)
    assert set(gn) == {(h, c + c2, eps) for h, c, c2, eps, _ in GN_SHAPES}
    assert len(GN_SHAPES) == len({(h, c, c2, eps) for h, c, c2, eps, _ in GN_SHAPES})


def test_attention_levels_match_the_oracle_walk(walk):
    from test_igemm_shapes_gpu import ATTN_LEVELS
    _, attn = walk
    assert set(attn) == {(side * side, c) for side, c in ATTN_LEVELS}


@pytest.mark.parametrize("L", [24, 8])
def test_scaled_shape_lists_match_the_oracle_walk_off_the_grid(monkeypatch_module, L):
    """the lists hold map sides at L = 64; the GPU tests scale them by L / 64 (exact for every L % 8 == 0).  At L = 24 (maps 24, 12,
    6, 3) and L = 8 (maps 8, 4, 2, 1) the scaled lists are still exactly what the oracle normalises and attends over."""
    from test_igemm_shapes_gpu import ATTN_LEVELS, GN_SHAPES
    gn, attn = _walk(monkeypatch_module, L)
    assert all(h * L % 64 == 0 for h, *_ in GN_SHAPES) and all(side * L % 64 == 0 for side, _ in ATTN_LEVELS)
    assert set(gn) == {(h * L // 64, c + c2, eps) for h, c, c2, eps, _ in GN_SHAPES}
    assert len(set(gn)) == len(GN_SHAPES)
    assert set(attn) == {((side * L // 64) ** 2, c) for side, c in ATTN_LEVELS}
    assert len(set(attn)) == len(ATTN_LEVELS)

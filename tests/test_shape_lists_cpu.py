"""CPU suite: the layer lists the per-op GPU oracle tests run at every configuration's shapes (tests/test_igemm_shapes_gpu.py)
against the layer walk of oracle/unet.py.  The walk runs on the meta device (shapes only, no arithmetic) at B = 1, L = 64, with
F.group_norm and the attention function of the oracle recorded."""
import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope="module")
def walk(monkeypatch_module):
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
    y = o_unet.unet_forward(sd, torch.empty(1, 12, 64, 64, device="meta"), 499)
    assert tuple(y.shape) == (1, 4, 64, 64)
    return gn, attn


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

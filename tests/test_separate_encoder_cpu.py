"""CPU suite: the separate image encoder (modify_encoder(separate_encoder / separate_conv), unet.py:124-233) above the
library - schemas, checkpoint reading (detection, validation, the separate_conv fold), the restated forward's known answer
and the header."""
import os
import re
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from ldmseg_amd import weights
from ldmseg_amd.checkpoint import unet_state_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def zeros_of(schema):
    """a state dict of the schema's shapes that holds one float per tensor"""
    return OrderedDict((k, torch.zeros(1).expand(shp)) for k, shp in schema.items())


def sepenc_schema(add_adaptor):
    s = weights.unet_schema(4, False)
    s.update(weights.separate_encoder_schema(add_adaptor))
    return s


def test_schema_totals():
    s = sepenc_schema(False)
    assert (weights.count_params(s), len(s)) == (1_049_661_444, 780)
    s = sepenc_schema(True)
    assert (weights.count_params(s), len(s)) == (1_083_764_164, 788)
    extra = weights.separate_encoder_schema(True)
    assert not set(extra) & set(weights.unet_schema(4, False))
    base = weights.unet_schema(4, False)
    down = [k for k in base if k.startswith("down_blocks.")]
    assert [k for k in extra if k.startswith("down_blocks_additional.")] == ["down_blocks_additional." + k[12:] for k in down]
    assert all(extra["down_blocks_additional." + k[12:]] == base[k] for k in down)
    assert extra["conv_in_img.weight"] == (320, 4, 3, 3)
    assert [extra[f"adaptor_layers.{i}.weight"] for i in range(4)] == [(c, c, 3, 3) for c in (320, 640, 1280, 1280)]
    assert sum(base[k][0] for k in down if k.endswith("time_emb_proj.bias")) == 7040    # rows of the branch's time_emb_proj table
    assert list(weights.separate_conv_schema()) == ["conv_in_seg.weight", "conv_in_seg.bias"]
    # the new norm tensors are drawn as norms (gains around 1)
    small = OrderedDict((k, v) for k, v in extra.items() if k.startswith("down_blocks_additional.0.resnets.0.norm"))
    g = weights.generate(small, seed=3)
    assert (g["down_blocks_additional.0.resnets.0.norm1.weight"] - 1).abs().max() <= 0.1


@pytest.mark.parametrize("adaptor", [False, True])
def test_unet_state_from_detects_separate_encoder(adaptor):
    sd = zeros_of(sepenc_schema(adaptor))
    sd["new_conv.weight"] = torch.zeros(1)                      # unknown keys are dropped as before
    out = unet_state_from({"unet": OrderedDict(("module." + k, v) for k, v in sd.items())})
    assert list(out) == list(sepenc_schema(adaptor))
    assert tuple(out["conv_in.weight"].shape) == (320, 4, 3, 3)


def test_unet_state_from_validates_the_extra_tensors():
    sd = zeros_of(sepenc_schema(True))
    bad = OrderedDict(sd)
    bad["adaptor_layers.2.weight"] = torch.zeros(1).expand(1280, 640, 3, 3)
    with pytest.raises(ValueError, match="adaptor_layers.2.weight"):
        unet_state_from({"unet": bad})
    bad = OrderedDict(sd)
    del bad["down_blocks_additional.1.attentions.0.proj_in.bias"]
    with pytest.raises(KeyError, match="down_blocks_additional.1.attentions.0.proj_in.bias"):
        unet_state_from({"unet": bad})
    bad = OrderedDict(sd)
    del bad["adaptor_layers.3.bias"]
    with pytest.raises(KeyError, match="adaptor_layers.3.bias"):
        unet_state_from({"unet": bad})
    bad = OrderedDict(sd)
    bad["conv_in.weight"] = torch.zeros(1).expand(320, 8, 3, 3)   # the reference keeps the 4-channel conv_in here
    with pytest.raises(ValueError, match="conv_in.weight"):
        unet_state_from({"unet": bad})
    bad = OrderedDict(sd)
    bad["conv_in_img.weight"] = torch.zeros(1).expand(320, 8, 3, 3)
    with pytest.raises(ValueError, match="conv_in_img.weight"):
        unet_state_from({"unet": bad})


def test_separate_encoder_with_attn2_is_refused():
    s = weights.unet_schema(4, True)
    s.update(weights.separate_encoder_schema(False))
    for cross_attention in (False, True):
        with pytest.raises(NotImplementedError, match="separate image encoder"):
            unet_state_from({"unet": zeros_of(s)}, cross_attention=cross_attention)
    with pytest.raises(NotImplementedError, match="separate image encoder"):
        unet_state_from({"unet": zeros_of(sepenc_schema(False))}, cross_attention=True)


def test_separate_conv_folds_into_an_8_channel_conv_in():
    s = weights.unet_schema(4, False)
    s.update(weights.separate_conv_schema())
    sd = zeros_of(s)
    g = torch.Generator().manual_seed(5)
    for k in ("conv_in.weight", "conv_in.bias", "conv_in_seg.weight", "conv_in_seg.bias"):
        sd[k] = torch.randn(s[k], generator=g)
    out = unet_state_from({"unet": sd})
    assert list(out) == list(weights.unet_schema(8, False))      # loads as a plain 8-channel UNet
    assert tuple(out["conv_in.weight"].shape) == (320, 8, 3, 3)
    seg, img = torch.randn(2, 4, 9, 9, generator=g), torch.randn(2, 4, 9, 9, generator=g)
    ref = (F.conv2d(seg.double(), sd["conv_in_seg.weight"].double(), sd["conv_in_seg.bias"].double(), padding=1) +
           F.conv2d(img.double(), sd["conv_in.weight"].double(), sd["conv_in.bias"].double(), padding=1))
    got = F.conv2d(torch.cat([seg, img], 1).double(), out["conv_in.weight"].double(), out["conv_in.bias"].double(), padding=1)
    assert float((got - ref).abs().max()) < 1e-6
    assert tuple(sd["conv_in.weight"].shape) == (320, 4, 3, 3)   # the caller's dict is left as it was
    bad = OrderedDict(sd)
    bad["conv_in_seg.weight"] = torch.zeros(1).expand(320, 8, 3, 3)
    with pytest.raises(ValueError, match="conv_in_seg.weight"):
        unet_state_from({"unet": bad})
    both = zeros_of(sepenc_schema(False))
    both.update(zeros_of(weights.separate_conv_schema()))
    with pytest.raises(ValueError, match="both"):
        unet_state_from({"unet": both})


@pytest.mark.parametrize("in_ch,cross", [(8, False), (12, False), (8, True)])
def test_plain_checkpoints_keep_their_key_list(in_ch, cross):
    s = weights.unet_schema(in_ch, cross)
    sd = zeros_of(s)
    sd["new_conv.weight"] = torch.zeros(1)
    out = unet_state_from({"unet": sd}, cross_attention=cross)
    assert list(out) == list(s)
    assert all(out[k] is sd[k] for k in s)


def test_restatement_known_answer():
    """With conv_in_img.* and adaptor_layers.* zeroed every image residual is exactly zero, and the forward is the plain
    8-channel UNet's whose conv_in has zero filters on the image half - bit for bit."""
    from oracle import unet as o_unet
    import unet_sepenc_ref as ref
    sd = weights.generate(sepenc_schema(True), seed=21)
    for k in sd:
        if k.startswith(("conv_in_img.", "adaptor_layers.")):
            sd[k] = torch.zeros_like(sd[k])
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 16, 16, generator=g)
    t = torch.tensor([19, 500])
    torch.set_num_threads(8)
    with torch.no_grad():
        assert all(float(r.abs().max()) == 0.0 for r in ref.image_residuals(sd, x[:, 4:]))
        a = ref.sepenc_forward(sd, x, t, timestep_img=torch.tensor(300))
        b = o_unet.unet_forward(ref.plain_equivalent(sd), x, t)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0.1
    assert torch.equal(a, b)


def test_header_declares_the_image_timestep_forward():
    txt = open(os.path.join(ROOT, "include", "ldmseg_hip.h")).read()
    m = re.search(r"int ldmseg_unet_forward_img\(([^)]*)\)", txt)
    assert m, "ldmseg_unet_forward_img is not declared"
    args = m.group(1)
    assert all(a in args for a in ("timg_dev", "timg_count", "timg_host", "t_dev", "t_count", "t_host"))
    ops = open(os.path.join(ROOT, "include", "ldmseg_hip_ops.h")).read()
    assert re.search(r"int ldmseg_op_skip_add\(", ops)
    from ldmseg_amd import _lib
    assert "ldmseg_unet_forward_img" in _lib.SIGNATURES and "ldmseg_op_skip_add" in _lib.SIGNATURES

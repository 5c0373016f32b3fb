"""CPU suite of the CLIP vision encoder: the torch reference the GPU tests compare the library with
(tests/clip_vision_ref.py) is pinned against transformers' own classes and against outputs transformers produced; the
schema, the two key layouts, and the launch sites of csrc/clip_vision.hip."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_vision_ref as R                                   # noqa: E402
from conftest import GOLDEN                                   # noqa: E402
from golden.make_golden_clip import load_weights              # noqa: E402
from test_launch_sites_cpu import CSRC, bare_launches, logged_launches   # noqa: E402

FULL = dict(hidden=1024, intermediate=4096, layers=24, heads=16, image=224, patch=14, projection_dim=768)


def _weights(cfg, seed):
    from ldmseg_amd import weights
    schema = weights.clip_vision_schema(**cfg)
    return weights.generate(schema, seed=seed, norm_keys=weights.clip_vision_norm_keys(schema))


def test_schema_parameter_counts():
    from ldmseg_amd import weights
    assert weights.count_params(weights.clip_vision_schema()) == 303_179_776
    full = weights.clip_vision_schema(projection_dim=768)
    assert weights.count_params(full) == 303_966_208
    assert len(full) == 392
    small = weights.clip_vision_schema(**R.SMALL)
    assert small["embeddings.position_embedding.weight"] == (10, 128) and small["visual_projection.weight"] == (96, 128)


def test_generated_weights_treat_layernorms_and_embeddings():
    sd = _weights(R.SMALL, 0)
    for k in ("pre_layrnorm.weight", "post_layernorm.weight", "encoder.layers.1.layer_norm2.weight"):
        assert float((sd[k] - 1).abs().max()) <= 0.1 + 1e-6, k          # gains 1 +- 0.1, not biases
    full = _weights(dict(FULL, layers=1), 0)
    pos = full["embeddings.position_embedding.weight"]
    assert abs(float(pos.std()) - 0.02) < 1e-3                          # CLIP's initialisation scale, not U(+-sqrt(3 / 1024))
    assert abs(float(full["embeddings.class_embedding"].std()) - 0.02) < 3e-3


def test_reference_matches_transformers_outputs_fixture():
    """always runs: the fixture holds what transformers computed (tests/golden/make_golden_clip.py)"""
    z = np.load(os.path.join(GOLDEN, "clip_vision.npz"))
    sd = load_weights(z)
    out = R.forward(sd, torch.from_numpy(z["pixel_values"]), R.SMALL["heads"])
    for k in ("last_hidden_state", "pooler_output", "image_embeds"):
        e = R.rel_err(out[k], torch.from_numpy(z[k]))
        print(k, e)
        assert e <= 1e-5, (k, e)


@pytest.mark.parametrize("name,B", [("small", 2), ("full", 1)])
def test_reference_matches_transformers(name, B):
    tf = pytest.importorskip("transformers")
    c = R.SMALL if name == "small" else FULL
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = _weights(c, 3)
    cfg = tf.CLIPVisionConfig(hidden_size=c["hidden"], intermediate_size=c["intermediate"], num_hidden_layers=c["layers"],
                              num_attention_heads=c["heads"], image_size=c["image"], patch_size=c["patch"],
                              projection_dim=c["projection_dim"])
    x = torch.randn(B, 3, c["image"], c["image"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        mp = tf.CLIPVisionModelWithProjection(cfg).eval()
        full = {(k if k.startswith("visual_projection") else "vision_model." + k): v for k, v in sd.items()}
        missing, unexpected = mp.load_state_dict(full, strict=False)
        assert not unexpected and all("position_ids" in m for m in missing)
        op = mp(pixel_values=x)
        ov = mp.vision_model(pixel_values=x)
        # CLIPVisionModel on its own: whichever key layout this transformers release uses must load through strip_prefix
        mv = tf.CLIPVisionModel(cfg).eval()
        keys = [k for k in mv.state_dict() if "position_ids" not in k]
        plain = {k: sd[R.strip_prefix({k: 0}).popitem()[0]] for k in keys}
        mv.load_state_dict(plain, strict=False)
        oplain = mv(pixel_values=x)
        ref = R.forward(sd, x, c["heads"])
        ref_plain = R.forward(plain, x, c["heads"])
    for got, want, what in ((ref["last_hidden_state"], ov.last_hidden_state, "last_hidden_state"),
                            (ref["pooler_output"], ov.pooler_output, "pooler_output"),
                            (ref["image_embeds"], op.image_embeds, "image_embeds"),
                            (ref_plain["last_hidden_state"], oplain.last_hidden_state, "CLIPVisionModel.last_hidden_state")):
        e = R.rel_err(got, want)
        print(name, what, e)
        assert e <= 1e-5, (what, e)
    T = (c["image"] // c["patch"]) ** 2 + 1
    assert tuple(R.last_feat(ref, False).shape) == (B, c["hidden"], T)          # MyCLIPVisionModel
    assert tuple(R.last_feat(ref, True).shape) == (B, c["projection_dim"], 1)   # MyCLIPVisionModelWithProjection


def test_both_key_layouts_load():
    from ldmseg_amd.models import clip_vision as cv
    sd = _weights(R.SMALL, 0)
    pref = {(k if k.startswith("visual_projection") else "vision_model." + k): v for k, v in sd.items()}
    pref["vision_model.embeddings.position_ids"] = torch.arange(10).unsqueeze(0)
    for layout in (sd, pref):
        s = cv.strip_vision_prefix(layout)
        assert set(sd) <= set(s)
        cfg = cv.config_from_state_dict(s)
        assert cfg == R.SMALL
    x = torch.randn(1, 3, 42, 42, generator=torch.Generator().manual_seed(0))
    a, b = R.forward(sd, x, 2), R.forward(pref, x, 2)
    assert torch.equal(a["image_embeds"], b["image_embeds"])
    with pytest.raises(RuntimeError):
        cv.CLIPVisionDescriptor(sd, device="cpu")


def test_quick_gelu_fold():
    """x * sigmoid(1.702 x) == silu(1.702 x) / 1.702: what lets fc1 run on the existing SiLU epilogue"""
    x = torch.linspace(-12, 12, 4001)
    a = x * torch.sigmoid(1.702 * x)
    b = torch.nn.functional.silu(1.702 * x) / 1.702
    assert float((a - b).abs().max()) < 1e-6


def test_clip_vision_launches_are_logged():
    """every launch of csrc/clip_vision.hip goes through LDMSEG_LAUNCH with a name that carries its template arguments"""
    txt = open(os.path.join(CSRC, "clip_vision.hip")).read()
    assert bare_launches("clip_vision.hip", txt) == []
    assert len(logged_launches(txt)) >= 4
    assert not logged_launches(txt, "LDMSEG_LAUNCH_GEMM")          # no GEMM kernels of its own
    for kern in ("clip_patch_rows", "clip_tokens", "clip_pooled_ln", "clip_rows_to_f32"):
        assert re.search(r'launch_name\("' + kern + r'<%s', txt), kern
    # the scan sees a bare launch
    assert bare_launches("x", txt.replace("LDMSEG_LAUNCH(launch_name(\"clip_tokens<%s>\", \"f32\"), ", "hipLaunchKernelGGL(", 1))
    from ldmseg_amd import build
    assert "clip_vision.hip" in build.SOURCES

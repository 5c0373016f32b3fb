"""CPU suite of the CLIP text encoder: the torch reference the GPU tests compare the library with (tests/clip_text_ref.py)
is pinned against transformers' CLIPTextModel and against outputs transformers produced; the schema, the two key layouts,
the reference's own causality, and the launch sites of csrc/clip_text.hip."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_text_ref as R                                     # noqa: E402
from conftest import GOLDEN                                   # noqa: E402
from golden.make_golden_clip import load_weights              # noqa: E402
from golden.make_golden_clip_text import load_into, text_model   # noqa: E402
from test_launch_sites_cpu import CSRC, bare_launches, logged_launches   # noqa: E402


def _weights(cfg, seed):
    from ldmseg_amd import weights
    schema = weights.clip_text_schema(**cfg)
    return weights.generate(schema, seed=seed, norm_keys=weights.clip_text_norm_keys(schema))


def test_schema_parameter_counts():
    from ldmseg_amd import weights
    full = weights.clip_text_schema()
    assert weights.count_params(full) == 123_060_480
    assert len(full) == 196
    small = weights.clip_text_schema(**R.SMALL)
    assert small["embeddings.token_embedding.weight"] == (512, 128) and small["embeddings.position_embedding.weight"] == (77, 128)
    assert "embeddings.position_ids" not in full


def test_generated_weights_treat_layernorms_and_embeddings():
    from ldmseg_amd import weights
    sd = _weights(R.SMALL, 0)
    for k in ("final_layer_norm.weight", "encoder.layers.1.layer_norm2.weight", "encoder.layers.0.layer_norm1.weight"):
        assert float((sd[k] - 1).abs().max()) <= 0.1 + 1e-6, k          # gains 1 +- 0.1, not biases
    for k in ("embeddings.token_embedding.weight", "embeddings.position_embedding.weight"):
        assert abs(float(sd[k].std()) - 0.02) < 1e-3, k                 # CLIP's initialisation scale
    # the new embedding key belongs to no earlier schema: no tensor generated before this key existed has changed
    for schema in (weights.clip_vision_schema(projection_dim=768), weights.unet_schema(8, True), weights.vae_schema()):
        assert "embeddings.token_embedding.weight" not in schema


def test_reference_matches_transformers_outputs_fixture():
    """always runs: the fixture holds what transformers computed (tests/golden/make_golden_clip_text.py)"""
    path = os.path.join(GOLDEN, "clip_text.npz")
    assert os.path.getsize(path) < 1_000_000
    z = np.load(path)
    sd = load_weights(z)
    out = R.forward(sd, torch.from_numpy(z["input_ids"]), R.SMALL["heads"])
    e = R.rel_err(out, torch.from_numpy(z["last_hidden_state"]))
    print("last_hidden_state", e)
    assert e <= 1e-5, e


@pytest.mark.parametrize("name", ["small", "full"])
def test_reference_matches_transformers(name):
    tf = pytest.importorskip("transformers")
    c = R.SMALL if name == "small" else R.FULL
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = _weights(c, 3)
    ids = R.prompt_ids([5, 40, 76], c["positions"], c["vocab"], seed=1)
    with torch.no_grad():
        model = text_model(tf, c)
        loaded = load_into(model, sd)              # whichever key layout this transformers release uses
        want = model(input_ids=ids).last_hidden_state
        got = R.forward(sd, ids, c["heads"])
        got_loaded = R.forward(loaded, ids, c["heads"])
    e = R.rel_err(got, want)
    print(name, "last_hidden_state", e)
    assert e <= 1e-5, e
    assert torch.equal(got, got_loaded)
    assert tuple(got.shape) == (3, c["positions"], c["hidden"])


def test_both_key_layouts_load():
    from ldmseg_amd.models import clip_text as ct
    from ldmseg_amd.models import CLIPTextEncoder, strip_text_prefix
    sd = _weights(R.SMALL, 0)
    pref = {"text_model." + k: v for k, v in sd.items()}
    pref["text_model.embeddings.position_ids"] = torch.arange(77).unsqueeze(0)
    for layout in (sd, pref):
        s = strip_text_prefix(layout)
        assert set(sd) <= set(s)
        assert ct.config_from_state_dict(s) == R.SMALL           # round trip: schema -> tensors -> configuration
    ids = R.prompt_ids([3, 30], 77, 512)
    assert torch.equal(R.forward(sd, ids, 2), R.forward(pref, ids, 2))
    from ldmseg_amd import weights
    full = ct.config_from_state_dict({k: torch.empty(v, device="meta") for k, v in weights.clip_text_schema().items()})
    assert full == R.FULL
    with pytest.raises(RuntimeError):
        CLIPTextEncoder(sd, device="cpu")


def test_reference_is_causal():
    """rows [:20] of a 77-token run equal the 20-token run: later tokens do not reach earlier rows (up to the GEMMs' blocking,
    which depends on the row count)"""
    sd = _weights(R.SMALL, 2)
    ids = R.prompt_ids([50, 76, 10], 77, 512, seed=4)
    with torch.no_grad():
        a = R.forward(sd, ids, 2)
        b = R.forward(sd, ids[:, :20], 2)
    e = R.rel_err(a[:, :20], b)
    print("causality", e)
    assert e <= 1e-5
    # and a change behind position p leaves rows < p alone
    ids2 = ids.clone()
    ids2[:, 33:] = 7
    with torch.no_grad():
        c = R.forward(sd, ids2, 2)
    assert R.rel_err(c[:, :33], a[:, :33]) <= 1e-5 and R.rel_err(c[:, 33:], a[:, 33:]) > 1e-2


def test_output_indexing():
    from ldmseg_amd.models.clip_text import CLIPTextOutput
    t = torch.zeros(2, 3)
    o = CLIPTextOutput(last_hidden_state=t)
    assert o[0] is t and o.last_hidden_state is t and o["last_hidden_state"] is t


def test_clip_text_launches_are_logged():
    """every launch of csrc/clip_text.hip goes through LDMSEG_LAUNCH with a name that carries its template arguments; the causal
    attention is launched under names of its own"""
    txt = open(os.path.join(CSRC, "clip_text.hip")).read()
    assert bare_launches("clip_text.hip", txt) == []
    assert len(logged_launches(txt)) >= 4
    assert not logged_launches(txt, "LDMSEG_LAUNCH_GEMM")          # no GEMM kernels of its own
    for kern in ("clip_text_tokens", "clip_text_final_ln"):
        assert re.search(r'launch_name\("' + kern + r'<%s', txt), kern
    att = open(os.path.join(CSRC, "attention.hip")).read()
    assert re.search(r'launch_name\("attn_causal<%s,%d,%d>"', att) and re.search(r'launch_name\("attn_causal_x3<%d,%d>"', att)
    assert "launch_attention_causal" in att
    # the scan sees a bare launch
    assert bare_launches("x", txt.replace("LDMSEG_LAUNCH(launch_name(\"clip_text_tokens<%s>\", \"f32\"), ", "hipLaunchKernelGGL(", 1))
    from ldmseg_amd import build
    assert "clip_text.hip" in build.SOURCES

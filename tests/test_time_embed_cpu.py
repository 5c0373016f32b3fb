"""CPU suite: the float64 reference of the time-embedding path (tests/time_embed_ref.py) against the oracle it stands next to,
and the refusals of the three entry points that reach the path's kernels (no device is touched: a refusal comes first).

tests/test_time_embed_gpu.py holds the kernels to this reference."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import time_embed_ref as ref
import unet_sepenc_ref
from oracle import unet as o_unet

_MEM = C.create_string_buffer(64)
P = C.c_void_p(C.addressof(_MEM))                 # a non-null pointer that nothing reads


def _args_id(args):
    """test id of an argument tuple: the pointer by name, since its address differs from process to process"""
    return "(" + ", ".join("P" if a is P else str(a) for a in args) + ")"


def test_sinusoid_reference_vs_oracle():
    """every t of the training range: the oracle's fp32 sinusoid lies within half the bound the kernel is held to"""
    t = torch.arange(1000)
    got = o_unet.timestep_embedding(t).double().numpy()
    ratio = np.abs(got - ref.sinusoid(t)) / ref.sinusoid_tol(t)
    assert ratio.shape == (1000, 320)
    print(f"oracle fp32 sinusoid vs float64: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 0.5
    # the bound tells a wrong frequency from a rounding: 159 in place of 160, already at t = 1
    wrong = np.exp(-np.log(1e4) * np.arange(160) / 159.0)
    bad = np.concatenate([np.cos(wrong), np.sin(wrong)])[None, :]
    assert (np.abs(bad - ref.sinusoid([1])) / ref.sinusoid_tol([1])).max() > 1000


def test_sinusoid_layout_and_known_values():
    s = ref.sinusoid([0, 1])
    assert s.shape == (2, 320)
    assert np.array_equal(s[0], np.r_[np.ones(160), np.zeros(160)])
    assert s[1, 0] == np.cos(1.0) and s[1, 160] == np.sin(1.0)                  # f_0 = 1
    assert abs(s[1, 159] - np.cos(1e-4 ** (159 / 160))) < 1e-15
    assert ref.sinusoid_tol([0]).max() == 2.0 ** -22                            # t = 0: the rounding of the result alone


def test_prefix_lists_follow_the_model_definition():
    from ldmseg_amd import weights
    tail = "time_emb_proj.weight"
    main = weights.unet_schema(12, False)
    assert [k[:-len(tail)] for k in main if k.endswith(tail)] == ref.MAIN_PREFIXES
    extra = weights.separate_encoder_schema(True)
    assert [k[:-len(tail)] for k in extra if k.endswith(tail)] == ref.IMAGE_PREFIXES
    assert sum(main[p + tail][0] for p in ref.MAIN_PREFIXES) == 20160
    assert sum(extra[p + tail][0] for p in ref.IMAGE_PREFIXES) == 7040


@pytest.fixture(scope="module")
def time_sd64():
    """the time-embedding tensors of a separate-encoder state dict (both tables), float64"""
    from ldmseg_amd import weights
    full = weights.unet_schema(4, False)
    full.update(weights.separate_encoder_schema(True))
    keys = ref.time_keys(ref.MAIN_PREFIXES + ref.IMAGE_PREFIXES)
    sd = weights.generate(OrderedDict((k, full[k]) for k in keys), seed=21)
    return {k: v.double() for k, v in sd.items()}


@pytest.mark.parametrize("table", ["main", "image"])
def test_rows_reference_equals_the_oracle_chain(time_sd64, table):
    """the chain of oracle/unet.py (unet_forward's time_embedding lines, resnet's time_emb_proj line) and the embedding of
    tests/unet_sepenc_ref.py in float64, from the oracle's own sinusoid, against `rows` from the same sinusoid"""
    prefixes = ref.MAIN_PREFIXES if table == "main" else ref.IMAGE_PREFIXES
    ts = torch.tensor([999, 500, 259, 19, 1, 0])
    sinus = o_unet.timestep_embedding(ts).double()
    sd = time_sd64
    emb = F.linear(sinus, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    emb = F.linear(F.silu(emb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    assert torch.equal(emb, unet_sepenc_ref._embed(sd, ts, len(ts)))
    want = torch.cat([F.linear(F.silu(emb), sd[p + "time_emb_proj.weight"], sd[p + "time_emb_proj.bias"]) for p in prefixes], 1).numpy()
    got = ref.rows(sd, ts, prefixes, sinus=sinus)
    assert got.shape == want.shape == (6, 20160 if table == "main" else 7040)
    # two float64 evaluations in different summation orders: K = 1280 terms of magnitude <= max|want| each
    assert np.abs(got - want).max() <= 1280 * 2.0 ** -52 * np.abs(want).max()
    # and from its own float64 sinusoid the reference moves by what the oracle's fp32 sinusoid is off, no more than 1e-5
    own = ref.rows(sd, ts, prefixes)
    assert 0 < np.abs(own - want).max() / np.abs(want).max() < 1e-5


def test_linear_bound_is_met_by_an_fp32_evaluation():
    """the bound's own sanity: torch's fp32 F.linear / F.silu stay inside it, a dropped SiLU or bias does not"""
    g = torch.Generator().manual_seed(5)
    x = 3.0 * torch.randn(3, 320, generator=g)
    W = torch.randn(64, 320, generator=g) / 320 ** 0.5
    b = 0.1 * torch.randn(64, generator=g)
    for si in (0, 1):
        for so in (0, 1):
            v = F.linear(F.silu(x) if si else x, W, b)
            got = (F.silu(v) if so else v).double().numpy()
            want, bound = ref.small_linear(x, W, b, si, so), ref.small_linear_bound(x, W, b, si, so)
            assert (np.abs(got - want) / bound).max() < 1.0, (si, so)
            assert (np.abs(ref.small_linear(x, W, b, 1 - si, so) - want) / bound).max() > 1e3
            assert (np.abs(ref.small_linear(x, W, b, si, 1 - so) - want) / bound).max() > 1e3
            assert (np.abs(ref.small_linear(x, W, None, si, so) - want) / bound).max() > 1e3


def test_descending_timesteps():
    for n in (1, 2, 64, 65, 130):
        ts = ref.descending_timesteps(n)
        assert len(ts) == n == len(set(ts)) and ts[0] == 999 and ts == sorted(ts, reverse=True)
        assert n == 1 or ts[-1] == 0


# ------------------------------------------------------------------ refusals (no device needed)
@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("args", [
    (None, 1, 5, 0, P), (None, 1, 5, -1, P), (None, 1, 5, 2, None),            # B < 1, no output
    (P, 0, 0, 2, P), (P, 3, 0, 2, P), (P, 2, 0, 3, P), (P, -1, 0, 3, P),       # t_dev with t_count not in {1, B}
], ids=_args_id)
def test_time_sinusoid_refusals(lib, args):
    assert lib.ldmseg_op_time_sinusoid(*args, None) == -2


@pytest.mark.parametrize("args", [
    (None, P, P, 1, 1, 1, 0, 0, P), (P, None, P, 1, 1, 1, 0, 0, P), (P, P, P, 1, 1, 1, 0, 0, None),
    (P, P, None, 0, 1, 1, 0, 0, P), (P, P, None, 1, 0, 1, 0, 0, P), (P, P, None, 1, 1, 0, 0, 0, P), (P, P, P, -3, 64, 8, 1, 1, P),
], ids=_args_id)
def test_small_linear_refusals(lib, args):
    assert lib.ldmseg_op_small_linear(*args, None) == -2


def test_unet_time_rows_refusals_without_a_handle(lib):
    """(what a handle refuses - n < 1, a negative timestep, a table it does not have - runs in the GPU suite)"""
    ts = (C.c_int64 * 2)(999, 0)
    total = C.c_int(-7)
    assert lib.ldmseg_unet_time_rows(None, ts, 2, 0, None, C.byref(total), None) == -2
    assert lib.ldmseg_unet_time_rows(None, ts, 2, 0, P, C.byref(total), None) == -2
    assert lib.ldmseg_unet_time_rows(None, None, 0, 3, None, None, None) == -2
    assert total.value == -7

"""CPU suite: the staging of the single-operator entry points (csrc/ops_api.hip) on a machine without a device.

There every hipMalloc fails, so each staged entry point must come back with LDMSEG_E_OOM (-6) from its first staging buffer
and launch nothing - the dummy pointers below are never dereferenced - while a shape the entry point refuses still returns
-2: the argument checks come before the staging.  Skipped where a device is present (there an allocation succeeds)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine without a device: hipMalloc must fail")

E_SHAPE, E_OOM = -2, -6
_MEM = C.create_string_buffer(64)
P = C.c_void_p(C.addressof(_MEM))                 # a non-null pointer that nothing reads
SEG = (C.c_int64 * 1)(8)                          # ldmseg_op_skip_add reads its segment lengths on the host

# entry point -> (smallest valid call, a call it refuses); the trailing stream argument (null) is appended below
CASES = {
    # x, gamma, beta, M, C, eps, silu, dtype, out
    "layernorm": ((P, P, P, 1, 64, 1e-5, 0, 0, P), (P, P, P, 0, 64, 1e-5, 0, 0, P)),
    # ..., silu, inplace, dtype, out
    "layernorm_io": ((P, P, P, 1, 64, 1e-5, 0, 0, 0, P), (P, P, P, 1, 0, 1e-5, 0, 0, 0, P)),
    # qkv, B, N, C, heads, dtype, out
    "attention": ((P, 1, 16, 40, 1, 0, P), (P, 1, 16, 41, 1, 0, P)),
    "attention_causal": ((P, 1, 8, 64, 1, 0, P), (P, 1, 8, 65, 1, 0, P)),
    # q, kv, B, N, S, C, heads, dtype, out
    "attention_cross": ((P, P, 1, 1, 1, 40, 1, 0, P), (P, P, 1, 1, 0, 40, 1, 0, P)),
    # qkv, B, N, C, heads, out, time_iters, us_per_launch
    "attention_fp8": ((P, 1, 64, 40, 1, P, 0, None), (P, 1, 64, 64, 1, P, 0, None)),
    # x, w, bias, resid, rowbias, rows_per_image, M, K, N, geglu, silu, splits, dtype, out
    "linear": ((P, P, None, None, None, 1, 1, 32, 32, 0, 0, 0, 0, P), (P, P, None, None, None, 1, 1, 33, 32, 0, 0, 0, 0, P)),
    # x, x2, w, bias, B, Ci, Ci2, H, W, Co, k, stride, up, dtype, out
    "conv2d": ((P, None, P, None, 1, 4, 0, 1, 1, 5, 1, 1, 0, 0, P), (P, P, P, None, 1, 4, 4, 1, 1, 5, 1, 1, 0, 0, P)),
    # x, x2, w, bias, resid, rowbias, B, Ci, Ci2, H, W, Co, k, stride, up, geglu, silu, splits, dtype, out
    "igemm": ((P, None, P, None, None, None, 1, 4, 0, 1, 1, 5, 1, 1, 0, 0, 0, 0, 0, P),
              (P, P, P, None, None, None, 1, 4, 4, 1, 1, 5, 1, 1, 0, 0, 0, 0, 0, P)),
    # x, w, bias, resid, B, Ci, H, W, Co, k, stride, pad, silu, epi, n_store, dtype, out
    "vae_conv": ((P, P, None, None, 1, 4, 1, 1, 5, 1, 1, -1, 0, 0, 0, 0, P), (P, P, None, None, 1, 4, 1, 1, 5, 2, 1, -1, 0, 0, 0, 0, P)),
    # x, w, bias, B, Ci, H, W, Co, dtype, out
    "convt2": ((P, P, None, 1, 32, 1, 1, 4, 0, P), (P, P, None, 1, 32, 1, 1, 5, 0, P)),
    # a, b, bias, M, N, K, rows_f32, dtype, out
    "gemm_dynamic": ((P, P, None, 1, 32, 32, 0, 0, P), (P, P, None, 1, 33, 32, 0, 0, P)),
    # x, x2, gamma, beta, B, C, C2, HW, eps, silu, dtype, out
    "groupnorm": ((P, None, P, P, 1, 32, 0, 1, 1e-5, 0, 0, P), (P, None, P, P, 0, 32, 0, 1, 1e-5, 0, 0, P)),
    # x, w, bias, rowbias, gamma, beta, B, Ci, H, W, Co, eps, silu, splits, dtype, out (the smallest map with a fused finish)
    "conv_groupnorm": ((P, P, P, None, P, P, 8, 32, 8, 8, 1280, 1e-5, 1, 2, 0, P), (P, P, P, None, P, P, 8, 32, 8, 8, 1280, 1e-5, 1, 1, 0, P)),
    # x, gamma, beta, w, bias, M, K, N, eps, geglu, dtype, out
    "ln_linear": ((P, P, P, P, None, 1, 32, 160, 1e-5, 0, 0, P), (P, P, P, P, None, 1, 33, 160, 1e-5, 0, 0, P)),
    # h, x, gamma, beta, w1, b1, w2, b2, wp, bp, M, C, eps, dtype, mode, out, time_iters, us_per_call
    "transformer_ff": ((P,) * 10 + (1, 32, 1e-5, 0, 0, P, 0, None), (P,) * 10 + (1, 33, 1e-5, 0, 0, P, 0, None)),
    # x, wp, bp, gamma, beta, wq, wk, wv, M, C, eps, dtype, mode, h_out, qkv_out, time_iters, us_per_call
    "transformer_in": ((P,) * 8 + (1, 32, 1e-5, 0, 0, P, P, 0, None), (P,) * 8 + (1, 33, 1e-5, 0, 0, P, P, 0, None)),
    # g, h, x, w2, b2, wp, bp, M, C, rows_per_image, dtype, out
    "chained_ff_out": ((P,) * 7 + (1, 640, 1, 0, P), (P,) * 7 + (0, 640, 1, 0, P)),
    # a, b, seg_elems, n_segs, dtype, out
    "skip_add": ((P, P, SEG, 1, 0, P), (P, P, SEG, 0, 0, P)),
    # sc, rows, n, scale, dtype, out
    "softmax_rows": ((P, 1, 4, 1.0, 0, P), (P, 1, 4, 0.0, 0, P)),
    # x, B, C, H, W, dtype, out
    "bilinear2x": ((P, 1, 4, 1, 1, 0, P), (P, 0, 4, 1, 1, 0, P)),
    # x, B, C, H, W, mask_th, ignore_label, dtype, ids, prob
    "bilinear2x_argmax": ((P, 1, 4, 1, 1, -1.0, 255, 0, P, None), (P, 0, 4, 1, 1, -1.0, 255, 0, P, None)),
    # img, B, H, W, S, P, mean, std, resample, dtype, out
    "clip_patch_rows": ((P, 1, 14, 14, 14, 14, None, None, 0, 0, P), (P, 1, 14, 14, 15, 14, None, None, 0, 0, P)),
    # ids, tok, pos, R, T, C, vocab, dtype, out
    "clip_text_tokens": ((P, P, P, 1, 1, 64, 2, 0, P), (P, P, P, 0, 1, 64, 2, 0, P)),
}


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_failed_staging_allocation_is_oom_and_refusals_come_first(lib, name):
    fn = getattr(lib, "ldmseg_op_" + name)
    valid, refused = CASES[name]
    assert fn(*refused, None) == E_SHAPE
    assert fn(*valid, None) == E_OOM

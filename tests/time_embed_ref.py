"""Test support: the time-embedding path in float64, and the error bounds its fp32 kernels are held to.

The operations are restated from their definitions, not from the kernels:

* ``sinusoid(t)``      diffusers Timesteps(320, flip_sin_to_cos=True, freq_shift=0): [cos(t f_i) | sin(t f_i)],
                       f_i = exp(-ln(1e4) i / 160), i < 160;
* ``small_linear``     act_out(act_in(x) W^T + b) with silu(x) = x / (1 + exp(-x)) where a flag is set;
* ``rows``             linear_1 -> SiLU -> linear_2 -> time_emb_proj(SiLU(.)) of every resnet of a table, concatenated in
                       model order.  The order is that of the model definition: ``MAIN_PREFIXES`` = the down blocks, the mid
                       block, the up blocks (20160 columns), ``IMAGE_PREFIXES`` = the eight resnets of
                       down_blocks_additional (7040 columns).

The bounds are derived, not tuned; none of them was taken from what a kernel gives.

Sinusoid.  ``sinusoid_tol(t)[.., i] = 2^-22 (1 + t f_i (1 + |ln f_i|))``: cos and sin have derivative at most 1, so an error of
the argument passes through unamplified, and the fp32 argument t f_i carries a few roundings - of the exponent
-ln(1e4) i / 160 (a relative error u of the exponent is a relative error |ln f_i| u of f_i), of exp and of the product (relative
to t f_i) - on top of the rounding of the result itself (the 1).  2^-22 = 4 u leaves room for four such roundings each.

Linear, per output: ``(ceil(K / 64) + 8) 2^-23 sum_k |x_k| |w_k|`` with the sum in float64.  A lane of the kernel's wave adds
ceil(K / 64) fused multiply-adds, six shuffle levels add the 64 lanes and one addition brings the bias: the first-order bound
of that chain is (ceil(K / 64) + 7) u sum|x_k w_k| with u = 2^-24; it is doubled for the higher-order terms.  The bound has no
term for the bias itself, so it holds where the bias does not dominate the products: ``small_linear_bound`` refuses inputs
with |b_n| > 16 sum_k |x_k| |w_k| (the rounding of the last addition, u (sum + |b|), then no longer fits into the doubling).
With silu_in, x_k is the exact SiLU and ``sum_k delta(x_k) |w_k|`` is added, ``delta(x) = (|x| + 4) 2^-23 |silu(x)|``: v_exp_f32 on
-x log2(e) sees an argument whose rounding is a relative error |x| ln 2 log2(e) u = |x| u of the exponential, v_exp_f32 and
v_rcp_f32 are 1 ulp each, the addition and the final product one rounding each (the 4), doubled.  With silu_out the same
delta of the pre-activation is added to the output's bound.
"""
import math

import numpy as np

HALF = 160
TIME_DIM = 1280
U23 = 2.0 ** -23

MAIN_PREFIXES = ([f"down_blocks.{i}.resnets.{j}." for i in range(4) for j in range(2)]
                 + [f"mid_block.resnets.{j}." for j in range(2)]
                 + [f"up_blocks.{i}.resnets.{j}." for i in range(4) for j in range(3)])
IMAGE_PREFIXES = [f"down_blocks_additional.{i}.resnets.{j}." for i in range(4) for j in range(2)]


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def freqs():
    return np.exp(-math.log(1e4) * np.arange(HALF, dtype=np.float64) / HALF)


def sinusoid(t):
    """t: n integers -> float64 [n, 320]"""
    arg = _f64(t).reshape(-1, 1) * freqs()[None, :]
    return np.concatenate([np.cos(arg), np.sin(arg)], axis=1)


def sinusoid_tol(t):
    """the allowed absolute error of each of the 320 columns, float64 [n, 320]"""
    f = freqs()
    tol = 2.0 ** -22 * (1.0 + _f64(t).reshape(-1, 1) * (f * (1.0 + np.abs(np.log(f))))[None, :])
    return np.concatenate([tol, tol], axis=1)


def silu(x):
    x = _f64(x)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def silu_delta(x):
    x = _f64(x)
    return (np.abs(x) + 4.0) * U23 * np.abs(silu(x))


def small_linear(x, W, b=None, silu_in=False, silu_out=False):
    """x [B, K], W [N, K], b [N] or None -> float64 [B, N]"""
    x, W = _f64(x), _f64(W)
    v = (silu(x) if silu_in else x) @ W.T
    if b is not None:
        v = v + _f64(b)[None, :]
    return silu(v) if silu_out else v


def small_linear_bound(x, W, b=None, silu_in=False, silu_out=False):
    """the allowed absolute error of each output, float64 [B, N] (module docstring)"""
    x, W = _f64(x), _f64(W)
    K = x.shape[1]
    aw = np.abs(W).T
    mag = np.abs(silu(x) if silu_in else x) @ aw
    if b is not None:
        assert (np.abs(_f64(b))[None, :] <= 16.0 * mag).all(), "a bias dominates its products: the bound does not cover this input"
    bound = (math.ceil(K / 64) + 8) * U23 * mag
    if silu_in:
        bound = bound + silu_delta(x) @ aw
    if silu_out:
        bound = bound + silu_delta(small_linear(x, W, b, silu_in, False))
    return bound


def embed(sd, ts, sinus=None):
    """time_embedding(sinusoid(ts)) -> float64 [n, 1280]; sinus: the sinusoid to start from instead of this module's"""
    s = sinusoid(ts) if sinus is None else _f64(sinus)
    e = small_linear(s, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"], False, True)
    return small_linear(e, sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])


def rows(sd, ts, prefixes, sinus=None):
    """the time-embedding rows of n timesteps for the resnets under `prefixes`, float64 [n, sum of their channels]"""
    emb = embed(sd, ts, sinus)
    return np.concatenate([small_linear(emb, sd[p + "time_emb_proj.weight"], sd[p + "time_emb_proj.bias"], True, False)
                           for p in prefixes], axis=1)


def time_keys(prefixes):
    """the state-dict keys `rows` reads for a table"""
    keys = [f"time_embedding.linear_{i}.{w}" for i in (1, 2) for w in ("weight", "bias")]
    return keys + [p + "time_emb_proj." + w for p in prefixes for w in ("weight", "bias")]


def descending_timesteps(n):
    """n distinct timesteps descending from 999 and ending at 0 (n = 1: [999])"""
    if n == 1:
        return [999]
    return [int(round(999 * (n - 1 - i) / (n - 1))) for i in range(n)]

"""GPU suite: the time-embedding path - time_sinus_kernel and small_linear_kernel (csrc/misc.hip), which run in fp32 in every
forward of every compute mode and stay out of the dispatch log, and the host logic around them: time_mlp's chunks of 64 rows,
the table of the sampling loops and its growth beyond 64 steps, and the three ways a forward takes its timestep.

The kernels are held to the float64 restatement and the derived bounds of tests/time_embed_ref.py; the handle's rows are
held bit for bit to what this file composes from the two operators on the state dict's own tensors, in the model's order.

Measured on an MI355X, largest error / bound over all cases of a test:
    time_sinus_kernel     0.276  (t = 1000; 0.270 at t = 999, 0.122 at t = 1, exact at t = 0)
    small_linear_kernel   0.048  (B 2, K 64, N 1281, both SiLU flags); 0.023 at (3, 320, 1280) with silu_in; 0.011 on inputs
                          in +-30, where the delta term of the hardware exp / rcp is largest; 0.039 at B = 65
Max-norm relative error of the rows of the 130 timesteps from 999 down to 0 against the float64 rows:
    table                       fp32 CPU chain of oracle/unet.py    device
    plain UNet, main            7.975e-06                           7.740e-06
    separate encoder, main      8.401e-06                           8.579e-06
    separate encoder, image     9.164e-06                           9.147e-06
(both are the fp32 rounding of the sinusoid's argument at large t, carried through the three Linears; the device is allowed
16 times the CPU chain's error)."""
import ctypes as C

import numpy as np
import pytest
import torch

import time_embed_ref as ref
from conftest import rel_err
from oracle import unet as o_unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 640                                            # NaN guard elements (two sinusoid rows) before and behind every output


def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Guarded:
    """a device output of n floats with NaN guards on both sides"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
        self.out = self.buf[GUARD:GUARD + n]

    def read(self, *shape):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert torch.isnan(b[:GUARD]).all() and torch.isnan(b[GUARD + self.n:]).all(), "a guard element was written"
        out = b[GUARD:GUARD + self.n]
        assert torch.isfinite(out).all()
        return out.reshape(*shape).clone()


# ------------------------------------------------------------------ 1. the sinusoid
TS = [0, 1, 2, 19, 259, 500, 998, 999, 1000]


def run_sinusoid(t_dev, t_count, t_host, B):
    g = Guarded(B * 320)
    assert lib().ldmseg_op_time_sinusoid(P(t_dev), t_count, t_host, B, P(g.out), None) == 0
    return g.read(B, 320)


def test_sinusoid_vs_float64():
    per_sample = run_sinusoid(torch.tensor(TS, dtype=torch.int64, device=DEV), len(TS), 0, len(TS))
    ratio = np.abs(per_sample.double().numpy() - ref.sinusoid(TS)) / ref.sinusoid_tol(TS)
    worst = ratio.max(axis=1)
    print("sinusoid error / bound per timestep: " + ", ".join(f"t={t} {r:.3f}" for t, r in zip(TS, worst)))
    assert ratio.shape == (len(TS), 320) and worst.max() <= 1.0, dict(zip(TS, worst))
    # the three routes agree bit for bit at equal t
    for t in TS:
        row = per_sample[TS.index(t)]
        one = run_sinusoid(torch.tensor([t], dtype=torch.int64, device=DEV), 1, -5, 3)      # (t_host is ignored with t_dev)
        assert all(torch.equal(one[b], row) for b in range(3)), ("one-element t_dev", t)
        if t in (0, 500, 999):
            host = run_sinusoid(None, 1, t, 2)
            assert torch.equal(host[0], row) and torch.equal(host[1], row), ("host scalar", t)
    assert torch.equal(per_sample[0], torch.cat([torch.ones(160), torch.zeros(160)]))         # t = 0: exactly [1 | 0]


def test_sinusoid_refusals_on_the_device():
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.zeros(4 * 320, device=DEV)
    for count, B in ((0, 2), (3, 2), (2, 4)):
        assert lib().ldmseg_op_time_sinusoid(P(t), count, 0, B, P(out), None) == -2
    assert lib().ldmseg_op_time_sinusoid(None, 1, 0, 0, P(out), None) == -2
    assert lib().ldmseg_op_time_sinusoid(None, 1, 0, 2, None, None) == -2


# ------------------------------------------------------------------ 2. the linear
def run_small_linear(x, W, b, silu_in, silu_out):
    B, K = x.shape
    N = W.shape[0]
    g = Guarded(B * N)
    assert lib().ldmseg_op_small_linear(P(x), P(W), P(b), B, K, N, silu_in, silu_out, P(g.out), None) == 0
    return g.read(B, N)


# B, K, N, silu_in, silu_out, bias, input
LINEAR_CASES = ([(3, 320, 1280, si, so, True, "randn3") for si in (0, 1) for so in (0, 1)]
                + [(B, 64, 8, 1, 0, True, "randn3") for B in (1, 7, 8, 9, 64, 65)]          # 65: no limit at 64 rows
                + [(2, K, 4, 0, 1, True, "randn3") for K in (1, 63, 64, 65, 1280)]
                + [(2, 64, N, 1, 1, True, "randn3") for N in (1, 3, 4, 5, 1281)]
                + [(3, 320, 1280, 1, 0, False, "randn3"), (2, 65, 5, 0, 0, False, "randn3")]
                + [(3, 320, 1280, 1, 1, True, "pm30"), (3, 320, 1280, 1, 0, True, "pm30")])


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_small_linear_vs_float64(case):
    B, K, N, si, so, bias, kind = case
    g = torch.Generator().manual_seed(B * 100003 + K * 101 + N + 7 * si + 13 * so)
    if kind == "pm30":            # both tails of SiLU: exp(-x) up to e^30, and the end points themselves
        x = 60.0 * torch.rand(B, K, generator=g) - 30.0
        x[0, 0], x[0, 1] = -30.0, 30.0
    else:
        x = 3.0 * torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = 0.1 * torch.randn(N, generator=g) if bias else None
    got = run_small_linear(x.to(DEV), W.to(DEV), b.to(DEV) if bias else None, si, so)
    want, bound = ref.small_linear(x, W, b, si, so), ref.small_linear_bound(x, W, b, si, so)
    ratio = float((np.abs(got.double().numpy() - want) / bound).max())
    print(f"small_linear {case}: error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_small_linear_refusals_on_the_device():
    x = torch.zeros(64, device=DEV)
    for args in ((None, P(x), None, 1, 8, 8), (P(x), None, None, 1, 8, 8), (P(x), P(x), None, 0, 8, 8), (P(x), P(x), None, 1, 0, 8),
                 (P(x), P(x), None, 1, 8, 0)):
        assert lib().ldmseg_op_small_linear(*args, 0, 0, P(x), None) == -2
    assert lib().ldmseg_op_small_linear(P(x), P(x), None, 1, 8, 8, 0, 0, None, None) == -2


# ------------------------------------------------------------------ 3. the rows of a handle
@pytest.fixture(scope="module")
def sep_sd():
    """as tests/test_separate_encoder_gpu.py builds it"""
    from ldmseg_amd import weights
    s = weights.unet_schema(4, False)
    s.update(weights.separate_encoder_schema(True))
    return weights.generate(s, seed=21)


@pytest.fixture(scope="module")
def handles(unet_sd, sep_sd):
    """name -> (handle, state dict): the fp32 UNet of the parity tests and a separate-encoder handle in the perf mode (the time
    path is fp32 in every mode)"""
    from ldmseg_amd.models import UNet
    made = {"plain": (UNet(unet_sd, in_channels=12, device=DEV, compute_dtype="fp32"), unet_sd),
            "sepenc": (UNet(sep_sd, in_channels=8, device=DEV, compute_dtype="bf16"), sep_sd)}
    yield made
    made.clear()


TABLES = [("plain", 0), ("sepenc", 0), ("sepenc", 1)]
PREFIXES = {0: ref.MAIN_PREFIXES, 1: ref.IMAGE_PREFIXES}
TOTAL = {0: 20160, 1: 7040}


def time_rows(u, ts, table):
    arr = (C.c_int64 * len(ts))(*ts)
    total = C.c_int(0)
    assert lib().ldmseg_unet_time_rows(u._h, arr, len(ts), table, None, C.byref(total), None) == 0
    assert total.value == TOTAL[table]
    g = Guarded(len(ts) * total.value)
    total2 = C.c_int(0)
    with torch.cuda.device(DEV):
        assert lib().ldmseg_unet_time_rows(u._h, arr, len(ts), table, P(g.out), C.byref(total2), None) == 0
    assert total2.value == total.value
    return g.read(len(ts), total.value)


@pytest.fixture(scope="module")
def rows130(handles):
    """(handle name, table) -> the rows of the 130 descending timesteps, computed once"""
    ts = ref.descending_timesteps(130)
    return ts, {(name, table): time_rows(handles[name][0], ts, table) for name, table in TABLES}


def composed_rows(sd_dev, ts, prefixes):
    """the rows from the two operators on the state dict's tensors: sinusoid, linear_1 + SiLU, linear_2, time_emb_proj(SiLU(.))"""
    n = len(ts)
    t = torch.tensor(ts, dtype=torch.int64, device=DEV)
    sinus, e1, emb = (torch.empty(n, c, device=DEV) for c in (320, 1280, 1280))
    assert lib().ldmseg_op_time_sinusoid(P(t), n, 0, n, P(sinus), None) == 0
    w = lambda k: P(sd_dev[k])
    assert lib().ldmseg_op_small_linear(P(sinus), w("time_embedding.linear_1.weight"), w("time_embedding.linear_1.bias"), n, 320, 1280,
                                        0, 1, P(e1), None) == 0
    assert lib().ldmseg_op_small_linear(P(e1), w("time_embedding.linear_2.weight"), w("time_embedding.linear_2.bias"), n, 1280, 1280,
                                        0, 0, P(emb), None) == 0
    outs = []
    for p in prefixes:
        cout = sd_dev[p + "time_emb_proj.bias"].numel()
        o = torch.empty(n, cout, device=DEV)
        assert lib().ldmseg_op_small_linear(P(emb), w(p + "time_emb_proj.weight"), w(p + "time_emb_proj.bias"), n, 1280, cout, 1, 0,
                                            P(o), None) == 0
        outs.append(o)
    torch.cuda.synchronize()
    return torch.cat(outs, dim=1).cpu()


@pytest.mark.parametrize("name,table", TABLES)
def test_rows_equal_the_composed_operators(handles, rows130, name, table):
    """the wiring - table order, SiLU flags, chunk offsets - with no tolerance"""
    u, sd = handles[name]
    sd_dev = {k: sd[k].to(DEV).contiguous() for k in ref.time_keys(PREFIXES[table])}
    for n in (1, 64, 65, 130):
        ts = ref.descending_timesteps(n)
        got = rows130[1][name, table] if n == 130 else time_rows(u, ts, table)
        want = composed_rows(sd_dev, ts, PREFIXES[table])
        assert got.shape == want.shape == (n, TOTAL[table])
        same = (got == want).all(dim=1)
        assert same.all(), (n, "rows that differ", (~same).nonzero().flatten().tolist()[:8])


@pytest.mark.parametrize("name,table", TABLES)
def test_rows_do_not_depend_on_the_chunk(handles, rows130, name, table):
    """row i of the 130-row call (three chunks, the last of two rows) = the one-row call for its timestep"""
    u, _ = handles[name]
    ts, rows = rows130
    for i, t in enumerate(ts):
        assert torch.equal(time_rows(u, [t], table)[0], rows[name, table][i]), (i, t)


CHAIN_FACTOR = 16            # hardware exp / rcp in SiLU and another summation order, over the fp32 CPU chain's own error


@pytest.mark.parametrize("name,table", TABLES)
def test_rows_vs_float64(handles, rows130, name, table):
    _, sd = handles[name]
    ts, rows = rows130
    prefixes = PREFIXES[table]
    want = ref.rows(sd, ts, prefixes)
    with torch.no_grad():          # the fp32 chain of oracle/unet.py: unet_forward's embedding, resnet's time_emb_proj line
        F = torch.nn.functional
        emb = o_unet.timestep_embedding(torch.tensor(ts))
        emb = F.linear(emb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
        emb = F.linear(F.silu(emb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
        cpu = torch.cat([F.linear(F.silu(emb), sd[p + "time_emb_proj.weight"], sd[p + "time_emb_proj.bias"]) for p in prefixes], 1)
    e_cpu, e_gpu = rel_err(cpu, want), rel_err(rows[name, table], want)
    print(f"rows {name} table {table}: fp32 CPU chain {e_cpu:.3e}, device {e_gpu:.3e} against float64")
    assert 0 < e_cpu < 1e-5
    assert e_gpu <= CHAIN_FACTOR * e_cpu


def test_time_rows_refusals(handles):
    plain, sep = handles["plain"][0], handles["sepenc"][0]
    out = torch.zeros(2 * 20160, device=DEV)
    total = C.c_int(0)
    two = (C.c_int64 * 2)(999, 0)
    neg = (C.c_int64 * 2)(999, -1)
    call = lambda h, ts, n, table: lib().ldmseg_unet_time_rows(h._h, ts, n, table, P(out), C.byref(total), None)
    assert call(plain, two, 0, 0) == -2 and call(plain, two, -1, 0) == -2
    assert call(plain, neg, 2, 0) == -2 and call(sep, neg, 2, 1) == -2
    assert call(plain, two, 2, 1) == -2                          # no image table on a plain handle
    assert call(plain, two, 2, 2) == -2 and call(sep, two, 2, 2) == -2 and call(sep, two, 2, -1) == -2
    assert lib().ldmseg_unet_time_rows(plain._h, two, 2, 0, P(out), None, None) == -2
    assert call(plain, two, 2, 0) == 0 and total.value == 20160
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 4. the routes of a forward
def test_forward_timestep_routes_agree(handles, unet_sd):
    u, _ = handles["plain"]
    x = torch.randn(2, 12, 16, 16, generator=torch.Generator().manual_seed(18))
    x_d = x.to(DEV)
    base = u(x_d, 500).sample.clone()
    assert torch.isfinite(base).all()
    for form in (torch.tensor(500), torch.tensor([500], device=DEV), torch.tensor(500, device=DEV), torch.tensor([500, 500], device=DEV)):
        assert torch.equal(u(x_d, form).sample, base), (form.device, tuple(form.shape))
    assert not torch.equal(u(x_d, torch.tensor([500, 499], device=DEV)).sample[1], base[1])   # (the second entry is read)
    with torch.no_grad():
        want = o_unet.unet_forward(unet_sd, x, torch.tensor(0))
    e = rel_err(u(x_d, 0).sample, want)
    print(f"forward at t = 0, fp32, B=2 L=16: rel_err {e:.3e}")
    assert e < 1e-3


# ------------------------------------------------------------------ 5. sampling beyond 64 steps
def test_sample_beyond_64_steps(handles, sched_kw):
    """65 steps - a second chunk of one row in time_mlp, a table of 128 - native loop = Python loop; then 5, 130 and 5 steps on the
    same handle: the table is freed and regrown to 256 rows in between and the 5-step result does not move"""
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    u, _ = handles["plain"]
    tr = TrainerDiffusion(None, u, DDIMNoiseScheduler(**sched_kw))
    rgb = (0.18215 * torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(1234))).to(DEV)
    a = tr.sample([""], num_inference_steps=65, seed=42, rgb_latents=rgb)
    s = DDIMNoiseScheduler(**sched_kw)
    s.set_timesteps_inference(65, device=DEV)
    assert len(s.timesteps) == 65
    b = tr.sample([""], num_inference_steps=65, seed=42, rgb_latents=rgb, scheduler=s, python_loop=True)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), rel_err(a, b)
    first = tr.sample([""], num_inference_steps=5, seed=42, rgb_latents=rgb).clone()
    long = tr.sample([""], num_inference_steps=130, seed=42, rgb_latents=rgb)
    again = tr.sample([""], num_inference_steps=5, seed=42, rgb_latents=rgb)
    assert torch.isfinite(long).all() and not torch.equal(long, first)
    assert torch.equal(first, again)

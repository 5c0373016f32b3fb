"""GPU parity of the CLIP text encoder (csrc/clip_text.hip, the causal form of the head-dim-64 attention and the clip-text
executor): the causal attention, the two row-local kernels and the encoder's GEMM launches one by one, then the whole model
against tests/clip_text_ref.py (which the CPU suite pins against transformers), the handle's behaviour, then the
text-conditioned sampler end to end.

The bf16 bound of the whole-model cases is not a constant: each case computes, on the CPU and from the reference alone, the
error of a bf16 simulation of the network (operands and stored activations rounded per op, fp32 accumulation) against the
fp32 reference on the case's own weights and ids; the library's bf16 result must lie within 2x that figure (the simulation
leaves the accumulation order out).  Measured figures: DESIGN.md 3.11."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_text_ref as R                                     # noqa: E402
from conftest import rel_err                                  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, X3, X3W = 0, 1, 2, 3
MODES = ("fp32", "bf16", "bf16x3")
GEMM_DT = {"fp32": F32, "bf16": BF16, "bf16x3": X3W}          # (handles hold their weights as hi | lo planes)
GEMM_TOL = {F32: 1e-4, BF16: 1.5e-2, X3W: 2e-4}               # the bounds of test_clip_vision_gpu.py
HID, MLP, T77 = 768, 3072, 77


@pytest.fixture(scope="module")
def L():
    from ldmseg_amd import _lib
    return _lib


def dev(t):
    return t.to(DEV, torch.float32).contiguous() if t is not None else None


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------ causal attention, head dim 64
def causal_inputs(B, N, heads):
    """inputs as test_clip_vision_gpu.py::test_attention_head_dim_64 builds them: Q doubled, one dominant key"""
    Cc = 64 * heads
    g = torch.Generator().manual_seed(N + Cc)
    qkv = torch.randn(B, N, 3 * Cc, generator=g)
    qkv[:, :, :Cc] *= 2.0
    qkv[0, N // 2, Cc:Cc + 40] += 6.0
    return qkv


def causal_ref(src, B, N, heads):
    """fp64 masked softmax: key j contributes to query i iff j <= i"""
    Cc = 64 * heads
    q, k, v = (t.view(B, N, heads, 64).transpose(1, 2).double() for t in src.chunk(3, -1))
    s = (q @ k.transpose(-1, -2)) * 64 ** -0.5
    s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, Cc).float()


def run_causal(L, qkv, B, N, heads, dt):
    out = torch.empty(B, N, 64 * heads, device=DEV)
    dq = dev(qkv)
    assert L.lib().ldmseg_op_attention_causal(P(dq), B, N, 64 * heads, heads, dt, P(out), None) == 0, L.lib().ldmseg_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", [F32, BF16, X3])
@pytest.mark.parametrize("B,N,heads", [(1, 1, 1), (2, 20, 2), (16, 77, 12), (3, 64, 12), (3, 65, 12), (1, 77, 1)])
def test_attention_causal(L, dt, B, N, heads):
    qkv = causal_inputs(B, N, heads)
    src = bf16_round(qkv) if dt == BF16 else qkv
    ref = causal_ref(src, B, N, heads)
    out = run_causal(L, qkv, B, N, heads, dt)
    assert bool(torch.isfinite(out).all())
    e = rel_err(out, ref)
    print("causal attention d=64", dt, (B, N, heads), e)
    assert e < (2e-2 if dt == BF16 else 2e-5)


@pytest.mark.parametrize("dt", [F32, BF16, X3])
@pytest.mark.parametrize("p", [1, 33, 64, 76])
def test_attention_causal_mask_is_exact(L, dt, p):
    """K / V rows >= p replaced by other values: output rows < p do not change by a bit (a masked score is -inf before the row
    maximum, its probability exactly zero)"""
    B, N, heads = 2, 77, 12
    Cc = 64 * heads
    qkv = causal_inputs(B, N, heads)
    other = qkv.clone()
    g = torch.Generator().manual_seed(p)
    other[:, p:, Cc:] = 3.0 * torch.randn(B, N - p, 2 * Cc, generator=g) + 1.0
    a = run_causal(L, qkv, B, N, heads, dt)
    b = run_causal(L, other, B, N, heads, dt)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert torch.equal(a[:, :p], b[:, :p])
    assert not torch.equal(a[:, p:], b[:, p:])                  # (the replaced rows do reach the rows that may see them)


# ------------------------------------------------------------------ front and final kernels
@pytest.mark.parametrize("R_,T", [(1, 1), (4, 77), (3, 20)])
def test_tokens_kernel(L, R_, T):
    vocab, Cc = 1000, HID
    g = torch.Generator().manual_seed(R_ + T)
    tok, pos = 0.02 * torch.randn(vocab, Cc, generator=g), 0.02 * torch.randn(77, Cc, generator=g)
    pos[:, 7] += 50.0
    ids = torch.randint(0, vocab, (R_, T), generator=g)
    ids[0, 0], ids[-1, -1] = vocab - 1, 0
    want = tok[ids] + pos[:T].unsqueeze(0)
    dtok, dpos, dids = dev(tok), dev(pos), ids.to(DEV)
    for dt in (F32, BF16):
        out = torch.empty(R_ * T, Cc, device=DEV)
        assert L.lib().ldmseg_op_clip_text_tokens(P(dids), P(dtok), P(dpos), R_, T, Cc, vocab, dt, P(out), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().view(R_, T, Cc)
        assert torch.equal(got, want if dt == F32 else bf16_round(want)), dt


@pytest.mark.parametrize("M,Cc", [(1, 768), (308, 768), (77, 128), (5, 1280)])
def test_final_ln_kernel(L, M, Cc):
    g = torch.Generator().manual_seed(M + Cc)
    x = torch.randn(M, Cc, generator=g) * 1.5 + 0.5
    x[:, 7 % Cc] += 27.0
    gamma, beta = 1 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    dx, dg, db = dev(x), dev(gamma), dev(beta)
    for dt in (F32, BF16):
        src = bf16_round(x) if dt == BF16 else x
        want = F.layer_norm(src.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
        out = torch.empty(M, Cc, device=DEV)
        assert L.lib().ldmseg_op_clip_text_final_ln(P(dx), P(dg), P(db), M, Cc, 1e-5, dt, P(out), None) == 0
        torch.cuda.synchronize()
        e = rel_err(out, want)
        print("final_ln", (M, Cc), dt, e)
        assert e <= 1e-5


# ------------------------------------------------------------------ the encoder's GEMM launches
GEMM_NAMES = {m: set() for m in MODES}      # dispatch names the per-op cases ran, per mode (read by the coverage test below)
GEMM_DONE = set()                           # (mode, R) whose per-op cases ran (and passed) in this session


def _logged(L, mode, fn):
    L.igemm_log(True)
    try:
        r = fn()
        torch.cuda.synchronize()
        GEMM_NAMES[mode] |= L.igemm_log_read()
    finally:
        L.igemm_log(False)
    return r


def _plain_gemm(L, mode, x, w, b, resid):
    """ldmseg_op_igemm with k = 1, H = M, W = 1: the engine's launch path with its own split-K plan"""
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty(N, M, device=DEV)
    xt, rt = dev(x.t()), dev(resid.t()) if resid is not None else None
    dw, db = dev(w), dev(b)
    r = _logged(L, mode, lambda: L.lib().ldmseg_op_igemm(P(xt), None, P(dw), P(db), P(rt), None, 1, K, 0, M, 1, N, 1, 1, 0, 0, 0, 0,
                                                          GEMM_DT[mode], P(out), None))
    assert r == 0, L.lib().ldmseg_last_error()
    return out.t()


def run_encoder_gemms(L, mode, R_):
    """layer_norm1 -> q|k|v (2304 / 768, folded LayerNorm), out_proj and fc2 with the residual (768 / 768, 768 / 3072),
    layer_norm2 -> fc1 -> quick_gelu (3072 / 768, folded LayerNorm + SiLU epilogue with the 1.702 fold, the reference being the
    textbook x * sigmoid(1.702 x)) at M = 77 R against F.linear on rounded operands."""
    torch.set_num_threads(16)
    dt = GEMM_DT[mode]
    tol = GEMM_TOL[dt]
    M = T77 * R_
    g = torch.Generator().manual_seed(R_)
    rnd = bf16_round if dt == BF16 else (lambda t: t)
    x = torch.randn(M, HID, generator=g) * 1.5 + 0.5
    gamma, beta = 1 + 0.2 * torch.randn(HID, generator=g), 0.2 * torch.randn(HID, generator=g)
    lib = L.lib()

    def ln_linear(N, silu):
        w = torch.randn(N, HID, generator=g) / HID ** 0.5
        b = 0.1 * torch.randn(N, generator=g)
        y = F.linear(F.layer_norm(rnd(x), (HID,), gamma, beta, 1e-5).double(), w.double(), b.double())
        out = torch.empty(M, N, device=DEV)
        dx, dg, db_, = dev(x), dev(gamma), dev(beta)
        if silu:
            y = y * torch.sigmoid(1.702 * y)                      # quick_gelu, fold undone: the library gets 1.702 w, 1.702 b
            dw, dbias = dev(1.702 * w), dev(1.702 * b)
            r = _logged(L, mode, lambda: lib.ldmseg_op_ln_linear_silu(P(dx), P(dg), P(db_), P(dw), P(dbias), M, HID, N, 1e-5, dt, P(out), None))
            out = out / 1.702                                     # (the executor folds this factor into fc2's weights)
        else:
            dw, dbias = dev(w), dev(b)
            r = _logged(L, mode, lambda: lib.ldmseg_op_ln_linear(P(dx), P(dg), P(db_), P(dw), P(dbias), M, HID, N, 1e-5, 0, dt, P(out), None))
        assert r == 0, lib.ldmseg_last_error()
        torch.cuda.synchronize()
        return rel_err(out, y)

    figures = {"ln1->qkv": ln_linear(3 * HID, False), "ln2->fc1+quick_gelu": ln_linear(MLP, True)}
    for name, K in (("out_proj", HID), ("fc2", MLP)):
        xa = torch.randn(M, K, generator=g)
        w = torch.randn(HID, K, generator=g) / K ** 0.5
        b = 0.1 * torch.randn(HID, generator=g)
        res = torch.randn(M, HID, generator=g)
        ref = F.linear(rnd(xa).double(), rnd(w).double(), b.double()) + rnd(res).double()
        figures[name] = rel_err(_plain_gemm(L, mode, xa, w, b, res), ref)
    print("text encoder GEMMs", mode, "R =", R_, figures)
    for name, e in figures.items():
        assert e < tol, (name, e, L.igemm_last_kernel())
    GEMM_DONE.add((mode, R_))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R_", [2, 16])
def test_encoder_gemm_shapes(L, mode, R_):
    run_encoder_gemms(L, mode, R_)


# ------------------------------------------------------------------ whole model
class Bench:
    """weights, CPU references and library handles of one (configuration, outlier) pair, built on demand and shared"""

    def __init__(self, cfg, outliers):
        from ldmseg_amd import weights
        self.cfg = cfg
        schema = weights.clip_text_schema(**cfg)
        sd = weights.generate(schema, seed=23, norm_keys=weights.clip_text_norm_keys(schema))
        if outliers:
            # a few channels far above the rest, same sign so that the row mean moves too (real CLIP residual streams)
            sd["embeddings.position_embedding.weight"][:, 7] += 50.0
            sd["embeddings.position_embedding.weight"][:, min(300, cfg["hidden"] - 1)] += 30.0
        self.sd = sd
        self.handles, self.refs = {}, {}

    def model(self, mode):
        from ldmseg_amd.models import CLIPTextEncoder
        if mode not in self.handles:
            self.handles[mode] = CLIPTextEncoder(self.sd, device=DEV, compute_dtype=mode)
        return self.handles[mode]

    def ids(self, starts, T=None, seed=0):
        return R.prompt_ids(starts, T or self.cfg["positions"], self.cfg["vocab"], seed=seed)

    def ref(self, key, ids):
        """(fp32 reference, simulated bf16 error), cached per key"""
        if key not in self.refs:
            torch.set_num_threads(16)
            with torch.no_grad():
                ref = R.forward(self.sd, ids, self.cfg["heads"])
                sim = R.forward(self.sd, ids, self.cfg["heads"], rnd=bf16_round)
            assert bool(torch.isfinite(ref).all())
            self.refs[key] = (ref, rel_err(sim, ref))
        return self.refs[key]


_BENCHES = {}


def bench(size, outliers):
    if (size, outliers) not in _BENCHES:
        _BENCHES[(size, outliers)] = Bench(R.SMALL if size == "small" else R.FULL, outliers)
    return _BENCHES[(size, outliers)]


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("size", ["small", "full"])
def test_whole_model(size, outliers):
    """last_hidden_state at R = 4 (padding from positions 1, 6, 40 and 76) in the three modes against the reference: fp32 / bf16x3
    <= 1e-3, bf16 <= 2x the CPU-simulated bf16 error of the same weights and ids.  outliers: +50 on channel 7 and +30 on channel
    300 of every position row, where the folded LayerNorm's rstd * (acc - mean * c1) would lose digits."""
    bn = bench(size, outliers)
    ids = bn.ids([1, 6, 40, 76])
    ref, sim = bn.ref("r4", ids)
    for mode in MODES:
        m = bn.model(mode)
        out = m(ids.to(DEV))
        torch.cuda.synchronize()
        hid = out[0]
        assert hid is out.last_hidden_state and hid.dtype == torch.float32 and hid.is_cuda
        assert hid.shape == (4, bn.cfg["positions"], bn.cfg["hidden"]) and bool(torch.isfinite(hid).all())
        e = rel_err(hid, ref)
        print(f"whole model {size} outliers={outliers}", mode, "last_hidden_state %.3e" % e, "(simulated bf16 %.3e)" % sim,
              "output max %.2f" % float(ref.abs().max()))
        if mode == "bf16":
            assert e <= 2 * sim, (e, sim)
        else:
            assert e <= 1e-3, (mode, e)
        assert torch.equal(m.forward(ids.to(torch.int32))[0], hid)          # int32 ids on the CPU: the same call
    if size == "full":
        assert bn.model("fp32").num_parameters == 123_060_480


@pytest.mark.parametrize("mode", MODES)
def test_every_gemm_of_a_forward_was_compared(L, mode):
    """the dispatch log of one full-size forward at R = 2 and at R = 16: every GEMM-family kernel in it is one the per-op cases
    above ran (and compared) - the project's coverage rule applied to this executor"""
    for R_ in (2, 16):
        if (mode, R_) not in GEMM_DONE:          # (run on its own: the per-op comparisons first)
            run_encoder_gemms(L, mode, R_)
    bn = bench("full", False)
    m = bn.model(mode)
    seen = set()
    for R_ in (2, 16):
        ids = bn.ids([3 + 4 * i for i in range(R_)], seed=R_).to(DEV)
        L.igemm_log(True)
        try:
            m(ids)
            torch.cuda.synchronize()
            seen |= L.igemm_log_read()
        finally:
            L.igemm_log(False)
    print(mode, sorted(seen))
    assert seen and seen <= GEMM_NAMES[mode], (sorted(seen - GEMM_NAMES[mode]), sorted(GEMM_NAMES[mode]))
    # and the other kernels of a forward are the text executor's own, the causal attention among them
    L.igemm_log(L.LOG_ALL)
    try:
        m(bn.ids([5, 9]).to(DEV))
        torch.cuda.synchronize()
        every = L.igemm_log_read()
    finally:
        L.igemm_log(False)
    tag = "bf16" if mode == "bf16" else "f32"
    assert {f"clip_text_tokens<{tag}>", f"clip_text_final_ln<{tag}>"} <= every, sorted(every)
    assert ("attn_causal_x3<64,1>" if mode == "bf16x3" else f"attn_causal<{tag},64,1>") in every, sorted(every)
    assert not any(n.startswith(("attn<", "attn_x3<", "attn3", "clip_rows_to_f32")) for n in every), sorted(every)


# ------------------------------------------------------------------ handle behaviour
def test_handle_reuse_across_shapes():
    """one handle across (R, T) = (16, 77) -> (2, 77) -> (2, 20) -> (16, 77): bit-equal to fresh handles"""
    from ldmseg_amd.models import CLIPTextEncoder
    bn = bench("small", False)
    ids16 = bn.ids([2 + 4 * i for i in range(16)], seed=3).to(DEV)
    calls = [ids16, ids16[:2].contiguous(), ids16[:2, :20].contiguous(), ids16]
    for mode in MODES:
        m = bn.model(mode)
        outs = [m(x)[0].clone() for x in calls]
        assert torch.equal(outs[0], outs[3])
        for x, o in zip(calls[:3], outs):
            fresh = CLIPTextEncoder(bn.sd, device=DEV, compute_dtype=mode)
            assert torch.equal(fresh(x)[0], o), (mode, tuple(x.shape))
            del fresh


@pytest.mark.parametrize("size", ["small", "full"])
def test_later_tokens_do_not_reach_earlier_rows(size):
    """through the handle: changing ids[:, p:] leaves rows < p bit-equal"""
    bn = bench(size, False)
    ids = bn.ids([10, 50, 76], seed=8)
    for mode in MODES:
        m = bn.model(mode)
        a = m(ids.to(DEV))[0].clone()
        for p in (1, 33, 64, 76):
            other = ids.clone()
            other[:, p:] = torch.randint(0, bn.cfg["vocab"], (3, 77 - p), generator=torch.Generator().manual_seed(p))
            b = m(other.to(DEV))[0]
            assert torch.equal(a[:, :p], b[:, :p]), (mode, p)
            assert not torch.equal(a[:, p:], b[:, p:])


def test_bad_inputs_raise(L):
    from ldmseg_amd import _lib
    from ldmseg_amd.models import CLIPTextEncoder
    full, small = bench("full", False), bench("small", False)
    m = full.model("fp32")
    ids = full.ids([4])
    with pytest.raises(ValueError):
        m(torch.cat([ids, ids[:, :1]], 1))                                              # T = 78
    with pytest.raises(ValueError):
        m(ids[0])                                                                       # rank 1
    with pytest.raises(ValueError):
        m(ids.float())
    bad = ids.clone()
    bad[0, 3] = 49408
    with pytest.raises(IndexError):
        m(bad)
    bad[0, 3] = -1
    with pytest.raises(IndexError):
        m(bad.to(DEV))
    with pytest.raises(RuntimeError):
        CLIPTextEncoder(small.sd, device="cpu")
    with pytest.raises(KeyError):
        CLIPTextEncoder({k: v for k, v in small.sd.items() if "fc2.bias" not in k}, device=DEV)
    # configurations the kernels do not serve: LDMSEG_E_SHAPE at create time, never a fallback
    for badcfg in (dict(heads=4), dict(heads=1)):                                       # head dim 32 / 128
        with pytest.raises(RuntimeError, match="code -2"):
            CLIPTextEncoder(small.sd, device=DEV, config=dict(R.SMALL, **badcfg))
    n, names, ptrs, numels, keep = _lib.weight_arrays(small.sd, torch.device(DEV))
    for fields in ((512, 77, 128, 520, 2, 2),                                           # MLP size no multiple of 64
                   (512, 77, 1344, 512, 2, 21),                                         # wider than the statistics kernel serves
                   (512, 77, 96, 512, 2, 2),                                            # hidden no multiple of 64
                   (512, 77, 128, 512, 2, 2)):                                          # (the last one is valid: the loop's control)
        cfg = _lib.ClipTextCfg(*fields, _lib.F32, 0)
        h = C.c_void_p()
        rc = L.lib().ldmseg_clip_text_create(C.byref(cfg), n, names, ptrs, numels, C.byref(h))
        if fields == (512, 77, 128, 512, 2, 2):
            assert rc == 0, L.lib().ldmseg_last_error()
            # call-time shape checks of the C ABI itself
            x = small.ids([3]).to(DEV)
            out = torch.empty(1, 78, 128, device=DEV)
            st = _lib.stream_ptr(torch.device(DEV))
            assert L.lib().ldmseg_clip_text_forward(h, P(x), 1, 78, P(out), st) == -2
            assert L.lib().ldmseg_clip_text_forward(h, P(x), 1, 0, P(out), st) == -2
            assert L.lib().ldmseg_clip_text_forward(h, P(x), 0, 77, P(out), st) == -2
            assert L.lib().ldmseg_clip_text_forward(h, None, 1, 77, P(out), st) == -1
            assert L.lib().ldmseg_clip_text_forward(h, P(x), 1, 77, P(out), st) == 0
            torch.cuda.synchronize()
            L.lib().ldmseg_clip_text_destroy(h)
        else:
            assert rc == -2 and not h.value, (fields, rc)
    del keep
    wrong = dict(small.sd)
    wrong["final_layer_norm.weight"] = torch.ones(64)
    with pytest.raises(RuntimeError, match="code -4"):
        CLIPTextEncoder(wrong, device=DEV, config=dict(R.SMALL))
    assert m.eval() is m and m.to("cpu") is m and m.requires_grad_(False) is m


# ------------------------------------------------------------------ end to end
class StandInTokenizer:
    """what the sampler needs of a CLIPTokenizer: BOS, one id per word (a hash of it), EOS padding to model_max_length"""
    model_max_length = 77
    vocab, bos, eos = 49408, 49406, 49407

    class Batch:
        def __init__(self, ids):
            self.input_ids = ids

    def __call__(self, prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt"):
        import zlib
        ids = torch.full((len(prompts), max_length), self.eos, dtype=torch.int64)
        ids[:, 0] = self.bos
        for r, text in enumerate(prompts):
            for t, word in enumerate(text.split()[:max_length - 2]):
                ids[r, t + 1] = zlib.crc32(word.encode()) % self.bos
        return self.Batch(ids)


class CpuTextEncoder(torch.nn.Module):
    """the reference forward on the CPU behind CLIPTextModel's call surface (a plain torch module in the text encoder slot)"""

    def __init__(self, sd, heads):
        super().__init__()
        self.sd, self.heads = sd, heads

    def forward(self, input_ids):
        torch.set_num_threads(16)
        return (R.forward(self.sd, input_ids.cpu(), self.heads).to(input_ids.device),)


def test_text_conditioned_sampling_end_to_end(sched_kw):
    """TrainerDiffusion with the library's text encoder and a stand-in tokenizer on a cross-attention fp32 UNet, L = 16, 4 guided
    steps: the context is cat([uncond, text]) of direct encoder calls, native guided loop == python loop bitwise, and both lie
    within 1e-3 of the run whose context the reference computes on the CPU behind a plain torch module."""
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet, CLIPTextEncoder
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    bn = bench("full", False)
    unet = UNet(weights.generate(weights.unet_schema(8, True), seed=11), in_channels=8, device=DEV, compute_dtype="fp32",
                cross_attention=True)
    enc = CLIPTextEncoder(bn.sd, device=DEV, compute_dtype="fp32")
    tok = StandInTokenizer()

    def sched():
        s = DDIMNoiseScheduler(**sched_kw)
        s.set_timesteps_inference(4)
        return s
    g = torch.Generator().manual_seed(6)
    rgb = (0.18215 * torch.randn(2, 4, 16, 16, generator=g)).to(DEV)
    noise = torch.randn(2, 4, 16, 16, generator=g)
    prompts = ["a photo of two cats on a couch", "street with a red bus"]
    tr = TrainerDiffusion(None, unet, None, textencoder=enc, tokenizer=tok)
    ehs, mult = tr.encoder_hidden_states(prompts)
    assert mult == 2 and ehs.shape == (4, 77, 768) and ehs.dtype == torch.float32
    direct = torch.cat([enc(tok([""] * 2).input_ids)[0], enc(tok(prompts).input_ids)[0]])
    assert torch.equal(ehs, direct)
    assert not torch.equal(ehs[:2], ehs[2:])
    a = tr.sample(prompts, 4, 7.5, rgb_latents=rgb, scheduler=sched(), latents=noise)
    b = tr.sample(prompts, 4, 7.5, rgb_latents=rgb, scheduler=sched(), latents=noise, python_loop=True)
    assert torch.equal(a, b)
    tr2 = TrainerDiffusion(None, unet, None, textencoder=CpuTextEncoder(bn.sd, 12), tokenizer=tok)
    ehs2, _ = tr2.encoder_hidden_states(prompts)
    assert ehs2.shape == ehs.shape and rel_err(ehs, ehs2) <= 1e-3
    c = tr2.sample(prompts, 4, 7.5, rgb_latents=rgb, scheduler=sched(), latents=noise)
    e = rel_err(a, c)
    print("end to end: context", rel_err(ehs, ehs2), "latents", e)
    assert bool(torch.isfinite(a).all()) and e <= 1e-3

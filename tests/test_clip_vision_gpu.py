"""GPU parity of the CLIP vision encoder (csrc/clip_vision.hip + the clip-vision executor): the head-dim-64 attention, the
encoder's GEMM launches and the front kernel one by one, then the whole model against tests/clip_vision_ref.py (which the
CPU suite pins against transformers), then the conditioned sampler end to end.

bf16 bounds of the whole-model cases are not constants: each case computes, on the CPU and from the reference alone, the
error of a bf16 simulation of the network (operands and stored activations rounded per op, fp32 accumulation) against the
fp32 reference on the case's own weights and input; the library's bf16 result must lie within 2x that figure (the
simulation leaves the accumulation order out).  Figures seen on an MI355X (2026-10-16), full size, B = 3, max-norm relative,
last_hidden_state / image_embeds: simulated 2.13e-2 / 1.16e-2, library bf16 1.95e-2 / 1.34e-2; with the outlier channels
simulated 2.82e-2 / 1.28e-2, library 2.71e-2 / 1.26e-2; fp32 <= 1.3e-6 and bf16x3 <= 1.1e-5 throughout."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_vision_ref as R                                   # noqa: E402
from conftest import rel_err                                  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, X3, X3W = 0, 1, 2, 3
FULL = dict(hidden=1024, intermediate=4096, layers=24, heads=16, image=224, patch=14, projection_dim=768)
MODES = ("fp32", "bf16", "bf16x3")
GEMM_DT = {"fp32": F32, "bf16": BF16, "bf16x3": X3W}          # (handles hold their weights as hi | lo planes)
GEMM_TOL = {F32: 1e-4, BF16: 1.5e-2, X3W: 2e-4}      # (X3W: the bound of test_ops_gpu.py::test_split_bf16_layernorm_folded_gemm)


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


# ------------------------------------------------------------------ attention, head dim 64
@pytest.mark.parametrize("dt", [F32, BF16, X3])
@pytest.mark.parametrize("B,N,heads", [(1, 10, 2), (2, 257, 16), (8, 257, 16), (1, 64, 1), (3, 300, 4)])
def test_attention_head_dim_64(L, dt, B, N, heads):
    """inputs as test_ops_gpu.py::test_attention builds them: Q doubled, one dominant key, bf16 operands rounded first"""
    Cc = 64 * heads
    g = torch.Generator().manual_seed(N + Cc)
    qkv = torch.randn(B, N, 3 * Cc, generator=g)
    qkv[:, :, :Cc] *= 2.0
    qkv[0, N // 2, Cc:Cc + 40] += 6.0
    src = bf16_round(qkv) if dt == BF16 else qkv
    q, k, v = (t.view(B, N, heads, 64).transpose(1, 2).double() for t in src.chunk(3, -1))
    ref = (torch.softmax((q @ k.transpose(-1, -2)) * 64 ** -0.5, -1) @ v).transpose(1, 2).reshape(B, N, Cc).float()
    out = torch.empty(B, N, Cc, device=DEV)
    dq = dev(qkv)
    assert L.lib().ldmseg_op_attention(P(dq), B, N, Cc, heads, dt, P(out), None) == 0, L.lib().ldmseg_last_error()
    torch.cuda.synchronize()
    e = rel_err(out, ref)
    print("attention d=64", dt, (B, N, heads), e)
    assert e < (2e-2 if dt == BF16 else 2e-5)


# ------------------------------------------------------------------ the encoder's GEMM launches
GEMM_NAMES = {m: set() for m in MODES}      # dispatch names the per-op cases ran, per mode (read by the coverage test below)
GEMM_DONE = set()                           # (mode, B) whose per-op cases ran (and passed) in this session


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


def run_encoder_gemms(L, mode, B):
    """layer_norm1 -> q|k|v (3072 / 1024, folded LayerNorm), out_proj and fc2 with the residual (1024 / 1024, 1024 / 4096),
    layer_norm2 -> fc1 -> quick_gelu (4096 / 1024, folded LayerNorm + SiLU epilogue with the 1.702 fold, the reference being the
    textbook x * sigmoid(1.702 x)), and the patch GEMM (K = 640) at M = 257 B (256 B) against F.linear on rounded operands."""
    torch.set_num_threads(16)
    dt = GEMM_DT[mode]
    tol = GEMM_TOL[dt]
    M = 257 * B
    g = torch.Generator().manual_seed(B)
    rnd = bf16_round if dt == BF16 else (lambda t: t)
    x = torch.randn(M, 1024, generator=g) * 1.5 + 0.5
    gamma, beta = 1 + 0.2 * torch.randn(1024, generator=g), 0.2 * torch.randn(1024, generator=g)
    lib = L.lib()

    def ln_linear(N, silu):
        w = torch.randn(N, 1024, generator=g) / 32.0
        b = 0.1 * torch.randn(N, generator=g)
        y = F.linear(F.layer_norm(rnd(x), (1024,), gamma, beta, 1e-5).double(), w.double(), b.double())
        out = torch.empty(M, N, device=DEV)
        dx, dg, db_, = dev(x), dev(gamma), dev(beta)
        if silu:
            y = y * torch.sigmoid(1.702 * y)                      # quick_gelu, fold undone: the library gets 1.702 w, 1.702 b
            dw, dbias = dev(1.702 * w), dev(1.702 * b)
            r = _logged(L, mode, lambda: lib.ldmseg_op_ln_linear_silu(P(dx), P(dg), P(db_), P(dw), P(dbias), M, 1024, N, 1e-5, dt, P(out), None))
            out = out / 1.702                                     # (the executor folds this factor into fc2's weights)
        else:
            dw, dbias = dev(w), dev(b)
            r = _logged(L, mode, lambda: lib.ldmseg_op_ln_linear(P(dx), P(dg), P(db_), P(dw), P(dbias), M, 1024, N, 1e-5, 0, dt, P(out), None))
        assert r == 0, lib.ldmseg_last_error()
        torch.cuda.synchronize()
        return rel_err(out, y)

    figures = {"ln1->qkv": ln_linear(3072, False), "ln2->fc1+quick_gelu": ln_linear(4096, True)}
    for name, K, Mrows in (("out_proj", 1024, M), ("fc2", 4096, M), ("patch", 640, 256 * B)):
        xa = torch.randn(Mrows, K, generator=g)
        w = torch.randn(1024, K, generator=g) / K ** 0.5
        b = 0.1 * torch.randn(1024, generator=g) if name != "patch" else None
        res = torch.randn(Mrows, 1024, generator=g) if name != "patch" else None
        ref = F.linear(rnd(xa).double(), rnd(w).double(), b.double() if b is not None else None)
        if res is not None:
            ref = ref + rnd(res).double()
        figures[name] = rel_err(_plain_gemm(L, mode, xa, w, b, res), ref)
    print("encoder GEMMs", mode, "B =", B, figures)
    for name, e in figures.items():
        assert e < tol, (name, e, L.igemm_last_kernel())
    GEMM_DONE.add((mode, B))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 8])
def test_encoder_gemm_shapes(L, mode, B):
    run_encoder_gemms(L, mode, B)


# ------------------------------------------------------------------ front kernel
@pytest.mark.parametrize("H,W", [(512, 512), (480, 640), (224, 224), (37, 53)])
def test_front_kernel(L, H, W):
    """resize + normalise + im2col in one kernel against F.interpolate, (x - mean) / std, F.unfold on the CPU"""
    B, S, Pp = 2, 224, 14
    img = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    ref = F.unfold(R.norm_resize(img, S), Pp, stride=Pp).transpose(1, 2).reshape(B * 256, 588)
    mean, std = (C.c_float * 3)(*R.PIXEL_MEAN_CLIP), (C.c_float * 3)(*R.PIXEL_STD_CLIP)
    dimg = dev(img)
    for dt in (F32, BF16):
        out = torch.empty(B * 256, 640, device=DEV)
        assert L.lib().ldmseg_op_clip_patch_rows(P(dimg), B, H, W, S, Pp, mean, std, 1, dt, P(out), None) == 0
        torch.cuda.synchronize()
        out = out.cpu()
        assert float(out[:, 588:].abs().max()) == 0.0              # the K padding
        got = out[:, :588]
        if dt == F32:
            e = float((got - ref).abs().max())
            print("front kernel fp32", (H, W), e)
            assert e <= 1e-5
        else:
            rr = bf16_round(ref)
            ulp = torch.maximum(rr.abs(), torch.tensor(2.0 ** -126)).log2().floor().add(-7).exp2()      # bf16: 8 significant bits
            assert bool(((got - rr).abs() <= ulp).all()), float(((got - rr).abs() / ulp).max())
    # the prepared-input entry copies pixel_values as they are
    pv = R.norm_resize(img, S)
    out = torch.empty(B * 256, 640, device=DEV)
    dpv = dev(pv)
    assert L.lib().ldmseg_op_clip_patch_rows(P(dpv), B, S, S, S, Pp, None, None, 0, F32, P(out), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[:, :588], F.unfold(pv, Pp, stride=Pp).transpose(1, 2).reshape(B * 256, 588))


# ------------------------------------------------------------------ whole model
class Bench:
    """weights, inputs, CPU references and library handles of one (configuration, outlier) pair, built on demand and shared"""

    def __init__(self, cfg, outliers):
        from ldmseg_amd import weights
        self.cfg = cfg
        schema = weights.clip_vision_schema(**cfg)
        sd = weights.generate(schema, seed=21, norm_keys=weights.clip_vision_norm_keys(schema))
        if outliers:
            # a few channels far above the rest, same sign so that the row mean moves too (real CLIP-L residual streams)
            sd["embeddings.class_embedding"][7] += 50.0
            sd["embeddings.position_embedding.weight"][:, 7] += 50.0
            sd["embeddings.position_embedding.weight"][:, min(300, cfg["hidden"] - 1)] += 30.0
        self.sd = sd
        self.handles, self.refs = {}, {}

    def model(self, mode):
        from ldmseg_amd.models import CLIPVisionDescriptor
        if mode not in self.handles:
            self.handles[mode] = CLIPVisionDescriptor(self.sd, projection=True, device=DEV, compute_dtype=mode)
        return self.handles[mode]

    def pixels(self, B, seed=0):
        return torch.randn(B, 3, self.cfg["image"], self.cfg["image"], generator=torch.Generator().manual_seed(100 + B + seed))

    def ref(self, key, x):
        """(fp32 reference, simulated bf16 error of last_hidden_state, of image_embeds), cached per input key"""
        if key not in self.refs:
            torch.set_num_threads(16)
            with torch.no_grad():
                ref = R.forward(self.sd, x, self.cfg["heads"])
                sim = R.forward(self.sd, x, self.cfg["heads"], rnd=bf16_round)
            self.refs[key] = (ref, rel_err(sim["last_hidden_state"], ref["last_hidden_state"]),
                              rel_err(sim["image_embeds"], ref["image_embeds"]))
        return self.refs[key]


_BENCHES = {}


def bench(size, outliers):
    if (size, outliers) not in _BENCHES:
        # one full-size set of handles at a time: each holds 1.2 GB (fp32) of parameters
        for k in [k for k in _BENCHES if k[0] == "full" and size == "full"]:
            del _BENCHES[k]
        _BENCHES[(size, outliers)] = Bench(R.SMALL if size == "small" else FULL, outliers)
    return _BENCHES[(size, outliers)]


def check_outputs(mode, hid, emb, ref, sim_h, sim_e, what):
    eh, ee = rel_err(hid, ref["last_hidden_state"]), rel_err(emb, ref["image_embeds"])
    print(what, mode, "last_hidden_state %.3e image_embeds %.3e" % (eh, ee), "(simulated bf16 %.3e %.3e)" % (sim_h, sim_e))
    if mode == "bf16":
        assert eh <= 2 * sim_h and ee <= 2 * sim_e, (what, eh, sim_h, ee, sim_e)
    else:
        assert eh <= 1e-3 and ee <= 1e-3, (what, mode, eh, ee)


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("size", ["small", "full"])
def test_whole_model(size, outliers):
    """last_hidden_state, image_embeds and the wrappers' last_feat at B = 1 and 3 in the three modes against the reference;
    fp32 / bf16x3 <= 1e-3, bf16 <= 2x the CPU-simulated bf16 error of the same weights and input.  outliers: +50 on channel 7 of
    the class token and every position row, +30 on channel 300 of the position table - after pre_layrnorm these channels sit
    near 27 against a typical 1, which is where the folded LayerNorm's rstd * (acc - mean * c1) would lose digits."""
    bn = bench(size, outliers)
    T = (bn.cfg["image"] // bn.cfg["patch"]) ** 2 + 1
    for B in (1, 3):
        x = bn.pixels(B)
        ref, sim_h, sim_e = bn.ref(("pv", B), x)
        dx = x.to(DEV)
        for mode in MODES:
            m = bn.model(mode)
            hid, emb = m.encode(dx)
            torch.cuda.synchronize()
            assert hid.shape == (B, T, bn.cfg["hidden"]) and emb.shape == (B, bn.cfg["projection_dim"])
            check_outputs(mode, hid, emb, ref, sim_h, sim_e, f"{size} outliers={outliers} B={B}")
            lf = m(dx)["last_feat"]
            assert lf.shape == (B, bn.cfg["projection_dim"], 1) and torch.equal(lf, emb.unsqueeze(-1))
    # the clip_image wrapper: [B, hidden, T]
    from ldmseg_amd.models import CLIPVisionDescriptor
    plain = CLIPVisionDescriptor({k: v for k, v in bn.sd.items() if not k.startswith("visual_projection")}, device=DEV,
                                 compute_dtype="fp32")
    lf = plain(dx)["last_feat"]
    assert lf.shape == (3, bn.cfg["hidden"], T)
    assert rel_err(lf, R.last_feat(ref, False)) <= 1e-3
    assert bn.model("fp32").num_parameters == plain.num_parameters + bn.cfg["projection_dim"] * bn.cfg["hidden"]
    if size == "full":
        assert plain.num_parameters == 303_179_776


@pytest.mark.parametrize("mode", MODES)
def test_every_gemm_of_a_forward_was_compared(L, mode):
    """the dispatch log of one full-size forward at B = 1 and at B = 8: every GEMM-family kernel in it is one the per-op cases
    above ran (and compared) - the project's coverage rule applied to this executor"""
    for B in (1, 8):
        if (mode, B) not in GEMM_DONE:          # (run on its own: the per-op comparisons first)
            run_encoder_gemms(L, mode, B)
    m = bench("full", False).model(mode)
    seen = set()
    for B in (1, 8):
        x = bench("full", False).pixels(B).to(DEV)
        L.igemm_log(True)
        try:
            m.encode(x)
            torch.cuda.synchronize()
            seen |= L.igemm_log_read()
        finally:
            L.igemm_log(False)
    print(mode, sorted(seen))
    assert seen and seen <= GEMM_NAMES[mode], (sorted(seen - GEMM_NAMES[mode]), sorted(GEMM_NAMES[mode]))


@pytest.mark.parametrize("H,W", [(512, 512), (480, 640)])
def test_describe_from_raw_images(H, W):
    """describe(rgb): the fused front end against the reference fed with the CPU's F.interpolate + normalise"""
    bn = bench("full", False)
    B = 2
    rgb = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H))
    x = R.norm_resize(rgb, 224)
    ref, sim_h, sim_e = bn.ref(("rgb", H, W), x)
    from ldmseg_amd.models import CLIPVisionDescriptor
    for mode in MODES:
        ctx = bn.model(mode).describe(rgb.to(DEV))
        assert ctx.shape == (B, 1, 768)
        e = rel_err(ctx[:, 0], ref["image_embeds"])
        print("describe", (H, W), mode, "image_embeds", e, "simulated", sim_e)
        assert e <= (2 * sim_e if mode == "bf16" else 1e-3)
    plain_sd = {k: v for k, v in bn.sd.items() if not k.startswith("visual_projection")}
    for mode in MODES:
        m = CLIPVisionDescriptor(plain_sd, device=DEV, compute_dtype=mode)
        ctx = m.describe(rgb.to(DEV))
        assert ctx.shape == (B, 257, 1024)
        e = rel_err(ctx, ref["last_hidden_state"])
        print("describe", (H, W), mode, "last_hidden_state", e, "simulated", sim_h)
        assert e <= (2 * sim_h if mode == "bf16" else 1e-3)
        del m


def test_determinism_equivariance_and_handle_reuse():
    bn = bench("small", False)
    from ldmseg_amd.models import CLIPVisionDescriptor
    for mode in MODES:
        m = bn.model(mode)
        x8 = bn.pixels(8, seed=1).to(DEV)
        a = m.encode(x8)
        b = m.encode(x8)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                      # determinism
        perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], device=DEV)
        c = m.encode(x8[perm].contiguous())
        assert torch.equal(c[0], a[0][perm]) and torch.equal(c[1], a[1][perm])          # batch-permutation equivariance
        # one handle across B = 1 -> 8 -> 2 equals fresh handles
        outs = [m.encode(x8[:n].contiguous()) for n in (1, 8, 2)]
        for n, o in zip((1, 8, 2), outs):
            fresh = CLIPVisionDescriptor(bn.sd, projection=True, device=DEV, compute_dtype=mode)
            f = fresh.encode(x8[:n].contiguous())
            assert torch.equal(o[0], f[0]) and torch.equal(o[1], f[1]), (mode, n)
        rgb = torch.rand(2, 3, 64, 80, generator=torch.Generator().manual_seed(2)).to(DEV)
        assert torch.equal(m.describe(rgb), m.describe(rgb))


def plain_sd_of(sd):
    return {k: v for k, v in sd.items() if not k.startswith("visual_projection")}


def test_bad_inputs_raise(L):
    from ldmseg_amd import _lib
    from ldmseg_amd.models import CLIPVisionDescriptor
    bn = bench("small", False)
    m = bn.model("fp32")
    with pytest.raises(RuntimeError):
        m.encode(torch.zeros(1, 3, 42, 42))                                             # CPU tensor
    with pytest.raises(ValueError):
        m.encode(torch.zeros(1, 3, 56, 56, device=DEV))
    with pytest.raises(ValueError):
        m.describe(torch.zeros(1, 4, 56, 56, device=DEV))
    with pytest.raises(RuntimeError):
        CLIPVisionDescriptor(bn.sd, device="cpu")
    with pytest.raises(KeyError):
        CLIPVisionDescriptor({k: v for k, v in bn.sd.items() if "fc2.bias" not in k}, device=DEV)
    plain_sd = {k: v for k, v in bn.sd.items() if not k.startswith("visual_projection")}
    with pytest.raises(KeyError):
        CLIPVisionDescriptor(plain_sd, projection=True, device=DEV)
    # configurations the kernels do not serve: LDMSEG_E_SHAPE, never a fallback
    for bad in (dict(heads=4), dict(heads=1)):                                          # head dim 32 / 128
        with pytest.raises(RuntimeError, match="code -2"):
            CLIPVisionDescriptor(bn.sd, device=DEV, config=dict(R.SMALL, **bad))
    for bad in (dict(intermediate=520),                                                 # MLP size no multiple of 64
                dict(hidden=1344, heads=21)):                                           # wider than the statistics kernel serves
        with pytest.raises(RuntimeError, match="code -2"):
            CLIPVisionDescriptor(bn.sd, device=DEV, config=dict(R.SMALL, **bad))
    # (the Python schema refuses these two before the library sees them: through the C ABI)
    n, names, ptrs, numels, keep = _lib.weight_arrays(plain_sd_of(bn.sd), torch.device(DEV))
    for fields in ((128, 512, 2, 2, 45, 14, 0),                                         # image no multiple of the patch
                   (96, 512, 2, 2, 42, 14, 0),                                          # hidden no multiple of 64
                   (128, 512, 2, 2, 42, 14, 0)):                                        # (the last one is valid: the loop's control)
        cfg = _lib.ClipVisionCfg(*fields, _lib.F32, 0)
        h = C.c_void_p()
        rc = L.lib().ldmseg_clip_vision_create(C.byref(cfg), n, names, ptrs, numels, C.byref(h))
        if fields[0] == 128 and fields[4] == 42:
            assert rc == 0, L.lib().ldmseg_last_error()
            L.lib().ldmseg_clip_vision_destroy(h)
        else:
            assert rc == -2 and not h.value, (fields, rc)
    del keep
    # a mis-sized tensor: LDMSEG_E_WEIGHT
    wrong = dict(bn.sd)
    wrong["pre_layrnorm.weight"] = torch.ones(64)
    with pytest.raises(RuntimeError, match="code -4"):
        CLIPVisionDescriptor(wrong, device=DEV, config=dict(R.SMALL))
    # image_embeds from a handle without projection: LDMSEG_E_ARG
    plain = CLIPVisionDescriptor(plain_sd, device=DEV, compute_dtype="fp32")
    x = torch.zeros(1, 3, 42, 42, device=DEV)
    emb = torch.empty(1, 96, device=DEV)
    assert L.lib().ldmseg_clip_vision_forward(plain._h, P(x), 1, None, P(emb), _lib.stream_ptr(x.device)) == -1
    assert L.lib().ldmseg_clip_vision_forward(plain._h, P(x), 0, None, None, _lib.stream_ptr(x.device)) == -2


# ------------------------------------------------------------------ end to end
class HelperDescriptor(torch.nn.Module):
    """the reference forward on the CPU behind the reference wrappers' interface (a plain torch module in the descriptor slot)"""

    def __init__(self, sd, heads, projection):
        super().__init__()
        self.sd, self.heads, self.projection = sd, heads, projection

    def forward(self, x):
        torch.set_num_threads(16)
        out = R.forward(self.sd, x.detach().cpu().float(), self.heads)
        return {"last_feat": R.last_feat(out, self.projection).to(x.device)}


class ClipHelperDescriptor(HelperDescriptor):       # (a class name with "clip" in it: norm_resize_images dispatches on that)
    pass


@pytest.mark.parametrize("projection", [False, True])
def test_conditioned_sampling_end_to_end(sched_kw, projection):
    """TrainerDiffusion with the library's descriptor on a cross-attention UNet (encoder_hid_proj for the 1024-wide patch
    features, none for the 768-wide projected embedding), L = 16, 4 steps: native guided loop == python loop bitwise, and both
    equal the run whose context the reference computes on the CPU behind a plain torch module (fp32 UNet + descriptor, 1e-3)."""
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet, CLIPVisionDescriptor
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    bn = bench("full", False)
    usd = weights.generate(weights.unet_schema(8, True), seed=11)
    if not projection:
        usd.update(weights.generate(weights.hid_proj_schema(), seed=12))
    unet = UNet(usd, in_channels=8, device=DEV, compute_dtype="fp32", cross_attention=True)
    sd = bn.sd if projection else {k: v for k, v in bn.sd.items() if not k.startswith("visual_projection")}
    desc = CLIPVisionDescriptor(sd, projection=projection, device=DEV, compute_dtype="fp32")

    def sched():
        s = DDIMNoiseScheduler(**sched_kw)
        s.set_timesteps_inference(4)
        return s
    g = torch.Generator().manual_seed(6)
    rgb = (0.18215 * torch.randn(2, 4, 16, 16, generator=g)).to(DEV)
    noise = torch.randn(2, 4, 16, 16, generator=g)
    images = torch.rand(2, 3, 128, 160, generator=g).to(DEV)
    tr = TrainerDiffusion(None, unet, None, image_descriptor_model=desc)
    ehs, mult = tr.encoder_hidden_states(["", ""], images)
    assert mult == 2 and ehs.shape == ((4, 1, 768) if projection else (4, 257, 1024))
    a = tr.sample(["", ""], 4, 7.5, rgb_latents=rgb, rgb_images=images, scheduler=sched(), latents=noise)
    b = tr.sample(["", ""], 4, 7.5, rgb_latents=rgb, rgb_images=images, scheduler=sched(), latents=noise, python_loop=True)
    assert torch.equal(a, b)
    # the module-call surface takes the path any torch module takes and gives the same context up to the front end's rounding
    tr2 = TrainerDiffusion(None, unet, None, image_descriptor_model=ClipHelperDescriptor(bn.sd, 16, projection))
    ehs2, _ = tr2.encoder_hidden_states(["", ""], images)
    assert ehs2.shape == ehs.shape and rel_err(ehs, ehs2) <= 1e-3
    c = tr2.sample(["", ""], 4, 7.5, rgb_latents=rgb, rgb_images=images, scheduler=sched(), latents=noise)
    e = rel_err(a, c)
    print("end to end, projection =", projection, "context", rel_err(ehs, ehs2), "latents", e)
    assert e <= 1e-3


@pytest.mark.parametrize("mode", ["clip_image", "clip_image_proj"])
def test_main_ldm_eval_with_image_descriptors(tmp_path, mode):
    """tools/main_ldm_eval.py --image-descriptors on its default path (generated weights: the 8-channel cross-attention UNet, with
    encoder_hid_proj for clip_image, and the full-size CLIP vision encoder), two small images with ground-truth PNGs: exit code,
    PQ table, prediction PNGs at each image's own size."""
    import subprocess
    import numpy as np
    from PIL import Image
    from ldmseg_amd.evaluations import id2rgb
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    img_dir, gt_dir, out_dir = tmp_path / "rgb", tmp_path / "pan", tmp_path / "out"
    img_dir.mkdir()
    gt_dir.mkdir()
    for i, (h, w) in enumerate([(120, 160), (144, 100)]):
        a = (torch.rand(h // 8, w // 8, 3, generator=torch.Generator().manual_seed(40 + i)).numpy() * 255).astype(np.uint8)
        Image.fromarray(a).resize((w, h), Image.BILINEAR).save(img_dir / f"{i:03d}.jpg")
        gt = np.zeros((h, w), np.int64)
        gt[:h // 2] = 7 + i
        gt[h // 2:, :w // 2] = 3000
        Image.fromarray(id2rgb(gt)).save(gt_dir / f"{i:03d}.png")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "latent-diffusion-segmentation_amd")]))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "main_ldm_eval.py"), "--images", str(img_dir), "--panoptic", str(gt_dir),
                        "--size", "128", "--steps", "2", "--batch", "2", "--dtype", "bf16", "--count-th", "32", "--mask-th", "0.02",
                        "--out", str(out_dir), "--image-descriptors", mode], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "PQ" in r.stdout and "num_predictions" in r.stdout
    assert sorted(os.listdir(out_dir)) == ["000.png", "001.png", "predictions.json"]
    assert np.asarray(Image.open(out_dir / "001.png")).shape[:2] == (144, 100)

"""GPU suite: cross-attention conditioning and classifier-free guidance (image_descriptors none / clip_image /
clip_image_proj of the reference) - the cross-attention operator against fp64, the GEMMs attn2 adds against F.linear, whole
forwards against the oracle (oracle/unet.py restates attn2 with a context), the guided sampling loop against the Python loop
(bit for bit) and a reference-order oracle loop, and the rejections."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import ddim as o_ddim, unet as o_unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, X3 = 0, 1, 2


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ operator
def cross_ref(q, kv, B, N, S, Cc):
    d = Cc // 8
    qh = q.double().view(B, N, 8, d).transpose(1, 2)
    k = kv[..., :Cc].double().view(B, S, 8, d).transpose(1, 2)
    v = kv[..., Cc:].double().view(B, S, 8, d).transpose(1, 2)
    o = torch.softmax((qh @ k.transpose(-1, -2)) * d ** -0.5, -1) @ v
    return o.transpose(1, 2).reshape(B, N, Cc)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [64, 1024, 4096])
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("S", [1, 7, 77, 257, 1000])
def test_attention_cross_op(B, N, d, S):
    Cc = 8 * d
    g = torch.Generator().manual_seed(B * 100003 + N * 31 + d * 7 + S)
    q = (2.0 * torch.randn(B, N, Cc, generator=g)).to(DEV)          # sharper softmax
    kv = torch.randn(B, S, 2 * Cc, generator=g).to(DEV)
    kv[:, S // 2, :40] += 4.0                                       # one dominant key (running-max rescale across tiles)
    for dt, tol in ((F32, 2e-5), (BF16, 2e-2), (X3, 1e-4)):
        qs, kvs = (bf16_round(q), bf16_round(kv)) if dt == BF16 else (q, kv)
        ref = cross_ref(qs, kvs, B, N, S, Cc)
        out = torch.empty(B, N, Cc, device=DEV)
        assert lib().ldmseg_op_attention_cross(P(q), P(kv), B, N, S, Cc, 8, dt, P(out), None) == 0
        torch.cuda.synchronize()
        assert rel_err(out, ref) < tol, (dt, rel_err(out, ref))
        if S == 1:                                                  # one key: every query row gets that key's value
            v = kvs[:, :, Cc:].expand(B, N, Cc)
            assert torch.equal(out, v), dt


def test_attention_cross_op_rejects_unsupported_head_dim():
    q = torch.zeros(1, 64, 8 * 48, device=DEV)
    kv = torch.zeros(1, 7, 2 * 8 * 48, device=DEV)
    out = torch.empty_like(q)
    assert lib().ldmseg_op_attention_cross(P(q), P(kv), 1, 64, 7, 8 * 48, 8, F32, P(out), None) == -2


# ------------------------------------------------------------------ the GEMMs attn2 adds (B = 16, L = 64)
GEMM_MODES = ((0, 2e-5), (1, 2e-2), (3, 1e-4))      # fp32, bf16, split-bf16 with the weights as hi | lo planes (bf16x3 handles)


def _linear_op(x, w, b, dt):
    """F.linear(x, w, b) as the engine launches it (a 1x1 conv over M token rows)."""
    M, K = x.shape
    N = w.shape[0]
    xs = x.t().contiguous().view(1, K, M, 1)
    out = torch.empty(1, N, M, 1, device=DEV)
    assert lib().ldmseg_op_conv2d(P(xs), None, P(w.contiguous()), P(b), 1, K, 0, M, 1, N, 1, 1, 0, dt, P(out), None) == 0
    torch.cuda.synchronize()
    return out.view(N, M).t()


@pytest.mark.parametrize("Cc,tokens", [(320, 4096), (640, 1024), (1280, 256), (1280, 64)])
def test_to_q_with_folded_norm2(Cc, tokens):
    M = 16 * tokens
    g = torch.Generator().manual_seed(Cc + tokens)
    x = (torch.randn(M, Cc, generator=g) * 1.5 + 0.3).to(DEV)
    gam = (1 + 0.1 * torch.randn(Cc, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(Cc, generator=g)).to(DEV)
    w = (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).to(DEV)
    for dt, tol in GEMM_MODES:
        xs, ws = (bf16_round(x), bf16_round(w)) if dt == 1 else (x, w)
        ref = F.linear(F.layer_norm(xs.double(), (Cc,), gam.double(), bet.double(), 1e-5), ws.double())
        out = torch.empty(M, Cc, device=DEV)
        assert lib().ldmseg_op_ln_linear(P(x), P(gam), P(bet), P(w), None, M, Cc, Cc, 1e-5, 0, dt, P(out), None) == 0
        torch.cuda.synchronize()
        assert rel_err(out, ref) < tol, (dt, rel_err(out, ref))


@pytest.mark.parametrize("S", [77, 257])
@pytest.mark.parametrize("Cc", [320, 640, 1280])
def test_context_kv_gemm(S, Cc):
    M = 16 * S
    g = torch.Generator().manual_seed(S * 3 + Cc)
    ctx = torch.randn(M, 768, generator=g).to(DEV)
    w = (torch.randn(2 * Cc, 768, generator=g) / 768 ** 0.5).to(DEV)            # to_k | to_v, no bias
    zero = torch.zeros(2 * Cc, device=DEV)
    for dt, tol in GEMM_MODES:
        xs, ws = (bf16_round(ctx), bf16_round(w)) if dt == 1 else (ctx, w)
        ref = F.linear(xs.double(), ws.double())
        assert rel_err(_linear_op(ctx, w, zero, dt), ref) < tol, dt


@pytest.mark.parametrize("S", [77, 257])
def test_encoder_hid_proj_gemm(S):
    M = 16 * S
    g = torch.Generator().manual_seed(S)
    x = torch.randn(M, 1024, generator=g).to(DEV)
    w = (torch.randn(768, 1024, generator=g) / 32.0).to(DEV)
    b = (0.05 * torch.randn(768, generator=g)).to(DEV)
    for dt, tol in GEMM_MODES:
        xs, ws = (bf16_round(x), bf16_round(w)) if dt == 1 else (x, w)
        ref = F.linear(xs.double(), ws.double(), b.double())
        assert rel_err(_linear_op(x, w, b, dt), ref) < tol, dt


# ------------------------------------------------------------------ whole forward
@pytest.fixture(scope="module")
def cross_sd():
    from ldmseg_amd import weights
    sd = weights.generate(weights.unet_schema(8, True), seed=11)
    sd.update(weights.generate(weights.hid_proj_schema(), seed=12))
    return sd


@pytest.fixture(scope="module")
def cross_unets(cross_sd):
    from ldmseg_amd.models import UNet
    plain = {k: v for k, v in cross_sd.items() if not k.startswith("encoder_hid_proj.")}
    out = {m: UNet(plain, in_channels=8, device=DEV, compute_dtype=m, cross_attention=True) for m in ("fp32", "bf16", "bf16x3")}
    out["proj_fp32"] = UNet(cross_sd, in_channels=8, device=DEV, compute_dtype="fp32", cross_attention=True)
    out["proj_bf16"] = UNet(cross_sd, in_channels=8, device=DEV, compute_dtype="bf16", cross_attention=True)
    return out


def test_cross_unet_structure(cross_unets):
    assert cross_unets["fp32"].num_parameters == 859_532_484
    assert cross_unets["proj_fp32"].num_parameters == 860_319_684
    assert cross_unets["fp32"].config.cross_attention_dim == 768
    assert cross_unets["fp32"].workspace_bytes(2, 16) > 0


@pytest.mark.parametrize("B,Ls,t", [(2, 16, 999), (2, 32, [19, 500]), (1, 64, 259)])
def test_cross_forward_vs_oracle(cross_unets, cross_sd, B, Ls, t):
    g = torch.Generator().manual_seed(Ls * 5 + B)
    x = torch.randn(B, 8, Ls, Ls, generator=g)
    ctx = torch.randn(B, 77, 768, generator=g)
    tt = torch.tensor(t)
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = o_unet.unet_forward(cross_sd, x, tt, encoder_hidden_states=ctx)
    tdev = tt.to(DEV) if tt.dim() else tt
    for m, tol in (("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16", 6e-2)):
        out = cross_unets[m](x.to(DEV), tdev, encoder_hidden_states=ctx.to(DEV)).sample
        assert rel_err(out, ref) < tol, (m, rel_err(out, ref))


@pytest.mark.parametrize("B,Ls,S", [(2, 16, 257), (2, 32, 1)])
def test_cross_forward_with_encoder_hid_proj_vs_oracle(cross_unets, cross_sd, B, Ls, S):
    """clip_image: [B, 257, 1024] patch features through encoder_hid_proj (applied by the test before the oracle);
    clip_image_proj-like: one 768-wide token ([B, 1, 768]) on the same handle."""
    g = torch.Generator().manual_seed(Ls + S)
    x = torch.randn(B, 8, Ls, Ls, generator=g)
    wide = S > 1
    ctx = torch.randn(B, S, 1024 if wide else 768, generator=g)
    ctx_o = F.linear(ctx, cross_sd["encoder_hid_proj.weight"], cross_sd["encoder_hid_proj.bias"]) if wide else ctx
    tt = torch.tensor(333)
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = o_unet.unet_forward(cross_sd, x, tt, encoder_hidden_states=ctx_o)
    for m, tol in (("proj_fp32", 1e-3), ("proj_bf16", 6e-2)):
        out = cross_unets[m](x.to(DEV), tt, encoder_hidden_states=ctx.to(DEV)).sample
        assert rel_err(out, ref) < tol, (m, rel_err(out, ref))


def test_zero_attn2_out_equals_plain_unet(cross_sd):
    """Known answer: with attn2.to_out.0 zeroed, the cross-attention block adds exactly nothing."""
    from ldmseg_amd.models import UNet
    sd = {k: v for k, v in cross_sd.items() if not k.startswith("encoder_hid_proj.")}
    for k in list(sd):
        if ".attn2.to_out.0." in k:
            sd[k] = torch.zeros_like(sd[k])
    cross = UNet(sd, in_channels=8, device=DEV, compute_dtype="fp32", cross_attention=True)
    plain_sd = {k: v for k, v in sd.items() if ".attn2." not in k and ".norm2." not in k or ".resnets." in k}
    plain = UNet(plain_sd, in_channels=8, device=DEV, compute_dtype="fp32")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 16, 16, generator=g).to(DEV)
    ctx = torch.randn(2, 77, 768, generator=g).to(DEV)
    a = cross(x, 500, encoder_hidden_states=ctx).sample
    b = plain(x, 500).sample
    assert rel_err(a, b) < 1e-6
    # rejections of the context argument
    with pytest.raises(NotImplementedError):
        plain(x, 500, encoder_hidden_states=ctx)
    out = torch.empty(2, 4, 16, 16, device=DEV)
    from ldmseg_amd import _lib
    assert lib().ldmseg_unet_forward_ctx(plain._h, P(x), None, 1, 500, 2, 16, P(ctx), 77, 768, P(out),
                                         _lib.stream_ptr(x.device)) == -1
    with pytest.raises(RuntimeError, match="code -1"):
        cross(x, 500)                                                   # a cross handle needs its context
    with pytest.raises(RuntimeError, match="code -1"):
        cross.forward_parts(x[:, :4].contiguous(), x[:, 4:].contiguous(), None, 500)
    with pytest.raises(RuntimeError, match="code -1"):
        cross(x, 500, encoder_hidden_states=torch.zeros(2, 77, 1024, device=DEV))   # no encoder_hid_proj on this handle
    with pytest.raises(RuntimeError, match="code -1"):
        cross(x, 500, encoder_hidden_states=torch.zeros(2, 77, 512, device=DEV))


# ------------------------------------------------------------------ guided sampling
@pytest.fixture(scope="module")
def sched_factory(sched_kw):
    from ldmseg_amd.schedulers import DDIMNoiseScheduler

    def make(n=4):
        s = DDIMNoiseScheduler(**sched_kw)
        s.set_timesteps_inference(n)
        return s
    return make


def _trainer(unet, **kw):
    from ldmseg_amd.trainers import TrainerDiffusion
    return TrainerDiffusion(None, unet, None, **kw)


def _inputs(B=2, L=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = (0.18215 * torch.randn(B, 4, L, L, generator=g)).to(DEV)
    noise = torch.randn(B, 4, L, L, generator=g)
    return rgb, noise


@pytest.mark.parametrize("mode,mult,gs", [("bf16", 1, 1.0), ("bf16", 1, 7.5), ("bf16", 2, 1.0), ("bf16", 2, 7.5), ("fp32", 2, 7.5)])
def test_guided_loop_native_equals_python(cross_unets, sched_factory, mode, mult, gs):
    tr = _trainer(cross_unets[mode])
    rgb, noise = _inputs()
    g = torch.Generator().manual_seed(17)
    ctx = torch.randn(mult * 2, 77, 768, generator=g).to(DEV)
    lat = noise.to(DEV)
    for ret_all in (False, True):
        a = tr._sample_native_guided(sched_factory(), lat.clone(), rgb, ctx, mult, gs, ret_all)
        b = tr._sample_python_guided(sched_factory(), lat.clone(), rgb, ctx, mult, gs, ret_all)
        torch.cuda.synchronize()
        assert a.shape == b.shape == ((8 if ret_all else 2), 4, 16, 16)
        assert torch.equal(a, b), (mode, mult, gs, ret_all, rel_err(a, b))


def reference_loop(sd, sched_kw, latents, rgb, ehs, multiplier, guidance_scale, n=4):
    """trainers_ldm_cond.py:1121-1160 transcribed on the oracle UNet and scheduler (CPU fp32)."""
    so = o_ddim.OracleDDIM(**sched_kw)
    so.set_timesteps_inference(n)
    latents = latents * so.init_noise_sigma
    rgb_latents = torch.cat([rgb] * multiplier)
    for idx, t in enumerate(so.timesteps):
        latent_model_input = torch.cat([latents] * multiplier)
        inputs = torch.cat([latent_model_input, rgb_latents], dim=1)
        noise_pred = o_unet.unet_forward(sd, inputs, t, encoder_hidden_states=ehs)
        if multiplier > 1:
            noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
            noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
        prev, x0 = so.step(noise_pred, t, latents)
        latents = x0 if idx == len(so.timesteps) - 1 else prev
    return latents


def test_guided_loop_vs_reference_order_oracle(cross_unets, cross_sd, sched_factory, sched_kw):
    tr = _trainer(cross_unets["fp32"])
    rgb, noise = _inputs(seed=4)
    g = torch.Generator().manual_seed(23)
    ctx = torch.randn(4, 77, 768, generator=g)
    out = tr._sample_native_guided(sched_factory(), noise.to(DEV), rgb, ctx.to(DEV), 2, 7.5, False)
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = reference_loop(cross_sd, sched_kw, noise, rgb.cpu(), ctx, 2, 7.5)
    assert rel_err(out, ref) < 2e-3


class ClipVisionStandIn(torch.nn.Module):
    """Stands in for MyCLIPVisionModel (descriptors.py:25-40): images [B,3,224,224] -> {'last_feat': [B, 1024, 9]}."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.w = torch.nn.Parameter(torch.randn(1024, 3, generator=g), requires_grad=False)
        self.seen = None

    def forward(self, x):
        self.seen = x
        f = F.adaptive_avg_pool2d(x, 3).flatten(2)                      # [B, 3, 9]
        return {"last_feat": torch.einsum("dc,bcs->bds", self.w, f)}


class TokenizerStandIn:
    model_max_length = 77

    def __call__(self, prompts, padding="max_length", max_length=77, truncation=False, return_tensors="pt"):
        ids = torch.zeros(len(prompts), max_length, dtype=torch.int64)
        for i, p in enumerate(prompts):
            toks = [49406] + [ord(c) % 1000 for c in p][:max_length - 2] + [49407]
            ids[i, :len(toks)] = torch.tensor(toks) % 1000
        return type("Tok", (), {"input_ids": ids})()


class TextEncoderStandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(1000, 768)
        with torch.no_grad():
            self.emb.weight.copy_(torch.randn(1000, 768, generator=torch.Generator().manual_seed(2)))

    def forward(self, ids):
        return (self.emb(ids),)


def test_trainer_sample_with_descriptor_model(cross_unets, sched_factory):
    desc = ClipVisionStandIn().to(DEV)
    tr = _trainer(cross_unets["proj_bf16"], image_descriptor_model=desc)
    rgb, noise = _inputs(seed=6)
    images = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(8)).to(DEV)
    ehs, mult = tr.encoder_hidden_states(["", ""], images)
    # what the reference builds (:1100-1107, :663-675)
    x = F.interpolate(images, size=(224, 224), mode="bilinear", align_corners=False)
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073], device=DEV).view(1, 3, 1, 1)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711], device=DEV).view(1, 3, 1, 1)
    x = (x - mean) / std
    assert torch.equal(desc.seen, x)
    d = desc(x)["last_feat"]
    d = d.view(d.shape[0], d.shape[1], -1).permute(0, 2, 1)
    assert mult == 2 and torch.equal(ehs, torch.cat([d] * 2).float()) and ehs.shape == (4, 9, 1024)
    a = tr.sample(["", ""], 4, 7.5, rgb_latents=rgb, rgb_images=images, scheduler=sched_factory(), latents=noise)
    b = tr.sample(["", ""], 4, 7.5, rgb_latents=rgb, rgb_images=images, scheduler=sched_factory(), latents=noise,
                  python_loop=True)
    c = tr._sample_native_guided(sched_factory(), noise.to(DEV), rgb, ehs, 2, 7.5, False)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_trainer_sample_with_text_encoder(cross_unets, cross_sd, sched_factory, sched_kw):
    tok, te = TokenizerStandIn(), TextEncoderStandIn().to(DEV)
    tr = _trainer(cross_unets["fp32"], textencoder=te, tokenizer=tok)
    rgb, noise = _inputs(seed=9)
    prompts = ["a photo of a cat", "two dogs"]
    ehs, mult = tr.encoder_hidden_states(prompts)
    text = te(tok(prompts, max_length=77).input_ids.to(DEV))[0]
    unc = te(tok(["", ""], max_length=77).input_ids.to(DEV))[0]
    assert mult == 2 and torch.equal(ehs, torch.cat([unc, text])) and ehs.shape == (4, 77, 768)
    a = tr.sample(prompts, 4, 7.5, rgb_latents=rgb, scheduler=sched_factory(), latents=noise)
    b = tr.sample(prompts, 4, 7.5, rgb_latents=rgb, scheduler=sched_factory(), latents=noise, python_loop=True)
    assert torch.equal(a, b)
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = reference_loop(cross_sd, sched_kw, noise, rgb.cpu(), ehs.cpu(), 2, 7.5)
    assert rel_err(a, ref) < 2e-3


def test_guided_loop_rejections(cross_unets, sched_factory):
    from ldmseg_amd import _lib
    u = cross_unets["bf16"]
    tr = _trainer(u)
    rgb, noise = _inputs()
    ctx = torch.zeros(4, 77, 768, device=DEV)
    cfg, keep = tr._loop_cfg(sched_factory())
    lat = noise.to(DEV).contiguous()
    st = _lib.stream_ptr(lat.device)
    cfg.self_condition = 1                                            # self-conditioning with guidance (reference defect)
    assert lib().ldmseg_sample_loop_guided(u._h, C.byref(cfg), P(lat), P(rgb), 2, 16, P(ctx), 77, 768, 2, 7.5, None, st) == -1
    assert b"self_condition" in lib().ldmseg_last_error()
    cfg.self_condition = 0
    assert lib().ldmseg_sample_loop_guided(u._h, C.byref(cfg), P(lat), P(rgb), 2, 16, None, 77, 768, 2, 7.5, None, st) == -1
    assert lib().ldmseg_sample_loop_guided(u._h, C.byref(cfg), P(lat), P(rgb), 2, 16, P(ctx), 77, 1024, 2, 7.5, None, st) == -1
    assert lib().ldmseg_sample_loop_guided(u._h, C.byref(cfg), P(lat), P(rgb), 2, 16, P(ctx), 77, 768, 3, 7.5, None, st) == -1
    assert lib().ldmseg_sample_loop(u._h, C.byref(cfg), P(lat), P(rgb), 2, 16, None, st) == -1     # plain loop: cross handle
    del keep
    tr12 = _trainer(u, self_condition=True, textencoder=TextEncoderStandIn().to(DEV), tokenizer=TokenizerStandIn())
    with pytest.raises(ValueError):
        tr12.sample(["", ""], 4, rgb_latents=rgb, scheduler=sched_factory(), latents=noise)

"""GPU suite: the UNet's separate image encoder (modify_encoder(separate_encoder=True[, add_adaptor=True]),
ldmseg/models/unet.py:42-63, 301-385) - the skip-add operator, the adaptor convs at the shapes the plain UNet never
launches, whole forwards against the restatement in tests/unet_sepenc_ref.py, the known answer against a plain 8-channel
handle, the sampling loop (native = Python bit for bit, once-per-call = every-step bit for bit, nothing kept across calls or
shapes, and against the reference-order oracle loop) and the refusals.

Measured on an MI355X (max-norm relative error of the whole forwards against the CPU restatement, worst of the four cases):
see DESIGN.md section 3.12."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import unet_sepenc_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                                             # guard elements behind every segment of ldmseg_op_skip_add
GEMM_MODES = ((0, 2e-5), (1, 2e-2), (3, 1e-4))        # as tests/test_cross_attention_gpu.py: fp32, bf16, bf16x3 (hi | lo planes)
FORWARD_TOL = (("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16", 6e-2))


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------ 1. the add
def forward_segments(B, L):
    """element counts of the 12 skip connections of one forward"""
    out = [B * L * L * 320]
    for i, c in enumerate((320, 640, 1280, 1280)):
        s = L >> i
        out += [B * s * s * c] * 2
        if i < 3:
            out.append(B * (s // 2) * (s // 2) * c)
    return out


SEGMENT_LISTS = [[8], [1280], [24, 1288, 8], [3 * 1280, 3 * 1280 * 4, 320 * 24 * 24], forward_segments(1, 8),
                 [5, 2 ** 20 + 3], [2 ** 20 + 3, 5], [1, 7, 9, 16, 4]]


@pytest.mark.parametrize("segs", SEGMENT_LISTS, ids=lambda s: "-".join(map(str, s[:4])) + ("+" if len(s) > 4 else ""))
@pytest.mark.parametrize("dt", [0, 1])
def test_skip_add_op(segs, dt):
    total = sum(segs) + GUARD * len(segs)
    g = torch.Generator().manual_seed(len(segs) * 1009 + segs[0])
    a = torch.randn(total, generator=g)
    b = 3.0 * torch.randn(total, generator=g)
    out0 = torch.full((total,), -768.0)                # (exact in bf16)
    a_d, b_d, out = a.to(DEV), b.to(DEV), out0.to(DEV)
    n = (C.c_int64 * len(segs))(*segs)
    assert lib().ldmseg_op_skip_add(P(a_d), P(b_d), n, len(segs), dt, P(out), None) == 0
    torch.cuda.synchronize()
    out = out.cpu()
    want = (a + b) if dt == 0 else (bf16_round(a) + bf16_round(b)).to(torch.bfloat16).to(torch.float32)
    off = 0
    for k, e in enumerate(segs):
        assert torch.equal(out[off:off + e], want[off:off + e]), (k, e)
        assert torch.equal(out[off + e:off + e + GUARD], out0[off + e:off + e + GUARD]), ("guard", k, e)
        off += e + GUARD


def test_skip_add_op_rejections():
    """(dst = a, the in-place form the engine uses for 11 of the 12 skips, runs in every forward of this file)"""
    x = torch.zeros(64, device=DEV)
    one = (C.c_int64 * 1)(8)
    assert lib().ldmseg_op_skip_add(P(x), P(x), one, 0, 0, P(x), None) == -2
    assert lib().ldmseg_op_skip_add(P(x), P(x), one, 1, 2, P(x), None) == -2
    many = (C.c_int64 * 13)(*([1] * 13))
    assert lib().ldmseg_op_skip_add(P(x), P(x), many, 13, 0, P(x), None) == -2
    assert lib().ldmseg_op_skip_add(None, P(x), one, 1, 0, P(x), None) == -2


# ------------------------------------------------------------------ 2. adaptor convs
@pytest.mark.parametrize("L", [16, 64])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_adaptor_conv_shapes(L, level):
    """adaptor_layers[i] also runs on block i's downsampled output: 3x3 C -> C at (320, L/2), (640, L/4), (1280, L/8), maps
    on which the plain UNet has no C -> C conv of that width."""
    Cc, side, B = (320, 640, 1280)[level], L >> (level + 1), 2
    g = torch.Generator().manual_seed(L * 10 + level)
    x = torch.randn(B, Cc, side, side, generator=g)
    w = torch.randn(Cc, Cc, 3, 3, generator=g) * (3.0 / (9 * Cc)) ** 0.5
    b = 0.05 * torch.randn(Cc, generator=g)
    torch.set_num_threads(16)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), b.to(DEV)
    for dt, tol in GEMM_MODES:
        xs, ws = (bf16_round(x), bf16_round(w)) if dt == 1 else (x, w)
        want = F.conv2d(xs.double(), ws.double(), b.double(), padding=1)
        out = torch.empty(B, Cc, side, side, device=DEV)
        assert lib().ldmseg_op_conv2d(P(x_d), None, P(w_d), P(b_d), B, Cc, 0, side, side, Cc, 3, 1, 0, dt, P(out), None) == 0
        torch.cuda.synchronize()
        e = rel_err(out, want)
        print(f"adaptor conv C={Cc} side={side} dt={dt}: rel_err {e:.3e}")
        assert e < tol, (dt, e)


# ------------------------------------------------------------------ handles
@pytest.fixture(scope="module")
def sep_sd():
    """one generated state dict with adaptors; the adaptor-less one is the same dict without adaptor_layers.*"""
    from ldmseg_amd import weights
    s = weights.unet_schema(4, False)
    s.update(weights.separate_encoder_schema(True))
    return weights.generate(s, seed=21)


def without_adaptors(sd):
    return {k: v for k, v in sd.items() if not k.startswith("adaptor_layers.")}


@pytest.fixture(scope="module")
def sep_unets(sep_sd):
    """(mode, adaptor) -> handle, built when first asked for"""
    from ldmseg_amd.models import UNet
    made = {}

    def get(mode, adaptor=True):
        if (mode, adaptor) not in made:
            sd = sep_sd if adaptor else without_adaptors(sep_sd)
            made[(mode, adaptor)] = UNet(sd, in_channels=8, device=DEV, compute_dtype=mode)
        return made[(mode, adaptor)]
    yield get
    made.clear()


# ------------------------------------------------------------------ 3. structure
def test_structure(sep_unets):
    u = sep_unets("bf16", False)
    assert u.separate_encoder and u.in_channels == 8 and not u.cross_attention
    assert u.num_parameters == 1_049_661_444
    assert sep_unets("bf16", True).num_parameters == 1_083_764_164
    assert u.workspace_bytes(2, 16) > 0
    from ldmseg_amd.trainers import TrainerDiffusion
    assert TrainerDiffusion(None, u, None).self_condition is False


# ------------------------------------------------------------------ 4. whole forwards
@pytest.mark.parametrize("adaptor", [True, False], ids=["adaptor", "plain"])
@pytest.mark.parametrize("B,L,t,t_img", [(1, 8, 999, None), (2, 16, [19, 500], None), (3, 24, 500, [0, 7, 300]), (1, 32, 259, 40)])
def test_forward_vs_restatement(sep_unets, sep_sd, adaptor, B, L, t, t_img):
    g = torch.Generator().manual_seed(L * 7 + B)
    x = torch.randn(B, 8, L, L, generator=g)
    tt = torch.tensor(t)
    ti = None if t_img is None else torch.tensor(t_img)
    sd = sep_sd if adaptor else without_adaptors(sep_sd)
    torch.set_num_threads(16)
    with torch.no_grad():
        want = ref.sepenc_forward(sd, x, tt, ti)
    x_d = x.to(DEV)
    tdev = tt.to(DEV) if tt.dim() else tt
    tidev = ti if ti is None or ti.dim() == 0 else ti.to(DEV)
    errs = {}
    for m, tol in FORWARD_TOL:
        u = sep_unets(m, adaptor)
        out = u(x_d, tdev, timestep_img=tidev).sample
        errs[m] = rel_err(out, want)
        if ti is None:                                 # the un-concatenated entry means timestep_img = 0 too
            parts = u.forward_parts(x_d[:, :4].contiguous(), x_d[:, 4:].contiguous(), None, tdev).sample
            assert torch.equal(parts, out), m
    print(f"forward B={B} L={L} adaptor={adaptor}: " + ", ".join(f"{m} {e:.3e}" for m, e in errs.items()))
    for m, tol in FORWARD_TOL:
        assert errs[m] < tol, (m, errs[m])


def test_timestep_img_forms_agree(sep_unets):
    """int, 0-d tensor, [B] tensor on either device: one value, one result; None = 0; another value, another result."""
    u = sep_unets("bf16")
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 8, 16, 16, generator=g).to(DEV)
    base = u(x, 500, timestep_img=40).sample
    for form in (torch.tensor(40), torch.tensor(40, device=DEV), torch.tensor([40, 40]), torch.tensor([40, 40], device=DEV)):
        assert torch.equal(u(x, 500, timestep_img=form).sample, base)
    zero = u(x, 500).sample
    assert torch.equal(u(x, 500, timestep_img=0).sample, zero)
    assert rel_err(base, zero) > 1e-2                  # (timestep_img reaches the output)
    swapped = u(torch.cat([x[:, :4], x[:, 4:].flip(0)], 1).contiguous(), 500).sample
    assert rel_err(swapped, zero) > 1e-1               # (and so does the image half)


# ------------------------------------------------------------------ 5. known answer
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_zeroed_branch_equals_plain_unet(sep_sd, mode):
    """conv_in_img.* and adaptor_layers.* zeroed: every residual is exactly zero, adding it changes no value, and the main
    path is the plain 8-channel handle's launches on a conv_in with zero filters over the image half."""
    from ldmseg_amd.models import UNet
    sd = {k: (torch.zeros_like(v) if k.startswith(("conv_in_img.", "adaptor_layers.")) else v) for k, v in sep_sd.items()}
    sep = UNet(sd, in_channels=8, device=DEV, compute_dtype=mode)
    plain = UNet(ref.plain_equivalent(sd), in_channels=8, device=DEV, compute_dtype=mode)
    assert not plain.separate_encoder
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 16, 16, generator=g).to(DEV)
    t = torch.tensor([19, 500], device=DEV)
    a = sep(x, t, timestep_img=300).sample
    b = plain(x, t, timestep_img=300).sample           # (ignored there, as the reference ignores it)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. / 7. the loop
@pytest.fixture(scope="module")
def sched_factory(sched_kw):
    from ldmseg_amd.schedulers import DDIMNoiseScheduler

    def make(n=4):
        s = DDIMNoiseScheduler(**sched_kw)
        s.set_timesteps_inference(n)
        return s
    return make


def _trainer(unet):
    from ldmseg_amd.trainers import TrainerDiffusion
    return TrainerDiffusion(None, unet, None)


def _inputs(B=2, L=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = (0.18215 * torch.randn(B, 4, L, L, generator=g)).to(DEV)
    noise = torch.randn(B, 4, L, L, generator=g)
    return rgb, noise


class every_step:
    """debug key 25 = 1 inside the block (the loop computes the image branch in every step), restored after it"""

    def __enter__(self):
        self.old = lib().ldmseg_debug_get(25)
        assert lib().ldmseg_debug_set(25, 1) == 0

    def __exit__(self, *exc):
        lib().ldmseg_debug_set(25, self.old)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_loop_native_equals_python_and_every_step(sep_unets, sched_factory, mode):
    assert lib().ldmseg_debug_get(25) == 0             # the shipped default: once per call
    tr = _trainer(sep_unets(mode))
    rgb, noise = _inputs()
    prompts = [""] * 2
    for ret_all in (False, True):
        kw = dict(rgb_latents=rgb, latents=noise, return_all_latents=ret_all)
        a = tr.sample(prompts, scheduler=sched_factory(), **kw)
        b = tr.sample(prompts, scheduler=sched_factory(), python_loop=True, **kw)
        with every_step():
            c = tr.sample(prompts, scheduler=sched_factory(), **kw)
        torch.cuda.synchronize()
        assert a.shape == ((8 if ret_all else 2), 4, 16, 16)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (mode, ret_all, rel_err(a, b))
        assert torch.equal(a, c), (mode, ret_all, rel_err(a, c))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_inpaint_loop_every_step_equals_once(sep_unets, sched_factory, mode):
    tr = _trainer(sep_unets(mode))
    rgb, _ = _inputs(seed=6)
    g = torch.Generator().manual_seed(8)
    known = torch.rand(2, 1, 16, 16, generator=g) < 0.4
    z0 = torch.randn(2, 4, 16, 16, generator=g).to(DEV)
    kw = dict(known_mask=known, known_latents=z0, seed=31, rgb_latents=rgb)
    a = tr.sample_inpaint([""] * 2, scheduler=sched_factory(), **kw)
    with every_step():
        b = tr.sample_inpaint([""] * 2, scheduler=sched_factory(), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), (mode, rel_err(a, b))


def test_nothing_is_kept_across_calls_or_shapes(sep_unets, sep_sd, sched_factory):
    """A second call with other rgb_latents, and calls at (2,16) -> (1,8) -> (2,16) on one handle, equal what handles that
    never ran anything else give."""
    from ldmseg_amd.models import UNet
    used = _trainer(sep_unets("bf16"))
    rgb1, noise = _inputs(seed=3)
    rgb2, _ = _inputs(seed=4)
    rgb_s, noise_s = _inputs(B=1, L=8, seed=5)

    def run(tr, rgb, nz):
        return tr.sample([""] * rgb.shape[0], scheduler=sched_factory(), rgb_latents=rgb, latents=nz)
    fresh_a = run(_trainer(UNet(sep_sd, in_channels=8, device=DEV, compute_dtype="bf16")), rgb2, noise)
    fresh_b = run(_trainer(UNet(sep_sd, in_channels=8, device=DEV, compute_dtype="bf16")), rgb_s, noise_s)
    first = run(used, rgb1, noise)
    second = run(used, rgb2, noise)
    small = run(used, rgb_s, noise_s)
    again = run(used, rgb2, noise)
    torch.cuda.synchronize()
    assert rel_err(first, second) > 1e-2               # (the image half matters)
    assert torch.equal(second, fresh_a)
    assert torch.equal(small, fresh_b)
    assert torch.equal(again, fresh_a)


def test_loop_vs_reference_order_oracle(sep_unets, sep_sd, sched_factory, sched_kw):
    tr = _trainer(sep_unets("fp32"))
    rgb, noise = _inputs(seed=4)
    out = tr.sample([""] * 2, scheduler=sched_factory(), rgb_latents=rgb, latents=noise)
    torch.set_num_threads(16)
    with torch.no_grad():
        want = ref.reference_loop(sep_sd, sched_kw, noise, rgb.cpu())
    e = rel_err(out, want)
    print(f"four-step loop, fp32, B=2 L=16: rel_err {e:.3e}")
    assert e < 2e-3


# ------------------------------------------------------------------ 8. refusals
def _create_code(in_channels, cross_attention):
    """ldmseg_unet_create on a weight list that only names conv_in_img.weight: the configuration is judged first"""
    from ldmseg_amd import _lib
    w = torch.zeros(320 * 4 * 9, device=DEV)
    cfg = _lib.UNetCfg(in_channels, cross_attention, _lib.BF16, 0)
    names = (C.c_char_p * 1)(b"conv_in_img.weight")
    ptrs = (C.c_void_p * 1)(w.data_ptr())
    numels = (C.c_int64 * 1)(w.numel())
    h = C.c_void_p()
    code = lib().ldmseg_unet_create(C.byref(cfg), 1, names, ptrs, numels, C.byref(h))
    return code, lib().ldmseg_last_error().decode()


def test_refusals(sep_unets, sep_sd, sched_factory):
    from ldmseg_amd import _lib
    from ldmseg_amd.models import UNet
    # separate encoder with cross-attention / with another channel count
    code, msg = _create_code(8, 1)
    assert code == -1 and "cross_attention" in msg
    for ch in (4, 12):
        code, msg = _create_code(ch, 0)
        assert code == -1 and "in_channels 8" in msg
    small = {k: v for k, v in sep_sd.items() if k.startswith("conv_in")}
    with pytest.raises(NotImplementedError, match="cross_attention"):
        UNet(small, in_channels=8, device=DEV, cross_attention=True)
    with pytest.raises(ValueError, match="in_channels=8"):
        UNet(small, in_channels=12, device=DEV)
    # the guided loop
    u = sep_unets("bf16")
    tr = _trainer(u)
    rgb, noise = _inputs()
    ctx = torch.zeros(2, 77, 768, device=DEV)
    cfg, keep = tr._loop_cfg(sched_factory())
    lat = noise.to(DEV)
    code = lib().ldmseg_sample_loop_guided(u._h, C.byref(cfg), P(lat), P(rgb), 2, 16, P(ctx), 77, 768, 1, 1.0, None,
                                           _lib.stream_ptr(rgb.device))
    assert code == -1 and "separate-encoder" in lib().ldmseg_last_error().decode()
    with pytest.raises(RuntimeError, match="code -1"):
        tr._sample_native_guided(sched_factory(), lat.clone(), rgb, ctx, 1, 1.0, False)
    # timg_count
    x = torch.zeros(2, 8, 16, 16, device=DEV)
    out = torch.empty(2, 4, 16, 16, device=DEV)
    ti = torch.zeros(3, dtype=torch.int64, device=DEV)
    for count in (0, 3):
        code = lib().ldmseg_unet_forward_img(u._h, P(x), None, 1, 500, P(ti), count, 0, 2, 16, P(out), _lib.stream_ptr(x.device))
        assert code == -1 and "timg_count" in lib().ldmseg_last_error().decode()
    with pytest.raises(ValueError, match="one entry per sample"):
        u(x, 500, timestep_img=ti)
    with pytest.raises(RuntimeError, match="timg_count"):             # (a CPU tensor is counted by the library)
        u(x, 500, timestep_img=torch.zeros(3, dtype=torch.int64))
    torch.cuda.synchronize()

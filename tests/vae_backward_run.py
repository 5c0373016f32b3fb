"""GPU-side helpers of the decoder-backward tests: objects per (configuration, mode), the direct call of
ldmseg_vae_decode_backward, and the per-kernel checks of one decoder shape - every backward operator entry of csrc/ops_api.hip at the
layer shapes of the configuration against torch.autograd.grad of the matching torch op in fp64 (bound: vae_backward_ref.BOUND), and
the forward operators at the same shapes for the dispatch-log proof."""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

import vae_backward_ref as R

DEV = "cuda:0"
OP_DTYPE = {"fp32": 0, "bf16x3": 3}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


@functools.lru_cache(maxsize=None)
def vae(name, mode):
    from ldmseg_amd.models import GeneralVAESeg
    return GeneralVAESeg(R.state_dict(name), device=DEV, compute_dtype=mode, scaling_factor=0.2, **R.CONFIGS[name])


def decode_backward(v, z, gl, keys, want_z=True, z_scale=1.0, numel_of=None, raw=False):
    """One ldmseg_vae_decode_backward call -> {key: gradient, "z": gradient} on the device (raw: the return code instead of a check).
    keys: names to ask for; a (key, None) pair passes a NULL pointer for that key."""
    from ldmseg_amd import _lib
    sd = v._dec_sd
    zc, glc = dev(z), dev(gl)
    B, _, L, _ = zc.shape
    names, bufs = [], []
    for k in keys:
        null = isinstance(k, tuple)
        k = k[0] if null else k
        names.append(k)
        bufs.append(None if null else torch.full_like(sd[k], float("nan")) if k in sd else torch.empty(4, device=DEV))
    n = len(names)
    c_names = (C.c_char_p * max(n, 1))(*[k.encode() for k in names])
    c_ptrs = (C.c_void_p * max(n, 1))(*[None if b is None else b.data_ptr() for b in bufs])
    numels = [(numel_of or {}).get(k, sd[k].numel() if k in sd else 4) for k in names]
    c_numels = (C.c_int64 * max(n, 1))(*numels)
    gz = torch.full_like(zc, float("nan")) if want_z else None
    with torch.cuda.device(DEV):
        code = _lib.lib().ldmseg_vae_decode_backward(v._h, P(zc), float(z_scale), B, L, P(glc), P(gz), n, c_names, c_ptrs, c_numels,
                                                     _lib.stream_ptr(torch.device(DEV)))
    if raw:
        msg = _lib.lib().ldmseg_last_error()
        return code, (msg.decode() if msg else "")
    _lib.check(code, "ldmseg_vae_decode_backward")
    torch.cuda.synchronize()
    out = {k: b for k, b in zip(names, bufs) if b is not None}
    if want_z:
        out["z"] = gz
    return out


def logged(fn):
    """fn() with the dispatch log on -> (result, set of kernel names)"""
    from ldmseg_amd import _lib
    _lib.igemm_log(_lib.LOG_ALL)
    try:
        res = fn()
        torch.cuda.synchronize()
        names = _lib.igemm_log_read()
    finally:
        _lib.igemm_log(False)
    return res, names


# ------------------------------------------------------------------ the layers of a configuration
def layers(name, B, L):
    """[(kind, dict)] of the decoder's layers at one shape, forward order"""
    cfg = R.CONFIGS[name]
    out = [("conv", dict(B=B, Ci=cfg["latent_channels"], Co=cfg["int_channels"], H=L, nchw_dx=1))]
    side, cin = L, cfg["int_channels"]
    for _ in range(cfg["num_upscalers"]):
        out.append(("convt", dict(B=B, Ci=cin, Co=cfg["upscale_channels"], H=side)))
        side, cin = 2 * side, cfg["upscale_channels"]
        out.append(("ln", dict(M=B * side * side, C=cin, H2=side)))
    out.append(("gn", dict(B=B, C=cin, HW=side * side)))
    out.append(("conv", dict(B=B, Ci=cin, Co=cfg["out_channels"], H=side, nchw_dx=0)))
    return out


def _gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0xffffff)      # (hash() of a str differs per process)


def _ok(lib, code):
    assert code == 0, (code, lib.ldmseg_last_error())
    torch.cuda.synchronize()


def _other(h, w):
    """the second side of a map as part of a seed key, where it differs from the first (square maps keep the seeds they had)"""
    return () if w == h else (w,)


def report(what, e):
    print(f"{what}: {e:.3e}")
    return e


def check_conv(lib, q, mode, forward=False):
    """3x3 conv: weight + bias gradient, data gradient (the latents' through the fp32 NCHW epilogue) vs F.conv2d under fp64 autograd"""
    B, Ci, Co, H, W = q["B"], q["Ci"], q["Co"], q["H"], q.get("W", q["H"])
    g = _gen("conv", B, Ci, Co, H, *_other(H, W))
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    b = torch.randn(Co, generator=g)
    dy = torch.randn(B, Co, H, W, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xd, wd, bd, padding=1)
    rx, rw, rb = torch.autograd.grad(y, [xd, wd, bd], dy.double())
    dt = OP_DTYPE[mode]
    dx_, dw_, db_, dy_ = dev(x), dev(w), dev(b), dev(dy)
    if forward:
        out = torch.empty(B, Co, H, W, device=DEV)
        _ok(lib, lib.ldmseg_op_vae_conv(P(dx_), P(dw_), P(db_), None, B, Ci, H, W, Co, 3, 1, -1, 0, 0 if q["nchw_dx"] else 2, 0, dt, P(out), None))
        assert report(f"conv fwd {q} {mode}", R.metric(out, y.detach())) < R.BOUND
    gw, gb = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV), torch.full((Co,), float("nan"), device=DEV)
    _ok(lib, lib.ldmseg_op_conv_wgrad(P(dx_), P(dy_), B, Ci, H, W, Co, dt, P(gw), P(gb), None))
    assert report(f"conv wgrad {q} {mode}", R.metric(gw, rw)) < R.BOUND
    assert report(f"conv bgrad {q} {mode}", R.metric(gb, rb)) < R.BOUND
    gx = torch.full((B, Ci, H, W), float("nan"), device=DEV)
    _ok(lib, lib.ldmseg_op_conv_dgrad(P(dy_), P(dw_), B, Ci, H, W, Co, q["nchw_dx"], dt, P(gx), None))
    assert report(f"conv dgrad {q} {mode}", R.metric(gx, rx)) < R.BOUND


def check_convt(lib, q, mode, forward=False):
    B, Ci, Co, H, W = q["B"], q["Ci"], q["Co"], q["H"], q.get("W", q["H"])
    g = _gen("convt", B, Ci, Co, H, *_other(H, W))
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Ci, Co, 2, 2, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g)
    dy = torch.randn(B, Co, 2 * H, 2 * W, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv_transpose2d(xd, wd, bd, stride=2)
    rx, rw, rb = torch.autograd.grad(y, [xd, wd, bd], dy.double())
    dt = OP_DTYPE[mode]
    dx_, dw_, db_, dy_ = dev(x), dev(w), dev(b), dev(dy)
    if forward:
        out = torch.empty(B, Co, 2 * H, 2 * W, device=DEV)
        _ok(lib, lib.ldmseg_op_convt2(P(dx_), P(dw_), P(db_), B, Ci, H, W, Co, dt, P(out), None))
        assert report(f"convt fwd {q} {mode}", R.metric(out, y.detach())) < R.BOUND
    gw, gb = torch.full((Ci, Co, 2, 2), float("nan"), device=DEV), torch.full((Co,), float("nan"), device=DEV)
    _ok(lib, lib.ldmseg_op_convt2_wgrad(P(dx_), P(dy_), B, Ci, H, W, Co, dt, P(gw), P(gb), None))
    assert report(f"convt wgrad {q} {mode}", R.metric(gw, rw)) < R.BOUND
    assert report(f"convt bgrad {q} {mode}", R.metric(gb, rb)) < R.BOUND
    gx = torch.full((B, Ci, H, W), float("nan"), device=DEV)
    _ok(lib, lib.ldmseg_op_convt2_dgrad(P(dy_), P(dw_), B, Ci, H, W, Co, dt, P(gx), None))
    assert report(f"convt dgrad {q} {mode}", R.metric(gx, rx)) < R.BOUND


def phase_major(t, B, H2, C, W2=None):
    """[B * H2 * W2, C] rows (image, Y, X) -> [B, H2/2, W2/2, 2x2, C] rows (W2 = H2 where not given)"""
    W2 = H2 if W2 is None else W2
    return t.view(B, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


def check_ln(lib, q, mode, forward=False, pm=1):
    """LayerNorm2d + SiLU backward over pixel rows, stored phase-major as the decoder's backward stores it (pm = 0: in row order)"""
    M, Cn, H2, W2 = q["M"], q["C"], q["H2"], q.get("W2", q["H2"])
    B = M // (H2 * W2)
    g = _gen("ln", M, Cn, *_other(H2, W2))
    x = torch.randn(M, Cn, generator=g) * 3 + 1
    x[::7] *= 20.0                                             # rows of very different scale
    gamma = 1 + 0.1 * torch.randn(Cn, generator=g)
    beta = 0.1 * torch.randn(Cn, generator=g)
    dy = torch.randn(M, Cn, generator=g)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.silu(F.layer_norm(xd, (Cn,), gd, bd, 1e-6))
    rx, rg, rb = torch.autograd.grad(y, [xd, gd, bd], dy.double())
    dx_, dg_, db_, dy_ = dev(x), dev(gamma), dev(beta), dev(dy)
    if forward:
        out = torch.empty(M, Cn, device=DEV)
        _ok(lib, lib.ldmseg_op_layernorm_io(P(dx_), P(dg_), P(db_), M, Cn, 1e-6, 1, 0, 0, P(out), None))
        assert report(f"ln fwd {q}", R.metric(out, y.detach())) < R.BOUND
    gx, gg, gb = (torch.full(s, float("nan"), device=DEV) for s in ((M, Cn), (Cn,), (Cn,)))
    _ok(lib, lib.ldmseg_op_layernorm_silu_bwd(P(dx_), P(dy_), P(dg_), P(db_), M, Cn, 1e-6, pm, H2, W2, P(gx), P(gg), P(gb), None))
    want = phase_major(rx, B, H2, Cn, W2) if pm else rx
    assert report(f"ln bwd dx {q} pm={pm}", R.metric(gx, want)) < R.BOUND
    assert report(f"ln bwd dgamma {q}", R.metric(gg, rg)) < R.BOUND
    assert report(f"ln bwd dbeta {q}", R.metric(gb, rb)) < R.BOUND


def check_gn(lib, q, mode, forward=False):
    B, Cn, HW = q["B"], q["C"], q["HW"]
    g = _gen("gn", B, Cn, HW, *(("far",) if q.get("far") else ()))
    grp = torch.arange(Cn) // (Cn // 32)
    mean = 2.0 - 4.0 * (grp % 2).float() + 0.5 * torch.randn(Cn, generator=g)      # neighbouring groups differ
    std = 0.5 + 1.5 * (grp % 3).float()
    if q.get("far"):                                           # every channel mean 1000, deviation 1: E[x^2] - E[x]^2 cancels 6 digits
        mean, std = torch.full((Cn,), 1000.0), torch.ones(Cn)
    x = torch.randn(B, Cn, HW, generator=g) * std[None, :, None] + mean[None, :, None]
    gamma = 1 + 0.1 * torch.randn(Cn, generator=g)
    beta = 0.1 * torch.randn(Cn, generator=g)
    dy = torch.randn(B, Cn, HW, generator=g)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.silu(F.group_norm(xd, 32, gd, bd, 1e-5))
    rx, rg, rb = torch.autograd.grad(y, [xd, gd, bd], dy.double())
    dx_, dg_, db_, dy_ = dev(x), dev(gamma), dev(beta), dev(dy)
    if forward:
        out = torch.empty(B, Cn, HW, device=DEV)
        _ok(lib, lib.ldmseg_op_groupnorm(P(dx_), None, P(dg_), P(db_), B, Cn, 0, HW, 1e-5, 1, 0, P(out), None))
        assert report(f"gn fwd {q}", R.metric(out, y.detach())) < R.BOUND
    gx, gg, gb = (torch.full(s, float("nan"), device=DEV) for s in ((B, Cn, HW), (Cn,), (Cn,)))
    _ok(lib, lib.ldmseg_op_groupnorm_silu_bwd(P(dx_), P(dy_), P(dg_), P(db_), B, Cn, HW, 1e-5, P(gx), P(gg), P(gb), None))
    assert report(f"gn bwd dx {q}", R.metric(gx, rx)) < R.BOUND
    assert report(f"gn bwd dgamma {q}", R.metric(gg, rg)) < R.BOUND
    assert report(f"gn bwd dbeta {q}", R.metric(gb, rb)) < R.BOUND


CHECK = {"conv": check_conv, "convt": check_convt, "ln": check_ln, "gn": check_gn}

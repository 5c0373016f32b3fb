"""ldmseg_vae_encode_backward and ldmseg_vae_load_encoder on the GPU: every gradient of the encoder against the fp64
torch-CPU reference of tests/vae_encode_backward_ref.py (metric max|g - g64| / max|g64|, bound 1e-3, "fp32" and "bf16x3"; torch's own
fp32 CPU autograd is printed beside it) and the structural properties of the entry."""
import ctypes as C

import pytest
import torch

import vae_backward_run as G
import vae_encode_backward_ref as R
import vae_encode_backward_run as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def all_keys(name):
    return R.encoder_keys(R.CONFIGS[name])


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def test_the_encoder_has_twenty_tensors_with_real_channels_only():
    keys = all_keys("seg")
    assert len(keys) == 20
    assert tuple(R.state_dict("seg")["encoder.0.weight"].shape) == (32, 7, 3, 3)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.SHAPES, ids=ident)
def test_all_gradients_vs_fp64_reference(case, mode):
    name, B, H = case
    torch.set_num_threads(16)
    x, gm = R.inputs(name, B, H)
    got = E.encode_backward(E.vae(name, mode), name, x, gm, all_keys(name))
    r64, r32 = R.reference(name, B, H), R.reference_fp32(name, B, H)
    assert set(got) == set(r64)
    worst, worst32 = {}, {}
    for k in r64:
        e, e32 = R.metric(got[k], r64[k]), R.metric(r32[k], r64[k])
        print(f"{name} B={B} H={H} {mode} {k}: library {e:.3e}  torch fp32 CPU {e32:.3e}")
        c = R.tensor_class(k)
        worst[c], worst32[c] = max(worst.get(c, 0.0), e), max(worst32.get(c, 0.0), e32)
    print(f"{name} B={B} H={H} {mode} worst per class: " + ", ".join(f"{c} {e:.2e} (torch fp32 {worst32[c]:.2e})" for c, e in sorted(worst.items())))
    for k in r64:
        assert torch.isfinite(got[k]).all(), k
        assert R.metric(got[k], r64[k]) < R.BOUND, (case, mode, k)


@pytest.mark.parametrize("mode", R.MODES)
def test_zero_gradient_in_gives_exact_zeros(mode):
    name, B, H = "seg", 2, 24
    x, gm = R.inputs(name, B, H)
    got = E.encode_backward(E.vae(name, mode), name, x, torch.zeros_like(gm), all_keys(name))
    for k, g in got.items():
        assert torch.count_nonzero(g) == 0, k


@pytest.mark.parametrize("mode", R.MODES)
def test_batch_gradient_is_the_sum_of_its_images(mode):
    name, B, H = "seg", 3, 40
    x, gm = R.inputs(name, B, H)
    v = E.vae(name, mode)
    whole = E.encode_backward(v, name, x, gm, all_keys(name))
    parts = [E.encode_backward(v, name, x[b:b + 1], gm[b:b + 1], all_keys(name)) for b in range(B)]
    for k in all_keys(name):
        total = sum(p[k].double() for p in parts).cpu()
        assert R.metric(whole[k], total) < R.BOUND, k


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", [("seg", 3, 40), ("reduced", 2, 24)], ids=ident)
def test_no_halo_crosses_an_image(case, mode):
    """grad_moments non-zero in image 0 only: every op of the encoder is per image, so the gradients equal image 0 run alone"""
    name, B, H = case
    x, gm = R.inputs(name, B, H)
    gm = gm.clone()
    gm[1:] = 0
    v = E.vae(name, mode)
    got = E.encode_backward(v, name, x, gm, all_keys(name))
    alone = E.encode_backward(v, name, x[:1], gm[:1], all_keys(name))
    for k in all_keys(name):
        assert torch.count_nonzero(alone[k]) > 0, k
        assert R.metric(got[k], alone[k].double().cpu()) < 1e-5, k      # (the slices of the pixel axis differ: fp32 rounding only)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", [("seg", 1, 16), ("seg", 2, 24)], ids=ident)
def test_two_calls_give_identical_bits(case, mode):
    """one pixel slice at full resolution (16^2) and several (2 x 24^2: tests/test_wgrad_plan_ex_cpu.py keeps that true)"""
    name, B, H = case
    x, gm = R.inputs(name, B, H)
    v = E.vae(name, mode)
    a = E.encode_backward(v, name, x, gm, all_keys(name))
    v.encode_moments(G.dev(x))                                   # another call on the handle in between: the backward keeps no state
    b = E.encode_backward(v, name, x, gm, all_keys(name))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_absent_and_null_names_leave_the_rest_unchanged():
    name, B, H = "seg", 2, 24
    x, gm = R.inputs(name, B, H)
    v = E.vae(name, "fp32")
    keys = all_keys(name)
    full = E.encode_backward(v, name, x, gm, keys)
    some = E.encode_backward(v, name, x, gm, [keys[0], (keys[1], None), keys[5], keys[-2], keys[-4]])
    assert set(some) == {keys[0], keys[5], keys[-2], keys[-4]}
    for k in some:
        assert torch.equal(some[k], full[k]), k
    # only the head: the chain below it is not run, its result is the same
    head = E.encode_backward(v, name, x, gm, keys[-2:])
    for k in head:
        assert torch.equal(head[k], full[k]), k
    assert E.encode_backward(v, name, x, gm, []) == {}


def test_errors_come_with_a_message_and_launch_nothing():
    name, B, H = "seg", 1, 16
    x, gm = R.inputs(name, B, H)
    keys = all_keys(name)
    v, vb = E.vae(name, "fp32"), E.vae(name, "bf16")
    for call, word in ((lambda: E.encode_backward(vb, name, x, gm, keys, raw=True), "fp32-storage"),
                       (lambda: E.encode_backward(v, name, x, gm, ["encoder.1.weight"], raw=True), "not an encoder parameter"),
                       (lambda: E.encode_backward(v, name, x, gm, ["decoder.0.weight"], raw=True), "not an encoder parameter"),
                       (lambda: E.encode_backward(v, name, x, gm, [keys[0]], numel_of={keys[0]: 7}, raw=True), "elements")):
        (code, msg), names = G.logged(call)
        assert code == -1 and word in msg, (code, msg)
        assert not names, names


def _load(lib, v, sd, keys):
    n = len(keys)
    ts = [G.dev(sd[k]) for k in keys]
    names = (C.c_char_p * n)(*[k.encode() for k in keys])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    numels = (C.c_int64 * n)(*[t.numel() for t in ts])
    code = lib.ldmseg_vae_load_encoder(v._h, n, names, ptrs, numels, None)
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("mode", R.MODES)
def test_load_encoder_makes_the_handle_one_built_from_the_new_tensors(lib, mode):
    """forward and backward, bitwise: an object built from state dict A and loaded with B's encoder equals an object built from B"""
    from ldmseg_amd import weights
    from ldmseg_amd.models import GeneralVAESeg
    name, B, H = "seg", 2, 24
    cfg = R.CONFIGS[name]
    sd_b = R.state_dict(name)
    sd_a = weights.generate(R.schema(cfg), seed=99)
    keys = all_keys(name)
    v = GeneralVAESeg(sd_a, device=G.DEV, compute_dtype=mode, **cfg)
    fresh = E.vae(name, mode)
    x, gm = R.inputs(name, B, H)
    assert not torch.equal(v.encode_moments(G.dev(x) * 2 - 1), fresh.encode_moments(G.dev(x) * 2 - 1))
    assert _load(lib, v, sd_b, keys) == 0
    assert torch.equal(v.encode_moments(G.dev(x) * 2 - 1), fresh.encode_moments(G.dev(x) * 2 - 1))
    a, b = E.encode_backward(v, name, x, gm, keys), E.encode_backward(fresh, name, x, gm, keys)
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def test_load_encoder_errors(lib):
    v = E.vae("seg", "fp32")
    t = torch.zeros(16, device=G.DEV)
    for key, numel in (("encoder.1.weight", 16), ("encoder.0.bias", 16), ("decoder.0.bias", 256)):
        names, ptrs, numels = (C.c_char_p * 1)(key.encode()), (C.c_void_p * 1)(t.data_ptr()), (C.c_int64 * 1)(numel)
        assert lib.ldmseg_vae_load_encoder(v._h, 1, names, ptrs, numels, None) == -1
        assert lib.ldmseg_last_error()


def _per_kernel_checks(lib, name, B, H, mode):
    """every operator entry the encoder's backward is made of, at the layer shapes of one call, each compared with the fp64 torch op
    (forward) or torch.autograd.grad of it (backward) under the gate: a kernel name in the log of this function has been compared at
    that launch shape"""
    import torch.nn.functional as F
    cfg = R.CONFIGS[name]
    dt = G.OP_DTYPE[mode]
    P, dev = G.P, G.dev
    layers = R.conv_layers(cfg)
    for i, (idx, Ci, Co, stride, level) in enumerate(layers):
        side = H >> level
        g = G._gen("enc-layer", idx, B, side)
        xc, wc, bc = torch.randn(B, Ci, side, side, generator=g), torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5, torch.randn(Co, generator=g)
        xd, wd, bd = (t.double().requires_grad_(True) for t in (xc, wc, bc))
        y = F.conv2d(xd, wd, bd, stride=stride, padding=1)
        dyc = torch.randn(y.shape, generator=g)
        rx, rw, rb = torch.autograd.grad(y, [xd, wd, bd], dyc.double())
        x, w, b, dy = dev(xc), dev(wc), dev(bc), dev(dyc)
        what = f"{name} B={B} H={H} {mode} encoder.{idx}"
        if i < len(layers) - 1:                                  # the forward again: the SiLU-less store form (+ silu_fwd where SiLU follows)
            out = torch.empty(y.shape, device=G.DEV)
            G._ok(lib, lib.ldmseg_op_vae_conv(P(x), P(w), P(b), None, B, Ci, side, side, Co, 3, stride, -1, 0, 0, (Co + 31) // 32 * 32, dt, P(out), None))
            assert R.metric(out, y.detach()) < R.BOUND, what
            if stride == 2 or i == 0:
                a, du = torch.empty_like(out), torch.empty_like(out)
                G._ok(lib, lib.ldmseg_op_silu_fwd(P(out), out.numel(), P(a), None))
                ud = out.double().cpu().requires_grad_(True)
                act = F.silu(ud)
                assert R.metric(a, act.detach()) < 1e-5, what
                G._ok(lib, lib.ldmseg_op_silu_bwd(P(out), P(dy), out.numel(), P(du), None))
                assert R.metric(du, torch.autograd.grad(act, [ud], dyc.double())[0]) < 1e-5, what
        gw, gb = torch.full((Co, Ci, 3, 3), float("nan"), device=G.DEV), torch.full((Co,), float("nan"), device=G.DEV)
        G._ok(lib, lib.ldmseg_op_conv_wgrad_ex(P(x), P(dy), B, Ci, side, side, Co, stride, dt, P(gw), P(gb), None))
        assert R.metric(gw, rw) < R.BOUND and R.metric(gb, rb) < R.BOUND, what
        if i > 0:
            gx = torch.full((B, Ci, side, side), float("nan"), device=G.DEV)
            if stride == 2:
                G._ok(lib, lib.ldmseg_op_conv_s2_dgrad(P(dy), P(w), B, Ci, side, side, Co, dt, P(gx), None))
            else:
                G._ok(lib, lib.ldmseg_op_conv_dgrad(P(dy), P(w), B, Ci, side, side, Co, 0, dt, P(gx), None))
            assert R.metric(gx, rx) < R.BOUND, what
    l = H // 8
    G.check_gn(lib, dict(B=B, C=cfg["int_channels"], HW=l * l), mode, forward=True)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.SHAPES, ids=ident)
def test_every_encode_backward_launch_is_compared_per_kernel(lib, case, mode):
    """The dispatch log of one encode_backward call, per shape and mode: every kernel name in it (template arguments included) is
    also logged by the per-kernel checks at the layer shapes of that call, which compare every result with fp64."""
    name, B, H = case
    torch.set_num_threads(16)
    x, gm = R.inputs(name, B, H)
    v = E.vae(name, mode)
    _, used = G.logged(lambda: E.encode_backward(v, name, x, gm, all_keys(name)))
    fam = "x3" if mode == "bf16x3" else "f32"
    assert any(n.startswith(f"wgrad9<{fam},32,32>/taps9") for n in used) and any(n.endswith("/s2") for n in used), used
    assert "silu_bwd<f32>" in used and "silu_fwd<f32>" in used and "gn_silu_bwd_stats<f32>" in used and any(n.startswith("igemm<") for n in used)
    _, tested = G.logged(lambda: _per_kernel_checks(lib, name, B, H, mode))
    assert used <= tested, sorted(used - tested)

"""Every weight-gradient kernel the by-width chooser can name (csrc/vae_bwd.hip, csrc/wgrad_plan.h) against
torch.autograd.grad of F.conv2d in fp64, at the widths of tests/wgrad_cases.py: partial tiles, two tiles per axis, odd non-square
maps, one slice and several - and the item walk: a workgroup that takes several (tile, slice) items gives the bits of one workgroup
per item (debug key 26 hands the chooser a smaller CU count; the slicing, and with it the order of every addition, is a function of
the shape alone).  Metric max|g - g64| / max|g64|, bound 1e-3, in the fp32 and the split-bf16 products; the walk is exact."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import vae_backward_ref as RD
import vae_backward_run as G
import vae_encode_backward_ref as R
import vae_encode_backward_run as E
import wgrad_cases as WC

pytestmark = pytest.mark.gpu
P, dev, DEV = G.P, G.dev, G.DEV
KEY_CUS = 26


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


@contextlib.contextmanager
def chooser_cus(lib, cus):
    """debug key 26 = cus inside the block, 0 (the device's) after it"""
    try:
        assert lib.ldmseg_debug_set(KEY_CUS, cus) == 0
        yield
    finally:
        lib.ldmseg_debug_set(KEY_CUS, 0)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and fp64 gradients of one launch, computed once and shared (do not modify)"""
    B, Ci, Co, H, W, stride = shape
    torch.set_num_threads(16)
    return R.conv_case(B, Ci, Co, H, W, stride)


def _device_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _plan(lib, shape, mode, cus):
    code, line, f, _ = R.wgrad_plan_ex(lib, *WC.desc(*shape), x3=int(mode != "fp32"), cus=cus)
    assert code == 0, shape
    return line.split()[0], f


def _wgrad(lib, shape, mode, x_, dy_):
    B, Ci, Co, H, W, stride = shape
    gw, gb = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV), torch.full((Co,), float("nan"), device=DEV)
    G._ok(lib, lib.ldmseg_op_conv_wgrad_ex(P(x_), P(dy_), B, Ci, H, W, Co, stride, G.OP_DTYPE[mode], P(gw), P(gb), None))
    return gw, gb


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", WC.launches(), ids=WC.ident)
def test_weight_bias_and_data_gradient_vs_fp64_autograd(lib, shape, mode):
    B, Ci, Co, H, W, stride = shape
    x, w, dy, rx, rw, rb = _case(shape)
    dt = G.OP_DTYPE[mode]
    x_, dy_, w_ = dev(x), dev(dy), dev(w)                        # (kept alive: the entries take raw pointers)
    assert lib.ldmseg_debug_get(KEY_CUS) == 0
    name, f = _plan(lib, shape, mode, _device_cus())
    (gw, gb), names = G.logged(lambda: _wgrad(lib, shape, mode, x_, dy_))
    assert name in names, (name, names)                          # the kernel the plan predicts is the one that ran
    what = f"{name} {WC.ident(shape)}"
    if (B, H, W) != WC.ODD:
        assert int(f["slices"]) > 1, f                           # the slab sum adds several slices
    if (Ci, Co, stride) == WC.BIG:
        assert int(f["tiles"]) == 270 and int(f["slices"]) == 1
        if _device_cus() <= 256:
            assert f["one_per_cu"] == "0" and int(f["grid"]) == _device_cus(), f      # workgroups walk the items
    assert G.report(f"{what} wgrad", R.metric(gw, rw)) < R.BOUND
    assert G.report(f"{what} bgrad", R.metric(gb, rb)) < R.BOUND
    gx = torch.full((B, Ci, H, W), float("nan"), device=DEV)
    if stride == 2:
        if Ci % 4:
            return
        G._ok(lib, lib.ldmseg_op_conv_s2_dgrad(P(dy_), P(w_), B, Ci, H, W, Co, dt, P(gx), None))
    else:
        G._ok(lib, lib.ldmseg_op_conv_dgrad(P(dy_), P(w_), B, Ci, H, W, Co, 0, dt, P(gx), None))
    assert G.report(f"{what} dgrad", R.metric(gx, rx)) < R.BOUND


def test_the_walk_launches_name_all_eighteen_kernels(lib):
    for mode in R.MODES:
        names = {_plan(lib, s, mode, 256)[0] for s in WC.walk_launches()}
        assert len(names) == 18, sorted(names)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", WC.walk_launches(), ids=WC.ident)
def test_a_workgroup_that_walks_several_items_gives_the_same_bits(lib, shape, mode):
    """the chooser told of 3 CUs (a four-slice all-taps launch: one workgroup takes two items, two take one) and of 1 (one workgroup
    walks everything; kept to launches of at most 36 items) against the device's own count"""
    x, w, dy, rx, rw, rb = _case(shape)
    x_, dy_ = dev(x), dev(dy)
    name, f0 = _plan(lib, shape, mode, _device_cus())
    items = int(f0["tiles"]) * int(f0["slices"])
    assert int(f0["slices"]) > 1 and items > 3
    (gw0, gb0), names = G.logged(lambda: _wgrad(lib, shape, mode, x_, dy_))
    assert name in names, (name, names)
    assert G.report(f"{name} {WC.ident(shape)} wgrad", R.metric(gw0, rw)) < R.BOUND
    assert G.report(f"{name} {WC.ident(shape)} bgrad", R.metric(gb0, rb)) < R.BOUND
    for cus in (3, 1) if items <= 36 else (3,):
        n, f = _plan(lib, shape, mode, cus)
        assert n == name and f["one_per_cu"] == "0" and int(f["grid"]) == cus, f
        assert (f["tiles"], f["slices"], f["steps"]) == (f0["tiles"], f0["slices"], f0["steps"])
        with chooser_cus(lib, cus):
            assert lib.ldmseg_debug_get(KEY_CUS) == cus
            (gw, gb), names = G.logged(lambda: _wgrad(lib, shape, mode, x_, dy_))
        assert name in names, (name, names)
        assert torch.equal(gw, gw0) and torch.equal(gb, gb0), (name, cus)
    assert lib.ldmseg_debug_get(KEY_CUS) == 0


# (entry, B, Ci, Co, H, W, taps): the decoder's rule (128 x 128 whatever the widths).  3x3: 18 tiles x 2 slices; the transposed conv
# of the decoder's widths is ONE item (N = 4 Co = 128, C = 64, 120 pixels) - nothing to walk, it is held to the same bits all the
# same - and 160 -> 64 is 2 x 2 tiles of the one-tap form, the second column tile 32 wide
DECODER_RULE = [("conv", 2, 256, 128, 16, 16, 9), ("convt", 2, 64, 32, 6, 10, 1), ("convt", 2, 160, 64, 6, 10, 1)]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", DECODER_RULE, ids=WC.ident)
def test_the_decoders_rule_walks_to_the_same_bits(lib, case, mode):
    kind, B, Ci, Co, H, W, taps = case
    g = G._gen("walk", *case)
    x = dev(torch.randn(B, Ci, H, W, generator=g))
    dy = dev(torch.randn(B, Co, H, W, generator=g) if kind == "conv" else torch.randn(B, Co, 2 * H, 2 * W, generator=g))
    N = WC.storage(Co) if kind == "conv" else 4 * Co
    dt = G.OP_DTYPE[mode]

    def run():
        gw = torch.full((Co, Ci, 3, 3) if kind == "conv" else (Ci, Co, 2, 2), float("nan"), device=DEV)
        gb = torch.full((Co,), float("nan"), device=DEV)
        fn = lib.ldmseg_op_conv_wgrad if kind == "conv" else lib.ldmseg_op_convt2_wgrad
        G._ok(lib, fn(P(x), P(dy), B, Ci, H, W, Co, dt, P(gw), P(gb), None))
        return gw, gb

    def plan(cus):
        code, line, f = RD.wgrad_plan(lib, B * H * W, N, WC.storage(Ci), taps, int(mode != "fp32"), cus)
        assert code == 0
        return line.split()[0], f

    name, f0 = plan(_device_cus())
    items = int(f0["tiles"]) * int(f0["slices"])
    (gw0, gb0), names = G.logged(run)
    assert name in names, (name, names)
    # (both ops are linear in w: the weight gradient does not depend on its value)
    wd = torch.zeros(gw0.shape, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double().cpu(), wd, padding=1) if kind == "conv" else F.conv_transpose2d(x.double().cpu(), wd, stride=2)
    rw, = torch.autograd.grad(y, [wd], dy.double().cpu())
    assert G.report(f"{name} {WC.ident(case)} wgrad", R.metric(gw0, rw)) < R.BOUND
    assert G.report(f"{name} {WC.ident(case)} bgrad", R.metric(gb0, dy.double().cpu().sum((0, 2, 3)))) < R.BOUND
    for cus in (3, 1):
        n, f = plan(cus)
        assert n == name and (f["tiles"], f["slices"], f["steps"]) == (f0["tiles"], f0["slices"], f0["steps"])
        assert f["one_per_cu"] == ("0" if items > cus else "1") and int(f["grid"]) == min(cus, items), f
        with chooser_cus(lib, cus):
            gw, gb = run()
        assert torch.equal(gw, gw0) and torch.equal(gb, gb0), (name, cus)
    assert lib.ldmseg_debug_get(KEY_CUS) == 0
    if case != DECODER_RULE[1]:
        assert items > 3                                         # (these two walk at 3 and at 1)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", [("seg", 1, 16), ("reduced", 2, 24)], ids=WC.ident)
def test_encode_backward_on_five_cus_gives_the_same_bits(lib, case, mode):
    name, B, H = case
    x, gm = R.inputs(name, B, H)
    v = E.vae(name, mode)
    keys = R.encoder_keys(R.CONFIGS[name])
    a = E.encode_backward(v, name, x, gm, keys)
    with chooser_cus(lib, 5):
        b = E.encode_backward(v, name, x, gm, keys)
    assert lib.ldmseg_debug_get(KEY_CUS) == 0
    assert set(a) == set(b) == set(keys)
    for k in keys:
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", [("seg", 1, 2), RD.MULTI_SLICE], ids=WC.ident)
def test_decode_backward_on_five_cus_gives_the_same_bits(lib, case, mode):
    name, B, L = case
    z, gl = RD.inputs(name, B, L)
    v = G.vae(name, mode)
    keys = RD.decoder_keys(RD.CONFIGS[name])
    a = G.decode_backward(v, z, gl, keys)
    with chooser_cus(lib, 5):
        b = G.decode_backward(v, z, gl, keys)
    assert lib.ldmseg_debug_get(KEY_CUS) == 0
    assert set(a) == set(b) == set(keys) | {"z"}
    for k in a:
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k

"""Parity of the SHIPPED implicit-GEMM instantiations at the real UNet launch shapes of the three single-GPU
configurations of BASELINE.json: configs[1] (B = 8, L = 64), configs[3] (B = 16, L = 64), configs[4] (B = 4, L = 128).

Every distinct conv / Linear / GEGLU launch shape of a UNet forward of each configuration is launched through
``ldmseg_op_igemm`` - the engine's own launch path: NHWC operands, the engine's split-K plan, the row-major store /
GEGLU epilogues, residual and time-embedding bias rows - in bf16, fp32 and bf16x3 (split-bf16 products on weight planes) under
the shipped tile policy, and compared with the torch-CPU op the reference executes there (F.conv2d / F.linear / GEGLU of
diffusers 0.16.1).  So is every GroupNorm (including the conv -> GroupNorm fused finish) and every self-attention
level, in each compute mode.  Each test records, through the dispatch log at its every-family level (csrc/kernels.h
LDMSEG_LAUNCH), every kernel it launched - name, template arguments and run-time form; the last test runs full-size forwards with the dispatch log on and
fails if the forward launched a kernel that no per-op oracle comparison above has exercised at that configuration's shapes.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
X3W = 3     # operator dtype 3: fp32 tensors, split-bf16 products, weights as hi | lo planes - what a bf16x3 handle runs
# (batch, latent size): the measured launch table (csrc/igemm_tuned.inc) has entries - instantiation x K-slice count - for
# exactly these three; every other shape goes through the rules that the same lists exercise (tests/test_offgrid_shapes_gpu.py runs
# the helpers below at configurations off the power-of-two grid, where those rules fall the other way)
CONFIGS = [(8, 64), (16, 64), (4, 128)]
CFG_IDS = [f"b{b}l{l}" for b, l in CONFIGS]
# compute modes of the forward: "bf16fp8" = bf16 with UNet.set_attention_fp8() (BASELINE configs[4]); it runs what bf16 runs
# except the fp8 attention levels, so the proof checks it against SEEN["bf16"] | SEEN["bf16fp8"]
MODES = ("bf16", "fp32", "bf16x3", "bf16fp8")
MODE = {BF16: "bf16", F32: "fp32"}
SEEN = {(c, m): set() for c in CONFIGS for m in MODES}


@contextlib.contextmanager
def recorded(L, seen, cfg, *modes):
    """dispatch log on (every family) around the body; every name it logged is added to seen[(cfg, mode)] of each mode given"""
    L.igemm_log(L.LOG_ALL)
    try:
        yield
        torch.cuda.synchronize()
        names = L.igemm_log_read()
    finally:
        L.igemm_log(False)
    for m in modes:
        seen[(cfg, m)] |= names


@pytest.fixture(scope="module")
def L():
    from ldmseg_amd import _lib
    assert _lib.lib().ldmseg_debug_get(1) == _lib.lib().ldmseg_debug_get(-1), "a previous test leaked a tile policy"
    assert _lib.lib().ldmseg_debug_get(12) == 3 and _lib.lib().ldmseg_debug_get(14) == 3, "a previous test leaked a fused-kernel switch"
    assert _lib.lib().ldmseg_debug_get(19) == 1 and _lib.lib().ldmseg_debug_get(17) == 0 and _lib.lib().ldmseg_debug_get(20) == 1 and \
        _lib.lib().ldmseg_debug_get(21) == 1 and _lib.lib().ldmseg_debug_get(22) == 1, \
        "a previous test leaked a GEMM-path switch"
    return _lib


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def dev(t):
    return t.to("cuda", torch.float32).contiguous() if t is not None else None


def P(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# (H, Ci, Ci2, Co, k, stride, up, geglu, resid, rowbias)  -  H = input side AT L = 64 (scaled by L / 64 for the other latent size)
SHAPES = [
    # ---- 64x64 maps (M = 32768)
    (64, 320, 0, 320, 3, 1, 0, 0, 0, 1),      # resnet conv1 (+ time-embedding row)
    (64, 320, 0, 320, 3, 1, 0, 0, 1, 0),      # resnet conv2 (+ residual)
    (64, 320, 320, 320, 3, 1, 0, 0, 0, 1),    # up-path conv1 on cat([h, skip])
    (64, 640, 320, 320, 3, 1, 0, 0, 0, 1),
    (64, 12, 0, 320, 3, 1, 0, 0, 0, 0),       # conv_in
    (64, 320, 0, 320, 1, 1, 0, 0, 1, 0),      # proj_out / to_out (+ residual)
    (64, 320, 0, 320, 1, 1, 0, 0, 0, 0),      # proj_in
    (64, 320, 0, 960, 1, 1, 0, 0, 0, 0),      # fused q|k|v
    (64, 320, 0, 2560, 1, 1, 0, 1, 0, 0),     # GEGLU
    (64, 1280, 0, 320, 1, 1, 0, 0, 1, 0),     # ff.net.2 (+ residual)
    (64, 320, 320, 320, 1, 1, 0, 0, 0, 0),    # conv_shortcut on a concat
    (64, 640, 320, 320, 1, 1, 0, 0, 0, 0),
    (32, 640, 0, 640, 3, 1, 1, 0, 0, 0),      # upsampler conv: nearest x2 folded into the gather (M = 32768)
    (64, 320, 0, 320, 3, 2, 0, 0, 0, 0),      # downsampler conv, stride 2 (M = 8192)
    # ---- 32x32 maps (M = 8192)
    (32, 640, 0, 640, 3, 1, 0, 0, 0, 1),
    (32, 640, 0, 640, 3, 1, 0, 0, 1, 0),
    (32, 320, 0, 640, 3, 1, 0, 0, 0, 1),
    (32, 640, 640, 640, 3, 1, 0, 0, 0, 1),
    (32, 1280, 640, 640, 3, 1, 0, 0, 0, 1),
    (32, 640, 320, 640, 3, 1, 0, 0, 0, 1),
    (32, 640, 0, 640, 1, 1, 0, 0, 1, 0),
    (32, 640, 0, 1920, 1, 1, 0, 0, 0, 0),
    (32, 640, 0, 5120, 1, 1, 0, 1, 0, 0),
    (32, 2560, 0, 640, 1, 1, 0, 0, 1, 0),
    (32, 2560, 640, 640, 1, 1, 0, 0, 1, 0),   # ff.net.2 + proj_out chained into one Linear over cat([g, h]) (+ x) - round 5
    (32, 320, 0, 640, 1, 1, 0, 0, 0, 0),
    (32, 1280, 640, 640, 1, 1, 0, 0, 0, 0),
    (32, 640, 640, 640, 1, 1, 0, 0, 0, 0),
    (32, 640, 320, 640, 1, 1, 0, 0, 0, 0),
    (16, 1280, 0, 1280, 3, 1, 1, 0, 0, 0),    # upsampler conv 16 -> 32 (M = 8192)
    (32, 640, 0, 640, 3, 2, 0, 0, 0, 0),      # downsampler (M = 2048)
    # ---- 16x16 maps (M = 2048)
    (16, 1280, 0, 1280, 3, 1, 0, 0, 0, 1),
    (16, 1280, 0, 1280, 3, 1, 0, 0, 1, 0),
    (16, 640, 0, 1280, 3, 1, 0, 0, 0, 1),
    (16, 1280, 1280, 1280, 3, 1, 0, 0, 0, 1),
    (16, 1280, 640, 1280, 3, 1, 0, 0, 0, 1),
    (16, 1280, 0, 1280, 1, 1, 0, 0, 1, 0),
    (16, 1280, 0, 3840, 1, 1, 0, 0, 0, 0),
    (16, 1280, 0, 10240, 1, 1, 0, 1, 0, 0),
    (16, 5120, 0, 1280, 1, 1, 0, 0, 1, 0),
    (16, 5120, 1280, 1280, 1, 1, 0, 0, 1, 0),  # chained ff.net.2 + proj_out
    (16, 640, 0, 1280, 1, 1, 0, 0, 0, 0),
    (16, 1280, 1280, 1280, 1, 1, 0, 0, 0, 0),
    (16, 1280, 640, 1280, 1, 1, 0, 0, 0, 0),
    (8, 1280, 0, 1280, 3, 1, 1, 0, 0, 0),     # upsampler conv 8 -> 16 (M = 2048)
    (16, 1280, 0, 1280, 3, 2, 0, 0, 0, 0),    # downsampler (M = 512)
    # ---- 8x8 maps (M = 512)
    (8, 1280, 0, 1280, 3, 1, 0, 0, 0, 1),
    (8, 1280, 0, 1280, 3, 1, 0, 0, 1, 0),
    (8, 1280, 1280, 1280, 3, 1, 0, 0, 0, 1),
    (8, 1280, 0, 1280, 1, 1, 0, 0, 1, 0),
    (8, 1280, 0, 3840, 1, 1, 0, 0, 0, 0),
    (8, 1280, 0, 10240, 1, 1, 0, 1, 0, 0),
    (8, 5120, 0, 1280, 1, 1, 0, 0, 1, 0),
    (8, 5120, 1280, 1280, 1, 1, 0, 0, 1, 0),   # chained ff.net.2 + proj_out
    (8, 1280, 1280, 1280, 1, 1, 0, 0, 0, 0),
]


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("case", SHAPES)
def test_unet_layer_shape_vs_oracle(L, dt, cfg, case):
    check_layer_shape(L, SEEN, dt, cfg, case)


def check_layer_shape(L, seen, dt, cfg, case):
    H, Ci, Ci2, Co, k, stride, up, geglu, use_res, use_rb = case
    B, lat = cfg
    H = H * lat // 64
    torch.set_num_threads(64)
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    ct = Ci + Ci2
    x = torch.randn(B, Ci, H, H, generator=g)
    x2 = torch.randn(B, Ci2, H, H, generator=g) if Ci2 else None
    w = torch.randn(Co, ct, k, k, generator=g) / (ct * k * k) ** 0.5
    b = torch.randn(Co, generator=g)
    rb = torch.randn(B, Co, generator=g) if use_rb else None
    xin = torch.cat([x, x2], 1) if Ci2 else x
    xin_r, w_r = (bf16_round(xin), bf16_round(w)) if dt == BF16 else (xin, w)
    if up:
        xin_r = F.interpolate(xin_r, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin_r, w_r, b, stride=stride, padding=k // 2)
    if rb is not None:
        ref = ref + rb[:, :, None, None]
    if geglu:
        a, gate = ref.chunk(2, 1)
        ref = a * F.gelu(gate)
    res = torch.randn(ref.shape, generator=g) if use_res else None
    if res is not None:
        ref = ref + (bf16_round(res) if dt == BF16 else res)
    out = torch.empty(ref.shape, device="cuda")
    dx, dx2, dw, db, dres, drb = dev(x), dev(x2), dev(w), dev(b), dev(res), dev(rb)
    with recorded(L, seen, cfg, MODE[dt]):
        r = L.lib().ldmseg_op_igemm(P(dx), P(dx2), P(dw), P(db), P(dres), P(drb), B, Ci, Ci2, H, H, Co, k, stride, up, geglu,
                                    0, 0, dt, P(out), None)
        assert r == 0, L.lib().ldmseg_last_error()
    name = L.igemm_last_kernel()
    # bf16: operands rounded identically, the difference is accumulation order + the bf16 rounding of the stored output
    e = rel_err(out, ref)
    assert e < (8e-3 if dt == BF16 else 1e-4), (cfg, case, name)
    if dt == F32:
        # bf16x3: the same unrounded reference, the bound of the split-bf16 operator tests (test_ops_gpu X3_CASES)
        out3 = torch.empty(ref.shape, device="cuda")
        with recorded(L, seen, cfg, "bf16x3"):
            r = L.lib().ldmseg_op_igemm(P(dx), P(dx2), P(dw), P(db), P(dres), P(drb), B, Ci, Ci2, H, H, Co, k, stride, up, geglu,
                                        0, 0, X3W, P(out3), None)
            assert r == 0, L.lib().ldmseg_last_error()
        name3 = L.igemm_last_kernel()
        assert name3.startswith("igemm<f32,") and ",x3w>" in name3, name3
        e3 = rel_err(out3, ref)
        assert e3 < 1e-4, (cfg, case, name3, e3, f"exact-fp32 kernel: {e:.2e}")
    if "/splitk-cf" in name:
        # the same instantiation writes plain slabs where the consumer is not the launch itself (resnet conv1 -> norm2 on the small
        # maps: the fused finish + GroupNorm kernel reads them): compare that form here too - bit for bit with the in-launch finish
        lib = L.lib()
        saved = lib.ldmseg_debug_get(23)
        out2 = torch.empty(ref.shape, device="cuda")
        try:
            assert lib.ldmseg_debug_set(23, 0) == 0
            with recorded(L, seen, cfg, MODE[dt]):
                assert lib.ldmseg_op_igemm(P(dx), P(dx2), P(dw), P(db), P(dres), P(drb), B, Ci, Ci2, H, H, Co, k, stride, up, geglu,
                                           0, 0, dt, P(out2), None) == 0
            name2 = L.igemm_last_kernel()
        finally:
            lib.ldmseg_debug_set(23, saved)
        assert name2.split(" ")[0] == name.split(" ")[0].replace("/splitk-cf", "/splitk"), (name, name2)
        assert torch.equal(out2, out), (cfg, case, name2)


LN_SHAPES = [   # (M at B = 8 / L = 64, K = C, N, geglu): norm1 -> q|k|v and norm3 -> ff.net.0.proj of every transformer level
    (32768, 320, 960, 0), (32768, 320, 2560, 1), (8192, 640, 1920, 0), (8192, 640, 5120, 1),
    (2048, 1280, 3840, 0), (2048, 1280, 10240, 1), (512, 1280, 3840, 0), (512, 1280, 10240, 1),
]


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("M,K,N,geglu", LN_SHAPES)
def test_unet_layernorm_folded_gemm_vs_oracle(L, dt, cfg, M, K, N, geglu):
    check_layernorm_folded_gemm(L, SEEN, dt, cfg, M, K, N, geglu)


def check_layernorm_folded_gemm(L, seen, dt, cfg, M, K, N, geglu):
    """LayerNorm -> Linear / GEGLU of the transformer blocks as the engine runs them: one statistics pass, then the GEMM
    on the un-normalised tokens with gamma folded into the weights and rstd*(acc - mean*c1) + c2 in the epilogue (its own
    template instantiations, ',ln').  Reference: F.layer_norm + F.linear (+ GEGLU); the tokens carry a large common offset
    (mean 3, std 1.5) so the mean cancellation of the epilogue is exercised."""
    torch.set_num_threads(64)
    M = M * cfg[0] * cfg[1] * cfg[1] // (8 * 64 * 64)
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g) * 1.5 + 3.0
    gamma = 1 + 0.2 * torch.randn(K, generator=g)
    beta = 0.2 * torch.randn(K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    xr = bf16_round(x) if dt == BF16 else x
    y = F.linear(F.layer_norm(xr, (K,), gamma, beta, 1e-5), w, b)
    if geglu:
        a, gate = y.chunk(2, -1)
        y = a * F.gelu(gate)
    out = torch.empty(y.shape, device="cuda")
    dx, dg, db, dw, dbias = dev(x), dev(gamma), dev(beta), dev(w), dev(b)
    with recorded(L, seen, cfg, MODE[dt]):
        assert L.lib().ldmseg_op_ln_linear(P(dx), P(dg), P(db), P(dw), P(dbias), M, K, N, 1e-5, geglu, dt, P(out), None) == 0
    name = L.igemm_last_kernel()
    assert ",ln" in name
    # bf16: gamma*W and the output are rounded to bf16 (the unfolded form rounds LN(x) and W instead)
    e = rel_err(out, y)
    assert e < (1.5e-2 if dt == BF16 else 1e-4), name
    if dt == F32:       # bf16x3 (weight planes); bound of the split-bf16 LayerNorm-fold operator test (test_ops_gpu)
        out3 = torch.empty(y.shape, device="cuda")
        with recorded(L, seen, cfg, "bf16x3"):
            assert L.lib().ldmseg_op_ln_linear(P(dx), P(dg), P(db), P(dw), P(dbias), M, K, N, 1e-5, geglu, X3W, P(out3), None) == 0
        name3 = L.igemm_last_kernel()
        assert ",ln" in name3 and ",x3w>" in name3, name3
        e3 = rel_err(out3, y)
        assert e3 < 2e-4, (name3, e3, f"exact-fp32 kernel: {e:.2e}")


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_conv_out_shape_vs_oracle(L, dt, cfg):
    check_conv_out_shape(L, SEEN, dt, cfg)


def check_conv_out_shape(L, seen, dt, cfg, tail=True):
    """conv_out: 320 -> 4 channels at the full latent resolution, written straight to fp32 NCHW (EPI_NCHW_F32, the narrow-N tile).
    tail: the shape has the step-tail kernel (conv_out_tail_ok), so the bf16 forward runs conv_out through it."""
    B, lat = cfg
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 320, lat, lat, generator=g)
    w = torch.randn(4, 320, 3, 3, generator=g) / 2880 ** 0.5
    b = torch.randn(4, generator=g)
    xr, wr = (bf16_round(x), bf16_round(w)) if dt == BF16 else (x, w)
    ref = F.conv2d(xr, wr, b, padding=1)
    out = torch.empty(ref.shape, device="cuda")
    dx, dw, db = dev(x), dev(w), dev(b)
    with recorded(L, seen, cfg, MODE[dt]):
        assert L.lib().ldmseg_op_conv2d(P(dx), None, P(dw), P(db), B, 320, 0, lat, lat, 4, 3, 1, 0, dt, P(out), None) == 0
    assert rel_err(out, ref) < (1e-3 if dt == BF16 else 1e-4)
    if dt == F32:           # bf16x3 (dtype 3: weight planes, what the handles hold), same unrounded reference
        out3 = torch.empty(ref.shape, device="cuda")
        with recorded(L, seen, cfg, "bf16x3"):
            assert L.lib().ldmseg_op_conv2d(P(dx), None, P(dw), P(db), B, 320, 0, lat, lat, 4, 3, 1, 0, X3W, P(out3), None) == 0
        assert ",x3w>" in L.igemm_last_kernel(), L.igemm_last_kernel()
        assert rel_err(out3, ref) < 1e-4, rel_err(out3, ref)
    if dt == BF16 and tail:     # the bf16 forward runs conv_out as the halo-resident stencil of tail.hip
        out2 = torch.empty(ref.shape, device="cuda")
        with recorded(L, seen, cfg, "bf16"):
            assert L.lib().ldmseg_op_conv_out_tail(P(dx), P(dw), P(db), B, lat, lat, P(out2), 0, 0, None, 0, 0, 1.0, None, None, None,
                                                   None, None, None, 0.0, 0.0, None, None) == 0
        assert rel_err(out2, ref) < 1e-3


# conv2 + conv_shortcut of the resnets whose input and output channel counts differ, as the bf16 forward runs them (round 5):
# ONE launch, K = 9 * C + Cs + Cs2.  (H at L = 64, C = cout, Cs = hidden channels, Cs2 = skip channels of torch.cat([h, skip], 1))
XT_SHAPES = [
    (64, 320, 640, 320), (64, 320, 320, 320),                                           # up_blocks.3
    (32, 640, 1280, 640), (32, 640, 640, 640), (32, 640, 640, 320), (32, 640, 320, 0),  # up_blocks.2, down_blocks.1.resnets.0
    (16, 1280, 1280, 1280), (16, 1280, 1280, 640), (16, 1280, 640, 0),                  # up_blocks.1, down_blocks.2.resnets.0
    (8, 1280, 1280, 1280),                                                              # up_blocks.0
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("case", XT_SHAPES)
def test_resnet_tail_one_launch_vs_oracle(L, cfg, case):
    check_resnet_tail_one_launch(L, SEEN, cfg, case)


def check_resnet_tail_one_launch(L, seen, cfg, case):
    """F.conv2d(h, w2, b2, padding=1) + F.conv2d(cat([x, skip]), ws, bs) (diffusers ResnetBlock2D: conv2 + conv_shortcut) against the
    engine's single extra-tap launch at the configuration's shapes; records the ',xt' instantiation that ran."""
    import ctypes as C
    H, Cc, Cs, Cs2 = case
    B, lat = cfg
    H = H * lat // 64
    torch.set_num_threads(64)
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    h = torch.randn(B, Cc, H, H, generator=g)
    xs = torch.randn(B, Cs, H, H, generator=g)
    xs2 = torch.randn(B, Cs2, H, H, generator=g) if Cs2 else None
    w2 = torch.randn(Cc, Cc, 3, 3, generator=g) / (9 * Cc) ** 0.5
    ws = torch.randn(Cc, Cs + Cs2, 1, 1, generator=g) / (Cs + Cs2) ** 0.5
    b2, bs = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    xin = torch.cat([xs, xs2], 1) if Cs2 else xs
    ref = F.conv2d(bf16_round(h), bf16_round(w2), b2, padding=1) + F.conv2d(bf16_round(xin), bf16_round(ws), bs)
    out = torch.empty(ref.shape, device="cuda")
    dh, dxs, dxs2, dw2, dws, db2, dbs = dev(h), dev(xs), dev(xs2), dev(w2), dev(ws), dev(b2), dev(bs)
    with recorded(L, seen, cfg, "bf16"):
        r = L.lib().ldmseg_op_conv3x3_plus_1x1(P(dh), P(dw2), P(db2), P(dxs), P(dxs2), P(dws), P(dbs), B, Cc, Cs, Cs2, H, H, Cc, 0, BF16,
                                               P(out), 0, None, None)
        assert r == 0, (r, L.lib().ldmseg_last_error())
    name = L.igemm_last_kernel()
    assert ",xt" in name, name
    assert rel_err(out, ref) < 8e-3, (cfg, case, name)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_fused_feed_forward_at_config_shape(L, cfg):
    check_fused_feed_forward(L, SEEN, cfg)


def check_fused_feed_forward(L, seen, cfg):
    """The row-local fused feed-forward kernel (tfuse.hip: LayerNorm_3 -> GEGLU -> ff.net.2 (+h) -> proj_out (+x)) that the
    bf16 forward runs on the 320-channel level, at this configuration's token count M = B * L * L, against torch on the same
    bf16-rounded operands (the arithmetic of oracle/unet.py::transformer)."""
    from test_ops_gpu import _ff_case, _ff_ref, _ff_run
    B, lat = cfg
    M = B * lat * lat
    case = _ff_case(M, 320, 7 + M)
    ref = _ff_ref(*case)
    for mode, name in ((3, "mlp_fused<bf16,proj=1>"), (1, "mlp_fused<bf16,proj=0>")):
        with recorded(L, seen, cfg, "bf16"):
            out, _ = _ff_run(L, case, M, 320, mode)
        assert name in seen[(cfg, "bf16")]
        l2 = float((out.double() - ref.double()).norm() / ref.double().norm())
        assert torch.isfinite(out).all() and l2 < 6e-3 and rel_err(out, ref) < 3e-2, (cfg, mode, l2)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_fused_transformer_entry_at_config_shape(L, cfg):
    check_fused_transformer_entry(L, SEEN, cfg)


def check_fused_transformer_entry(L, seen, cfg):
    """The row-local fused entry kernel (tproj.hip: proj_in -> LayerNorm_1 -> q|k|v) that the bf16 forward runs on the
    320-channel level, at this configuration's token count, against torch on the same bf16-rounded operands."""
    from test_ops_gpu import _tin_case, _tin_ref, _tin_run
    B, lat = cfg
    M = B * lat * lat
    case = _tin_case(M, 320, 11 + M)
    href, qref = _tin_ref(*case)
    with recorded(L, seen, cfg, "bf16"):
        h, qkv, _ = _tin_run(L, case, M, 320, 1)
    assert "proj_ln_qkv<bf16>" in seen[(cfg, "bf16")]
    l2 = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    assert torch.isfinite(qkv).all() and l2(h, href) < 3e-3 and l2(qkv, qref) < 6e-3, (cfg, l2(h, href), l2(qkv, qref))


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_fused_transformer_entry_with_groupnorm_at_config_shape(L, cfg):
    check_fused_transformer_entry_with_groupnorm(L, SEEN, cfg)


def check_fused_transformer_entry_with_groupnorm(L, seen, cfg):
    """The same kernel with the transformer's GroupNorm folded in (statistics pass + apply sweep on the LDS tile: what the bf16
    forward launches since round 5), at this configuration's image count and map size, against torch GroupNorm -> proj_in ->
    LayerNorm_1 -> q|k|v on the bf16-rounded operands."""
    import torch.nn.functional as F
    from test_ops_gpu import _gtin_run, _tin_case, _tin_ref, bf16_round
    B, lat = cfg
    HW, M = lat * lat, B * lat * lat
    g = torch.Generator().manual_seed(13 + M)
    case = _tin_case(M, 320, 17 + M)
    x = torch.randn(B, HW, 320, generator=g) * (0.5 + torch.rand(1, 1, 320, generator=g)) + 2.0 * torch.randn(1, 1, 320, generator=g)
    gg = 1 + 0.3 * torch.randn(320, generator=g)
    gb = 0.3 * torch.randn(320, generator=g)
    xn = F.group_norm(bf16_round(x).permute(0, 2, 1).reshape(B, 320, HW, 1), 32, gg, gb, 1e-6).reshape(B, 320, HW).permute(0, 2, 1)
    href, qref = _tin_ref(xn.reshape(M, 320), *case[1:])
    with recorded(L, seen, cfg, "bf16"):
        h, qkv, _ = _gtin_run(L, x.reshape(M, 320), gg, gb, B, 1, case, M, 320, 1)
    assert "proj_ln_qkv<bf16,gn>" in seen[(cfg, "bf16")]
    l2 = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    assert torch.isfinite(qkv).all() and l2(h, href) < 4e-3 and l2(qkv, qref) < 7e-3, (cfg, l2(h, href), l2(qkv, qref))


# ---- GroupNorm: every (C, C2, eps, SiLU) a forward normalises, per map side at L = 64 (scaled by L / 64).  C2 = the skip
# channels of torch.cat([h, skip], 1) the up-path resnets normalise.  eps 1e-5 + SiLU: resnet norm1 / norm2 and conv_norm_out;
# eps 1e-6, no SiLU: the transformers' norm (the bf16 forward folds the 320-channel one into the fused entry kernel).
# tests/test_shape_lists_cpu.py checks this list (and ATTN_LEVELS below) against the layer walk of oracle/unet.py.
GN_SHAPES = [
    (64, 320, 0, 1e-5, 1), (64, 640, 320, 1e-5, 1), (64, 320, 320, 1e-5, 1), (64, 320, 0, 1e-6, 0),
    (32, 320, 0, 1e-5, 1), (32, 640, 0, 1e-5, 1), (32, 1280, 640, 1e-5, 1), (32, 640, 640, 1e-5, 1), (32, 640, 320, 1e-5, 1),
    (32, 640, 0, 1e-6, 0),
    (16, 640, 0, 1e-5, 1), (16, 1280, 0, 1e-5, 1), (16, 1280, 1280, 1e-5, 1), (16, 1280, 640, 1e-5, 1), (16, 1280, 0, 1e-6, 0),
    (8, 1280, 0, 1e-5, 1), (8, 1280, 1280, 1e-5, 1), (8, 1280, 0, 1e-6, 0),
]


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("case", GN_SHAPES)
def test_unet_groupnorm_shape_vs_oracle(L, dt, cfg, case):
    check_groupnorm_shape(L, SEEN, dt, cfg, case)


def check_groupnorm_shape(L, seen, dt, cfg, case):
    """F.group_norm(cat([x, x2], 1), 32) (+ SiLU) in fp64 on the storage-rounded input against ldmseg_op_groupnorm at the
    configuration's (B, C, C2, H x W): the kernel form the launcher picks there (gn_group / gn_coop / gn_one / gn_fused / gn_small /
    gn_partial + gn_apply: chosen from B * groups, the map size and the CU count) is the one the forward runs.  Two launches, bit
    for bit.  The bf16x3 forward runs the fp32 kernels."""
    H, Cc, C2, eps, silu = case
    B, lat = cfg
    H = H * lat // 64
    HW = H * H
    torch.set_num_threads(64)
    g = torch.Generator().manual_seed(Cc + 7 * C2 + HW + B)
    x = torch.randn(B, Cc, HW, generator=g) * 2 + 0.5
    x[:, :, : HW // 3] += 3.0
    x2 = torch.randn(B, C2, HW, generator=g) - 1.0 if C2 else None
    gamma = 1 + 0.1 * torch.randn(Cc + C2, generator=g)
    beta = 0.1 * torch.randn(Cc + C2, generator=g)
    xin = torch.cat([x, x2], 1) if C2 else x
    ref = F.group_norm((bf16_round(xin) if dt == BF16 else xin).double(), 32, gamma.double(), beta.double(), eps)
    if silu:
        ref = F.silu(ref)
    outs = [torch.empty(B, Cc + C2, HW, device="cuda") for _ in range(2)]
    dx, dx2, dg, db = dev(x), dev(x2), dev(gamma), dev(beta)
    with recorded(L, seen, cfg, *(("bf16",) if dt == BF16 else ("fp32", "bf16x3"))):
        for o in outs:
            assert L.lib().ldmseg_op_groupnorm(P(dx), P(dx2), P(dg), P(db), B, Cc, C2, HW, eps, silu, dt, P(o), None) == 0
    assert torch.isfinite(outs[0]).all()
    assert rel_err(outs[0], ref) < (8e-3 if dt == BF16 else 5e-5), (cfg, case)
    assert torch.equal(outs[0], outs[1]), (cfg, case)


# resnet conv1 -> norm2 on the smaller maps: (H at L = 64, Ci = conv1's input channels, Co).  Where the conv runs as K slices the
# forward sums them inside the GroupNorm launch (launch_finish_groupnorm, finish_gn_kernel) instead of storing the conv output.
CONV_GN_SHAPES = [
    (32, 320, 640), (32, 640, 640), (32, 1920, 640), (32, 1280, 640), (32, 960, 640),
    (16, 640, 1280), (16, 1280, 1280), (16, 2560, 1280), (16, 1920, 1280),
    (8, 1280, 1280), (8, 2560, 1280),
]


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_conv_groupnorm_fused_finish_at_config_shapes(L, dt, cfg):
    assert check_conv_groupnorm_fused_finish(L, SEEN, dt, cfg) >= 1, cfg


def check_conv_groupnorm_fused_finish(L, seen, dt, cfg):
    """ldmseg_op_conv_groupnorm at every resnet conv1 -> norm2 shape of the configuration, with the K-slice count the engine plans
    there (read from the plain conv launch), against F.conv2d + time-embedding row + F.group_norm + SiLU in fp64 on the rounded
    operands.  Shapes the engine does not K-slice (one slice planned) or has no fused form for (-4) are skipped over; at least one shape per configuration is
    fused (the 8x8 level always is).  The bf16x3 forward runs the fp32 finish kernel after its own split-bf16 K slices."""
    B, lat = cfg
    torch.set_num_threads(64)
    fused = 0
    for H, Ci, Co in CONV_GN_SHAPES:
        H = H * lat // 64
        g = torch.Generator().manual_seed(Ci + H + Co)
        x = torch.randn(B, Ci, H, H, generator=g)
        w = torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5
        b = torch.randn(Co, generator=g)
        rb = 2.0 * torch.randn(B, Co, generator=g)
        gamma = 1 + 0.1 * torch.randn(Co, generator=g)
        beta = 0.1 * torch.randn(Co, generator=g)
        dx, dw, db, drb, dg, dbe = dev(x), dev(w), dev(b), dev(rb), dev(gamma), dev(beta)
        probe = torch.empty(B, Co, H, H, device="cuda")
        assert L.lib().ldmseg_op_igemm(P(dx), None, P(dw), P(db), None, P(drb), B, Ci, 0, H, H, Co, 3, 1, 0, 0, 0, 0, dt, P(probe),
                                       None) == 0
        torch.cuda.synchronize()
        splits = int(L.igemm_last_kernel().split("splits=")[1].split()[0])
        if splits < 2:
            continue
        rnd = bf16_round if dt == BF16 else (lambda t: t)
        h = F.conv2d(rnd(x).double(), rnd(w).double(), b.double(), padding=1) + rb.double()[:, :, None, None]
        ref = F.silu(F.group_norm(h, 32, gamma.double(), beta.double(), 1e-5))
        out = torch.empty(ref.shape, device="cuda")
        with recorded(L, seen, cfg, *(("bf16",) if dt == BF16 else ("fp32", "bf16x3"))):
            r = L.lib().ldmseg_op_conv_groupnorm(P(dx), P(dw), P(db), P(drb), P(dg), P(dbe), B, Ci, H, H, Co, 1e-5, 1, splits, dt,
                                                 P(out), None)
            if r == -4:         # no finish-GroupNorm instantiation for the shape (finish_groupnorm_ok): the engine keeps conv and norm apart
                continue
            assert r == 0, (r, L.lib().ldmseg_last_error(), H, Ci, Co)
        fused += 1
        assert torch.isfinite(out).all()
        assert rel_err(out, ref) < (8e-3 if dt == BF16 else 2e-4), (cfg, H, Ci, Co, splits)
    return fused


# ---- self-attention: every (map side at L = 64, C) level of the UNet, 8 heads (head dim 40 / 80 / 160 / 160)
ATTN_LEVELS = [(64, 320), (32, 640), (16, 1280), (8, 1280)]
ATTN_DT = {"bf16": BF16, "fp32": F32, "bf16x3": 2}      # 2: fp32 tensors, split-bf16 products (unet.hip launches it so)


def attention_rows(qkv, B, N, Cc):
    """query rows the reference covers: about 256 evenly spaced ones plus the last 130 (the ragged end of every tile form)"""
    step = max(1, N // 256)
    return sorted(set(range(0, N, step)) | set(range(max(0, N - 130), N)))


def attention_ref_rows(src, rows, Cc):
    """fp64 softmax(q k^T d^-1/2) v of ONE image [N, 3C] for the given query rows, every key; query chunks keep the score
    matrix small (a 16384^2 fp64 matrix per head would be 2 GB)"""
    d = Cc // 8
    q, k, v = src.double().chunk(3, -1)
    k = k.reshape(-1, 8, d).transpose(0, 1)
    v = v.reshape(-1, 8, d).transpose(0, 1)
    q = q[rows].reshape(-1, 8, d).transpose(0, 1)
    outs = []
    for r0 in range(0, q.shape[1], 128):
        outs.append(torch.softmax((q[:, r0:r0 + 128] @ k.transpose(-1, -2)) * d ** -0.5, -1) @ v)
    return torch.cat(outs, 1).transpose(0, 1).reshape(len(rows), Cc)


def _attn_case(B, N, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3 * Cc, generator=g)
    qkv[:, :, :Cc] *= 2.0                       # sharper softmax
    for b in (0, B - 1):
        qkv[b, N // 2, Cc:Cc + 40] += 6.0       # one dominant key: the running-max rescale path
    return qkv


@pytest.mark.parametrize("mode", ["bf16", "fp32", "bf16x3"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("level", ATTN_LEVELS)
def test_unet_attention_level_vs_oracle(L, mode, cfg, level):
    check_attention_level(L, SEEN, mode, cfg, level)


def check_attention_level(L, seen, mode, cfg, level):
    """ldmseg_op_attention at the configuration's (B, N = H x W, C) of every transformer level, in the operator dtype the forward
    launches for the mode (the 4- / 8-wave forms are chosen from B * heads * ceil(N / 256), head dim 160 goes to attention.hip):
    the first and last image against fp64 on the storage-rounded input, on sampled query rows.  Bounds of test_attention /
    test_split_bf16_attention (test_ops_gpu)."""
    side, Cc = level
    B, lat = cfg
    N = (side * lat // 64) ** 2
    torch.set_num_threads(64)
    qkv = _attn_case(B, N, Cc, N + Cc + B)
    out = torch.empty(B, N, Cc, device="cuda")
    dq = dev(qkv)
    with recorded(L, seen, cfg, mode):
        assert L.lib().ldmseg_op_attention(P(dq), B, N, Cc, 8, ATTN_DT[mode], P(out), None) == 0, L.lib().ldmseg_last_error()
    assert torch.isfinite(out).all()
    src = bf16_round(qkv) if mode == "bf16" else qkv
    rows = attention_rows(qkv, B, N, Cc)
    for b in (0, B - 1):
        ref = attention_ref_rows(src[b], rows, Cc)
        e = rel_err(out[b, rows].cpu(), ref)
        assert e < {"bf16": 2e-2, "fp32": 2e-5, "bf16x3": 1e-4}[mode], (cfg, level, mode, b, e)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_unet_attention_fp8_level_vs_oracle(L, cfg):
    check_attention_fp8_level(L, SEEN, cfg)


def check_attention_fp8_level(L, seen, cfg):
    """ldmseg_op_attention_fp8 at the head-dim-40 level of the configuration (the only one a bf16 forward with set_attention_fp8()
    takes to the fp8 path: N >= 4096 on whole 128-key tiles): first and last image against fp64 on the same e4m3-quantised
    operands and on the unquantised ones.  Bounds of test_attention_fp8_path (test_ops_gpu)."""
    from test_ops_gpu import fp8_e4m3_round
    B, lat = cfg
    N, Cc, d = lat * lat, 320, 40
    torch.set_num_threads(64)
    g = torch.Generator().manual_seed(N + B)
    qkv = torch.randn(B, N, 3 * Cc, generator=g)
    qkv[:, :, :Cc] *= 1.5
    out = torch.empty(B, N, Cc, device="cuda")
    dq = dev(qkv)
    with recorded(L, seen, cfg, "bf16fp8"):
        assert L.lib().ldmseg_op_attention_fp8(P(dq), B, N, Cc, 8, P(out), 0, None, None) == 0
    assert torch.isfinite(out).all()
    # (N <= 4096: every query row, so that the max-norm is taken over the same population as in test_attention_fp8_path)
    rows = list(range(N)) if N <= 4096 else attention_rows(qkv, B, N, Cc)
    sc = torch.tensor(d ** -0.5, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    for b in (0, B - 1):
        src = bf16_round(qkv[b])
        q8 = fp8_e4m3_round(src[:, :Cc] * sc) / sc               # the kernel quantises q * d^-1/2 log2 e
        ref8 = attention_ref_rows(torch.cat([q8, fp8_e4m3_round(src[:, Cc:])], -1), rows, Cc)
        ref = attention_ref_rows(src, rows, Cc)
        o = out[b, rows].cpu()
        e_same, e_total = rel_err(o, ref8), rel_err(o, ref)
        l2 = float((o.double() - ref).norm() / ref.norm())
        print(f"fp8 attention {cfg} image {b}: vs quantised operands {e_same:.3e}, vs unquantised {e_total:.3e}, rel-L2 {l2:.3e}")
        assert e_same < 4e-2 and e_total < 0.2 and l2 < 0.1, (cfg, b, e_same, e_total, l2)


GN_FAMILY = ("gn_", "finish_gn<")
ATTN_FAMILY = ("attn", "kv_to_")


# (mode, operator dtype of its GEMMs)
@pytest.mark.parametrize("mode,dt", [("bf16", BF16), ("fp32", F32), ("bf16x3", X3W), ("bf16fp8", BF16)])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_every_forward_instantiation_is_oracle_tested(L, unet_sd, cfg, mode, dt):
    check_every_forward_instantiation(L, SEEN, unet_sd, cfg, mode, dt)


def check_every_forward_instantiation(L, seen, unet_sd, cfg, mode, dt, fp8_level=None):
    """Run a forward of the configuration (BASELINE configs[1] / [3] / [4]) in the compute mode with the dispatch log on: every
    kernel it launches - igemm instantiation (tile shape, wave layout, ring depth, K-sliced or not, split-bf16 marker), GroupNorm /
    LayerNorm-statistics / attention form with its template arguments, fused kernels - must be one that a per-op test above has
    just compared with the oracle AT THIS CONFIGURATION'S shapes and in this mode.  bf16fp8 = bf16 with set_attention_fp8().
    fp8_level: whether a bf16fp8 forward must / must not launch an fp8 attention kernel (None: must from 4096 tokens up, the
    tuned configurations' rule).  Returns the names the forward launched."""
    from ldmseg_amd.models import UNet
    B, lat = cfg
    u = UNet(unet_sd, in_channels=12, device="cuda:0", compute_dtype="bf16" if mode == "bf16fp8" else mode)
    if mode == "bf16fp8":
        u.set_attention_fp8()
    x = torch.randn(B, 12, lat, lat, generator=torch.Generator().manual_seed(1)).cuda()
    L.igemm_log(L.LOG_ALL)
    try:
        y = u(x, 499).sample
        torch.cuda.synchronize()
        used = L.igemm_log_read()
    finally:
        L.igemm_log(False)
    assert torch.isfinite(y).all()
    assert len(used) >= 4, used
    fam = {"igemm": sorted(n for n in used if n.startswith("igemm<")), "gn": sorted(n for n in used if n.startswith(GN_FAMILY)),
           "attn": sorted(n for n in used if n.startswith(ATTN_FAMILY))}
    print(f"{cfg} {mode}: {len(used)} names - " + ", ".join(f"{k} {len(v)}" for k, v in fam.items()) +
          f", other {len(used) - sum(len(v) for v in fam.values())}")
    assert fam["gn"] and fam["attn"], (cfg, mode, sorted(used))
    if mode == "bf16x3":
        assert all(",x3w>" in n for n in fam["igemm"]), fam["igemm"]      # every GEMM of the mode on the split-bf16 K loop
    if fp8_level is None:
        fp8_level = True if lat * lat >= 4096 else None
    if mode == "bf16fp8" and fp8_level is not None:
        assert any(n.startswith(("attn_mx<", "attn_fp8<")) for n in fam["attn"]) == fp8_level, fam["attn"]
    tested = seen[(cfg, mode)] | (seen[(cfg, "bf16")] if mode == "bf16fp8" else set())
    missing = used - tested
    assert not missing, (f"{cfg} {mode}: forward kernels without a per-op oracle test: {sorted(missing)}; "
                         f"tested: {sorted(tested)}")
    return used

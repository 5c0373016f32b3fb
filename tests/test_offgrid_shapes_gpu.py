"""The per-op oracle comparisons of tests/test_igemm_shapes_gpu.py and its closing proof, away from the power-of-two shape grid.

The C ABI takes any batch B >= 1 and any latent side L % 8 == 0; the tuned configurations (and every forward test on the grid
L in {16, 32, 64, 128}) only ever give the kernels row counts M = B * H * W that are whole 128- / 256-row tiles and maps with
HW % 128 == 0.  The configurations below put every level of the UNet on the other side of those rules - partial GEMM tiles that
straddle an image boundary, the fused transformer entry declining or running without its GroupNorm fold, no step tail, attention
over 25 / 81 / 9 / 1 tokens, a one-pixel GroupNorm, 3x3 convs whose taps are mostly padding - and two of them reuse the tuned
launch-table entries' M with images of another size:

  (1, 8)     maps 8, 4, 2, 1: M = 64, 16, 4, 1
  (3, 24)    M = 1728, 432, 108, 27: no level is a multiple of 128; B * groups = 96
  (2, 40)    M = 3200 (% 128 == 0) with HW = 1600 (% 128 != 0): fused entry without the GroupNorm fold
  (5, 40)    odd batch with B * groups >= 128; M = 8000, 2000, 500, 125
  (3, 72)    N = 5184 >= 4096 tokens but not whole 128-key tiles: set_attention_fp8() must leave the level on the bf16 kernel
  (2, 96)    N = 9216 = 72 x 128: the fp8 path away from the grid; M = 18432, 4608 untuned
  (2, 128), (32, 32)   the tuned entries' M (32768, 8192, 2048, 512) made of another (B, H)

Every list of test_igemm_shapes_gpu.py runs here through that file's helpers: same references (torch on the CPU, fp32 / fp64 on
storage-rounded operands), same bounds, the shapes scaled by L / 64 (tests/test_shape_lists_cpu.py checks that scaling against
the oracle's layer walk at L = 24 and L = 8).  Where an operator documents that it declines a shape, the test asserts the return
code and records nothing; the closing proof then requires that whatever the forward launches instead was compared here.
"""
import ctypes as C

import pytest
import torch

import test_igemm_shapes_gpu as G
from test_igemm_shapes_gpu import ATTN_LEVELS, BF16, F32, GN_SHAPES, LN_SHAPES, MODES, SHAPES, XT_SHAPES, P, bf16_round, dev, recorded
from test_igemm_shapes_gpu import L  # noqa: F401  (the module-scoped library fixture, with its leaked-switch checks)

pytestmark = pytest.mark.gpu

OFFGRID = [(1, 8), (3, 24), (2, 40), (5, 40), (3, 72), (2, 96), (2, 128), (32, 32)]
OFF_IDS = [f"b{b}l{l}" for b, l in OFFGRID]
SEEN = {(c, m): set() for c in OFFGRID for m in MODES}


# ---- the documented shape rules of the operators that may decline (csrc/kernels.h)
def entry_fused_ok(cfg):        # proj_qkv_fused_ok: whole 128-row tiles
    return (cfg[0] * cfg[1] * cfg[1]) % 128 == 0


def entry_gn_fold_ok(cfg):      # proj_qkv_gn_fold_ok: every image is whole 128-row tiles
    return entry_fused_ok(cfg) and (cfg[1] * cfg[1]) % 128 == 0


def tail_ok(cfg):               # conv_out_tail_ok: 8 x 16 pixel tiles
    return cfg[1] % 16 == 0


def fp8_level(cfg):             # the engine's rule for a handle with set_attention_fp8(): N >= 4096 on whole 128-key tiles
    n = cfg[1] * cfg[1]
    return n >= 4096 and n % 128 == 0


def test_offgrid_rules_are_exercised():
    """the configuration list puts each rule on both sides (a list edited later cannot quietly stop doing so)"""
    for rule in (entry_fused_ok, entry_gn_fold_ok, tail_ok, fp8_level):
        assert {rule(c) for c in OFFGRID} == {True, False}, rule.__name__
    assert any(entry_fused_ok(c) and not entry_gn_fold_ok(c) for c in OFFGRID)
    assert any(c[1] * c[1] >= 4096 and not fp8_level(c) for c in OFFGRID)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
@pytest.mark.parametrize("case", SHAPES)
def test_offgrid_layer_shape_vs_oracle(L, dt, cfg, case):
    G.check_layer_shape(L, SEEN, dt, cfg, case)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
@pytest.mark.parametrize("M,K,N,geglu", LN_SHAPES)
def test_offgrid_layernorm_folded_gemm_vs_oracle(L, dt, cfg, M, K, N, geglu):
    """(includes what only a ragged bf16 forward launches on the 320-channel level: the row statistics and the q|k|v GEMM with the
    LayerNorm fold at K = 320, which the fused entry kernel replaces wherever M % 128 == 0)"""
    G.check_layernorm_folded_gemm(L, SEEN, dt, cfg, M, K, N, geglu)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
def test_offgrid_conv_out_vs_oracle(L, dt, cfg):
    """conv_out as the GEMM and, where the step tail has the shape, as the tail kernel; elsewhere the tail operator returns -2"""
    G.check_conv_out_shape(L, SEEN, dt, cfg, tail=tail_ok(cfg))
    if dt == BF16 and not tail_ok(cfg):
        B, lat = cfg
        x = torch.zeros(B, 320, lat, lat, device="cuda")
        w = torch.zeros(4, 320, 3, 3, device="cuda")
        b = torch.zeros(4, device="cuda")
        out = torch.full((B, 4, lat, lat), 7.0, device="cuda")
        r = L.lib().ldmseg_op_conv_out_tail(P(x), P(w), P(b), B, lat, lat, P(out), 0, 0, None, 0, 0, 1.0, None, None, None, None, None,
                                            None, 0.0, 0.0, None, None)
        torch.cuda.synchronize()
        assert r == -2 and bool((out == 7.0).all()), r


@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
@pytest.mark.parametrize("case", XT_SHAPES)
def test_offgrid_resnet_tail_one_launch_vs_oracle(L, cfg, case):
    """(igemm_xt_ok does not look at the row count: the extra-tap launch takes every one of these shapes)"""
    G.check_resnet_tail_one_launch(L, SEEN, cfg, case)


@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
def test_offgrid_fused_feed_forward(L, cfg):
    """(mlp_fused_ok has no row-count rule: the kernel masks its own last tile)"""
    G.check_fused_feed_forward(L, SEEN, cfg)


def _entry_call(L, cfg, with_gn):
    """the fused entry operator (mode 1; with_gn: GroupNorm folded in) on this configuration's rows; returns its code and outputs"""
    from test_ops_gpu import _tin_case
    B, lat = cfg
    M = B * lat * lat
    case = [dev(t) for t in _tin_case(M, 320, 11 + M)]
    h = torch.full((M, 320), 7.0, device="cuda")
    qkv = torch.full((M, 960), 7.0, device="cuda")
    us = C.c_float(0)
    if with_gn:
        gg, gb = torch.ones(320, device="cuda"), torch.zeros(320, device="cuda")
        r = L.lib().ldmseg_op_gn_transformer_in(P(case[0]), P(gg), P(gb), 1e-6, B, 1, *[P(t) for t in case[1:]], M, 320, 1e-5, BF16, 1,
                                                P(h), P(qkv), 0, C.byref(us), None)
    else:
        r = L.lib().ldmseg_op_transformer_in(*[P(t) for t in case], M, 320, 1e-5, BF16, 1, P(h), P(qkv), 0, C.byref(us), None)
    torch.cuda.synchronize()
    return r, h, qkv


@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
def test_offgrid_fused_transformer_entry(L, cfg):
    """proj_in -> LayerNorm_1 -> q|k|v in one launch where M % 128 == 0; elsewhere the operator returns -2, writes nothing, and the
    forward runs proj_in, the row statistics and the LayerNorm-folded q|k|v GEMM (SHAPES / LN_SHAPES above) instead"""
    if entry_fused_ok(cfg):
        return G.check_fused_transformer_entry(L, SEEN, cfg)
    with recorded(L, SEEN, cfg):                    # (records into no mode: only reads the log)
        r, h, qkv = _entry_call(L, cfg, False)
    assert r == -2 and bool((h == 7.0).all()) and bool((qkv == 7.0).all()), r


@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
def test_offgrid_fused_transformer_entry_with_groupnorm(L, cfg):
    """the same with the transformer's GroupNorm folded in, where every image is whole 128-row tiles; elsewhere -2 and the forward
    runs the 320-channel GroupNorm as a launch of its own (GN_SHAPES, eps 1e-6)"""
    if entry_gn_fold_ok(cfg):
        return G.check_fused_transformer_entry_with_groupnorm(L, SEEN, cfg)
    with recorded(L, SEEN, cfg):
        r, h, qkv = _entry_call(L, cfg, True)
    assert r == -2 and bool((h == 7.0).all()) and bool((qkv == 7.0).all()), r


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
@pytest.mark.parametrize("case", GN_SHAPES)
def test_offgrid_groupnorm_shape_vs_oracle(L, dt, cfg, case):
    G.check_groupnorm_shape(L, SEEN, dt, cfg, case)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
def test_offgrid_conv_groupnorm_fused_finish(L, dt, cfg):
    """every resnet conv1 -> norm2 shape the engine K-slices and has a finish-GroupNorm instantiation for (the operator returns -4
    for the others, and a configuration may have none: conv and norm then run apart, as SHAPES and GN_SHAPES compare them)"""
    fused = G.check_conv_groupnorm_fused_finish(L, SEEN, dt, cfg)
    print(f"{cfg} dt {dt}: {fused} conv -> GroupNorm shapes on the fused finish")


@pytest.mark.parametrize("mode", ["bf16", "fp32", "bf16x3"])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
@pytest.mark.parametrize("level", ATTN_LEVELS)
def test_offgrid_attention_level_vs_oracle(L, mode, cfg, level):
    """(below 512 tokens the reference covers every query row)"""
    side, Cc = level
    N = (side * cfg[1] // 64) ** 2
    if N < 512:
        assert G.attention_rows(None, cfg[0], N, Cc) == list(range(N))
    G.check_attention_level(L, SEEN, mode, cfg, level)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_offgrid_single_token_attention_is_v(L, mode):
    """the 1x1 map of L = 8: softmax over one key is 1, so the output is v itself - exactly (bf16: of the rounded input)"""
    cfg, Cc, N = (1, 8), 1280, 1
    for B in (1, 3):
        qkv = G._attn_case(B, N, Cc, 5 + B)
        if mode == "bf16":
            qkv = bf16_round(qkv)
        out = torch.empty(B, N, Cc, device="cuda")
        dq = dev(qkv)
        with recorded(L, SEEN, cfg, *((mode,) if B == 1 else ())):
            assert L.lib().ldmseg_op_attention(P(dq), B, N, Cc, 8, G.ATTN_DT[mode], P(out), None) == 0, L.lib().ldmseg_last_error()
        assert torch.equal(out.cpu(), qkv[:, :, 2 * Cc:]), (mode, B)


@pytest.mark.parametrize("cfg", [c for c in OFFGRID if fp8_level(c)], ids=[i for c, i in zip(OFFGRID, OFF_IDS) if fp8_level(c)])
def test_offgrid_attention_fp8_level_vs_oracle(L, cfg):
    """only where the engine itself takes the fp8 path (fp8_level): the operator accepts ragged N, the engine sends it none"""
    G.check_attention_fp8_level(L, SEEN, cfg)


@pytest.mark.parametrize("mode,dt", [("bf16", BF16), ("fp32", F32), ("bf16x3", G.X3W), ("bf16fp8", BF16)])
@pytest.mark.parametrize("cfg", OFFGRID, ids=OFF_IDS)
def test_every_offgrid_forward_instantiation_is_oracle_tested(L, unet_sd, cfg, mode, dt):
    """the closing proof of test_igemm_shapes_gpu.py at the off-grid configurations: every kernel a forward launches there is one
    the tests above compared with the oracle at that configuration's shapes.  A bf16 forward with set_attention_fp8() launches an
    fp8 attention kernel exactly where fp8_level holds ((3, 72): 5184 tokens, not whole key tiles, stays on the bf16 kernel).  The
    per-op tests must have recorded something of each family, so a configuration they all declined cannot pass."""
    tested = SEEN[(cfg, mode)] | (SEEN[(cfg, "bf16")] if mode == "bf16fp8" else set())
    assert any(n.startswith("igemm<") for n in tested), (cfg, mode)
    assert any(n.startswith(G.GN_FAMILY) for n in tested), (cfg, mode)
    assert any(n.startswith(G.ATTN_FAMILY) for n in tested), (cfg, mode)
    used = G.check_every_forward_instantiation(L, SEEN, unet_sd, cfg, mode, dt, fp8_level=fp8_level(cfg))
    print(f"{cfg} {mode} launched: {sorted(used)}")

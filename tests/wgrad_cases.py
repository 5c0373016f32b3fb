"""The shapes the by-width weight-gradient kernels (csrc/vae_bwd.hip) are run at by the operator tests, as data: no GPU
and no library here.  tests/test_wgrad_kernels_gpu.py runs them, tests/test_vae_encode_backward_ops_gpu.py runs NARROW and STRIDE2,
and tests/test_wgrad_plan_ex_cpu.py holds that together with the two encoder configurations they reach every kernel the chooser can
name.

A launch is (B, Ci, Co, H, W, stride) of ldmseg_op_conv_wgrad_ex: x [B,Ci,H,W], dy on the conv's output map."""

# ---- tests/test_vae_encode_backward_ops_gpu.py
# (B, Ci, Co, H, W): tiles 32 x 32, 64 x 64 and 32 x 32 with 7 real input channels (25 padded channels that never reach dW);
# maps 16^2, 24^2 and the odd 5 x 7: a partial pixel step, borders a large share
NARROW = [(1, 32, 32, 16, 16), (2, 32, 32, 24, 24), (3, 32, 32, 5, 7), (2, 64, 64, 16, 16), (1, 64, 64, 24, 24), (3, 64, 64, 5, 7),
          (2, 7, 32, 16, 16), (1, 7, 32, 24, 24), (3, 7, 32, 5, 7)]
# 32 -> 64 runs on the all-taps tile (64 x 32), the wider ones on one tile per tap; 7 -> 64 on the odd map: all-taps with the bottom
# and right padding taps
STRIDE2 = [(2, 32, 64, 16, 16), (3, 7, 64, 5, 7), (2, 64, 128, 12, 12), (2, 128, 256, 6, 6), (3, 128, 256, 5, 7)]

# ---- tests/test_wgrad_kernels_gpu.py
# (Ci, Co, stride): the eight kernels no configuration reaches, widths that leave a 128 tile three quarters full (C = 96, N = 96),
# two tiles per axis the second of which is 32 wide (160), and 6 x 5 x 9 = 270 tiles: more items than an MI355X has CUs
ODD = (3, 5, 7)                    # (B, H, W): odd, not square, a partial 32-pixel step, images that differ; stride 2: 3 x 4 out
BIG = (672, 544, 1)                # runs on ODD only
WIDTHS = [(20, 48, 1),             # wgrad9<64,32>: 48 real of 64 rows, 20 real of 32 channels
          (40, 24, 2),             # wgrad9<32,64>/s2
          (96, 64, 1), (96, 64, 2),            # wgrad<64,128>[/s2], C = 96
          (32, 96, 1), (32, 96, 2),            # wgrad<128,32>[/s2], N = 96
          (64, 128, 1),            # wgrad<128,64>
          (128, 32, 2),            # wgrad<32,128>/s2
          (160, 160, 1), (160, 160, 2),        # wgrad<128,128>[/s2], 2 x 2 tiles
          BIG]                     # wgrad<128,128>, the item walk at 256 CUs
# the widths that, with WIDTHS, give every one of the 18 kernel names a multi-slice launch (the item-walk test): the two existing
# narrow layers and the six names WIDTHS reaches at one stride only
WALK_MORE = [(32, 32, 1), (64, 64, 1), (32, 32, 2), (32, 64, 2), (64, 64, 2), (64, 32, 1), (64, 128, 2), (128, 32, 1)]


def multi_slice_map(stride):
    """(B, H, W) whose OUTPUT map holds 2 x 24 x 24 = 1152 pixels: 36 steps, cut into four slices"""
    return (2, 24, 24) if stride == 1 else (2, 48, 48)


def launches():
    """every launch of test_wgrad_kernels_gpu.py's oracle test: (B, Ci, Co, H, W, stride)"""
    out = []
    for Ci, Co, stride in WIDTHS:
        out.append(ODD[:1] + (Ci, Co) + ODD[1:] + (stride,))
        if (Ci, Co, stride) != BIG:
            B, H, W = multi_slice_map(stride)
            out.append((B, Ci, Co, H, W, stride))
    return out


def walk_launches():
    """one multi-slice launch per kernel name"""
    out = []
    for Ci, Co, stride in [w for w in WIDTHS if w != BIG] + WALK_MORE:
        B, H, W = multi_slice_map(stride)
        out.append((B, Ci, Co, H, W, stride))
    return out


def storage(c):
    return (c + 31) // 32 * 32


def out_side(h, stride):
    return (h - 1) // 2 + 1 if stride == 2 else h


def desc(B, Ci, Co, H, W, stride):
    """(P of the OUTPUT map, N, C, taps, stride) of the launch, storage widths: the arguments of ldmseg_op_wgrad_plan_ex"""
    return B * out_side(H, stride) * out_side(W, stride), storage(Co), storage(Ci), 9, stride


def ident(s):
    return "x".join(map(str, s))

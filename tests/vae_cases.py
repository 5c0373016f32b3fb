"""The launch lists of csrc/vae.hip as pure functions of (B, H[, W]): what the seg-VAE (encode, decode per tail, reconstruct) and the
image-VAE encoder launch, in launch order.  No GPU and no library: tests/test_vae_shape_lists_cpu.py checks the lists against the
layer walk of oracle/vae.py and oracle/vae_image.py, tests/test_vae_shapes_gpu.py launches every entry through the operators of
csrc/ops_api.hip and compares it with the torch-CPU op.

An entry is a namedtuple; maps are (H, W) of the launch's INPUT.  `tile` on a conv: the layer stores its output channels rounded up
to the K tile of the compute dtype (64 bf16 / 32 fp32) as explicit zeros (conv_shape n_store) - the seg-VAE encoder's 32-channel
level and the image VAE's conv_out; the operator dtype decides the number, so the list only carries the flag."""
from collections import namedtuple

Conv = namedtuple("Conv", "B Ci Co k stride pad silu resid epi H W tile")            # pad -1 = k // 2; epi "store" | "nchw_f32"
ConvT = namedtuple("ConvT", "B Ci Co H W")                                             # ConvTranspose2d k 2 s 2 (EPI_CONVT2, N = 4 Co)
GroupNorm = namedtuple("GroupNorm", "B C HW eps silu")
LayerNorm = namedtuple("LayerNorm", "M C eps silu inplace")
Gemm = namedtuple("Gemm", "M N K rows_f32 bias")                                        # activation x activation (w_dynamic)
Softmax = namedtuple("Softmax", "rows n scale")
Posterior = namedtuple("Posterior", "B HW noise")
Bilinear = namedtuple("Bilinear", "B C H W")                                             # x2 -> fp32 NCHW
BilinearArgmax = namedtuple("BilinearArgmax", "B C H W")
Pack = namedtuple("Pack", "B C HW")                                                      # fp32 NCHW -> NHWC (outside the dispatch log)
PostprocTail = namedtuple("PostprocTail", "kind B C H W")                                # postproc.hip tails (outside the dispatch log)

SEG = dict(in_channels=7, int_channels=256, out_channels=128, block_out_channels=(32, 64, 128, 256), latent_channels=4,
           num_upscalers=2, upscale_channels=256)
KL_CH = (128, 256, 512, 512)
DECODE_TAILS = ("logits", "logits_x2", "argmax", "panoptic", "semseg")
RECONSTRUCT_TAILS = ("panoptic", "semseg")

# (B, H, W) the GPU tests run
SEG_CONFIGS = [(2, 64, 64), (1, 40, 40)]                     # the second: maps 40 / 20 / 10 / 5, off the power-of-two grid
IMG_CONFIGS = [(1, 64, 64), (2, 128, 64), (1, 64, 192)]      # 64, 128 and 192 tokens (the last no multiple of 128)
# the workload: a 512 x 512 image
SEG_WORKLOAD = (1, 512, 512)
IMG_WORKLOAD = (1, 512, 512)


def conv(B, Ci, Co, H, W, k=3, stride=1, pad=-1, silu=0, resid=0, epi="store", tile=0):
    return Conv(B, Ci, Co, k, stride, pad, silu, resid, epi, H, W, tile)


def conv_out_hw(c):
    if c.k == 3 and c.stride == 2:
        return (c.H // 2, c.W // 2) if c.pad == 0 else ((c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1)
    return c.H, c.W


def seg_encode(B, H, W=None):
    """ldmseg_vae_encode (vae_encode_body: vae_trunk over encoder_rows, then the head conv): square maps only (W is accepted for symmetry and must equal H)"""
    assert W in (None, H) and H % 8 == 0
    c = SEG
    boc = c["block_out_channels"]
    out = [Pack(B, c["in_channels"], H * H), conv(B, c["in_channels"], boc[0], H, H, silu=1, tile=1)]
    h = H
    for i in range(3):
        out.append(conv(B, boc[i], boc[i], h, h, tile=1))
        out.append(conv(B, boc[i], boc[i + 1], h, h, stride=2, silu=1, tile=1))
        h = (h - 1) // 2 + 1
    out.append(conv(B, boc[3], c["int_channels"], h, h))
    out.append(GroupNorm(B, c["int_channels"], h * h, 1e-6, 1))
    out.append(conv(B, c["int_channels"], 2 * c["latent_channels"], h, h, epi="nchw_f32"))
    return out


def seg_decode(B, L, tail):
    """ldmseg_vae_decode* (vae_decode_body: vae_trunk over decoder_rows, the head conv, the tail) on [B, 4, L, L] latents"""
    assert tail in DECODE_TAILS
    c = SEG
    out = [Pack(B, c["latent_channels"], L * L), conv(B, c["latent_channels"], c["int_channels"], L, L)]
    h, cin = L, c["int_channels"]
    for _ in range(c["num_upscalers"]):
        out.append(ConvT(B, cin, c["upscale_channels"], h, h))
        h, cin = 2 * h, c["upscale_channels"]
        out.append(LayerNorm(B * h * h, cin, 1e-6, 1, 1))
    out.append(GroupNorm(B, cin, h * h, 1e-5, 1))
    Co = c["out_channels"]
    out.append(conv(B, cin, Co, h, h, epi="nchw_f32" if tail == "logits" else "store"))
    if tail == "logits_x2":
        out.append(Bilinear(B, Co, h, h))
    elif tail == "argmax":
        out.append(BilinearArgmax(B, Co, h, h))
    elif tail != "logits":
        out.append(PostprocTail(tail, B, Co, h, h))
    return out


def seg_reconstruct(B, H, tail):
    """ldmseg_vae_reconstruct_* (vae_reconstruct): encode -> posterior mode -> decode -> the tail"""
    assert tail in RECONSTRUCT_TAILS
    l = H // 8
    return seg_encode(B, H) + [Posterior(B, l * l, 0)] + seg_decode(B, l, tail)


def _resnet(B, cin, cout, H, W):
    out = [GroupNorm(B, cin, H * W, 1e-6, 1), conv(B, cin, cout, H, W), GroupNorm(B, cout, H * W, 1e-6, 1)]
    if cin != cout:
        out.append(conv(B, cin, cout, H, W, k=1))
    out.append(conv(B, cout, cout, H, W, resid=1))
    return out


def img_encode(B, H, W):
    """ldmseg_vae_image_encode (klenc_encode_impl); the attention's three GEMMs and its softmax run once per image"""
    assert H % 8 == 0 and W % 8 == 0 and (H // 8) * (W // 8) % 64 == 0
    out = [Pack(B, 3, H * W), conv(B, 3, KL_CH[0], H, W)]
    cin, h, w = KL_CH[0], H, W
    for i in range(4):
        for _ in range(2):
            out += _resnet(B, cin, KL_CH[i], h, w)
            cin = KL_CH[i]
        if i < 3:
            out.append(conv(B, cin, cin, h, w, stride=2, pad=0))
            h, w = h // 2, w // 2
    C, N = 512, h * w
    out += _resnet(B, C, C, h, w)
    out += [GroupNorm(B, C, N, 1e-6, 0), conv(B, C, C, h, w, k=1), conv(B, C, C, h, w, k=1)]
    for _ in range(B):
        out += [Gemm(N, N, C, 1, 0), Softmax(N, N, C ** -0.5), Gemm(C, N, C, 0, 0), Gemm(N, C, N, 0, 1)]
    out.append(conv(B, C, C, h, w, k=1, resid=1))
    out += _resnet(B, C, C, h, w)
    out.append(GroupNorm(B, C, N, 1e-6, 1))
    out.append(conv(B, C, 8, h, w, tile=1))
    out.append(conv(B, 8, 8, h, w, k=1, epi="nchw_f32"))
    return out


def seg_lists(B, H, W=None):
    """{entry name: launch list} of every seg-VAE entry at one configuration"""
    d = {"encode": seg_encode(B, H)}
    for t in DECODE_TAILS:
        d["decode_" + t] = seg_decode(B, H // 8, t)
    for t in RECONSTRUCT_TAILS:
        d["reconstruct_" + t] = seg_reconstruct(B, H, t)
    return d


def img_lists(B, H, W):
    return {"encode": img_encode(B, H, W)}


def distinct(lists):
    """the distinct entries of {name: list}, in first-seen order"""
    seen, out = set(), []
    for lst in lists.values():
        for e in lst:
            if (type(e), e) not in seen:          # (namedtuples of different types with equal fields compare equal)
                seen.add((type(e), e))
                out.append(e)
    return out


# ---- the launch description ldmseg_op_igemm_plan takes, per GEMM entry and operator dtype (tests/igemm_desc.py FIELDS order)
EPI = {"store": 0, "nchw_f32": 2}
EPI_CONVT2, EPI_ROWS_F32 = 3, 4
F32, BF16, X3, X3W = 0, 1, 2, 3


def k_tile(dt):
    return 64 if dt == BF16 else 32


def n_store(c, dt):
    """storage channel count of a conv's output: the real count, or rounded up to the K tile where the layer does that"""
    from igemm_desc import rup
    return rup(c.Co, k_tile(dt)) if c.tile else c.Co


def igemm_desc(e, dt):
    """17-int description of the igemm launch behind a Conv / ConvT / Gemm entry in operator dtype dt (0 fp32, 1 bf16, 3 bf16x3);
    an activation x activation GEMM of the bf16x3 mode splits both operands in the K loop (x3 = 1: operator dtype 2)"""
    from igemm_desc import make_desc, pick_bn, rup
    a = k_tile(dt)
    if isinstance(e, Conv):
        ns = n_store(e, dt)
        Ho, Wo = conv_out_hw(e)
        return make_desc(M=e.B * Ho * Wo, N=rup(ns, pick_bn(ns, 0)), C0=rup(e.Ci, a), taps=e.k * e.k, stride=e.stride, epi=EPI[e.epi],
                         region=1), dt
    if isinstance(e, ConvT):
        return make_desc(M=e.B * e.H * e.W, N=rup(4 * e.Co, pick_bn(4 * e.Co, 0)), C0=e.Ci, epi=EPI_CONVT2, region=1), dt
    if isinstance(e, Gemm):
        return make_desc(M=e.M, N=e.N, C0=e.K, epi=EPI_ROWS_F32 if e.rows_f32 else 0, region=1), (X3 if dt == X3W else dt)
    raise TypeError(e)


# ---- cases beyond the configurations' own lists: instantiations the workload (a 512 x 512 image, B = 1) plans that no list entry
# at SEG_CONFIGS / IMG_CONFIGS plans.  tests/test_vae_shape_lists_cpu.py::test_workload_instantiations_are_planned_by_a_gpu_case
# fails while one is missing; each case says whether a smaller shape reaches the instantiation or only the workload's own does.
# Every one below is the cheapest shape (fewest multiply-adds, over B x side for the convs and the token count for the GEMMs) of a
# workload entry's own form that plans the instantiation: a smaller shape reaches each, none needs the workload's own size.
EXTRA_CASES = [
    # 128 x 128 tiles, 8 waves, pipelined (bf16 and fp32): the first transposed conv at 64 x 64 -> more batch on a 32 x 32 map
    ConvT(3, 256, 256, 32, 32),
    # 256 x 128 tiles, 8 waves (bf16 / fp32 pipelined, bf16x3 plain loop): conv_in of the image VAE at 512 x 512 -> 248 x 248 is the
    # smallest map with 240 row tiles
    conv(1, 3, 128, 248, 248),
    # 256 x 128 tiles with loader waves (bf16, K slices of >= 24 tiles): the logits head at 256 x 256 -> 248 x 248
    conv(1, 256, 128, 248, 248, epi="nchw_f32"),
    # 128 x 128 tiles, 4 compute + 4 loader waves (fp32, >= 40 K tiles, one work item per CU): the second downsampler at 256 x 256
    # -> two images at 160 x 160
    conv(2, 256, 256, 160, 160, stride=2, pad=0),
    # the same tile on K slices (fp32): O = P V + b_v at 4096 tokens -> 3264 tokens
    Gemm(3264, 512, 3264, 0, 1),
    # 64 x 128 tiles, two workgroups per CU (bf16x3, weight planes): the first transposed conv at 64 x 64 -> 48 x 48
    ConvT(1, 256, 256, 48, 48),
    # 256 x 128 plain-loop tiles with both operands split in the K loop (bf16x3): S = Q K^T at 4096 tokens -> 2816 tokens
    Gemm(2816, 2816, 512, 1, 0),
    # 64 x 128 tiles on K slices, both operands split (bf16x3): O = P V + b_v at 4096 tokens -> 1280 tokens
    Gemm(1280, 512, 1280, 0, 1),
]


# ---- inputs and fp64 reference of the fused argmax tail, shared by the CPU check of the left-out share and the GPU test
ARGMAX_LEFT_OUT_CAP = 0.01


def argmax_case(B, C, H, W, seed=0):
    """logits [B,C,H,W]: unit normal with a smooth per-class field on top, so neighbouring pixels mostly agree on the class (as
    decoder logits do) while class boundaries - where the two largest interpolated logits cross - still occur"""
    import torch
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(B, C, max(H // 4, 1), max(W // 4, 1), generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return 2.0 * field + torch.randn(B, C, H, W, generator=g)


def argmax_reference(x):
    """fp64 bilinear x2 (align_corners=False) of x as stored -> (ids, max-softmax prob, keep): keep leaves out the pixels whose two
    largest logits lie within the fp32 rounding of the kernel's interpolation of each other - three products and three sums per
    logit, each half an ulp of at most max|x|: 6 * 2^-24 * max|x|, doubled because both logits carry it"""
    import torch
    y = torch.nn.functional.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    top = y.topk(2, dim=1).values
    tol = 2 * 6 * 2.0 ** -24 * float(x.abs().max())
    keep = (top[:, 0] - top[:, 1]) > tol
    return y.argmax(1), torch.softmax(y, 1).amax(1), keep

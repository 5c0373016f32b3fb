"""Per-launch oracle comparison of every kernel the two VAEs launch (csrc/vae.hip), in bf16, fp32 and bf16x3, and the proof that
nothing they launch escapes it.

tests/vae_cases.py holds the launch lists of the seg-VAE (encode, decode per tail, reconstruct) and of the image-VAE encoder as
functions of (B, H, W); tests/test_vae_shape_lists_cpu.py proves them equal to the layer walk of the oracle.  Here every distinct entry
of the lists at every configuration - and the extra cases that reach the instantiations only the 512 x 512 workload plans - is launched
through the operators of csrc/ops_api.hip that fill IgemmParams the way vae.hip does, and compared with the torch-CPU op on inputs
rounded as the kernel stores them (fp64 for the norms, the GEMMs, softmax and the tails; fp32 for the convs, as
test_igemm_shapes_gpu.py does).  Each test records what the dispatch log named; the closing tests run the models' own entry points
with the log on and fail on a name no per-launch test recorded at that configuration and mode.

Bounds (max-norm relative unless said otherwise).  From the suite, for the forms it already has: conv with identical operand rounding
and fp32 output 1e-3 bf16 / 2e-5 fp32 (test_ops_gpu.test_conv2d); the store epilogue 8e-3 bf16 (one bf16 rounding of the output,
2^-9, of a value up to max|ref|, plus the accumulation-order term) / 2e-5 fp32; GroupNorm 8e-3 / 5e-5; LayerNorm 8e-3 / 2e-5
(test_ops_gpu.test_layernorm); split-bf16 products 1e-4 (test_split_bf16_*).  Where a helper of test_igemm_shapes_gpu.py covers the form
it is called, with its bounds.  Derived here, each next to its use: fp32 score rows out of a bf16 GEMM, the softmax rows, the posterior
sample, the argmax tail.
"""
import pytest
import torch
import torch.nn.functional as F

import vae_cases as V
from conftest import rel_err
from test_igemm_shapes_gpu import BF16, F32, X3W, P, bf16_round, check_groupnorm_shape, check_layer_shape, dev, recorded
from test_igemm_shapes_gpu import L  # noqa: F401  (the module-scoped library fixture, with its leaked-switch checks)

pytestmark = pytest.mark.gpu

X3 = 2          # operator dtype 2: both operands split in the K loop (an activation x activation GEMM of the bf16x3 mode)
MODES = ("bf16", "fp32", "bf16x3")
EXTRA = ("extra", None)
KEYS = [("seg", c) for c in V.SEG_CONFIGS] + [("img", c) for c in V.IMG_CONFIGS] + [EXTRA]
SEEN = {(k, m): set() for k in KEYS for m in MODES}

# Kernels the models launch outside the dispatch log, and the test that compares each:
#   pack_concat3_kernel (launch_pack_nchw: fp32 NCHW -> NHWC at the API boundary, with the input's mul / add) - every operator call
#       of this file stages its NCHW input through it; with mul / add: tests/test_path_gpu.py::test_vae_vs_oracle_larger
#   the postproc.hip tails behind the decoder (launch_panoptic_from_decoder, launch_semseg_from_decoder) -
#       tests/test_postprocess_gpu.py::test_fused_tail_resampling_and_postprocess and
#       tests/test_semseg_eval_gpu.py::test_semseg_tail_on_a_given_map
OUTSIDE_THE_LOG = {V.Pack: "tests/test_path_gpu.py::test_vae_vs_oracle_larger",
                   V.PostprocTail: "tests/test_postprocess_gpu.py::test_fused_tail_resampling_and_postprocess, "
                                   "tests/test_semseg_eval_gpu.py::test_semseg_tail_on_a_given_map"}


def entries(kind):
    """[(key, entry)] of one entry type over every configuration's lists and the extra cases, each once per configuration"""
    out = []
    for key in KEYS:
        if key == EXTRA:
            lst = V.EXTRA_CASES
        else:
            lst = V.distinct(V.seg_lists(*key[1]) if key[0] == "seg" else V.img_lists(*key[1]))
        out += [(key, e) for e in lst if type(e) is kind]
    return out


def ident(v):
    if isinstance(v, tuple) and not hasattr(v, "_fields"):
        return v[0] + ("" if v[1] is None else "_b%dh%dw%d" % v[1])
    if hasattr(v, "_fields"):
        return "-".join(str(x) for x in v)
    return None


def test_every_list_entry_has_a_per_launch_test():
    kinds = {type(e) for key in KEYS if key != EXTRA for e in V.distinct(V.seg_lists(*key[1]) if key[0] == "seg" else V.img_lists(*key[1]))}
    assert kinds == {V.Conv, V.ConvT, V.GroupNorm, V.LayerNorm, V.Gemm, V.Softmax, V.Posterior, V.Bilinear, V.BilinearArgmax} | set(OUTSIDE_THE_LOG)


def modes_of(dt):
    return ("bf16",) if dt == BF16 else ("fp32", "bf16x3")


def view(key, cfg):
    """SEEN as the helpers of test_igemm_shapes_gpu.py index it: {(cfg, mode): set}"""
    return {(cfg, m): SEEN[(key, m)] for m in MODES}


def rnd(dt):
    return bf16_round if dt == BF16 else (lambda t: t)


def report(what, e):
    print(f"{what}: {e:.3e}")
    return e


# ------------------------------------------------------------------ convs
def run_conv(L, e, dt, x, w, b, res):
    Ho, Wo = V.conv_out_hw(e)
    out = torch.empty(e.B, e.Co, Ho, Wo, device="cuda")
    dx, dw, db, dres = dev(x), dev(w), dev(b), dev(res)         # (kept alive across the call)
    r = L.lib().ldmseg_op_vae_conv(P(dx), P(dw), P(db), P(dres), e.B, e.Ci, e.H, e.W, e.Co, e.k, e.stride, e.pad, e.silu,
                                   V.EPI[e.epi], V.n_store(e, dt) if e.tile else 0, dt, P(out), None)
    assert r == 0, (r, L.lib().ldmseg_last_error(), e)
    torch.cuda.synchronize()
    return out


def conv_case(e):
    g = torch.Generator().manual_seed(hash(tuple(e[:8]) + tuple(e[9:])) & 0xffff)
    x = torch.randn(e.B, e.Ci, e.H, e.W, generator=g)
    if e.pad == 0:
        # a constant offset: a zero row / column read in the wrong place (top / left instead of bottom / right, or a valid last row
        # taken for padding) moves an edge output by about 3 * sum of three taps' weights ~ 3 * sqrt(3 Ci) / sqrt(9 Ci) = 1.7,
        # a tenth of max|ref| (~ 4.5 sigma of sqrt(1 + 9)) and far above the bound
        x = x + 3.0
    w = torch.randn(e.Co, e.Ci, e.k, e.k, generator=g) / (e.Ci * e.k * e.k) ** 0.5
    b = torch.randn(e.Co, generator=g)
    Ho, Wo = V.conv_out_hw(e)
    res = torch.randn(e.B, e.Co, Ho, Wo, generator=g) if e.resid else None
    return x, w, b, res


def conv_ref(e, x, w, b, res):
    if e.pad == 0:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=e.stride)
    else:
        y = F.conv2d(x, w, b, stride=e.stride, padding=e.k // 2)
    if res is not None:
        y = y + res
    return F.silu(y) if e.silu else y


def check_vae_conv(L, key, dt, e):
    torch.set_num_threads(16)
    if (key != EXTRA and e.H == e.W and e.stride == 1 and not e.silu and not e.tile and e.epi == "store" and e.Ci % 64 == 0):
        # a form check_layer_shape covers (square map, padding k / 2, store epilogue, optional residual; no channel-major packing at
        # these channel counts, so ldmseg_op_igemm fills the launch exactly as Exec::conv does): its references and bounds
        cfg = (e.B, 64)
        check_layer_shape(L, view(key, cfg), dt, cfg, (e.H, e.Ci, 0, e.Co, e.k, 1, 0, 0, e.resid, 0))
        return
    x, w, b, res = conv_case(e)
    r = rnd(dt)
    ref = conv_ref(e, r(x), r(w), b, r(res) if res is not None else None)
    with recorded(L, SEEN, key, *modes_of(dt)[:1]):
        out = run_conv(L, e, dt, x, w, b, res)
    name = L.igemm_last_kernel()
    err = report(f"conv {ident(e)} dt={dt} {name}", rel_err(out, ref))
    if e.epi == "nchw_f32":
        assert err < (1e-3 if dt == BF16 else 2e-5), (e, name, err)        # identical operand rounding, fp32 output
    else:
        assert err < (8e-3 if dt == BF16 else 2e-5), (e, name, err)        # + the bf16 rounding of the stored output
    if dt == F32:
        with recorded(L, SEEN, key, "bf16x3"):
            out3 = run_conv(L, e, X3W, x, w, b, res)
        name3 = L.igemm_last_kernel()
        assert ",x3w>" in name3, name3
        err3 = report(f"conv {ident(e)} x3w {name3}", rel_err(out3, ref))
        assert err3 < 1e-4, (e, name3, err3)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.Conv), ids=ident)
def test_conv_launch_vs_oracle(L, dt, key, e):
    check_vae_conv(L, key, dt, e)


# The pad-0 downsampler beyond the maps the model can reach (H, W multiples of 8 there): odd and even sides, H != W, a partial last
# row tile.  With an odd side the appended zero row / column is never read (output i reads rows 2i .. 2i + 2 <= H - 1): a kernel
# that zeroes the last valid row fails here; with an even side the last output reads the zero row.
DOWN_EDGE = [(1, 128, 13, 18), (2, 128, 16, 11), (1, 256, 7, 7), (1, 64, 10, 24)]


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("B,Cc,H,W", DOWN_EDGE)
def test_pad0_downsampler_edges(L, dt, B, Cc, H, W):
    check_vae_conv(L, EXTRA, dt, V.conv(B, Cc, Cc, H, W, stride=2, pad=0))


# ------------------------------------------------------------------ transposed convs
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.ConvT), ids=ident)
def test_transposed_conv_launch_vs_oracle(L, dt, key, e):
    """EPI_CONVT2 at N = 4 Co = 1024 against F.conv_transpose2d; bounds of test_ops_gpu.test_convt2_and_bilinear"""
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(e.H * 31 + e.B)
    x = torch.randn(e.B, e.Ci, e.H, e.W, generator=g)
    w = torch.randn(e.Ci, e.Co, 2, 2, generator=g) / e.Ci ** 0.5
    b = torch.randn(e.Co, generator=g)
    r = rnd(dt)
    ref = F.conv_transpose2d(r(x), r(w), b, stride=2)
    dx, dw, db = dev(x), dev(w), dev(b)
    for d, mode, bound in ((dt, modes_of(dt)[0], 8e-3 if dt == BF16 else 2e-5),) + (((X3W, "bf16x3", 1e-4),) if dt == F32 else ()):
        out = torch.empty(ref.shape, device="cuda")
        with recorded(L, SEEN, key, mode):
            assert L.lib().ldmseg_op_convt2(P(dx), P(dw), P(db), e.B, e.Ci, e.H, e.W, e.Co, d, P(out), None) == 0
        name = L.igemm_last_kernel()
        assert (",x3w>" in name) == (d == X3W), name
        err = report(f"convt {ident(e)} dt={d} {name}", rel_err(out, ref))
        assert err < bound, (e, name, err)


# ------------------------------------------------------------------ norms
def check_vae_groupnorm(L, key, dt, e):
    """F.group_norm(32 groups) (+ SiLU) in fp64 on the storage-rounded input; bounds of check_groupnorm_shape.  Neighbouring groups
    get means 12 apart (and different spreads): with 4 channels per group one 8-element bf16 vector holds two groups, and a vector
    normalised with the statistics of its first element's group comes out wrong by several standard deviations."""
    torch.set_num_threads(16)
    cpg = e.C // 32
    g = torch.Generator().manual_seed(e.C + e.HW + e.B)
    grp = torch.arange(e.C) // cpg
    mean = 6.0 - 12.0 * (grp % 2).float() + 0.5 * torch.randn(e.C, generator=g)
    std = 0.5 + 1.5 * (grp % 3).float()
    x = torch.randn(e.B, e.C, e.HW, generator=g) * std[None, :, None] + mean[None, :, None]
    x[:, :, : e.HW // 3] += 2.0
    gamma = 1 + 0.1 * torch.randn(e.C, generator=g)
    beta = 0.1 * torch.randn(e.C, generator=g)
    ref = F.group_norm(rnd(dt)(x).double(), 32, gamma.double(), beta.double(), e.eps)
    if e.silu:
        ref = F.silu(ref)
    outs = [torch.empty(e.B, e.C, e.HW, device="cuda") for _ in range(2)]
    dx, dg, db = dev(x), dev(gamma), dev(beta)
    with recorded(L, SEEN, key, *modes_of(dt)):
        for o in outs:
            assert L.lib().ldmseg_op_groupnorm(P(dx), None, P(dg), P(db), e.B, e.C, 0, e.HW, e.eps, e.silu, dt, P(o), None) == 0
    assert torch.isfinite(outs[0]).all()
    err = report(f"groupnorm {ident(e)} dt={dt}", rel_err(outs[0], ref))
    assert err < (8e-3 if dt == BF16 else 5e-5), (e, err)
    assert torch.equal(outs[0], outs[1]), e


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.GroupNorm), ids=ident)
def test_groupnorm_launch_vs_oracle(L, dt, key, e):
    side = int(round(e.HW ** 0.5))
    if side * side == e.HW and e.C // 32 != 4:
        # a square map: the helper of test_igemm_shapes_gpu.py, its inputs and bounds
        cfg = (e.B, 64)
        check_groupnorm_shape(L, view(key, cfg), dt, cfg, (side, e.C, 0, e.eps, e.silu))
    check_vae_groupnorm(L, key, dt, e)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.LayerNorm), ids=ident)
def test_layernorm2d_in_place_vs_oracle(L, dt, key, e):
    """LayerNorm2d + SiLU over the channels of every pixel (NHWC rows), as the decoder runs it behind each transposed conv: in
    place.  fp64 F.layer_norm + SiLU on the storage-rounded rows, bounds of test_ops_gpu.test_layernorm; the in-place launch
    against the out-of-place one bit for bit (a row read after a neighbour's write would differ)."""
    assert e.inplace == 1
    g = torch.Generator().manual_seed(e.M + e.C)
    x = torch.randn(e.M, e.C, generator=g) * 3 + 1
    x[::7] *= 20.0                                           # rows of very different scale
    gamma = 1 + 0.1 * torch.randn(e.C, generator=g)
    beta = 0.1 * torch.randn(e.C, generator=g)
    ref = F.layer_norm(rnd(dt)(x).double(), (e.C,), gamma.double(), beta.double(), e.eps)
    if e.silu:
        ref = F.silu(ref)
    dx, dg, db = dev(x), dev(gamma), dev(beta)
    out = {}
    with recorded(L, SEEN, key, *modes_of(dt)):
        for inplace in (1, 0):
            out[inplace] = torch.empty(e.M, e.C, device="cuda")
            assert L.lib().ldmseg_op_layernorm_io(P(dx), P(dg), P(db), e.M, e.C, e.eps, e.silu, inplace, dt, P(out[inplace]), None) == 0
    torch.cuda.synchronize()
    err = report(f"layernorm {ident(e)} dt={dt}", rel_err(out[1], ref))
    assert err < (8e-3 if dt == BF16 else 2e-5), (e, err)
    assert torch.equal(out[1], out[0]), e


# ------------------------------------------------------------------ the single-head attention of the image VAE
def gemm_case(e):
    """operands of one of the three attention GEMMs, shaped like what the model feeds it"""
    g = torch.Generator().manual_seed(e.M * 7 + e.N * 3 + e.K + e.rows_f32)
    if e.bias:              # O = P V + b_v: rows of P are softmax rows (one dominant entry in some), b = V^T [C][tokens]
        s = torch.randn(e.M, e.K, generator=g) * 3
        s[::5, 3] += 12.0
        a = torch.softmax(s, -1)
        b = torch.randn(e.N, e.K, generator=g)
        bias = torch.randn(e.N, generator=g)
    else:
        a = torch.randn(e.M, e.K, generator=g)
        b = torch.randn(e.N, e.K, generator=g)
        bias = None
        if not e.rows_f32:  # V^T = W_v X^T: a weight matrix on the left
            a = a / e.K ** 0.5
    return a, b, bias


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.Gemm), ids=ident)
def test_attention_gemm_launch_vs_oracle(L, dt, key, e):
    """out = a b^T (+ bias) with an activation as the weight operand (w_dynamic), against the fp64 product of the operands as stored.
    Score rows (EPI_ROWS_F32): both operands rounded identically and the output fp32, i.e. the conv bound 1e-3 bf16 / 2e-5 fp32; the
    store epilogue adds the bf16 rounding of the output: 8e-3.  bf16x3 (operator dtype 2, both operands split in the K loop): 1e-4,
    the bound of test_split_bf16_gemm_vs_fp32_reference."""
    torch.set_num_threads(16)
    a, b, bias = gemm_case(e)
    r = rnd(dt)
    ref = r(a).double() @ r(b).double().t()
    if bias is not None:
        ref = ref + bias.double()
    da, db_, dbias = dev(a), dev(b), dev(bias)
    bound = (1e-3 if e.rows_f32 else 8e-3) if dt == BF16 else 2e-5
    for d, mode, bd in ((dt, modes_of(dt)[0], bound),) + (((X3, "bf16x3", 1e-4),) if dt == F32 else ()):
        out = torch.empty(e.M, e.N, device="cuda")
        with recorded(L, SEEN, key, mode):
            rc = L.lib().ldmseg_op_gemm_dynamic(P(da), P(db_), P(dbias), e.M, e.N, e.K, e.rows_f32, d, P(out), None)
            assert rc == 0, (rc, e)
        name = L.igemm_last_kernel()
        assert (",x3>" in name) == (d == X3), name
        err = report(f"gemm {ident(e)} dt={d} {name}", rel_err(out, ref))
        assert err < bd, (e, name, err)


def softmax_case(rows, n, seed):
    """score rows as S = Q K^T leaves them, before the d^-1/2 scale: spread 60, every fourth row shifted to about +300, every fourth
    to about -300, and in every fourth one entry 300 above the rest (it then holds nearly all the mass: the others are 1e-6 and
    below)"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, n, generator=g) * 60.0
    s[1::4] += 300.0
    s[2::4] -= 300.0
    dom = torch.arange(3, rows, 4)
    s[dom, torch.randint(0, n, (len(dom),), generator=g)] += 300.0
    return s


def check_softmax_rows(L, key, dt, rows, n, scale):
    """torch.softmax(scale * s, -1) in fp64 (scale as the fp32 number the kernel multiplies by), compared ELEMENT-wise relative: a
    max-norm would hide every entry next to a dominant one.
    fp32: the exponent v * scale - m carries three fp32 roundings of numbers up to |v * scale| <= 32 here (3 * 32 * 2^-24 = 5.7e-6 absolute,
    which is the relative error of the exponential), __expf adds the rounding of x * log2(e) (46 * 2^-24 * ln 2 = 1.9e-6) and one ulp;
    the row sum and the division 2^-23: 8e-6 in all -> bound 1e-5 (measured on the MI355X: 2.3e-6 at most).  bf16 adds the rounding
    of the stored probability: round-to-nearest on 8 significant bits is at most 2^-8 / (1 + 2^-8) = 3.891e-3 relative, which with the
    1e-5 above stays under the bound 2^-8 = 3.906e-3 (measured: 3.885e-3)."""
    s = softmax_case(rows, n, rows + n)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    assert float((s * sc).abs().max()) <= 32.0 and float(s.abs().max()) > 300.0
    ref = torch.softmax(s.double() * sc, -1)
    out = torch.empty(rows, n, device="cuda")
    ds = dev(s)
    with recorded(L, SEEN, key, *modes_of(dt)):
        assert L.lib().ldmseg_op_softmax_rows(P(ds), rows, n, sc, dt, P(out), None) == 0
    torch.cuda.synchronize()
    o = out.double().cpu()
    big = ref > 1e-30                       # (bf16 and fp32 share the exponent range; nothing here is below 1e-30 anyway)
    assert bool(big.all())
    err = report(f"softmax {rows}x{n} dt={dt}", float(((o - ref).abs() / ref).max()))
    assert err < (2.0 ** -8 if dt == BF16 else 1e-5), (rows, n, err)
    assert float((o.sum(-1) - 1).abs().max()) < (2.0 ** -8 if dt == BF16 else 1e-5)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.Softmax), ids=ident)
def test_softmax_rows_launch_vs_oracle(L, dt, key, e):
    check_softmax_rows(L, key, dt, e.rows, e.n, e.scale)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("rows,n", [(5, 4), (7, 260), (3, 4096)])
def test_softmax_rows_edges(L, dt, rows, n):
    """a row count that leaves waves of the last block without a row, row lengths of one vector, of a partial last sweep (260 = 256 +
    4) and of the workload (4096 tokens)"""
    check_softmax_rows(L, EXTRA, dt, rows, n, 512 ** -0.5)


# ------------------------------------------------------------------ posterior
def posterior_ref(mom, noise):
    mean, logvar = mom.double().chunk(2, 1)
    std = torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    return mean, std, (mean if noise is None else mean + std * noise.double())


def run_posterior(L, key, mom, noise, B, l):
    out = torch.empty(B, 4, l, l, device="cuda")
    dm, dn = dev(mom), dev(noise)
    with recorded(L, SEEN, key, *MODES):            # fp32 in every compute mode
        assert L.lib().ldmseg_vae_posterior(P(dm), P(dn), 1.0, B, l, P(out), None) == 0
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("key,e", entries(V.Posterior), ids=ident)
def test_posterior_mode_launch_vs_oracle(L, key, e):
    """noise = NULL, what the reconstruct chain launches: the mode of the posterior is its mean, bit for bit, whatever logvar holds"""
    assert not e.noise
    l = int(round(e.HW ** 0.5))
    g = torch.Generator().manual_seed(e.HW)
    mom = torch.randn(e.B, 8, l, l, generator=g) * 3
    mom[:, 4:] = torch.randn(e.B, 4, l, l, generator=g) * 40          # logvar far beyond both clamp bounds
    out = run_posterior(L, key, mom, None, e.B, l)
    assert torch.equal(out, mom[:, :4])


@pytest.mark.parametrize("B,l", [(2, 8), (1, 5), (3, 33)])
def test_posterior_sample_clamps(L, B, l):
    """mean + exp(0.5 clamp(logvar, -30, 20)) noise with logvar from -60 to 50: values inside, on and beyond both bounds.  Half of the
    means are zero, so that the lower bound is visible at all (std = e^-15 = 3e-7 disappears next to a mean of order one).
    Element-wise: |out - ref| <= 4e-6 (|mean| + std |noise|) - the argument 0.5 lv <= 15 times log2(e) rounded to fp32 moves the
    exponential by 22 * 2^-24 * ln 2 = 9e-7 relative, expf itself 2 ulp, product and sum one each: 1.3e-6, times 3 (measured: 1.1e-7)."""
    g = torch.Generator().manual_seed(B * 100 + l)
    mom = torch.randn(B, 8, l, l, generator=g)
    lv = torch.rand(B, 4, l, l, generator=g) * 110 - 60
    flat = lv.view(-1)
    flat[:8] = torch.tensor([-30.0, 20.0, -30.5, 20.5, -29.5, 19.5, -60.0, 50.0])
    mom[:, 4:] = lv
    mom[:, :4][torch.rand(B, 4, l, l, generator=g) < 0.5] = 0.0
    noise = torch.randn(B, 4, l, l, generator=g)
    assert float(lv.min()) < -31 and float(lv.max()) > 21
    mean, std, ref = posterior_ref(mom, noise)
    out = run_posterior(L, EXTRA, mom, noise, B, l).double()
    scale = mean.abs() + std * noise.double().abs()
    err = report(f"posterior B={B} l={l}", float(((out - ref).abs() / scale.clamp_min(1e-300)).max()))
    assert torch.isfinite(out).all() and err < 4e-6, err


# ------------------------------------------------------------------ the tails behind the logits
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.Bilinear), ids=ident)
def test_bilinear2x_launch_vs_oracle(L, dt, key, e):
    """F.interpolate(scale_factor=2, 'bilinear', align_corners=False) of the logits as stored; bound of test_convt2_and_bilinear"""
    x = V.argmax_case(e.B, e.C, e.H, e.W, seed=e.H + 1)
    ref = F.interpolate(rnd(dt)(x).double(), scale_factor=2, mode="bilinear", align_corners=False)
    out = torch.empty(ref.shape, device="cuda")
    dx = dev(x)
    with recorded(L, SEEN, key, *modes_of(dt)):
        assert L.lib().ldmseg_op_bilinear2x(P(dx), e.B, e.C, e.H, e.W, dt, P(out), None) == 0
    torch.cuda.synchronize()
    assert report(f"bilinear {ident(e)} dt={dt}", rel_err(out, ref)) < 1e-5


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("key,e", entries(V.BilinearArgmax), ids=ident)
def test_bilinear_argmax_launch_vs_oracle(L, dt, key, e):
    """the fused argmax tail on given logits against argmax / max-softmax of the fp64 interpolation (vae_cases.argmax_reference).
    Pixels whose two largest reference logits lie within the interpolation's rounding of each other are left out - at most 1 % (the
    CPU suite checks the same inputs against that cap); on every other pixel the id is exact.  Max-softmax probability, relative: the
    exponent v - m carries the interpolation's rounding of both logits (2 * 6 * 2^-24 * max|x| with max|x| < 16: 1.1e-5 absolute =
    relative on exp) plus __expf (4e-6 at |x| <= 32) and the 128-term sum: 2e-5 bound (measured: 8.2e-7).  With mask_th: ids below the threshold become
    ignore_label; pixels whose probability lies within that bound of the threshold are left out too."""
    x = V.argmax_case(e.B, e.C, e.H, e.W, seed=e.H)
    xs = rnd(dt)(x)
    assert float(xs.abs().max()) < 16
    ids_ref, prob_ref, keep = V.argmax_reference(xs)
    left_out = 1.0 - float(keep.double().mean())
    assert left_out <= V.ARGMAX_LEFT_OUT_CAP, left_out
    ids = torch.empty(e.B, 2 * e.H, 2 * e.W, dtype=torch.int64, device="cuda")
    prob = torch.empty(e.B, 2 * e.H, 2 * e.W, device="cuda")
    dx = dev(x)
    with recorded(L, SEEN, key, *modes_of(dt)):
        assert L.lib().ldmseg_op_bilinear2x_argmax(P(dx), e.B, e.C, e.H, e.W, -1.0, 0, dt, P(ids), P(prob), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu()[keep], ids_ref[keep]), (e, int((ids.cpu()[keep] != ids_ref[keep]).sum()))
    perr = report(f"argmax prob {ident(e)} dt={dt} left out {left_out:.2e}",
                  float(((prob.cpu().double() - prob_ref).abs() / prob_ref)[keep].max()))
    assert perr < 2e-5, perr
    # thresholded: the median probability as mask_th, ignore_label 999
    th = float(prob_ref.median())
    ids2 = torch.empty_like(ids)
    assert L.lib().ldmseg_op_bilinear2x_argmax(P(dx), e.B, e.C, e.H, e.W, th, 999, dt, P(ids2), None, None) == 0
    torch.cuda.synchronize()
    th32 = float(torch.tensor(th, dtype=torch.float32))
    sure = keep & ((prob_ref - th32).abs() > 2e-5 * prob_ref)
    want = torch.where(prob_ref < th32, torch.full_like(ids_ref, 999), ids_ref)
    assert float(sure.double().mean()) > 0.98 and torch.equal(ids2.cpu()[sure], want[sure])


# ------------------------------------------------------------------ closing proofs
def logged(L, fn):
    L.igemm_log(L.LOG_ALL)
    try:
        fn()
        torch.cuda.synchronize()
        return L.igemm_log_read()
    finally:
        L.igemm_log(False)


def assert_covered(used, key, mode, what):
    igemm = sorted(n for n in used if n.startswith("igemm<"))
    assert igemm, (what, sorted(used))
    if mode == "bf16x3":
        assert all(",x3w>" in n or ",x3>" in n for n in igemm), igemm
    missing = used - SEEN[(key, mode)]
    print(f"{what} {key} {mode}: {len(used)} names, {len(igemm)} igemm")
    assert not missing, (f"{what} {key} {mode}: kernels without a per-launch oracle test: {sorted(missing)}; "
                         f"tested: {sorted(SEEN[(key, mode)])}")


@pytest.mark.parametrize("mode", MODES)
def test_every_seg_vae_launch_is_oracle_tested(L, vae_sd, mode):
    """encode_moments, decode with each tail and both reconstruct entries at every configuration, with the dispatch log on: every
    name must have been recorded by a per-launch test above at that configuration and in this mode"""
    from ldmseg_amd.models import GeneralVAESeg
    v = GeneralVAESeg(vae_sd, scaling_factor=0.2, device="cuda:0", compute_dtype=mode)
    for B, H, _ in V.SEG_CONFIGS:
        key = ("seg", (B, H, H))
        g = torch.Generator().manual_seed(H)
        x = (torch.rand(B, 7, H, H, generator=g) > 0.5).float().cuda()
        z = torch.randn(B, 4, H // 8, H // 8, generator=g).cuda()
        sizes = [(H - 3, H + 5)] * B
        calls = {
            "encode": lambda: v.encode_moments(x, in_mul=2.0, in_add=-1.0),
            "decode_logits": lambda: v.decode(z, interpolate=False),
            "decode_logits_x2": lambda: v.decode(z, interpolate=True),
            "decode_argmax": lambda: v.decode_argmax(z, return_prob=True),
            "decode_panoptic": lambda: v.decode_panoptic(z, (H, H), sizes, count_th=4),
            "decode_semseg": lambda: v.decode_semseg(z, (H + 1, H - 2)),
            "reconstruct_panoptic": lambda: v.reconstruct_panoptic(x, (H, H), sizes, in_mul=2.0, in_add=-1.0, count_th=4),
            "reconstruct_semseg": lambda: v.reconstruct_semseg(x, (H + 1, H - 2), in_mul=2.0, in_add=-1.0),
        }
        assert set(calls) == set(V.seg_lists(B, H))
        for what, fn in calls.items():
            used = logged(L, fn)
            assert_covered(used, key, mode, what)
            lst = V.seg_lists(B, H)[what]
            assert any(n.startswith("posterior_sample<") for n in used) == any(isinstance(e, V.Posterior) for e in lst), (what, used)
            assert any(n.startswith("bilinear_argmax<") for n in used) == any(isinstance(e, V.BilinearArgmax) for e in lst), (what, used)
            assert any(n.startswith("bilinear2x<") for n in used) == any(isinstance(e, V.Bilinear) for e in lst), (what, used)
            assert any(n.startswith("layernorm<") for n in used) == any(isinstance(e, V.LayerNorm) for e in lst), (what, used)


@pytest.mark.parametrize("mode", MODES)
def test_every_image_vae_launch_is_oracle_tested(L, mode):
    from ldmseg_amd import weights
    from ldmseg_amd.models import GeneralVAEImage
    sd = weights.generate(weights.vae_image_schema(), seed=11, norm_keys=weights.VAE_IMAGE_NORM_KEYS)
    v = GeneralVAEImage(sd, scaling_factor=0.18215, device="cuda:0", compute_dtype=mode)
    for B, H, W in V.IMG_CONFIGS:
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
        out = {}
        used = logged(L, lambda: out.setdefault("m", v.encode_moments(x, in_mul=2.0, in_add=-1.0)))
        assert torch.isfinite(out["m"]).all() and out["m"].shape == (B, 8, H // 8, W // 8)
        assert any(n.startswith("softmax_rows<") for n in used) and any(n.startswith("gn_") for n in used), sorted(used)
        assert_covered(used, ("img", (B, H, W)), mode, "encode")

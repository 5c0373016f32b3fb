"""How each operator of csrc/ops_api.hip turns its arguments into the launch description ``ldmseg_op_igemm_plan`` takes, and the
call itself: shared by tests/test_igemm_plan_cpu.py and tests/test_ops_gpu.py::test_igemm_plan_equals_launch."""
import ctypes as C

FIELDS = ("M", "N", "C0", "C1", "C2", "C3", "taps", "stride", "up", "up4", "cm", "epi", "lnf", "x3", "splits", "no_finish", "region")
F32, BF16, X3W = 0, 1, 3
DEFAULT_POLICY = 61


def rup(a, b):
    return (a + b - 1) // b * b


def pick_bn(n, geglu):       # igemm_pick_bn: the N tile weights are padded to
    return 128 if geglu else 160 if n % 160 == 0 else 128 if n >= 128 else 64 if n > 32 else 32


def make_desc(**kw):
    d = dict.fromkeys(FIELDS, 0)
    d.update({"taps": 1, "stride": 1, **kw})
    return [d[f] for f in FIELDS]


def desc_igemm(B, Ci, Ci2, H, W, Co, k, stride, up, geglu, splits, dt, knobs=None, extras=False):
    """ldmseg_op_igemm.  knobs: {debug key: value} where not shipped (the K order and the phase-conv form depend on them);
    extras: a residual, a bias row or SiLU is given (an upsampler conv then keeps its nine taps)"""
    kn = {1: DEFAULT_POLICY << 8, 5: -1, 9: -1, 21: 1, **(knobs or {})}
    a = 64 if dt == BF16 else 32
    c0, c1 = rup(Ci, a), rup(Ci2, a) if Ci2 else 0
    Np = rup(Co, pick_bn(Co, geglu))
    Hl, Wl = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = ((Hl - 1) // 2 + 1, (Wl - 1) // 2 + 1) if k == 3 and stride == 2 else (Hl, Wl)
    cm = (not geglu and k == 3 and stride == 1 and not up and kn[9] != 0 and dt == BF16 and Np % 160 == 0 and
          (kn[9] == 1 or (H * W >= 4096 and c0 + c1 >= 640)) and Ci % a == 0 and Ci2 % a == 0)
    stock = kn[1] >> 8 == DEFAULT_POLICY and kn[5] < 0
    if (up and k == 3 and stride == 1 and not Ci2 and not geglu and not extras and kn[21] and dt == BF16 and c0 % 64 == 0 and Np % 160 == 0 and
            (B * H * W) % 256 == 0 and stock and Ci == c0):
        return make_desc(M=4 * B * H * W, N=Np, C0=c0, taps=4, up4=1, splits=splits, region=1)
    return make_desc(M=B * Ho * Wo, N=Np, C0=c0, C1=c1, taps=k * k, stride=stride, up=up, cm=int(cm), epi=int(geglu), splits=splits, region=1)


def desc_ln_linear(M, K, N, geglu):
    """ldmseg_op_ln_linear / _silu: non-GEGLU N padded to the 160-column tile of the folded instantiations"""
    Np = rup(N, 160 if not geglu and N % 160 else pick_bn(N, geglu))
    return make_desc(M=M, N=Np, C0=K, epi=int(geglu), lnf=1)


def desc_conv3x3_plus_1x1(B, Cc, Cs, Cs2, H, W, Co, splits):
    return make_desc(M=B * H * W, N=rup(Co, pick_bn(Co, 0)), C0=Cc, C2=Cs, C3=Cs2, taps=9, splits=splits, region=1)


def desc_conv_groupnorm(B, Ci, H, W, Co, splits):
    return make_desc(M=B * H * W, N=rup(Co, pick_bn(Co, 0)), C0=Ci, taps=9, splits=splits, no_finish=1)


def plan(lib, desc, dtype, cus):
    """(return code, string) of ldmseg_op_igemm_plan"""
    buf = C.create_string_buffer(128)
    r = lib.ldmseg_op_igemm_plan((C.c_int * len(FIELDS))(*desc), dtype, cus, buf, 128)
    return r, buf.value.decode()

"""The attention launches whose dispatch tools/record_attn_dispatch.py records (tests/golden/attn_dispatch.json) and that
tests/test_attn_plan_cpu.py replays through ldmseg_op_attention_plan, the cases whose output bytes
tests/test_ops_gpu.py::test_attention_plan_equals_launch pins, and the closed-form inputs both sides build (gn_cases.hashed: no
library RNG, the same bytes on any machine)."""
import ctypes as C
import hashlib

from gn_cases import hashed

F32, BF16, X3 = 0, 1, 2
SELF, CAUSAL, FP8, CROSS = 0, 1, 2, 3                # AttnDesc::kind (csrc/attn_plan.h)
ATTN_FAMILY = ("attn", "kv_to_", "attention_cross_kernel<")
KEY2 = tuple(range(16))                              # debug key 2: every value the rule lists (1..14) and one to either side
KEY15 = (1, 0, 0x101, 0x111, 0x121, 0x131)           # debug key 15: shipped, scaled MFMAs off, and the four forms of the mx kernel
KEYS = {2: 0, 15: 1}                                 # shipped values (the getter of key 15 answers 0x31 for the shipped 1)
CONFIGS = [(8, 64), (16, 64), (4, 128)]              # = tests/test_igemm_shapes_gpu.py
OFFGRID = [(1, 8), (3, 24), (2, 40), (5, 40), (3, 72), (2, 96), (2, 128), (32, 32)]     # = tests/test_offgrid_shapes_gpu.py
ATTN_LEVELS = [(64, 320), (32, 640), (16, 1280), (8, 1280)]      # (map side at L = 64, C), 8 heads
# (B, N, C) at 8 heads of the self-attention tests of tests/test_ops_gpu.py (fp8 ones: OPS_FP8) and the single-token test of the
# off-grid suite
OPS_SELF = [(1, 256, 320), (2, 64, 320), (1, 1024, 320), (1, 256, 640), (2, 4, 1280), (1, 64, 1280), (1, 100, 640), (1, 320, 1280),
            (1, 4096, 320), (2, 1024, 320), (1, 200, 640), (8, 1024, 640), (8, 1024, 320), (1, 200, 320), (3, 1000, 320), (1, 33, 320),
            (1, 640, 320), (1, 640, 640), (4, 2048, 320), (4, 2048, 640), (1, 16384, 320), (2, 4096, 320), (2, 1024, 640), (8, 256, 1280),
            (3, 64, 1280), (1, 33, 640), (1, 1, 1280), (3, 1, 1280)]
OPS_FP8 = [(1, 256, 320), (2, 1024, 320), (1, 200, 640), (1, 4096, 640), (1, 4096, 320), (1, 100, 320), (2, 128, 320), (1, 384, 320),
           (1, 16384, 320)]
CLIP_VISION = [(1, 10, 2), (2, 257, 16), (8, 257, 16), (1, 64, 1), (3, 300, 4)]          # (B, N, heads) at head dim 64
CLIP_TEXT = [(1, 1, 1), (2, 20, 2), (16, 77, 12), (3, 64, 12), (3, 65, 12), (1, 77, 1), (2, 77, 12)]
CROSS_B, CROSS_N, CROSS_D, CROSS_S = (1, 3), (64, 1024, 4096), (40, 80, 160), (1, 7, 77, 257, 1000)     # test_cross_attention_gpu.py
# what the launchers refuse: head dim 48, C % heads != 0; causal attention at a head dim other than 64
REJECT_SELF = [(1, 64, 384, 8), (1, 64, 324, 8), (2, 200, 100, 3)]
REJECT_CAUSAL = [(2, 77, 320, 8), (1, 77, 384, 8), (1, 77, 700, 12)]
GRID_N = (1, 33, 64, 128, 200, 255, 256, 257, 384, 768, 769, 1000, 1024, 4096, 5184)
GRID_B = (1, 2, 4, 8, 16)
GRID_D = (40, 64, 80, 160, 48)
MAX_ELEMS = 1 << 24                                  # B * N * 3C of a recorded launch of the small-shape grid


def _uniq(seq):
    seen, out = set(), []
    for s in seq:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def _levels(levels=ATTN_LEVELS):
    return [(B, (side * lat // 64) ** 2, c, 8) for B, lat in CONFIGS + OFFGRID for side, c in levels]


def _grid(ns=GRID_N, bs=GRID_B, ds=GRID_D):
    return [(B, N, 8 * d, 8) for d in ds for B in bs for N in ns if B * N * 24 * d <= MAX_ELEMS]


def self_shapes():
    """every (B, N, C, heads) of ldmseg_op_attention in the recording (each at three dtypes and every value of key 2)"""
    return _uniq(_levels() + [(B, N, c, 8) for B, N, c in OPS_SELF] + [(B, N, 64 * h, h) for B, N, h in CLIP_VISION] + REJECT_SELF
                 + _grid())


def causal_shapes():
    """(B, N, C, heads) of ldmseg_op_attention_causal (three dtypes; no knob reaches it)"""
    return _uniq([(B, N, 64 * h, h) for B, N, h in CLIP_TEXT] + REJECT_CAUSAL
                 + [(B, N, 768, 12) for B in (1, 2, 8) for N in (1, 33, 64, 65, 77, 128, 200, 257)])


def fp8_shapes():
    """(B, N, C, heads) of ldmseg_op_attention_fp8 (bf16; every value of key 15): the head-dim-40 and -80 levels, the fp8 tests of
    tests/test_ops_gpu.py and the grid"""
    return _uniq(_levels(ATTN_LEVELS[:2]) + [(B, N, c, 8) for B, N, c in OPS_FP8] + _grid())


def cross_shapes():
    """(B, N, S, C, heads) of ldmseg_op_attention_cross (three dtypes)"""
    out = [(B, N, S, 8 * d, 8) for B in CROSS_B for N in CROSS_N for d in CROSS_D for S in CROSS_S]
    out += [(B, N, 77, 8 * d, 8) for d in (48, 64) for B in (1, 2) for N in (1, 200)] + [(1, 64, 7, 324, 8), (2, 64, 77, 320, 8)]
    return _uniq(out)


# ---- output digests: (kind, B, N, S, C, heads, dtype, key 2) under the shipped key 15.  Every form: attention.hip at one and two
# query fragments and in every dtype, attention3.hip and attention4.hip at 4 and 8 waves, the causal form, both fp8 forms (mx at 4
# and 8 waves), the cross kernel; ragged key tiles and partly empty query blocks (33, 200, 257, 1000 tokens).
def _dt3(kind, B, N, S, c, heads):
    return [(kind, B, N, S, c, heads, dt, 0) for dt in (BF16, F32, X3)]


DIGEST_CASES = (
    _dt3(SELF, 1, 33, 0, 320, 8) + _dt3(SELF, 1, 200, 0, 640, 8) + _dt3(SELF, 3, 1000, 0, 320, 8)
    + _dt3(SELF, 8, 1024, 0, 320, 8)                  # B * heads * ceil(N / 256) = 256: the 8-wave form
    + _dt3(SELF, 8, 768, 0, 320, 8)                   # 192: the 4-wave form
    + _dt3(SELF, 1, 64, 0, 1280, 8) + _dt3(SELF, 2, 257, 0, 1024, 16) + _dt3(CAUSAL, 2, 77, 0, 768, 12)
    + [(FP8, 2, 128, 0, 320, 8, BF16, 0),             # mx form at 4 waves (N % 256 != 0)
       (FP8, 1, 256, 0, 320, 8, BF16, 0),             # mx form at 8 waves
       (FP8, 1, 200, 0, 640, 8, BF16, 0)]             # unscaled fp8
    + _dt3(CROSS, 2, 64, 77, 320, 8)
    + [(SELF, 1, 200, 0, 320, 8, BF16, v) for v in (1, 2, 7, 9, 13)])


def run_case(lib, case, dev="cuda", x=None):
    """launches the case's operator on closed-form inputs (x: a preallocated input to launch on instead, dispatch recording):
    (return code, SHA-256 of the fp32 output or None)"""
    import torch
    kind, B, N, S, c, heads, dt = case[:7]
    P = lambda t: C.c_void_p(t.data_ptr())
    digest = x is None
    if kind == CROSS:
        q = x if x is not None else (2.0 * hashed(B * N * c, 11)).to(dev)
        kv = x if x is not None else hashed(B * S * 2 * c, 12).to(dev)
        out = torch.empty(B * N * c, device=dev)
        r = lib.ldmseg_op_attention_cross(P(q), P(kv), B, N, S, c, heads, dt, P(out), None)
    else:
        qkv = x if x is not None else hashed(B * N * 3 * c, 10).to(dev)
        out = torch.empty(B * N * c, device=dev)
        if kind == FP8:
            r = lib.ldmseg_op_attention_fp8(P(qkv), B, N, c, heads, P(out), 0, None, None)
        else:
            r = (lib.ldmseg_op_attention_causal if kind == CAUSAL else lib.ldmseg_op_attention)(P(qkv), B, N, c, heads, dt, P(out), None)
    if not digest or r != 0:
        return r, None
    torch.cuda.synchronize()
    return r, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def plan(lib, kind, B, N, S, c, heads, dt):
    """(return code, plan line) of ldmseg_op_attention_plan under the current knobs"""
    buf = C.create_string_buffer(256)
    r = lib.ldmseg_op_attention_plan(kind, B, N, S, c, heads, dt, buf, 256)
    return r, buf.value.decode() if r == 0 else ""


def plan_names(line):
    """'a grid=.. block=.. + b grid=.. block=..' -> ['a', 'b']"""
    return [part.split(" grid=")[0] for part in line.split(" + ")] if line else []

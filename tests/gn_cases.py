"""The GroupNorm launches whose dispatch tools/record_gn_dispatch.py records (tests/golden/gn_dispatch.json) and that
tests/test_gn_plan_cpu.py replays through ldmseg_op_groupnorm_plan, the cases whose output bytes
tests/test_ops_gpu.py::test_groupnorm_plan_equals_launch pins, and the closed-form inputs both sides build (no library RNG: the
same bytes on any machine)."""
import ctypes as C
import hashlib

F32, BF16 = 0, 1
VARIANTS = (0, 1, 2, 4, 8, 32, 33, 36, 37)           # debug key 8: every bit the chooser reads, and the combinations tests set
GN_FAMILY = ("gn_", "finish_gn<")
CONFIGS = [(8, 64), (16, 64), (4, 128)]              # = tests/test_igemm_shapes_gpu.py
OFFGRID = [(1, 8), (3, 24), (2, 40), (5, 40), (3, 72), (2, 96), (2, 128), (32, 32)]     # = tests/test_offgrid_shapes_gpu.py
# (map side at L = 64, C, C2) of GN_SHAPES and (side, Co) of CONV_GN_SHAPES in tests/test_igemm_shapes_gpu.py
# (tests/test_gn_plan_cpu.py checks that these cover those lists)
GN_LEVELS = [(64, 320, 0), (64, 640, 320), (64, 320, 320), (32, 320, 0), (32, 640, 0), (32, 1280, 640), (32, 640, 640), (32, 640, 320),
             (16, 640, 0), (16, 1280, 0), (16, 1280, 1280), (16, 1280, 640), (8, 1280, 0), (8, 1280, 1280)]
CONV_GN_LEVELS = [(32, 640), (16, 1280), (8, 1280)]
# (B, C, C2, HW) of the GroupNorm tests of tests/test_ops_gpu.py
OPS_CASES = [(2, 320, 0, 4096), (8, 1280, 0, 256), (8, 1280, 0, 16), (8, 320, 0, 4096), (8, 1280, 0, 64), (8, 2560, 0, 64), (8, 640, 0, 1024),
             (2, 320, 0, 256), (1, 640, 320, 64), (1, 1280, 640, 16), (3, 256, 0, 1024), (1, 2560, 0, 4), (2, 1280, 0, 1), (8, 1280, 640, 256),
             (4, 2560, 0, 64), (8, 256, 0, 100), (16, 640, 0, 1024), (4, 640, 0, 1024), (8, 512, 0, 1156), (8, 256, 0, 2500),
             (8, 1280, 1280, 256), (8, 640, 320, 400), (4, 320, 320, 4096), (16, 320, 0, 4096), (8, 320, 0, 3969), (4, 320, 0, 16384),
             (1, 640, 0, 4096)]
# (B, Co, HW) of test_conv_groupnorm_fused_finish
OPS_CONV_CASES = [(8, 1280, 64), (8, 1280, 256), (8, 640, 256), (8, 320, 64)]
# what launch_groupnorm refuses: channels per group below a 16-byte vector (and not exactly two groups per vector), a first source
# that is not whole vectors
REJECTS = [(4, 32, 0, 64), (4, 64, 0, 64), (2, 316, 4, 256), (2, 300, 20, 256)]
MAX_ELEMS = 1 << 24                                  # of a recorded launch of the small-shape grid


def gn_shapes():
    """every (B, C, C2, HW) of the dispatch recording, in a fixed order"""
    out = []
    for B, lat in CONFIGS + OFFGRID:
        for side, c, c2 in GN_LEVELS:
            out.append((B, c, c2, (side * lat // 64) ** 2))
    out += OPS_CASES + REJECTS
    for B in (1, 2, 3, 4, 5, 8, 12, 16):
        for c, c2 in ((128, 0), (256, 0), (320, 0), (512, 0), (640, 0), (960, 0), (1280, 0), (1920, 0), (2560, 0), (320, 320), (640, 320),
                      (1280, 640), (1280, 1280), (128, 128)):
            for hw in (16, 64, 100, 256, 400, 1024, 1156, 3969, 4096, 16384):
                if B * (c + c2) * hw <= MAX_ELEMS:
                    out.append((B, c, c2, hw))
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def conv_gn_shapes():
    """every (B, Co, HW) of the finish + GroupNorm recording"""
    out = [(B, co, (side * lat // 64) ** 2) for B, lat in CONFIGS + OFFGRID for side, co in CONV_GN_LEVELS] + OPS_CONV_CASES
    out += [(B, co, hw) for B in (2, 3, 4, 6, 8) for co in (256, 320, 640, 1280, 2560) for hw in (16, 64, 100, 144, 256, 400)]
    return sorted(set(out))


# ---- output digests: (B, C, C2, HW, dtype, key 8).  At least two per form; the cooperative form at 1, 2, 4 and 8 splits; at most
# 2^22 elements.  PAIRS: two launches one step to either side of one comparison of the rule (their plans must differ).
DIGEST_CASES = [
    (4, 640, 0, 256, BF16, 0), (4, 640, 0, 1156, BF16, 0),                     # gn_group, 10 / 20 accesses per thread
    (5, 256, 0, 1024, BF16, 32), (12, 320, 0, 1024, F32, 0),                   # gn_coop, 1 split
    (16, 320, 0, 400, BF16, 2), (8, 320, 0, 1024, F32, 0),                     # 2 splits (bf16: from 16x16 maps up, key 8 bit 1)
    (4, 640, 0, 1024, BF16, 32), (2, 640, 0, 2500, F32, 0),                    # 4 splits
    (1, 320, 0, 4096, BF16, 0), (1, 320, 320, 4096, F32, 0), (2, 320, 0, 3969, BF16, 0),      # 8 splits
    (3, 256, 0, 100, BF16, 0), (3, 256, 0, 100, F32, 0), (8, 1280, 0, 64, BF16, 0), (8, 1280, 0, 64, F32, 0),      # gn_one
    (8, 1280, 0, 256, F32, 0), (4, 128, 0, 16, F32, 0),
    (8, 1280, 0, 144, BF16, 0), (8, 1280, 0, 400, BF16, 32),                   # bf16 with 6 / 12 vectors per thread
    (8, 1280, 0, 256, F32, 4), (8, 640, 0, 400, BF16, 37), (4, 2560, 0, 64, BF16, 4), (4, 1280, 0, 400, F32, 0),     # gn_fused
    (4, 128, 0, 16, BF16, 0), (4, 640, 0, 100, BF16, 0), (8, 320, 0, 64, BF16, 0), (4, 320, 0, 16, F32, 0),          # gn_small
    (1, 256, 0, 100, BF16, 0), (1, 256, 0, 100, F32, 0), (2, 320, 0, 256, BF16, 0), (1, 640, 320, 64, F32, 0),       # gn_partial + gn_apply
    (2, 320, 0, 4096, BF16, 1), (1, 1280, 640, 16, BF16, 0),
]
PAIRS = [
    # B * groups at the gn_group / gn_small floor of 128 (32 groups: 96 | 128)
    ((3, 640, 0, 256, BF16, 0), (4, 640, 0, 256, BF16, 0)),
    ((3, 128, 0, 16, BF16, 0), (4, 128, 0, 16, BF16, 0)),
    # B * groups / GB at the floor of 96 workgroups (64 | 96)
    ((2, 1280, 0, 256, F32, 0), (3, 1280, 0, 256, F32, 0)),
    # vectors per thread at 12 | 13 (gn_one | gn_fused) and 22 | 23 (gn_fused | two launches): fp32 x 1280 has 25 pixels per trip
    ((4, 1280, 0, 300, F32, 0), (4, 1280, 0, 301, F32, 0)),
    ((4, 1280, 0, 550, F32, 0), (4, 1280, 0, 551, F32, 0)),
    # 8-byte accesses of a slice at 5120 | 5121 (gn_group<10> | gn_group<20>)
    ((4, 128, 0, 5120, BF16, 0), (4, 128, 0, 5121, BF16, 0)),
    # pixels at 255 | 256 (gn_group from 16x16 maps up) and at 1023 | 1024 (the cooperative floor, gn_group off)
    ((4, 640, 0, 255, BF16, 0), (4, 640, 0, 256, BF16, 0)),
    ((4, 640, 0, 1023, BF16, 32), (4, 640, 0, 1024, BF16, 32)),
]


# finish + GroupNorm behind a small conv (B, Ci, H, Co, K slices, dtype): 2 / 6 / 12 vectors per thread, one and two groups per workgroup
CONV_DIGEST_CASES = [(8, 64, 8, 1280, 2, BF16), (8, 64, 8, 1280, 2, F32), (8, 64, 16, 640, 3, BF16), (3, 64, 10, 256, 2, F32),
                     (8, 64, 16, 1280, 2, F32), (6, 128, 12, 640, 2, BF16), (8, 64, 20, 1280, 2, BF16)]


def digest_cases():
    out = list(DIGEST_CASES)
    for a, b in PAIRS:
        out += [c for c in (a, b) if c not in out]
    return out


def hashed(n, seed):
    """n fp32 values in [-4, 4) on a 2^-13 grid from an integer hash of (index, seed): exact in fp32, the same everywhere"""
    import torch
    h = (torch.arange(n, dtype=torch.int64) * 0x9E3779B1 + seed * 0x85EBCA6B) & 0xffffffff
    for _ in range(2):
        h = ((h ^ (h >> 16)) * 0x45D9F3B) & 0xffffffff
    h = h ^ (h >> 16)
    return ((h & 0xffff) - 32768).to(torch.float32) / 8192.0


def run_digest_case(lib, case, dev="cuda"):
    """launches ldmseg_op_groupnorm on the case's closed-form inputs (eps 1e-5, SiLU on): (return code, SHA-256 of the fp32 output)"""
    import torch
    B, Cc, C2, HW, dt, _ = case
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    x = (hashed(B * Cc * HW, 1) + 0.5).reshape(B, Cc, HW).to(dev)
    x2 = (hashed(B * C2 * HW, 2) - 1.0).reshape(B, C2, HW).to(dev) if C2 else None
    gamma = (1 + hashed(Cc + C2, 3) / 32).to(dev)
    beta = (hashed(Cc + C2, 4) / 32).to(dev)
    out = torch.empty(B, Cc + C2, HW, device=dev)
    r = lib.ldmseg_op_groupnorm(P(x), P(x2), P(gamma), P(beta), B, Cc, C2, HW, 1e-5, 1, dt, P(out), None)
    torch.cuda.synchronize()
    return r, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def run_conv_digest_case(lib, case, dev="cuda"):
    """the same for ldmseg_op_conv_groupnorm (3x3 conv as K slices, bias, per-image row, GroupNorm, SiLU)"""
    import torch
    B, Ci, H, Co, splits, dt = case
    P = lambda t: C.c_void_p(t.data_ptr())
    x = hashed(B * Ci * H * H, 5).reshape(B, Ci, H, H).to(dev)
    w = (hashed(Co * Ci * 9, 6) / 64).reshape(Co, Ci, 3, 3).to(dev)
    b, rb = (hashed(Co, 7) / 4).to(dev), (hashed(B * Co, 8) / 2).reshape(B, Co).to(dev)
    gamma, beta = (1 + hashed(Co, 3) / 32).to(dev), (hashed(Co, 4) / 32).to(dev)
    out = torch.empty(B, Co, H, H, device=dev)
    r = lib.ldmseg_op_conv_groupnorm(P(x), P(w), P(b), P(rb), P(gamma), P(beta), B, Ci, H, H, Co, 1e-5, 1, splits, dt, P(out), None)
    torch.cuda.synchronize()
    return r, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def plan(lib, B, Cc, C2, HW, dt, cus, region_ok=1, groups=32):
    """(return code, plan line) of ldmseg_op_groupnorm_plan"""
    buf = C.create_string_buffer(256)
    r = lib.ldmseg_op_groupnorm_plan(B, Cc, C2, HW, groups, dt, cus, region_ok, buf, 256)
    return r, buf.value.decode() if r == 0 else ""


def conv_plan(lib, B, Co, HW, dt):
    buf = C.create_string_buffer(256)
    r = lib.ldmseg_op_conv_groupnorm_plan(B, Co, HW, dt, buf, 256)
    return r, buf.value.decode() if r == 0 else ""


def plan_names(line):
    """'a + b splits=..' -> ['a', 'b']"""
    return line.split(" splits=")[0].split(" + ") if line else []

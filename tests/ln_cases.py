"""Cases shared by tools/record_ln_dispatch.py, tests/test_ln_plan_cpu.py and test_ops_gpu.py::test_layernorm_plan_equals_launch:
which LayerNorm / row-statistics launches are recorded, how one is run through the operators, and how the chooser is asked.

A case is (M, C, dtype, stats, key 8).  stats = 0 is ldmseg_op_layernorm.  stats = 1 is the statistics pass in front of a
folded-LayerNorm GEMM; the only operator that launches it is ldmseg_op_ln_linear, whose GEMM takes whole K tiles, so the
statistics cases exist at the widths that are a multiple of the tile (64 channels in bf16, 32 in fp32) and at no other."""
import ctypes as C

F32, BF16 = 0, 1
KEY8 = (0, 16)                                       # debug key 8 bit 4 (kGnRowstats1): the one-row-per-wave statistics form
LN_FAMILY = ("layernorm<", "rowstats<")
PC = {F32: 4, BF16: 8}                               # elements of a 16-byte vector
BKE = {F32: 32, BF16: 64}                            # elements of a K tile of the GEMM behind the statistics pass
# vectors per row to either side of every comparison of the rule: 8 / 16 / 32 / 64 lanes x 5 vectors (40, 80, 160, 320) and the
# vectors per lane of a wave (64, 128, 192, 256, 320)
NVEC = (1, 40, 41, 64, 65, 80, 81, 128, 129, 160, 161, 192, 193, 256, 257, 320, 321)
CLIP_C = (768, 1024)                                 # the CLIP encoders' widths
RAGGED_C = (6, 12)                                   # not whole vectors: 6 in both dtypes, 12 in bf16
WIDE_STATS_C = {F32: 41 * 32, BF16: 41 * 64}         # 328 vectors: the narrowest whole-K-tile row the statistics pass refuses
LN_N = 160                                           # output columns of the GEMM behind the statistics pass (one tile, no padding)


def m_values(C_, dt, stats, key8):
    """1, 9 and - at the narrowest row the operator takes - 9 rows past (grid cap x rows per workgroup and trip) of the form that
    runs there, so that its grid-stride loop is taken: layernorm<T,1,4[,stats]> 2048 x 16, rowstats<T,8,2> 4096 x 64"""
    if C_ != (BKE[dt] if stats else PC[dt]):
        return (1, 9)
    return (1, 9, (4096 * 64 if stats and not key8 else 2048 * 16) + 9)


def ln_cases():
    """every (M, C, dtype, stats, key 8) of the recording, in a fixed order"""
    out = []
    for dt in (F32, BF16):
        widths = sorted(set([n * PC[dt] for n in NVEC] + list(CLIP_C) + list(RAGGED_C) + [BKE[dt], WIDE_STATS_C[dt]]))
        for stats in (0, 1):
            for c in widths:
                if stats and c % BKE[dt]:
                    continue
                for key8 in KEY8:
                    out += [(m, c, dt, stats, key8) for m in m_values(c, dt, stats, key8)]
    return out


def inputs(case):
    """seeded CPU inputs of a case: x [M, C] with a common offset, gamma, beta, and for the statistics cases w [LN_N, C], bias"""
    import torch
    M, C_, dt, stats, _ = case
    g = torch.Generator().manual_seed(M + 7 * C_)
    x = torch.randn(M, C_, generator=g) * (1.5 if stats else 3.0) + (3.0 if stats else 1.0)
    gamma = 1 + 0.1 * torch.randn(C_, generator=g)
    beta = 0.1 * torch.randn(C_, generator=g)
    if not stats:
        return x, gamma, beta, None, None
    return x, gamma, beta, torch.randn(LN_N, C_, generator=g) / C_ ** 0.5, torch.randn(LN_N, generator=g)


def run_case(L, case, dev="cuda", io=None):
    """launches the case with the dispatch log on and key 8 set (and put back): (return code, LayerNorm-family names logged, fp32
    output on the device or None).  io: None = ldmseg_op_layernorm, 0 / 1 = ldmseg_op_layernorm_io out of place / in place."""
    import torch
    M, C_, dt, stats, key8 = case
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    x, gamma, beta, w, b = (t.to(dev) if t is not None else None for t in inputs(case))
    out = torch.zeros(M, LN_N if stats else C_, device=dev)
    assert lib.ldmseg_debug_set(8, key8) == 0
    L.igemm_log(L.LOG_ALL)
    try:
        if stats:
            r = lib.ldmseg_op_ln_linear(P(x), P(gamma), P(beta), P(w), P(b), M, C_, LN_N, 1e-5, 0, dt, P(out), None)
        elif io is None:
            r = lib.ldmseg_op_layernorm(P(x), P(gamma), P(beta), M, C_, 1e-5, 0, dt, P(out), None)
        else:
            r = lib.ldmseg_op_layernorm_io(P(x), P(gamma), P(beta), M, C_, 1e-5, 0, io, dt, P(out), None)
        torch.cuda.synchronize()
        names = sorted(n for n in L.igemm_log_read() if n.startswith(LN_FAMILY))
    finally:
        lib.ldmseg_debug_set(8, 0)
        L.igemm_log(False)
    return r, names, out if r == 0 else None


def reference(case):
    """what the operator of run_case computes, in fp32 on the CPU from the storage-rounded input"""
    import torch.nn.functional as F
    _, C_, dt, stats, _ = case
    x, gamma, beta, w, b = inputs(case)
    if dt == BF16:
        x = x.bfloat16().float()
    y = F.layer_norm(x, (C_,), gamma, beta, 1e-5)
    return F.linear(y, w, b) if stats else y


def plan(lib, M, C_, dt, stats):
    """(return code, plan line) of ldmseg_op_layernorm_plan under the current key 8"""
    buf = C.create_string_buffer(128)
    r = lib.ldmseg_op_layernorm_plan(M, C_, dt, stats, buf, 128)
    return r, buf.value.decode() if r == 0 else ""


def plan_name(line):
    """'name grid=GX block=T' -> 'name'"""
    return line.split(" grid=")[0]

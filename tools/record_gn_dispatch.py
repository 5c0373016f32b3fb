"""Record what the built library's GroupNorm launcher decides, on the GPU it runs on: tests/golden/gn_dispatch.json.

    python tools/record_gn_dispatch.py [out.json]        (LDMSEG_HIP_LIB selects another build of the library)

For every shape of tests/gn_cases.py, both dtypes and every value of debug key 8 there: ldmseg_op_groupnorm /
ldmseg_op_conv_groupnorm with the dispatch log at level 2, and the GroupNorm-family names the launch logged (the log keeps
distinct names, sorted) or its negative return code.  For the digest cases also the SHA-256 of the fp32 output on the
closed-form inputs of gn_cases.py.  tests/test_gn_plan_cpu.py replays the names through ldmseg_op_groupnorm_plan, and
tests/test_ops_gpu.py::test_groupnorm_plan_equals_launch the digests.  The committed fixture was recorded on an MI355X with
the library of the commit before the chooser moved into csrc/gn_plan.h."""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "latent-diffusion-segmentation_amd")]

import torch  # noqa: E402

import gn_cases as G  # noqa: E402
from ldmseg_amd import _lib  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gn_dispatch.json")
    lib = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    shapes, conv_shapes = G.gn_shapes(), G.conv_gn_shapes()
    nmax = max(B * (c + c2) * hw for B, c, c2, hw in shapes)
    x, x2, out = (torch.zeros(nmax, device="cuda") for _ in range(3))
    vec = torch.ones(1 << 17, device="cuda")          # gamma, beta, bias, per-image rows
    CI = 64                                          # the finish + GroupNorm launch does not depend on the conv's input channels
    cmax = max(B * co * hw for B, co, hw in conv_shapes)
    cx = torch.zeros(max(B * CI * hw for B, _, hw in conv_shapes), device="cuda")
    cw = torch.zeros(max(co for _, co, _ in conv_shapes) * CI * 9, device="cuda")
    cout = torch.zeros(cmax, device="cuda")
    names, skipped = [], []
    gn = {(s, dt): [] for s in shapes for dt in (G.F32, G.BF16)}
    conv = {(s, dt): [] for s in conv_shapes for dt in (G.F32, G.BF16)}

    def logged():
        fam = sorted(n for n in _lib.igemm_log_read() if n.startswith(G.GN_FAMILY))
        s = " + ".join(fam)
        if s not in names:
            names.append(s)
        return names.index(s)

    try:
        for vi, v in enumerate(G.VARIANTS):
            assert lib.ldmseg_debug_set(8, v) == 0
            for B, c, c2, hw in shapes:
                for dt in (G.F32, G.BF16):
                    _lib.igemm_log(_lib.LOG_ALL)
                    r = lib.ldmseg_op_groupnorm(P(x), P(x2) if c2 else None, P(vec), P(vec), B, c, c2, hw, 1e-5, 1, dt, P(out), None)
                    gn[(B, c, c2, hw), dt].append(logged() if r == 0 else r)
            for B, co, hw in conv_shapes:
                side = math.isqrt(hw)
                assert side * side == hw
                for dt in (G.F32, G.BF16):
                    _lib.igemm_log(_lib.LOG_ALL)
                    r = lib.ldmseg_op_conv_groupnorm(P(cx), P(cw), P(vec), P(vec), P(vec), P(vec), B, CI, side, side, co, 1e-5, 1, 2, dt,
                                                     P(cout), None)
                    if r not in (0, -4):
                        skipped.append([B, co, hw, dt, v, r])
                    conv[(B, co, hw), dt].append(logged() if r == 0 else r)
            torch.cuda.synchronize()
        digests, conv_digests = [], []
        for case in G.digest_cases():
            lib.ldmseg_debug_set(8, case[5])
            r, d = G.run_digest_case(lib, case)
            assert r == 0, (case, r)
            digests.append(list(case) + [d])
        lib.ldmseg_debug_set(8, 0)
        for case in G.CONV_DIGEST_CASES:
            r, d = G.run_conv_digest_case(lib, case)
            assert r == 0, (case, r)
            conv_digests.append(list(case) + [d])
    finally:
        lib.ldmseg_debug_set(8, 0)
        _lib.igemm_log(False)
    fx = {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "device": torch.cuda.get_device_name(0),
          "variants": list(G.VARIANTS), "names": names,
          # one entry per (shape, dtype): per value of "variants" the index into "names", or the negative return code
          "gn_fields": ["B", "C", "C2", "HW", "dtype", "per_variant"], "gn": [list(s) + [dt, v] for (s, dt), v in gn.items()],
          "conv_fields": ["B", "Co", "HW", "dtype", "per_variant"], "conv": [list(s) + [dt, v] for (s, dt), v in conv.items()],
          "digests": digests, "conv_digests": conv_digests}
    with open(out_path, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
        f.write("\n")
    nv = len(G.VARIANTS)
    print(f"{len(gn) * nv} GroupNorm + {len(conv) * nv} finish-GroupNorm records, {len(names)} distinct launches, {len(digests) + len(conv_digests)} digests, "
          f"{len(skipped)} skipped {skipped[:5]} -> {out_path}")


if __name__ == "__main__":
    main()

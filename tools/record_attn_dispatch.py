"""Record what the built library's attention launchers decide, on the GPU it runs on: tests/golden/attn_dispatch.json.

    python tools/record_attn_dispatch.py [out.json [commit id of the library]]    (LDMSEG_HIP_LIB selects another build)

For every shape of tests/attn_cases.py: ldmseg_op_attention (three dtypes, every value of debug key 2 there),
ldmseg_op_attention_causal (three dtypes), ldmseg_op_attention_fp8 (every value of debug key 15 there) and
ldmseg_op_attention_cross (three dtypes) with the dispatch log at level 2, and the attention-family names the launch logged
(the log keeps distinct names, sorted) or its negative return code.  For the digest cases also the SHA-256 of the fp32 output
on the closed-form inputs of attn_cases.py.  tests/test_attn_plan_cpu.py replays the names through ldmseg_op_attention_plan,
and tests/test_ops_gpu.py::test_attention_plan_equals_launch the digests.  The committed fixture was recorded on an MI355X
with the library of the commit before the rule moved into csrc/attn_plan.h ("parent" in the file)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "latent-diffusion-segmentation_amd")]

import torch  # noqa: E402

import attn_cases as A  # noqa: E402
from ldmseg_amd import _lib  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attn_dispatch.json")
    if len(sys.argv) > 2:
        parent = sys.argv[2]
    else:
        parent = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    lib = _lib.lib()
    selfs, causals, fp8s, crosses = A.self_shapes(), A.causal_shapes(), A.fp8_shapes(), A.cross_shapes()
    nmax = max([B * N * 3 * c for B, N, c, _ in selfs + causals + fp8s] + [B * max(N, 2 * S) * c for B, N, S, c, _ in crosses])
    x = torch.zeros(nmax, device="cuda")
    names = []
    rec_self = {(s, dt): [] for s in selfs for dt in (A.F32, A.BF16, A.X3)}
    rec_fp8 = {s: [] for s in fp8s}
    rec_causal, rec_cross, digests = [], [], []

    def launch(case):
        _lib.igemm_log(_lib.LOG_ALL)
        r, _ = A.run_case(lib, case, x=x)
        if r != 0:
            return r
        s = " + ".join(sorted(n for n in _lib.igemm_log_read() if n.startswith(A.ATTN_FAMILY)))
        if s not in names:
            names.append(s)
        return names.index(s)

    try:
        for v in A.KEY2:
            assert lib.ldmseg_debug_set(2, v) == 0
            for (B, N, c, h), dt in rec_self:
                rec_self[(B, N, c, h), dt].append(launch((A.SELF, B, N, 0, c, h, dt)))
            torch.cuda.synchronize()
        lib.ldmseg_debug_set(2, A.KEYS[2])
        for v in A.KEY15:
            assert lib.ldmseg_debug_set(15, v) == 0
            for B, N, c, h in fp8s:
                rec_fp8[B, N, c, h].append(launch((A.FP8, B, N, 0, c, h, A.BF16)))
            torch.cuda.synchronize()
        lib.ldmseg_debug_set(15, A.KEYS[15])
        for dt in (A.F32, A.BF16, A.X3):
            for B, N, c, h in causals:
                rec_causal.append([B, N, c, h, dt, launch((A.CAUSAL, B, N, 0, c, h, dt))])
            for B, N, S, c, h in crosses:
                rec_cross.append([B, N, S, c, h, dt, launch((A.CROSS, B, N, S, c, h, dt))])
        torch.cuda.synchronize()
        for case in A.DIGEST_CASES:
            lib.ldmseg_debug_set(2, case[7])
            r, d = A.run_case(lib, case)
            assert r == 0, (case, r)
            digests.append(list(case) + [d])
    finally:
        lib.ldmseg_debug_set(2, A.KEYS[2])
        lib.ldmseg_debug_set(15, A.KEYS[15])
        _lib.igemm_log(False)
    fx = {"parent": parent, "device": torch.cuda.get_device_name(0), "key2": list(A.KEY2), "key15": list(A.KEY15), "names": names,
          # per entry: the index into "names" or the negative return code - one per value of "key2" / "key15" where a list
          "self_fields": ["B", "N", "C", "heads", "dtype", "per_key2"], "self": [list(s) + [dt, v] for (s, dt), v in rec_self.items()],
          "fp8_fields": ["B", "N", "C", "heads", "per_key15"], "fp8": [list(s) + [v] for s, v in rec_fp8.items()],
          "causal_fields": ["B", "N", "C", "heads", "dtype", "name"], "causal": rec_causal,
          "cross_fields": ["B", "N", "S", "C", "heads", "dtype", "name"], "cross": rec_cross,
          "digest_fields": ["kind", "B", "N", "S", "C", "heads", "dtype", "key2", "sha256"], "digests": digests}
    with open(out_path, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
        f.write("\n")
    n = len(rec_self) * len(A.KEY2) + len(rec_fp8) * len(A.KEY15) + len(rec_causal) + len(rec_cross)
    print(f"{n} records, {len(names)} distinct launches, {len(digests)} digests -> {out_path}")


if __name__ == "__main__":
    main()

"""Record what the built library's LayerNorm and row-statistics launchers decide, on the GPU it runs on: tests/golden/ln_dispatch.json.

    python tools/record_ln_dispatch.py [out.json]        (LDMSEG_HIP_LIB selects another build of the library)

For every case of tests/ln_cases.py - the widths to either side of each comparison of the rule in both dtypes, the CLIP widths,
rows that are not whole vectors, debug key 8 at 0 and 16, M = 1, 9 and one value past the grid cap of the narrowest form:
ldmseg_op_layernorm (stats = 0) or ldmseg_op_ln_linear (stats = 1: its statistics pass) with the dispatch log at level 2, and the
LayerNorm-family name the launch logged or the operator's negative return code (a refused statistics pass comes back from
ldmseg_op_ln_linear as -3, a failed step).  tests/test_ln_plan_cpu.py replays the names through ldmseg_op_layernorm_plan, and
tests/test_ops_gpu.py::test_layernorm_plan_equals_launch ties them to real launches.  The committed fixture was recorded on an
MI355X with the library of the commit before the chooser moved into csrc/ln_plan.h."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "latent-diffusion-segmentation_amd")]

import torch  # noqa: E402

import ln_cases as G  # noqa: E402
from ldmseg_amd import _lib  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ln_dispatch.json")
    cases = []
    for case in G.ln_cases():
        r, names, _ = G.run_case(_lib, case)
        assert r < 0 or len(names) == 1, (case, r, names)
        cases.append(list(case) + [names[0] if r == 0 else r])
    fx = {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "device": torch.cuda.get_device_name(0), "fields": ["M", "C", "dtype", "stats", "key8", "launch"], "cases": cases}
    with open(out_path, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
        f.write("\n")
    names = sorted({c[-1] for c in cases if isinstance(c[-1], str)})
    print(f"{len(cases)} records, {len(names)} distinct launches, {sum(1 for c in cases if not isinstance(c[-1], str))} refusals -> {out_path}")


if __name__ == "__main__":
    main()

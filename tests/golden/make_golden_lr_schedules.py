"""Writes tests/golden/lr_schedules.npz by RUNNING the reference's own learning-rate schedule functions (only where the reference
checkout exists): cosine_scheduler, warmup_scheduler and step_scheduler of ldmseg/utils/utils.py.  Packages the reference imports at
module level but that are not installed are handed out as MagicMock packages by a sys.meta_path finder (make_golden_loss.py).
Nothing of the reference is copied: the fixture holds the arguments of every case (one JSON string) and the float64 arrays its
functions returned.

    python tests/golden/make_golden_lr_schedules.py [path of the reference checkout]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_loss import StubFinder, STUBS  # noqa: E402

OUT = os.path.join(HERE, "lr_schedules.npz")
KEEP = 300                                     # entries kept of the base configuration's tables

# name -> (function, positional arguments (base_value, final_value, epochs, niter_per_ep), keyword arguments, entries kept or None)
CASES = {}
for fn in ("cosine", "warmup", "step"):
    extra = {"decay_epochs": [1, 2], "decay_rate": 0.1} if fn == "step" else {}
    for w in (None, 0, 5):
        CASES[f"{fn}/3x7/warmup_{w}"] = (fn, (1e-4, 1e-6, 3, 7), dict(extra, warmup_iters=w), None)
    CASES[f"{fn}/3x7/warmup_5_from_1e-5"] = (fn, (1e-4, 1e-6, 3, 7), dict(extra, warmup_iters=5, start_warmup_value=1e-5), None)
    # tools/configs/base/base.yaml: lr 1e-4, final_lr 1e-6, warmup_iters 200; 10 epochs of 500 iterations, the first KEEP entries
    base_extra = {"decay_epochs": [20, 40], "decay_rate": 0.1} if fn == "step" else {}
    CASES[f"{fn}/base"] = (fn, (1e-4, 1e-6, 10, 500), dict(base_extra, warmup_iters=200), KEEP)
CASES["step/default_decay_epochs"] = ("step", (1e-3, 0.0, 50, 3), dict(warmup_iters=4), None)


def import_reference(ref):
    import importlib.util
    absent = [n for n in STUBS + ("scipy",) if n not in sys.modules and importlib.util.find_spec(n) is None]
    sys.meta_path.insert(0, StubFinder(absent + ["transformers"]))
    sys.path.insert(0, ref)
    from ldmseg.utils.utils import cosine_scheduler, step_scheduler, warmup_scheduler
    return {"cosine": cosine_scheduler, "warmup": warmup_scheduler, "step": step_scheduler}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LDMSEG_REFERENCE", "")
    if not os.path.isdir(ref):
        raise SystemExit(f"reference checkout not found at {ref}")
    fns = import_reference(ref)
    out = {}
    for name, (fn, args, kw, keep) in CASES.items():
        a = np.asarray(fns[fn](*args, **kw))
        assert a.dtype == np.float64 and a.shape == (args[2] * args[3],), (name, a.dtype, a.shape)
        out[name] = a if keep is None else a[:keep]
    out["cases"] = np.array(json.dumps({k: [v[0], list(v[1]), v[2], v[3]] for k, v in CASES.items()}))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(CASES)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

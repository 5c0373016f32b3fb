"""Cost of the separate image encoder in the sampling loop (bf16 perf mode, B=8, L=64, 50 steps by default).

  python tools/sepenc_loop_bench.py [--out profiles/sepenc_loop.json]
      in ONE process, after a warm-up loop of each, alternates timed 50-step ldmseg_sample_loop calls of
        (a) a plain 8-channel handle,
        (b) a separate-encoder handle (with adaptors): the image branch once per call, one add per step,
        (c) the same handle under debug key 25 = 1: the branch in every step, the form the reference runs,
      `--rounds` timed regions each (device synchronise before and after every region, host clock around it), and writes
      ms per step of the three with their spread, (b) - (a) and (c) - (b).
  python tools/sepenc_loop_bench.py --rocprof [--rocprof-dir DIR]
      two loops of (b) under rocprofv3 --kernel-trace --stats in a child process, then the skip_add kernel's row of the kernel
      statistics and the bytes it moves (read a, read b, write dst = 3 x the residual bytes) over its average time.

Prints one JSON line per result."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"
SCHED_KW = dict(prediction_type="epsilon", beta_schedule="scaled_linear", num_train_timesteps=1000, beta_start=0.00085,
                beta_end=0.012, clip_sample=False, set_alpha_to_one=False)
RESIDUAL_ELEMS_64 = 6_635_520          # elements of the 12 skip connections per image at L = 64


def residual_bytes(B, L):
    return B * RESIDUAL_ELEMS_64 * (L // 8) ** 2 // 64 * 2          # bf16


def handles(plain_too=True):
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet
    schema = weights.unet_schema(4, False)
    schema.update(weights.separate_encoder_schema(True))
    sd = weights.generate(schema, seed=21)
    sep = UNet(sd, in_channels=8, device=DEV, compute_dtype="bf16")
    plain = None
    if plain_too:
        psd = weights.generate(weights.unet_schema(8, False), seed=21)
        plain = UNet(psd, in_channels=8, device=DEV, compute_dtype="bf16")
    return sep, plain


def looper(unet, B, L, steps):
    import torch
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    sch = DDIMNoiseScheduler(**SCHED_KW)
    sch.set_timesteps_inference(steps)
    tr = TrainerDiffusion(None, unet, sch)
    g = torch.Generator().manual_seed(1)
    rgb = (0.18215 * torch.randn(B, 4, L, L, generator=g)).to(DEV)
    lat = torch.randn(B, 4, L, L, generator=g).to(DEV)
    unet.reserve(B, L)
    return lambda: tr._sample_native(sch, lat, rgb, False)


def region(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def measure(args):
    import torch
    from ldmseg_amd import _lib
    lib = _lib.lib()
    sep, plain = handles()
    run_sep, run_plain = looper(sep, args.B, args.L, args.steps), looper(plain, args.B, args.L, args.steps)
    key25 = lib.ldmseg_debug_get(25)

    def run_every_step():
        lib.ldmseg_debug_set(25, 1)
        try:
            return run_sep()
        finally:
            lib.ldmseg_debug_set(25, key25)
    variants = (("plain8", run_plain), ("sepenc_once", run_sep), ("sepenc_every_step", run_every_step))
    outs = {}
    for name, fn in variants:                      # warm-up: every shape, every kernel instantiation
        _, outs[name] = region(fn)
    same = bool(torch.equal(outs["sepenc_once"], outs["sepenc_every_step"]))
    ms = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            ms[name].append(region(fn)[0] / args.steps)
    res = {"what": "sepenc_loop", "B": args.B, "L": args.L, "steps": args.steps, "rounds": args.rounds, "dtype": "bf16",
           "once_equals_every_step": same, "residual_MB": round(residual_bytes(args.B, args.L) / 1e6, 1)}
    for name, _ in variants:
        v = ms[name]
        res[name] = {"ms_per_step_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                     "all": [round(x, 4) for x in v]}
    med = {n: statistics.median(ms[n]) for n in ms}
    res["once_minus_plain_ms_per_step"] = round(med["sepenc_once"] - med["plain8"], 4)
    res["every_step_minus_once_ms_per_step"] = round(med["sepenc_every_step"] - med["sepenc_once"], 4)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def trace_child(args):
    import torch
    sep, _ = handles(plain_too=False)
    run = looper(sep, args.B, args.L, args.steps)
    for _ in range(2):
        run()
    torch.cuda.synchronize()


def rocprof(args):
    out = args.rocprof_dir or tempfile.mkdtemp(prefix="sepenc_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", "--B", str(args.B), "--L", str(args.L),
           "--steps", str(args.steps)]
    r = subprocess.run(cmd, timeout=900)
    if r.returncode != 0:
        print(json.dumps({"what": "rocprof", "error": r.returncode}))
        return
    nbytes = 3 * residual_bytes(args.B, args.L)
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "skip_add" in row.get("Name", ""):
                    avg_ns = float(row.get("AverageNs", 0))
                    print(json.dumps({"what": "rocprof", "kernel": row["Name"][:80], "calls": row.get("Calls"),
                                      "avg_us": round(avg_ns / 1e3, 2), "min_us": round(float(row.get("MinNs", 0)) / 1e3, 2),
                                      "max_us": round(float(row.get("MaxNs", 0)) / 1e3, 2), "total_pct": row.get("Percentage"),
                                      "bytes": nbytes, "TB_per_s": round(nbytes / avg_ns / 1e3, 3) if avg_ns else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sepenc_loop.json"))
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-dir", default=None, help="where rocprofv3 writes its output (default: a fresh temporary directory)")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if args.rocprof:
        return rocprof(args)
    if args.trace_child:
        return trace_child(args)
    measure(args)


if __name__ == "__main__":
    main()

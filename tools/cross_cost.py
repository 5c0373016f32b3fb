"""Cost of cross-attention conditioning (bf16 perf mode).

  python tools/cross_cost.py                 forward at B=16, L=64, S=77 of a cross-attention handle against a handle on the same
                                             weights without attn2; one guided 50-step loop (multiplier 2) at B=8
  python tools/cross_cost.py --rocprof [--rocprof-dir DIR]
                                             the same forward under rocprofv3 --kernel-trace --stats in a child process, then the
                                             attention_cross_kernel rows of its kernel statistics

Prints one JSON line per measurement.  Timing: HIP events around `iters` back-to-back calls after `warmup` calls."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def models():
    from ldmseg_amd import weights
    from ldmseg_amd.models import UNet
    sd = weights.generate(weights.unet_schema(8, True), seed=0)
    cross = UNet(sd, in_channels=8, device=DEV, compute_dtype="bf16", cross_attention=True)
    plain = UNet({k: v for k, v in sd.items() if ".attn2." not in k and not (".norm2." in k and ".transformer_blocks." in k)},
                 in_channels=8, device=DEV, compute_dtype="bf16")
    return cross, plain


def forward_cost(cross, plain, B, L, S, warmup, iters):
    import torch
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 8, L, L, generator=g).to(DEV)
    ctx = torch.randn(B, S, 768, generator=g).to(DEV)
    t = torch.tensor([500], device=DEV)
    ms_c = timed(lambda: cross(x, t, encoder_hidden_states=ctx), warmup, iters)
    ms_p = timed(lambda: plain(x, t), warmup, iters)
    return {"what": "forward", "B": B, "L": L, "S": S, "cross_ms": round(ms_c, 3), "plain_ms": round(ms_p, 3),
            "overhead_pct": round(100.0 * (ms_c / ms_p - 1.0), 2)}


def loop_cost(cross, B, L, S, steps, iters):
    import torch
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    kw = dict(prediction_type="epsilon", beta_schedule="scaled_linear", num_train_timesteps=1000, beta_start=0.00085,
              beta_end=0.012, clip_sample=False, set_alpha_to_one=False)
    sch = DDIMNoiseScheduler(**kw)
    sch.set_timesteps_inference(steps)
    tr = TrainerDiffusion(None, cross, sch)
    g = torch.Generator().manual_seed(1)
    rgb = torch.randn(B, 4, L, L, generator=g).to(DEV)
    lat = torch.randn(B, 4, L, L, generator=g).to(DEV)
    ctx = torch.randn(2 * B, S, 768, generator=g).to(DEV)
    ms = timed(lambda: tr._sample_native_guided(sch, lat, rgb, ctx, 2, 7.5, False), 1, iters)
    return {"what": "guided_loop", "B": B, "L": L, "S": S, "steps": steps, "multiplier": 2, "loop_ms": round(ms, 2),
            "ms_per_step": round(ms / steps, 3), "image_steps_per_s": round(1000.0 * B * steps / ms, 1)}


def rocprof(args):
    out = args.rocprof_dir or tempfile.mkdtemp(prefix="cross_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--forward-only", "--iters", "5", "--warmup", "2"]
    r = subprocess.run(cmd, timeout=900)
    if r.returncode != 0:
        print(json.dumps({"what": "rocprof", "error": r.returncode}))
        return
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "attention_cross" in row.get("Name", ""):
                    print(json.dumps({"what": "rocprof", "kernel": row["Name"][:80], "calls": row.get("Calls"),
                                      "avg_us": round(float(row.get("AverageNs", 0)) / 1e3, 2),
                                      "total_pct": row.get("Percentage")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--S", type=int, default=77)
    ap.add_argument("--loop-B", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-dir", default=None, help="where rocprofv3 writes its output (default: a fresh temporary directory)")
    args = ap.parse_args()
    if args.rocprof:
        return rocprof(args)
    cross, plain = models()
    print(json.dumps(forward_cost(cross, plain, args.B, args.L, args.S, args.warmup, args.iters)), flush=True)
    if not args.forward_only:
        print(json.dumps(loop_cost(cross, args.loop_B, args.L, args.S, args.steps, 2)), flush=True)


if __name__ == "__main__":
    main()

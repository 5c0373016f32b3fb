"""Whole UNet forwards, one handle across changing shapes, and the native sampling loop away from the power-of-two shape grid
(tests/test_offgrid_shapes_gpu.py has the per-op comparisons and the coverage proof for the same configurations).

Forward bounds are those of test_path_gpu.py::test_unet_fp32_parity_vs_oracle: fp32 and bf16x3 within 1e-3 (max-norm relative)
of oracle/unet.py on the CPU, bf16 within 6e-2 max-norm and 3e-2 relative L2.  The oracle itself run in torch bf16 on the CPU
differs from its fp32 run by 1.6e-2 .. 1.9e-2 max-norm and 1.5e-2 .. 1.8e-2 relative L2 at (1,8), (2,16), (3,24), (2,40), (1,72) -
the same on and off the grid - so the bf16 bounds leave room for a correct implementation at these shapes."""
import pytest
import torch

from conftest import rel_err
from oracle import unet as o_unet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORWARD_SHAPES = [(1, 8), (3, 24), (2, 40), (5, 40), (3, 72), (2, 96)]
IDS = [f"b{b}l{l}" for b, l in FORWARD_SHAPES]
TIMESTEPS = [19, 500, 981, 259, 740]


@pytest.fixture(scope="module")
def handles(unet_sd):
    """one handle per compute mode, reused across every shape of this file in the order the tests come"""
    from ldmseg_amd.models import UNet
    return {m: UNet(unet_sd, in_channels=12, device=DEV, compute_dtype=m) for m in ("fp32", "bf16x3", "bf16")}


def _inputs(B, Ls, seed=0):
    g = torch.Generator().manual_seed(1000 * B + Ls + seed)
    x = torch.randn(B, 12, Ls, Ls, generator=g)
    t = torch.tensor(TIMESTEPS[:B]) if B > 1 else torch.tensor(999)
    return x, t


def _run(u, x, t):
    return u(x.to(DEV), t.to(DEV) if t.dim() else t).sample


@pytest.mark.parametrize("B,Ls", FORWARD_SHAPES, ids=IDS)
def test_offgrid_forward_vs_oracle(handles, unet_sd, B, Ls):
    """fp32, bf16x3 and bf16 forwards at an off-grid (B, L), per-image timesteps, against the oracle.  B >= 3 or L >= 72: the first
    and the last image against single-image oracle forwards (the last image's rows end in the partial tile of every level)."""
    torch.set_num_threads(32)
    x, t = _inputs(B, Ls)
    outs = {m: _run(u, x, t).cpu() for m, u in handles.items()}
    images = [0, B - 1] if (B >= 3 or Ls >= 72) else None
    with torch.no_grad():
        if images is None:
            pairs = [("all", slice(0, B), o_unet.unet_forward(unet_sd, x, t))]
        else:
            pairs = [(i, slice(i, i + 1), o_unet.unet_forward(unet_sd, x[i:i + 1], t[i:i + 1])) for i in sorted(set(images))]
    for m, out in outs.items():
        assert out.shape == (B, 4, Ls, Ls) and torch.isfinite(out).all(), m
    for tag, sl, ref in pairs:
        e = {m: rel_err(out[sl], ref) for m, out in outs.items()}
        l2 = {m: float((out[sl] - ref).norm() / ref.norm()) for m, out in outs.items()}
        print(f"forward B={B} L={Ls} image {tag}: fp32 {e['fp32']:.2e}  bf16x3 {e['bf16x3']:.2e} (rel-L2 {l2['bf16x3']:.2e})  "
              f"bf16 {e['bf16']:.2e} (rel-L2 {l2['bf16']:.2e})")
        assert e["fp32"] < 1e-3, (B, Ls, tag, e)
        assert e["bf16x3"] < 1e-3, (B, Ls, tag, e)
        assert e["bf16"] < 6e-2 and l2["bf16"] < 3e-2, (B, Ls, tag, e, l2)


@pytest.mark.parametrize("B,Ls", [(5, 40), (3, 24)], ids=["b5l40", "b3l24"])
def test_offgrid_batch_equals_single_images(handles, B, Ls):
    """fp32: image i of the batch against the same image run alone at B = 1.  Each is within 1e-3 of the same oracle value, so
    the two are within 2e-3 of each other; a tile that read a neighbour image's rows would not be."""
    u = handles["fp32"]
    x, t = _inputs(B, Ls, seed=7)
    batch = _run(u, x, t).cpu()
    for i in range(B):
        alone = _run(u, x[i:i + 1], t[i:i + 1]).cpu()
        e = rel_err(batch[i:i + 1], alone)
        print(f"batch B={B} L={Ls} image {i} vs alone: {e:.2e}")
        assert e < 2e-3, (B, Ls, i, e)


SEQUENCE = [(3, 24), (1, 8), (5, 40), (3, 24), (2, 96), (1, 8)]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_one_handle_across_changing_shapes(unet_sd, mode):
    """A handle called at growing and shrinking (B, L) (the workspace is reallocated on growth; split-K tickets, GroupNorm hand-off
    regions and cached plans are per handle and depend on the shape): every output bit-identical to what a fresh handle gives for
    that shape alone, repeated shapes bit-identical to their first run."""
    from ldmseg_amd.models import UNet
    make = lambda: UNet(unet_sd, in_channels=12, device=DEV, compute_dtype=mode)
    fresh = {}
    for cfg in sorted(set(SEQUENCE)):
        u = make()
        fresh[cfg] = _run(u, *_inputs(*cfg, seed=3)).cpu()
        assert torch.isfinite(fresh[cfg]).all(), cfg
        del u
    u = make()
    first = {}
    for step, cfg in enumerate(SEQUENCE):
        out = _run(u, *_inputs(*cfg, seed=3)).cpu()
        assert torch.equal(out, fresh[cfg]), (mode, step, cfg, rel_err(out, fresh[cfg]))
        assert torch.equal(out, first.setdefault(cfg, out)), (mode, step, cfg)


@pytest.mark.parametrize("Ls", [16, 24, 40])
def test_sample_native_equals_python_loop_bf16(unet_sd, sched_kw, Ls):
    """test_path_gpu.py::test_sample_native_equals_python_loop in bf16, B = 3: at L = 16 the native loop ends every step in the
    fused step tail (conv_out + scheduler update + next input), at L = 24 and 40 the tail has no tile for the map and the loop runs
    the plain conv_out GEMM and the scheduler kernel.  Both must equal the Python loop bit for bit."""
    from ldmseg_amd.models import UNet
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    u = UNet(unet_sd, in_channels=12, device=DEV, compute_dtype="bf16")
    tr = TrainerDiffusion(None, u, DDIMNoiseScheduler(**sched_kw))
    assert tr.self_condition
    prompts = ["", "", ""]
    rgb = (0.18215 * torch.randn(3, 4, Ls, Ls, generator=torch.Generator().manual_seed(1234 + Ls))).to(DEV)
    a = tr.sample(prompts, num_inference_steps=5, seed=42, rgb_latents=rgb)
    s = DDIMNoiseScheduler(**sched_kw)
    s.set_timesteps_inference(5, device=DEV)
    b = tr.sample(prompts, num_inference_steps=5, seed=42, rgb_latents=rgb, scheduler=s, python_loop=True)
    assert a.shape == (3, 4, Ls, Ls) and torch.isfinite(a).all()
    assert torch.equal(a, b), (Ls, rel_err(a, b))
    allv = tr.sample(prompts, num_inference_steps=5, seed=42, rgb_latents=rgb, return_all_latents=True)
    assert allv.shape == (15, 4, Ls, Ls) and torch.equal(allv[-3:], a)

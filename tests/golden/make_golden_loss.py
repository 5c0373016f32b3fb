"""Writes tests/golden/diffusion_loss.npz by RUNNING the reference's own training-step functions (only where the reference
checkout exists): TrainerDiffusion.compute_loss, loss_fn, get_loss_weight_mask and predict_sample, called unbound on a
SimpleNamespace self that carries the reference DDIMNoiseScheduler and a fixed stand-in epsilon network
(tests/diffusion_loss_ref.py::StandIn, this project's code).  Packages the reference imports at module level but that are not
installed are handed out as MagicMock packages by a sys.meta_path finder.  Nothing of the reference is copied: the fixture
holds the inputs, the stand-in's weights and the arrays its functions returned.

    python tests/golden/make_golden_loss.py [path of the reference checkout]
"""
import importlib.abc
import importlib.machinery
import importlib.util
import itertools
import json
import os
import sys
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diffusion_loss_ref as R   # noqa: E402

OUT = os.path.join(HERE, "diffusion_loss.npz")
SCHED = dict(prediction_type="epsilon", beta_schedule="scaled_linear", num_train_timesteps=1000, beta_start=0.00085,
             beta_end=0.012, steps_offset=1, clip_sample=False, set_alpha_to_one=False, thresholding=False,
             dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0, weight="none", max_snr=5.0,
             verbose=False)
STUBS = ("wandb", "termcolor", "torchvision", "diffusers", "detectron2", "easydict", "panopticapi", "hydra", "omegaconf", "cv2")

# (name, B, L, timesteps)
SHAPES = (("a", 2, 8, (0, 999)), ("b", 3, 24, (999, 0, 417)))
# every combination at the small shape; at the larger one a set in which every value of every option occurs
OPTIONS = dict(kind=R.LOSS_KINDS, ptype=("epsilon", "sample"), weight=("none", "max_clamp_snr"), mask=(0, 1), paste=(0, 1),
               ohem=(1.0, 0.5))
CASES_B = (("l1", "epsilon", "none", 0, 0, 1.0), ("l2", "sample", "max_clamp_snr", 1, 1, 0.5),
           ("smooth_l1", "epsilon", "max_clamp_snr", 1, 0, 0.5), ("l2", "epsilon", "none", 1, 1, 1.0),
           ("smooth_l1", "sample", "none", 0, 1, 1.0), ("l1", "sample", "max_clamp_snr", 0, 0, 0.5))


class StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, roots):
        self.roots = set(roots)

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in self.roots:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = MagicMock(name=spec.name)
        m.__path__ = []
        m.__spec__ = spec
        m.__name__ = spec.name
        m.__loader__ = self
        return m

    def exec_module(self, module):
        pass


def import_reference(ref):
    absent = [n for n in STUBS if n not in sys.modules and importlib.util.find_spec(n) is None]
    sys.meta_path.insert(0, StubFinder(absent))
    sys.path.insert(0, ref)
    from ldmseg.schedulers.ddim_scheduler import DDIMNoiseScheduler
    from ldmseg.trainers.trainers_ldm_cond import TrainerDiffusion
    return TrainerDiffusion, DDIMNoiseScheduler


def case_key(shape, kind, ptype, weight, mask, paste, ohem):
    return f"{shape}/{kind}/{ptype}/{weight}/m{mask}/p{paste}/o{ohem}"


def loss_goldens(T, DDIM, out):
    g = torch.Generator().manual_seed(20)
    w = 0.3 * torch.randn(4, 8, generator=g)
    out["standin_w"] = w.numpy()
    net = R.StandIn(w)
    scheds = {(p, m): DDIM(**{**SCHED, "prediction_type": p, "weight": m}) for p in OPTIONS["ptype"] for m in OPTIONS["weight"]}
    ac = scheds[("epsilon", "none")].alphas_cumprod
    out["alphas_cumprod"] = ac.numpy()
    out["weights_max_clamp_snr"] = scheds[("epsilon", "max_clamp_snr")].weights.numpy().astype(np.float32)
    # the square roots as the reference's add_noise / remove_noise form them on this host (`table[t] ** 0.5`).  torch's pow is
    # not the correctly rounded square root at a handful of the 1000 entries, and the device's square root (the one ldmseg_add_noise
    # has always used) is not at about a quarter of them (device_sqrt_differs.json, measured on an MI355X): `sqrt_exact` marks the
    # timesteps at which all three agree, and every timestep of this fixture is taken from them (checked where it is used)
    t_all = torch.arange(len(ac))
    sa, sb = ac[t_all] ** 0.5, (1 - ac[t_all]) ** 0.5
    out["sqrt_a"], out["sqrt_b"] = sa.numpy(), sb.numpy()
    out["sqrt_exact"] = (sa.numpy() == np.sqrt(ac.numpy())) & (sb.numpy() == np.sqrt((1 - ac).numpy()))
    with open(os.path.join(HERE, "device_sqrt_differs.json")) as f:
        out["sqrt_exact"][json.load(f)["device_differs"]] = False
    keys = []
    for name, B, L, ts in SHAPES:
        t = torch.tensor(ts, dtype=torch.long)
        assert out["sqrt_exact"][t.numpy()].all(), ts
        latents = 0.5 * torch.randn(B, 4, L, L, generator=g)
        original = latents + 0.05 * torch.randn(B, 4, L, L, generator=g)
        rgb = 0.18215 * 4 * torch.randn(B, 4, L, L, generator=g)
        noise = torch.randn(B, 4, L, L, generator=g)
        loss_mask = (torch.rand(B, L, L, generator=g) < 0.7).float() * (1.0 / torch.randint(1, 9, (B, L, L), generator=g).float())
        loss_mask[B - 1] = 0.                                           # one sample's mask is all zero
        paste = torch.rand(B, 4, L, L, generator=g) < 0.3
        noisy = scheds[("epsilon", "none")].add_noise(latents, noise, t)
        assert torch.equal(noisy, R.add_noise(latents, noise, t, sa, sb))
        for k, v in (("t", t), ("latents", latents), ("original", original), ("rgb", rgb), ("noise", noise),
                     ("loss_mask", loss_mask), ("paste", paste), ("noisy", noisy)):
            out[f"{name}/{k}"] = v.numpy()
        out[f"{name}/prediction"] = net(torch.cat([noisy, rgb], dim=1), t).sample.numpy()
        cases = list(itertools.product(*OPTIONS.values())) if name == "a" else CASES_B
        for kind, ptype, weight, mask, paste_on, ohem in cases:
            sch = scheds[(ptype, weight)]
            seen = {}

            def loss_fn(x, y, reduction='none', mask=None, _seen=seen, _self=None):
                r = T.loss_fn(_self, x, y, reduction=reduction, mask=mask)
                _seen["loss_fn"] = r.clone()
                return r
            ns = SimpleNamespace(self_condition=False, rgb_noise_level=0, cond_noise_level=0, noise_scheduler=sch, unet_model=net,
                                 training_loss_type=kind, ohem_ratio=ohem)
            ns.loss_fn = lambda *a, _ns=ns, **kw: loss_fn(*a, _self=_ns, **kw)
            loss, noisy_o, pl, t_o = T.compute_loss(
                ns, noise, t, noisy.clone(), rgb, None, loss_mask if mask else None, latents=latents, original_latents=original,
                inpainting_masks=paste if paste_on else None)
            # the element loss behind the timestep weights: the reference's own expression (:597) on its loss_fn output
            elem = seen["loss_fn"] * sch.weights[t][:, None, None, None]
            flat = elem.view(-1)
            again = (torch.topk(flat, int(ohem * flat.numel()))[0] if ohem < 1. else flat).mean()
            assert torch.equal(again, loss), (again, loss)
            assert torch.equal(noisy_o, noisy) and torch.equal(t_o, t)
            key = case_key(name, kind, ptype, weight, mask, paste_on, ohem)
            keys.append(key)
            out[key + "/loss"] = np.float32(loss)
            ek = f"{name}/elem/{kind}/{ptype}/{weight}/m{mask}"            # shared by the paste / ohem variants
            if ek in out:
                assert np.array_equal(out[ek], elem.numpy())
            out[ek] = elem.numpy()
            out[ek + "/sums"] = R.exact_sample_sums(elem)
            pk = f"{name}/pred_latents/{ptype}/p{paste_on}"
            if pk in out:
                assert np.array_equal(out[pk], pl.numpy())
            out[pk] = pl.numpy()
    out["loss_cases"] = np.asarray(keys)


def mask_goldens(T, out):
    g = torch.Generator().manual_seed(21)
    ids = torch.tensor([0, 1, 2, 3, 4, 5, 255])
    keys = []
    for name, (Hi, Wi) in (("s32", (32, 32)), ("s37x53", (37, 53)), ("s16", (16, 16))):
        B = 3
        # blocky maps, so that the resized images hold runs of one id
        coarse = ids[torch.randint(0, len(ids), (B, (Hi + 3) // 4, (Wi + 3) // 4), generator=g)]
        targets = coarse.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2)[:, :Hi, :Wi].contiguous()
        targets[1] = 0                                                   # one image is all ignore_label
        padding = torch.ones(B, Hi, Wi, dtype=torch.bool)
        padding[:, Hi - Hi // 3:, :] = False
        padding[0, :, Wi - Wi // 4:] = False
        out[f"mask/{name}/targets"] = targets.numpy()
        out[f"mask/{name}/padding"] = padding.numpy()
        for size in ((8, 8), (24, 24)):
            for type_mask, ignore in (("ignore", 0), ("padding", 0), ("counts", 0), ("counts", 255)):
                ns = SimpleNamespace(ds=SimpleNamespace(ignore_label=ignore))
                m = T.get_loss_weight_mask(ns, targets, ignore_label=ignore, mode='nearest', size=size, device='cpu',
                                           type_mask=type_mask, padding_mask=padding)
                key = f"mask/{name}/{size[0]}/{type_mask}/{ignore}"
                keys.append(key)
                out[key] = m.numpy()
    assert T.get_loss_weight_mask(SimpleNamespace(), targets, type_mask='none') is None
    out["mask_cases"] = np.asarray(keys)


def predict_goldens(T, DDIM, out):
    net = R.StandIn(torch.from_numpy(out["standin_w"]))
    keys = []
    for name, B, L, _ in SHAPES:
        latents, rgb = torch.from_numpy(out[f"{name}/latents"]), torch.from_numpy(out[f"{name}/rgb"])
        for ptype, tmax, seed in (("epsilon", None, 123), ("sample", 500, 124)):
            sch = DDIM(**{**SCHED, "prediction_type": ptype})
            ns = SimpleNamespace(noise_scheduler=sch, unet_model=net)
            while True:                                                  # the first seed from `seed` on whose timesteps qualify
                torch.manual_seed(seed)                                  # the draws of :468-472
                noise = torch.randn_like(latents)
                t = torch.randint(0, tmax if tmax is not None else sch.num_train_timesteps, (B,), dtype=torch.long)
                if out["sqrt_exact"][t.numpy()].all() and len(set(t.tolist())) == B:
                    break
                seed += 1
            torch.manual_seed(seed)
            pred = T.predict_sample(ns, latents, rgb, None, tmax=tmax)
            key = f"predict/{name}/{ptype}"
            assert out["sqrt_exact"][t.numpy()].all(), (key, t, "choose another seed")
            keys.append(key)
            out[key + "/noise"], out[key + "/t"], out[key + "/pred"] = noise.numpy(), t.numpy(), pred.numpy()
            sa, sb = torch.from_numpy(out["sqrt_a"]), torch.from_numpy(out["sqrt_b"])
            assert torch.equal(pred, R.predict_sample(net, latents, rgb, noise, t, sa, sb, ptype)), key
    out["predict_cases"] = np.asarray(keys)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LDMSEG_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "ldmseg")):
        print("reference checkout not given (argument or LDMSEG_REFERENCE); nothing to do")
        return
    T, DDIM = import_reference(ref)
    out = {}
    with torch.no_grad():
        loss_goldens(T, DDIM, out)
        mask_goldens(T, out)
        predict_goldens(T, DDIM, out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

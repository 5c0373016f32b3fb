"""Bit identity and launch identity of two builds of libldmseg_hip.so: every scenario group below runs twice, each in a fresh
child process - the parent commit's library (tools/ab/lib_parent.so, selected through LDMSEG_HIP_LIB), then this tree's - with the
profiler on, on inputs and weights drawn from fixed seeds.  A child records, per scenario, the SHA-256 of every output tensor, the
(family, label) sequence of ldmseg_profile_dump and the workspace bytes the library reports; this process compares the two
records and prints one table row per scenario.  Equal means equal: there is no tolerance.

    python tools/runtime_ab.py [--groups unet,cross,...] [--table profiles/runtime_split_ab.txt] [--host-times]

Each child runs under its own time limit and the run stops at the first child that fails, faults or is killed."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_LIB = os.path.join(ROOT, "tools", "ab", "lib_parent.so")
GROUPS = ["unet", "cross", "sepenc", "loops", "guided", "fallbacks", "vae", "vae_train", "clip", "knobs"]
CHILD_SECONDS = 400
KW = dict(prediction_type="epsilon", beta_schedule="scaled_linear", num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
          clip_sample=False, set_alpha_to_one=False)
MODES3 = ("bf16", "fp32", "bf16x3")
MODES2 = ("bf16", "fp32")
SHAPES = ((2, 16), (1, 24))          # B, L: on and off the power-of-two grid


# ---------------------------------------------------------------------------------------------------------------- child
class Recorder(object):
    """record(name, fn): fn() -> (tensors, workspace bytes or None) under a freshly reset profiler"""

    def __init__(self):
        import torch
        from ldmseg_amd import _lib
        self.torch, self.lib = torch, _lib.lib()
        self.lib.ldmseg_profile_enable(1)
        self.out = {}
        self.dump = tempfile.NamedTemporaryFile(suffix=".csv", delete=False).name

    def record(self, name, fn):
        torch = self.torch
        self.lib.ldmseg_profile_reset()
        res, ws_bytes = fn()
        torch.cuda.synchronize()
        tensors = [t for t in (res if isinstance(res, (list, tuple)) else [res]) if t is not None]
        hashes = [hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for t in tensors]
        assert self.lib.ldmseg_profile_dump(self.dump.encode()) == 0
        with open(self.dump) as f:
            launches = [",".join(l.split(",")[:-2]) for l in f.read().splitlines()[1:]]       # family,label (a label may hold commas)
        assert name not in self.out, name
        self.out[name] = {"hashes": hashes, "launches": launches, "bytes": ws_bytes}
        return res


def randn(shape, seed, scale=1.0):
    import torch
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to("cuda:0")


_sd_cache = {}


def state_dict(kind):
    from ldmseg_amd import weights as W
    if kind not in _sd_cache:
        if kind in ("unet8", "unet12"):
            sd = W.generate(W.unet_schema(int(kind[4:]), False), seed=0)
        elif kind in ("cross", "cross_proj"):
            sd = W.generate(W.unet_schema(8, True), seed=11)
            if kind == "cross_proj":
                sd.update(W.generate(W.hid_proj_schema(), seed=12))
        elif kind in ("sepenc", "sepenc_adaptor"):
            s = W.unet_schema(4, False)
            s.update(W.separate_encoder_schema(kind == "sepenc_adaptor"))
            sd = W.generate(s, seed=21)
        elif kind == "vae":
            sd = W.generate(W.vae_schema(), seed=7, norm_keys=W.VAE_NORM_KEYS)
        elif kind == "vae_image":
            sd = W.generate(W.vae_image_schema(), seed=11, norm_keys=W.VAE_IMAGE_NORM_KEYS)
        _sd_cache[kind] = sd
    return _sd_cache[kind]


def unet(kind, mode, **kw):
    from ldmseg_amd.models import UNet
    ic = 12 if kind == "unet12" else 8
    return UNet(state_dict(kind), in_channels=ic, device="cuda:0", compute_dtype=mode, **kw)


def trainer(u):
    from ldmseg_amd.schedulers import DDIMNoiseScheduler
    from ldmseg_amd.trainers import TrainerDiffusion
    return TrainerDiffusion(None, u, DDIMNoiseScheduler(**KW))


def timesteps(B):
    import torch
    return {"host": 500, "dev1": torch.tensor([500], device="cuda:0"), "devB": torch.tensor([500 - 37 * b for b in range(B)], device="cuda:0")}


def g_unet(rec):
    for kind in ("unet8", "unet12"):
        ic = int(kind[4:])
        for mode in MODES3:
            u = unet(kind, mode)
            for B, L in SHAPES:
                x = randn((B, ic, L, L), 100 + ic + L)
                for tname, t in timesteps(B).items():
                    rec.record(f"forward ic{ic} {mode} B{B} L{L} t={tname}", lambda: (u(x, t).sample, u.workspace_bytes(B, L)))
                parts = (x[:, 0:4].contiguous(), x[:, 4:8].contiguous(), x[:, 8:12].contiguous() if ic == 12 else None)
                rec.record(f"forward_parts ic{ic} {mode} B{B} L{L} cond={int(ic == 12)}",
                           lambda: (u.forward_parts(parts[0], parts[1], parts[2], 321).sample, u.workspace_bytes(B, L)))
            if kind == "unet12" and mode == "bf16":
                # workspace_bytes and reserve on a fresh handle, then a forward: the same bytes, no re-plan
                f = unet(kind, mode)
                B, L = SHAPES[0]
                before = f.workspace_bytes(B, L)
                f.reserve(B, L)
                rec.record("workspace_bytes, reserve, forward", lambda: (f(randn((B, ic, L, L), 7), 10).sample, [before, f.workspace_bytes(B, L)]))
                f.set_attention_fp8(64)          # a threshold the smallest level (L / 8 squared... the 16x16 map: 256 tokens) reaches
                rec.record("set_attention_fp8(64) forward B2 L16", lambda: (f(randn((B, ic, L, L), 7), 10).sample, f.workspace_bytes(B, L)))
                rec.record("set_attention_fp8(64) forward B1 L64", lambda: (f(randn((1, ic, 64, 64), 8), 10).sample, f.workspace_bytes(1, 64)))
            del u


def g_cross(rec):
    B, L, S = 2, 16, 5
    for kind, dim in (("cross", 768), ("cross_proj", 1024)):
        for mode in MODES2:
            u = unet(kind, mode, cross_attention=True)
            x, ctx = randn((B, 8, L, L), 31), randn((B, S, dim), 32)
            for tname, t in timesteps(B).items():
                rec.record(f"forward_ctx {kind} {mode} ctx_dim={dim} S={S} t={tname}",
                           lambda: (u(x, t, encoder_hidden_states=ctx).sample, u.workspace_bytes(B, L)))
            del u


def g_sepenc(rec):
    import torch
    B, L = 2, 16
    for kind in ("sepenc", "sepenc_adaptor"):
        for mode in MODES2:
            u = unet(kind, mode)
            x = randn((B, 8, L, L), 41)
            ti = {"none": None, "host": 40, "dev1": torch.tensor([40], device="cuda:0"), "devB": torch.tensor([40, 300], device="cuda:0")}
            for name, t in ti.items():
                rec.record(f"forward_img {kind} {mode} timg={name}", lambda: (u(x, 500, timestep_img=t).sample, u.workspace_bytes(B, L)))
            rec.record(f"forward_parts {kind} {mode}", lambda: (u.forward_parts(x[:, :4].contiguous(), x[:, 4:].contiguous(), None, 500).sample, None))
            del u


def loop(tr, B, L, seed=42, steps=3, all_latents=False):
    rgb = randn((B, 4, L, L), 1234, 0.18215)
    return tr.sample([""] * B, num_inference_steps=steps, seed=seed, rgb_latents=rgb, return_all_latents=all_latents)


def inpaint_loop(tr, B, L):
    import torch
    rgb = randn((B, 4, L, L), 1234, 0.18215)
    known = (torch.rand((B, 1, L, L), generator=torch.Generator().manual_seed(5)) > 0.5).to("cuda:0")
    return tr.sample_inpaint([""] * B, known, randn((B, 4, L, L), 6), num_inference_steps=3, seed=42, rgb_latents=rgb)


def check_fused_loop(rec, name, steps=3):
    """the fused tail ran in every step and only step 1 packed its input: family 4's unlabelled launches are the input packs
    (the loop's forwards take their time-embedding rows from the table)"""
    launches = rec.out[name]["launches"]
    assert sum("conv_out_tail ddim=1" in l for l in launches) == steps, (name, launches)
    assert sum(l == "4," for l in launches) == 1, (name, [l for l in launches if l.startswith("4,")])


def g_loops(rec):
    from ldmseg_amd import _lib
    B, L = 2, 16
    for mode in MODES2:
        u = unet("unet8", mode)
        tr = trainer(u)
        rec.record(f"sample_loop plain {mode}", lambda: (loop(tr, B, L), u.workspace_bytes(B, L)))
        rec.record(f"sample_loop all_latents {mode}", lambda: (loop(tr, B, L, all_latents=True), None))
        rec.record(f"sample_loop inpainting {mode}", lambda: (inpaint_loop(tr, B, L), None))
        if mode == "bf16":
            for n in ("plain", "all_latents", "inpainting"):
                check_fused_loop(rec, f"sample_loop {n} bf16")
            rec.record("sample_loop plain bf16 B1 L24", lambda: (loop(tr, 1, 24), u.workspace_bytes(1, 24)))
        del u, tr
        u = unet("unet12", mode)
        tr = trainer(u)
        rec.record(f"sample_loop self-conditioned {mode}", lambda: (loop(tr, B, L), u.workspace_bytes(B, L)))
        if mode == "bf16":
            check_fused_loop(rec, "sample_loop self-conditioned bf16")
        del u, tr
    for kind in ("sepenc", "sepenc_adaptor"):
        u = unet(kind, "bf16")
        tr = trainer(u)
        for every in (0, 1):
            _lib.check(_lib.lib().ldmseg_debug_set(25, every))
            rec.record(f"sample_loop {kind} bf16 key25={every}", lambda: (loop(tr, B, L), u.workspace_bytes(B, L)))
        _lib.check(_lib.lib().ldmseg_debug_set(25, 0))
        del u, tr


def g_guided(rec):
    B, L, S = 2, 16, 5
    for mode in MODES2:
        u = unet("cross", mode, cross_attention=True)
        tr = trainer(u)
        sch = tr.noise_scheduler
        for mult in (1, 2):
            def run():
                sch.set_timesteps_inference(3)
                rgb, lat, ctx = randn((B, 4, L, L), 1234, 0.18215), randn((B, 4, L, L), 42), randn((mult * B, S, 768), 33)
                return tr._sample_native_guided(sch, lat, rgb, ctx, mult, 7.5, True), u.workspace_bytes(mult * B, L)
            name = f"sample_loop_guided {mode} multiplier={mult}"
            rec.record(name, run)
            # the context's K|V: 16 Linears of K = 768 in step 1 only (no other launch of the UNet has that K)
            kv = [l for l in rec.out[name]["launches"] if " K=768 " in l]
            assert len(kv) == 16, (name, len(kv))
        del u, tr


def g_fallbacks(rec):
    from ldmseg_amd import _lib
    lib = _lib.lib()
    B, L = 2, 16
    for key in (12, 14, 16, 19, 20, 21, 22, 23):
        shipped = lib.ldmseg_debug_get(key)
        _lib.check(lib.ldmseg_debug_set(key, 0))
        u = unet("unet12", "bf16")           # (a fresh handle: created and planned under the knob)
        tr = trainer(u)
        x = randn((B, 12, L, L), 51)
        rec.record(f"key {key}=0 forward bf16", lambda: (u(x, 500).sample, u.workspace_bytes(B, L)))
        rec.record(f"key {key}=0 sample_loop bf16", lambda: (loop(tr, B, L), None))
        del u, tr
        _lib.check(lib.ldmseg_debug_set(key, shipped))


def g_vae(rec):
    import torch
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.models.vae import GeneralVAEImage
    B, L, H = 2, 8, 64
    for mode in MODES3:
        v = GeneralVAESeg(state_dict("vae"), scaling_factor=0.2, device="cuda:0", compute_dtype=mode)
        z = randn((B, 4, L, L), 61)
        x = (torch.rand((B, 7, H, H), generator=torch.Generator().manual_seed(62)) > 0.5).float().to("cuda:0")
        S = 8 * L
        sizes, boxes = [(S - 3, S - 9), (S // 2, S)], [(0, 0, S - 4, S - 8), (2, 1, S - 6, S - 2)]
        tg = torch.randint(0, 128, (B, S, S), generator=torch.Generator().manual_seed(63)).to("cuda:0")

        def pan(fn, first, **kw):
            outs, st = fn(first, (S, S), sizes, boxes, return_stats=True, count_th=8, **kw)
            return [o[0] for o in outs] + st["labels"] + [st["counts"], st["mask_counts"], st["keep"]], None

        def sem(fn, first, **kw):
            counts = torch.zeros((3, 128), dtype=torch.int64, device="cuda:0")
            preds = fn(first, (S, S), tg, counts, ignore_index=0, **kw)
            return [preds, counts], None
        rec.record(f"vae decode interpolate=0 {mode}", lambda: (v.decode(z, interpolate=False, z_scale=5.0), None))
        rec.record(f"vae decode interpolate=1 {mode}", lambda: (v.decode(z, interpolate=True, z_scale=5.0), None))
        rec.record(f"vae decode_argmax {mode}", lambda: (list(v.decode_argmax(z, z_scale=5.0, mask_th=0.02, return_prob=True)), None))
        rec.record(f"vae decode_panoptic {mode}", lambda: pan(v.decode_panoptic, z, z_scale=5.0))
        rec.record(f"vae decode_panoptic topk_diff {mode}", lambda: pan(v.decode_panoptic, z, z_scale=5.0, threshold_mode="topk_diff", mask_th=0.1))
        rec.record(f"vae decode_semseg {mode}", lambda: sem(v.decode_semseg, z, z_scale=5.0, mask_th=0.02))
        rec.record(f"vae encode {mode}", lambda: (v.encode_moments(x, 2.0, -1.0), None))
        rec.record(f"vae reconstruct_semseg {mode}", lambda: sem(v.reconstruct_semseg, x, in_mul=2.0, in_add=-1.0))
        rec.record(f"vae reconstruct_panoptic {mode}", lambda: pan(v.reconstruct_panoptic, x, in_mul=2.0, in_add=-1.0))
        del v
        k = GeneralVAEImage(state_dict("vae_image"), device="cuda:0", compute_dtype=mode)
        for h, w in ((64, 64), (64, 128)):
            rec.record(f"image vae encode {h}x{w} {mode}", lambda: (k.encode_moments(randn((B, 3, h, w), 64), 2.0, -1.0), None))

        def refused():       # 8 x 9 latent pixels are no multiple of the 64 the mid-block attention serves: the same refusal
            try:
                k.encode_moments(randn((B, 3, 64, 72), 64), 2.0, -1.0)
            except RuntimeError as e:
                return None, str(e)
            return None, "accepted"
        rec.record(f"image vae encode 64x72 {mode} (refused)", refused)
        del k


def g_vae_train(rec):
    """The seg-VAE's training entries on fp32-storage handles (fp32 and bf16x3, whose hi | lo planes the build and the load entries
    split), at a power-of-two shape and at H = 40 (maps 40 / 20 / 10 / 5): both backwards with every gradient and with the single
    gradients at which the encoder's chain ends early, the load entries followed by a forward (those also in bf16) and by both
    backwards on the reloaded handle, and one TrainerAE.training_step with the library's optimiser."""
    import torch
    from collections import OrderedDict
    from ldmseg_amd import _lib
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.models.vae import _name_arrays
    from ldmseg_amd.optim import AdamW
    from ldmseg_amd.trainers import TrainerAE
    lib, sd = _lib.lib(), state_dict("vae")
    enc, dec = [k for k in sd if k.startswith("encoder.")], [k for k in sd if k.startswith("decoder.")]
    assert len(enc) == 20 and len(dec) == 14
    stream = lambda: _lib.stream_ptr(torch.device("cuda:0"))

    def make(mode):
        return GeneralVAESeg(sd, scaling_factor=0.2, device="cuda:0", compute_dtype=mode)

    def backward(v, first, grad, names, grad_z=None):
        """one ldmseg_vae_{decode,encode}_backward call (decode: `first` has the 4 latent channels) for the gradients of `names`"""
        grads = OrderedDict((k, torch.full(tuple(sd[k].shape), float("nan"), device="cuda:0")) for k in names)
        n, c_names, c_ptrs, c_numels = _name_arrays(grads)
        B, C, S, _ = first.shape
        if C == 4:
            code = lib.ldmseg_vae_decode_backward(v._h, _lib.ptr(first), 5.0, B, S, _lib.ptr(grad), _lib.ptr(grad_z), n, c_names, c_ptrs, c_numels, stream())
        else:
            code = lib.ldmseg_vae_encode_backward(v._h, _lib.ptr(first), 2.0, -1.0, B, S, _lib.ptr(grad), n, c_names, c_ptrs, c_numels, stream())
        _lib.check(code, "backward")
        return list(grads.values()) + [grad_z], None

    def load(v, half, names, seed):
        ts = OrderedDict((k, randn(tuple(sd[k].shape), seed + i, 0.05)) for i, k in enumerate(names))
        n, c_names, c_ptrs, c_numels = _name_arrays(ts)
        _lib.check(getattr(lib, "ldmseg_vae_load_" + half)(v._h, n, c_names, c_ptrs, c_numels, stream()), "load_" + half)
        torch.cuda.synchronize()          # (the sources live until the packs have read them)

    for B, H in ((2, 64), (1, 40)):
        L = H // 8
        x = (torch.rand((B, 7, H, H), generator=torch.Generator().manual_seed(81)) > 0.5).float().to("cuda:0")
        z, gl, gm = randn((B, 4, L, L), 82), randn((B, 128, 4 * L, 4 * L), 83), randn((B, 8, L, L), 84)
        for mode in MODES3:
            tag = f"{mode} B{B} H{H}"
            v = make(mode)
            if mode != "bf16":
                rec.record(f"decode_backward every gradient, grad_z, z_scale=5 {tag}", lambda: backward(v, z, gl, dec, torch.empty_like(z)))
                rec.record(f"decode_backward decoder.6.bias only, grad_z null {tag}", lambda: backward(v, z, gl, ["decoder.6.bias"]))
                rec.record(f"encode_backward every gradient {tag}", lambda: backward(v, x, gm, enc))
                for k in ("encoder.15.weight", "encoder.13.weight", "encoder.8.weight", "encoder.0.bias"):      # head, GroupNorm, layer 5, layer 0
                    rec.record(f"encode_backward {k} only {tag}", lambda: backward(v, x, gm, [k]))
            load(v, "decoder", ["decoder.2.weight", "decoder.10.bias"], 90)
            rec.record(f"load_decoder decoder.2.weight + decoder.10.bias, decode {tag}", lambda: (v.decode(z, interpolate=False, z_scale=5.0), None))
            load(v, "encoder", ["encoder.3.weight"], 95)
            rec.record(f"load_encoder encoder.3.weight, encode {tag}", lambda: (v.encode_moments(x, 2.0, -1.0), None))
            if mode == "bf16":
                continue
            rec.record(f"encode_backward every gradient, reloaded handle {tag}", lambda: backward(v, x, gm, enc))
            rec.record(f"decode_backward every gradient, reloaded handle {tag}", lambda: backward(v, z, gl, dec, torch.empty_like(z)))
            del v
            t = make(mode)
            tr = TrainerAE(t, loss_weights={"ce": 1.0, "mask": 1.0, "kl": 1e-4},
                           loss_kwargs=dict(num_points=64, oversample_ratio=3, importance_sample_ratio=0.75, temperature=1.0))
            opt = AdamW(t.parameters(), lr=1e-3)
            ids = torch.randint(0, 12, (B, L, L), generator=torch.Generator().manual_seed(85)).repeat_interleave(8, 1).repeat_interleave(8, 2)
            bits = (2.0 * torch.stack([(ids >> i) % 2 for i in range(7)], dim=1).float() - 1.0).to("cuda:0")

            def step():
                losses = tr.training_step(bits, ids.to("cuda:0"), opt, clip_grad=1.0, generator=torch.Generator(device="cuda:0").manual_seed(20),
                                          point_generator=torch.Generator().manual_seed(0))
                return list(losses) + [tr.last_grad_norm] + list(t.parameters()), None
            rec.record(f"training_step library AdamW, clip 1.0 {tag}", step)
            del t, tr, opt


def g_clip(rec):
    import torch
    from ldmseg_amd import weights as W
    from ldmseg_amd.models.clip_text import CLIPTextEncoder
    from ldmseg_amd.models.clip_vision import CLIPVisionDescriptor
    vcfg = dict(hidden=128, intermediate=512, layers=2, heads=2, image=42, patch=14, projection_dim=96)
    tcfg = dict(vocab=512, hidden=128, intermediate=512, layers=2, heads=2, positions=77)
    vs, ts = W.clip_vision_schema(**vcfg), W.clip_text_schema(**tcfg)
    vsd = W.generate(vs, seed=21, norm_keys=W.clip_vision_norm_keys(vs))
    tsd = W.generate(ts, seed=23, norm_keys=W.clip_text_norm_keys(ts))
    ids = torch.randint(0, 512, (2, 7), generator=torch.Generator().manual_seed(71))
    for mode in MODES3:
        m = CLIPVisionDescriptor(vsd, projection=True, device="cuda:0", compute_dtype=mode)
        rec.record(f"clip vision forward {mode}", lambda: (list(m.encode(randn((2, 3, 42, 42), 72))), None))
        rec.record(f"clip vision describe {mode}", lambda: (m.describe(randn((2, 3, 50, 61), 73).abs().clamp(0, 1)), None))
        del m
        t = CLIPTextEncoder(tsd, device="cuda:0", compute_dtype=mode)
        rec.record(f"clip text forward R=2 T=7 {mode}", lambda: (t(ids)[0], None))
        del t


def g_knobs(rec):
    """ldmseg_debug_get of every key after a fixed sequence of sets (no launch: integers only)"""
    from ldmseg_amd import _lib
    lib = _lib.lib()
    keys = list(range(-1, 27))
    shipped = [lib.ldmseg_debug_get(k) for k in keys]
    sets = [(1, 3), (2, 1), (5, -1), (8, 2), (9, 1), (10, 1), (11, 7), (12, 1), (13, 256), (14, 1), (15, 0), (16, 0), (19, 0), (20, 0),
            (21, 0), (22, 4), (23, 0x305), (24, -1), (25, 1), (6, 1), (7, 1)]
    codes = [lib.ldmseg_debug_set(k, v) for k, v in sets]
    unknown = [lib.ldmseg_debug_set(k, 1) for k in (-1, 0, 17, 18, 26, 99)]
    msg = _lib.lib().ldmseg_last_error().decode()
    after = [lib.ldmseg_debug_get(k) for k in keys]
    rec.out["debug_get of keys -1..26"] = {"hashes": [], "launches": [], "bytes": [shipped, codes, unknown, msg, after]}


def host_times(out_path, calls=200, repeats=5):
    """Host cost of the seg-VAE entries (the launch sequences being equal, the GPU time is): wall-clock milliseconds of `calls`
    back-to-back calls with one final synchronize, `repeats` times per entry, at B = 2, H = 64 in fp32, profiler off."""
    import time
    import torch
    from ldmseg_amd import _lib
    from ldmseg_amd.models import GeneralVAESeg
    from ldmseg_amd.models.vae import _name_arrays
    lib, sd = _lib.lib(), state_dict("vae")
    v = GeneralVAESeg(sd, scaling_factor=0.2, device="cuda:0", compute_dtype="fp32")
    B, H, L = 2, 64, 8
    x = (torch.rand((B, 7, H, H), generator=torch.Generator().manual_seed(81)) > 0.5).float().to("cuda:0")
    z, gl, gm = randn((B, 4, L, L), 82), randn((B, 128, 4 * L, 4 * L), 83), randn((B, 8, L, L), 84)
    gz, s = torch.empty_like(z), _lib.stream_ptr(torch.device("cuda:0"))
    ge = {k: torch.empty(tuple(t.shape), device="cuda:0") for k, t in sd.items() if k.startswith("encoder.")}
    gd = {k: torch.empty(tuple(t.shape), device="cuda:0") for k, t in sd.items() if k.startswith("decoder.")}
    ae, ad = _name_arrays(ge), _name_arrays(gd)
    entries = {
        "encode": lambda: v.encode_moments(x, 2.0, -1.0),
        "decode": lambda: v.decode(z, interpolate=False, z_scale=5.0),
        "encode_backward": lambda: _lib.check(lib.ldmseg_vae_encode_backward(v._h, _lib.ptr(x), 2.0, -1.0, B, H, _lib.ptr(gm), *ae, s)),
        "decode_backward": lambda: _lib.check(lib.ldmseg_vae_decode_backward(v._h, _lib.ptr(z), 5.0, B, L, _lib.ptr(gl), _lib.ptr(gz), *ad, s)),
    }
    out = {}
    for name, fn in entries.items():
        fn()
        torch.cuda.synchronize()
        out[name] = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out[name].append(round((time.perf_counter() - t0) * 1e3, 3))
    with open(out_path, "w") as f:
        json.dump(out, f)


def child(group, out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-segmentation_amd")]
    if group == "host_times":
        return host_times(out_path)
    rec = Recorder()
    globals()["g_" + group](rec)
    with open(out_path, "w") as f:
        json.dump(rec.out, f)


# --------------------------------------------------------------------------------------------------------------- parent
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default=",".join(GROUPS))
    ap.add_argument("--table", default=None)
    ap.add_argument("--host-times", action="store_true", help="also time the seg-VAE entries' host cost under both libraries")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.out)
    assert os.path.exists(PARENT_LIB), "build the parent commit's library into tools/ab/lib_parent.so first"
    rows, all_equal = [], True
    tmp = tempfile.mkdtemp()

    def both(g):
        """the records of child `g` under the parent's library, then under this tree's; None when one of them did not end well"""
        recs = {}
        for side in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("LDMSEG_HIP_LIB", None)
            if side == "parent":
                env["LDMSEG_HIP_LIB"] = PARENT_LIB
            out = os.path.join(tmp, f"{g}_{side}.json")
            cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", g, "--out", out]
            print("#", side, g, flush=True)
            r = subprocess.run(cmd, env=env)
            if r.returncode != 0:
                print(f"child {side}/{g} ended with status {r.returncode}: stopping here", flush=True)
                return None
            with open(out) as f:
                recs[side] = json.load(f)
        return recs

    for g in a.groups.split(","):
        recs = both(g)
        if recs is None:
            return 2
        p, t = recs["parent"], recs["tree"]
        if list(p) != list(t):
            print(f"group {g}: the two builds ran different scenarios")
            return 2
        for name in p:
            eq = [p[name][k] == t[name][k] for k in ("hashes", "launches", "bytes")]
            all_equal &= all(eq)
            rows.append((f"{g}: {name}", len(p[name]["hashes"]), len(p[name]["launches"]), "equal" if all(eq) else
                         "DIFFERENT (" + ", ".join(k for k, e in zip(("outputs", "launches", "workspace bytes"), eq) if not e) + ")"))
            if not eq[1]:
                for i, (x, y) in enumerate(zip(p[name]["launches"], t[name]["launches"])):
                    if x != y:
                        print(f"  first differing launch {i}: parent {x!r} tree {y!r}")
                        break
    w = max(len(r[0]) for r in rows)
    lines = [f"{'scenario':<{w}}  outputs  launches  parent vs this tree"] + [f"{n:<{w}}  {h:>7}  {l:>8}  {e}" for n, h, l, e in rows]
    lines.append(f"{len(rows)} scenarios: " + ("every hash, launch sequence and byte count equal" if all_equal else "DIFFERENCES, see above"))
    if a.host_times:
        recs = both("host_times")
        if recs is None:
            return 2
        lines += ["", "host time: ms of 200 back-to-back calls + one synchronize, B = 2, H = 64, fp32, five repeats (parent | this tree)"]
        for name in recs["parent"]:
            pt, tt = recs["parent"][name], recs["tree"][name]
            lines.append(f"{name:<16} parent {pt} min {min(pt)} max {max(pt)} | tree {tt} median {sorted(tt)[len(tt) // 2]}")
    print("\n".join(lines))
    if a.table:
        with open(a.table, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())

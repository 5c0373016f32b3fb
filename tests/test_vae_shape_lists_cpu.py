"""CPU suite: the launch lists of the two VAEs (tests/vae_cases.py, what tests/test_vae_shapes_gpu.py launches entry by entry)
against the layer walk of oracle/vae.py and oracle/vae_image.py.  The walk runs on the meta device (shapes only) at every
configuration of the GPU tests with F.conv2d, F.conv_transpose2d, F.group_norm, F.pad, F.linear, torch.bmm and torch.softmax recorded;
the lists must be exactly what the oracle executes - none missing, none extra, in the same order.

The last test needs no device either: ``ldmseg_op_igemm_plan`` names the igemm instantiation of every GEMM entry at the workload
size (a 512 x 512 image, B = 1); each of those names must also be planned by some case the GPU tests run."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import vae_cases as V
from conftest import GOLDEN


@pytest.fixture()
def recorder(monkeypatch):
    """patches the functional ops of both oracle modules; returns the list the calls are appended to"""
    from oracle import vae as o_vae, vae_image as o_img
    assert o_vae.F is F and o_img.F is F and o_img.torch is torch
    log = []
    real = {n: getattr(F, n) for n in ("conv2d", "conv_transpose2d", "group_norm", "pad", "linear")}
    real_bmm, real_softmax = torch.bmm, torch.softmax

    def conv2d(x, w, b=None, stride=1, padding=0):
        log.append(("conv2d", x.shape[0], w.shape[1], w.shape[0], w.shape[2], stride, padding, x.shape[2], x.shape[3], b is not None))
        return real["conv2d"](x, w, b, stride=stride, padding=padding)

    def conv_transpose2d(x, w, b=None, stride=1):
        assert tuple(w.shape[2:]) == (2, 2) and stride == 2
        log.append(("convt", x.shape[0], w.shape[0], w.shape[1], x.shape[2], x.shape[3]))
        return real["conv_transpose2d"](x, w, b, stride=stride)

    def group_norm(x, groups, w, b, eps):
        assert groups == 32
        log.append(("gn", x.shape[0], x.shape[1], x.shape[2] * x.shape[3], eps))
        return real["group_norm"](x, groups, w, b, eps)

    def pad(x, p):
        log.append(("pad", tuple(p)))
        return real["pad"](x, p)

    def linear(x, w, b=None):
        log.append(("linear", x.shape[0], x.shape[1], w.shape[1], w.shape[0]))
        return real["linear"](x, w, b)

    def bmm(a, b):
        log.append(("bmm", a.shape[0], a.shape[1], b.shape[2], a.shape[2]))
        return real_bmm(a, b)

    def softmax(x, dim):
        assert dim == -1
        log.append(("softmax", x.shape[0], x.shape[1], x.shape[2]))
        return real_softmax(x, dim)

    for n, f in (("conv2d", conv2d), ("conv_transpose2d", conv_transpose2d), ("group_norm", group_norm), ("pad", pad), ("linear", linear)):
        monkeypatch.setattr(F, n, f)
    monkeypatch.setattr(torch, "bmm", bmm)
    monkeypatch.setattr(torch, "softmax", softmax)
    return log


def as_oracle_ops(entries):
    """a launch list as the sequence of recorded oracle calls it stands for.  Pack / LayerNorm / Posterior / tail entries have no
    recorded call (the oracle's LayerNorm2d is written out); a pad-0 stride-2 conv is F.pad(0,1,0,1) + a conv without padding on the
    padded map; the attention's per-image launches are the oracle's batched ops."""
    ops, i = [], 0
    while i < len(entries):
        e = entries[i]
        nxt = entries[i + 1] if i + 1 < len(entries) else None
        if (isinstance(e, V.Conv) and isinstance(nxt, V.Conv) and e.k == 1 and not e.resid and nxt.k == 3 and nxt.resid and
                e.Ci != e.Co and (nxt.Ci, nxt.Co) == (e.Co, e.Co)):
            # a resnet whose channel count changes: the model launches conv_shortcut before conv2 (its output is conv2's residual),
            # the oracle calls it after conv2
            ops += as_oracle_ops([nxt]) + as_oracle_ops([e])
            i += 2
            continue
        if isinstance(e, V.Conv):
            if e.pad == 0:
                ops.append(("pad", (0, 1, 0, 1)))
                ops.append(("conv2d", e.B, e.Ci, e.Co, e.k, e.stride, 0, e.H + 1, e.W + 1, True))
            else:
                ops.append(("conv2d", e.B, e.Ci, e.Co, e.k, e.stride, e.k // 2, e.H, e.W, True))
        elif isinstance(e, V.ConvT):
            ops.append(("convt", e.B, e.Ci, e.Co, e.H, e.W))
        elif isinstance(e, V.GroupNorm):
            ops.append(("gn", e.B, e.C, e.HW, e.eps))
        elif isinstance(e, V.Bilinear):
            ops.append(("interpolate", e.B, e.C, e.H, e.W))
        elif isinstance(e, V.Gemm):
            # B x (scores, softmax, V^T, P V) behind the q and k 1x1 convs, the output projection behind them
            B = sum(1 for x in entries if isinstance(x, V.Softmax))
            group = entries[i:i + 4 * B]
            assert all(group[4 * b:4 * b + 4] == group[:4] for b in range(B))
            s, sm, vt, pv = group[:4]
            N, C = s.M, s.K
            assert (s, vt, pv) == (V.Gemm(N, N, C, 1, 0), V.Gemm(C, N, C, 0, 0), V.Gemm(N, C, N, 0, 1)) and sm == V.Softmax(N, N, C ** -0.5)
            ops += [("linear", B, N, C, C), ("bmm", B, N, N, C), ("softmax", B, N, N), ("bmm", B, N, C, N)]
            i += 4 * B - 1
        i += 1
    return ops


def fold_attention_linears(ops):
    """the oracle's attention applies q, k, v as three F.linear calls and the output projection as a fourth; the model runs q, k and
    the projection as 1x1 convs over the map and v as the V^T GEMM: rewrite the recorded calls into that form"""
    out, i = [], 0
    while i < len(ops):
        if ops[i][0] == "linear":
            (_, B, N, C, C2), gn = ops[i], out[-1]
            assert ops[i + 1] == ops[i + 2] == ops[i] and C == C2 and gn[0] == "gn" and gn[3] == N
            assert [o[0] for o in ops[i + 3:i + 7]] == ["bmm", "softmax", "bmm", "linear"] and ops[i + 6] == ops[i]
            hw = [o for o in out if o[0] == "conv2d"][-1]
            H, W = hw[7], hw[8]
            assert H * W == N
            c1 = ("conv2d", B, C, C, 1, 1, 0, H, W, True)
            out += [c1, c1, ("linear", B, N, C, C)] + list(ops[i + 3:i + 6]) + [c1]
            i += 7
        else:
            out.append(ops[i])
            i += 1
    return out


def meta_sd(schema):
    return {k: torch.empty(shape, device="meta") for k, shape in schema.items()}


@pytest.mark.parametrize("B,H,W", V.SEG_CONFIGS + [V.SEG_WORKLOAD])
def test_seg_vae_lists_are_what_the_oracle_executes(recorder, B, H, W):
    from ldmseg_amd import weights
    from oracle import vae as o_vae
    sd = meta_sd(weights.vae_schema())
    lists = V.seg_lists(B, H, W)
    mom = o_vae.encode_moments(sd, torch.empty(B, 7, H, H, device="meta"))
    assert tuple(mom.shape) == (B, 8, H // 8, H // 8)
    enc_ops = list(recorder)
    assert enc_ops == as_oracle_ops(lists["encode"])
    del recorder[:]
    z = torch.empty(B, 4, H // 8, H // 8, device="meta")
    y = o_vae.decode(sd, z, interpolate=False)
    assert tuple(y.shape) == (B, 128, H // 2, H // 2)
    dec_ops = list(recorder)
    for t in V.DECODE_TAILS:
        lst = lists["decode_" + t]
        assert dec_ops == [o for o in as_oracle_ops(lst) if o[0] != "interpolate"], t
        # every transposed conv is followed by the in-place LayerNorm2d + SiLU over its output (written out in the oracle)
        for i, e in enumerate(lst):
            if isinstance(e, V.ConvT):
                assert lst[i + 1] == V.LayerNorm(e.B * 4 * e.H * e.W, e.Co, 1e-6, 1, 1), (t, i)
        assert sum(isinstance(e, V.LayerNorm) for e in lst) == sum(isinstance(e, V.ConvT) for e in lst) == 2
        last = lst[-1]
        want = {"logits": V.Conv, "logits_x2": V.Bilinear, "argmax": V.BilinearArgmax, "panoptic": V.PostprocTail, "semseg": V.PostprocTail}[t]
        assert isinstance(last, want) and (last.B, last.H, last.W) == (B, H // 2, H // 2)
    for t in V.RECONSTRUCT_TAILS:
        lst = lists["reconstruct_" + t]
        assert [o for o in as_oracle_ops(lst)] == enc_ops + dec_ops, t
        post = [i for i, e in enumerate(lst) if isinstance(e, V.Posterior)]
        assert post == [len(lists["encode"])] and lst[post[0]] == V.Posterior(B, (H // 8) ** 2, 0)


@pytest.mark.parametrize("B,H,W", V.IMG_CONFIGS + [V.IMG_WORKLOAD])
def test_image_vae_list_is_what_the_oracle_executes(recorder, B, H, W):
    from ldmseg_amd import weights
    from oracle import vae_image as o_img
    sd = meta_sd(weights.vae_image_schema())
    mom = o_img.encode_moments(sd, torch.empty(B, 3, H, W, device="meta"))
    assert tuple(mom.shape) == (B, 8, H // 8, W // 8)
    got = fold_attention_linears(list(recorder))
    lst = V.img_lists(B, H, W)["encode"]
    assert got == as_oracle_ops(lst)
    assert sum(isinstance(e, V.Softmax) for e in lst) == B and sum(isinstance(e, V.Gemm) for e in lst) == 3 * B


def test_lists_hold_the_forms_the_issue_names():
    """the launch forms the per-launch tests exist for are in the lists at the GPU configurations"""
    img = V.distinct({str(c): V.img_encode(*c) for c in V.IMG_CONFIGS})
    seg = V.distinct({f"{c}{k}": l for c in V.SEG_CONFIGS for k, l in V.seg_lists(*c).items()})
    down = [e for e in img if isinstance(e, V.Conv) and e.pad == 0]
    assert down and all(e.stride == 2 and e.k == 3 for e in down) and any(e.H != e.W for e in down)
    assert any(isinstance(e, V.GroupNorm) and e.C == 128 for e in img)                      # 4 channels per group
    assert {e.N for e in img if isinstance(e, V.Gemm) and e.rows_f32} == {64, 128, 192}
    assert any(isinstance(e, V.Conv) and (e.Ci, e.Co, e.stride, e.silu, e.tile) == (32, 64, 2, 1, 1) for e in seg)
    assert any(isinstance(e, V.Conv) and (e.Ci, e.Co, e.epi) == (256, 8, "nchw_f32") for e in seg)
    assert any(isinstance(e, V.Conv) and (e.Ci, e.Co) == (4, 256) for e in seg)
    assert any(isinstance(e, V.ConvT) and 4 * e.Co == 1024 for e in seg)
    assert any(isinstance(e, V.LayerNorm) and e.inplace for e in seg)
    assert any(isinstance(e, V.Posterior) and not e.noise for e in seg)
    assert any(isinstance(e, V.BilinearArgmax) for e in seg)
    assert any(e.H % 8 for e in seg if isinstance(e, V.Conv))                                 # (1, 40, 40): maps 20 / 10 / 5


MODES = {"bf16": V.BF16, "fp32": V.F32, "bf16x3": V.X3W}


def planned_names(lib, entries, dt, cus):
    from igemm_desc import plan
    names = {}
    for e in entries:
        if isinstance(e, (V.Conv, V.ConvT, V.Gemm)):
            desc, pdt = V.igemm_desc(e, dt)
            r, line = plan(lib, desc, pdt, cus)
            assert r == 0, (e, dt, r)
            names.setdefault(line.split(" ")[0], e)
    return names


def workload_plan(mode):
    """{name: first entry} planned in one mode at the workload size, by every case the GPU tests run, by the configurations' own lists"""
    from ldmseg_amd import _lib
    lib = _lib.lib()
    cus = json.load(open(os.path.join(GOLDEN, "gn_dispatch.json")))["cus"]
    assert lib.ldmseg_debug_get(1) == lib.ldmseg_debug_get(-1), "a tile policy is set"
    dt = MODES[mode]
    work = V.distinct(V.seg_lists(*V.SEG_WORKLOAD)) + V.distinct(V.img_lists(*V.IMG_WORKLOAD))
    own = []
    for c in V.SEG_CONFIGS:
        own += V.distinct(V.seg_lists(*c))
    for c in V.IMG_CONFIGS:
        own += V.distinct(V.img_lists(*c))
    return planned_names(lib, work, dt, cus), planned_names(lib, list(V.EXTRA_CASES) + own, dt, cus), planned_names(lib, own, dt, cus)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_workload_instantiations_are_planned_by_a_gpu_case(mode):
    """Every igemm instantiation the chooser plans for the lists at the workload size (seg-VAE H = 512, image VAE 512 x 512, B = 1,
    on the CU count of tests/golden/gn_dispatch.json) is also planned by a case the GPU tests run: an entry of the lists at
    SEG_CONFIGS / IMG_CONFIGS or one of vae_cases.EXTRA_CASES."""
    want, have, own = workload_plan(mode)
    missing = {n: e for n, e in want.items() if n not in have}
    assert not missing, f"{mode}: planned at the workload size only: {missing}"
    assert own and len(want) >= 4
    if mode == "bf16x3":
        assert all(",x3" in n for n in want), sorted(want)


def test_every_extra_case_plans_a_workload_instantiation_the_lists_miss():
    """no dead weight in vae_cases.EXTRA_CASES: each plans, in some mode, an instantiation of the workload that the configurations' own
    lists do not"""
    from ldmseg_amd import _lib
    lib = _lib.lib()
    cus = json.load(open(os.path.join(GOLDEN, "gn_dispatch.json")))["cus"]
    gaps = {}
    for mode, dt in MODES.items():
        want, _, own = workload_plan(mode)
        gaps[dt] = set(want) - set(own)
    assert any(gaps.values())
    for e in V.EXTRA_CASES:
        assert any(set(planned_names(lib, [e], dt, cus)) & gaps[dt] for dt in MODES.values()), e


@pytest.mark.parametrize("rounded", [False, True])
def test_argmax_reference_leaves_out_at_most_one_percent(rounded):
    """the inputs of the GPU argmax comparison, judged by the reference alone: the pixels whose two largest fp64 logits lie within the
    interpolation's rounding of each other (left out there) stay under the cap, for fp32 logits and for bf16-stored ones (where
    exact ties exist)"""
    shapes = {(e.B, e.C, e.H, e.W) for c in V.SEG_CONFIGS for l in V.seg_lists(*c).values() for e in l if isinstance(e, V.BilinearArgmax)}
    assert len(shapes) == len(V.SEG_CONFIGS)
    for B, C, H, W in sorted(shapes):
        x = V.argmax_case(B, C, H, W, seed=H)
        if rounded:
            x = x.to(torch.bfloat16).float()
        ids, prob, keep = V.argmax_reference(x)
        left_out = 1.0 - float(keep.double().mean())
        assert left_out <= V.ARGMAX_LEFT_OUT_CAP, (B, C, H, W, rounded, left_out)
        assert ids.shape == (B, 2 * H, 2 * W) and len(ids.unique()) > 8 and float(prob.min()) > 0

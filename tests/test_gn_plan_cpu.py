"""The GroupNorm launch chooser (csrc/gn_plan.h) without a GPU.

``ldmseg_op_groupnorm_plan`` / ``ldmseg_op_conv_groupnorm_plan`` answer, for a described launch, the names the dispatch log holds
after the real one.  tests/golden/gn_dispatch.json holds what the library decided on an MI355X before the chooser was factored out
of the launcher (tools/record_gn_dispatch.py over the shapes of tests/gn_cases.py: every GroupNorm shape of
tests/test_igemm_shapes_gpu.py at its own and the off-grid configurations, every GroupNorm case of tests/test_ops_gpu.py, a grid
of small shapes, both dtypes, nine values of debug key 8) and the chooser has to return every one of those answers exactly.
(tests/test_ops_gpu.py::test_groupnorm_plan_equals_launch ties the export to real launches and pins their output bytes.)"""
import json
import os
import re

import pytest

from conftest import GOLDEN

import gn_cases as G

KEYS = {8: 0, 11: 100}          # the debug keys with a getter that the chooser / launcher read, and their shipped values
REQUIRED = (["gn_group<bf16,10,2>", "gn_group<bf16,20,2>", "gn_one<bf16,6,GB=2>"]
            + [f"gn_coop<bf16,21,512,GB={g}>" for g in (1, 2, 4)] + [f"gn_coop<f32,21,512,GB={g}>" for g in (1, 2)]
            + [f"gn_one<{t},{m},GB=1>" for t in ("bf16", "f32") for m in (2, 6, 12)]
            + [f"gn_fused<{t},22,GB={g}>" for t in ("bf16", "f32") for g in (1, 2)]
            + [f"gn_small<{t},12>" for t in ("bf16", "f32")] + [f"gn_apply<{t}> + gn_partial<{t}>" for t in ("bf16", "f32")])


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(GOLDEN, "gn_dispatch.json")))


def test_fixture_covers_the_rule(fx):
    assert tuple(fx["variants"]) == G.VARIANTS and fx["cus"] == 256          # an MI355X
    nv = len(G.VARIANTS)
    assert all(len(r[-1]) == nv for r in fx["gn"] + fx["conv"])
    assert (len(fx["gn"]) + len(fx["conv"])) * nv >= 2000
    assert {tuple(r[:4]) for r in fx["gn"]} == set(G.gn_shapes()) and {tuple(r[:3]) for r in fx["conv"]} == set(G.conv_gn_shapes())
    names = set(fx["names"][i] for r in fx["gn"] + fx["conv"] for i in r[-1] if i >= 0)
    assert not [n for n in REQUIRED if n not in names]
    for m in (2, 6, 12):
        assert any(re.fullmatch(rf"finish_gn<(bf16|f32),{m},GB=[12]>", n) for n in names), m
    # rejections: channels per group below a vector without the two-group case, a source that is not whole vectors (the third
    # cause - more than 32 groups on the two-launch path - cannot be recorded: the operator always normalises 32 groups;
    # test_chooser_rejects_what_the_launcher_rejects asks the chooser directly)
    rec = {(tuple(r[:4]), r[4]): r[-1] for r in fx["gn"]}
    assert set(rec[(4, 32, 0, 64), G.F32]) == {-2} and set(rec[(4, 64, 0, 64), G.BF16]) == {-2} and min(rec[(4, 64, 0, 64), G.F32]) >= 0
    assert set(rec[(2, 316, 4, 256), G.BF16]) == {-2} and min(rec[(2, 316, 4, 256), G.F32]) >= 0
    assert any(-4 in r[-1] for r in fx["conv"])


def test_case_lists_cover_the_gpu_suites():
    from test_igemm_shapes_gpu import CONFIGS, CONV_GN_SHAPES, GN_SHAPES
    from test_offgrid_shapes_gpu import OFFGRID
    assert G.CONFIGS == CONFIGS and G.OFFGRID == OFFGRID
    assert {(h, c, c2) for h, c, c2, _, _ in GN_SHAPES} == set(G.GN_LEVELS)
    assert {(h, co) for h, _, co in CONV_GN_SHAPES} == set(G.CONV_GN_LEVELS)


def test_chooser_returns_every_recorded_dispatch(lib, fx):
    assert all(lib.ldmseg_debug_get(k) == v for k, v in KEYS.items()), "a previous test leaked a knob"
    wrong = []
    try:
        for vi, v in enumerate(fx["variants"]):
            assert lib.ldmseg_debug_set(8, v) == 0
            for what, recs, ask in (("gn", fx["gn"], lambda a: G.plan(lib, *a, fx["cus"])), ("conv", fx["conv"], lambda a: G.conv_plan(lib, *a))):
                for r in recs:
                    ni = r[-1][vi]
                    want = (0, fx["names"][ni].split(" + ")) if ni >= 0 else (ni, [])
                    code, line = ask(r[:-1])
                    if (code, sorted(G.plan_names(line))) != want:        # (the dispatch log keeps distinct names, sorted)
                        wrong.append((what, r[:-1], v, want, (code, line)))
    finally:
        for k, v in KEYS.items():
            lib.ldmseg_debug_set(k, v)
    assert not wrong, (len(wrong), wrong[:5])
    assert all(lib.ldmseg_debug_get(k) == v for k, v in KEYS.items())


def test_restated_ladder_examples(lib):
    """the examples of the rule at 256 CUs that the recording is expected to contain (the recording is the authority)"""
    first = lambda *a, **kw: G.plan(lib, *a, 256, **kw)[1].split(" ")[0]
    assert first(4, 128, 0, 16, G.BF16) == "gn_small<bf16,12>"
    assert first(4, 256, 0, 400, G.BF16) == "gn_group<bf16,10,2>"
    assert first(3, 256, 0, 100, G.BF16) == "gn_one<bf16,2,GB=1>"
    assert G.plan(lib, 1, 256, 0, 100, G.BF16, 256)[1].startswith("gn_partial<bf16> + gn_apply<bf16> ")
    assert G.plan(lib, 1, 320, 0, 4096, G.BF16, 256)[1].startswith("gn_coop<bf16,21,512,GB=4> splits=8 ")
    try:
        lib.ldmseg_debug_set(8, 37)
        assert first(4, 256, 0, 400, G.BF16) == "gn_fused<bf16,22,GB=1>"
    finally:
        lib.ldmseg_debug_set(8, 0)


def test_chooser_rejects_what_the_launcher_rejects(lib):
    # the two-launch path combines 32 groups at most; the other forms take up to 64
    assert G.plan(lib, 1, 512, 0, 100, G.BF16, 256, groups=64)[0] == -2
    assert G.plan(lib, 1, 512, 0, 100, G.BF16, 256, groups=32)[1].startswith("gn_partial<bf16> + gn_apply<bf16> ")
    assert G.plan(lib, 4, 512, 0, 100, G.BF16, 256, groups=64)[1].startswith("gn_one<bf16,2,GB=1> ")
    assert G.plan(lib, 4, 1040, 0, 100, G.BF16, 256, groups=65)[0] == -2
    # no hand-off region: no cooperative kernel at any group block, the rest of the rule applies
    assert G.plan(lib, 1, 320, 0, 4096, G.BF16, 256, region_ok=0)[1].startswith("gn_partial<bf16> + gn_apply<bf16> ")
    assert G.plan(lib, 8, 640, 0, 1024, G.F32, 256, region_ok=0)[1].startswith("gn_fused<f32,22,GB=1> ")
    # the cooperative grid is bound by the CU count
    assert G.plan(lib, 8, 640, 0, 1024, G.F32, 256)[1] == "gn_coop<f32,21,512,GB=1> splits=1 grid=256x1 block=512"
    assert G.plan(lib, 8, 640, 0, 1024, G.F32, 255)[1] == "gn_coop<f32,21,512,GB=2> splits=1 grid=128x1 block=512"
    assert G.plan(lib, 8, 640, 0, 1024, G.F32, 127)[1].startswith("gn_fused<f32,22,GB=1> ")
    assert G.conv_plan(lib, 8, 320, 64, G.BF16)[0] == -4 and G.conv_plan(lib, 8, 1280, 64, G.BF16)[0] == 0

"""The LayerNorm / row-statistics launch chooser (csrc/ln_plan.h) without a GPU.

``ldmseg_op_layernorm_plan`` answers, for a described launch, the name the dispatch log holds after the real one.
tests/golden/ln_dispatch.json holds what the library decided on an MI355X before the chooser was factored out of the launchers
(tools/record_ln_dispatch.py over the cases of tests/ln_cases.py) and the chooser has to return every one of those answers exactly.
(tests/test_ops_gpu.py::test_layernorm_plan_equals_launch ties the export to real launches.)"""
import json
import os

import pytest

from conftest import GOLDEN

import ln_cases as G

# every name launch_ln_plan (csrc/norm.hip) can emit
REQUIRED = ([f"layernorm<{t},{v}>" for t in ("bf16", "f32") for v in ("1,4", "2,4", "3,2", "5,1")]
            + [f"layernorm<{t},{v},stats>" for t in ("bf16", "f32") for v in ("1,4", "2,4", "3,2", "5,2")]
            + [f"rowstats<{t},{lanes},2>" for t in ("bf16", "f32") for lanes in (8, 16, 32, 64)])


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(GOLDEN, "ln_dispatch.json")))


def test_fixture_covers_the_rule(fx):
    assert [tuple(c[:5]) for c in fx["cases"]] == G.ln_cases() and fx["cus"] == 256          # an MI355X
    rec = {tuple(c[:5]): c[5] for c in fx["cases"]}
    names = {v for v in rec.values() if isinstance(v, str)}
    assert sorted(names) == sorted(REQUIRED)
    # both refusals: a row that is not whole 16-byte vectors (12 channels: bf16 only), and one wider than 5 vectors per lane of a
    # wave, normalised and - at 328 vectors, under either value of key 8 - as statistics (a failed step of ldmseg_op_ln_linear: -3)
    for key8 in G.KEY8:
        assert rec[1, 6, G.F32, 0, key8] == rec[1, 6, G.BF16, 0, key8] == rec[9, 12, G.BF16, 0, key8] == -2
        assert rec[9, 12, G.F32, 0, key8] == "layernorm<f32,1,4>"
        for dt in (G.F32, G.BF16):
            assert rec[9, 320 * G.PC[dt], dt, 0, key8].endswith(",5,1>") and rec[9, 321 * G.PC[dt], dt, 0, key8] == -2
            assert rec[9, 320 * G.PC[dt], dt, 1, key8] in names and rec[9, G.WIDE_STATS_C[dt], dt, 1, key8] == -3
    # the grid-stride loop of the narrowest forms ran
    assert rec[2048 * 16 + 9, 8, G.BF16, 0, 0] == "layernorm<bf16,1,4>" and rec[4096 * 64 + 9, 64, G.BF16, 1, 0] == "rowstats<bf16,8,2>"
    assert rec[2048 * 16 + 9, 32, G.F32, 1, 16] == "layernorm<f32,1,4,stats>"


def test_chooser_returns_every_recorded_dispatch(lib, fx):
    assert lib.ldmseg_debug_get(8) == 0, "a previous test leaked a knob"
    wrong = []
    try:
        for M, C_, dt, stats, key8, want in fx["cases"]:
            assert lib.ldmseg_debug_set(8, key8) == 0
            code, line = G.plan(lib, M, C_, dt, stats)
            if (code, G.plan_name(line)) != ((0, want) if isinstance(want, str) else (-2, "")):
                wrong.append(((M, C_, dt, stats, key8), want, (code, line)))
    finally:
        lib.ldmseg_debug_set(8, 0)
    assert not wrong, (len(wrong), wrong[:5])
    assert lib.ldmseg_debug_get(8) == 0


def test_restated_grid_examples(lib):
    """the grids of the rule: rows per four-wave workgroup and trip, capped at 2048 (a wave per row) / 4096 (lanes share a row)"""
    assert G.plan(lib, 77, 320, G.BF16, 0)[1] == "layernorm<bf16,1,4> grid=5 block=256"
    assert G.plan(lib, 1 << 20, 2560, G.BF16, 0)[1] == "layernorm<bf16,5,1> grid=2048 block=256"
    assert G.plan(lib, 32768, 320, G.BF16, 1)[1] == "rowstats<bf16,8,2> grid=512 block=256"
    assert G.plan(lib, 1 << 20, 1280, G.F32, 1)[1] == "rowstats<f32,64,2> grid=4096 block=256"
    assert G.plan(lib, 0, 320, G.BF16, 0)[1] == "layernorm<bf16,1,4> grid=1 block=256"

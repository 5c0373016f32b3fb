"""The igemm tile chooser (csrc/igemm_plan.h) without a GPU.

``ldmseg_op_igemm_plan`` answers, for a described launch, the string ``ldmseg_igemm_last_kernel`` reports after the real one.
tests/golden/igemm_dispatch.json holds what the library decided on an MI355X before the chooser was factored out of the launcher
- every launch shape of tests/test_igemm_shapes_gpu.py at its own and at the off-grid configurations, in bf16, fp32 and the
plane-split mode, plus every value of the tile-policy, forced-entry, K-order, extra-tap, phase-conv, in-launch-finish and
table-override knobs that a test or tuning tool sets, at the shapes of each map level - and the chooser has to return every one
of those strings exactly.  (tests/test_ops_gpu.py::test_igemm_plan_equals_launch ties the export to real launches.)

(tests/igemm_desc.py restates how each operator of csrc/ops_api.hip turns its arguments into a launch description.)"""
import json
import os

import pytest

from conftest import GOLDEN

from igemm_desc import BF16, F32, FIELDS, X3W, make_desc, desc_conv3x3_plus_1x1, plan

KEYS = (1, 5, 9, 19, 21, 23, 24)          # ldmseg_debug_set keys the chooser reads
UNSET = {5: -1, 24: -1}                   # the two without a getter: their shipped value


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def test_chooser_returns_every_recorded_dispatch(lib):
    fx = json.load(open(os.path.join(GOLDEN, "igemm_dispatch.json")))
    assert tuple(fx["fields"]) == FIELDS and tuple(fx["keys"]) == KEYS
    assert len(fx["parent"]) == 40 and len(fx["records"]) > 2000
    shipped = dict(zip(KEYS, fx["shipped"]))
    assert all(lib.ldmseg_debug_get(k) == shipped[k] for k in KEYS if k not in UNSET), "a previous test leaked a knob"
    wrong = []
    try:
        state = None
        for di, dt, ki, ni in sorted(fx["records"], key=lambda r: r[2]):
            if ki != state:
                for k, v in zip(KEYS, fx["knobs"][ki]):
                    assert lib.ldmseg_debug_set(k, v) == 0
                state = ki
            want = (0, fx["names"][ni]) if ni >= 0 else (-2, "")
            got = plan(lib, fx["descs"][di], dt, fx["cus"])
            if got != want:
                wrong.append((dict(zip(FIELDS, fx["descs"][di])), dt, dict(zip(KEYS, fx["knobs"][ki])), want, got))
    finally:
        for k in KEYS:
            lib.ldmseg_debug_set(k, shipped[k])
    assert not wrong, (len(wrong), wrong[:5])
    for k in KEYS:
        if k not in UNSET:
            assert lib.ldmseg_debug_get(k) == shipped[k], k
    assert shipped[1] == lib.ldmseg_debug_get(-1) and all(shipped[k] == v for k, v in UNSET.items())


@pytest.mark.parametrize("what,desc,dt", [
    ("GEGLU with N % 128 != 0", make_desc(M=2048, N=2720, C0=1280, epi=1), BF16),
    ("an extra tap in fp32", desc_conv3x3_plus_1x1(8, 640, 320, 0, 32, 32, 640, 1), F32),
    ("up4 with M % 1024 != 0", make_desc(M=4 * 3 * 24 * 24, N=640, C0=640, taps=4, up4=1), BF16),
    ("LayerNorm folded on a 64-column split-bf16 tile", make_desc(M=2048, N=64, C0=320, lnf=1), X3W),    # no such instantiation
])
def test_chooser_rejects_what_launch_igemm_rejects(lib, what, desc, dt):
    assert plan(lib, desc, dt, 256)[0] == -2, what
    ok = list(desc)                       # the neighbouring valid launch is planned: the -2 is the check's, not a bad description
    if "GEGLU" in what:
        ok[FIELDS.index("N")] = 2560
    elif "fp32" in what:
        dt = BF16
    elif "LayerNorm" in what:
        ok[FIELDS.index("N")] = 160
    else:
        ok[FIELDS.index("M")] = 4 * 4 * 16 * 16
    r, s = plan(lib, ok, dt, 256)
    assert r == 0 and s.startswith("igemm<"), (what, r, s)

"""CPU suite: the learning-rate tables of ldmseg_amd/trainers/lr_schedules.py equal, to the bit, the arrays the reference's
cosine_scheduler / warmup_scheduler / step_scheduler returned (tests/golden/lr_schedules.npz, written by
tests/golden/make_golden_lr_schedules.py; the fixture carries every case's arguments)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "lr_schedules.npz"))


def _functions():
    from ldmseg_amd.trainers import lr_schedules as S
    return {"cosine": S.cosine_scheduler, "warmup": S.warmup_scheduler, "step": S.step_scheduler}


def test_fixture_holds_the_cases_the_schedules_are_checked_on(fixture):
    cases = json.loads(str(fixture["cases"]))
    for fn in ("cosine", "warmup", "step"):
        for w in (None, 0, 5):
            f, args, kw, keep = cases[f"{fn}/3x7/warmup_{w}"]
            assert f == fn and args[2:] == [3, 7] and kw["warmup_iters"] == w and keep is None
        f, args, kw, keep = cases[f"{fn}/base"]
        assert args[0] == 1e-4 and kw["warmup_iters"] == 200 and keep == 300 and fixture[f"{fn}/base"].shape == (300,)


def test_every_table_equals_the_reference_functions_array_to_the_bit(fixture):
    fns = _functions()
    cases = json.loads(str(fixture["cases"]))
    assert len(cases) >= 15
    for name, (fn, args, kw, keep) in cases.items():
        got = fns[fn](*args, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (args[2] * args[3],), name
        want = fixture[name]
        got = got if keep is None else got[:keep]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, np.abs(got - want).max())


def test_warm_up_ends_at_the_base_value_and_the_tables_have_their_shapes():
    fns = _functions()
    for fn in fns.values():
        t = fn(1e-4, 1e-6, 3, 7, warmup_iters=5)
        assert t[0] == 0.0 and t[4] == 1e-4 and t[5] == 1e-4 and len(t) == 21
    assert fns["cosine"](1e-4, 1e-6, 3, 7)[-1] > 1e-6                       # the cosine stops one iteration short of final_value
    assert np.all(fns["warmup"](1e-4, 1e-6, 3, 7) == 1e-4)
    s = fns["step"](1.0, 0.0, 3, 7, decay_epochs=[1, 2], decay_rate=0.5)
    assert list(s[[0, 6, 7, 13, 14, 20]]) == [1.0, 1.0, 0.5, 0.5, 0.25, 0.25]
    with pytest.raises(ValueError):
        fns["warmup"](1e-4, 1e-6, 1, 3, warmup_iters=5)                    # a warm-up longer than the run

"""The weight-gradient launch chooser (csrc/wgrad_plan.h) without a GPU: ``ldmseg_op_wgrad_plan`` answers, for a described launch,
the tile, the slicing of the pixel axis and the grid.  Properties the decoder's backward relies on."""
import pytest

import vae_backward_ref as R

STEP, MIN_STEPS, TARGET = 32, 8, 256


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def _all_descs():
    out = []
    for name, B, L in R.ALL_SHAPES + [("seg", 8, 64)]:            # + the workload
        out += R.wgrad_descs(name, B, L)
    return sorted(set(out))


def _ints(f):
    per, steps = f["steps"].split("/")
    return dict(tiles=int(f["tiles"]), slices=int(f["slices"]), per=int(per), steps=int(steps), grid=int(f["grid"]),
                one=int(f["one_per_cu"]))


@pytest.mark.parametrize("x3", [0, 1])
def test_every_shape_gets_a_plan_and_slices_cover_the_pixels_once(lib, x3):
    for P, N, C, taps in _all_descs():
        code, line, f = R.wgrad_plan(lib, P, N, C, taps, x3)
        assert code == 0, (P, N, C, taps)
        assert line.startswith(f"wgrad<{'x3' if x3 else 'f32'},128,128>/taps{taps} ")
        q = _ints(f)
        assert q["steps"] == -(-P // STEP)
        assert q["tiles"] == -(-N // 128) * -(-C // 128) * taps
        # slice s takes steps [s * per, min(steps, (s + 1) * per)): together every step exactly once, none empty
        assert (q["slices"] - 1) * q["per"] < q["steps"] <= q["slices"] * q["per"]
        covered = sum(min(q["steps"], (s + 1) * q["per"]) - s * q["per"] for s in range(q["slices"]))
        assert covered == q["steps"]
        # a slice is worth a workgroup only from MIN_STEPS steps on, and the items aim at the target
        assert q["slices"] == 1 or (q["steps"] // q["slices"] >= MIN_STEPS and q["tiles"] * q["slices"] <= TARGET)


def test_grid_is_at_most_the_cu_count_where_one_item_per_cu(lib):
    for cus in (256, 304, 64, 8):
        for P, N, C, taps in _all_descs():
            q = _ints(R.wgrad_plan(lib, P, N, C, taps, 0, cus)[2])
            items = q["tiles"] * q["slices"]
            if q["one"]:
                assert q["grid"] == items <= cus
            else:
                assert items > cus and q["grid"] == cus


def test_reduction_order_is_a_function_of_the_shape_alone(lib):
    """slices and steps per slice - the order every addition of the result is made in - do not move with the device or the mode"""
    for P, N, C, taps in _all_descs():
        seen = set()
        for cus in (8, 64, 256, 304):
            for x3 in (0, 1):
                f = R.wgrad_plan(lib, P, N, C, taps, x3, cus)[2]
                seen.add((f["tiles"], f["slices"], f["steps"]))
        assert len(seen) == 1, (P, N, C, taps, seen)


def test_refusals(lib):
    assert R.wgrad_plan(lib, 0, 128, 256, 9)[0] == -2
    assert R.wgrad_plan(lib, 64, 128, 256, 4)[0] == -2           # taps 9 or 1
    assert R.wgrad_plan(lib, 64, 24, 256, 9)[0] == -2            # columns come as 16-channel fragments
    assert R.wgrad_plan(lib, 64, 128, 256, 9, 0, 0)[0] == -2


def test_multi_slice_case_is_the_smallest(lib):
    """R.MULTI_SLICE is the smallest (fewest logits pixels, then smallest batch; B <= 3) shape of the real decoder whose last conv's
    weight gradient runs as more than one pixel slice; the regular shapes up to it run as one"""
    best = None
    for L in range(1, 33):
        for B in (1, 2, 3):
            P, N, C, taps = R.last_conv_wgrad_desc("seg", B, L)
            if int(R.wgrad_plan(lib, P, N, C, taps)[2]["slices"]) > 1 and (best is None or (P, B) < best[0]):
                best = ((P, B), ("seg", B, L))
    assert best[1] == R.MULTI_SLICE
    name, B, L = R.MULTI_SLICE
    assert int(R.wgrad_plan(lib, *R.last_conv_wgrad_desc(name, B, L))[2]["slices"]) == 2
    # and the workload's last conv is cut into as many slices as fill the target
    f = R.wgrad_plan(lib, *R.last_conv_wgrad_desc("seg", 8, 64))[2]
    assert f["tiles"] == "18" and f["slices"] == "14" and f["one_per_cu"] == "1"

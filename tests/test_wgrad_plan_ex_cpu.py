"""The by-width weight-gradient chooser (csrc/wgrad_plan.h wgrad_choose) without a GPU: ``ldmseg_op_wgrad_plan_ex``
answers, for a launch of the encoder's backward, the tile (32 | 64 | 128 rows of dY by 32 | 64 | 128 channels of X), the slicing of
the OUTPUT map's pixel axis and the grid.  The decoder's rule (``ldmseg_op_wgrad_plan``) is restated here and held unchanged."""
import pytest

import vae_backward_ref as RD
import vae_encode_backward_ref as R
import wgrad_cases as WC

STEP, MIN_STEPS, TARGET = 32, 8, 256
WORKLOAD = ("seg", 8, 512)


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def _all_descs():
    out = []
    for name, B, H in R.SHAPES + [WORKLOAD]:
        out += R.wgrad_descs(name, B, H)
    return sorted(set(out))


def _ints(f):
    per, steps = f["steps"].split("/")
    return dict(tiles=int(f["tiles"]), slices=int(f["slices"]), per=int(per), steps=int(steps), grid=int(f["grid"]), one=int(f["one_per_cu"]))


def _tile(width):
    return 32 if width <= 32 else 64 if width <= 64 else 128


def _all_taps(N, C, taps):
    """a 3x3 layer whose two widths fit 64: one workgroup owns the nine taps of the tile (N x 9 C outputs)"""
    return taps == 9 and N <= 64 and C <= 64


def test_executed_macs_are_at_most_twice_the_layers_own():
    """for each of the nine encoder convs of the default configuration: tiles x tile area x taps <= 2 x the MACs of (N, C) rounded
    up to 32 (the 128 x 128 tile alone executes 16 x on encoder.2 and 4 x on the head)"""
    from ldmseg_amd import _lib
    lib = _lib.lib()
    descs = R.wgrad_descs(*WORKLOAD)
    assert len(descs) == 9
    for P, N, C, taps, stride in descs:
        for x3 in (0, 1):
            code, line, f, macs = R.wgrad_plan_ex(lib, P, N, C, taps, stride, x3)
            assert code == 0, (P, N, C, stride)
            own = N * C * taps                       # N, C are the storage widths: already multiples of 32
            assert macs == _ints(f)["tiles"] * (taps if _all_taps(N, C, taps) else 1) * _tile(N) * _tile(C)      # tiles x tile area x taps
            assert macs <= 2 * own, (line, macs, own)
    # the two full-resolution layers, encoder.3 and encoder.5 own all nine taps; the wide layers keep one tile per tap
    names = [R.wgrad_plan_ex(lib, P, N, C, taps, stride)[1].split()[0] for P, N, C, taps, stride in descs]
    assert names == ["wgrad9<f32,32,32>/taps9", "wgrad9<f32,32,32>/taps9", "wgrad9<f32,64,32>/taps9/s2", "wgrad9<f32,64,64>/taps9",
                     "wgrad<f32,128,64>/taps9/s2", "wgrad<f32,128,128>/taps9", "wgrad<f32,128,128>/taps9/s2", "wgrad<f32,128,128>/taps9",
                     "wgrad<f32,32,128>/taps9"]


@pytest.mark.parametrize("x3", [0, 1])
def test_every_shape_gets_a_plan_and_no_slice_is_empty(lib, x3):
    for P, N, C, taps, stride in _all_descs():
        code, line, f, _ = R.wgrad_plan_ex(lib, P, N, C, taps, stride, x3)
        assert code == 0, (P, N, C, taps, stride)
        nine = _all_taps(N, C, taps)
        name = f"wgrad{'9' if nine else ''}<{'x3' if x3 else 'f32'},{_tile(N)},{_tile(C)}>/taps{taps}" + ("/s2" if stride == 2 else "")
        assert line.split()[0] == name, line
        q = _ints(f)
        assert q["steps"] == -(-P // STEP)
        assert q["tiles"] == -(-N // _tile(N)) * -(-C // _tile(C)) * (1 if nine else taps)
        assert (q["slices"] - 1) * q["per"] < q["steps"] <= q["slices"] * q["per"]          # the last slice is not empty
        covered = sum(min(q["steps"], (s + 1) * q["per"]) - s * q["per"] for s in range(q["slices"]))
        assert covered == q["steps"]
        assert q["slices"] == 1 or (q["steps"] // q["slices"] >= MIN_STEPS and q["tiles"] * q["slices"] <= TARGET)


def test_plans_differ_across_cu_counts_in_the_grid_alone(lib):
    for P, N, C, taps, stride in _all_descs():
        seen = set()
        for cus in (8, 64, 256, 304):
            for x3 in (0, 1):
                line, f = R.wgrad_plan_ex(lib, P, N, C, taps, stride, x3, cus)[1:3]
                q = _ints(f)
                assert q["grid"] == (q["tiles"] * q["slices"] if q["one"] else cus) <= cus
                seen.add((line.split()[0].replace("x3", "f32"), f["tiles"], f["slices"], f["steps"], f["block"]))
        assert len(seen) == 1, (P, N, C, taps, stride, seen)


def test_gpu_shapes_hold_a_single_slice_and_a_multi_slice_full_resolution_layer(lib):
    """encoder.2 (32 -> 32 at full resolution) runs as one slice at the smallest GPU shape and as several at the others"""
    slices = {}
    for name, B, H in R.SHAPES:
        P, N, C, taps, stride = R.wgrad_descs(name, B, H)[1]
        assert (P, N, C, stride) == (B * H * H, 32, 32, 1)
        slices[name, B, H] = int(R.wgrad_plan_ex(lib, P, N, C, taps, stride)[2]["slices"])
    assert slices["seg", 1, 16] == 1
    assert slices["seg", 2, 24] > 1 and slices["seg", 3, 40] > 1


def _names(lib, descs, x3):
    return {R.wgrad_plan_ex(lib, P, N, C, taps, stride, x3)[1].split()[0] for P, N, C, taps, stride in descs}


def _names_before(lib, x3):
    """kernel names of the launches the suite compared with fp64 before tests/wgrad_cases.py had lists of its own: NARROW, STRIDE2
    and the two encoder configurations at the shapes of tests/test_vae_encode_backward_gpu.py"""
    descs = [WC.desc(B, Ci, Co, H, W, 1) for B, Ci, Co, H, W in WC.NARROW] + [WC.desc(B, Ci, Co, H, W, 2) for B, Ci, Co, H, W in WC.STRIDE2]
    for name, B, H in R.SHAPES:
        descs += R.wgrad_descs(name, B, H)
    assert {name for name, _, _ in R.SHAPES} == set(R.CONFIGS)
    return _names(lib, descs, x3)


@pytest.mark.parametrize("x3", [0, 1])
def test_every_kernel_the_chooser_can_name_has_a_gpu_case(lib, x3):
    """ldmseg_op_wgrad_plan_ex over every pair of storage widths 32 .. 1024 of a 3x3 layer, both strides: 18 kernel names per mode,
    each of them launched and compared with fp64 by a GPU test - a kernel added to the chooser without a case fails here.
    The per-tap form with BOTH tiles <= 64 (4 tile pairs x 2 strides x 2 modes = 16 instantiations) is not built: the chooser gives
    every such 3x3 layer the all-taps tile and no entry passes the by-width rule with one tap, so launch_wgrad's table has no row
    for them and the enumeration never names them."""
    fam = "x3" if x3 else "f32"
    named = set()
    for stride in (1, 2):
        for N in range(32, 1025, 32):
            for C in range(32, 1025, 32):
                code, line, _, _ = R.wgrad_plan_ex(lib, 1152, N, C, 9, stride, x3)
                assert code == 0, (N, C, stride)
                named.add(line.split()[0])
    print(f"{fam}: {len(named)} kernel names: " + " ".join(sorted(named)))
    assert len(named) == 18
    for tn in (32, 64):
        for tc in (32, 64):
            for s2 in ("", "/s2"):
                assert f"wgrad<{fam},{tn},{tc}>/taps9{s2}" not in named and f"wgrad9<{fam},{tn},{tc}>/taps9{s2}" in named
    before = _names_before(lib, x3)
    oracle = _names(lib, [WC.desc(*s) for s in WC.launches()], x3)          # tests/test_wgrad_kernels_gpu.py, against fp64
    missing = {f"wgrad9<{fam},64,32>/taps9", f"wgrad9<{fam},32,64>/taps9/s2", f"wgrad<{fam},64,128>/taps9", f"wgrad<{fam},64,128>/taps9/s2",
               f"wgrad<{fam},128,32>/taps9", f"wgrad<{fam},128,32>/taps9/s2", f"wgrad<{fam},128,64>/taps9", f"wgrad<{fam},32,128>/taps9/s2"}
    assert len(before) == 10 and named - before == missing
    assert missing <= oracle
    assert named == before | oracle, sorted(named ^ (before | oracle))
    assert named == _names(lib, [WC.desc(*s) for s in WC.walk_launches()], x3)        # and each has a multi-slice item-walk case


def test_the_multi_slice_maps_are_cut_into_four_slices_and_the_wide_case_outnumbers_the_cus(lib):
    for shape in WC.launches() + WC.walk_launches():
        f = _ints(R.wgrad_plan_ex(lib, *WC.desc(*shape))[2])
        if (shape[0], shape[3], shape[4]) == WC.ODD:
            assert f["slices"] == 1
        else:
            assert f["slices"] == 4 and f["steps"] == 36, shape
    B, H, W = WC.ODD
    f = _ints(R.wgrad_plan_ex(lib, *WC.desc(B, WC.BIG[0], WC.BIG[1], H, W, WC.BIG[2]))[2])
    assert f["tiles"] == 270 and f["one"] == 0 and f["grid"] == 256


def test_the_chooser_cu_key_reads_back_and_counts_negative_values_as_zero(lib):
    """debug key 26 (the CU count handed to the chooser; tests/test_wgrad_kernels_gpu.py): default 0 = the device's"""
    try:
        assert lib.ldmseg_debug_get(26) == 0
        assert lib.ldmseg_debug_set(26, 7) == 0 and lib.ldmseg_debug_get(26) == 7
        assert lib.ldmseg_debug_set(26, -3) == 0 and lib.ldmseg_debug_get(26) == 0
    finally:
        lib.ldmseg_debug_set(26, 0)


def test_refusals(lib):
    assert R.wgrad_plan_ex(lib, 64, 64, 32, 1, 2)[0] == -2        # stride 2 is a 3x3 conv's
    assert R.wgrad_plan_ex(lib, 64, 64, 32, 9, 3)[0] == -2
    assert R.wgrad_plan_ex(lib, 0, 64, 32, 9, 1)[0] == -2
    assert R.wgrad_plan_ex(lib, 64, 24, 32, 9, 1)[0] == -2


def _decoder_line(P, N, C, taps, x3, cus):
    """the decoder's rule as DESIGN 8.6 states it: the 128 x 128 tile"""
    tiles = -(-N // 128) * -(-C // 128) * taps
    steps = -(-P // STEP)
    want = max(1, min(TARGET // tiles, steps // MIN_STEPS))
    per = -(-steps // want)
    slices = -(-steps // per)
    items = tiles * slices
    one = 1 if items <= cus else 0
    return (f"wgrad<{'x3' if x3 else 'f32'},128,128>/taps{taps} tiles={tiles} slices={slices} steps={per}/{steps} "
            f"grid={items if one else cus} block=256 one_per_cu={one}")


def test_the_decoders_plan_lines_are_unchanged(lib):
    descs = set()
    for name, B, L in RD.ALL_SHAPES + [("seg", 8, 64)]:
        descs |= set(RD.wgrad_descs(name, B, L))
    for P, N, C, taps in sorted(descs):
        for x3 in (0, 1):
            for cus in (64, 256, 304):
                assert RD.wgrad_plan(lib, P, N, C, taps, x3, cus)[1] == _decoder_line(P, N, C, taps, x3, cus)

"""The fused candidate kernels of the sizes whose horizontal filter pass has the 4x4x4-block matrix form
(rdo_mc_matrix4_layout, rdo_cand_plan.hpp: 8 bits, 16x16 -- four candidates per wave -- and 8x8 -- eight), bit for bit
against the oracle's r1o_rdo_cand_batch: prediction, SAD, SATD and coefficients.  The families are those of
test_gpu_mc_matrix.py, built for what this form can get wrong: every block of four lanes carries its own candidate's
taps, so within every run of NC candidates all col_frac and mode_x differ; accumulators at both ends of their range;
windows in the padding; launches whose last wave is not full; and whatever lies behind a window in LDS (the next
candidate's window, the staged source block).  Everything goes through the public entry point, so the tests hold for a
size whether its kernel takes the matrix form or the v_dot4 one."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_mc_matrix import (PH, PW, REGULAR, SHARP, SHORT, SMOOTH, blank, check, oracle_run, planes,
                                range_ends)
from test_mc_matrix_layout import BIAS, HALF

pytestmark = pytest.mark.gpu

SIZES = [pytest.param(16, 16, 2, id="16x16"), pytest.param(8, 8, 1, id="8x8")]   # (w, h, tx_size)


def runs_differ(c, nc, *fields):
    """within every aligned run of nc candidates (a wave), all values of each field differ"""
    for f in fields:
        v = np.sort(c[f].reshape(-1, nc), axis=1)
        if not (v[:, 1:] != v[:, :-1]).all():
            return False
    return True


@pytest.mark.parametrize("my", range(4), ids=["y_regular", "y_smooth", "y_sharp", "y_bilinear"])
@pytest.mark.parametrize("w,h,ts", SIZES)
def test_filter_grid(ctx, oracle, w, h, ts, my):
    """all 16 col_frac x all four mode_x, crossed with row_frac {0, 1, 8, 15}.  A wave is four candidates (16x16): all
    four col_frac and all four mode_x differ.  Or eight (8x8): all eight col_frac differ, and each half of the wave holds
    all four mode_x (there are only four filter sets)"""
    org, ref = planes()
    nc = 64 // w
    i = np.arange(256)
    c = blank(256, w, h, np.random.default_rng(10 * w + my))
    c["col_frac"] = i % 16
    c["mode_x"] = (i // 16 + i) % 4
    c["row_frac"] = np.array([0, 1, 8, 15])[i // 64]
    c["mode_y"] = my
    seen = {(int(a), int(b), int(r)) for a, b, r in zip(c["col_frac"], c["mode_x"], c["row_frac"])}
    assert len(seen) == 16 * 4 * 4
    assert runs_differ(c, nc, "col_frac") and runs_differ(c, 4, "mode_x")
    check(ctx, org, ref, w, h, ts, c)


@pytest.mark.parametrize("w,h,ts", SIZES)
def test_wave_composition(ctx, oracle, w, h, ts):
    """waves (runs of NC candidates) whose filters are all six-tap, all SHARP, and mixed inside a wave on either axis"""
    org, ref = planes()
    nc = 64 // w
    rng = np.random.default_rng(300 + w)
    runs = 96
    c = blank(runs * nc, w, h, rng)
    run = np.repeat(np.arange(runs), nc)
    kind = run % 4                                        # 0 short, 1 sharp, 2 sharp on x only, 3 sharp on y only
    short = lambda: rng.choice(SHORT, len(c))
    c["mode_x"] = np.where((kind == 1) | (kind == 2), SHARP, short())
    c["mode_y"] = np.where((kind == 1) | (kind == 3), SHARP, short())
    # mixed inside a wave: every eighth run alternates SHARP / REGULAR on x and the reverse on y, slot by slot
    alt = run % 8 == 7
    even = np.arange(len(c)) % 2 == 0
    c["mode_x"] = np.where(alt, np.where(even, SHARP, REGULAR), c["mode_x"])
    c["mode_y"] = np.where(alt, np.where(even, REGULAR, SHARP), c["mode_y"])
    waves = c.reshape(-1, nc)
    ny, nx = (waves["mode_y"] == SHARP).sum(axis=1), (waves["mode_x"] == SHARP).sum(axis=1)
    assert ((ny > 0) & (ny < nc)).any() and ((nx > 0) & (nx < nc)).any()        # mixed on either axis
    assert (ny == 0).any() and (ny == nc).any() and ((nx == nc) & (ny == 0)).any() and ((nx == 0) & (ny == nc)).any()
    check(ctx, org, ref, w, h, ts, c)


@pytest.mark.parametrize("mode", [SHARP, SMOOTH], ids=["sharp", "smooth"])
@pytest.mark.parametrize("w,h,ts", SIZES)
def test_accumulator_extremes(ctx, oracle, w, h, ts, mode):
    """reference planes of 0 / 255 chosen by tap sign (period 8 in x; even rows for the top of the range, odd rows for
    the bottom) drive the horizontal accumulator of the set's widest rows to both ends (-7106 / 23494 over the two sets,
    test_gpu_mc_matrix.py::test_the_two_filter_sets_span_the_accumulator_range)"""
    org, _ = planes()
    lo, cf_lo, hi, cf_hi = range_ends(mode)
    nc = 64 // w
    for cf, end in ((cf_hi, hi), (cf_lo, lo)):
        taps = HALF[mode, cf]
        ref = O.HostPlane(PW, PH, 8, fill=0)
        x = np.arange(ref.stride)
        top = np.where(taps[(x - ref.xorigin) % 8] > 0, 255, 0)      # column 0 of a window at rx = 3 (mod 8)
        ref.data[0::2] = top
        ref.data[1::2] = 255 - top
        n = 6 * nc + 1
        c = blank(n, w, h, np.random.default_rng(400 + w + cf))
        c["col_frac"], c["mode_x"] = cf, mode
        c["rx"][: 4 * nc] = 3 + 8 * (np.arange(4 * nc) % 16)         # aligned with the pattern; the rest anywhere
        c["ry"][: 4 * nc] = np.arange(4 * nc)
        win = ref.data[ref.yorigin + c["ry"][0] - 3: ref.yorigin + c["ry"][0] + h + 4,
                       ref.xorigin + c["rx"][0] - 3: ref.xorigin + c["rx"][0] + w + 4].astype(np.int64) - 128
        acc = BIAS + sum(taps[t] * win[:, t: t + w] for t in range(8))
        assert end in (int(acc.max()), int(acc.min())) and acc.min() >= -7106 and acc.max() <= 23494
        check(ctx, org, ref, w, h, ts, c)


@pytest.mark.parametrize("w,h,ts", SIZES)
def test_windows_in_the_padding(ctx, oracle, w, h, ts):
    """rx, ry from -50 to 50 past the far edges: the window lies partly or wholly in the padding"""
    org, ref = planes()
    rng = np.random.default_rng(500 + w)
    c = blank(256, w, h, rng)
    c["rx"] = rng.integers(-50, PW - w + 51, 256)
    c["ry"] = rng.integers(-50, PH - h + 51, 256)
    c["rx"][:4], c["ry"][:4] = (-50, PW - w + 50, -50, PW - w + 50), (-50, -50, PH - h + 50, PH - h + 50)
    check(ctx, org, ref, w, h, ts, c)


@pytest.mark.parametrize("w,h,ts", SIZES)
def test_counts(ctx, oracle, w, h, ts):
    """n = 1, n = NC + 1 and n = 8 NC + 3: the last wave's repeated slots and the grid rounding"""
    org, ref = planes()
    nc = 64 // w
    c = blank(8 * nc + 3, w, h, np.random.default_rng(600 + w))
    want = oracle_run(org, ref, w, h, ts, c)
    for n in (1, nc + 1, 8 * nc + 3):
        check(ctx, org, ref, w, h, ts, c, want, n)


@pytest.mark.parametrize("w,h,ts", SIZES)
def test_prediction_ignores_what_lies_behind_the_window(ctx, oracle, w, h, ts):
    """the last quad's fragments read one row past the window -- the next candidate's window, the staged source block
    for the last one: the same reference windows with other source blocks, other partners and in every slot of the wave
    give the same pred"""
    org, ref = planes()
    nc = 64 // w
    rng = np.random.default_rng(700 + w)
    n = 128
    c = blank(n, w, h, rng)
    base = check(ctx, org, ref, w, h, ts, c)["pred"]
    moved = c.copy()
    moved["ox"] = (c["ox"] + 1 + rng.integers(0, PW - w, n)) % (PW - w + 1)
    moved["oy"] = (c["oy"] + 1 + rng.integers(0, PH - h, n)) % (PH - h + 1)
    assert ((moved["ox"] != c["ox"]) | (moved["oy"] != c["oy"])).all()
    assert np.array_equal(check(ctx, org, ref, w, h, ts, moved)["pred"], base)
    other = c.copy()                                      # slot 0 of every wave keeps its candidate, the partners change
    keep = np.arange(n) % nc == 0
    other[~keep] = blank(n - n // nc, w, h, rng)
    assert np.array_equal(check(ctx, org, ref, w, h, ts, other)["pred"][keep], base[keep])
    for k in range(1, nc):                                # every candidate in every other slot of a wave
        shifted = np.concatenate([blank(k, w, h, rng), c])
        assert np.array_equal(check(ctx, org, ref, w, h, ts, shifted)["pred"][k:], base)

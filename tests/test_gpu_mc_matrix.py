"""The fused candidate kernels whose horizontal filter pass runs on the matrix pipe (rdo_mc_matrix, rdo_cand_plan.hpp:
8 bits, 64x64 -- one candidate per wave -- and 32x32 -- two), bit for bit against the oracle's r1o_rdo_cand_batch:
prediction, SAD, SATD and coefficients.  The lists are built for what that pass can get wrong: every horizontal tap
row against a spread of vertical ones, the composition of a wave (the two candidates of a 32x32 wave feed different B
fragments), accumulators at both ends of their range, windows in the padding, launches whose last wave is not full,
and whatever lies behind the window in LDS (the source block, the partner's window)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_compound as TC
from test_mc_matrix_layout import BIAS, HALF

pytestmark = pytest.mark.gpu

PW, PH = 192, 160                    # pads 88 (HostPlane's default)
REGULAR, SMOOTH, SHARP, BILINEAR = 0, 1, 2, 3
SHORT = (REGULAR, SMOOTH, BILINEAR)
SIZES = [pytest.param(64, 64, 4, id="64x64"), pytest.param(32, 32, 3, id="32x32")]   # (w, h, tx_size)


@functools.lru_cache(maxsize=None)
def planes():
    rng = np.random.default_rng(2200)
    return O.HostPlane(PW, PH, 8, rng=rng), O.HostPlane(PW, PH, 8, rng=rng)


def blank(n, w, h, rng):
    """n candidates with source blocks and windows inside the visible area, fractions and modes random"""
    c = np.zeros(n, O.RDO_CAND)
    c["ox"] = rng.integers(0, PW - w + 1, n)
    c["oy"] = rng.integers(0, PH - h + 1, n)
    c["rx"] = rng.integers(0, PW - w + 1, n)
    c["ry"] = rng.integers(0, PH - h + 1, n)
    c["col_frac"] = rng.integers(0, 16, n)
    c["row_frac"] = rng.integers(0, 16, n)
    c["mode_x"] = rng.integers(0, 4, n)
    c["mode_y"] = rng.integers(0, 4, n)
    return c


def oracle_run(org, ref, w, h, ts, c):
    n = len(c)
    po, pr = org.cstruct(), ref.cstruct()
    want = {"sad": np.zeros(n, np.uint32), "satd": np.zeros(n, np.uint32), "coeffs": np.zeros((n, w * h), np.int16),
            "pred": np.zeros((n, h, w), np.uint8)}
    assert O.lib().r1o_rdo_cand_batch(C.byref(po), C.byref(pr), w, h, ts, O.ptr(c), n, O.ptr(want["sad"]),
                                      O.ptr(want["satd"]), O.ptr(want["coeffs"]), O.ptr(want["pred"])) == 0
    return want


def device_run(ctx, org, ref, w, h, c):
    o = ctx.rdo_cand_batch(TC.dev_plane(org), TC.dev_plane(ref), w, h, c, want_pred=True)
    return {"pred": o["pred"].cpu().numpy().view(np.uint8).reshape(len(c), h, w),
            "sad": o["sad"].cpu().numpy().view(np.uint32), "satd": o["satd"].cpu().numpy().view(np.uint32),
            "coeffs": o["coeffs"].cpu().numpy()}


def check(ctx, org, ref, w, h, ts, c, want=None, n=None):
    """all four outputs of the first n candidates, bit for bit; returns the device's"""
    want = want or oracle_run(org, ref, w, h, ts, c)
    n = len(c) if n is None else n
    got = device_run(ctx, org, ref, w, h, c[:n])
    for k in ("pred", "sad", "satd", "coeffs"):
        bad = np.nonzero((got[k] != want[k][:n]).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, (k, "%d of %d candidates differ, first %d: %s" % (bad.size, n, bad[0], c[bad[0]]))
    return got


@pytest.mark.parametrize("my", range(4), ids=["y_regular", "y_smooth", "y_sharp", "y_bilinear"])
@pytest.mark.parametrize("w,h,ts", SIZES)
def test_filter_grid(ctx, oracle, w, h, ts, my):
    """all 16 col_frac x all four mode_x, crossed with row_frac {0, 1, 8, 15}; neighbours in the list -- the two
    candidates of a 32x32 wave -- differ in col_frac AND mode_x"""
    org, ref = planes()
    i = np.arange(256)
    c = blank(256, w, h, np.random.default_rng(10 * w + my))
    c["col_frac"] = i % 16
    c["mode_x"] = (i // 16 + i) % 4
    c["row_frac"] = np.array([0, 1, 8, 15])[i // 64]
    c["mode_y"] = my
    seen = {(int(a), int(b), int(r)) for a, b, r in zip(c["col_frac"], c["mode_x"], c["row_frac"])}
    assert len(seen) == 16 * 4 * 4
    assert (c["col_frac"][0::2] != c["col_frac"][1::2]).all() and (c["mode_x"][0::2] != c["mode_x"][1::2]).all()
    check(ctx, org, ref, w, h, ts, c)


@pytest.mark.parametrize("w,h,ts", SIZES)
def test_wave_composition(ctx, oracle, w, h, ts):
    """waves (runs of NC candidates) whose filters are all six-tap, all SHARP, and mixed on either axis"""
    org, ref = planes()
    nc = 64 // w
    rng = np.random.default_rng(300 + w)
    runs = 96
    c = blank(runs * nc, w, h, rng)
    kind = np.repeat(np.arange(runs) % 4, nc)            # 0 short, 1 sharp, 2 sharp on x only, 3 sharp on y only
    short = lambda: rng.choice(SHORT, len(c))
    c["mode_x"] = np.where((kind == 1) | (kind == 2), SHARP, short())
    c["mode_y"] = np.where((kind == 1) | (kind == 3), SHARP, short())
    if nc > 1:                                            # mixed inside a wave: every eighth run alternates
        alt = (np.repeat(np.arange(runs), nc) % 8 == 7) & (np.arange(len(c)) % 2 == 0)
        c["mode_x"] = np.where(alt, SHARP, c["mode_x"])
        c["mode_y"] = np.where(alt, REGULAR, c["mode_y"])
        pairs = c.reshape(-1, 2)
        mixed = ((pairs["mode_y"] == SHARP).sum(axis=1) == 1)
        assert mixed.any() and ((pairs["mode_x"][:, 0] != pairs["mode_x"][:, 1]) &
                                (pairs["col_frac"][:, 0] != pairs["col_frac"][:, 1])).any()
    assert all((kind == k).any() for k in range(4))
    check(ctx, org, ref, w, h, ts, c)


def range_ends(mode):
    """(lowest accumulator, its col_frac, highest, its col_frac) of a filter set over all windows of 8-bit pixels"""
    lo = [int(BIAS - 128 * h[h > 0].sum() + 127 * h[h < 0].sum()) for h in HALF[mode]]
    hi = [int(BIAS + 127 * h[h > 0].sum() - 128 * h[h < 0].sum()) for h in HALF[mode]]
    return min(lo), int(np.argmin(lo)), max(hi), int(np.argmax(hi))


def test_the_two_filter_sets_span_the_accumulator_range():
    ends = [range_ends(m) for m in (SHARP, SMOOTH)]
    assert (min(e[0] for e in ends), max(e[2] for e in ends)) == (-7106, 23494)


@pytest.mark.parametrize("mode", [SHARP, SMOOTH], ids=["sharp", "smooth"])
@pytest.mark.parametrize("w,h,ts", SIZES)
def test_accumulator_extremes(ctx, oracle, w, h, ts, mode):
    """reference planes of 0 / 255 chosen by tap sign (period 8 in x; even rows for the top of the range, odd rows for
    the bottom) drive the horizontal accumulator of the set's widest rows to both ends"""
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
        c["rx"][: 4 * nc] = 3 + 8 * np.arange(4 * nc)                # aligned with the pattern; the rest anywhere
        c["ry"][: 4 * nc] = np.arange(4 * nc)
        # the accumulators these windows produce do reach the end
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
    """n = 1, n = NC + 1 and n not a multiple of 8 NC: the last wave's repeated slots and the grid rounding"""
    org, ref = planes()
    nc = 64 // w
    c = blank(8 * nc + 3, w, h, np.random.default_rng(600 + w))
    want = oracle_run(org, ref, w, h, ts, c)
    for n in (1, nc + 1, 8 * nc + 3):
        check(ctx, org, ref, w, h, ts, c, want, n)


@pytest.mark.parametrize("w,h,ts", SIZES)
def test_prediction_ignores_what_lies_behind_the_window(ctx, oracle, w, h, ts):
    """the A fragments read past the window -- the staged source block, at 32x32 the partner's window: the same
    reference windows with other source blocks, other partners and the other slot of the wave give the same pred"""
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
    if nc == 2:
        other = c.copy()                                  # every odd slot gets another candidate
        other[1::2] = blank(n // 2, w, h, rng)
        assert np.array_equal(check(ctx, org, ref, w, h, ts, other)["pred"][0::2], base[0::2])
        shifted = np.concatenate([blank(1, w, h, rng), c])      # every candidate in the other slot of its wave
        assert np.array_equal(check(ctx, org, ref, w, h, ts, shifted)["pred"][1:], base)

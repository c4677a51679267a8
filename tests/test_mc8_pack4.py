"""The shift-free pack of the 8-bit motion compensation (mc8_column_t<.., PACK4>, rav1e_amd/csrc/cand_common.hpp) on
the host.  The horizontal accumulator of a window row is

    hacc = sum_k h[k] * (p[k] - 128) + 8192 + 2 + 32 = 4 * mid' + fraction,     h = taps / 2,

the old form packs mid' = hacc >> 2 of two rows as i16 x 2, the new one clears the two fraction bits of each half of
the packed low words and carries 4 * mid'.  That is exact if hacc fits i16 (its low 16 bits are then the value), and
the vertical v_dot2 sums, four times the old ones, must fit i32; >> 13 then returns the bits of >> 11.  Checked over
every row of the project's tap table (kSubpel, mc_common.hpp), and by a NumPy model of both forms against the
oracle's put_8tap on windows of 0 / 255 chosen per tap sign -- the windows that drive the accumulators to their
extremes -- for every filter pair and every fraction pair, zero fractions and SHARP (the eight-tap path) included."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = 8192 + 2 + 32
N = 8                       # block side of the model: 8 x 8 output pixels from a 15 x 15 window


def _table():
    src = open(os.path.join(ROOT, "rav1e_amd", "csrc", "mc_common.hpp")).read()
    m = re.search(r"kSubpel\[6\]\[16\]\[8\] = \{(.*?)\};", src, re.S)
    t = np.array([int(v) for v in re.findall(r"-?\d+", m.group(1))], np.int64).reshape(6, 16, 8)
    assert (t.sum(axis=2) == 128).all() and (t % 2 == 0).all()
    return t


TAB = _table()


def hacc_range(taps):
    """[min, max] of the horizontal accumulator over all windows of 8-bit pixels"""
    h = taps // 2
    pos, neg = h[h > 0].sum(), h[h < 0].sum()
    return int(pos * -128 + neg * 127 + BIAS), int(pos * 127 + neg * -128 + BIAS)


def test_accumulator_fits_i16_for_every_row_of_the_table():
    lo = min(hacc_range(TAB[f, q])[0] for f in range(6) for q in range(16))
    hi = max(hacc_range(TAB[f, q])[1] for f in range(6) for q in range(16))
    assert (lo, hi) == (-7106, 23494)
    assert -32768 <= lo and hi <= 32767
    # the frac-0 row (128 at tap 3, h = 64) is one of them: the copy and the 1-D cases go through the same path
    assert hacc_range(TAB[0, 0]) == (64 * -128 + BIAS, 64 * 127 + BIAS)


def test_vertical_sum_fits_i32():
    worst = 0
    for fx in range(6):
        for qx in range(16):
            lo, hi = hacc_range(TAB[fx, qx])
            lo4, hi4 = lo & ~3, hi & ~3            # 4 * mid'
            for fy in range(6):
                for qy in range(16):
                    u = TAB[fy, qy]
                    up, un = int(u[u > 0].sum()), int(u[u < 0].sum())
                    worst = max(worst, abs(up * hi4 + un * lo4), abs(up * lo4 + un * hi4))
    assert worst < (1 << 31)
    assert worst == 4720576 and worst < (1 << 23)      # a 23-bit magnitude: nowhere near the accumulator's width


def model(win, xt, yt):
    """both column forms of mc8_column_t on a (..., 15, 15) window of 8-bit pixels -> (old, new), (..., 8, 8)"""
    q = win.astype(np.int32) - 128
    h = (xt // 2).astype(np.int32)
    acc = np.full(q.shape[:-1] + (N,), BIAS, np.int32)
    for k in range(8):
        acc = acc + h[k] * q[..., k:k + N]
    assert acc.min() >= -32768 and acc.max() <= 32767
    mid = (acc >> 2).astype(np.int16).astype(np.int32)                               # ashr_pair: i16 halves
    m4 = (acc.astype(np.uint32) & 0xFFFF & 0xFFFC).astype(np.uint16).view(np.int16).astype(np.int32)   # perm, and
    a_old = np.zeros(q.shape[:-2] + (N, N), np.int64)
    a_new = np.zeros_like(a_old)
    for k in range(8):
        a_old += int(yt[k]) * mid[..., k:k + N, :]
        a_new += int(yt[k]) * m4[..., k:k + N, :]
    assert (a_new == 4 * a_old).all() and np.abs(a_new).max() < (1 << 31)
    return np.clip(a_old >> 11, 0, 255).astype(np.uint8), np.clip(a_new >> 13, 0, 255).astype(np.uint8)


def extreme_windows(xt, yt):
    """four 15 x 15 windows: 255 where the tap that output pixel (0, 0) puts on the pixel has the wanted sign on each
    axis, 0 elsewhere (period 8: the other output pixels meet the pattern shifted) -- and two flat ones"""
    sx = np.resize(np.where(xt >= 0, 1, -1), 15)
    sy = np.resize(np.where(yt >= 0, 1, -1), 15)
    wins = []
    for gx in (1, -1):
        for gy in (1, -1):
            wins.append(np.where(np.outer(sy * gy, sx * gx) > 0, 255, 0))
    # rows alone / columns alone: the extremes of hacc itself under a flat vertical filter
    wins.append(np.where(np.outer(np.ones(15, int), sx) > 0, 255, 0))
    wins.append(np.where(np.outer(np.ones(15, int), -sx) > 0, 255, 0))
    wins.append(np.full((15, 15), 255))
    wins.append(np.zeros((15, 15), int))
    return np.array(wins, np.uint8)


@pytest.fixture(scope="module")
def oracle():
    return O.lib()


@pytest.mark.parametrize("my", range(4), ids=["y_regular", "y_smooth", "y_sharp", "y_bilinear"])
@pytest.mark.parametrize("mx", range(4), ids=["x_regular", "x_smooth", "x_sharp", "x_bilinear"])
def test_both_forms_are_put_8tap_on_extreme_windows(oracle, mx, my):
    """8 x 8 blocks: get_filter takes the table row of the mode itself (mc.rs:238-247), as the fused kernels' sizes do"""
    compared = 0
    seen_lo, seen_hi = 1 << 30, -(1 << 30)
    want = np.zeros((N, N), np.uint8)
    for cf in range(16):
        for rf in range(16):
            xt, yt = TAB[mx, cf], TAB[my, rf]
            wins = extreme_windows(xt, yt)
            old, new = model(wins, xt, yt)
            assert np.array_equal(old, new), (mx, my, cf, rf)
            for i, w in enumerate(wins):
                w = np.ascontiguousarray(w)
                src = w.ctypes.data + 3 * 15 + 3
                oracle.r1o_put_8tap(O.ptr(want), N, src, 15, N, N, cf, rf, mx, my, 8, 0)
                assert np.array_equal(new[i], want), (mx, my, cf, rf, i)
                compared += want.size
            lo, hi = hacc_range(xt)
            seen_lo, seen_hi = min(seen_lo, lo), max(seen_hi, hi)
    assert compared == 16 * 16 * 8 * N * N
    assert -32768 <= seen_lo and seen_hi <= 32767


def test_the_extreme_windows_reach_the_accumulator_range():
    """the sign-chosen windows do drive hacc to the ends hacc_range computes (SHARP, fraction 8: the widest row)"""
    xt = TAB[2, 8]
    wins = extreme_windows(xt, TAB[3, 0])
    q = wins.astype(np.int32) - 128
    acc = sum((xt[k] // 2) * q[..., k:k + N] for k in range(8)) + BIAS
    lo, hi = hacc_range(xt)
    assert acc.max() == hi and acc.min() == lo


def test_kernel_text_states_the_form_modelled_here():
    txt = open(os.path.join(ROOT, "rav1e_amd", "csrc", "cand_common.hpp")).read()
    assert "return pk_pair(hacc(r), hacc(r + 1)) & 0xfffcfffcu;" in txt
    assert "a0 >>= PACK4 ? 13 : 11;" in txt and "a1 >>= PACK4 ? 13 : 11;" in txt
    assert "constexpr int32_t bias = 8192 + 2 + (PREP ? 0 : 32);" in txt
    assert 'static_assert(!(PREP && PACK4)' in txt

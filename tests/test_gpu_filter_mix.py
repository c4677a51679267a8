"""The wave-uniform choice between the 6-tap and the 8-tap form of the fast column filter (taps_six and
mc8_column_t / mc16_column_t in cand_common.hpp, k_mc_mfma in mc_mfma.hip), pinned by construction.  A wave of the fast kernels owns NC = 64 / max(w, h) consecutive
candidates and takes the short form only when every one of them has zero outer taps, so the lists here come in
aligned runs of NC: all {REGULAR, SMOOTH, BILINEAR}, all SHARP, a mix, SHARP on one axis only, and a last wave that
is not full.  Every entry point on that filter is compared bit for bit with the oracle: put / prep, the matrix-core
twin, the compound candidate and the fused candidate."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_compound as TC

pytestmark = pytest.mark.gpu

PW, PH, SLACK = 96, 80, 60          # windows cross the padding (88 px) on every side
REGULAR, SMOOTH, SHARP, BILINEAR = 0, 1, 2, 3
SHORT = (REGULAR, SMOOTH, BILINEAR)  # zero outer taps at every fraction
# (w, h, tx_size): the 4-tap index rule and TS = 4; the two axes under different index rules; 8 candidates per wave;
# packed groups of 16 rows and the fused kernel's tile SATD
SHAPES = [(4, 4, 0), (4, 8, 5), (8, 8, 1), (16, 16, 2)]
DEPTHS = [8, 10, 12]
RUNS = ("short", "sharp", "mixed", "sharp_x", "sharp_y")


def run_modes(kind, nc, rng):
    """(mode_x, mode_y) of the nc candidates of one run"""
    short = lambda: rng.choice(SHORT, nc)
    if kind == "short":
        return short(), short()
    if kind == "sharp":
        return np.full(nc, SHARP), np.full(nc, SHARP)
    if kind == "mixed":
        alt = np.arange(nc) % 2 == 0
        return np.where(alt, SHARP, short()), np.where(alt, short(), SHARP)
    if kind == "sharp_x":
        return np.full(nc, SHARP), short()
    return short(), np.full(nc, SHARP)


@functools.lru_cache(maxsize=None)
def case(bd, w, h):
    """the planes, the candidate list and the oracle's put / prep of one (bit depth, shape), made once"""
    rng = np.random.default_rng(1000 * bd + 10 * w + h)
    org, ref, ref1 = (O.HostPlane(PW, PH, bd, rng=rng) for _ in range(3))
    nc = 64 // max(w, h)
    n = len(RUNS) * nc + max(1, nc // 2)                # the last wave is not full
    c = np.zeros(n, O.MC_CAND)
    c["rx"] = rng.integers(-SLACK, PW - w + SLACK + 1, n)
    c["ry"] = rng.integers(-SLACK, PH - h + SLACK + 1, n)
    c["col_frac"] = rng.integers(1, 16, n)
    c["row_frac"] = rng.integers(1, 16, n)
    for r in range(len(RUNS) + 1):                      # the four structural cases at the head of every run
        c["col_frac"][r * nc: r * nc + 4: 2] = 0        # (0, 0), (f, 0), (0, f), (f, f)
        c["row_frac"][r * nc: r * nc + 2] = 0
    for r, kind in enumerate(RUNS):
        c["mode_x"][r * nc: (r + 1) * nc], c["mode_y"][r * nc: (r + 1) * nc] = run_modes(kind, nc, rng)
    c["mode_x"][len(RUNS) * nc:] = rng.choice(SHORT, n - len(RUNS) * nc)
    c["mode_y"][len(RUNS) * nc:] = rng.choice(SHORT, n - len(RUNS) * nc)
    check_input(c, nc)
    pr = ref.cstruct()
    put = np.zeros((n, h, w), TC.px_dtype(bd))
    prep = np.zeros((n, h, w), np.int16)
    assert O.lib().r1o_mc_put_batch(C.byref(pr), w, h, O.ptr(c), n, O.ptr(put)) == 0
    assert O.lib().r1o_mc_prep_batch(C.byref(pr), w, h, O.ptr(c), n, O.ptr(prep)) == 0
    for a in (put, prep):                               # shared among the tests, left as they are
        a.setflags(write=False)
    return (org, ref, ref1), c, put, prep


def check_input(c, nc):
    """what the list is built for, so that an edit cannot empty a class"""
    runs = [c[r * nc: (r + 1) * nc] for r in range(len(RUNS))]
    short = lambda m: np.isin(m, SHORT)
    assert all(len(r) == nc for r in runs) and len(c) % nc != 0
    assert short(runs[0]["mode_x"]).all() and short(runs[0]["mode_y"]).all()
    assert (runs[1]["mode_x"] == SHARP).all() and (runs[1]["mode_y"] == SHARP).all()
    for f in ("mode_x", "mode_y"):
        assert (runs[2][f] == SHARP).any() and short(runs[2][f]).any()
    assert (runs[3]["mode_x"] == SHARP).all() and short(runs[3]["mode_y"]).all()
    assert short(runs[4]["mode_x"]).all() and (runs[4]["mode_y"] == SHARP).all()
    for r in runs:
        for f in ("col_frac", "row_frac"):
            assert (r[f] == 0).any() and (r[f] != 0).any()


CASES = [pytest.param(bd, w, h, ts, id="%dbit-%dx%d" % (bd, w, h)) for bd in DEPTHS for (w, h, ts) in SHAPES]


@pytest.mark.parametrize("bd,w,h,ts", CASES)
def test_put_prep(ctx, oracle, bd, w, h, ts):
    (_, ref, _), c, put, prep = case(bd, w, h)
    d = TC.dev_plane(ref)
    assert np.array_equal(ctx.put_8tap_batch(d, w, h, c).cpu().numpy().view(TC.px_dtype(bd)), put)
    assert np.array_equal(ctx.prep_8tap_batch(d, w, h, c).cpu().numpy(), prep)


@pytest.mark.parametrize("s", [8, 16])
def test_mfma_twin(ctx, oracle, s):
    (_, ref, _), c, put, prep = case(8, s, s)
    d = TC.dev_plane(ref)
    assert np.array_equal(ctx.mc_batch_mfma(d, s, s, c).cpu().numpy(), put)
    assert np.array_equal(ctx.mc_batch_mfma(d, s, s, c, prep=True).cpu().numpy(), prep)


@pytest.mark.parametrize("bd,w,h,ts", CASES)
def test_compound(ctx, oracle, bd, w, h, ts):
    from rav1e_amd.api import COMPOUND_CAND
    planes, m, _, _ = case(bd, w, h)
    n = len(m)
    rng = np.random.default_rng(7 * bd + w + h)
    c = np.zeros(n, COMPOUND_CAND)
    c["ox"] = rng.integers(0, PW - w + 1, n)
    c["oy"] = rng.integers(0, PH - h + 1, n)
    # the second reference: the first one's list turned by one candidate inside each run, so that both columns of a
    # lane see every fraction case and the modes (one pair per candidate) keep their runs
    nc = 64 // max(w, h)
    turn = np.arange(n) // nc * nc + (np.arange(n) % nc + 1) % nc
    turn[turn >= n] = len(RUNS) * nc
    for i, src in enumerate((m, m[turn])):
        c["rx%d" % i], c["ry%d" % i] = src["rx"], src["ry"]
        c["col_frac%d" % i], c["row_frac%d" % i] = src["col_frac"], src["row_frac"]
    c["mode_x"], c["mode_y"] = m["mode_x"], m["mode_y"]
    TC.check_all(ctx, oracle, planes, [TC.dev_plane(p) for p in planes], w, h, c, TC.ALL3)


@pytest.mark.parametrize("bd,w,h,ts", CASES)
def test_fused_candidate(ctx, oracle, bd, w, h, ts):
    (org, ref, _), m, put, _ = case(bd, w, h)
    n = len(m)
    rng = np.random.default_rng(11 * bd + w + h)
    c = np.zeros(n, O.RDO_CAND)
    c["ox"] = rng.integers(0, PW - w + 1, n)
    c["oy"] = rng.integers(0, PH - h + 1, n)
    for f in ("rx", "ry", "col_frac", "row_frac", "mode_x", "mode_y"):
        c[f] = m[f]
    po, pr = org.cstruct(), ref.cstruct()
    wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    wco = np.zeros((n, w * h), np.int16 if bd == 8 else np.int32)
    wpred = np.zeros((n, h, w), TC.px_dtype(bd))
    assert oracle.r1o_rdo_cand_batch(C.byref(po), C.byref(pr), w, h, ts, O.ptr(c), n, O.ptr(wsad), O.ptr(wsatd),
                                     O.ptr(wco), O.ptr(wpred)) == 0
    assert np.array_equal(wpred, put)                   # the oracle agrees with itself
    o = ctx.rdo_cand_batch(TC.dev_plane(org), TC.dev_plane(ref), w, h, c, want_pred=True)
    assert np.array_equal(o["pred"].cpu().numpy().view(TC.px_dtype(bd)), wpred)
    assert np.array_equal(o["sad"].cpu().numpy().view(np.uint32), wsad)
    assert np.array_equal(o["satd"].cpu().numpy().view(np.uint32), wsatd)
    assert np.array_equal(o["coeffs"].cpu().numpy(), wco)

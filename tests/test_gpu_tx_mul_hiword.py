"""The fused candidate kernels' high-word multiplies (m24w, tx_common.hpp; rdo_mul_hiword, rdo_cand_plan.hpp) on the
device: r1_rdo_cand_batch at 8 bits against the scalar oracle, bit for bit on SAD, SATD and every coefficient, at 8x8 /
16x16 / 32x32 / 64x64 on a 128x128 plane pair, launches of 11 / 7 / 3 / 2 candidates (a wave owns 8 / 4 / 2 / 1: the
last wave of the first three repeats a slot).

Random leg: random planes, motion vectors, fractions, filters and transform types.

Sign-pattern leg: planes of 0 / 255 pixels whose difference is +-255 in the sign pattern tests/golden/fwd_tx_ref.npz
keeps for the (size, type) -- the pattern that drives that network's intermediates furthest -- and its negative, zero
motion vector and zero fraction, so the prediction is the reference block and the residual is the pattern at full
scale.  Every type the size admits: one launch per type (every wave of one type: the scalar switch between the 1-D
kernels), then launches with a different type in every candidate of a wave (8x8, 16x16; DCT / IDTX at 32x32: the
per-lane switch).  Each leg counts what it compared."""
import ctypes as C
import functools

import numpy as np
import pytest

import fwd_tx_ref_util as U
import oracle_lib as O
from test_gpu_parity import dev_plane

pytestmark = pytest.mark.gpu

BD = 8
SIDES = {1: 8, 2: 16, 3: 32, 4: 64}                         # TxSize id -> side
COUNT = {1: 11, 2: 7, 3: 3, 4: 2}                           # candidates per launch
TYPES = {1: list(range(16)), 2: list(range(16)), 3: [0, 9], 4: [0]}
PW = PH = 128


def _slot(ts, j):
    """top-left of the j-th pattern block of a size: block 2 k is type k's pattern, 2 k + 1 its negative"""
    n = SIDES[ts]
    return (j % (PW // n)) * n, (j // (PW // n)) * n


@functools.lru_cache(maxsize=None)
def _pattern_planes(ts):
    """(source, reference, their device twins) for one size: the sign patterns of its types at full scale from the top
    left, random below them"""
    rng = np.random.default_rng(2400 + ts)
    a, b = O.HostPlane(PW, PH, BD, rng=rng), O.HostPlane(PW, PH, BD, rng=rng)
    va, vb = a.view(), b.view()
    gold = {(c.ts, c.tt): c for c in U.load()[BD]}
    n = SIDES[ts]
    for k, tt in enumerate(TYPES[ts]):
        sg = gold[ts, tt].res[0] >= 0                        # (h, w) sign block of the golden case
        for neg in (0, 1):
            x, y = _slot(ts, 2 * k + neg)
            va[y:y + n, x:x + n] = np.where(sg != bool(neg), 255, 0)
            vb[y:y + n, x:x + n] = np.where(sg != bool(neg), 0, 255)
    return a, b, dev_plane(a), dev_plane(b)


@functools.lru_cache(maxsize=None)
def _random_planes():
    rng = np.random.default_rng(2424)
    a, b = O.HostPlane(PW, PH, BD, rng=rng), O.HostPlane(PW, PH, BD, rng=rng)
    return a, b, dev_plane(a), dev_plane(b)


def _launch(ctx, oracle, planes, ts, c, key):
    """one launch against the oracle -> values compared"""
    a, b, da, db = planes
    n, w = len(c), SIDES[ts]
    pa, pb = a.cstruct(), b.cstruct()
    wsad, wsatd, wco = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, w * w), np.int16)
    assert oracle.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), w, w, ts, O.ptr(c), n, O.ptr(wsad), O.ptr(wsatd),
                                     O.ptr(wco), None) == 0
    o = ctx.rdo_cand_batch(da, db, w, w, c)
    assert np.array_equal(o["sad"].cpu().numpy().view(np.uint32), wsad), (key, "sad")
    assert np.array_equal(o["satd"].cpu().numpy().view(np.uint32), wsatd), (key, "satd")
    got = o["coeffs"].cpu().numpy()
    bad = np.flatnonzero((got != wco).any(1))
    assert not len(bad), (key, "coeffs", bad.tolist())
    return 2 * n + wco.size


@pytest.mark.parametrize("ts", sorted(SIDES), ids=["8x8", "16x16", "32x32", "64x64"])
def test_random_planes(ctx, oracle, ts):
    w, n = SIDES[ts], COUNT[ts]
    assert ts == 4 or n % (64 // w) != 0                     # the last wave is ragged
    rng = np.random.default_rng(2430 + ts)
    compared = 0
    for rep in range(4):
        c = np.zeros(n, O.RDO_CAND)
        c["ox"], c["oy"] = rng.integers(0, PW - w + 1, n), rng.integers(0, PH - w + 1, n)
        # references anywhere the window (block + 3 / 4 pixels) stays inside plane + pads: up to 64 outside the frame
        c["rx"], c["ry"] = rng.integers(-64, PW - w + 64, n), rng.integers(-64, PH - w + 64, n)
        c["col_frac"], c["row_frac"] = rng.integers(0, 16, n), rng.integers(0, 16, n)
        c["mode_x"], c["mode_y"] = rng.integers(0, 4, n), rng.integers(0, 4, n)
        c["tx_type"] = rng.choice(TYPES[ts], n)
        compared += _launch(ctx, oracle, _random_planes(), ts, c, (w, "random", rep))
    assert compared == 4 * (2 * n + n * w * w)


def _pattern_cands(ts, blocks):
    """candidates on pattern blocks (type index k, negative?): zero motion, whole-pel"""
    c = np.zeros(len(blocks), O.RDO_CAND)
    for i, (k, neg) in enumerate(blocks):
        c["ox"][i], c["oy"][i] = _slot(ts, 2 * k + neg)
        c["tx_type"][i] = TYPES[ts][k]
    c["rx"], c["ry"] = c["ox"], c["oy"]
    return c


@pytest.mark.parametrize("ts", sorted(SIDES), ids=["8x8", "16x16", "32x32", "64x64"])
def test_full_scale_sign_patterns(ctx, oracle, ts):
    planes = _pattern_planes(ts)
    w, n, nt = SIDES[ts], COUNT[ts], len(TYPES[ts])
    compared = launches = 0
    # one type per launch: the pattern and its negative, alternating
    for k in range(nt):
        c = _pattern_cands(ts, [(k, i & 1) for i in range(n)])
        r = [planes[0].view()[sl].astype(np.int64) - planes[1].view()[sl].astype(np.int64)
             for sl in ((slice(int(c["oy"][i]), int(c["oy"][i]) + w), slice(int(c["ox"][i]), int(c["ox"][i]) + w))
                        for i in (0, 1))]
        assert (np.abs(r[0]) == 255).all() and np.array_equal(r[0], -r[1])     # full scale, a pattern and its negative
        compared += _launch(ctx, oracle, planes, ts, c, (w, "uniform", TYPES[ts][k]))
        launches += 1
    # a different type in every candidate of a wave: every (type, sign) once, in launches of n
    if nt > 1:
        blocks = [(k, neg) for neg in (0, 1) for k in range(nt)]
        for s in range(0, len(blocks), n):
            part = (blocks[s:s + n] + blocks)[:n]
            nc = 64 // w
            assert len(set(k for k, _ in part[:nc])) == min(nc, nt)
            compared += _launch(ctx, oracle, planes, ts, _pattern_cands(ts, part), (w, "mixed", s))
            launches += 1
    assert launches == nt + (-(-2 * nt // n) if nt > 1 else 0) and compared == launches * (2 * n + n * w * w)

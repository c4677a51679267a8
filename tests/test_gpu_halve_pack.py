"""The fused candidate kernels' two-instruction halving (m24h, tx_common.hpp) and shift-free motion-compensation pack
(mc8_column_t<.., PACK4>, cand_common.hpp) on the device: r1_rdo_cand_batch against the scalar oracle, bit for bit on
SAD, SATD and every coefficient, at 8x8 / 16x16 / 32x32 / 64x64, 8 and 10 bits, launches of 2 NC + 1 candidates (NC =
the candidates a wave owns: the last wave is ragged).

Transform leg: zero-motion blocks whose residual is +-(2^bd - 1) in the sign pattern tests/golden/fwd_tx_ref.npz
keeps for the (size, type) -- the pattern that drives that transform's intermediates furthest -- its negative, and
random blocks; the seven types of the encoder at 8x8 / 16x16 (one type per launch: the wave-uniform switch; one
launch with the types interleaved: the per-lane one), DCT and IDTX at 32x32, DCT at 64x64.

Filter leg: every filter pair with the fractions {0, 1, 8, 15} on both axes, references read from a plane of 0 /
(2^bd - 1) pixels (random, checkerboard, stripes): saturated windows, where the horizontal accumulator and the
vertical sum are largest.  Each leg counts what it compared.  (No instantiation of the quantizer chains takes either
form -- rdo_halve2 / rdo_mc_pack4 of rdo_cand_plan.hpp, pinned by tests/test_tx_halve2.py -- so they have no leg here.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import fwd_tx_ref_util as U
import oracle_lib as O
from test_gpu_parity import dev_plane

pytestmark = pytest.mark.gpu

SIDES = {1: 8, 2: 16, 3: 32, 4: 64}                         # TxSize id -> side
ENC_TYPES = [0, 1, 2, 3, 9, 10, 11]                         # DCT_DCT, ADST_DCT, DCT_ADST, ADST_ADST, IDTX, V_DCT, H_DCT
TYPES = {1: ENC_TYPES, 2: ENC_TYPES, 3: [0, 9], 4: [0]}
PW, PH = 256, 320
FRACS = (0, 1, 8, 15)


def _slot(ts, k):
    """top-left of the k-th pattern block of a size inside the 128-wide pattern area"""
    return k * SIDES[ts], {4: 0, 3: 64, 2: 96, 1: 112}[ts]


@functools.lru_cache(maxsize=None)
def _tx_planes(bd):
    """(source, reference, their device twins): x < 128 the sign patterns at full scale, 128 <= x < 256 their
    negatives, rows 128 .. 319 random"""
    rng = np.random.default_rng(2000 + bd)
    mx = (1 << bd) - 1
    a, b = O.HostPlane(PW, PH, bd, rng=rng), O.HostPlane(PW, PH, bd, rng=rng)
    va, vb = a.view(), b.view()
    gold = {(c.ts, c.tt): c for c in U.load()[bd]}
    for ts, n in SIDES.items():
        for k, tt in enumerate(TYPES[ts]):
            sg = gold[ts, tt].res[0] >= 0                    # (h, w) sign block of the golden case
            x, y = _slot(ts, k)
            va[y:y + n, x:x + n], vb[y:y + n, x:x + n] = np.where(sg, mx, 0), np.where(sg, 0, mx)
            va[y:y + n, 128 + x:128 + x + n], vb[y:y + n, 128 + x:128 + x + n] = np.where(sg, 0, mx), np.where(sg, mx, 0)
    return a, b, dev_plane(a), dev_plane(b)


@functools.lru_cache(maxsize=None)
def _mc_planes(bd):
    """(source: random, reference: 0 / max pixels) and their device twins.  Reference, pads included: random 0 / max,
    with a checkerboard, one- and two-pixel stripes of both directions laid over parts of it"""
    rng = np.random.default_rng(2100 + bd)
    mx = (1 << bd) - 1
    a, b = O.HostPlane(PW, PH, bd, rng=rng), O.HostPlane(PW, PH, bd, rng=rng)
    d = b.data
    d[:] = rng.integers(0, 2, d.shape).astype(d.dtype) * mx
    yy, xx = np.mgrid[0:d.shape[0], 0:d.shape[1]]
    y0, x0 = b.yorigin, b.xorigin
    for i, pat in enumerate(((xx + yy) & 1, xx & 1, yy & 1, (xx >> 1) & 1, (yy >> 1) & 1)):
        sl = (slice(y0 + 64 * (i // 2), y0 + 64 * (i // 2) + 64), slice(x0 + 128 * (i % 2), x0 + 128 * (i % 2) + 128))
        d[sl] = (pat[sl] * mx).astype(d.dtype)
    return a, b, dev_plane(a), dev_plane(b)


def _u(t, dtype):
    return t.cpu().numpy().view(dtype)


def _launch(ctx, oracle, a, b, da, db, ts, c, bd, key):
    """one launch against the oracle -> values compared"""
    n, w = len(c), SIDES[ts]
    pa, pb = a.cstruct(), b.cstruct()
    ct = np.int16 if bd == 8 else np.int32
    wsad, wsatd, wco = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, w * w), ct)
    assert oracle.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), w, w, ts, O.ptr(c), n, O.ptr(wsad), O.ptr(wsatd),
                                     O.ptr(wco), None) == 0
    o = ctx.rdo_cand_batch(da, db, w, w, c)
    assert np.array_equal(_u(o["sad"], np.uint32), wsad), (key, "sad")
    assert np.array_equal(_u(o["satd"], np.uint32), wsatd), (key, "satd")
    got = o["coeffs"].cpu().numpy()
    bad = np.flatnonzero((got != wco).any(1))
    assert not len(bad), (key, "coeffs", bad.tolist())
    return 2 * n + wco.size


def _tx_cands(rng, ts, types):
    """candidate i: type types[i]; the first of a type sits on its sign pattern, the second on the negative, the
    rest anywhere in the random rows.  Zero motion, whole-pel."""
    n, w = len(types), SIDES[ts]
    c = np.zeros(n, O.RDO_CAND)
    c["tx_type"] = types
    seen = {}
    for i, tt in enumerate(types):
        k = seen.get(tt, 0)
        seen[tt] = k + 1
        if k < 2:
            x, y = _slot(ts, TYPES[ts].index(tt))
            c["ox"][i], c["oy"][i] = x + 128 * k, y
        else:
            c["ox"][i], c["oy"][i] = rng.integers(0, PW - w + 1), rng.integers(128, PH - w + 1)
    c["rx"], c["ry"] = c["ox"], c["oy"]
    return c


@pytest.mark.parametrize("ts", sorted(SIDES), ids=["8x8", "16x16", "32x32", "64x64"])
@pytest.mark.parametrize("bd", [8, 10])
def test_transforms_on_full_scale_sign_patterns(ctx, oracle, bd, ts):
    a, b, da, db = _tx_planes(bd)
    w = SIDES[ts]
    mx = (1 << bd) - 1
    n = 2 * (64 // w) + 1
    rng = np.random.default_rng(2200 + 10 * bd + ts)
    runs = [[tt] * n for tt in TYPES[ts]]
    if len(TYPES[ts]) > 1:
        runs.append([TYPES[ts][i % len(TYPES[ts])] for i in range(n)])
    compared = 0
    for types in runs:
        c = _tx_cands(rng, ts, types)
        if types[0] == types[1]:      # the blocks are what the docstring says: full scale, a pattern and its negative
            r = [a.view()[sl].astype(np.int64) - b.view()[sl].astype(np.int64)
                 for sl in ((slice(int(c["oy"][i]), int(c["oy"][i]) + w), slice(int(c["ox"][i]), int(c["ox"][i]) + w))
                            for i in (0, 1))]
            assert (np.abs(r[0]) == mx).all() and np.array_equal(r[0], -r[1])
        compared += _launch(ctx, oracle, a, b, da, db, ts, c, bd, (bd, w, tuple(types[:3])))
    assert compared == len(runs) * (2 * n + n * w * w)


@pytest.mark.parametrize("ts", sorted(SIDES), ids=["8x8", "16x16", "32x32", "64x64"])
@pytest.mark.parametrize("bd", [8, 10])
def test_every_filter_pair_on_saturated_windows(ctx, oracle, bd, ts):
    a, b, da, db = _mc_planes(bd)
    w = SIDES[ts]
    n = 2 * (64 // w) + 1
    rng = np.random.default_rng(2300 + 10 * bd + ts)
    combos = [(mx, my, cf, rf) for mx in range(4) for my in range(4) for cf in FRACS for rf in FRACS]
    assert len(combos) == 256
    compared = launches = 0
    for s in range(0, len(combos), n):
        part = combos[s:s + n]
        part = part + combos[:n - len(part)]                 # the last launch is full too: 2 NC + 1 every time
        c = np.zeros(n, O.RDO_CAND)
        c["mode_x"], c["mode_y"] = [p[0] for p in part], [p[1] for p in part]
        c["col_frac"], c["row_frac"] = [p[2] for p in part], [p[3] for p in part]
        c["ox"], c["oy"] = rng.integers(0, PW - w + 1, n), rng.integers(0, PH - w + 1, n)
        # references anywhere the window (block + 3 / 4 pixels) stays inside plane + pads: up to 64 outside the frame
        c["rx"], c["ry"] = rng.integers(-64, PW - w + 64, n), rng.integers(-64, PH - w + 64, n)
        compared += _launch(ctx, oracle, a, b, da, db, ts, c, bd, (bd, w, part[0]))
        launches += 1
    assert launches == -(-256 // n) and compared == launches * (2 * n + n * w * w)

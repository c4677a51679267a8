"""The fused candidate kernel's SATD with the horizontal pass in registers (blocks with both sides >= 16, up to
10 bits: the packed vertical intermediates go through an LDS tile that aliases the dead window and source block),
and the lane-stage path that every other size and 12-bit keep.  Everything bit for bit against the CPU oracle:
  1. residuals of +-(2^bd - 1) in every Walsh sign pattern of an 8x8 tile -- single coefficients of 64 * max, the i16
     intermediates at their proven bound (32 * max), which random planes never come near;
  2. ragged waves: n = 1, NC - 1, NC, NC + 1, 2 NC + 1 candidates of distinct content, sad / satd / coeffs (the tile
     aliases memory the later phases reuse);
  3. partial outputs;
  4. the sibling entry points that share phase B (quantizer legs, type search, intra prediction source)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import TX_SIZES, dev_plane, rand_rdo_cands

pytestmark = pytest.mark.gpu

PW = PH = 160
TILED = [(16, 16), (32, 32), (64, 64), (16, 32), (32, 16), (32, 64), (64, 32), (16, 64), (64, 16)]   # take the tile path
PINNED = [(8, 8), (8, 16), (16, 8), (4, 16)]                                                    # stay on lane stages
Q = 80                # a plane is four quadrants of 80 x 80 (ten tiles a side), one sign pattern each


def _sign_patterns():
    """(name, 80 x 80 array of +-1): the 64 Walsh patterns of an 8x8 tile tiled over the quadrant, all-positive,
    all-negative, and all-positive with the sign alternating from tile to tile"""
    x = np.arange(Q)
    had = np.array([[1 - 2 * (bin(u & k).count("1") & 1) for k in range(8)] for u in range(8)])
    out = [("walsh%d%d" % (v, u), np.outer(had[v][x & 7], had[u][x & 7])) for v in range(8) for u in range(8)]
    out.append(("positive", np.ones((Q, Q), np.int64)))
    out.append(("negative", -np.ones((Q, Q), np.int64)))
    out.append(("tile_alternating", np.outer(1 - 2 * ((x >> 3) & 1), 1 - 2 * ((x >> 3) & 1))))
    return out


def _extreme_planes(bd, four):
    """org / ref whose difference at zero MV is +-(2^bd - 1) with the sign of pattern four[q] in quadrant q"""
    org, ref = O.HostPlane(PW, PH, bd, fill=0), O.HostPlane(PW, PH, bd, fill=0)
    mx = (1 << bd) - 1
    for q, (_, s) in enumerate(four):
        y0, x0 = (q >> 1) * Q, (q & 1) * Q
        org.view()[y0:y0 + Q, x0:x0 + Q] = np.where(s > 0, mx, 0)
        ref.view()[y0:y0 + Q, x0:x0 + Q] = np.where(s > 0, 0, mx)
    return org, ref


def _oracle_cand(oracle, a, b, w, h, c):
    ts, n = TX_SIZES.index((w, h)), len(c)
    ct = np.int16 if a.bit_depth == 8 else np.int32
    pa, pb = a.cstruct(), b.cstruct()
    sad, satd, co = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, w * h), ct)
    assert oracle.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, O.ptr(sad), O.ptr(satd),
                                     O.ptr(co), None) == 0
    return sad, satd, co


def _check_cand(ctx, oracle, a, b, da, db, w, h, c, key):
    sad, satd, co = _oracle_cand(oracle, a, b, w, h, c)
    o = ctx.rdo_cand_batch(da, db, w, h, c)
    assert np.array_equal(o["sad"].cpu().numpy().view(np.uint32), sad), (key, "sad")
    assert np.array_equal(o["satd"].cpu().numpy().view(np.uint32), satd), (key, "satd")
    assert np.array_equal(o["coeffs"].cpu().numpy(), co), (key, "coeffs")
    return satd


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_satd_at_the_range_limits(ctx, oracle, bd):
    sizes = TILED + PINNED if bd <= 10 else [(16, 16), (64, 64)]   # 12-bit: i32 lane stages, must still agree
    pats = _sign_patterns()
    mx = (1 << bd) - 1
    for p0 in range(0, len(pats), 4):
        four = [pats[min(p0 + q, len(pats) - 1)] for q in range(4)]
        a, b = _extreme_planes(bd, four)
        da, db = dev_plane(a), dev_plane(b)
        for (w, h) in sizes:
            c = np.zeros(4, O.RDO_CAND)
            c["ox"] = c["rx"] = [0, Q, 0, Q]
            c["oy"] = c["ry"] = [0, 0, Q, Q]
            satd = _check_cand(ctx, oracle, a, b, da, db, w, h, c, (bd, w, h, [n for n, _ in four]))
            if min(w, h) >= 8:
                # an 8x8 tile of +-max in a Walsh pattern (or constant) has one coefficient, 64 * max
                assert (satd == ((w * h * mx + 4) >> 3)).all(), (bd, w, h, "closed form")


@pytest.mark.parametrize("bd", [8, 10])
def test_ragged_waves_of_distinct_candidates(ctx, oracle, bd):
    rng = np.random.default_rng(1300 + bd)
    a, b = O.HostPlane(PW, PH, bd, rng=rng), O.HostPlane(PW, PH, bd, rng=rng)
    da, db = dev_plane(a), dev_plane(b)
    for (w, h) in ((16, 16), (32, 32), (64, 64)):
        nc = 64 // max(w, h)
        for n in sorted({1, nc - 1, nc, nc + 1, 2 * nc + 1} - {0}):
            c = rand_rdo_cands(rng, n, PW, PH, w, h, 40, TX_SIZES.index((w, h)))
            c["col_frac"] = rng.integers(1, 16, n)      # sub-pel both ways: every candidate its own prediction
            c["row_frac"] = rng.integers(1, 16, n)
            _check_cand(ctx, oracle, a, b, da, db, w, h, c, (bd, w, h, n))


@pytest.mark.parametrize("bd", [8, 10])
def test_partial_outputs(ctx, oracle, bd):
    rng = np.random.default_rng(1400 + bd)
    a, b = O.HostPlane(PW, PH, bd, rng=rng), O.HostPlane(PW, PH, bd, rng=rng)
    da, db = dev_plane(a), dev_plane(b)
    for (w, h) in ((16, 16), (32, 32), (64, 64), (16, 64)):
        n = 2 * (64 // max(w, h)) + 1
        c = rand_rdo_cands(rng, n, PW, PH, w, h, 40, TX_SIZES.index((w, h)))
        sad, satd, co = _oracle_cand(oracle, a, b, w, h, c)
        o = ctx.rdo_cand_batch(da, db, w, h, c, want_coeffs=False, want_sad=False)   # the kernel returns after the SATD
        assert np.array_equal(o["satd"].cpu().numpy().view(np.uint32), satd), (bd, w, h, "satd only")
        o = ctx.rdo_cand_batch(da, db, w, h, c, want_satd=False)                     # the tile is never written
        assert "satd" not in o
        assert np.array_equal(o["sad"].cpu().numpy().view(np.uint32), sad), (bd, w, h, "no satd: sad")
        assert np.array_equal(o["coeffs"].cpu().numpy(), co), (bd, w, h, "no satd: coeffs")


def _u(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("bd", [8, 10])
def test_quantizer_legs_and_type_search(ctx, oracle, bd, w):
    """r1_rdo_full_cand_batch (QM 1), r1_rdo_pixel_cand_batch (QM 2, source block kept behind the work area at
    16x16) and the type search on the same candidates: SATD and every other output"""
    h, ts = w, TX_SIZES.index((w, w))
    rng = np.random.default_rng(1500 + bd + w)
    a = O.HostPlane(PW, PH, bd, rng=rng)
    b = O.HostPlane(PW, PH, bd, rng=rng)
    b.data[...] = np.clip(a.data.astype(np.int64) + rng.integers(-12, 13, a.data.shape) * (1 << (bd - 8)), 0,
                          (1 << bd) - 1).astype(a.data.dtype)
    da, db = dev_plane(a), dev_plane(b)
    ct, dt = (np.int16, np.uint8) if bd == 8 else (np.int32, np.uint16)
    n, carea, qi = 2 * (64 // w) + 1, w * h, 70
    c = rand_rdo_cands(rng, n, PW, PH, w, h, 8, ts)
    c["rx"], c["ry"] = c["ox"] + rng.integers(-2, 3, n), c["oy"] + rng.integers(-2, 3, n)
    pa, pb = a.cstruct(), b.cstruct()
    wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    weob, wdist, wrate = np.zeros(n, np.uint16), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    wq, wrec = np.zeros((n, carea), ct), np.zeros((n, h, w), dt)
    assert oracle.r1o_rdo_full_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, qi, 0, 0, 0, O.ptr(wsad),
                                          O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wrate), O.ptr(wq)) == 0
    o = ctx.rdo_full_cand_batch(da, db, w, h, c, qi, want_qcoeffs=True)
    key = (bd, w, "full")
    assert np.array_equal(_u(o["sad"], np.uint32), wsad), key
    assert np.array_equal(_u(o["satd"], np.uint32), wsatd), key
    assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
    assert np.array_equal(_u(o["eob"], np.uint16), weob), key
    assert np.array_equal(_u(o["tx_dist"], np.uint64), wdist), key
    assert np.array_equal(_u(o["est_rate"], np.uint64), wrate), key
    for kind in (2, 3):
        assert oracle.r1o_rdo_pixel_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, qi, 0, 0, 0, kind,
                                               None, 0, 0, 0, O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist),
                                               O.ptr(wq), O.ptr(wrec), None) == 0
        o = ctx.rdo_pixel_cand_batch(da, db, w, h, c, qi, kind, want_qcoeffs=True, want_rec=True)
        key = (bd, w, "pixel", kind)
        assert np.array_equal(_u(o["sad"], np.uint32), wsad), key
        assert np.array_equal(_u(o["satd"], np.uint32), wsatd), key
        assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
        assert np.array_equal(_u(o["eob"], np.uint16), weob), key
        assert np.array_equal(_u(o["rec"], dt), wrec), key
        assert np.array_equal(_u(o["dist"], np.uint64), wdist), key
    mask = ctx.tx_type_mask(ts, True)
    nt = bin(mask).count("1")
    c["tx_type"] = 0
    for kind in (0, 3):
        weob, wdist, wrate = np.zeros((n, nt), np.uint16), np.zeros((n, nt), np.uint64), np.zeros((n, nt), np.uint64)
        wq, wrec = np.zeros((n, nt, carea), ct), np.zeros((n, nt, h, w), dt)
        assert oracle.r1o_rdo_txsearch_batch(C.byref(pa), C.byref(pb), None, w, h, ts, O.ptr(c), n, mask, qi, 0, 0, 0,
                                             kind, None, 0, 0, 0, O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist),
                                             O.ptr(wrate) if kind == 0 else None, O.ptr(wq),
                                             O.ptr(wrec) if kind else None) == 0
        o = ctx.rdo_txsearch_batch(da, db, w, h, c, mask, qi, kind, want_sad=True, want_satd=True,
                                   want_est_rate=kind == 0, want_qcoeffs=True, want_rec=bool(kind))
        key = (bd, w, "txsearch", kind, hex(mask))
        assert np.array_equal(_u(o["sad"], np.uint32), wsad), key
        assert np.array_equal(_u(o["satd"], np.uint32), wsatd), key
        assert np.array_equal(_u(o["eob"], np.uint16), weob), key
        assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
        assert np.array_equal(_u(o["dist"], np.uint64), wdist), key
        if kind:
            assert np.array_equal(_u(o["rec"], dt), wrec), key
        else:
            assert np.array_equal(_u(o["est_rate"], np.uint64), wrate), key


@pytest.mark.parametrize("ts", [2, 3])
@pytest.mark.parametrize("bd", [8, 10])
def test_intra_prediction_source(ctx, oracle, bd, ts):
    """r1_rdo_intra_cand_batch: the tile lies over the edge arrays and the late-staged source block"""
    import test_gpu_rdo_intra as RI
    w, h = RI.TX_DIMS[ts]
    rec, org = RI._planes(bd, 1600 + 10 * ts + bd, PW, PH)
    drec, dorg = RI._dev_plane(rec), RI._dev_plane(org)
    rng = np.random.default_rng(1700 + 10 * ts + bd)
    n = 2 * (64 // w) + 1
    mask = ctx.tx_type_mask(ts, False) if w <= 16 else 1
    for kind in (0, 3):
        cs = RI.make_case(rng, ctx, rec, drec, ts, n, 1)
        RI.check_call(ctx, oracle, org, dorg, ts, bd, cs, 1, mask, 90, kind, None, None, 0, 0, True,
                      ("satd tile", ts, bd, kind))

"""The folded column pass of the fused kernels (fwd_col_m24, tx_common.hpp: unshifted residuals in, shift[1] applied on
the way out) on the device, against the CPU oracle, on residuals built to sit where the fold could go wrong: every
halving it drops is exact only on the multiples of 2^k it tracks, so the blocks are, in turn, a +-max checkerboard,
all -1, all -3 (odd, negative: the sign correction of TX_RSHIFT1 would matter were a halving dropped too late) and
random.  One 192x192 padded plane pair per bit depth holds the four in its quadrants; a candidate is a zero-motion
block inside one quadrant, so its residual is that quadrant's pattern.

For 8 and 10 bits, every one of the 19 sizes and every admissible type: one launch of 2 NC + 1 candidates (NC = the
candidates a wave owns: the last wave is partial; four where NC = 1, one per pattern), raw coefficients, SAD and SATD
against r1o_rdo_cand_batch -- one type per launch is the wave-uniform switch of the sizes up to 16x16, and one more
launch per size with the types interleaved is the per-lane switch.  The same blocks go once through
r1_rdo_full_cand_batch and r1_rdo_pixel_cand_batch at one qindex, and the plane pair once through
r1_rdo_intra_split_batch (source = the first plane, reconstruction = the second)."""
import ctypes as C
import functools

import numpy as np
import pytest

import intra_split_util as SU
import oracle_lib as O
from test_gpu_parity import TX_SIZES, dev_plane

pytestmark = pytest.mark.gpu

PW = PH = 192
Q = 96          # quadrant side: a 64x64 block fits with room to move
QI = 70


@functools.lru_cache(maxsize=None)
def _planes(bd):
    """(source, reference) host planes and their device twins: quadrant 0 +-max checkerboard, 1 all -1, 2 all -3,
    3 random"""
    rng = np.random.default_rng(1700 + bd)
    mx = (1 << bd) - 1
    a, b = O.HostPlane(PW, PH, bd, rng=rng), O.HostPlane(PW, PH, bd, rng=rng)
    va, vb = a.view(), b.view()
    yy, xx = np.mgrid[0:Q, 0:Q]
    ck = ((xx + yy) & 1).astype(va.dtype)
    va[:Q, :Q], vb[:Q, :Q] = ck * mx, (1 - ck) * mx
    base = rng.integers(0, mx - 2, (Q, Q)).astype(va.dtype)
    va[:Q, Q:], vb[:Q, Q:] = base, base + 1
    va[Q:, :Q], vb[Q:, :Q] = base.T, base.T + 3
    return a, b, dev_plane(a), dev_plane(b)


def _cands(rng, n, w, h, types):
    """candidate i sits in quadrant i % 4, anywhere the block fits; zero motion, whole-pel"""
    c = np.zeros(n, O.RDO_CAND)
    q = np.arange(n) % 4
    c["ox"] = c["rx"] = (q & 1) * Q + rng.integers(0, Q - w + 1, n)
    c["oy"] = c["ry"] = (q >> 1) * Q + rng.integers(0, Q - h + 1, n)
    c["tx_type"] = types
    return c


def _n(w, h):
    nc = 64 // max(w, h)
    return 2 * nc + 1 if nc > 1 else 4


def _valid(ts):
    from rav1e_amd.types import valid_av1_transform
    return [t for t in range(16) if valid_av1_transform(ts, t)]


def _u(t, dtype):
    return t.cpu().numpy().view(dtype)


def _check_residuals(a, b, c, w, h, bd):
    """the blocks are what the docstring says"""
    mx = (1 << bd) - 1
    for i in range(min(len(c), 4)):
        sl = (slice(int(c["oy"][i]), int(c["oy"][i]) + h), slice(int(c["ox"][i]), int(c["ox"][i]) + w))
        r = a.view()[sl].astype(np.int64) - b.view()[sl].astype(np.int64)
        if i == 0:
            assert (np.abs(r) == mx).all() and (r[0, 0] == -r[0, 1]) and (r[0, 0] == -r[1, 0])
        elif i < 3:
            assert (r == (-1, -3)[i - 1]).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_raw_coefficients_sad_satd_every_size_and_type(ctx, oracle, bd):
    a, b, da, db = _planes(bd)
    pa, pb = a.cstruct(), b.cstruct()
    rng = np.random.default_rng(1800 + bd)
    ct = np.int16 if bd == 8 else np.int32
    launches = 0
    for ts, (w, h) in enumerate(TX_SIZES):
        n, valid = _n(w, h), _valid(ts)
        runs = [[t] * n for t in valid]
        if len(valid) > 1:
            runs.append([valid[i % len(valid)] for i in range(n)])      # per-lane switch: mixed waves
        for types in runs:
            c = _cands(rng, n, w, h, types)
            _check_residuals(a, b, c, w, h, bd)
            wsad, wsatd, wco = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, w * h), ct)
            assert oracle.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, O.ptr(wsad), O.ptr(wsatd),
                                             O.ptr(wco), None) == 0
            o = ctx.rdo_cand_batch(da, db, w, h, c)
            key = (bd, w, h, types[:4])
            assert np.array_equal(_u(o["sad"], np.uint32), wsad), (key, "sad")
            assert np.array_equal(_u(o["satd"], np.uint32), wsatd), (key, "satd")
            got = o["coeffs"].cpu().numpy()
            bad = np.flatnonzero((got != wco).any(1))
            assert not len(bad), (key, "coeffs", [(int(i), int(i) % 4) for i in bad])
            launches += 1
    assert launches == sum(len(_valid(ts)) + (len(_valid(ts)) > 1) for ts in range(len(TX_SIZES)))


@pytest.mark.parametrize("bd", [8, 10])
def test_quantizer_chains_on_the_same_blocks(ctx, oracle, bd):
    a, b, da, db = _planes(bd)
    pa, pb = a.cstruct(), b.cstruct()
    rng = np.random.default_rng(1900 + bd)
    ct, dt = (np.int16, np.uint8) if bd == 8 else (np.int32, np.uint16)
    for ts, (w, h) in enumerate(TX_SIZES):
        n, valid = _n(w, h), _valid(ts)
        c = _cands(rng, n, w, h, [valid[i % len(valid)] for i in range(n)])
        carea = min(w, 32) * min(h, 32)
        wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        weob, wdist, wrate = np.zeros(n, np.uint16), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        wq, wrec = np.zeros((n, carea), ct), np.zeros((n, h, w), dt)
        assert oracle.r1o_rdo_full_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, QI, 0, 0, 0, O.ptr(wsad),
                                              O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wrate), O.ptr(wq)) == 0
        o = ctx.rdo_full_cand_batch(da, db, w, h, c, QI, want_qcoeffs=True)
        key = (bd, w, h, "full")
        assert np.array_equal(_u(o["sad"], np.uint32), wsad), key
        assert np.array_equal(_u(o["satd"], np.uint32), wsatd), key
        assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
        assert np.array_equal(_u(o["eob"], np.uint16), weob), key
        assert np.array_equal(_u(o["tx_dist"], np.uint64), wdist), key
        assert np.array_equal(_u(o["est_rate"], np.uint64), wrate), key
        assert oracle.r1o_rdo_pixel_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, QI, 0, 0, 0, 2, None, 0,
                                               0, 0, O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wq),
                                               O.ptr(wrec), None) == 0
        o = ctx.rdo_pixel_cand_batch(da, db, w, h, c, QI, 2, want_qcoeffs=True, want_rec=True)
        key = (bd, w, h, "pixel")
        assert np.array_equal(_u(o["sad"], np.uint32), wsad), key
        assert np.array_equal(_u(o["satd"], np.uint32), wsatd), key
        assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
        assert np.array_equal(_u(o["eob"], np.uint16), weob), key
        assert np.array_equal(_u(o["rec"], dt), wrec), key
        assert np.array_equal(_u(o["dist"], np.uint64), wdist), key


# (block w, block h, TxSize): the four k_intra_split<., TL> of a bit depth
SPLIT_SHAPES = [(8, 8, 0), (16, 16, 1), (32, 32, 2), (64, 64, 3)]


@pytest.mark.parametrize("bw,bh,ts", SPLIT_SHAPES)
@pytest.mark.parametrize("bd", [8, 10])
def test_intra_split_on_the_same_planes(ctx, oracle, bd, bw, bh, ts):
    import test_gpu_rdo_intra_split as SP
    a, b, da, db = _planes(bd)
    t = SU.TX_SIDE[ts]
    n = 64 // t + 1
    rng = np.random.default_rng(2000 + bd + ts)
    tile = (0, 0, PW, PH)
    cands = SP.make_cands(rng, n, bw, bh, t, PW, PH, inside_only=True)
    q = np.arange(n) % 4          # one block per quadrant in turn
    cands["x"] = (q & 1) * Q + rng.integers(0, (Q - bw) // 4 + 1, n) * 4
    cands["y"] = (q >> 1) * Q + rng.integers(0, (Q - bh) // 4 + 1, n) * 4
    mask = 0x20B & ctx.tx_type_mask(ts, False) if t <= 16 else 1
    got = SP.one_launch(ctx, da, db, tile, bw, bh, ts, cands, True, mask, QI, 0, None)
    want = SU.oracle_split(oracle, a, b, tile, bw, bh, ts, cands, True, mask, QI, 0, None)
    SP._same(got, want, list(got), (bd, bw, bh, ts, hex(mask)), "oracle composition")

"""tests/golden/fwd_tx_ref.npz (gen_fwd_tx_ref.py: the reference's `forward_transform` executed whole from its
text, ten structured blocks per (size, type, bit depth)) against the CPU side of the project:

  * the C oracle's 2-D transform, every block, both coefficient widths at 8 bits;
  * the analytic bounds of tools/tx_range.py -- what makes the 24-bit multiplies, the int16 column tile and the
    24-bit quantizer of the fused kernels exact -- against the magnitudes the executed reference reached;
  * where the reference tree is present, the oracle's 13 1-D networks against the translated reference networks
    on far more lanes than a fixture can hold."""
import os
import sys

import numpy as np
import pytest

import fwd_tx_ref_util as U
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
NCASES = 160        # (tx_size, valid tx_type) pairs, WHT at 4x4 included
COL_TILE_BOUND = {8: 8193, 10: 16433, 12: 16445}


def test_fixture_holds_every_case_and_every_block_kind():
    R = U.load()
    for bd in U.BITDEPTHS:
        cases = R[bd]
        assert len(cases) == NCASES and len({(c.ts, c.tt) for c in cases}) == NCASES
        assert sum(c.tt == 16 for c in cases) == 1
        lim = (1 << bd) - 1
        for c in cases:
            assert len(c.res) == (10 if c.w * c.h <= 1024 else 7), (bd, c.ts, c.tt)
            assert c.coef.dtype == (np.int16 if bd == 8 else np.int32)
            by = dict(zip(c.names, c.res))
            assert (np.abs(by["sign"]) == lim).all()        # all +lim where neither network multiplies
            assert int(np.abs(by["rand"]).max()) <= lim and len(np.unique(by["rand"])) > 8
            assert (by["const+"] == lim).all() and (by["const-"] == -lim).all()
            for k in ("checker", "rows", "cols"):
                assert set(np.unique(by[k])) == {-lim, lim}
            assert by["checker"][0, 0] == by["checker"][1, 1] == lim and by["checker"][0, 1] == by["checker"][1, 0] == -lim
            assert (by["rows"][0] == lim).all() and (by["rows"][1] == -lim).all()
            assert (by["cols"][:, 0] == lim).all() and (by["cols"][:, 1] == -lim).all()
            if len(c.res) == 10:
                assert int(np.abs(by["small"]).max()) <= 2 and (by["small"] == -1).mean() > 0.3
                assert by["impulse"][-1, -1] == -lim and np.count_nonzero(by["impulse"]) == 1
                assert not by["zero"].any()
            # the recorded coefficient maximum is the stored coefficients' (nothing was narrowed away)
            assert np.array_equal(np.abs(c.coef.astype(np.int64)).max(1), c.stats[:, 2])


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_oracle_forward_transform_equals_executed_reference(oracle, bd):
    nblocks = 0
    for c in U.load()[bd]:
        res = np.ascontiguousarray(c.res)
        n = len(res)
        for cb in ((2, 4) if bd == 8 else (4,)):
            got = np.zeros((n, c.w * c.h), np.int16 if cb == 2 else np.int32)
            assert oracle.r1o_fwd_txfm_batch(O.ptr(res), O.ptr(got), n, c.ts, c.tt, bd, cb) == 0
            bad = np.flatnonzero((got != c.coef).any(1))
            assert not len(bad), (bd, c.ts, c.tt, cb, [c.names[i] for i in bad])
        nblocks += n
    assert nblocks == 1591


@pytest.fixture(scope="module")
def analysis():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tx_range
    return {r[:3]: r[3] for r in tx_range.analyse()}, tx_range.shifted_coefficient_bound()


def test_analytic_bounds_hold_for_the_executed_reference(analysis):
    """tests/test_tx_range.py states its three claims against oracle/fwd_tx_np.py; here they meet what the
    reference itself reached on blocks built to come close.  Soundness checks: no margin.  (WHT has no row in the
    analysis: it multiplies nowhere and is not offered to the fused kernels.)"""
    mul_bound, coef_bound = analysis
    nchecked = 0
    for bd in U.BITDEPTHS:
        for c in U.load()[bd]:
            if c.tt == 16:
                assert not c.stats[:, 0].any()
                continue
            mulmax, colmax, cmax = (int(v) for v in c.stats.max(0))
            assert mulmax <= mul_bound[bd, c.ts, c.tt], (bd, c.ts, c.tt, mulmax)
            if max(c.w, c.h) <= 16:
                assert colmax <= COL_TILE_BOUND[bd], (bd, c.ts, c.tt, colmax)
            lts = (c.w * c.h > 256) + (c.w * c.h > 1024)
            assert cmax << lts <= coef_bound[bd], (bd, c.ts, c.tt, cmax)
            nchecked += 1
    assert nchecked == 3 * (NCASES - 1)


def lanes_for(n, rng):
    """residual range, the full i16 range, and +-lim sign patterns: all of them for n <= 16"""
    x = [rng.integers(-255, 256, (20000, n)), rng.integers(-4095 * 4, 4095 * 4 + 1, (30000, n)),
         rng.integers(-32768, 32768, (50000, n))]
    if n <= 16:
        bits = (np.arange(1 << n)[:, None] >> np.arange(n)) & 1
        sg = 1 - 2 * bits
    else:
        sg = rng.choice([-1, 1], (20000, n))
    for lim in (255, 1023, 4095):
        x.append(sg * lim)
    return np.ascontiguousarray(np.concatenate(x).astype(np.int32))


@needs_ref
def test_oracle_1d_networks_equal_translated_reference_at_scale(oracle):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_fwd_tx_golden as FT
    ns, _ = FT.load_reference_1d()
    rng = np.random.default_rng(20261020)
    f = oracle.r1o_fwd_txfm_1d
    for t in range(13):
        n = FT.TXFM_LEN[t]
        x = lanes_for(n, rng)
        assert len(x) >= 100000
        want = FT.run_1d(ns, t, x)
        got = x.copy()
        base, step = got.ctypes.data, got.strides[0]
        for i in range(len(got)):
            f(base + i * step, t)
        bad = np.flatnonzero((got != want).any(1))
        assert not len(bad), (t, len(bad), x[bad[0]].tolist())

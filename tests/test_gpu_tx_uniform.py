"""The fused candidate kernel's vote on a wave's transform types (TX_VOTE, rdo_cand_kernel.hpp): a wave whose candidates
all carry one type switches between the 1-D kernels with a scalar branch, a wave of mixed types (or of a type whose
class in a pass is the identity) keeps the per-lane switch.  The one decision is the vote, and it can go wrong only at
the wave boundaries: so tiny batches whose type lists put the boundaries everywhere, each bit for bit against the CPU
oracle on SAD, SATD and every coefficient.  A wave holds NC = 64 / max(w, h) candidates.  The 32x32 kernel does not
vote (profiles/r16_txuniform_notes.md) and its cases pin that its results stay what they were; the quantizer chains'
kernels are the parent's byte for byte, so there is no full-chain case."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import TX_SIZES, dev_plane, rand_rdo_cands

pytestmark = pytest.mark.gpu

PW = PH = 96
DCT_DCT, ADST_DCT, DCT_ADST, ADST_ADST, FLIPADST_DCT, DCT_FLIPADST, FLIPADST_FLIPADST = 0, 1, 2, 3, 4, 5, 6
ADST_FLIPADST, FLIPADST_ADST, IDTX, V_DCT, H_DCT = 7, 8, 9, 10, 11
RDO_TYPES = (DCT_DCT, ADST_DCT, DCT_ADST, ADST_ADST, IDTX, V_DCT, H_DCT)   # RAV1E_TX_TYPES


@functools.lru_cache(maxsize=None)
def _planes(bd):
    rng = np.random.default_rng(1600 + bd)
    a, b = O.HostPlane(PW, PH, bd, rng=rng), O.HostPlane(PW, PH, bd, rng=rng)
    return a, b, dev_plane(a), dev_plane(b)


def _cands(bd, w, h, types):
    """one candidate per entry of `types`; position, motion vector and filter depend on (bd, w, h, n) only, so that
    two type lists of one length describe the same predictions"""
    n = len(types)
    rng = np.random.default_rng(1000 * bd + 10 * w + h + n)
    c = rand_rdo_cands(rng, n, PW, PH, w, h, 8, TX_SIZES.index((w, h)))
    c["tx_type"] = types
    return c


def _run(ctx, oracle, bd, w, h, types):
    """GPU against oracle for one type list; returns the coefficients, (n, w * h)"""
    a, b, da, db = _planes(bd)
    c = _cands(bd, w, h, types)
    n, ts = len(c), TX_SIZES.index((w, h))
    pa, pb = a.cstruct(), b.cstruct()
    sad, satd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    co = np.zeros((n, w * h), np.int16 if bd == 8 else np.int32)
    assert oracle.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, O.ptr(sad), O.ptr(satd),
                                     O.ptr(co), None) == 0
    o = ctx.rdo_cand_batch(da, db, w, h, c)
    key = (bd, w, h, list(types))
    assert np.array_equal(o["sad"].cpu().numpy().view(np.uint32), sad), (key, "sad")
    assert np.array_equal(o["satd"].cpu().numpy().view(np.uint32), satd), (key, "satd")
    got = o["coeffs"].cpu().numpy()
    bad = np.nonzero((got != co).any(axis=1))[0]
    assert bad.size == 0, (key, "coeffs of candidates", bad.tolist())
    return co


def _waves(types, nc):
    return [list(types[i:i + nc]) for i in range(0, len(types), nc)]


def _assert_mixed(types, nc, waves):
    """the waves named really hold two or more types, every other wave one"""
    for i, wv in enumerate(_waves(types, nc)):
        assert (len(set(wv)) >= 2) == (i in waves), (types, nc, i)


@pytest.mark.parametrize("bd", [8, 10])
def test_8x8_wave_boundaries(ctx, oracle, bd):
    w = h = 8
    nc, n = 8, 17                      # two full waves and one with a single live candidate
    # (a) every wave uniform, DCT_DCT
    types = [DCT_DCT] * n
    _assert_mixed(types, nc, ())
    _run(ctx, oracle, bd, w, h, types)
    # (b) every wave uniform on a flipped type: up-down only, left-right only, both -- and the flips do something
    plain = _run(ctx, oracle, bd, w, h, [ADST_ADST] * n)
    for t in (FLIPADST_ADST, ADST_FLIPADST, FLIPADST_FLIPADST):
        co = _run(ctx, oracle, bd, w, h, [t] * n)
        assert (co != plain).any(axis=1).all(), (bd, t, "a flipped type gave the unflipped type's coefficients")
    # (b') uniform on the types whose class is the identity in one pass or in both
    for t in (IDTX, V_DCT, H_DCT):
        _run(ctx, oracle, bd, w, h, [t] * n)
    # (c) wave 0 uniform, wave 1 with one odd type in its last slot, wave 2 alone
    for t, odd in ((DCT_DCT, ADST_ADST), (ADST_DCT, DCT_DCT), (FLIPADST_DCT, V_DCT), (DCT_DCT, IDTX)):
        types = [t] * n
        types[2 * nc - 1] = odd
        _assert_mixed(types, nc, (1,))
        _run(ctx, oracle, bd, w, h, types)
    # (d) the seven RDO types in turn: every wave of two or more candidates is mixed
    types = [RDO_TYPES[i % 7] for i in range(n)]
    _assert_mixed(types, nc, (0, 1))
    _run(ctx, oracle, bd, w, h, types)
    # (e) the only live slot of wave 1 differs from wave 0's type: its dead slots repeat IT, both waves are uniform
    for t, last in ((DCT_DCT, ADST_FLIPADST), (FLIPADST_ADST, DCT_DCT), (IDTX, ADST_ADST)):
        types = [t] * nc + [last]
        _assert_mixed(types, nc, ())
        co = _run(ctx, oracle, bd, w, h, types)
        same = _run(ctx, oracle, bd, w, h, [t] * (nc + 1))
        assert np.array_equal(co[:nc], same[:nc]) and not np.array_equal(co[nc], same[nc]), (bd, t, last)


@pytest.mark.parametrize("bd", [8, 10])
def test_16x16_wave_boundaries(ctx, oracle, bd):
    w = h = 16
    nc, n = 4, 5
    _run(ctx, oracle, bd, w, h, [DCT_DCT] * n)                                   # (a)
    plain = _run(ctx, oracle, bd, w, h, [ADST_ADST] * n)
    co = _run(ctx, oracle, bd, w, h, [FLIPADST_FLIPADST] * n)
    assert (co != plain).any(axis=1).all(), (bd, "flips")
    for t in (IDTX, V_DCT, H_DCT):
        _run(ctx, oracle, bd, w, h, [t] * n)
    for t, odd in ((DCT_DCT, DCT_ADST), (ADST_ADST, H_DCT)):                      # (c): one wave, odd type last
        types = [t] * (nc - 1) + [odd] + [t]
        _assert_mixed(types, nc, (0,))
        _run(ctx, oracle, bd, w, h, types)
    types = [RDO_TYPES[(i + 3) % 7] for i in range(n)]                           # (d)
    _assert_mixed(types, nc, (0,))
    _run(ctx, oracle, bd, w, h, types)


@pytest.mark.parametrize("bd", [8, 10])
def test_32x32_dct_and_identity(ctx, oracle, bd):
    w = h = 32
    nc = 2
    for types, mixed in (([DCT_DCT] * 3, ()), ([IDTX] * 3, ()), ([DCT_DCT, IDTX, DCT_DCT], (0,)),
                         ([IDTX, DCT_DCT, IDTX], (0,)), ([DCT_DCT, DCT_DCT, IDTX], ())):
        _assert_mixed(types, nc, mixed)
        _run(ctx, oracle, bd, w, h, types)


@pytest.mark.parametrize("bd", [8, 10])
def test_8x16_column_and_row_classes_differ(ctx, oracle, bd):
    w, h = 8, 16
    nc, n = 4, 5
    for t in (ADST_DCT, DCT_ADST, V_DCT, H_DCT, FLIPADST_DCT):
        _run(ctx, oracle, bd, w, h, [t] * n)
    types = [ADST_DCT, DCT_ADST, ADST_DCT, FLIPADST_FLIPADST, V_DCT]
    _assert_mixed(types, nc, (0,))
    _run(ctx, oracle, bd, w, h, types)

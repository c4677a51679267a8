"""Every forward-transform path of the device against tests/golden/fwd_tx_ref.npz: coefficients the reference's
`forward_transform` produced when its text was executed whole (gen_fwd_tx_ref.py), on blocks built to reach what
the narrow arithmetic of the fused kernels can hold -- the separable worst-case sign block, constants,
alternations, a small mostly odd and negative block, an impulse, zero -- next to a random one.  No oracle stands
between the kernels and these numbers in legs 1 and 2; leg 3 puts the fixture's coefficients through the oracle's
quantizer, which quant_ref.npz pins on its own.

  leg 1  k_fwd_tx: all blocks of a case in one launch, tiled to the ragged counts of test_fwd_txfm_batch_vs_oracle
         (67 / 9; 10 or 11 where a case of more than 256 pixels holds ten blocks), so later waves,
         every block slot of a wave and the tail meet the fixture; both widths at 8 bits.
  leg 2  k_rdo_cand without a quantizer (the m24 networks): src = max(res, 0), ref = max(-res, 0), zero fractions,
         so the residual is the fixture's block.  Once per case with one type for every candidate (the scalar arm of
         the wave's vote for sides <= 16), once per size with the types of all its cases interleaved (the per-lane
         arm).  The candidate's type lives in device memory where the entry point cannot read it, and the kernel's
         shifts are those of the sixteen types of the tx sets: WHT is not offered to this entry point (the header
         calls such a candidate's result unspecified) and its only device path is leg 1.
  leg 3  the type search (int16 column tile up to 16x16, 24-bit quantizer): dense `pred`, the full inter mask of
         the size so that column groups share a tile, transform-domain distortion, at qindex 1 (the smallest that
         is lossy: 0 is the reference's lossless mode) and 100 -- and at 0 as well, which the entry point takes
         like any other index (the smallest divisors of the tables: the largest quantized values).  A type the
         size's mask does not hold (WHT; 16x16 has the twelve types of its inter set) is refused by the entry
         point, and the refusal is asserted.

Each leg counts its (case, block) comparisons and asserts the total."""
import functools

import numpy as np
import pytest

import fwd_tx_ref_util as U
import oracle_lib as O
from test_gpu_parity import TX_SIZES, dev_plane

pytestmark = pytest.mark.gpu

NBLOCKS = 1591          # per bit depth: 157 cases of ten blocks, 3 of seven
NBLOCKS_WHT = 10
NBLOCKS_16X16_OUTSIDE_INTER_SET = 40    # tx types 12..15 at 16x16


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _by_size(bd):
    out = {}
    for c in U.load()[bd]:
        assert TX_SIZES[c.ts] == (c.w, c.h)
        out.setdefault(c.ts, []).append(c)
    return out


def _off_wave_multiple(n, nc):
    return n + 1 if nc > 1 and n % nc == 0 else n


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_fwd_tx_kernel_batched(ctx, bd):
    compared = 0
    for c in U.load()[bd]:
        # the ragged counts of test_fwd_txfm_batch_vs_oracle, raised where a case holds more blocks than that and
        # kept off the multiple of the 64 / max(w, h) blocks a wave owns
        n = _off_wave_multiple(max(67 if c.w * c.h <= 256 else 9, len(c.res)), 64 // max(c.w, c.h))
        res, want = U.tiled(c, n)
        dres = _t(res)
        for cb in ((2, 4) if bd == 8 else (4,)):
            got = ctx.forward_transform_batch(dres, c.ts, c.tt, bd, cb).cpu().numpy()
            assert got.dtype == (np.int16 if cb == 2 else np.int32)
            bad = np.flatnonzero((got != want).any(1))
            assert not len(bad), (bd, c.ts, c.tt, cb, [(int(i), c.names[i % len(c.names)]) for i in bad])
        compared += len(set(np.arange(n) % len(c.res)))        # the distinct blocks this launch held
    assert compared == NBLOCKS


class _Size:
    """The distinct residual blocks of one (bit depth, tx_size) as a source and a reference plane on the device:
    the blocks every type shares, then the sign block of each case."""

    def __init__(self, bd, cases):
        self.bd, self.cases = bd, cases
        c0 = cases[0]
        self.w, self.h, self.ts = c0.w, c0.h, c0.ts
        self.nshared = len(c0.res) - 1
        for c in cases:
            assert np.array_equal(c.res[1:], c0.res[1:])
        self.blocks = np.concatenate([c0.res[1:]] + [c.res[:1] for c in cases]).astype(np.int64)
        k = len(self.blocks)
        cols = 5
        rows = (k + cols - 1) // cols
        self.src = O.HostPlane(cols * self.w, rows * self.h, bd)
        self.ref = O.HostPlane(cols * self.w, rows * self.h, bd)
        self.x = (np.arange(k) % cols) * self.w
        self.y = (np.arange(k) // cols) * self.h
        for i, b in enumerate(self.blocks):
            sl = (slice(self.y[i], self.y[i] + self.h), slice(self.x[i], self.x[i] + self.w))
            self.src.view()[sl] = np.maximum(b, 0)
            self.ref.view()[sl] = np.maximum(-b, 0)
        self.sad = np.abs(self.blocks).sum((1, 2))          # int64
        self.dsrc, self.dref = dev_plane(self.src), dev_plane(self.ref)

    def distinct(self, ci, j):
        """index into self.blocks of block j of case ci"""
        return self.nshared + ci if j == 0 else j - 1

    def cands(self, idx, types):
        c = np.zeros(len(idx), O.RDO_CAND)
        c["ox"] = c["rx"] = self.x[idx]
        c["oy"] = c["ry"] = self.y[idx]
        c["tx_type"] = types
        return c


@functools.lru_cache(maxsize=None)
def _sizes(bd):
    return {ts: _Size(bd, cases) for ts, cases in _by_size(bd).items()}


def _check_cand(ctx, s, ci_of, j_of, key):
    """one k_rdo_cand launch: candidate i is block j_of[i] of case ci_of[i], carrying that case's type"""
    idx = np.array([s.distinct(ci, j) for ci, j in zip(ci_of, j_of)])
    c = s.cands(idx, [s.cases[ci].tt for ci in ci_of])
    o = ctx.rdo_cand_batch(s.dsrc, s.dref, s.w, s.h, c, want_satd=False)
    sad = o["sad"].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(sad, s.sad[idx]), (key, "sad")
    got = o["coeffs"].cpu().numpy()
    want = np.stack([s.cases[ci].coef[j] for ci, j in zip(ci_of, j_of)])
    assert got.dtype == want.dtype
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), (key, [(int(i), s.cases[ci_of[i]].tt, s.cases[ci_of[i]].names[j_of[i]]) for i in bad])


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_fused_candidate_raw_coefficients(ctx, bd):
    uniform = mixed = 0
    for ts, s in _sizes(bd).items():
        nc = 64 // max(s.w, s.h)        # candidates of a wave
        live = [ci for ci, c in enumerate(s.cases) if c.tt != 16]
        nb = s.nshared + 1
        # one type for every candidate of the launch
        for ci in live:
            n = _off_wave_multiple(max(3 * nc + 1, nb), nc)
            _check_cand(ctx, s, [ci] * n, [i % nb for i in range(n)], (bd, ts, s.cases[ci].tt, "uniform"))
            uniform += nb
        # the types of all cases in turn: every wave of two or more candidates holds more than one type
        n = _off_wave_multiple(len(live) * nb, nc)
        ci_of = [live[i % len(live)] for i in range(n)]
        j_of = [(i // len(live)) % nb for i in range(n)]
        if len(live) > 1 and nc > 1:
            types = [s.cases[ci].tt for ci in ci_of]
            assert all(len(set(types[i:i + nc])) > 1 for i in range(0, n - 1, nc))
        assert {(ci, j) for ci, j in zip(ci_of, j_of)} == {(ci, j) for ci in live for j in range(nb)}
        _check_cand(ctx, s, ci_of, j_of, (bd, ts, "interleaved"))
        mixed += len(live) * nb
    assert uniform == mixed == NBLOCKS - NBLOCKS_WHT


@pytest.mark.parametrize("qindex", [0, 1, 100])
@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_type_search_quantizes_reference_coefficients(ctx, oracle, bd, qindex):
    from rav1e_amd.api import R1Error
    ct = np.int16 if bd == 8 else np.int32
    pt = np.uint8 if bd == 8 else np.uint16
    compared = refused = 0
    for ts, s in _sizes(bd).items():
        mask = ctx.tx_type_mask(ts, True, rav1e_types_only=False)
        k = len(s.blocks)
        c = s.cands(np.arange(k), 0)                         # the type field is ignored
        pred = _t(np.maximum(-s.blocks, 0).astype(pt).view(np.uint8 if bd == 8 else np.int16))
        o = ctx.rdo_txsearch_batch(s.dsrc, None, s.w, s.h, c, mask, qindex, 0, want_qcoeffs=True, pred=pred)
        eob = o["eob"].cpu().numpy().view(np.uint16)
        qco = o["qcoeffs"].cpu().numpy()
        area = min(s.w, 32) * min(s.h, 32)
        assert qco.shape == (k, bin(mask).count("1"), area) and qco.dtype == ct
        for ci, case in enumerate(s.cases):
            nb = len(case.res)
            if not (mask >> case.tt) & 1:
                with pytest.raises(R1Error):
                    ctx.rdo_txsearch_batch(s.dsrc, None, s.w, s.h, c, 1 << case.tt, qindex, 0, pred=pred)
                refused += nb
                continue
            slot = bin(mask & ((1 << case.tt) - 1)).count("1")
            co = np.ascontiguousarray(case.coef)
            wq, wr = np.zeros((nb, area), ct), np.zeros((nb, area), ct)
            weob, wd, wrate = np.zeros(nb, np.uint16), np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
            assert oracle.r1o_quantize_rdo_batch(O.ptr(co), s.w * s.h, nb, ts, case.tt, qindex, bd, 0, 0, 0,
                                                 co.itemsize, O.ptr(wq), O.ptr(weob), O.ptr(wr), O.ptr(wd),
                                                 O.ptr(wrate)) == 0
            idx = np.array([s.distinct(ci, j) for j in range(nb)])
            key = (bd, ts, case.tt, qindex)
            bad = np.flatnonzero(eob[idx, slot] != weob)
            assert not len(bad), (key, "eob", [case.names[j] for j in bad])
            bad = np.flatnonzero((qco[idx, slot] != wq).any(1))
            assert not len(bad), (key, "qcoeffs", [case.names[j] for j in bad])
            compared += nb
    assert refused == NBLOCKS_WHT + NBLOCKS_16X16_OUTSIDE_INTER_SET
    assert compared == NBLOCKS - refused

"""The oracle against tests/golden/inv_path_ref.npz: reconstructions the reference's `encode_tx_block` produced when
its text was executed whole (gen_inv_path_ref.py) on the blocks of fwd_tx_ref.npz at qindex 1 and 255 -- the largest
quantized levels and the largest steps the quantizer can hand to dequantize -> inverse_transform_add.

oracle/inv_tx_1d.inc and the product's copy are the same text, so every GPU-vs-oracle test of a reconstruction
compares the 1-D networks with themselves; this file is what those tests rest on.  It also asserts, from the counts
the generator observed in the executed run, how far the fixture reaches (docs/PARITY.md has the table and what the
quantizer cannot reach)."""
import ctypes as C

import numpy as np
import pytest

import intra_split_util as SU
import inv_path_ref_util as U
import oracle_lib as O

NBLOCKS = 1750          # per bit depth: 1666 of the plain family (98 of them with intra offsets), 84 flat
NSPLIT = 8              # per bit depth: four block sizes at two qindex
SPLIT_TX = 32


def _block_plane(a, bd):
    h, w = a.shape
    p = O.HostPlane(w, h, bd, 8, 8)
    p.view()[:] = a
    return p


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_oracle_reproduces_the_executed_chain(oracle, bd):
    """per block three comparisons: r1o_rdo_pixel_cand_batch on (source, dense prediction) -> eob, quantized
    coefficients, reconstruction, and with R1_DIST_WSSE the sum of squared differences against the fixture's
    reconstruction; r1o_dequantize on the stored levels -> the stored rcoeffs; r1o_inv_txfm_add_batch on the stored
    rcoeffs -> the stored reconstruction"""
    hbd = int(bd > 8)
    ct, dt = (np.int32, np.uint16) if hbd else (np.int16, np.uint8)
    compared = 0
    for b in U.load():
        if b.bd != bd:
            continue
        key = (b.family, bd, b.ts, b.tt, b.qindex, b.is_intra, b.name)
        area = min(b.w, 32) * min(b.h, 32)
        org = _block_plane(b.src, bd)
        pa = org.cstruct()
        c = np.zeros(1, O.RDO_CAND)
        c["tx_type"] = b.tt
        eob, dist = np.zeros(1, np.uint16), np.zeros(1, np.uint64)
        qc, rec = np.zeros(area, ct), np.zeros((b.h, b.w), dt)
        pred = np.ascontiguousarray(b.pred)
        assert oracle.r1o_rdo_pixel_cand_batch(C.byref(pa), None, b.w, b.h, b.ts, O.ptr(c), 1, b.qindex, b.is_intra, 0, 0,
                                               2, None, 0, 0, 0, None, None, O.ptr(eob), O.ptr(dist), O.ptr(qc),
                                               O.ptr(rec), O.ptr(pred)) == 0
        assert int(eob[0]) == b.eob, (key, "eob")
        assert np.array_equal(qc, b.qc), (key, "qcoeffs")
        assert np.array_equal(rec, b.rec), (key, "rec")
        assert int(dist[0]) == int(((b.src.astype(np.int64) - b.rec) ** 2).sum()), (key, "dist")
        compared += 1
        want_qc = np.ascontiguousarray(b.qc)
        dq = np.zeros(area, ct)
        oracle.r1o_dequantize(O.ptr(want_qc), O.ptr(dq), b.ts, b.qindex, bd, 0, 0, hbd)
        assert np.array_equal(dq, b.dq), (key, "dequantize")
        compared += 1
        want_dq = np.ascontiguousarray(b.dq)
        rec2 = np.zeros((b.h, b.w), dt)
        assert oracle.r1o_inv_txfm_add_batch(O.ptr(want_dq), area, O.ptr(pred), O.ptr(rec2), 1, b.ts, b.tt, bd,
                                             ct().itemsize, dt().itemsize) == 0
        assert np.array_equal(rec2, b.rec), (key, "inverse_transform_add")
        compared += 1
    assert compared == 3 * NBLOCKS


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_oracle_reproduces_the_split_loop(oracle, bd):
    """the split-loop cases through the oracle's composition of tests/intra_split_util.py (edges -> prediction -> one
    transform block -> scatter, block k + 1 predicted from what block k left): eob, levels and the block's
    reconstruction; r1o_dequantize on the stored levels of every transform block"""
    hbd = int(bd > 8)
    compared = txs = 0
    for s in U.load_splits():
        if s.bd != bd:
            continue
        key = (bd, s.bs, s.ts, s.tt, s.mode, s.qindex)
        mid = 1 << (bd - 1)
        org = O.HostPlane(s.plane_w, s.plane_h, bd, 16, 16, fill=mid)
        org.view()[s.y:s.y + s.bs, s.x:s.x + s.bs] = s.src
        rec = O.HostPlane(s.plane_w, s.plane_h, bd, 16, 16, fill=mid)
        cands = np.zeros(1, SU.SPLIT_CAND)
        cands["x"], cands["y"], cands["mode"] = s.x, s.y, s.mode
        o = SU.oracle_split(oracle, org, rec, (0, 0, s.plane_w, s.plane_h), s.bs, s.bs, s.ts, cands, False, 1 << s.tt,
                            s.qindex, 2)
        assert np.array_equal(o["eob"][0, 0], s.eob), (key, "eob")
        assert np.array_equal(o["qcoeffs"][0, 0], s.qc), (key, "qcoeffs")
        assert np.array_equal(o["rec"][0, 0], s.rec), (key, "rec")
        assert int(o["dist"][0, 0]) == int(((s.src.astype(np.int64) - s.rec) ** 2).sum()), (key, "dist")
        compared += 1
        for k in range(s.ntx):
            q = np.ascontiguousarray(s.qc[k])
            dq = np.zeros_like(q)
            oracle.r1o_dequantize(O.ptr(q), O.ptr(dq), s.ts, s.qindex, bd, 0, 0, hbd)
            assert np.array_equal(dq, s.dq[k]), (key, k, "dequantize")
            txs += 1
    assert (compared, txs) == (NSPLIT, SPLIT_TX)


# What the executed run reached, per bit depth: written down from the committed fixture so that a regenerated one
# cannot quietly lose reach.  (blocks whose pixel clamp engaged, pixels it changed) of the plain and flat families;
# pixels the clamp changed in the split-loop cases; column-pass clamp_value calls that changed their argument in the
# split-loop cases.
REACH = {8: (906, 29811, 2086, 0), 10: (974, 31672, 2142, 2), 12: (1212, 41697, 3010, 0)}
# The largest |quantized level| of the fixture (the families, the split loop): docs/PARITY.md records them next to the
# 389 of rdo_intra_ref.npz.  Printed, not a threshold: the values follow from the blocks and qindex 1.
LARGEST_LEVEL = {8: (4080, 3056), 10: (14549, 10904), 12: (43680, 32735)}


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_reach_of_the_fixture(bd):
    blocks = [b for b in U.load() if b.bd == bd]
    splits = [s for s in U.load_splits() if s.bd == bd]
    assert len(blocks) == NBLOCKS and len(splits) == NSPLIT
    # every size x type of the families at both qindex, nothing dropped or thinned by strict mode
    assert {b.qindex for b in blocks} == set(U.QINDEX)
    assert not any(b.halvings or b.strict_trips for b in blocks) and not any(s.halvings for s in splits)
    # the pixel clamp engaged in some case of every size
    for ts in range(19):
        assert any(b.pix_clamps for b in blocks if b.ts == ts and b.family == U.PLAIN), (bd, ts)
    got = (sum(b.pix_clamps > 0 for b in blocks), sum(b.pix_clamps for b in blocks),
           sum(int(s.pix_clamps.sum()) for s in splits), sum(int(s.col_clamps.sum()) for s in splits))
    print("bit depth", bd, "reach", got)
    assert all(g >= w for g, w in zip(got, REACH[bd])), (got, REACH[bd])
    # levels of both signs, blocks that quantize to nothing and blocks that fill the coded area
    assert any((b.qc < 0).any() for b in blocks) and any(b.eob == 0 for b in blocks)
    assert any(b.eob == min(b.w, 32) * min(b.h, 32) for b in blocks)
    lv = (max(int(np.abs(b.qc.astype(np.int64)).max()) for b in blocks),
          max(int(np.abs(s.qc.astype(np.int64)).max()) for s in splits))
    print("bit depth", bd, "largest |level|: families", lv[0], "split loop", lv[1])
    assert lv[0] >= LARGEST_LEVEL[bd][0] and lv[1] >= LARGEST_LEVEL[bd][1]

"""tests/golden/rdo_intra_split_ref.npz without a GPU: the composition r1_rdo_intra_split_batch is specified as
(tests/intra_split_util.oracle_split: r1o_get_intra_edges -> r1o_predict_intra -> r1o_rdo_txsearch_batch -> store, per
transform block on a private copy of the reconstruction) reproduces every array the reference's encode_tx_block left
when it was executed over the transform blocks of an intra block; and the host glue builds the descriptors."""
import numpy as np
import pytest

import intra_split_util as SU
import rdo_intra_split_cases as SC


@pytest.fixture(scope="module")
def cases():
    return SC.load()


def test_fixture_covers_what_it_claims(cases):
    assert len(cases) >= 40
    assert {c.mode for c in cases if (c.bw, c.bh, c.ts, c.bd) == (8, 8, 0, 8)} == set(range(13))
    shapes = {(c.bw, c.bh, c.t) for c in cases}
    assert {(16, 16, 4), (16, 16, 8), (32, 32, 16), (32, 32, 8), (64, 64, 32), (64, 64, 16), (16, 8, 8), (8, 16, 8),
            (16, 8, 4), (16, 4, 4)} <= shapes
    assert {c.bd for c in cases} == {8, 10, 12}
    assert len({c.tx_type for c in cases}) >= 3
    assert {c.enable_ief for c in cases} == {0, 1} and {c.ief for c in cases} == {0, 1, 2}
    # cut by the frame edge: a skipped last column, and a last column that is partly visible
    assert any(c.skipped.any() and c.vis_w % c.t == 0 and c.vis_w < c.bw for c in cases)
    assert any(0 < c.vis_w % c.t for c in cases)
    assert any(c.vis_h < c.bh for c in cases)
    assert any(c.tr.any() for c in cases) and any(c.bl.any() for c in cases)
    assert any((c.eob == 0)[~c.skipped].any() for c in cases) and any((c.eob != 0).all() for c in cases)


def test_oracle_composition_reproduces_the_fixture(cases, oracle):
    """eob, qcoeffs, the final reconstruction (over the transform blocks that are not skipped), the transform-domain
    distortion per transform block, and the four pixel-domain distortions -- directly where the block lies inside the
    frame, and for every case over the visible part of the composition's reconstruction (compute_distortion clips)"""
    import ctypes as C
    import oracle_lib as O
    for c in cases:
        org, rec = c.org_plane(), c.rec_plane()
        cands = np.zeros(1, SU.SPLIT_CAND)
        tr, bl = c.masks()
        cands[0] = (c.x, c.y, c.mode, c.angle_delta, c.ief, 0, tr, bl)
        mask = 1 << c.tx_type
        key = (c.i, c.bd, c.bw, c.bh, c.t, c.mode, c.angle_delta)
        o = SU.oracle_split(oracle, org, rec, c.tile, c.bw, c.bh, c.ts, cands, c.enable_ief, mask, c.qidx, 0)
        assert np.array_equal(o["eob"][0, 0], c.eob), (key, "eob")
        assert np.array_equal(o["qcoeffs"][0, 0].astype(np.int64), c.qc.astype(np.int64)), (key, "qcoeffs")
        assert np.array_equal(o["dist"][0, 0], c.txd), (key, "transform-domain distortion")
        assert np.array_equal(o["rec"][0, 0][c.coded_mask], c.rec[c.coded_mask]), (key, "rec")
        for j, (kind, scaled) in enumerate(SC.DIST_RUNS):
            sc = c.scales if scaled else None
            o = SU.oracle_split(oracle, org, rec, c.tile, c.bw, c.bh, c.ts, cands, c.enable_ief, mask, c.qidx, kind, sc)
            assert np.array_equal(o["eob"][0, 0], c.eob), (key, "eob", kind)
            if c.inside:
                assert int(o["dist"][0, 0]) == int(c.dist[j]), (key, "dist", j)
            # the visible part, from the reconstruction (what the header tells the caller to do at a frame edge)
            bp = O.HostPlane(c.bw, c.bh, c.bd, 0, 0)
            bp.data[:c.bh, :c.bw] = o["rec"][0, 0]
            dc = np.zeros(1, O.DIST_CAND)
            dc["ox"], dc["oy"] = c.x, c.y
            pa, pb, d = org.cstruct(), bp.cstruct(), np.zeros(1, np.uint64)
            assert oracle.r1o_dist_scaled_batch(kind, C.byref(pa), C.byref(pb), c.vis_w, c.vis_h, O.ptr(dc), 1,
                                                O.ptr(sc) if scaled else None, sc.shape[1] if scaled else 0, 0, 0,
                                                O.ptr(d)) == 0
            assert int(d[0]) == int(c.dist[j]), (key, "visible dist", j)


def test_glue_builds_the_descriptors(cases):
    from rav1e_amd.rdo_glue import intra_split_cands, intra_split_masks, sub_tx_size, tx_split_blocks
    from rav1e_amd.types import TxSize
    for c in cases:
        d = intra_split_cands(c.blocks(), c.bw, c.bh, c.ts)
        tr, bl = c.masks()
        assert (int(d["x"][0]), int(d["y"][0]), int(d["mode"][0]), int(d["angle_delta"][0]), int(d["ief"][0]),
                int(d["tr_mask"][0]), int(d["bl_mask"][0])) == (c.x, c.y, c.mode, c.angle_delta, c.ief, tr, bl), c.i
        assert d.dtype.itemsize == 12
        # the transform blocks the loop visits are rdo_glue.tx_split_blocks'
        visited = [k for k, _, _ in tx_split_blocks(c.x >> 2, c.y >> 2, c.bw, c.bh, c.t, c.t, (c.plane_w + 3) >> 2,
                                                    (c.plane_h + 3) >> 2)]
        assert visited == [k for k in range(c.ntx) if not c.skipped[k]], c.i
        # the availability masks, as the glue computes them (a skipped transform block was never asked in the fixture)
        keep = sum(1 << k for k in range(c.ntx) if not c.skipped[k])
        m = intra_split_masks(c.bw, c.bh, c.ts, c.x >> 2, c.y >> 2, c.x, c.y, c.plane_w, c.plane_h)
        assert (m[0] & keep, m[1] & keep) == (tr, bl), c.i
    # sub_tx_size_map, all 19 entries (src/context/transform_unit.rs:85-105)
    want = ["4X4", "4X4", "8X8", "16X16", "32X32", "4X4", "4X4", "8X8", "8X8", "16X16", "16X16", "32X32", "32X32", "4X8",
            "8X4", "8X16", "16X8", "16X32", "32X16"]
    assert [sub_tx_size(t).name for t in TxSize] == ["TX_" + w for w in want]


def test_availability_sweep():
    """has_top_right / has_bottom_left of the glue against the reference's executed answers: every block size up to
    64x64, every transform size in scope, every transform block, every aligned position of three superblocks of a
    192x192 frame (first row / column, inside, against the right / bottom edge)"""
    from rav1e_amd.rdo_glue import has_bottom_left, has_top_right
    G = np.load(SC.PATH)
    S = G["sweep"].astype(int)
    assert len(S) > 10000 and 0.2 < S[:, 7].mean() < 0.8 and 0.2 < S[:, 8].mean() < 0.8
    assert {(int(r[0]), int(r[1]), SC.TX_SIDE[int(r[2])]) for r in S} >= {
        (8, 8, 4), (16, 16, 4), (16, 16, 8), (32, 32, 8), (32, 32, 16), (64, 64, 16), (64, 64, 32), (16, 8, 8), (8, 16, 8),
        (16, 4, 4), (4, 16, 4), (64, 16, 16), (16, 64, 16), (32, 8, 8), (8, 32, 8), (64, 32, 32), (32, 64, 32)}
    frame = 192
    for bw, bh, ts, x, y, bx, by, tr, bl in S:
        t = SC.TX_SIDE[ts]
        xk, yk, bx4, by4 = x + bx * t, y + by * t, bx * (t >> 2), by * (t >> 2)
        key = (bw, bh, t, x, y, bx, by)
        assert has_top_right(bw, bh, x >> 2, y >> 2, by4 != 0 or y > 0, xk + t < frame, t, by4, bx4) == bool(tr), key
        assert has_bottom_left(bw, bh, x >> 2, y >> 2, yk + t < frame, bx4 != 0 or x > 0, t, by4, bx4) == bool(bl), key

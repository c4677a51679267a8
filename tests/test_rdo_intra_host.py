"""r1_rdo_intra_cand_batch without a device: the exported symbol, the signature against the header, and every
argument refusal -- all of them come before anything touches a device, so a stand-in context (a zeroed block of
memory the checks only take addresses in) is enough to reach them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_library_exports_intra_cand_symbol():
    from rav1e_amd import _lib
    assert "r1_rdo_intra_cand_batch" in _lib.SYMBOLS
    L = _lib.load()
    assert L.r1_rdo_intra_cand_batch.restype is C.c_int
    assert L.r1_abi_version() == 7          # an addition under ABI 7


def test_signature_matches_the_header():
    """the ctypes argument list has one entry per parameter of the header's declaration, pointers where the header
    has pointers"""
    from rav1e_amd import _lib
    text = open(os.path.join(ROOT, "include", "rav1e_amd.h")).read()
    m = re.search(r"\bint r1_rdo_intra_cand_batch\((.*?)\);", text, re.S)
    assert m, "the header declares r1_rdo_intra_cand_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SYMBOLS["r1_rdo_intra_cand_batch"]
    assert res is C.c_int and len(args) == len(params) == 29
    for p, a in zip(params, args):
        is_ptr = "*" in p
        assert is_ptr == (a in (C.c_void_p, C.POINTER(_lib.R1Plane), C.POINTER(_lib.R1QuantParams))), (p, a)
    assert [p.split()[-1].lstrip("*") for p in params][5:13] == ["cands", "n", "edge_group", "pos_xy", "edges",
                                                                 "edge_stride", "lens", "ac"]


class Call:
    """a valid call (8x8, 8-bit, 10 candidates in 2 groups of 5) on host memory with a stand-in context; `go` applies
    overrides by parameter name and returns the status"""

    def __init__(self):
        from rav1e_amd import _lib
        from rav1e_amd.api import INTRA_CAND
        self.L = _lib.load()
        self.fake_ctx = (C.c_uint8 * 65536)()
        self.pix = np.zeros((64, 64), np.uint8)
        self.plane = _lib.R1Plane(self.pix.ctypes.data, 64, 64, 32, 32, 16, 16, 1, 8)
        self.qp = _lib.R1QuantParams()
        self.qp.bit_depth = 8
        self.qp.qindex = 60
        self.cands = np.zeros(10, INTRA_CAND)
        self.cands["avail_w"], self.cands["avail_h"] = 8, 8
        self.pos = np.zeros((2, 2), np.int16)
        self.edges = np.zeros((2, 257), np.uint8)
        self.lens = np.zeros((2, 2), np.uint8)
        self.ac = np.zeros((10, 64), np.int16)
        self.eob = np.full(10 * 5, 0xBEEF, np.uint16)
        self.dist = np.zeros(10 * 5, np.uint64)
        self.names = ["ctx", "org", "w", "h", "tx_size", "cands", "n", "edge_group", "pos_xy", "edges", "edge_stride",
                      "lens", "ac", "tx_type_mask", "params", "dist_kind", "scales", "scale_stride", "xdec", "ydec",
                      "sad_out", "satd_out", "eob_out", "dist_out", "est_rate_out", "qcoeffs_out", "rec_out",
                      "pred_out", "stream"]

    def go(self, **over):
        p = lambda a: a.ctypes.data
        v = dict(ctx=C.addressof(self.fake_ctx), org=C.byref(self.plane), w=8, h=8, tx_size=1, cands=p(self.cands),
                 n=10, edge_group=5, pos_xy=p(self.pos), edges=p(self.edges), edge_stride=257, lens=p(self.lens),
                 ac=p(self.ac), tx_type_mask=0x20F, params=C.byref(self.qp), dist_kind=3, scales=None, scale_stride=0,
                 xdec=0, ydec=0, sad_out=None, satd_out=None, eob_out=p(self.eob), dist_out=p(self.dist),
                 est_rate_out=None, qcoeffs_out=None, rec_out=None, pred_out=None, stream=None)
        assert set(over) <= set(v), over
        v.update(over)
        rc = self.L.r1_rdo_intra_cand_batch(*[v[k] for k in self.names])
        assert (self.eob == 0xBEEF).all()      # nothing was written
        return rc


@pytest.fixture(scope="module")
def call():
    return Call()


def test_null_context_is_einval(call):
    assert call.go(ctx=None) == EINVAL


def test_empty_batch_is_ok_without_a_device(call):
    """n = 0 passes every check and launches nothing: the valid argument set really is valid"""
    assert call.go(n=0) == 0


@pytest.mark.parametrize("over", [
    # what r1_rdo_txsearch_batch rejects
    dict(org=None), dict(params=None), dict(eob_out=None), dict(dist_out=None), dict(tx_size=19), dict(tx_size=-1),
    dict(w=16), dict(h=4), dict(tx_type_mask=0), dict(tx_type_mask=0x10000), dict(dist_kind=1), dict(dist_kind=4),
    dict(xdec=2), dict(ydec=-1), dict(dist_kind=3, xdec=1), dict(scales=1, scale_stride=0),
    dict(dist_kind=0, rec_out=1), dict(dist_kind=3, est_rate_out=1),
    dict(tx_size=3, w=32, h=32, tx_type_mask=0x3),          # ADST has no 32-point kernel
    dict(tx_size=4, w=64, h=64, tx_type_mask=0x201),        # a 64-point side codes DCT_DCT only
    # the intra source
    dict(edge_group=0), dict(edge_group=-5), dict(edge_group=3), dict(edge_group=4), dict(edge_stride=256),
    dict(cands=None), dict(edges=None), dict(lens=None), dict(pos_xy=None),
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_bad_arguments_are_einval(call, over):
    assert call.go(**over) == EINVAL


def test_bit_depth_mismatch_is_einval(call):
    call.qp.bit_depth = 10
    try:
        assert call.go() == EINVAL
    finally:
        call.qp.bit_depth = 8


def test_cfl_mode_without_ac_is_einval(call):
    """mode 13 needs its AC block: refused where the host can read the descriptors"""
    call.cands["mode"][7] = 13
    try:
        assert call.go(ac=None) == EINVAL
    finally:
        call.cands["mode"][7] = 0


# ---- the reference-executed fixture (tests/golden/gen_rdo_intra_ref.py) against the oracle's entry points ----
@pytest.fixture(scope="module")
def cases():
    import rdo_intra_cases as RC
    return RC.load()


def test_fixture_loads_and_covers_the_branches(cases):
    assert 140 <= len(cases) <= 160
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rdo_intra_ref.npz")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "rdo_pixel_ref.npz"))
    luma = [c for c in cases if not c.chroma]
    assert {c.mode for c in luma} == set(range(13))
    assert {(c.mode, c.angle_delta) for c in luma if c.bd == 8 and c.ts == 1 and 1 <= c.mode <= 8} == \
        {(m, d) for m in range(1, 9) for d in (-3, 0, 3)}
    assert {(c.w, c.h) for c in luma} == {(4, 4), (8, 8), (16, 16), (4, 16), (16, 4), (32, 32), (64, 64), (64, 16)}
    assert {c.bd for c in luma} == {8, 10, 12} and {c.bd for c in luma if c.ts != 1} == {8, 10}
    assert {c.ief for c in luma} == {0, 1, 2} and {c.enable_ief for c in luma} == {0, 1}
    assert {c.variant for c in luma} == {0, 1, 2, 3}
    assert any(c.avail_w < c.w for c in luma) and any(c.avail_h < c.h for c in luma)
    assert {c.mode for c in cases if c.chroma} == {0, 13} and all((c.w, c.h, c.dec) == (8, 8, 1) for c in cases if c.chroma)
    # the question the fixture settles: where does the pre-screen's shared (no-mode) edge set predict differently?
    differ = [c for c in cases if not c.shared_ok]
    assert differ and all(c.enable_ief and c.w + c.h >= 24 and 90 < c.angle < 180 for c in differ)
    assert all(c.shared_ok for c in cases if not (c.enable_ief and c.w + c.h >= 24 and 90 < c.angle < 180))


def test_fixture_edges_equal_the_oracles_get_intra_edges(cases, oracle):
    import oracle_lib as O
    for c in cases:
        rec = c.rec_plane()
        got = np.zeros(257, c.dt)
        lens = (C.c_int * 2)()
        oracle.r1o_get_intra_edges(O.ptr(got), lens, rec.block_ptr(0, 0), rec.stride, c.x, c.y, c.plane_w, c.plane_h,
                                   c.ts, c.bd, c.mode, c.enable_ief, c.angle_delta, c.has_tr, c.has_bl, int(c.bd > 8))
        assert (lens[0], lens[1]) == (c.left_len, c.above_len), c.i
        lo, hi = 128 - c.left_len, 129 + c.above_len
        assert np.array_equal(got[lo:hi].astype(np.int64), c.edge[lo:hi].astype(np.int64)), c.i


def test_oracle_composition_reproduces_every_stored_output(cases, oracle):
    """r1o_dispatch_predict_intra on the fixture's edge buffer -> r1o_rdo_txsearch_batch: the prediction, eob,
    qcoeffs, reconstruction, the four pixel-domain distortions (blocks that lie whole inside the plane: the
    reference measures the visible part only) and the transform-domain distortion"""
    import oracle_lib as O
    for c in cases:
        w, h = c.w, c.h
        ct = np.int16 if c.bd == 8 else np.int32
        edge = c.edge.astype(c.dt)
        pred = np.zeros((1, h, w), c.dt)
        assert oracle.r1o_dispatch_predict_intra(
            c.pmode, c.variant, O.ptr(pred[0]), w, c.ts, c.bd, O.ptr(c.ac) if c.ac is not None else None, c.angle,
            c.ief, O.ptr(edge), c.left_len, c.above_len, c.avail_w, c.avail_h, int(c.bd > 8)) == 0
        assert np.array_equal(pred[0], c.pred), (c.i, "pred")
        org, grid, rc = c.org_plane(), c.scale_grid(), c.rdo_cand()
        pa = org.cstruct()
        carea = min(w, 32) * min(h, 32)

        def run(kind, scaled):
            eob, dist, rate = np.zeros(1, np.uint16), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
            qc, rec = np.zeros(carea, ct), np.zeros((h, w), c.dt)
            assert oracle.r1o_rdo_txsearch_batch(
                C.byref(pa), None, O.ptr(pred), w, h, c.ts, O.ptr(rc), 1, 1, c.qidx, 1, 0, 0, kind,
                O.ptr(grid) if scaled else None, grid.shape[1], c.dec, c.dec, None, None, O.ptr(eob), O.ptr(dist),
                O.ptr(rate) if kind == 0 else None, O.ptr(qc), O.ptr(rec) if kind else None) == 0
            assert int(eob[0]) == c.eob, (c.i, kind, "eob")
            assert np.array_equal(qc.astype(np.int64), c.qc.astype(np.int64)), (c.i, kind, "qcoeffs")
            if kind:
                assert np.array_equal(rec, c.rec), (c.i, kind, "rec")
            return int(dist[0])
        import rdo_intra_cases as RC
        if c.chroma:
            run(2, False)
        else:
            for j, (kind, scaled) in enumerate(RC.DIST_RUNS):
                d = run(kind, scaled)
                if c.inside:
                    assert d == int(c.dist[j]), (c.i, "dist", j, d, int(c.dist[j]))
        assert run(0, False) == int(c.txd[0]), (c.i, "tx-domain distortion")

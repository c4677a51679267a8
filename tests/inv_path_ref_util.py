"""Reader of tests/golden/inv_path_ref.npz and inv_path_ref_dq.npz (gen_inv_path_ref.py: `encode_tx_block` executed
whole from the reference's text on the residual blocks of fwd_tx_ref.npz).  A plain reader: nothing here computes a
coefficient or a pixel.  Shared by test_inv_path_ref.py and test_gpu_inv_path_ref.py; loaded once."""
import functools
import os
from collections import namedtuple

import numpy as np

import fwd_tx_ref_util as FU

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH, PATH_DQ = os.path.join(GOLD, "inv_path_ref.npz"), os.path.join(GOLD, "inv_path_ref_dq.npz")
BITDEPTHS = (8, 10, 12)
QINDEX = (1, 255)
PLAIN, FLAT = 0, 1

# One executed block.  res: the residual block the fixture was made from, (h, w) int64, already halved `halvings`
# times; src / pred / rec: (h, w) pixels; qc / dq: coded area, T::Coeff
Block = namedtuple("Block", "family bd ts tt qindex is_intra name halvings eob cast_changed row_clamps col_clamps "
                            "pix_clamps strict_trips w h res src pred qc dq rec")
# One case of the split loop.  src / rec: (bs, bs) pixels; eob: (ntx,); qc / dq: (ntx, t * t); the clamp counts per
# transform block
Split = namedtuple("Split", "bd bs ts tt mode qindex x y plane_w plane_h halvings t ntx src rec eob qc dq "
                            "cast_changed row_clamps col_clamps pix_clamps")


def pix_dtype(bd):
    return np.uint8 if bd == 8 else np.uint16


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def _residuals():
    """{(bd, ts, tt): {block name: (h, w) int64}}: the blocks of fwd_tx_ref.npz; the impulse, which that file does not
    hold above area 1024, as gen_fwd_tx_ref.py defines it"""
    out = {}
    for bd, cases in FU.load().items():
        for c in cases:
            d = {n: c.res[i].astype(np.int64) for i, n in enumerate(c.names)}
            imp = np.zeros((c.h, c.w), np.int64)
            imp[-1, -1] = -((1 << bd) - 1)
            assert "impulse" not in d or np.array_equal(d["impulse"], imp)
            d["impulse"] = imp
            out[bd, c.ts, c.tt] = d
    return out


@functools.lru_cache(maxsize=None)
@functools.lru_cache(maxsize=None)
def _files():
    """both files as plain dicts: a member is decompressed once"""
    with np.load(PATH) as G, np.load(PATH_DQ) as D:
        return {k: G[k] for k in G.files}, {k: D[k] for k in D.files}


@functools.lru_cache(maxsize=None)
def load():
    """-> [Block, ...] in stored order (bit depth, then family / size / type / qindex / block).  Arrays are
    read-only."""
    G, D = _files()
    cols = [str(c) for c in G["columns"]]
    assert cols == ["family", "bd", "tx_size", "tx_type", "qindex", "is_intra", "block", "halvings", "eob", "cast_changed",
                    "row_clamps", "col_clamps", "pix_clamps", "strict_trips"]
    names = [str(s) for s in G["names"]]
    resid = _residuals()
    pos = {bd: [0, 0] for bd in BITDEPTHS}
    out = []
    for row in G["blocks"]:
        family, bd, ts, tt, qindex, is_intra, b, halvings = (int(v) for v in row[:8])
        r = resid[bd, ts, tt][names[b]]
        h, w = r.shape
        res = np.sign(r) * (np.abs(r) >> halvings)
        area = min(w, 32) * min(h, 32)
        p = pos[bd]
        qc, dq = G["qc_%d" % bd][p[0]:p[0] + area], D["dq_%d" % bd][p[0]:p[0] + area]
        rms = G["rms_%d" % bd][p[1]:p[1] + w * h].reshape(h, w).astype(np.int64)
        p[0] += area
        p[1] += w * h
        mid = 1 << (bd - 1)
        if family == PLAIN:
            src, pred = np.maximum(res, 0), np.maximum(-res, 0)
        else:
            src, pred = mid + (res >> 1), np.full((h, w), mid, np.int64)
        rec = src + rms
        dt = pix_dtype(bd)
        assert 0 <= min(src.min(), pred.min(), rec.min()) and max(src.max(), pred.max(), rec.max()) < (1 << bd)
        src, pred, rec = src.astype(dt), pred.astype(dt), rec.astype(dt)
        _ro(res, src, pred, rec)
        out.append(Block(family, bd, ts, tt, qindex, is_intra, names[b], halvings, *(int(v) for v in row[8:14]),
                         w, h, res, src, pred, qc, dq, rec))
    for bd in BITDEPTHS:
        assert pos[bd] == [len(G["qc_%d" % bd]), len(G["rms_%d" % bd])], "inv_path_ref.npz: layout and table disagree"
        assert len(D["dq_%d" % bd]) == len(G["qc_%d" % bd])
    return out


def cases(family=None, bd=None):
    """{(family, bd, ts, tt, qindex, is_intra): [Block, ...]} in stored order"""
    out = {}
    for b in load():
        if (family is None or b.family == family) and (bd is None or b.bd == bd):
            out.setdefault((b.family, b.bd, b.ts, b.tt, b.qindex, b.is_intra), []).append(b)
    return out


@functools.lru_cache(maxsize=None)
def load_splits():
    G, D = _files()
    assert [str(c) for c in G["split_columns"]][:11] == ["bd", "block_size", "tx_size", "tx_type", "mode", "qindex", "x",
                                                         "y", "plane_w", "plane_h", "halvings"]
    assert [str(c) for c in G["split_tx_columns"]] == ["case", "k", "eob", "cast_changed", "row_clamps", "col_clamps",
                                                       "pix_clamps"]
    tx = G["split_tx"]
    pos = {bd: [0, 0] for bd in BITDEPTHS}
    out = []
    for ci, row in enumerate(G["split"]):
        bd, bs, ts, tt, mode, qindex, x, y, pw, ph, halvings = (int(v) for v in row[:11])
        t = (4, 8, 16, 32)[ts]
        ntx = (bs // t) ** 2
        mine = tx[tx[:, 0] == ci]
        assert np.array_equal(mine[:, 1], np.arange(ntx))
        p = pos[bd]
        qc = G["split_qc_%d" % bd][p[0]:p[0] + ntx * t * t].reshape(ntx, t * t)
        dq = D["split_dq_%d" % bd][p[0]:p[0] + ntx * t * t].reshape(ntx, t * t)
        src = G["split_src_%d" % bd][p[1]:p[1] + bs * bs].reshape(bs, bs).astype(np.int64)
        rec = src + G["split_rms_%d" % bd][p[1]:p[1] + bs * bs].reshape(bs, bs)
        p[0] += ntx * t * t
        p[1] += bs * bs
        dt = pix_dtype(bd)
        src, rec = src.astype(dt), rec.astype(dt)
        _ro(src, rec)
        out.append(Split(bd, bs, ts, tt, mode, qindex, x, y, pw, ph, halvings, t, ntx, src, rec,
                         mine[:, 2].astype(np.uint16), qc, dq, mine[:, 3], mine[:, 4], mine[:, 5], mine[:, 6]))
    for bd in BITDEPTHS:
        assert pos[bd] == [len(G["split_qc_%d" % bd]), len(G["split_src_%d" % bd])]
    return out


def tiled_index(nb, n):
    """n launch slots over nb blocks, round-robin"""
    return np.arange(n) % nb


def launch_count(w, h, nb):
    """the ragged block counts of the forward test: 67 up to area 256 and 9 above, raised to the case's block count and
    kept off a multiple of the 64 / max(w, h) blocks a wave owns"""
    n = max(67 if w * h <= 256 else 9, nb)
    nc = 64 // max(w, h)
    return n + 1 if nc > 1 and n % nc == 0 else n

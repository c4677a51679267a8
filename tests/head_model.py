"""TEST INFRASTRUCTURE: a Python-int model of r1_intra_head_rate_batch, r1_partition_rate_batch and
r1_intra_head_commit_batch -- rdo_glue's head statements (head_symbols, partition_symbol, head_nbr_store,
head_nbr_reset_left) written on coeff_rate_model's WriterCounter and update_cdf against a types.HEAD_CDF_CONTEXT record.

Pinned by tests/golden/head_ref.npz (tests/test_head_ref.py: every rate, rng, adapted CDF and context array of the
fixture); the GPU tests compare the library against it.  Nothing here is imported by the product.

`OFF` names one behaviour to turn off, for the sensitivity tests: each is a trap of the reference's head that a
restatement could drop without any other case noticing."""
import os

import numpy as np

from coeff_rate_model import Counter, update_cdf
from rav1e_amd import rdo_glue as G
from rav1e_amd.types import HEAD_CDF_CONTEXT, HEAD_NBR_CONTEXT, BlockSize

INVALID = 0xFFFFFFFF
OFF = set()     # of: "angle_shared_row", "cfl_shared_row", "small_rows", "rect_partition", "sub8", "tile_relative", "edge_gather"


def cdf_record(packed):
    """one HEAD_CDF_CONTEXT record (a copy) from the fixture's packed uint16 row"""
    return np.array(packed, np.uint16).view(HEAD_CDF_CONTEXT)[0].copy()


def nbr_record(packed):
    return np.array(packed, np.uint8).view(HEAD_NBR_CONTEXT)[0].copy()


def nbr_arrays(rec):
    """the dict of arrays rdo_glue's statements take; views of the record, so stores land in it"""
    return {n: rec[n] for n in HEAD_NBR_CONTEXT.names}


def _row(cdf, field, row):
    a = cdf[field]
    for i in (row if isinstance(row, tuple) else (row,)):
        a = a[i]
    return a


def _gather(row, which):
    """partition_gather_vert_alike (2) / _horz_alike (1): out[0] of the two-entry CDF (partition_unit.rs:131-193) with
    cdf_element_prob (cdf_context.rs:721-724) over the ten-entry row"""
    n = len(row)
    prob = lambda e: (int(row[e - 1]) if e > 0 else 32768) - (int(row[e]) if e + 1 < n else 0)
    return sum(prob(e) for e in G._PARTITION_GATHER[which]) & 0xFFFF


def write(w, cdf, sym, adapt):
    """one symbol of a head on counter w; adapt: update the row in `cdf` behind it (symbol_with_update!)"""
    field, row, n, s, gather = sym
    r = _row(cdf, field, row)
    if gather and "edge_gather" not in OFF:             # (off: as if the edge wrote on the row itself, with its update)
        w.symbol(s, (_gather(r, gather), 0))
        return
    vals = [int(v) for v in r[:n]]
    w.symbol(s, vals)
    if adapt:
        update_cdf(vals, s)
        r[:n] = vals


def _mutated(syms, bo_x, bo_y):
    """the symbol list with the behaviours named in OFF turned off"""
    out = []
    for (field, row, n, s, g) in syms:
        if "small_rows" in OFF:
            if field == "partition_w8":
                field, n = "partition", 10
            if field == "tx_size_8x8":
                field, row, n = "tx_size", (0, row), 3
            elif field == "tx_size" and row[0] == 2:     # as if 64x64 shared the 32x32 category
                row = (1, row[1])
        out.append((field, row, n, s, g))
    return out


def symbols(nbr, blk, tr, coded=False):
    """rdo_glue.head_symbols of a block (bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma, tx_mode_select) and a trial
    (y_mode, uv_mode, angle_y, angle_uv, alpha_u, alpha_v, tx_size); coded: the winner as the commit replays it"""
    bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma, tms = [int(v) for v in blk]
    if "tile_relative" in OFF:       # as if `above` / `left` existed wherever the arrays hold something
        syms = G.head_symbols(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma, tms, *tr, coded=coded)
        if syms != G.HEAD_REFUSED:
            fixed = []
            for (field, row, n, s, g) in syms:
                if field == "skip":
                    row = int(bool(nbr["above_skip"][bo_x])) + int(bool(nbr["left_skip"][bo_y % 16]))
                if field == "kf_y":
                    row = (G._INTRA_MODE_CONTEXT[int(nbr["above_mode"][bo_x]) % 13],
                           G._INTRA_MODE_CONTEXT[int(nbr["left_mode"][bo_y % 16]) % 13])
                fixed.append((field, row, n, s, g))
            syms = fixed
        return syms
    syms = G.head_symbols(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma, tms, *tr, coded=coded)
    if syms == G.HEAD_REFUSED:
        return syms
    w, h = BlockSize(bsize).dims
    if "rect_partition" in OFF and w != h and bsize >= 3 and not coded:
        # as if a rectangle wrote PARTITION_NONE like the square of its long side
        p = G.partition_symbol(nbr, G.block_size(max(w, h), max(w, h)), bo_x, bo_y, mi_cols, mi_rows, 0)
        if isinstance(p, tuple):
            syms = [p] + syms
    if "sub8" in OFF and min(BlockSize(bsize).dims) < 8 and 1 <= int(tr[0]) <= 8 and int(bsize) < 3:
        # as if a block below 8x8 wrote its luma angle delta too
        k = next(i for i, sy in enumerate(syms) if sy[0] == "kf_y")
        syms = syms[:k + 1] + [("angle_delta", int(tr[0]) - 1, 7, int(tr[2]) + 3, 0)] + syms[k + 1:]
    return _mutated(syms, bo_x, bo_y)


def head_rate(cdf, syms, rng0=0x8000):
    """-> (rate in 1/8 bit, rng behind the head) on a fresh counter; `cdf` is not written (the trial's rollback)"""
    if syms == G.HEAD_REFUSED:
        return INVALID, None
    scratch = cdf.copy()
    w = Counter()
    w.rng = rng0
    tell = w.tell_frac()
    seen = set()
    for sym in syms:
        key = (sym[0], sym[1])
        again = key in seen
        seen.add(key)
        if again and ((sym[0] == "angle_delta" and "angle_shared_row" in OFF) or (sym[0] == "cfl_alpha" and "cfl_shared_row" in OFF)):
            write(w, cdf.copy(), sym, False)       # the second symbol on the row as it stood in front of the first
        else:
            write(w, scratch, sym, True)
    return w.tell_frac() - tell, w.rng


def head_commit(cdf, syms):
    """the winner's replay: its symbols adapt `cdf` in place"""
    assert syms != G.HEAD_REFUSED
    w = Counter()
    for sym in syms:
        write(w, cdf, sym, True)


def partition_rate(cdf, nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, partition, rng0=0x8000):
    """r1_partition_rate_batch for one node: -> (rate, rng behind); (0, rng0) where nothing is written"""
    sym = G.partition_symbol(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, partition)
    if sym == G.HEAD_REFUSED:
        return INVALID, None
    if sym is None:
        return 0, rng0
    return head_rate(cdf, _mutated([sym], bo_x, bo_y), rng0)


def partition_event(cdf, nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, partition):
    """the walker's partition symbol as the commit replays it: the row adapts unless an edge arm wrote it"""
    sym = G.partition_symbol(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, partition)
    assert sym != G.HEAD_REFUSED
    if sym is not None:
        head_commit(cdf, _mutated([sym], bo_x, bo_y))


def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_ref.npz"))


class Rows:
    """a table of the fixture by column name"""

    def __init__(self, G_, rows, cols):
        self.rows, self.cols = G_[rows], [str(c) for c in G_[cols]]

    def __len__(self):
        return len(self.rows)

    def __call__(self, k):
        return {c: int(v) for c, v in zip(self.cols, self.rows[k])}


def blk_of(r, seq=None):
    """(bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma, tx_mode_select) of a single row, or of an event row of `seq`"""
    s = seq if seq is not None else r
    return (r["bsize"], r["bo_x"], r["bo_y"], s["mi_cols"], s["mi_rows"], r["has_chroma"], s["tx_mode_select"])


def trial_of(r):
    return tuple(r[k] for k in ("y_mode", "uv_mode", "angle_y", "angle_uv", "alpha_u", "alpha_v", "tx_size"))

"""TEST INFRASTRUCTURE: tests/golden/coeff_nbr_ref.npz (gen_coeff_nbr_ref.py) as test cases, and the host replay of the
carried neighbour contexts -- rdo_glue.block_chain_ctx chained with rdo_glue.coeff_nbr_store / coeff_nbr_reset_left on
one pair of arrays, the block in between walked by tests/coeff_cdf_model.py.  Nothing here is imported by the product."""
import os

import numpy as np

import coeff_rate_block_model as BM
import coeff_cdf_model as DM
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import COEFF_NBR_CONTEXT, NBR_BLOCK

EXTRA_COLS = ("bo_x", "bo_y", "mi_width", "mi_height", "w_in_b", "h_in_b", "skip", "kind")


class NbrCase(DM.CdfCase):
    """one row of a sequence: a coded block, a skipped one (skip = 1) or reset_left_contexts (kind = 1)"""

    def __init__(self, G, k):
        super().__init__(G, k)
        for name, v in zip(EXTRA_COLS, G["case_rows"][k][len(DM.COLS):]):
            setattr(self, name, int(v))
        self.above, self.left = G["case_above"][k], G["case_left"][k]          # behind the row
        self.bsize = RG.block_size(self.bw, self.bh)

    def chain_ctx(self, above, left):
        """rdo_glue.block_chain_ctx on the arrays in front -> a BLOCK_CHAIN_CTX record"""
        t = RG.block_chain_ctx(above, left, self.bo_x, self.bo_y, self.bsize, self.xdec, self.ydec, self.mi_width, self.mi_height,
                               self.w_in_b, self.h_in_b, self.y_mode, 0, 0)
        return np.array([t], BM.BLOCK_DTYPE)[0]

    def desc(self, nbr=0):
        return RG.nbr_block(nbr, self.bo_x, self.bo_y, self.mi_width, self.mi_height, self.w_in_b, self.h_in_b, self.y_mode, 0, 0,
                            self.do_chroma, self.skip)


class NbrSequence:
    def __init__(self, G, s, cases):
        self.s, self.name = s, str(G["seq_names"][s])
        self.rows = [c for c in cases if c.seq == s]
        assert [c.step for c in self.rows] == list(range(int(G["seq_len"][s])))
        self.above0, self.left0 = G["seq_above"][s], G["seq_left"][s]
        self.packed = G["seq_ctx"][s]                     # [0: in front, 1: behind the last row][3930]
        self.cb = self.rows[0].cb

    def context(self, behind=False):
        return DM.context_from_packed(self.packed[int(behind)])

    def nbr_record(self):
        rec = np.zeros(1, COEFF_NBR_CONTEXT)[0]
        rec["above"], rec["left"] = self.above0, self.left0
        return rec


def load_fixture():
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_nbr_ref.npz"))
    assert tuple(str(c) for c in G["columns"]) == DM.COLS + EXTRA_COLS
    cases = [NbrCase(G, k) for k in range(len(G["case_rows"]))]
    return G, [NbrSequence(G, s, cases) for s in range(len(G["seq_len"]))]


def replay(seq, store=RG.coeff_nbr_store, check=None):
    """The sequence on one pair of arrays and one CDF context by the host statements alone.  check(row, above, left,
    block record or None, model result or None) is called behind every row.  -> (above, left, cdf context)"""
    above, left = seq.above0.copy(), seq.left0.copy()
    cdf = seq.context()
    for c in seq.rows:
        blk = res = None
        if c.kind == 1:
            RG.coeff_nbr_reset_left(left, 3)
        elif c.skip:
            assert store(above, left, c.bo_x, c.bo_y, c.bsize, c.xdec, c.ydec, c.do_chroma, True)
        else:
            blk = c.chain_ctx(above, left)
            res = DM.adapt(cdf, c.qc, c.eobs, *c.geo, c.trial, blk)
            assert store(above, left, c.bo_x, c.bo_y, c.bsize, c.xdec, c.ydec, c.do_chroma, False,
                         np.array(res["ctx"], np.uint8).reshape(3, 2, 16))
        if check:
            check(c, above, left, blk, res)
    return above, left, cdf


def descs_of(tuples):
    return np.array(tuples, NBR_BLOCK)

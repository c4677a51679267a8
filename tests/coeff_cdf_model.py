"""TEST INFRASTRUCTURE: a NumPy model of r1_coeff_cdf_slice_batch and r1_coeff_cdf_adapt_batch -- the gather of an
R1CoeffCdfs slice out of an R1CoeffCdfContext, the scatter of its adapted rows back, and a block's winner replayed
between the two.

Built on tests/coeff_rate_block_model.py (plane_grids, the record types), tests/coeff_rate_chain_model.py (the carried
writer and the CDF replay of one transform block) and rdo_glue.txb_ctx, none of them edited.  What this file states:
  * the gather rule (tests/golden/gen_coeff_rate_block_ref.py::leaves)            `slice_map`, `gather`
  * which rows a plane owns: luma txb_skip rows 0-6, plane type 0 and the tx-type table; chroma txb_skip rows 7-12 and
    plane type 1                                                                  `scatter`
  * the block: both slices cut from the context in front of the block (the rows a plane owns are touched by that plane
    alone, so cutting the chroma slice behind the luma scatter gives the same), luma walked and scattered, U and V
    walked and scattered                                                          `adapt`
`whole_tables=True` is the wrong scatter the fixture's 4:4:4 sequences are there to catch: every row of the slice goes
back, so the chroma slice's stale copy of txb_skip rows 0-6 lands on what luma just adapted.
It is pinned by tests/golden/coeff_cdf_ref.npz (tests/test_coeff_cdf_ref.py).  Nothing here is imported by the product."""
import os

import numpy as np

import coeff_rate_model as M
import coeff_rate_chain_model as CM
import coeff_rate_block_model as BM
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import COEFF_CDF_CONTEXT

INVALID = M.INVALID
CTX_U16 = COEFF_CDF_CONTEXT.itemsize // 2       # 3936: 3930 entries and the padding
# the tx-type table of a TxSet (TxSet order as M.NUM_TX_SET): get_tx_set_index -> intra_tx_{1,2} / inter_tx_{1,2,3}
TX_TABLE = {1: "inter_tx_3", 2: "intra_tx_2", 3: "intra_tx_1", 4: "inter_tx_2", 5: "inter_tx_1"}


def slice_map(ts, plane_type, is_inter, reduced):
    """[(slice field, context field, index into it, rows, n, (own_lo, own_hi))]: the slice's rows r < rows, entries
    < n are context[field][index][r][:n] (inter tx_type: the one row context[field][index])"""
    lw, lh = M.TX_W[ts].bit_length() - 3, M.TX_H[ts].bit_length() - 3
    tctx = M.txs_ctx(ts)
    ems = min(lw + lh + 4 - 4, 6)                 # area_log2 - 4
    pt = plane_type
    m = [("txb_skip", "txb_skip", (tctx,), M.TXB_SKIP_CONTEXTS, 2, (7, 13) if pt else (0, 7)),
         ("eob_flag", "eob_flag%d" % (16 << ems), (pt,), 2, 5 + ems, (0, 2)),
         ("eob_extra", "eob_extra", (tctx, pt), M.EOB_COEF_CONTEXTS, 2, (0, M.EOB_COEF_CONTEXTS)),
         ("coeff_base_eob", "coeff_base_eob", (tctx, pt), M.SIG_COEF_CONTEXTS_EOB, 3, (0, M.SIG_COEF_CONTEXTS_EOB)),
         ("coeff_base", "coeff_base", (tctx, pt), M.SIG_COEF_CONTEXTS, 4, (0, M.SIG_COEF_CONTEXTS)),
         ("coeff_br", "coeff_br", (min(tctx, 3), pt), M.LEVEL_CONTEXTS, M.BR_CDF_SIZE, (0, M.LEVEL_CONTEXTS)),
         ("dc_sign", "dc_sign", (pt,), M.DC_SIGN_CONTEXTS, 2, (0, M.DC_SIGN_CONTEXTS))]
    tset = M.tx_set(ts, is_inter, reduced)
    if pt == 0 and M.NUM_TX_SET[tset] > 1:
        sq = min(lw, lh)
        rows = 1 if is_inter else M.INTRA_MODES
        m.append(("tx_type", TX_TABLE[tset], (sq,), rows, M.NUM_TX_SET[tset], (0, rows)))
    return m


def _rows(ctx, field, index, rows):
    a = ctx[field][index]
    return a.reshape(rows, -1)          # the inter tables hold one row per sqr size


def gather(ctx, ts, plane_type, is_inter, reduced):
    """the R1CoeffCdfs slice of one COEFF_CDF_CONTEXT record; every entry the rule does not fill is 0"""
    rec = np.zeros(1, M.CDFS_DTYPE)[0]
    for f, cf, index, rows, n, _own in slice_map(ts, plane_type, is_inter, reduced):
        rec[f][:rows, :n] = _rows(ctx, cf, index, rows)
    return rec


def scatter(ctx, rec, ts, plane_type, is_inter, reduced, whole_tables=False):
    """the rows the plane owns back into the context (in place)"""
    for f, cf, index, rows, n, (lo, hi) in slice_map(ts, plane_type, is_inter, reduced):
        if whole_tables:
            lo, hi = 0, rows
        _rows(ctx, cf, index, rows)[lo:hi] = rec[f][lo:hi, :n]


def adapt(ctx, qcs, eobs, bw, bh, tx_size, xdec, ydec, is_inter, reduced, trial, block, whole_tables=False):
    """One trial of r1_coeff_cdf_adapt_batch on one COEFF_CDF_CONTEXT record, adapted IN PLACE (untouched for a
    refused trial).  qcs / eobs / trial / block as coeff_rate_block_model.coeff_rate_block; cdf_sel / cdf_sel_uv are
    ignored.  -> {"rate", "rng", "ctx" [96]}"""
    grids = BM.plane_grids(bw, bh, tx_size, xdec, ydec, is_inter)
    uv_ts = grids[1][0]
    cdfs = np.stack([gather(ctx, tx_size, 0, is_inter, reduced), gather(ctx, uv_ts, 1, is_inter, reduced)])
    blk = block.copy()
    blk["cdf_sel"], blk["cdf_sel_uv"] = 0, 1
    # the refusal conditions and the numbers: the block model on these two slices
    r = BM.coeff_rate_block(qcs, eobs, bw, bh, tx_size, xdec, ydec, is_inter, reduced, trial, blk, cdfs)
    if r["rate"] == INVALID:
        return {"rate": INVALID, "rng": 0, "ctx": [0] * 96}
    # the same walk again with the records kept: the model above adapts private copies and drops them
    mi_w, mi_h = int(block["mi_w"]), int(block["mi_h"])
    clips = [(int(block["clip_w4"]), int(block["clip_h4"]))] + [(int(block["clip_uv_w4"]), int(block["clip_uv_h4"]))] * 2
    y_mode = int(block["y_mode"])
    types = (int(trial["tx_type"]), int(trial["uv_tx_type"]), int(trial["uv_tx_type"]))
    n_planes = 3 if int(trial["do_chroma"]) else 1
    w = M.Counter()
    w.rng = int(trial["rng"])
    tell0 = w.tell_frac()
    nb = [[int(v) for v in block["ctx"][p].reshape(32)] for p in range(3)]
    for p in range(n_planes):
        ts, ntx, gw, tw4, th4, xd, yd, ax, ay, plane_bsize = grids[p]
        rec = cdfs[min(p, 1)]                         # V continues on U's record
        above, left = nb[p][:16], nb[p][16:]
        for k in CM.coded_txbs(grids[p][1:9], mi_w, mi_h):
            x4, y4 = (k % gw) * tw4, (k // gw) * th4
            sw, sh = min(tw4, clips[p][0] - x4), min(th4, clips[p][1] - y4)
            skip_ctx, sign_ctx = RG.txb_ctx(above[x4:x4 + max(sw, 0)], left[y4:y4 + max(sh, 0)], p, plane_bsize, ts)
            _rate, cul = CM.carried_txb(w, rec, qcs[p][k], eobs[p][k], ts, types[p], p, is_inter, reduced, skip_ctx, sign_ctx,
                                        y_mode)
            above[x4:x4 + tw4] = [cul] * tw4
            left[y4:y4 + th4] = [cul] * th4
        nb[p] = above + left
        if p != 1:
            scatter(ctx, rec, ts, int(p != 0), is_inter, reduced, whole_tables)
    out = {"rate": w.tell_frac() - tell0, "rng": w.rng, "ctx": nb[0] + nb[1] + nb[2]}
    assert (out["rate"], out["rng"], out["ctx"]) == (r["rate"], r["rng"], r["ctx"])
    return out


# ---- tests/golden/coeff_cdf_ref.npz (gen_coeff_cdf_ref.py) as test cases
COLS = ("seq", "step", "bw", "bh", "ts", "xdec", "ydec", "tt", "uv_tt", "inter", "red", "cb", "y_mode", "uv_mode", "do_chroma",
        "uv_ts", "bw_uv", "bh_uv", "mi_w", "mi_h", "clip_w4", "clip_h4", "clip_uv_w4", "clip_uv_h4", "rng0", "rate", "rng_out",
        "qc_off_y", "qc_off_u", "qc_off_v")


def context_from_packed(packed):
    """the fixture's packed context (3930 uint16, R1CoeffCdfContext's field order) -> one COEFF_CDF_CONTEXT record"""
    rec = np.zeros(1, COEFF_CDF_CONTEXT)
    rec.view("<u2")[:len(packed)] = packed
    return rec[0]


def packed_of(rec):
    return np.array(rec, COEFF_CDF_CONTEXT).reshape(1).view("<u2")[:CTX_U16 - 6].copy()


class CdfCase:
    """one block of a sequence"""

    def __init__(self, G, k):
        for name, v in zip(COLS, G["case_rows"][k]):
            setattr(self, name, int(v))
        self.k = k
        self.name = str(G["case_names"][k])
        gw, gh = CM.grid(self.bw, self.bh, self.ts)
        self.ntx = (gw * gh, self.bw_uv * self.bh_uv, self.bw_uv * self.bh_uv)
        self.area = (int(np.prod(M.coded_dims(self.ts))),) + (int(np.prod(M.coded_dims(self.uv_ts))),) * 2
        offs = (self.qc_off_y, self.qc_off_u, self.qc_off_v)
        self.qc = [G["case_qc"][offs[p]:offs[p] + self.ntx[p] * self.area[p]].reshape(self.ntx[p], self.area[p]) for p in range(3)]
        self.eobs = [G["case_eobs"][k][p][:self.ntx[p]] for p in range(3)]
        self.ctx_in, self.ctx_out = G["case_ctx_in"][k], G["case_ctx_out"][k]
        self.block = np.zeros(1, BM.BLOCK_DTYPE)[0]
        self.block["ctx"] = self.ctx_in.reshape(3, 2, 16)
        for f in ("mi_w", "mi_h", "clip_w4", "clip_h4", "clip_uv_w4", "clip_uv_h4", "y_mode"):
            self.block[f] = getattr(self, f)
        self.trial = np.zeros(1, BM.TRIAL_DTYPE)[0]
        self.trial["rng"], self.trial["tx_type"], self.trial["uv_tx_type"] = self.rng0, self.tt, self.uv_tt
        self.trial["do_chroma"] = self.do_chroma
        self.geo = (self.bw, self.bh, self.ts, self.xdec, self.ydec, self.inter, self.red)

    def adapt(self, ctx, **kw):
        return adapt(ctx, self.qc, self.eobs, *self.geo, self.trial, self.block, **kw)


class Sequence:
    def __init__(self, G, s, cases):
        self.s, self.name = s, str(G["seq_names"][s])
        self.blocks = [c for c in cases if c.seq == s]
        assert [c.step for c in self.blocks] == list(range(int(G["seq_len"][s])))
        self.packed = G["seq_ctx"][s]                     # [step 0 .. 6][3930]: in front, behind block 0, ...
        self.cb = self.blocks[0].cb

    def context(self, step):
        """the context behind `step` blocks"""
        return context_from_packed(self.packed[step])


def load_fixture():
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_cdf_ref.npz"))
    assert tuple(str(c) for c in G["columns"]) == COLS
    cases = [CdfCase(G, k) for k in range(len(G["case_rows"]))]
    return G, [Sequence(G, s, cases) for s in range(len(G["seq_len"]))]

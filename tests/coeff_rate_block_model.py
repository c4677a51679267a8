"""TEST INFRASTRUCTURE: a Python-int model of r1_coeff_rate_block_batch -- the coefficient rate of a whole block as the
mode decision measures it (luma_chroma_mode_rdo, src/rdo.rs:855-945): write_coeffs_lv_map
(src/context/block_unit.rs:1783-1857) over the luma transform blocks, then U's, then V's, of ONE write_tx_blocks /
write_tx_tree call with luma_only = false (src/encoder.rs:2202-2240), on ONE writer that starts at a handed-over rng.

Built on tests/coeff_rate_model.py (the block body), tests/coeff_rate_chain_model.py (the carried writer and the CDF
replay) and rdo_glue.txb_ctx / chroma_tx_grid.  What this file states itself:
  * the three loops, the chroma tx_bo arithmetic and the skip test     src/encoder.rs:2276-2311, 2352-2403, 2440-2476,
                                                                        2513-2561, 1441
  * frame_clipped_txw / txh per plane from the descriptor's clips      src/encoder.rs:1561-1566
  * the two CDF records: luma's for plane 0, the chroma one for U, carried into V
  * the start state: a Counter whose rng is the trial's, bits 0
It is pinned by tests/golden/coeff_rate_block_ref.npz (tests/test_coeff_rate_block_ref.py).  Nothing here is imported
by the product."""
import os

import numpy as np

import coeff_rate_model as M
import coeff_rate_chain_model as CM
from rav1e_amd import rdo_glue as RG

INVALID = M.INVALID
BLOCK_DTYPE = np.dtype([("ctx", "u1", (3, 2, 16)), ("mi_w", "u1"), ("mi_h", "u1"), ("clip_w4", "u1"), ("clip_h4", "u1"),
                        ("clip_uv_w4", "u1"), ("clip_uv_h4", "u1"), ("y_mode", "u1"), ("cdf_sel", "u1"), ("cdf_sel_uv", "u1"),
                        ("reserved", "u1", (3,))])
TRIAL_DTYPE = np.dtype([("first_y", "<u4"), ("first_u", "<u4"), ("first_v", "<u4"), ("block", "<u4"), ("rng", "<u2"),
                        ("tx_type", "u1"), ("uv_tx_type", "u1"), ("do_chroma", "u1"), ("reserved", "u1", (3,))])


def plane_grids(bw, bh, tx_size, xdec, ydec, is_inter):
    """per plane (tx_size, ntx, gw, tw4, th4, xdec, ydec, adj_x, adj_y, plane_bsize): the luma grid and the chroma grid of
    encoder.rs:2327-2338 / 2492-2505 with the one-unit shift of a 4-wide / 4-high block (2365-2368)"""
    bsize = CM.BLOCK_DIMS[(bw, bh)]
    luma = (tx_size,) + CM.luma_grid(bw, bh, tx_size) + (bsize,)
    uv_ts, bw_uv, bh_uv = RG.chroma_tx_grid(bsize, xdec, ydec, is_inter)
    uv_ts = int(uv_ts)
    pb = CM.BLOCK_DIMS[(max(4, bw >> xdec), max(4, bh >> ydec))]          # subsampled_size
    uv = (uv_ts, bw_uv * bh_uv, max(bw_uv, 1), M.TX_W[uv_ts] >> 2, M.TX_H[uv_ts] >> 2, xdec, ydec, int(bw == 4) * xdec,
          int(bh == 4) * ydec, pb)
    return luma, uv, uv


def uv_type_ok(uv_ts, uv_tt):
    """the scans av1_scan_orders holds for a chroma size: 32-point sides know DCT_DCT and IDTX only"""
    return 0 <= uv_tt < 16 and (uv_tt in (0, 9) or max(M.TX_W[uv_ts], M.TX_H[uv_ts]) < 32)


def coeff_rate_block(qcs, eobs, bw, bh, tx_size, xdec, ydec, is_inter, reduced, trial, block, cdfs, carry_uv_cdfs=True,
                     handover_rng=True, chroma_clip=True):
    """One trial.  qcs[p] [ntx_p][coded area], eobs[p] [ntx_p] by raster index (the trial's own blocks: `first` / `step`
    are the batch's business); trial: one TRIAL_DTYPE record; block: one BLOCK_DTYPE record; cdfs: the CDFS_DTYPE array
    cdf_sel / cdf_sel_uv pick from (never written).
    -> {"rate", "plane_rate" [3], "rng", "cul" [3][16], "ctx" [96], "tell" [3][16] (tell_frac behind block k minus the
    start state's; a block that is not coded repeats the value in front of it)}.
    The three switches exist for the sensitivity tests: V starting from the chroma snapshot again, a fresh writer in
    place of the handed-over rng, the chroma span of get_txb_ctx unclipped."""
    grids = plane_grids(bw, bh, tx_size, xdec, ydec, is_inter)
    mi_w, mi_h = int(block["mi_w"]), int(block["mi_h"])
    clips = [(int(block["clip_w4"]), int(block["clip_h4"]))] + [(int(block["clip_uv_w4"]), int(block["clip_uv_h4"]))] * 2
    y_mode, sels = int(block["y_mode"]), (int(block["cdf_sel"]), int(block["cdf_sel_uv"]), int(block["cdf_sel_uv"]))
    types = (int(trial["tx_type"]), int(trial["uv_tx_type"]), int(trial["uv_tx_type"]))
    rng0 = int(trial["rng"])
    n_planes = 3 if int(trial["do_chroma"]) else 1
    bad = {"rate": INVALID, "plane_rate": [0] * 3, "rng": 0, "cul": [[0] * 16 for _ in range(3)], "ctx": [0] * 96,
           "tell": [[0] * 16 for _ in range(3)]}

    coded = [CM.coded_txbs(g[1:9], mi_w, mi_h) for g in grids]

    if rng0 < 0x8000 or y_mode >= M.INTRA_MODES or sels[0] >= len(cdfs) or mi_w > clips[0][0] or mi_h > clips[0][1]:
        return bad
    if types[0] >= 16 or not (M.tx_type_mask(tx_size, is_inter, reduced) >> types[0]) & 1:
        return bad
    if n_planes == 3 and (sels[1] >= len(cdfs) or not uv_type_ok(grids[1][0], types[1])):
        return bad
    for p in range(n_planes):
        ts, ntx, gw, tw4, th4 = grids[p][:5]
        W, H = M.coded_dims(ts)
        for k in coded[p]:
            if int(eobs[p][k]) > W * H:
                return bad
            if p and (clips[p][0] - (k % gw) * tw4 < 1 or clips[p][1] - (k // gw) * th4 < 1):
                return bad
    w = M.Counter()
    if handover_rng:
        w.rng = rng0
    tell0 = w.tell_frac()
    ctx = [[int(v) for v in block["ctx"][p].reshape(32)] for p in range(3)]
    cul, tell, plane_rate = [[0] * 16 for _ in range(3)], [[0] * 16 for _ in range(3)], [0] * 3
    rec = None
    for p in range(n_planes):
        ts, ntx, gw, tw4, th4, xd, yd, ax, ay, plane_bsize = grids[p]
        if p == 0 or p == 1 or not carry_uv_cdfs:
            rec = np.array(cdfs[sels[p]], M.CDFS_DTYPE)         # the plane type's snapshot; V continues on U's record
        above, left = ctx[p][:16], ctx[p][16:]
        t_p = w.tell_frac()
        for k in coded[p]:
            x4, y4 = (k % gw) * tw4, (k // gw) * th4
            sw, sh = min(tw4, clips[p][0] - x4), min(th4, clips[p][1] - y4)      # frame_clipped_txw >> 2 (encoder.rs:1561-1566)
            if p and not chroma_clip:
                sw, sh = tw4, th4
            skip_ctx, sign_ctx = RG.txb_ctx(above[x4:x4 + max(sw, 0)], left[y4:y4 + max(sh, 0)], p, plane_bsize, ts)
            _rate, cul[p][k] = CM.carried_txb(w, rec, qcs[p][k], eobs[p][k], ts, types[p], p, is_inter, reduced, skip_ctx,
                                              sign_ctx, y_mode)
            tell[p][k] = w.tell_frac() - tell0
            above[x4:x4 + tw4] = [cul[p][k]] * tw4
            left[y4:y4 + th4] = [cul[p][k]] * th4
        ctx[p] = above + left
        plane_rate[p] = w.tell_frac() - t_p
    # tell: carried across blocks that are not coded and across planes, as the fixture stores it
    last = 0
    for p in range(3):
        done = set(coded[p]) if p < n_planes else set()
        for k in range(16):
            if k in done:
                last = tell[p][k]
            tell[p][k] = last
    return {"rate": w.tell_frac() - tell0, "plane_rate": plane_rate, "rng": w.rng, "cul": cul, "ctx": ctx[0] + ctx[1] + ctx[2],
            "tell": tell}


def coeff_rate_block_batch(planes, steps, bw, bh, tx_size, xdec, ydec, is_inter, reduced, trials, blocks, cdfs):
    """the batch as r1_coeff_rate_block_batch reads it: planes = [(qcoeffs [n_txb, area], eobs [n_txb])] x 3 (chroma
    entries None when no array is handed over), steps = (step_y, step_uv)
    -> (rate uint32 [n], plane_rate uint32 [n, 3], rng uint16 [n], cul uint8 [n, 3, 16], ctx uint8 [n, 3, 2, 16])"""
    n = len(trials)
    grids = plane_grids(bw, bh, tx_size, xdec, ydec, is_inter)
    rate, plane_rate, rng = np.zeros(n, np.uint32), np.zeros((n, 3), np.uint32), np.zeros(n, np.uint16)
    cul, ctx = np.zeros((n, 3, 16), np.uint8), np.zeros((n, 3, 2, 16), np.uint8)
    for i, tr in enumerate(trials):
        ok = int(tr["block"]) < len(blocks)
        qcs, eobs = [None] * 3, [None] * 3
        for p in range(3 if int(tr["do_chroma"]) else 1):
            ntx, step = grids[p][1], steps[0 if p == 0 else 1]
            first = int(tr[("first_y", "first_u", "first_v")[p]])
            if ntx == 0:
                qcs[p], eobs[p] = [], []
            elif planes[p] is None or planes[p][0] is None:
                ok = False
            elif ntx and first + (ntx - 1) * step >= len(planes[p][1]):
                ok = False
            elif ok:
                at = [first + k * step for k in range(ntx)]
                qcs[p], eobs[p] = [planes[p][0][a] for a in at], [planes[p][1][a] for a in at]
        if not ok:
            rate[i] = INVALID
            continue
        r = coeff_rate_block(qcs, eobs, bw, bh, tx_size, xdec, ydec, is_inter, reduced, tr, blocks[int(tr["block"])], cdfs)
        rate[i], plane_rate[i], rng[i], cul[i] = r["rate"], r["plane_rate"], r["rng"], r["cul"]
        ctx[i] = np.array(r["ctx"], np.uint8).reshape(3, 2, 16)
    return rate, plane_rate, rng, cul, ctx


# ---- tests/golden/coeff_rate_block_ref.npz (gen_coeff_rate_block_ref.py) as test cases
COLS = ("bw", "bh", "ts", "xdec", "ydec", "tt", "uv_tt", "inter", "red", "cb", "y_mode", "uv_mode", "do_chroma", "uv_ts", "bw_uv",
        "bh_uv", "mi_w", "mi_h", "clip_w4", "clip_h4", "clip_uv_w4", "clip_uv_h4", "nhead", "rng0", "head", "rate", "rng_out",
        "qc_off_y", "qc_off_u", "qc_off_v")


class BlockCase:
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
        self.tell, self.cul = G["case_tell"][k], G["case_cul"][k]
        self.ctx_in, self.ctx_out = G["case_ctx_in"][k], G["case_ctx_out"][k]
        self.cdfs = np.ascontiguousarray(G["case_cdfs"][k]).view(M.CDFS_DTYPE).reshape(2)
        self.block = np.zeros(1, BLOCK_DTYPE)[0]
        self.block["ctx"] = self.ctx_in.reshape(3, 2, 16)
        for f in ("mi_w", "mi_h", "clip_w4", "clip_h4", "clip_uv_w4", "clip_uv_h4", "y_mode"):
            self.block[f] = getattr(self, f)
        self.block["cdf_sel"], self.block["cdf_sel_uv"] = 0, 1
        self.trial = np.zeros(1, TRIAL_DTYPE)[0]
        self.trial["rng"], self.trial["tx_type"], self.trial["uv_tx_type"] = self.rng0, self.tt, self.uv_tt
        self.trial["do_chroma"] = self.do_chroma

    def coded(self, p):
        """raster indices of plane p's transform blocks the loop codes"""
        if p and not self.do_chroma:
            return []
        g = plane_grids(self.bw, self.bh, self.ts, self.xdec, self.ydec, self.inter)[p]
        return CM.coded_txbs(g[1:9], self.mi_w, self.mi_h)

    def model(self, **kw):
        return coeff_rate_block(self.qc, self.eobs, self.bw, self.bh, self.ts, self.xdec, self.ydec, self.inter, self.red,
                                self.trial, self.block, self.cdfs, **kw)


def load_fixture():
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_rate_block_ref.npz"))
    return G, [BlockCase(G, k) for k in range(len(G["case_rows"]))]

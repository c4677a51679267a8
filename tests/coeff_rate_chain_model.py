"""TEST INFRASTRUCTURE: a Python-int model of r1_coeff_rate_chain_batch -- the coefficient rate of a block's luma
transform blocks as rdo_tx_size_type measures it (src/rdo.rs:725-802, 1744-1799): write_coeffs_lv_map
(src/context/block_unit.rs:1783-1857) once per coded transform block, in raster order, on ONE writer, ONE CDF state and
ONE pair of neighbour-context arrays.

Built on tests/coeff_rate_model.py (the block body, pinned by coeff_rate_ref.npz) and rdo_glue.txb_ctx (get_txb_ctx,
pinned there too).  What this file states itself is what carries from one transform block to the next:
  * the loop, its skip test and frame_clipped_txw / txh    src/encoder.rs:2276-2311, 2440-2476, 1561-1566
  * the writer: coeff_rate makes its writer through the module's `Counter` name, so the carried one is handed out
    there for the length of the call; its final (bits, rng) come back in coeff_rate's result
  * the CDFs: coeff_rate adapts a private copy of the record it is given; the carried record is brought up to date by
    replaying the symbol list it returns through update_cdf with each row's own length (src/ec.rs:935-955)
  * set_coeff_context over the full tw / 4, th / 4 span   src/context/block_unit.rs:333-347
It is pinned by tests/golden/coeff_rate_chain_ref.npz (tests/test_coeff_rate_chain_ref.py).  Nothing here is imported
by the product."""
import os
from unittest import mock

import numpy as np

import coeff_rate_model as M
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import BlockSize

INVALID = M.INVALID
CHAIN_DTYPE = np.dtype([("above", "u1", (16,)), ("left", "u1", (16,)), ("mi_w", "u1"), ("mi_h", "u1"), ("clip_w4", "u1"),
                        ("clip_h4", "u1"), ("y_mode", "u1"), ("cdf_sel", "u1"), ("reserved", "u1", (2,))])
BLOCK_DIMS = {b.dims: int(b) for b in BlockSize}


def grid(bw, bh, tx_size):
    tw, th = M.TX_W[tx_size], M.TX_H[tx_size]
    return bw // tw, bh // th


def row_len(field, tx_size, is_inter, reduced):
    """the length update_cdf sees for a row of R1CoeffCdfs"""
    if field == M.F_EOB_FLAG:
        return 5 + min(M.TX_W[tx_size].bit_length() + M.TX_H[tx_size].bit_length() - 6, 6)
    if field == M.F_TX_TYPE:
        return M.NUM_TX_SET[M.tx_set(tx_size, is_inter, reduced)]
    return (2, 0, 2, 3, 4, 4, 2)[field]


def luma_grid(bw, bh, tx_size):
    """the grid tuple (ntx, gw, tw4, th4, xdec, ydec, adj_x, adj_y) of a block's luma transform blocks"""
    gw, gh = grid(bw, bh, tx_size)
    return (gw * gh, gw, M.TX_W[tx_size] >> 2, M.TX_H[tx_size] >> 2, 0, 0, 0, 0)


def coded_txbs(g, mi_w, mi_h):
    """raster indices of the transform blocks of grid g = (ntx, gw, tw4, th4, xdec, ydec, adj_x, adj_y) the loop codes:
    those whose LUMA-unit origin lies inside the tile (encoder.rs:1441, 2282, 2446)"""
    ntx, gw, tw4, th4, xd, yd, ax, ay = g
    return [k for k in range(ntx) if (((k % gw) * tw4) << xd) - ax < mi_w and (((k // gw) * th4) << yd) - ay < mi_h]


def carried_txb(w, rec, qc, eob, tx_size, tx_type, plane, is_inter, reduced, skip_ctx, sign_ctx, y_mode, carry_cdfs=True):
    """write_coeffs_lv_map for one transform block on the carried writer w and the carried CDF record rec (both
    updated in place; rec stays as it is without carry_cdfs) -> (the block's rate, cul_level)"""
    with mock.patch.object(M, "Counter", lambda: w):
        r = M.coeff_rate(qc, int(eob), tx_size, tx_type, plane, is_inter, reduced, skip_ctx, sign_ctx, y_mode, rec)
    assert r[0] != INVALID and (r[2], r[3]) == (w.bits, w.rng)
    if carry_cdfs:
        for (cid, s) in r[4]:
            f, row = cid >> 6, cid & 63
            n = row_len(f, tx_size, is_inter, reduced)
            head = [int(v) for v in rec[M.FIELDS[f]][row][:n]]
            M.update_cdf(head, s)
            rec[M.FIELDS[f]][row][:n] = head
    return r[0], r[1]


def coeff_rate_chain(qcs, eobs, bw, bh, tx_size, tx_type, is_inter, reduced, chain, cdfs, carry_cdfs=True,
                     set_context=True, clipped_span=True, skip_test=True):
    """One trial.  qcs [ntx][coded area], eobs [ntx] by raster index; chain: one CHAIN_DTYPE record; cdfs: the
    CDFS_DTYPE array the record's cdf_sel picks from (never written).
    -> {"rate", "txb_rate" [ntx], "cul" [ntx], "ctx" [32], "tell" [ntx] (tell_frac behind block k minus the fresh
    writer's; a skipped block repeats the value in front of it)}.  The four switches exist for the sensitivity tests."""
    tw, th = M.TX_W[tx_size], M.TX_H[tx_size]
    gw, gh = grid(bw, bh, tx_size)
    ntx = gw * gh
    tw4, th4 = tw >> 2, th >> 2
    area = min(tw, 32) * min(th, 32)
    mi_w, mi_h, clip_w4, clip_h4 = (int(chain[f]) for f in ("mi_w", "mi_h", "clip_w4", "clip_h4"))
    y_mode, sel = int(chain["y_mode"]), int(chain["cdf_sel"])
    coded = coded_txbs(luma_grid(bw, bh, tx_size), mi_w, mi_h)
    bad ={"rate": INVALID, "txb_rate": [0] * ntx, "cul": [0] * ntx, "ctx": [0] * 32, "tell": [0] * ntx}
    if y_mode >= M.INTRA_MODES or sel >= len(cdfs) or mi_w > clip_w4 or mi_h > clip_h4:
        return bad
    if any(int(eobs[k]) > area for k in coded):
        return bad
    if not skip_test:
        coded = list(range(ntx))
    rec = np.array(cdfs[sel], M.CDFS_DTYPE)             # the carried CDF state
    above, left = [int(v) for v in chain["above"]], [int(v) for v in chain["left"]]
    w = M.Counter()
    tell0 = w.tell_frac()
    txb_rate, cul, tell = [0] * ntx, [0] * ntx, [0] * ntx
    for k in range(ntx):
        if k not in coded:
            tell[k] = w.tell_frac() - tell0
            continue
        x4, y4 = (k % gw) * tw4, (k // gw) * th4
        sw = min(tw4, clip_w4 - x4) if clipped_span else tw4          # frame_clipped_txw >> 2 (encoder.rs:1561-1566)
        sh = min(th4, clip_h4 - y4) if clipped_span else th4
        skip_ctx, sign_ctx = RG.txb_ctx(above[x4:x4 + max(sw, 0)], left[y4:y4 + max(sh, 0)], 0, BLOCK_DIMS[(bw, bh)], tx_size)
        txb_rate[k], cul[k] = carried_txb(w, rec, qcs[k], eobs[k], tx_size, tx_type, 0, is_inter, reduced, skip_ctx, sign_ctx,
                                          y_mode, carry_cdfs)
        tell[k] = w.tell_frac() - tell0
        if set_context:
            above[x4:x4 + tw4] = [cul[k]] * tw4
            left[y4:y4 + th4] = [cul[k]] * th4
    return {"rate": w.tell_frac() - tell0, "txb_rate": txb_rate, "cul": cul, "ctx": above + left, "tell": tell}


def types_of(mask):
    return [t for t in range(16) if (mask >> t) & 1]


def coeff_rate_chain_batch(qcoeffs, eobs, tx_mask, bw, bh, tx_size, order, is_inter, reduced, chains, cdfs):
    """the batch as r1_coeff_rate_chain_batch lays it out: qcoeffs [n * nt * ntx, area], eobs [n * nt * ntx] in `order`
    -> (rate uint32 [n * nt], txb_rate uint32 [n * nt, ntx], cul uint8 [n * nt, ntx], ctx uint8 [n * nt, 32])"""
    types = types_of(tx_mask)
    nt, n = len(types), len(chains)
    gw, gh = grid(bw, bh, tx_size)
    ntx = gw * gh
    rate = np.zeros(n * nt, np.uint32)
    txb, cul, ctx = np.zeros((n * nt, ntx), np.uint32), np.zeros((n * nt, ntx), np.uint8), np.zeros((n * nt, 32), np.uint8)
    for i in range(n):
        for j, t in enumerate(types):
            at = [(i * nt + j) * ntx + k if order == 0 else (i * ntx + k) * nt + j for k in range(ntx)]
            r = coeff_rate_chain([qcoeffs[a] for a in at], [eobs[a] for a in at], bw, bh, tx_size, t, is_inter, reduced,
                                 chains[i], cdfs)
            s = i * nt + j
            rate[s], txb[s], cul[s], ctx[s] = r["rate"], r["txb_rate"], r["cul"], r["ctx"]
    return rate, txb, cul, ctx


def reorder(a, n, nt, ntx, order):
    """a laid out [n][nt][ntx][..] (order 0) -> the layout of `order`"""
    a = np.asarray(a)
    v = a.reshape((n, nt, ntx) + a.shape[1:])
    if order == 1:
        v = v.transpose((0, 2, 1) + tuple(range(3, v.ndim)))
    return np.ascontiguousarray(v).reshape(a.shape)


def random_chains(rng, n, n_cdfs, bw, bh):
    """descriptors with non-zero neighbours of every sign and a frame / tile edge through some of the blocks"""
    c = np.zeros(n, CHAIN_DTYPE)
    for r in c:
        kind = int(rng.integers(0, 4))
        hi = (1, 4, 64, 64)[kind]
        r["above"] = rng.integers(0, hi, 16) | (rng.integers(0, 3, 16) << 6 if kind == 3 else 0)
        r["left"] = rng.integers(0, hi, 16) | (rng.integers(0, 3, 16) << 6 if kind >= 2 else 0)
        edge = int(rng.integers(0, 4))
        r["mi_w"] = int(rng.integers(1, bw // 4 + 1)) if edge & 1 else 255
        r["mi_h"] = int(rng.integers(1, bh // 4 + 1)) if edge & 2 else 255
        r["clip_w4"], r["clip_h4"] = r["mi_w"], r["mi_h"]
        r["y_mode"], r["cdf_sel"] = rng.integers(0, 13), rng.integers(0, n_cdfs)
    return c


# ---- tests/golden/coeff_rate_chain_ref.npz (gen_coeff_rate_chain_ref.py) as test cases
COLS = ("bw", "bh", "ts", "tt", "inter", "red", "cb", "y_mode", "mi_w", "mi_h", "clip_w4", "clip_h4", "rate", "indep", "qc_off")


class ChainCase:
    def __init__(self, G, k):
        for name, v in zip(COLS, G["case_rows"][k]):
            setattr(self, name, int(v))
        self.k = k
        self.name = str(G["case_names"][k])
        gw, gh = grid(self.bw, self.bh, self.ts)
        self.ntx = gw * gh
        W, H = M.coded_dims(self.ts)
        self.area = W * H
        self.qc = G["case_qc"][self.qc_off:self.qc_off + self.ntx * self.area].reshape(self.ntx, self.area)
        self.eobs = G["case_eobs"][k][:self.ntx]
        self.tell = G["case_tell"][k][:self.ntx]
        self.cul = G["case_cul"][k][:self.ntx]
        self.ctx_in, self.ctx_out = G["case_ctx_in"][k], G["case_ctx_out"][k]
        self.cdfs = np.ascontiguousarray(G["case_cdfs"][k]).view(M.CDFS_DTYPE)
        self.chain = np.zeros(1, CHAIN_DTYPE)[0]
        self.chain["above"], self.chain["left"] = self.ctx_in[:16], self.ctx_in[16:]
        for f in ("mi_w", "mi_h", "clip_w4", "clip_h4", "y_mode"):
            self.chain[f] = getattr(self, f)

    def coded(self):
        """raster indices of the transform blocks the loop codes"""
        return coded_txbs(luma_grid(self.bw, self.bh, self.ts), self.mi_w, self.mi_h)

    def model(self, **kw):
        return coeff_rate_chain(self.qc, self.eobs, self.bw, self.bh, self.ts, self.tt, self.inter, self.red, self.chain,
                                self.cdfs, **kw)


def load_fixture():
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_rate_chain_ref.npz"))
    return G, [ChainCase(G, k) for k in range(len(G["case_rows"]))]

#!/usr/bin/env python3
"""tests/golden/coeff_cdf_ref.npz: the coefficient CDFs of the reference's CDFContext carried from block to block --
write_coeffs_lv_map (src/context/block_unit.rs:1783-1857) EXECUTED WHOLE through tools/rustlite over SEQUENCES of 3-6
blocks on ONE ContextWriter whose `fc` is never rolled back between the blocks, so every block starts from what the
blocks in front of it left: what r1_coeff_cdf_adapt_batch has to leave in an R1CoeffCdfContext.

Modelled on gen_coeff_rate_block_ref.py (the same files, stand-ins and restatements, stated there): per block the luma
transform blocks, then U's, then V's (src/encoder.rs:2276-2311, 2352-2403, 2440-2476, 2513-2561) on a fresh
WriterBase<WriterCounter> whose rng alone is set to the block's start value (that file asserts this equals a writer
with head symbols in front).  Every block lies inside its tile and frame: the edges are that fixture's business.

Stored: the packed context (the coefficient fields of CDFContext in the order and shapes of R1CoeffCdfContext, `fields`
/ `field_shapes`) in front of every sequence and behind every block (`seq_ctx` [sequence][step 0..6][3930]; steps past a
sequence's length repeat its last), and per block the inputs (`case_rows`, columns = COLS of tests/coeff_cdf_model.py,
`case_qc`, `case_eobs`, `case_ctx_in`), the rate, the final rng and the 96 context bytes behind it (`case_ctx_out`).

The sequences are chosen for where a scatter of adapted rows can go wrong (the names say which):
  444same    4:4:4 blocks whose luma and chroma txs_ctx are equal: both halves of one txb_skip table adapt in one block
  flag       16x16 then 8x16 / 16x8 transforms: txs_ctx 2 all, eob_flag256 against eob_flag128
  br3        64x64 then 32x32 in 4:4:4: txs_ctx 4 writes coeff_br[3], which txs_ctx 3 reads
  mixed      16x16 4:2:0 with 8x8 chroma, then an 8x8 luma block, then 4x4s
  txtype     inter then intra, reduced set on and off: all five tx-type tables
  zero       all-zero eobs: only txb_skip moves
  nochroma   4x16 in 4:2:0 (an empty chroma grid), 4x4 at an even position (has_chroma false)
  counters   levels that reach coeff_br on contexts whose counters start at 15, 16, 31 and 32
every block's DC goes through the shared dc_sign; coefficients are i16 (cb 2) and i32 (cb 4) by sequence.

Run in the build container:  python tests/golden/gen_coeff_cdf_ref.py
"""
import numpy as np

import reflib as L
from reflib import R
from gen_coeff_rate_ref import FILES, CW, BC

TX_W = (4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64)
TX_H = (4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16)
CS_NAME = {(1, 1): "Cs420", (1, 0): "Cs422", (0, 0): "Cs444"}
MAX_STEPS = 6
COLS = ("seq", "step", "bw", "bh", "ts", "xdec", "ydec", "tt", "uv_tt", "inter", "red", "cb", "y_mode", "uv_mode", "do_chroma",
        "uv_ts", "bw_uv", "bh_uv", "mi_w", "mi_h", "clip_w4", "clip_h4", "clip_uv_w4", "clip_uv_h4", "rng0", "rate", "rng_out",
        "qc_off_y", "qc_off_u", "qc_off_v")
# the coefficient side of CDFContext (src/context/cdf_context.rs:23-96) in R1CoeffCdfContext's order
FIELD_NAMES = ("txb_skip_cdf", "eob_extra_cdf", "coeff_base_eob_cdf", "coeff_base_cdf", "coeff_br_cdf", "dc_sign_cdf",
               "eob_flag_cdf16", "eob_flag_cdf32", "eob_flag_cdf64", "eob_flag_cdf128", "eob_flag_cdf256", "eob_flag_cdf512",
               "eob_flag_cdf1024", "intra_tx_1_cdf", "intra_tx_2_cdf", "inter_tx_1_cdf", "inter_tx_2_cdf", "inter_tx_3_cdf")

# (bw, bh, luma tx_size, xdec, ydec, is_inter) per block; the sequence's reduced-set flag and coefficient width
B = lambda bw, bh, ts, cs=(1, 1), inter=0, zero=False, even=False: (bw, bh, ts, cs[0], cs[1], inter, zero, even)
C444, C422 = (0, 0), (1, 0)
SEQUENCES = (
    ("444same a", 0, 2, [B(8, 8, 1, C444), B(8, 8, 1, C444, 1), B(8, 8, 1, C444)]),
    ("444same b", 0, 4, [B(16, 16, 2, C444, 1), B(16, 16, 2, C444), B(8, 8, 1, C444), B(16, 16, 2, C444)]),
    ("444same c", 1, 2, [B(4, 4, 0, C444), B(4, 4, 0, C444, 1), B(4, 4, 0, C444), B(32, 32, 3, C444), B(32, 32, 3, C444, 1)]),
    ("444same d", 0, 4, [B(8, 16, 7, C444), B(16, 8, 8, C444, 1), B(8, 16, 7, C444, 1)]),
    ("flag a", 0, 2, [B(16, 16, 2), B(16, 16, 7), B(16, 16, 8), B(16, 16, 2)]),
    ("flag b", 0, 4, [B(16, 16, 2, C444, 1), B(8, 16, 7, C444, 1), B(16, 8, 8, C444), B(16, 16, 2, C444)]),
    ("flag c", 1, 2, [B(16, 8, 8, C422), B(16, 16, 2, C422), B(16, 8, 8, C422, 1)]),
    ("flag d", 0, 2, [B(32, 32, 3), B(32, 32, 9, (1, 1), 1), B(32, 32, 10), B(32, 16, 10)]),
    ("br3 a", 0, 2, [B(64, 64, 4, C444), B(32, 32, 3, C444), B(64, 64, 4, C444, 1)]),
    ("br3 b", 0, 4, [B(64, 64, 4, C444, 1), B(32, 32, 3, C444, 1), B(32, 32, 3, C444), B(64, 64, 4, C444)]),
    ("br3 c", 1, 4, [B(64, 64, 4), B(32, 32, 3), B(64, 32, 12), B(32, 32, 3, (1, 1), 1)]),
    ("mixed a", 0, 2, [B(16, 16, 2), B(8, 8, 1), B(4, 4, 0), B(4, 4, 0), B(8, 8, 1, (1, 1), 1)]),
    ("mixed b", 0, 4, [B(16, 16, 1), B(8, 8, 1, (1, 1), 1), B(8, 8, 0), B(16, 16, 2, (1, 1), 1), B(8, 4, 6), B(4, 8, 5)]),
    ("mixed c", 1, 2, [B(16, 16, 2, C422), B(8, 8, 1, C422), B(16, 16, 1, C422, 1), B(8, 8, 1, C422, 1)]),
    ("mixed d", 0, 4, [B(64, 16, 18, C444), B(16, 16, 2, C444), B(64, 64, 2, C444, 1)]),
    ("txtype a", 0, 2, [B(8, 8, 1, (1, 1), 1), B(8, 8, 1), B(16, 16, 2, (1, 1), 1), B(16, 16, 2), B(32, 32, 3, (1, 1), 1), B(8, 8, 0)]),
    ("txtype b", 1, 4, [B(8, 8, 1, (1, 1), 1), B(8, 8, 1), B(16, 16, 2, (1, 1), 1), B(16, 16, 2), B(4, 4, 0, (1, 1), 1), B(4, 4, 0)]),
    ("txtype c", 0, 4, [B(8, 8, 0, (1, 1), 1), B(8, 8, 0), B(16, 8, 8, (1, 1), 1), B(16, 8, 8), B(8, 16, 7, (1, 1), 1)]),
    ("txtype d", 1, 2, [B(16, 16, 1, C444, 1), B(16, 16, 1, C444), B(32, 32, 3, C444, 1), B(16, 4, 14, C444)]),
    ("txtype e", 0, 2, [B(8, 8, 1), B(8, 8, 1), B(8, 8, 1), B(8, 8, 1, (1, 1), 1), B(8, 8, 1, (1, 1), 1), B(8, 8, 1, (1, 1), 1)]),
    ("zero a", 0, 2, [B(16, 16, 1, (1, 1), 0, True), B(16, 16, 1, (1, 1), 1, True), B(8, 8, 1, (1, 1), 0, True), B(16, 16, 1)]),
    ("zero b", 1, 4, [B(8, 8, 1, C444, 0, True), B(8, 8, 1, C444, 1, True), B(8, 8, 1, C444), B(8, 8, 1, C444, 0, True)]),
    ("zero c", 0, 4, [B(64, 64, 4, C444, 0, True), B(32, 32, 3, C444, 0, True), B(64, 64, 2, (1, 1), 1, True)]),
    ("nochroma a", 0, 2, [B(4, 16, 13), B(4, 16, 13, (1, 1), 1), B(4, 4, 0, (1, 1), 0, False, True), B(4, 4, 0), B(16, 4, 14)]),
    ("nochroma b", 1, 4, [B(4, 4, 0, (1, 1), 1, False, True), B(4, 16, 13), B(8, 8, 1), B(4, 4, 0, (1, 1), 0, False, True)]),
    ("nochroma c", 0, 4, [B(4, 8, 5, (1, 1), 0, False, True), B(8, 4, 6, (1, 1), 1, False, True), B(4, 8, 5), B(16, 4, 14, (1, 1), 1)]),
    ("counters a", 0, 2, [B(8, 8, 1), B(8, 8, 1, (1, 1), 1), B(8, 8, 1), B(8, 8, 1, (1, 1), 1)]),
    ("counters b", 0, 4, [B(16, 16, 2, C444), B(16, 16, 2, C444, 1), B(16, 16, 2, C444)]),
    ("counters c", 1, 2, [B(4, 4, 0, C444), B(4, 4, 0, C444), B(4, 4, 0, C444, 1), B(4, 4, 0, C444), B(4, 4, 0, C444, 1), B(4, 4, 0, C444)]),
    ("counters d", 0, 4, [B(32, 32, 3), B(32, 32, 3, (1, 1), 1), B(16, 16, 2), B(32, 32, 3)]),
    ("counters e", 0, 2, [B(64, 64, 4, C444), B(64, 64, 4, C444, 1), B(32, 32, 3, C444)]),
    ("long a", 0, 2, [B(16, 16, 0), B(16, 16, 0, (1, 1), 1), B(16, 16, 0, C444)]),
    ("long b", 1, 4, [B(32, 32, 1, C444, 1), B(16, 16, 2, C444), B(32, 16, 10, C444)]),
    ("long c", 0, 2, [B(16, 64, 17), B(64, 16, 18, (1, 1), 1), B(16, 16, 2)]),
    ("long d", 0, 4, [B(8, 32, 15, C444), B(32, 8, 16, C444, 1), B(8, 8, 1, C444), B(32, 8, 16, C422)]),
    ("long e", 1, 2, [B(32, 64, 11), B(64, 32, 12, C444), B(32, 32, 3, C444, 1), B(16, 32, 9, C444)]),
    ("rect a", 0, 2, [B(8, 16, 7), B(16, 8, 8, C444), B(8, 16, 5, C444, 1), B(16, 8, 6)]),
    ("rect b", 0, 4, [B(16, 32, 9, C444), B(32, 16, 10, C422), B(16, 32, 2), B(32, 16, 2, C422, 1)]),
    ("rect c", 1, 4, [B(4, 8, 5, C444), B(8, 4, 6, C444, 1), B(4, 16, 13, C444), B(16, 4, 14, C444, 1), B(8, 8, 1, C444)]),
    ("rect d", 0, 2, [B(16, 16, 8), B(16, 16, 7, C444, 1), B(16, 16, 14, C444), B(16, 16, 13, (1, 1), 1)]),
)


def nest(x):
    return [nest(x[i]) for i in range(len(x))] if hasattr(x, "__len__") else int(x)


def main():
    c = L.crate(*FILES)
    L.load_v_frame_types(c)
    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants][:19]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    bs_names = [v[0] for v in c.enums["BlockSize"].variants]
    BlockSize = {n: L.enum(c, "BlockSize", n) for n in bs_names}
    PM = [L.enum(c, "PredictionMode", v[0]) for v in c.enums["PredictionMode"].variants]
    pm_names = [v[0] for v in c.enums["PredictionMode"].variants]
    assert pm_names[13] == "UV_CFL_PRED" and pm_names[14] == "NEARESTMV"
    NEARESTMV = PM[14]
    CS = {k: L.enum(c, "ChromaSampling", v) for k, v in CS_NAME.items()}
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    new_counter = c.get("new", owner="WriterCounter")
    new_fc = c.get("new", owner="CDFContext")
    wclm = c.get("write_coeffs_lv_map", owner="ContextWriter")
    get_set = c.get("get_tx_set")
    has_chroma = c.get("has_chroma")
    uv_intra = c.get("uv_intra_mode_to_tx_type_context")
    max_rect = c.const_value("max_txsize_rect_lookup")
    tx_used = np.array(c.const_value("av1_tx_used").tolist(), np.int32)
    orders = c.const_value("av1_scan_orders")
    for ts in range(19):
        assert (int(c.call_method(TxSize[ts], "width", [])), int(c.call_method(TxSize[ts], "height", []))) == (TX_W[ts], TX_H[ts])
    mi = lambda obj, name: int(c.call_method(obj, name, []))
    rng = np.random.default_rng(20261021)

    def chroma_of(bname, xdec, ydec, inter):
        """(plane_bsize name, uv_tx_size, bw_uv, bh_uv): subsampled_size / largest_chroma_tx_size executed, the grid
        arithmetic of encoder.rs:2327-2338 / 2492-2505"""
        plane_bsize = c.call_method(c.call_method(BlockSize[bname], "subsampled_size", [xdec, ydec]), "unwrap", [])
        uv_ts = int(c.call_method(BlockSize[bname], "largest_chroma_tx_size", [xdec, ydec]).disc)
        if inter:
            mt = max_rect[bs_names.index(bname)]
            w_mi, h_mi = mi(mt, "width_mi"), mi(mt, "height_mi")
        else:
            w_mi, h_mi = mi(BlockSize[bname], "width_mi"), mi(BlockSize[bname], "height_mi")
        bw_uv, bh_uv = w_mi >> xdec, h_mi >> ydec
        if bw_uv == 0 or bh_uv == 0:
            bw_uv = 1
            bh_uv = 1
        bw_uv //= mi(TxSize[uv_ts], "width_mi")
        bh_uv //= mi(TxSize[uv_ts], "height_mi")
        return bs_names[int(plane_bsize.disc)], uv_ts, bw_uv, bh_uv

    def pack(fc):
        return np.concatenate([np.array(nest(getattr(fc, f)), np.int64).reshape(-1) for f in FIELD_NAMES]).astype(np.uint16)

    def seed_counters(fc):
        """every coefficient CDF's counter at one of update_cdf's rate steps (and around them)"""
        def walk(x):
            if hasattr(x[0], "__len__"):
                for i in range(len(x)):
                    walk(x[i])
            else:
                x[len(x) - 1] = (15, 16, 31, 32, 14, 30, 0, int(rng.integers(0, 33)))[int(rng.integers(0, 8))]
        for f in FIELD_NAMES:
            walk(getattr(fc, f))

    def fill(area, scan, eob, pool, big, dc_sign):
        q = np.zeros(area, np.int64)
        if eob == 0:
            return q
        mags = rng.choice(pool, eob)
        if mags[-1] == 0:
            mags[-1] = int(rng.choice([1, 2, 3, 15, big]))
        vals = mags * rng.choice([-1, 1], eob)
        if eob > 1:
            vals[0] = abs(int(vals[0]) or 1) * dc_sign
        q[np.array(scan[:eob], np.int64)] = vals
        return q

    def neighbours(kinds):
        ab, lf = [], []
        for kind in kinds:
            if kind == 0:
                ab.append([0] * 64)
                lf.append([0] * 16)
                continue
            hi = (0, 4, 64)[kind]
            a = rng.integers(0, hi, 64) | (rng.integers(0, 3, 64) << 6)
            l = rng.integers(0, hi, 16) | (rng.integers(0, 3, 16) << 6)
            a[rng.integers(0, 64, 20)] = 0
            l[rng.integers(0, 16, 5)] = 0
            ab.append([int(v) for v in a])
            lf.append([int(v) for v in l])
        return ab, lf

    rows, names, qc_all = [], [], []
    acc = {k: [] for k in ("eobs", "ctx_in", "ctx_out")}
    seq_ctx, seq_len, seq_names = [], [], []
    bi = 0
    for si, (sname, red, cb, blocks) in enumerate(SEQUENCES):
        assert 3 <= len(blocks) <= MAX_STEPS
        fc = new_fc({}, (10, 40, 100, 200)[si % 4])
        if sname.startswith("counters") or si % 3 == 2:
            seed_counters(fc)
        ctxs = [pack(fc)]
        big = 32767 if cb == 2 else (1 << 20) - 1
        for step, (bw, bh, ts, xdec, ydec, inter, zero, even) in enumerate(blocks):
            bname = "BLOCK_%dX%d" % (bw, bh)
            bsize = BlockSize[bname]
            tw, th = TX_W[ts], TX_H[ts]
            gw, gh = bw // tw, bh // th
            area = min(tw, 32) * min(th, 32)
            pname, uv_ts, bw_uv, bh_uv = chroma_of(bname, xdec, ydec, inter)
            n_uv = bw_uv * bh_uv
            uv_area = min(TX_W[uv_ts], 32) * min(TX_H[uv_ts], 32)
            utw_mi, uth_mi = TX_W[uv_ts] >> 2, TX_H[uv_ts] >> 2
            w_mi, h_mi = bw >> 2, bh >> 2
            # the block's place: sub-8x8 blocks at the odd offsets that carry the chroma, or (`even`) at those that do not
            bo_x = (bw >> 2) * ((bi % 3) + 1)
            bo_y = ((bh >> 2) * (bi % 4)) % 16
            if bw == 4 and xdec:
                bo_x = (bo_x & ~1) + (0 if even else 1)
            if bh == 4 and ydec:
                bo_y = (bo_y & ~1) + (0 if even else 1)
            do_chroma = bool(has_chroma({}, TBO(BO(x=bo_x, y=bo_y)), bsize, xdec, ydec, CS[(xdec, ydec)]))
            assert do_chroma == (not even), (sname, step)
            sd = int(get_set({}, TxSize[ts], bool(inter), bool(red)).disc)
            allowed = [t for t in ((9, 10, 11, 0, 1, 3, 12, 5) if inter else (0, 1, 3, 10, 11, 9, 2)) if tx_used[sd][t]]
            tt = allowed[(bi + step) % len(allowed)]
            y_mode, uv_mode = bi % 13, (bi * 3 + step) % 14
            style = (bi + step) % 5
            if sname.startswith("counters"):
                style = (2, 4)[step % 2]                     # levels that reach coeff_br, and beyond it
            pool = {0: [0, 0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 14, 15], 2: [1, 2, 3, 14, 15, 127, 128, big], 3: [0, 0, 0, 1],
                    4: [0, 1, 2, 3, 4, 7, 15, 16, 17, 127, 128, 300, big // 7, big]}[style]
            scan = [int(v) for v in orders[ts][tt].scan]
            eobs_y, qcs_y = np.zeros(gw * gh, np.int64), np.zeros((gw * gh, area), np.int64)
            for k in range(gw * gh):
                if zero or (style == 3 and k == 1):
                    continue
                long_eob = sname.startswith("long") and k == 0
                eob = area if (long_eob and area <= 256) or (rng.integers(0, 6) == 0 and area <= 64) else \
                    int(rng.integers(1, min(area, 300 if long_eob else 40) + 1))
                eobs_y[k] = eob
                qcs_y[k] = fill(area, scan, eob, pool, big, (-1, 0, 1)[(bi + k) % 3])
            if inter:
                uv_tt = int(c.call_method(TxType[tt], "uv_inter", [TxSize[uv_ts]]).disc) if eobs_y.any() else 0
            else:
                uv_tt = 0 if TX_W[uv_ts] >= 32 or TX_H[uv_ts] >= 32 else int(uv_intra({}, PM[uv_mode]).disc)
            uv_scan = [int(v) for v in orders[uv_ts][uv_tt].scan]
            qs_uv, es_uv = [], []
            for p in (1, 2):
                q, e = np.zeros((n_uv, uv_area), np.int64), np.zeros(n_uv, np.int64)
                for k in range(n_uv):
                    if zero or (bi + p + k) % 7 == 0:
                        continue
                    e[k] = uv_area if rng.integers(0, 5) == 0 and uv_area <= 64 else int(rng.integers(1, min(uv_area, 30) + 1))
                    q[k] = fill(uv_area, uv_scan, int(e[k]), pool, big, (-1, 0, 1)[(bi + k + p) % 3])     # a coded chroma DC
                qs_uv.append(q)
                es_uv.append(e)
            qcs, eobs = [qcs_y, qs_uv[0], qs_uv[1]], [eobs_y, es_uv[0], es_uv[1]]
            above0, left0 = neighbours([(bi + step + p) % 3 for p in range(3)])
            rng0 = 0x8000 if (bi + step) % 2 == 0 else int(rng.integers(0x8000, 0x10000))

            # ---- the block on the sequence's ContextWriter: a new BlockContext and counter, the SAME fc
            bc = BC(above_coeff_context=R.RSlice([R.RSlice(list(above0[p])) for p in range(3)]),
                    left_coeff_context=R.RSlice([R.RSlice(list(left0[p])) for p in range(3)]))
            cw, w = CW(bc=bc, fc=fc), new_counter({})
            w.rng = rng0
            g = {"T": "i16" if cb == 2 else "i32", "W": "WriterBase"}
            tell0 = int(c.call_method(w, "tell_frac", []))
            for by in range(gh):                                          # luma: encoder.rs:2276-2311, 2440-2476
                for bx in range(gw):
                    k = by * gw + bx
                    tbx, tby = bo_x + bx * (tw >> 2), bo_y + by * (th >> 2)
                    ret = wclm(g, cw, w, 0, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[0][k]]), int(eobs[0][k]),
                               NEARESTMV if inter else PM[y_mode], TxSize[ts], TxType[tt], bsize, 0, 0, bool(red), tw, th)
                    assert ret is (int(eobs[0][k]) != 0)
            if do_chroma:                                                 # chroma: encoder.rs:2352-2403, 2513-2561
                for p in (1, 2):
                    for by in range(bh_uv):
                        for bx in range(bw_uv):
                            k = by * bw_uv + bx
                            tbx = bo_x + ((bx * utw_mi) << xdec) - int(w_mi == 1) * xdec
                            tby = bo_y + ((by * uth_mi) << ydec) - int(h_mi == 1) * ydec
                            ret = wclm(g, cw, w, p, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[p][k]]), int(eobs[p][k]),
                                       NEARESTMV if inter else PM[uv_mode], TxSize[uv_ts], TxType[uv_tt], BlockSize[pname], xdec,
                                       ydec, bool(red), TX_W[uv_ts], TX_H[uv_ts])
                            assert ret is (int(eobs[p][k]) != 0)
            rate, rng_out = int(c.call_method(w, "tell_frac", [])) - tell0, int(w.rng)
            ctxs.append(pack(fc))

            ux, uy = bo_x - int(w_mi == 1) * xdec, bo_y - int(h_mi == 1) * ydec
            origin = [(bo_x, bo_y % 16), (ux >> xdec, (uy % 16) >> ydec), (ux >> xdec, (uy % 16) >> ydec)]

            def window(ab, lf):
                out = []
                for p in range(3):
                    x0, y0 = origin[p]
                    out += ([int(v) for v in list(ab[p])[x0:x0 + 16]] + [0] * 16)[:16]
                    out += ([int(v) for v in list(lf[p])[y0:y0 + 16]] + [0] * 16)[:16]
                return out

            offs = []
            for p in range(3):
                offs.append(len(qc_all))
                for q in qcs[p]:
                    qc_all.extend(int(v) for v in q)
            rows.append((si, step, bw, bh, ts, xdec, ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, int(do_chroma), uv_ts, bw_uv,
                         bh_uv, 255, 255, 255, 255, 255, 255, rng0, rate, rng_out, offs[0], offs[1], offs[2]))
            names.append("%s/%d %dx%d/%dx%d %d%d i%d t%d" % (sname, step, bw, bh, tw, th, xdec, ydec, inter, tt))
            e = np.zeros((3, 16), np.uint16)
            for p in range(3):
                e[p, :len(eobs[p])] = eobs[p]
            acc["eobs"].append(e)
            acc["ctx_in"].append(np.array(window(above0, left0), np.uint8))
            acc["ctx_out"].append(np.array(window(bc.above_coeff_context, bc.left_coeff_context), np.uint8))
            print(len(rows), names[-1], "uv_tt", uv_tt, "chroma", int(do_chroma), "eobs", [[int(v) for v in e_] for e_ in eobs],
                  hex(rng0), "rate", rate, "moved", int((ctxs[-1] != ctxs[-2]).sum()), flush=True)
            bi += 1
        seq_len.append(len(blocks))
        seq_names.append(sname)
        seq_ctx.append(np.stack(ctxs + [ctxs[-1]] * (MAX_STEPS + 1 - len(ctxs))))

    shapes = np.zeros((len(FIELD_NAMES), 4), np.int32)
    fc = new_fc({}, 40)
    for i, f in enumerate(FIELD_NAMES):
        s = np.array(nest(getattr(fc, f))).shape
        shapes[i, :len(s)] = s
    out = {"columns": np.array(COLS), "case_rows": np.array(rows, np.int64), "case_names": np.array(names),
           "case_qc": np.array(qc_all, np.int32), "case_eobs": np.stack(acc["eobs"]), "case_ctx_in": np.stack(acc["ctx_in"]),
           "case_ctx_out": np.stack(acc["ctx_out"]), "seq_ctx": np.stack(seq_ctx), "seq_len": np.array(seq_len, np.int32),
           "seq_names": np.array(seq_names), "fields": np.array(FIELD_NAMES), "field_shapes": shapes}
    print("sequences:", len(seq_len), "blocks:", len(rows), flush=True)
    L.save("coeff_cdf_ref.npz", out)


if __name__ == "__main__":
    main()

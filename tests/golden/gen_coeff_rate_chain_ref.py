#!/usr/bin/env python3
"""tests/golden/coeff_rate_chain_ref.npz: the coefficient rate of a block coded as SEVERAL luma transform blocks, as
rdo_tx_size_type measures it per transform depth (src/rdo.rs:725-802 around write_tx_blocks / write_tx_tree with
luma_only = true, src/rdo.rs:1744-1799), computed by the REFERENCE'S OWN SOURCE TEXT through tools/rustlite.

Executed whole, once per coded transform block, on ONE ContextWriter / BlockContext / WriterBase<WriterCounter>:
  write_coeffs_lv_map with get_txb_ctx and set_coeff_context inside it     src/context/block_unit.rs:1783-1857
  and everything gen_coeff_rate_ref.py lists below it (same files, same stand-ins: symbol_with_update! without the
  rollback log, ContextWriter / BlockContext as plain objects, cdf() .. cdf_5d() by declared type).
STATED HERE, as gen_rdo_intra_split_ref.py states it (the functions themselves want the pixel pipeline in front):
  the loop over the transform-block grid in raster order with the tile-grid test
                                                 src/encoder.rs:2276-2311 (write_tx_blocks), 2440-2476 (write_tx_tree)
  frame_clipped_txw / frame_clipped_txh          src/encoder.rs:1561-1566 (xdec = ydec = 0)
The rate is tell_frac behind the last block minus tell_frac of the fresh counter (src/rdo.rs:1744-1799 with the block
in place of one transform block).

The block lies at (bo_x, bo_y) of a tile at the frame's origin whose grid (mi_width, mi_height) and whose frame
(w_in_b, h_in_b) are chosen per case; above_coeff_context[0] holds 64 entries, left_coeff_context[0] 16.

Per case: the geometry and switches (`case_rows`, columns = COLS of tests/coeff_rate_chain_model.py), `case_geom`
(bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b), the coefficients and eobs by raster index (a block the loop skips
keeps zeros), the whole context arrays in front (`case_above`, `case_left`) and the 32 bytes the block covers in front
and behind (`case_ctx_in`, `case_ctx_out`), tell_frac behind every block minus the fresh counter's (`case_tell`; a
skipped block repeats the value in front of it), cul_level per block (read back from above_coeff_context), the
R1CoeffCdfs slice in front, the total rate, and `indep`: the sum of the rates of the same blocks each written alone
from the same start (fresh counter, unadapted CDFs, the contexts in front) -- what a caller without the chain would
have summed.
Real content: cases of rdo_intra_split_ref.npz (write_tx_blocks) and the write_tx_tree cases of rdo_txsearch_ref.npz,
with the coefficients and eobs recorded there, on CDFContext::new(q) of the case's quantizer class.

Run in the build container:  python tests/golden/gen_coeff_rate_chain_ref.py
"""
import copy
import os

import numpy as np

import reflib as L
from reflib import R
from gen_coeff_rate_ref import FILES, FIELDS, Obj, CW, BC

TX_W = (4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64)
TX_H = (4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16)
# (bw, bh, tx_size): 2x2; ntx 16 at span 1 and span 4; one row, one column; rectangular transforms (coded 16x32);
# four chunks; ntx 1
SHAPES = ((8, 8, 0), (16, 16, 0), (64, 64, 2), (16, 4, 0), (4, 16, 0), (32, 8, 8), (16, 64, 9), (64, 64, 3), (64, 64, 4),
          (8, 8, 1))
ROUNDS = 5


def main():
    c = L.crate(*FILES)
    K = lambda name: int(c.const_value(name))
    dims = {n: K(n) for n in ("TXB_SKIP_CONTEXTS", "EOB_COEF_CONTEXTS", "SIG_COEF_CONTEXTS_EOB", "SIG_COEF_CONTEXTS",
                              "LEVEL_CONTEXTS", "BR_CDF_SIZE", "DC_SIGN_CONTEXTS", "INTRA_MODES")}
    shapes = (("txb_skip", dims["TXB_SKIP_CONTEXTS"], 2), ("eob_flag", 2, 11), ("eob_extra", dims["EOB_COEF_CONTEXTS"], 2),
              ("coeff_base_eob", dims["SIG_COEF_CONTEXTS_EOB"], 3), ("coeff_base", dims["SIG_COEF_CONTEXTS"], 4),
              ("coeff_br", dims["LEVEL_CONTEXTS"], dims["BR_CDF_SIZE"]), ("dc_sign", dims["DC_SIGN_CONTEXTS"], 2),
              ("tx_type", dims["INTRA_MODES"], 16))
    assert tuple(s[0] for s in shapes) == FIELDS
    rec_len = sum(r * n for _, r, n in shapes)
    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants][:19]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    BlockSize = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
    PM = [L.enum(c, "PredictionMode", v[0]) for v in c.enums["PredictionMode"].variants]
    pm_names = [v[0] for v in c.enums["PredictionMode"].variants]
    NEARESTMV = PM[pm_names.index("NEARESTMV")]
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    new_counter = c.get("new", owner="WriterCounter")
    new_fc = c.get("new", owner="CDFContext")
    wclm = c.get("write_coeffs_lv_map", owner="ContextWriter")
    txs_ctx_fn = c.get("get_txsize_entropy_ctx", owner="ContextWriter")
    set_index = c.get("get_tx_set_index")
    get_set = c.get("get_tx_set")
    num_tx_set = [int(v) for v in c.const_value("num_tx_set")]
    tx_used = np.array(c.const_value("av1_tx_used").tolist(), np.int32)
    orders = c.const_value("av1_scan_orders")
    for ts in range(19):
        assert (int(c.call_method(TxSize[ts], "width", [])), int(c.call_method(TxSize[ts], "height", []))) == (TX_W[ts], TX_H[ts])

    def leaves(fc, ts, is_inter, reduced):
        """the luma R1CoeffCdfs slice of a CDFContext (include/rav1e_amd.h), as gen_coeff_rate_ref.py gathers it"""
        tctx = int(txs_ctx_fn({}, TxSize[ts]))
        ems = min(int(c.call_method(TxSize[ts], "area_log2", [])) - 4, 6)
        sq = int(c.call_method(TxSize[ts], "sqr", []).disc)
        res = [(0, r, 2, fc.txb_skip_cdf[tctx][r]) for r in range(dims["TXB_SKIP_CONTEXTS"])]
        flag = getattr(fc, "eob_flag_cdf%d" % (16 << ems))[0]
        res += [(1, r, 5 + ems, flag[r]) for r in range(2)]
        res += [(2, r, 2, fc.eob_extra_cdf[tctx][0][r]) for r in range(dims["EOB_COEF_CONTEXTS"])]
        res += [(3, r, 3, fc.coeff_base_eob_cdf[tctx][0][r]) for r in range(dims["SIG_COEF_CONTEXTS_EOB"])]
        res += [(4, r, 4, fc.coeff_base_cdf[tctx][0][r]) for r in range(dims["SIG_COEF_CONTEXTS"])]
        res += [(5, r, dims["BR_CDF_SIZE"], fc.coeff_br_cdf[min(tctx, 3)][0][r]) for r in range(dims["LEVEL_CONTEXTS"])]
        res += [(6, r, 2, fc.dc_sign_cdf[0][r]) for r in range(dims["DC_SIGN_CONTEXTS"])]
        nset = num_tx_set[int(get_set({}, TxSize[ts], bool(is_inter), bool(reduced)).disc)]
        if nset > 1:
            idx = int(set_index({}, TxSize[ts], bool(is_inter), bool(reduced)))
            if is_inter:
                res.append((7, 0, nset, getattr(fc, "inter_tx_%d_cdf" % idx)[sq]))
            else:
                tab = getattr(fc, "intra_tx_%d_cdf" % idx)[sq]
                res += [(7, r, nset, tab[r]) for r in range(dims["INTRA_MODES"])]
        return res

    base = [0]
    for _, r, n in shapes:
        base.append(base[-1] + r * n)

    def gather(lv):
        rec = np.zeros(rec_len, np.uint16)
        for (f, r, n, a) in lv:
            o = base[f] + r * shapes[f][2]
            rec[o:o + n] = [int(v) for v in a]
        return rec

    rng = np.random.default_rng(20261019)

    def seed_random(lv):
        """valid CDFs with counters on either side of update_cdf's rate steps (15 / 16, 31 / 32)"""
        for (f, r, n, a) in lv:
            v = np.sort(rng.choice(np.arange(64, 32704), n - 1, replace=False))[::-1]
            for i in range(n - 1):
                a[i] = int(v[i])
            a[n - 1] = (15, 16, 31, 32, 14, 30, 0, int(rng.integers(0, 33)))[int(rng.integers(0, 8))]

    fcs = {q: new_fc({}, q) for q in (10, 40, 100, 200)}

    def run_case(bw, bh, ts, tt, inter, red, cb, y_mode, geom, above0, left0, qcs, eobs, fc0):
        """the loop of write_tx_blocks / write_tx_tree over the luma transform blocks (encoder.rs:2276-2311, 2440-2476)
        around write_coeffs_lv_map with frame_clipped_* of encoder.rs:1561-1566; then every coded block alone"""
        bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b = geom
        tw, th = TX_W[ts], TX_H[ts]
        gw, gh = bw // tw, bh // th
        bsize = BlockSize["BLOCK_%dX%d" % (bw, bh)]
        pred = NEARESTMV if inter else PM[y_mode]
        g = {"T": "i16" if cb == 2 else "i32", "W": "WriterBase"}

        def state():
            bc = BC(above_coeff_context=R.RSlice([R.RSlice(list(above0)) for _ in range(3)]),
                    left_coeff_context=R.RSlice([R.RSlice(list(left0)) for _ in range(3)]))
            return bc, CW(bc=bc, fc=copy.deepcopy(fc0)), new_counter({})

        def write(cw, w, bx, by):
            tbx, tby = bo_x + bx * (tw >> 2), bo_y + by * (th >> 2)
            clipped_w = min((w_in_b - tbx) << 2, tw)            # the tile lies at the frame's origin: frame_bo = tx_bo
            clipped_h = min((h_in_b - tby) << 2, th)
            k = by * gw + bx
            ret = wclm(g, cw, w, 0, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[k]]), int(eobs[k]), pred, TxSize[ts],
                       TxType[tt], bsize, 0, 0, bool(red), clipped_w, clipped_h)
            assert ret is (int(eobs[k]) != 0)
            return tbx

        bc, cw, w = state()
        tell0 = int(c.call_method(w, "tell_frac", []))
        tell, cul, coded = [], [], []
        for by in range(gh):
            for bx in range(gw):
                if bo_x + bx * (tw >> 2) >= mi_width or bo_y + by * (th >> 2) >= mi_height:
                    tell.append(tell[-1] if tell else 0)
                    cul.append(0)
                    continue
                tbx = write(cw, w, bx, by)
                tell.append(int(c.call_method(w, "tell_frac", [])) - tell0)
                cul.append(int(bc.above_coeff_context[0][tbx]))
                coded.append((bx, by))
        ctx_out = [int(v) for v in list(bc.above_coeff_context[0])[bo_x:bo_x + 16]] + \
                  ([int(v) for v in list(bc.left_coeff_context[0])[bo_y:]] + [0] * 16)[:16]
        assert all(list(bc.above_coeff_context[p]) == list(above0) for p in (1, 2))
        indep = 0
        for (bx, by) in coded:
            _, cw1, w1 = state()
            t1 = int(c.call_method(w1, "tell_frac", []))
            write(cw1, w1, bx, by)
            indep += int(c.call_method(w1, "tell_frac", [])) - t1
        return (tell[-1] if coded else 0), tell, cul, ctx_out, indep, len(coded)

    rows, names, geoms, qc_all = [], [], [], []
    eobs_all, tell_all, cul_all, ctx_in_all, ctx_out_all, above_all, left_all, cdf_all = [], [], [], [], [], [], [], []

    def add(name, bw, bh, ts, tt, inter, red, cb, y_mode, geom, above0, left0, qcs, eobs, fc0):
        rate, tell, cul, ctx_out, indep, ncoded = run_case(bw, bh, ts, tt, inter, red, cb, y_mode, geom, above0, left0, qcs,
                                                           eobs, fc0)
        bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b = geom
        pad = lambda v, dt: np.array(list(v) + [0] * (16 - len(v)), dt)
        rows.append((bw, bh, ts, tt, inter, red, cb, y_mode, min(255, mi_width - bo_x), min(255, mi_height - bo_y),
                     min(255, w_in_b - bo_x), min(255, h_in_b - bo_y), rate, indep, len(qc_all)))
        names.append(name)
        geoms.append(geom)
        for q in qcs:
            qc_all.extend(int(v) for v in q)
        eobs_all.append(pad([int(e) for e in eobs], np.uint16))
        tell_all.append(pad(tell, np.uint32))
        cul_all.append(pad(cul, np.uint8))
        ctx_in_all.append(np.array(list(above0[bo_x:bo_x + 16]) + (list(left0[bo_y:]) + [0] * 16)[:16], np.uint8))
        ctx_out_all.append(np.array(ctx_out, np.uint8))
        above_all.append(np.array(above0, np.uint8))
        left_all.append(np.array(left0, np.uint8))
        cdf_all.append(gather(leaves(fc0, ts, inter, red)))
        print(len(rows), name, "tt", tt, "inter", inter, "red", red, "cb", cb, "y_mode", y_mode, "geom", geom, "eobs",
              [int(e) for e in eobs], "coded", ncoded, "rate", rate, "indep", indep, "cul", cul, flush=True)

    def neighbours(kind):
        """above_coeff_context[0] (64 entries) / left_coeff_context[0] (16): 0 = the frame's first block"""
        if kind == 0:
            return [0] * 64, [0] * 16
        hi = (0, 4, 64)[kind]
        a = rng.integers(0, hi, 64) | (rng.integers(0, 3, 64) << 6)
        l = rng.integers(0, hi, 16) | (rng.integers(0, 3, 16) << 6)
        a[rng.integers(0, 64, 20)] = 0
        l[rng.integers(0, 16, 5)] = 0
        return [int(v) for v in a], [int(v) for v in l]

    # ---------------- synthetic cases: every shape ROUNDS times, the other properties cycling against it
    ci = 0
    for rnd in range(ROUNDS):
        for (bw, bh, ts) in SHAPES:
            tw, th = TX_W[ts], TX_H[ts]
            W, H = min(tw, 32), min(th, 32)
            area = W * H
            gw, gh = bw // tw, bh // th
            ntx = gw * gh
            inter, red = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 0))[(ci + rnd) % 5]
            sd = int(get_set({}, TxSize[ts], bool(inter), bool(red)).disc)
            allowed = [t for t in (0, 10, 11, 9, 1, 3) if tx_used[sd][t]]       # DCT_DCT, V_DCT, H_DCT, IDTX: the three classes
            tt = allowed[(ci // 2) % len(allowed)]
            cb = 2 if ci % 2 == 0 else 4
            y_mode = ci % 13
            # the block's place and the tile / frame edges through it
            bo_x = (bw >> 2) * ((ci % 3) + 1)
            bo_y = ((bh >> 2) * (ci % 4)) % 16
            edge = ci % 7
            mi_w, mi_h = 255, 255                        # relative to the block, as the descriptor holds them
            if edge in (3, 5) and gw > 1:
                mi_w = (bw >> 2) - (tw >> 2)             # the last column is not coded
            if edge in (4, 5) and gh > 1:
                mi_h = (bh >> 2) - (th >> 2)             # the last row is not coded
            clip_w, clip_h = mi_w, mi_h
            if edge == 6:
                if tw >= 8:
                    mi_w = clip_w = (bw >> 2) - 1        # the last column is coded with a clipped span
                if th >= 8:
                    mi_h = clip_h = (bh >> 2) - 1
            if edge == 3 and mi_w != 255:
                clip_w = mi_w + 3                        # a tile edge inside the frame
            geom = (bo_x, bo_y, min(bo_x + mi_w, 1000), min(bo_y + mi_h, 1000), min(bo_x + clip_w, 1000), min(bo_y + clip_h, 1000))
            coded = [by * gw + bx for by in range(gh) for bx in range(gw)
                     if bx * (tw >> 2) < mi_w and by * (th >> 2) < mi_h]
            # eobs: zero first / in the middle / last / everywhere / nowhere
            pat = ci % 6
            big = 32767 if cb == 2 else (1 << 20) - 1
            pool = {0: [0, 0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 14, 15], 2: [1, 2, 3, 14, 15, 127, 128, big],
                    3: [0, 0, 0, 1], 4: [0, 1, 2, 3, 4, 7, 15, 16, 17, 127, 128, 300, big // 7, big]}[(ci + rnd) % 5]
            eobs = np.zeros(ntx, np.int64)
            qcs = np.zeros((ntx, area), np.int64)
            scan = [int(v) for v in orders[ts][tt].scan]
            for n_, k in enumerate(coded):
                zero = {0: False, 1: n_ == 0, 2: n_ == len(coded) // 2, 3: n_ == len(coded) - 1, 4: True,
                        5: rng.integers(0, 3) == 0}[pat]
                if zero:
                    continue
                if (bw, bh, ts) == (64, 64, 3):
                    eob = (300, 257, 1024, 700, 513)[(n_ + rnd) % 5]            # past one chunk of 256
                else:
                    eob = area if rng.integers(0, 5) == 0 and area <= 256 else int(rng.integers(1, min(area, 40) + 1))
                mags = rng.choice(pool, eob)
                if (bw, bh, ts) == (64, 64, 3) and rnd % 2 == 0:
                    mags = rng.choice([0, 0, 1, 1, 2, 3], eob)                  # one coeff_base row hit hundreds of times
                if mags[-1] == 0:
                    mags[-1] = int(rng.choice([1, 2, 3, 15, big]))
                vals = mags * rng.choice([-1, 1], eob)
                if eob > 1:
                    vals[0] = abs(int(vals[0]) or 1) * (-1, 0, 1)[(ci + n_) % 3]  # negative, zero and positive DC
                eobs[k] = eob
                qcs[k, np.array(scan[:eob], np.int64)] = vals
            above0, left0 = neighbours((ci + rnd) % 3)
            kind = ci % 2                               # 0: CDFContext::new(q), 1: seeded, counters at the rate steps
            fc0 = copy.deepcopy(fcs[(10, 40, 100, 200)[(ci // 2) % 4]])
            if kind == 1:
                seed_random(leaves(fc0, ts, inter, red))
            add("%dx%d/%dx%d r%d e%d p%d c%d" % (bw, bh, tw, th, rnd, edge, pat, kind), bw, bh, ts, tt, inter, red, cb, y_mode,
                geom, above0, left0, qcs, eobs, fc0)
            ci += 1
    rr = np.array(rows, np.int64)
    assert set(rr[rr[:, 4] == 0][:, 7]) == set(range(13)), "every y_mode on an intra case"
    assert {0, 9, 10, 11} <= set(rr[:, 3]), sorted(set(rr[:, 3]))

    # ---------------- real content: write_tx_blocks cases of rdo_intra_split_ref.npz
    here = os.path.dirname(os.path.abspath(__file__))
    S = np.load(os.path.join(here, "rdo_intra_split_ref.npz"))
    col = {n: i for i, n in enumerate(S["columns"])}
    picked = 0
    for i, row in enumerate(S["cases"]):
        v = lambda n: int(row[col[n]])
        bw, bh, ts = v("bw"), v("bh"), v("ts")
        right_or_bottom = v("coded") < (bw // TX_W[ts]) * (bh // TX_H[ts])
        if not (right_or_bottom or i % 4 == 1) or bw * bh > 1024:
            continue
        mi_width, mi_height = (v("plane_w") + 3) // 4, (v("plane_h") + 3) // 4
        geom = (v("x") >> 2, (v("y") >> 2) % 16, mi_width, mi_height - (v("y") >> 2) + (v("y") >> 2) % 16, mi_width,
                mi_height - (v("y") >> 2) + (v("y") >> 2) % 16)
        above0, left0 = neighbours(1 + i % 2)
        add("intra_split %d" % i, bw, bh, ts, v("tx_type"), 0, 0, 2 if v("bd") == 8 else 4, v("mode"), geom, above0, left0,
            S["qc_%d" % i].astype(np.int64), S["eob_%d" % i], copy.deepcopy(fcs[40 if v("qidx") <= 60 else (100 if v("qidx") <= 120 else 200)]))
        picked += 1
    assert picked >= 8, picked
    # ---------------- real content: write_tx_tree cases of rdo_txsearch_ref.npz
    T = np.load(os.path.join(here, "rdo_txsearch_ref.npz"))
    fw, fh = int(T["tsr_frame"][0]), int(T["tsr_frame"][1])
    mi_width, mi_height = (fw + 3) // 4, (fh + 3) // 4
    picked = 0
    for i, key in enumerate(T["txs_keys"]):
        key = str(key)
        bw, bh, tw, th, n_tx = (int(x) for x in T["txs_geom_" + key])
        bd, _bs, ts, qidx, bx, by = key.split("_")
        bd, ts, qidx, bx, by = int(bd), int(ts), int(qidx), int(bx), int(by)
        if i % 3 == 0 or bw * bh > 1024 or by % 16 + (bh >> 2) > 16:      # left_coeff_context holds one superblock
            continue
        gw, gh = bw // tw, bh // th
        coded = [y * gw + x for y in range(gh) for x in range(gw)
                 if bx + x * (tw >> 2) < mi_width and by + y * (th >> 2) < mi_height]
        assert len(coded) == n_tx, (key, coded, n_tx)
        types = [int(t) for t in T["txs_types_" + key]]
        j = i % len(types)
        area = min(tw, 32) * min(th, 32)
        qcs, eobs = np.zeros((gw * gh, area), np.int64), np.zeros(gw * gh, np.int64)
        for n_, k in enumerate(coded):
            qcs[k], eobs[k] = T["txs_qc_" + key][j][n_], T["txs_eob_" + key][j][n_]
        geom = (bx, by % 16, mi_width, mi_height - by + by % 16, mi_width, mi_height - by + by % 16)
        above0, left0 = neighbours(i % 3)
        add("tx_tree " + key, bw, bh, ts, types[j], 1, 0, 2 if bd == 8 else 4, 0, geom, above0, left0, qcs, eobs,
            copy.deepcopy(fcs[40 if qidx <= 60 else (100 if qidx <= 120 else 200)]))
        picked += 1
    assert picked >= 8, picked

    out = {"case_rows": np.array(rows, np.int64), "case_names": np.array(names), "case_geom": np.array(geoms, np.int32),
           "case_qc": np.array(qc_all, np.int32), "case_eobs": np.stack(eobs_all), "case_tell": np.stack(tell_all),
           "case_cul": np.stack(cul_all), "case_ctx_in": np.stack(ctx_in_all), "case_ctx_out": np.stack(ctx_out_all),
           "case_above": np.stack(above_all), "case_left": np.stack(left_all), "case_cdfs": np.stack(cdf_all)}
    print("cases:", len(rows), flush=True)
    L.save("coeff_rate_chain_ref.npz", out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tests/golden/coeff_rate_ref.npz: the real coefficient rate of one transform block as rdo_tx_type_decision
measures it per transform type (src/rdo.rs:1744-1799: a fresh WriterCounter, tell_frac, write the block, tell_frac,
roll the CDFs back), computed by the REFERENCE'S OWN SOURCE TEXT through tools/rustlite.

Executed whole, on a WriterBase<WriterCounter> made by the executed WriterCounter::new():
  write_coeffs_lv_map, encode_eob, encode_coeffs, encode_coeff_signs   src/context/block_unit.rs:1783-2016
  BlockContext::get_txb_ctx, set_dc_sign, set_coeff_context           src/context/block_unit.rs:325-352, 442-526
  write_tx_type, get_tx_set, get_tx_set_index, txb_init_levels, get_eob_pos_token, get_nz_mag, get_nz_map_ctx*,
  get_nz_map_contexts, get_br_ctx, get_txsize_entropy_ctx, get_txb_bhl  src/context/transform_unit.rs
  symbol, bool, bit, write_golomb, tell, tell_frac, store, lr_compute, frac_compute, update_cdf   src/ec.rs
  CDFContext::new(q) with the default tables of src/entropymode.rs / src/token_cdfs.rs through cdf() .. cdf_5d()
  av1_get_coded_tx_size (src/context/mod.rs:95-102), av1_scan_orders (src/scan_order.rs)

Restatements (docs/PARITY.md, "coefficient rate"):
  * symbol_with_update! (src/context/cdf_context.rs:564-579) expands to what Writer::symbol_with_update
    (src/ec.rs:548-562) does without the rollback log: `w.symbol(s, cdf); update_cdf(cdf, s)` on the CDF array
    itself (tools/rustlite/transpile.py).  CDFOffset and CDFContextLog are not modelled.
  * Where the reference rolls the CDFs back (cw.rollback, rdo.rs:1799) the generator starts every case from a saved
    copy of `fc`.
  * ContextWriter / BlockContext are plain objects with the fields the text reads (bc, fc; above_coeff_context,
    left_coeff_context).
  * cdf() .. cdf_5d() take CDF_LEN (and the outer lengths) from the declared type of the item they initialise: the
    transpiler has no type inference for a const generic that only the return type fixes.

CDF snapshots: CDFContext::new(q) for the four quantizer classes; the same state after it has coded earlier fixture
blocks without a roll-back (adapted rows, non-zero counters); seeded random CDFs that satisfy symbol()'s
debug_assert!s, scattered into the CDFContext the text reads, with counters that include 0, 15, 16, 31 and 32.
Each case stores the R1CoeffCdfs slice it used (gathered as include/rav1e_amd.h says) as run-time data.

Per case: the inputs, rate, cul_level (the value handed to set_coeff_context, read back from above_coeff_context),
the writer's final (bits, rng) and the list of (cdf id, symbol) in coding order (id = field * 64 + row, fields in
R1CoeffCdfs order).  Also: get_txb_ctx on 200 random neighbour arrays, every table the kernel restates, the
dimension constants of R1CoeffCdfs.

Run in the build container:  python tests/golden/gen_coeff_rate_ref.py
"""
import copy

import numpy as np

import reflib as L
from reflib import R

FILES = ["ec.rs", "context/mod.rs", "context/block_unit.rs", "context/transform_unit.rs", "context/cdf_context.rs",
         "transform/mod.rs", "scan_order.rs", "util/mod.rs", "util/cdf.rs", "partition.rs", "predict.rs"]
FIELDS = ("txb_skip", "eob_flag", "eob_extra", "coeff_base_eob", "coeff_base", "coeff_br", "dc_sign", "tx_type")
RAV1E_TYPES = (0, 1, 2, 3, 9, 10, 11)        # RAV1E_TX_TYPES (pinned by rdo_txsearch_ref.npz)


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class CW(Obj):
    _rname = "ContextWriter"


class BC(Obj):
    _rname = "BlockContext"


def main():
    c = L.crate(*FILES)
    trace = []
    c.define_py("r1_sym_trace", lambda _g, cdf, s: trace.append((id(cdf), int(s))))
    K = lambda name: int(c.const_value(name))
    dims = {n: K(n) for n in ("TXB_SKIP_CONTEXTS", "EOB_COEF_CONTEXTS", "SIG_COEF_CONTEXTS_EOB", "SIG_COEF_CONTEXTS",
                              "LEVEL_CONTEXTS", "BR_CDF_SIZE", "DC_SIGN_CONTEXTS", "INTRA_MODES")}
    shapes = (("txb_skip", dims["TXB_SKIP_CONTEXTS"], 2), ("eob_flag", 2, 11), ("eob_extra", dims["EOB_COEF_CONTEXTS"], 2),
              ("coeff_base_eob", dims["SIG_COEF_CONTEXTS_EOB"], 3), ("coeff_base", dims["SIG_COEF_CONTEXTS"], 4),
              ("coeff_br", dims["LEVEL_CONTEXTS"], dims["BR_CDF_SIZE"]), ("dc_sign", dims["DC_SIGN_CONTEXTS"], 2),
              ("tx_type", dims["INTRA_MODES"], 16))
    rec_len = sum(r * n for _, r, n in shapes)

    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants][:19]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    BlockSize = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
    bs_names = [v[0] for v in c.enums["BlockSize"].variants]
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
    coded = c.get("av1_get_coded_tx_size")
    get_txb_ctx = c.get("get_txb_ctx", owner="BlockContext")
    tw = [int(c.call_method(t, "width", [])) for t in TxSize]
    th = [int(c.call_method(t, "height", [])) for t in TxSize]
    cw_ = [int(c.call_method(coded({}, t), "width", [])) for t in TxSize]
    ch_ = [int(c.call_method(coded({}, t), "height", [])) for t in TxSize]
    num_tx_set = [int(v) for v in c.const_value("num_tx_set")]
    tx_used = np.array(c.const_value("av1_tx_used").tolist(), np.int32)

    out = {"dims": np.array([dims[n] for n in ("TXB_SKIP_CONTEXTS", "EOB_COEF_CONTEXTS", "SIG_COEF_CONTEXTS_EOB",
                                               "SIG_COEF_CONTEXTS", "LEVEL_CONTEXTS", "BR_CDF_SIZE", "DC_SIGN_CONTEXTS",
                                               "INTRA_MODES")], np.int32),
           "tx_wh": np.array([tw, th, cw_, ch_], np.int32)}

    # ---------------- the tables the kernel restates, as the executed text holds them
    for name in ("av1_tx_ind", "eob_to_pos_small", "eob_to_pos_large", "k_eob_group_start", "k_eob_offset_bits",
                 "nz_map_ctx_offset_1d", "av1_nz_map_ctx_offset", "num_tx_set", "av1_tx_used"):
        out["tab_" + name] = np.array(c.const_value(name).tolist(), np.int32)
    out["tab_tx_type_to_class"] = np.array([int(v.disc) for v in c.const_value("tx_type_to_class")], np.int32)
    out["tab_txs_ctx"] = np.array([int(txs_ctx_fn({}, t)) for t in TxSize], np.int32)
    out["tab_tx_set"] = np.array([[[int(get_set({}, t, bool(i), bool(r)).disc) for r in (0, 1)] for i in (0, 1)]
                                  for t in TxSize], np.int32)
    orders = c.const_value("av1_scan_orders")
    scan_off, scan_all = np.zeros((19, 16), np.int64), []
    pos = 0
    for ts in range(19):
        for tt in range(16):
            s = [int(v) for v in orders[ts][tt].scan]
            scan_off[ts, tt] = pos
            scan_all.extend(s)
            pos += len(s)
            assert len(s) == cw_[ts] * ch_[ts]
    out["scan_off"], out["scan_all"] = scan_off, np.array(scan_all, np.uint16)

    # ---------------- the R1CoeffCdfs slice of a CDFContext: its leaves, in struct order
    def leaves(fc, ts, plane_type, is_inter, reduced):
        """[(field index, row, n, the CDF array of fc), ..]: what include/rav1e_amd.h says the host gathers"""
        tctx = int(txs_ctx_fn({}, TxSize[ts]))
        ems = min(int(c.call_method(TxSize[ts], "area_log2", [])) - 4, 6)
        sq = int(c.call_method(TxSize[ts], "sqr", []).disc)
        res = [(0, r, 2, fc.txb_skip_cdf[tctx][r]) for r in range(dims["TXB_SKIP_CONTEXTS"])]
        flag = getattr(fc, "eob_flag_cdf%d" % (16 << ems))[plane_type]
        res += [(1, r, 5 + ems, flag[r]) for r in range(2)]
        res += [(2, r, 2, fc.eob_extra_cdf[tctx][plane_type][r]) for r in range(dims["EOB_COEF_CONTEXTS"])]
        res += [(3, r, 3, fc.coeff_base_eob_cdf[tctx][plane_type][r]) for r in range(dims["SIG_COEF_CONTEXTS_EOB"])]
        res += [(4, r, 4, fc.coeff_base_cdf[tctx][plane_type][r]) for r in range(dims["SIG_COEF_CONTEXTS"])]
        res += [(5, r, dims["BR_CDF_SIZE"], fc.coeff_br_cdf[min(tctx, 3)][plane_type][r])
                for r in range(dims["LEVEL_CONTEXTS"])]
        res += [(6, r, 2, fc.dc_sign_cdf[plane_type][r]) for r in range(dims["DC_SIGN_CONTEXTS"])]
        nset = num_tx_set[int(get_set({}, TxSize[ts], bool(is_inter), bool(reduced)).disc)]
        if nset > 1:
            idx = int(set_index({}, TxSize[ts], bool(is_inter), bool(reduced)))
            if is_inter:
                res.append((7, 0, nset, getattr(fc, "inter_tx_%d_cdf" % idx)[sq]))
            else:
                tab = getattr(fc, "intra_tx_%d_cdf" % idx)[sq]
                res += [(7, r, nset, tab[r]) for r in range(dims["INTRA_MODES"])]
        for (_f, _r, n, a) in res:
            assert len(a) == n, (FIELDS[_f], _r, n, len(a))
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

    def scatter(lv, rec):
        for (f, r, n, a) in lv:
            o = base[f] + r * shapes[f][2]
            for i in range(n):
                a[i] = int(rec[o + i])

    rng = np.random.default_rng(20261018)

    def random_rec(lv):
        rec = np.zeros(rec_len, np.uint16)
        for (f, r, n, _a) in lv:
            o = base[f] + r * shapes[f][2]
            v = np.sort(rng.choice(np.arange(64, 32704), n - 1, replace=False))[::-1]
            if rng.integers(0, 4) == 0:      # a skewed row: one symbol takes nearly everything
                v = np.sort(np.concatenate([rng.integers(32000, 32704, n - 1 - (n - 1) // 2),
                                            rng.integers(64, 700, (n - 1) // 2)]))[::-1]
            rec[o:o + n - 1] = v
            rec[o + n - 1] = (0, 15, 16, 31, 32, int(rng.integers(0, 33)))[int(rng.integers(0, 6))]
        return rec

    # ---------------- the cases
    def bigger(w, h):
        for (a, b) in ((2 * w, 2 * h), (2 * w, h), (w, 2 * h)):
            if "BLOCK_%dX%d" % (a, b) in BlockSize:
                return "BLOCK_%dX%d" % (a, b)
        return None

    # neighbour contexts that reach every txb_skip_ctx / dc_sign_ctx: (above fill, left fill, use a larger plane_bsize)
    NEIGH = ((0, 0, 0), (0, 0, 1), (0, 2, 1), (0, 5, 1), (1, 2, 1), (2, 9, 1), (7, 8, 1), (3, 0, 0), (0, 63, 1), (40, 1, 1), (5, 6, 0))
    SIGNS = ((), (1,), (2,), (1, 1, 2), (2, 2, 1), (1, 2))
    fcs = [new_fc({}, q) for q in (10, 40, 100, 200)]
    fc_adapt = [copy.deepcopy(f) for f in fcs]
    rows = []
    qc_all, sym_all, cdf_recs = [], [], []
    ci = changed = 0
    for ts in range(19):
        W, H = cw_[ts], ch_[ts]
        area = W * H
        combos = []
        for (plane, inter, red) in ((0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 0), (2, 1, 1)):
            sd = int(get_set({}, TxSize[ts], bool(inter), bool(red)).disc)
            for tt in RAV1E_TYPES:
                if tx_used[sd][tt]:
                    combos.append((plane, inter, red, tt))
        eobs = sorted(set([0, 1, 2, area // 8, area // 8 + 1, area // 4, area // 4 + 1, area - 1, area] +
                          [g for g in (3, 5, 9, 17, 33, 65, 129, 257, 513) if g <= area] +
                          [g - 1 for g in (5, 9, 17, 33, 65, 129, 257, 513) if g <= area]))
        ncase = max(len(eobs), len(combos))
        for k in range(ncase):
            plane, inter, red, tt = combos[(k + ci) % len(combos)]
            eob = eobs[k % len(eobs)] if k < len(eobs) else int(rng.integers(1, min(area, 40) + 1))
            cb = 2 if ci % 2 == 0 else 4
            # --- coefficients: the first eob scan positions, the last of them non-zero
            scan = scan_all[scan_off[ts, tt]:scan_off[ts, tt] + area]
            big = 32767 if cb == 2 else (1 << 20) - 1
            style = ci % 5
            pool = {0: [0, 0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 14, 15], 2: [1, 2, 3, 14, 15, 127, 128, big],
                    3: [0, 0, 0, 1], 4: [0, 1, 2, 3, 4, 7, 15, 16, 17, 127, 128, 300, big // 7, big]}[style]
            qc = np.zeros(area, np.int64)
            if eob:
                mags = rng.choice(pool, eob)
                if style == 3 and eob > 100:
                    mags[:] = 1                        # one coeff_base row hit hundreds of times
                if mags[-1] == 0:
                    mags[-1] = int(rng.choice([1, 2, 3, 15, big]))
                sg = rng.choice([-1, 1], eob)
                vals = mags * sg
                vals[0] = (abs(vals[0]) or 0) * (-1, 0, 1)[ci % 3] if eob > 1 else vals[0]
                if eob == 1 and vals[0] == 0:
                    vals[0] = -3
                qc[np.array(scan[:eob], np.int64)] = vals
            # --- neighbours
            af, lf, want_big = NEIGH[ci % len(NEIGH)]
            bname = bigger(tw[ts], th[ts]) if want_big else None
            if bname is None:
                bname = "BLOCK_%dX%d" % (tw[ts], th[ts])
            above, left = [af] * 32, [lf] * 32
            for i, s in enumerate(SIGNS[(ci // 2) % len(SIGNS)]):
                if (plane == 0 or af or i % 2) and i % 2 == 0:
                    j = i % max(1, tw[ts] >> 2)
                    above[j] = (above[j] & 63) | (s << 6)
                elif plane == 0 or lf:
                    j = i % max(1, th[ts] >> 2)
                    left[j] = (left[j] & 63) | (s << 6)
            y_mode = (ci * 5) % 13
            pred = NEARESTMV if inter else PM[y_mode]
            # --- the CDF snapshot
            kind = ci % 3                  # 0: CDFContext::new(q), 1: adapted, 2: random
            qi = (ci // 3) % 4
            fc = copy.deepcopy(fcs[qi] if kind != 1 else fc_adapt[qi])
            lv = leaves(fc, ts, int(plane != 0), inter, red)
            if kind == 2:
                scatter(lv, random_rec(lv))
            snap = gather(lv)
            ids = {id(a): f * 64 + r for (f, r, _n, a) in lv}

            def run(fc_):
                bc = BC(above_coeff_context=R.RSlice([R.RSlice(list(above)) for _ in range(3)]),
                        left_coeff_context=R.RSlice([R.RSlice(list(left)) for _ in range(3)]))
                cw = CW(bc=bc, fc=fc_)
                bo = TBO(BO(x=0, y=0))
                tc = get_txb_ctx({}, bc, BlockSize[bname], TxSize[ts], plane, bo, 0, 0, tw[ts], th[ts])
                w = new_counter({})
                tell = int(c.call_method(w, "tell_frac", []))
                del trace[:]
                g = {"T": "i16" if cb == 2 else "i32", "W": "WriterBase"}
                ret = wclm(g, cw, w, plane, bo, R.RSlice([int(v) for v in qc]), eob, pred, TxSize[ts], TxType[tt],
                           BlockSize[bname], 0, 0, bool(red), tw[ts], th[ts])
                rate = int(c.call_method(w, "tell_frac", [])) - tell
                assert ret is (eob != 0)
                return rate, int(bc.above_coeff_context[plane][0]), int(w.s.bits), int(w.rng), tc

            rate, cul, bits, wrng, tc = run(fc)
            syms = [(ids[i], s) for (i, s) in trace]       # KeyError: a symbol outside the gathered slice
            changed += int((gather(lv) != snap).any())      # the updates land in the CDFContext the slice was read from
            if kind == 1:                                   # adapt the running state with this block (no roll-back)
                r2 = run(fc_adapt[qi])
                assert r2[:4] == (rate, cul, bits, wrng)
            rows.append((ts, tt, plane, inter, red, y_mode, int(tc.txb_skip_ctx), int(tc.dc_sign_ctx), eob, cb, rate, cul,
                         bits, wrng, len(qc_all), len(sym_all), len(syms), kind, bs_names.index(bname)))
            qc_all.extend(int(v) for v in qc)
            sym_all.extend(syms)
            cdf_recs.append(snap)
            print(len(rows), "ts", ts, "tt", tt, "plane", plane, "inter", inter, "red", red, "eob", eob, "cb", cb,
                  "ctx", (int(tc.txb_skip_ctx), int(tc.dc_sign_ctx)), "kind", kind, "rate", rate, "cul", cul, "syms",
                  len(syms), flush=True)
            ci += 1
    rows = np.array(rows, np.int64)
    assert changed > len(rows) * 9 // 10, changed
    assert set(rows[:, 6]) == set(range(dims["TXB_SKIP_CONTEXTS"])), sorted(set(rows[:, 6]))
    assert set(rows[:, 7]) == set(range(dims["DC_SIGN_CONTEXTS"]))
    out["case_rows"] = rows       # columns: see COLS in tests/test_coeff_rate_ref.py
    out["case_qc"] = np.array(qc_all, np.int32)
    out["case_syms"] = np.array(sym_all, np.uint16).reshape(-1, 2)
    out["case_cdfs"] = np.stack(cdf_recs)
    print("cases:", len(rows), "symbols:", len(sym_all), flush=True)

    # ---------------- get_txb_ctx on random neighbour arrays
    trows = []
    for i in range(200):
        ts = int(rng.integers(0, 19))
        plane = int(rng.integers(0, 3))
        bname = bigger(tw[ts], th[ts]) if rng.integers(0, 2) else None
        if bname is None:
            bname = "BLOCK_%dX%d" % (tw[ts], th[ts])
        mode = i % 5
        hi = (1, 4, 64, 192, 4)[mode]
        above = [int(v) for v in rng.integers(0, hi, 16)]
        left = [int(v) for v in rng.integers(0, 64 if mode == 4 else hi, 16)]      # mode 4: one side below 4, one above
        if i % 7 == 0:
            above = [0] * 16
        if i % 11 == 0:
            left = [0] * 16
        bc = BC(above_coeff_context=R.RSlice([R.RSlice(above + [0] * 16) for _ in range(3)]),
                left_coeff_context=R.RSlice([R.RSlice(left + [0] * 16) for _ in range(3)]))
        tc = get_txb_ctx({}, bc, BlockSize[bname], TxSize[ts], plane, TBO(BO(x=0, y=0)), 0, 0, tw[ts], th[ts])
        trows.append(above + left + [plane, bs_names.index(bname), ts, int(tc.txb_skip_ctx), int(tc.dc_sign_ctx)])
    out["txb_rows"] = np.array(trows, np.int32)     # above[16], left[16], plane, plane_bsize, tx_size, txb_skip_ctx, dc_sign_ctx
    out["block_wh"] = np.array([[int(c.call_method(BlockSize[n], "width", [])), int(c.call_method(BlockSize[n], "height", []))]
                                for n in bs_names], np.int32)
    L.save("coeff_rate_ref.npz", out)


if __name__ == "__main__":
    main()

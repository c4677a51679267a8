#!/usr/bin/env python3
"""tests/golden/coeff_rate_block_ref.npz: the coefficient rate of a WHOLE block -- its luma transform blocks, then U's,
then V's, on one writer behind a few head symbols -- as the mode decision measures it (luma_chroma_mode_rdo,
src/rdo.rs:855-945; encode_block_post_cdef ends in one write_tx_blocks / write_tx_tree call with luma_only = false,
src/encoder.rs:2202-2240), computed by the REFERENCE'S OWN SOURCE TEXT through tools/rustlite.

Executed whole, once per coded transform block, on ONE ContextWriter / BlockContext / WriterBase<WriterCounter>:
  write_coeffs_lv_map with get_txb_ctx and set_coeff_context inside it, planes 0, 1 and 2
                                                                            src/context/block_unit.rs:1783-1857
  and everything gen_coeff_rate_ref.py lists below it (same files, same stand-ins, imported from there)
  has_chroma, largest_chroma_tx_size, subsampled_size, uv_intra_mode_to_tx_type_context, TxType::uv_inter:
  per case, and swept over all 22 block sizes x the three subsamplings x odd and even block positions (`sweep_*`)
  the head: k in {0, 1, 7} Writer::bool / Writer::symbol calls on the fresh counter in front of the coefficients
STATED HERE, as gen_coeff_rate_chain_ref.py states the luma loop (the functions want the pixel pipeline in front):
  the three loops and their tx_bo arithmetic   src/encoder.rs:2276-2311, 2352-2403 (write_tx_blocks),
                                                2440-2476, 2513-2561 (write_tx_tree)
  the chroma grid                               src/encoder.rs:2327-2338, 2492-2505
  the skip test of encode_tx_block              src/encoder.rs:1441
  frame_clipped_txw / frame_clipped_txh         src/encoder.rs:1561-1566 with the plane's xdec / ydec
  uv_tx_type                                    src/encoder.rs:2346-2350, 2507-2511
The start state is produced the reference's way: the head symbols are written on the fresh counter, `rng` and tell_frac
are recorded there.  Asserted per case with a head: the coefficient part run again on a SECOND fresh counter whose rng
alone is set to the recorded value gives the same tell_frac difference and the same final rng -- so
rate_from_fresh == head + (tell_frac behind - tell_frac of the start state), the sum a caller of the library forms.

The block lies at (bo_x, bo_y) of a tile at the frame's origin whose grid (mi_width, mi_height) and whose frame
(w_in_b, h_in_b) are chosen per case; above_coeff_context[p] holds 64 entries, left_coeff_context[p] 16, each plane
its own.

Per case: `case_rows` (columns = COLS of tests/coeff_rate_block_model.py), `case_geom`, the coefficients by plane and
raster index (`case_qc` at the three offsets of the row), `case_eobs` [3][16], the whole context arrays in front
(`case_above` [3][64], `case_left` [3][16]), the 96 bytes the descriptor holds in front and behind (`case_ctx_in`,
`case_ctx_out`: [plane][above 16, left 16]), `case_tell` [3][16] (tell_frac behind every block minus tell_frac of the
start state; a block that is not coded repeats the value in front of it), `case_cul` [3][16], both R1CoeffCdfs slices
in front (`case_cdfs` [2]: luma, chroma), the start and final rng, the head's tell_frac difference, the total rate.
Real content: the luma coefficients of rdo_intra_split_ref.npz / rdo_txsearch_ref.npz cases, with synthetic chroma.

Run in the build container:  python tests/golden/gen_coeff_rate_block_ref.py
"""
import copy
import os

import numpy as np

import reflib as L
from reflib import R
from gen_coeff_rate_ref import FILES, FIELDS, CW, BC

TX_W = (4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64)
TX_H = (4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16)
# (bw, bh, luma tx_size, xdec, ydec): one 4x4 chroma block behind four / one luma blocks; 16x16 / 8x8 in the three
# subsamplings (4:2:2: an 8x16 chroma transform); four 32x32 chroma blocks per plane behind one and sixteen luma blocks;
# 64x16; the sub-8x8 shapes of 4:2:0
SHAPES = ((8, 8, 0, 1, 1), (8, 8, 1, 1, 1), (16, 16, 1, 1, 1), (16, 16, 1, 1, 0), (16, 16, 1, 0, 0), (64, 64, 4, 0, 0),
          (64, 64, 2, 0, 0), (64, 16, 18, 0, 0), (4, 4, 0, 1, 1), (4, 8, 5, 1, 1), (8, 4, 6, 1, 1), (4, 16, 13, 1, 1),
          (16, 4, 14, 1, 1))
ROUNDS = 6
CS_NAME = {(1, 1): "Cs420", (1, 0): "Cs422", (0, 0): "Cs444"}


def main():
    c = L.crate(*FILES)
    L.load_v_frame_types(c)
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
    txs_ctx_fn = c.get("get_txsize_entropy_ctx", owner="ContextWriter")
    set_index = c.get("get_tx_set_index")
    get_set = c.get("get_tx_set")
    has_chroma = c.get("has_chroma")
    uv_intra = c.get("uv_intra_mode_to_tx_type_context")
    max_rect = c.const_value("max_txsize_rect_lookup")
    num_tx_set = [int(v) for v in c.const_value("num_tx_set")]
    tx_used = np.array(c.const_value("av1_tx_used").tolist(), np.int32)
    orders = c.const_value("av1_scan_orders")
    for ts in range(19):
        assert (int(c.call_method(TxSize[ts], "width", [])), int(c.call_method(TxSize[ts], "height", []))) == (TX_W[ts], TX_H[ts])
    mi = lambda obj, name: int(c.call_method(obj, name, []))

    def chroma_of(bname, xdec, ydec, inter):
        """-> None where subsampled_size refuses, else (plane_bsize name, uv_tx_size, bw_uv, bh_uv): the executed
        subsampled_size / largest_chroma_tx_size and the grid arithmetic of encoder.rs:2327-2338 (intra; bw *
        tx_size.width_mi() is bsize.width_mi() for a transform that divides the block) / 2492-2505 (inter)"""
        sub = c.call_method(BlockSize[bname], "subsampled_size", [xdec, ydec])
        if "Err" in str(sub):
            return None
        plane_bsize = c.call_method(sub, "unwrap", [])
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

    # ---------------- the sweep: 22 block sizes x three subsamplings x odd and even positions
    sweep = []
    for bi, bname in enumerate(bs_names):
        for (xdec, ydec) in ((1, 1), (1, 0), (0, 0)):
            for (px, py) in ((0, 0), (1, 0), (0, 1), (1, 1)):
                hc = bool(has_chroma({}, TBO(BO(x=6 + px, y=4 + py)), BlockSize[bname], xdec, ydec, CS[(xdec, ydec)]))
                row = [bi, xdec, ydec, px, py, int(hc)]
                for inter in (0, 1):
                    ch = chroma_of(bname, xdec, ydec, inter)
                    row += [-1, -1, -1, -1] if ch is None else [bs_names.index(ch[0]), ch[1], ch[2], ch[3]]
                sweep.append(row)
    assert len(bs_names) == 22 and len(sweep) == 22 * 12
    sweep_uv_intra = [int(uv_intra({}, PM[m]).disc) for m in range(14)]
    sweep_uv_inter = [[int(c.call_method(TxType[t], "uv_inter", [TxSize[ts]]).disc) for ts in range(19)] for t in range(16)]
    sweep_block_wh = [[mi(BlockSize[n], "width"), mi(BlockSize[n], "height")] for n in bs_names]

    def leaves(fc, ts, plane_type, is_inter, reduced):
        """the (txs_ctx(ts), plane_type) R1CoeffCdfs slice of a CDFContext (include/rav1e_amd.h), as gen_coeff_rate_ref.py
        gathers it; the tx_type rows belong to the luma slice only"""
        tctx = int(txs_ctx_fn({}, TxSize[ts]))
        ems = min(int(c.call_method(TxSize[ts], "area_log2", [])) - 4, 6)
        sq = int(c.call_method(TxSize[ts], "sqr", []).disc)
        res = [(0, r, 2, fc.txb_skip_cdf[tctx][r]) for r in range(dims["TXB_SKIP_CONTEXTS"])]
        flag = getattr(fc, "eob_flag_cdf%d" % (16 << ems))[plane_type]
        res += [(1, r, 5 + ems, flag[r]) for r in range(2)]
        res += [(2, r, 2, fc.eob_extra_cdf[tctx][plane_type][r]) for r in range(dims["EOB_COEF_CONTEXTS"])]
        res += [(3, r, 3, fc.coeff_base_eob_cdf[tctx][plane_type][r]) for r in range(dims["SIG_COEF_CONTEXTS_EOB"])]
        res += [(4, r, 4, fc.coeff_base_cdf[tctx][plane_type][r]) for r in range(dims["SIG_COEF_CONTEXTS"])]
        res += [(5, r, dims["BR_CDF_SIZE"], fc.coeff_br_cdf[min(tctx, 3)][plane_type][r]) for r in range(dims["LEVEL_CONTEXTS"])]
        res += [(6, r, 2, fc.dc_sign_cdf[plane_type][r]) for r in range(dims["DC_SIGN_CONTEXTS"])]
        nset = num_tx_set[int(get_set({}, TxSize[ts], bool(is_inter), bool(reduced)).disc)]
        if plane_type == 0 and nset > 1:
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

    rng = np.random.default_rng(20261020)

    def seed_random(lv):
        """valid CDFs with counters on either side of update_cdf's rate steps (15 / 16, 31 / 32)"""
        for (f, r, n, a) in lv:
            v = np.sort(rng.choice(np.arange(64, 32704), n - 1, replace=False))[::-1]
            for i in range(n - 1):
                a[i] = int(v[i])
            a[n - 1] = (15, 16, 31, 32, 14, 30, 0, int(rng.integers(0, 33)))[int(rng.integers(0, 8))]

    fcs = {q: new_fc({}, q) for q in (10, 40, 100, 200)}
    HEAD_CDFS = ([30000, 20000, 9000, 0], [16000, 5], [32000, 31000, 700, 650, 600, 90, 32], [120, 64, 0])

    def write_head(w, nhead, salt):
        """nhead arbitrary Writer::bool / Writer::symbol calls: CDFs the coefficients never touch"""
        for i in range(nhead):
            if (i + salt) % 2:
                c.call_method(w, "bool", [bool((i + salt) % 3 == 0), (12000, 16384, 700, 32000)[(i + salt) % 4]])
            else:
                cdf = HEAD_CDFS[(i + salt) % len(HEAD_CDFS)]
                c.call_method(w, "symbol", [(i * 5 + salt) % len(cdf), R.RSlice(list(cdf))])

    def run_case(bw, bh, ts, xdec, ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, do_chroma, geom, above0, left0, qcs, eobs,
                 fc0, nhead, salt):
        bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b = geom
        bname = "BLOCK_%dX%d" % (bw, bh)
        bsize = BlockSize[bname]
        tw, th = TX_W[ts], TX_H[ts]
        gw, gh = bw // tw, bh // th
        g = {"T": "i16" if cb == 2 else "i32", "W": "WriterBase"}
        pname, uv_ts, bw_uv, bh_uv = chroma_of(bname, xdec, ydec, inter)
        utw_mi, uth_mi = TX_W[uv_ts] >> 2, TX_H[uv_ts] >> 2
        w_mi, h_mi = bw >> 2, bh >> 2      # bw * tx_size.width_mi() (2366) and max_tx_size.width_mi() (2527) alike

        def coefficients(w, bc, cw):
            """the three loops -> (tell_frac behind every block [3][16], cul_level [3][16], coded count)"""
            tell = [[None] * 16 for _ in range(3)]
            cul = [[0] * 16 for _ in range(3)]
            ncoded = 0
            tf = lambda: int(c.call_method(w, "tell_frac", []))
            # luma: encoder.rs:2276-2311, 2440-2476
            for by in range(gh):
                for bx in range(gw):
                    k = by * gw + bx
                    tbx, tby = bo_x + bx * (tw >> 2), bo_y + by * (th >> 2)
                    if tbx >= mi_width or tby >= mi_height:
                        tell[0][k] = tf()
                        continue
                    clipped_w = min((w_in_b - tbx) << 2, tw)            # the tile lies at the frame's origin: frame_bo = tx_bo
                    clipped_h = min((h_in_b - tby) << 2, th)
                    ret = wclm(g, cw, w, 0, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[0][k]]), int(eobs[0][k]),
                               NEARESTMV if inter else PM[y_mode], TxSize[ts], TxType[tt], bsize, 0, 0, bool(red), clipped_w,
                               clipped_h)
                    assert ret is (int(eobs[0][k]) != 0)
                    tell[0][k] = tf()
                    cul[0][k] = int(bc.above_coeff_context[0][tbx])
                    ncoded += 1
            if not do_chroma:
                return tell, cul, ncoded
            # chroma: encoder.rs:2352-2403, 2513-2561
            for p in (1, 2):
                for by in range(bh_uv):
                    for bx in range(bw_uv):
                        k = by * bw_uv + bx
                        tbx = bo_x + ((bx * utw_mi) << xdec) - int(w_mi == 1) * xdec
                        tby = bo_y + ((by * uth_mi) << ydec) - int(h_mi == 1) * ydec
                        if tbx >= mi_width or tby >= mi_height:             # encoder.rs:1441
                            tell[p][k] = tf()
                            continue
                        assert (((w_in_b - tbx) << 2) >> xdec) >= 4 and (((h_in_b - tby) << 2) >> ydec) >= 4     # 1559-1560
                        clipped_w = min(((w_in_b - tbx) << 2) >> xdec, TX_W[uv_ts])
                        clipped_h = min(((h_in_b - tby) << 2) >> ydec, TX_H[uv_ts])
                        ret = wclm(g, cw, w, p, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[p][k]]), int(eobs[p][k]),
                                   NEARESTMV if inter else PM[uv_mode], TxSize[uv_ts], TxType[uv_tt], BlockSize[pname], xdec, ydec,
                                   bool(red), clipped_w, clipped_h)
                        assert ret is (int(eobs[p][k]) != 0)
                        tell[p][k] = tf()
                        cul[p][k] = int(bc.above_coeff_context[p][tbx >> xdec])
                        ncoded += 1
            return tell, cul, ncoded

        def state():
            bc = BC(above_coeff_context=R.RSlice([R.RSlice(list(above0[p])) for p in range(3)]),
                    left_coeff_context=R.RSlice([R.RSlice(list(left0[p])) for p in range(3)]))
            return bc, CW(bc=bc, fc=copy.deepcopy(fc0)), new_counter({})

        bc, cw, w = state()
        tell_fresh = int(c.call_method(w, "tell_frac", []))
        write_head(w, nhead, salt)
        rng0, tell_h = int(w.rng), int(c.call_method(w, "tell_frac", []))
        tell, cul, ncoded = coefficients(w, bc, cw)
        tell_end, rng_out = int(c.call_method(w, "tell_frac", [])), int(w.rng)
        # the 96 bytes the descriptor holds, behind
        ux, uy = bo_x - int(w_mi == 1) * xdec, bo_y - int(h_mi == 1) * ydec
        origin = [(bo_x, bo_y % 16), (ux >> xdec, (uy % 16) >> ydec), (ux >> xdec, (uy % 16) >> ydec)]

        def window(ab, lf):
            out = []
            for p in range(3):
                x0, y0 = origin[p]
                out += ([int(v) for v in list(ab[p])[x0:x0 + 16]] + [0] * 16)[:16]
                out += ([int(v) for v in list(lf[p])[y0:y0 + 16]] + [0] * 16)[:16]
            return out

        ctx_in, ctx_out = window(above0, left0), window(bc.above_coeff_context, bc.left_coeff_context)
        if nhead:       # the device's way: a fresh counter that takes over nothing but rng
            bc2, cw2, w2 = state()
            w2.rng = rng0
            t2 = int(c.call_method(w2, "tell_frac", []))
            coefficients(w2, bc2, cw2)
            assert int(c.call_method(w2, "tell_frac", [])) - t2 == tell_end - tell_h and int(w2.rng) == rng_out
            assert tell_end - tell_fresh == (tell_h - tell_fresh) + (int(c.call_method(w2, "tell_frac", [])) - t2)
        else:
            assert rng0 == 0x8000 and tell_h == tell_fresh
        # tell_frac behind every block, relative to the start state; blocks outside a grid repeat what lies in front
        rel, last = [[0] * 16 for _ in range(3)], 0
        for p in range(3):
            for k in range(16):
                if tell[p][k] is not None:
                    last = tell[p][k] - tell_h
                rel[p][k] = last
        clip_uv = (min(255, (((w_in_b - ux) << 2) >> xdec) >> 2), min(255, (((h_in_b - uy) << 2) >> ydec) >> 2))
        return dict(rate=tell_end - tell_h, head=tell_h - tell_fresh, rng0=rng0, rng_out=rng_out, tell=rel, cul=cul, ctx_in=ctx_in,
                    ctx_out=ctx_out, ncoded=ncoded, uv_ts=uv_ts, bw_uv=bw_uv, bh_uv=bh_uv, clip_uv=clip_uv)

    rows, names, geoms, qc_all = [], [], [], []
    acc = {k: [] for k in ("eobs", "tell", "cul", "ctx_in", "ctx_out", "above", "left", "cdfs")}

    def add(name, bw, bh, ts, xdec, ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, do_chroma, geom, above0, left0, qcs, eobs,
            fc0, nhead, salt):
        r = run_case(bw, bh, ts, xdec, ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, do_chroma, geom, above0, left0, qcs, eobs,
                     fc0, nhead, salt)
        bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b = geom
        offs = []
        for p in range(3):
            offs.append(len(qc_all))
            for q in qcs[p]:
                qc_all.extend(int(v) for v in q)
        rows.append((bw, bh, ts, xdec, ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, int(do_chroma), r["uv_ts"], r["bw_uv"],
                     r["bh_uv"], min(255, mi_width - bo_x), min(255, mi_height - bo_y), min(255, w_in_b - bo_x),
                     min(255, h_in_b - bo_y), r["clip_uv"][0], r["clip_uv"][1], nhead, r["rng0"], r["head"], r["rate"], r["rng_out"],
                     offs[0], offs[1], offs[2]))
        names.append(name)
        geoms.append(geom)
        e = np.zeros((3, 16), np.uint16)
        for p in range(3):
            e[p, :len(eobs[p])] = eobs[p]
        acc["eobs"].append(e)
        acc["tell"].append(np.array(r["tell"], np.uint32))
        acc["cul"].append(np.array(r["cul"], np.uint8))
        acc["ctx_in"].append(np.array(r["ctx_in"], np.uint8))
        acc["ctx_out"].append(np.array(r["ctx_out"], np.uint8))
        acc["above"].append(np.array(above0, np.uint8))
        acc["left"].append(np.array(left0, np.uint8))
        acc["cdfs"].append(np.stack([gather(leaves(fc0, ts, 0, inter, red)), gather(leaves(fc0, r["uv_ts"], 1, inter, red))]))
        print(len(rows), name, "tt", tt, "uv_tt", uv_tt, "inter", inter, "cb", cb, "chroma", int(do_chroma), "geom", geom, "eobs",
              [[int(v) for v in e_] for e_ in eobs], "coded", r["ncoded"], "head", nhead, hex(r["rng0"]), r["head"], "rate", r["rate"],
              flush=True)

    def neighbours(kinds):
        """above_coeff_context[p] (64 entries) / left_coeff_context[p] (16) per plane: kind 0 = the frame's first block,
        3 = DC signs that cancel across above and left (every entry a sign, as many negative as positive)"""
        ab, lf = [], []
        for kind in kinds:
            if kind == 0:
                ab.append([0] * 64)
                lf.append([0] * 16)
                continue
            if kind == 3:
                ab.append([int(v) | (1 << 6) for v in rng.integers(1, 64, 64)])
                lf.append([int(v) + (2 << 6) for v in rng.integers(1, 64, 16)])
                continue
            hi = (0, 4, 64)[kind]
            a = rng.integers(0, hi, 64) | (rng.integers(0, 3, 64) << 6)
            l = rng.integers(0, hi, 16) | (rng.integers(0, 3, 16) << 6)
            a[rng.integers(0, 64, 20)] = 0
            l[rng.integers(0, 16, 5)] = 0
            ab.append([int(v) for v in a])
            lf.append([int(v) for v in l])
        return ab, lf

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

    def chroma_blocks(uv_ts, uv_tt, n_uv, cb, style, zero_u, zero_v, ci, long_eob=False):
        """synthetic U and V transform blocks -> ([U blocks, V blocks], [U eobs, V eobs])"""
        W, H = min(TX_W[uv_ts], 32), min(TX_H[uv_ts], 32)
        area = W * H
        big = 32767 if cb == 2 else (1 << 20) - 1
        pool = {0: [0, 0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 14, 15], 2: [1, 2, 3, 14, 15, 127, 128, big], 3: [0, 0, 0, 1],
                4: [0, 1, 2, 3, 4, 7, 15, 16, 17, 127, 128, 300, big // 7, big]}[style]
        scan = [int(v) for v in orders[uv_ts][uv_tt].scan]
        qs, es = [], []
        for p, zero in ((1, zero_u), (2, zero_v)):
            q, e = np.zeros((n_uv, area), np.int64), np.zeros(n_uv, np.int64)
            for k in range(n_uv):
                if zero or (style == 3 and k == 1):
                    continue
                if long_eob:
                    eob = (300, 1024, 257, 513, 700)[(k + p + ci) % 5]           # past one chunk of 256
                else:
                    eob = area if rng.integers(0, 5) == 0 and area <= 64 else int(rng.integers(1, min(area, 30) + 1))
                e[k] = eob
                q[k] = fill(area, scan, eob, pool, big, (-1, 0, 1)[(ci + k + p) % 3])
            qs.append(q)
            es.append(e)
        return qs, es

    cyc = {}

    def synth(ci, rnd, bw, bh, ts, xdec, ydec, force=None):
        """one synthetic case; force = (tx_type, eob pattern): an inter, full-set case of that luma type"""
        tw, th = TX_W[ts], TX_H[ts]
        W, H = min(tw, 32), min(th, 32)
        area = W * H
        gw, gh = bw // tw, bh // th
        ntx = gw * gh
        bname = "BLOCK_%dX%d" % (bw, bh)
        inter, red = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (1, 0))[(ci + rnd) % 6] if force is None else (1, 0)
        sd = int(get_set({}, TxSize[ts], bool(inter), bool(red)).disc)
        allowed = [t for t in ((9, 10, 11, 0, 1, 3) if inter else (0, 1, 3, 10, 11, 9)) if tx_used[sd][t]]
        _pname, uv_ts, bw_uv, bh_uv = chroma_of(bname, xdec, ydec, inter)
        key = (inter, red, bw_uv * bh_uv > 0)       # every class of a set in turn on the shapes that have a chroma grid
        cyc[key] = cyc.get(key, -1) + 1
        tt = allowed[cyc[key] % len(allowed)] if force is None else force[0]
        cb = 2 if ci % 2 == 0 else 4
        y_mode, uv_mode = ci % 13, (ci * 3 + rnd) % 14
        # the block's place (both parities of a sub-8x8 block's offset) and the tile / frame edges through it
        small = bw == 4 or bh == 4
        bo_x = ((bw >> 2) * ((ci % 3) + 1) + (rnd % 2 if bw == 4 else 0)) if small else (bw >> 2) * ((ci % 3) + 1)
        bo_y = ((bh >> 2) * (ci % 4)) % 16
        if bh == 4:
            bo_y = (bo_y + (rnd // 2) % 2) % 16
        if bw == 4 and bh == 4:
            bo_x, bo_y = 6 + (rnd % 2), 4 + ((rnd // 2) % 2)
        edge = (ci + rnd) % 7
        mi_w, mi_h = 255, 255                        # relative to the block, as the descriptor holds them
        if edge in (3, 5) and bw >= 16:
            mi_w = (bw >> 2) // 2                    # the right half is not coded: luma columns and the last chroma column
        if edge in (4, 5) and bh >= 16:
            mi_h = (bh >> 2) // 2
        clip_w, clip_h = mi_w, mi_h
        if edge == 6:
            if bw >= 16:
                mi_w = clip_w = (bw >> 2) - 1        # the last column is coded with a clipped span, luma and chroma
            if bh >= 16:
                mi_h = clip_h = (bh >> 2) - 1
        if edge == 3 and mi_w != 255:
            clip_w = mi_w + 3                        # a tile edge inside the frame
        geom = (bo_x, bo_y, min(bo_x + mi_w, 1000), min(bo_y + mi_h, 1000), min(bo_x + clip_w, 1000), min(bo_y + clip_h, 1000))
        do_chroma = bool(has_chroma({}, TBO(BO(x=bo_x, y=bo_y)), BlockSize[bname], xdec, ydec, CS[(xdec, ydec)]))
        coded = [by * gw + bx for by in range(gh) for bx in range(gw) if bx * (tw >> 2) < mi_w and by * (th >> 2) < mi_h]
        # eob == 0: nowhere / in all of U / in all of V / everywhere / in luma only / here and there
        pat = (ci + 2 * rnd) % 6 if force is None else force[1]
        big = 32767 if cb == 2 else (1 << 20) - 1
        style = (ci + rnd) % 5
        pool = {0: [0, 0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 14, 15], 2: [1, 2, 3, 14, 15, 127, 128, big],
                3: [0, 0, 0, 1], 4: [0, 1, 2, 3, 4, 7, 15, 16, 17, 127, 128, 300, big // 7, big]}[style]
        eobs_y = np.zeros(ntx, np.int64)
        qcs_y = np.zeros((ntx, area), np.int64)
        scan = [int(v) for v in orders[ts][tt].scan]
        for n_, k in enumerate(coded):
            if pat in (3, 4) or (pat == 5 and rng.integers(0, 3) == 0):
                continue
            eob = area if rng.integers(0, 5) == 0 and area <= 256 else int(rng.integers(1, min(area, 40) + 1))
            eobs_y[k] = eob
            qcs_y[k] = fill(area, scan, eob, pool, big, (-1, 0, 1)[(ci + n_) % 3])
        # uv_tx_type: encoder.rs:2346-2350 (intra), 2507-2511 (inter: partition_has_coeff of the luma loop)
        if inter:
            has_coeff = any(int(eobs_y[k]) for k in coded)
            uv_tt = int(c.call_method(TxType[tt], "uv_inter", [TxSize[uv_ts]]).disc) if has_coeff else 0
        else:
            uv_tt = 0 if TX_W[uv_ts] >= 32 or TX_H[uv_ts] >= 32 else int(uv_intra({}, PM[uv_mode]).disc)
        qs_uv, es_uv = chroma_blocks(uv_ts, uv_tt, bw_uv * bh_uv, cb, style, pat in (1, 3), pat in (2, 3), ci,
                                     long_eob=(bw, bh, xdec) == (64, 64, 0) and rnd % 2 == 0)
        above0, left0 = neighbours([(ci + rnd + p) % 4 for p in range(3)])
        kind = ci % 2                               # 0: CDFContext::new(q), 1: seeded, counters at the rate steps
        fc0 = copy.deepcopy(fcs[(10, 40, 100, 200)[(ci // 2) % 4]])
        if kind == 1:
            seed_random(leaves(fc0, ts, 0, inter, red))
            seed_random(leaves(fc0, uv_ts, 1, inter, red))
        nhead = (0, 1, 7)[(ci + rnd) % 3]
        add("%dx%d/%dx%d %d%d r%d e%d p%d c%d h%d%s" % (bw, bh, tw, th, xdec, ydec, rnd, edge, pat, kind, nhead, "" if force is None else " t%d" % tt), bw, bh, ts, xdec,
            ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, do_chroma, geom, above0, left0, [qcs_y, qs_uv[0], qs_uv[1]],
            [eobs_y, es_uv[0], es_uv[1]], fc0, nhead, ci)

    # ---------------- synthetic cases: every shape ROUNDS times, the other properties cycling against it
    ci = 0
    for rnd in range(ROUNDS):
        for shape in SHAPES:
            synth(ci, rnd, *shape)
            ci += 1
    # the chroma classes IDTX / V_DCT / H_DCT through uv_inter, where the size allows them: 4x4, 8x8 and 8x16 chroma
    for rnd, (shape, tt) in enumerate(((SHAPES[1], 9), (SHAPES[1], 10), (SHAPES[1], 11), (SHAPES[4], 10), (SHAPES[3], 11),
                                       (SHAPES[2], 10))):
        synth(ci, rnd, *shape, force=(tt, 0))
        ci += 1

    # ---------------- real content: luma of rdo_intra_split_ref.npz (write_tx_blocks) with synthetic chroma, 4:2:0
    here = os.path.dirname(os.path.abspath(__file__))
    S = np.load(os.path.join(here, "rdo_intra_split_ref.npz"))
    col = {n: i for i, n in enumerate(S["columns"])}
    picked = 0
    for i, row in enumerate(S["cases"]):
        v = lambda n: int(row[col[n]])
        bw, bh, ts = v("bw"), v("bh"), v("ts")
        if i % 5 != 1 or bw * bh > 1024 or picked >= 6:
            continue
        mi_width, mi_height = (v("plane_w") + 3) // 4, (v("plane_h") + 3) // 4
        bo_x, bo_y = v("x") >> 2, (v("y") >> 2) % 16
        # fi.w_in_b / h_in_b count whole 8x8s (an even number of units); the tile grid keeps the plane's own size
        even = lambda n: (n + 1) & ~1
        geom = (bo_x, bo_y, mi_width, mi_height - (v("y") >> 2) + bo_y, even(mi_width), even(mi_height) - (v("y") >> 2) + bo_y)
        bname = "BLOCK_%dX%d" % (bw, bh)
        do_chroma = bool(has_chroma({}, TBO(BO(x=bo_x, y=bo_y)), BlockSize[bname], 1, 1, CS[(1, 1)]))
        _pname, uv_ts, bw_uv, bh_uv = chroma_of(bname, 1, 1, 0)
        uv_mode = i % 14
        uv_tt = 0 if TX_W[uv_ts] >= 32 or TX_H[uv_ts] >= 32 else int(uv_intra({}, PM[uv_mode]).disc)
        cb = 2 if v("bd") == 8 else 4
        qs_uv, es_uv = chroma_blocks(uv_ts, uv_tt, bw_uv * bh_uv, cb, i % 3, False, False, i)
        above0, left0 = neighbours([1 + (i + p) % 2 for p in range(3)])
        add("intra_split %d" % i, bw, bh, ts, 1, 1, v("tx_type"), uv_tt, 0, 0, cb, v("mode"), uv_mode, do_chroma, geom, above0, left0,
            [S["qc_%d" % i].astype(np.int64), qs_uv[0], qs_uv[1]], [S["eob_%d" % i], es_uv[0], es_uv[1]],
            copy.deepcopy(fcs[40 if v("qidx") <= 60 else (100 if v("qidx") <= 120 else 200)]), (1, 7, 0)[picked % 3], i)
        picked += 1
    assert picked >= 4, picked
    # ---------------- real content: luma of the write_tx_tree cases of rdo_txsearch_ref.npz with synthetic chroma, 4:2:0
    T = np.load(os.path.join(here, "rdo_txsearch_ref.npz"))
    fw, fh = int(T["tsr_frame"][0]), int(T["tsr_frame"][1])
    mi_width, mi_height = (fw + 3) // 4, (fh + 3) // 4
    picked = 0
    for i, key in enumerate(T["txs_keys"]):
        key = str(key)
        bw, bh, tw, th, n_tx = (int(x) for x in T["txs_geom_" + key])
        bd, _bs, ts, qidx, bx, by = key.split("_")
        bd, ts, qidx, bx, by = int(bd), int(ts), int(qidx), int(bx), int(by)
        if i % 4 != 1 or bw * bh > 1024 or by % 16 + (bh >> 2) > 16 or picked >= 6:
            continue
        gw, gh = bw // tw, bh // th
        coded = [y * gw + x for y in range(gh) for x in range(gw) if bx + x * (tw >> 2) < mi_width and by + y * (th >> 2) < mi_height]
        assert len(coded) == n_tx, (key, coded, n_tx)
        types = [int(t) for t in T["txs_types_" + key]]
        j = i % len(types)
        area = min(tw, 32) * min(th, 32)
        qcs, eobs = np.zeros((gw * gh, area), np.int64), np.zeros(gw * gh, np.int64)
        for n_, k in enumerate(coded):
            qcs[k], eobs[k] = T["txs_qc_" + key][j][n_], T["txs_eob_" + key][j][n_]
        even = lambda n: (n + 1) & ~1
        geom = (bx, by % 16, mi_width, mi_height - by + by % 16, even(mi_width), even(mi_height) - by + by % 16)
        bname = "BLOCK_%dX%d" % (bw, bh)
        do_chroma = bool(has_chroma({}, TBO(BO(x=bx, y=by % 16)), BlockSize[bname], 1, 1, CS[(1, 1)]))
        _pname, uv_ts, bw_uv, bh_uv = chroma_of(bname, 1, 1, 1)
        uv_tt = int(c.call_method(TxType[types[j]], "uv_inter", [TxSize[uv_ts]]).disc) if eobs.any() else 0
        cb = 2 if bd == 8 else 4
        qs_uv, es_uv = chroma_blocks(uv_ts, uv_tt, bw_uv * bh_uv, cb, i % 3, False, False, i)
        above0, left0 = neighbours([(i + p) % 3 for p in range(3)])
        add("tx_tree " + key, bw, bh, ts, 1, 1, types[j], uv_tt, 1, 0, cb, 0, 0, do_chroma, geom, above0, left0,
            [qcs, qs_uv[0], qs_uv[1]], [eobs, es_uv[0], es_uv[1]],
            copy.deepcopy(fcs[40 if qidx <= 60 else (100 if qidx <= 120 else 200)]), (7, 0, 1)[picked % 3], i)
        picked += 1
    assert picked >= 4, picked

    out = {"case_rows": np.array(rows, np.int64), "case_names": np.array(names), "case_geom": np.array(geoms, np.int32),
           "case_qc": np.array(qc_all, np.int32), "case_eobs": np.stack(acc["eobs"]), "case_tell": np.stack(acc["tell"]),
           "case_cul": np.stack(acc["cul"]), "case_ctx_in": np.stack(acc["ctx_in"]), "case_ctx_out": np.stack(acc["ctx_out"]),
           "case_above": np.stack(acc["above"]), "case_left": np.stack(acc["left"]), "case_cdfs": np.stack(acc["cdfs"]),
           "sweep_rows": np.array(sweep, np.int32), "sweep_uv_intra": np.array(sweep_uv_intra, np.int32),
           "sweep_uv_inter": np.array(sweep_uv_inter, np.int32), "sweep_block_wh": np.array(sweep_block_wh, np.int32)}
    print("cases:", len(rows), flush=True)
    L.save("coeff_rate_block_ref.npz", out)


if __name__ == "__main__":
    main()

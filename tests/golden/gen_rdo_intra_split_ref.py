#!/usr/bin/env python3
"""tests/golden/rdo_intra_split_ref.npz: an INTRA block coded with transforms smaller than the block, computed by the
REFERENCE'S OWN SOURCE TEXT through tools/rustlite -- what rdo_tx_size_type's split depths (src/rdo.rs:725-802) make
write_tx_blocks do, and what r1_rdo_intra_split_batch computes in one launch.

  the loop of write_tx_blocks                     src/encoder.rs:2276-2311, STATED HERE (the function itself wants
                                                  get_qidx, has_chroma and the chroma half behind it): raster order
                                                  over the transform-block grid, the tile-grid test of line 2282,
                                                  qc.update once in front of it as at 2267
      encode_tx_block WHOLE, once per transform block, on ONE tile state: block k + 1 is predicted from the
      reconstruction block k left in ts.rec       src/encoder.rs:1404-1661 (need_recon_pixel = true)
          get_intra_edges -> has_top_right / has_bottom_left with the block's (bx, by)   src/partition.rs:639-898
          predict_intra, diff, forward_transform, quantize, dequantize, inverse_transform_add
  pass 1: RDOType::PixelDistRealRate, then compute_distortion(luma_only = true) (src/rdo.rs:254-347) for Tune::Psnr /
          Psychovisual, each without and with a DistortionScale grid
  pass 2: RDOType::TxDistEstRate with use_tx_domain_distortion: the transform-domain distortion per transform block

Stand-ins as in gen_rdo_intra_ref.py (get_func, CoeffRecorder, BitCounter, tile_state, frame_invariants).

Per case (row i of `cases`, named by `columns`): src_i (bh, bw) source block; nb_i the `rec` pixels the edges can reach
-- rows [nb_y, ..) x columns [nb_x, ..) of the plane, from one pixel left of / above the block to one transform
size right of / below it, clipped to the plane; per transform block k (raster index; a skipped one keeps zeros) tr_i /
bl_i = has_top_right / has_bottom_left as get_intra_edges would ask them, eob_i, qc_i, txd_i; rec_i the final (bh, bw)
block of ts.rec; dist_i (sse, cdef, sse scaled, cdef scaled) over the visible part; scales_i.
`sweep` (named by `sweep_columns`): the two availability answers (src/recon_intra.rs, executed) for every block size up
to 64x64, every transform size in scope, every transform block, at every aligned position of three superblocks of a
192x192 frame.

Run in the build container:  python tests/golden/gen_rdo_intra_split_ref.py
"""
import os

import numpy as np

import gen_fwd_tx_golden as FT
import reflib as L
from reflib import R
from gen_rdo_glue_ref import FILES, TX_W, TX_H, Obj, BitCounter, make_struct
from gen_rdo_pixel_ref import CoeffRecorder
from gen_rdo_intra_ref import MODES

FW = FH = 132          # a multiple of 4 (whole mode-info units), not of 8
PAD = 72
PLACES = ("origin", "row0", "col0", "inside", "right", "bottom")


def case_list():
    """(bd, bw, bh, ts, mode, angle_delta, place, enable_ief, neighbours, tx_type)"""
    cases = []
    k = 0

    def add(bd, bw, bh, ts, mode, delta, place=None, tx_type=None):
        nonlocal k
        tt = tx_type if tx_type is not None else ((0, 1, 9, 3)[k % 4] if TX_W[ts] <= 16 else 0)
        cases.append((bd, bw, bh, ts, mode, delta if 1 <= mode <= 8 else 0, place or PLACES[k % 6], (k // 2) % 3 != 2,
                      ("smooth", "plain")[(k + k // 6) % 2], tt))
        k += 1
    for mode in range(13):                                   # 8x8 / 4x4, every mode
        add(8, 8, 8, 0, mode, (-3, 0, 3)[mode % 3])
    for bd in (8, 10):                                       # 16x16: angles that use top-right and bottom-left
        for ts in (0, 1):
            for mode, delta in ((3, 0), (8, -3), (7, 3)):    # D45, D67 - 9, D203 + 9
                add(bd, 16, 16, ts, mode, delta)
    add(8, 16, 16, 1, 4, 3, "right")                         # last 8x8 column partly visible
    add(10, 16, 16, 0, 6, -3, "right")                       # last three 4x4 columns skipped
    add(8, 16, 16, 1, 12, 0, "bottom")
    add(8, 32, 32, 2, 3, 3, "inside")
    add(10, 32, 32, 2, 7, 0, "right")
    add(8, 32, 32, 1, 8, 0, "col0")
    add(10, 32, 32, 1, 9, 0, "bottom")
    add(10, 64, 64, 3, 5, -3, "origin")
    add(10, 64, 64, 3, 3, 0, "inside")
    add(10, 64, 64, 2, 7, 3, "row0")
    add(8, 16, 8, 1, 3, 0, "inside")
    add(8, 8, 16, 1, 7, 0, "inside")
    add(10, 16, 8, 0, 8, 3, "row0")
    add(8, 16, 4, 0, 4, 0, "col0")
    add(12, 16, 16, 1, 3, -3, "inside")
    return cases


def main():
    c = L.crate(*FILES)
    L.load_v_frame_types(c)
    ns, _ = FT.load_reference_1d()

    def get_func(_g, t):
        idx = t.disc if hasattr(t, "disc") else int(t)
        name, n = FT.TXFM[idx], FT.TXFM_LEN[idx]

        def run(coeffs):
            buf = FT.Buf(n)
            for i in range(n):
                buf[i] = FT.V(np.array([coeffs[i]], np.int32))
            ns[name](buf)
            for i in range(n):
                coeffs[i] = int(buf[i].v[0])
        return run
    c.define_py("get_func", get_func)

    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    BlockSize = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
    PM = [L.enum(c, "PredictionMode", n) for n in MODES]
    DS = L.struct(c, "DistortionScale")
    TileStateMut = L.struct(c, "TileStateMut")
    CBI = L.struct(c, "CodedBlockInfo")
    PSBO, SBO = L.struct(c, "PlaneSuperBlockOffset"), L.struct(c, "SuperBlockOffset")
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    PlaneOffset = R.PlaneOffset
    qc_default = c.get("default", owner="QuantizationContext")
    qc_update = c.get("update", owner="QuantizationContext")
    etb = c.get("encode_tx_block")
    cdist = c.get("compute_distortion")
    ief_new = c.get("new", owner="IntraEdgeFilterParameters")
    use_smooth = c.get("use_smooth_filter", owner="IntraEdgeFilterParameters")
    above_info = c.get("above_block_info", owner="TileStateMut")
    left_info = c.get("left_block_info", owner="TileStateMut")
    has_tr, has_bl = c.get("has_top_right"), c.get("has_bottom_left")
    RDO_PIX = L.enum(c, "RDOType", "PixelDistRealRate")
    RDO_TX = L.enum(c, "RDOType", "TxDistEstRate")
    INTRA_FRAME, NONE_FRAME = L.enum(c, "RefType", "INTRA_FRAME"), L.enum(c, "RefType", "NONE_FRAME")
    rng = np.random.default_rng(20261019)
    out = {}
    imp_w, imp_h = (FW + 7) // 8, (FH + 7) // 8
    mi_w, mi_h = (FW + 3) // 4, (FH + 3) // 4

    def tile_state(planes_in, planes_rec, qc, cbi):
        inp = Obj(planes=R.RSlice(planes_in))
        return make_struct(
            TileStateMut, sbo=PSBO(SBO(x=0, y=0)), sb_size_log2=6, sb_width=(FW + 63) // 64,
            sb_height=(FH + 63) // 64, mi_width=mi_w, mi_height=mi_h, width=FW, height=FH,
            input=inp, input_tile=Obj(planes=R.RSlice([p.as_region() for p in planes_in])),
            rec=Obj(planes=R.RSlice([p.as_region() for p in planes_rec])), qc=qc, coded_block_info=cbi)

    def frame_invariants(bd, qidx, tune, scales, enable_ief, tx_domain=False):
        cfd = R.NONE
        if scales is not None:
            cfd = R.Some(Obj(distortion_scales=R.RSlice([DS(int(v)) for v in scales.ravel()]), w_in_imp_b=imp_w,
                             h_in_imp_b=imp_h))
        return Obj(sequence=Obj(bit_depth=bd, enable_intra_edge_filter=enable_ief,
                                chroma_sampling=L.enum(c, "ChromaSampling", "Cs420")),
                   width=FW, height=FH, w_in_b=mi_w, h_in_b=mi_h,
                   use_tx_domain_distortion=tx_domain, base_q_idx=qidx,
                   dc_delta_q=R.RSlice([0, 0, 0]), ac_delta_q=R.RSlice([0, 0, 0]),
                   dist_scale=R.RSlice([DS(1 << 14)] * 3),
                   config=Obj(temporal_rdo=(lambda: scales is not None), tune=L.enum(c, "Tune", tune)),
                   coded_frame_data=cfd, cpu_feature_level=None, use_reduced_tx_set=False)

    # ---- the sweep: has_top_right / has_bottom_left for every (block size, transform size in scope, bx, by) at every
    # aligned block position of three superblocks of a 192x192 frame -- (0, 0): the frame's first row / column,
    # (1, 1): inside, (2, 2): against its right / bottom edge -- asked as get_intra_edges asks them
    SW = 192
    sweep = []
    for name in BlockSize:
        sw_, sh_ = (int(v) for v in name.split("_")[1].split("X"))
        if max(sw_, sh_) > 64:
            continue
        for ts_ in range(4):
            t_ = TX_W[ts_]
            if sw_ % t_ or sh_ % t_ or not 2 <= (sw_ // t_) * (sh_ // t_) <= 16:
                continue
            for sb in (0, 1, 2):
                for py in range(sb * 64, sb * 64 + 64, sh_):
                    for px in range(sb * 64, sb * 64 + 64, sw_):
                        pbo = TBO(BO(x=px >> 2, y=py >> 2))
                        for by_ in range(sh_ // t_):
                            for bx_ in range(sw_ // t_):
                                xk, yk, bx4, by4 = px + bx_ * t_, py + by_ * t_, bx_ * (t_ >> 2), by_ * (t_ >> 2)
                                a = has_tr({}, BlockSize[name], pbo, by4 != 0 or py > 0, xk + t_ < SW, TxSize[ts_], by4, bx4, 0, 0)
                                b = has_bl({}, BlockSize[name], pbo, yk + t_ < SW, bx4 != 0 or px > 0, TxSize[ts_], by4, bx4, 0, 0)
                                sweep.append((sw_, sh_, ts_, px, py, bx_, by_, int(bool(a)), int(bool(b))))
    out["sweep"] = np.array(sweep, np.uint8)
    out["sweep_columns"] = np.array(["bw", "bh", "ts", "x", "y", "bx", "by", "has_tr", "has_bl", "frame=192"])
    print("sweep:", len(sweep), "questions", flush=True)

    cases = case_list()
    limit = int(os.environ.get("R1_INTRA_CASES", "0"))
    if limit:
        cases = cases[::max(1, len(cases) // limit)]
    rows = []
    for ci, (bd, bw, bh, ts, mode, delta, place, enable_ief, nbk, tx_type) in enumerate(cases):
        g = dict(L.pixel_type(bd), W="BitCounter")
        g1 = L.pixel_type(bd)
        dt = L.np_dtype(bd)
        mx = (1 << bd) - 1
        t = TX_W[ts]
        gw, gh = bw // t, bh // t
        ntx = gw * gh
        # the block's place in the plane, on the block grid
        gx, gy = (FW + bw - 1) // bw, (FH + bh - 1) // bh
        x, y = {"origin": (0, 0), "row0": (min(2, gx - 1) * bw, 0), "col0": (0, min(2, gy - 1) * bh),
                "inside": (min(1, gx - 2) * bw, min(1, gy - 2) * bh), "right": ((gx - 1) * bw, min(1, gy - 1) * bh),
                "bottom": (min(1, gx - 1) * bw, (gy - 1) * bh)}[place]
        qidx = (40, 100, 180)[ci % 3]
        yy, xx = np.mgrid[0:FH + 2 * PAD, 0:FW + 2 * PAD]
        rec0 = mx * (0.5 + 0.3 * np.sin(xx / (3.0 + ci % 7)) * np.cos(yy / (2.0 + ci % 5))) + \
            rng.integers(-(12 << (bd - 8)), (12 << (bd - 8)) + 1, xx.shape)
        rec0 = np.clip(rec0, 0, mx)
        amp = (4, 10, 28)[ci % 3] << (bd - 8)
        src0 = np.clip(rec0 + rng.integers(-amp, amp + 1, xx.shape), 0, mx)
        rec0, src0 = rec0.astype(dt), src0.astype(dt)
        scales = rng.integers(1 << 12, 1 << 16, (imp_h, imp_w)).astype(np.uint32)

        refs = R.array(INTRA_FRAME, NONE_FRAME)
        plain = CBI(luma_mode=R.Some(PM[0]), chroma_mode=R.Some(PM[0]), reference_types=refs)
        smooth = CBI(luma_mode=R.Some(PM[9 + ci % 3]), chroma_mode=R.Some(PM[9 + ci % 3]), reference_types=refs)
        grid = [[plain] * mi_w for _ in range(mi_h)]
        bo_x, bo_y = x >> 2, y >> 2
        if nbk == "smooth":
            if bo_y > 0:
                grid[bo_y - 1][bo_x] = smooth
            elif bo_x > 0:
                grid[bo_y][bo_x - 1] = smooth
        cbi = R.RSlice([R.RSlice(r) for r in grid])
        bsize = BlockSize["BLOCK_%dX%d" % (bw, bh)]
        bo = TBO(BO(x=bo_x, y=bo_y))
        # write_tx_blocks hands every transform block IntraParam::AngleDelta(angle_delta.y)
        iparam = c.G["_E"]("IntraParam", "AngleDelta", 0, (delta,))
        acs = R.RSlice([])

        def planes(arr):
            return [L.plane_from_padded(arr, bd, PAD, PAD, 0, 0)]

        def block(pl):
            cfg = pl.cfg
            o = np.zeros((bh, bw), dt)
            for r in range(bh):
                base = (cfg.yorigin + y + r) * cfg.stride + cfg.xorigin + x
                o[r] = pl.data[base:base + bw]
            return o

        def run_blocks(rdo, fi):
            """the loop of write_tx_blocks (encoder.rs:2267-2311) for the luma plane"""
            p_in, p_rec = planes(src0), planes(rec0)
            qc = qc_default({})
            qc_update({}, qc, qidx, TxSize[ts], True, bd, 0, 0)
            tsm = tile_state(p_in, p_rec, qc, cbi)
            wr, cw = BitCounter(), CoeffRecorder()
            per = {}
            for by in range(gh):
                for bx in range(gw):
                    tbx, tby = bo_x + bx * (t >> 2), bo_y + by * (t >> 2)
                    if tbx >= mi_w or tby >= mi_h:
                        continue
                    n_calls = len(cw.calls)
                    res = etb(g, fi, tsm, cw, wr, 0, bo, bx, by, TBO(BO(x=tbx, y=tby)), PM[mode], TxSize[ts],
                              TxType[tx_type], bsize, PlaneOffset(x=tbx * 4, y=tby * 4), False, qidx, acs, iparam, rdo,
                              True)
                    assert len(cw.calls) == n_calls + 1
                    per[by * gw + bx] = (res, cw.calls[-1])
            return per, tsm, p_rec[0]

        # has_top_right / has_bottom_left as get_intra_edges asks them for transform block (bx, by)
        tr, bl = np.zeros(ntx, np.uint8), np.zeros(ntx, np.uint8)
        for by in range(gh):
            for bx in range(gw):
                xk, yk = x + bx * t, y + by * t
                if (xk >> 2) >= mi_w or (yk >> 2) >= mi_h:
                    continue
                bx4, by4 = bx * (t >> 2), by * (t >> 2)
                have_top, have_left = by4 != 0 or bo_y > 0, bx4 != 0 or bo_x > 0
                tr[by * gw + bx] = bool(has_tr({}, bsize, bo, have_top, xk + t < FW, TxSize[ts], by4, bx4, 0, 0))
                bl[by * gw + bx] = bool(has_bl({}, bsize, bo, yk + t < FH, have_left, TxSize[ts], by4, bx4, 0, 0))
        ief = 0
        if 1 <= mode <= 8 and enable_ief:
            ts0 = tile_state(planes(src0), planes(rec0), qc_default({}), cbi)
            prm = ief_new({}, 0, above_info(g1, ts0, bo, 0, 0), left_info(g1, ts0, bo, 0, 0))
            ief = 2 if use_smooth({}, prm) else 1
        # pass 1: the pixel-domain leg
        fi0 = frame_invariants(bd, qidx, "Psnr", None, enable_ief)
        per, tsm, prp = run_blocks(RDO_PIX, fi0)
        eobs, qcs = np.zeros(ntx, np.int32), np.zeros((ntx, t * t), np.int32)
        for k, ((has_coeff, d0), (qcf, eob, _, _)) in per.items():
            assert d0._0 == 0
            eobs[k], qcs[k] = int(eob), np.array(qcf, np.int32)
        rec_blk = block(prp)
        dists = []
        for (tune, sc) in (("Psnr", None), ("Psychovisual", None), ("Psnr", scales), ("Psychovisual", scales)):
            fi = frame_invariants(bd, qidx, tune, sc, enable_ief)
            dists.append(cdist(g1, fi, tsm, bsize, False, bo, True)._0)
        # pass 2: the transform-domain distortion per transform block (same reconstruction)
        fit = frame_invariants(bd, qidx, "Psnr", None, enable_ief, tx_domain=True)
        per2, _, prp2 = run_blocks(RDO_TX, fit)
        assert np.array_equal(block(prp2), rec_blk)
        txd = np.zeros(ntx, np.uint64)
        for k, ((_, d), (qcf, eob, _, _)) in per2.items():
            assert int(eob) == eobs[k]
            txd[k] = d._0
        i = len(rows)
        nx0, ny0 = max(x - 1, 0), max(y - 1, 0)
        nx1, ny1 = min(x + bw + t, FW), min(y + bh + t, FH)
        out["src_%d" % i] = block(planes(src0)[0])
        out["nb_%d" % i] = rec0[PAD + ny0:PAD + ny1, PAD + nx0:PAD + nx1]
        out["tr_%d" % i], out["bl_%d" % i] = tr, bl
        out["eob_%d" % i], out["txd_%d" % i] = eobs.astype(np.uint16), txd
        out["qc_%d" % i] = qcs if bd > 8 else qcs.astype(np.int16)
        out["rec_%d" % i] = rec_blk
        out["dist_%d" % i] = np.array(dists, np.uint64)
        out["scales_%d" % i] = scales
        rows.append((bd, bw, bh, ts, mode, delta, int(enable_ief), ief, x, y, nx0, ny0, FW, FH, tx_type, qidx, len(per)))
        print(ci, "/", len(cases), (bd, bw, bh, ts, MODES[mode], delta, place, enable_ief, nbk, tx_type), "ief", ief,
              "tr", tr.tolist(), "bl", bl.tolist(), "eob", eobs.tolist(), dists, txd.tolist(), flush=True)
    out["cases"] = np.array(rows, np.int64)
    out["columns"] = np.array(["bd", "bw", "bh", "ts", "mode", "angle_delta", "enable_ief", "ief", "x", "y", "nb_x", "nb_y",
                               "plane_w", "plane_h", "tx_type", "qidx", "coded"])
    L.save(os.environ.get("R1_SPLIT_OUT", "rdo_intra_split_ref.npz"), out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tests/golden/rdo_intra_ref.npz: encode_tx_block with INTRA prediction modes, computed by the REFERENCE'S OWN
SOURCE TEXT through tools/rustlite.  The other RDO fixtures (gen_rdo_pixel_ref.py, gen_rdo_txsearch_ref.py) pass
NEWMV with the prediction already in `rec`; here every run enters the function in front of the transform:

  encode_tx_block WHOLE                           src/encoder.rs:1404-1661
      ts.above_block_info / ts.left_block_info    src/tiling/tile_state.rs:229-264 (executed: they index a
                                                  coded_block_info grid that holds the recorded neighbour info)
      IntraEdgeFilterParameters::new              src/predict.rs:543-569
      get_intra_edges(.., Some(mode), ..)         src/partition.rs:639-898
      PredictionMode::predict_intra -> dispatch_predict_intra and its kernels   src/predict.rs:205-249, 705-1505
      diff -> forward_transform -> quantize -> dequantize -> inverse_transform_add into ts.rec
  pass 1: RDOType::PixelDistRealRate, then compute_distortion (src/rdo.rs:254-347) for Tune::Psnr / Psychovisual,
          each without and with a DistortionScale grid (rec does not depend on the tune: one encode_tx_block run)
  pass 2: RDOType::TxDistEstRate: the transform-domain distortion the function returns

and, per case, the QUESTION r1_rdo_intra_cand_batch's edge_group rests on: is an edge set built with no mode and
IntraParam::None (what the intra pre-screen shares among the modes of a block) interchangeable with the
Some(mode) set inside this chain?  Both sets are built, both predictions are made by predict_intra, and
`shared_ok` records whether they are equal.

Stand-ins (as in gen_rdo_pixel_ref.py): get_func, the ContextWriter recorder, v_frame's ChromaSampling;
FrameInvariants / Sequence / TileStateMut field values are plain data.  Chroma cases (4:2:0 plane, 8x8) carry no
pixel-domain distortions: compute_distortion with luma_only = false wants all three planes of a coded partition.

Per case (row i of `cases`, named by `columns`): src_i (h, w) source block; the `rec` neighbourhood get_intra_edges
can reach, clipped to the plane: nbt_i = row y - 1, columns [nb_x, x + w + h) (absent when y = 0) and nbl_i = column
x - 1, rows [nb_y, y + h + w) (absent when x = 0); edge_i (257 entries, 0xFFFF where the function wrote nothing) with
left_len / above_len; pred_i, rec_i, qc_i, eob; dist_i (sse, cdef, sse scaled, cdef scaled); txd_i the
transform-domain distortion; scales_i the DistortionScale grid; ac_i (CFL).

Run in the build container:  python tests/golden/gen_rdo_intra_ref.py
"""
import os

import numpy as np

import gen_fwd_tx_golden as FT
import reflib as L
from reflib import R
from gen_rdo_glue_ref import FILES, TX_W, TX_H, Obj, BitCounter, make_struct
from gen_rdo_pixel_ref import CoeffRecorder

MODES = ["DC_PRED", "V_PRED", "H_PRED", "D45_PRED", "D135_PRED", "D113_PRED", "D157_PRED", "D203_PRED",
         "D67_PRED", "SMOOTH_PRED", "SMOOTH_V_PRED", "SMOOTH_H_PRED", "PAETH_PRED", "UV_CFL_PRED"]
FW = FH = 132          # a multiple of 4 (whole mode-info units), not of 8
PAD = 72


def case_list():
    """(bd, ts, mode, angle_delta, place, enable_ief, neighbours, chroma, alpha): the smallest set that reaches every
    branch -- all 13 luma modes with deltas -3 / 0 / +3 on 8-bit 8x8, a rotating subset elsewhere"""
    places = ("origin", "row0", "col0", "inside", "right", "bottom")
    cases = []
    k = 0

    def add(bd, ts, mode, delta, chroma=False, alpha=0):
        nonlocal k
        cases.append((bd, ts, mode, delta, places[k % 6], (k // 2) % 3 != 2, ("smooth", "plain")[(k + k // 6) % 2],
                      chroma, alpha))
        k += 1
    for mode in range(13):
        for delta in ((-3, 0, 3) if 1 <= mode <= 8 else (0,)):
            add(8, 1, mode, delta)
    for mode in (0, 1, 3, 4, 6, 7, 8, 9, 11, 12):
        add(10, 1, mode, (0, -3, 3)[mode % 3] if 1 <= mode <= 8 else 0)
    for mode in (2, 3, 5, 7, 10, 12):
        add(12, 1, mode, (3, 0, -3)[mode % 3] if 1 <= mode <= 8 else 0)
    rot = 0
    for ts in (0, 2, 13, 14, 3, 4, 18):
        for bd in (8, 10):
            for j in range(7):
                mode = (0, 3, 4, 5, 7, 8, 6, 1, 2, 9, 10, 11, 12)[(rot + 2 * j) % 13]
                add(bd, ts, mode, (0, 3, -3)[(rot + j) % 3] if 1 <= mode <= 8 else 0)
            rot += 3
    for bd in (8, 10):
        add(bd, 1, 13, 0, True, -7 if bd == 8 else 11)
        add(bd, 1, 0, 0, True)
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
    IEF = L.struct(c, "IntraEdgeFilterParameters")
    PSBO, SBO = L.struct(c, "PlaneSuperBlockOffset"), L.struct(c, "SuperBlockOffset")
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    PlaneOffset = R.PlaneOffset
    qc_default = c.get("default", owner="QuantizationContext")
    qc_update = c.get("update", owner="QuantizationContext")
    etb = c.get("encode_tx_block")
    cdist = c.get("compute_distortion")
    get_edges = c.get("get_intra_edges")
    predict_intra = c.get("predict_intra", owner="PredictionMode")
    ief_new = c.get("new", owner="IntraEdgeFilterParameters")
    use_smooth = c.get("use_smooth_filter", owner="IntraEdgeFilterParameters")
    above_info = c.get("above_block_info", owner="TileStateMut")
    left_info = c.get("left_block_info", owner="TileStateMut")
    has_tr, has_bl = c.get("has_top_right"), c.get("has_bottom_left")
    supersample = c.get("supersample_chroma_bsize")
    RDO_PIX = L.enum(c, "RDOType", "PixelDistRealRate")
    RDO_TX = L.enum(c, "RDOType", "TxDistEstRate")
    IP_NONE = L.enum(c, "IntraParam", "None")
    INTRA_FRAME, NONE_FRAME = L.enum(c, "RefType", "INTRA_FRAME"), L.enum(c, "RefType", "NONE_FRAME")
    rng = np.random.default_rng(20261018)
    out = {}
    imp_w, imp_h = (FW + 7) // 8, (FH + 7) // 8

    def tile_state(planes_in, planes_rec, qc, cbi):
        inp = Obj(planes=R.RSlice(planes_in))
        return make_struct(
            TileStateMut, sbo=PSBO(SBO(x=0, y=0)), sb_size_log2=6, sb_width=(FW + 63) // 64,
            sb_height=(FH + 63) // 64, mi_width=(FW + 3) // 4, mi_height=(FH + 3) // 4, width=FW, height=FH,
            input=inp, input_tile=Obj(planes=R.RSlice([p.as_region() for p in planes_in])),
            rec=Obj(planes=R.RSlice([p.as_region() for p in planes_rec])), qc=qc, coded_block_info=cbi)

    def frame_invariants(bd, qidx, tune, scales, enable_ief, tx_domain=False):
        cfd = R.NONE
        if scales is not None:
            cfd = R.Some(Obj(distortion_scales=R.RSlice([DS(int(v)) for v in scales.ravel()]), w_in_imp_b=imp_w,
                             h_in_imp_b=imp_h))
        return Obj(sequence=Obj(bit_depth=bd, enable_intra_edge_filter=enable_ief,
                                chroma_sampling=L.enum(c, "ChromaSampling", "Cs420")),
                   width=FW, height=FH, w_in_b=(FW + 3) // 4, h_in_b=(FH + 3) // 4,
                   use_tx_domain_distortion=tx_domain, base_q_idx=qidx,
                   dc_delta_q=R.RSlice([0, 0, 0]), ac_delta_q=R.RSlice([0, 0, 0]),
                   dist_scale=R.RSlice([DS(1 << 14)] * 3),
                   config=Obj(temporal_rdo=(lambda: scales is not None), tune=L.enum(c, "Tune", tune)),
                   coded_frame_data=cfd, cpu_feature_level=None, use_reduced_tx_set=False)

    cases = case_list()
    limit = int(os.environ.get("R1_INTRA_CASES", "0"))
    if limit:
        cases = cases[::max(1, len(cases) // limit)]
    rows = []
    for ci, (bd, ts, mode, delta, place, enable_ief, nbk, chroma, alpha) in enumerate(cases):
        g = dict(L.pixel_type(bd), W="BitCounter")
        g1 = L.pixel_type(bd)
        dt = L.np_dtype(bd)
        mx = (1 << bd) - 1
        w, h = TX_W[ts], TX_H[ts]
        xdec = ydec = 1 if chroma else 0
        if chroma and place in ("right", "bottom"):
            place = "inside"          # (a 4:2:0 plane of a frame that is no multiple of 8 has no whole 8x8 block there)
        pw, ph = FW >> xdec, FH >> ydec                   # the plane the block lies in
        # the block's place in its plane, on the block grid
        gx, gy = (pw + w - 1) // w, (ph + h - 1) // h
        x, y = {"origin": (0, 0), "row0": (min(2, gx - 1) * w, 0), "col0": (0, min(2, gy - 1) * h),
                "inside": (min(1, gx - 2) * w, min(1, gy - 2) * h), "right": ((gx - 1) * w, min(1, gy - 1) * h),
                "bottom": (min(1, gx - 1) * w, (gy - 1) * h)}[place]
        qidx = (40, 100, 180)[ci % 3]
        # smooth-ish reconstructed plane with texture (real pixels in the padding too); source = rec + noise
        yy, xx = np.mgrid[0:ph + 2 * PAD, 0:pw + 2 * PAD]
        rec0 = mx * (0.5 + 0.3 * np.sin(xx / (3.0 + ci % 7)) * np.cos(yy / (2.0 + ci % 5))) + \
            rng.integers(-(12 << (bd - 8)), (12 << (bd - 8)) + 1, xx.shape)
        rec0 = np.clip(rec0, 0, mx)
        amp = (4, 10, 28)[ci % 3] << (bd - 8)
        src0 = np.clip(rec0 + rng.integers(-amp, amp + 1, xx.shape), 0, mx)
        rec0, src0 = rec0.astype(dt), src0.astype(dt)
        scales = rng.integers(1 << 12, 1 << 16, (imp_h, imp_w)).astype(np.uint32)

        # the neighbours' block info (luma mode-info units): a smooth and a non-smooth neighbour occur
        refs = R.array(INTRA_FRAME, NONE_FRAME)
        # (the modes are stored as Some(mode): IntraEdgeFilterParameters::new turns them into options with `.into()`,
        # which the transpiler passes through unchanged)
        plain = CBI(luma_mode=R.Some(PM[0]), chroma_mode=R.Some(PM[0]), reference_types=refs)
        smooth = CBI(luma_mode=R.Some(PM[9 + ci % 3]), chroma_mode=R.Some(PM[9 + ci % 3]), reference_types=refs)
        mi_w, mi_h = (FW + 3) // 4, (FH + 3) // 4
        grid = [[plain] * mi_w for _ in range(mi_h)]
        bo_x, bo_y = (x << xdec) >> 2, (y << ydec) >> 2
        if chroma:
            bo_x, bo_y = bo_x | 1, bo_y | 1                # the odd luma block carries the chroma of a 4:2:0 8x8
        if nbk == "smooth":
            if bo_y > 0:
                grid[bo_y - 1][bo_x] = smooth
            elif bo_x > 0:
                grid[bo_y][bo_x - 1] = smooth
        cbi = R.RSlice([R.RSlice(r) for r in grid])
        bsize = BlockSize["BLOCK_%dX%d" % (w << xdec, h << ydec)]
        bo = TBO(BO(x=bo_x, y=bo_y))
        tx_bo = TBO(BO(x=(x << xdec) >> 2, y=(y << ydec) >> 2))
        iparam = c.G["_E"]("IntraParam", "AngleDelta", 0, (delta,)) if delta else \
            (c.G["_E"]("IntraParam", "Alpha", 0, (alpha,)) if mode == 13 else IP_NONE)
        acv = None
        if mode == 13:
            acv = rng.integers(-(1 << (bd + 1)), 1 << (bd + 1), w * h).astype(np.int16)
            acv -= np.int16(acv.astype(np.int64).sum() // (w * h))
        acs = R.RSlice([int(v) for v in acv]) if acv is not None else R.RSlice([])
        p = 1 if chroma else 0

        def planes(arr):
            """[luma, chroma] planes (p = 1) or [luma] with `arr` as plane p"""
            pl = L.plane_from_padded(arr, bd, PAD, PAD, xdec, ydec)
            if not chroma:
                return [pl]
            return [L.plane_from_array(np.zeros((FH, FW), dt), bd, PAD, PAD), pl]

        def block(pl):
            cfg = pl.cfg
            o = np.zeros((h, w), dt)
            for r in range(h):
                base = (cfg.yorigin + y + r) * cfg.stride + cfg.xorigin + x
                o[r] = pl.data[base:base + w]
            return o

        def run_etb(rdo, skip, fi):
            p_in, p_rec = planes(src0), planes(rec0)
            qc = qc_default({})
            qc_update({}, qc, qidx, TxSize[ts], True, bd, 0, 0)      # as write_tx_blocks does for an intra luma mode
            tsm = tile_state(p_in, p_rec, qc, cbi)
            wr, cw = BitCounter(), CoeffRecorder()
            res = etb(g, fi, tsm, cw, wr, p, bo, 0, 0, tx_bo, PM[mode], TxSize[ts], TxType[0], bsize,
                      PlaneOffset(x=x, y=y), skip, qidx, acs, iparam, rdo, False)
            return res, tsm, p_rec[p], cw, wr

        fi0 = frame_invariants(bd, qidx, "Psnr", None, enable_ief)
        # (a) the prediction the function makes: skip = true leaves right behind predict_intra
        _, _, prp, _, _ = run_etb(RDO_PIX, True, fi0)
        pred_some = block(prp)
        # (b) the edge buffer it built, the availability answers it got, and the pre-screen's shared set
        rec_pl = planes(rec0)[p]
        region = rec_pl.as_region()

        def edges_of(opt_mode, ip):
            buf = R.Aligned(R.RSlice([0xFFFF] * 257))
            e = get_edges(g1, buf, region, bo, 0, 0, bsize, PlaneOffset(x=x, y=y), TxSize[ts], bd, opt_mode,
                          bool(enable_ief), ip)
            full = np.full(257, 0xFFFF, np.uint16)
            full[128 - e._0.len():128] = e._0.tolist()
            full[128] = e._1.tolist()[0]
            full[129:129 + e._2.len()] = e._2.tolist()
            return e, full, (e._0.len(), e._2.len())
        e_some, edge_full, lens = edges_of(R.Some(PM[mode]), iparam)
        e_none, _, _ = edges_of(R.NONE, IP_NONE)
        is_dir = 1 <= mode <= 8
        ief_p = R.NONE
        ief = 0
        if is_dir and enable_ief:
            pxd, pyd = (0, 0) if p == 0 else (xdec, ydec)
            ts0 = tile_state(planes(src0), planes(rec0), qc_default({}), cbi)
            prm = ief_new({}, p, above_info(g1, ts0, bo, pxd, pyd), left_info(g1, ts0, bo, pxd, pyd))
            ief_p = R.Some(prm)
            ief = 2 if use_smooth({}, prm) else 1
        tile_rect = Obj(x=0, y=0, width=pw, height=ph)
        sc_pl = planes(rec0)[p]
        sreg = sc_pl._region(x, y, w, h)
        predict_intra(g1, PM[mode], tile_rect, sreg, TxSize[ts], bd, acs, iparam, ief_p, e_none, None)
        pred_none = block(sc_pl)
        sc_pl2 = planes(rec0)[p]
        predict_intra(g1, PM[mode], tile_rect, sc_pl2._region(x, y, w, h), TxSize[ts], bd, acs, iparam, ief_p,
                      e_some, None)
        assert np.array_equal(block(sc_pl2), pred_some)          # the direct call reproduces the function's own
        shared_ok = bool(np.array_equal(pred_none, pred_some))
        rect_w, rect_h = pw, ph
        sps = supersample({}, bsize, xdec, ydec)
        have_top = bo_y > (1 if ydec else 0)
        have_left = bo_x > (1 if xdec else 0)
        tr = bool(y != 0 and has_tr({}, sps, bo, have_top, x + w < rect_w, TxSize[ts], 0, 0, xdec, ydec))
        bl = bool(x != 0 and has_bl({}, sps, bo, y + h < rect_h, have_left, TxSize[ts], 0, 0, xdec, ydec))
        # pass 1: the pixel-domain leg
        (has_coeff, d0), tsm, prp, cw, wr = run_etb(RDO_PIX, False, fi0)
        assert d0._0 == 0 and len(cw.calls) == 1 and not wr.bits
        qcf, eob, _, _ = cw.calls[0]
        rec_blk = block(prp)
        dists = [0, 0, 0, 0]
        if not chroma:
            dists = []
            for (tune, sc) in (("Psnr", None), ("Psychovisual", None), ("Psnr", scales), ("Psychovisual", scales)):
                fi = frame_invariants(bd, qidx, tune, sc, enable_ief)
                dists.append(cdist(g1, fi, tsm, bsize, False, bo, True)._0)
        # pass 2: the transform-domain distortion
        fit = frame_invariants(bd, qidx, "Psnr", None, enable_ief, tx_domain=True)
        (_, dt_), _, prp2, cw2, wr2 = run_etb(RDO_TX, False, fit)
        assert not cw2.calls and len(wr2.bits) == 1              # the rate is estimated, nothing is coded
        i = len(rows)
        nx0, ny0 = max(x - 1, 0), max(y - 1, 0)
        nx1, ny1 = min(x + w + h, pw), min(y + h + w, ph)
        out["src_%d" % i] = block(planes(src0)[p])
        if y > 0:
            out["nbt_%d" % i] = rec0[PAD + y - 1, PAD + nx0:PAD + nx1]
        if x > 0:
            out["nbl_%d" % i] = rec0[PAD + ny0:PAD + ny1, PAD + x - 1]
        out["edge_%d" % i] = edge_full.astype(dt) if bd > 8 else edge_full.astype(np.uint16)
        out["pred_%d" % i] = pred_some
        out["rec_%d" % i] = rec_blk
        out["qc_%d" % i] = np.array(qcf, np.int32)
        out["scales_%d" % i] = scales
        if acv is not None:
            out["ac_%d" % i] = acv
        rows.append((bd, ts, mode, delta, alpha, int(enable_ief), ief, x, y, nx0, ny0, pw, ph, xdec, int(tr), int(bl),
                     lens[0], lens[1], qidx, int(eob), int(shared_ok), int(has_coeff is True)))
        out["dist_%d" % i] = np.array(dists, np.uint64)
        out["txd_%d" % i] = np.array([dt_._0], np.uint64)
        print(ci, "/", len(cases), (bd, ts, mode, delta, place, enable_ief, nbk), "ief", ief, "eob", eob,
              "shared_ok", shared_ok, dists, dt_._0, flush=True)
    out["cases"] = np.array(rows, np.int64)
    out["columns"] = np.array(["bd", "ts", "mode", "angle_delta", "alpha", "enable_ief", "ief", "x", "y", "nb_x",
                               "nb_y", "plane_w", "plane_h", "dec", "has_tr", "has_bl", "left_len", "above_len",
                               "qidx", "eob", "shared_ok", "has_coeff"])
    bad = [r for r in rows if not r[20]]
    print("intra encode_tx_block:", len(rows), "cases;", len(bad), "where the shared (no-mode) edge set predicts "
          "differently:", sorted({(TX_W[r[1]], TX_H[r[1]], MODES[r[2]], r[3], r[5]) for r in bad}))
    L.save("rdo_intra_ref.npz", out)


if __name__ == "__main__":
    main()

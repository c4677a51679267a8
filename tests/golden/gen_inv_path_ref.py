#!/usr/bin/env python3
"""tests/golden/inv_path_ref.npz (+ inv_path_ref_dq.npz): the pixel-domain chain behind the quantizer
(dequantize -> inverse_transform_add -> add -> pixel clamp) computed by the REFERENCE'S OWN SOURCE TEXT, on the
residual blocks of fwd_tx_ref.npz -- blocks built to reach the limits of the narrow arithmetic.

  encode_tx_block, RDOType::PixelDistRealRate, fi.use_tx_domain_distortion = false   src/encoder.rs:1404-1661
      executed WHOLE as in gen_rdo_pixel_ref.py (diff -> forward_transform -> QuantizationContext::quantize ->
      [write_coeffs_lv_map: the recording stand-in] -> dequantize -> inverse_transform_add into ts.rec), the crate
      transpiled with strict=True: every arithmetic result and `let` is range-checked like a debug build.
Nothing is imported from oracle/ or tests/*_util.py.

Families
  plain  pred = max(-res, 0), src = max(res, 0): the residual is the block itself (leg 2 of the forward test).
         NEWMV, quantizer offsets of an inter block.  Every (tx_size, tx_type) of the inter set of the size
         (get_tx_set(size, is_inter = true, reduced = false) executed, av1_tx_used read), bit depths 8 / 10 / 12,
         qindex 1 (the smallest lossy index: the largest levels) and 255 (the largest steps).  Up to area 256 the
         blocks sign, rand, checker, small, impulse of fwd_tx_ref.npz; above, sign, rand, impulse.  At 8x8 of every
         bit depth the same cases once more with the quantizer offsets of an intra block (is_intra = 1).
  flat   pred == 2^(bd-1) as DC_PRED makes it from a plane of mid-grey (encode_tx_block predicts: an intra block with
         both edges), src = pred + (res >> 1), which lies in [-2^(bd-1), 2^(bd-1) - 1]; intra quantizer offsets;
         the types of the intra set at 8x8, 16x16, 32x32, 16x32 (the three routes of an intra candidate call);
         blocks sign, rand, impulse.
  split  executed as gen_rdo_intra_split_ref.py does it: the loop of write_tx_blocks (src/encoder.rs:2276-2311)
         stated here, encode_tx_block whole once per transform block on ONE tile state, block k + 1 predicted from
         what block k left in ts.rec.  8x8/4x4, 16x16/8x8, 32x32/16x16, 64x64/32x32 at each bit depth and both
         qindex; the block at (64, 64) of a mid-grey plane; the source of transform block k is mid-grey plus
         (k even) or minus (k odd) the sign block of the case's type at half amplitude, clipped to the pixel range;
         DC / V / H / Paeth in turn, no edge filter; the type moves through the intra set of the transform size.

Observed from the executed run, per block (nothing of it is restated here):
  * clamp_value (src/transform/mod.rs:311) is wrapped in a shim that calls the transpiled function and counts the
    calls whose result differs from the argument, split by the `bit` argument AND by pass.  The pass is observed as
    well: inside inverse_transform_add the first round_shift with a shift below 3 is the column pass's
    INV_INTERMEDIATE_SHIFTS one (:1690); the row pass and the networks only ever shift by 12.  At 8 bits both passes
    clamp to 16 bits, so `bit` alone could not tell them apart.  A count covers the driver's clamp and the clamps
    inside the 1-D network of that pass.
  * pixels where the final clamp(v + r, 0, max) (:1701) changed its argument.
  * dequantize's rcoeffs as it left them, and whether T::cast_from changed a value: the same call once more at
    T = i32, compared.
  * strict mode: a block on which a range check trips is not dropped; its amplitude is halved (res -> trunc(res / 2))
    until it runs, and the number of halvings is stored.

Layout (few large arrays).  One row of `blocks` per executed block, in order:
  blocks  (n, 14) int32, named by `columns`: family, bd, tx_size, tx_type, qindex, is_intra, block (index into
          `names`), halvings, eob, cast_changed, row_clamps, col_clamps, pix_clamps, strict_trips
  qc_<bd>   quantized coefficients as handed to write_coeffs_lv_map, first min(w,32) * min(h,32) of each block
  rms_<bd>  reconstruction minus source, (h * w) per block, int16 (the source is the block's definition above)
  split   (24, 12) int32, named by `split_columns`; split_tx (96, 7) int32, named by `split_tx_columns`: one row per
          transform block in call order (case, raster index, eob, cast_changed, the three clamp counts)
  split_src_<bd>, split_rms_<bd>  the (bs * bs) source block and reconstruction minus source of each case
  split_qc_<bd>                   (t * t) levels per transform block
  inv_path_ref_dq.npz: dq_<bd> and split_dq_<bd>, rcoeffs as dequantize wrote them, same extent as the levels
  (T::Coeff: int16 at 8 bits).  A second file because no file of this repository may exceed 1 MiB.
R1_INV_PATH_SIZES=0,5 limits a run to those tx sizes of the families (a quick look, never the committed file).

Run in the build container:  python tests/golden/gen_inv_path_ref.py        (20 s on 8 cores)
"""
import multiprocessing
import os
import sys

import numpy as np

import gen_fwd_tx_golden as FT
import reflib as L
from reflib import R
from gen_rdo_glue_ref import FILES, TX_W, TX_H, Obj, BitCounter, make_struct
from gen_rdo_pixel_ref import CoeffRecorder
from gen_rdo_intra_ref import MODES

NAMES = ["sign", "rand", "const+", "const-", "checker", "rows", "cols", "small", "impulse", "zero"]
SMALL_BLOCKS = (0, 1, 4, 7, 8)
BIG_BLOCKS = (0, 1, 8)
QINDEX = (1, 255)
FLAT_SIZES = (1, 2, 3, 9)
INTRA_OFFSET_SIZE = 1
COLUMNS = ["family", "bd", "tx_size", "tx_type", "qindex", "is_intra", "block", "halvings", "eob", "cast_changed",
           "row_clamps", "col_clamps", "pix_clamps", "strict_trips"]
FW = FH = 128
BX, BY = 8, 4               # the block's place in mode-info units: (32, 16) px


def fwd_blocks():
    """{(bd, ts, tt): {block name index: (h, w) int64}} read back from fwd_tx_ref.npz (its layout: gen_fwd_tx_ref.py)"""
    G = np.load(os.path.join(L.HERE, "fwd_tx_ref.npz"))
    assert [str(s) for s in G["blocks"]] == NAMES
    out, pos, seen = {}, {}, {}
    for bd, ts, tt, nb, w, h in (tuple(int(v) for v in r) for r in G["cases"]):
        p = pos.setdefault(bd, [0, 0])
        if (bd, ts) not in seen:
            n = (nb - 1) * w * h
            seen[bd, ts] = G["shared_%d" % bd][p[0]:p[0] + n].reshape(nb - 1, h, w).astype(np.int64)
            p[0] += n
        sg = G["sign_%d" % bd][p[1]:p[1] + w * h].reshape(h, w).astype(np.int64)
        p[1] += w * h
        d = {0: sg}
        for i, b in enumerate(seen[bd, ts]):
            d[i + 1] = b
        imp = np.zeros((h, w), np.int64)        # gen_fwd_tx_ref.shared_blocks: not stored above area 1024
        imp[h - 1, w - 1] = -((1 << bd) - 1)
        assert 8 not in d or np.array_equal(d[8], imp)
        d[8] = imp
        out[bd, ts, tt] = d
    return out


class World:
    """the transpiled crate with the counting shims in place"""

    def __init__(self):
        c = self.c = L.crate(*FILES, strict=True)
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

        # ---- the shims.  Each calls what it wraps and only looks at the arguments and the result.
        self.inside = False         # inside inverse_transform_add
        self.col = False            # ... and past the first INV_INTERMEDIATE_SHIFTS round_shift
        self.clamps = {}            # (pass, bit) -> calls whose result differs
        self.pix = 0
        self.dq = None
        self.cast_changed = 0
        self.bd = 0
        real_cv = c.fns["clamp_value"][0]
        real_ita = c.fns["inverse_transform_add"][0]
        real_dq = c.fns["dequantize"][0]
        assert not c.fns.get("round_shift") and not c.fns.get("clamp")     # v_frame's: the transpiler's runtime

        def clamp_value(g, value, bit):
            o = c._call_info(real_cv, g, (value, bit))
            if self.inside and o != value:
                k = (int(self.col), int(bit))
                self.clamps[k] = self.clamps.get(k, 0) + 1
            return o

        def round_shift(g, v, bit):
            if self.inside and bit < 3:
                self.col = True
            return R.round_shift(v, bit)

        def clamp(g, v, lo, hi):
            o = R.clamp3(v, lo, hi)
            if self.inside and self.col and lo == 0 and hi == (1 << self.bd) - 1 and o != v:
                self.pix += 1
            return o

        def ita(g, *args):
            self.inside, self.col = True, False
            try:
                return c._call_info(real_ita, g, args)
            finally:
                self.inside = False

        def dequantize(g, qindex, coeffs, eob, rcoeffs, *rest):
            r = c._call_info(real_dq, g, (qindex, coeffs, eob, rcoeffs) + rest)
            self.dq = [int(v) for v in rcoeffs]
            wide = R.RSlice([0] * len(self.dq))
            c._call_info(real_dq, {"T": "i32"}, (qindex, R.RSlice([int(v) for v in coeffs]), eob, wide) + rest)
            self.cast_changed = int([int(v) for v in wide] != self.dq)
            return r
        for name, fn in (("clamp_value", clamp_value), ("round_shift", round_shift), ("clamp", clamp),
                         ("inverse_transform_add", ita), ("dequantize", dequantize)):
            c.define_py(name, fn)

        self.TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants]
        self.TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
        self.BlockSize = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
        self.PM = {n: L.enum(c, "PredictionMode", n) for n in ("DC_PRED", "NEWMV")}
        self.PMODE = [L.enum(c, "PredictionMode", n) for n in MODES]
        self.DS = L.struct(c, "DistortionScale")
        self.TileStateMut = L.struct(c, "TileStateMut")
        self.CBI = L.struct(c, "CodedBlockInfo")
        self.PSBO, self.SBO = L.struct(c, "PlaneSuperBlockOffset"), L.struct(c, "SuperBlockOffset")
        self.TBO, self.BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
        self.qc_default = c.get("default", owner="QuantizationContext")
        self.qc_update = c.get("update", owner="QuantizationContext")
        self.etb = c.get("encode_tx_block")
        self.RDO_PIX = L.enum(c, "RDOType", "PixelDistRealRate")
        self.refs = R.array(L.enum(c, "RefType", "INTRA_FRAME"), L.enum(c, "RefType", "NONE_FRAME"))
        get_set = c.get("get_tx_set")
        used = c.const_value("av1_tx_used")
        self.types = {inter: [[t for t in range(16) if int(used[int(get_set({}, self.TxSize[ts], inter, False).disc)][t])]
                              for ts in range(19)] for inter in (False, True)}

    def fi(self, bd, qidx):
        c = self.c
        return Obj(sequence=Obj(bit_depth=bd, enable_intra_edge_filter=True,
                                chroma_sampling=L.enum(c, "ChromaSampling", "Cs420")),
                   width=FW, height=FH, w_in_b=FW // 4, h_in_b=FH // 4, use_tx_domain_distortion=False,
                   base_q_idx=qidx, dc_delta_q=R.RSlice([0, 0, 0]), ac_delta_q=R.RSlice([0, 0, 0]),
                   dist_scale=R.RSlice([self.DS(1 << 14)] * 3),
                   config=Obj(temporal_rdo=(lambda: False), tune=L.enum(c, "Tune", "Psnr")),
                   coded_frame_data=R.NONE, cpu_feature_level=None, use_reduced_tx_set=False)

    def run(self, family, bd, ts, tt, qidx, is_intra, res):
        """one encode_tx_block -> (eob, qcoeffs, rcoeffs, rec - src, row, col, pix clamps, cast_changed)"""
        c = self.c
        w, h = TX_W[ts], TX_H[ts]
        dt = L.np_dtype(bd)
        mid = 1 << (bd - 1)
        src = np.zeros((FH, FW), np.int64) if family == 0 else np.full((FH, FW), mid, np.int64)
        pred = src.copy()
        sl = (slice(BY * 4, BY * 4 + h), slice(BX * 4, BX * 4 + w))
        if family == 0:
            src[sl], pred[sl] = np.maximum(res, 0), np.maximum(-res, 0)
        else:
            src[sl] = mid + (res >> 1)
        assert src.min() >= 0 and src.max() < (1 << bd)
        p_in = L.plane_from_array(src.astype(dt), bd, 16, 16, pad_value=mid)
        p_rec = L.plane_from_array(pred.astype(dt), bd, 16, 16, pad_value=mid)
        qc = self.qc_default({})
        self.qc_update({}, qc, qidx, self.TxSize[ts], bool(is_intra), bd, 0, 0)
        dc = self.CBI(luma_mode=R.Some(self.PM["DC_PRED"]), chroma_mode=R.Some(self.PM["DC_PRED"]),
                      reference_types=self.refs)
        cbi = R.RSlice([R.RSlice([dc] * (FW // 4)) for _ in range(FH // 4)])
        tsm = make_struct(
            self.TileStateMut, sbo=self.PSBO(self.SBO(x=0, y=0)), sb_size_log2=6, sb_width=FW // 64,
            sb_height=FH // 64, mi_width=FW // 4, mi_height=FH // 4, width=FW, height=FH,
            input=Obj(planes=R.RSlice([p_in])), input_tile=Obj(planes=R.RSlice([p_in.as_region()])),
            rec=Obj(planes=R.RSlice([p_rec.as_region()])), qc=qc, coded_block_info=cbi)
        g = dict(L.pixel_type(bd), W="BitCounter")
        wr, cw = BitCounter(), CoeffRecorder()
        bo = self.TBO(self.BO(x=BX, y=BY))
        self.clamps, self.pix, self.dq, self.cast_changed, self.bd = {}, 0, None, 0, bd
        mode = self.PM["NEWMV" if family == 0 else "DC_PRED"]
        iparam = L.enum(c, "IntraParam", "None") if family == 0 else c.G["_E"]("IntraParam", "AngleDelta", 0, (0,))
        self.etb(g, self.fi(bd, qidx), tsm, cw, wr, 0, bo, 0, 0, bo, mode, self.TxSize[ts], self.TxType[tt],
                 self.BlockSize["BLOCK_%dX%d" % (w, h)], R.PlaneOffset(x=BX * 4, y=BY * 4), False, qidx, R.RSlice([]),
                 iparam, self.RDO_PIX, family == 1)
        assert len(cw.calls) == 1 and not wr.bits
        qcf, eob, cw_, ch_ = cw.calls[0]
        assert (cw_, ch_) == (w, h)
        rec = L.plane_to_array(p_rec, dt).astype(np.int64)
        outside = rec.copy()
        outside[sl] = pred[sl]
        assert np.array_equal(outside, pred)            # only the block was written
        if family == 1 and eob == 0:
            assert (rec[sl] == mid).all()               # DC_PRED of a mid-grey plane
        area = min(w, 32) * min(h, 32)
        assert not any(qcf[area:]) and not any(self.dq[area:])
        row_bit, col_bit = bd + 8, max(bd + 6, 16)
        assert set(self.clamps) <= {(0, row_bit), (1, col_bit)}, self.clamps
        return (eob, np.array(qcf[:area], np.int64), np.array(self.dq[:area], np.int64), (rec - src)[sl],
                self.clamps.get((0, row_bit), 0), self.clamps.get((1, col_bit), 0), self.pix, self.cast_changed)


    def run_split(self, bd, bs, ts, tt, mode, qidx, halvings):
        """the loop of write_tx_blocks over the bs x bs block at (SPLIT_XY, SPLIT_XY), as gen_rdo_intra_split_ref.py
        states it: encode_tx_block once per transform block in raster order on ONE tile state
        -> (src block, per transform block (eob, qc, dq, row, col, pix clamps, cast_changed), rec - src)"""
        c = self.c
        t = TX_W[ts]
        gw = bs // t
        dt = L.np_dtype(bd)
        mid, mx = 1 << (bd - 1), (1 << bd) - 1
        sign = halve(BLOCKS[bd, ts, tt][0], halvings) >> 1
        src = np.full((FH, FW), mid, np.int64)
        for k in range(gw * gw):
            y0, x0 = SPLIT_XY + (k // gw) * t, SPLIT_XY + (k % gw) * t
            src[y0:y0 + t, x0:x0 + t] = np.clip(mid + (sign if k % 2 == 0 else -sign), 0, mx)
        p_in = L.plane_from_array(src.astype(dt), bd, 16, 16, pad_value=mid)
        p_rec = L.plane_from_array(np.full((FH, FW), mid, dt), bd, 16, 16, pad_value=mid)
        qc = self.qc_default({})
        self.qc_update({}, qc, qidx, self.TxSize[ts], True, bd, 0, 0)
        dc = self.CBI(luma_mode=R.Some(self.PM["DC_PRED"]), chroma_mode=R.Some(self.PM["DC_PRED"]),
                      reference_types=self.refs)
        cbi = R.RSlice([R.RSlice([dc] * (FW // 4)) for _ in range(FH // 4)])
        tsm = make_struct(
            self.TileStateMut, sbo=self.PSBO(self.SBO(x=0, y=0)), sb_size_log2=6, sb_width=FW // 64,
            sb_height=FH // 64, mi_width=FW // 4, mi_height=FH // 4, width=FW, height=FH,
            input=Obj(planes=R.RSlice([p_in])), input_tile=Obj(planes=R.RSlice([p_in.as_region()])),
            rec=Obj(planes=R.RSlice([p_rec.as_region()])), qc=qc, coded_block_info=cbi)
        fi = self.fi(bd, qidx)
        fi.sequence.enable_intra_edge_filter = False
        g = dict(L.pixel_type(bd), W="BitCounter")
        wr, cw = BitCounter(), CoeffRecorder()
        bo_x = bo_y = SPLIT_XY >> 2
        bo = self.TBO(self.BO(x=bo_x, y=bo_y))
        iparam = c.G["_E"]("IntraParam", "AngleDelta", 0, (0,))
        self.bd = bd
        per = []
        for by in range(gw):
            for bx in range(gw):
                tbx, tby = bo_x + bx * (t >> 2), bo_y + by * (t >> 2)
                self.clamps, self.pix, self.dq, self.cast_changed = {}, 0, None, 0
                self.etb(g, fi, tsm, cw, wr, 0, bo, bx, by, self.TBO(self.BO(x=tbx, y=tby)), self.PMODE[mode],
                         self.TxSize[ts], self.TxType[tt], self.BlockSize["BLOCK_%dX%d" % (bs, bs)],
                         R.PlaneOffset(x=tbx * 4, y=tby * 4), False, qidx, R.RSlice([]), iparam, self.RDO_PIX, True)
                qcf, eob, _, _ = cw.calls[-1]
                row_bit, col_bit = bd + 8, max(bd + 6, 16)
                assert set(self.clamps) <= {(0, row_bit), (1, col_bit)}, self.clamps
                per.append((eob, np.array(qcf[:t * t], np.int64), np.array(self.dq[:t * t], np.int64),
                            self.clamps.get((0, row_bit), 0), self.clamps.get((1, col_bit), 0), self.pix,
                            self.cast_changed))
        assert len(cw.calls) == gw * gw and not wr.bits
        rec = L.plane_to_array(p_rec, dt).astype(np.int64)
        sl = (slice(SPLIT_XY, SPLIT_XY + bs), slice(SPLIT_XY, SPLIT_XY + bs))
        outside = rec.copy()
        outside[sl] = mid
        assert (outside == mid).all()                    # only the block was written
        return src[sl], per, (rec - src)[sl]


SPLIT_XY = 64           # the block's corner: superblock-aligned, both edges inside the plane
SPLIT_COLUMNS = ["bd", "block_size", "tx_size", "tx_type", "mode", "qindex", "x", "y", "plane_w", "plane_h", "halvings",
                 "strict_trips"]
SPLIT_TX_COLUMNS = ["case", "k", "eob", "cast_changed", "row_clamps", "col_clamps", "pix_clamps"]


def split_list():
    """(bd, block size, tx_size, tx_type index into the intra set, mode, qindex): 8x8/4x4, 16x16/8x8, 32x32/16x16,
    64x64/32x32 at each bit depth, every one at both qindex; DC / V / H / Paeth in turn (no edge beyond the block's
    own row and column, no edge filter), the type moving through the intra set of the transform size"""
    out = []
    for bd in (8, 10, 12):
        for ts in range(4):
            for qidx in QINDEX:
                k = len(out)
                out.append((bd, 2 * TX_W[ts], ts, k, (0, 1, 2, 12)[(k // 2) % 4], qidx))
    return out


def split_unit(args):
    bd, bs, ts, ti, mode, qidx = args
    types = WORLD.types[False][ts]
    tt = types[ti % len(types)]
    trips = 0
    for k in range(16):
        try:
            src, per, rms = WORLD.run_split(bd, bs, ts, tt, mode, qidx, k)
            break
        except R.Panic as e:
            assert "does not fit" in str(e) or "overflow" in str(e), (args, str(e))
            trips += 1
    else:
        raise SystemExit("no amplitude of split case %r runs under strict mode" % (args,))
    return (bd, bs, ts, tt, mode, qidx, SPLIT_XY, SPLIT_XY, FW, FH, k, trips), per, (src, rms)


def halve(res, k):
    return np.sign(res) * (np.abs(res) >> k)


WORLD = None        # built once, in front of the fork
BLOCKS = None


def unit(args):
    """every block of one (family, bd, tx_size, is_intra)"""
    family, bd, ts, is_intra = args
    W = WORLD
    rows, qcs, dqs, rms = [], [], [], []
    w, h = TX_W[ts], TX_H[ts]
    names = (SMALL_BLOCKS if w * h <= 256 else BIG_BLOCKS) if family == 0 else BIG_BLOCKS
    for tt in W.types[family == 0][ts]:
        for qidx in QINDEX:
            for b in names:
                res = BLOCKS[bd, ts, tt][b]
                trips = 0
                for k in range(16):
                    try:
                        eob, qc, dq, rm, nrow, ncol, npix, cast = W.run(family, bd, ts, tt, qidx, is_intra, halve(res, k))
                        break
                    except R.Panic as e:
                        assert "does not fit" in str(e) or "overflow" in str(e), (args, tt, qidx, b, str(e))
                        trips += 1
                else:
                    raise SystemExit("no amplitude of %r runs under strict mode" % ((args, tt, qidx, b),))
                rows.append((family, bd, ts, tt, qidx, is_intra, b, k, eob, cast, nrow, ncol, npix, trips))
                qcs.append(qc)
                dqs.append(dq)
                rms.append(rm.ravel())
    return rows, qcs, dqs, rms


def narrow(arrs, dtype):
    """the arrays end to end in the file's type, which must hold every value"""
    a = np.concatenate(arrs)
    assert np.array_equal(a.astype(dtype), a)
    return a.astype(dtype)


def main():
    global WORLD, BLOCKS
    WORLD, BLOCKS = World(), fwd_blocks()
    limit = os.environ.get("R1_INV_PATH_SIZES")         # e.g. "0,5": a subset of the sizes, for a quick look
    sizes = [int(s) for s in limit.split(",")] if limit else list(range(19))
    units = []
    for bd in (8, 10, 12):
        units += [(0, bd, ts, 0) for ts in sizes]
        units += [(0, bd, ts, 1) for ts in sizes if ts == INTRA_OFFSET_SIZE]
        units += [(1, bd, ts, 1) for ts in sizes if ts in FLAT_SIZES]
    nproc = int(os.environ.get("R1_GEN_PROCS", "0")) or min(16, os.cpu_count() or 1)
    # largest units first; the results are put back into the order of `units`
    order = sorted(range(len(units)), key=lambda i: -TX_W[units[i][2]] * TX_H[units[i][2]])
    with multiprocessing.get_context("fork").Pool(nproc) as pool:
        res = pool.map(unit, [units[i] for i in order], chunksize=1)
        splits = pool.map(split_unit, split_list() if not limit else [], chunksize=1)
    done = dict(zip(order, res))
    out, dq_out = {}, {}
    rows = []
    for bd in (8, 10, 12):
        ct = np.int16 if bd == 8 else np.int32
        qcs, dqs, rms = [], [], []
        for i, u in enumerate(units):
            if u[1] != bd:
                continue
            r, q, d, m = done[i]
            rows += r
            qcs += q
            dqs += d
            rms += m
        out["qc_%d" % bd], dq_out["dq_%d" % bd] = narrow(qcs, ct), narrow(dqs, ct)
        out["rms_%d" % bd] = narrow(rms, np.int16)
        mine = [s for s in splits if s[0][0] == bd]
        if mine:
            out["split_qc_%d" % bd] = narrow([p[1] for s in mine for p in s[1]], ct)
            dq_out["split_dq_%d" % bd] = narrow([p[2] for s in mine for p in s[1]], ct)
            out["split_rms_%d" % bd] = narrow([s[2][1].ravel() for s in mine], np.int16)
            out["split_src_%d" % bd] = narrow([s[2][0].ravel() for s in mine], np.uint16)
    if splits:
        out["split"] = np.array([s[0] for s in splits], np.int32)
        out["split_columns"] = np.array(SPLIT_COLUMNS)
        out["split_tx"] = np.array([(ci, k, p[0], p[6], p[3], p[4], p[5]) for ci, s in enumerate(splits)
                                    for k, p in enumerate(s[1])], np.int32)
        out["split_tx_columns"] = np.array(SPLIT_TX_COLUMNS)
    out["blocks"] = np.array(rows, np.int32)
    out["columns"] = np.array(COLUMNS)
    out["names"] = np.array(NAMES)
    L.save("inv_path_ref.npz", out)
    L.save("inv_path_ref_dq.npz", dq_out)
    b = out["blocks"]
    print(len(b), "blocks;", int((b[:, 7] > 0).sum()), "halved;", "clamped row/col/pix:",
          int((b[:, 10] > 0).sum()), int((b[:, 11] > 0).sum()), int((b[:, 12] > 0).sum()))


if __name__ == "__main__":
    sys.exit(main())

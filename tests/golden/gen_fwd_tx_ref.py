#!/usr/bin/env python3
"""tests/golden/fwd_tx_ref.npz: `forward_transform` computed by the REFERENCE'S OWN SOURCE TEXT, whole.

  transform::forward::rust::forward_transform   src/transform/forward.rs:71-161
      the WHOLE function as written: valid_av1_transform, Txfm2DFlipCfg::fwd (shift rows, 1-D types,
      flips; forward_shared.rs:83-137), the column pass with the up-down flip, the two
      av1_round_shift_array calls around it, the left-right flip into `buf`, the row pass, the
      32x32-chunked transposed store and T::cast_from (i16 for 8-bit pixels, i32 above),
  `impl TxOperations for i32` (forward.rs:37-65): tx_mul, rshift1, add, sub, add_avg, sub_avg are
      transpiled and CALLED for every butterfly; nothing of them is restated here,
  and the 13 1-D networks of the impl_1d_tx! macro body (forward_shared.rs:179-1797) as translated
      by gen_fwd_tx_golden.py, bound to get_func the way gen_rdo_glue_ref.py binds them -- with the
      one difference that a lane is a plain i32 whose six operations are the transpiled trait
      methods above, so the crate's strict range checks cover the butterflies as well.

tools/rustlite transpiles these items at run time (strict=True: every arithmetic result is checked
against its Rust type, so a block that runs to the end overflows nowhere and a debug and a release
build of the reference agree on it).  Nothing is imported from oracle/.

Cases: every (tx_size, valid tx_type, bit depth 8/10/12), WHT at 4x4 included: 160 x 3.
Blocks per case, lim = 2^bd - 1 (BLOCKS names them in stored order):
  sign     outer(s_col, s_row) * lim.  s_col / s_row: the sign pattern of the tx_mul input with the
           largest L1 impulse response inside the column / row network, impulse responses taken by
           running the translated reference networks on unit impulses; reversed again for the
           flipped types so that the network sees the pattern, not its mirror image
  rand     uniformly random in [-lim, lim]
  const+ / const-          every residual +lim / -lim
  checker / rows / cols    one-pixel checkerboard, alternating rows, alternating columns, at +-lim
  small    [-2, 2], mostly odd and negative: rshift1, add_avg and the rounding terms decide
  impulse  a single -lim at the last row and last column
  zero     all zero
Up to area 1024 a case holds all ten.  Above (64x64, 32x64, 64x32) it holds the first seven: the
sign block, one random block and every member of the constant and alternating groups.
All blocks but `sign` depend on (bit depth, size) only and are stored once per size.

Recorded per block from the executed run (stats[case, block] = mulmax, colmax, cmax):
  mulmax   the largest |self| any tx_mul call saw,
  colmax   the largest magnitude handed to a row network, i.e. what `buf` holds after shift[1],
  cmax     the largest |coefficient| written (before T::cast_from narrows it).

Layout of the file (few large arrays: a zip member per case would cost more than the data):
  cases   (ncase, 6) int32: bit depth, tx_size, tx_type, number of blocks, w, h; cases of one bit
          depth are contiguous and in (tx_size, tx_type) order
  shared_<bd>  int16, per tx_size in order: (nshared, h, w) flattened   (rand .. zero)
  sign_<bd>    int16, per case in order: (h, w) flattened
  coef_<bd>    int16 at 8 bits, int32 above, per case in order: (nblocks, w * h) flattened
  stats   (ncase, 10, 3) int64
tests/fwd_tx_ref_util.py reads it back.

Run in the build container:  python tests/golden/gen_fwd_tx_ref.py
"""
import os
import sys

import numpy as np

# (gen_fwd_tx_golden puts oracle/ on sys.path for its own hand-stated 2-D driver; nothing here calls that driver,
# and no module of oracle/ may be imported below, by that path or by a name that happens to live there)
import gen_fwd_tx_golden as FT
import reflib as L
from reflib import R

FILES = ["transform/forward.rs", "transform/forward_shared.rs", "transform/mod.rs"]
TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
BLOCKS = ["sign", "rand", "const+", "const-", "checker", "rows", "cols", "small", "impulse", "zero"]
NBIG = 7            # blocks of a case above area 1024


class Lane:
    """One i32 lane.  Every operation is the transpiled `impl TxOperations for i32` method."""
    __slots__ = ("v",)
    ops = None          # name -> transpiled function
    mulmax = 0

    def __init__(self, v):
        self.v = v

    def tx_mul(self, shift, mul):
        a = -self.v if self.v < 0 else self.v
        if a > Lane.mulmax:
            Lane.mulmax = a
        return Lane(Lane.ops["tx_mul"]({"SHIFT": shift}, self.v, mul))

    def rshift1(self):
        return Lane(Lane.ops["rshift1"]({}, self.v))

    def add(self, b):
        return Lane(Lane.ops["add"]({}, self.v, b.v))

    def sub(self, b):
        return Lane(Lane.ops["sub"]({}, self.v, b.v))

    def add_avg(self, b):
        return Lane(Lane.ops["add_avg"]({}, self.v, b.v))

    def sub_avg(self, b):
        return Lane(Lane.ops["sub_avg"]({}, self.v, b.v))

    def copy_fn(self):
        return self


def worst_signs(ns, ttype):
    """sign pattern of the tx_mul input with the largest L1 impulse response (numpy lanes, one
    lane per impulse; the networks are the translated reference text)"""
    n = FT.TXFM_LEN[ttype]
    recs = []
    orig = FT.V.tx_mul

    def spy(self, shift, mul):
        recs.append(self.v.astype(np.int64).copy())
        return orig(self, shift, mul)
    FT.V.tx_mul = spy
    try:
        FT.run_1d(ns, ttype, np.eye(n, dtype=np.int32) * (1 << 12))
    finally:
        FT.V.tx_mul = orig
    if not recs:
        return np.ones(n, np.int64)
    a = np.stack(recs)                  # (tx_mul call, impulse position)
    s = np.sign(a[np.abs(a).sum(1).argmax()])
    s[s == 0] = 1
    return s


def shared_blocks(rng, bd, w, h):
    lim = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    small = rng.choice([-2, -1, 0, 1, 2], (h, w), p=[0.1, 0.55, 0.1, 0.15, 0.1])
    imp = np.zeros((h, w), np.int64)
    imp[h - 1, w - 1] = -lim
    b = [rng.integers(-lim, lim + 1, (h, w)),
         np.full((h, w), lim), np.full((h, w), -lim),
         np.where((yy + xx) & 1, -lim, lim), np.where(yy & 1, -lim, lim), np.where(xx & 1, -lim, lim),
         small, imp, np.zeros((h, w), np.int64)]
    return np.stack(b).astype(np.int16)


def main():
    c = L.crate(*FILES, strict=True)
    src = open(os.path.join(L.REF_SRC, "transform", "forward_shared.rs")).read()
    ns_lane = {"Buf": FT.Buf}
    exec(compile(FT.translate(src), "<forward_shared.rs translated>", "exec"), ns_lane)
    ns_np = {"V": FT.V, "Buf": FT.Buf}
    exec(compile(FT.translate(src), "<forward_shared.rs translated>", "exec"), ns_np)
    Lane.ops = {k: c.get(k, owner="i32") for k in ("tx_mul", "rshift1", "add", "sub", "add_avg", "sub_avg")}
    row_in = []         # per get_func call of one forward_transform: max |input|

    def get_func(_g, t):
        idx = t.disc if hasattr(t, "disc") else int(t)
        name, n = FT.TXFM[idx], FT.TXFM_LEN[idx]

        def run(coeffs):
            buf = FT.Buf(n)
            m = 0
            for i in range(n):
                v = int(coeffs[i])
                m = max(m, abs(v))
                buf[i] = Lane(v)
            row_in.append(m)
            ns_lane[name](buf)
            for i in range(n):
                coeffs[i] = buf[i].v
        return run
    c.define_py("get_func", get_func)

    ft = c.get("forward_transform")
    valid = c.get("valid_av1_transform")
    cfg_fwd = c.get("fwd", owner="Txfm2DFlipCfg")
    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    assert len(TxSize) == 19 and len(TxType) == 17
    signs = [worst_signs(ns_np, t) for t in range(13)]
    rng = np.random.default_rng(20261020)
    out = {}
    cases, stats = [], []
    for bd in (8, 10, 12):
        lim = (1 << bd) - 1
        ct = np.int16 if bd == 8 else np.int32
        g = {"T": "i16" if bd == 8 else "i32"}
        shared, sign, coef = [], [], []
        for ts in range(19):
            w, h = TX_W[ts], TX_H[ts]
            nb = len(BLOCKS) if w * h <= 1024 else NBIG
            sh = shared_blocks(rng, bd, w, h)[:nb - 1]
            shared.append(sh.ravel())
            for tt in range(17):
                if not valid({}, TxSize[ts], TxType[tt]):
                    continue
                if tt == 16 and ts != 0:
                    continue    # Txfm2DFlipCfg::fwd unwraps a None for WHT beyond 4 points: a panic
                cfg = cfg_fwd({}, TxType[tt], TxSize[ts], bd)
                s_col, s_row = signs[cfg.txfm_type_col.disc], signs[cfg.txfm_type_row.disc]
                assert len(s_col) == h and len(s_row) == w
                if cfg.ud_flip:
                    s_col = s_col[::-1]
                if cfg.lr_flip:
                    s_row = s_row[::-1]
                sg = (np.outer(s_col, s_row) * lim).astype(np.int16)
                sign.append(sg.ravel())
                st = np.zeros((len(BLOCKS), 3), np.int64)
                for i, res in enumerate([sg] + list(sh)):
                    outp = R.RSlice([0] * (w * h))
                    del row_in[:]
                    Lane.mulmax = 0
                    inp = R.RSlice([int(v) for v in res.ravel()])
                    ft(g, inp, outp, w, TxSize[ts], TxType[tt], bd, None)
                    assert len(row_in) == w + h
                    co = np.array([int(v) for v in outp], np.int64)
                    st[i] = (Lane.mulmax, max(row_in[w:]), int(np.abs(co).max()))
                    if bd == 8:
                        # T::cast_from narrows to i16 here.  The same block at T = i32 shows what was
                        # narrowed: nothing, so one stored array serves both coefficient widths.
                        wide = R.RSlice([0] * (w * h))
                        ft({"T": "i32"}, inp, wide, w, TxSize[ts], TxType[tt], bd, None)
                        assert [int(v) for v in wide] == list(co), "an 8-bit coefficient does not fit i16"
                    coef.append(co.astype(ct))
                stats.append(st)
                cases.append((bd, ts, tt, nb, w, h))
            print("bd", bd, "tx_size", ts, "done,", len(cases), "cases", flush=True)
        out["shared_%d" % bd] = np.concatenate(shared)
        out["sign_%d" % bd] = np.concatenate(sign)
        out["coef_%d" % bd] = np.concatenate(coef)
    out["cases"] = np.array(cases, np.int32)
    out["stats"] = np.stack(stats)
    out["blocks"] = np.array(BLOCKS)
    L.save("fwd_tx_ref.npz", out)
    print(len(cases), "cases;", sum(cs[3] for cs in cases), "blocks")


if __name__ == "__main__":
    sys.exit(main())

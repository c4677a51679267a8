#!/usr/bin/env python3
"""tests/golden/me_ref_12.npz: the 12-bit sibling of me_ref.npz -- one tile search and eight
RDO-time block searches computed by the REFERENCE'S OWN SOURCE TEXT (the functions
gen_me_ref.py lists), transpiled by tools/rustlite and executed here.  Same keys as
me_ref.npz; a file and a seed of its own, so me_ref.npz is never rewritten.

The case: 136 x 72 (cropped superblocks) at 12 bits, smooth texture displaced by a
half-pel amount, previous-frame predictors, 1/8-pel vectors allowed.  The blocks: 8x8,
16x8, 8x16, 16x16 (the sizes whose SATD the device computes in packed 16-bit lanes at
8 / 10 bits and must not at 12), 32x32, 64x64, 4x4 and 16x64.

Run in the build container:  python tests/golden/gen_me_ref_12.py
"""
import time

import numpy as np

import reflib as L
from reflib import R
from gen_me_ref import World, lambdas, smooth

NAME, W, H, BD = "d0", 136, 72, 12
ME_LAMBDA = 4.96          # gen_me_ref.py's 8-bit 0.31 at the 12-bit scale
SIZES = [(8, 8), (16, 8), (8, 16), (16, 16), (32, 32), (64, 64), (4, 4), (16, 64)]


def main():
    c = L.crate("me.rs", "mc.rs", "dist.rs", "predict.rs", "context/block_unit.rs", "context/superblock_unit.rs")
    est_tile, est = c.get("estimate_tile_motion"), c.get("estimate_motion")
    rng = np.random.default_rng(71200)
    out = {}
    t0 = time.time()
    # the reference: the texture displaced by (2.5, -1) pixels (the mean of two integer shifts)
    # plus noise, so that the sub-pel diamond of the block searches has something to find
    big = smooth(rng, W, H, BD)
    org = big[32:32 + H, 32:32 + W]
    ref = (big[33:33 + H, 30:30 + W] + big[33:33 + H, 29:29 + W] + 1) >> 1
    refs = [np.clip(ref + rng.integers(-8, 9, ref.shape), 0, (1 << BD) - 1)]
    cols, rows = (W + 3) // 4, (H + 3) // 4
    tile = (0, 0, W, H)
    prev = np.zeros((rows, cols, 3), np.int64)
    prev[..., 0] = rng.integers(-96, 97, (rows, cols))
    prev[..., 1] = rng.integers(-96, 97, (rows, cols))
    prev[..., 2] = rng.integers(0, 1 << 24, (rows, cols))
    wd = World(c, BD, org, refs, [prev], tile, 1, 0, 1, ME_LAMBDA)
    g = L.pixel_type(BD)
    est_tile(g, wd.fi, wd.ts, wd.inter_cfg)
    out[NAME + "_meta"] = np.array([W, H, BD, *tile, 1, 0, 1, 1, 1])
    out[NAME + "_lambda"] = np.array(lambdas(ME_LAMBDA), np.uint32)
    for s in range(3):
        out["%s_org%d" % (NAME, s)] = wd.org_imgs[s].astype(np.uint16)
        out["%s_ref0_%d" % (NAME, s)] = wd.ref_imgs[0][s].astype(np.uint16)
    out[NAME + "_stats0"] = wd.stats_array(0).astype(np.int64)
    out[NAME + "_prev0"] = prev
    print(NAME, "tile ME done in %.0f s" % (time.time() - t0), "nonzero mvs:",
          int((out[NAME + "_stats0"][..., :2] != 0).any(-1).sum()), flush=True)
    # ---- RDO-time estimate_motion(.., Some(pmv), corner, false, 0, None), one block of every size
    t0 = time.time()
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    SM = "MVSamplingMode"
    blks, res = [], []
    for bi, (bw, bh) in enumerate(SIZES):
        bx = int(rng.integers(0, (W - bw) // bw + 1)) * (bw // 4)
        by = int(rng.integers(0, (H - bh) // bh + 1)) * (bh // 4)
        cm = bi % 5
        if cm == 0:
            corner, code = L.enum(c, SM, "INIT"), 0
        else:
            right, bottom = bool((cm - 1) & 1), bool((cm - 1) & 2)
            corner = R.REnum(SM, "CORNER", 1, (right, bottom))
            code = 1 | (right << 1) | (bottom << 2)
        pmv = [(int(rng.integers(-40, 41)), int(rng.integers(-40, 41))) for _ in range(2)]
        pm = R.Some(R.array(*[wd.MV(row=r_, col=c_) for r_, c_ in pmv]))
        r = est(g, wd.fi, wd.ts, bw, bh, TBO(BO(x=bx, y=by)), wd.ref_types[0], pm, corner, False, 0, R.NONE)
        r = r.p[0]
        blks.append((bx, by, bw, bh, code, pmv[0][0], pmv[0][1], pmv[1][0], pmv[1][1]))
        res.append((r.mv.row, r.mv.col, r.rd.sad, r.rd.cost))
    out[NAME + "_blk"] = np.array(blks, np.int64)
    out[NAME + "_blkout"] = np.array(res, np.int64)
    out[NAME + "_blkcfg"] = np.array([1, 0])
    print(NAME, len(blks), "block searches in %.0f s" % (time.time() - t0), "fractional mvs:",
          int((out[NAME + "_blkout"][:, :2] & 7).any(-1).sum()), flush=True)
    assert int(out[NAME + "_org0"].max()) > 1023 and int(out[NAME + "_ref0_0"].max()) > 1023
    L.save("me_ref_12.npz", out)


if __name__ == "__main__":
    main()

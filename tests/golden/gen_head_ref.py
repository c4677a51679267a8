#!/usr/bin/env python3
"""tests/golden/head_ref.npz: the head symbols of an intra block of an intra frame -- what a mode trial of
luma_chroma_mode_rdo writes in front of the coefficients (src/rdo.rs:866-907 through encode_block_pre_cdef /
encode_block_post_cdef, src/encoder.rs:1896-1913, 1969-1970, 2086-2136), what the coded block leaves in BlockContext and
`fc`, and the partition walker's symbol and context update (src/encoder.rs:2896-2906, 3214-3220) -- EXECUTED through
tools/rustlite on a fresh WriterCounter:
  write_partition (with partition_gather_vert_alike / _horz_alike and partition_plane_context), write_skip (skip_context),
  write_cfl_alphas (CFLParams::from_alpha, joint_sign, context, index), update_partition_context
                                                                        src/context/partition_unit.rs
  write_intra_mode_kf, write_angle_delta, write_intra_uv_mode, update_tx_size_context, reset_left_contexts
                                                                        src/context/block_unit.rs
  write_tx_size_intra (get_tx_size_context, tx_size_to_depth, bsize_to_max_depth, bsize_to_tx_size_cat)
                                                                        src/context/transform_unit.rs
  has_chroma, BlockSize::cfl_allowed, PredictionMode::is_directional / is_cfl, CDFContext::new, symbol, update_cdf,
  tell_frac.
All of these files load whole.  Restatements (docs/PARITY.md, "head symbols"):
  * the ORDER of the calls and their conditions (rdo.rs:870-877, encoder.rs:1913, 2086-2136) is this file's `head()`;
    the conditions themselves are evaluated by the executed text (`bsize >= BLOCK_8X8` on the enum, is_directional,
    cfl_allowed, has_chroma).
  * TileBlocksMut (src/tiling/tile_blocks.rs: a macro over raw pointers) is `Blocks` below: a real 2-D array of Block
    stand-ins with above_of / left_of / cols / rows and for_each's clipping (206-224) behind set_mode / set_skip /
    set_tx_size.  Block::is_inter runs from the text on the stand-in's `mode`.
  * symbol_with_update!, ContextWriter / BlockContext: as gen_coeff_rate_ref.py states.
  * Where the reference rolls a trial back, the generator runs it on a deep copy of `fc`; a trial never touches `bc`.

(a) `single_*`: trials on eight seeded (BlockContext, CDFContext) pairs -- CDFContext::new at the four qindex classes
    and four adapted and randomised ones; neighbour arrays and a blocks array seeded around one cursor row each -- chosen
    per trap (the names say which) and then at random over every block size, mode, delta, alpha and depth.
(b) `seq_* / ev_* / trial_* / part_*`: sequences of up to 16 events in real coding order on ONE BlockContext, blocks
    array and `fc`: per block the walker's partition symbols in front (the tile writer: they only adapt), every trial's
    rate and rng on a copy, then the prescribed winner coded for real (without the trial's own PARTITION_NONE: the real
    partition symbol is the walker's), then update_partition_context where the walker
    calls it, then every array and the packed CDFs behind it.  `reset` events call reset_left_contexts(3).
(c) `part_*_case`: write_partition alone, all four types, the three edge arms, from a given rng.
The row buffers of R1HeadNbrContext (above / left mode and skip) behind an event are read off the blocks array: entry x
of `above` is the cell of column x coded last, entry r of `left` the cell of rows = r mod 16 coded last.  What pins them
is that every later trial's rate comes from above_of / left_of on the 2-D array.

Run in the build container:  python tests/golden/gen_head_ref.py
"""
import copy

import numpy as np

import reflib as L
from reflib import R
from gen_coeff_rate_ref import FILES, CW, BC

WIDTH = 1024
# R1HeadCdfContext: (field of the reference's CDFContext, shape), in the struct's order
CDF_FIELDS = (("partition_w8_cdf", (4, 4)), ("partition_cdf", (12, 10)), ("partition_w128_cdf", (4, 8)),
              ("skip_cdfs", (3, 2)), ("kf_y_cdf", (5, 5, 13)), ("y_mode_cdf", (4, 13)), ("uv_mode_cdf", (13, 13)),
              ("uv_mode_cfl_cdf", (13, 14)), ("angle_delta_cdf", (8, 7)), ("cfl_sign_cdf", (8,)), ("cfl_alpha_cdf", (6, 16)),
              ("tx_size_8x8_cdf", (3, 2)), ("tx_size_cdf", (3, 3, 3)))
CDF_LEN = sum(int(np.prod(s)) for _, s in CDF_FIELDS) + 1          # one entry of padding: 1096
NBR_LEN = 512 + 8 + 1024 + 16 + 2 * (1024 + 16)                    # 3640
C420, C444 = (1, 1), (0, 0)
SINGLE_COLS = ("ctx", "bo_x", "bo_y", "mi_cols", "mi_rows", "bsize", "has_chroma", "tx_mode_select", "y_mode", "uv_mode",
               "angle_y", "angle_uv", "alpha_u", "alpha_v", "tx_size", "rate", "rng", "xdec", "ydec")
EV_COLS = ("seq", "step", "kind", "bsize", "bo_x", "bo_y", "has_chroma", "n_trials", "trial_off", "winner", "n_parts",
           "part_off", "upc_subsize", "upc_bsize", "upc_x", "upc_y")
TRIAL_COLS = ("y_mode", "uv_mode", "angle_y", "angle_uv", "alpha_u", "alpha_v", "tx_size", "rate", "rng")
PART_COLS = ("bsize", "bo_x", "bo_y", "ptype")
PCASE_COLS = ("ctx", "bsize", "bo_x", "bo_y", "mi_cols", "mi_rows", "ptype", "rng0", "rate", "rng")
SEQ_COLS = ("q", "xdec", "ydec", "mi_cols", "mi_rows", "n_events", "tx_mode_select")
NONE, HORZ, VERT, SPLIT = 0, 1, 2, 3
DC, V, H, D45, D135, D113, D157, D203, D67, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH, CFL = range(14)


class Blk:
    _rname = "Block"

    def __init__(self, mode, skip):
        self.mode, self.skip, self.txsize, self.stamp = mode, skip, None, 0


class Blocks:
    """TileBlocksMut over a real 2-D array (see the module text)"""

    def __init__(self, cols, rows, dc):
        self.grid = [[Blk(dc, False) for _ in range(cols)] for _ in range(rows)]
        self.clock = 0

    def cols(self):
        return len(self.grid[0])

    def rows(self):
        return len(self.grid)

    def __getitem__(self, i):
        if isinstance(i, int):
            return self.grid[i]
        return self.grid[i._0.y][i._0.x]

    def above_of(self, bo):
        return self.grid[bo._0.y - 1][bo._0.x]

    def left_of(self, bo):
        return self.grid[bo._0.y][bo._0.x - 1]

    def for_each(self, bo, w_mi, h_mi, f):          # tile_blocks.rs:206-224
        x, y = bo._0.x, bo._0.y
        bw = w_mi
        if x + bw >= self.cols():
            bw = self.cols() - x
        self.clock += 1
        for dy in range(h_mi):
            if y + dy >= self.rows():
                continue
            for b in self.grid[y + dy][x:x + bw]:
                f(b)
                b.stamp = self.clock


def main():
    c = L.crate(*FILES)
    L.load_v_frame_types(c)
    c.load("context/partition_unit.rs")
    bs_names = [v[0] for v in c.enums["BlockSize"].variants][:22]
    BS = [L.enum(c, "BlockSize", n) for n in bs_names]
    bs_w = [int(c.call_method(b, "width_mi", [])) for b in BS]
    bs_h = [int(c.call_method(b, "height_mi", [])) for b in BS]
    bs_of = {(w * 4, h * 4): i for i, (w, h) in enumerate(zip(bs_w, bs_h))}
    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants][:19]
    PM = [L.enum(c, "PredictionMode", v[0]) for v in c.enums["PredictionMode"].variants]
    PT = [L.enum(c, "PartitionType", v[0]) for v in c.enums["PartitionType"].variants]
    CS = {C420: L.enum(c, "ChromaSampling", "Cs420"), C444: L.enum(c, "ChromaSampling", "Cs444")}
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    new_counter = c.get("new", owner="WriterCounter")
    new_fc = c.get("new", owner="CDFContext")
    F = {n: c.get(n, owner="ContextWriter") for n in ("write_partition", "write_skip", "write_intra_mode_kf", "write_angle_delta",
                                                      "write_intra_uv_mode", "write_cfl_alphas", "write_tx_size_intra")}
    upd_tx = c.get("update_tx_size_context", owner="BlockContext")
    upd_part = c.get("update_partition_context", owner="BlockContext")
    reset_left = c.get("reset_left_contexts", owner="BlockContext")
    from_alpha = c.get("from_alpha", owner="CFLParams")
    has_chroma = c.get("has_chroma")
    max_rect = [int(v.disc) for v in c.const_value("max_txsize_rect_lookup")][:22]
    sub_map = [int(v.disc) for v in c.const_value("sub_tx_size_map")]
    g = {"W": "WriterBase"}
    # `bsize >= BLOCK_8X8` / `bsize > BLOCK_4X4` are comparisons of the enum's discriminants (derive(PartialOrd))
    I_8X8, I_4X4 = bs_names.index("BLOCK_8X8"), bs_names.index("BLOCK_4X4")
    tx_of = {(int(c.call_method(t, "width", [])), int(c.call_method(t, "height", []))): i for i, t in enumerate(TxSize)}
    rng = np.random.default_rng(20261023)
    tell = lambda w: int(c.call_method(w, "tell_frac", []))

    def depths(bsize):
        """the transform sizes at depth 0, 1, 2 of the block (rdo_tx_size_type walks the same map)"""
        t = max_rect[bsize]
        out = [t]
        for _ in range(2):
            if sub_map[t] == t:
                break
            t = sub_map[t]
            out.append(t)
        return out

    def pack_fc(fc):
        out = [np.array([int(v) for v in np.array(R_list(getattr(fc, f))).reshape(-1)], np.int64) for f, _ in CDF_FIELDS]
        for a, (f, s) in zip(out, CDF_FIELDS):
            assert a.size == int(np.prod(s)), (f, a.size, s)
        return np.concatenate(out + [np.zeros(1, np.int64)]).astype(np.uint16)

    def R_list(v):
        return [R_list(x) for x in v] if hasattr(v, "__iter__") else int(v)

    def pack_nbr(bc):
        bl = bc.blocks
        rows, cols = bl.rows(), bl.cols()
        am, ak = np.zeros(WIDTH, np.uint8), np.zeros(WIDTH, np.uint8)
        lm, lk = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
        for x in range(cols):
            b = max((bl.grid[y][x] for y in range(rows)), key=lambda b: b.stamp)
            if b.stamp:
                am[x], ak[x] = int(b.mode.disc), int(b.skip)
        for r in range(16):
            cells = [b for y in range(r, rows, 16) for b in bl.grid[y]]
            b = max(cells, key=lambda b: b.stamp) if cells else None
            if b is not None and b.stamp:
                lm[r], lk[r] = int(b.mode.disc), int(b.skip)
        return np.concatenate([np.array([int(v) for v in a], np.uint8) for a in
                               (bc.above_partition_context, bc.left_partition_context, bc.above_tx_context,
                                bc.left_tx_context)] + [am, lm, ak, lk])

    def head(cw, w, bsize, bo_x, bo_y, xdec, ydec, tx_mode_select, tr, trial=True):
        """one mode trial's head on writer w: rdo.rs:870-877, then encoder.rs:1913, 2086-2102, 2132-2136.  trial=False:
        the block as it is coded for real -- encode_block_pre_cdef / encode_block_post_cdef alone; its partition symbol is
        the walker's (encoder.rs:2688, 2781, 2862)"""
        y_mode, uv_mode, ay, auv, au, av, ts = tr
        tbo = TBO(BO(x=bo_x, y=bo_y))
        bs = BS[bsize]
        if trial and bsize >= I_8X8 and bool(c.call_method(bs, "is_sqr", [])):
            F["write_partition"](g, cw, w, tbo, PT[NONE], bs)
        F["write_skip"](g, cw, w, tbo, False)
        F["write_intra_mode_kf"](g, cw, w, tbo, PM[y_mode])
        if bool(c.call_method(PM[y_mode], "is_directional", [])) and bsize >= I_8X8:
            F["write_angle_delta"](g, cw, w, ay, PM[y_mode])
        if bool(has_chroma({}, tbo, bs, xdec, ydec, CS[(xdec, ydec)])):
            F["write_intra_uv_mode"](g, cw, w, PM[uv_mode], PM[y_mode], bs)
            if bool(c.call_method(PM[uv_mode], "is_cfl", [])):
                assert bool(c.call_method(bs, "cfl_allowed", []))
                F["write_cfl_alphas"](g, cw, w, from_alpha({}, au, av))
            if bool(c.call_method(PM[uv_mode], "is_directional", [])) and bsize >= I_8X8:
                F["write_angle_delta"](g, cw, w, auv, PM[uv_mode])
        if tx_mode_select and bsize > I_4X4:
            F["write_tx_size_intra"](g, cw, w, tbo, bs, TxSize[ts])

    def trial(cw, bsize, bo_x, bo_y, xdec, ydec, tms, tr):
        """-> (rate, rng) on a fresh counter and a copy of fc (the reference's rollback)"""
        w = new_counter({})
        t0 = tell(w)
        head(CW(bc=cw.bc, fc=copy.deepcopy(cw.fc)), w, bsize, bo_x, bo_y, xdec, ydec, tms, tr)
        return tell(w) - t0, int(w.rng)

    def chroma_here(bsize, bo_x, bo_y, xdec, ydec):
        return int(bool(has_chroma({}, TBO(BO(x=bo_x, y=bo_y)), BS[bsize], xdec, ydec, CS[(xdec, ydec)])))

    def random_trial(bsize, style=None):
        """a valid trial of the block: CFL only where cfl_allowed, a depth of the block"""
        y_mode = int(rng.integers(0, 13))
        cfl_ok = bool(c.call_method(BS[bsize], "cfl_allowed", []))
        uv_mode = int(rng.integers(0, 14 if cfl_ok else 13))
        au, av = 0, 0
        if uv_mode == CFL:
            while au == 0 and av == 0:
                au, av = int(rng.integers(-16, 17)), int(rng.integers(-16, 17))
                if rng.integers(0, 4) == 0:
                    au = 0
                elif rng.integers(0, 4) == 0:
                    av = 0
        ds = depths(bsize)
        return (y_mode, uv_mode, int(rng.integers(-3, 4)), int(rng.integers(-3, 4)), au, av, ds[int(rng.integers(0, len(ds)))])

    def adapt_at_random(fc, n):
        """what earlier blocks could have left: every head row hit a few times"""
        upd = c.get("update_cdf")
        for f, shape in CDF_FIELDS:
            arr = getattr(fc, f)
            for idx in np.ndindex(*shape[:-1]):
                row = arr
                for i in idx:
                    row = row[i]
                for _ in range(int(rng.integers(0, n))):
                    upd({}, row, int(rng.integers(0, shape[-1])))

    out = {"cdf_fields": np.array([f for f, _ in CDF_FIELDS]), "block_wh": np.array([bs_w, bs_h], np.int32) * 4,
           "tab_max_txsize_rect": np.array(max_rect, np.int32), "tab_sub_tx_size": np.array(sub_map, np.int32),
           "tab_partition_context": np.array(c.const_value("partition_context_lookup").tolist(), np.int32)[:22],
           "tab_is_directional": np.array([int(bool(c.call_method(m, "is_directional", []))) for m in PM[:14]], np.int32),
           "tab_cfl_allowed": np.array([int(bool(c.call_method(b, "cfl_allowed", []))) for b in BS], np.int32),
           "tab_is_sqr": np.array([int(bool(c.call_method(b, "is_sqr", []))) for b in BS], np.int32)}

    # ---------------- (a) single trials on seeded contexts
    PART_VALUES = (31, 30, 28, 24, 16, 0)
    TX_VALUES = (4, 8, 16, 32, 64)
    # (qindex, adapted, cursor row, tile columns, tile rows, sampling)
    SEEDS = ((10, 0, 0, 64, 64, C420), (40, 0, 5, 44, 32, C420), (100, 0, 16, 64, 20, C444), (200, 0, 35, 1024, 64, C420),
             (10, 1, 8, 64, 64, C420), (40, 1, 17, 40, 24, C444), (100, 1, 2, 64, 64, C420), (200, 1, 48, 1024, 52, C444))
    ctxs = []
    for (q, adapted, y0, cols, rows, cs) in SEEDS:
        fc = new_fc({}, q)
        if adapted:
            adapt_at_random(fc, 40)
        bl = Blocks(cols, rows, PM[DC])
        for row in bl.grid:                       # cells nothing may read
            for b in row:
                b.mode, b.skip = PM[int(rng.integers(0, 13))], bool(rng.integers(0, 2))
        lmode, lskip = PM[int(rng.integers(0, 13))], bool(rng.integers(0, 2))
        for b in bl.grid[y0]:                     # the cursor row: whatever bo_x, left_of reads this
            b.mode, b.skip = lmode, lskip
        bc = BC(above_partition_context=R.RSlice([int(v) for v in rng.choice(PART_VALUES, 512)]),
                left_partition_context=R.RSlice([int(v) for v in rng.choice(PART_VALUES, 8)]),
                above_tx_context=R.RSlice([int(v) for v in rng.choice(TX_VALUES, WIDTH)]),
                left_tx_context=R.RSlice([int(v) for v in rng.choice(TX_VALUES, 16)]), blocks=bl)
        ctxs.append((CW(bc=bc, fc=fc), y0, cols, rows, cs))
    out["single_cdf"] = np.stack([pack_fc(cw.fc) for cw, *_ in ctxs])
    nbrs = []
    for cw, y0, cols, rows, cs in ctxs:
        # the row buffers as the cursor row sees them: `above` is the row over it, `left` holds the cursor row's own cell
        # at y0 % 16; every entry nothing may read (the rest of `left`, `above` on a tile's first row, columns past the
        # tile) is seeded garbage
        bc, bl = cw.bc, cw.bc.blocks
        am, ak = rng.integers(0, 13, WIDTH).astype(np.uint8), rng.integers(0, 2, WIDTH).astype(np.uint8)
        lm, lk = rng.integers(0, 13, 16).astype(np.uint8), rng.integers(0, 2, 16).astype(np.uint8)
        if y0 > 0:
            for x in range(cols):
                am[x], ak[x] = int(bl.grid[y0 - 1][x].mode.disc), int(bl.grid[y0 - 1][x].skip)
        lm[y0 % 16], lk[y0 % 16] = int(bl.grid[y0][0].mode.disc), int(bl.grid[y0][0].skip)
        nbrs.append(np.concatenate([np.array([int(v) for v in a], np.uint8) for a in
                                    (bc.above_partition_context, bc.left_partition_context, bc.above_tx_context,
                                     bc.left_tx_context)] + [am, lm, ak, lk]))
    out["single_nbr"] = np.stack(nbrs)

    singles, single_names = [], []

    def single(name, k, bsize, bo_x, tr, tms=1):
        cw, y0, cols, rows, (xdec, ydec) = ctxs[k]
        assert bo_x + 0 < cols and bo_x % min(bs_w[bsize], 16) == 0, (name, bo_x)
        rate, r = trial(cw, bsize, bo_x, y0, xdec, ydec, tms, tr)
        singles.append((k, bo_x, y0, cols, rows, bsize, chroma_here(bsize, bo_x, y0, xdec, ydec), tms) + tuple(tr) +
                       (rate, r, xdec, ydec))
        single_names.append(name)
        print(len(singles), name, "rate", rate, "rng", r, flush=True)

    B = lambda w, h: bs_of[(w, h)]
    T = lambda w, h: tx_of[(w, h)]
    # the traps, by name (tests/test_head_ref.py turns each behaviour off and names these cases)
    for k in (0, 4, 6):
        single("angle same row y=uv D45", k, B(16, 16), 8, (D45, D45, 2, -1, 0, 0, T(16, 16)))
        single("angle same row y=uv V", k, B(32, 32), 8, (V, V, -3, 3, 0, 0, T(16, 16)))
        single("angle two rows", k, B(16, 16), 8, (D45, D67, 2, -1, 0, 0, T(16, 16)))
        single("cfl same row NEG NEG", k, B(16, 16), 4, (DC, CFL, 0, 0, -3, -7, T(8, 8)))
        single("cfl same row POS POS", k, B(8, 8), 4, (PAETH, CFL, 0, 0, 12, 2, T(8, 8)))
        single("cfl two rows NEG POS", k, B(16, 16), 4, (DC, CFL, 0, 0, -3, 7, T(16, 16)))
        single("cfl one alpha ZERO POS", k, B(32, 32), 0, (H, CFL, 1, 0, 0, 16, T(32, 32)))
        single("cfl one alpha NEG ZERO", k, B(32, 32), 8, (SMOOTH, CFL, 0, 0, -1, 0, T(16, 16)))
        single("8x8 w8 rows depth 0", k, B(8, 8), 6, (D135, SMOOTH_V, 1, 0, 0, 0, T(8, 8)))
        single("8x8 w8 rows depth 1", k, B(8, 8), 6, (DC, DC, 0, 0, 0, 0, T(4, 4)))
        single("64x64 cat 3 depth 0", k, B(64, 64), 16, (DC, D203, 0, 2, 0, 0, T(64, 64)))
        single("64x64 cat 3 depth 2", k, B(64, 64), 16, (D113, DC, -2, 0, 0, 0, T(16, 16)))
        single("rect 16x8 no partition depth 1", k, B(16, 8), 4, (D157, D157, 3, 3, 0, 0, T(8, 8)))
        single("rect 8x32 no partition depth 2", k, B(8, 32), 2, (V, H, 0, -2, 0, 0, T(8, 8)))
        single("rect 64x16 depth 1 no cfl", k, B(64, 16), 16, (SMOOTH_H, PAETH, 0, 0, 0, 0, T(32, 16)))
        single("4x16 angle delta no partition", k, B(4, 16), 3, (D67, D45, -1, 1, 0, 0, T(4, 8)))
        single("16x4 angle delta", k, B(16, 4), 4, (H, V, 2, -3, 0, 0, T(16, 4)))
        single("4x4 no partition no angle no tx", k, B(4, 4), 3, (D45, D135, 0, 0, 0, 0, T(4, 4)))
        single("4x4 even column", k, B(4, 4), 2, (D45, D135, 0, 0, 0, 0, T(4, 4)))
        single("4x8 no angle", k, B(4, 8), 5, (V, CFL, 0, 0, 5, -5, T(4, 8)))
        single("8x4 no angle depth 1", k, B(8, 4), 6, (D203, D203, 0, 0, 0, 0, T(4, 4)))
        single("tile left edge", k, B(16, 16), 0, (D45, SMOOTH, 1, 0, 0, 0, T(8, 8)))
        single("no tx_mode_select", k, B(32, 32), 8, (DC, V, 0, 1, 0, 0, T(32, 32)), 0)
    single("column 1020", 3, B(16, 16), 1020, (D45, CFL, -2, 0, 9, 9, T(16, 16)))
    single("column 1023", 3, B(4, 4), 1023, (PAETH, H, 0, 0, 0, 0, T(4, 4)))
    single("column 1022 8x8", 7, B(8, 8), 1022, (V, V, 3, -3, 0, 0, T(4, 4)))
    single("column 1008 64x64", 3, B(64, 64), 1008, (SMOOTH, D45, 0, 1, 0, 0, T(32, 32)))
    # neither rows nor columns: nothing of the partition is written (write_partition returns first)
    single("corner no partition symbol", 5, B(64, 64), 32, (DC, DC, 0, 0, 0, 0, T(64, 64)))
    for i in range(220):
        k = i % len(ctxs)
        cw, y0, cols, rows, (xdec, ydec) = ctxs[k]
        while True:
            bsize = int(rng.choice([b for b in range(22) if bs_w[b] <= 16 and bs_h[b] <= 16]))
            w4 = bs_w[bsize]
            bo_x = int(rng.integers(0, cols // w4)) * w4
            if cols == 1024 and rng.integers(0, 2):
                bo_x = 1024 - w4 * int(rng.integers(1, 4))
            hbs = w4 // 2
            sq = w4 == bs_h[bsize] and w4 >= 2
            if sq and ((bo_x + hbs < cols) != (y0 + hbs < rows)):
                continue                           # an edge arm: PARTITION_NONE is asserted against there
            break
        single("random %d" % i, k, bsize, bo_x, random_trial(bsize), int(rng.integers(0, 8) != 0))
    out["single_rows"] = np.array(singles, np.int64)
    out["single_names"] = np.array(single_names)
    out["single_cols"] = np.array(SINGLE_COLS)

    # ---------------- (c) write_partition alone
    pcases = []
    for k, (cw, y0, cols, rows, cs) in enumerate(ctxs):
        for bsize in (B(8, 8), B(16, 16), B(32, 32), B(64, 64)):
            w4 = bs_w[bsize]
            hbs = w4 // 2
            xs = sorted({0, w4, ((cols - 1) // w4) * w4, ((cols - hbs - 1) // w4) * w4})
            for bo_x in xs:
                if bo_x >= cols:
                    continue
                has_cols, has_rows = bo_x + hbs < cols, y0 + hbs < rows
                if has_rows and has_cols:
                    types = (NONE, HORZ, VERT, SPLIT)
                elif has_cols:
                    types = (SPLIT, HORZ)
                elif has_rows:
                    types = (SPLIT, VERT)
                else:
                    types = (SPLIT,)
                if not (has_rows and has_cols) and (has_rows or has_cols) and bsize == B(8, 8):
                    continue                       # assert!(bsize > BLOCK_8X8)
                for p in types:
                    w = new_counter({})
                    w.rng = 0x8000 if len(pcases) % 3 == 0 else int(rng.integers(0x8000, 0x10000))
                    rng0, t0 = int(w.rng), tell(w)
                    F["write_partition"](g, CW(bc=cw.bc, fc=copy.deepcopy(cw.fc)), w, TBO(BO(x=bo_x, y=y0)), PT[p], BS[bsize])
                    pcases.append((k, bsize, bo_x, y0, cols, rows, p, rng0, tell(w) - t0, int(w.rng)))
    out["part_case_rows"] = np.array(pcases, np.int64)
    out["part_case_cols"] = np.array(PCASE_COLS)
    print("partition cases:", len(pcases), "edge arms:", sum(1 for r in pcases if not (r[2] + bs_w[r[1]] // 2 < r[4] and r[3] + bs_h[r[1]] // 2 < r[5])), flush=True)

    # ---------------- (b) sequences
    RESET = "reset"

    def blk(w, h, x, y, parts=(), upc=None, n_trials=4):
        """parts: the walker's symbols in front ((node w, x, y, type), ..); upc: (node w, x, y, sub w, sub h) behind"""
        return (B(w, h), x, y, tuple(parts), upc, n_trials)

    def none(w, x, y, parts=(), n_trials=4):
        """a square block coded whole: PARTITION_NONE at its own node, the context update behind it"""
        return blk(w, w, x, y, tuple(parts) + ((w, x, y, NONE),), (w, x, y, w, w), n_trials)

    def quad(w, x, y, parts=()):
        s = w >> 2
        return [none(w, x, y, tuple(parts) + ((2 * w, x, y, SPLIT),)), none(w, x + s, y), none(w, x, y + s), none(w, x + s, y + s)]

    BIG = (256, 256)
    SEQUENCES = (
        ("sb32 420", 10, C420, BIG, 1, quad(32, 0, 0) + [RESET] + quad(32, 0, 16)[:3]),
        ("sbrow 444", 40, C444, BIG, 1, [none(64, 0, 0), none(64, 16, 0), RESET, none(64, 0, 16)] +
         quad(32, 16, 16) + [blk(64, 16, 32, 16), blk(64, 16, 32, 20), blk(64, 32, 32, 24),
                             blk(8, 32, 48, 16), blk(8, 32, 50, 16)]),
        ("mixed 420", 100, C420, BIG, 1, [none(64, 0, 0), none(32, 16, 0, ((64, 16, 0, SPLIT),)),
                                          none(16, 24, 0, ((32, 24, 0, SPLIT),)), none(16, 28, 0), none(16, 24, 4),
                                          none(8, 28, 4, ((16, 28, 4, SPLIT),)), none(8, 30, 4), none(8, 28, 6),
                                          blk(4, 4, 30, 6, ((8, 30, 6, SPLIT),)), blk(4, 4, 31, 6), blk(4, 4, 30, 7),
                                          blk(4, 4, 31, 7, (), (8, 30, 6, 4, 4)), none(32, 16, 8), none(32, 24, 8)]),
        ("rect 420", 200, C420, BIG, 1, [blk(64, 32, 0, 0, ((64, 0, 0, HORZ),)), blk(64, 32, 0, 8, (), (64, 0, 0, 64, 32)),
                                         blk(32, 64, 16, 0, ((64, 16, 0, VERT),)), blk(32, 64, 24, 0, (), (64, 16, 0, 32, 64)),
                                         RESET, blk(16, 8, 0, 16, ((64, 0, 16, SPLIT), (32, 0, 16, SPLIT), (16, 0, 16, HORZ))),
                                         blk(16, 8, 0, 18, (), (16, 0, 16, 16, 8)),
                                         blk(8, 16, 4, 16, ((16, 4, 16, VERT),)), blk(8, 16, 6, 16, (), (16, 4, 16, 8, 16)),
                                         blk(8, 4, 0, 20, ((16, 0, 20, SPLIT), (8, 0, 20, HORZ))), blk(8, 4, 0, 21, (), (8, 0, 20, 8, 4)),
                                         blk(4, 8, 2, 20, ((8, 2, 20, VERT),)), blk(4, 8, 3, 20, (), (8, 2, 20, 4, 8)),
                                         none(8, 0, 22), none(8, 2, 22)]),
        ("rect 444", 10, C444, BIG, 1, [blk(32, 16, 0, 0, ((64, 0, 0, SPLIT), (32, 0, 0, HORZ))), blk(32, 16, 0, 4, (), (32, 0, 0, 32, 16)),
                                        blk(16, 32, 8, 0, ((32, 8, 0, VERT),)), blk(16, 32, 12, 0, (), (32, 8, 0, 16, 32)),
                                        blk(4, 8, 0, 8, ((32, 0, 8, SPLIT), (16, 0, 8, SPLIT), (8, 0, 8, VERT))), blk(4, 8, 1, 8, (), (8, 0, 8, 4, 8)),
                                        blk(4, 4, 2, 8, ((8, 2, 8, SPLIT),)), blk(4, 4, 3, 8), blk(4, 4, 2, 9), blk(4, 4, 3, 9, (), (8, 2, 8, 4, 4)),
                                        none(8, 0, 10), none(8, 2, 10), none(16, 4, 8), none(16, 0, 12), none(16, 4, 12)]),
        # tiles whose edges cut superblocks: the walker's SPLIT through the two-entry CDFs, a corner node that writes nothing
        ("edge 420", 40, C420, (22, 10), 1, [none(32, 0, 0, ((64, 0, 0, SPLIT),)), none(32, 8, 0),
                                             blk(16, 8, 0, 8, ((32, 0, 8, SPLIT), (16, 0, 8, HORZ)), (16, 0, 8, 16, 8)),
                                             blk(16, 8, 4, 8, ((16, 4, 8, HORZ),), (16, 4, 8, 16, 8)),
                                             blk(32, 16, 8, 8, ((32, 8, 8, HORZ),), (32, 8, 8, 32, 16)),
                                             none(16, 16, 0, ((64, 16, 0, SPLIT), (32, 16, 0, SPLIT))),
                                             none(8, 20, 0, ((16, 20, 0, SPLIT),)), none(8, 20, 2), none(16, 16, 4),
                                             none(8, 20, 4, ((16, 20, 4, SPLIT),)), none(8, 20, 6),
                                             none(8, 16, 8, ((32, 16, 8, SPLIT), (16, 16, 8, SPLIT))), none(8, 18, 8),
                                             none(8, 20, 8, ((16, 20, 8, SPLIT),))]),
        ("edge 444", 100, C444, (26, 12), 1, [none(32, 0, 0, ((64, 0, 0, SPLIT),)), none(32, 8, 0),
                                              none(16, 0, 8, ((32, 0, 8, SPLIT),)), none(16, 4, 8),
                                              blk(16, 8, 8, 8, ((32, 8, 8, SPLIT), (16, 8, 8, HORZ))), blk(16, 8, 8, 10, (), (16, 8, 8, 16, 8)),
                                              none(8, 12, 8, ((16, 12, 8, SPLIT),)), none(8, 14, 8), none(8, 12, 10), none(8, 14, 10),
                                              none(32, 16, 0, ((64, 16, 0, SPLIT),)),
                                              none(8, 24, 0, ((32, 24, 0, SPLIT), (16, 24, 0, SPLIT))), none(8, 24, 2),
                                              blk(8, 4, 24, 4, ((16, 24, 4, SPLIT), (8, 24, 4, HORZ))), blk(8, 4, 24, 5, (), (8, 24, 4, 8, 4)),
                                              none(8, 24, 6)]),
        ("far 420", 200, C420, (1024, 64), 1, [none(32, 1008, 0, ((64, 1008, 0, SPLIT),)), none(32, 1016, 0), none(16, 1008, 8, ((32, 1008, 8, SPLIT),)),
                                               none(16, 1012, 8), none(16, 1008, 12), none(16, 1012, 12),
                                               none(16, 1016, 8, ((32, 1016, 8, SPLIT),)), none(16, 1020, 8), none(16, 1016, 12),
                                               none(8, 1020, 12, ((16, 1020, 12, SPLIT),)), none(8, 1022, 12),
                                               blk(8, 4, 1020, 14, ((8, 1020, 14, HORZ),)), blk(8, 4, 1020, 15, (), (8, 1020, 14, 8, 4)),
                                               blk(4, 4, 1022, 14, ((8, 1022, 14, SPLIT),)), blk(4, 4, 1023, 14),
                                               blk(4, 4, 1022, 15)]),
        # (one superblock row each: the columns to the left of these blocks are never coded, so a second row would read
        # `left` entries that no block of a real tile could have left)
        ("far 444", 10, C444, (1024, 64), 1, [blk(16, 64, 1008, 0), blk(16, 64, 1012, 0), none(32, 1016, 0),
                                              blk(32, 8, 1016, 8), blk(32, 8, 1016, 10), blk(16, 4, 1016, 12),
                                              blk(16, 4, 1016, 13), blk(16, 4, 1016, 14), blk(16, 4, 1016, 15),
                                              blk(4, 16, 1020, 12), blk(4, 16, 1021, 12), blk(4, 16, 1022, 12),
                                              blk(4, 16, 1023, 12)]),
        ("no tx select 420", 40, C420, BIG, 0, quad(16, 0, 0, ((64, 0, 0, SPLIT), (32, 0, 0, SPLIT))) + [none(32, 8, 0), none(32, 0, 8)]),
    )
    evs, trials, parts, ev_cdf, ev_nbr, ev_names = [], [], [], [], [], []
    seq_meta, seq_cdf0, seq_nbr0, seq_names = [], [], [], []
    for si, (sname, q, (xdec, ydec), (cols, rows), tms, events) in enumerate(SEQUENCES):
        assert len(events) <= 16, (sname, len(events))
        fc = new_fc({}, q)
        bl = Blocks(cols, rows, PM[DC])
        bc = BC(above_partition_context=R.RSlice([0] * 512), left_partition_context=R.RSlice([0] * 8),
                above_tx_context=R.RSlice([0] * WIDTH), left_tx_context=R.RSlice([0] * 16),
                above_coeff_context=R.RSlice([R.RSlice([0] * WIDTH) for _ in range(3)]),
                left_coeff_context=R.RSlice([R.RSlice([0] * 16) for _ in range(3)]), blocks=bl)
        cw = CW(bc=bc, fc=fc)
        seq_cdf0.append(pack_fc(fc))
        seq_nbr0.append(pack_nbr(bc))
        tile_w = new_counter({})        # the tile's writer: what the walker's symbols go to (only their adaptation is kept)
        for step, ev in enumerate(events):
            if ev == RESET:
                reset_left({}, bc, 3)
                evs.append((si, step, 1, 0, 0, 0, 0, 0, len(trials), -1, 0, len(parts), -1, 0, 0, 0))
                ev_names.append("%s/%d reset_left_contexts" % (sname, step))
            else:
                bsize, bo_x, bo_y, pp, upc, n_trials = ev
                assert bo_x < cols and bo_y < rows and bo_x % min(bs_w[bsize], 16) == 0 and bo_y % min(bs_h[bsize], 16) == 0, (sname, step)
                part_off = len(parts)
                for (nw, nx, ny, ptype) in pp:
                    F["write_partition"](g, cw, tile_w, TBO(BO(x=nx, y=ny)), PT[ptype], BS[B(nw, nw)])
                    parts.append((B(nw, nw), nx, ny, ptype))
                trial_off = len(trials)
                # a trap per trial slot where the block allows it: equal directional modes, equal CFL signs
                cfl_ok = bool(c.call_method(BS[bsize], "cfl_allowed", []))
                for j in range(n_trials):
                    tr = random_trial(bsize)
                    if j == 1:
                        m = int(rng.integers(1, 9))
                        tr = (m, m) + tr[2:]
                    if j == 2 and cfl_ok:
                        s = int(rng.choice([-1, 1]))
                        tr = (tr[0], CFL, tr[2], tr[3], s * int(rng.integers(1, 17)), s * int(rng.integers(1, 17)), tr[6])
                    if tr[1] != CFL:
                        tr = tr[:4] + (0, 0) + tr[6:]
                    rate, r = trial(cw, bsize, bo_x, bo_y, xdec, ydec, tms, tr)
                    trials.append(tuple(tr) + (rate, r))
                winner = (si + step) % n_trials
                tr = trials[trial_off + winner][:7]
                # the winner for real (encoder.rs:1900, 1969-1970, 2132-2136; update_tx_size_context for 4x4 is 2166)
                tbo = TBO(BO(x=bo_x, y=bo_y))
                def code(b, tr=tr):                 # set_skip, set_mode, set_tx_size: one for_each each in the reference
                    b.skip, b.mode, b.txsize = False, PM[tr[0]], TxSize[tr[6]]
                bl.for_each(tbo, bs_w[bsize], bs_h[bsize], code)
                head(cw, new_counter({}), bsize, bo_x, bo_y, xdec, ydec, tms, tr, trial=False)
                if tms:
                    upd_tx({}, bc, tbo, BS[bsize], TxSize[tr[6]], False)
                u = (-1, 0, 0, 0)
                if upc is not None:
                    nw, nx, ny, sw, sh = upc
                    upd_part({}, bc, TBO(BO(x=nx, y=ny)), BS[B(sw, sh)], BS[B(nw, nw)])
                    u = (B(sw, sh), B(nw, nw), nx, ny)
                evs.append((si, step, 0, bsize, bo_x, bo_y, chroma_here(bsize, bo_x, bo_y, xdec, ydec), n_trials, trial_off, winner,
                            len(pp), part_off) + u)
                ev_names.append("%s/%d %s @%d,%d" % (sname, step, bs_names[bsize], bo_x, bo_y))
            ev_cdf.append(pack_fc(fc))
            ev_nbr.append(pack_nbr(bc))
            print(len(evs), ev_names[-1], flush=True)
        seq_meta.append((q, xdec, ydec, cols, rows, len(events), tms))
        seq_names.append(sname)
    out.update({"seq_rows": np.array(seq_meta, np.int64), "seq_cols": np.array(SEQ_COLS), "seq_names": np.array(seq_names),
                "seq_cdf0": np.stack(seq_cdf0), "seq_nbr0": np.stack(seq_nbr0),
                "ev_rows": np.array(evs, np.int64), "ev_cols": np.array(EV_COLS), "ev_names": np.array(ev_names),
                "ev_cdf": np.stack(ev_cdf), "ev_nbr": np.stack(ev_nbr),
                "trial_rows": np.array(trials, np.int64), "trial_cols": np.array(TRIAL_COLS),
                "part_rows": np.array(parts, np.int64).reshape(-1, 4), "part_cols": np.array(PART_COLS)})
    assert out["single_cdf"].shape[1] == CDF_LEN and out["single_nbr"].shape[1] == NBR_LEN
    print("singles:", len(singles), "sequences:", len(seq_meta), "events:", len(evs), "trials:", len(trials), flush=True)
    L.save("head_ref.npz", out)


if __name__ == "__main__":
    main()

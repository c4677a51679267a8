#!/usr/bin/env python3
"""tests/golden/mvref_ref.npz: the MV reference stack of an inter block -- find_mvrefs (src/context/block_unit.rs:1423-1442)
over a tile's blocks array -- EXECUTED through tools/rustlite, loaded from the reference where it lies:
  find_mvrefs, setup_mvref_list, scan_row_mbmi, scan_col_mbmi, scan_blk_mbmi, add_ref_mv_candidate,
  add_extra_mv_candidate, find_matching_mv, find_matching_mv_and_update_weight,
  find_matching_comp_mv_and_update_weight, add_offset, find_valid_row_offs, find_valid_col_offs, Block::is_inter
                                                                        src/context/block_unit.rs
  has_tr, BlockSize::width_mi / height_mi / width / height              src/partition.rs
  PredictionMode::has_newmv                                             src/predict.rs
  MotionVector, CandidateMV, RefType::to_index, the constants (REF_CAT_LEVEL, MVREF_ROW_COLS, REFMV_OFFSET, ..).
Restatements (docs/PARITY.md, "MV stack"):
  * TileBlocksMut (src/tiling/tile_blocks.rs: a macro over raw pointers) is `Blocks` below: a real 2-D array of Block
    stand-ins with cols / rows / x / y / frame_cols / frame_rows, indexing by row and by TileBlockOffset (an index past
    the row or the array panics, as the slice does), and for_each's clipping (206-224) behind set_skip, set_block_size,
    set_mode, set_ref_frames and set_motion_vectors (227-277); set_block_size takes n4_w / n4_h from the executed
    width_mi / height_mi.
  * Block::default() (block_unit.rs:194-211) is Blk.__init__: DC_PRED, [INTRA_FRAME; 2], zero vectors, BLOCK_64X64 and
    its executed width_mi / height_mi.
  * FrameInvariants is an object with ref_frame_sign_bias alone; ArrayVec<CandidateMV, 9> is a growable list.
  * The coding order (`walk`): the partition tree of each 64x64 superblock in raster order, a node's children in the
    order of encode_partition_*: NONE, HORZ, VERT, SPLIT, HORZ_4, VERT_4, at a tile edge only what write_partition
    admits (src/context/partition_unit.rs:267-357): SPLIT or HORZ without rows below, SPLIT or VERT without columns to
    the right, SPLIT without both; a block whose origin lies outside the tile is not coded.  The winner of each block is
    prescribed (seeded), stored as encode_block_pre_cdef / encode_block_post_cdef store it (src/encoder.rs:1900,
    1968-1972); an intra winner stores {INTRA_FRAME, NONE_FRAME} and zero vectors (rdo.rs:866-907 codes it so).
  * The tags of the single queries are predicates on the geometry and on the executed results, stated in `tags_of`.
Every blocks array comes from such a walk: no cell is filled at random.  Cases dropped: 0 -- a panic of the executed
text ends the generator.

(a) `seq_* / ev_* / sq_*`: per tile the blocks in coding order; in front of each the stacks of three single references
    and one compound pair, behind it the winner stored; `snap_<k>`: the whole array in front of chosen events and behind
    the last.
(b) `q_*`: single queries on those snapshots at the place of the next block: the block's own size and the smaller
    first blocks the partition could have put there, every single reference and four compound pairs; named by tag.
(c) `has_tr`: has_tr executed at every aligned position of a superblock for the 22 block sizes (-1: not aligned).

Run in the build container:  python tests/golden/gen_mvref_ref.py
"""
import numpy as np

import reflib as L
from reflib import R
from gen_coeff_rate_ref import FILES, CW, BC

DROPPED = 0
INTRA_FRAME, NONE_FRAME = 0, 8
EV_COLS = ("seq", "step", "bsize", "bo_x", "bo_y", "mode", "ref0", "ref1", "mv0_row", "mv0_col", "mv1_row", "mv1_col", "skip",
           "q_off", "n_q", "snap_before")
Q_COLS = ("snap", "seq", "bo_x", "bo_y", "bsize", "ref0", "ref1", "is_compound", "mode_context", "count", "tags")
SEQ_COLS = ("cols", "rows", "tile_x", "tile_y", "frame_cols", "frame_rows", "n_events", "final_snap")
TAGS = ("tie", "full8", "step16", "odd4", "no_up", "no_left", "tr_at_cols", "clamped", "empty", "extra", "processed",
        "double_ref")
SIGN_BIAS = (0, 0, 0, 0, 1, 1, 1)              # fi.ref_frame_sign_bias: the three backward references


def main():
    c = L.crate(*FILES)
    L.load_v_frame_types(c)
    c.load("context/superblock_unit.rs")
    MV = L.struct(c, "MotionVector")
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    RT = [L.enum(c, "RefType", v[0]) for v in c.enums["RefType"].variants]
    PM = [L.enum(c, "PredictionMode", v[0]) for v in c.enums["PredictionMode"].variants]
    assert [v[0] for v in c.enums["RefType"].variants][::8] == ["INTRA_FRAME", "NONE_FRAME"] and len(PM) == 34
    bs_names = [v[0] for v in c.enums["BlockSize"].variants][:22]
    BS = [L.enum(c, "BlockSize", n) for n in bs_names]
    bs_w = [int(c.call_method(b, "width_mi", [])) for b in BS]
    bs_h = [int(c.call_method(b, "height_mi", [])) for b in BS]
    bs_of = {(w, h): i for i, (w, h) in enumerate(zip(bs_w, bs_h))}
    B64 = bs_of[(16, 16)]
    find = c.get("find_mvrefs", owner="ContextWriter")
    has_tr = c.get("has_tr")
    rng = np.random.default_rng(20261104)

    class Blk:
        _rname = "Block"

        def __init__(self):                                   # Block::default()
            self.mode, self.skip, self.bsize = PM[0], False, BS[B64]
            self.ref_frames = R.RSlice([RT[INTRA_FRAME], RT[INTRA_FRAME]])
            self.mv = R.RSlice([MV(row=0, col=0), MV(row=0, col=0)])
            self.n4_w, self.n4_h = bs_w[B64], bs_h[B64]

    class Blocks:
        def __init__(self, cols, rows, x, y, frame_cols, frame_rows):
            self.grid = [R.RSlice([Blk() for _ in range(cols)]) for _ in range(rows)]
            self._g = (cols, rows, x, y, frame_cols, frame_rows)

        cols = lambda self: self._g[0]
        rows = lambda self: self._g[1]
        x = lambda self: self._g[2]
        y = lambda self: self._g[3]
        frame_cols = lambda self: self._g[4]
        frame_rows = lambda self: self._g[5]

        def __getitem__(self, i):
            if isinstance(i, int):
                if not 0 <= i < self.rows():
                    raise R.Panic("assertion failed: index < self.rows")
                return self.grid[i]
            return self[int(i._0.y)][int(i._0.x)]             # RSlice panics past the row

        def for_each(self, bo_x, bo_y, bsize, f):             # tile_blocks.rs:206-224
            bw, bh = bs_w[bsize], bs_h[bsize]
            if bo_x + bw >= self.cols():
                bw = self.cols() - bo_x
            for y in range(bh):
                if bo_y + y >= self.rows():
                    continue
                for k in range(bo_x, bo_x + bw):
                    f(self.grid[bo_y + y][k])

        def set_skip(self, x, y, bsize, skip):
            self.for_each(x, y, bsize, lambda b: setattr(b, "skip", skip))

        def set_block_size(self, x, y, bsize):
            def f(b):
                b.bsize, b.n4_w, b.n4_h = BS[bsize], bs_w[bsize], bs_h[bsize]
            self.for_each(x, y, bsize, f)

        def set_mode(self, x, y, bsize, mode):
            self.for_each(x, y, bsize, lambda b: setattr(b, "mode", PM[mode]))

        def set_ref_frames(self, x, y, bsize, r):
            self.for_each(x, y, bsize, lambda b: setattr(b, "ref_frames", R.RSlice([RT[r[0]], RT[r[1]]])))

        def set_motion_vectors(self, x, y, bsize, mvs):
            self.for_each(x, y, bsize, lambda b: setattr(b, "mv", R.RSlice([MV(row=mvs[0][0], col=mvs[0][1]),
                                                                          MV(row=mvs[1][0], col=mvs[1][1])])))

        def pack(self):
            out = np.zeros((self.rows(), self.cols(), 8), np.int16)
            for y, row in enumerate(self.grid):
                for x, b in enumerate(row):
                    out[y, x] = (int(b.mv[0].row), int(b.mv[0].col), int(b.mv[1].row), int(b.mv[1].col),
                                 int(b.ref_frames[0].disc) | (int(b.ref_frames[1].disc) << 8),
                                 int(b.mode.disc) | (int(b.n4_w) << 8), int(b.n4_h) | (int(b.bsize.disc) << 8), int(b.skip))
            return out.view(np.uint8).reshape(self.rows(), self.cols(), 16)

    class FI:
        _rname = "FrameInvariants"
        ref_frame_sign_bias = R.RSlice([bool(v) for v in SIGN_BIAS])

    def stack_of(bl, x, y, bsize, refs, comp):
        """find_mvrefs executed -> (mode_context, [(this row, this col, comp row, comp col, weight), ..])"""
        st = R.RSlice([])
        ctx = find({"T": "u8"}, CW(bc=BC(blocks=bl), fc=None), TBO(BO(x=x, y=y)), R.RSlice([RT[refs[0]], RT[refs[1]]]), st,
                   BS[bsize], FI(), bool(comp))
        return int(ctx), [(int(s.this_mv.row), int(s.this_mv.col), int(s.comp_mv.row), int(s.comp_mv.col), int(s.weight))
                          for s in st]

    def walk(cols, rows, split_bias, busy=False):
        """the blocks of a tile in coding order (see the module text) -> [(bsize, x, y), ..].  busy: rows 0 .. 7 down to
        4x4, 32x32 blocks below them -- eight distinct neighbours over one block, the full stack"""
        out = []

        def emit(w, h, x, y):
            if x < cols and y < rows:
                out.append((bs_of[(w, h)], x, y))

        def node(bs, x, y):
            if x >= cols or y >= rows:
                return
            hbs = bs // 2
            has_cols, has_rows = x + hbs < cols, y + hbs < rows
            if busy:
                kind = "SPLIT" if (bs == 16 or y < 8) else "NONE"
            elif bs == 16 and cols >= 48 and whole_sb[0] % 6 in (1, 3, 5):
                kind = {1: "NONE", 3: "HORZ_4", 5: "VERT_4"}[whole_sb[0] % 6]      # in turn: 64x64, four 64x16, four 16x64
            elif has_cols and has_rows:
                opts = ["NONE", "HORZ", "VERT", "SPLIT"] + (["HORZ_4", "VERT_4"] if bs >= 4 else [])
                p = np.array([1.0, 1.0, 1.0, split_bias] + ([0.7, 0.7] if bs >= 4 else []))
                kind = opts[int(rng.choice(len(opts), p=p / p.sum()))]
            elif has_cols:
                kind = "HORZ" if rng.integers(0, 3) == 0 else "SPLIT"
            elif has_rows:
                kind = "VERT" if rng.integers(0, 3) == 0 else "SPLIT"
            else:
                kind = "SPLIT"
            if bs == 16 and cols >= 48:
                whole_sb[0] += 1                           # the superblocks of a tile three wide, counted
            if kind == "NONE":
                emit(bs, bs, x, y)
            elif kind == "HORZ":
                emit(bs, hbs, x, y), emit(bs, hbs, x, y + hbs)
            elif kind == "VERT":
                emit(hbs, bs, x, y), emit(hbs, bs, x + hbs, y)
            elif kind == "HORZ_4":
                for k in range(4):
                    emit(bs, bs // 4, x, y + k * (bs // 4))
            elif kind == "VERT_4":
                for k in range(4):
                    emit(bs // 4, bs, x + k * (bs // 4), y)
            elif bs == 2:
                for (dx, dy) in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    emit(1, 1, x + dx, y + dy)
            else:
                for (dx, dy) in ((0, 0), (hbs, 0), (0, hbs), (hbs, hbs)):
                    node(hbs, x + dx, y + dy)

        for sy in range(0, rows, 16):
            for sx in range(0, cols, 16):
                node(16, sx, sy)
        return out

    whole_sb = [0]
    POOL = ((8, -16), (8, -16), (-40, 24), (0, 0), (12, 12), (-3, 5), (64, -64), (9, -16))

    def some_mv(big):
        if big and rng.integers(0, 12) == 0:               # what the final clamp moves
            return (int(rng.choice([-1, 1])) * int(rng.integers(3000, 12000)), int(rng.choice([-1, 1])) * int(rng.integers(3000, 12000)))
        if rng.integers(0, 3):
            return POOL[int(rng.integers(0, len(POOL)))]
        return (int(rng.integers(-80, 81)), int(rng.integers(-80, 81)))

    def winner(intra_share, busy=False):
        """(mode, (ref0, ref1), ((row, col), (row, col)), skip)"""
        if busy:                                            # one reference, vectors all different
            return (int(rng.choice([14, 19])), (1, NONE_FRAME), ((int(rng.integers(-2000, 2000)), int(rng.integers(-2000, 2000))), (0, 0)), 0)
        u = rng.random()
        skip = int(rng.integers(0, 4) == 0)
        if u < intra_share:
            return (int(rng.integers(0, 13)), (INTRA_FRAME, NONE_FRAME), ((0, 0), (0, 0)), 0)
        if u < intra_share + (1 - intra_share) * 0.65:
            ref = int(rng.choice([1, 1, 1, 4, 4, 7, 7, 2]))
            return (int(rng.choice([14, 15, 18, 19, 19])), (ref, NONE_FRAME), (some_mv(True), (0, 0)), skip)
        refs = ((1, 7), (1, 7), (1, 7), (1, 4), (4, 7), (1, 1))[int(rng.integers(0, 6))]
        return (int(rng.choice([20, 21, 24, 32, 33])), refs, (some_mv(True), some_mv(False)), skip)

    def tags_of(bl, x, y, bsize, refs, comp, ctx, st):
        """the names a single query goes by: predicates on the geometry and the executed result"""
        cols, rows, w, h = bl.cols(), bl.rows(), bs_w[bsize], bs_h[bsize]
        t = set()
        if any(a[4] == b[4] and a[:4] != b[:4] for a, b in zip(st, st[1:])):
            t.add("tie")
        if len(st) == 8:
            t.add("full8")
        if w == 16 or h == 16:
            t.add("step16")
        if (w == 1 and x & 1) or (h == 1 and y & 1):
            t.add("odd4")
        if y == 0:
            t.add("no_up")
        if x == 0:
            t.add("no_left")
        if x + w == cols and y > 0:
            t.add("tr_at_cols")
        # the clamp's bounds around the block's place in the frame (block_unit.rs:1385-1415), restated
        fx, fy = bl.x() + x, bl.y() + y
        xb = (-fx * 32 - 128 - w * 32, (bl.frame_cols() - fx - w) * 32 + 128 + w * 32)
        yb = (-fy * 32 - 128 - h * 32, (bl.frame_rows() - fy - h) * 32 + 128 + h * 32)
        if any(e[0] in yb or e[2] in yb or e[1] in xb or e[3] in xb for e in st):
            t.add("clamped")
        if not st:
            t.add("empty")
        if st and st[-1][4] == 2:                          # a weight of exactly 2 is the extra search's
            t.add("extra")
        # processed_rows / processed_cols can skip a far row or column only behind a neighbour at least as wide (tall) as
        # the block and 16 units or more deep, in one of the rows (columns) a scan starts from
        if w >= 2 and any(bl.grid[y - k][xx].n4_w >= w and bl.grid[y - k][xx].n4_h >= 4
                          for k in range(1, 5) if y - k >= 0 for xx in (x, x + 1) if xx < cols):
            t.add("processed")
        if h >= 2 and any(bl.grid[yy][x - k].n4_h >= h and bl.grid[yy][x - k].n4_w >= 4
                          for k in range(1, 5) if x - k >= 0 for yy in (y, y + 1) if yy < rows):
            t.add("processed")
        for yy, xx in ((y - 1, x), (y, x - 1)):
            if yy >= 0 and xx >= 0:
                b = bl.grid[yy][xx]
                if int(b.mode.disc) >= 14 and int(b.ref_frames[0].disc) == int(b.ref_frames[1].disc) == refs[0]:
                    t.add("double_ref")
        return sum(1 << TAGS.index(n) for n in t)

    out = {"block_wh4": np.array([bs_w, bs_h], np.int32), "tag_names": np.array(TAGS), "dropped": np.array(DROPPED),
           "sign_bias": np.array(SIGN_BIAS + (0,), np.uint8)}

    # ---------------- (c) has_tr at every aligned position of a superblock
    tr = np.full((22, 16, 16), -1, np.int8)
    for b in range(22):
        for y in range(0, 16, min(bs_h[b], 16)):
            for x in range(0, 16, min(bs_w[b], 16)):
                tr[b, y, x] = int(bool(has_tr({}, TBO(BO(x=x, y=y)), BS[b])))
    out["has_tr"] = tr

    # ---------------- (a) sequences, (b) single queries on their snapshots
    # (name, cols, rows, tile_x, tile_y, frame_cols, frame_rows, split bias, intra share, a snapshot every .. events)
    TILES = (("edge 22x10 whole frame", 22, 10, 0, 0, 22, 10, 2.0, 0.2, 4),
             ("edge 26x12 at 32,16", 26, 12, 32, 16, 64, 40, 2.5, 0.15, 5),
             ("sb 16x16", 16, 16, 0, 0, 16, 16, 2.0, 0.2, 3),
             ("edge 22x10 frame corner", 22, 10, 16, 16, 38, 26, 1.5, 0.1, 3),
             ("intra 16x16", 16, 16, 0, 0, 48, 16, 1.5, 0.9, 4),
             ("small 26x12", 26, 12, 0, 8, 26, 20, 4.0, 0.1, 6),
             ("big 48x32", 48, 32, 0, 0, 48, 32, 1.0, 0.1, 3),
             ("busy 16x16", 16, 16, 0, 0, 16, 16, 0.0, 0.0, 37))
    SEQ_QUERIES = (((1, NONE_FRAME), 0), ((4, NONE_FRAME), 0), ((7, NONE_FRAME), 0), ((1, 7), 1))
    PAIRS = ((1, 7), (1, 4), (4, 7), (1, 1))
    evs, sq_rows, sq_stack, q_rows, q_stack, q_names, seq_rows, seq_names, snaps = [], [], [], [], [], [], [], [], []

    def pad(st):
        a = np.zeros((9, 5), np.int32)
        if st:
            a[:len(st)] = st
        return a

    for si, (name, cols, rows, tx, ty, fc, fr, split_bias, intra_share, every) in enumerate(TILES):
        bl = Blocks(cols, rows, tx, ty, fc, fr)
        busy = name.startswith("busy")
        order = walk(cols, rows, split_bias, busy)
        for step, (bsize, x, y) in enumerate(order):
            snap_before = -1
            if step % every == 0 or (busy and bs_w[bsize] >= 8):
                snap_before = len(snaps)
                snaps.append(bl.pack())
                w, h = bs_w[bsize], bs_h[bsize]
                # the block itself and the smaller first blocks the partition could have put at this origin
                sizes = [bsize] + [bs_of[s] for s in ((max(w // 2, 1), h), (w, max(h // 2, 1)), (max(w // 2, 1), max(h // 2, 1)),
                                                      (max(w // 4, 1), h), (w, max(h // 4, 1))) if s in bs_of and s != (w, h)]
                for b in dict.fromkeys(sizes):
                    for refs, comp in [((r, NONE_FRAME), 0) for r in range(1, 8)] + [(p, 1) for p in PAIRS]:
                        ctx, st = stack_of(bl, x, y, b, refs, comp)
                        tg = tags_of(bl, x, y, b, refs, comp, ctx, st)
                        q_rows.append((snap_before, si, x, y, b, refs[0], refs[1], comp, ctx, len(st), tg))
                        q_stack.append(pad(st))
                        q_names.append("%s/%d %s @%d,%d refs %d,%d [%s]" % (name, step, bs_names[b], x, y, refs[0], refs[1],
                                                                          " ".join(n for k, n in enumerate(TAGS) if tg >> k & 1)))
            q_off = len(sq_rows)
            for refs, comp in SEQ_QUERIES:
                ctx, st = stack_of(bl, x, y, bsize, refs, comp)
                sq_rows.append((refs[0], refs[1], comp, ctx, len(st)))
                sq_stack.append(pad(st))
            mode, refs, mvs, skip = winner(intra_share, busy)
            bl.set_skip(x, y, bsize, bool(skip))            # encoder.rs:1900, 1968-1972
            bl.set_block_size(x, y, bsize)
            bl.set_mode(x, y, bsize, mode)
            bl.set_ref_frames(x, y, bsize, refs)
            bl.set_motion_vectors(x, y, bsize, mvs)
            evs.append((si, step, bsize, x, y, mode, refs[0], refs[1], mvs[0][0], mvs[0][1], mvs[1][0], mvs[1][1], skip, q_off,
                        len(SEQ_QUERIES), snap_before))
        seq_rows.append((cols, rows, tx, ty, fc, fr, len(order), len(snaps)))
        snaps.append(bl.pack())
        seq_names.append(name)
        print(name, "blocks:", len(order), "single queries so far:", len(q_rows), flush=True)

    q = np.array(q_rows, np.int64)
    coded = {e[2] for e in evs}
    assert coded == {b for b in range(22) if max(bs_w[b], bs_h[b]) <= 16}, "a block size is never coded: %r" % sorted(coded)
    for k, n in enumerate(TAGS):
        print("tag %-15s %d" % (n, int(((q[:, 10] >> k) & 1).sum())))
        assert ((q[:, 10] >> k) & 1).sum() >= 3, "no case for " + n
    ctxs = sorted(set(int(v) for v in q[:, 8]) | set(int(r[3]) for r in sq_rows))
    print("mode_context values:", ctxs)
    assert set(ctxs) >= {0, 17, 33, 50, 51, 66, 67, 84, 85}, "a mode_context arm has no case"
    tr_q = {(int(tr[r[4], r[3] & 15, r[2] & 15]), bool(r[2] + bs_w[r[4]] == TILES[r[1]][1])) for r in q_rows}
    print("has_tr x at-the-right-edge over the single queries:", sorted(tr_q))
    out.update({"seq_rows": np.array(seq_rows, np.int64), "seq_cols": np.array(SEQ_COLS), "seq_names": np.array(seq_names),
                "ev_rows": np.array(evs, np.int64), "ev_cols": np.array(EV_COLS),
                "sq_rows": np.array(sq_rows, np.int64), "sq_stack": np.stack(sq_stack),
                "q_rows": q, "q_cols": np.array(Q_COLS), "q_stack": np.stack(q_stack), "q_names": np.array(q_names),
                "n_snaps": np.array(len(snaps))})
    for k, s in enumerate(snaps):
        out["snap_%d" % k] = s
    print("sequences:", len(seq_rows), "events:", len(evs), "sequence queries:", len(sq_rows), "single queries:", len(q_rows),
          "snapshots:", len(snaps), "dropped:", DROPPED, flush=True)
    L.save("mvref_ref.npz", out)


if __name__ == "__main__":
    main()

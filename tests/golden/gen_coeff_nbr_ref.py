#!/usr/bin/env python3
"""tests/golden/coeff_nbr_ref.npz: the coefficient neighbour contexts of the reference's BlockContext carried from block
to block -- write_coeffs_lv_map (src/context/block_unit.rs:1783-1857, with get_txb_ctx 442-526 and set_coeff_context
333-348 inside it), reset_skip_context (src/context/partition_unit.rs:434-469) and reset_left_contexts
(src/context/block_unit.rs:394-401) EXECUTED through tools/rustlite over SEQUENCES of up to 12 blocks at real positions
of a tile in coding order, on ONE BlockContext (above_coeff_context[3][1024], left_coeff_context[3][16]) and ONE `fc` per
sequence, with nothing re-randomised between the blocks: what r1_coeff_nbr_gather_batch has to cut and
r1_coeff_nbr_store_batch has to leave in an R1CoeffNbrContext, with r1_coeff_cdf_adapt_batch's CDF context beside it.

Modelled on gen_coeff_cdf_ref.py (the same files, stand-ins and restatements, stated there and in
gen_coeff_rate_block_ref.py): per coded block the luma transform blocks, then U's, then V's (src/encoder.rs:2276-2311,
2352-2403, 2440-2476, 2513-2561) on a fresh WriterBase<WriterCounter> whose rng alone is set to the block's start value; a
transform block whose origin lies at or beyond the tile's mi_width / mi_height is not coded (encoder.rs:1441), one that
straddles the frame edge is coded with frame_clipped_txw / txh (1561-1566).  The tile lies at the frame's origin.
A skipped block calls reset_skip_context alone; a "reset" row calls reset_left_contexts(3).

Stored per row (`case_rows`: the columns of tests/coeff_cdf_model.py, then bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b,
skip, kind (0 block, 1 reset_left_contexts)): the inputs (`case_qc`, `case_eobs`, `case_ctx_in`), the rate, the final rng,
the 96 context bytes behind it (`case_ctx_out`) and the WHOLE arrays behind it (`case_above` [row][3][1024], `case_left`
[row][3][16]); per sequence the arrays in front (`seq_above`, `seq_left`: zero, or seeded around the blocks so that bytes
outside a span show when they move) and the packed CDF context in front and behind (`seq_ctx` [sequence][2][3930]).

The sequences are chosen for where a gather or a scatter can go wrong (the names say which):
  sb32       the four 32x32 blocks of a superblock, then its right neighbour: `left` is consumed across the boundary
  sbrow      a second superblock row behind reset_left_contexts
  mixed      sizes from 64x64 down to 4x4 in partition order
  sub8       4x4 / 4x8 / 8x4 at odd and even offsets: chroma carried or not, the one-unit chroma shift
  4x16       4x16 and 16x4 in 4:2:0: an empty chroma grid
  skip       skipped blocks between coded ones, a skipped 4x16 at an even offset among them (three planes reset)
  edge       a tile whose mi_width / mi_height cut the last block: uncoded transform blocks pass through, coded ones
             write their span past mi_width
  far        blocks at bo_x >= 1008: a 16-entry window meets entry 1023
  zero       all-zero eobs
  rect       the 1:2 and 1:4 sizes
4:2:0, 4:2:2 and 4:4:4; intra and inter; coefficients are i16 (cb 2) and i32 (cb 4) by sequence.

Run in the build container:  python tests/golden/gen_coeff_nbr_ref.py [--stop-before "far 444"]
(the option is for the mutation checks of docs/PARITY.md: it ends the run in front of a sequence a mutated reference
panics in; `far 444` stands last for that reason)
"""
import sys

import numpy as np

import reflib as L
from reflib import R
from gen_coeff_rate_ref import FILES, CW, BC
from gen_coeff_cdf_ref import TX_W, TX_H, CS_NAME, COLS, FIELD_NAMES, nest

EXTRA_COLS = ("bo_x", "bo_y", "mi_width", "mi_height", "w_in_b", "h_in_b", "skip", "kind")
MAX_ROWS = 12
WIDTH = 1024
C420, C422, C444 = (1, 1), (1, 0), (0, 0)
RESET = "reset"
# a block: (bw, bh, luma tx_size, bo_x, bo_y, is_inter, skip, all-zero eobs)
B = lambda bw, bh, ts, x, y, inter=0, skip=0, zero=0: (bw, bh, ts, x, y, inter, skip, zero)
BIG = (4096, 4096, 4096, 4096)          # (mi_width, mi_height, w_in_b, h_in_b): no edge near


def quad(size, ts, x, y, inter=0):
    """the four size x size blocks of the 2*size square at (x, y), in partition order"""
    s = size >> 2
    return [B(size, size, ts, x + dx * s, y + dy * s, inter) for dy in (0, 1) for dx in (0, 1)]


# (name, sampling, reduced set, coefficient bytes, seeded arrays, tile geometry, rows)
SEQUENCES = (
    ("sb32 420", C420, 0, 2, 0, BIG, quad(32, 3, 0, 0) + [B(32, 32, 3, 16, 0), B(32, 32, 2, 24, 0, 1), B(32, 32, 3, 16, 8)]),
    ("sb32 444 inter", C444, 0, 4, 1, BIG, quad(32, 3, 16, 0, 1) + [B(32, 32, 3, 32, 0, 1), B(32, 32, 2, 40, 0), B(32, 32, 3, 32, 8, 1)]),
    ("sb32 422", C422, 1, 2, 1, BIG, quad(32, 3, 0, 16) + [B(32, 32, 3, 16, 16), B(32, 32, 2, 24, 16, 1)]),
    ("sbrow 420", C420, 0, 2, 0, BIG, [B(64, 64, 4, 0, 0), B(64, 64, 3, 16, 0, 1), RESET, B(64, 64, 4, 0, 16), B(32, 32, 3, 16, 16),
                                      B(32, 32, 3, 24, 16, 1), B(32, 32, 2, 16, 24)]),
    ("sbrow 444 inter", C444, 1, 4, 1, BIG, quad(32, 3, 0, 0, 1) + [RESET] + quad(32, 2, 0, 16, 1) + [RESET, B(16, 16, 2, 0, 32)]),
    ("sbrow 422", C422, 0, 2, 1, BIG, [B(64, 64, 4, 0, 0), B(64, 32, 12, 16, 0), B(64, 32, 12, 16, 8, 1), RESET, B(64, 64, 4, 0, 16),
                                      B(32, 16, 10, 16, 16)]),
    ("mixed 420", C420, 0, 2, 1, BIG, [B(64, 64, 4, 0, 0), B(32, 32, 3, 16, 0), B(16, 16, 2, 24, 0), B(16, 16, 1, 28, 0, 1), B(16, 16, 2, 24, 4),
                                      B(8, 8, 1, 28, 4), B(8, 8, 0, 30, 4, 1), B(8, 8, 1, 28, 6), B(4, 4, 0, 30, 6), B(4, 4, 0, 31, 6),
                                      B(4, 4, 0, 30, 7, 1), B(4, 4, 0, 31, 7)]),
    ("mixed 444", C444, 0, 4, 0, BIG, [B(64, 64, 4, 16, 0, 1), B(32, 32, 3, 32, 0), B(16, 16, 2, 40, 0), B(8, 8, 1, 44, 0, 1), B(4, 4, 0, 46, 0),
                                      B(4, 4, 0, 47, 0, 1), B(4, 4, 0, 46, 1), B(4, 4, 0, 47, 1), B(8, 8, 1, 44, 2), B(16, 16, 1, 40, 4)]),
    ("mixed 422", C422, 0, 2, 0, BIG, [B(64, 64, 4, 0, 0), B(32, 32, 3, 16, 0, 1), B(16, 16, 2, 24, 0), B(8, 8, 1, 28, 0), B(4, 4, 0, 30, 0),
                                      B(4, 4, 0, 31, 0, 1), B(8, 4, 6, 30, 1), B(16, 8, 8, 28, 2), B(16, 4, 14, 24, 4, 1)]),
    ("sub8 420", C420, 0, 2, 1, BIG, [B(4, 4, 0, 4, 0), B(4, 4, 0, 5, 0), B(4, 4, 0, 4, 1, 1), B(4, 4, 0, 5, 1), B(4, 8, 5, 6, 0), B(4, 8, 5, 7, 0, 1),
                                     B(8, 4, 6, 4, 2), B(8, 4, 6, 4, 3, 1), B(8, 8, 1, 6, 2), B(8, 8, 0, 8, 0, 1), B(4, 4, 0, 10, 0), B(4, 4, 0, 11, 0)]),
    ("sub8 422", C422, 1, 4, 1, BIG, [B(4, 4, 0, 2, 4), B(4, 4, 0, 3, 4, 1), B(4, 4, 0, 2, 5), B(4, 4, 0, 3, 5), B(8, 4, 6, 4, 4), B(8, 4, 6, 4, 5, 1),
                                     B(8, 8, 1, 6, 4), B(16, 4, 14, 8, 4)]),
    ("sub8 444 inter", C444, 0, 2, 0, BIG, [B(4, 4, 0, 0, 14, 1), B(4, 4, 0, 1, 14, 1), B(4, 8, 5, 2, 14, 1), B(8, 4, 6, 4, 14, 1), B(8, 4, 6, 4, 15),
                                           B(4, 4, 0, 0, 15, 1), B(4, 16, 13, 6, 12, 1), B(8, 8, 1, 8, 14)]),
    ("4x16 420", C420, 0, 2, 1, BIG, [B(4, 16, 13, 8, 0), B(4, 16, 13, 9, 0, 1), B(4, 16, 13, 10, 0), B(4, 16, 13, 11, 0), B(16, 4, 14, 12, 0),
                                     B(16, 4, 14, 12, 1, 1), B(16, 4, 14, 12, 2), B(16, 4, 14, 12, 3), B(16, 16, 2, 8, 4), B(16, 16, 2, 12, 4, 1)]),
    ("4x16 420 inter", C420, 1, 4, 0, BIG, [B(16, 16, 2, 0, 0, 1), B(4, 16, 13, 4, 0, 1), B(4, 16, 13, 5, 0, 1), B(16, 4, 14, 0, 4, 1), B(16, 4, 14, 0, 5, 1),
                                           B(8, 8, 1, 4, 4, 1), B(8, 16, 7, 6, 0, 1)]),
    ("skip 420", C420, 0, 2, 1, BIG, [B(16, 16, 2, 0, 0), B(16, 16, 2, 4, 0, 0, 1), B(16, 16, 2, 0, 4, 1), B(4, 16, 13, 4, 4, 0, 1), B(4, 16, 13, 5, 4, 0, 1),
                                     B(4, 16, 13, 6, 4), B(4, 16, 13, 7, 4, 1), B(8, 8, 1, 8, 0), B(4, 4, 0, 10, 0, 0, 1), B(4, 4, 0, 11, 0), B(4, 4, 0, 10, 1, 0, 1),
                                     B(4, 4, 0, 11, 1, 0, 1)]),
    ("skip 444", C444, 0, 4, 1, BIG, [B(32, 32, 3, 0, 0), B(32, 32, 3, 8, 0, 1, 1), B(16, 16, 2, 0, 8), B(16, 16, 2, 4, 8, 0, 1), B(16, 4, 14, 0, 12, 1, 1),
                                     B(16, 4, 14, 0, 13), B(8, 8, 1, 4, 12), B(4, 8, 5, 6, 12, 0, 1), B(4, 8, 5, 7, 12)]),
    ("skip 422", C422, 0, 2, 1, BIG, [B(16, 16, 2, 4, 8), B(16, 8, 8, 8, 8, 0, 1), B(16, 8, 8, 8, 10, 1), B(8, 4, 6, 12, 8, 0, 1), B(4, 4, 0, 14, 8, 0, 1),
                                     B(4, 4, 0, 15, 8), B(16, 4, 14, 12, 9, 1, 1), B(8, 8, 1, 12, 10)]),
    ("edge 420", C420, 0, 2, 1, (22, 10, 22, 10), [B(32, 32, 2, 0, 0), B(32, 32, 2, 8, 0, 1), B(32, 32, 2, 16, 0), B(32, 32, 2, 0, 8), B(32, 32, 3, 8, 8),
                                                  B(32, 32, 1, 16, 8, 1)]),
    ("edge 444 inter", C444, 0, 4, 1, (21, 7, 22, 8), [B(16, 16, 1, 12, 0, 1), B(16, 16, 1, 16, 0, 1), B(16, 16, 2, 20, 0, 1), B(16, 16, 0, 12, 4, 1),
                                                      B(16, 16, 1, 16, 4), B(16, 16, 0, 20, 4, 1)]),
    ("edge 422", C422, 0, 2, 0, (28, 14, 30, 14), [B(64, 64, 2, 0, 0), B(64, 64, 2, 16, 0, 1), B(32, 16, 1, 16, 12)]),
    ("far 420", C420, 0, 2, 1, (1024, 64, 1024, 64), [B(32, 32, 3, 1008, 0), B(32, 32, 3, 1016, 0, 1), B(16, 16, 2, 1008, 8), B(16, 16, 2, 1012, 8), B(16, 16, 2, 1016, 8),
                                                     B(16, 16, 2, 1020, 8, 1), B(4, 4, 0, 1022, 12), B(4, 4, 0, 1023, 12), B(4, 4, 0, 1022, 13), B(4, 4, 0, 1023, 13)]),
    ("zero 420", C420, 0, 2, 1, BIG, [B(16, 16, 2, 4, 0), B(16, 16, 1, 8, 0, 0, 0, 1), B(16, 16, 2, 12, 0, 1, 0, 1), B(16, 16, 2, 4, 4), B(8, 8, 1, 8, 4, 0, 0, 1),
                                     B(4, 4, 0, 11, 5, 1, 0, 1), B(16, 16, 2, 12, 4)]),
    ("zero 444 inter", C444, 1, 4, 1, BIG, [B(8, 8, 1, 2, 2, 1), B(8, 8, 1, 4, 2, 1, 0, 1), B(8, 8, 0, 6, 2, 1, 0, 1), B(8, 8, 1, 2, 4, 1), B(32, 32, 3, 8, 0, 1, 0, 1),
                                           B(8, 8, 1, 4, 4, 1)]),
    ("rect 420 inter", C420, 0, 4, 0, BIG, [B(64, 32, 12, 0, 0, 1), B(64, 32, 12, 0, 8, 1), B(32, 64, 11, 16, 0, 1), B(16, 64, 17, 24, 0, 1), B(16, 64, 17, 28, 0),
                                           RESET, B(64, 16, 18, 0, 16, 1), B(32, 8, 16, 0, 20), B(32, 8, 16, 0, 22, 1), B(8, 32, 15, 8, 24, 1), B(16, 32, 9, 12, 24), B(32, 16, 10, 16, 16, 1)]),
    ("far 444", C444, 0, 4, 1, (1024, 64, 1024, 64), [B(16, 16, 2, 1016, 0, 1), B(16, 16, 2, 1020, 0), B(4, 16, 13, 1022, 4), B(4, 16, 13, 1023, 4, 1),
                                                     B(8, 8, 1, 1020, 4, 0, 1), RESET, B(64, 64, 4, 1008, 16)]),
)


def main():
    c = L.crate(*FILES)
    L.load_v_frame_types(c)
    try:
        c.load("context/partition_unit.rs")
    except Exception as e:              # docs/PARITY.md says what was loaded in its place
        print("partition_unit.rs does not load whole (%s: %s): loading reset_skip_context by its span" % (type(e).__name__, e))
        text = open(L.REF_SRC + "/context/partition_unit.rs").read().split("\n")
        start = next(i for i, l in enumerate(text) if "pub fn reset_skip_context(" in l)
        end = next(i for i in range(start, len(text)) if text[i] == "  }")
        c.load_text("<context/partition_unit.rs: reset_skip_context>", "impl BlockContext<'_> {\n" + "\n".join(text[start:end + 1]) + "\n}\n")
    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants][:19]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    bs_names = [v[0] for v in c.enums["BlockSize"].variants]
    BlockSize = {n: L.enum(c, "BlockSize", n) for n in bs_names}
    PM = [L.enum(c, "PredictionMode", v[0]) for v in c.enums["PredictionMode"].variants]
    NEARESTMV = PM[14]
    CS = {k: L.enum(c, "ChromaSampling", v) for k, v in CS_NAME.items()}
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    new_counter = c.get("new", owner="WriterCounter")
    new_fc = c.get("new", owner="CDFContext")
    wclm = c.get("write_coeffs_lv_map", owner="ContextWriter")
    reset_skip = c.get("reset_skip_context", owner="BlockContext")
    reset_left = c.get("reset_left_contexts", owner="BlockContext")
    get_set = c.get("get_tx_set")
    has_chroma = c.get("has_chroma")
    uv_intra = c.get("uv_intra_mode_to_tx_type_context")
    max_rect = c.const_value("max_txsize_rect_lookup")
    tx_used = np.array(c.const_value("av1_tx_used").tolist(), np.int32)
    orders = c.const_value("av1_scan_orders")
    assert int(c.const_value("COEFF_CONTEXT_MAX_WIDTH")) == WIDTH
    mi = lambda obj, name: int(c.call_method(obj, name, []))
    rng = np.random.default_rng(20261022)

    def chroma_of(bname, xdec, ydec, inter):
        plane_bsize = c.call_method(c.call_method(BlockSize[bname], "subsampled_size", [xdec, ydec]), "unwrap", [])
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

    def pack(fc):
        return np.concatenate([np.array(nest(getattr(fc, f)), np.int64).reshape(-1) for f in FIELD_NAMES]).astype(np.uint16)

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

    def arrays_of(bc):
        return (np.array([[int(v) for v in bc.above_coeff_context[p]] for p in range(3)], np.uint8),
                np.array([[int(v) for v in bc.left_coeff_context[p]] for p in range(3)], np.uint8))

    rows, names, qc_all = [], [], []
    acc = {k: [] for k in ("eobs", "ctx_in", "ctx_out", "above", "left")}
    seq_ctx, seq_len, seq_names, seq_above, seq_left = [], [], [], [], []
    bi = 0
    # mutation checks (R1_REF_SRC, R1_GOLDEN_OUT): `--stop-before NAME` ends the run in front of a sequence a mutated
    # reference panics in, so that the sequences in front of it can be compared row by row
    stop = sys.argv[sys.argv.index("--stop-before") + 1] if "--stop-before" in sys.argv else None
    for si, (sname, (xdec, ydec), red, cb, seeded, (mi_width, mi_height, w_in_b, h_in_b), events) in enumerate(SEQUENCES):
        assert len(events) <= MAX_ROWS, sname
        if sname == stop:
            break
        fc = new_fc({}, (10, 40, 100, 200)[si % 4])
        ctx_front = pack(fc)
        above0, left0 = np.zeros((3, WIDTH), np.uint8), np.zeros((3, 16), np.uint8)
        if seeded:          # what earlier blocks could have left (below 192), around the sequence's blocks
            xs = [e[3] for e in events if e != RESET]
            lo, hi = max(0, min(xs) - 24), min(WIDTH, max(xs) + 40)
            above0[:, lo:hi] = rng.integers(0, 64, (3, hi - lo)) | (rng.integers(0, 3, (3, hi - lo)) << 6)
            above0[:, lo:hi][rng.integers(0, 4, (3, hi - lo)) == 0] = 0
            left0[:] = rng.integers(0, 64, (3, 16)) | (rng.integers(0, 3, (3, 16)) << 6)
        bc = BC(above_coeff_context=R.RSlice([R.RSlice([int(v) for v in above0[p]]) for p in range(3)]),
                left_coeff_context=R.RSlice([R.RSlice([int(v) for v in left0[p]]) for p in range(3)]),
                left_partition_context=R.RSlice([3] * 16), left_tx_context=R.RSlice([5] * 16))
        cw = CW(bc=bc, fc=fc)
        seq_above.append(above0)
        seq_left.append(left0)
        big = 32767 if cb == 2 else (1 << 20) - 1
        for step, ev in enumerate(events):
            if ev == RESET:
                reset_left({}, bc, 3)
                assert not any(bc.left_partition_context) and not any(bc.left_tx_context)
                ab, lf = arrays_of(bc)
                rows.append((si, step, 4, 4, 0, xdec, ydec) + (0,) * (len(COLS) - 7) + (0, 0, mi_width, mi_height, w_in_b, h_in_b, 0, 1))
                names.append("%s/%d reset_left_contexts" % (sname, step))
                acc["eobs"].append(np.zeros((3, 16), np.uint16))
                acc["ctx_in"].append(np.zeros(96, np.uint8))
                acc["ctx_out"].append(np.zeros(96, np.uint8))
                acc["above"].append(ab)
                acc["left"].append(lf)
                print(len(rows), names[-1], flush=True)
                continue
            bw, bh, ts, bo_x, bo_y, inter, skip, zero = ev
            assert bo_x < mi_width and bo_y < mi_height and bo_x % min(bw >> 2, 16) == 0 and bo_y % min(bh >> 2, 16) == 0, (sname, step)
            bname = "BLOCK_%dX%d" % (bw, bh)
            bsize = BlockSize[bname]
            tw, th = TX_W[ts], TX_H[ts]
            gw, gh = bw // tw, bh // th
            area = min(tw, 32) * min(th, 32)
            pname, uv_ts, bw_uv, bh_uv = chroma_of(bname, xdec, ydec, inter)
            n_uv = bw_uv * bh_uv
            uv_area = min(TX_W[uv_ts], 32) * min(TX_H[uv_ts], 32)
            utw_mi, uth_mi = TX_W[uv_ts] >> 2, TX_H[uv_ts] >> 2
            w_mi, h_mi = bw >> 2, bh >> 2
            tbo = TBO(BO(x=bo_x, y=bo_y))
            do_chroma = bool(has_chroma({}, tbo, bsize, xdec, ydec, CS[(xdec, ydec)]))
            sd = int(get_set({}, TxSize[ts], bool(inter), bool(red)).disc)
            allowed = [t for t in ((9, 10, 11, 0, 1, 3, 12, 5) if inter else (0, 1, 3, 10, 11, 9, 2)) if tx_used[sd][t]]
            tt = allowed[(bi + step) % len(allowed)]
            y_mode, uv_mode = bi % 13, (bi * 3 + step) % 14
            style = (bi + step) % 4
            pool = {0: [0, 0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 14, 15], 2: [1, 2, 3, 14, 15, 127, 128, big], 3: [0, 0, 0, 1]}[style]
            scan = [int(v) for v in orders[ts][tt].scan]
            eobs_y, qcs_y = np.zeros(gw * gh, np.int64), np.zeros((gw * gh, area), np.int64)
            for k in range(gw * gh):
                if zero or skip or (style == 3 and k == 1):
                    continue
                eob = area if rng.integers(0, 8) == 0 and area <= 16 else int(rng.integers(1, min(area, 12) + 1))
                eobs_y[k] = eob
                qcs_y[k] = fill(area, scan, eob, pool, big, (-1, 0, 1)[(bi + k) % 3])
            ab_front, lf_front = arrays_of(bc)
            ux, uy = bo_x - int(w_mi == 1) * xdec, bo_y - int(h_mi == 1) * ydec
            origin = [(bo_x, bo_y % 16), (ux >> xdec, (uy % 16) >> ydec), (ux >> xdec, (uy % 16) >> ydec)]

            def window(ab, lf):
                out = []
                for p in range(3):
                    x0, y0 = origin[p]
                    out += ([int(v) for v in ab[p][x0:x0 + 16]] + [0] * 16)[:16]
                    out += ([int(v) for v in lf[p][y0:y0 + 16]] + [0] * 16)[:16]
                return out

            coded_luma = [k for k in range(gw * gh) if bo_x + (k % gw) * (tw >> 2) < mi_width and bo_y + (k // gw) * (th >> 2) < mi_height]
            if inter:
                uv_tt = int(c.call_method(TxType[tt], "uv_inter", [TxSize[uv_ts]]).disc) if eobs_y[coded_luma].any() else 0
            else:
                uv_tt = 0 if TX_W[uv_ts] >= 32 or TX_H[uv_ts] >= 32 else int(uv_intra({}, PM[uv_mode]).disc)
            uv_scan = [int(v) for v in orders[uv_ts][uv_tt].scan]
            qs_uv, es_uv = [], []
            for p in (1, 2):
                q, e = np.zeros((n_uv, uv_area), np.int64), np.zeros(n_uv, np.int64)
                for k in range(n_uv):
                    if zero or skip or (bi + p + k) % 7 == 0:
                        continue
                    e[k] = int(rng.integers(1, min(uv_area, 10) + 1))
                    q[k] = fill(uv_area, uv_scan, int(e[k]), pool, big, (-1, 0, 1)[(bi + k + p) % 3])
                qs_uv.append(q)
                es_uv.append(e)
            qcs, eobs = [qcs_y, qs_uv[0], qs_uv[1]], [eobs_y, es_uv[0], es_uv[1]]
            rng0 = 0x8000 if (bi + step) % 2 == 0 else int(rng.integers(0x8000, 0x10000))
            rate, rng_out = 0, rng0
            if skip:
                reset_skip({}, bc, tbo, bsize, xdec, ydec, CS[(xdec, ydec)])
            else:
                w = new_counter({})
                w.rng = rng0
                g = {"T": "i16" if cb == 2 else "i32", "W": "WriterBase"}
                tell0 = int(c.call_method(w, "tell_frac", []))
                for by in range(gh):                                          # luma: encoder.rs:2276-2311, 2440-2476
                    for bx in range(gw):
                        k = by * gw + bx
                        tbx, tby = bo_x + bx * (tw >> 2), bo_y + by * (th >> 2)
                        if tbx >= mi_width or tby >= mi_height:               # encoder.rs:1441
                            continue
                        clipped_w, clipped_h = min((w_in_b - tbx) << 2, tw), min((h_in_b - tby) << 2, th)
                        ret = wclm(g, cw, w, 0, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[0][k]]), int(eobs[0][k]),
                                   NEARESTMV if inter else PM[y_mode], TxSize[ts], TxType[tt], bsize, 0, 0, bool(red), clipped_w, clipped_h)
                        assert ret is (int(eobs[0][k]) != 0)
                if do_chroma:                                                 # chroma: encoder.rs:2352-2403, 2513-2561
                    for p in (1, 2):
                        for by in range(bh_uv):
                            for bx in range(bw_uv):
                                k = by * bw_uv + bx
                                tbx = bo_x + ((bx * utw_mi) << xdec) - int(w_mi == 1) * xdec
                                tby = bo_y + ((by * uth_mi) << ydec) - int(h_mi == 1) * ydec
                                if tbx >= mi_width or tby >= mi_height:
                                    continue
                                assert (((w_in_b - tbx) << 2) >> xdec) >= 4 and (((h_in_b - tby) << 2) >> ydec) >= 4     # 1559-1560
                                clipped_w = min(((w_in_b - tbx) << 2) >> xdec, TX_W[uv_ts])
                                clipped_h = min(((h_in_b - tby) << 2) >> ydec, TX_H[uv_ts])
                                ret = wclm(g, cw, w, p, TBO(BO(x=tbx, y=tby)), R.RSlice([int(v) for v in qcs[p][k]]), int(eobs[p][k]),
                                           NEARESTMV if inter else PM[uv_mode], TxSize[uv_ts], TxType[uv_tt], BlockSize[pname], xdec,
                                           ydec, bool(red), clipped_w, clipped_h)
                                assert ret is (int(eobs[p][k]) != 0)
                rate, rng_out = int(c.call_method(w, "tell_frac", [])) - tell0, int(w.rng)
            ab, lf = arrays_of(bc)
            offs = []
            for p in range(3):
                offs.append(len(qc_all))
                for q in qcs[p]:
                    qc_all.extend(int(v) for v in q)
            clip_uv = (min(255, (((w_in_b - ux) << 2) >> xdec) >> 2), min(255, (((h_in_b - uy) << 2) >> ydec) >> 2))
            rows.append((si, step, bw, bh, ts, xdec, ydec, tt, uv_tt, inter, red, cb, y_mode, uv_mode, int(do_chroma), uv_ts, bw_uv,
                         bh_uv, min(255, mi_width - bo_x), min(255, mi_height - bo_y), min(255, w_in_b - bo_x), min(255, h_in_b - bo_y),
                         clip_uv[0], clip_uv[1], rng0, rate, rng_out, offs[0], offs[1], offs[2],
                         bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b, skip, 0))
            names.append("%s/%d %dx%d/%dx%d @%d,%d i%d t%d%s" % (sname, step, bw, bh, tw, th, bo_x, bo_y, inter, tt, " skip" if skip else ""))
            e = np.zeros((3, 16), np.uint16)
            for p in range(3):
                e[p, :len(eobs[p])] = eobs[p]
            acc["eobs"].append(e)
            acc["ctx_in"].append(np.array(window(ab_front, lf_front), np.uint8))
            acc["ctx_out"].append(np.array(window(ab, lf), np.uint8))
            acc["above"].append(ab)
            acc["left"].append(lf)
            print(len(rows), names[-1], "uv_tt", uv_tt, "chroma", int(do_chroma), "rate", rate, "moved",
                  int((ab != ab_front).sum()), int((lf != lf_front).sum()), flush=True)
            bi += 1
        seq_len.append(len(events))
        seq_names.append(sname)
        seq_ctx.append(np.stack([ctx_front, pack(fc)]))

    out = {"columns": np.array(COLS + EXTRA_COLS), "case_rows": np.array(rows, np.int64), "case_names": np.array(names),
           "case_qc": np.array(qc_all, np.int32), "case_eobs": np.stack(acc["eobs"]), "case_ctx_in": np.stack(acc["ctx_in"]),
           "case_ctx_out": np.stack(acc["ctx_out"]), "case_above": np.stack(acc["above"]), "case_left": np.stack(acc["left"]),
           "seq_above": np.stack(seq_above), "seq_left": np.stack(seq_left), "seq_ctx": np.stack(seq_ctx),
           "seq_len": np.array(seq_len, np.int32), "seq_names": np.array(seq_names), "fields": np.array(FIELD_NAMES)}
    print("sequences:", len(seq_len), "rows:", len(rows), flush=True)
    L.save("coeff_nbr_ref.npz", out)


if __name__ == "__main__":
    main()

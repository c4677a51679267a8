#!/usr/bin/env python3
"""tests/golden/tile_chain_ref.npz: the intra decision loop of a tile CARRIED from block to block -- search, real rate,
RD pick, winner commit, CDF adapt, neighbour-context store -- computed by the REFERENCE'S OWN SOURCE TEXT through
tools/rustlite (strict) on ONE tile state (ts.rec), ONE BlockContext and ONE ContextWriter / `fc` per case.  Block k + 1
is predicted from the pixels block k's winner left, measured against the CDFs it adapted and the contexts it stored.
It pins the chain r1_coeff_nbr_gather_batch -> r1_rdo_intra_cand_batch / r1_rdo_intra_split_batch -> the rate calls ->
r1_rd_pick_batch -> r1_rd_commit_batch (rec_trials -> the live plane) -> r1_rd_winner_tx_type_batch ->
r1_coeff_cdf_adapt_batch -> r1_coeff_nbr_store_batch as a whole.

Executed whole, per trial (mode, depth, transform type):
  encode_tx_block                src/encoder.rs:1404-1661, RDOType::PixelDistRealRate, need_recon_pixel = true, with the REAL
      write_coeffs_lv_map (src/context/block_unit.rs:1783-1857: get_txb_ctx, set_coeff_context, the symbol coder of
      src/ec.rs on a WriterBase<WriterCounter> made by WriterCounter::new()) -- no recording stand-in: what
      encode_tx_block hands the entropy coder (frame_clipped_txw / txh, plane_bsize, the type, the mode) is the text's own
      get_intra_edges -> has_top_right / has_bottom_left, predict_intra, diff, forward_transform, quantize, dequantize,
      inverse_transform_add INTO ts.rec
  compute_distortion             src/rdo.rs:254-347, luma_only = true, Tune::Psnr
  compute_rd_cost                src/rdo.rs:718-723
  get_tx_set, av1_tx_used, RAV1E_TX_TYPES, CDFContext::new, reset_left_contexts (src/context/block_unit.rs:394-401)

Stated here (the functions want the whole block coder in front of them; each is executed with scripted inputs by
gen_rd_pick_ref.py or stated likewise by gen_rdo_intra_split_ref.py):
  the loop of write_tx_blocks    src/encoder.rs:2267-2311: qc.update, raster order over the transform blocks, ONE writer
  the type loop of rdo_tx_type_decision   src/rdo.rs:1732-1818: a fresh WriterCounter per type, rate = the tell_frac
      difference, the early exit behind the first type, `rd < best_rd`
  the depth carry of rdo_tx_size_type     src/rdo.rs:748-799, two depths: the block's own transform size, then
      sub_tx_size_map of it
  the mode loop of luma_chroma_mode_rdo   src/rdo.rs:923-938: `rd < best` in trial order over compute_rd_cost(rate +
      rate_add, distortion); rate_add stands for the head symbols, which stay the host's business (rd_pick_ref.npz):
      seeded numbers below 400, except that on even blocks, where two modes' distortions allow it, two of them are set
      so that the two modes cost EXACTLY the same and less than the others (make_tie; lambda is a whole number in those
      cases) -- `<` keeps the earlier mode, `<=` would keep the later
  checkpoint / rollback          every trial starts from a saved copy of `fc`, the BlockContext arrays and ts.rec
  the winner's commit            coded_block_info[..].luma_mode = the winner (src/encoder.rs:2181-2196), then the winner
      recoded once more on the live state with luma_only = true: its reconstruction stays in ts.rec, its adapted CDFs
      in `fc`, its set_coeff_context spans in the BlockContext
  the coding order               src/encoder.rs encode_tile: superblock rows, reset_left_contexts(planes) in front of
      each, superblocks left to right, the partition quad-tree inside a 64x64 superblock
Restatements as in gen_coeff_rate_ref.py (symbol_with_update!, ContextWriter / BlockContext as plain objects, cdf()
lengths) and gen_rdo_glue_ref.py (get_func, v_frame's ChromaSampling).

Out of scope: the chroma half of a block (luma_only everywhere: planes 1 and 2 of the contexts stay zero), blocks cut by
the frame (pinned singly in rdo_intra_split_ref.npz), the SMOOTH modes (none is among a case's K modes, so the intra
edge filter's smooth flag, which reads the neighbours' winning modes, is constant; the neighbours' modes are carried in
coded_block_info all the same).

Per case `c` (row of `cases`, named by `columns`; `names`): c_src, c_rec0 (the plane in front; inside the tile no pixel of
it may be read before it is written), c_final; c_modes (K), c_types (2, 7) / c_nt (2): the types each depth visits;
c_blocks (n, 3): x, y, reset_left_contexts in front; c_rate_add (n, K); per (block, mode, depth, type slot): c_eob
(.., 4), c_qc (.., bs * bs: the transform blocks in raster order, each its coded area), c_rate, c_dist, c_rd; per (block,
mode): c_mode_pick (depth, slot; -1: nothing kept), c_mode_rd; per block: c_win (mode index, depth, slot, type),
c_best_rd (uint64 bits), c_ctx_in / c_ctx_out (the 96 context bytes in front of / behind the block), c_cdf (the packed CDF
context behind it; c_cdf0 in front of the first), c_above / c_left (behind it), c_rec (the block of ts.rec behind it),
c_carry (1: the block's winner predicted from what a NON-winning trial of the block before would have left differs).
c_counts (named by `count_names`): the conditions asserted at the end of the run.

Run in the build container:  python tests/golden/gen_tile_chain_ref.py
(R1_TILE_CASES=name,name: only those cases, for the mutation checks of docs/PARITY.md)
"""
import copy
import multiprocessing
import os
import struct
import sys

import numpy as np

import gen_fwd_tx_golden as FT
import reflib as L
from reflib import R
from gen_rdo_glue_ref import FILES as PIXEL_FILES, TX_W, Obj, make_struct
from gen_coeff_rate_ref import FILES as CODER_FILES, CW, BC
from gen_coeff_cdf_ref import FIELD_NAMES, nest

F64_MAX = sys.float_info.max
PAD = 72
WIDTH = 1024
SUB_TX = {3: 2, 2: 1, 1: 0}                # sub_tx_size_map for the square sizes in scope (checked against the text)
TX_OF = {8: 1, 16: 2, 32: 3}
# (name, bit depth, tile w, tile h, block, modes, qindex, lambda, seed)
CASES = (
    ("w64h32_8bit_b16", 8, 64, 32, 16, (0, 3, 7, 12), 84, 256.0, 11),       # DC, D45, D203, PAETH
    ("w32h32_10bit_b8", 10, 32, 32, 8, (0, 8, 7), 72, 2600.0, 12),          # DC, D67, D203
    ("w64h64_8bit_b32", 8, 64, 64, 32, (1, 3), 96, 416.0, 13),              # V, D45
    ("w64h128_8bit_b32", 8, 64, 128, 32, (2, 8), 100, 448.0, 14),           # H, D67: two superblock rows
    ("w32h32_10bit_b8_second", 10, 32, 32, 8, (0, 8, 7), 72, 2600.0, 15),   # the second tile of the two-tile run: one quantizer, one lambda
)
COLUMNS = ("bd", "w", "h", "bs", "ts0", "ts1", "k", "qindex", "nblocks")
COUNT_NAMES = ("depth0_wins", "depth1_wins", "distinct_modes", "distinct_types", "ctx_nonzero_and_changed",
               "carry_visible", "runner_up_within_1pct", "early_exits", "mode_ties")


def coding_order(w, h, bs):
    """(x, y, reset_left_contexts in front) of every bs x bs block: superblock rows, superblocks left to right, the
    partition quad-tree inside a 64x64 superblock"""
    out = []

    def walk(x, y, size, found):
        if x >= w or y >= h:
            return
        if size == bs:
            found.append((x, y))
            return
        half = size // 2
        for dy in (0, 1):
            for dx in (0, 1):
                walk(x + dx * half, y + dy * half, half, found)
    for sby in range(0, h, 64):
        row = []
        for sbx in range(0, w, 64):
            walk(sbx, sby, 64, row)
        out += [(x, y, int(i == 0)) for i, (x, y) in enumerate(row)]
    return out


def source(rng, bd, w, h):
    """a gradient with texture: flat, striped and noisy regions, so that modes, depths and types all have somewhere to win"""
    mx = (1 << bd) - 1
    s = 1 << (bd - 8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = 60 + 0.9 * xx + 0.5 * yy
    a += 26 * np.sin((xx + yy) / 2.3) * (((xx // 16 + yy // 16) % 3) == 0)          # diagonal stripes
    a += 30 * np.sign(np.sin(xx / 1.7)) * (((xx // 16 + yy // 16) % 3) == 1) * ((yy // 8) % 2)
    a += 22 * np.sin(yy / 1.3) * (((xx // 8 + yy // 16) % 4) == 2)
    a += rng.integers(-5, 6, (h, w))
    a[(yy > 0.8 * xx + 6) & (yy < 0.8 * xx + 14)] += 45                              # a slanted edge
    return np.clip(a * s, 0, mx)


def build():
    files = list(PIXEL_FILES) + [f for f in CODER_FILES if f not in PIXEL_FILES]
    c = L.crate(*files, strict=True)
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
    return c


CRATE = None          # built once, in front of the fork


def run_case(case):
    c = CRATE
    name, bd, fw, fh, bs, modes, qindex, lam, seed = case
    TxSize = [L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants]
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants]
    BlockSize = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
    PM = [L.enum(c, "PredictionMode", v[0]) for v in c.enums["PredictionMode"].variants]
    DS = L.struct(c, "DistortionScale")
    SD = L.struct(c, "ScaledDistortion")
    TileStateMut = L.struct(c, "TileStateMut")
    CBI = L.struct(c, "CodedBlockInfo")
    PSBO, SBO = L.struct(c, "PlaneSuperBlockOffset"), L.struct(c, "SuperBlockOffset")
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    qc_default = c.get("default", owner="QuantizationContext")
    qc_update = c.get("update", owner="QuantizationContext")
    etb = c.get("encode_tx_block")
    cdist = c.get("compute_distortion")
    rd_cost = c.get("compute_rd_cost")
    new_counter = c.get("new", owner="WriterCounter")
    new_fc = c.get("new", owner="CDFContext")
    reset_left = c.get("reset_left_contexts", owner="BlockContext")
    get_set = c.get("get_tx_set")
    tx_used = c.const_value("av1_tx_used")
    rav1e_types = [int(t.disc) for t in c.const_value("RAV1E_TX_TYPES")]
    sub_map = c.const_value("sub_tx_size_map")
    RDO_PIX = L.enum(c, "RDOType", "PixelDistRealRate")
    INTRA_FRAME, NONE_FRAME = L.enum(c, "RefType", "INTRA_FRAME"), L.enum(c, "RefType", "NONE_FRAME")
    assert int(c.const_value("COEFF_CONTEXT_MAX_WIDTH")) == WIDTH

    rng = np.random.default_rng(20261100 + seed)
    K = len(modes)
    dt = L.np_dtype(bd)
    mx = (1 << bd) - 1
    g = dict(L.pixel_type(bd), W="WriterBase")
    g1 = L.pixel_type(bd)
    mi_w, mi_h = fw >> 2, fh >> 2
    sizes = (TX_OF[bs], SUB_TX[TX_OF[bs]])
    assert int(sub_map[sizes[0]].disc) == sizes[1]
    bsize = BlockSize["BLOCK_%dX%d" % (bs, bs)]
    types = [[t for t in rav1e_types if int(tx_used[int(get_set({}, TxSize[ts], False, False).disc)][t])] for ts in sizes]
    order = coding_order(fw, fh, bs)
    nb = len(order)
    assert nb == (fw // bs) * (fh // bs)

    src = source(rng, bd, fw, fh).astype(dt)
    src_pad = np.pad(src, PAD, mode="edge")
    # what lies in the plane before the tile is coded: noise, inside the tile and around it -- a pixel of it that a
    # prediction reads shows as a mismatch against any chain that starts from other pixels
    rec0_pad = rng.integers(0, mx + 1, src_pad.shape).astype(dt)
    p_in = [L.plane_from_padded(src_pad, bd, PAD, PAD, 0, 0)]
    p_rec = [L.plane_from_padded(rec0_pad, bd, PAD, PAD, 0, 0)]
    refs = R.array(INTRA_FRAME, NONE_FRAME)
    cbi = R.RSlice([R.RSlice([CBI(luma_mode=R.Some(PM[0]), chroma_mode=R.Some(PM[0]), reference_types=refs)
                              for _ in range(mi_w)]) for _ in range(mi_h)])
    qc = qc_default({})
    tsm = make_struct(TileStateMut, sbo=PSBO(SBO(x=0, y=0)), sb_size_log2=6, sb_width=(fw + 63) // 64,
                      sb_height=(fh + 63) // 64, mi_width=mi_w, mi_height=mi_h, width=fw, height=fh,
                      input=Obj(planes=R.RSlice(p_in)), input_tile=Obj(planes=R.RSlice([p.as_region() for p in p_in])),
                      rec=Obj(planes=R.RSlice([p.as_region() for p in p_rec])), qc=qc, coded_block_info=cbi)
    fi = Obj(sequence=Obj(bit_depth=bd, enable_intra_edge_filter=True, chroma_sampling=L.enum(c, "ChromaSampling", "Cs420")),
             width=fw, height=fh, w_in_b=mi_w, h_in_b=mi_h, use_tx_domain_distortion=False, base_q_idx=qindex,
             dc_delta_q=R.RSlice([0, 0, 0]), ac_delta_q=R.RSlice([0, 0, 0]), dist_scale=R.RSlice([DS(1 << 14)] * 3),
             config=Obj(temporal_rdo=(lambda: False), tune=L.enum(c, "Tune", "Psnr")), coded_frame_data=R.NONE,
             cpu_feature_level=None, use_reduced_tx_set=False, lambda_=float(lam))
    fc = new_fc({}, qindex)
    bc = BC(above_coeff_context=R.RSlice([R.RSlice([0] * WIDTH) for _ in range(3)]),
            left_coeff_context=R.RSlice([R.RSlice([0] * 16) for _ in range(3)]),
            left_partition_context=R.RSlice([0] * 16), left_tx_context=R.RSlice([0] * 16))
    cw = CW(bc=bc, fc=fc)
    iparam = c.G["_E"]("IntraParam", "AngleDelta", 0, (0,))
    acs = R.RSlice([])
    plane = p_rec[0]
    cfg = plane.cfg

    def pack(f):
        return np.concatenate([np.array(nest(getattr(f, n)), np.int64).reshape(-1) for n in FIELD_NAMES]).astype(np.uint16)

    def arrays():
        return (np.array([[int(v) for v in bc.above_coeff_context[p]] for p in range(3)], np.uint8),
                np.array([[int(v) for v in bc.left_coeff_context[p]] for p in range(3)], np.uint8))

    def window(ab, lf, x, y):
        bo_x, bo_y = x >> 2, y >> 2
        origin = [(bo_x, bo_y % 16), (bo_x >> 1, (bo_y % 16) >> 1), (bo_x >> 1, (bo_y % 16) >> 1)]
        o = []
        for p in range(3):
            x0, y0 = origin[p]
            o += ([int(v) for v in ab[p][x0:x0 + 16]] + [0] * 16)[:16]
            o += ([int(v) for v in lf[p][y0:y0 + 16]] + [0] * 16)[:16]
        return np.array(o, np.uint8)

    def block_of(x, y, w=bs, h=bs):
        o = np.zeros((h, w), dt)
        for r in range(h):
            base = (cfg.yorigin + y + r) * cfg.stride + cfg.xorigin + x
            o[r] = plane.data[base:base + w]
        return o

    def put_block(x, y, a):
        for r in range(a.shape[0]):
            base = (cfg.yorigin + y + r) * cfg.stride + cfg.xorigin + x
            plane.data[base:base + a.shape[1]] = [int(v) for v in a[r]]

    def save_state():
        return (copy.deepcopy(cw.fc), [[int(v) for v in bc.above_coeff_context[p]] for p in range(3)],
                [[int(v) for v in bc.left_coeff_context[p]] for p in range(3)], list(plane.data))

    def restore(s):
        """the generator's form of cw.rollback: `fc`, the context arrays and ts.rec as saved"""
        cw.fc = copy.deepcopy(s[0])
        bc.above_coeff_context = R.RSlice([R.RSlice(list(r)) for r in s[1]])
        bc.left_coeff_context = R.RSlice([R.RSlice(list(r)) for r in s[2]])
        plane.data[:] = s[3]

    def code(x, y, mode, ts, tt):
        """one (mode, transform size, type) of the block at (x, y) on the state as it stands: the loop of
        write_tx_blocks (encoder.rs:2267-2311) on a fresh WriterCounter, then compute_distortion"""
        t = TX_W[ts]
        bo_x, bo_y = x >> 2, y >> 2
        bo = TBO(BO(x=bo_x, y=bo_y))
        qc_update({}, qc, qindex, TxSize[ts], True, bd, 0, 0)
        w = new_counter({})
        tell = int(c.call_method(w, "tell_frac", []))
        gw = bs // t
        eobs, qcs = [], []
        for by in range(gw):
            for bx in range(gw):
                tbx, tby = bo_x + bx * (t >> 2), bo_y + by * (t >> 2)
                assert tbx < mi_w and tby < mi_h
                del cw_calls[:]
                etb(g, fi, tsm, cw, w, 0, bo, bx, by, TBO(BO(x=tbx, y=tby)), PM[mode], TxSize[ts], TxType[tt], bsize,
                    R.PlaneOffset(x=tbx * 4, y=tby * 4), False, qindex, acs, iparam, RDO_PIX, True)
                assert len(cw_calls) == 1
                qcs.append(cw_calls[0][0])
                eobs.append(cw_calls[0][1])
        rate = int(c.call_method(w, "tell_frac", [])) - tell
        dist = cdist(g1, fi, tsm, bsize, False, bo, True)
        rd = float(rd_cost(g1, fi, rate, dist))
        return dict(eob=eobs, qc=np.concatenate(qcs), rate=rate, dist=int(dist._0), rd=rd, rec=block_of(x, y))

    # write_coeffs_lv_map is executed as it stands; this wrapper only notes the (qcoeffs, eob) the text hands it
    cw_calls = []
    real_wclm = c.find_method("ContextWriter", "write_coeffs_lv_map")

    def noting(gg, self_, w, p, tx_bo, qcoeffs, eob, *rest):
        cw_calls.append((np.array([int(v) for v in qcoeffs], np.int32), int(eob)))
        return c._call_info(real_wclm, gg, (self_, w, p, tx_bo, qcoeffs, eob) + rest)
    c.define_py("r1_noting_wclm", noting)
    c.methods["ContextWriter"]["write_coeffs_lv_map"] = [c.fns.pop("r1_noting_wclm")[0]]

    def predict_only(x, y, mode, ts):
        """encode_tx_block with skip = true: get_intra_edges and predict_intra into ts.rec, nothing else"""
        bo = TBO(BO(x=x >> 2, y=y >> 2))
        etb(g, fi, tsm, cw, new_counter({}), 0, bo, 0, 0, bo, PM[mode], TxSize[ts], TxType[0], bsize,
            R.PlaneOffset(x=x, y=y), True, qindex, acs, iparam, RDO_PIX, True)
        return block_of(x, y)

    NT, NTX = 7, 4
    o = dict(eob=np.zeros((nb, K, 2, NT, NTX), np.uint16), qc=np.zeros((nb, K, 2, NT, bs * bs), np.int32),
             rate=np.zeros((nb, K, 2, NT), np.uint32), dist=np.zeros((nb, K, 2, NT), np.uint64),
             rd=np.zeros((nb, K, 2, NT), np.float64), mode_pick=np.zeros((nb, K, 2), np.int8),
             mode_rd=np.zeros((nb, K), np.float64), win=np.zeros((nb, 4), np.int32), best_rd=np.zeros(nb, np.uint64),
             ctx_in=np.zeros((nb, 96), np.uint8), ctx_out=np.zeros((nb, 96), np.uint8), cdf=np.zeros((nb, 3930), np.uint16),
             above=np.zeros((nb, 3, WIDTH), np.uint8), left=np.zeros((nb, 3, 16), np.uint8), rec=np.zeros((nb, bs, bs), dt),
             carry=np.zeros(nb, np.uint8), rate_add=rng.integers(0, 400, (nb, K)).astype(np.uint32))
    o["cdf0"] = pack(cw.fc)
    early = close = ties = 0

    def make_tie(adds, rates, dists):
        """the head rates of an even block, where two modes allow it, set so that the two cost EXACTLY the same and
        less than every other mode: lambda is a whole number here, so lambda * (rate / 8) + distortion is exact and two
        costs are equal when lambda * (rate_i - rate_j) == 8 * (dist_j - dist_i).  `rd < best` keeps the earlier mode"""
        if lam != int(lam):
            return 0
        for i in range(K):
            for j in range(i + 1, K):
                num = (dists[j] - dists[i]) * 8
                if num % int(lam):
                    continue
                a_j = int(adds[j])
                a_i = rates[j] + a_j + num // int(lam) - rates[i]
                if a_i < 0:
                    a_i, a_j = 0, a_j - a_i
                if max(a_i, a_j) > 4000:
                    continue
                adds[i], adds[j] = a_i, a_j
                tie = int(lam) * (rates[i] + a_i) + 8 * dists[i]
                assert tie == int(lam) * (rates[j] + a_j) + 8 * dists[j]
                for m in range(K):
                    if m not in (i, j):
                        short = tie - (int(lam) * (rates[m] + int(adds[m])) + 8 * dists[m])
                        if short >= 0:
                            adds[m] = int(adds[m]) + short // int(lam) + 1 + int(adds[m]) % 7
                return 1
        return 0
    alt = None                                  # (x, y, block): what a non-winning trial of the block before would have left
    for bi, (x, y, reset) in enumerate(order):
        if reset:
            reset_left({}, bc, 3)
        o["ctx_in"][bi] = window(*arrays(), x, y)
        start = save_state()
        trials = {}
        best_mode, best = -1, F64_MAX
        for mi, mode in enumerate(modes):
            best_rd, pick = F64_MAX, (-1, -1)
            for d, ts in enumerate(sizes):
                type_rd, type_slot = F64_MAX, 0
                for slot, tt in enumerate(types[d]):
                    restore(start)
                    r = trials[(mi, d, slot)] = code(x, y, mode, ts, tt)
                    ntx = len(r["eob"])
                    o["eob"][bi, mi, d, slot, :ntx], o["qc"][bi, mi, d, slot] = r["eob"], r["qc"]
                    o["rate"][bi, mi, d, slot], o["dist"][bi, mi, d, slot], o["rd"][bi, mi, d, slot] = r["rate"], r["dist"], r["rd"]
                # rdo_tx_type_decision's rule (rdo.rs:1803-1817) over the executed costs, cur_best_rd = best_rd
                for slot in range(len(types[d])):
                    rd = trials[(mi, d, slot)]["rd"]
                    if slot == 0 and rd > best_rd:
                        early += 1
                        break
                    if rd < type_rd:
                        type_rd, type_slot = rd, slot
                if type_rd < best_rd:               # rdo_tx_size_type (rdo.rs:780-784)
                    best_rd, pick = type_rd, (d, type_slot)
            o["mode_pick"][bi, mi] = pick
        kept = [trials[(mi,) + tuple(int(v) for v in o["mode_pick"][bi, mi])] for mi in range(K)]
        if bi % 2 == 0:
            ties += make_tie(o["rate_add"][bi], [t["rate"] for t in kept], [t["dist"] for t in kept])
        for mi in range(K):
            rd = float(rd_cost(g1, fi, kept[mi]["rate"] + int(o["rate_add"][bi, mi]), SD(kept[mi]["dist"])))
            o["mode_rd"][bi, mi] = rd
            if rd < best:                           # luma_chroma_mode_rdo (rdo.rs:934)
                best, best_mode = rd, mi
        d, slot = (int(v) for v in o["mode_pick"][bi, best_mode])
        o["win"][bi] = (best_mode, d, slot, types[d][slot])
        o["best_rd"][bi] = struct.unpack("<Q", struct.pack("<d", best))[0]
        # a runner-up within 1 %: any other trial, costed with its mode's rate_add
        for (mi, dd, ss), r in trials.items():
            if (mi, dd, ss) != (best_mode, d, slot):
                other = float(rd_cost(g1, fi, r["rate"] + int(o["rate_add"][bi, mi]), SD(r["dist"])))
                if other <= best * 1.01:
                    close += 1
                    break
        # is the reconstruction carry visible?  this block's winner predicted from the other past
        restore(start)
        if alt is not None:
            real = predict_only(x, y, modes[best_mode], sizes[0])
            restore(start)
            put_block(*alt)
            o["carry"][bi] = int(not np.array_equal(predict_only(x, y, modes[best_mode], sizes[0]), real))
            restore(start)
        # the commit: the winner's mode into coded_block_info, the winner recoded on the live state
        for yy in range(bs >> 2):
            for xx in range(bs >> 2):
                cbi[(y >> 2) + yy][(x >> 2) + xx] = CBI(luma_mode=R.Some(PM[modes[best_mode]]),
                                                        chroma_mode=R.Some(PM[modes[best_mode]]), reference_types=refs)
        r = code(x, y, modes[best_mode], sizes[d], types[d][slot])
        wt = trials[(best_mode, d, slot)]
        assert r["rate"] == wt["rate"] and r["dist"] == wt["dist"] and np.array_equal(r["rec"], wt["rec"])
        ab, lf = arrays()
        o["ctx_out"][bi], o["above"][bi], o["left"][bi] = window(ab, lf, x, y), ab, lf
        o["cdf"][bi], o["rec"][bi] = pack(cw.fc), r["rec"]
        losers = [t for k_, t in trials.items() if k_ != (best_mode, d, slot) and not np.array_equal(t["rec"], r["rec"])]
        alt = (x, y, losers[len(losers) // 2]["rec"]) if losers else None
        print(name, bi, (x, y), "win mode", modes[best_mode], "depth", d, "type", types[d][slot], "rd", best,
              "carry", int(o["carry"][bi]), flush=True)

    final = L.plane_to_array(plane, dt)
    counts = (int((o["win"][:, 1] == 0).sum()), int((o["win"][:, 1] == 1).sum()), len(set(o["win"][:, 0].tolist())),
              len(set(o["win"][:, 3].tolist())),
              int(sum(o["ctx_in"][k].any() and not np.array_equal(o["ctx_in"][k], o["ctx_in"][k - 1]) for k in range(1, nb))),
              int(o["carry"].sum()), close, early, ties)
    out = {name + "_" + k: v for k, v in o.items()}
    if bd == 8:
        out[name + "_qc"] = o["qc"].astype(np.int16)
        assert np.array_equal(out[name + "_qc"], o["qc"])
    out.update({name + "_src": src, name + "_rec0": rec0_pad[PAD:PAD + fh, PAD:PAD + fw], name + "_final": final,
                name + "_modes": np.array(modes, np.int32), name + "_nt": np.array([len(t) for t in types], np.int32),
                name + "_types": np.array([t + [-1] * (NT - len(t)) for t in types], np.int32),
                name + "_blocks": np.array(order, np.int32), name + "_lam": np.array(lam, np.float64),
                name + "_counts": np.array(counts, np.int64)})
    row = (bd, fw, fh, bs, sizes[0], sizes[1], K, qindex, nb)
    print(name, dict(zip(COUNT_NAMES, counts)), flush=True)
    return name, row, out


def main():
    global CRATE
    CRATE = build()
    pick = os.environ.get("R1_TILE_CASES")
    cases = [cs for cs in CASES if not pick or cs[0] in pick.split(",")]
    with multiprocessing.get_context("fork").Pool(min(len(cases), os.cpu_count() or 1)) as pool:
        results = pool.map(run_case, cases, chunksize=1)
    out = {"names": np.array([r[0] for r in results]), "cases": np.array([r[1] for r in results], np.int64),
           "columns": np.array(COLUMNS), "count_names": np.array(COUNT_NAMES), "fields": np.array(FIELD_NAMES)}
    for _, _, o in results:
        out.update(o)
    L.save("tile_chain_ref.npz", out)
    # conditions, behind the save so that a mutated reference (docs/PARITY.md) still leaves its file to compare
    for name, row, o in results:
        cnt = dict(zip(COUNT_NAMES, (int(v) for v in o[name + "_counts"])))
        assert cnt["ctx_nonzero_and_changed"] >= 1 and cnt["carry_visible"] >= 1, (name, cnt)
        if name == CASES[0][0]:
            assert cnt["distinct_modes"] >= 3 and cnt["distinct_types"] >= 2, (name, cnt)
    total = {k: sum(int(o[n + "_counts"][i]) for n, _, o in results) for i, k in enumerate(COUNT_NAMES)}
    assert total["depth0_wins"] >= 1 and total["depth1_wins"] >= 1 and total["runner_up_within_1pct"] >= 1, total
    assert total["mode_ties"] >= 1, total
    print("conditions hold:", total)


if __name__ == "__main__":
    main()

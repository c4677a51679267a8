#!/usr/bin/env python3
"""tests/golden/rd_pick_ref.npz: the RD decision -- compute_rd_cost, the transform-type loop with its early exit, the
carry across the transform depths -- computed by the REFERENCE'S OWN SOURCE TEXT through tools/rustlite.  It pins
rdo_glue.pick_tx_type / pick_first_min / tx_size_type_decision and, through them, r1_rd_pick_batch.

Executed whole:
  compute_rd_cost            src/rdo.rs:718-723
  rdo_tx_type_decision       src/rdo.rs:1701-1823
  rdo_tx_size_type           src/rdo.rs:725-802
  get_tx_set, av1_tx_used, sub_tx_size_map, max_txsize_rect_lookup, RAV1E_TX_TYPES, has_chroma, TxSize::block_size,
  PredictionMode::is_intra: real.

Scripted stand-ins for what the two functions call (the numbers they would produce are the CASE's inputs):
  WriterCounter::new()       an object whose tell_frac() answers 0, then the case's rate of the (depth, type) that
                             write_tx_blocks / write_tx_tree was called with in between
  write_tx_blocks, write_tx_tree          note the (tx_size, tx_type) of the call; return (false, the case's distortion)
  compute_distortion, compute_tx_distortion   return the case's distortion of that (tx_size, tx_type); cases alternate
                             fi.use_tx_domain_distortion so that both arms run
  motion_compensate, cw.checkpoint, cw.rollback   do nothing

One line of the reference text is rewritten before it is parsed (as refmacro.unpointer does elsewhere): in
rdo_tx_size_type
    let mut cw_checkpoint: Option<ContextWriterCheckpoint> = None;
becomes `= Some(cw.checkpoint(&tile_bo, fi.sequence.chroma_sampling));` -- what the first rdo_tx_type_decision call
stores there (rdo.rs:1717-1722), hoisted.  The transpiler passes an `Option` local by value, so the callee's store
through `&mut cw_checkpoint` has nowhere to land; the checkpoint is a do-nothing stand-in here either way.
rdo_tx_type_decision called directly gets a Some(..) from the generator for the same reason.

Stated by hand (the mode loop of luma_chroma_mode_rdo, src/rdo.rs:923-938, is not executed: it drags the whole block
coder in): the fm_* groups apply `rd < best` in trial order to costs that compute_rd_cost itself produced.

Keys:
  cost_lam / cost_rate / cost_dist -> cost_rd: single compute_rd_cost calls; cost_kind 0 = the edge grid (rates 0, 1, 7,
      8, 2^32 - 2; distortions around 2^53, 2^63 + 2^10 + 1, 2^64 - 1; lambda 0, 8, inexact ones), 1 = tuples whose
      twice-rounded lambda * (rate / 8) + dist differs from the fused result (found with exact rationals;
      n_fused_differs of them)
  tt_*: rdo_tx_type_decision: tt_lam, tt_cur (cur_best_rd), tt_nt, tt_rate / tt_dist (n, 16) -> tt_slot (-1: nothing
      kept: the function returned f64::MAX), tt_rd, tt_evals (compute_rd_cost calls made: 1 after an early exit)
  sz_*: rdo_tx_size_type: sz_lam, sz_ndepth, sz_nt (n, 3), sz_rate / sz_dist (n, 3, 16) -> sz_depth, sz_slot, sz_rd (the
      cost compute_rd_cost returned for that trial), sz_evals (n, 3)
  fm_*: fm_lam, fm_n, fm_rate, fm_add, fm_dist (n, 16), fm_best_in -> fm_rd (n, 16) executed per trial on rate + add,
      fm_idx (-1: the carried one stays)
  *_names: the cases' names (the mutation checks of docs/PARITY.md name them)

Run in the build container:  python tests/golden/gen_rd_pick_ref.py
"""
import os
import struct
import sys
from fractions import Fraction

import numpy as np

import reflib as L
from reflib import R

F64_MAX = sys.float_info.max
REWRITE = ("let mut cw_checkpoint: Option<ContextWriterCheckpoint> = None;",
           "let mut cw_checkpoint: Option<ContextWriterCheckpoint> = Some(cw.checkpoint(&tile_bo, fi.sequence.chroma_sampling));")


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def stub(c, name, fn, owner=None):
    """the Python callable fn(_g, *args) in place of a reference function or associated function"""
    c.define_py("r1_stub_" + name, fn)
    info = c.fns.pop("r1_stub_" + name)[0]
    if owner:
        c.methods.setdefault(owner, {})[name] = [info]
    else:
        c.fns[name] = [info]


def main():
    c = L.crate("transform/mod.rs", "context/transform_unit.rs", "partition.rs", "predict.rs", "context/mod.rs",
                "util/mod.rs")
    text = open(os.path.join(L.REF_SRC, "rdo.rs")).read()
    assert text.count(REWRITE[0]) == 1
    c.load_text("rdo.rs", text.replace(*REWRITE))
    c.define_enum("ChromaSampling", ["Cs420", "Cs422", "Cs444", "Cs400"])
    SD = L.struct(c, "ScaledDistortion")
    cur = {}          # the running case: table[(tx_size disc, tx_type disc)] = (rate, dist); `at` = the last call's key

    class Counter:
        def __init__(self):
            self.calls = 0

        def tell_frac(self):
            self.calls += 1
            return 0 if self.calls == 1 else cur["table"][cur["at"]][0]

    class Writer:
        def checkpoint(self, *a):
            return "checkpoint"

        def rollback(self, *a):
            return None

    def write_tx(ts_arg, tt_arg):
        def f(_g, *a):
            cur["at"] = (int(a[ts_arg].disc), int(a[tt_arg].disc))
            return (False, SD(cur["table"][cur["at"]][1]))
        return f

    def dist(_g, *a):
        return SD(cur["table"][cur["at"]][1])
    stub(c, "new", lambda _g: Counter(), owner="WriterCounter")
    stub(c, "write_tx_blocks", write_tx(9, 10))
    stub(c, "write_tx_tree", write_tx(8, 9))
    stub(c, "compute_distortion", dist)
    stub(c, "compute_tx_distortion", dist)
    stub(c, "motion_compensate", lambda _g, *a: None)
    type_decision = c.get("rdo_tx_type_decision")
    size_type = c.get("rdo_tx_size_type")
    rd_cost = c.get("compute_rd_cost")
    evals = []
    c.G[rd_cost.__name__] = lambda *a: evals.append((cur.get("at"), float(rd_cost(*a)))) or evals[-1][1]

    g = {"T": "u16"}
    cs = L.enum(c, "ChromaSampling", "Cs420")
    TxSize = {v[0]: L.enum(c, "TxSize", v[0]) for v in c.enums["TxSize"].variants}
    TxType = [L.enum(c, "TxType", v[0]) for v in c.enums["TxType"].variants][:16]
    BlockSize = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
    DC_PRED, NEARESTMV = L.enum(c, "PredictionMode", "DC_PRED"), L.enum(c, "PredictionMode", "NEARESTMV")
    INTRA, LAST = L.enum(c, "RefType", "INTRA_FRAME"), L.enum(c, "RefType", "LAST_FRAME")
    MV = L.struct(c, "MotionVector")
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    get_set = c.get("get_tx_set")
    tx_used = c.const_value("av1_tx_used")
    rav1e_types = c.const_value("RAV1E_TX_TYPES")
    ts = Obj(input=Obj(planes=R.RSlice([Obj(cfg=R.PlaneConfig.new(64, 64, 1, 1, 0, 0, 2))] * 3)))
    mvs = R.RSlice([MV(row=0, col=0)] * 2)
    bo = TBO(BO(x=0, y=0))

    def make_fi(lam, tx_domain):
        return Obj(lambda_=float(lam), use_tx_domain_distortion=bool(tx_domain), sequence=Obj(chroma_sampling=cs),
                   enable_inter_txfm_split=False, tx_mode_select=True, use_reduced_tx_set=False,
                   config=Obj(speed_settings=Obj(transform=Obj(rdo_tx_decision=True))))

    def cost(lam, rate, dist_):
        return float(rd_cost(g, make_fi(lam, 0), int(rate), SD(int(dist_))))

    def fused(lam, rate, dist_):
        # `distortion.0 as f64` rounds first (to nearest even); the multiply-add on that is exact and rounded once
        return float(Fraction(float(lam)) * Fraction(int(rate), 8) + Fraction(float(int(dist_))))

    out = {}
    rng = np.random.default_rng(20261020)

    # ---------------- compute_rd_cost alone
    rows = []
    lams = [0.0, 8.0, 1.0, 0.1, 1.0 / 3.0, 123.456789, 2.0 ** -20 * 3.3, 1e9 / 7.0]
    rates = [0, 1, 7, 8, 2 ** 32 - 2]
    dists = [0, 1, 8, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, 2 ** 63 + 2 ** 10, 2 ** 63 + 2 ** 10 + 1,
             2 ** 64 - 1]
    for lam in lams:
        for r in rates:
            for d in dists:
                rows.append((lam, r, d, 0))
    n_diff = 0
    while n_diff < 64:
        lam = float(rng.choice([rng.uniform(0.01, 300.0), rng.uniform(1e3, 1e7), 0.1 * int(rng.integers(1, 100))]))
        r = int(rng.integers(1, 1 << int(rng.integers(4, 31))))
        d = int(rng.integers(0, 1 << int(rng.integers(4, 50))))
        twice = lam * (r / 8.0) + float(d)
        if twice != fused(lam, r, d):
            rows.append((lam, r, d, 1))
            n_diff += 1
    out["cost_lam"] = np.array([r[0] for r in rows], np.float64)
    out["cost_rate"] = np.array([r[1] for r in rows], np.uint32)
    out["cost_dist"] = np.array([r[2] for r in rows], np.uint64)
    out["cost_kind"] = np.array([r[3] for r in rows], np.uint8)
    out["cost_rd"] = np.array([cost(*r[:3]) for r in rows], np.float64)
    out["n_fused_differs"] = np.array(n_diff, np.int32)

    # ---------------- rdo_tx_type_decision
    # nt comes from the transform size, the block kind and the list handed in
    SHAPES = {1: ("TX_64X64", "BLOCK_64X64", DC_PRED, rav1e_types), 2: ("TX_32X32", "BLOCK_32X32", NEARESTMV, rav1e_types),
              5: ("TX_16X16", "BLOCK_16X16", DC_PRED, rav1e_types), 7: ("TX_8X8", "BLOCK_8X8", DC_PRED, rav1e_types),
              16: ("TX_8X8", "BLOCK_8X8", NEARESTMV, R.RSlice(list(TxType)))}

    def visited(tx_size, inter, types):
        s = int(get_set({}, TxSize[tx_size], bool(inter), False).disc)
        return [int(t.disc) for t in types if int(tx_used[s][int(t.disc)])]

    B = 2 ** 53
    big = 2 ** 63 + 2 ** 10
    c8 = cost(8.0, 8, 0)
    tt_cases = [
        # name, lambda, cur_best_rd, rates, dists
        ("tie_rate8_dist0_vs_rate0_dist8", 8.0, F64_MAX, [8, 0], [0, 8]),
        ("tie_rate0_dist8_vs_rate8_dist0", 8.0, F64_MAX, [0, 8, 16, 0, 3], [8, 0, 0, 9, 9]),
        ("tie_slots_0_and_3", 8.0, F64_MAX, [4, 9, 9, 4, 9, 9, 9], [20, 30, 31, 20, 40, 50, 60]),
        ("tie_slots_0_and_3_later_lower", 8.0, F64_MAX, [4, 9, 9, 4, 9, 2, 2], [20, 30, 31, 20, 40, 21, 21]),
        ("tie_all_equal_16", 2.0, F64_MAX, [4] * 16, [7] * 16),
        ("exit_slot0_above_later_below", 8.0, 100.0, [8, 0, 0, 0, 0], [93, 1, 2, 3, 4]),
        ("exit_slot0_above_later_below_7", 1.0, cost(1.0, 80, 50), [81, 0, 0, 0, 0, 0, 0], [50, 1, 1, 1, 1, 1, 1]),
        ("no_exit_slot0_equal_cur", 8.0, c8, [8, 0, 1, 1, 1], [0, 3, 9, 9, 9]),
        ("no_exit_slot0_equal_cur_is_min", 8.0, c8, [8, 9, 9, 9, 9], [0, 9, 9, 9, 9]),
        ("no_exit_slot0_below_cur", 8.0, 100.0, [8, 0, 0, 0, 0], [91, 95, 1, 1, 0]),
        ("exit_nt1", 1.0, 5.0, [8], [5]),
        ("keep_nt1", 1.0, 7.0, [8], [5]),
        ("nt2_second", 3.5, F64_MAX, [9, 1], [100, 100]),
        ("lambda0_dist_only", 0.0, F64_MAX, [2 ** 32 - 2, 0, 7, 1, 8], [5, 5, 4, 4, 9]),
        ("lambda0_exit", 0.0, 3.0, [0, 0, 0, 0, 0], [4, 1, 1, 1, 1]),
        ("dist_2p53_plus1_ties_to_even", 0.0, F64_MAX, [0, 0], [B + 1, B]),
        ("dist_2p53_plus1_after_2p53", 0.0, F64_MAX, [0, 0], [B, B + 1]),
        ("dist_2p53_plus1_converted_before_fma", 1.0, F64_MAX, [5, 0], [B + 1, B + 1]),
        ("dist_2p53_plus3_rounds_up", 0.0, F64_MAX, [0, 0, 0, 0, 0], [B + 4, B + 3, B + 2, B + 1, B + 3]),
        ("dist_2p63_2p10_plus1_rounds_up", 1.0, F64_MAX, [0, 0], [big + 2 ** 11, big + 1]),
        ("dist_2p63_exact_then_above", 1.0, F64_MAX, [0, 0, 0, 0, 0, 0, 0], [big + 1, big, big, big - 1, big, big, big]),
        ("dist_u64_max", 1.0, F64_MAX, [8, 0, 1, 7, 8], [2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 2048, 2 ** 64 - 1]),
        ("dist_u64_max_exit", 1.0, 2.0 ** 63, [0, 0], [2 ** 64 - 1, 0]),
        ("rates_0_1_7_8", 1.0, F64_MAX, [8, 7, 1, 0, 1, 7, 8], [10, 10, 10, 10, 10, 10, 10]),
        ("rate_u32_max_less_1", 0.5, F64_MAX, [2 ** 32 - 2, 2 ** 32 - 2, 8, 7, 7], [0, 1, 2 ** 28, 2 ** 28, 2 ** 28 + 1]),
        ("inexact_lambda_third", 1.0 / 3.0, F64_MAX, [3, 6, 9, 1, 2, 12, 24], [100, 100, 99, 100, 100, 99, 98]),
        ("inexact_lambda_16", 0.1, F64_MAX, list(range(16, 0, -1)), [50 + (i * 7) % 5 for i in range(16)]),
    ]
    # the fused / unfused tuples as pairs: the second slot sits where the twice-rounded value would put it
    diff_rows = [r for r in rows if r[3] == 1]
    for i in range(0, 16, 2):
        (la, ra, da, _), (_lb, rb, db, _) = diff_rows[i], diff_rows[i + 1]
        tt_cases.append(("fused_pair_%d" % (i // 2), la, F64_MAX, [ra, rb, ra, rb, ra], [da, db, da + 1, db + 1, da]))
    names, rec = [], []
    for i, (name, lam, cur_best, rates_, dists_) in enumerate(tt_cases):
        nt = len(rates_)
        tx_size, bsize, mode, types = SHAPES[nt]
        inter = mode is NEARESTMV
        order = visited(tx_size, inter, types)
        assert len(order) == nt, (name, order)
        tsd = int(TxSize[tx_size].disc)
        cur["table"] = {(tsd, t): (int(r), int(d)) for t, r, d in zip(order, rates_, dists_)}
        cur.pop("at", None)
        del evals[:]
        ref = R.RSlice([LAST if inter else INTRA, INTRA])
        s = int(get_set({}, TxSize[tx_size], bool(inter), False).disc)
        tx_set = get_set({}, TxSize[tx_size], bool(inter), False)
        assert int(tx_set.disc) == s
        ty, rd = type_decision(g, make_fi(lam, i % 2), ts, Writer(), R.Some("checkpoint"), mode, ref, mvs, BlockSize[bsize],
                               bo, TxSize[tx_size], tx_set, types, float(cur_best))
        slot = -1 if float(rd) == F64_MAX else order.index(int(ty.disc))
        assert slot >= 0 or int(ty.disc) == 0
        names.append(name)
        rec.append((lam, cur_best, nt, rates_, dists_, slot, float(rd), len(evals)))
        print("tt", name, "nt", nt, "-> slot", slot, "rd", float(rd), "evals", len(evals), flush=True)
    n = len(rec)
    out["tt_names"] = np.array(names)
    out["tt_lam"] = np.array([r[0] for r in rec], np.float64)
    out["tt_cur"] = np.array([r[1] for r in rec], np.float64)
    out["tt_nt"] = np.array([r[2] for r in rec], np.int32)
    out["tt_rate"], out["tt_dist"] = np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint64)
    for i, r in enumerate(rec):
        out["tt_rate"][i, :r[2]], out["tt_dist"][i, :r[2]] = r[3], [int(v) for v in r[4]]
    out["tt_slot"] = np.array([r[5] for r in rec], np.int32)
    out["tt_rd"] = np.array([r[6] for r in rec], np.float64)
    out["tt_evals"] = np.array([r[7] for r in rec], np.int32)
    assert {int(v) for v in out["tt_nt"]} == {1, 2, 5, 7, 16}

    # ---------------- rdo_tx_size_type: an intra 16x16 block tries 16x16 (5 types), 8x8 (7), 4x4 (7); an 8x8 block
    # 8x8 and 4x4
    def flat(nt, rate, dist_):
        return [rate] * nt, [dist_] * nt
    sz_cases = [
        # name, lambda, block, per depth (rates, dists)
        ("depth0_wins", 8.0, 16, [flat(5, 8, 100), flat(7, 8, 120), flat(7, 8, 130)]),
        ("depth1_wins", 8.0, 16, [flat(5, 8, 100), ([8, 8, 8, 1, 8, 8, 8], [100, 100, 100, 90, 100, 100, 100]), flat(7, 8, 95)]),
        ("depth2_wins", 8.0, 16, [flat(5, 8, 100), ([8] * 7, [100, 90, 90, 90, 90, 90, 90]), ([0] * 7, [97, 60, 50, 50, 70, 50, 80])]),
        ("depth2_wins_over_depth0", 1.0, 16, [flat(5, 16, 50), flat(7, 16, 60), ([16, 16, 16, 16, 16, 16, 8], [50] * 7)]),
        ("none_after_depth0", 8.0, 16, [([9, 8, 8, 9, 9], [100, 100, 100, 100, 100]), flat(7, 8, 101), flat(7, 9, 100)]),
        ("exit_depth1_hides_lower_slot", 8.0, 16, [flat(5, 8, 100), ([8, 0, 0, 0, 0, 0, 0], [101, 1, 1, 1, 1, 1, 1]),
                                                   ([8, 0, 0, 0, 0, 0, 0], [93, 90, 99, 99, 99, 99, 99])]),
        ("exit_depth1_and_depth2", 8.0, 16, [flat(5, 8, 100), ([8, 0, 0, 0, 0, 0, 0], [101, 1, 1, 1, 1, 1, 1]),
                                             ([9, 0, 0, 0, 0, 0, 0], [100, 1, 1, 1, 1, 1, 1])]),
        ("tie_with_carried_keeps_depth0", 8.0, 16, [flat(5, 8, 100), ([8, 8, 0, 16, 16, 16, 16], [100, 100, 108, 100, 100, 100, 100]),
                                                    ([0] * 7, [108] * 7)]),
        ("slot0_equal_carried_no_exit", 8.0, 16, [flat(5, 8, 100), ([8, 8, 8, 8, 8, 8, 7], [100] * 7), flat(7, 16, 100)]),
        ("slot0_equal_carried_twice", 8.0, 16, [flat(5, 8, 100), ([8, 8, 8, 8, 8, 8, 8], [100] * 7), ([0, 0, 0, 0, 0, 0, 0], [108, 109, 109, 107, 109, 107, 109])]),
        ("lambda0", 0.0, 16, [([2 ** 32 - 2] * 5, [7, 6, 6, 7, 7]), ([0] * 7, [6, 1, 1, 1, 1, 1, 1]), ([0] * 7, [6, 5, 5, 5, 5, 5, 5])]),
        ("big_dist_rounding", 0.0, 16, [([0] * 5, [B + 3, B + 4, B + 4, B + 4, B + 4]), ([0] * 7, [B + 3] + [B + 2] * 6),
                                        ([0] * 7, [B + 1, B, B - 1, B, B, B, B])]),
        ("inexact_lambda", 1.0 / 3.0, 16, [([3, 6, 9, 1, 2], [100, 100, 99, 100, 100]), ([1, 1, 1, 1, 1, 1, 1], [100, 100, 100, 100, 100, 100, 99]),
                                           ([2, 1, 1, 1, 1, 1, 1], [99, 99, 99, 99, 99, 98, 98])]),
        ("block8_depth1_wins", 8.0, 8, [flat(7, 8, 100), ([8, 8, 8, 8, 8, 4, 4], [100] * 7)]),
        ("block8_exit", 8.0, 8, [([8, 8, 7, 8, 8, 8, 7], [100] * 7), ([8, 0, 0, 0, 0, 0, 0], [100, 0, 0, 0, 0, 0, 0])]),
    ]
    SIZES = {16: ["TX_16X16", "TX_8X8", "TX_4X4"], 8: ["TX_8X8", "TX_4X4"]}
    names, rec = [], []
    for i, (name, lam, blk, depths) in enumerate(sz_cases):
        sizes = SIZES[blk]
        orders = [visited(t, False, rav1e_types) for t in sizes]
        cur["table"] = {}
        for t, order, (rates_, dists_) in zip(sizes, orders, depths):
            assert len(order) == len(rates_) == len(dists_), (name, t, order)
            for ty, r, d in zip(order, rates_, dists_):
                cur["table"][(int(TxSize[t].disc), ty)] = (int(r), int(d))
        cur.pop("at", None)
        del evals[:]
        tx_size, tx_type = size_type(g, make_fi(lam, i % 2), ts, Writer(), BlockSize["BLOCK_%dX%d" % (blk, blk)], bo, DC_PRED,
                                     R.RSlice([INTRA, INTRA]), mvs, False)
        depth = [int(TxSize[t].disc) for t in sizes].index(int(tx_size.disc))
        slot = orders[depth].index(int(tx_type.disc))
        per_depth = [sum(1 for at, _ in evals if at[0] == int(TxSize[t].disc)) for t in sizes]
        rd = [v for at, v in evals if at == (int(tx_size.disc), int(tx_type.disc))][0]
        names.append(name)
        rec.append((lam, len(sizes), depths, depth, slot, rd, per_depth))
        print("sz", name, "-> depth", depth, "slot", slot, "rd", rd, "evals", per_depth, flush=True)
    n = len(rec)
    out["sz_names"] = np.array(names)
    out["sz_lam"] = np.array([r[0] for r in rec], np.float64)
    out["sz_ndepth"] = np.array([r[1] for r in rec], np.int32)
    out["sz_nt"] = np.zeros((n, 3), np.int32)
    out["sz_rate"], out["sz_dist"] = np.zeros((n, 3, 16), np.uint32), np.zeros((n, 3, 16), np.uint64)
    out["sz_evals"] = np.zeros((n, 3), np.int32)
    for i, r in enumerate(rec):
        for d, (rates_, dists_) in enumerate(r[2]):
            out["sz_nt"][i, d] = len(rates_)
            out["sz_rate"][i, d, :len(rates_)], out["sz_dist"][i, d, :len(rates_)] = rates_, [int(v) for v in dists_]
            out["sz_evals"][i, d] = r[6][d]
    out["sz_depth"] = np.array([r[3] for r in rec], np.int32)
    out["sz_slot"] = np.array([r[4] for r in rec], np.int32)
    out["sz_rd"] = np.array([r[5] for r in rec], np.float64)

    # ---------------- `rd < best` over executed costs (the mode loop; the loop itself is stated here)
    fm_cases = [
        # name, lambda, carried best_rd, rates, rate_adds, dists
        ("fm_tie_8_0_vs_0_8", 8.0, F64_MAX, [8, 0], [0, 0], [0, 8]),
        ("fm_add_decides", 8.0, F64_MAX, [8, 8, 8, 8], [3, 2, 2, 9], [50, 50, 50, 50]),
        ("fm_add_makes_tie", 8.0, F64_MAX, [8, 6, 7, 5], [0, 2, 1, 3], [10, 10, 10, 10]),
        ("fm_tie_with_carried", 8.0, c8, [0, 8, 16], [0, 0, 0], [8, 0, 9]),
        ("fm_below_carried", 8.0, c8, [0, 7, 16], [0, 0, 0], [8, 0, 9]),
        ("fm_all_above_carried", 1.0, 3.0, [8, 9, 10, 11, 12], [0] * 5, [3, 3, 3, 3, 3]),
        ("fm_lambda0", 0.0, F64_MAX, [2 ** 32 - 2, 1, 7, 8], [0, 5, 5, 5], [9, 9, 8, 8]),
        ("fm_add_to_u32_max_less_1", 1.0, F64_MAX, [2 ** 32 - 10, 8], [8, 2 ** 32 - 10], [0, 0]),
        ("fm_big_dist", 0.0, F64_MAX, [0] * 7, [0] * 7, [2 ** 64 - 1, big + 1, big + 2 ** 11, B + 3, B + 4, B + 1, B]),
        ("fm_sixteen", 0.1, F64_MAX, list(range(1, 17)), [16 - i for i in range(16)], [40 - (i % 4) for i in range(16)]),
        ("fm_inexact", 1.0 / 3.0, cost(1.0 / 3.0, 5, 99), [3, 6, 5, 4], [2, 0, 0, 0], [99, 99, 99, 99]),
    ]
    for i in range(16, 32, 4):
        q = diff_rows[i:i + 4]
        fm_cases.append(("fm_fused_%d" % (i // 4), q[0][0], F64_MAX, [r[1] for r in q], [0, 1, 0, 1], [r[2] for r in q]))
    n = len(fm_cases)
    out["fm_names"] = np.array([f[0] for f in fm_cases])
    out["fm_lam"] = np.array([f[1] for f in fm_cases], np.float64)
    out["fm_best_in"] = np.array([f[2] for f in fm_cases], np.float64)
    out["fm_n"] = np.array([len(f[3]) for f in fm_cases], np.int32)
    out["fm_rate"], out["fm_add"] = np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint32)
    out["fm_dist"], out["fm_rd"] = np.zeros((n, 16), np.uint64), np.zeros((n, 16), np.float64)
    out["fm_idx"] = np.zeros(n, np.int32)
    for i, (name, lam, best, rates_, adds, dists_) in enumerate(fm_cases):
        k, idx = len(rates_), -1
        out["fm_rate"][i, :k], out["fm_add"][i, :k], out["fm_dist"][i, :k] = rates_, adds, [int(v) for v in dists_]
        for j in range(k):
            rd = cost(lam, rates_[j] + adds[j], dists_[j])
            out["fm_rd"][i, j] = rd
            if rd < best:
                best, idx = rd, j
        out["fm_idx"][i] = idx
        print("fm", name, "-> idx", idx, flush=True)
    L.save("rd_pick_ref.npz", out)
    # self-checks, behind the save so that a mutated reference (docs/PARITY.md) still leaves its file to compare:
    # the function is fused -- what it returned is the exact value rounded once -- and every depth wins somewhere
    assert all(v == fused(*r[:3]) for v, r in zip(out["cost_rd"], rows))
    assert {int(v) for v in out["sz_depth"]} == {0, 1, 2}
    bits = lambda v: struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    print("cost tuples:", len(rows), "fused != twice-rounded:", n_diff, "first cost bits: %016x" % bits(out["cost_rd"][0]))


if __name__ == "__main__":
    main()

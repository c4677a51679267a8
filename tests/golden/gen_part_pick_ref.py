#!/usr/bin/env python3
"""tests/golden/part_pick_ref.npz: the partition decision -- the RD comparison a quad-tree node makes between coding
its block whole and coding it as two or four sub-blocks -- computed by the REFERENCE'S OWN SOURCE TEXT through
tools/rustlite.  It pins rdo_glue.partition_pick_bottomup / partition_pick_topdown and, through them,
r1_rd_partition_pick_batch.

Executed whole, unrewritten (no line of the reference text is changed):
  encode_partition_bottomup  src/encoder.rs:2633-2915   (recursion included)
  rdo_partition_decision     src/rdo.rs:1949-2024
  rdo_partition_simple       src/rdo.rs:1866-1940
  rdo_partition_none         src/rdo.rs:1849-1862
  get_sub_partitions         src/rdo.rs:1825-1846
  compute_rd_cost            src/rdo.rs:718-723
  BlockSize::subsize / width_mi / height_mi / is_sqr, FrameType::has_inter, ScaledDistortion::zero: real.

Scripted stand-ins for what they call (the numbers they would produce are the CASE's inputs):
  rdo_mode_decision          returns a PartitionParameters stand-in whose rd_cost is the case's cost of that
                             (bsize, offset); intra, so save_block_motion is never due
  cw.write_partition         advances the counting writer's tell_frac by the case's rate of that (offset, partition,
                             bsize); w_pre_cdef and w_post_cdef are the same counting writer, cw.bc.cdef_coded false
  encode_block_with_modes, save_block_motion   record their calls
  cw.checkpoint / rollback, the writers' checkpoint / rollback, cw.bc.update_partition_context   do nothing

What a trial left is READ, not restated: a profile hook (sys.setprofile) looks at the local variables of the executing
reference functions -- best_rd, best_partition, early_exit, must_split of encode_partition_bottomup when one of its
trials begins (its cw.rollback) and when it returns; best_rd / best_partition of rdo_partition_decision at the
cw.rollback behind each trial; the value rdo_partition_simple returns, with its has_cols / has_rows, which tells a
refusal by the early exit from one by an absent child.  A child's cost is what the nested call returned.

Keys (one row per trial, in the order the trials END -- the trials of a node's children lie between its own; a node's
first trial has t_first = 1, and t_best_in is what the node's previous trial left):
  t_case, t_node (row of the n_* arrays), t_first, t_rule (0 bottom-up, 1 top-down), t_partition, t_rate (-1: the 0.0
  arm), t_lam, t_ee (fi.enable_early_exit), t_must, t_ref (ref_rd_cost), t_child (n, 4): a cost, -1.0 = absent, -2.0 =
  never evaluated (the trial had ended: any value must do), t_best_in -> t_best_rd (the node's best_rd behind the
  trial; compare as bits), t_best_part (-1: PARTITION_INVALID), t_early (bottom-up: early_exit; top-down: refused by
  the early exit), t_kept
  n_case, n_bsize, n_x, n_y (mi units), n_rule, n_rd, n_part: every node evaluated, with what it returned; n_part_in:
  cached_block.part_type of a top-down node (-1 otherwise)
  c_names, c_family, c_rule, c_root (node row), c_mi_w, c_mi_h; e_case, e_bsize, e_x, e_y: the recorded
  encode_block_with_modes calls of each case in order -- what the selects must reproduce (the last call that covers a
  4x4 cell is what stands there)
  enum_partition_names / enum_partition_discs: PartitionType as the reference's text declares it (src/partition.rs:114-126)
  count_*: how many trials / cases of each required kind the file holds (the tests assert them as lower bounds)

Run in the build container:  python tests/golden/gen_part_pick_ref.py
"""
import random
import sys
import zlib
from fractions import Fraction

import numpy as np

import reflib as L
from reflib import R

F64_MAX = sys.float_info.max
ABSENT, UNEVALUATED = -1.0, -2.0


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def stub(c, name, fn):
    """the Python callable fn(_g, *args) in place of a reference function"""
    c.define_py("r1_stub_" + name, fn)
    c.fns[name] = [c.fns.pop("r1_stub_" + name)[0]]


def main():
    c = L.crate("partition.rs", "context/mod.rs", "util/mod.rs", "rdo.rs", "encoder.rs")
    c.define_enum("ChromaSampling", ["Cs420", "Cs422", "Cs444", "Cs400"])
    BS = {v[0]: L.enum(c, "BlockSize", v[0]) for v in c.enums["BlockSize"].variants}
    BS_BY_DISC = {int(v.disc): k for k, v in BS.items()}
    PT = {v[0]: L.enum(c, "PartitionType", v[0]) for v in c.enums["PartitionType"].variants}
    CS = {k: L.enum(c, "ChromaSampling", k) for k in ("Cs420", "Cs422", "Cs444")}
    KEY = L.enum(c, "FrameType", "KEY")
    RDO = L.enum(c, "RDOType", "PixelDistRealRate")
    TBO, BO = L.struct(c, "TileBlockOffset"), L.struct(c, "BlockOffset")
    PGP = L.struct(c, "PartitionGroupParameters")
    part_disc = lambda p: -1 if p.var == "PARTITION_INVALID" else int(p.disc)
    assert [part_disc(PT[k]) for k in ("PARTITION_NONE", "PARTITION_HORZ", "PARTITION_VERT", "PARTITION_SPLIT")] == [0, 1, 2, 3]

    cur = {}          # the running case: cost(bsize name, x, y), rate(x, y, partition disc, bsize name), the event log
    ev = []

    class Counter:    # w_pre_cdef and w_post_cdef
        def __init__(self):
            self.frac = 0

        def tell_frac(self):
            return self.frac

        def checkpoint(self):
            return "w"

        def rollback(self, _):
            return None

    class Writer:     # cw
        def __init__(self):
            self.bc = Obj(cdef_coded=False, update_partition_context=lambda *a: None)

        def checkpoint(self, *a):
            return "cw"

        def rollback(self, _):            # the profile hook reads the caller's locals here
            return None

        def write_partition(self, w, bo, partition, bsize):
            r = int(cur["rate"](int(bo._0.x), int(bo._0.y), part_disc(partition), BS_BY_DISC[int(bsize.disc)]))
            ev.append(("write_partition", part_disc(partition), r))
            on_symbol(part_disc(partition), r)
            w.frac += r

    def mode_decision(_g, fi, ts, cw, bsize, bo, inter_cfg):
        name = BS_BY_DISC[int(bsize.disc)]
        cost = float(cur["cost"](name, int(bo._0.x), int(bo._0.y)))
        ev.append(("mode", int(bsize.disc), int(bo._0.x), int(bo._0.y), cost))
        on_mode(int(bsize.disc), int(bo._0.x), int(bo._0.y), cost)
        return Obj(rd_cost=cost, bsize=bsize, bo=bo, pred_mode_luma=Obj(is_intra=lambda: True))

    stub(c, "rdo_mode_decision", mode_decision)
    stub(c, "encode_block_with_modes",
         lambda _g, *a: ev.append(("encode", int(a[5].disc), int(a[6]._0.x), int(a[6]._0.y))))
    stub(c, "save_block_motion", lambda _g, *a: ev.append(("motion",)))
    bottomup = c.get("encode_partition_bottomup")
    decision = c.get("rdo_partition_decision")

    # ---- the observer: the executing reference functions' own local variables, read while they run
    trials, nodes = [], []
    stack = []        # the encode_partition_bottomup calls in progress
    td = {}           # the rdo_partition_decision call in progress

    def snap_bu(fr):
        lo = fr.f_locals
        return (float(lo["best_rd"]), part_disc(lo["best_partition"]), bool(lo.get("early_exit", False)),
                bool(lo["must_split"]))

    def close(nd, state):
        """the node's open trial ends: `state` is what the reference holds behind it"""
        t = nd.pop("open", None)
        if t is None:
            return
        best, part, early, must = state
        # an entry the reference passed over lies outside the tile (encoder.rs:2802); one behind the child at which the
        # trial ended early was never looked at
        last = max(t["child"])
        child = [t["child"].get(k, UNEVALUATED if early and k > last else ABSENT) for k in range(4)]
        if t["partition"] in (1, 2):
            child[2] = child[3] = ABSENT
        trials.append(dict(case=cur["case"], node=nd["row"], first=int(not nd["n"]), rule=0, partition=t["partition"],
                           rate=t["rate"], lam=cur["lam"], ee=int(cur["ee"]), must=int(must), ref=nd["ref"], child=child,
                           best_in=nd["best"], best_rd=best, best_part=part, early=int(early),
                           kept=int(part == t["partition"])))
        nd["best"], nd["n"] = best, nd["n"] + 1

    def on_mode(bs, x, y, cost):
        if td:
            td["open"]["child"][len(td["open"]["child"])] = cost
            return
        nd = stack[-1]
        assert (nd["bs"], nd["x"], nd["y"]) == (bs, x, y)
        nd["open"] = dict(partition=0, rate=nd.pop("symbol", (0, -1))[1], child={0: cost})

    def on_symbol(partition, r):
        if td:
            if "open" in td and td["open"]["partition"] == partition and td["open"]["rate"] == -1 and not td["open"]["child"]:
                td["open"]["rate"] = r
            return                    # (else: a child's PARTITION_NONE symbol inside rdo_partition_simple)
        stack[-1]["symbol"] = (partition, r)

    def prof(fr, event, arg):
        name = fr.f_code.co_name
        if name.startswith("f_encode_partition_bottomup"):
            if event == "call":
                lo = fr.f_locals
                bs, x, y = int(lo["bsize"].disc), int(lo["tile_bo"]._0.x), int(lo["tile_bo"]._0.y)
                if stack:             # a child of the open trial: the symbol in front of the first one opened it
                    par = stack[-1]
                    if "open" not in par:
                        partition, r = par.pop("symbol")
                        par["open"] = dict(partition=partition, rate=r, child={})
                    k = {1: int(y > par["y"]), 2: int(x > par["x"]), 3: int(x > par["x"]) + 2 * int(y > par["y"])}[par["open"]["partition"]]
                    par["open"]["slot"] = k
                nodes.append([cur["case"], bs, x, y, 0, F64_MAX, -1, -1])
                stack.append(dict(row=len(nodes) - 1, bs=bs, x=x, y=y, ref=float(lo["ref_rd_cost"]), best=F64_MAX, n=0))
            elif event == "return":
                nd = stack.pop()
                if "must_split" in fr.f_locals:
                    close(nd, snap_bu(fr))
                nodes[nd["row"]][5], nodes[nd["row"]][6] = float(arg.rd_cost), part_disc(arg.part_type)
                if stack:
                    stack[-1]["open"]["child"][stack[-1]["open"].pop("slot")] = float(arg.rd_cost)
        elif name.startswith("f_rdo_partition_simple"):
            if event == "call":
                td["open"] = dict(partition=part_disc(fr.f_locals["partition"]), rate=-1, child={})
            elif event == "return":
                lo = fr.f_locals
                refused = isinstance(arg, R.REnum) and arg.var == "None"
                td["open"]["early"] = int(refused and bool(lo.get("has_cols")) and bool(lo.get("has_rows")))
                td["open"]["absent"] = int(refused and not td["open"]["early"])
        elif name.startswith("f_rdo_partition_none") and event == "call":
            td["open"] = dict(partition=0, rate=-1, child={}, early=0, absent=0)
        elif name == "rollback" and event == "call" and isinstance(fr.f_locals.get("self"), Writer):
            f = fr.f_back
            while not f.f_code.co_name.startswith(("f_encode_partition_bottomup", "f_rdo_partition_decision")):
                f = f.f_back
            if f.f_code.co_name.startswith("f_encode_partition_bottomup"):
                stack[-1].pop("symbol", None)
                close(stack[-1], snap_bu(f))
            else:
                t = td.pop("open")
                best, part = float(f.f_locals["best_rd"]), part_disc(f.f_locals["best_partition"])
                n_eval = len(t["child"])
                visited = {0: 1, 1: 2, 2: 2, 3: 4}[t["partition"]]
                child = [t["child"].get(k, UNEVALUATED) if k < visited else ABSENT for k in range(4)]
                if t["absent"]:
                    child[n_eval] = ABSENT
                trials.append(dict(case=cur["case"], node=td["row"], first=int(not td["n"]), rule=1, partition=t["partition"],
                                   rate=t["rate"], lam=cur["lam"], ee=int(cur["ee"]), must=0, ref=F64_MAX, child=child,
                                   best_in=td["best"], best_rd=best, best_part=part, early=t["early"],
                                   kept=int(part == t["partition"] and best != td["best"])))
                td["best"], td["n"] = best, td["n"] + 1

    def make_fi(lam, ee, cs="Cs420", pmin="BLOCK_8X8", pmax="BLOCK_64X64", nsq="BLOCK_8X8"):
        return Obj(lambda_=float(lam), enable_early_exit=bool(ee), frame_type=KEY, sequence=Obj(chroma_sampling=CS[cs]),
                   partition_range=Obj(min=BS[pmin], max=BS[pmax]),
                   config=Obj(speed_settings=Obj(partition=Obj(non_square_partition_max_threshold=BS[nsq]))))

    g = {"T": "u16", "W": "WriterCounter"}
    cases, encodes = [], []

    def run(name, family, rule, root, mi, lam, ee, cost, rate, ref=F64_MAX, cached=(F64_MAX, "PARTITION_INVALID"),
            types=("PARTITION_SPLIT", "PARTITION_NONE"), **fi_kw):
        """one case: `root` = (bsize name, x, y) in a tile of mi = (mi_width, mi_height)"""
        del ev[:]
        cur.update(case=len(cases), lam=float(lam), ee=bool(ee), cost=cost, rate=rate)
        fi, ts, cw, w = make_fi(lam, ee, **fi_kw), Obj(mi_width=mi[0], mi_height=mi[1]), Writer(), Counter()
        bo = TBO(BO(x=root[1], y=root[2]))
        first_node, first_trial = len(nodes), len(trials)
        sys.setprofile(prof)
        try:
            if rule == 0:
                out = bottomup(g, fi, ts, cw, w, w, BS[root[0]], bo, float(ref), Obj(), Obj())
            else:
                nodes.append([len(cases), int(BS[root[0]].disc), root[1], root[2], 1, F64_MAX, -1, part_disc(PT[cached[1]])])
                td.update(row=len(nodes) - 1, best=float(cached[0]), n=0)
                out = decision(g, fi, ts, cw, w, w, BS[root[0]], bo,
                               PGP(rd_cost=float(cached[0]), part_type=PT[cached[1]], part_modes=R.RSlice([])),
                               R.RSlice([PT[t] for t in types]), RDO, Obj())
                nodes[td["row"]][5], nodes[td["row"]][6] = float(out.rd_cost), part_disc(out.part_type)
                td.clear()
        finally:
            sys.setprofile(None)
        assert not stack and not td
        for e in ev:
            if e[0] == "encode":
                encodes.append((len(cases), e[1], e[2], e[3]))
        assert not any(e[0] == "motion" for e in ev)
        mine = trials[first_trial:]
        # what the function returned is what the last trial of its node left
        last = [t for t in mine if t["node"] == first_node][-1]
        assert (last["best_rd"], last["best_part"]) == (float(out.rd_cost), part_disc(out.part_type)), (name, last, out.rd_cost)
        cases.append(dict(name=name, family=family, rule=rule, root=first_node, mi=mi))
        print("%-34s %-6s rule %d: %3d nodes %3d trials -> %s rd %r" % (name, family, rule, len(nodes) - first_node, len(mine),
                                                                        part_disc(out.part_type), float(out.rd_cost)), flush=True)
        return mine

    rng = random.Random(20261021)
    DIM = lambda name: tuple(int(v) for v in name.split("_")[1].split("X"))

    # ---------------- trees: integer costs, lambdas and rates whose products are exact, so that nothing rounds and
    # only the cases built for an addition order or for a fused multiply can tell those apart
    def tree_cost(seed, scale, bias):
        def f(name, x, y):
            w, h = DIM(name)
            r = random.Random(zlib.crc32(repr((seed, name, x, y)).encode()))
            # per pixel between 1 and `scale`; whole blocks pay `bias` per cent more or less than their parts
            return float(int(w * h * r.randint(100, 100 * scale) * (100 + bias) // 100) * 7 + r.randint(0, 6))
        return f

    def tree_rate(seed):
        return lambda x, y, p, name: random.Random(zlib.crc32(repr((seed, x, y, p, name)).encode())).randint(1, 400) * 8

    TREES = [
        # name, root, mi, lambda, bias, with a twin without the early exit, kw
        ("tree64_full", ("BLOCK_64X64", 0, 0), (16, 16), 8.0, 0, False, {}),
        ("tree64_edge_w40_h24", ("BLOCK_64X64", 0, 0), (10, 6), 8.0, 0, True, {}),
        ("tree64_second_sb_w84_h36", ("BLOCK_64X64", 16, 0), (21, 9), 1.0, 0, False, {}),
        ("tree32_max16", ("BLOCK_32X32", 0, 0), (8, 8), 8.0, -20, False, dict(pmax="BLOCK_16X16")),
        ("tree32_nsq32", ("BLOCK_32X32", 0, 0), (8, 8), 8.0, 5, True, dict(nsq="BLOCK_32X32")),
        ("tree32_nsq32_422", ("BLOCK_32X32", 0, 0), (8, 8), 8.0, 5, True, dict(nsq="BLOCK_32X32", cs="Cs422")),
        ("tree32_nsq32_422_edge", ("BLOCK_32X32", 0, 0), (7, 5), 8.0, 0, False, dict(nsq="BLOCK_32X32", cs="Cs422")),
        ("tree32_nsq32_444_edge", ("BLOCK_32X32", 8, 8), (15, 13), 3.0, 0, False, dict(nsq="BLOCK_32X32", cs="Cs444")),
        ("tree16_min4", ("BLOCK_16X16", 0, 0), (4, 4), 8.0, 10, False, dict(pmin="BLOCK_4X4", nsq="BLOCK_16X16")),
        ("tree16_min4_edge", ("BLOCK_16X16", 0, 0), (3, 3), 8.0, 0, False, dict(pmin="BLOCK_4X4", nsq="BLOCK_16X16")),
        ("tree32_lambda0", ("BLOCK_32X32", 0, 0), (8, 8), 0.0, 0, False, dict(nsq="BLOCK_16X16")),
    ]
    for i, (name, root, mi, lam, bias, twin, kw) in enumerate(TREES):
        for ee in (True, False) if twin else (True,):
            run(name + ("" if ee else "_noexit"), "tree", 0, root, mi, lam, ee, tree_cost(i, 3, bias), tree_rate(i), **kw)
    # the same numbers through the top-down decision of one node: SPLIT then NONE, NONE then SPLIT, with HORZ and VERT,
    # from a cached whole block, at a frame edge (a simple partition with an absent child is refused)
    TD = [
        ("td32", ("BLOCK_32X32", 0, 0), (8, 8), 8.0, 0, {}),
        ("td32_parts_cheap", ("BLOCK_32X32", 0, 0), (8, 8), 2.0, 60, {}),
        ("td32_all_four", ("BLOCK_32X32", 0, 0), (8, 8), 8.0, 0, dict(types=("PARTITION_NONE", "PARTITION_HORZ", "PARTITION_VERT", "PARTITION_SPLIT"))),
        ("td16_all_four_parts_cheap", ("BLOCK_16X16", 4, 4), (16, 16), 4.0, 30, dict(types=("PARTITION_HORZ", "PARTITION_SPLIT", "PARTITION_VERT", "PARTITION_NONE"))),
        ("td64_edge_w56", ("BLOCK_64X64", 0, 0), (14, 16), 8.0, 0, {}),
        ("td64_edge_h40_horz_vert", ("BLOCK_64X64", 0, 0), (16, 10), 8.0, 0, dict(types=("PARTITION_HORZ", "PARTITION_VERT", "PARTITION_SPLIT", "PARTITION_NONE"))),
        ("td8_min4", ("BLOCK_8X8", 0, 0), (2, 2), 8.0, 20, {}),
        ("td32_lambda0", ("BLOCK_32X32", 0, 0), (8, 8), 0.0, 20, {}),
    ]
    for i, (name, root, mi, lam, bias, kw) in enumerate(TD):
        for ee in (True, False):
            run(name + ("" if ee else "_noexit"), "tree", 1, root, mi, lam, ee, tree_cost(100 + i, 3, bias), tree_rate(100 + i), **kw)
        # from a cached decision: the cached type is not tried again, its cost is what the others have to beat
        cost = tree_cost(100 + i, 3, bias)
        cached = cost(root[0], root[1], root[2])
        run(name + "_cached_none", "tree", 1, root, mi, lam, True, cost, tree_rate(100 + i), cached=(cached, "PARTITION_NONE"), **kw)

    # ---------------- one 16x16 node over 8x8 leaves whose own symbol costs nothing, so that the children's costs
    # are the numbers below as they stand.  (name, lambda, ref, whole, rate of NONE / HORZ / VERT / SPLIT, the four 8x8
    # costs; the halves of HORZ and VERT cost `half` each)
    def flat(whole, rates, quarters, half=1e6):
        def cost(name, x, y):
            if name == "BLOCK_16X16":
                return whole
            if name == "BLOCK_8X8":
                return quarters[(x > 0) + 2 * (y > 0)]
            return half[(x > 0) + (y > 0)] if isinstance(half, (list, tuple)) else half
        return cost, (lambda x, y, p, name: rates[p] if name == "BLOCK_16X16" else 0)

    R16 = ("BLOCK_16X16", 0, 0)
    NSQ = dict(nsq="BLOCK_16X16")
    FLAT = [
        # family tie: rd == best_rd keeps the earlier; with the early exit on, `>=` ends the trial there
        ("tie_split_equals_none", "tie", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (25.0, 25.0, 25.0, 25.0), {}),
        ("tie_at_second_child_then_zeros", "tie", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (50.0, 50.0, 0.0, 0.0), {}),
        ("tie_horz_equals_none", "tie", 1.0, F64_MAX, 64.0, (16, 16, 16, 800), (40.0,) * 4, dict(half=(32.0, 32.0), **NSQ)),
        ("tie_vert_equals_horz", "tie", 1.0, F64_MAX, 500.0, (16, 16, 16, 800), (40.0,) * 4, dict(half=(32.0, 32.0), **NSQ)),
        ("tie_with_ref", "tie", 8.0, 58.0, 100.0, (8, 999, 999, 8), (25.0, 25.0, 25.0, 25.0), {}),
        # family exit: each condition alone
        ("exit_on_best_at_child2", "exit", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (60.0, 60.0, 1.0, 1.0), {}),
        ("exit_on_best_at_last_child", "exit", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (30.0, 30.0, 30.0, 30.0), {}),
        ("exit_on_ref_below_best", "exit", 8.0, 50.0, 100.0, (8, 999, 999, 8), (20.0, 20.0, 20.0, 20.0), {}),
        ("exit_on_ref_at_first_child", "exit", 8.0, 10.0, 100.0, (8, 999, 999, 8), (20.0, 1.0, 1.0, 1.0), {}),
        ("exit_on_ref_horz_only", "exit", 8.0, 70.0, 100.0, (8, 8, 8, 8), (10.0,) * 4, dict(half=(40.0, 40.0), **NSQ)),
        ("no_exit_split_wins", "exit", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (20.0, 20.0, 20.0, 20.0), {}),
        ("no_exit_all_four_tried_vert_wins", "exit", 8.0, F64_MAX, 100.0, (8, 16, 8, 8), (30.0,) * 4, dict(half=(45.0, 44.0), **NSQ)),
        # family max: a child that returns f64::MAX is skipped
        ("child_max_skipped", "max", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (20.0, F64_MAX, 20.0, 20.0), {}),
        ("child_max_first_and_last", "max", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (F64_MAX, 20.0, 20.0, F64_MAX), {}),
        ("child_max_all", "max", 8.0, F64_MAX, 100.0, (8, 999, 999, 8), (F64_MAX,) * 4, {}),
        ("whole_max", "max", 8.0, F64_MAX, F64_MAX, (8, 999, 999, 8), (20.0, 20.0, 20.0, 20.0), {}),
        # family lambda0
        ("lambda0_rates_ignored", "lambda0", 0.0, F64_MAX, 100.0, (4000, 1, 1, 1), (25.0, 25.0, 25.0, 24.0), NSQ),
        ("tie_lambda0", "tie", 0.0, F64_MAX, 100.0, (1, 1, 1, 4000), (25.0, 25.0, 25.0, 25.0), {}),
    ]
    for name, family, lam, ref, whole, rates, quarters, kw in FLAT:
        kw = dict(kw)
        cost, rate = flat(whole, rates, quarters, kw.pop("half", 1e6))
        for ee in (True, False):
            run(name + ("" if ee else "_noexit"), family, 0, R16, (4, 4), lam, ee, cost, rate, ref=ref, **kw)
    # the same flat numbers top-down: the early exit is `sum > best_rd`, strictly, and the cost is not in the sum
    TDFLAT = [
        ("td_tie_sum_equals_best_no_exit", "tie", 8.0, (100.0, "PARTITION_NONE"), (8, 8, 8, 0), (25.0, 25.0, 25.0, 25.0)),
        ("td_tie_rd_equals_best", "tie", 8.0, (108.0, "PARTITION_NONE"), (8, 8, 8, 8), (25.0, 25.0, 25.0, 25.0)),
        ("td_exit_sum_above_best_at_child3", "exit", 8.0, (70.0, "PARTITION_NONE"), (8, 8, 8, 8), (25.0, 25.0, 25.0, 1.0)),
        ("td_exit_sum_above_best_at_last", "exit", 8.0, (99.0, "PARTITION_NONE"), (8, 8, 8, 8), (25.0, 25.0, 25.0, 25.0)),
        ("td_no_exit_cost_lifts_above_best", "exit", 8.0, (100.0, "PARTITION_NONE"), (8, 8, 8, 80), (25.0, 25.0, 25.0, 24.0)),
        ("td_split_wins", "exit", 8.0, (100.0, "PARTITION_NONE"), (8, 8, 8, 8), (20.0, 20.0, 20.0, 20.0)),
        ("td_child_max", "max", 8.0, (100.0, "PARTITION_NONE"), (8, 8, 8, 8), (20.0, F64_MAX, 20.0, 20.0)),
        ("td_lambda0", "lambda0", 0.0, (100.0, "PARTITION_NONE"), (8, 8, 8, 4000), (25.0, 25.0, 25.0, 24.0)),
    ]
    for name, family, lam, cached, rates, quarters in TDFLAT:
        cost, rate = flat(cached[0], rates, quarters)
        for ee in (True, False):
            run(name + ("" if ee else "_noexit"), family, 1, R16, (4, 4), lam, ee, cost, rate, cached=cached,
                types=("PARTITION_SPLIT",))

    # ---------------- tuples on which the two addition orders differ: ((cost + c0) + c1) + c2) + c3 against
    # cost + (((0 + c0) + c1) + c2) + c3).  lambda = 1 and a rate that is a multiple of 8 make the cost an integer
    # that no fused multiply can change; the children are fractions.  Found by evaluating both orders exactly
    # (Fraction) and rounding at every step as f64 does
    def rnd(fr):
        return float(fr)          # Fraction -> f64 rounds to nearest even

    def order_bu(cost, ch):
        rd = cost
        for v in ch:
            rd = rnd(Fraction(rd) + Fraction(v))
        return rd

    def order_td(cost, ch):
        sm = 0.0
        for v in ch:
            sm = rnd(Fraction(sm) + Fraction(v))
        return rnd(Fraction(cost) + Fraction(sm))

    n_order = 0
    while n_order < 12:
        r8 = rng.randint(1, 5000)
        ch = tuple(rng.uniform(1.0, 10.0 ** rng.randint(1, 6)) for _ in range(4))
        if order_bu(float(r8), ch) == order_td(float(r8), ch):
            continue
        whole = 2.0 * (sum(ch) + r8)        # the whole block loses, so that the sum itself is what is kept
        cost, rate = flat(whole, (0, 0, 0, r8 * 8), ch)
        a = run("order_%d_bottomup" % n_order, "order", 0, R16, (4, 4), 1.0, False, cost, rate)
        b = run("order_%d_topdown" % n_order, "order", 1, R16, (4, 4), 1.0, False, cost, rate,
                cached=(F64_MAX, "PARTITION_INVALID"), types=("PARTITION_SPLIT",))
        assert a[-1]["best_rd"] == order_bu(float(r8), ch) and b[-1]["best_rd"] == order_td(float(r8), ch)
        assert a[-1]["best_rd"] != b[-1]["best_rd"]
        n_order += 1

    # ---------------- tuples on which fusing the multiply into the first addition differs:
    # fma(lambda, rate / 8, c0) != round(lambda * rate / 8) + c0.  Bottom-up the whole-block trial (c0 + cost, one
    # addition: no order to swap); top-down HORZ over (c0, 0.0): cost + (c0 + 0).  No tie, no early exit
    n_fused = 0
    while n_fused < 12:
        lam = rng.choice([rng.uniform(0.01, 300.0), rng.uniform(1e3, 1e6), 0.1 * rng.randint(1, 100)])
        r = rng.randint(1, 1 << rng.randint(4, 20))
        c0 = rng.uniform(1.0, 10.0 ** rng.randint(1, 7))
        cst = rnd(Fraction(lam) * Fraction(r, 8))
        twice = rnd(Fraction(cst) + Fraction(c0))
        fused = rnd(Fraction(lam) * Fraction(r, 8) + Fraction(c0))
        if twice == fused:
            continue
        cost, rate = flat(c0, (r, r, r, r), (c0, 0.0, 0.0, 0.0), half=(c0, 0.0))
        a = run("fused_%d_bottomup" % n_fused, "fused", 0, R16, (4, 4), lam, False, cost, rate, pmin="BLOCK_16X16")
        b = run("fused_%d_topdown" % n_fused, "fused", 1, R16, (8, 8), lam, False, cost, rate, types=("PARTITION_HORZ",))
        assert a[-1]["best_rd"] == twice and b[-1]["best_rd"] == twice, (a[-1]["best_rd"], b[-1]["best_rd"], twice, fused)
        n_fused += 1

    # ---------------- the file
    out = {}
    n = len(trials)
    for key, dt in (("case", np.int32), ("node", np.int32), ("first", np.uint8), ("rule", np.uint8), ("partition", np.int8),
                    ("rate", np.int64), ("lam", np.float64), ("ee", np.uint8), ("must", np.uint8), ("ref", np.float64),
                    ("best_in", np.float64), ("best_rd", np.float64), ("best_part", np.int8), ("early", np.uint8),
                    ("kept", np.uint8)):
        out["t_" + key] = np.array([t[key] for t in trials], dt)
    out["t_child"] = np.array([t["child"] for t in trials], np.float64).reshape(n, 4)
    nd = np.array([r[:5] + [r[6], r[7]] for r in nodes], np.int32)
    for k, key in enumerate(("case", "bsize", "x", "y", "rule", "part", "part_in")):
        out["n_" + key] = nd[:, k].copy()
    out["n_rd"] = np.array([r[5] for r in nodes], np.float64)
    out["enum_partition_names"] = np.array([v[0] for v in c.enums["PartitionType"].variants])
    out["enum_partition_discs"] = np.array([int(PT[v[0]].disc) for v in c.enums["PartitionType"].variants], np.int32)
    out["c_names"] = np.array([cs["name"] for cs in cases])
    out["c_family"] = np.array([cs["family"] for cs in cases])
    out["c_rule"] = np.array([cs["rule"] for cs in cases], np.uint8)
    out["c_root"] = np.array([cs["root"] for cs in cases], np.int32)
    out["c_mi_w"] = np.array([cs["mi"][0] for cs in cases], np.int32)
    out["c_mi_h"] = np.array([cs["mi"][1] for cs in cases], np.int32)
    en = np.array(encodes, np.int32).reshape(-1, 4)
    for k, key in enumerate(("case", "bsize", "x", "y")):
        out["e_" + key] = en[:, k].copy()
    T = out
    bu, tdn = T["t_rule"] == 0, T["t_rule"] == 1
    fam = out["c_family"][T["t_case"]]
    present = T["t_child"] >= 0
    simple = T["t_partition"] > 0
    counts = {
        "trials": n, "cases": len(cases), "nodes": len(nodes),
        "trees_64_to_8": len({int(cs) for cs in T["t_case"][(out["n_bsize"][T["t_node"]] == int(BS["BLOCK_8X8"].disc))]} &
                             {i for i, cs in enumerate(cases) if int(nodes[cs["root"]][1]) == int(BS["BLOCK_64X64"].disc)}),
        "must_split": int((T["t_must"] == 1).sum()),
        "absent_child": int((simple & bu & (T["t_child"] == ABSENT)[:, [0, 1]].any(1)).sum() +
                            (simple & bu & (T["t_partition"] == 3) & (T["t_child"] == ABSENT).any(1)).sum()),
        "td_absent_refused": int((tdn & simple & (T["t_child"] == ABSENT)[:, :2].any(1)).sum()),
        "cs422_nodes_without_vert": len({c_ for c_, nm in enumerate(out["c_names"]) if "422" in str(nm)}),
        "tie": int((fam == "tie").sum()),
        "exit_best": int((bu & (T["t_early"] == 1) & (T["t_ref"] == F64_MAX)).sum()),
        "exit_ref": int((bu & (T["t_early"] == 1) & (T["t_ref"] != F64_MAX)).sum()),
        "exit_topdown": int((tdn & (T["t_early"] == 1)).sum()),
        "noexit_twins": int((T["t_ee"] == 0).sum()),
        "child_max": int(((T["t_child"] == F64_MAX).any(1)).sum()),
        "lambda0": int((T["t_lam"] == 0.0).sum()),
        "order_differs": n_order, "fused_differs": n_fused,
        "rate_none_arm": int((T["t_rate"] < 0).sum()),
    }
    for k, v in counts.items():
        out["count_" + k] = np.array(v, np.int32)
        print("count_%s = %d" % (k, v))
    L.save("part_pick_ref.npz", out)
    assert all(v > 0 for v in counts.values()), counts


if __name__ == "__main__":
    main()

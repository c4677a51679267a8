"""What tests/test_mvref_ref.py and tests/test_gpu_mvref.py share: the fixture tests/golden/mvref_ref.npz as tiles and
records, and LOCAL COPIES of rdo_glue.find_mvrefs with one behaviour switched off (the sensitivity tests): the copy is the
statement's own text with one stated edit, so it cannot drift from the statement."""
import inspect
import os

import numpy as np

from rav1e_amd import rdo_glue as G
from rav1e_amd.types import MV_BLOCK, MV_QUERY, MV_STACK, MV_TRIAL, MVREF_REFUSED, TILE_BLOCK

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    return dict(np.load(os.path.join(HERE, "golden", "mvref_ref.npz")))


class Rows:
    def __init__(self, fx, rows, cols):
        self.a, self.names = fx[rows], [str(c) for c in fx[cols]]

    def __len__(self):
        return len(self.a)

    def __call__(self, k):
        return {n: int(v) for n, v in zip(self.names, self.a[k])}


FX = load_fixture()
SEQS = Rows(FX, "seq_rows", "seq_cols")
EVS = Rows(FX, "ev_rows", "ev_cols")
QS = Rows(FX, "q_rows", "q_cols")
TAGS = [str(t) for t in FX["tag_names"]]
SIGN_BIAS = [int(v) for v in FX["sign_bias"]]


def cells_of(snap):
    """a snapshot as a fresh (rows, cols) array of TILE_BLOCK"""
    a = FX["snap_%d" % snap]
    return np.ascontiguousarray(a).view(TILE_BLOCK).reshape(a.shape[0], a.shape[1]).copy()


def tile_of(si, cells):
    s = SEQS(si)
    assert cells.shape == (s["rows"], s["cols"])
    return {"cells": cells, "tile_x": s["tile_x"], "tile_y": s["tile_y"], "frame_cols": s["frame_cols"], "frame_rows": s["frame_rows"]}


def fresh_tile(si):
    s = SEQS(si)
    return tile_of(si, G.tile_blocks_default(s["rows"], s["cols"]))


def tagged(name):
    k = TAGS.index(name)
    return {i for i in range(len(QS)) if (int(FX["q_rows"][i][10]) >> k) & 1}


def want_q(i):
    """the fixture's answer to single query i, in the statement's form"""
    r = QS(i)
    return r["mode_context"], [tuple(int(v) for v in e) for e in FX["q_stack"][i][:r["count"]]]


def want_sq(i):
    r = FX["sq_rows"][i]
    return int(r[3]), [tuple(int(v) for v in e) for e in FX["sq_stack"][i][:int(r[4])]]


def stack_record(res):
    """a statement's answer as an MV_STACK record (count 0xFF and nothing else for a refusal)"""
    rec = np.zeros((), MV_STACK)
    if res == G.MV_REFUSED:
        rec["count"] = MVREF_REFUSED
        return rec
    ctx, st = res
    rec["count"], rec["mode_context"] = len(st), ctx
    for k, e in enumerate(st):
        rec["cand"][k]["this_mv"], rec["cand"][k]["comp_mv"], rec["cand"][k]["weight"] = e[:2], e[2:4], e[4]
    return rec


def trial_record(block, mode, refs, mvs, skip):
    t = np.zeros((), MV_TRIAL)
    t["block"], t["mode"], t["ref_frames"], t["skip"], t["mv"] = block, mode, refs, skip, mvs
    return t


def event_winner(ev):
    return ev["mode"], (ev["ref0"], ev["ref1"]), ((ev["mv0_row"], ev["mv0_col"]), (ev["mv1_row"], ev["mv1_col"])), ev["skip"]


# ---- one behaviour off: (text of the statement, what stands in its place)
EDITS = {
    "sort_ascending": [("stack.sort(key=lambda e: -e[4])", "stack.sort(key=lambda e: e[4])")],
    # a sort that is not stable: equal weights come out in the opposite order
    "sort_unstable": [("stack.sort(key=lambda e: -e[4])", "stack.reverse(); stack.sort(key=lambda e: -e[4])")],
    "no_add_offset": [("e[4] += REF_CAT_LEVEL", "e[4] += 0")],
    "processed_ignored": [('st["rows" if horizontal else "cols"] = inc - offset - 1', "pass")],
    "full_stack_match_not_counted": [("                    stack.append(list(key) + [weight])\n",
                                      "                    stack.append(list(key) + [weight])\n"
                                      "                else:\n                    return False\n")],
    "clamp_tile_relative": [('fx, fy = int(tile["tile_x"]) + bo_x, int(tile["tile_y"]) + bo_y', "fx, fy = bo_x, bo_y")],
    "no_odd_arm": [("if (pos & 1) and target < 2:", "if False:")],
    "no_step_16": [("if target >= 16:", "if False:")],
    "one_ref_of_a_neighbour": [("for i in range(2) if refs[i] == r0]", "for i in range(1) if refs[i] == r0]")],
    "no_sign_bias": [("if bool(sign_bias[cand_ref - 1]) != bool(sign_bias[r0 - 1]):", "if False:"),
                     ("flip = bool(sign_bias[cand_ref - 1]) != bool(sign_bias[want - 1])", "flip = False")],
    "no_extra_dedupe": [("if all((e[0], e[1]) != mv for e in stack):", "if True:")],
    "no_extra_search": [("if len(stack) < 2:  ", "if False:  ")],
    "tr_never": [("if has_tr(bo_x, bo_y, bsize) and bo_y > 0:", "if False:")],
    "min_weight_dropped": [("weight = max(weight, inc)", "weight = inc")],
}


def mutant(name):
    src = inspect.getsource(G.find_mvrefs)
    for old, new in EDITS[name]:
        assert src.count(old) == 1, (name, old)
        src = src.replace(old, new)
    ns = dict(G.__dict__)
    exec(compile(src, "<find_mvrefs without %s>" % name, "exec"), ns)
    return ns["find_mvrefs"]


def run_singles(find=None):
    """every single query of the fixture through `find` -> the list of answers"""
    find = find or G.find_mvrefs
    out, tiles = [], {}
    for i in range(len(QS)):
        r = QS(i)
        if r["snap"] not in tiles:
            tiles[r["snap"]] = tile_of(r["seq"], cells_of(r["snap"]))
        out.append(find(tiles[r["snap"]], r["bo_x"], r["bo_y"], r["bsize"], (r["ref0"], r["ref1"]), r["is_compound"], SIGN_BIAS))
    return out


def singles_moved(find=None):
    return {i for i, got in enumerate(run_singles(find)) if got != want_q(i)}


def blocks_and_queries(items):
    """[(tile index, bo_x, bo_y, bsize, [(ref0, ref1, is_compound), ..]), ..] -> (MV_BLOCK array, MV_QUERY array)"""
    nq = sum(len(it[4]) for it in items)
    blocks, queries = np.zeros(len(items), MV_BLOCK), np.zeros(nq, MV_QUERY)
    q = 0
    for b, (tile, x, y, bsize, qs) in enumerate(items):
        blocks[b] = (tile, x, y, bsize, len(qs), 0, q)
        for (r0, r1, comp) in qs:
            queries[q] = (b, (r0, r1), comp, 0)
            q += 1
    return blocks, queries

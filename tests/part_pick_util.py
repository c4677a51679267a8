"""What tests/test_part_pick_ref.py and tests/test_gpu_part_pick.py share: the fixture's trials as Python values, and a
copy of the two host statements (rdo_glue.partition_pick_bottomup / partition_pick_topdown) with the three switches of
the mutation checks docs/PARITY.md lists."""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_MAX = sys.float_info.max
ABSENT, UNEVALUATED = -1.0, -2.0
# a child the reference never looked at, because the trial had ended: any cost must do, and this one would show
NEVER = 12345.0
VISITED = {0: 1, 1: 2, 2: 2, 3: 4}


def load():
    return np.load(os.path.join(ROOT, "tests", "golden", "part_pick_ref.npz"))


def bits(v):
    return np.array(v, np.float64).view(np.uint64)


def children(ref, i):
    """trial i's four entries: a cost, or None for an absent one"""
    return [None if v == ABSENT else NEVER if v == UNEVALUATED else float(v) for v in ref["t_child"][i]]


def rate(ref, i):
    return None if int(ref["t_rate"][i]) < 0 else int(ref["t_rate"][i])


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def model(rule, best_rd, partition, lam, r, kids, must, ref_rd, ee, ge=True, swap=False, fuse=False):
    """-> (kept, rd, early).  ge=False: the bottom-up early exit with `>` for `>=`.  swap: each rule adds in the OTHER
    rule's order.  fuse: the multiply of the cost fused into the first addition it meets."""
    r8 = 0.0 if r is None else r / 8.0          # exact
    cost = 0.0 if r is None else fma(lam, r8, 0.0)
    kids = list(kids)[:VISITED[partition]]
    if partition == 0:
        if kids[0] is None:
            return False, 0.0, False
        if rule == 1:
            return kids[0] < best_rd, kids[0], False
        return True, (fma(lam, r8, kids[0]) if fuse and r is not None else kids[0] + cost), False
    cost_first = (rule == 0) != swap            # ((cost + c0) + c1) + ...   against   cost + (((0 + c0) + c1) + ...)
    total, n_added, rd = 0.0, 0, cost
    for c in kids:
        if c is None:
            if rule == 1:
                return False, total, False
            continue
        if rule == 0 and c == F64_MAX:
            continue
        if cost_first:
            rd = fma(lam, r8, c) if fuse and r is not None and n_added == 0 else rd + c
        total = total + c
        n_added += 1
        if not cost_first:
            rd = fma(lam, r8, total) if fuse and r is not None else cost + total
        if rule == 0:
            over = (rd >= best_rd or rd >= ref_rd) if ge else (rd > best_rd or rd > ref_rd)
            if not must and ee and over:
                return False, rd, True
        elif ee and total > best_rd:
            return False, total, True
    return rd < best_rd, rd, False


def replay(ref, fn):
    """every trial through fn(i) -> (kept, rd, early): the names of the cases where a trial's outcome -- best_rd as
    bits, best_partition, the early-exit flag -- is not the recorded one"""
    moved = set()
    for i in range(len(ref["t_case"])):
        kept, rd, early = fn(i)
        best = rd if kept else float(ref["t_best_in"][i])
        part = int(ref["t_partition"][i]) if kept else None
        ok = bits(best) == bits(ref["t_best_rd"][i]) and int(early) == int(ref["t_early"][i]) and \
            int(kept) == int(ref["t_kept"][i]) and (part is None or part == int(ref["t_best_part"][i]))
        if not ok:
            moved.add(str(ref["c_names"][ref["t_case"][i]]))
    return moved


def model_trial(ref, i, **kw):
    return model(int(ref["t_rule"][i]), float(ref["t_best_in"][i]), int(ref["t_partition"][i]), float(ref["t_lam"][i]),
                 rate(ref, i), children(ref, i), bool(ref["t_must"][i]), float(ref["t_ref"][i]), bool(ref["t_ee"][i]), **kw)


# ---- the closed loop: one 16x16 node of a tile, coded whole and as four 8x8
def node_cases():
    """(whole, split): two tile_chain_util cases over the same 16x16 pixels, CDFs, quantizer and lambda -- one 16x16
    block (transform depths 16x16, 8x8), four 8x8 blocks in coding order (8x8, 4x4) -- cut out of the first case of
    tests/golden/tile_chain_ref.npz (8 bits).  Only the inputs are taken: what they decide is computed by
    tile_chain_util.host_chain and by the device chain"""
    import tile_chain_util as TC
    from rav1e_amd import rdo_glue as RG
    base = TC.load()[0]
    assert base.bd == 8 and base.bs == 16
    full = [0, 1, 2, 3, 9, 10, 11]

    def make(bs, sizes, nt, types, blocks):
        c = object.__new__(TC.Case)
        c.name = "node16_b%d" % bs
        c.bd, c.w, c.h, c.bs, c.k, c.qindex, c.lam = 8, 16, 16, bs, base.k, base.qindex, base.lam
        c.ts0, c.ts1 = sizes
        c.nblocks = len(blocks)
        c.src, c.rec0 = base.src[:16, :16].copy(), base.rec0[:16, :16].copy()
        c.modes, c.cdf0 = base.modes, base.cdf0
        c.nt, c.types = np.array(nt, base.nt.dtype), np.array(types, base.types.dtype)
        c.blocks = np.array(blocks, base.blocks.dtype)
        c.rate_add = base.rate_add[:len(blocks)].copy()
        c.qc = np.zeros(0, base.qc.dtype)
        c.sizes = sizes
        c.t = (TC.SU.TX_SIDE[sizes[0]], TC.SU.TX_SIDE[sizes[1]])
        c.ntx = (1, 4)
        c.masks = tuple(sum(1 << int(t) for t in c.types[d][:c.nt[d]]) for d in range(2))
        c.mi_w, c.mi_h = 4, 4
        c.bsize = RG.block_size(bs, bs)
        c.dt = np.uint8
        return c
    whole = make(16, base.sizes, base.nt.tolist(), base.types.tolist(), [[0, 0, 1]])
    split = make(8, (1, 0), [7, 7], [full, full], [[0, 0, 1], [8, 0, 0], [0, 8, 0], [8, 8, 0]])
    return whole, split

"""Reader of tests/golden/fwd_tx_ref.npz (gen_fwd_tx_ref.py: `forward_transform` executed whole from
the reference's text).  Shared by test_fwd_tx_ref.py and test_gpu_fwd_tx_ref.py; loaded once."""
import functools
import os
from collections import namedtuple

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_tx_ref.npz")
BITDEPTHS = (8, 10, 12)

# res: (nb, h, w) int16 residual blocks; coef: (nb, w * h) T::Coeff; stats: (nb, 3) mulmax, colmax, cmax
Case = namedtuple("Case", "bd ts tt w h res coef stats names")


@functools.lru_cache(maxsize=None)
def load():
    """-> {bit depth: [Case, ...]} in (tx_size, tx_type) order.  Arrays are read-only."""
    G = np.load(PATH)
    names = [str(s) for s in G["blocks"]]
    out = {bd: [] for bd in BITDEPTHS}
    pos = {bd: [0, 0, 0] for bd in BITDEPTHS}      # cursor into shared / sign / coef
    arrs = {bd: (G["shared_%d" % bd], G["sign_%d" % bd], G["coef_%d" % bd]) for bd in BITDEPTHS}
    shared_of = {}
    for row, st in zip(G["cases"], G["stats"]):
        bd, ts, tt, nb, w, h = (int(v) for v in row)
        shared, sign, coef = arrs[bd]
        p = pos[bd]
        if (bd, ts) not in shared_of:
            n = (nb - 1) * w * h
            shared_of[bd, ts] = shared[p[0]:p[0] + n].reshape(nb - 1, h, w)
            p[0] += n
        sg = sign[p[1]:p[1] + w * h].reshape(1, h, w)
        p[1] += w * h
        co = coef[p[2]:p[2] + nb * w * h].reshape(nb, w * h)
        p[2] += nb * w * h
        res = np.concatenate([sg, shared_of[bd, ts]])
        for a in (res, co):
            a.setflags(write=False)
        out[bd].append(Case(bd, ts, tt, w, h, res, co, st[:nb], names[:nb]))
    for bd in BITDEPTHS:
        assert pos[bd] == [len(a) for a in arrs[bd]], "fwd_tx_ref.npz: layout and case table disagree"
    return out


def tiled(case, n):
    """the case's blocks repeated round-robin up to n: (res (n, h, w), coef (n, w * h))"""
    idx = np.arange(n) % len(case.res)
    return np.ascontiguousarray(case.res[idx]), np.ascontiguousarray(case.coef[idx])

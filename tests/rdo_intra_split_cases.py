"""tests/golden/rdo_intra_split_ref.npz (tests/golden/gen_rdo_intra_split_ref.py: the reference's encode_tx_block
executed once per transform block of an intra block, in write_tx_blocks' order, on one tile state) as test cases."""
import os

import numpy as np

import oracle_lib as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdo_intra_split_ref.npz")
TX_SIDE = (4, 8, 16, 32)
# compute_distortion's four runs: (dist_kind, with the scale grid)
DIST_RUNS = ((2, False), (3, False), (2, True), (3, True))


class Case:
    def __init__(self, G, i):
        cols = [str(c) for c in G["columns"]]
        for name, v in zip(cols, G["cases"][i]):
            setattr(self, name, int(v))
        self.i = i
        self.t = TX_SIDE[self.ts]
        self.gw, self.gh = self.bw // self.t, self.bh // self.t
        self.ntx = self.gw * self.gh
        self.dt = np.uint8 if self.bd == 8 else np.uint16
        for k in ("src", "nb", "tr", "bl", "eob", "txd", "qc", "rec", "dist", "scales"):
            setattr(self, k, G["%s_%d" % (k, i)])
        self.tile = (0, 0, self.plane_w, self.plane_h)
        mi_w, mi_h = (self.plane_w + 3) >> 2, (self.plane_h + 3) >> 2
        self.coded_mask = np.zeros((self.bh, self.bw), bool)     # the pixels of transform blocks that are not skipped
        self.skipped = np.zeros(self.ntx, bool)
        for k in range(self.ntx):
            xk, yk = (k % self.gw) * self.t, (k // self.gw) * self.t
            if ((self.x + xk) >> 2) >= mi_w or ((self.y + yk) >> 2) >= mi_h:
                self.skipped[k] = True
            else:
                self.coded_mask[yk:yk + self.t, xk:xk + self.t] = True
        assert int((~self.skipped).sum()) == self.coded
        self.vis_w, self.vis_h = min(self.bw, self.plane_w - self.x), min(self.bh, self.plane_h - self.y)
        self.inside = self.vis_w == self.bw and self.vis_h == self.bh

    def rec_plane(self):
        """the plane with the recorded neighbourhood in place; what the edges cannot reach holds a constant"""
        p = O.HostPlane(self.plane_w, self.plane_h, self.bd, fill=(1 << self.bd) - 3)
        v = p.view()
        v[self.nb_y:self.nb_y + self.nb.shape[0], self.nb_x:self.nb_x + self.nb.shape[1]] = self.nb
        return p

    def org_plane(self):
        """the source block at its place (a block cut by the frame edge continues into the padding)"""
        p = O.HostPlane(self.plane_w, self.plane_h, self.bd, fill=1 << (self.bd - 1))
        y0, x0 = p.yorigin + self.y, p.xorigin + self.x
        p.data[y0:y0 + self.bh, x0:x0 + self.bw] = self.src
        return p

    def blocks(self):
        """the argument of rdo_glue.intra_split_cands"""
        return [(self.x, self.y, self.mode, self.angle_delta, self.ief, self.tr.tolist(), self.bl.tolist())]

    def masks(self):
        return (sum(1 << k for k in range(self.ntx) if self.tr[k]), sum(1 << k for k in range(self.ntx) if self.bl[k]))


def load():
    G = np.load(PATH)
    return [Case(G, i) for i in range(len(G["cases"]))]

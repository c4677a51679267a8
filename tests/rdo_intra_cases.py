"""tests/golden/rdo_intra_ref.npz (gen_rdo_intra_ref.py: the reference's encode_tx_block executed with intra modes)
turned into the inputs of the project's entry points -- shared by the host test (oracle composition) and the GPU
test (r1_intra_edges_batch -> r1_rdo_intra_cand_batch)."""
import os

import numpy as np

import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdo_intra_ref.npz")
TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
MODE_ANGLE = [0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0, 0]
# dist_i of the fixture: compute_distortion for (Tune::Psnr, Psychovisual) x (no scale grid, scale grid)
DIST_RUNS = ((2, False), (3, False), (2, True), (3, True))


class Case:
    def __init__(self, G, i):
        cols = [str(c) for c in G["columns"]]
        for name, v in zip(cols, G["cases"][i]):
            setattr(self, name, int(v))
        self.i = i
        self.w, self.h = TX_W[self.ts], TX_H[self.ts]
        self.dt = np.uint8 if self.bd == 8 else np.uint16
        for k in ("src", "edge", "pred", "rec", "qc", "dist", "txd", "scales"):
            setattr(self, k, G["%s_%d" % (k, i)])
        self.nbt = G["nbt_%d" % i] if "nbt_%d" % i in G.files else None
        self.nbl = G["nbl_%d" % i] if "nbl_%d" % i in G.files else None
        self.ac = G["ac_%d" % i] if "ac_%d" % i in G.files else None
        self.chroma = self.dec == 1
        # the whole block lies inside the plane: compute_distortion measured all of it
        self.inside = self.x + self.w <= self.plane_w and self.y + self.h <= self.plane_h
        # PredictionMode::predict_intra's remaps (src/predict.rs:205-249): what the R1IntraCand carries
        x, y = self.x, self.y
        self.variant = 0 if (x == 0 and y == 0) else (1 if y == 0 else (2 if x == 0 else 3))
        m = self.mode
        if m == 12:
            m = (0, 2, 1, 12)[self.variant]
        if m == 13 and self.alpha == 0:
            m = 0
        self.pmode = m
        self.angle = self.alpha if m == 13 else MODE_ANGLE[m] + 3 * self.angle_delta
        self.avail_w = min(self.w, self.plane_w - x)
        self.avail_h = min(self.h, self.plane_h - y)

    def _plane(self):
        return O.HostPlane(self.plane_w, self.plane_h, self.bd, 88, 88)

    def rec_plane(self):
        """a plane that holds the recorded neighbourhood (everything get_intra_edges can reach), zero elsewhere"""
        p = self._plane()
        v = p.view()
        if self.nbt is not None:
            v[self.y - 1, self.nb_x:self.nb_x + len(self.nbt)] = self.nbt
        if self.nbl is not None:
            v[self.nb_y:self.nb_y + len(self.nbl), self.x - 1] = self.nbl
        return p

    def org_plane(self):
        """the source block at its place (a block cut by the frame edge reaches into the padding)"""
        p = self._plane()
        p.data[p.yorigin + self.y:p.yorigin + self.y + self.h, p.xorigin + self.x:p.xorigin + self.x + self.w] = self.src
        return p

    def scale_grid(self):
        """the fixture's grid, widened so that a block cut by the frame edge stays inside it"""
        s = self.scales
        g = np.full((s.shape[0] + 8, s.shape[1] + 8), 1 << 14, np.uint32)
        g[:s.shape[0], :s.shape[1]] = s
        return g

    def edge_cand(self, shared=False):
        from rav1e_amd.api import INTRA_EDGE_CAND
        c = np.zeros(1, INTRA_EDGE_CAND)
        c["x"], c["y"] = self.x, self.y
        c["mode"], c["angle_delta"] = (-1, 0) if shared else (self.mode, self.angle_delta)
        c["flags"] = self.enable_ief | self.has_tr << 1 | self.has_bl << 2
        return c

    def intra_cand(self):
        from rav1e_amd.api import INTRA_CAND
        c = np.zeros(1, INTRA_CAND)
        c["mode"], c["variant"], c["angle"], c["ief"] = self.pmode, self.variant, self.angle, self.ief
        c["avail_w"], c["avail_h"] = self.avail_w, self.avail_h
        return c

    def rdo_cand(self):
        c = np.zeros(1, O.RDO_CAND)
        c["ox"], c["oy"] = self.x, self.y
        return c


def load():
    G = np.load(GOLD)
    return [Case(G, i) for i in range(len(G["cases"]))]

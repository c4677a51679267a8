"""The closed three-depth intra decision as a chain of launches with no host read in it: search -> rate -> pick at
16x16 / 8x8 / 4x4, the pick over the modes, the three commits.  tests/test_gpu_rd_pick.py holds it to the host
statements; tools/bench_rd_pick.py times it against the route through the host (and adds that route itself)."""
import numpy as np

MODES = (0, 1, 2, 9)                      # DC_PRED, V_PRED, H_PRED, SMOOTH_PRED: no mode that needs an edge set of its own
BASE_ANGLE = {0: 0, 1: 90, 2: 180, 9: 0}
MASK = 0x0E0F                             # RAV1E_TX_TYPES
S = 16                                    # the block
DEPTH_TX = (2, 1, 0)                      # TX_16X16, TX_8X8, TX_4X4
DEPTH_NTX = (1, 4, 16)
CALL_MODE = 3                             # call_id of the pick over the modes


class Chain:
    """search -> rate -> pick at three depths, the pick over the modes, the commits.  Blocks at (bx[i], by[i]) of
    org / rec (multiples of 16); the winners' reconstructions go to `dst`."""

    def __init__(self, ctx, org, rec, dst, bx, by, qindex=100, lam=203.25, seed=1):
        import torch
        import coeff_rate_model as M
        from rav1e_amd import rdo_glue as RG
        from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND, INTRA_SPLIT_CAND
        from rav1e_amd.types import TXB_CHAIN_CTX
        self.torch, self.ctx, self.org, self.rec, self.dst = torch, ctx, org, rec, dst
        self.qindex, self.lam = qindex, float(lam)
        K = self.K = len(MODES)
        nb = self.nb = len(bx)
        n = self.n = nb * K
        self.nt = bin(MASK).count("1")
        fw, fh = rec.width, rec.height
        self.tile = (0, 0, fw, fh)
        rng = np.random.default_rng(seed)
        x, y = np.repeat(bx, K), np.repeat(by, K)                # candidate c = block * K + mode index
        mode = np.tile(np.array(MODES), nb)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        ec = np.zeros(nb, INTRA_EDGE_CAND)
        ec["x"], ec["y"], ec["mode"], ec["flags"] = bx, by, -1, 1
        self.d_edge = dev(ec)
        var = np.where((x == 0) & (y == 0), 0, np.where(y == 0, 1, np.where(x == 0, 2, 3)))
        ic = np.zeros(n, INTRA_CAND)
        ic["mode"], ic["variant"], ic["angle"] = mode, var, [BASE_ANGLE[m] for m in mode]
        ic["avail_w"], ic["avail_h"] = np.minimum(S, fw - x), np.minimum(S, fh - y)
        self.d_cand = dev(ic)
        self.pos = torch.from_numpy(np.stack([bx, by], 1).astype(np.int16)).cuda()
        self.d_split = []
        for d in (1, 2):
            sc = np.zeros(n, INTRA_SPLIT_CAND)
            sc["x"], sc["y"], sc["mode"] = x, y, mode
            sc["tr_mask"], sc["bl_mask"] = rng.integers(0, 1 << DEPTH_NTX[d], n), rng.integers(0, 1 << DEPTH_NTX[d], n)
            self.d_split.append(dev(sc))
        above, left = rng.integers(0, 64, fw // 4 + 16).tolist(), rng.integers(0, 64, 32).tolist()
        ch = np.array([RG.txb_chain_ctx(above, left, int(xx) >> 2, int(yy) >> 2, S, S, fw >> 2, fh >> 2, fw >> 2, fh >> 2,
                                        int(m), i % 2) for i, (xx, yy, m) in enumerate(zip(x, y, mode))], TXB_CHAIN_CTX)
        self.d_chain = dev(ch)
        # depth 0 asks the chain call for the 7 types the candidate call ran: the inter set of 16x16 holds them (the
        # intra one only 5); the set only selects the tx_type CDF row
        self.inter = (True, False, False)
        self.d_cdfs = [dev(M.random_cdfs(rng, 2, DEPTH_TX[d], int(self.inter[d]), 0)) for d in range(3)]
        self.rate_add = torch.from_numpy(rng.integers(0, 400, n).astype(np.int32)).cuda()
        self.search, self.rate = [{}, {}, {}], [{}, {}, {}]
        self.win = {}
        self.ar16, self.ar_nb = torch.arange(S, device="cuda"), torch.arange(nb, device="cuda")
        self.st0, self.blk0 = ctx.rd_pick_state(n), ctx.rd_pick_state(nb)     # fresh states, cloned on the device per pass

    # ---- the six launches in front of the decision
    def launches(self, d):
        ctx = self.ctx
        if d == 0:
            edges, lens = ctx.intra_edges_batch(self.rec, self.tile, DEPTH_TX[0], self.d_edge, n=self.nb)
            o = ctx.rdo_intra_cand_batch(self.org, S, S, self.d_cand, self.pos, edges, lens, MASK, self.qindex, 2,
                                         edge_group=self.K, n=self.n, want_qcoeffs=True, want_rec=True, outs=self.search[0])
        else:
            o = ctx.rdo_intra_split_batch(self.org, self.rec, self.tile, S, S, DEPTH_TX[d], self.d_split[d - 1], MASK,
                                          self.qindex, 2, n=self.n, want_qcoeffs=True, want_rec=True, outs=self.search[d])
        self.search[d] = o
        self.rate[d] = ctx.coeff_rate_chain_batch(o["qcoeffs"], o["eob"], MASK, S, S, DEPTH_TX[d], 0, self.inter[d],
                                                  self.d_chain, self.d_cdfs[d], want_txb_rate=False, want_cul_level=False,
                                                  outs=self.rate[d])

    def new_wins(self):
        torch = self.torch
        return {"eob_win": torch.full((self.nb, 16), 0x5A5A, dtype=torch.int16, device="cuda"),
                "qcoeffs_win": torch.full((self.nb, S * S), 0x5A5A, dtype=self.search[0]["qcoeffs"].dtype, device="cuda"),
                "side_win": torch.full((self.nb, 32), 0x5A, dtype=torch.uint8, device="cuda")}

    def device_route(self, search=True, wins=None):
        torch, ctx, K, nt = self.torch, self.ctx, self.K, self.nt
        st = self.st0.clone()
        for d in range(3):
            if search:
                self.launches(d)
            ctx.rd_pick_batch(self.rate[d]["rate"], self.search[d]["dist"], st, 1, nt, self.lam, rule=1, call_id=d)
        # the mode states' rate (offset 16) and distortion (offset 8) as the dense arrays the pick over the modes reads.
        # A mode state that kept nothing holds rate 0 and distortion 0 and would cost its rate_add alone: it is handed
        # on as the invalid rate 0xFFFFFFFF, which costs +infinity
        kept = st.view(torch.int8)[:, 23] >= 0
        mode_rate = torch.where(kept, st.view(torch.int32)[:, 4], torch.full_like(st.view(torch.int32)[:, 4], -1))
        blk = self.blk0.clone()
        ctx.rd_pick_batch(mode_rate.contiguous(), st.view(torch.int64)[:, 1].contiguous(), blk, K, 1,
                          self.lam, rule=0, call_id=CALL_MODE, rate_add=self.rate_add)
        # the winning mode's state per block, its row = the mode: trial (block * K + mode) * nt + slot of its depth
        m = blk.view(torch.int16)[:, 10].to(torch.int64).clamp(min=0)
        win = st.view(self.nb, K, 24)[self.ar_nb, m].contiguous()
        win.view(torch.int16)[:, 10] = m.to(torch.int16)
        o = wins if wins is not None else self.win
        for d in range(3):
            o = ctx.rd_commit_batch(win, d, K, nt, coeffs=(self.search[d]["eob"], self.search[d]["qcoeffs"]),
                                    ntx=DEPTH_NTX[d], order=0, side=self.rate[d]["ctx"], rec_trials=self.search[d]["rec"],
                                    rec=self.dst, pos_xy=self.pos, outs=o)
        if wins is None:
            self.win = o
        return st, blk, win, o

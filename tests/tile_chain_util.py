"""tests/golden/tile_chain_ref.npz (gen_tile_chain_ref.py) as test cases, and the carried intra decision loop of a tile
built twice from what exists without the fixture:

  host_chain     the oracle's pixel composition (intra_split_util.oracle_split on a host plane the loop writes winners
                 into), the coefficient models (coeff_rate_block_model, coeff_cdf_model) and the product's host glue
                 (rdo_glue.block_chain_ctx, coeff_nbr_store, coeff_nbr_reset_left, tx_size_type_decision -> pick_tx_type,
                 pick_first_min, winner_tx_type).  Three switches take one carry out each (the sensitivity tests).
  DeviceChain    the chain of INTEGRATION.md, section 4 ("... from block to block, without the host"): every launch of every block of one or
                 more tiles enqueued on one stream with no host read, device clones of the plane, the CDF context and
                 the neighbour context behind every block.

Both return the fixture's per-block arrays under the fixture's names (`ARRAYS`), so one comparison serves both.
"""
import os

import numpy as np

import coeff_cdf_model as DM
import coeff_rate_block_model as BM
import intra_split_util as SU
import oracle_lib as O
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import BLOCK_CHAIN_CTX

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_chain_ref.npz")
TRIAL_ARRAYS = ("eob", "qc", "rate", "dist", "rd")
DECISION_ARRAYS = ("mode_pick", "mode_rd", "win", "best_rd")
STATE_ARRAYS = ("ctx_in", "ctx_out", "cdf", "above", "left", "rec")
ARRAYS = TRIAL_ARRAYS + DECISION_ARRAYS + STATE_ARRAYS
NT, NTX = 7, 4


class Case:
    def __init__(self, G, i):
        self.name = str(G["names"][i])
        for k, v in zip((str(c) for c in G["columns"]), G["cases"][i]):
            setattr(self, k, int(v))
        for k in ARRAYS + ("src", "rec0", "final", "modes", "nt", "types", "blocks", "rate_add", "cdf0", "carry", "counts"):
            setattr(self, k, G[self.name + "_" + k])
        self.lam = float(G[self.name + "_lam"])
        self.counts = dict(zip((str(c) for c in G["count_names"]), (int(v) for v in self.counts)))
        self.sizes = (self.ts0, self.ts1)
        self.t = (SU.TX_SIDE[self.ts0], SU.TX_SIDE[self.ts1])
        self.ntx = (1, 4)
        self.masks = tuple(sum(1 << int(t) for t in self.types[d][:self.nt[d]]) for d in range(2))
        self.mi_w, self.mi_h = self.w >> 2, self.h >> 2
        self.bsize = RG.block_size(self.bs, self.bs)
        self.dt = np.uint8 if self.bd == 8 else np.uint16

    def planes(self):
        """(org, rec) host planes: the source and what lies in the plane before the tile is coded; the padding holds a
        constant no prediction may read (every edge beyond the tile is unavailable)"""
        org = O.HostPlane(self.w, self.h, self.bd, fill=1 << (self.bd - 1))
        rec = O.HostPlane(self.w, self.h, self.bd, fill=(1 << self.bd) - 3)
        org.view()[:], rec.view()[:] = self.src, self.rec0
        return org, rec

    def split_cands(self, d, x, y):
        """the K descriptors of depth d for the block at tile position (x, y): rdo_glue.intra_split_masks, the ief of a
        directional mode among plain neighbours"""
        tr, bl = RG.intra_split_masks(self.bs, self.bs, self.sizes[d], x >> 2, y >> 2, x, y, self.w, self.h)
        c = np.zeros(self.k, SU.SPLIT_CAND)
        for i, m in enumerate(self.modes):
            c[i] = (x, y, int(m), 0, int(1 <= int(m) <= 8), 0, tr, bl)
        return c

    def block_records(self, above, left, x, y):
        return np.array([RG.block_chain_ctx(above, left, x >> 2, y >> 2, self.bsize, 1, 1, self.mi_w, self.mi_h, self.mi_w,
                                            self.mi_h, int(m), 0, 0) for m in self.modes], BLOCK_CHAIN_CTX)

    def empty(self):
        nb, K, bs = self.nblocks, self.k, self.bs
        return dict(eob=np.zeros((nb, K, 2, NT, NTX), np.uint16), qc=np.zeros((nb, K, 2, NT, bs * bs), self.qc.dtype),
                    rate=np.zeros((nb, K, 2, NT), np.uint32), dist=np.zeros((nb, K, 2, NT), np.uint64),
                    rd=np.zeros((nb, K, 2, NT), np.float64), mode_pick=np.zeros((nb, K, 2), np.int8),
                    mode_rd=np.zeros((nb, K), np.float64), win=np.zeros((nb, 4), np.int32), best_rd=np.zeros(nb, np.uint64),
                    ctx_in=np.zeros((nb, 96), np.uint8), ctx_out=np.zeros((nb, 96), np.uint8),
                    cdf=np.zeros((nb, 3930), np.uint16), above=np.zeros((nb, 3, 1024), np.uint8),
                    left=np.zeros((nb, 3, 16), np.uint8), rec=np.zeros((nb, bs, bs), self.dt))


def load():
    G = np.load(PATH)
    return [Case(G, i) for i in range(len(G["names"]))]


def moved(case, got, arrays=ARRAYS):
    """{array name: the blocks at which `got` differs from the fixture}"""
    out = {}
    for k in arrays:
        want, have = getattr(case, k), got[k]
        assert want.shape == have.shape and want.dtype == have.dtype, (case.name, k, want.shape, have.shape, want.dtype, have.dtype)
        out[k] = [b for b in range(case.nblocks) if want[b].tobytes() != have[b].tobytes()]
    return out


def decide(case, bi, rates, dists):
    """the decision of one block from its trials' rates and distortions [K][2][NT]: the type loop with its early exit and
    the depth carry per mode, then `rd < best` over the modes with rate_add -> (mode_pick [K][2], mode_rd [K], win [4],
    best_rd bits)"""
    picks, mode_rd, best_rates, best_dists = [], [], [], []
    for mi in range(case.k):
        per_r = [[int(v) for v in rates[mi][d][:case.nt[d]]] for d in range(2)]
        per_d = [[int(v) for v in dists[mi][d][:case.nt[d]]] for d in range(2)]
        depth, slot, _rd = RG.tx_size_type_decision(per_r, per_d, case.lam)
        picks.append((depth, slot))
        best_rates.append(per_r[depth][slot])
        best_dists.append(per_d[depth][slot])
        mode_rd.append(RG.compute_rd_cost(case.lam, per_r[depth][slot] + int(case.rate_add[bi, mi]),
                                          RG.dist_as_f64(per_d[depth][slot])))
    idx, best, _rate, _dist = RG.pick_first_min(best_rates, best_dists, case.lam, rate_adds=[int(v) for v in case.rate_add[bi]])
    depth, slot = picks[idx]
    tx_type, _uv = RG.winner_tx_type(slot, case.masks[depth], 0)
    return picks, mode_rd, (idx, depth, slot, tx_type), int(np.array(best, np.float64).view(np.uint64))


def host_chain(case, L, write_back=True, cdf_carry=True, nbr_store=True):
    """the loop on the host.  write_back / cdf_carry / nbr_store = False: the winner's reconstruction, its adapted CDFs
    or its context spans are dropped instead of carried"""
    c = case
    org, rec = c.planes()
    tile = (0, 0, c.w, c.h)
    above, left = np.zeros((3, 1024), np.uint8), np.zeros((3, 16), np.uint8)
    cdf = np.array(DM.context_from_packed(c.cdf0))
    out = c.empty()
    for bi, (x, y, reset) in enumerate(c.blocks.tolist()):
        if reset:
            RG.coeff_nbr_reset_left(left)
        blk = c.block_records(above, left, x, y)
        out["ctx_in"][bi] = blk[0]["ctx"].reshape(96)
        searched, side = [], {}
        for d, ts in enumerate(c.sizes):
            o = SU.oracle_split(L, org, rec, tile, c.bs, c.bs, ts, c.split_cands(d, x, y), True, c.masks[d], c.qindex, 2)
            searched.append(o)
            slices = np.stack([DM.gather(cdf, ts, 0, 0, 0)])
            nt, ntx = int(c.nt[d]), c.ntx[d]
            out["eob"][bi, :, d, :nt, :ntx] = o["eob"]
            out["qc"][bi, :, d, :nt] = o["qcoeffs"].reshape(c.k, nt, -1)
            out["dist"][bi, :, d, :nt] = o["dist"]
            for mi in range(c.k):
                for slot in range(nt):
                    trial = np.array([RG.block_rate_trial(0, 0, 0, 0, int(c.types[d][slot]), 0, False)], BM.TRIAL_DTYPE)[0]
                    r = BM.coeff_rate_block([o["qcoeffs"][mi, slot], [], []], [o["eob"][mi, slot], [], []], c.bs, c.bs, ts, 1, 1,
                                            0, 0, trial, blk[mi], slices)
                    assert r["rate"] != BM.INVALID
                    out["rate"][bi, mi, d, slot] = r["rate"]
                    out["rd"][bi, mi, d, slot] = RG.compute_rd_cost(c.lam, r["rate"], RG.dist_as_f64(int(o["dist"][mi, slot])))
                    side[(mi, d, slot)] = (trial, r["ctx"])
        picks, mode_rd, win, best_bits = decide(c, bi, out["rate"][bi], out["dist"][bi])
        out["mode_pick"][bi], out["mode_rd"][bi], out["win"][bi], out["best_rd"][bi] = picks, mode_rd, win, best_bits
        mi, d, slot, _tt = win
        o = searched[d]
        if write_back:
            rec.view()[y:y + c.bs, x:x + c.bs] = o["rec"][mi, slot]
        trial, ctx_behind = side[(mi, d, slot)]
        if cdf_carry:
            r = DM.adapt(cdf, [o["qcoeffs"][mi, slot], [], []], [o["eob"][mi, slot], [], []], c.bs, c.bs, c.sizes[d], 1, 1, 0, 0,
                         trial, blk[mi])
            assert r["rate"] == int(out["rate"][bi, mi, d, slot]) and r["ctx"] == ctx_behind
        if nbr_store:
            assert RG.coeff_nbr_store(above, left, x >> 2, y >> 2, c.bsize, 1, 1, False, False,
                                      np.array(ctx_behind, np.uint8).reshape(3, 2, 16))
        out["ctx_out"][bi] = ctx_behind
        out["cdf"][bi], out["above"][bi], out["left"][bi] = DM.packed_of(cdf), above, left
        out["rec"][bi] = rec.view()[y:y + c.bs, x:x + c.bs]
    out["final"] = rec.view().copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
BASE_ANGLE = (0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0)
CALL_MODE = 3                               # call_id of the pick over the modes


class DeviceChain:
    """One or more tiles side by side in one plane, tile s = cases[s] (same geometry, quantizer and lambda) at plane
    column s * w: block k of every tile in one step.  The candidate launches run per tile (the tile rectangle is an
    argument of theirs); gather, slice, rates, picks, commit, winner type, adapt and store take all tiles in one launch
    each, so one commit stores one block per tile into the plane the next step's launches predict from.
    dorg / drec: device planes (any layout) of width len(cases) * w; dcdf / dnbr: (S, 7872) / (S, 3120) uint8 device
    views of the tiles' CDF and neighbour contexts."""

    def __init__(self, ctx, cases, dorg, drec, dcdf, dnbr, write_back=True):
        import torch
        from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND
        from rav1e_amd.types import BLOCK_RATE_TRIAL, NBR_BLOCK
        c = self.c = cases[0]
        for o in cases[1:]:
            assert (o.bd, o.w, o.h, o.bs, o.k, o.qindex, o.lam) == (c.bd, c.w, c.h, c.bs, c.k, c.qindex, c.lam)
            assert o.modes.tolist() == c.modes.tolist() and o.blocks.tolist() == c.blocks.tolist()
        self.torch, self.ctx, self.cases, self.S = torch, ctx, cases, len(cases)
        self.dorg, self.drec, self.dcdf, self.dnbr = dorg, drec, dcdf, dnbr
        self.write_back = write_back        # False: the commit leaves the plane alone (the sensitivity test)
        self.n = self.S * c.k
        self.uv_ts = int(RG.largest_chroma_tx_size(c.bsize, 1, 1))
        self.ar = torch.arange(self.S, device="cuda")
        self.rate_add = [torch.from_numpy(np.concatenate([o.rate_add[bi] for o in cases]).astype(np.uint32).view(np.int32)).cuda()
                         for bi in range(c.nblocks)]
        self.types = (INTRA_CAND, INTRA_EDGE_CAND, BLOCK_RATE_TRIAL, NBR_BLOCK)
        # the trial arrays of the two rate calls: trial (candidate i, slot j) reads the candidate call's transform blocks
        # at (i * nt + j) * ntx, the gathered record i, the type of slot j
        self.trials = []
        for d in range(2):
            nt, ntx = int(c.nt[d]), c.ntx[d]
            tr = np.array([RG.block_rate_trial((i * nt + j) * ntx, 0, 0, i, int(c.types[d][j]), 0, False)
                           for i in range(self.n) for j in range(nt)], BLOCK_RATE_TRIAL)
            self.trials.append(self._dev(tr))
        self.steps = []

    def _dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()

    def step(self, bi):
        torch, ctx, c, S, K, n = self.torch, self.ctx, self.c, self.S, self.c.k, self.n
        INTRA_CAND, INTRA_EDGE_CAND, BLOCK_RATE_TRIAL, NBR_BLOCK = self.types
        x, y, reset = (int(v) for v in c.blocks[bi])
        bs = c.bs
        if reset:
            ctx.coeff_nbr_reset_left_batch(self.dnbr, list(range(S)), 3)
        # 1. gather: one desc per (tile, mode) on the tile's context; cdf_sel = the tile's slice
        descs = np.array([RG.nbr_block(s, x >> 2, y >> 2, c.mi_w, c.mi_h, c.mi_w, c.mi_h, int(m), s, 0, False, False)
                          for s in range(S) for m in c.modes], NBR_BLOCK)
        blocks = ctx.coeff_nbr_gather_batch(self.dnbr, descs, bs, bs, 1, 1)["blocks"]
        # 2. the candidate launches on the live plane, per tile
        search = [[], []]
        tr0, bl0 = RG.intra_split_masks(bs, bs, c.ts0, x >> 2, y >> 2, x, y, c.w, c.h)
        var = 0 if (x == 0 and y == 0) else (1 if y == 0 else (2 if x == 0 else 3))
        for s in range(S):
            tile = (s * c.w, 0, c.w, c.h)
            ec, ic = np.zeros(K, INTRA_EDGE_CAND), np.zeros(K, INTRA_CAND)
            for i, m in enumerate(int(v) for v in c.modes):
                ec[i] = (x, y, m, 0, 1 | (tr0 << 1) | (bl0 << 2), 0)
                pm = {0: 0, 2: 1, 1: 2, 3: 12}[var] if m == 12 else m        # Paeth at a tile edge (predict.rs:141-148)
                ic[i] = (pm, var, BASE_ANGLE[pm], int(1 <= m <= 8), bs, bs, 0)
            edges, lens = ctx.intra_edges_batch(self.drec, tile, c.ts0, ec)
            pos = torch.tensor([[s * c.w + x, y]] * K, dtype=torch.int16, device="cuda")
            search[0].append(ctx.rdo_intra_cand_batch(self.dorg, bs, bs, ic, pos, edges, lens, c.masks[0], c.qindex, 2,
                                                      want_qcoeffs=True, want_rec=True))
            search[1].append(ctx.rdo_intra_split_batch(self.dorg, self.drec, tile, bs, bs, c.ts1, c.split_cands(1, x, y),
                                                       c.masks[1], c.qindex, 2, want_qcoeffs=True, want_rec=True))
        o = [{k: torch.cat([t[k] for t in search[d]]).contiguous() for k in ("eob", "dist", "qcoeffs", "rec")} for d in range(2)]
        # 3. slice, 4. rates, 5. the picks per depth on the (tile, mode) states
        st = ctx.rd_pick_state(n)
        rates = []
        for d, ts in enumerate(c.sizes):
            cdfs = ctx.coeff_cdf_slice_batch(self.dcdf, ts, 0, 0, 0)
            ro = ctx.coeff_rate_block_batch(o[d]["qcoeffs"].view(-1), o[d]["eob"].view(-1), 1, None, 1, self.trials[d], bs, bs, ts,
                                            1, 1, 0, blocks.view(-1), cdfs, want_plane_rate=False, want_rng=False,
                                            want_cul_level=False)
            rates.append(ro)
            ctx.rd_pick_batch(ro["rate"], o[d]["dist"].view(-1), st, 1, int(c.nt[d]), c.lam, rule=1, call_id=d)
        # the pick over the modes (rate_add: the head symbols), then the winning mode's state per tile, its row = the mode
        blk = ctx.rd_pick_state(S)
        ctx.rd_pick_batch(st.view(torch.int32)[:, 4].contiguous(), st.view(torch.int64)[:, 1].contiguous(), blk, K, 1, c.lam,
                          rule=0, call_id=CALL_MODE, rate_add=self.rate_add[bi])
        m = blk.view(torch.int16)[:, 10].to(torch.int64).clamp(min=0)
        win = st.view(S, K, 24)[self.ar, m].contiguous()
        win.view(torch.int16)[:, 10] = m.to(torch.int16)
        win_blocks = blocks.view(S, K, -1)[self.ar, m].contiguous()
        pos = torch.tensor([[s * c.w + x, y] for s in range(S)], dtype=torch.int16, device="cuda")
        store_descs = np.array([RG.nbr_block(s, x >> 2, y >> 2, c.mi_w, c.mi_h, c.mi_w, c.mi_h, 0, s, 0, False, False)
                                for s in range(S)], NBR_BLOCK)
        wins, win_trials, adapts = [], [], []
        for d, ts in enumerate(c.sizes):
            nt, ntx, area = int(c.nt[d]), c.ntx[d], min(c.t[d], 32) ** 2
            w = {"eob_win": torch.full((S, 16), 0x5A5A, dtype=torch.int16, device="cuda"),
                 "qcoeffs_win": torch.zeros((S, 16 * area), dtype=o[d]["qcoeffs"].dtype, device="cuda"),
                 "side_win": torch.full((S, 96), 0x5A, dtype=torch.uint8, device="cuda")}
            # 6. commit: the winner's reconstruction into the SAME plane the next step's launches read
            w = ctx.rd_commit_batch(win, d, K, nt, coeffs=(o[d]["eob"].view(-1), o[d]["qcoeffs"].view(-1)), ntx=ntx, order=0,
                                    side=rates[d]["ctx"].view(n * nt, 96),
                                    rec_trials=o[d]["rec"].view(n * nt, bs, bs) if self.write_back else None,
                                    rec=self.drec, pos_xy=pos, store_w=self.drec.width, store_h=self.drec.height, outs=w)
            wt = np.array([RG.block_rate_trial(s * 16, 0, 0, s, 15, 0, False) for s in range(S)], BLOCK_RATE_TRIAL)
            dwt = self._dev(wt)
            ctx.rd_winner_tx_type_batch(win, d, c.masks[d], 0, self.uv_ts, dwt)                              # 7.
            ao = ctx.coeff_cdf_adapt_batch(w["qcoeffs_win"].view(-1), w["eob_win"].view(-1), 1, None, 1, dwt.view(-1), bs, bs, ts,
                                           1, 1, 0, win_blocks.view(-1), self.dcdf, state=win, call_id=d)    # 8.
            ctx.coeff_nbr_store_batch(self.dnbr, store_descs, bs, bs, ts, 1, 1, ctx_in=w["side_win"].view(-1), state=win,
                                      call_id=d)                                                             # 9.
            wins.append(w)
            win_trials.append(dwt)
            adapts.append(ao)
        self.steps.append(dict(blocks=blocks, o=o, rates=rates, st=st, blk=blk, win=win, wins=wins, win_trials=win_trials,
                               adapts=adapts, plane=self.drec.buf.clone(), cdf=self.dcdf.clone(), nbr=self.dnbr.clone()))

    def run(self):
        for bi in range(self.c.nblocks):
            self.step(bi)
        self.torch.cuda.synchronize()                    # the first host read of the case
        return self

    def results(self, s):
        """tile s as the fixture's arrays (`ARRAYS` less rd and mode_rd, which no launch writes out), plus
        `state_rd` (n, K): the rd each mode's state kept, `adapt_rate` (n): the winner's replayed rate"""
        from rav1e_amd.types import BLOCK_RATE_TRIAL, COEFF_NBR_CONTEXT, RD_PICK
        c, K = self.cases[s], self.c.k
        out = c.empty()
        out["state_rd"], out["adapt_rate"] = np.zeros((c.nblocks, K), np.float64), np.zeros(c.nblocks, np.uint32)
        p = self.drec
        for bi, t in enumerate(self.steps):
            x, y, _ = (int(v) for v in c.blocks[bi])
            for d in range(2):
                nt, ntx = int(c.nt[d]), c.ntx[d]
                o = t["o"][d]
                sl = slice(s * K, (s + 1) * K)
                out["eob"][bi, :, d, :nt, :ntx] = o["eob"].cpu().numpy().view(np.uint16).reshape(-1, nt, ntx)[sl]
                out["qc"][bi, :, d, :nt] = o["qcoeffs"].cpu().numpy().reshape(self.n, nt, -1)[sl]
                out["dist"][bi, :, d, :nt] = o["dist"].cpu().numpy().view(np.uint64).reshape(-1, nt)[sl]
                out["rate"][bi, :, d, :nt] = t["rates"][d]["rate"].cpu().numpy().view(np.uint32).reshape(-1, nt)[sl]
            st = t["st"].cpu().numpy().view(RD_PICK).ravel()[s * K:(s + 1) * K]
            out["mode_pick"][bi] = np.stack([st["best_call"], st["best_slot"]], 1)
            out["state_rd"][bi] = st["best_rd"]
            blk = t["blk"].cpu().numpy().view(RD_PICK).ravel()[s]
            win = t["win"].cpu().numpy().view(RD_PICK).ravel()[s]
            d = int(win["best_call"])
            assert int(blk["best_call"]) == CALL_MODE and int(win["best_row"]) == int(blk["best_row"]) and d in (0, 1)
            wt = t["win_trials"][d].cpu().numpy().reshape(-1).view(BLOCK_RATE_TRIAL)[s]
            other = t["win_trials"][1 - d].cpu().numpy().reshape(-1).view(BLOCK_RATE_TRIAL)[s]
            assert int(other["tx_type"]) == 15                                  # the depth that lost wrote nothing
            out["win"][bi] = (int(blk["best_row"]), d, int(win["best_slot"]), int(wt["tx_type"]))
            out["best_rd"][bi] = np.array(blk["best_rd"], np.float64).view(np.uint64)
            out["ctx_in"][bi] = t["blocks"].cpu().numpy().reshape(self.S, K, -1)[s, 0].view(BLOCK_CHAIN_CTX)["ctx"].reshape(96)
            out["ctx_out"][bi] = t["wins"][d]["side_win"].cpu().numpy()[s]
            assert (t["wins"][1 - d]["side_win"].cpu().numpy()[s] == 0x5A).all()
            out["adapt_rate"][bi] = t["adapts"][d]["rate"].cpu().numpy().view(np.uint32)[s]
            assert t["adapts"][d]["ctx"].cpu().numpy().reshape(self.S, 96)[s].tolist() == out["ctx_out"][bi].tolist()
            out["cdf"][bi] = DM.packed_of(t["cdf"].cpu().numpy().reshape(-1).view(DM.COEFF_CDF_CONTEXT)[s])
            nbr = t["nbr"].cpu().numpy().reshape(-1).view(COEFF_NBR_CONTEXT)[s]
            out["above"][bi], out["left"][bi] = nbr["above"], nbr["left"]
            body = t["plane"].cpu().numpy()[p.off:p.off + p.nbytes]
            plane = (body if p.bpp == 1 else body.view(np.uint16)).reshape(p.alloc_height, p.stride)
            y0, x0 = p.yorigin + y, p.xorigin + s * c.w + x
            out["rec"][bi] = plane[y0:y0 + c.bs, x0:x0 + c.bs]
        return out

"""The carried intra decision loop of a tile with its head symbols on the device: the chain of
tests/tile_chain_util.DeviceChain on the smallest case of tests/golden/tile_chain_ref.npz, where the mode pick's
rate_add is no longer an input but what r1_intra_head_rate_batch wrote on the tile's device-resident head contexts
(each mode's transform size read from the depth picks the launches in front of it left), and
r1_intra_head_commit_batch replays every block's winner behind the block.  One stream, no host read until the case ends.

Compared, array for array, with the SAME loop on the host (tile_chain_util.host_chain) whose rate_add comes from
tests/head_model.py on host copies of the two head contexts: every trial and decision array of the chain, the rate_add of
every block and mode, and both head contexts behind every block.  No tolerance.

tile_chain_util is imported as it stands: the device loop is its DeviceChain behind a context proxy that answers the mode
pick's rate_add, the host loop its host_chain with `decide` told the model's rate_add first."""
import numpy as np
import pytest

import coeff_cdf_model as DM
import head_model as M
import layout_util as LU
import tile_chain_util as TC
from coeff_rate_gpu_util import _guards_intact
from test_gpu_coeff_cdf import _dev_contexts
from test_gpu_coeff_nbr import _dev_nbr, _shifted_intact, NBR_BYTES
from test_gpu_head import _dev_bytes
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import COEFF_NBR_CONTEXT, HEAD_BLOCK, HEAD_COMMIT, HEAD_NBR_CONTEXT, HEAD_TRIAL

pytestmark = pytest.mark.gpu

CHECKED = tuple(k for k in TC.ARRAYS if k not in ("rd", "mode_rd"))       # no launch writes a trial's rd out


def _head_trials(c):
    """one head per mode: the chroma mode is the luma mode (a directional one puts both angle deltas on one row)"""
    return [(int(m), int(m), 1 if 1 <= int(m) <= 8 else 0, -2 if 1 <= int(m) <= 8 else 0, 0, 0) for m in c.modes]


def _head_block(c, x, y):
    return (int(c.bsize), x >> 2, y >> 2, c.mi_w, c.mi_h, 1, 1)


class _HeadCtx:
    """the product's Context, with the mode pick's rate_add answered by r1_intra_head_rate_batch"""

    def __init__(self, ctx, chain):
        self._ctx, self._chain = ctx, chain

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def rd_pick_batch(self, rate, dist, state, group, nt, lam, rule=0, call_id=0, rate_add=None, **kw):
        ch = self._chain
        if call_id != TC.CALL_MODE:
            ch.depth_state = state                     # the (tile, mode) states the depth calls leave their picks in
            return self._ctx.rd_pick_batch(rate, dist, state, group, nt, lam, rule=rule, call_id=call_id, rate_add=rate_add, **kw)
        got = self._ctx.intra_head_rate_batch(ch.dhead_nbr, ch.dhead_cdf, ch.head_blocks, ch.head_trials,
                                              depth_state=ch.depth_state, tx_sizes=ch.tx_sizes)
        ch.head_rate_add.append(got["rate_add"])
        ch.mode_state = state
        return self._ctx.rd_pick_batch(rate, dist, state, group, nt, lam, rule=rule, call_id=call_id, rate_add=got["rate_add"], **kw)


class HeadChain(TC.DeviceChain):
    def __init__(self, ctx, cases, dorg, drec, dcdf, dnbr, dhead_nbr, dhead_cdf):
        super().__init__(ctx, cases, dorg, drec, dcdf, dnbr)
        self.ctx = _HeadCtx(ctx, self)
        self.dhead_nbr, self.dhead_cdf = dhead_nbr, dhead_cdf
        c = self.c
        self.tx_sizes = (c.ts0, c.ts1, c.ts1)
        self.head_rate_add, self.head_states = [], []

    def step(self, bi):
        c, S, K = self.c, self.S, self.c.k
        x, y, reset = (int(v) for v in c.blocks[bi])
        if reset:
            self.ctx.head_nbr_reset_left_batch(self.dhead_nbr, list(range(S)))
        blk = _head_block(c, x, y)
        self.head_blocks = np.array([(s, s) + blk[1:5] + (blk[0], blk[5], blk[6], 0) for s in range(S)], HEAD_BLOCK)
        self.head_trials = np.array([(s,) + h + (0, (0, 0, 0)) for s in range(S) for h in _head_trials(c)], HEAD_TRIAL)
        super().step(bi)
        # the winner's head: state s of the mode pick names the mode as its row; the block is its own partition node
        node = (int(c.bsize), x >> 2, y >> 2)
        commits = np.array([(s, node[1], node[2], node[0], 0, node[0], 0, (0, 0, 0, 0)) for s in range(S)], HEAD_COMMIT)
        self.ctx.intra_head_commit_batch(self.dhead_nbr, self.dhead_cdf, self.head_blocks, self.head_trials, commits, self.mode_state,
                                         TC.CALL_MODE, K, 1, depth_state=self.depth_state, tx_sizes=self.tx_sizes)
        self.head_states.append((self.dhead_nbr.clone(), self.dhead_cdf.clone()))


def host_head_chain(case, L, cdf0):
    """tile_chain_util.host_chain with the head on the host: `decide` first writes the model's rate_add of the block into
    the case, then decides as it always does, then the winner's head is committed to the host head contexts"""
    import copy
    c = copy.copy(case)
    c.rate_add = np.zeros_like(case.rate_add)
    cdf, rec = M.cdf_record(cdf0), np.zeros(1, HEAD_NBR_CONTEXT)[0]
    nbr = M.nbr_arrays(rec)
    states = []
    plain = TC.decide

    def decide(cc, bi, rates, dists):
        x, y, reset = (int(v) for v in cc.blocks[bi])
        if reset:
            RG.head_nbr_reset_left(nbr)
        blk = _head_block(cc, x, y)
        trs = []
        for mi, h in enumerate(_head_trials(cc)):
            per_r = [[int(v) for v in rates[mi][d][:cc.nt[d]]] for d in range(2)]
            per_d = [[int(v) for v in dists[mi][d][:cc.nt[d]]] for d in range(2)]
            depth, _slot, _rd = RG.tx_size_type_decision(per_r, per_d, cc.lam)
            trs.append(h + (cc.sizes[depth],))
            rate, _rng = M.head_rate(cdf, M.symbols(nbr, blk, trs[-1]))
            assert rate != M.INVALID
            cc.rate_add[bi, mi] = rate
        out = plain(cc, bi, rates, dists)
        win = trs[out[2][0]]
        M.partition_event(cdf, nbr, blk[0], blk[1], blk[2], blk[3], blk[4], 0)
        M.head_commit(cdf, M.symbols(nbr, blk, win, coded=True))
        RG.head_nbr_store(nbr, blk[0], blk[1], blk[2], blk[3], blk[4], win[0], win[6], 1, (blk[1], blk[2], blk[0], blk[0]))
        states.append((rec.copy(), cdf.copy()))
        return out

    TC.decide = decide
    try:
        out = TC.host_chain(c, L)
    finally:
        TC.decide = plain
    return out, c.rate_add, states


def test_the_chain_with_its_head_on_the_device(ctx, oracle):
    cases = TC.load()
    c = min(cases, key=lambda t: (t.nblocks * t.k * t.bs * t.bs, t.w * t.h))
    cdf0 = M.load_fixture()["seq_cdf0"][0]
    want, want_add, want_states = host_head_chain(c, oracle, cdf0)
    org, rec = c.planes()
    _, dorg = LU.relayout(org, LU.KINDS[0], 8, 8)
    _, drec = LU.relayout(rec, LU.KINDS[0], 8, 8)
    raw_c, dcdf, _ = _dev_contexts([DM.context_from_packed(c.cdf0)])
    raw_n, dnbr, _ = _dev_nbr(np.zeros(1, COEFF_NBR_CONTEXT))
    raw_hn, dhead_nbr = _dev_bytes(np.zeros(1, HEAD_NBR_CONTEXT))
    raw_hc, dhead_cdf = _dev_bytes(cdf0)
    chain = HeadChain(ctx, [c], dorg, drec, dcdf, dnbr, dhead_nbr, dhead_cdf).run()
    got = chain.results(0)
    moved = {k: [b for b in range(c.nblocks) if want[k][b].tobytes() != got[k][b].tobytes()] for k in CHECKED}
    assert not any(moved.values()), {k: v for k, v in moved.items() if v}
    for bi in range(c.nblocks):
        assert chain.head_rate_add[bi].cpu().numpy().view(np.uint32).tolist() == [int(v) for v in want_add[bi]], bi
        hn, hc = chain.head_states[bi]
        assert hn.cpu().numpy().tobytes() == want_states[bi][0].tobytes(), bi
        assert hc.cpu().numpy().tobytes() == want_states[bi][1].tobytes(), bi
    # the head's rate took part in the decision: it is not the fixture's seeded rate_add, and it moves with the state
    assert want_add.tolist() != c.rate_add.tolist() and len({tuple(r) for r in want_add.tolist()}) > 1
    assert _guards_intact(raw_c) and _shifted_intact(raw_n, (1, NBR_BYTES)) and _guards_intact(raw_hn) and _guards_intact(raw_hc)

"""r1_rd_pick_batch / r1_rd_commit_batch on the GPU: every case of tests/golden/rd_pick_ref.npz (the reference's
compute_rd_cost, rdo_tx_type_decision and rdo_tx_size_type executed) through the C ABI, bit for bit; random picks
against the exact-rational host statements of rdo_glue; the commit against a NumPy gather on plane layouts the ABI
admits; one closed chain of three depths, a pick over the modes and three commits with no host read in it."""
import os
import sys

import numpy as np
import pytest

from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import PICK_FIRST_MIN, PICK_TX_TYPE, RD_PICK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_MAX = sys.float_info.max
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "rd_pick_ref.npz"))


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed[a.dtype]) if a.dtype in signed else a).cuda()


def fresh(n, best_rd=None):
    st = np.zeros(n, RD_PICK)
    st["best_rd"], st["best_row"], st["best_slot"], st["best_call"] = F64_MAX, -1, -1, -1
    if best_rd is not None:
        st["best_rd"] = best_rd
    return st


def pick(ctx, rate, dist, st, group, nt, lam, rule, call_id, rate_add=None):
    """host arrays in -> (states, invalid) out"""
    import torch
    d_st = _t(st.view(np.uint8).reshape(len(st), 24))
    o = ctx.rd_pick_batch(_t(np.asarray(rate, np.uint32).ravel()), _t(np.asarray(dist, np.uint64).ravel()), d_st, group, nt, lam,
                          rule=rule, call_id=call_id, rate_add=None if rate_add is None else _t(np.asarray(rate_add, np.uint32).ravel()),
                          want_invalid=True)
    torch.cuda.synchronize()
    return d_st.cpu().numpy().view(RD_PICK).ravel(), o["invalid"].cpu().numpy()


def same_states(got, want, key=None):
    for f in RD_PICK.names:
        g, w = (got[f].view(np.uint64), want[f].view(np.uint64)) if f == "best_rd" else (got[f], want[f])
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (key, f, "first bad state", int(bad[0]), got[bad[0]], want[bad[0]])


def keep(st, i, rd, dist, rate, row, slot, call):
    st[i] = (rd, dist, rate, row, slot, call)


# ---------------------------------------------------------------- 1. the fixture
def tt_expect(ref, i, call_id):
    """the state behind case i of rdo_tx_type_decision: kept when the function's minimum is below what was carried"""
    st = fresh(1, ref["tt_cur"][i])
    s = int(ref["tt_slot"][i])
    if s >= 0 and ref["tt_rd"][i] < ref["tt_cur"][i]:
        keep(st, 0, ref["tt_rd"][i], ref["tt_dist"][i, s], ref["tt_rate"][i, s], 0, s, call_id)
    return st


def test_type_decision_cases_one_by_one(ctx, ref):
    kept = 0
    for i, name in enumerate(ref["tt_names"]):
        nt = int(ref["tt_nt"][i])
        got, inv = pick(ctx, ref["tt_rate"][i, :nt], ref["tt_dist"][i, :nt], fresh(1, ref["tt_cur"][i]), 1, nt,
                        float(ref["tt_lam"][i]), PICK_TX_TYPE, i % 128)
        same_states(got, tt_expect(ref, i, i % 128), str(name))
        assert inv.tolist() == [0], name
        kept += int(got["best_call"][0] >= 0)
    assert 0 < kept < len(ref["tt_names"])


@pytest.mark.parametrize("nt", [1, 2, 5, 7, 16])
def test_type_decision_cases_batched_257(ctx, ref, nt):
    """the cases of one nt, cyclically, as one call of 257 states: not a multiple of the wave or of the states a
    workgroup holds"""
    idx = [i for i in range(len(ref["tt_names"])) if ref["tt_nt"][i] == nt]
    n = 257
    rows = [idx[k % len(idx)] for k in range(n)]
    lams = sorted({float(ref["tt_lam"][i]) for i in idx})
    for lam in lams:                                   # lambda is an argument of the call
        sel = [i for i in rows if float(ref["tt_lam"][i]) == lam]
        sel = (sel * n)[:n]
        st = fresh(n, ref["tt_cur"][sel])
        got, inv = pick(ctx, ref["tt_rate"][sel, :nt], ref["tt_dist"][sel, :nt], st, 1, nt, lam, PICK_TX_TYPE, 5)
        want = np.concatenate([tt_expect(ref, i, 5) for i in sel])
        same_states(got, want, (nt, lam))
        assert not inv.any()


def test_depth_sequences_as_chained_calls(ctx, ref):
    import torch
    for i, name in enumerate(ref["sz_names"]):
        d_st = ctx.rd_pick_state(1)
        for d in range(int(ref["sz_ndepth"][i])):
            nt = int(ref["sz_nt"][i, d])
            ctx.rd_pick_batch(_t(ref["sz_rate"][i, d, :nt]), _t(ref["sz_dist"][i, d, :nt]), d_st, 1, nt, float(ref["sz_lam"][i]),
                              rule=PICK_TX_TYPE, call_id=d)
        torch.cuda.synchronize()
        got = d_st.cpu().numpy().view(RD_PICK).ravel()
        d, s = int(ref["sz_depth"][i]), int(ref["sz_slot"][i])
        want = fresh(1)
        keep(want, 0, ref["sz_rd"][i], ref["sz_dist"][i, d, s], ref["sz_rate"][i, d, s], 0, s, d)
        same_states(got, want, str(name))


def test_depth_sequences_batched_257(ctx, ref):
    """the same sequences, those of one lambda and one nt shape cyclically, as three chained calls of 257 states"""
    import torch
    n = 257
    shapes = sorted({(float(ref["sz_lam"][i]), int(ref["sz_ndepth"][i]), tuple(int(v) for v in ref["sz_nt"][i]))
                     for i in range(len(ref["sz_names"]))})
    seen = 0
    for lam, nd, nts in shapes:
        idx = [i for i in range(len(ref["sz_names"]))
               if (float(ref["sz_lam"][i]), int(ref["sz_ndepth"][i]), tuple(int(v) for v in ref["sz_nt"][i])) == (lam, nd, nts)]
        seen += len(idx)
        sel = [idx[k % len(idx)] for k in range(n)]
        d_st = ctx.rd_pick_state(n)
        for d in range(nd):
            ctx.rd_pick_batch(_t(ref["sz_rate"][sel, d, :nts[d]].ravel()), _t(ref["sz_dist"][sel, d, :nts[d]].ravel()), d_st, 1, nts[d],
                              lam, rule=PICK_TX_TYPE, call_id=d)
        torch.cuda.synchronize()
        want = fresh(n)
        for k, i in enumerate(sel):
            d, s = int(ref["sz_depth"][i]), int(ref["sz_slot"][i])
            keep(want, k, ref["sz_rd"][i], ref["sz_dist"][i, d, s], ref["sz_rate"][i, d, s], 0, s, d)
        same_states(d_st.cpu().numpy().view(RD_PICK).ravel(), want, (lam, nd, nts))
    assert seen == len(ref["sz_names"])


def test_cost_rows_bit_for_bit(ctx, ref):
    """every executed compute_rd_cost row -- the rate / distortion / lambda edge grid and the tuples where a multiply
    and an add round differently from the fused form -- as a state of one trial (group 1, nt 1, R1_PICK_FIRST_MIN from
    f64::MAX), one call per distinct lambda: best_rd is the reference's cost bit for bit, the rate and distortion are
    the inputs; a cost that is not below f64::MAX keeps nothing"""
    lams = ref["cost_lam"]
    seen = 0
    for lam in np.unique(lams):
        sel = np.nonzero(lams == lam)[0]
        seen += len(sel)
        got, inv = pick(ctx, ref["cost_rate"][sel], ref["cost_dist"][sel], fresh(len(sel)), 1, 1, float(lam), PICK_FIRST_MIN, 11)
        want = fresh(len(sel))
        for k, i in enumerate(sel):
            if ref["cost_rd"][i] < F64_MAX:
                keep(want, k, ref["cost_rd"][i], ref["cost_dist"][i], ref["cost_rate"][i], 0, 0, 11)
        same_states(got, want, float(lam))
        assert not inv.any()
    assert seen == len(lams) == 504 and int((ref["cost_kind"] == 1).sum()) >= 50


@pytest.mark.parametrize("group,nt", [(1, 16), (4, 4), (13, 2)])
def test_first_min_cases_batched_257(ctx, ref, group, nt):
    """the `rd < best` groups as one call of 257 states per lambda; a group's trials fill the first entries of the
    state's group x nt, the rest are invalid slots (+infinity: they never win and raise invalid_out)"""
    T = group * nt
    n = 257
    for lam in sorted({float(v) for v in ref["fm_lam"]}):
        idx = [i for i in range(len(ref["fm_names"])) if float(ref["fm_lam"][i]) == lam]
        sel = [idx[k % len(idx)] for k in range(n)]
        rate, add, dist = np.full((n, T), INVALID, np.uint32), np.zeros((n, T), np.uint32), np.zeros((n, T), np.uint64)
        want = fresh(n, ref["fm_best_in"][sel])
        for k, i in enumerate(sel):
            m = int(ref["fm_n"][i])
            rate[k, :m], add[k, :m], dist[k, :m] = ref["fm_rate"][i, :m], ref["fm_add"][i, :m], ref["fm_dist"][i, :m]
            j = int(ref["fm_idx"][i])
            if j >= 0:
                keep(want, k, ref["fm_rd"][i, j], dist[k, j], int(rate[k, j]) + int(add[k, j]), j // nt, j % nt, 9)
        got, inv = pick(ctx, rate, dist, fresh(n, ref["fm_best_in"][sel]), group, nt, lam, PICK_FIRST_MIN, 9, rate_add=add)
        same_states(got, want, (group, nt, lam))
        assert inv.tolist() == [int(ref["fm_n"][i] < T) for i in sel]


def test_invalid_rate_in_slot_0_and_in_a_middle_slot(ctx):
    rate = np.array([[INVALID, 0, 0, 0, 0], [8, 0, INVALID, 0, 0], [8, 9, 9, 9, 9], [8, 0, 0, 0, INVALID - 1]], np.uint32)
    add = np.array([[0] * 5, [0] * 5, [0] * 5, [0, 0, 0, 0, 1]], np.uint32)
    dist = np.array([[0, 1, 1, 1, 1], [100, 50, 0, 60, 60], [1] * 5, [1] * 5], np.uint64)
    # R1_PICK_TX_TYPE: an invalid first slot is above anything carried, f64::MAX included: nothing is kept
    got, inv = pick(ctx, rate, dist, fresh(4), 1, 5, 8.0, PICK_TX_TYPE, 2, rate_add=add)
    want = fresh(4)
    keep(want, 1, 50.0, 50, 0, 0, 1, 2)
    keep(want, 2, 9.0, 1, 8, 0, 0, 2)
    keep(want, 3, 1.0, 1, 0, 0, 1, 2)
    same_states(got, want, "tx_type")
    assert inv.tolist() == [1, 1, 0, 1]
    # R1_PICK_FIRST_MIN: the invalid slot is skipped, the rest compete
    got, inv = pick(ctx, rate, dist, fresh(4), 1, 5, 8.0, PICK_FIRST_MIN, 3, rate_add=add)
    keep(want, 0, 1.0, 1, 0, 0, 1, 3)
    want["best_call"][1:] = 3
    same_states(got, want, "first_min")
    assert inv.tolist() == [1, 1, 0, 1]
    # without invalid_out the call is the same
    import torch
    d_st = _t(fresh(4).view(np.uint8).reshape(4, 24))
    o = ctx.rd_pick_batch(_t(rate.ravel()), _t(dist.ravel()), d_st, 1, 5, 8.0, rule=PICK_FIRST_MIN, call_id=3, rate_add=_t(add.ravel()))
    torch.cuda.synchronize()
    assert "invalid" not in o
    same_states(d_st.cpu().numpy().view(RD_PICK).ravel(), want, "no invalid_out")


# ---------------------------------------------------------------- 2. random picks against the exact-rational statements
def model_pick(rate, add, dist, st, group, nt, lam, rule, call_id):
    want = st.copy()
    T = group * nt
    for s in range(len(st)):
        r = [int(a) + int(b) for a, b in zip(rate[s], add[s])]
        carried = float(st["best_rd"][s])
        if rule == PICK_TX_TYPE:
            assert max(r) < INVALID
            slot, rd = RG.pick_tx_type(r, [RG.dist_as_f64(d) for d in dist[s]], lam, carried)
            if slot is not None and rd < carried:
                keep(want, s, rd, dist[s][slot], r[slot], 0, slot, call_id)
        else:
            idx, rd, rt, ds = RG.pick_first_min(rate[s], dist[s], lam, best=(None, carried, 0, 0), rate_adds=add[s])
            if idx is not None:
                keep(want, s, rd, ds, rt, idx // nt, idx % nt, call_id)
    assert T == len(rate[0])
    return want


@pytest.mark.parametrize("n,group,nt,rule", [(1, 256, 16, 0), (1, 1, 1, 1), (63, 1, 7, 1), (63, 64, 2, 0), (65, 13, 5, 0),
                                             (65, 1, 16, 1), (1000, 1, 7, 1), (1000, 4, 1, 0), (2, 4096, 1, 0), (3, 100, 3, 0)])
def test_random_picks_equal_the_host_statements(ctx, n, group, nt, rule):
    """two chained calls per shape: small integers with lambda = 8 (ties everywhere, within a call and with what the
    first call kept), then wide values with an inexact lambda; invalid rates among the FIRST_MIN trials"""
    rng = np.random.default_rng(n * 10007 + group * 17 + nt)
    T = group * nt
    for lam, hi_r, hi_d in ((8.0, 6, 6), (0.1 * float(rng.integers(1, 5000)), 1 << 20, 1 << 40)):
        st = fresh(n)
        for call_id in (0, 1):
            rate = rng.integers(0, hi_r, (n, T)).astype(np.uint32)
            add = rng.integers(0, 3, (n, T)).astype(np.uint32)
            dist = rng.integers(0, hi_d, (n, T)).astype(np.uint64)
            if rule == PICK_FIRST_MIN:
                rate[rng.random((n, T)) < 0.05] = INVALID
            want = model_pick(rate, add, dist, st, group, nt, lam, rule, call_id)
            got, inv = pick(ctx, rate, dist, st, group, nt, lam, rule, call_id, rate_add=add)
            same_states(got, want, (n, group, nt, rule, lam, call_id))
            assert inv.tolist() == (rate == INVALID).any(axis=1).astype(int).tolist()
            st = got
        assert (st["best_call"] >= 0).all()


# ---------------------------------------------------------------- 3. the commit against a NumPy gather
COMMIT_CASES = [
    # bw, bh, bit depth, layout, ntx, order, coeff bytes, side bytes, group, shift (the grid starts at x = -2), max rectangle
    (4, 4, 8, "odd", 1, 0, 2, 1, 3, 0, 0),
    (4, 4, 10, "tight", 4, 1, 4, 32, 1, 1, 0),
    (16, 16, 8, "tight", 4, 0, 2, 96, 2, 1, 0),
    (16, 16, 10, "odd", 16, 1, 4, 1, 1, 0, 0),
    (64, 16, 8, "odd", 16, 0, 4, 32, 3, 1, 1),
    (64, 16, 10, "tight", 1, 0, 2, 32, 2, 0, 0),
    (64, 64, 8, "tight", 4, 1, 2, 96, 1, 0, 1),
    (64, 64, 10, "odd", 16, 0, 4, 32, 2, 1, 0),
]


@pytest.mark.parametrize("bw,bh,bd,kind,ntx,order,cb,side_bytes,group,shift,maxrect", COMMIT_CASES)
def test_commit_equals_a_numpy_gather(ctx, bw, bh, bd, kind, ntx, order, cb, side_bytes, group, shift, maxrect):
    import torch
    import layout_util as LU
    import oracle_lib as O
    rng = np.random.default_rng(bw * 1000 + bh * 10 + bd + ntx)
    nt, call_id, area = 3, 4, 16 if ntx == 16 else 64
    # a 4 x 3 grid of blocks: the last column is cut to 2 pixels and the last row to 6 (2 for the 4-pixel block)
    W = 3 * bw + (0 if shift else 2)
    H = 2 * bh + (6 if bh > 6 else 2)
    xs = [c * bw - (2 if shift else 0) for c in range(4)]
    ys = [r * bh for r in range(3)]
    pos = np.array([(x, y) for y in ys for x in xs], np.int16)
    n = len(pos)
    hp, dp = LU.relayout(O.HostPlane(W, H, bd, xpad=8, ypad=8, rng=rng), kind, 8, 8)
    store_w, store_h = (hp.stride - hp.xorigin, hp.alloc_height - hp.yorigin) if maxrect else (W, H)
    # states: won by this call, by another call, by none, interleaved; one with a row and one with a slot out of range
    st = fresh(n)
    who = np.array([call_id, call_id + 1, -1] * n)[:n]
    st["best_call"] = who
    st["best_row"], st["best_slot"] = rng.integers(0, group, n), rng.integers(0, nt, n)
    st["best_row"][who == -1] = -1
    st["best_slot"][who == -1] = -1
    st["best_row"][3], st["best_slot"][6] = group, nt            # 3 and 6 are states of this call: nothing written for them
    assert who[3] == call_id and who[6] == call_id
    trials = n * group * nt
    cdt = np.int16 if cb == 2 else np.int32
    eobs = rng.integers(0, area + 1, trials * ntx).astype(np.uint16)
    qc = rng.integers(-30000, 30000, (trials * ntx, area)).astype(cdt)
    side = rng.integers(0, 256, (trials, side_bytes)).astype(np.uint8)
    pdt = np.uint8 if bd == 8 else np.uint16
    recs = rng.integers(0, 1 << bd, (trials, bh, bw)).astype(pdt)
    # gap entries behind each state's row; 5 of them leave the rows without 16-byte alignment (the kernel's
    # element-wide copy), 24 keep it (the 16-byte copy)
    win_stride = ntx * area + (5 if ntx == 4 else 24)
    eob_win = np.full((n, 16), 0x5A5A, np.uint16)
    q_win = np.full((n, win_stride), 0x5A5A5A5A if cb == 4 else 0x5A5A, cdt)
    s_win = np.full((n, side_bytes), 0x5A, np.uint8)
    want_plane = hp.data.copy()
    want_e, want_q, want_s = eob_win.copy(), q_win.copy(), s_win.copy()
    written = 0
    for s in range(n):
        row, slot = int(st["best_row"][s]), int(st["best_slot"][s])
        if who[s] != call_id or not (0 <= row < group and 0 <= slot < nt):
            continue
        t = (s * group + row) * nt + slot
        for k in range(ntx):
            b = t * ntx + k if order == 0 else (s * ntx + k) * nt + slot
            want_e[s, k] = eobs[b]
            want_q[s, k * area:(k + 1) * area] = qc[b]
        want_s[s] = side[t]
        for y in range(bh):
            for x in range(bw):
                px, py = int(pos[s, 0]) + x, int(pos[s, 1]) + y
                if 0 <= px < store_w and 0 <= py < store_h:
                    want_plane[hp.yorigin + py, hp.xorigin + px] = recs[t, y, x]
                    written += 1
    assert written > 0
    d_st = _t(st.view(np.uint8).reshape(n, 24))
    outs = {"eob_win": _t(eob_win), "qcoeffs_win": _t(q_win)[:, :], "side_win": _t(s_win)}
    o = ctx.rd_commit_batch(d_st, call_id, group, nt, coeffs=(_t(eobs), _t(qc)), ntx=ntx, order=order, side=_t(side),
                            rec_trials=_t(recs), rec=dp, pos_xy=_t(pos), store_w=store_w, store_h=store_h, outs=outs)
    torch.cuda.synchronize()
    assert np.array_equal(dp.host(), want_plane) and dp.guards_intact()
    assert np.array_equal(o["eob_win"].cpu().numpy().view(np.uint16), want_e)
    assert np.array_equal(o["qcoeffs_win"].cpu().numpy(), want_q)
    assert np.array_equal(o["side_win"].cpu().numpy(), want_s)
    assert d_st.cpu().numpy().tobytes() == st.tobytes()             # the states are read, never written
    # a part that is absent: the others alone give the same, and nothing of the absent part is touched
    dp.upload(hp)
    o2 = ctx.rd_commit_batch(d_st, call_id, group, nt, side=_t(side), outs={"side_win": _t(s_win)})
    torch.cuda.synchronize()
    assert np.array_equal(o2["side_win"].cpu().numpy(), want_s) and np.array_equal(dp.host(), hp.data)


# ---------------------------------------------------------------- 4. one closed chain
def test_closed_chain_three_depths_modes_and_commits(ctx):
    """24 intra blocks of 16x16 on a 96x64 10-bit plane, 4 modes: intra candidates (7 types) -> chain rate -> pick 0;
    the 8x8 split -> rate -> pick 1; the 4x4 split -> rate -> pick 2; the pick over the modes with a rate_add; three
    commits -- enqueued with no host read (tests/rd_chain_util.py: the chain tools/bench_rd_pick.py times).  Then
    the same arrays are downloaded and decided by tx_size_type_decision / pick_first_min, and gathered with NumPy.
    (Depth 0 asks the rate call for the 16x16 INTER set: that one holds the 7 types the candidate call ran.)"""
    import torch
    import layout_util as LU
    import oracle_lib as O
    import rd_chain_util as B
    from rav1e_amd.api import Plane
    W, H, bd, K, nt = 96, 64, 10, 4, 7
    rng = np.random.default_rng(424)
    # the source: noise on the left (the largest transform wins there), an 8x8 and a 4x4 checkerboard to the right of it
    # (flat transform blocks one and two depths down); the reconstruction around the blocks: the source, slightly off
    horg = O.HostPlane(W, H, bd, rng=rng)
    yy, xx = np.mgrid[0:H, 0:W]
    vis = horg.data[horg.yorigin:horg.yorigin + H, horg.xorigin:horg.xorigin + W]
    for x0, cell in ((32, 8), (64, 4)):
        vis[:, x0:x0 + 32] = (200 + 500 * ((xx // cell + yy // cell) % 2))[:, x0:x0 + 32]
    hrec = O.HostPlane(W, H, bd, rng=rng)
    hrec.data[...] = np.clip(horg.data.astype(np.int64) + rng.integers(-2, 3, horg.data.shape), 0, 1023)
    org, rec = (Plane.from_numpy(h.data, W, H, bd, 88, 88) for h in (horg, hrec))
    hdst, dst = LU.relayout(O.HostPlane(W, H, bd, xpad=8, ypad=8, rng=rng), "odd", 8, 8)
    bx, by = np.meshgrid(np.arange(W // 16) * 16, np.arange(H // 16) * 16)
    bx, by = bx.ravel(), by.ravel()
    ch = B.Chain(ctx, org, rec, dst, bx, by, qindex=90, lam=37.3, seed=7)
    assert ch.nb == 24 and ch.n == 96
    st, blk, win, o = ch.device_route(search=True, wins=None)
    wins = {k: o[k] for k in ("eob_win", "qcoeffs_win", "side_win")}
    torch.cuda.synchronize()                                       # the first host read
    st, blk, win = (t.cpu().numpy().view(RD_PICK).ravel() for t in (st, blk, win))
    rate = [ch.rate[d]["rate"].cpu().numpy().view(np.uint32).reshape(96, nt) for d in range(3)]
    dist = [ch.search[d]["dist"].cpu().numpy().view(np.uint64).reshape(96, nt) for d in range(3)]
    assert all((r != INVALID).all() for r in rate)
    adds = ch.rate_add.cpu().numpy().view(np.uint32)
    # ---- the decisions by the host statements
    want_st = fresh(96)
    for c in range(96):
        depth, slot, rd = RG.tx_size_type_decision([r[c] for r in rate], [d[c] for d in dist], ch.lam)
        keep(want_st, c, rd, dist[depth][c, slot], rate[depth][c, slot], 0, slot, depth)
    same_states(st, want_st, "mode states")
    want_blk, want_win = fresh(24), fresh(24)
    for b in range(24):
        sl = slice(b * K, (b + 1) * K)
        idx, rd, rt, ds = RG.pick_first_min(want_st["best_rate"][sl], want_st["best_dist"][sl], ch.lam, rate_adds=adds[sl])
        keep(want_blk, b, rd, ds, rt, idx, 0, B.CALL_MODE)
        want_win[b] = want_st[b * K + idx]
        want_win["best_row"][b] = idx
    same_states(blk, want_blk, "block states")
    same_states(win, want_win, "winners")
    print("depths of the mode states:", np.bincount(want_st["best_call"], minlength=3).tolist(), "of the winners:",
          np.bincount(want_win["best_call"], minlength=3).tolist(), "modes:", np.bincount(want_blk["best_row"], minlength=4).tolist())
    assert len(set(want_win["best_call"].tolist())) >= 2 and len(set(want_blk["best_row"].tolist())) >= 2
    # ---- the gather
    want_plane = hdst.data.copy()
    want_e, want_q, want_s = np.zeros((24, 16), np.int16), np.zeros((24, 256), np.int32), np.zeros((24, 32), np.uint8)
    for b in range(24):
        d, t = int(want_win["best_call"][b]), (b * K + int(want_win["best_row"][b])) * nt + int(want_win["best_slot"][b])
        ntx = B.DEPTH_NTX[d]
        want_e[b, :ntx] = ch.search[d]["eob"].cpu().numpy().reshape(-1, ntx)[t]
        want_q[b] = ch.search[d]["qcoeffs"].cpu().numpy().reshape(-1, 256)[t]
        want_s[b] = ch.rate[d]["ctx"].cpu().numpy().reshape(-1, 32)[t]
        blk_px = ch.search[d]["rec"].cpu().numpy().view(np.uint16).reshape(-1, 16, 16)[t]
        want_plane[hdst.yorigin + by[b]:hdst.yorigin + by[b] + 16, hdst.xorigin + bx[b]:hdst.xorigin + bx[b] + 16] = blk_px
    assert np.array_equal(dst.host(), want_plane) and dst.guards_intact()
    assert np.array_equal(wins["eob_win"].cpu().numpy(), want_e)
    assert np.array_equal(wins["qcoeffs_win"].cpu().numpy(), want_q)
    assert np.array_equal(wins["side_win"].cpu().numpy(), want_s)

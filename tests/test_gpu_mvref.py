"""r1_tile_blocks_reset_batch, r1_tile_blocks_store_batch, r1_mvref_stack_batch and r1_mvref_pmv_batch on the GPU, bit-exact
and through the C ABI, with guard bytes around every blocks array and every output: every single query of
tests/golden/mvref_ref.npz (the reference's find_mvrefs executed on real blocks arrays) as whole R1MvStack structs, one
launch per snapshot; every sequence enqueued whole on one stream (stack -> store per block, nothing read until the end);
the store's gate, clipping and intra arm; the reset; batches of 1 .. 257 blocks with 1 .. 8 queries each against the
statements; the pmv hand-over into r1_estimate_motion_batch; every device refusal; and one closed loop
(reset, then stack -> pmv -> store per block) against the same loop on the host statements.  No tolerance."""
import numpy as np
import pytest

import mvref_model as M
from coeff_rate_gpu_util import GUARD, _guarded, _guards_intact, _t
from rav1e_amd import rdo_glue as G
from rav1e_amd.types import MV_BLOCK, MV_QUERY, MV_STACK, MV_TRIAL, MVREF_REFUSED, RD_PICK, TILE_BLOCK

pytestmark = pytest.mark.gpu

FX, QS, EVS, SEQS = M.FX, M.QS, M.EVS, M.SEQS
SEQ_IDS = [str(n).replace(" ", "_") for n in FX["seq_names"]]


def dev_tile(ctx, si, cells=None, stride=None):
    """a sequence's tile on the device between guard bytes, holding `cells` (or guard bytes) -> (raw, tile dict)"""
    import torch
    s = SEQS(si)
    stride = s["cols"] if stride is None else stride
    raw, view = _guarded((s["rows"] * stride * TILE_BLOCK.itemsize,), torch.uint8)
    if cells is not None:
        full = np.full((s["rows"], stride), 0, TILE_BLOCK)
        full.view(np.uint8)[:] = GUARD
        full[:, :s["cols"]] = cells
        view.copy_(_t(full.view(np.uint8).reshape(-1)))
    return raw, ctx.tile_blocks(s["cols"], s["rows"], s["tile_x"], s["tile_y"], s["frame_cols"], s["frame_rows"], stride=stride, cells=view)


def host_cells(tile, stride=None):
    stride = tile["stride"] if stride is None else stride
    return tile["cells"].cpu().numpy().view(TILE_BLOCK).reshape(tile["rows"], stride)


def out_stacks(n):
    import torch
    return _guarded((n * MV_STACK.itemsize,), torch.uint8)


def expect(results):
    """statements' answers as MV_STACK records on an output that held guard bytes: a refusal writes its count alone"""
    out = np.zeros(len(results), MV_STACK)
    for k, r in enumerate(results):
        if r == G.MV_REFUSED:
            out[k:k + 1].view(np.uint8)[:] = GUARD
            out[k]["count"] = MVREF_REFUSED
        else:
            out[k] = M.stack_record(r)
    return out


def read(view):
    return view.cpu().numpy().view(MV_STACK)


def test_stacks_of_every_snapshot(ctx):
    by_snap = {}
    for i in range(len(QS)):
        by_snap.setdefault(QS(i)["snap"], []).append(i)
    for snap, idx in sorted(by_snap.items()):
        si = QS(idx[0])["seq"]
        raw, tile = dev_tile(ctx, si, M.cells_of(snap))
        items, order = {}, []
        for i in idx:
            r = QS(i)
            items.setdefault((0, r["bo_x"], r["bo_y"], r["bsize"]), []).append((i, (r["ref0"], r["ref1"], r["is_compound"])))
        blocks, queries = M.blocks_and_queries([k + ([q for _, q in v],) for k, v in items.items()])
        order = [i for v in items.values() for i, _ in v]
        oraw, out = out_stacks(len(queries))
        ctx.mvref_stack_batch([tile], blocks, queries, M.SIGN_BIAS, out=out)
        got = read(out)
        want = expect([M.want_q(i) for i in order])
        bad = [str(FX["q_names"][order[k]]) for k in range(len(order)) if got[k].tobytes() != want[k].tobytes()]
        assert not bad, (snap, len(bad), bad[:5])
        assert _guards_intact(oraw) and _guards_intact(raw)
        assert np.array_equal(host_cells(tile), M.cells_of(snap))              # the array is only read


@pytest.mark.parametrize("si", range(len(SEQS)), ids=SEQ_IDS)
def test_sequence_enqueued_whole(ctx, si):
    evs = [EVS(k) for k in range(len(EVS)) if EVS(k)["seq"] == si]
    raw, tile = dev_tile(ctx, si)
    blocks, queries, trials = np.zeros(len(evs), MV_BLOCK), np.zeros(4 * len(evs), MV_QUERY), np.zeros(len(evs), MV_TRIAL)
    for e, ev in enumerate(evs):
        assert ev["n_q"] == 4
        blocks[e] = (0, ev["bo_x"], ev["bo_y"], ev["bsize"], 4, 0, 4 * e)
        for q in range(4):
            r0, r1, comp = (int(v) for v in FX["sq_rows"][ev["q_off"] + q][:3])
            queries[4 * e + q] = (0, (r0, r1), comp, 0)              # every launch holds one block: index 0
        mode, refs, mvs, skip = M.event_winner(ev)
        trials[e] = M.trial_record(e, mode, refs, mvs, skip)
    db, dq, dt = (_t(a.view(np.uint8).reshape(-1)) for a in (blocks, queries, trials))
    oraw, out = out_stacks(len(queries))
    ctx.tile_blocks_reset_batch([tile])
    for e in range(len(evs)):
        ctx.mvref_stack_batch([tile], db[16 * e:16 * (e + 1)], dq, M.SIGN_BIAS, out=out, max_queries=4)
        ctx.tile_blocks_store_batch([tile], db, dt[16 * e:16 * (e + 1)])
    got = read(out)                                                    # the first read
    want = expect([M.want_sq(ev["q_off"] + q) for ev in evs for q in range(4)])
    bad = [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])
    assert np.array_equal(host_cells(tile), M.cells_of(SEQS(si)["final_snap"]))
    assert _guards_intact(raw) and _guards_intact(oraw)


def test_reset(ctx):
    """Block::default() over whole arrays, row padding included; an array that is not selected stays"""
    s = SEQS(0)
    raw0, t0 = dev_tile(ctx, 0, stride=s["cols"] + 5)
    raw1, t1 = dev_tile(ctx, 1)
    raw2, t2 = dev_tile(ctx, 2)
    ctx.tile_blocks_reset_batch([t0, t1, t2], sel=[2, 0])
    assert np.array_equal(host_cells(t0), G.tile_blocks_default(s["rows"], s["cols"] + 5))
    assert np.array_equal(host_cells(t2), G.tile_blocks_default(SEQS(2)["rows"], SEQS(2)["cols"]))
    assert (t1["cells"].cpu().numpy() == GUARD).all()
    ctx.tile_blocks_reset_batch([t0, t1, t2])
    assert np.array_equal(host_cells(t1), G.tile_blocks_default(SEQS(1)["rows"], SEQS(1)["cols"]))
    assert all(_guards_intact(r) for r in (raw0, raw1, raw2))


def test_store_gate_clipping_and_intra(ctx):
    si = 0                                                                # 22 x 10: both edges cut a superblock
    s = SEQS(si)
    stride = s["cols"] + 3
    start = M.cells_of(s["final_snap"])
    raw, tile = dev_tile(ctx, si, start, stride=stride)
    # (bo_x, bo_y, bsize): inside; cut at the right; cut at the bottom; cut at both; width exactly to the edge; 4x4
    places = [(0, 0, 9), (20, 0, 6), (8, 8, 9), (16, 8, 12), (18, 4, 6), (21, 9, 0), (4, 4, 17), (12, 0, 16)]
    blocks = np.zeros(len(places), MV_BLOCK)
    for b, (x, y, bs) in enumerate(places):
        blocks[b] = (0, x, y, bs, 0, 0, 0)
    # two trials per block (group 1, nt 2); an inter winner, an intra one, a compound one
    winners = [(19, (1, 8), ((5, -7), (0, 0)), 1), (3, (4, 7), ((9, 9), (8, 8)), 0), (33, (1, 7), ((-300, 20), (7, -1)), 0)]
    trials = np.zeros(2 * len(places), MV_TRIAL)
    for b in range(len(places)):
        trials[2 * b] = M.trial_record(b, *winners[(b + 1) % 3])
        trials[2 * b + 1] = M.trial_record(b, *winners[b % 3])
    st = np.zeros(len(places), RD_PICK)
    st["best_rd"], st["best_row"], st["best_slot"], st["best_call"] = 1.0, 0, 1, 2
    # the gate: blocks 3 and 5 were won by another call; block 6 names a slot outside nt
    st["best_call"][3], st["best_call"][5], st["best_slot"][6] = 1, -1, 2
    # overlapping extents are the caller's to avoid: run the disjoint ones together
    acting = [0, 1, 2, 4, 7]
    want = {"cells": start.copy(), "tile_x": 0, "tile_y": 0, "frame_cols": s["frame_cols"], "frame_rows": s["frame_rows"]}
    keep = st.copy()
    keep["best_call"][[b for b in range(len(places)) if b not in acting]] = -1
    ctx.tile_blocks_store_batch([tile], blocks, trials, state=_t(keep.view(np.uint8).reshape(-1)), call_id=2, group=1, nt=2)
    for b in acting:
        G.tile_blocks_store(want, *places[b], *winners[b % 3])
    got = host_cells(tile, stride)
    assert np.array_equal(got[:, :s["cols"]], want["cells"])
    assert (got[:, s["cols"]:].view(np.uint8) == GUARD).all() and _guards_intact(raw)      # nothing past the tile's columns
    # the gate alone: nothing acts
    ctx.tile_blocks_store_batch([tile], blocks, trials, state=_t(st.view(np.uint8).reshape(-1)), call_id=5, group=1, nt=2)
    only = st.copy()
    only["best_call"][:] = -1
    only["best_call"][6], only["best_call"][3] = 2, 1                      # a slot outside nt; another call's winner
    ctx.tile_blocks_store_batch([tile], blocks, trials, state=_t(only.view(np.uint8).reshape(-1)), call_id=2, group=1, nt=2)
    assert np.array_equal(host_cells(tile, stride)[:, :s["cols"]], want["cells"])
    # state == NULL: desc s acts on trial s
    ctx.tile_blocks_store_batch([tile], blocks, trials[6:7])               # trial 6: block 3, cut at both edges
    G.tile_blocks_store(want, *places[3], *winners[(3 + 1) % 3])
    got = host_cells(tile, stride)
    assert np.array_equal(got[:, :s["cols"]], want["cells"]) and (got[:, s["cols"]:].view(np.uint8) == GUARD).all()
    # nothing is written for a trial or block that is out of range, a bad size, a place outside the tile, a bad mode
    bad_blocks = blocks.copy()
    bad_blocks[0]["bsize"], bad_blocks[1]["bsize"], bad_blocks[2]["bo_x"], bad_blocks[4]["tile"] = 22, 15, 22, 1
    bad_trials = trials.copy()
    bad_trials[14]["block"], bad_trials[10]["mode"] = 99, 34
    ctx.tile_blocks_store_batch([tile], bad_blocks, bad_trials[[0, 2, 4, 8, 10, 14]])
    assert np.array_equal(host_cells(tile, stride)[:, :s["cols"]], want["cells"]) and _guards_intact(raw)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batches(ctx, n):
    """n blocks over three tiles with 1 .. 8 queries each, against the statements (refusals included)"""
    rng = np.random.default_rng(n)
    seqs = [6, 1, 0]
    tiles, host = [], []
    for si in seqs:
        cells = M.cells_of(SEQS(si)["final_snap"])
        tiles.append(dev_tile(ctx, si, cells))
        host.append(M.tile_of(si, cells))
    evs = {si: [EVS(k) for k in range(len(EVS)) if EVS(k)["seq"] == si] for si in seqs}
    items = []
    for b in range(n):
        t = int(rng.integers(0, 3))
        ev = evs[seqs[t]][int(rng.integers(0, len(evs[seqs[t]])))]
        qs = []
        for _ in range(1 + b % 8):
            if rng.integers(0, 3) == 0:
                qs.append((int(rng.integers(1, 8)), int(rng.integers(1, 8)), 1))
            else:
                qs.append((int(rng.integers(0, 8)), 8, 0))
        items.append((t, ev["bo_x"], ev["bo_y"], ev["bsize"], qs))
    blocks, queries = M.blocks_and_queries(items)
    oraw, out = out_stacks(len(queries))
    ctx.mvref_stack_batch([t for _, t in tiles], blocks, queries, M.SIGN_BIAS, out=out)
    want = expect([G.find_mvrefs(host[t], x, y, bs, (r0, r1), comp, M.SIGN_BIAS) for (t, x, y, bs, qs) in items for (r0, r1, comp) in qs])
    got = read(out)
    bad = [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])
    assert sum(1 for w in want if w["count"] not in (0, MVREF_REFUSED)) >= len(want) // 4
    assert _guards_intact(oraw) and all(_guards_intact(r) for r, _ in tiles)


def test_device_refusals(ctx):
    """every refusal of the header: count 0xFF and nothing else of the struct written; its neighbours are answered"""
    si = 0
    s = SEQS(si)
    cells = M.cells_of(s["final_snap"])
    raw, tile = dev_tile(ctx, si, cells)
    host = M.tile_of(si, cells)
    ok_q = (1, 8, 0)
    items = [(0, 4, 4, 6, [ok_q]),                 # 0: answered
             (1, 4, 4, 6, [ok_q]),                 # 1: names no descriptor
             (0, 4, 4, 22, [ok_q]),                # 2: bsize past the enum
             (0, 0, 0, 13, [ok_q]), (0, 0, 0, 14, [ok_q]), (0, 0, 0, 15, [ok_q]),      # 3-5: a 128-point side
             (0, 22, 4, 6, [ok_q]), (0, 4, 10, 6, [ok_q]),                              # 6-7: outside the tile
             (0, 4, 4, 6, [(8, 8, 0), (9, 8, 0), (1, 9, 0), (1, 8, 1), (1, 0, 1), (0, 8, 0), ok_q]),   # 8: the references
             (0, 8, 4, 6, [ok_q] * 8)]     # 9: more queries than max_queries allows (below)
    blocks, queries = M.blocks_and_queries(items)
    queries[len(queries) - 9]["block"] = 3         # the last query of item 8 names another block
    oraw, out = out_stacks(len(queries))
    ctx.mvref_stack_batch([tile], blocks, queries, M.SIGN_BIAS, out=out, max_queries=7)
    got = read(out)
    res = []
    for (t, x, y, bs, qs) in items:
        for (r0, r1, comp) in qs:
            res.append(G.MV_REFUSED if t == 1 else G.find_mvrefs(host, x, y, bs, (r0, r1), comp, M.SIGN_BIAS))
    res[len(res) - 9] = G.MV_REFUSED
    res[-8:] = [G.MV_REFUSED] * 8
    want = expect(res)
    assert [int(w["count"] == MVREF_REFUSED) for w in want] == [0] + [1] * 7 + [1, 1, 1, 1, 1, 0, 1] + [1] * 8
    assert want[0]["count"] > 0 and want[13].tobytes() == M.stack_record((0, [])).tobytes()
    assert got.tobytes() == want.tobytes(), [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]
    assert _guards_intact(oraw)
    # a cell the walk reads whose sides are no block's; a reference above NONE_FRAME where the extra search reads it
    x, y, bs = 4, 4, 6
    for field, v in (("n4_w", 0), ("n4_w", 3), ("n4_w", 32), ("n4_h", 0), ("n4_h", 6), ("n4_h", 17)):
        c2 = cells.copy()
        c2[y - 1, x][field] = v
        raw2, t2 = dev_tile(ctx, si, c2)
        blocks, queries = M.blocks_and_queries([(0, x, y, bs, [ok_q]), (0, 0, 0, 6, [ok_q])])
        oraw, out = out_stacks(2)
        ctx.mvref_stack_batch([t2], blocks, queries, M.SIGN_BIAS, out=out)
        want = expect([G.MV_REFUSED, G.find_mvrefs(M.tile_of(si, c2), 0, 0, 6, (1, 8), 0, M.SIGN_BIAS)])
        assert G.find_mvrefs(M.tile_of(si, c2), x, y, bs, (1, 8), 0, M.SIGN_BIAS) == G.MV_REFUSED
        assert read(out).tobytes() == want.tobytes(), (field, v)
    c2 = G.tile_blocks_default(s["rows"], s["cols"])
    t2h = M.tile_of(si, c2)
    G.tile_blocks_store(t2h, 0, 0, 6, 19, (9, 8), ((1, 1), (0, 0)), 0)
    raw2, t2 = dev_tile(ctx, si, c2)
    blocks, queries = M.blocks_and_queries([(0, 0, 4, 6, [ok_q])])
    oraw, out = out_stacks(1)
    ctx.mvref_stack_batch([t2], blocks, queries, M.SIGN_BIAS, out=out)
    assert G.find_mvrefs(t2h, 0, 4, 6, (1, 8), 0, M.SIGN_BIAS) == G.MV_REFUSED and read(out).tobytes() == expect([G.MV_REFUSED]).tobytes()
    # where the reference would index past the row: a far row that starts one column in, on an odd-width tile
    odd = ctx.tile_blocks(5, 8)
    ctx.tile_blocks_reset_batch([odd])
    oh = {"cells": G.tile_blocks_default(8, 5), "tile_x": 0, "tile_y": 0, "frame_cols": 5, "frame_rows": 8}
    blocks, queries = M.blocks_and_queries([(0, 4, 4, 0, [ok_q]), (0, 0, 4, 0, [ok_q])])
    oraw, out = out_stacks(2)
    ctx.mvref_stack_batch([odd], blocks, queries, M.SIGN_BIAS, out=out)
    res = [G.find_mvrefs(oh, 4, 4, 0, (1, 8), 0, M.SIGN_BIAS), G.find_mvrefs(oh, 0, 4, 0, (1, 8), 0, M.SIGN_BIAS)]
    assert res[0] == G.MV_REFUSED and res[1] != G.MV_REFUSED and read(out).tobytes() == expect(res).tobytes()
    # a query index past n_queries is not written at all
    blocks, queries = M.blocks_and_queries([(0, 4, 4, 6, [ok_q, ok_q])])
    oraw, out = out_stacks(2)
    ctx.mvref_stack_batch([tile], blocks, queries[:1], M.SIGN_BIAS, out=out[:MV_STACK.itemsize])
    assert (out[MV_STACK.itemsize:].cpu().numpy() == GUARD).all() and read(out)[0]["count"] != MVREF_REFUSED


def test_pmv_hand_over_into_block_motion_search(ctx):
    """the stacks' first two vectors written into an R1MeBlockCand array, then r1_estimate_motion_batch on it, equals the
    same call with the host-filled pmv: the smallest block case of me_ref.npz"""
    import os
    import test_gpu_ref_vectors as RV
    from rav1e_amd.api import ME_RESULT
    O = RV.O
    ME = np.load(os.path.join(RV.GOLD, "me_ref.npz"))
    names = [n for n in RV._me_ref_cases() if n + "_blk" in ME.files]
    name = min(names, key=lambda n: (int(ME[n + "_meta"][0]) * int(ME[n + "_meta"][1]), len(ME[n + "_blk"])))
    w, h, bd, tx, ty, tw, th, hp, full, scale, n_refs, _ = [int(v) for v in ME[name + "_meta"]]
    pads = (88, 44, 22)
    lam = [int(v) for v in ME[name + "_lambda"]]
    org = [RV.dev_plane(O.plane_from_image(ME["%s_org%d" % (name, s)].astype(np.int64), bd, pads[s], pads[s])) for s in range(3)]
    ref = [RV.dev_plane(O.plane_from_image(ME["%s_ref0_%d" % (name, s)].astype(np.int64), bd, pads[s], pads[s])) for s in range(3)]
    stats, _ = RV._me_stats_tensor(ME["%s_stats0" % name])
    prev, _ = RV._me_stats_tensor(ME["%s_prev0" % name])
    job = dict(org=org, ref=ref, stats=stats, prev=prev, tile=(tx, ty, tw, th))
    blk = ME[name + "_blk"]
    use_satd, fmode = [int(v) for v in ME[name + "_blkcfg"]]
    cols, rows = (w + 3) // 4, (h + 3) // 4
    n = len(blk)
    # stacks whose first two vectors are the fixture's pmv: count 2, 1 (pmv[1] zero) and 0 in turn, and one refused
    stacks = np.zeros(n, MV_STACK)
    c = np.zeros(n, O.ME_BLOCK_CAND)
    c["bx"], c["by"], c["w"], c["h"], c["corner"] = blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3], blk[:, 4]
    host = c.copy()
    for i in range(n):
        pmv = blk[i, 5:9].reshape(2, 2)
        count = (2, 1, 0, 3)[i % 4]
        stacks[i]["count"] = count
        stacks[i]["cand"][0]["this_mv"], stacks[i]["cand"][1]["this_mv"] = pmv[0], pmv[1]
        stacks[i]["cand"][2]["this_mv"], stacks[i]["cand"][0]["comp_mv"] = (77, -77), (55, 55)
        host[i]["pmv"] = G.mvref_pmv([tuple(int(v) for v in stacks[i]["cand"][k]["this_mv"]) + (0, 0, 0) for k in range(count)])
    refused = n - 1
    stacks[refused]["count"] = MVREF_REFUSED
    c["pmv"][refused] = host["pmv"][refused] = ((3, -3), (2, 2))          # what the array held stays
    assert c.dtype.itemsize == 16 and c.dtype.fields["pmv"][1] == 8
    import torch
    raw, dc = _guarded((n * 16,), torch.uint8)
    dc.copy_(_t(c.view(np.uint8).reshape(-1)))
    ctx.mvref_pmv_batch(_t(stacks.view(np.uint8).reshape(-1)), dc, 16, offset=8)
    assert np.array_equal(dc.cpu().numpy().view(O.ME_BLOCK_CAND), host) and _guards_intact(raw)
    kw = dict(use_satd=bool(use_satd), filter_mode=fmode, allow_hp=bool(hp))
    got = ctx.estimate_motion_batch(job, dc, cols, rows, bd, lam, n=n, **kw).cpu().numpy().view(ME_RESULT)
    want = ctx.estimate_motion_batch(job, host, cols, rows, bd, lam, **kw).cpu().numpy().view(ME_RESULT)
    assert np.array_equal(got, want)
    full_pmv = [i for i in range(n) if i % 4 == 0 and i != refused]
    ref_out = ME[name + "_blkout"]
    for i in full_pmv:                                                    # where pmv is the fixture's, so is the answer
        g = (int(got["row"][i]), int(got["col"][i]), int(got["sad"][i]), int(got["cost"][i]))
        assert g == tuple(int(v) for v in ref_out[i]), (i, g, ref_out[i])


def test_closed_loop(ctx):
    """the 16 x 16 tile: reset, then per block stack -> pmv -> store of the prescribed winner, nothing read until the end,
    against the same loop on the host statements"""
    import torch
    si = [str(n) for n in FX["seq_names"]].index("sb 16x16")
    evs = [EVS(k) for k in range(len(EVS)) if EVS(k)["seq"] == si]
    QUERIES = ((1, 8, 0), (4, 8, 0), (7, 8, 0), (1, 7, 1), (2, 8, 0))
    nq = len(QUERIES)
    raw, tile = dev_tile(ctx, si)
    host = M.fresh_tile(si)
    blocks, queries, trials = np.zeros(len(evs), MV_BLOCK), np.zeros(nq * len(evs), MV_QUERY), np.zeros(len(evs), MV_TRIAL)
    want_stacks, want_pmv = [], []
    for e, ev in enumerate(evs):
        blocks[e] = (0, ev["bo_x"], ev["bo_y"], ev["bsize"], nq, 0, nq * e)
        for q, (r0, r1, comp) in enumerate(QUERIES):
            queries[nq * e + q] = (0, (r0, r1), comp, 0)
            res = G.find_mvrefs(host, ev["bo_x"], ev["bo_y"], ev["bsize"], (r0, r1), comp, M.SIGN_BIAS)
            want_stacks.append(res)
            want_pmv.append(G.mvref_pmv(res[1]))
        mode, refs, mvs, skip = M.event_winner(ev)
        trials[e] = M.trial_record(e, mode, refs, mvs, skip)
        G.tile_blocks_store(host, ev["bo_x"], ev["bo_y"], ev["bsize"], mode, refs, mvs, skip)
    db, dq, dt = (_t(a.view(np.uint8).reshape(-1)) for a in (blocks, queries, trials))
    oraw, out = out_stacks(len(queries))
    praw, pmv = _guarded((len(queries) * 16,), torch.uint8)
    ctx.tile_blocks_reset_batch([tile])
    for e in range(len(evs)):
        ctx.mvref_stack_batch([tile], db[16 * e:16 * (e + 1)], dq, M.SIGN_BIAS, out=out, max_queries=nq)
        lo = nq * e
        ctx.mvref_pmv_batch(out[lo * MV_STACK.itemsize:(lo + nq) * MV_STACK.itemsize], pmv, 16, offset=lo * 16 + 8)
        ctx.tile_blocks_store_batch([tile], db, dt[16 * e:16 * (e + 1)])
    assert read(out).tobytes() == expect(want_stacks).tobytes()
    got_pmv = pmv.cpu().numpy().reshape(-1, 16)
    assert (got_pmv[:, :8] == GUARD).all()
    assert np.array_equal(got_pmv[:, 8:].copy().view(np.int16).reshape(-1, 2, 2), np.array(want_pmv, np.int16))
    assert np.array_equal(host_cells(tile), host["cells"])
    assert any(len(r[1]) >= 2 for r in want_stacks) and all(_guards_intact(r) for r in (raw, oraw, praw))

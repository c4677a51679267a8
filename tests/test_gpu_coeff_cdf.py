"""r1_coeff_cdf_slice_batch and r1_coeff_cdf_adapt_batch on the GPU, bit-exact and through the C ABI: the slices
against the model's gather; every sequence of tests/golden/coeff_cdf_ref.npz (the reference's write_coeffs_lv_map
executed block after block on one ContextWriter, no rollback) as that many adapt launches on ONE device context with
nothing downloaded in between; the rate against r1_coeff_rate_block_batch on slices cut from the same context; ragged
batches; the gate; refused trials; one closed loop search -> rate -> pick -> commit -> adapt.  No tolerance anywhere."""
import numpy as np
import pytest

import coeff_rate_block_model as BM
import coeff_cdf_model as DM
from coeff_rate_gpu_util import GUARD, GUARD_BYTES, _guarded, _guards_intact, _t
from rav1e_amd.types import COEFF_CDF_CONTEXT, RD_PICK

pytestmark = pytest.mark.gpu

CTX_BYTES = COEFF_CDF_CONTEXT.itemsize


def _dev_contexts(recs):
    """COEFF_CDF_CONTEXT records -> (the guarded buffer, its (n, 7872) uint8 view); the padding of every record is
    poisoned: it must come back as it went"""
    import torch
    a = np.ascontiguousarray(np.array(recs, COEFF_CDF_CONTEXT).reshape(-1))
    a["pad"] = 0x5A5A
    raw, view = _guarded((len(a), CTX_BYTES), torch.uint8)
    view.copy_(_t(a.view(np.uint8).reshape(len(a), CTX_BYTES)))
    return raw, view, a


def _host_contexts(view):
    return view.cpu().numpy().reshape(-1).view(COEFF_CDF_CONTEXT)


def _upload(planes, cb):
    """[(qc [n_txb, area], eobs [n_txb])] x 3 (chroma None) -> (qcoeffs_y, eobs_y, chroma tuple or None)"""
    dt = np.int16 if cb == 2 else np.int32
    dev = []
    for pl in planes:
        if pl is not None:
            dev += [_t(np.asarray(pl[0]).astype(dt).reshape(-1)), _t(np.asarray(pl[1]).astype(np.uint16).view(np.int16).reshape(-1))]
    return dev[0], dev[1], (None if planes[1] is None else tuple(dev[2:6]))


def _adapt(ctx, planes, cb, trials, geo, blocks, dctx, state=None, call_id=0):
    """one r1_coeff_cdf_adapt_batch call, every output between guard bytes and poisoned -> device tensors
    {"rate", "rng", "ctx"} and their raw buffers"""
    import torch
    bw, bh, ts, xdec, ydec, inter, red = geo
    n = len(trials)
    qy, ey, chroma = _upload(planes, cb)
    raws, outs = {}, {}
    for k, shape, dtype in (("rate", (n,), torch.int32), ("rng", (n,), torch.int16), ("ctx", (n, 3, 2, 16), torch.uint8)):
        raws[k], outs[k] = _guarded(shape, dtype)
    ctx.coeff_cdf_adapt_batch(qy, ey, 1, chroma, 1, trials, bw, bh, ts, xdec, ydec, inter, blocks, dctx, use_reduced_tx_set=red,
                              state=state, call_id=call_id, outs=outs)
    return outs, raws


def _planes_of(cases):
    planes = [(np.concatenate([c.qc[p] for c in cases]), np.concatenate([c.eobs[p] for c in cases])) for p in range(3)]
    if cases[0].ntx[1] == 0:
        planes = [planes[0], None, None]
    trials = np.array([c.trial for c in cases], BM.TRIAL_DTYPE)
    blocks = np.array([c.block for c in cases], BM.BLOCK_DTYPE)
    for i, c in enumerate(cases):
        for p, f in enumerate(("first_y", "first_u", "first_v")):
            trials[f][i] = sum(x.ntx[p] for x in cases[:i])
        trials["block"][i] = i
    return planes, trials, blocks


@pytest.fixture(scope="module")
def fixture():
    return DM.load_fixture()


@pytest.fixture(scope="module")
def replayed(ctx, fixture):
    """every sequence (the 16-bit ones again as 32-bit coefficients): per block one slice pair cut from the device
    context, one r1_coeff_rate_block_batch on it, one r1_coeff_cdf_adapt_batch, a device copy of the context -- all
    enqueued with no host read; everything is downloaded behind the sequence's last launch"""
    import torch
    _, seqs = fixture
    runs = []
    for s in seqs:
        for cb in ((2, 4) if s.cb == 2 else (4,)):
            raw, dctx, _ = _dev_contexts([s.context(0)])
            steps = []
            for c in s.blocks:
                planes, trials, blocks = _planes_of([c])
                blocks["cdf_sel"], blocks["cdf_sel_uv"] = 0, 1
                cdfs = torch.cat([ctx.coeff_cdf_slice_batch(dctx, c.ts, 0, c.inter, c.red),
                                  ctx.coeff_cdf_slice_batch(dctx, c.uv_ts, 1, c.inter, c.red)])
                qy, ey, chroma = _upload(planes, cb)
                ro = ctx.coeff_rate_block_batch(qy, ey, 1, chroma, 1, trials, *c.geo[:6], blocks, cdfs, use_reduced_tx_set=c.red)
                outs, raws = _adapt(ctx, planes, cb, trials, c.geo, blocks, dctx)
                steps.append((c, ro, outs, raws, raw.clone()))
            torch.cuda.synchronize()
            runs.append((s, cb, steps))
    return runs


def test_a_slices_equal_the_models_gather(ctx, fixture):
    """(a) all 19 sizes x 2 plane types x inter / intra x reduced on / off on fixture contexts and seeded random ones; the
    entries the rule does not fill are 0 (the model's), 256 guard bytes around the output intact, contexts untouched"""
    import torch
    _, seqs = fixture
    rng = np.random.default_rng(7001)
    recs = [seqs[i].context(j) for i, j in ((0, 0), (8, 3), (15, 6), (16, 4), (39, 2))]
    rand = np.zeros(4, COEFF_CDF_CONTEXT)
    rand.view("<u2")[...] = rng.integers(1, 0x10000, rand.view("<u2").shape)
    recs += list(rand)
    raw_c, dctx, host = _dev_contexts(recs)
    n = len(recs)
    raw, out = _guarded((n, 1088), torch.uint8)
    for ts in range(19):
        for pt in (0, 1):
            for inter in (0, 1):
                for red in (0, 1):
                    out.fill_(0x77)
                    ctx.coeff_cdf_slice_batch(dctx, ts, pt, inter, red, out=out)
                    got = out.cpu().numpy()
                    for i in range(n):
                        want = DM.gather(host[i], ts, pt, inter, red)
                        assert got[i].tobytes() == want.tobytes(), (ts, pt, inter, red, i)
    assert _guards_intact(raw) and _guards_intact(raw_c)
    assert _host_contexts(dctx).tobytes() == host.tobytes()


def test_b_every_sequence_on_one_device_context(replayed):
    """(b) the whole struct behind every step -- padding and 256 guard bytes included -- and rate, rng_out and ctx_out
    against the fixture"""
    seen = set()
    for s, cb, steps in replayed:
        for c, _ro, outs, raws, snap in steps:
            key = (s.name, c.step, cb)
            buf = snap.cpu().numpy()
            assert (buf[:GUARD_BYTES] == GUARD).all() and (buf[-GUARD_BYTES:] == GUARD).all(), key
            got = buf[GUARD_BYTES:-GUARD_BYTES].view("<u2")
            assert np.array_equal(got[:3930], s.packed[c.step + 1]), (key, np.nonzero(got[:3930] != s.packed[c.step + 1])[0][:8])
            assert (got[3930:] == 0x5A5A).all(), key
            assert all(_guards_intact(r) for r in raws.values()), key
            assert int(outs["rate"].cpu().numpy().view(np.uint32)[0]) == c.rate, key
            assert int(outs["rng"].cpu().numpy().view(np.uint16)[0]) == c.rng_out, key
            assert outs["ctx"].cpu().numpy().reshape(96).tolist() == c.ctx_out.tolist(), key
        seen.add((s.s, cb))
    assert {cb for _, cb in seen} == {2, 4} and len({s for s, _ in seen}) >= 40


def test_c_rate_equals_the_block_rate_on_the_cut_slices(replayed):
    """(c) at every step, rate, rng and ctx of the adapt call are r1_coeff_rate_block_batch's on the two slices
    r1_coeff_cdf_slice_batch cut from the same context in front of the step"""
    for s, cb, steps in replayed:
        for c, ro, outs, _raws, _snap in steps:
            for k in ("rate", "rng", "ctx"):
                assert ro[k].cpu().numpy().tobytes() == outs[k].cpu().numpy().tobytes(), (s.name, c.step, cb, k)
            assert int(ro["rate"].cpu().numpy().view(np.uint32)[0]) != BM.INVALID


def _pool(fixture, geo_cb):
    """the fixture blocks of one (geometry, width) and the context in front of each"""
    _, seqs = fixture
    return [(c, s.context(c.step)) for s in seqs for c in s.blocks if c.geo + (c.cb,) == geo_cb]


def _batch(fixture, geo_cb, n, rng):
    """n trials of one call: blocks of the pool in turn, each on a context of its own (the block's own, or another
    stored one of the same fixture)"""
    _, seqs = fixture
    pool = _pool(fixture, geo_cb)
    assert len(pool) >= 2, geo_cb
    cases = [pool[i % len(pool)][0] for i in range(n)]
    recs = [pool[i % len(pool)][1] if i % 3 else seqs[int(rng.integers(0, len(seqs)))].context(int(rng.integers(0, 7)))
            for i in range(n)]
    planes, trials, blocks = _planes_of(cases)
    return cases, recs, planes, trials, blocks


def _model(cases, recs):
    want = np.array(recs, COEFF_CDF_CONTEXT).reshape(-1).copy()
    res = [c.adapt(want[i:i + 1][0]) for i, c in enumerate(cases)]
    return want, res


@pytest.mark.parametrize("n", [1, 4, 5, 257])
def test_d_ragged_batches(ctx, fixture, n):
    """(d) n contexts in one call -- a lone trial, a full workgroup, one over, 64 workgroups and one wave -- against the
    model, in both widths"""
    import torch
    rng = np.random.default_rng(7100 + n)
    for geo_cb in ((8, 8, 1, 0, 0, 0, 0, 2), (4, 4, 0, 0, 0, 0, 1, 2))[n == 257:]:      # the large batch on the small blocks
        cases, recs, planes, trials, blocks = _batch(fixture, geo_cb, n, rng)
        want, res = _model(cases, recs)
        for cb in (2, 4):
            raw, dctx, _ = _dev_contexts(recs)
            outs, raws = _adapt(ctx, planes, cb, trials, geo_cb[:7], blocks, dctx)
            torch.cuda.synchronize()
            got = _host_contexts(dctx)
            want["pad"] = 0x5A5A
            bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
            assert not bad, (geo_cb, cb, n, bad[:5])
            assert _guards_intact(raw) and all(_guards_intact(r) for r in raws.values())
            assert outs["rate"].cpu().numpy().view(np.uint32).tolist() == [r["rate"] for r in res]
            assert outs["rng"].cpu().numpy().view(np.uint16).tolist() == [r["rng"] for r in res]
            assert outs["ctx"].cpu().numpy().reshape(n, 96).tolist() == [r["ctx"] for r in res]


def _states(calls):
    st = np.zeros(len(calls), RD_PICK)
    st["best_rd"], st["best_row"], st["best_slot"], st["best_call"] = 1.0, 0, 0, calls
    return _t(st.view(np.uint8).reshape(len(calls), RD_PICK.itemsize))


def test_e_gate(ctx, fixture):
    """(e) with a state array where every second best_call differs from call_id (another call's, or none), those
    contexts and their poisoned outputs are byte-identical afterwards; the others adapt as without a gate"""
    import torch
    rng = np.random.default_rng(7200)
    geo_cb = (8, 8, 1, 0, 0, 0, 0, 2)
    cases, recs, planes, trials, blocks = _batch(fixture, geo_cb, 7, rng)
    want, res = _model(cases, recs)
    calls = [1, 0, 1, -1, 1, 2, 1]
    raw, dctx, host = _dev_contexts(recs)
    outs, raws = _adapt(ctx, planes, 2, trials, geo_cb[:7], blocks, dctx, state=_states(calls), call_id=1)
    torch.cuda.synchronize()
    got = _host_contexts(dctx)
    want["pad"] = 0x5A5A
    rate, rngs, cb = outs["rate"].cpu().numpy().view(np.uint32), outs["rng"].cpu().numpy().view(np.uint16), outs["ctx"].cpu().numpy()
    for i, call in enumerate(calls):
        if call == 1:
            assert got[i].tobytes() == want[i].tobytes() and got[i].tobytes() != host[i].tobytes(), i
            assert (int(rate[i]), int(rngs[i]), cb[i].reshape(96).tolist()) == (res[i]["rate"], res[i]["rng"], res[i]["ctx"]), i
        else:
            assert got[i].tobytes() == host[i].tobytes(), i
            assert rate[i] == 0xA5A5A5A5 and rngs[i] == 0xA5A5 and (cb[i] == GUARD).all(), i
    assert _guards_intact(raw) and all(_guards_intact(r) for r in raws.values())


def test_f_a_refused_trial_leaves_its_context(ctx, fixture):
    """(f) an eob above the coded area, rng < 0x8000: rate 0xFFFFFFFF, zero side outputs, the context byte for byte as
    it was; the neighbours -- the same workgroup and the next -- adapt as in the clean batch.  What the host can see is
    R1_EINVAL and launches nothing."""
    import torch
    from rav1e_amd.api import R1Error
    rng = np.random.default_rng(7300)
    geo_cb = (8, 8, 1, 0, 0, 0, 0, 2)
    cases, recs, planes, trials, blocks = _batch(fixture, geo_cb, 6, rng)
    want, res = _model(cases, recs)
    want["pad"] = 0x5A5A
    planes = [(q.copy(), e.copy()) for q, e in planes]
    planes[2][1][int(trials["first_v"][1])] = 65          # V of trial 1: an 8x8 transform holds 64
    trials["rng"][4] = 0x7FFF
    raw, dctx, host = _dev_contexts(recs)
    outs, raws = _adapt(ctx, planes, 2, trials, geo_cb[:7], blocks, dctx)
    torch.cuda.synchronize()
    got = _host_contexts(dctx)
    rate, rngs, cb = outs["rate"].cpu().numpy().view(np.uint32), outs["rng"].cpu().numpy().view(np.uint16), outs["ctx"].cpu().numpy()
    for i in range(6):
        if i in (1, 4):
            assert got[i].tobytes() == host[i].tobytes(), i
            assert rate[i] == BM.INVALID and rngs[i] == 0 and not cb[i].any(), i
        else:
            assert got[i].tobytes() == want[i].tobytes(), i
            assert (int(rate[i]), int(rngs[i]), cb[i].reshape(96).tolist()) == (res[i]["rate"], res[i]["rng"], res[i]["ctx"]), i
    assert _guards_intact(raw) and all(_guards_intact(r) for r in raws.values())
    # host refusals: no context, a call_id outside 0..127 with a state, what the block call refuses
    before = dctx.clone()
    qy, ey, chroma = _upload(planes, 2)
    args = (qy, ey, 1, chroma, 1, trials, 8, 8, 1, 0, 0, 0, blocks, dctx)
    for kw in (dict(state=_states([0] * 6), call_id=128), dict(state=_states([0] * 6), call_id=-1)):
        with pytest.raises(R1Error):
            ctx.coeff_cdf_adapt_batch(*args, **kw)
    with pytest.raises(R1Error):
        ctx.coeff_cdf_adapt_batch(qy, ey, 0, chroma, 1, trials, 8, 8, 1, 0, 0, 0, blocks, dctx)
    base = [ctx.h, qy.data_ptr(), ey.data_ptr(), ey.numel(), 1, None, None, None, None, 0, 1, 2, _t(trials.view(np.uint8)).data_ptr(),
            0, 8, 8, 1, 0, 0, 0, 0, _t(blocks.view(np.uint8)).data_ptr(), 6, None, None, 0, None, None, None, None]
    assert ctx.lib.r1_coeff_cdf_adapt_batch(*base) == -1                       # NULL contexts, even with n = 0
    assert ctx.lib.r1_coeff_cdf_slice_batch(ctx.h, None, 1, 1, 0, 0, 0, dctx.data_ptr(), None) == -1
    assert ctx.lib.r1_coeff_cdf_slice_batch(ctx.h, dctx.data_ptr(), 1, 19, 0, 0, 0, dctx.data_ptr(), None) == -1
    assert ctx.lib.r1_coeff_cdf_slice_batch(ctx.h, dctx.data_ptr(), 1, 1, 2, 0, 0, dctx.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(before, dctx)


def test_g_closed_loop_search_rate_pick_commit_adapt(ctx, fixture):
    """(g) two blocks' decisions side by side, three blocks deep: r1_rdo_intra_split_batch (five intra candidates per
    decision, 16x16 under 8x8 transforms, DCT_DCT) -> the luma slice cut from each decision's context ->
    r1_coeff_rate_block_batch -> r1_rd_pick_batch -> r1_rd_commit_batch with win_stride = 16 * coded area ->
    r1_coeff_cdf_adapt_batch from the committed arrays, gated by the pick's state -- enqueued with no host read.  Then
    the same arrays are downloaded, decided by rdo_glue.pick_first_min on the model's rates and replayed by the model."""
    import torch
    import test_gpu_rdo_intra_split as TS
    from rav1e_amd import rdo_glue as RG
    _, seqs = fixture
    S, K, bw, ts, ntx, area, lam = 2, 5, 16, 1, 4, 64, 41.5
    geo = (bw, bw, ts, 1, 1, 0, 0)
    rec, org = TS._planes(8, 7400)
    drec, dorg = TS._dev_plane(rec), TS._dev_plane(org)
    rng = np.random.default_rng(7401)
    recs = [seqs[4].context(0), seqs[12].context(2)]
    raw, dctx, host0 = _dev_contexts(recs)
    blocks = np.zeros(S, BM.BLOCK_DTYPE)
    blocks["mi_w"] = blocks["mi_h"] = blocks["clip_w4"] = blocks["clip_h4"] = blocks["clip_uv_w4"] = blocks["clip_uv_h4"] = 255
    blocks["ctx"] = rng.integers(0, 64, (S, 3, 2, 16)) | (rng.integers(0, 3, (S, 3, 2, 16)) << 6)
    blocks["cdf_sel"] = np.arange(S)
    trials = np.zeros(S * K, BM.TRIAL_DTYPE)
    trials["first_y"], trials["block"], trials["rng"] = np.arange(S * K) * ntx, np.arange(S * K) // K, 0x8000
    win_trials = np.zeros(S, BM.TRIAL_DTYPE)
    win_trials["first_y"], win_trials["block"], win_trials["rng"] = np.arange(S) * 16, np.arange(S), 0x8000
    steps = []
    for step in range(3):
        cands = TS.make_cands(rng, S * K, bw, bw, 8, TS.W, TS.H, inside_only=True)
        blocks["y_mode"] = cands["mode"][::K]
        o = ctx.rdo_intra_split_batch(dorg, drec, (0, 0, TS.W, TS.H), bw, bw, ts, cands, 0x0001, 60, 2, want_qcoeffs=True)     # dist_kind R1_DIST_WSSE: one distortion per trial
        cdfs = ctx.coeff_cdf_slice_batch(dctx, ts, 0, 0, 0)
        ro = ctx.coeff_rate_block_batch(o["qcoeffs"].view(-1), o["eob"].view(-1), 1, None, 1, trials, *geo[:6], blocks, cdfs)
        st = ctx.rd_pick_state(S)
        ctx.rd_pick_batch(ro["rate"], o["dist"].view(-1), st, K, 1, lam, call_id=step)
        wins = {"eob_win": torch.zeros((S, 16), dtype=torch.int16, device="cuda"),
                "qcoeffs_win": torch.zeros((S, 16 * area), dtype=o["qcoeffs"].dtype, device="cuda")}
        wins = ctx.rd_commit_batch(st, step, K, 1, coeffs=(o["eob"].view(-1), o["qcoeffs"].view(-1)), ntx=ntx, outs=wins)
        ao = ctx.coeff_cdf_adapt_batch(wins["qcoeffs_win"].view(-1), wins["eob_win"].view(-1), 1, None, 1, win_trials, *geo[:6],
                                       blocks, dctx, state=st, call_id=step)
        steps.append((o, ro, st, ao, blocks.copy(), dctx.clone()))
    torch.cuda.synchronize()                                           # the first host read
    want = host0.copy()
    rows = []
    for step, (o, ro, st, ao, blk, snap) in enumerate(steps):
        qc, eob = o["qcoeffs"].cpu().numpy().reshape(S * K, ntx, area), o["eob"].cpu().numpy().view(np.uint16).reshape(S * K, ntx)
        dist = o["dist"].cpu().numpy().view(np.uint64).reshape(S, K)
        state = st.cpu().numpy().view(RD_PICK).ravel()
        for s in range(S):
            slices = np.stack([DM.gather(want[s], ts, 0, 0, 0)] * 2)
            b = blk[s].copy()
            b["cdf_sel"] = 0
            rates = [BM.coeff_rate_block([qc[s * K + i], [], []], [eob[s * K + i], [], []], *geo, trials[s * K + i], b, slices)["rate"]
                     for i in range(K)]
            assert ro["rate"].cpu().numpy().view(np.uint32)[s * K:(s + 1) * K].tolist() == rates, (step, s)
            idx, _rd, _rt, _ds = RG.pick_first_min(rates, dist[s], lam)
            assert (int(state["best_row"][s]), int(state["best_call"][s])) == (idx, step), (step, s)
            rows.append(idx)
            r = DM.adapt(want[s:s + 1][0], [qc[s * K + idx], [], []], [eob[s * K + idx], [], []], *geo, win_trials[s], blk[s])
            assert int(ao["rate"].cpu().numpy().view(np.uint32)[s]) == r["rate"] == rates[idx], (step, s)
            assert ao["ctx"].cpu().numpy().reshape(S, 96)[s].tolist() == r["ctx"], (step, s)
        assert _host_contexts(snap).tobytes() == want.tobytes(), step
    assert len(set(rows)) >= 2 and want.tobytes() != host0.tobytes()
    assert _guards_intact(raw)

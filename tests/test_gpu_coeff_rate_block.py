"""r1_coeff_rate_block_batch on the GPU, integer-exact and through the C ABI: every case of
tests/golden/coeff_rate_block_ref.npz (the reference's write_coeffs_lv_map executed over a block's luma, U and V
transform blocks on one writer behind a few head symbols) in both coefficient widths, luma-only trials against
r1_coeff_rate_chain_batch called here, trials that share one luma set, ragged batches against the Python model the
fixture pins (tests/coeff_rate_block_model.py), odd element offsets with guard bytes around every output, bad
device-resident data, host refusals."""
import numpy as np
import pytest

import coeff_rate_model as M
import coeff_rate_chain_model as CM
import coeff_rate_block_model as BM
from coeff_rate_gpu_util import GUARD, _guarded, _guards_intact, _t

pytestmark = pytest.mark.gpu

OUTS = ("rate", "plane_rate", "rng", "cul_level", "ctx")


def _shifted(host, lead):
    """the array on the device behind `lead` elements (rows) of poison: an odd element offset into its buffer"""
    host = np.ascontiguousarray(host)
    poison = GUARD if host.dtype == np.uint8 else 0x5A5A
    whole = _t(np.concatenate([np.full((lead,) + host.shape[1:], poison, host.dtype), host]))
    return (whole, lead, poison), whole[lead:]


def _call(ctx, planes, steps, cb, trials, geo, blocks, cdfs, side=True, lead=0):
    """host arrays in, (rate [n], plane_rate [n, 3], rng [n], cul [n, 3, 16], ctx [n, 96]) out.  planes: [(qc [n_txb, area],
    eobs [n_txb])] x 3, the chroma entries None for a call without chroma arrays; geo = (bw, bh, ts, xdec, ydec, inter, red).
    Every output sits between guard bytes; the device copies of the inputs are compared with what was uploaded.
    lead: descriptors, snapshots and coefficient arrays start that many elements (records) into their buffers."""
    import torch
    bw, bh, ts, xdec, ydec, inter, red = geo
    n = len(trials)
    dt = np.int16 if cb == 2 else np.int32
    host, dev, keep = [], [], []
    for pl in planes:
        if pl is None:
            continue
        hq, he = np.asarray(pl[0]).astype(dt), np.asarray(pl[1]).astype(np.uint16).view(np.int16).reshape(-1)
        for h in (hq, he):
            whole, view = _shifted(h.reshape(-1), lead) if lead else (None, _t(h.reshape(-1)))
            host.append(h.reshape(-1))
            dev.append(view)
            keep.append(whole)
    chroma = None if planes[1] is None else tuple(dev[2:6])
    descs = []
    for h, size in ((trials, 24), (blocks, 108), (cdfs, 1088)):
        hb = np.ascontiguousarray(h).view(np.uint8).reshape(len(h), size)
        whole, view = _shifted(hb, lead) if lead else (None, _t(hb))
        host.append(hb.reshape(-1))
        dev.append(view.reshape(-1))
        keep.append(whole)
        descs.append(view.reshape(-1))
    raws, outs = {}, {}
    for k, shape, dtype in (("rate", (n,), torch.int32), ("plane_rate", (n, 3), torch.int32), ("rng", (n,), torch.int16),
                            ("cul_level", (n, 3, 16), torch.uint8), ("ctx", (n, 3, 2, 16), torch.uint8)):
        raws[k], outs[k] = _guarded(shape, dtype)
    o = ctx.coeff_rate_block_batch(dev[0], dev[1], steps[0], chroma, steps[1], descs[0], bw, bh, ts, xdec, ydec, inter, descs[1],
                                   descs[2], use_reduced_tx_set=red, want_plane_rate=side, want_rng=side, want_cul_level=side,
                                   want_ctx=side, outs=outs if side else {"rate": outs["rate"]})
    torch.cuda.synchronize()
    assert all(_guards_intact(r) for r in raws.values())
    for h, d in zip(host, dev):
        assert d.cpu().numpy().tobytes() == h.tobytes()
    for k in keep:            # the poison in front of a shifted input is as it was
        if k is not None:
            whole, n_lead, poison = k
            assert (whole[:n_lead].cpu().numpy() == poison).all()
    rate = outs["rate"].cpu().numpy().view(np.uint32)
    if not side:
        assert set(o) == {"rate"}
        assert all(bool((raws[k] == GUARD).all()) for k in OUTS[1:])       # a NULL optional output: nothing written
        return rate, None, None, None, None
    return (rate, outs["plane_rate"].cpu().numpy().view(np.uint32), outs["rng"].cpu().numpy().view(np.uint16),
            outs["cul_level"].cpu().numpy(), outs["ctx"].cpu().numpy().reshape(n, 96))


def _assert_equal(got, want, key):
    for name, g, w in zip(OUTS, got, want):
        g, w = np.asarray(g), np.asarray(w).reshape(np.asarray(g).shape)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (key, name, "first bad trial", int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist())


def _batch_of(cases):
    """fixture cases of one call -> (planes, trials, blocks, cdfs): every case its own blocks, block state and snapshots"""
    planes = [(np.concatenate([c.qc[p] for c in cases]), np.concatenate([c.eobs[p] for c in cases])) for p in range(3)]
    trials = np.array([c.trial for c in cases], BM.TRIAL_DTYPE)
    blocks = np.array([c.block for c in cases], BM.BLOCK_DTYPE)
    for i, c in enumerate(cases):
        for p, f in enumerate(("first_y", "first_u", "first_v")):
            trials[f][i] = sum(x.ntx[p] for x in cases[:i])
        trials["block"][i] = i
        blocks["cdf_sel"][i], blocks["cdf_sel_uv"][i] = 2 * i, 2 * i + 1
    return planes, trials, blocks, np.concatenate([c.cdfs for c in cases])


@pytest.fixture(scope="module")
def fixture():
    return BM.load_fixture()


def test_every_fixture_case_in_both_widths(ctx, fixture):
    """1: rate, per-plane rates (differences of the recorded tell_frac values), final rng, cul_level and the 96 context
    bytes of every case; the cases grouped into calls by everything a call fixes.  A case runs in the width it was
    generated for, and the 16-bit cases again as 32-bit coefficients."""
    _, cases = fixture
    groups = {}
    for c in cases:
        widths = (2, 4) if c.cb == 2 else (4,)
        for cb in widths:
            groups.setdefault((c.bw, c.bh, c.ts, c.xdec, c.ydec, c.inter, c.red, cb), []).append(c)
    seen = set()
    for key, cs in sorted(groups.items()):
        planes, trials, blocks, cdfs = _batch_of(cs)
        if cs[0].ntx[1] == 0:
            planes = [planes[0], None, None]          # 4x16 / 16x4 in 4:2:0: no chroma transform block, no chroma arrays
        got = _call(ctx, planes, (1, 1), key[7], trials, key[:7], blocks, cdfs)
        ends = np.stack([c.tell[:, 15].astype(np.int64) for c in cs])       # tell_frac behind each plane's last block
        want_plane = np.diff(np.concatenate([np.zeros((len(cs), 1), np.int64), ends], axis=1), axis=1)
        want = ([c.rate for c in cs], want_plane, [c.rng_out for c in cs], [c.cul for c in cs], [c.ctx_out for c in cs])
        _assert_equal(got, want, key)
        assert (got[1].sum(axis=1) == got[0]).all()
        seen |= {(c.k, key[7]) for c in cs}
    assert {k for k, _ in seen} == set(range(len(cases))) and {cb for _, cb in seen} == {2, 4}


def test_luma_only_trials_equal_the_chain_call(ctx):
    """2: on the chain fixture's inputs, do_chroma = 0 and rng = 0x8000 give what r1_coeff_rate_chain_batch gives in this
    test: with one type per block (luma step 1) and with two types per transform block (luma step nt = 2, the layout of
    r1_rdo_txsearch_batch)"""
    _, cases = CM.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c.bw, c.bh, c.ts, c.tt, c.inter, c.red, c.cb), []).append(c)
    stepped = 0
    for (bw, bh, ts, tt, inter, red, cb), cs in sorted(groups.items()):
        n, ntx = len(cs), cs[0].ntx
        chains = np.array([c.chain for c in cs], CM.CHAIN_DTYPE)
        chains["cdf_sel"] = np.arange(n)
        cdfs = np.concatenate([c.cdfs for c in cs])
        blocks = np.zeros(n, BM.BLOCK_DTYPE)
        blocks["ctx"][:, 0, 0], blocks["ctx"][:, 0, 1] = chains["above"], chains["left"]
        blocks["ctx"][:, 1:] = 0x47                       # chroma bytes pass through untouched
        for f in ("mi_w", "mi_h", "clip_w4", "clip_h4", "y_mode", "cdf_sel"):
            blocks[f] = chains[f]
        qc, eobs = np.concatenate([c.qc for c in cs]), np.concatenate([c.eobs for c in cs])
        # a partner type of the same class (the same scan order, so the fixture's coefficients stay well-formed)
        partner = {0: 1, 1: 0, 3: 0, 9: 0, 10: 12, 11: 13}.get(tt)
        mask1 = 1 << tt
        variants = [(mask1, 1, qc, eobs, [tt])]
        if partner is not None and (M.tx_type_mask(ts, inter, red) >> partner) & 1:
            types = sorted((tt, partner))
            q2 = np.repeat(qc, 2, axis=0)                 # order 1: [block][transform block][type]
            e2 = np.repeat(eobs, 2)
            variants.append((mask1 | 1 << partner, 2, q2, e2, types))
            stepped += 1
        for mask, nt, q, e, types in variants:
            import torch
            dq, de = _t(q.astype(np.int16 if cb == 2 else np.int32)), _t(e.astype(np.uint16).view(np.int16))
            o = ctx.coeff_rate_chain_batch(dq, de, mask, bw, bh, ts, 1 if nt == 2 else 0, inter, chains, cdfs, use_reduced_tx_set=red)
            torch.cuda.synchronize()
            trials = np.zeros(n * nt, BM.TRIAL_DTYPE)
            for i in range(n):
                for j, t in enumerate(types):
                    trials[i * nt + j] = (i * ntx * nt + j, 0, 0, i, 0x8000, t, 0, 0, (0, 0, 0))
            got = _call(ctx, [(q, e), None, None], (nt, 1), cb, trials, (bw, bh, ts, 1, 1, inter, red), blocks, cdfs)
            key = (bw, bh, ts, tt, inter, red, cb, nt)
            want_rate = o["rate"].cpu().numpy().view(np.uint32).reshape(-1)
            assert (got[0] == want_rate).all() and (want_rate != BM.INVALID).all(), key
            assert (got[1][:, 0] == want_rate).all() and not got[1][:, 1:].any(), key
            assert (got[3][:, 0, :ntx] == o["cul_level"].cpu().numpy().reshape(n * nt, ntx)).all() and not got[3][:, 1:].any(), key
            assert (got[4][:, :32] == o["ctx"].cpu().numpy().reshape(n * nt, 32)).all() and (got[4][:, 32:] == 0x47).all(), key
            if nt == 1:
                assert got[0].tolist() == [c.rate for c in cs], key
    assert stepped >= 10


def _random_batch(rng, geo, cb, n, n_sets=None, n_blocks=3):
    """n trials of one call on random well-formed coefficients: n_sets luma / chroma sets (default: one per trial) that
    the trials index at random, n_blocks block states with edges and non-zero contexts, 2 * n_blocks snapshots, every
    legal luma and chroma type, random rng"""
    bw, bh, ts, xdec, ydec, inter, red = geo
    luma, uv, _ = BM.plane_grids(bw, bh, ts, xdec, ydec, inter)
    n_sets = n if n_sets is None else n_sets
    big = 32767 if cb == 2 else (1 << 20) - 1
    pool = np.array([0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 9, 14, 15, 16, 127, 128, 300, big])
    y_types = [t for t in range(16) if (M.tx_type_mask(ts, inter, red) >> t) & 1]
    uv_types = [t for t in range(16) if BM.uv_type_ok(uv[0], t)]
    set_types = [(int(rng.choice(y_types)), int(rng.choice(uv_types))) for _ in range(n_sets)]
    planes = []
    for p, g in enumerate((luma, uv, uv)):
        tsz, ntx = g[0], g[1]
        W, H = M.coded_dims(tsz)
        q, e = np.zeros((n_sets * ntx, W * H), np.int64), np.zeros(n_sets * ntx, np.int64)
        for s in range(n_sets * ntx):
            r = rng.random()
            eob = 0 if r < 0.25 else (W * H if r < 0.3 else int(rng.integers(1, min(W * H, 24) + 1)))
            e[s] = eob
            if eob:
                scan = np.array(M.scan_order(tsz, set_types[s // ntx][p != 0])[:eob])
                v = rng.choice(pool, eob) * rng.choice([-1, 1], eob)
                if v[-1] == 0:
                    v[-1] = rng.choice([-1, 1, 2, -3, 15, -big])
                q[s, scan] = v
        planes.append((q, e))
    blocks = np.zeros(n_blocks, BM.BLOCK_DTYPE)
    for i, b in enumerate(blocks):
        b["ctx"] = rng.integers(0, 64, (3, 2, 16)) | (rng.integers(0, 3, (3, 2, 16)) << 6)
        b["ctx"][rng.integers(0, 3)] = 0
        edge = int(rng.integers(0, 3))
        b["mi_w"] = b["clip_w4"] = 255 if edge != 1 or bw < 16 else (bw >> 2) - 1
        b["mi_h"] = b["clip_h4"] = 255 if edge != 2 or bh < 16 else (bh >> 2) // 2
        adj_x, adj_y = int(bw == 4) * xdec, int(bh == 4) * ydec
        b["clip_uv_w4"] = min(255, ((int(b["clip_w4"]) + adj_x) << 2 >> xdec) >> 2)
        b["clip_uv_h4"] = min(255, ((int(b["clip_h4"]) + adj_y) << 2 >> ydec) >> 2)
        b["y_mode"], b["cdf_sel"], b["cdf_sel_uv"] = rng.integers(0, 13), 2 * i, 2 * i + 1
    cdfs = np.concatenate([np.stack([M.random_cdfs(rng, 1, ts, inter, red)[0], M.random_cdfs(rng, 1, uv[0], inter, red)[0]])
                           for _ in range(n_blocks)])
    trials = np.zeros(n, BM.TRIAL_DTYPE)
    for i, t in enumerate(trials):
        s = i if n_sets == n else int(rng.integers(0, n_sets))
        t["first_y"], t["first_u"], t["first_v"] = s * luma[1], s * uv[1], s * uv[1]
        t["block"], t["rng"] = rng.integers(0, n_blocks), rng.choice([0x8000, 0xFFFF, int(rng.integers(0x8000, 0x10000))])
        t["tx_type"], t["uv_tx_type"], t["do_chroma"] = set_types[s][0], set_types[s][1], rng.integers(0, 4) != 0
    return planes, trials, blocks, cdfs


def _model(planes, steps, geo, trials, blocks, cdfs):
    return BM.coeff_rate_block_batch(planes, steps, *geo, trials, blocks, cdfs)


def test_trials_that_share_a_luma_set_equal_private_copies(ctx):
    """3: two (and more) trials name the same luma transform blocks through first_y and differ in their chroma; the
    results are those of the same trials on private copies of the luma blocks, and the model's"""
    rng = np.random.default_rng(9301)
    for geo, cb in (((16, 16, 1, 1, 1, 0, 0), 2), ((64, 64, 2, 0, 0, 1, 0), 4), ((8, 8, 0, 1, 1, 1, 0), 2)):
        planes, trials, blocks, cdfs = _random_batch(rng, geo, cb, 6)
        ntx = BM.plane_grids(*geo[:5], geo[5])[0][1]
        trials["do_chroma"] = 1
        trials["tx_type"] = trials["tx_type"][0]
        shared = trials.copy()
        shared["first_y"] = 0                          # everyone reads luma set 0 ...
        private = trials.copy()                        # ... or its own copy of it
        lq = np.concatenate([planes[0][0][:ntx]] * 6)
        le = np.concatenate([planes[0][1][:ntx]] * 6)
        a = _call(ctx, planes, (1, 1), cb, shared, geo, blocks, cdfs)
        b = _call(ctx, [(lq, le), planes[1], planes[2]], (1, 1), cb, private, geo, blocks, cdfs)
        _assert_equal(a, b, geo)
        _assert_equal(a, _model(planes, (1, 1), geo, shared, blocks, cdfs), geo)
        assert (a[0] != BM.INVALID).all() and len(set(a[0].tolist())) > 1


@pytest.mark.parametrize("geo", [(8, 8, 0, 1, 1, 0, 0), (16, 16, 1, 1, 0, 1, 0), (64, 64, 2, 0, 0, 0, 1), (4, 8, 5, 1, 1, 1, 1),
                                 (4, 16, 13, 1, 1, 0, 0), (64, 16, 18, 0, 0, 1, 0)])
def test_ragged_batches_equal_the_model(ctx, geo):
    """4: n = 1, 5, 7 (a lone trial, ragged last workgroups) against the model, both widths, trials that pick their sets
    and block states at random; at n = 5 also with no optional output"""
    rng = np.random.default_rng(9400 + sum(geo) * 7 + geo[2])
    for step, n in enumerate((1, 5, 7)):
        cb = (2, 4)[(step + geo[2]) % 2]
        planes, trials, blocks, cdfs = _random_batch(rng, geo, cb, n, n_sets=max(1, n - 2))
        want = _model(planes, (1, 1), geo, trials, blocks, cdfs)
        _assert_equal(_call(ctx, planes, (1, 1), cb, trials, geo, blocks, cdfs), want, (geo, n))
        assert (want[0] != BM.INVALID).all()
        if n == 5:
            assert (_call(ctx, planes, (1, 1), cb, trials, geo, blocks, cdfs, side=False)[0] == want[0]).all()


def test_odd_element_offsets_and_guards(ctx):
    """5: the trial, block and snapshot arrays start one record, the coefficient and eob arrays one element (2 or 4
    bytes) into their buffers; luma step 3 and chroma step 2 leave foreign blocks between a trial's own;
    256 poison bytes around every output stay as they were (checked in _call for every test of this file)"""
    rng = np.random.default_rng(9500)
    for geo, cb in (((16, 16, 1, 1, 1, 0, 0), 2), ((8, 8, 0, 1, 1, 1, 0), 4)):
        planes, trials, blocks, cdfs = _random_batch(rng, geo, cb, 5)
        grids = BM.plane_grids(*geo[:5], geo[5])
        # spread: transform block k of set s moves from s * ntx + k to (s * ntx) * step + k * step
        spread, steps = [], (3, 2)
        for p, (q, e) in enumerate(planes):
            st = steps[0 if p == 0 else 1]
            q2, e2 = np.full((len(q) * st, q.shape[1]), 1, q.dtype), np.full(len(e) * st, 1, e.dtype)
            q2[::st], e2[::st] = q, e
            spread.append((q2, e2))
        tr = trials.copy()
        tr["first_y"] *= steps[0]
        tr["first_u"] *= steps[1]
        tr["first_v"] *= steps[1]
        want = _model(planes, (1, 1), geo, trials, blocks, cdfs)
        assert [grids[p][1] for p in range(3)] == [4, 1, 1]
        _assert_equal(_call(ctx, spread, steps, cb, tr, geo, blocks, cdfs, lead=1), want, geo)
        _assert_equal(_model(spread, steps, geo, tr, blocks, cdfs), want, geo)


def test_bad_device_data_marks_its_trial_only(ctx):
    """6: every device-resident fault of the header gives its trial 0xFFFFFFFF and zero side outputs; the other trials of
    the batch -- the same workgroup and the next -- keep the values of the clean batch"""
    rng = np.random.default_rng(9600)
    geo, cb = (16, 16, 1, 1, 1, 0, 0), 2
    planes, trials, blocks, cdfs = _random_batch(rng, geo, cb, 6, n_blocks=6)
    trials["do_chroma"], trials["block"] = 1, np.arange(6)
    blocks["mi_w"] = blocks["mi_h"] = blocks["clip_w4"] = blocks["clip_h4"] = 255
    blocks["clip_uv_w4"] = blocks["clip_uv_h4"] = 127
    clean = _call(ctx, planes, (1, 1), cb, trials, geo, blocks, cdfs)
    _assert_equal(clean, _model(planes, (1, 1), geo, trials, blocks, cdfs), "clean")
    assert (clean[0] != BM.INVALID).all()
    V = 2       # the victim: inside the first workgroup of four

    def check(name, planes_=planes, trials_=trials, blocks_=blocks, victims=(V,)):
        got = _call(ctx, planes_, (1, 1), cb, trials_, geo, blocks_, cdfs)
        for i in range(6):
            if i in victims:
                assert got[0][i] == BM.INVALID and not got[1][i].any() and got[2][i] == 0 and not got[3][i].any() \
                    and not got[4][i].any(), (name, i)
            else:
                for k in range(5):
                    assert (np.asarray(got[k][i]) == np.asarray(clean[k][i])).all(), (name, i, OUTS[k])

    def with_trial(**kw):
        t = trials.copy()
        for f, v in kw.items():
            t[f][V] = v
        return t

    def with_block(**kw):
        b = blocks.copy()
        for f, v in kw.items():
            b[f][V] = v
        return b

    check("tx_type outside the set", trials_=with_trial(tx_type=next(t for t in range(16) if not (M.tx_type_mask(1, 0, 0) >> t) & 1)))
    check("tx_type 16", trials_=with_trial(tx_type=16))
    check("tx_type 255", trials_=with_trial(tx_type=255))
    check("uv_tx_type 16", trials_=with_trial(uv_tx_type=16))
    check("rng below 0x8000", trials_=with_trial(rng=0x7FFF))
    check("rng 0", trials_=with_trial(rng=0))
    check("block beyond n_blocks", trials_=with_trial(block=6))
    check("block 2^32 - 1", trials_=with_trial(block=0xFFFFFFFF))
    n_y, n_uv = len(planes[0][1]), len(planes[1][1])
    check("first_y beyond the array", trials_=with_trial(first_y=n_y - 3))
    check("first_y 2^32 - 1", trials_=with_trial(first_y=0xFFFFFFFF))
    check("first_u beyond the array", trials_=with_trial(first_u=n_uv))
    check("first_v beyond the array", trials_=with_trial(first_v=n_uv + 7))
    check("y_mode 13", blocks_=with_block(y_mode=13))
    check("cdf_sel beyond n_cdfs", blocks_=with_block(cdf_sel=12))
    check("cdf_sel_uv beyond n_cdfs", blocks_=with_block(cdf_sel_uv=255))
    check("mi_w above clip_w4", blocks_=with_block(mi_w=4, clip_w4=3))
    check("mi_h above clip_h4", blocks_=with_block(mi_h=200, clip_h4=199))
    check("chroma clip below the grid, w", blocks_=with_block(clip_uv_w4=0))
    check("chroma clip below the grid, h", blocks_=with_block(clip_uv_h4=0))
    for p in range(3):
        e = [x[1].copy() for x in planes]
        e[p][int(trials[("first_y", "first_u", "first_v")[p]][V]) + (3 if p == 0 else 0)] = 64 + 1      # 8x8 luma and chroma transforms
        check("eob above the coded area, plane %d" % p, planes_=[(planes[i][0], e[i]) for i in range(3)])
    # chroma asked for where the call has no chroma arrays: every trial with do_chroma fails, the others are the chain's
    t = trials.copy()
    t["do_chroma"] = [1, 0, 1, 0, 0, 1]
    got = _call(ctx, [planes[0], None, None], (1, 1), cb, t, geo, blocks, cdfs)
    assert [int(v) == BM.INVALID for v in got[0]] == [True, False, True, False, False, True]
    t0 = trials.copy()
    t0["do_chroma"] = 0
    luma_only = _call(ctx, planes, (1, 1), cb, t0, geo, blocks, cdfs)
    for i in (1, 3, 4):
        assert all((np.asarray(got[k][i]) == np.asarray(luma_only[k][i])).all() for k in range(5)), i
    # a 32-point chroma transform knows DCT_DCT and IDTX only
    geo2 = (64, 64, 4, 0, 0, 1, 0)
    planes2, trials2, blocks2, cdfs2 = _random_batch(rng, geo2, 4, 5)
    trials2["do_chroma"] = 1
    clean2 = _call(ctx, planes2, (1, 1), 4, trials2, geo2, blocks2, cdfs2)
    assert (clean2[0] != BM.INVALID).all()
    trials2["uv_tx_type"][1] = 10
    got2 = _call(ctx, planes2, (1, 1), 4, trials2, geo2, blocks2, cdfs2)
    assert got2[0][1] == BM.INVALID and not got2[4][1].any()
    assert all((np.delete(np.asarray(got2[k]), 1, axis=0) == np.delete(np.asarray(clean2[k]), 1, axis=0)).all() for k in range(5))


def test_host_refusals_launch_nothing(ctx):
    """7: what the host can see returns R1_EINVAL on a live context with n = 3, and no output byte changes"""
    import torch
    rng = np.random.default_rng(9700)
    geo, cb = (16, 16, 1, 1, 1, 0, 0), 2
    planes, trials, blocks, cdfs = _random_batch(rng, geo, cb, 3)
    dev = [_t(np.asarray(a).astype(np.int16 if i % 2 == 0 else np.uint16).view(np.int16).reshape(-1))
           for i, a in enumerate(x for pl in planes for x in pl)]
    dtr, dbl, dcd = (_t(np.ascontiguousarray(a).view(np.uint8).reshape(-1)) for a in (trials, blocks, cdfs))
    outs = [torch.full((3 * k,), GUARD, dtype=torch.uint8, device="cuda") for k in (4, 12, 2, 48, 96)]
    base = dict(qcoeffs_y=dev[0].data_ptr(), eobs_y=dev[1].data_ptr(), n_txb_y=len(planes[0][1]), step_y=1,
                qcoeffs_u=dev[2].data_ptr(), eobs_u=dev[3].data_ptr(), qcoeffs_v=dev[4].data_ptr(), eobs_v=dev[5].data_ptr(),
                n_txb_uv=len(planes[1][1]), step_uv=1, coeff_bytes=2, trials=dtr.data_ptr(), n=3, bw=16, bh=16, tx_size=1, xdec=1,
                ydec=1, is_inter=0, use_reduced_tx_set=0, blocks=dbl.data_ptr(), n_blocks=3, cdfs=dcd.data_ptr(), n_cdfs=6,
                rate_out=outs[0].data_ptr(), plane_rate_out=outs[1].data_ptr(), rng_out=outs[2].data_ptr(),
                cul_level_out=outs[3].data_ptr(), ctx_out=outs[4].data_ptr())
    order = list(base)

    def call(**over):
        v = dict(base, **over)
        rc = ctx.lib.r1_coeff_rate_block_batch(ctx.h, *[v[k] for k in order], None)
        torch.cuda.synchronize()
        return rc

    bad = [dict(coeff_bytes=3), dict(tx_size=19), dict(tx_size=-1), dict(bw=12), dict(bw=128, bh=128, tx_size=4), dict(bw=64, bh=8),
           dict(tx_size=2, bw=8, bh=8), dict(tx_size=0, bw=32, bh=32), dict(xdec=0, ydec=1), dict(xdec=2), dict(ydec=-1),
           dict(bw=8, bh=16, xdec=1, ydec=0), dict(step_y=0), dict(step_uv=-1), dict(n_txb_y=-1), dict(n_txb_uv=-1), dict(n_blocks=0),
           dict(n_cdfs=0), dict(n_cdfs=257), dict(qcoeffs_y=None), dict(eobs_y=None), dict(trials=None), dict(blocks=None),
           dict(cdfs=None), dict(rate_out=None), dict(qcoeffs_u=None), dict(eobs_v=None), dict(qcoeffs_v=None, eobs_v=None)]
    for over in bad:
        assert call(**over) == -1, over
        assert all(bool((o == GUARD).all()) for o in outs), over
    assert call() == 0
    got = outs[0].cpu().numpy().view(np.uint32)
    assert (got == _model(planes, (1, 1), geo, trials, blocks, cdfs)[0]).all()

"""r1_rdo_intra_cand_batch on the GPU: the intra candidate in one launch (prediction made on the CU) against
  * the two-launch device route it replaces: r1_predict_intra_batch -> r1_rdo_txsearch_batch(pred = ...), and
  * the oracle's composition r1o_dispatch_predict_intra -> r1o_rdo_txsearch_batch on the same edge buffers,
bit for bit, on seeded inputs at the smallest shapes that reach each path of the kernel."""
import ctypes as C

import numpy as np
import pytest

import cand_size_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

TX_DIMS = K.TX_DIMS
GUARD = 0x5A


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_plane(hp):
    from rav1e_amd.api import Plane
    return Plane.from_numpy(hp.data, hp.width, hp.height, hp.bit_depth, hp.xpad, hp.ypad)


def _guarded(shape, dtype):
    """a device tensor of `shape` inside a buffer with 64 guard bytes before and behind it"""
    import torch
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((n + 128,), GUARD, dtype=torch.uint8, device="cuda")
    return raw, raw[64:64 + n].view(dtype).view(*shape)


def _guards_intact(raw):
    g = raw.cpu().numpy()
    return bool((g[:64] == GUARD).all() and (g[-64:] == GUARD).all())


def make_case(rng, ctx, rec, drec, ts, n, group, chroma=False):
    """n candidates in n / group blocks of the plane `rec` (random positions on the block grid, tile = the frame,
    blocks at the origin, in the first row / column and cut by the right / bottom frame edge among them): the edge
    sets from r1_intra_edges_batch -- mode-specific when group == 1, mode None when the modes of a block share one
    -- and the R1IntraCand list after predict_intra's PAETH / CFL remaps."""
    from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND
    w, h = TX_DIMS[ts]
    ns = n // group
    gx, gy = (rec.width + w - 1) // w, (rec.height + h - 1) // h
    bx, by = rng.integers(0, gx, ns) * w, rng.integers(0, gy, ns) * h
    # the geometries every call must hold when it has room for them
    fixed = [(0, 0), (0, (gy - 1) * h), ((gx - 1) * w, 0), ((gx - 1) * w, (gy - 1) * h), (w, 0), (0, h)]
    for k, (x, y) in enumerate(fixed[:ns]):
        bx[k], by[k] = x, y
    sets = np.repeat(np.arange(ns), group)
    x, y = bx[sets], by[sets]
    if chroma:
        mode = rng.choice([0, 13], n)
    else:
        mode = rng.integers(0, 13, n)
        mode[:min(n, 3)] = 0                      # DC at the fixed geometries: lens (0, 0), (full, 0), (0, full)
    delta = np.where((mode >= 1) & (mode <= 8), rng.integers(-3, 4, n), 0)
    flags_s = rng.integers(0, 8, ns)
    flags = flags_s[sets]
    ec = np.zeros(ns, INTRA_EDGE_CAND)
    ec["x"], ec["y"], ec["flags"] = bx, by, flags_s
    if group == 1:
        ec["mode"], ec["angle_delta"] = mode, delta
    else:
        ec["mode"] = -1
    edges, lens = ctx.intra_edges_batch(drec, (0, 0, rec.width, rec.height), ts, ec)
    var = np.where((x == 0) & (y == 0), 0, np.where(y == 0, 1, np.where(x == 0, 2, 3)))
    pm = mode.copy()
    pa = pm == 12
    pm = np.where(pa & (var == 0), 0, np.where(pa & (var == 2), 1, np.where(pa & (var == 1), 2, pm)))
    alpha = rng.integers(-16, 17, n)
    pm = np.where((pm == 13) & (alpha == 0), 0, pm)
    base_angle = np.array([0, 90, 180, 45, 135, 113, 157, 203, 67] + [0] * 5)[pm]
    angle = np.where(pm == 13, alpha, base_angle + 3 * delta)
    ief = np.where(flags & 1, rng.integers(1, 3, n), 0)
    ic = np.zeros(n, INTRA_CAND)
    ic["mode"], ic["variant"], ic["angle"], ic["ief"] = pm, var, angle, ief
    ic["avail_w"] = np.minimum(w, rec.width - x).clip(1, 64)
    ic["avail_h"] = np.minimum(h, rec.height - y).clip(1, 64)
    # candidate order: one wave holds different modes and different edge sets
    if group == 1:
        perm = rng.permutation(n)
        ic, sets, x, y = ic[perm], sets[perm], x[perm], y[perm]
        import torch
        dperm = torch.from_numpy(perm).cuda()
        edges, lens = edges[dperm].contiguous(), lens[dperm].contiguous()
        bx, by = x.copy(), y.copy()
        sets = np.arange(n)
    ac = rng.integers(-2000, 2000, (n, w * h)).astype(np.int16) if chroma else None
    rc = np.zeros(n, O.RDO_CAND)
    rc["ox"], rc["oy"] = x, y
    pos = np.stack([bx, by], 1).astype(np.int16)
    return dict(ic=ic, rc=rc, sets=sets, edges=edges, lens=lens, pos=_t(pos), ac=ac)


def check_call(ctx, oracle, org, dorg, ts, bd, cs, group, mask, qi, kind, scales, dscales, xdec, ydec, full, key):
    """one fused call against the two-launch device route and the oracle composition; -> the oracle's eob"""
    import torch
    w, h = TX_DIMS[ts]
    n, nt = len(cs["ic"]), bin(mask).count("1")
    carea = min(w, 32) * min(h, 32)
    dt, ct = (np.uint8, np.int16) if bd == 8 else (np.uint16, np.int32)
    pt, cdt = (torch.uint8, torch.int16) if bd == 8 else (torch.int16, torch.int32)
    dac = _t(cs["ac"]) if cs["ac"] is not None else None
    # -- the fused launch, every output inside guard words
    spec = {"eob": ((n, nt), torch.int16), "dist": ((n, nt), torch.int64)}
    if full:
        spec.update(sad=((n,), torch.int32), satd=((n,), torch.int32), qcoeffs=((n, nt, carea), cdt),
                    pred=((n, h, w), pt))
        if kind:
            spec["rec"] = ((n, nt, h, w), pt)
        else:
            spec["est_rate"] = ((n, nt), torch.int64)
    raws, outs = {}, {}
    for k, (shape, dtype) in spec.items():
        raws[k], outs[k] = _guarded(shape, dtype)
    o = ctx.rdo_intra_cand_batch(dorg, w, h, cs["ic"], cs["pos"], cs["edges"], cs["lens"], mask, qi, kind,
                                 edge_group=group, ac=dac, scales=dscales, xdec=xdec, ydec=ydec, outs=outs)
    assert set(o) == set(spec), key
    torch.cuda.synchronize()
    for k in raws:
        assert _guards_intact(raws[k]), (key, k, "guard words")
    # -- the route it replaces, on the device
    dsets = torch.from_numpy(cs["sets"]).cuda()
    e_c, l_c = cs["edges"][dsets].contiguous(), cs["lens"][dsets].contiguous()
    pred = ctx.predict_intra_batch(ts, cs["ic"], e_c, l_c, bd, ac=dac)
    r = ctx.rdo_txsearch_batch(dorg, None, w, h, cs["rc"], mask, qi, kind, scales=dscales, xdec=xdec, ydec=ydec,
                               is_intra=1, want_sad=True, want_satd=True, want_est_rate=kind == 0,
                               want_qcoeffs=True, want_rec=bool(kind), pred=pred)
    r["pred"] = pred
    for k in spec:
        assert torch.equal(o[k], r[k]), (key, k, "two-launch route")
    # -- the oracle, call by call on the same edge buffers
    eh, lh = cs["edges"].cpu().numpy().view(dt), cs["lens"].cpu().numpy()
    wpred = np.zeros((n, h, w), dt)
    for i in range(n):
        c, s = cs["ic"][i], int(cs["sets"][i])
        assert oracle.r1o_dispatch_predict_intra(
            int(c["mode"]), int(c["variant"]), O.ptr(wpred[i]), w, ts, bd,
            O.ptr(cs["ac"][i]) if cs["ac"] is not None else None, int(c["angle"]), int(c["ief"]), O.ptr(eh[s]),
            int(lh[s, 0]), int(lh[s, 1]), int(c["avail_w"]), int(c["avail_h"]), int(bd > 8)) == 0
    wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    weob, wdist, wrate = np.zeros((n, nt), np.uint16), np.zeros((n, nt), np.uint64), np.zeros((n, nt), np.uint64)
    wq, wrec = np.zeros((n, nt, carea), ct), np.zeros((n, nt, h, w), dt)
    pa = org.cstruct()
    assert oracle.r1o_rdo_txsearch_batch(
        C.byref(pa), None, O.ptr(wpred), w, h, ts, O.ptr(cs["rc"]), n, mask, qi, 1, 0, 0, kind,
        O.ptr(scales) if scales is not None else None, scales.shape[1] if scales is not None else 0, xdec, ydec,
        O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wrate) if kind == 0 else None, O.ptr(wq),
        O.ptr(wrec) if kind else None) == 0
    assert np.array_equal(o["eob"].cpu().numpy().view(np.uint16), weob), (key, "eob", "oracle")
    assert np.array_equal(o["dist"].cpu().numpy().view(np.uint64), wdist), (key, "dist", "oracle")
    if full:
        assert np.array_equal(o["pred"].cpu().numpy().view(dt), wpred), (key, "pred", "oracle")
        assert np.array_equal(o["sad"].cpu().numpy().view(np.uint32), wsad), (key, "sad", "oracle")
        assert np.array_equal(o["satd"].cpu().numpy().view(np.uint32), wsatd), (key, "satd", "oracle")
        assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), (key, "qcoeffs", "oracle")
        if kind:
            assert np.array_equal(o["rec"].cpu().numpy().view(dt), wrec), (key, "rec", "oracle")
        else:
            assert np.array_equal(o["est_rate"].cpu().numpy().view(np.uint64), wrate), (key, "est_rate", "oracle")
    return weob


def _planes(bd, seed, width=204, height=140):
    """a reconstructed plane and a source plane near it; the frame is no multiple of 8, 16, 32 or 64, so the last
    block column / row of every size but 4-wide / 4-high has avail_w / avail_h below the block size"""
    rng = np.random.default_rng(seed)
    rec = O.HostPlane(width, height, bd, rng=rng)
    org = O.HostPlane(width, height, bd, rng=np.random.default_rng(seed))
    nz = rng.integers(-9, 10, org.data.shape) * (1 << (bd - 8))
    org.data[...] = np.clip(org.data.astype(np.int64) + nz, 0, (1 << bd) - 1).astype(org.data.dtype)
    return rec, org


# every (TxSize id, bit depth) with a fused point that test_gpu_depth12.py does not launch (cand_size_cases.py says
# which is which; test_cand_size_cases.py holds the table against the plan's 105 instantiations without a device)
CASES = K.INTRA_CASES


@pytest.mark.parametrize("ts,bd", CASES)
def test_intra_cand_equals_two_launch_route_and_oracle(ctx, oracle, ts, bd):
    """all 13 luma modes, angle deltas -3 .. 3, ief 0 / 1 / 2, every edge-set shape, blocks cut by the frame edge;
    n = 1, NC - 1, NC + 1, 3 NC + 1 (ragged last wave, replicated dead slots); edge_group 1 (shuffled, one set per
    candidate) and 5 (the modes of a block share a set); the three distortion kinds with a random scale grid; every
    optional output and the minimal set; guard words around every output.  The rows of K.INTRA_CASES_EOB hold a flat
    block at the origin (in every call, DC_PRED without neighbours: nothing to code) and must see zero and non-zero
    eob both"""
    w, h = TX_DIMS[ts]
    nc = 64 // max(w, h)
    rec, org = _planes(bd, 4200 + 10 * ts + bd)
    want_eob = (ts, bd) in K.INTRA_CASES_EOB
    if want_eob:
        rec.view()[:h, :w] = org.view()[:h, :w] = 128 << (bd - 8)
    drec, dorg = _dev_plane(rec), _dev_plane(org)
    rng = np.random.default_rng(977 + 31 * ts + bd)
    # (a block cut by the frame edge is evaluated whole, as the two-launch route does: the grid covers it)
    scales = rng.integers(1 << 12, 1 << 16, ((org.height + h + 7) // 8, (org.width + w + 7) // 8)).astype(np.uint32)
    dscales = _t(scales.view(np.int32))
    side = max(w, h)
    masks = [ctx.tx_type_mask(ts, False)] if side <= 16 else ([1, 0x201] if side == 32 else [1])
    if side <= 16:
        masks.append(1 << 9)          # a single type through the fan-out form
    step, eobs = 0, []
    for n0 in sorted({1, max(1, nc - 1), nc + 1, 3 * nc + 1}):
        for group in (1, 5):
            n = n0 if group == 1 else (n0 + 4) // 5 * 5
            kind = K.INTRA_KINDS[step % 3]
            full = step % 4 != 3
            mask = masks[step % len(masks)]
            qi = (40, 110, 200)[step % 3]
            cs = make_case(rng, ctx, rec, drec, ts, n, group)
            use_sc = step % 2 == 0
            eobs.append(check_call(ctx, oracle, org, dorg, ts, bd, cs, group, mask, qi, kind,
                                   scales if use_sc else None, dscales if use_sc else None, 0, 0, full,
                                   (ts, bd, n, group, kind, hex(mask), full)).ravel())
            step += 1
    assert step >= 3          # every kind of K.INTRA_KINDS was launched
    if want_eob:
        eobs = np.concatenate(eobs)
        assert (eobs == 0).any() and (eobs != 0).any(), (ts, bd, int((eobs == 0).sum()), len(eobs))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_intra_cand_cfl_on_a_420_chroma_plane(ctx, oracle, bd):
    """UV_CFL_PRED with its AC blocks (candidate i uses block i) and DC_PRED on a 4:2:0 chroma plane, 8x8: kind 0 and
    the weighted SSE with the luma scale grid at xdec = ydec = 1"""
    ts = 1
    rec, org = _planes(bd, 5100 + bd, 100, 68)
    drec, dorg = _dev_plane(rec), _dev_plane(org)
    assert bd != 12 or min(int(rec.view().max()), int(org.view().max())) > 1023   # 12-bit data, not 10
    rng = np.random.default_rng(61 + bd + (bd == 12))     # (73 draws no UV_CFL_PRED for the last call)
    scales = rng.integers(1 << 12, 1 << 16, ((2 * org.height + 23) // 8, (2 * org.width + 23) // 8)).astype(np.uint32)
    dscales = _t(scales.view(np.int32))
    for step, (n, group) in enumerate(((9, 1), (25, 5), (7, 1))):
        kind = (2, 0, 2)[step]
        cs = make_case(rng, ctx, rec, drec, ts, n, group, chroma=True)
        assert (cs["ic"]["mode"] == 13).any()
        eob = check_call(ctx, oracle, org, dorg, ts, bd, cs, group, ctx.tx_type_mask(ts, False), 90, kind, scales,
                         dscales, 1, 1, step != 2, ("cfl", bd, n, group, kind))
        assert (eob != 0).any()


def test_two_launch_route_scratch_ring_reuse_and_regrowth():
    """the two-launch route (16x16, 8-bit, dist_kind 0) keeps its R1RdoCand list and, without pred_out, its dense
    predictions in a ring of four scratch slots of the context: nine calls on ONE fresh context, enqueued back to
    back, n alternating between one edge group of 5 and forty (every second call regrows its slot, every call from
    the fifth on reuses one).  Each equals predict_intra_batch -> rdo_txsearch_batch(pred) on the same candidates."""
    import torch
    from rav1e_amd.api import Context
    ts, bd, group = 2, 8, 5
    w, h = TX_DIMS[ts]
    rec, org = _planes(bd, 8800)
    drec, dorg = _dev_plane(rec), _dev_plane(org)
    rng = np.random.default_rng(8801)
    own = Context(0)
    try:
        mask = own.tx_type_mask(ts, False)
        calls = [make_case(rng, own, rec, drec, ts, group * (1 if i % 2 == 0 else 40), group) for i in range(9)]
        got = [own.rdo_intra_cand_batch(dorg, w, h, cs["ic"], cs["pos"], cs["edges"], cs["lens"], mask, 90, 0,
                                        edge_group=group, want_est_rate=True, want_qcoeffs=True) for cs in calls]
        for i, (cs, o) in enumerate(zip(calls, got)):
            assert "pred" not in o
            dsets = torch.from_numpy(cs["sets"]).cuda()
            pred = own.predict_intra_batch(ts, cs["ic"], cs["edges"][dsets].contiguous(), cs["lens"][dsets].contiguous(), bd)
            r = own.rdo_txsearch_batch(dorg, None, w, h, cs["rc"], mask, 90, 0, is_intra=1, want_est_rate=True,
                                       want_qcoeffs=True, pred=pred)
            for k in ("eob", "dist", "est_rate", "qcoeffs"):
                assert torch.equal(o[k], r[k]), (i, k)
            assert int((o["eob"] != 0).sum()) > 0, i
    finally:
        own.close()


def test_intra_cand_rejects_bad_arguments(ctx):
    """the refusals that need a context: every one leaves without a launch"""
    from rav1e_amd.api import R1Error
    rec, org = _planes(8, 7)
    drec, dorg = _dev_plane(rec), _dev_plane(org)
    rng = np.random.default_rng(3)
    cs = make_case(rng, ctx, rec, drec, 1, 10, 5)
    a = (dorg, 8, 8, cs["ic"], cs["pos"], cs["edges"], cs["lens"])
    ctx.rdo_intra_cand_batch(*a, 0x20F, 60, 3, edge_group=5)                       # fine
    with pytest.raises(R1Error):
        ctx.rdo_intra_cand_batch(*a, 0x20F, 60, 3, edge_group=3)                   # 3 does not divide 10
    with pytest.raises(R1Error):
        ctx.rdo_intra_cand_batch(*a, 0x20F, 60, 3, edge_group=0)
    with pytest.raises(R1Error):
        ctx.rdo_intra_cand_batch(*a, 0, 60, 3, edge_group=5)                       # empty mask
    with pytest.raises(R1Error):
        ctx.rdo_intra_cand_batch(*a, 0x20F, 60, 3, edge_group=5, want_est_rate=True)   # est_rate with a pixel kind
    with pytest.raises(R1Error):
        ctx.rdo_intra_cand_batch(*a, 0x20F, 60, 0, edge_group=5, want_rec=True)    # rec with kind 0
    cfl = cs["ic"].copy()
    cfl["mode"][3] = 13
    with pytest.raises(R1Error):                                                    # UV_CFL_PRED without ac
        ctx.rdo_intra_cand_batch(dorg, 8, 8, cfl, *a[4:], 0x20F, 60, 3, edge_group=5)
    cs32 = make_case(rng, ctx, rec, drec, 3, 5, 5)
    with pytest.raises(R1Error):                                                    # ADST has no 32-point kernel
        ctx.rdo_intra_cand_batch(dorg, 32, 32, cs32["ic"], cs32["pos"], cs32["edges"], cs32["lens"], 0x3, 60, 3,
                                 edge_group=5)


def test_reference_fixture_through_the_fused_launch(ctx):
    """every case of rdo_intra_ref.npz (the reference's encode_tx_block executed with intra modes): the recorded
    neighbourhood -> r1_intra_edges_batch -> r1_rdo_intra_cand_batch with edge_group = 1.  eob, qcoeffs, rec, pred_out,
    the four pixel-domain distortions (blocks whole inside the plane: the reference measures the visible part) and
    the transform-domain distortion against the stored values; est_rate against the existing route on the device.
    Then once more with the pre-screen's shared (no-mode) edge set wherever the fixture says the sets are
    interchangeable -- and where it says they are not, the shared set must indeed predict differently."""
    import torch
    import rdo_intra_cases as RC
    cases = RC.load()
    n_shared = n_differ = 0
    for c in cases:
        w, h, key = c.w, c.h, (c.i, c.bd, c.ts, c.mode, c.angle_delta)
        drec, dorg = _dev_plane(c.rec_plane()), _dev_plane(c.org_plane())
        grid = _t(c.scale_grid().view(np.int32))
        ic = c.intra_cand()
        pos = _t(np.array([[c.x, c.y]], np.int16))
        dac = _t(c.ac.reshape(1, -1)) if c.ac is not None else None
        edges, lens = ctx.intra_edges_batch(drec, (0, 0, c.plane_w, c.plane_h), c.ts, c.edge_cand())
        lo, hi = 128 - c.left_len, 129 + c.above_len
        assert tuple(lens.cpu().numpy()[0]) == (c.left_len, c.above_len), key
        assert np.array_equal(edges.cpu().numpy().view(c.dt)[0, lo:hi].astype(np.int64), c.edge[lo:hi].astype(np.int64)), key

        def fused(kind, scaled, e=edges, l=lens, **kw):
            return ctx.rdo_intra_cand_batch(dorg, w, h, ic, pos, e, l, 1, c.qidx, kind, ac=dac,
                                            scales=grid if scaled else None, xdec=c.dec, ydec=c.dec, **kw)

        def check(o, kind, what):
            assert int(o["eob"].cpu().numpy().view(np.uint16)[0, 0]) == c.eob, (key, what, "eob")
            assert np.array_equal(o["qcoeffs"].cpu().numpy().ravel().astype(np.int64), c.qc.astype(np.int64)), (key, what, "qc")
            assert np.array_equal(o["pred"].cpu().numpy().view(c.dt)[0], c.pred), (key, what, "pred")
            if kind:
                assert np.array_equal(o["rec"].cpu().numpy().view(c.dt)[0, 0], c.rec), (key, what, "rec")
        runs = ((2, False),) if c.chroma else RC.DIST_RUNS
        for j, (kind, scaled) in enumerate(runs):
            o = fused(kind, scaled, want_qcoeffs=True, want_rec=True, want_pred=True)
            check(o, kind, (kind, scaled))
            if c.inside and not c.chroma:
                assert int(o["dist"].cpu().numpy().view(np.uint64)[0, 0]) == int(c.dist[j]), (key, "dist", j)
        o = fused(0, False, want_qcoeffs=True, want_pred=True, want_est_rate=True)
        check(o, 0, "tx")
        assert int(o["dist"].cpu().numpy().view(np.uint64)[0, 0]) == int(c.txd[0]), (key, "tx-domain distortion")
        pred = ctx.predict_intra_batch(c.ts, ic, edges, lens, c.bd, ac=dac)
        r = ctx.rdo_txsearch_batch(dorg, None, w, h, c.rdo_cand(), 1, c.qidx, 0, xdec=c.dec, ydec=c.dec, is_intra=1,
                                   want_est_rate=True, pred=pred)
        assert torch.equal(o["est_rate"], r["est_rate"]) and torch.equal(o["dist"], r["dist"]), (key, "est_rate")
        # the pre-screen's shared edge set
        es, ls = ctx.intra_edges_batch(drec, (0, 0, c.plane_w, c.plane_h), c.ts, c.edge_cand(shared=True))
        kind = 2 if c.chroma else 3
        o = fused(kind, False, es, ls, want_qcoeffs=True, want_rec=True, want_pred=True)
        if c.shared_ok:
            check(o, kind, "shared edge set")
            n_shared += 1
        else:
            assert not np.array_equal(o["pred"].cpu().numpy().view(c.dt)[0], c.pred), (key, "shared set differs")
            n_differ += 1
    assert n_shared + n_differ == len(cases) and n_differ >= 1

"""r1_coeff_rate_batch on the GPU, integer-exact: every case of tests/golden/coeff_rate_ref.npz (the reference's
write_coeffs_lv_map executed on a WriterCounter) through the C ABI, random slots against the Python model that the
fixture pins (tests/coeff_rate_model.py), the chain behind the candidate calls on one stream, snapshots left
untouched, guard bytes around every output, every refusal."""
import numpy as np
import pytest

import coeff_rate_model as M
from coeff_rate_gpu_util import GUARD, _guarded, _guards_intact, _t

pytestmark = pytest.mark.gpu

RAV1E_MASK = 0x0E0F


def _call(ctx, qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs, cb, want_cul=True):
    """host arrays in, (rate uint32 [n * nt], cul_level uint8 [n * nt] or None) out; outputs sit between guard bytes"""
    import torch
    nt = bin(mask).count("1")
    n = len(ctxs)
    dq = _t(np.asarray(qc).astype(np.int16 if cb == 2 else np.int32).reshape(n, nt, -1))
    de = _t(np.asarray(eobs).astype(np.uint16).view(np.int16).reshape(n, nt))
    raw_r, rate = _guarded((n, nt), torch.int32)
    raw_c, cul = _guarded((n, nt), torch.uint8)
    outs = {"rate": rate, "cul_level": cul} if want_cul else {"rate": rate}
    o = ctx.coeff_rate_batch(dq, de, mask, ts, plane, inter, ctxs, cdfs, use_reduced_tx_set=red, want_cul_level=want_cul,
                             outs=outs)
    torch.cuda.synchronize()
    assert _guards_intact(raw_r) and _guards_intact(raw_c)
    if not want_cul:
        assert "cul_level" not in o and bool((cul == GUARD).all())     # a NULL cul_level_out: nothing written
    return rate.cpu().numpy().view(np.uint32).ravel(), cul.cpu().numpy().ravel() if want_cul else None


def random_slots(rng, ts, types, n, cb, eob_choices=None):
    """n * nt coded-area blocks: the first eob scan positions of the slot's own scan order hold levels (small ones
    mostly, the thresholds 2 / 3 / 14 / 15 / 127 / 128 and large ones among them), the last of them non-zero"""
    W, H = M.coded_dims(ts)
    area = W * H
    big = 32767 if cb == 2 else (1 << 20) - 1
    pool = np.array([0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 9, 14, 15, 16, 127, 128, 300, big])
    prob = np.array([6, 6, 6, 6, 6, 6, 4, 4, 3, 2, 1, 1, 1, 1, 0.5, 0.5, 0.5, 0.5])
    prob = prob / prob.sum()
    qc = np.zeros((n * len(types), area), np.int64)
    eobs = np.zeros(n * len(types), np.int64)
    for s in range(n * len(types)):
        r = rng.random()
        if eob_choices is not None:
            eob = int(rng.choice(eob_choices))
        elif s < 2 and len(eobs) > 2:
            eob = (0, area)[s]               # every batch holds both ends
        else:
            eob = 0 if r < 0.08 else (area if r < 0.14 else (int(rng.integers(1, area + 1)) if r < 0.3 else
                                                             int(rng.integers(1, min(area, 24) + 1))))
        eobs[s] = eob
        if eob:
            scan = np.array(M.scan_order(ts, types[s % len(types)])[:eob])
            v = rng.choice(pool, eob, p=prob) * rng.choice([-1, 1], eob)
            if v[-1] == 0:
                v[-1] = rng.choice([-1, 1, 2, -3, 15, -big])
            qc[s, scan] = v
    return qc, eobs


def test_every_fixture_case_through_the_c_abi(ctx):
    """(a) the cases grouped into calls by (tx_size, type, plane, inter, reduced set, coefficient width); every case its
    own snapshot (cdf_sel = its index in the call)"""
    _, cases = M.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c.ts, c.tt, c.plane, c.inter, c.red, c.cb), []).append(c)
    seen = 0
    for (ts, tt, plane, inter, red, cb), cs in sorted(groups.items()):
        ctxs = np.zeros(len(cs), M.TXB_CTX_DTYPE)
        ctxs["txb_skip_ctx"] = [c.txb_skip_ctx for c in cs]
        ctxs["dc_sign_ctx"] = [c.dc_sign_ctx for c in cs]
        ctxs["y_mode"] = [c.y_mode for c in cs]
        ctxs["cdf_sel"] = np.arange(len(cs))
        cdfs = np.stack([c.cdfs for c in cs])
        rate, cul = _call(ctx, np.stack([c.qc for c in cs]), [c.eob for c in cs], 1 << tt, ts, plane, inter, red, ctxs, cdfs, cb)
        for i, c in enumerate(cs):
            assert (int(rate[i]), int(cul[i])) == (c.rate, c.cul), (c.k, ts, tt, plane, inter, red, cb, c.eob)
        seen += len(cs)
    assert seen == len(cases)


# 4x4 (one wave holds 16 coefficients), 4x16 / 16x4 (coded height != width), 8x8, 16x16 (one full chunk), 32x32 (four
# chunks), 16x64 (coded 16x32, a rectangular offset table), 64x64 (coded 32x32, eob_flag_cdf1024)
@pytest.mark.parametrize("ts", [0, 13, 14, 1, 2, 3, 17, 4])
def test_random_slots_equal_the_model(ctx, ts):
    """(b) n = 1, 63, 65, 257 (a lone slot, a ragged last workgroup either side of a multiple of 4); eobs of every kind
    mixed inside a batch, 0 and the whole area among them; n_cdfs 1 and 5 with random cdf_sel; both widths; every
    rav1e type of the largest set the size has, so all three tx classes where the size allows them"""
    rng = np.random.default_rng(7100 + ts)
    step = 0
    for n in (1, 63, 65, 257):
        inter, red, plane = ((1, 0, 0), (0, 0, 0), (1, 1, 1), (0, 1, 0))[step % 4]
        cb = (2, 4)[step % 2]
        n_cdfs = (1, 5)[(step // 2) % 2] if n > 1 else (1, 5)[ts % 2]
        mask = M.tx_type_mask(ts, inter, red) & RAV1E_MASK
        if n == 257:                         # the large batch with at most two types: the model is Python
            keep = [t for t in range(16) if (mask >> t) & 1]
            mask = sum(1 << t for t in {keep[0], keep[-1]})
        types = [t for t in range(16) if (mask >> t) & 1]
        qc, eobs = random_slots(rng, ts, types, n, cb)
        assert n == 1 or {0, qc.shape[1]} <= set(eobs.tolist())
        ctxs, cdfs = M.random_ctxs(rng, n, n_cdfs), M.random_cdfs(rng, n_cdfs, ts, inter, red)
        before = cdfs.copy()
        want_rate, want_cul = M.coeff_rate_batch(qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs)
        rate, cul = _call(ctx, qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs, cb)
        bad = np.nonzero((rate != want_rate) | (cul != want_cul))[0]
        assert len(bad) == 0, (ts, n, cb, n_cdfs, hex(mask), "first bad slot", int(bad[0]), int(eobs[bad[0]]),
                               int(rate[bad[0]]), int(want_rate[bad[0]]), int(cul[bad[0]]), int(want_cul[bad[0]]))
        assert before.tobytes() == cdfs.tobytes()
        step += 1


def _planes(bd, seed, width=204, height=140):
    import oracle_lib as O
    rng = np.random.default_rng(seed)
    ref = O.HostPlane(width, height, bd, rng=rng)
    org = O.HostPlane(width, height, bd, rng=np.random.default_rng(seed))
    nz = rng.integers(-9, 10, org.data.shape) * (1 << (bd - 8))
    org.data[...] = np.clip(org.data.astype(np.int64) + nz, 0, (1 << bd) - 1).astype(org.data.dtype)
    return ref, org


def _dev_plane(hp):
    from rav1e_amd.api import Plane
    return Plane.from_numpy(hp.data, hp.width, hp.height, hp.bit_depth, hp.xpad, hp.ypad)


def _check_chain(ctx, o, mask, ts, inter, ctxs, cdfs, lam, key):
    """o: the candidate call's outputs, still on the device and not yet waited for"""
    import torch
    from rav1e_amd import rdo_glue as RG
    r = ctx.coeff_rate_batch(o["qcoeffs"], o["eob"], mask, ts, 0, inter, ctxs, cdfs)      # same stream, no copy
    torch.cuda.synchronize()
    n, nt = r["rate"].shape
    qc = o["qcoeffs"].cpu().numpy().reshape(n * nt, -1)
    eobs = o["eob"].cpu().numpy().view(np.uint16).ravel()
    assert eobs.max() > 0, key
    want_rate, want_cul = M.coeff_rate_batch(qc, eobs, mask, ts, 0, inter, 0, ctxs, cdfs)
    rate = r["rate"].cpu().numpy().view(np.uint32)
    assert np.array_equal(rate.ravel(), want_rate), key
    assert np.array_equal(r["cul_level"].cpu().numpy().ravel(), want_cul), key
    dist = o["dist"].cpu().numpy().view(np.uint64)
    for i in range(n):
        for cur in (1e300, RG.compute_rd_cost(lam, int(rate[i, 0]), int(dist[i, 0])) * 0.99):
            got = RG.pick_tx_type(rate[i], dist[i], lam, cur)
            want = RG.pick_tx_type(want_rate.reshape(n, nt)[i], dist[i], lam, cur)
            assert got == want and (got[0] is None) == (cur < 1e300), (key, i)


@pytest.mark.parametrize("ts,bd", [(1, 8), (1, 10), (2, 8), (2, 10)])
def test_chain_behind_the_type_search_on_one_stream(ctx, ts, bd):
    """(c) r1_rdo_txsearch_batch(want_qcoeffs) -> r1_coeff_rate_batch on the same stream, nothing copied between; the
    model is fed the downloaded coefficients; pick_tx_type on both"""
    import oracle_lib as O
    w, h = M.TX_W[ts], M.TX_H[ts]
    ref, org = _planes(bd, 5300 + ts + bd)
    dref, dorg = _dev_plane(ref), _dev_plane(org)
    rng = np.random.default_rng(61 + ts + bd)
    n = 37
    c = np.zeros(n, O.RDO_CAND)
    c["ox"], c["oy"] = rng.integers(0, org.width - w, n), rng.integers(0, org.height - h, n)
    c["rx"], c["ry"] = c["ox"] + rng.integers(-3, 4, n), c["oy"] + rng.integers(-3, 4, n)
    c["col_frac"], c["row_frac"] = rng.integers(0, 16, n), rng.integers(0, 16, n)
    mask = ctx.tx_type_mask(ts, True)
    ctxs, cdfs = M.random_ctxs(rng, n, 3), M.random_cdfs(rng, 3, ts, 1, 0)
    o = ctx.rdo_txsearch_batch(dorg, dref, w, h, c, mask, 90, 2, want_qcoeffs=True)
    assert o["qcoeffs"].element_size() == (2 if bd == 8 else 4)
    _check_chain(ctx, o, mask, ts, 1, ctxs, cdfs, 0.8, (ts, bd))


def test_chain_behind_the_intra_candidate(ctx):
    """(c) one intra case: r1_intra_edges_batch -> r1_rdo_intra_cand_batch(want_qcoeffs) -> r1_coeff_rate_batch; y_mode =
    the candidate's mode"""
    import test_gpu_rdo_intra as TI
    ts, bd = 1, 8
    rec, org = TI._planes(bd, 88)
    drec, dorg = TI._dev_plane(rec), TI._dev_plane(org)
    rng = np.random.default_rng(89)
    n = 20
    cs = TI.make_case(rng, ctx, rec, drec, ts, n, 5)
    mask = ctx.tx_type_mask(ts, False)
    o = ctx.rdo_intra_cand_batch(dorg, 8, 8, cs["ic"], cs["pos"], cs["edges"], cs["lens"], mask, 70, 2, edge_group=5,
                                 want_qcoeffs=True)
    ctxs, cdfs = M.random_ctxs(rng, n, 2), M.random_cdfs(rng, 2, ts, 0, 0)
    ctxs["y_mode"] = cs["ic"]["mode"]
    assert ctxs["y_mode"].max() < 13
    _check_chain(ctx, o, mask, ts, 0, ctxs, cdfs, 1.3, "intra")


def test_snapshots_stay_untouched_and_calls_repeat(ctx):
    """(d) the same call twice, and two calls in flight on two streams, on snapshots that live on the device: equal
    results, `cdfs` byte for byte as uploaded"""
    import torch
    ts, inter, red, plane, cb, n = 2, 1, 0, 0, 2, 130
    rng = np.random.default_rng(404)
    mask = M.tx_type_mask(ts, inter, red) & RAV1E_MASK
    types = [t for t in range(16) if (mask >> t) & 1]
    qc, eobs = random_slots(rng, ts, types, n, cb)
    ctxs, cdfs = M.random_ctxs(rng, n, 5), M.random_cdfs(rng, 5, ts, inter, red)
    dq = _t(qc.astype(np.int16).reshape(n, len(types), -1))
    de = _t(eobs.astype(np.uint16).view(np.int16).reshape(n, len(types)))
    dctx = _t(ctxs.view(np.uint8).reshape(n, 4))
    dcdf = _t(cdfs.view(np.uint8).reshape(5, -1))
    call = lambda: ctx.coeff_rate_batch(dq, de, mask, ts, plane, inter, dctx, dcdf)
    first = call()
    second = call()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        third = call()
    with torch.cuda.stream(s2):
        fourth = call()
    torch.cuda.synchronize()
    want_rate, want_cul = M.coeff_rate_batch(qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs)
    for o in (first, second, third, fourth):
        assert np.array_equal(o["rate"].cpu().numpy().view(np.uint32).ravel(), want_rate)
        assert np.array_equal(o["cul_level"].cpu().numpy().ravel(), want_cul)
    assert dcdf.cpu().numpy().tobytes() == cdfs.tobytes()
    assert dctx.cpu().numpy().tobytes() == ctxs.tobytes()


def test_guards_and_the_optional_output(ctx):
    """(e) 256 guard bytes around both outputs (checked in every call of this file); without cul_level_out the rates
    are the same and nothing else is written"""
    ts, inter, red, plane, cb, n = 1, 0, 0, 0, 4, 45
    rng = np.random.default_rng(505)
    mask = M.tx_type_mask(ts, inter, red) & RAV1E_MASK
    types = [t for t in range(16) if (mask >> t) & 1]
    qc, eobs = random_slots(rng, ts, types, n, cb)
    ctxs, cdfs = M.random_ctxs(rng, n, 2), M.random_cdfs(rng, 2, ts, inter, red)
    rate, cul = _call(ctx, qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs, cb)
    rate2, none = _call(ctx, qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs, cb, want_cul=False)
    want_rate, want_cul = M.coeff_rate_batch(qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs)
    assert none is None and np.array_equal(rate, want_rate) and np.array_equal(rate2, want_rate)
    assert np.array_equal(cul, want_cul)


def test_refusals_and_invalid_slots(ctx):
    """(f) every R1_EINVAL of the header, each leaving without a launch; slots whose device-resident inputs are out
    of range, placed between valid ones, get 0xFFFFFFFF / 0 and their neighbours stay exact"""
    import torch
    from rav1e_amd.api import R1Error
    ts, inter, red, plane, cb, n = 1, 1, 0, 0, 2, 21
    rng = np.random.default_rng(606)
    mask = 0x0201
    types = [0, 9]
    qc, eobs = random_slots(rng, ts, types, n, cb, eob_choices=[1, 2, 7, 30, 64])
    ctxs, cdfs = M.random_ctxs(rng, n, 3), M.random_cdfs(rng, 3, ts, inter, red)
    dq = _t(qc.astype(np.int16).reshape(n, 2, -1))
    de = _t(eobs.astype(np.uint16).view(np.int16).reshape(n, 2))
    dctx, dcdf = _t(ctxs.view(np.uint8).reshape(n, 4)), _t(cdfs.view(np.uint8).reshape(3, -1))
    rate = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    L, R1_EINVAL = ctx.lib, -1

    def raw(h=None, q=dq.data_ptr(), cbytes=2, e=de.data_ptr(), m=mask, t=ts, p=plane, i=inter, r=red, cx=dctx.data_ptr(),
            cd=dcdf.data_ptr(), ncd=3, out=rate.data_ptr()):
        return L.r1_coeff_rate_batch(ctx.h if h is None else h, q, cbytes, e, n, m, t, p, i, r, cx, cd, ncd, out, None, None)

    assert raw() == 0
    for kw in (dict(q=None), dict(e=None), dict(cx=None), dict(cd=None), dict(out=None),          # a NULL required pointer
               dict(cbytes=1), dict(cbytes=3), dict(cbytes=8), dict(t=-1), dict(t=19),
               dict(m=0), dict(m=1 << 16), dict(m=0x80000001), dict(m=0x0203, r=1), dict(m=0x0401, r=1),   # outside the set
               dict(m=0x0203, t=3), dict(m=0x0201, t=4), dict(m=0x0201, t=3, i=0),                 # 32x32: DCT (+ IDTX inter)
               dict(ncd=0), dict(ncd=257), dict(ncd=-1), dict(p=-1), dict(p=3)):
        assert raw(**kw) == R1_EINVAL, kw
    assert L.r1_coeff_rate_batch(None, dq.data_ptr(), 2, de.data_ptr(), n, mask, ts, plane, inter, red, dctx.data_ptr(),
                                 dcdf.data_ptr(), 3, rate.data_ptr(), None, None) == R1_EINVAL
    with pytest.raises(R1Error):
        ctx.coeff_rate_batch(dq, de, 0, ts, plane, inter, dctx, dcdf)
    torch.cuda.synchronize()
    # --- invalid slots between valid ones
    area = 64
    bad_eobs, bad_ctxs = eobs.copy(), ctxs.copy()
    bad_eobs[2 * 3 + 1] = area + 1                 # candidate 3, second type only
    bad_eobs[2 * 9] = 0xFFFF
    bad_ctxs["cdf_sel"][5] = 3                     # = n_cdfs
    bad_ctxs["txb_skip_ctx"][11] = 13
    bad_ctxs["dc_sign_ctx"][12] = 3
    bad_ctxs["y_mode"][13] = 13
    bad_ctxs["cdf_sel"][20] = 255                  # the last candidate
    got_rate, got_cul = _call(ctx, qc, bad_eobs, mask, ts, plane, inter, red, bad_ctxs, cdfs, cb)
    want_rate, want_cul = M.coeff_rate_batch(qc, eobs, mask, ts, plane, inter, red, ctxs, cdfs)
    invalid = {2 * 3 + 1, 2 * 9} | {2 * i + j for i in (5, 11, 12, 13, 20) for j in (0, 1)}
    for s in range(2 * n):
        if s in invalid:
            assert (int(got_rate[s]), int(got_cul[s])) == (0xFFFFFFFF, 0), s
        else:
            assert (int(got_rate[s]), int(got_cul[s])) == (int(want_rate[s]), int(want_cul[s])), s
    # the model marks the same slots
    m_rate, m_cul = M.coeff_rate_batch(qc, bad_eobs, mask, ts, plane, inter, red, bad_ctxs, cdfs)
    assert np.array_equal(m_rate, got_rate) and np.array_equal(m_cul, got_cul)

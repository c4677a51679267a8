"""r1_coeff_rate_chain_batch on the GPU, integer-exact: every case of tests/golden/coeff_rate_chain_ref.npz (the
reference's write_coeffs_lv_map executed over a block's transform blocks on one writer) through the C ABI, random trials
against the Python model that the fixture pins (tests/coeff_rate_chain_model.py), one transform block against
r1_coeff_rate_batch, the chain behind the two launches that make the coefficients on one stream, inputs left untouched,
guard bytes around every output, bad device-resident data."""
import numpy as np
import pytest

import coeff_rate_model as M
import coeff_rate_chain_model as CM
from coeff_rate_gpu_util import GUARD, _guarded, _guards_intact, _t

pytestmark = pytest.mark.gpu

RAV1E_MASK = 0x0E0F
# (bw, bh, tx_size): the shapes of the fixture
SHAPES = [(8, 8, 0), (16, 16, 0), (64, 64, 2), (16, 4, 0), (4, 16, 0), (32, 8, 8), (16, 64, 9), (64, 64, 3), (64, 64, 4),
          (8, 8, 1)]


def _call(ctx, qc, eobs, mask, bw, bh, ts, order, inter, red, chains, cdfs, cb, side=True):
    """host arrays in (laid out as `order` says), (rate [n * nt], txb_rate [n * nt, ntx], cul [n * nt, ntx], ctx [n * nt, 32])
    out; every output sits between guard bytes; the device copies of the inputs are compared with what was uploaded"""
    import torch
    nt, n = bin(mask).count("1"), len(chains)
    gw, gh = CM.grid(bw, bh, ts)
    ntx = gw * gh
    hq = np.asarray(qc).astype(np.int16 if cb == 2 else np.int32).reshape(n * nt * ntx, -1)
    he = np.asarray(eobs).astype(np.uint16).view(np.int16).reshape(-1)
    hch = np.ascontiguousarray(chains).view(np.uint8).reshape(n, 40)
    hcd = np.ascontiguousarray(cdfs).view(np.uint8).reshape(len(cdfs), -1)
    dq, de, dch, dcd = _t(hq), _t(he), _t(hch), _t(hcd)
    raw_r, rate = _guarded((n, nt), torch.int32)
    raw_t, txb = _guarded((n, nt, ntx), torch.int32)
    raw_c, cul = _guarded((n, nt, ntx), torch.uint8)
    raw_x, cx = _guarded((n, nt, 32), torch.uint8)
    outs = {"rate": rate, "txb_rate": txb, "cul_level": cul, "ctx": cx} if side else {"rate": rate}
    o = ctx.coeff_rate_chain_batch(dq, de, mask, bw, bh, ts, order, inter, dch, dcd, use_reduced_tx_set=red,
                                   want_txb_rate=side, want_cul_level=side, want_ctx=side, outs=outs)
    torch.cuda.synchronize()
    assert all(_guards_intact(r) for r in (raw_r, raw_t, raw_c, raw_x))
    assert dq.cpu().numpy().tobytes() == hq.tobytes() and de.cpu().numpy().tobytes() == he.tobytes()
    assert dch.cpu().numpy().tobytes() == hch.tobytes() and dcd.cpu().numpy().tobytes() == hcd.tobytes()
    got_rate = rate.cpu().numpy().view(np.uint32).ravel()
    if not side:
        assert set(o) == {"rate"}
        assert all(bool((t == GUARD).all()) for t in (raw_t, raw_c, raw_x))     # a NULL optional output: nothing written
        return got_rate, None, None, None
    return (got_rate, txb.cpu().numpy().view(np.uint32).reshape(n * nt, ntx), cul.cpu().numpy().reshape(n * nt, ntx),
            cx.cpu().numpy().reshape(n * nt, 32))


def _assert_equal(got, want, key):
    for name, g, w in zip(("rate", "txb_rate", "cul_level", "ctx"), got, want):
        bad = np.nonzero((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (key, name, "first bad trial", int(bad[0]), np.asarray(g)[bad[0]].tolist(),
                               np.asarray(w)[bad[0]].tolist())


def random_trials(rng, bw, bh, ts, types, n, cb):
    """n * nt * ntx coded-area blocks in order 0: the first eob scan positions of the trial's own scan order hold levels
    (small ones mostly, the thresholds and large ones among them), the last of them non-zero; a quarter of the blocks
    have eob 0, a few the whole area"""
    W, H = M.coded_dims(ts)
    area = W * H
    gw, gh = CM.grid(bw, bh, ts)
    ntx, nt = gw * gh, len(types)
    big = 32767 if cb == 2 else (1 << 20) - 1
    pool = np.array([0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 9, 14, 15, 16, 127, 128, 300, big])
    prob = np.array([6, 6, 6, 6, 6, 6, 4, 4, 3, 2, 1, 1, 1, 1, 0.5, 0.5, 0.5, 0.5])
    prob = prob / prob.sum()
    qc = np.zeros((n * nt * ntx, area), np.int64)
    eobs = np.zeros(n * nt * ntx, np.int64)
    for s in range(n * nt * ntx):
        r = rng.random()
        eob = 0 if r < 0.25 else (area if r < 0.29 else (int(rng.integers(1, area + 1)) if r < 0.4 else
                                                         int(rng.integers(1, min(area, 20) + 1))))
        eobs[s] = eob
        if eob:
            scan = np.array(M.scan_order(ts, types[(s // ntx) % nt])[:eob])
            v = rng.choice(pool, eob, p=prob) * rng.choice([-1, 1], eob)
            if v[-1] == 0:
                v[-1] = rng.choice([-1, 1, 2, -3, 15, -big])
            qc[s, scan] = v
    return qc, eobs


def test_every_fixture_case_through_the_c_abi(ctx):
    """(a) rate, per-block rates (the differences of the recorded tell_frac values), cul_level, ctx_out of every case;
    the cases grouped into calls by everything a call fixes, every case its own snapshot (cdf_sel = its index)"""
    _, cases = CM.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c.bw, c.bh, c.ts, c.tt, c.inter, c.red, c.cb), []).append(c)
    seen = 0
    for (bw, bh, ts, tt, inter, red, cb), cs in sorted(groups.items()):
        chains = np.array([c.chain for c in cs], CM.CHAIN_DTYPE)
        chains["cdf_sel"] = np.arange(len(cs))
        cdfs = np.concatenate([c.cdfs for c in cs])
        qc = np.concatenate([c.qc for c in cs])
        eobs = np.concatenate([c.eobs for c in cs])
        rate, txb, cul, cx = _call(ctx, qc, eobs, 1 << tt, bw, bh, ts, seen % 2, inter, red, chains, cdfs, cb)   # nt = 1: both orders agree
        for i, c in enumerate(cs):
            key = (c.k, c.name)
            assert int(rate[i]) == c.rate, key
            assert txb[i].tolist() == np.diff(np.concatenate([[0], c.tell.astype(np.int64)])).tolist(), key
            assert cul[i].tolist() == c.cul.tolist() and cx[i].tolist() == c.ctx_out.tolist(), key
        seen += len(cs)
    assert seen == len(cases)


@pytest.mark.parametrize("bw,bh,ts", SHAPES)
def test_random_trials_equal_the_model(ctx, bw, bh, ts):
    """(b) n = 1, 5, 67 (a lone trial, a ragged last workgroup); n_cdfs 1 and 5 with random cdf_sel; both widths; two
    types where the set has them (the classes differ); order 0, and at n = 5 order 1 on the permuted inputs with the
    same results"""
    rng = np.random.default_rng(8200 + bw * 64 + bh + ts)
    gw, gh = CM.grid(bw, bh, ts)
    ntx = gw * gh
    for step, n in enumerate((1, 5, 67)):
        inter, red = ((1, 0), (0, 0), (1, 1))[step]
        cb = (2, 4)[(step + ts) % 2]
        n_cdfs = (1, 5, 5)[step] if ts % 2 else (5, 1, 5)[step]
        keep = CM.types_of(M.tx_type_mask(ts, inter, red) & RAV1E_MASK)
        types = sorted({keep[0], keep[-1]})
        mask = sum(1 << t for t in types)
        nt = len(types)
        qc, eobs = random_trials(rng, bw, bh, ts, types, n, cb)
        chains, cdfs = CM.random_chains(rng, n, n_cdfs, bw, bh), M.random_cdfs(rng, n_cdfs, ts, inter, red)
        want = CM.coeff_rate_chain_batch(qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs)
        got = _call(ctx, qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs, cb)
        _assert_equal(got, want, (bw, bh, ts, n, cb, n_cdfs, hex(mask), "order 0"))
        if n == 5:
            got1 = _call(ctx, CM.reorder(qc, n, nt, ntx, 1), CM.reorder(eobs, n, nt, ntx, 1), mask, bw, bh, ts, 1, inter, red,
                         chains, cdfs, cb)
            _assert_equal(got1, want, (bw, bh, ts, n, "order 1"))
            assert np.array_equal(CM.coeff_rate_chain_batch(CM.reorder(qc, n, nt, ntx, 1), CM.reorder(eobs, n, nt, ntx, 1), mask,
                                                            bw, bh, ts, 1, inter, red, chains, cdfs)[0], want[0])


@pytest.mark.parametrize("bw,bh,ts", [(8, 8, 1), (64, 64, 4), (16, 8, 8)])
def test_one_transform_block_equals_coeff_rate_batch(ctx, bw, bh, ts):
    """(c) ntx 1 against r1_coeff_rate_batch on the same device buffers, bit for bit: txb_skip_ctx 0, dc_sign_ctx from the
    descriptor's neighbours over the clipped span"""
    import torch
    from rav1e_amd import rdo_glue as RG
    rng = np.random.default_rng(8300 + ts)
    inter, red, cb, n, n_cdfs = ts == 8, 0, (2, 4)[ts % 2], 41, 3
    mask = M.tx_type_mask(ts, inter, red) & RAV1E_MASK
    types = CM.types_of(mask)
    nt = len(types)
    qc, eobs = random_trials(rng, bw, bh, ts, types, n, cb)
    chains, cdfs = CM.random_chains(rng, n, n_cdfs, bw, bh), M.random_cdfs(rng, n_cdfs, ts, inter, red)
    ctxs = np.zeros(n, M.TXB_CTX_DTYPE)
    for i, ch in enumerate(chains):
        sw, sh = min(bw >> 2, int(ch["clip_w4"])), min(bh >> 2, int(ch["clip_h4"]))
        ctxs[i] = (0, RG.txb_ctx(ch["above"][:sw], ch["left"][:sh], 0, CM.BLOCK_DIMS[(bw, bh)], ts)[1], ch["y_mode"], ch["cdf_sel"])
    dq = _t(qc.astype(np.int16 if cb == 2 else np.int32).reshape(n, nt, -1))
    de = _t(eobs.astype(np.uint16).view(np.int16).reshape(n, nt))
    dcd = _t(cdfs.view(np.uint8).reshape(n_cdfs, -1))
    a = ctx.coeff_rate_chain_batch(dq, de, mask, bw, bh, ts, 0, inter, chains, dcd)
    b = ctx.coeff_rate_batch(dq, de, mask, ts, 0, inter, ctxs, dcd)
    torch.cuda.synchronize()
    assert torch.equal(a["rate"], b["rate"]) and torch.equal(a["cul_level"].view(n, nt), b["cul_level"])
    assert torch.equal(a["txb_rate"].view(n, nt), a["rate"])
    assert len(set(a["rate"].cpu().numpy().ravel().tolist())) > n // 2       # not one value everywhere


def _check_chain(ctx, o, mask, bw, bh, ts, order, inter, chains, cdfs, key):
    """o: the outputs of the launch that made the coefficients, still on the device and not yet waited for"""
    import torch
    r = ctx.coeff_rate_chain_batch(o["qcoeffs"], o["eob"], mask, bw, bh, ts, order, inter, chains, cdfs)     # same stream, no copy
    torch.cuda.synchronize()
    n, nt = r["rate"].shape
    gw, gh = CM.grid(bw, bh, ts)
    qc = o["qcoeffs"].cpu().numpy().reshape(n * nt * gw * gh, -1)
    eobs = o["eob"].cpu().numpy().view(np.uint16).ravel()
    want = CM.coeff_rate_chain_batch(qc, eobs, mask, bw, bh, ts, order, inter, 0, chains, cdfs)
    got = (r["rate"].cpu().numpy().view(np.uint32).ravel(), r["txb_rate"].cpu().numpy().view(np.uint32).reshape(n * nt, -1),
           r["cul_level"].cpu().numpy().reshape(n * nt, -1), r["ctx"].cpu().numpy().reshape(n * nt, 32))
    _assert_equal(got, want, key)
    assert (want[0] != CM.INVALID).all() and (want[2] != 0).any(), key
    return want


@pytest.mark.parametrize("bw,ts,bd", [(16, 0, 8), (32, 1, 10)])
def test_chain_behind_the_intra_split_launch(ctx, bw, ts, bd):
    """(d) r1_rdo_intra_split_batch(want_qcoeffs) -> r1_coeff_rate_chain_batch(order 0) on one stream, nothing copied
    between; two types; blocks cut by the tile's right and bottom edges among them (their transform blocks beyond the
    edge are skipped by both launches); the model is fed the downloaded coefficients"""
    import test_gpu_rdo_intra_split as TS
    from rav1e_amd import rdo_glue as RG
    rec, org = TS._planes(bd, 900 + bd)
    drec, dorg = TS._dev_plane(rec), TS._dev_plane(org)
    rng = np.random.default_rng(910 + bd)
    n, t = 13, M.TX_W[ts]
    cands = TS.make_cands(rng, n, bw, bw, t, TS.W, TS.H)
    mask = 0x0003 if ts == 0 else 0x0201 & ctx.tx_type_mask(ts, False)
    assert bin(mask).count("1") == 2
    cdfs = M.random_cdfs(rng, 2, ts, 0, 0)
    above, left = rng.integers(0, 192, 64).tolist(), rng.integers(0, 192, 16).tolist()
    chains = np.array([RG.txb_chain_ctx(above, left, int(c["x"]) >> 2, int(c["y"]) >> 2, bw, bw, TS.W >> 2, TS.H >> 2, TS.W >> 2,
                                        TS.H >> 2, int(c["mode"]), i % 2) for i, c in enumerate(cands)], CM.CHAIN_DTYPE)
    assert (chains["mi_w"] < bw >> 2).any() and (chains["mi_h"] < bw >> 2).any()
    o = ctx.rdo_intra_split_batch(dorg, drec, (0, 0, TS.W, TS.H), bw, bw, ts, cands, mask, 60, 0, want_qcoeffs=True)
    assert o["qcoeffs"].element_size() == (2 if bd == 8 else 4)
    _check_chain(ctx, o, mask, bw, bw, ts, 0, 0, chains, cdfs, (bw, ts, bd))


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_behind_the_type_search_over_transform_blocks(ctx, bd):
    """(d) r1_rdo_txsearch_batch over the four 8x8 transform blocks of 16x16 inter blocks, block after block ->
    r1_coeff_rate_chain_batch(order 1) on the same stream"""
    import oracle_lib as O
    import test_gpu_coeff_rate as TC
    ref, org = TC._planes(bd, 5400 + bd)
    dref, dorg = TC._dev_plane(ref), TC._dev_plane(org)
    rng = np.random.default_rng(71 + bd)
    n, ts, bw = 19, 1, 16
    bx, by = rng.integers(0, (org.width - bw) // 4, n) * 4, rng.integers(0, (org.height - bw) // 4, n) * 4
    mvx, mvy = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
    c = np.zeros(n * 4, O.RDO_CAND)
    for i in range(n):
        for k in range(4):
            s = i * 4 + k
            c["ox"][s], c["oy"][s] = bx[i] + 8 * (k % 2), by[i] + 8 * (k // 2)
            c["rx"][s], c["ry"][s] = c["ox"][s] + mvx[i], c["oy"][s] + mvy[i]
    c["col_frac"], c["row_frac"] = np.repeat(rng.integers(0, 16, n), 4), np.repeat(rng.integers(0, 16, n), 4)
    mask = ctx.tx_type_mask(ts, True)
    chains, cdfs = CM.random_chains(rng, n, 3, bw, bw), M.random_cdfs(rng, 3, ts, 1, 0)
    chains["mi_w"] = chains["mi_h"] = chains["clip_w4"] = chains["clip_h4"] = 255       # every transform block was searched
    o = ctx.rdo_txsearch_batch(dorg, dref, 8, 8, c, mask, 90, 2, want_qcoeffs=True)
    _check_chain(ctx, o, mask, bw, bw, ts, 1, 1, chains, cdfs, bd)


def test_guards_untouched_inputs_and_null_outputs(ctx):
    """(e) 256 guard bytes around every output and the inputs byte for byte as uploaded (checked in every call of this
    file); without the optional outputs the rates are the same and nothing else is written; the call repeats"""
    bw, bh, ts, inter, red, cb, n = 16, 16, 1, 1, 0, 4, 23
    rng = np.random.default_rng(8500)
    mask = 0x0E01
    qc, eobs = random_trials(rng, bw, bh, ts, CM.types_of(mask), n, cb)
    chains, cdfs = CM.random_chains(rng, n, 2, bw, bh), M.random_cdfs(rng, 2, ts, inter, red)
    want = CM.coeff_rate_chain_batch(qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs)
    got = _call(ctx, qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs, cb)
    _assert_equal(got, want, "all outputs")
    rate2 = _call(ctx, qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs, cb, side=False)[0]
    assert np.array_equal(rate2, want[0])
    _assert_equal(_call(ctx, qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs, cb), want, "repeated")


def test_bad_device_data_marks_its_trial_only(ctx):
    """(f) each kind of bad device-resident data in one transform block of one trial (an eob above the coded area) or in
    one block's descriptor gives 0xFFFFFFFF and zero side outputs there only; the neighbours in the batch are exact"""
    bw, bh, ts, inter, red, cb, n = 16, 16, 1, 1, 0, 2, 14
    rng = np.random.default_rng(8600)
    mask, nt, ntx, area = 0x0201, 2, 4, 64
    qc, eobs = random_trials(rng, bw, bh, ts, [0, 9], n, cb)
    chains, cdfs = CM.random_chains(rng, n, 3, bw, bh), M.random_cdfs(rng, 3, ts, inter, red)
    chains["mi_w"][3] = chains["clip_w4"][3] = 255
    chains["mi_h"][3] = chains["clip_h4"][3] = 255
    chains["mi_w"][8], chains["clip_w4"][8] = 2, 2              # block 8: the right column is not coded
    want = CM.coeff_rate_chain_batch(qc, eobs, mask, bw, bh, ts, 0, inter, red, chains, cdfs)
    bad_eobs, bad = eobs.copy(), chains.copy()
    bad_eobs[(3 * nt + 1) * ntx + 2] = area + 1                 # block 3, second type only, third transform block
    bad_eobs[(6 * nt + 0) * ntx + 0] = 0xFFFF                   # block 6, first type (coded: mi_w, mi_h >= 1)
    bad_eobs[(8 * nt + 0) * ntx + 1] = 0xFFFF                   # block 8: a transform block that is not coded is not looked at
    bad["y_mode"][1] = 13
    bad["cdf_sel"][5] = 3                                       # = n_cdfs
    bad["mi_w"][10], bad["clip_w4"][10] = 3, 2                  # mi_w > clip_w4
    bad["mi_h"][11], bad["clip_h4"][11] = 255, 254              # mi_h > clip_h4
    bad["cdf_sel"][13] = 255                                    # the last block
    invalid = {3 * nt + 1, 6 * nt} | {i * nt + j for i in (1, 5, 10, 11, 13) for j in (0, 1)}
    got = _call(ctx, qc, bad_eobs, mask, bw, bh, ts, 0, inter, red, bad, cdfs, cb)
    for s in range(n * nt):
        if s in invalid:
            assert int(got[0][s]) == 0xFFFFFFFF and not got[1][s].any() and not got[2][s].any() and not got[3][s].any(), s
        else:
            assert all(np.array_equal(got[k][s], want[k][s]) for k in range(4)), s
    # the model marks the same trials
    _assert_equal(CM.coeff_rate_chain_batch(qc, bad_eobs, mask, bw, bh, ts, 0, inter, red, bad, cdfs), got, "model")
    rate_only = _call(ctx, qc, bad_eobs, mask, bw, bh, ts, 0, inter, red, bad, cdfs, cb, side=False)[0]
    assert np.array_equal(rate_only, got[0])

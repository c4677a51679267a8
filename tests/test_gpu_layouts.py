"""Every plane-taking and stride-taking entry point at layouts the ABI admits and no other GPU module produces
(tests/layout_util.py): "odd" planes -- odd stride, odd xorigin, the base one element past a 256-byte boundary --
and "tight" ones, a different kind for every plane of a call, and arrays whose row stride is not their width,
with poison in the gap.  The oracle runs on the same host layout (tests/test_oracle_layouts.py shows that it does
not care); values are compared bit for bit, a written plane over its WHOLE allocation, and the 256 guard bytes
around every device plane must survive."""
import ctypes as C

import numpy as np
import pytest

import layout_util as LU
import oracle_lib as O
from test_gpu_parity import rand_dist_cands, rand_mc_cands, rand_rdo_cands

pytestmark = pytest.mark.gpu

W, H = 96, 64
SWAP = [("odd", "tight"), ("tight", "odd")]
MC_PAD = 12          # candidates reach 8 px into the padding, the 8-tap window 3 / 4 px beyond the block


def _t(a):
    import torch
    return torch.from_numpy(LU._torch_view(np.ascontiguousarray(a))).cuda()


def _n(t, dtype):
    """device tensor -> numpy in the oracle's (unsigned) type"""
    return t.cpu().numpy().view(dtype)


def _pdt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _base(bd, seed, n=2, w=W, h=H):
    rng = np.random.default_rng(seed)
    return [O.HostPlane(w, h, bd, 16, 16, rng=rng) for _ in range(n)]


def _near(hp, seed, amp):
    """a plane close to hp (small residuals), noise padding"""
    rng = np.random.default_rng(seed)
    q = LU.lay(hp, None, 0, 0)
    q.data[...] = np.clip(hp.data.astype(np.int64) + rng.integers(-amp, amp + 1, hp.data.shape), 0,
                          (1 << hp.bit_depth) - 1).astype(hp.data.dtype)
    return q


def _scales(rng, extra=3):
    """a DistortionScale grid of the W x H plane, row stride cols + extra, 1 << 20 in the gap"""
    g = rng.integers(1 << 12, 1 << 16, ((H + 7) // 8, (W + 7) // 8)).astype(np.uint32)
    return LU.strided(g, extra, 1 << 20)


# ------------------------------------------------------------------ SAD / SATD, scaled distortions
@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_dist(ctx, oracle, bd, kinds):
    a, b = _base(bd, 10 + bd)
    a, b = LU.lay(a, kinds[0], 0, 0), LU.lay(b, kinds[1], 8, 8)
    da, db = LU.dev(a), LU.dev(b)
    rng = np.random.default_rng(20 + bd)
    hs, ds = _scales(rng)
    for (w, h) in ((8, 8), (64, 64)):
        c = rand_dist_cands(rng, 67, W, H, w, h, 8)
        for kind in (0, 1):
            got = _n(ctx.dist_batch(kind, da, db, w, h, c), np.uint32)
            assert np.array_equal(got, LU.o_dist(oracle, kind, a, b, w, h, c)), (bd, w, h, kind)
        c["ox"] &= ~7          # the scaled kinds work on the 8x8 importance grid
        c["oy"] &= ~7
        for kind in (2, 3):
            got = _n(ctx.dist_scaled_batch(kind, da, db, w, h, c, scales=ds), np.uint64)
            assert np.array_equal(got, LU.o_dist_scaled(oracle, kind, a, b, w, h, c, hs)), (bd, w, h, kind)
    assert LU.guards_intact(da, db)


# ------------------------------------------------------------------ put / prep / avg, the matrix-core variant
@pytest.mark.parametrize("kind", LU.KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_mc(ctx, oracle, bd, kind):
    """the window starts at rx - 3: an odd byte address in either layout for some candidates, in "odd" also for
    16-bit pixels an address that is no multiple of 4"""
    a = LU.lay(_base(bd, 30 + bd)[0], kind, MC_PAD, MC_PAD)
    da = LU.dev(a)
    rng = np.random.default_rng(40 + bd)
    for (w, h) in ((4, 4), (8, 8), (64, 64)):
        c = rand_mc_cands(rng, 41, W, H, w, h, 8)
        assert len({(bool(x), bool(y)) for x, y in zip(c["col_frac"], c["row_frac"])}) == 4
        put, prep = LU.o_mc(oracle, a, w, h, c)
        got_prep = ctx.prep_8tap_batch(da, w, h, c)
        assert np.array_equal(_n(ctx.put_8tap_batch(da, w, h, c), _pdt(bd)), put), (bd, w, "put")
        assert np.array_equal(got_prep.cpu().numpy(), prep), (bd, w, "prep")
        want_avg = np.zeros((41, h, w), _pdt(bd))
        oracle.r1o_mc_avg_batch(O.ptr(prep), O.ptr(np.ascontiguousarray(prep[::-1])), w, h, 41, bd, a.bpp,
                                O.ptr(want_avg))
        got = ctx.mc_avg_batch(got_prep, got_prep.flip(0).contiguous(), w, h, bd)
        assert np.array_equal(_n(got, _pdt(bd)), want_avg), (bd, w, "avg")
        if bd == 8 and w >= 8:
            assert np.array_equal(ctx.mc_batch_mfma(da, w, h, c).cpu().numpy(), put), (w, "mfma put")
            assert np.array_equal(ctx.mc_batch_mfma(da, w, h, c, prep=True).cpu().numpy(), prep), (w, "mfma prep")
    assert LU.guards_intact(da)


# ------------------------------------------------------------------ the fused candidates
FUSED = [(1, 8, 8), (2, 16, 16), (3, 32, 32), (4, 64, 64)]      # one size per staging mapping of WindowStage


def _fused_planes(bd, kinds, seed):
    a, b = _base(bd, seed)
    near = _near(a, seed + 1, 4)
    return LU.lay(a, kinds[0], 0, 0), LU.lay(b, kinds[1], MC_PAD, MC_PAD), LU.lay(near, kinds[1], MC_PAD, MC_PAD)


@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rdo_cand_and_full_cand(ctx, oracle, bd, kinds):
    a, b, near = _fused_planes(bd, kinds, 50 + bd)
    da, db, dn = LU.dev(a), LU.dev(b), LU.dev(near)
    rng = np.random.default_rng(60 + bd)
    ct = np.int16 if bd == 8 else np.int32
    for ts, w, h in FUSED:
        n = 45 if w * h <= 1024 else 11
        c = rand_rdo_cands(rng, n, W, H, w, h, 8, ts)
        pa, pb = a.cstruct(), b.cstruct()
        wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        wco, wpred = np.zeros((n, w * h), ct), np.zeros((n, h, w), _pdt(bd))
        assert oracle.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, O.ptr(wsad), O.ptr(wsatd),
                                         O.ptr(wco), O.ptr(wpred)) == 0
        o = ctx.rdo_cand_batch(da, db, w, h, c, want_pred=True)
        assert np.array_equal(_n(o["pred"], _pdt(bd)), wpred), (bd, w, "pred")
        assert np.array_equal(_n(o["sad"], np.uint32), wsad), (bd, w, "sad")
        assert np.array_equal(_n(o["satd"], np.uint32), wsatd), (bd, w, "satd")
        assert np.array_equal(o["coeffs"].cpu().numpy(), wco), (bd, w, "coeffs")
        carea = min(w, 32) * min(h, 32)
        for hp, dp, qi in ((b, db, 35), (near, dn, 110)):
            c2 = c.copy()
            if hp is near:
                c2["rx"], c2["ry"] = c2["ox"], c2["oy"]
            pb = hp.cstruct()
            weob, wdist, wrate = np.zeros(n, np.uint16), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            wq = np.zeros((n, carea), ct)
            assert oracle.r1o_rdo_full_cand_batch(C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c2), n, qi, 0, 0, 0,
                                                  O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wrate),
                                                  O.ptr(wq)) == 0
            o = ctx.rdo_full_cand_batch(da, dp, w, h, c2, qi, want_qcoeffs=True)
            key = (bd, w, qi)
            assert np.array_equal(_n(o["sad"], np.uint32), wsad), key
            assert np.array_equal(_n(o["satd"], np.uint32), wsatd), key
            assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
            assert np.array_equal(_n(o["eob"], np.uint16), weob), key
            assert np.array_equal(_n(o["tx_dist"], np.uint64), wdist), key
            assert np.array_equal(_n(o["est_rate"], np.uint64), wrate), key
    assert LU.guards_intact(da, db, dn)


@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rdo_pixel_pred_and_txsearch(ctx, oracle, bd, kinds):
    """r1_rdo_pixel_cand_batch, r1_rdo_pred_cand_batch and r1_rdo_txsearch_batch (from the reference plane and from
    a dense prediction), the scale grid strided"""
    a, b, near = _fused_planes(bd, kinds, 70 + bd)
    da, db, dn = LU.dev(a), LU.dev(b), LU.dev(near)
    rng = np.random.default_rng(80 + bd)
    ct, dt = (np.int16 if bd == 8 else np.int32), _pdt(bd)
    hs, ds = _scales(rng)
    for ts, w, h in FUSED:
        carea = min(w, 32) * min(h, 32)
        n = 45 if w * h <= 1024 else 11
        for hp, dp, qi, kind in ((b, db, 60, 3), (near, dn, 140, 2)):
            c = rand_rdo_cands(rng, n, W, H, w, h, 8, ts)
            if hp is near:
                c["rx"], c["ry"] = c["ox"], c["oy"]
            pa, pb = a.cstruct(), hp.cstruct()
            wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            weob, wdist = np.zeros(n, np.uint16), np.zeros(n, np.uint64)
            wq, wrec = np.zeros((n, carea), ct), np.zeros((n, h, w), dt)
            assert oracle.r1o_rdo_pixel_cand_batch(
                C.byref(pa), C.byref(pb), w, h, ts, O.ptr(c), n, qi, 0, 0, 0, kind, hs.ctypes.data, LU.row_stride(hs),
                0, 0, O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wq), O.ptr(wrec), None) == 0
            o = ctx.rdo_pixel_cand_batch(da, dp, w, h, c, qi, kind, scales=ds, want_qcoeffs=True, want_rec=True)
            key = (bd, w, qi, kind)
            assert np.array_equal(_n(o["sad"], np.uint32), wsad), key
            assert np.array_equal(_n(o["satd"], np.uint32), wsatd), key
            assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
            assert np.array_equal(_n(o["eob"], np.uint16), weob), key
            assert np.array_equal(_n(o["rec"], dt), wrec), key
            assert np.array_equal(_n(o["dist"], np.uint64), wdist), key
            # the same chain from a dense prediction: the oracle's own reconstruction of the other reference
            pred = wrec.copy()
            assert oracle.r1o_rdo_pixel_cand_batch(
                C.byref(pa), None, w, h, ts, O.ptr(c), n, qi, 1, 0, 0, kind, hs.ctypes.data, LU.row_stride(hs), 0, 0,
                O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), O.ptr(wq), O.ptr(wrec), O.ptr(pred)) == 0
            o = ctx.rdo_pixel_cand_batch(da, None, w, h, c, qi, kind, scales=ds, is_intra=1, want_qcoeffs=True,
                                         want_rec=True, pred=_t(pred))
            key = (bd, w, qi, kind, "pred")
            assert np.array_equal(_n(o["satd"], np.uint32), wsatd), key
            assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
            assert np.array_equal(_n(o["rec"], dt), wrec), key
            assert np.array_equal(_n(o["dist"], np.uint64), wdist), key
            # the transform-type fan-out on the same candidates
            mask = ctx.tx_type_mask(ts, not (hp is b))
            nt = bin(mask).count("1")
            c["tx_type"] = 0
            weob, wdist = np.zeros((n, nt), np.uint16), np.zeros((n, nt), np.uint64)
            wq, wrec = np.zeros((n, nt, carea), ct), np.zeros((n, nt, h, w), dt)
            for ref, prd in ((hp, None), (None, pred)):
                pb = ref.cstruct() if ref is not None else None
                assert oracle.r1o_rdo_txsearch_batch(
                    C.byref(pa), C.byref(pb) if pb is not None else None, O.ptr(prd), w, h, ts, O.ptr(c), n, mask, qi,
                    int(ref is None), 0, 0, kind, hs.ctypes.data, LU.row_stride(hs), 0, 0, O.ptr(wsad), O.ptr(wsatd),
                    O.ptr(weob), O.ptr(wdist), None, O.ptr(wq), O.ptr(wrec)) == 0
                o = ctx.rdo_txsearch_batch(da, dp if ref is not None else None, w, h, c, mask, qi, kind, scales=ds,
                                           is_intra=int(ref is None), want_sad=True, want_satd=True,
                                           want_qcoeffs=True, want_rec=True, pred=_t(prd) if prd is not None else None)
                key = (bd, w, qi, kind, hex(mask), ref is None)
                assert np.array_equal(_n(o["sad"], np.uint32), wsad), key
                assert np.array_equal(_n(o["satd"], np.uint32), wsatd), key
                assert np.array_equal(_n(o["eob"], np.uint16), weob), key
                assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
                assert np.array_equal(_n(o["rec"], dt), wrec), key
                assert np.array_equal(_n(o["dist"], np.uint64), wdist), key
    assert LU.guards_intact(da, db, dn)


@pytest.mark.parametrize("kinds", [("odd", "tight", "odd"), ("tight", "odd", "tight"), ("odd", "odd", "tight")])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rdo_compound_cand(ctx, oracle, bd, kinds):
    """the source and the two references each in a layout of their own"""
    from rav1e_amd.api import COMPOUND_CAND
    from test_gpu_compound import oracle_compound
    a, r0, r1 = _base(bd, 90 + bd, 3)
    a, r0, r1 = LU.lay(a, kinds[0], 0, 0), LU.lay(r0, kinds[1], MC_PAD, MC_PAD), LU.lay(r1, kinds[2], MC_PAD, MC_PAD)
    da, d0, d1 = LU.dev(a), LU.dev(r0), LU.dev(r1)
    rng = np.random.default_rng(95 + bd)
    for (w, h) in ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64)):
        n = 45 if w * h <= 1024 else 11
        c = np.zeros(n, COMPOUND_CAND)
        c["ox"], c["oy"] = rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)
        for f, lim in (("rx0", W - w), ("rx1", W - w), ("ry0", H - h), ("ry1", H - h)):
            c[f] = rng.integers(-8, lim + 9, n)
        for f in ("col_frac0", "row_frac0", "col_frac1", "row_frac1"):
            c[f] = rng.integers(0, 16, n)
        c["col_frac0"][:n // 4] = 0
        c["row_frac1"][n // 8:n // 4 + n // 8] = 0
        c["mode_x"], c["mode_y"] = rng.integers(0, 4, n), rng.integers(0, 4, n)
        pred, sad, satd = oracle_compound(oracle, a, r0, r1, w, h, c)
        o = ctx.rdo_compound_cand_batch(da, d0, d1, w, h, c, want_sad=True, want_satd=True, want_pred=True)
        assert np.array_equal(_n(o["pred"], _pdt(bd)), pred), (bd, w, kinds, "pred")
        assert np.array_equal(_n(o["sad"], np.uint32), sad), (bd, w, kinds, "sad")
        assert np.array_equal(_n(o["satd"], np.uint32), satd), (bd, w, kinds, "satd")
    assert LU.guards_intact(da, d0, d1)


# ------------------------------------------------------------------ plane_pad / plane_downsample
@pytest.mark.parametrize("kinds", [("odd", "tight"), ("tight", "odd"), (None, None)])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,fw,fh", [(71, 37, 71, 37), (200, 9, 200, 9), (72, 37, 71, 37)])
def test_plane_pad_and_downsample(ctx, oracle, w, h, fw, fh, bd, kinds):
    """both kinds fail aligned16() (csrc/plane_ops.hip) at either depth: k_plane_pad<BPP, false> and
    k_plane_downsample<BPP, false>.  The (None, None) rows are the HostPlane layout, the vector forms: at width 72
    with a 71-pixel frame the last 16-byte chunk of the visible row straddles the padded-from edge, the boundary
    between the vector branch and the per-pixel tail"""
    rng = np.random.default_rng(w + bd)
    full = LU.lay(O.HostPlane(w, h, bd, 16, 16, rng=rng), kinds[0], 16, 16)
    half = LU.lay(O.HostPlane((w + 1) // 2, (h + 1) // 2, bd, 8, 8, rng=rng), kinds[1], 8, 8)
    dfull, dhalf = LU.dev(full), LU.dev(half)
    LU.o_pad(oracle, full, fw, fh)
    ctx.plane_pad(dfull, fw, fh)
    assert np.array_equal(dfull.host(), full.data), (w, bd, kinds, "pad")
    LU.o_downsample(oracle, full, half, fw, fh, 1)
    a, b = dfull.cstruct(), dhalf.cstruct()
    assert ctx.lib.r1_plane_downsample(ctx.h, C.byref(a), C.byref(b), fw, fh, 1, 1, None) == 0
    assert np.array_equal(dhalf.host(), half.data), (w, bd, kinds, "downsample")
    assert np.array_equal(dfull.host(), full.data)          # the source is read only
    assert LU.guards_intact(dfull, dhalf)


# ------------------------------------------------------------------ CDEF
CDEF_KINDS = [(("odd", "tight", "odd"), ("tight", "odd", "tight")), (("tight", "odd", "tight"), ("odd", "tight", "odd"))]


def _cdef_dev_arrays(skip, ci, odd_ptr=False):
    """device views of the (strided) skip grid and index grid; odd_ptr: the skip grid's first byte at an odd address"""
    import torch
    dci = _t(ci.base)[:, :ci.shape[1]]
    flat = torch.from_numpy(np.concatenate([[LU.GUARD_BYTE] * int(odd_ptr), skip.base.reshape(-1)]).astype(np.uint8)).cuda()
    dskip = flat[int(odd_ptr):].view(skip.base.shape)[:, :skip.shape[1]]
    assert dskip.data_ptr() % 2 == int(odd_ptr) and dskip.stride(0) == LU.row_stride(skip)
    return dskip, dci


@pytest.mark.parametrize("odd_ptr", [False, True])
@pytest.mark.parametrize("kinds", CDEF_KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_filter_frame(ctx, oracle, bd, kinds, odd_ptr):
    """r1_cdef_filter_frame_plane and the analyse-then-filter pair, mi_stride = mi_cols + 3 (odd: every second skip
    row starts at an odd address, which the two-flags-in-one-load of k_cdef_frame must survive), sb_stride = n_sbx + 1;
    the output planes hold noise first, and all of it that CDEF does not write must still be there"""
    case = LU.cdef_case(bd)
    src, dst, skip, ci = LU.cdef_filter_planes(case, kinds[0], kinds[1], True)
    want = LU.cdef_filter_oracle(oracle, case, kinds[0], kinds[1], True)
    dsrc = [LU.dev(p) for p in src]
    dskip, dci = _cdef_dev_arrays(skip, ci, odd_ptr)
    w, h = case["w"], case["h"]
    da, va = ctx.cdef_analyze_frame(dsrc[0], w, h, skip.shape[1], skip.shape[0])
    for two_step in (False, True):
        ddst = [LU.dev(p) for p in dst]
        for p in range(3):
            xd = yd = 0 if p == 0 else 1
            if two_step:
                ctx.cdef_filter_frame_plane_dirs(da, va, dsrc[p], ddst[p], p, xd, yd, w, h, dskip, dci, case["ystr"],
                                                 case["uvstr"], case["damping"], bd)
            else:
                ctx.cdef_filter_frame_plane(dsrc[0], dsrc[p], ddst[p], p, xd, yd, w, h, dskip, dci, case["ystr"],
                                            case["uvstr"], case["damping"], bd)
            bad = np.argwhere(ddst[p].host() != want[p].data)
            assert len(bad) == 0, (bd, kinds, p, two_step, bad[:4])
        assert LU.guards_intact(*ddst)
    assert LU.guards_intact(*dsrc)
    assert any((LU.window(want[p]) != LU.window(src[p])).any() for p in range(3))


@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_find_dir_and_filter_block(ctx, oracle, bd, kinds):
    from rav1e_amd.api import CDEF_BLOCK_CAND, CDEF_DIR_CAND
    case = LU.cdef_case(bd)
    w, h = case["w"], case["h"]
    src = LU.lay(case["rec"][0], kinds[0], LU.CDEF_PAD, LU.CDEF_PAD)
    dsrc = LU.dev(src)
    nbx, nby = w // 8, h // 8
    dc = np.zeros(nbx * nby, CDEF_DIR_CAND)
    dc["x"], dc["y"] = np.tile(np.arange(nbx) * 8, nby), np.repeat(np.arange(nby) * 8, nbx)
    d, v = ctx.cdef_find_dir_batch(dsrc, dc)
    for i in range(len(dc)):
        var = C.c_uint32()
        wd = oracle.r1o_cdef_find_dir(src.block_ptr(int(dc["x"][i]), int(dc["y"][i])), src.stride, C.byref(var),
                                      bd - 8, int(bd > 8))
        assert (int(d[i]), int(v[i])) == (wd, var.value), (bd, kinds, i)
    rng = np.random.default_rng(7 + bd)
    for (xdec, ydec) in ((0, 0), (1, 1)):
        xs, ys = 8 >> xdec, 8 >> ydec
        gx, gy = w // xs - 2, h // ys - 2
        n = min(200, gx * gy)
        c = np.zeros(n, CDEF_BLOCK_CAND)
        pos = rng.permutation(gx * gy)[:n]
        c["x"], c["y"] = (pos % gx + 1) * xs, (pos // gx + 1) * ys
        c["pri_strength"] = rng.integers(0, 16, n) << (bd - 8)
        c["sec_strength"] = rng.choice([0, 1, 2, 4], n) << (bd - 8)
        c["dir"], c["damping"], c["edges"] = rng.integers(0, 8, n), rng.integers(3, 7, n) + (bd - 8), np.arange(n) % 16
        out = LU.lay(case["dst"][0], kinds[1], LU.CDEF_PAD, LU.CDEF_PAD)
        dout = LU.dev(out)
        ctx.cdef_filter_block_batch(dsrc, dout, xdec, ydec, c)
        for i in range(n):
            x, y = int(c["x"][i]), int(c["y"][i])
            oracle.r1o_cdef_filter_block(out.block_ptr(x, y), out.stride, src.block_ptr(x, y), src.stride,
                                         int(c["pri_strength"][i]), int(c["sec_strength"][i]), int(c["dir"][i]),
                                         int(c["damping"][i]), bd, xdec, ydec, int(c["edges"][i]), int(bd > 8))
        assert np.array_equal(dout.host(), out.data), (bd, kinds, xdec)
        assert LU.guards_intact(dout)
    assert LU.guards_intact(dsrc)


@pytest.mark.parametrize("kinds", CDEF_KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_strength_search_and_apply_area(ctx, oracle, bd, kinds):
    """r1_cdef_strength_search with mi_stride and scale_stride strided, then r1_cdef_apply_area of the picked indices
    into working copies that hold noise, compared over the whole allocation"""
    from rav1e_amd.api import TRIAL_UNIT
    case = LU.cdef_case(bd)
    prm = LU.cdef_search_params(case)
    P = LU.CDEF_PAD
    rec = [LU.lay(p, k, P, P) for p, k in zip(case["rec"], kinds[0])]
    src = [LU.lay(p, k, P, P) for p, k in zip(case["src"], kinds[1])]
    skip = LU.host_strided(case["skip"], 3, LU.flip_poison(case["skip"]))
    dskip, _ = _cdef_dev_arrays(skip, LU.host_strided(case["ci"], 1, 0))
    hs, ds = LU.strided(case["scales"], 3, 1 << 20)
    want_err, want_best = LU.o_cdef_search(oracle, rec, src, skip, hs, prm)
    drec, dsrc = [LU.dev(p) for p in rec], [LU.dev(p) for p in src]
    args = (list(prm.y_strengths), list(prm.uv_strengths), prm.damping, bd, prm.n_idx, 1, 1, prm.crop_w, prm.crop_h)
    err, best = ctx.cdef_strength_search(drec, dsrc, dskip, *args, area_sb=(prm.area_sb_w, prm.area_sb_h), scales=ds,
                                         dist_scale=list(prm.dist_scale))
    bad = np.argwhere(_n(err, np.uint64) != want_err)
    assert len(bad) == 0, (bd, kinds, bad[:4])
    assert np.array_equal(best.cpu().numpy(), want_best)
    assert (want_best == -1).any() and (want_best >= 0).any()
    # the later-pass entry point with no restoration unit returns the same numbers
    no_units = [np.zeros(0, TRIAL_UNIT)] * 3
    err2, _, best2 = ctx.cdef_lrf_trial_batch(drec, None, dsrc, dskip, no_units, *args,
                                              area_sb=(prm.area_sb_w, prm.area_sb_h), scales=ds,
                                              dist_scale=list(prm.dist_scale))
    assert np.array_equal(_n(err2, np.uint64), want_err) and np.array_equal(best2.cpu().numpy(), want_best)
    # the working copy, with an index map of its own (an index >= 0 on every superblock, -1 on one)
    import loop_decision_util as U
    U.sigs(oracle)
    idx = np.array([[3, -1, 5], [0, 7, 2]], np.int8)
    out = [LU.lay(p, k, P, P) for p, k in zip(case["dst"], kinds[1])]
    dout = [LU.dev(p) for p in out]
    ctx.cdef_apply_area(drec, dout, dskip, _t(idx), *args, area_sb=(prm.area_sb_w, prm.area_sb_h))
    assert oracle.r1o_cdef_apply_area(LU.planes3(rec), LU.planes3(out), skip.ctypes.data, LU.row_stride(skip),
                                      skip.shape[1], skip.shape[0], C.byref(prm), idx.ctypes.data) == 0
    for p in range(3):
        bad = np.argwhere(dout[p].host() != out[p].data)
        assert len(bad) == 0, (bd, kinds, p, bad[:4])
        assert (LU.window(out[p]) != LU.window(rec[p])).any()
    # trials on superblocks RESTORED with a self-guided choice; the second superblock of the first area (EDGE_LEFT)
    # reads the working copy just made, which lies in the layouts of kinds[1]
    units = [np.array([(0, 0, 64, 64, 3, 0, (10, -20), 0), (64, 0, 64, 64, 11, 1, (-40, 60), 1),
                       (0, 64, 64, 8, 14, 0, (-90, 20), 3)], TRIAL_UNIT),
             np.array([(32, 0, 32, 32, 5, 1, (20, 30), 1)], TRIAL_UNIT), np.zeros(0, TRIAL_UNIT)]
    n_sby, n_sbx = want_best.shape
    werr, werrp = np.zeros((n_sby, n_sbx, 8), np.uint64), np.zeros((n_sby, n_sbx, 8, 3), np.uint64)
    wbest = np.zeros((n_sby, n_sbx), np.int8)
    allu = np.concatenate(units)
    assert oracle.r1o_cdef_lrf_trial(LU.planes3(rec), LU.planes3(out), LU.planes3(src), skip.ctypes.data,
                                     LU.row_stride(skip), skip.shape[1], skip.shape[0], hs.ctypes.data,
                                     LU.row_stride(hs), C.byref(prm), allu.ctypes.data,
                                     (C.c_int32 * 3)(*[len(u) for u in units]), None, werr.ctypes.data,
                                     werrp.ctypes.data, wbest.ctypes.data) == 0
    err3, errp3, best3 = ctx.cdef_lrf_trial_batch(drec, dout, dsrc, dskip, units, *args,
                                                  area_sb=(prm.area_sb_w, prm.area_sb_h), scales=ds,
                                                  dist_scale=list(prm.dist_scale))
    assert np.array_equal(_n(errp3, np.uint64), werrp), (bd, kinds, np.argwhere(_n(errp3, np.uint64) != werrp)[:4])
    assert np.array_equal(_n(err3, np.uint64), werr) and np.array_equal(best3.cpu().numpy(), wbest)
    assert (werr != want_err).any()                        # the restoration changed what the trials measure
    for p in range(3):
        assert np.array_equal(dout[p].host(), out[p].data)          # the working copy is as it was
    assert LU.guards_intact(*drec, *dsrc, *dout)


# ------------------------------------------------------------------ deblocking
@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10])
def test_deblock(ctx, oracle, bd, kinds):
    """the four entry points with blocks_stride = blocks_cols + 2 (every edge set in the gap records), rec and src in
    different layouts, the three planes of the frame calls alternating; the filter runs in place, so the whole
    allocation is compared"""
    case = LU.deblock_case(bd)
    P, cw, ch, state = LU.DEBLOCK_PAD, case["cw"], case["ch"], case["state"]
    hb, db = LU.strided(case["blocks"], 2, 0xFF)
    k3 = (kinds[0], kinds[1], kinds[0])
    rec = [LU.lay(r, k, P, P) for (r, _), k in zip(case["planes"], k3)]
    src = [LU.lay(s, k, P, P) for (_, s), k in zip(case["planes"], (kinds[1], kinds[0], kinds[1]))]
    want_t = np.stack([LU.o_deblock_sse(oracle, rec[p], src[p], p, int(p > 0), int(p > 0), hb, cw, ch, bd)
                       for p in range(3)])
    dsrc = [LU.dev(p) for p in src]
    # plane by plane
    drec = [LU.dev(p) for p in rec]
    for p in range(3):
        xd = yd = int(p > 0)
        t = ctx.deblock_sse_plane(drec[p], dsrc[p], p, xd, yd, db, cw, ch)
        assert np.array_equal(t.cpu().numpy(), want_t[p]), (bd, kinds, p)
    got_t = ctx.deblock_sse_frame(drec, dsrc, 1, 1, db, cw, ch)
    assert np.array_equal(got_t.cpu().numpy(), want_t), (bd, kinds)
    for p in range(3):
        LU.o_deblock(oracle, state, rec[p], p, int(p > 0), int(p > 0), hb, cw, ch, bd)
        ctx.deblock_plane(state, drec[p], p, int(p > 0), int(p > 0), db, cw, ch)
        bad = np.argwhere(drec[p].host() != rec[p].data)
        assert len(bad) == 0, (bd, kinds, p, bad[:4])
        assert (LU.window(rec[p]) != LU.window(case["planes"][p][0])).any()      # the filter did something
    # the frame call on fresh copies of the unfiltered planes
    dfr = [LU.dev(LU.lay(r, k, P, P)) for (r, _), k in zip(case["planes"], k3)]
    ctx.deblock_frame(state, dfr, 1, 1, db, cw, ch)
    for p in range(3):
        assert np.array_equal(dfr[p].host(), rec[p].data), (bd, kinds, p, "frame")
    assert LU.guards_intact(*drec, *dsrc, *dfr)


# ------------------------------------------------------------------ restoration
@pytest.mark.parametrize("kinds", [("odd", "tight", "odd"), ("tight", "odd", "tight"), ("odd", "odd", "tight")])
@pytest.mark.parametrize("w", [64, 128])
@pytest.mark.parametrize("bd", [8, 10])
def test_lrf(ctx, oracle, bd, w, kinds):
    """r1_lrf_sgrproj_plane, r1_sgrproj_solve_batch and r1_lrf_search_batch on one and on two 64-pixel units.
    luma_block_moments (csrc/lrf_search.hip) loads eight source pixels at once where po = data + ((yorigin + y) * stride +
    xorigin + x) * BPP is a multiple of 8 * BPP, x a multiple of 8.  "tight" with 8 pixels of padding keeps that for
    every row at both depths (base aligned, xorigin 8, stride 80 or 144).  "odd" (base one element past the
    boundary, xorigin 9, stride 81 or 145: 1 + 9 + row * 81 elements) leaves one row in eight aligned, at 8 and at
    16 bits alike: the source plane in "odd" is the case that takes the pixel-by-pixel path."""
    import torch
    case = LU.lrf_case(bd, w)
    P = LU.LRF_PAD
    cdef, debl, out = [LU.lay(case[k], kd, P, P) for k, kd in zip(("cdef", "debl", "cdef"), kinds)]
    src = LU.lay(case["src"], kinds[1], P, P)
    dcdef, ddebl, dout, dsrc = LU.dev(cdef), LU.dev(debl), LU.dev(out), LU.dev(src)
    units = case["units"]
    du = torch.from_numpy(units.view(np.uint8).reshape(units.shape + (4,)).copy()).cuda()
    LU.o_lrf_plane(oracle, cdef, debl, out, 0, w, 64, 64, 64, 64, units, bd)
    ctx.lrf_sgrproj_plane(dcdef, ddebl, dout, 0, w, 64, 64, 64, du, 64)
    bad = np.argwhere(dout.host() != out.data)
    assert len(bad) == 0, (bd, w, kinds, bad[:4])
    assert (LU.window(out) != LU.window(cdef)).any()
    got = ctx.sgrproj_solve_batch(dcdef, dsrc, case["solve"], max_w=64, max_h=64).cpu().numpy()
    assert np.array_equal(got, LU.o_sgr_solve(oracle, cdef, src, case["solve"], bd)), (bd, w, kinds, "solve")
    hs, ds = LU.strided(case["scales"], 3, 1 << 20)
    wx, we = LU.o_lrf_search(oracle, cdef, src, case["search"], False, 0, 0, hs, 21000, bd)
    for mx in (64, 128):
        xqd, err = ctx.lrf_search_batch(dcdef, dsrc, case["search"], scales=ds, dist_scale=21000, max_w=mx, max_h=mx)
        assert np.array_equal(xqd.cpu().numpy(), wx), (bd, w, kinds, mx)
        assert np.array_equal(_n(err, np.uint64), we), (bd, w, kinds, mx)
    assert LU.guards_intact(dcdef, ddebl, dout, dsrc)


# ------------------------------------------------------------------ transforms and the quantizer (coeff_stride)
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ts,w,h", [(0, 4, 4), (2, 16, 16), (4, 64, 64)])
def test_coeff_stride(ctx, oracle, bd, ts, w, h):
    """coeff_stride = area + 5 with 0x7FFF in the gap; at 64 points also 32 * 32 + 5 where only the coded area is
    read (r1_inv_txfm_add_batch, r1_quantize_batch; r1_quantize_rdo_batch needs the full block)"""
    from rav1e_amd.types import valid_av1_transform
    rng = np.random.default_rng(ts * 10 + bd)
    n, area, carea = 23, w * h, min(w, 32) * min(h, 32)
    ct, cb = (np.int16, 2) if bd == 8 else (np.int32, 4)
    types = [t for t in range(16) if valid_av1_transform(ts, t)]
    for tx_type in (types[0], types[-1]):
        res = rng.integers(-(1 << bd) + 1, 1 << bd, (n, h, w)).astype(np.int16)
        res[: n // 2] //= 16
        co = np.zeros((n, area), ct)
        assert oracle.r1o_fwd_txfm_batch(O.ptr(res), O.ptr(co), n, ts, tx_type, bd, cb) == 0
        pred = rng.integers(0, 1 << bd, (n, h, w)).astype(_pdt(bd))
        for stride in sorted({area + 5, carea + 5}):
            full = stride >= area
            dense = np.ascontiguousarray(co[:, :min(stride - 5, area)])
            hc, dc = LU.strided(dense, 5, 0x7FFF)
            assert LU.row_stride(hc) == stride and dc.stride(0) == stride
            # quantize (+ dequantize)
            wq, wr, weob = np.zeros((n, carea), ct), np.zeros((n, carea), ct), np.zeros(n, np.uint16)
            assert oracle.r1o_quantize_batch(hc.ctypes.data, stride, n, ts, tx_type, 60, bd, 0, 0, 0, cb, O.ptr(wq),
                                             O.ptr(weob), O.ptr(wr)) == 0
            o = ctx.quantize_batch(dc, ts, tx_type, 60, bd, False)
            key = (bd, w, tx_type, stride)
            assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
            assert np.array_equal(_n(o["eobs"], np.uint16), weob), key
            assert np.array_equal(o["rcoeffs"].cpu().numpy(), wr), key
            assert (weob > 1).any()
            # the inverse transform of the dequantized block at the same stride
            hr, dr = LU.strided(wr, stride - carea, 0x7FFF)       # the coded area leads the block
            wrec = np.zeros((n, h, w), _pdt(bd))
            assert oracle.r1o_inv_txfm_add_batch(hr.ctypes.data, stride, O.ptr(pred), O.ptr(wrec), n, ts, tx_type, bd,
                                                 cb, 1 if bd == 8 else 2) == 0
            got = ctx.inverse_transform_add_batch(dr, _t(pred), ts, tx_type, bd)
            assert np.array_equal(_n(got, _pdt(bd)), wrec), key
            if full:
                wd, wrate = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
                assert oracle.r1o_quantize_rdo_batch(hc.ctypes.data, stride, n, ts, tx_type, 60, bd, 0, 0, 0, cb,
                                                     O.ptr(wq), O.ptr(weob), O.ptr(wr), O.ptr(wd), O.ptr(wrate)) == 0
                o = ctx.quantize_rdo_batch(dc, ts, tx_type, 60, bd, False)
                assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
                assert np.array_equal(_n(o["eobs"], np.uint16), weob), key
                assert np.array_equal(_n(o["tx_dist"], np.uint64), wd), key
                assert np.array_equal(_n(o["est_rate"], np.uint64), wrate), key



# ------------------------------------------------------------------ lookahead and frame glue
@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10])
def test_lookahead_maps(ctx, oracle, bd, kinds):
    """100 x 68 (no multiple of 8): the intra and inter cost maps, the importance block difference, the activity
    scales; motion vectors of up to 8 pixels, so the reference plane carries 8 + 4 pixels of padding"""
    w, h = 100, 68
    rng = np.random.default_rng(31 + bd)
    a, b = _base(bd, 130 + bd, 2, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    a.view()[:] = np.clip((np.sin(xx / 9.0) + np.cos(yy / 5.0)) * 60 * (1 << (bd - 8)) + (1 << (bd - 1)) +
                          rng.integers(-8, 9, (h, w)), 0, (1 << bd) - 1)
    # the activity mask reads its last blocks whole: up to 7 pixels of the source's right / bottom padding
    a, b = LU.lay(a, kinds[0], 8, 8), LU.lay(b, kinds[1], MC_PAD, MC_PAD)
    da, db = LU.dev(a), LU.dev(b)
    hb, wb = h // 8, w // 8
    pa, pb = a.cstruct(), b.cstruct()
    want = np.zeros(hb * wb, np.uint32)
    oracle.r1o_estimate_intra_costs(C.byref(pa), bd, O.ptr(want))
    assert np.array_equal(_n(ctx.estimate_intra_costs(da), np.uint32).ravel(), want), (bd, kinds, "intra")
    mvs = rng.integers(-64, 65, (hb, wb, 2)).astype(np.int16)
    want = np.zeros(hb * wb, np.uint32)
    oracle.r1o_estimate_inter_costs(C.byref(pa), C.byref(pb), O.ptr(mvs), O.ptr(want))
    assert np.array_equal(_n(ctx.estimate_inter_costs(da, db, _t(mvs)), np.uint32).ravel(), want), (bd, kinds, "inter")
    tot = oracle.r1o_importance_block_difference(C.byref(pa), C.byref(pb))
    assert ctx.importance_block_difference(da, db) == tot / (hb * wb)
    hv, hw = (h + 7) // 8, (w + 7) // 8
    wvar, wsc = np.zeros(hv * hw, np.uint32), np.zeros(hv * hw, np.uint32)
    oracle.r1o_activity_scales(C.byref(pa), O.ptr(wvar), O.ptr(wsc))
    var, sc = ctx.activity_scales(da)
    assert np.array_equal(_n(var, np.uint32).ravel(), wvar) and np.array_equal(_n(sc, np.uint32).ravel(), wsc)
    assert LU.guards_intact(da, db)


# ------------------------------------------------------------------ intra: edges -> predictors -> the fused candidate
EDGE_STRIDE = 257 + 7


def _edges(ctx, drec, tile, ts, ec):
    """r1_intra_edges_batch into sets EDGE_STRIDE pixels apart -> (edges view (n, 257), lens, the whole tensor)"""
    import torch
    from rav1e_amd.api import INTRA_EDGE_CAND, _pix_dtype
    n = len(ec)
    edges, big = LU.strided_out(n, 257, EDGE_STRIDE - 257, _pix_dtype(drec.bpp))
    lens = torch.empty((n, 2), dtype=torch.uint8, device="cuda")
    dc = torch.from_numpy(np.ascontiguousarray(ec, INTRA_EDGE_CAND).view(np.uint8)).cuda()
    pr = drec.cstruct()
    assert ctx.lib.r1_intra_edges_batch(ctx.h, C.byref(pr), *tile, ts, dc.data_ptr(), n, edges.data_ptr(), EDGE_STRIDE,
                                        lens.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert LU.gap_intact(big, 257)
    return edges, lens, big


def _oracle_edges(oracle, rec, tile, ts, ec, bd):
    """r1o_get_intra_edges per candidate -> (edges (n, 257), lens (n, 2))"""
    n, hbd = len(ec), int(bd > 8)
    e, l = np.zeros((n, 257), _pdt(bd)), np.zeros((n, 2), np.int32)
    for i in range(n):
        li, f = (C.c_int * 2)(), int(ec["flags"][i])
        oracle.r1o_get_intra_edges(O.ptr(e[i]), li, rec.block_ptr(tile[0], tile[1]), rec.stride, int(ec["x"][i]),
                                   int(ec["y"][i]), tile[2], tile[3], ts, bd, int(ec["mode"][i]), f & 1,
                                   int(ec["angle_delta"][i]), (f >> 1) & 1, (f >> 2) & 1, hbd)
        l[i] = li[0], li[1]
    return e, l


def _same_edges(got_e, got_l, want_e, want_l):
    assert np.array_equal(got_l, want_l)
    for i in range(len(want_l)):
        il, ia = want_l[i]
        assert np.array_equal(got_e[i, 128 - il:129 + ia], want_e[i, 128 - il:129 + ia]), i


@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_intra_edges_predict_satd_and_fused_candidate(ctx, oracle, bd, kinds):
    """98 x 70: blocks at the origin, in the first row and column, and cut by the right and the bottom edge, 13 luma
    modes each from one shared edge set.  The edge sets are EDGE_STRIDE apart, the seven pixels between them guarded
    on output, and the same buffer feeds r1_predict_intra_batch, r1_intra_satd_batch and r1_rdo_intra_cand_batch
    (edge_group 13, the scale grid strided).  A cut block's source reaches into the padding: 64 pixels of it."""
    from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND
    w_, h_ = 98, 70
    rng = np.random.default_rng(140 + bd)
    rec = _base(bd, 150 + bd, 1, w_, h_)[0]
    src = O.HostPlane(w_, h_, bd, 64, 64, rng=rng)
    rec, src = LU.lay(rec, kinds[0], 0, 0), LU.lay(src, kinds[1], 64, 64)
    drec, dsrc = LU.dev(rec), LU.dev(src)
    tile = (0, 0, w_, h_)
    hbd = int(bd > 8)
    grid = rng.integers(1 << 12, 1 << 16, (17, 21)).astype(np.uint32)       # a cut 64 x 64 block ends at (160, 128)
    hs, ds = LU.strided(grid, 3, 1 << 20)
    BASE = [0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0]
    for ts, w, h in ((0, 4, 4), (2, 16, 16), (4, 64, 64)):
        gx, gy = (w_ + w - 1) // w, (h_ + h - 1) // h
        nb = 10
        bx, by = rng.integers(0, gx, nb) * w, rng.integers(0, gy, nb) * h
        bx[:5], by[:5] = [0, w, 0, (gx - 1) * w, 0], [0, 0, h, 0, (gy - 1) * h]
        ec = np.zeros(nb, INTRA_EDGE_CAND)
        ec["x"], ec["y"], ec["mode"] = bx, by, -1
        ec["flags"] = 1 | (rng.integers(0, 4, nb) << 1)
        edges, lens, big = _edges(ctx, drec, tile, ts, ec)
        want_e, want_l = _oracle_edges(oracle, rec, tile, ts, ec, bd)
        _same_edges(_n(edges, _pdt(bd)), lens.cpu().numpy(), want_e, want_l)
        var = np.where((bx == 0) & (by == 0), 0, np.where(by == 0, 1, np.where(bx == 0, 2, 3)))
        pm, v13 = np.tile(np.arange(13), nb), np.repeat(var, 13)
        pm = np.where((pm == 12) & (v13 == 0), 0, np.where((pm == 12) & (v13 == 2), 1,
                      np.where((pm == 12) & (v13 == 1), 2, pm)))
        n = nb * 13
        ic = np.zeros(n, INTRA_CAND)
        ic["mode"], ic["variant"], ic["angle"] = pm, v13, np.array(BASE)[pm]
        ic["ief"] = np.where((pm >= 1) & (pm <= 8), np.tile(rng.integers(1, 3, 13), nb), 0)
        ic["avail_w"] = np.repeat(np.minimum(w, w_ - bx), 13)
        ic["avail_h"] = np.repeat(np.minimum(h, h_ - by), 13)
        pred = np.zeros((n, h, w), _pdt(bd))
        for i in range(n):
            b = i // 13
            assert oracle.r1o_dispatch_predict_intra(
                int(pm[i]), int(v13[i]), O.ptr(pred[i]), w, ts, bd, None, int(ic["angle"][i]), int(ic["ief"][i]),
                O.ptr(want_e[b]), int(want_l[b, 0]), int(want_l[b, 1]), int(ic["avail_w"][i]), int(ic["avail_h"][i]),
                hbd) == 0
        # the predictor alone takes one edge set per candidate: the shared sets, repeated at the same stride
        rep_e, rep_big = LU.strided_out(n, 257, EDGE_STRIDE - 257, edges.dtype)
        rep_e.copy_(edges.repeat_interleave(13, 0))
        got = ctx.predict_intra_batch(ts, ic, rep_e, lens.repeat_interleave(13, 0).contiguous(), bd)
        assert np.array_equal(_n(got, _pdt(bd)), pred), (bd, kinds, w, "predict")
        pos = _t(np.stack([bx, by], 1).astype(np.int16))
        want_satd = np.array([oracle.r1o_get_satd(src.block_ptr(int(bx[i // 13]), int(by[i // 13])), src.stride,
                                                  O.ptr(pred[i]), w, w, h, hbd) for i in range(n)], np.uint32)
        got = _n(ctx.intra_satd_batch(dsrc, ts, ic, 13, pos, edges, lens), np.uint32)
        assert np.array_equal(got, want_satd), (bd, kinds, w, "satd")
        # the fused candidate = the transform-type search on those predictions
        mask, kind, qi = ctx.tx_type_mask(ts, False), (3 if bd == 8 else 2), 70
        nt, carea = bin(mask).count("1"), min(w, 32) * min(h, 32)
        c = np.zeros(n, O.RDO_CAND)
        c["ox"], c["oy"] = np.repeat(bx, 13), np.repeat(by, 13)
        ct = np.int16 if bd == 8 else np.int32
        wsad, wsatd = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        weob, wdist = np.zeros((n, nt), np.uint16), np.zeros((n, nt), np.uint64)
        wq, wrec = np.zeros((n, nt, carea), ct), np.zeros((n, nt, h, w), _pdt(bd))
        pa = src.cstruct()
        assert oracle.r1o_rdo_txsearch_batch(
            C.byref(pa), None, O.ptr(pred), w, h, ts, O.ptr(c), n, mask, qi, 1, 0, 0, kind, hs.ctypes.data,
            LU.row_stride(hs), 0, 0, O.ptr(wsad), O.ptr(wsatd), O.ptr(weob), O.ptr(wdist), None, O.ptr(wq),
            O.ptr(wrec)) == 0
        o = ctx.rdo_intra_cand_batch(dsrc, w, h, ic, pos, edges, lens, mask, qi, kind, edge_group=13, scales=ds,
                                     want_sad=True, want_satd=True, want_qcoeffs=True, want_rec=True, want_pred=True)
        key = (bd, kinds, w)
        assert np.array_equal(_n(o["pred"], _pdt(bd)), pred), key
        assert np.array_equal(_n(o["sad"], np.uint32), wsad), key
        assert np.array_equal(_n(o["satd"], np.uint32), wsatd), key
        assert np.array_equal(_n(o["eob"], np.uint16), weob), key
        assert np.array_equal(o["qcoeffs"].cpu().numpy(), wq), key
        assert np.array_equal(_n(o["rec"], _pdt(bd)), wrec), key
        assert np.array_equal(_n(o["dist"], np.uint64), wdist), key
        assert LU.gap_intact(big, 257) and LU.gap_intact(rep_big, 257)
    assert LU.guards_intact(drec, dsrc)


@pytest.mark.parametrize("kinds", [("odd", "tight", "odd"), ("tight", "odd", "tight")])
@pytest.mark.parametrize("bd", [8, 10])
def test_cfl_ac_and_alpha_search(ctx, oracle, bd, kinds):
    """luma, the chroma reconstruction and the chroma source (4:2:0) each in a layout of their own, the chroma edge
    sets EDGE_STRIDE apart"""
    from rav1e_amd.api import CFL_AC_CAND, CFL_ALPHA_CAND, INTRA_EDGE_CAND
    rng = np.random.default_rng(160 + bd)
    luma = _base(bd, 170 + bd, 1)[0]
    lv = luma.view().astype(np.int64)
    sub = (lv[0::2, 0::2] + lv[0::2, 1::2] + lv[1::2, 0::2] + lv[1::2, 1::2]) // 4
    rec = LU.noise_padded(np.clip(sub // 2 + rng.integers(0, 1 << (bd - 1), sub.shape), 0, (1 << bd) - 1), bd, 16)
    src = LU.noise_padded(np.clip(sub * 3 // 4 + rng.integers(0, 1 << (bd - 2), sub.shape), 0, (1 << bd) - 1), bd, 16)
    luma, rec, src = LU.lay(luma, kinds[0], 0, 0), LU.lay(rec, kinds[1], 0, 0), LU.lay(src, kinds[2], 0, 0)
    dl, dr, dsrc = LU.dev(luma), LU.dev(rec), LU.dev(src)
    hbd = int(bd > 8)
    for ts, w, h in ((0, 4, 4), (2, 16, 16)):
        n = 12
        gx, gy = rec.width // w, rec.height // h
        bx, by = rng.integers(0, gx, n) * w, rng.integers(0, gy, n) * h
        bx[:3], by[:3] = [0, w, 0], [0, 0, h]
        ec = np.zeros(n, INTRA_EDGE_CAND)
        ec["x"], ec["y"], ec["mode"], ec["flags"] = bx, by, 13, 1
        tile = (0, 0, rec.width, rec.height)
        edges, lens, big = _edges(ctx, dr, tile, ts, ec)
        want_e, want_l = _oracle_edges(oracle, rec, tile, ts, ec, bd)
        _same_edges(_n(edges, _pdt(bd)), lens.cpu().numpy(), want_e, want_l)
        ac_c = np.zeros(n, CFL_AC_CAND)
        ac_c["x"], ac_c["y"] = bx * 2, by * 2
        ac = ctx.cfl_ac_batch(dl, w, h, 1, 1, ac_c)
        hac = np.zeros((n, w * h), np.int16)
        for i in range(n):
            oracle.r1o_pred_cfl_ac(O.ptr(hac[i]), luma.block_ptr(int(bx[i]) * 2, int(by[i]) * 2), luma.stride, w, h,
                                   0, 0, 1, 1, hbd)
        assert np.array_equal(ac.cpu().numpy(), hac), (bd, kinds, w, "ac")
        var = np.where((bx == 0) & (by == 0), 0, np.where(by == 0, 1, np.where(bx == 0, 2, 3)))
        cc = np.zeros(n, CFL_ALPHA_CAND)
        cc["x"], cc["y"], cc["variant"] = bx, by, var
        cc["vis_w"] = np.where(rng.random(n) < 0.3, rng.integers(1, w + 1, n), w)
        cc["vis_h"] = np.where(rng.random(n) < 0.3, rng.integers(1, h + 1, n), h)
        alpha, cost = ctx.cfl_alpha_search_batch(dsrc, ts, cc, edges, lens, ac)
        alpha, cost = alpha.cpu().numpy(), cost.cpu().numpy()
        for i in range(n):
            vw, vh = int(cc["vis_w"][i]), int(cc["vis_h"][i])
            s = src.view()[by[i]:by[i] + vh, bx[i]:bx[i] + vw].astype(np.int64)
            costs = {}
            for a in range(-16, 17):
                out = np.zeros((h, w), _pdt(bd))
                assert oracle.r1o_dispatch_predict_intra(13 if a else 0, int(var[i]), O.ptr(out), w, ts, bd,
                                                         O.ptr(hac[i]), a, 0, O.ptr(want_e[i]), int(want_l[i, 0]),
                                                         int(want_l[i, 1]), w, h, hbd) == 0
                d = s - out[:vh, :vw].astype(np.int64)
                costs[a] = int((d * d).sum())
            best, best_a, count = costs[0], 0, 2          # rdo_cfl_alpha's search order and early exit
            for a in range(1, 17):
                if costs[a] < best:
                    best, best_a, count = costs[a], a, count + 2
                if costs[-a] < best:
                    best, best_a, count = costs[-a], -a, count + 2
                if count < a:
                    break
            assert (int(alpha[i]), int(cost[i])) == (best_a, best), (bd, kinds, w, i)
        assert LU.gap_intact(big, 257)
    assert LU.guards_intact(dl, dr, dsrc)


# ------------------------------------------------------------------ motion estimation
@pytest.mark.parametrize("kinds", SWAP)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_motion_estimation(ctx, oracle, bd, kinds):
    """one 128 x 64 tile: the three pyramid levels of the source and of the reference in alternating kinds (the
    two planes of a level never share one), with the reference's padding (88 / 44 / 22); r1_estimate_tile_motion_batch
    at launch boundaries (launch_mode 1) and as the persistent launch (2), then r1_estimate_motion_batch"""
    from rav1e_amd.api import ME_RESULT, me_lambdas
    from test_gpu_parity import _me_images, _me_stats_numpy, _me_stats_tensor, uses_the_depth
    w, h = 128, 64
    org, ref = _me_images("smooth", w, h, bd, 7 * bd + w)
    assert uses_the_depth(bd, org, ref)
    pads = (88, 44, 22)
    po = [LU.lay(p, kinds[l & 1], pads[l], pads[l]) for l, p in enumerate(O.me_pyramid(org, bd))]
    pr = [LU.lay(p, kinds[~l & 1], pads[l], pads[l]) for l, p in enumerate(O.me_pyramid(ref, bd))]
    dpo, dpr = [LU.dev(p) for p in po], [LU.dev(p) for p in pr]
    rng = np.random.default_rng(w + bd)
    prev, init = np.zeros((h // 4, w // 4), O.ME_STATS), np.zeros((h // 4, w // 4), O.ME_STATS)
    for a, r in ((prev, 80), (init, 40)):
        a["row"], a["col"] = rng.integers(-r, r + 1, a.shape), rng.integers(-r, r + 1, a.shape)
        a["normalized_sad"] = rng.integers(0, 1 << 22, a.shape)
    lam = me_lambdas(30.0)
    want = init.copy()
    O.me_oracle(oracle, po, pr, w // 4, h // 4, (0, 0, w, h), bd, lam, want, prev)
    assert (want != init).any()
    for mode in (1, 2):
        st = _me_stats_tensor(init)
        job = dict(org=dpo, ref=dpr, stats=st, prev=_me_stats_tensor(prev), tile=(0, 0, w, h))
        ctx.estimate_tile_motion([job], w // 4, h // 4, bd, lam, launch_mode=mode)
        assert ctx.me_status(wait=True)[0]
        bad = np.argwhere(_me_stats_numpy(st) != want)
        assert len(bad) == 0, (bd, kinds, mode, bad[:5])
    sizes = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (16, 64), (64, 16)]
    c = np.zeros(4 * len(sizes), O.ME_BLOCK_CAND)
    for i in range(len(c)):
        bw, bh = sizes[i % len(sizes)]
        c["w"][i], c["h"][i] = bw, bh
        c["bx"][i], c["by"][i] = rng.integers(0, (w - bw) // 4 + 1), rng.integers(0, (h - bh) // 4 + 1)
        c["corner"][i] = rng.choice([0, 1, 3, 5, 7])
        c["pmv"][i] = rng.integers(-40, 41, (2, 2))
    job = dict(org=dpo, ref=dpr, stats=_me_stats_tensor(want), prev=_me_stats_tensor(prev), tile=(0, 0, w, h))
    for use_satd, fmode, hp in ((1, 0, 1), (0, 2, 0)):
        wres = O.me_block_oracle(oracle, po, pr, w // 4, h // 4, (0, 0, w, h), bd, lam, want, prev, c,
                                 use_satd=use_satd, filter_mode=fmode, allow_hp=hp)
        got = ctx.estimate_motion_batch(job, c, w // 4, h // 4, bd, lam, use_satd=bool(use_satd), filter_mode=fmode,
                                        allow_hp=bool(hp)).cpu().numpy().view(ME_RESULT)
        bad = np.nonzero(got != wres)[0]
        assert len(bad) == 0, (bd, kinds, use_satd, fmode, c[bad[0]], got[bad[0]], wres[bad[0]])
        assert not hp or (((wres["row"] | wres["col"]) & 7) != 0).any()      # the sub-pel diamond moved a block
    assert LU.guards_intact(*dpo, *dpr)

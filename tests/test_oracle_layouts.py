"""The CPU oracle and tests/layout_util.py are layout-independent: one call per oracle family gives the same
result on the HostPlane layout, on the "odd" and the "tight" layout of the same pixels, and with its strided
arrays dense or strided.  tests/test_gpu_layouts.py compares the library with the oracle on these layouts; without
this module a mismatch there could be the oracle's or the helper's."""
import numpy as np
import pytest

import layout_util as LU
import oracle_lib as O
from test_gpu_parity import rand_dist_cands, rand_mc_cands

LAYOUTS = [None, "odd", "tight"]      # None: the HostPlane layout itself


_lay = LU.lay


def _pairs():
    """layout pairs for the planes of a two-plane call: every layout meets every other"""
    return [(a, b) for a in LAYOUTS for b in LAYOUTS]


@pytest.mark.parametrize("kind", ["odd", "tight"])
@pytest.mark.parametrize("bd", [8, 10])
def test_relayout_geometry_and_content(bd, kind):
    hp = O.HostPlane(96, 64, bd, 24, 16, rng=np.random.default_rng(bd))
    for xpad, ypad in ((8, 8), (11, 3), (0, 0), (24, 16)):
        p = LU.lay(hp, kind, xpad, ypad)
        if kind == "odd":
            assert p.xorigin == xpad | 1 and p.yorigin == ypad + 1
            assert p.stride % 2 == 1 and 0 <= p.stride - (p.xorigin + 96 + xpad) <= 1
        else:
            assert (p.xorigin, p.yorigin, p.stride) == (xpad, ypad, 96 + 2 * xpad)
        assert p.alloc_height == p.yorigin + 64 + ypad and p.data.shape == (p.alloc_height, p.stride)
        assert p.data.dtype == hp.data.dtype and int(p.data.max()) < 1 << bd
        assert np.array_equal(LU.window(p, xpad, ypad), LU.window(hp, xpad, ypad))
        c = p.cstruct()
        assert (c.stride, c.xorigin, c.yorigin, c.alloc_height, c.bytes_per_px) == (
            p.stride, p.xorigin, p.yorigin, p.alloc_height, p.bpp)


def test_host_strided_keeps_values_and_poisons_the_gap():
    a = np.arange(12, dtype=np.uint32).reshape(3, 4)
    v = LU.host_strided(a, 3, 1 << 20)
    assert np.array_equal(v, a) and LU.row_stride(v) == 7 and (v.base[:, 4:] == 1 << 20).all()
    b = np.arange(48, dtype=np.uint8).reshape(2, 3, 8)
    v = LU.host_strided(b, 2, 0xFF)
    assert np.array_equal(v, b) and v.strides[0] // 8 == 5 and (v.base[:, 3:] == 0xFF).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_dist_batch(oracle, bd):
    rng = np.random.default_rng(bd)
    a, b = O.HostPlane(96, 64, bd, 8, 8, rng=rng), O.HostPlane(96, 64, bd, 8, 8, rng=rng)
    for (w, h) in ((8, 8), (64, 64)):
        c = rand_dist_cands(rng, 67, 96, 64, w, h, 8)
        for kind in (0, 1):
            want = LU.o_dist(oracle, kind, a, b, w, h, c)
            for ka, kb in _pairs():
                got = LU.o_dist(oracle, kind, _lay(a, ka, 0, 0), _lay(b, kb, 8, 8), w, h, c)
                assert np.array_equal(got, want), (bd, w, kind, ka, kb)
    scales = rng.integers(1 << 12, 1 << 16, (8, 12)).astype(np.uint32)
    c = rand_dist_cands(rng, 67, 96, 64, 8, 8, 0)
    c["ox"] &= ~7
    c["oy"] &= ~7
    for kind in (2, 3):
        want = LU.o_dist_scaled(oracle, kind, a, b, 8, 8, c, scales)
        got = LU.o_dist_scaled(oracle, kind, _lay(a, "odd", 0, 0), _lay(b, "tight", 0, 0), 8, 8, c,
                               LU.host_strided(scales, 3, 1 << 20))
        assert np.array_equal(got, want), (bd, kind)


@pytest.mark.parametrize("bd", [8, 10])
def test_mc_put_prep_batch(oracle, bd):
    rng = np.random.default_rng(10 + bd)
    a = O.HostPlane(96, 64, bd, 16, 16, rng=rng)
    for (w, h) in ((4, 4), (8, 8), (64, 64)):
        c = rand_mc_cands(rng, 41, 96, 64, w, h, 8)
        want = LU.o_mc(oracle, a, w, h, c)
        for k in ("odd", "tight"):
            got = LU.o_mc(oracle, LU.lay(a, k, 12, 12), w, h, c)     # 8 of slack + the 3 / 4 taps
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (bd, w, k)


@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_filter_tile_plane(oracle, bd):
    case = LU.cdef_case(bd)
    want = LU.cdef_filter_oracle(oracle, case, [None] * 3, [None] * 3, strided=False)
    for ks, kd in ((("odd", "tight", "odd"), ("tight", "odd", "tight")), (("tight", "odd", None), (None, "tight", "odd"))):
        got = LU.cdef_filter_oracle(oracle, case, ks, kd, strided=True)
        for p in range(3):
            assert np.array_equal(LU.window(got[p]), LU.window(want[p])), (bd, p, ks, kd)
            # what CDEF does not write keeps its content: the padding the layouts share
            assert np.array_equal(LU.window(got[p], LU.CDEF_PAD, LU.CDEF_PAD),
                                  LU.window(want[p], LU.CDEF_PAD, LU.CDEF_PAD))
    assert any((LU.window(want[p]) != LU.window(case["src"][p])).any() for p in range(3))


@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_strength_search(oracle, bd):
    case = LU.cdef_case(bd)
    prm = LU.cdef_search_params(case)
    want = LU.o_cdef_search(oracle, case["rec"], case["src"], case["skip"], case["scales"], prm)
    rec = [LU.lay(p, k, LU.CDEF_PAD, LU.CDEF_PAD) for p, k in zip(case["rec"], ("odd", "tight", "odd"))]
    src = [LU.lay(p, k, LU.CDEF_PAD, LU.CDEF_PAD) for p, k in zip(case["src"], ("tight", "odd", "tight"))]
    got = LU.o_cdef_search(oracle, rec, src, LU.host_strided(case["skip"], 3, LU.flip_poison(case["skip"])),
                           LU.host_strided(case["scales"], 3, 1 << 20), prm)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[1] == -1).any() and (want[1] >= 0).any()


@pytest.mark.parametrize("bd", [8, 10])
def test_deblock_plane(oracle, bd):
    case = LU.deblock_case(bd)
    blocks = case["blocks"]
    sblocks = LU.host_strided(blocks, 2, 0xFF)
    for pli in range(3):
        xd, yd = (0, 0) if pli == 0 else (1, 1)
        rec, src = case["planes"][pli]
        want_t = LU.o_deblock_sse(oracle, rec, src, pli, xd, yd, blocks, case["cw"], case["ch"], bd)
        want = LU.lay(rec, "tight", LU.DEBLOCK_PAD, LU.DEBLOCK_PAD)
        LU.o_deblock(oracle, case["state"], want, pli, xd, yd, blocks, case["cw"], case["ch"], bd)
        assert (LU.window(want) != LU.window(rec)).any()
        for kr, ks in (("odd", "tight"), ("tight", "odd")):
            r = LU.lay(rec, kr, LU.DEBLOCK_PAD, LU.DEBLOCK_PAD)
            s = LU.lay(src, ks, LU.DEBLOCK_PAD, LU.DEBLOCK_PAD)
            assert np.array_equal(LU.o_deblock_sse(oracle, r, s, pli, xd, yd, sblocks, case["cw"], case["ch"], bd), want_t)
            LU.o_deblock(oracle, case["state"], r, pli, xd, yd, sblocks, case["cw"], case["ch"], bd)
            assert np.array_equal(LU.window(r, LU.DEBLOCK_PAD, LU.DEBLOCK_PAD),
                                  LU.window(want, LU.DEBLOCK_PAD, LU.DEBLOCK_PAD)), (bd, pli, kr)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w", [64, 128])
def test_lrf_filter_solve_and_search(oracle, bd, w):
    case = LU.lrf_case(bd, w)
    P = LU.LRF_PAD

    def run(kc, kd, ko, scales):
        cdef, debl, out = _lay(case["cdef"], kc, P, P), _lay(case["debl"], kd, P, P), _lay(case["cdef"], ko, P, P)
        LU.o_lrf_plane(oracle, cdef, debl, out, 0, w, 64, 64, 64, 64, case["units"], bd)
        xqd = LU.o_sgr_solve(oracle, cdef, _lay(case["src"], kd, P, P), case["solve"], bd)
        sx, se = LU.o_lrf_search(oracle, cdef, _lay(case["src"], kd, P, P), case["search"], False, 0, 0, scales, 21000, bd)
        return LU.window(out, P, P).copy(), xqd, sx, se
    want = run(None, None, None, case["scales"])
    assert (want[0] != LU.window(case["cdef"], P, P)).any()
    for kc, kd, ko in (("odd", "tight", "odd"), ("tight", "odd", "tight"), ("odd", "odd", "tight")):
        got = run(kc, kd, ko, LU.host_strided(case["scales"], 3, 1 << 20))
        for g, x in zip(got, want):
            assert np.array_equal(g, x), (bd, w, kc, kd, ko)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,fw,fh", [(71, 37, 71, 37), (200, 9, 200, 9), (72, 37, 71, 37)])
def test_plane_pad_and_downsample(oracle, bd, w, h, fw, fh):
    rng = np.random.default_rng(w + bd)
    full = O.HostPlane(w, h, bd, 16, 16, rng=rng)
    half = O.HostPlane((w + 1) // 2, (h + 1) // 2, bd, 8, 8, rng=rng)
    want_f = LU.lay(full, "tight", 16, 16)
    LU.o_pad(oracle, want_f, fw, fh)
    want_h = LU.lay(half, "tight", 8, 8)
    LU.o_downsample(oracle, want_f, want_h, fw, fh, 1)
    for kf, kh in ((None, None), ("odd", "tight"), ("tight", "odd"), ("odd", "odd")):
        f, hf = _lay(full, kf, 16, 16), _lay(half, kh, 8, 8)
        LU.o_pad(oracle, f, fw, fh)
        assert np.array_equal(LU.window(f, 16, 16), LU.window(want_f, 16, 16)), (bd, w, kf)
        # the whole allocation is border: nothing of the layout's extra column / row keeps its noise
        pw = min(fw, w)
        assert (f.data[:, :f.xorigin] == f.data[:, f.xorigin:f.xorigin + 1]).all()
        assert (f.data[:, f.xorigin + pw:] == f.data[:, f.xorigin + pw - 1:f.xorigin + pw]).all()
        assert (f.data[:f.yorigin] == f.data[f.yorigin]).all()
        LU.o_downsample(oracle, f, hf, fw, fh, 1)
        assert np.array_equal(LU.window(hf, 8, 8), LU.window(want_h, 8, 8)), (bd, w, kf, kh)

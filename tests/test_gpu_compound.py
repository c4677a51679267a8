"""r1_rdo_compound_cand_batch (csrc/mc_compound.hip) on the device: the executed predict_inter_compound vectors,
exact parity with the oracle's own composition (r1o_mc_prep_batch x 2 -> r1o_mc_avg_batch -> r1o_dist_batch), the
chain into the dense-prediction entry points, the compound leg of the inter pre-screen, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import cand_size_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

PW, PH, PAD = 160, 128, 88
# every transform size (one k_compound_fast per size and depth; the 4-tap set among them) and the slab kernel with two
# and four slabs (128-wide / -high); test_cand_size_cases.py holds the table against the 19 x 3 without a device
SIZES = K.COMPOUND_SIZES
NS = (1, 5, 67)


def dev_plane(hp):
    from rav1e_amd.api import Plane
    return Plane.from_numpy(hp.data, hp.width, hp.height, hp.bit_depth, hp.xpad, hp.ypad)


def px_dtype(bd):
    return np.uint8 if bd == 8 else np.uint16


def make_cands(rng, w, h, n, k):
    """n candidates; `k` rotates which of the fixed patterns the first ones get, so that n = 1 meets them all over
    the sizes.  Fractions (col0, row0, col1, row1): both full-pel, one full-pel, crossed 1-D, and (15,15)/(1,1).
    Windows rows/columns [r - 3, r + size + 4): the four corner positions reach 40 px into the padding."""
    from rav1e_amd.api import COMPOUND_CAND
    c = np.zeros(n, COMPOUND_CAND)
    c["ox"] = rng.integers(0, PW - w + 1, n)
    c["oy"] = rng.integers(0, PH - h + 1, n)
    for f in ("rx0", "rx1"):
        c[f] = rng.integers(-20, PW - w + 21, n)
    for f in ("ry0", "ry1"):
        c[f] = rng.integers(-20, PH - h + 21, n)
    for f in ("col_frac0", "row_frac0", "col_frac1", "row_frac1"):
        c[f] = rng.integers(0, 16, n)
    c["mode_x"] = rng.integers(0, 4, n)              # REGULAR, SMOOTH, SHARP, BILINEAR
    c["mode_y"] = np.where(rng.integers(0, 2, n) == 1, c["mode_x"], rng.integers(0, 4, n))
    lo, hix, hiy = -40 + 3, PW + 40 - 4 - w, PH + 40 - 4 - h
    corners = [(lo, lo, hix, hiy), (hix, lo, lo, hiy), (lo, hiy, hix, lo), (hix, hiy, lo, lo)]
    for i in range(n):
        f = int(rng.integers(1, 16))
        pat = [(0, 0, 0, 0), (0, 0, f, f), (f, 0, 0, f), (15, 15, 1, 1), None, None][(i + k) % 6]
        if pat is not None:
            c["col_frac0"][i], c["row_frac0"][i], c["col_frac1"][i], c["row_frac1"][i] = pat
        if i < 4:
            c["rx0"][i], c["ry0"][i], c["rx1"][i], c["ry1"][i] = corners[(i + k) % 4]
    return c


def mc_cands(c, i):
    m = np.zeros(len(c), O.MC_CAND)
    m["rx"], m["ry"] = c["rx%d" % i], c["ry%d" % i]
    m["col_frac"], m["row_frac"] = c["col_frac%d" % i], c["row_frac%d" % i]
    m["mode_x"], m["mode_y"] = c["mode_x"], c["mode_y"]
    return m


def oracle_compound(oracle, org, r0, r1, w, h, c, dists=True):
    """the oracle's own composition -> (pred (n, h, w), sad or None, satd or None)"""
    n, bd = len(c), org.bit_depth
    ts = []
    for i, r in enumerate((r0, r1)):
        t = np.zeros((n, h, w), np.int16)
        pr = r.cstruct()
        assert oracle.r1o_mc_prep_batch(C.byref(pr), w, h, O.ptr(mc_cands(c, i)), n, O.ptr(t)) == 0
        ts.append(t)
    pred = np.zeros((n, h, w), px_dtype(bd))
    assert oracle.r1o_mc_avg_batch(O.ptr(ts[0]), O.ptr(ts[1]), w, h, n, bd, org.bpp, O.ptr(pred)) == 0
    if not dists:
        return pred, None, None
    hp = O.HostPlane(w, n * h, bd, 0, 0)             # the predictions stacked into one plane
    hp.view()[...] = pred.reshape(n * h, w)
    dc = np.zeros(n, O.DIST_CAND)
    dc["ox"], dc["oy"], dc["ry"] = c["ox"], c["oy"], np.arange(n) * h
    po, pp = org.cstruct(), hp.cstruct()
    out = []
    for kind in (0, 1):
        d = np.zeros(n, np.uint32)
        assert oracle.r1o_dist_batch(kind, C.byref(po), C.byref(pp), w, h, O.ptr(dc), n, O.ptr(d)) == 0
        out.append(d)
    return pred, out[0], out[1]


def gpu_outs(o, bd):
    """device outputs -> numpy in the oracle's types"""
    r = {}
    for k, v in o.items():
        a = v.cpu().numpy()
        r[k] = a.view(px_dtype(bd)) if k == "pred" else a.view(np.uint32)
    return r


def check_all(ctx, oracle, planes, dplanes, w, h, c, combos):
    org, r0, r1 = planes
    bd = org.bit_depth
    pred, sad, satd = oracle_compound(oracle, org, r0, r1, w, h, c)
    want = {"sad": sad, "satd": satd, "pred": pred}
    for keys in combos:
        o = ctx.rdo_compound_cand_batch(*dplanes, w, h, c, want_sad="sad" in keys, want_satd="satd" in keys,
                                        want_pred="pred" in keys)
        assert sorted(o) == sorted(keys)      # nothing else was allocated: the other pointers were NULL
        got = gpu_outs(o, bd)
        for k in keys:
            assert np.array_equal(got[k], want[k]), (bd, w, h, len(c), keys, k)


ALL3 = (("sad", "satd", "pred"),)
EACH = (("sad",), ("satd",), ("pred",), ("sad", "satd", "pred"))


# ---- 1. the executed predict_inter_compound cases ----
def test_compound_reference_vectors(ctx):
    """all 126 cases of rdo_glue_ref.npz (4x4 .. 64x64, bd 8 / 10 / 12, REGULAR and SHARP, one full-pel reference
    per triple); `compound` is ONE call of the new entry point with pred_out only"""
    import rdo_glue_cases as RC
    from rav1e_amd import rdo_glue as RG
    G = np.load(RC.GOLD)
    cache = {}

    def compound(bd, filt, refs, w, h, p0, p1):
        key = id(refs[0])
        if key not in cache:
            cache.clear()
            cache[key] = (refs, [dev_plane(p) for p in refs])   # holds refs: the id cannot be reused
        d0, d1 = cache[key][1]
        c = RG.compound_cands(0, 0, [(0, 0)], [(0, 0)], filt)
        for i, (x, y, cf, rf) in enumerate((p0, p1)):
            c["rx%d" % i], c["ry%d" % i], c["col_frac%d" % i], c["row_frac%d" % i] = x, y, cf, rf
        o = ctx.rdo_compound_cand_batch(d0, d0, d1, w, h, c, want_satd=False, want_pred=True)
        assert sorted(o) == ["pred"]
        return o["pred"].cpu().numpy().view(px_dtype(bd))
    assert RC.check_compound(G, compound) == 3 * 2 * 21


# ---- 2. parity with the oracle composition ----
@pytest.fixture(scope="module", params=list(K.COMPOUND_DEPTHS))
def random_planes(request):
    bd = request.param
    rng = np.random.default_rng(1000 + bd)
    hps = [O.HostPlane(PW, PH, bd, PAD, PAD, rng=rng) for _ in range(3)]
    return hps, [dev_plane(p) for p in hps]


def test_compound_parity_random(ctx, oracle, random_planes):
    """pred, SAD and SATD equal to the oracle's, every size x n; every output combination at n = 5"""
    planes, dplanes = random_planes
    rng = np.random.default_rng(7 + planes[0].bit_depth)
    k = 0
    for (w, h) in SIZES:
        for n in NS:
            c = make_cands(rng, w, h, n, k)
            k += 1
            check_all(ctx, oracle, planes, dplanes, w, h, c, EACH if n == 5 else ALL3)


@pytest.mark.parametrize("bd", list(K.COMPOUND_DEPTHS))
def test_compound_parity_saturated(ctx, oracle, bd):
    """PREP_BIAS and the final clamp: references that are all `max`, and a 0 / max checkerboard (the sharpest
    overshoot both filter passes can produce), in the three pairings"""
    mx = (1 << bd) - 1
    rng = np.random.default_rng(50 + bd)
    org = O.HostPlane(PW, PH, bd, PAD, PAD, rng=rng)
    full = O.HostPlane(PW, PH, bd, PAD, PAD, fill=mx)
    chk = O.HostPlane(PW, PH, bd, PAD, PAD)
    yy, xx = np.indices(chk.data.shape)
    chk.data[...] = ((xx + yy) & 1) * mx
    dev = {id(p): dev_plane(p) for p in (org, full, chk)}
    k = 0
    for (r0, r1) in ((full, full), (chk, chk), (full, chk)):
        for (w, h) in SIZES:
            c = make_cands(rng, w, h, 5, k)
            k += 1
            check_all(ctx, oracle, (org, r0, r1), (dev[id(org)], dev[id(r0)], dev[id(r1)]), w, h, c, ALL3)


def test_compound_non_block_size(ctx, oracle, random_planes):
    """a (w, h) r1_mc_prep_batch takes that is no BlockSize: the prediction matches, a distortion is refused"""
    from rav1e_amd.api import R1Error
    planes, dplanes = random_planes
    bd = planes[0].bit_depth
    rng = np.random.default_rng(99)
    for (w, h) in ((16, 6), (8, 2), (32, 100), (4, 64)):
        c = make_cands(rng, w, h, 9, w + h)
        pred, _, _ = oracle_compound(oracle, *planes, w, h, c, dists=False)
        o = ctx.rdo_compound_cand_batch(*dplanes, w, h, c, want_satd=False, want_pred=True)
        assert np.array_equal(gpu_outs(o, bd)["pred"], pred), (bd, w, h)
        for kw in (dict(want_satd=True), dict(want_sad=True, want_satd=False)):
            with pytest.raises(R1Error, match=r"\(-1\)"):
                ctx.rdo_compound_cand_batch(*dplanes, w, h, c, want_pred=True, **kw)


# ---- 3. the prediction feeds the dense-prediction chain ----
@pytest.mark.parametrize("size", [16, 8])
def test_compound_pred_chain(ctx, size):
    """pred_out -> r1_rdo_pred_cand_batch (cdef_dist, qindex 100) against the same call on prep x 2 -> avg"""
    import torch
    from rav1e_amd.api import RDO_CAND
    bd, n, w, h = 10, 33, size, size
    rng = np.random.default_rng(300 + size)
    hps = [O.HostPlane(PW, PH, bd, PAD, PAD, rng=rng) for _ in range(3)]
    d_org, d0, d1 = [dev_plane(p) for p in hps]
    c = make_cands(rng, w, h, n, 0)
    new = ctx.rdo_compound_cand_batch(d_org, d0, d1, w, h, c, want_satd=False, want_pred=True)["pred"]
    old = ctx.mc_avg_batch(ctx.prep_8tap_batch(d0, w, h, mc_cands(c, 0)), ctx.prep_8tap_batch(d1, w, h, mc_cands(c, 1)),
                           w, h, bd)
    assert torch.equal(new, old)
    rc = np.zeros(n, RDO_CAND)
    rc["ox"], rc["oy"] = c["ox"], c["oy"]
    outs = [ctx.rdo_pixel_cand_batch(d_org, None, w, h, rc, 100, 3, pred=p, want_qcoeffs=True, want_rec=True)
            for p in (new, old)]
    for k in ("eob", "dist", "sad", "satd", "qcoeffs", "rec"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert int(outs[0]["eob"].max()) > 0        # the chain quantized something


# ---- 4. the compound leg of the inter mode pre-screen ----
def test_compound_prescreen_leg(ctx, oracle):
    """per block 5 single-reference SATDs (r1_rdo_cand_batch) and 8 compound SATDs (the new entry point) in mode-set
    order -> r1_prescreen_select_batch(keep_head 0, k 9) = a stable argsort of the oracle's SATDs, cut to 9"""
    import torch
    from rav1e_amd.api import RDO_CAND
    bd, w, h, nb, ns, ncp, k = 8, 16, 16, 12, 5, 8, 9
    rng = np.random.default_rng(4)
    hps = [O.HostPlane(PW, PH, bd, PAD, PAD, rng=rng) for _ in range(3)]
    d_org, d0, d1 = [dev_plane(p) for p in hps]
    bx, by = rng.integers(0, PW - w + 1, nb), rng.integers(0, PH - h + 1, nb)
    sc = np.zeros(nb * ns, RDO_CAND)
    sc["ox"], sc["oy"] = np.repeat(bx, ns), np.repeat(by, ns)
    sc["rx"], sc["ry"] = sc["ox"] + rng.integers(-8, 9, nb * ns), sc["oy"] + rng.integers(-8, 9, nb * ns)
    sc["col_frac"], sc["row_frac"] = rng.integers(0, 16, nb * ns), rng.integers(0, 16, nb * ns)
    cc = make_cands(rng, w, h, nb * ncp, 0)
    cc["ox"], cc["oy"] = np.repeat(bx, ncp), np.repeat(by, ncp)
    cc[3 * ncp + 5] = cc[3 * ncp + 2]            # two identical candidates in block 3: a tie
    # oracle keys
    want_s = np.zeros(nb * ns, np.uint32)
    po, p0 = hps[0].cstruct(), hps[1].cstruct()
    assert oracle.r1o_rdo_cand_batch(C.byref(po), C.byref(p0), w, h, 2, O.ptr(sc), nb * ns, None, O.ptr(want_s),
                                     None, None) == 0
    _, _, want_c = oracle_compound(oracle, *hps, w, h, cc)
    assert want_c[3 * ncp + 5] == want_c[3 * ncp + 2]
    want_keys = np.concatenate([want_s.reshape(nb, ns), want_c.reshape(nb, ncp)], axis=1)
    want_idx = np.argsort(want_keys, axis=1, kind="stable")[:, :k]
    # device
    s = ctx.rdo_cand_batch(d_org, d0, w, h, sc, want_sad=False, want_satd=True, want_coeffs=False)["satd"]
    cp = ctx.rdo_compound_cand_batch(d_org, d0, d1, w, h, cc)["satd"]
    keys = torch.cat([s.view(nb, ns), cp.view(nb, ncp)], dim=1).contiguous()
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want_keys)
    idx = ctx.prescreen_select_batch(keys.view(-1), ns + ncp, 0, k).cpu().numpy()
    assert np.array_equal(idx, want_idx)
    row = list(idx[3])
    if 5 + 2 in row and 5 + 5 in row:
        assert row.index(5 + 2) < row.index(5 + 5)     # the tie keeps the list order


# ---- 5. argument checks on a live context ----
def test_compound_argument_checks(ctx):
    """every refusal is R1_EINVAL from the host-side checks, before any launch, and writes nothing"""
    import torch
    from rav1e_amd.api import COMPOUND_CAND, _dev_cands
    rng = np.random.default_rng(5)
    p8 = [dev_plane(O.HostPlane(PW, PH, 8, PAD, PAD, rng=rng)) for _ in range(3)]
    p10 = dev_plane(O.HostPlane(PW, PH, 10, PAD, PAD, rng=rng))
    n = 4
    c = np.zeros(n, COMPOUND_CAND)
    c["ox"] = c["oy"] = c["rx0"] = c["ry0"] = c["rx1"] = c["ry1"] = 8
    dc, _ = _dev_cands(c, COMPOUND_CAND)
    sad = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    satd = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    pred = torch.full((n, 256, 256), 0x5a, dtype=torch.uint8, device="cuda")    # room for the largest rejected size
    f = ctx.lib.r1_rdo_compound_cand_batch

    def call(org, r0, r1, w, h, cnt, outs=(sad, satd, pred), cands=dc):
        s = [pl.cstruct() for pl in (org, r0, r1)]
        rc = f(ctx.h, C.byref(s[0]), C.byref(s[1]), C.byref(s[2]), w, h, cands.data_ptr() if cands is not None else None,
               cnt, *[o.data_ptr() if o is not None else None for o in outs], None)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((sad == 0x5a5a5a5a).all()) and bool((satd == 0x5a5a5a5a).all()) and bool((pred == 0x5a).all())
    assert call(p8[0], p8[1], p10, 16, 16, n) == -1 and untouched()            # bit depth of ref1
    assert call(p8[0], p8[1], p8[2], 2, 16, n) == -1 and untouched()           # w = 2
    assert call(p8[0], p8[1], p8[2], 256, 16, n) == -1 and untouched()         # w = 256
    assert call(p8[0], p8[1], p8[2], 16, 7, n, (None, None, pred)) == -1 and untouched()   # odd h
    assert call(p8[0], p8[1], p8[2], 16, 16, n, (None, None, None)) == -1 and untouched()  # no output
    assert call(p8[0], p8[1], p8[2], 16, 16, n, cands=None) == -1 and untouched()          # no list
    assert call(p8[0], p8[1], p8[2], 16, 16, 0) == 0 and untouched()           # n = 0: nothing to do
    assert call(p8[0], p8[1], p8[2], 16, 16, n) == 0 and not untouched()       # and the accepted call does write

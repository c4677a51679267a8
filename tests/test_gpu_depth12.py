"""The kernel paths that exist only for 12-bit pixels, launched on the GPU and held bit for bit to the reference-executed
fixtures (me_ref_12.npz, lookahead_ref_12.npz) and to the CPU oracle:
  * the motion search: the tile kernels in launch modes 1 / 2 / 3 and both block kernels, whose 8x8 .. 16x16 sub-pel
    SATD must take the i32 Hadamard (cand_common.hpp::satd_column packs two i16 only up to 10 bits), on the fixture and
    on planes of 0 / 4095 on which the packed path, wrongly taken, leaves the i16 range;
  * the fused intra candidate at every size whose 12-bit instantiation no other test launches, on both routes
    (rdo_cand_plan.hpp::rdo_intra_route) wherever a size has both;
  * the four k_intra_split<12, TL> (with the 16x16 / 8x8 case of test_gpu_rdo_intra_split.py);
  * the lookahead cost maps on the 12-bit frames of lookahead_ref_12.npz.
Every case holds pixel values above 1023 and a result that is not its initial state."""
import os
import subprocess

import numpy as np
import pytest

import cand_size_cases as K
import oracle_lib as O
import test_gpu_rdo_intra as RI
import test_gpu_rdo_intra_split as SP
import test_oracle_me_ref as MR
from test_gpu_parity import _me_dev_pyr, _me_stats_numpy, _me_stats_tensor, dev_plane

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BD, MX = 12, 4095
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)     # the cost of a block the launch was not sized for


def _block_cands(blk):
    c = np.zeros(len(blk), O.ME_BLOCK_CAND)
    c["bx"], c["by"], c["w"], c["h"], c["corner"] = blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3], blk[:, 4]
    c["pmv"] = blk[:, 5:9].reshape(-1, 2, 2)
    return c


def _fractional(res):
    """block results with a vector component off the full-pel grid (vectors are in 1/8 pel)"""
    return ((res["row"] | res["col"]) & 7) != 0


# ------------------------------------------------ motion estimation: the reference-executed fixture
@pytest.fixture(scope="module")
def d0():
    """case d0 of me_ref_12.npz on the device, made once"""
    c = MR.load_case("d0")
    assert c["bd"] == BD and len(c["refs"]) == 1
    pyr, prev, want = c["refs"][0]
    assert min(int(c["org"][0].view().max()), int(pyr[0].view().max())) > 1023
    c.update(dorg=_me_dev_pyr(c["org"]), dref=_me_dev_pyr(pyr), prev=prev, want=want,
             cols=(c["w"] + 3) // 4, rows=(c["h"] + 3) // 4)
    return c


@pytest.mark.parametrize("launch_mode", [1, 2, 3])
def test_me_ref_12_tile_motion(ctx, d0, launch_mode):
    """r1_estimate_tile_motion_batch at launch boundaries (1) and as the persistent launch, pinned (2) and not (3),
    on what the reference's estimate_tile_motion produced: every MEStats entry"""
    init = np.zeros_like(d0["want"])
    assert (d0["want"] != init).any()
    st = _me_stats_tensor(init)
    job = dict(org=d0["dorg"], ref=d0["dref"], stats=st, prev=_me_stats_tensor(d0["prev"]), tile=d0["tile"])
    ctx.estimate_tile_motion([job], d0["cols"], d0["rows"], BD, d0["lam"], allow_hp=bool(d0["hp"]),
                             allow_full_search=bool(d0["full"]), me_range_scale=d0["scale"], launch_mode=launch_mode)
    ok, first_failed, calls = ctx.me_status(wait=True)        # no dependency wait ran out of patience
    assert ok and first_failed == 0 and calls >= 1, (ok, first_failed, calls)
    got = _me_stats_numpy(st)
    bad = np.argwhere(got != d0["want"])
    assert len(bad) == 0, (launch_mode, len(bad), bad[:4], got[tuple(bad[0])], d0["want"][tuple(bad[0])])


@pytest.mark.parametrize("kernel", ["k_me_blocks", "k_me_blocks_small"])
def test_me_ref_12_block_searches(ctx, d0, kernel):
    """r1_estimate_motion_batch on what the reference's estimate_motion produced, (mv, sad, cost) of every block:
    without max_w / max_h (one workgroup per block) and sized for 16x16 (one wave per block; the larger blocks of
    the list come back empty)"""
    from rav1e_amd.api import ME_RESULT
    blk, want = MR.REF["d0_blk"], MR.REF["d0_blkout"]
    use_satd, fmode = [int(v) for v in MR.REF["d0_blkcfg"]]
    c = _block_cands(blk)
    job = dict(org=d0["dorg"], ref=d0["dref"], stats=_me_stats_tensor(d0["want"]), prev=_me_stats_tensor(d0["prev"]),
               tile=d0["tile"])
    kw = dict(max_w=16, max_h=16) if kernel == "k_me_blocks_small" else {}
    got = ctx.estimate_motion_batch(job, c, d0["cols"], d0["rows"], BD, d0["lam"], use_satd=bool(use_satd),
                                    filter_mode=fmode, allow_hp=bool(d0["hp"]), **kw).cpu().numpy().view(ME_RESULT)
    fits = (c["w"] <= 16) & (c["h"] <= 16) if kw else np.ones(len(c), bool)
    assert {(8, 8), (16, 8), (8, 16), (16, 16)} <= {(int(w), int(h)) for w, h in zip(c["w"][fits], c["h"][fits])}
    assert (got["cost"][~fits] == NONE).all()
    n_frac = 0
    for i in np.nonzero(fits)[0]:
        g = (int(got["row"][i]), int(got["col"][i]), int(got["sad"][i]), int(got["cost"][i]))
        assert g == tuple(int(v) for v in want[i]), (kernel, i, blk[i], g, want[i])
        n_frac += int(want[i][0] & 7 != 0 or want[i][1] & 7 != 0)
    assert d0["hp"] and n_frac > 0           # the sub-pel diamond moved a block


# ------------------------------------------------ motion estimation: the amplitude limit
AW, AH, AX = 128, 64, 64       # the tile; columns [0, AX) hold the extreme part


def amplitude_planes():
    """org / ref of 128 x 64 at 12 bits.  Left half, `ref` the complement of `org` throughout (|org - ref| = 4095):
    flat 4095 over flat 0, a one-pixel checkerboard and a checkerboard of 8x8 cells.  Right half: smooth texture, the
    reference displaced by a half-pel amount plus noise, so that the searches still move."""
    rng = np.random.default_rng(1212)
    f = rng.standard_normal((AH + 64, AW + 64))
    for _ in range(3):
        f = (np.roll(f, 1, 0) + 2 * f + np.roll(f, -1, 0)) / 4
        f = (np.roll(f, 1, 1) + 2 * f + np.roll(f, -1, 1)) / 4
    f = ((f - f.min()) / (f.max() - f.min()) * MX).astype(np.int64)
    org = f[32:32 + AH, 32:32 + AW].copy()
    ref = np.clip(f[32 + 3:32 + 3 + AH, 32 - 5:32 - 5 + AW] + rng.integers(-40, 41, (AH, AW)), 0, MX)
    ref = (ref + np.roll(ref, 1, 1) + 1) >> 1
    yy, xx = np.mgrid[0:AH, 0:AX]
    ext = np.zeros((AH, AX), np.int64)
    ext[:32, :32] = MX                                           # flat halves in opposite phase
    ext[:32, 32:] = MX * ((xx[:32, 32:] + yy[:32, 32:]) & 1)
    ext[32:, 32:] = MX * (((xx[32:, 32:] >> 3) + (yy[32:, 32:] >> 3)) & 1)
    org[:, :AX], ref[:, :AX] = ext, MX - ext
    return org, ref


def packed_stage_max(d):
    """the largest magnitude in front of the last butterfly of satd_column's packed 8x8 Hadamard of the 8x8 residual
    `d`: the three vertical stages and the lane stages with masks 1 and 2 (a 4-point Hadamard over each half of a
    row); the stage after it is folded into max(|a|, |b|).  Up to 10 bits this is at most 32 * 1023 < 2^15."""
    h2 = np.array([[1, 1], [1, -1]])
    h4 = np.kron(h2, h2)
    return int(np.abs(np.kron(h2, h4) @ d @ np.kron(np.eye(2, dtype=np.int64), h4)).max())


_amp = {}


def _amp_case(ctx, oracle):
    """planes, the oracle's tile statistics and the block list of the amplitude tests, made once"""
    if _amp:
        return _amp
    from rav1e_amd.api import me_lambdas
    org, ref = amplitude_planes()
    assert int(org.max()) == MX and int(ref.max()) == MX
    po, pr = O.me_pyramid(org, BD), O.me_pyramid(ref, BD)
    lam = me_lambdas(30.0 * 16)          # the 8-bit tests' value at the 12-bit scale of the distortions
    init = np.zeros((AH // 4, AW // 4), O.ME_STATS)
    want = init.copy()
    O.me_oracle(oracle, po, pr, AW // 4, AH // 4, (0, 0, AW, AH), BD, lam, want)
    assert (want != init).any()
    # 8 blocks of each of the four sizes in the extreme part, 4 of each in the texture
    rng = np.random.default_rng(5)
    sizes = [(8, 8), (16, 8), (8, 16), (16, 16)]
    c = np.zeros(48, O.ME_BLOCK_CAND)
    for i in range(len(c)):
        bw, bh = sizes[i % 4]
        c["w"][i], c["h"][i] = bw, bh
        c["bx"][i] = rng.integers(0, (AX - bw) // 4 + 1) if i < 32 else rng.integers(AX // 4, (AW - bw) // 4 + 1)
        c["by"][i] = rng.integers(0, (AH - bh) // 4 + 1)
        c["corner"][i] = rng.choice([0, 1, 3, 5, 7])
        c["pmv"][i] = rng.integers(-40, 41, (2, 2))
    # these inputs are ones on which the 10-bit packed path gives another number: in every block of the extreme
    # part some 8x8 tile of org - ref leaves the i16 range before the packed Hadamard's last stage
    d = org - ref
    for i in range(32):
        x, y, bw, bh = int(c["bx"][i]) * 4, int(c["by"][i]) * 4, int(c["w"][i]), int(c["h"][i])
        assert x + bw <= AX
        m = max(packed_stage_max(d[y + ty:y + ty + 8, x + tx:x + tx + 8]) for ty in range(0, bh, 8) for tx in range(0, bw, 8))
        assert m > 32767, (i, m)
    _amp.update(po=po, pr=pr, dpo=_me_dev_pyr(po), dpr=_me_dev_pyr(pr), lam=lam, init=init, want=want, cands=c)
    return _amp


@pytest.mark.parametrize("launch_mode", [1, 2])
def test_amplitude_limit_tile_motion(ctx, oracle, launch_mode):
    a = _amp_case(ctx, oracle)
    st = _me_stats_tensor(a["init"])
    ctx.estimate_tile_motion([dict(org=a["dpo"], ref=a["dpr"], stats=st, tile=(0, 0, AW, AH))], AW // 4, AH // 4, BD,
                             a["lam"], launch_mode=launch_mode)
    assert ctx.me_status(wait=True)[0]
    got = _me_stats_numpy(st)
    bad = np.argwhere(got != a["want"])
    assert len(bad) == 0, (launch_mode, len(bad), bad[:4], got[tuple(bad[0])], a["want"][tuple(bad[0])])


@pytest.mark.parametrize("use_satd", [1, 0])
def test_amplitude_limit_block_searches(ctx, oracle, use_satd):
    """8x8, 16x8, 8x16, 16x16 through k_me_blocks and k_me_blocks_small against oracle/me.c; with SATD the residuals of
    the extreme part reach 32 * 4095 inside the Hadamard"""
    from rav1e_amd.api import ME_RESULT
    a = _amp_case(ctx, oracle)
    c = a["cands"]
    want = O.me_block_oracle(oracle, a["po"], a["pr"], AW // 4, AH // 4, (0, 0, AW, AH), BD, a["lam"], a["want"], None, c,
                             use_satd=use_satd, filter_mode=0, allow_hp=1)
    assert _fractional(want[:32]).any() and _fractional(want[32:]).any()
    assert int(want["sad"][:32].max()) > 32767
    job = dict(org=a["dpo"], ref=a["dpr"], stats=_me_stats_tensor(a["want"]), tile=(0, 0, AW, AH))
    for kw in ({}, dict(max_w=16, max_h=16)):
        got = ctx.estimate_motion_batch(job, c, AW // 4, AH // 4, BD, a["lam"], use_satd=bool(use_satd), filter_mode=0,
                                        allow_hp=True, **kw).cpu().numpy().view(ME_RESULT)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (use_satd, kw, len(bad), c[bad[0]], got[bad[0]], want[bad[0]])


# ------------------------------------------------ lookahead cost maps: the reference-executed fixture
def test_lookahead_ref_12_cost_maps(ctx):
    """estimate_intra_costs, importance_block_difference and the cost loop of estimate_inter_costs on the 12-bit frames
    of lookahead_ref_12.npz (dc = 128 << 4, SATD normalisation)"""
    import torch
    G = np.load(os.path.join(GOLD, "lookahead_ref_12.npz"))
    assert len(G["keys"]) == 2
    for k in G["keys"]:
        k = str(k)
        bd, w, h = [int(v) for v in k.split("_")[:3]]
        assert bd == BD and int(G["org_" + k].max()) > 1023 and int(G["ref_" + k].max()) > 1023
        hb, wb = h // 8, w // 8
        do = dev_plane(O.plane_from_image(G["org_" + k], bd, 16, 16))
        dr = dev_plane(O.plane_from_image(G["ref_" + k], bd, 16, 16))
        intra = ctx.estimate_intra_costs(do).cpu().numpy().view(np.uint32)
        assert intra.any() and np.array_equal(intra, G["intra_" + k]), k
        assert ctx.importance_block_difference(do, dr) == float(G["blockdiff_" + k][0]), k
        mvs = torch.from_numpy(np.ascontiguousarray(G["mv_" + k])).cuda()
        inter = ctx.estimate_inter_costs(do, dr, mvs).cpu().numpy().view(np.uint32)
        assert inter.any() and int(inter.astype(np.uint64).sum()) / (wb * hb) == float(G["inter_mean_" + k][0]), k


# ------------------------------------------------ the fused intra candidate, every 12-bit instantiation
# TxSize ids: 4x4, 32x32, 64x64, 4x16, 16x4, 16x64 and the pair 8x16 / 16x8 (8x8 and 16x16 are cases of
# test_gpu_rdo_intra.py at 12 bits)
INTRA_SIZES = K.DEPTH12_INTRA_SIZES
KINDS = K.INTRA_KINDS                # the three distortion kinds; dist_kind 0 is QM 1 of the plan, the others QM 2
TWO_LAUNCH = 2


@pytest.fixture(scope="module")
def intra_route(tmp_path_factory):
    """{(bit depth, log2 w, log2 h, QM): route} as rdo_intra_route itself answers (tests/c/rdo_intra_route_list.cpp,
    the host compiler alone)"""
    exe = str(tmp_path_factory.mktemp("rdo_route") / "rdo_intra_route_list")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "rav1e_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "rdo_intra_route_list.cpp")])
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe], text=True).splitlines()]
    assert len(rows) == 3 * 19 * 2
    return {r[:4]: r[4] for r in rows}


def _routes(intra_route, ts, kinds):
    w, h = RI.TX_DIMS[ts]
    return {intra_route[BD, w.bit_length() - 1, h.bit_length() - 1, 1 if kind == 0 else 2] for kind in kinds}


def test_every_12_bit_size_with_both_routes_is_among_the_cases(intra_route):
    both = [ts for ts in range(19) if TWO_LAUNCH in _routes(intra_route, ts, KINDS) and len(_routes(intra_route, ts, KINDS)) > 1]
    assert both, "no size has a fused and a two-launch point at 12 bits: the cases below prove less than they say"
    assert set(both) <= set(INTRA_SIZES), both
    # and where 12 bits has no fused point at all, the case is one of test_gpu_rdo_intra.py
    only_two = [ts for ts in range(19) if _routes(intra_route, ts, KINDS) == {TWO_LAUNCH}]
    assert set(only_two) <= {ts for ts, bd in RI.CASES if bd == BD}, only_two


@pytest.mark.parametrize("ts", INTRA_SIZES)
def test_intra_cand_12_bit_instantiations(ctx, oracle, intra_route, ts):
    """check_call of test_gpu_rdo_intra.py (the fused call against the two-launch device route and the oracle's
    composition) with n = NC + 1 candidates, one ragged wave: the three distortion kinds x edge_group 1 and 5"""
    w, h = RI.TX_DIMS[ts]
    nc = 64 // max(w, h)
    rec, org = SP._planes(BD, 1200 + ts)          # predictions near the source
    assert min(int(rec.view().max()), int(org.view().max())) > 1023
    # the block at the origin (in every call, DC_PRED first) is what DC_PRED gives without neighbours: eob 0 there
    rec.view()[:64, :64] = org.view()[:64, :64] = 128 << (BD - 8)
    drec, dorg = dev_plane(rec), dev_plane(org)
    rng = np.random.default_rng(1250 + ts)
    scales = rng.integers(1 << 12, 1 << 16, ((org.height + h + 7) // 8, (org.width + w + 7) // 8)).astype(np.uint32)
    dscales = RI._t(scales.view(np.int32))
    side = max(w, h)
    masks = [ctx.tx_type_mask(ts, False), 1 << 9] if side <= 16 else ([1, 0x201] if side == 32 else [1])
    eobs, taken = [], set()
    for step, (kind, group) in enumerate((k, g) for g in (1, 5) for k in KINDS):
        n = nc + 1 if group == 1 else (nc + 1 + 4) // 5 * 5
        mask, qi = masks[step % len(masks)], (60, 140, 255)[(step + step // 3) % 3]
        cs = RI.make_case(rng, ctx, rec, drec, ts, n, group)
        use_sc = step % 2 == 0
        eobs.append(RI.check_call(ctx, oracle, org, dorg, ts, BD, cs, group, mask, qi, kind, scales if use_sc else None,
                                  dscales if use_sc else None, 0, 0, step != 4,
                                  (ts, BD, n, group, kind, hex(mask), qi)).ravel())
        taken |= _routes(intra_route, ts, (kind,))
    # a size with a fused and a two-launch point at 12 bits went through one of each
    assert taken == _routes(intra_route, ts, KINDS)
    eobs = np.concatenate(eobs)
    assert (eobs == 0).any() and (eobs != 0).any(), (ts, int((eobs == 0).sum()), len(eobs))


# ------------------------------------------------ the intra transform split, the four k_intra_split<12, TL>
@pytest.mark.parametrize("bw,bh,ts", [(8, 8, 0), (32, 32, 2), (64, 64, 3), (64, 64, 2)])
def test_intra_split_12_bit_instantiations(ctx, oracle, bw, bh, ts):
    """the body of test_one_launch_equals_device_and_oracle_compositions (its assertions, zero and non-zero eob among
    them) at 12 bits: transform sides 4, 16 and 32; with its own (16, 16, TX_8X8, 12) all four sides are launched"""
    assert (bw, bh, ts, BD) not in SP.CASES
    rec, org = SP._planes(BD, 6100 + 100 * ts + bw + BD)      # the planes that body makes
    assert min(int(rec.view().max()), int(org.view().max())) > 1023
    SP.test_one_launch_equals_device_and_oracle_compositions(ctx, oracle, bw, bh, ts, BD)

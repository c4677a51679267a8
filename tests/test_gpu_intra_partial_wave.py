"""k_intra_predict with waves whose last candidate slots are dead while live lanes filter edges: the edge filter /
upsampler holds workgroup barriers that the dead lanes must reach too.  3 blocks x the 13 luma modes at every fixed
instantiation (4x4, 8x8, 16x16, 32x32) and the generic one (16x8), through both entry points that launch the kernel,
bit for bit against the oracle's r1o_dispatch_predict_intra (-> r1o_get_satd) on the same edge buffers:
  * r1_predict_intra_batch on the 39 candidates: 64 / W = 16, 8, 4, 2 divides none of 39, the last wave is ragged;
  * r1_intra_satd_batch with group = 13: a wave has 64 / W block slots, 3 of its 16, 8 or 4 live, and at 32x32 (2
    slots) the second wave of every mode has one."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SIZES = {0: (4, 4), 1: (8, 8), 2: (16, 16), 3: (32, 32), 8: (16, 8)}     # tx_size -> (w, h)
NB = 3
BASE = [0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0]
_cases = {}


def _case(ctx, oracle, bd, ts):
    """the candidates, the device edge sets and the oracle's predictions and SATDs of one (bit depth, size), made once"""
    key = (bd, ts)
    if key in _cases:
        return _cases[key]
    import torch
    from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND, Plane
    w, h = SIZES[ts]
    rng = np.random.default_rng(7100 + 16 * ts + bd)
    rec = O.HostPlane(96, 64, bd, rng=rng)
    src = O.HostPlane(96, 64, bd, rng=rng)
    drec = Plane.from_numpy(rec.data, rec.width, rec.height, bd, rec.xpad, rec.ypad)
    dsrc = Plane.from_numpy(src.data, src.width, src.height, bd, src.xpad, src.ypad)
    assert bd != 12 or min(int(rec.view().max()), int(src.view().max())) > 1023   # 12-bit data, not 10
    hbd = int(bd > 8)
    dt = np.uint16 if hbd else np.uint8
    bxs, bys = np.array([0, w, 0]), np.array([0, 0, h])      # the origin, the top row, the left column
    ec = np.zeros(NB, INTRA_EDGE_CAND)
    ec["x"], ec["y"] = bxs, bys
    ec["mode"] = -1                                           # IntraParam::None: the modes of a block share one set
    ec["flags"] = 1 | (rng.integers(0, 4, NB) << 1)
    edges, lens = ctx.intra_edges_batch(drec, (0, 0, rec.width, rec.height), ts, ec)
    he, hl = edges.cpu().numpy().view(dt), lens.cpu().numpy()
    var = np.where((bxs == 0) & (bys == 0), 0, np.where(bys == 0, 1, np.where(bxs == 0, 2, 3)))
    pm = np.tile(np.arange(13), NB)
    v13 = np.repeat(var, 13)
    # PAETH without both neighbours falls back (PredictionMode::predict_intra, predict.rs:116-140)
    pm = np.where((pm == 12) & (v13 == 0), 0, np.where((pm == 12) & (v13 == 2), 1,
                  np.where((pm == 12) & (v13 == 1), 2, pm)))
    angle = np.array(BASE)[pm]
    ief = np.where((pm >= 1) & (pm <= 8), rng.integers(1, 3, 13 * NB), 0)
    ic = np.zeros(13 * NB, INTRA_CAND)
    ic["mode"], ic["variant"], ic["angle"], ic["ief"] = pm, v13, angle, ief
    ic["avail_w"], ic["avail_h"] = w, h
    wpred = np.zeros((13 * NB, h, w), dt)
    wsatd = np.zeros(13 * NB, np.uint32)
    for i in range(13 * NB):
        b = i // 13
        assert oracle.r1o_dispatch_predict_intra(
            int(pm[i]), int(v13[i]), O.ptr(wpred[i]), w, ts, bd, None, int(angle[i]), int(ief[i]),
            O.ptr(he[b]), int(hl[b, 0]), int(hl[b, 1]), w, h, hbd) == 0
        wsatd[i] = oracle.r1o_get_satd(src.block_ptr(int(bxs[b]), int(bys[b])), src.stride, O.ptr(wpred[i]), w, w, h,
                                       hbd)
    pos = torch.from_numpy(np.stack([bxs, bys], 1).astype(np.int16)).cuda()
    sets = torch.from_numpy(np.repeat(np.arange(NB), 13)).cuda()
    _cases[key] = dict(ic=ic, dsrc=dsrc, edges=edges, lens=lens, pos=pos, sets=sets, wpred=wpred, wsatd=wsatd, dt=dt)
    return _cases[key]


@pytest.mark.parametrize("ts", sorted(SIZES))
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_predict_intra_ragged_last_wave(ctx, oracle, bd, ts):
    cs = _case(ctx, oracle, bd, ts)
    assert len(cs["ic"]) % (64 // SIZES[ts][0]) != 0
    got = ctx.predict_intra_batch(ts, cs["ic"], cs["edges"][cs["sets"]].contiguous(),
                                  cs["lens"][cs["sets"]].contiguous(), bd)
    got = got.cpu().numpy().view(cs["dt"])
    bad = np.nonzero((got != cs["wpred"]).any(axis=(1, 2)))[0]
    assert len(bad) == 0, (bd, ts, [(int(i), int(cs["ic"]["mode"][i])) for i in bad])


@pytest.mark.parametrize("ts", sorted(SIZES))
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_intra_satd_three_blocks_per_wave(ctx, oracle, bd, ts):
    cs = _case(ctx, oracle, bd, ts)
    got = ctx.intra_satd_batch(cs["dsrc"], ts, cs["ic"], 13, cs["pos"], cs["edges"], cs["lens"])
    got = got.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != cs["wsatd"])[0]
    assert len(bad) == 0, (bd, ts, [(int(i), int(cs["ic"]["mode"][i]), int(got[i]), int(cs["wsatd"][i])) for i in bad])

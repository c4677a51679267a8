"""Every inverse-transform path of the device against tests/golden/inv_path_ref.npz: reconstructions the reference's
`encode_tx_block` produced when its text was executed whole (gen_inv_path_ref.py) on the blocks of fwd_tx_ref.npz at
qindex 1 and 255 -- the largest levels and the largest steps the quantizer can hand to dequantize ->
inverse_transform_add -> add -> pixel clamp.  No oracle stands between the kernels and these numbers.

  leg 0  r1_dequantize_batch: the stored levels -> the stored rcoeffs (families and split loop).
  leg 1  k_inv_tx: the stored rcoeffs, and all of inv_tx_ref.npz, tiled to the ragged counts of the forward test
         (67 blocks up to area 256 and 9 above, raised to the block count and kept off a multiple of the blocks a
         wave owns), once at the tight stride and once at coeff_stride = coded area + 5 with a pattern behind every
         block's coefficients.
  leg 2  the plain QM == 2 slice of k_rdo_cand: r1_rdo_pred_cand_batch with the dense prediction and
         r1_rdo_pixel_cand_batch with the prediction as a reference plane and zero fractions, one launch per
         (case, qindex), blocks tiled as in leg 1: eob, levels, reconstruction, and under R1_DIST_WSSE without a scale
         grid the distortion, which must be NumPy's sum of (src - rec)^2 over the fixture's reconstruction.
  leg 3  r1_rdo_txsearch_batch: the dense prediction and the full inter mask of the size, all types of a size in one
         launch, each slot compared with the case of its type: the sizes that fan out and those that take one launch
         per type (32- and 64-point sides, 32x64 / 64x32 with the rectangular scaling on the cut input).
  leg 4  r1_rdo_intra_cand_batch: the flat family, DC_PRED from the edges of a mid-grey plane, at the sizes where the
         call takes each of its three routes, with edge_group 1 and 2.
  leg 5  r1_rdo_intra_split_batch: the split-loop cases.

Each leg counts its (case, block) comparisons and asserts the total."""
import functools

import numpy as np
import pytest

import inv_path_ref_util as U
import oracle_lib as O
from test_gpu_parity import TX_SIZES, dev_plane

pytestmark = pytest.mark.gpu

NBLOCKS = 1750          # per bit depth: 1666 plain (98 of them with intra offsets), 84 flat
NPLAIN, NFLAT = 1666, 84
NSPLIT, NSPLIT_TX = 8, 32
INV_TX_REF_BLOCKS = 2382    # inv_tx_ref.npz: 471 cases of five blocks, 9 (above area 1024) of three
PATTERN = 0x5A5A


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pix(a, bd):
    """pixels as the device tensors hold them"""
    return np.ascontiguousarray(a).view(np.uint8 if bd == 8 else np.int16)


def _sse(src, rec):
    return ((src.astype(np.int64) - rec.astype(np.int64)) ** 2).reshape(len(src), -1).sum(1)


# ---------------------------------------------------------------------------------------------------- leg 0
@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_dequantize_kernel(ctx, bd):
    compared = 0
    groups = {}
    for b in U.load():
        if b.bd == bd:
            groups.setdefault((b.ts, b.qindex), []).append((b.qc, b.dq))
    for s in U.load_splits():
        if s.bd == bd:
            groups.setdefault((s.ts, s.qindex), []).extend(zip(s.qc, s.dq))
    for (ts, qindex), pairs in groups.items():
        qc, dq = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        got = ctx.dequantize_batch(_t(qc), ts, qindex, bd).cpu().numpy()
        bad = np.flatnonzero((got != dq).any(1))
        assert not len(bad), (bd, ts, qindex, bad[:8].tolist())
        compared += len(pairs)
    assert compared == NBLOCKS + NSPLIT_TX


# ---------------------------------------------------------------------------------------------------- leg 1
def _inv_tx_both_strides(ctx, co, pred, rec, ts, tt, bd, key):
    """co (nb, area), pred / rec (nb, h, w) -> one tiled launch per stride"""
    w, h = TX_SIZES[ts]
    nb, area = co.shape
    n = U.launch_count(w, h, nb)
    idx = U.tiled_index(nb, n)
    dpred = _t(_pix(pred[idx], bd))
    want = rec[idx]
    for pad in (0, 5):
        wide = np.full((n, area + pad), PATTERN, co.dtype)
        wide[:, :area] = co[idx]
        got = ctx.inverse_transform_add_batch(_t(wide), dpred, ts, tt, bd).cpu().numpy().view(rec.dtype)
        bad = np.flatnonzero((got != want).reshape(n, -1).any(1))
        assert not len(bad), (key, "coeff_stride", area + pad, [(int(i), int(idx[i])) for i in bad[:8]])
    return nb


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_inv_tx_kernel_on_reference_rcoeffs(ctx, bd):
    """the rcoeffs `dequantize` wrote in the executed run; all blocks of one (size, type) share a launch, whatever
    their family, qindex and offsets"""
    groups = {}
    for b in U.load():
        if b.bd == bd:
            groups.setdefault((b.ts, b.tt), []).append(b)
    compared = 0
    for (ts, tt), bl in groups.items():
        compared += _inv_tx_both_strides(ctx, np.stack([b.dq for b in bl]), np.stack([b.pred for b in bl]),
                                         np.stack([b.rec for b in bl]), ts, tt, bd, (bd, ts, tt))
    assert compared == NBLOCKS


def test_inv_tx_kernel_on_inv_tx_ref_at_its_block_mapping(ctx):
    """inv_tx_ref.npz (clamp-exercising coefficients no quantizer produces) at the launch shapes above: later slots of
    a wave, later waves, the tail, and a stride above the coded area"""
    import os
    with np.load(os.path.join(U.GOLD, "inv_tx_ref.npz")) as G:
        keys = [k for k in G.files if k.endswith("_co")]
        assert len(keys) == 480
        compared = 0
        for k in keys:
            _, ts, tt, bd, _ = k.split("_")
            compared += _inv_tx_both_strides(ctx, G[k], G[k[:-3] + "_pred"], G[k[:-3] + "_rec"], int(ts), int(tt),
                                             int(bd), k)
    assert compared == INV_TX_REF_BLOCKS


# ---------------------------------------------------------------------------------------------------- legs 2, 3
class _Size:
    """The distinct (source, prediction) pairs of one (bit depth, tx_size, family) as planes on the device, and the
    dense predictions."""

    def __init__(self, bd, ts, blocks):
        self.bd, self.ts = bd, ts
        self.w, self.h = TX_SIZES[ts]
        self.index = {}
        src, pred = [], []
        for b in blocks:
            k = (b.family, b.res.tobytes())
            if k not in self.index:
                self.index[k] = len(src)
                src.append(b.src)
                pred.append(b.pred)
        self.src, self.pred = np.stack(src), np.stack(pred)
        k = len(src)
        cols = 5
        rows = (k + cols - 1) // cols
        hs, hr = O.HostPlane(cols * self.w, rows * self.h, bd), O.HostPlane(cols * self.w, rows * self.h, bd)
        self.x, self.y = (np.arange(k) % cols) * self.w, (np.arange(k) // cols) * self.h
        for i in range(k):
            sl = (slice(self.y[i], self.y[i] + self.h), slice(self.x[i], self.x[i] + self.w))
            hs.view()[sl], hr.view()[sl] = self.src[i], self.pred[i]
        self.dsrc, self.dref = dev_plane(hs), dev_plane(hr)

    def of(self, b):
        return self.index[b.family, b.res.tobytes()]

    def cands(self, idx, tt):
        c = np.zeros(len(idx), O.RDO_CAND)
        c["ox"] = c["rx"] = self.x[idx]
        c["oy"] = c["ry"] = self.y[idx]
        c["tx_type"] = tt
        return c


@functools.lru_cache(maxsize=None)
def _sizes(bd):
    by = {}
    for b in U.load():
        if b.bd == bd:
            by.setdefault(b.ts, []).append(b)
    return {ts: _Size(bd, ts, bl) for ts, bl in by.items()}


def _check_slots(got_eob, got_qc, got_rec, got_dist, blocks, idx, src, key):
    """slot i of a launch holds blocks[idx[i]]"""
    n = len(idx)
    bad = np.flatnonzero(got_eob != np.array([blocks[i].eob for i in idx]))
    assert not len(bad), (key, "eob", [blocks[idx[i]].name for i in bad[:8]])
    bad = np.flatnonzero((got_qc != np.stack([blocks[i].qc for i in idx])).any(1))
    assert not len(bad), (key, "qcoeffs", [blocks[idx[i]].name for i in bad[:8]])
    want = np.stack([blocks[i].rec for i in idx])
    bad = np.flatnonzero((got_rec != want).reshape(n, -1).any(1))
    assert not len(bad), (key, "rec", [blocks[idx[i]].name for i in bad[:8]])
    bad = np.flatnonzero(got_dist.astype(np.int64) != _sse(src, want))
    assert not len(bad), (key, "dist", [blocks[idx[i]].name for i in bad[:8]])


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_fused_candidate_plain_slice(ctx, bd):
    """both prediction sources of the plain kernel per (case, qindex); the flat family through the dense one"""
    dt = U.pix_dtype(bd)
    dense = planar = 0
    for (family, _, ts, tt, qindex, is_intra), blocks in U.cases(bd=bd).items():
        s = _sizes(bd)[ts]
        n = U.launch_count(s.w, s.h, len(blocks))
        idx = U.tiled_index(len(blocks), n)
        at = np.array([s.of(blocks[i]) for i in idx])
        c = s.cands(at, tt)
        key = (family, bd, ts, tt, qindex, is_intra)
        for pred in ((_t(_pix(s.pred[at], bd)), None) if family == U.PLAIN else (_t(_pix(s.pred[at], bd)),)):
            o = ctx.rdo_pixel_cand_batch(s.dsrc, s.dref, s.w, s.h, c, qindex, 2, is_intra=is_intra, want_sad=False,
                                         want_satd=False, want_qcoeffs=True, want_rec=True, pred=pred)
            _check_slots(o["eob"].cpu().numpy().view(np.uint16), o["qcoeffs"].cpu().numpy(),
                         o["rec"].cpu().numpy().view(dt), o["dist"].cpu().numpy().view(np.uint64), blocks, idx,
                         s.src[at], key + ("dense" if pred is not None else "plane",))
            if pred is not None:
                dense += len(blocks)
            else:
                planar += len(blocks)
    assert (dense, planar) == (NBLOCKS, NPLAIN)


@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_type_search(ctx, bd):
    """one launch per (size, qindex, offsets) with the full inter mask: every distinct block of the size under every
    type; a slot is compared where the fixture holds that block under that type (the sign block of a type only
    under its own)"""
    dt = U.pix_dtype(bd)
    compared = 0
    by = {}
    for (family, _, ts, tt, qindex, is_intra), blocks in U.cases(U.PLAIN, bd).items():
        by.setdefault((ts, qindex, is_intra), {})[tt] = blocks
    for (ts, qindex, is_intra), per_type in by.items():
        s = _sizes(bd)[ts]
        mask = ctx.tx_type_mask(ts, True, rav1e_types_only=False)
        assert mask == sum(1 << tt for tt in per_type), (ts, hex(mask))
        distinct = sorted({s.of(b) for bl in per_type.values() for b in bl})
        n = U.launch_count(s.w, s.h, len(distinct))
        at = np.array(distinct)[U.tiled_index(len(distinct), n)]
        o = ctx.rdo_txsearch_batch(s.dsrc, None, s.w, s.h, s.cands(at, 0), mask, qindex, 2, is_intra=is_intra,
                                   want_qcoeffs=True, want_rec=True, pred=_t(_pix(s.pred[at], bd)))
        eob, dist = o["eob"].cpu().numpy().view(np.uint16), o["dist"].cpu().numpy().view(np.uint64)
        qc, rec = o["qcoeffs"].cpu().numpy(), o["rec"].cpu().numpy().view(dt)
        for tt, blocks in per_type.items():
            slot = bin(mask & ((1 << tt) - 1)).count("1")
            where = {s.of(b): j for j, b in enumerate(blocks)}
            rows = np.array([i for i in range(n) if at[i] in where])
            idx = np.array([where[at[i]] for i in rows])
            assert set(idx) == set(range(len(blocks)))
            _check_slots(eob[rows, slot], qc[rows, slot], rec[rows, slot], dist[rows, slot], blocks, idx, s.src[at[rows]],
                         (bd, ts, tt, qindex, is_intra))
            compared += len(blocks)
    assert compared == NPLAIN


# ---------------------------------------------------------------------------------------------------- leg 4
@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_intra_candidate_routes(ctx, bd):
    """the flat family: 8x8 fans out; 16x16 fans out at 8 bits and takes the two launches above; 32x32 takes one
    launch per type at 8 bits and the two launches above; 16x32 takes one launch per type"""
    from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND
    dt = U.pix_dtype(bd)
    mid = 1 << (bd - 1)
    compared = 0
    by = {}
    for (family, _, ts, tt, qindex, is_intra), blocks in U.cases(U.FLAT, bd).items():
        assert is_intra == 1
        by.setdefault((ts, qindex), {})[tt] = blocks
    assert {ts for ts, _ in by} == {1, 2, 3, 9}
    for (ts, qindex), per_type in by.items():
        w, h = TX_SIZES[ts]
        mask = ctx.tx_type_mask(ts, False, rav1e_types_only=False)
        assert mask == sum(1 << tt for tt in per_type), (ts, hex(mask))
        srcs, index = [], {}
        for bl in per_type.values():
            for b in bl:
                if b.res.tobytes() not in index:
                    index[b.res.tobytes()] = len(srcs)
                    srcs.append(b.src)
        k = len(srcs)
        # the blocks in a row, one block in from the plane's corner: both edges lie inside the mid-grey plane
        org, rec = O.HostPlane((k + 1) * w, 2 * h, bd, fill=mid), O.HostPlane((k + 1) * w, 2 * h, bd, fill=mid)
        for i, a in enumerate(srcs):
            org.view()[h:2 * h, (i + 1) * w:(i + 2) * w] = a
        dorg, drec = dev_plane(org), dev_plane(rec)
        for group in (1, 2):
            nblk = U.launch_count(w, h, k) if group == 1 else k
            blk = U.tiled_index(k, nblk)
            ec = np.zeros(nblk, INTRA_EDGE_CAND)
            ec["x"], ec["y"], ec["mode"] = (blk + 1) * w, h, 0 if group == 1 else -1
            edges, lens = ctx.intra_edges_batch(drec, (0, 0, rec.width, rec.height), ts, ec)
            n = nblk * group
            at = np.repeat(blk, group)
            ic = np.zeros(n, INTRA_CAND)
            ic["mode"], ic["variant"], ic["avail_w"], ic["avail_h"] = 0, 3, w, h
            pos = np.stack([ec["x"], ec["y"]], 1).astype(np.int16)
            o = ctx.rdo_intra_cand_batch(dorg, w, h, ic, _t(pos), edges, lens, mask, qindex, 2, edge_group=group,
                                         want_qcoeffs=True, want_rec=True, want_pred=True)
            assert (o["pred"].cpu().numpy().view(dt) == mid).all(), (bd, ts, qindex, group, "pred")
            eob, dist = o["eob"].cpu().numpy().view(np.uint16), o["dist"].cpu().numpy().view(np.uint64)
            qc, rcn = o["qcoeffs"].cpu().numpy(), o["rec"].cpu().numpy().view(dt)
            for tt, blocks in per_type.items():
                slot = bin(mask & ((1 << tt) - 1)).count("1")
                where = {index[b.res.tobytes()]: j for j, b in enumerate(blocks)}
                rows = np.array([i for i in range(n) if at[i] in where])
                idx = np.array([where[at[i]] for i in rows])
                assert set(idx) == set(range(len(blocks)))
                _check_slots(eob[rows, slot], qc[rows, slot], rcn[rows, slot], dist[rows, slot], blocks, idx,
                             np.stack([srcs[at[i]] for i in rows]), (bd, ts, tt, qindex, "edge_group", group))
                compared += len(blocks)
    assert compared == 2 * NFLAT


# ---------------------------------------------------------------------------------------------------- leg 5
@pytest.mark.parametrize("bd", U.BITDEPTHS)
def test_intra_split_loop(ctx, bd):
    """block k + 1 predicted from what block k left, in one launch: eob, levels, the block's reconstruction and the
    distortion of every case; the case sits in the second slot of a launch of three as well"""
    from rav1e_amd.rdo_glue import intra_split_cands
    dt = U.pix_dtype(bd)
    mid = 1 << (bd - 1)
    compared = txs = 0
    for s in U.load_splits():
        if s.bd != bd:
            continue
        key = (bd, s.bs, s.ts, s.tt, s.mode, s.qindex)
        org = O.HostPlane(s.plane_w, s.plane_h, bd, fill=mid)
        org.view()[s.y:s.y + s.bs, s.x:s.x + s.bs] = s.src
        rec = O.HostPlane(s.plane_w, s.plane_h, bd, fill=mid)
        dorg, drec = dev_plane(org), dev_plane(rec)
        zeros = [0] * s.ntx
        # around the case: the same block of the source predicted by DC from the plane's corner, and by another mode
        blocks = [(0, 0, 0, 0, 0, zeros, zeros), (s.x, s.y, s.mode, 0, 0, zeros, zeros),
                  (s.x, s.y, (s.mode + 1) % 3, 0, 0, zeros, zeros)]
        cands = intra_split_cands(blocks, s.bs, s.bs, s.ts)
        o = ctx.rdo_intra_split_batch(dorg, drec, (0, 0, s.plane_w, s.plane_h), s.bs, s.bs, s.ts, cands, 1 << s.tt,
                                      s.qindex, 2, enable_intra_edge_filter=False, want_qcoeffs=True, want_rec=True)
        assert np.array_equal(o["eob"].cpu().numpy().view(np.uint16)[1, 0], s.eob), (key, "eob")
        assert np.array_equal(o["qcoeffs"].cpu().numpy()[1, 0], s.qc), (key, "qcoeffs")
        got = o["rec"].cpu().numpy().view(dt)[1, 0]
        assert np.array_equal(got, s.rec), (key, "rec")
        assert int(o["dist"].cpu().numpy().view(np.uint64)[1, 0]) == int(_sse(s.src[None], s.rec[None])[0]), (key, "dist")
        compared += 1
        txs += s.ntx
    assert (compared, txs) == (NSPLIT, NSPLIT_TX)

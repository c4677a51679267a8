"""The semantics of r1_rdo_intra_split_batch (include/rav1e_amd.h) as a host loop over calls that exist without it:
per trial (block, transform type) a private copy R of the reconstructed plane, and for every transform block k in
raster order  get_intra_edges(R) -> predict_intra -> the transform-type search with the type forced -> the
reconstruction stored into R.  Two backends:

  oracle_split   r1o_get_intra_edges, r1o_predict_intra, r1o_rdo_txsearch_batch, r1o_dist_scaled_batch (the CPU oracle)
  device_split   r1_intra_edges_batch, r1_predict_intra_batch, r1_rdo_txsearch_batch and a torch scatter, step k of
                 every trial of a round in one launch each.  Trials share one scratch plane per round, so a round
                 holds only blocks that cannot see each other's pixels.

Both return the arrays of the one launch: eob (n, nt, ntx); dist (n, nt, ntx) and est_rate under dist_kind 0, dist
(n, nt) under a pixel-domain kind; qcoeffs (n, nt, ntx, coded area); rec (n, nt, bh, bw).
"""
import ctypes as C

import numpy as np

import oracle_lib as O

SPLIT_CAND = np.dtype([("x", "<i2"), ("y", "<i2"), ("mode", "u1"), ("angle_delta", "i1"), ("ief", "u1"),
                       ("reserved", "u1"), ("tr_mask", "<u2"), ("bl_mask", "<u2")])
TX_SIDE = {0: 4, 1: 8, 2: 16, 3: 32}


def type_slots(mask):
    return [t for t in range(16) if (mask >> t) & 1]


def tx_blocks(x, y, bw, bh, t, tile_w, tile_h):
    """[(k, x_k, y_k, skipped)] of the block at tile position (x, y): raster order over the bw/t x bh/t grid; a
    transform block whose 4x4-unit origin is at or beyond the tile's 4x4 grid is skipped (encoder.rs:1441, 2282)"""
    mi_w, mi_h = (tile_w + 3) >> 2, (tile_h + 3) >> 2
    out = []
    for j in range(bh // t):
        for i in range(bw // t):
            xk, yk = x + i * t, y + j * t
            out.append((j * (bw // t) + i, xk, yk, (xk >> 2) >= mi_w or (yk >> 2) >= mi_h))
    return out


def _avail(t, plane_size, pos):
    return min(t, max(1, plane_size - pos))


def _initial_block(rec, tile, x, y, bw, bh):
    """what no step writes: `rec` inside the tile, 0 outside it"""
    tx, ty, tw, th = tile
    b = np.zeros((bh, bw), rec.data.dtype)
    vw, vh = max(0, min(bw, tw - x)), max(0, min(bh, th - y))
    if vw and vh:
        y0, x0 = rec.yorigin + ty + y, rec.xorigin + tx + x
        b[:vh, :vw] = rec.data[y0:y0 + vh, x0:x0 + vw]
    return b


def _clone(hp):
    p = O.HostPlane.__new__(O.HostPlane)
    p.__dict__.update(hp.__dict__)
    p.data = hp.data.copy()
    return p


def oracle_split(L, org, rec, tile, bw, bh, ts, cands, enable, mask, qindex, kind, scales=None):
    t, bd = TX_SIDE[ts], org.bit_depth
    hbd = int(bd > 8)
    dt, ct = (np.uint8, np.int16) if bd == 8 else (np.uint16, np.int32)
    tx, ty, tw, th = tile
    n, slots, ntx = len(cands), type_slots(mask), (bw // t) * (bh // t)
    nt = len(slots)
    eob = np.zeros((n, nt, ntx), np.uint16)
    dist = np.zeros((n, nt, ntx) if kind == 0 else (n, nt), np.uint64)
    rate = np.zeros((n, nt, ntx), np.uint64)
    qc = np.zeros((n, nt, ntx, t * t), ct)
    out_rec = np.zeros((n, nt, bh, bw), dt)
    pa = org.cstruct()
    sc_ptr, sc_stride = (O.ptr(scales), scales.shape[1]) if scales is not None else (None, 0)
    for i in range(n):
        c = cands[i]
        x, y, mode, delta, ief = int(c["x"]), int(c["y"]), int(c["mode"]), int(c["angle_delta"]), int(c["ief"])
        for j, tt in enumerate(slots):
            R = _clone(rec)
            B = _initial_block(rec, tile, x, y, bw, bh)
            for k, xk, yk, skipped in tx_blocks(x, y, bw, bh, t, tw, th):
                if skipped:
                    continue
                edge, lens = np.zeros(257, dt), (C.c_int * 2)()
                L.r1o_get_intra_edges(O.ptr(edge), lens, R.block_ptr(tx, ty), R.stride, xk, yk, tw, th, ts, bd, mode,
                                      int(enable), delta, (int(c["tr_mask"]) >> k) & 1, (int(c["bl_mask"]) >> k) & 1, hbd)
                pred = np.zeros((1, t, t), dt)
                assert L.r1o_predict_intra(mode, xk, yk, O.ptr(pred), t, ts, bd, None, delta, 0, ief, O.ptr(edge),
                                           lens[0], lens[1], _avail(t, rec.width, tx + xk),
                                           _avail(t, rec.height, ty + yk), hbd) == 0
                rc = np.zeros(1, O.RDO_CAND)
                rc["ox"], rc["oy"] = tx + xk, ty + yk
                sad, satd = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
                e1, d1, r1 = np.zeros(1, np.uint16), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
                q1, rec1 = np.zeros((1, t * t), ct), np.zeros((1, t, t), dt)
                # the reconstruction comes from a pixel-domain kind, the per-block distortion and rate from kind 0
                for kd in ((2, 0) if kind == 0 else (2,)):
                    assert L.r1o_rdo_txsearch_batch(
                        C.byref(pa), None, O.ptr(pred), t, t, ts, O.ptr(rc), 1, 1 << tt, qindex, 1, 0, 0, kd, None, 0, 0,
                        0, O.ptr(sad), O.ptr(satd), O.ptr(e1), O.ptr(d1), O.ptr(r1) if kd == 0 else None, O.ptr(q1),
                        O.ptr(rec1) if kd else None) == 0
                eob[i, j, k], qc[i, j, k] = e1[0], q1[0]
                if kind == 0:
                    dist[i, j, k], rate[i, j, k] = d1[0], r1[0]
                y0, x0 = R.yorigin + ty + yk, R.xorigin + tx + xk
                R.data[y0:y0 + t, x0:x0 + t] = rec1[0]
                B[yk - y:yk - y + t, xk - x:xk - x + t] = rec1[0]
            out_rec[i, j] = B
            if kind:
                bp = O.HostPlane(bw, bh, bd, 0, 0)
                bp.data[:bh, :bw] = B
                dc = np.zeros(1, O.DIST_CAND)
                dc["ox"], dc["oy"] = tx + x, ty + y
                pb, d = bp.cstruct(), np.zeros(1, np.uint64)
                assert L.r1o_dist_scaled_batch(kind, C.byref(pa), C.byref(pb), bw, bh, O.ptr(dc), 1, sc_ptr, sc_stride, 0,
                                               0, O.ptr(d)) == 0
                dist[i, j] = d[0]
    return dict(eob=eob, dist=dist, est_rate=rate, qcoeffs=qc, rec=out_rec)


def _interact(a, b, bw, bh):
    """the blocks at a and b: may one read what the other writes?  A block reads from one pixel left of / above it
    to its own size right of / below it (top-right and bottom-left edges) and writes its own rectangle."""
    def sees(p, q):
        return p[0] - 1 < q[0] + bw and q[0] < p[0] + 2 * bw and p[1] - 1 < q[1] + bh and q[1] < p[1] + 2 * bh
    return sees(a, b) or sees(b, a)


def device_split(ctx, dorg, drec, tile, bw, bh, ts, cands, enable, mask, qindex, kind, dscales=None):
    import torch
    from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND, DIST_CAND, RDO_CAND, Plane
    t, bd = TX_SIDE[ts], dorg.bit_depth
    tx, ty, tw, th = tile
    n, slots, ntx = len(cands), type_slots(mask), (bw // t) * (bh // t)
    nt = len(slots)
    pt, cdt = (torch.uint8, torch.int16) if bd == 8 else (torch.int16, torch.int32)
    dev = dict(device="cuda")
    eob = torch.zeros((n, nt, ntx), dtype=torch.int16, **dev)
    dist = torch.zeros((n, nt, ntx) if kind == 0 else (n, nt), dtype=torch.int64, **dev)
    rate = torch.zeros((n, nt, ntx), dtype=torch.int64, **dev)
    qc = torch.zeros((n, nt, ntx, t * t), dtype=cdt, **dev)
    out_rec = torch.zeros((n, nt, bh, bw), dtype=pt, **dev)
    rec_keep = drec.data.clone()
    # the scratch plane: `rec`'s own layout and content, restored before every round
    scratch = Plane.__new__(Plane)
    scratch.__dict__.update(drec.__dict__)
    scratch.data = drec.data.clone()
    # rounds of blocks that cannot see each other
    rounds = []
    for i in range(n):
        p = (int(cands["x"][i]), int(cands["y"][i]))
        for r in rounds:
            if not any(_interact(p, (int(cands["x"][m]), int(cands["y"][m])), bw, bh) for m in r):
                r.append(i)
                break
        else:
            rounds.append([i])
    base_angle = [0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0]
    for members in rounds:
        for j, tt in enumerate(slots):
            scratch.data.copy_(rec_keep)
            blocks = {}
            for i in members:
                x, y = int(cands["x"][i]), int(cands["y"][i])
                init = np.zeros((bh, bw), np.uint8 if bd == 8 else np.int16)
                blocks[i] = torch.from_numpy(init).cuda()
                vw, vh = max(0, min(bw, tw - x)), max(0, min(bh, th - y))
                if vw and vh:
                    y0, x0 = drec.yorigin + ty + y, drec.xorigin + tx + x
                    blocks[i][:vh, :vw] = rec_keep[y0:y0 + vh, x0:x0 + vw]
            for k in range(ntx):
                live = []
                for i in members:
                    kk, xk, yk, skipped = tx_blocks(int(cands["x"][i]), int(cands["y"][i]), bw, bh, t, tw, th)[k]
                    if not skipped:
                        live.append((i, xk, yk))
                if not live:
                    continue
                m = len(live)
                ec, ic, rc = np.zeros(m, INTRA_EDGE_CAND), np.zeros(m, INTRA_CAND), np.zeros(m, RDO_CAND)
                for s, (i, xk, yk) in enumerate(live):
                    c = cands[i]
                    mode, delta = int(c["mode"]), int(c["angle_delta"])
                    ec[s] = (xk, yk, mode, delta, int(enable) | (((int(c["tr_mask"]) >> k) & 1) << 1)
                             | (((int(c["bl_mask"]) >> k) & 1) << 2), 0)
                    var = 0 if (xk == 0 and yk == 0) else (1 if yk == 0 else (2 if xk == 0 else 3))
                    pm = {0: 0, 2: 1, 1: 2, 3: 12}[var] if mode == 12 else mode
                    ic[s] = (pm, var, base_angle[pm] + 3 * delta, int(c["ief"]), _avail(t, drec.width, tx + xk),
                             _avail(t, drec.height, ty + yk), 0)
                    rc["ox"][s], rc["oy"][s] = tx + xk, ty + yk
                edges, lens = ctx.intra_edges_batch(scratch, tile, ts, ec)
                pred = ctx.predict_intra_batch(ts, ic, edges, lens, bd)
                o = ctx.rdo_txsearch_batch(dorg, None, t, t, rc, 1 << tt, qindex, 2, is_intra=1, want_qcoeffs=True,
                                           want_rec=True, pred=pred)
                if kind == 0:
                    o0 = ctx.rdo_txsearch_batch(dorg, None, t, t, rc, 1 << tt, qindex, 0, is_intra=1,
                                                want_est_rate=True, pred=pred)
                for s, (i, xk, yk) in enumerate(live):
                    eob[i, j, k], qc[i, j, k] = o["eob"][s, 0], o["qcoeffs"][s, 0]
                    if kind == 0:
                        dist[i, j, k], rate[i, j, k] = o0["dist"][s, 0], o0["est_rate"][s, 0]
                    y0, x0 = drec.yorigin + ty + yk, drec.xorigin + tx + xk
                    scratch.data[y0:y0 + t, x0:x0 + t] = o["rec"][s, 0]
                    bx, by = xk - int(cands["x"][i]), yk - int(cands["y"][i])
                    blocks[i][by:by + t, bx:bx + t] = o["rec"][s, 0]
            for i in members:
                out_rec[i, j] = blocks[i]
                if kind:
                    bp = Plane(bw, bh, bd, 0, 0)
                    bp.data[:bh, :bw] = blocks[i]
                    dc = np.zeros(1, DIST_CAND)
                    dc["ox"], dc["oy"] = tx + int(cands["x"][i]), ty + int(cands["y"][i])
                    dist[i, j] = ctx.dist_scaled_batch(kind, dorg, bp, bw, bh, dc, scales=dscales)[0]
    assert torch.equal(drec.data, rec_keep), "the composition wrote the caller's plane"
    return dict(eob=eob, dist=dist, est_rate=rate, qcoeffs=qc, rec=out_rec)

#!/usr/bin/env python3
"""The intra transform-split candidate in one launch against the best route without it, same process, same inputs:

    python tools/bench_intra_split.py [--bit-depths 8,10] [--sizes 16,32] [--depths 1,2] [--kinds 3,0] [--reps 10] [--out F]

For every (block size s, split depth, bit depth, dist_kind): every s x s block of a 3840x2160 luma plane (padding 88) x
K = 4 intra modes, coded with the transform one or two depths below the block (rdo_glue.sub_tx_size), DCT_DCT, the
intra edge filter on, random has_top_right / has_bottom_left answers.
  (a) one launch   r1_rdo_intra_split_batch: the working reconstruction of every trial stays on the CU.
  (b) composition  what the library offers without it, batched across blocks: the K modes of a block need K private
                   reconstructions, so K scratch planes are restored from `rec` (part of the route: timed), and step k
                   of ALL blocks goes through K r1_intra_edges_batch launches (one per scratch plane), ONE
                   r1_rdo_intra_cand_batch launch (edge_group = 1) that leaves the reconstruction in HBM -- under
                   dist_kind 0, which gives none, + r1_dequantize_batch + r1_inv_txfm_add_batch on its prediction --
                   and one strided copy that scatters the n reconstructions into the scratch planes; behind the last
                   step K r1_dist_scaled_batch launches for a pixel-domain kind.
In (b) the blocks of a plane step in lockstep on ONE scratch plane per mode, so a block sees its neighbours' trial
reconstructions where (a) sees `rec`: the same work, not the same numbers.  Parity is therefore checked first on every
other block of every other block row (blocks that cannot see each other), where both must agree bit for bit in eob,
distortion and reconstruction; the timed runs then take all blocks.  Timing: HIP events on the launch stream, a
sustain window before every series, median of --reps, both sides alternately, best of two rounds.  One JSON line per
point."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bit-depths", default="8,10")
    ap.add_argument("--sizes", default="16,32")
    ap.add_argument("--depths", default="1,2")
    ap.add_argument("--kinds", default="3,0")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import time
    import torch
    from rav1e_amd import workload as W
    from rav1e_amd.api import (DIST_CAND, INTRA_CAND, INTRA_EDGE_CAND, INTRA_SPLIT_CAND, EDGE_LEN, Context, Plane,
                               _coeff_dtype, _pix_dtype, _stream_ptr)
    from rav1e_amd.rdo_glue import sub_tx_size
    from rav1e_amd.types import TxSize
    assert torch.cuda.is_available(), "bench_intra_split.py measures on a GPU; there is nothing to report without one"
    ctx = Context(0)
    fw, fh, K = args.width, args.height, args.k
    tile = (0, 0, fw, fh)

    def timed(f):
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.sustain_ms:
            f()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(x.elapsed_time(y) for x, y in ev)
        return ms[len(ms) // 2]

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    base_angle = np.array([0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0])

    class Setup:
        """both routes over the blocks of a regular grid: pitch = s (every block) or 2 s (blocks that cannot see each
        other); trial index = m * nb + b (mode-major: the trials of scratch plane m are contiguous)"""

        def __init__(self, org, rec, scratch, s, t, bd, kind, pitch, seed):
            self.org, self.rec, self.scratch, self.s, self.t, self.bd, self.kind, self.pitch = org, rec, scratch, s, t, bd, kind, pitch
            self.ts = int(TxSize.by_dims(t, t))
            bpp = org.bpp
            rng = np.random.default_rng(seed)
            self.nbx, self.nby = (fw - s) // pitch + 1, (fh - s) // pitch + 1
            bx, by = np.meshgrid(np.arange(self.nbx) * pitch, np.arange(self.nby) * pitch)
            bx, by = bx.ravel(), by.ravel()
            nb = self.nb = len(bx)
            n = self.n = nb * K
            g = s // t
            self.ntx = g * g
            mode = np.argsort(rng.random((nb, 13)), axis=1)[:, :K].T.ravel()          # (K, nb): distinct per block
            x, y = np.tile(bx, K), np.tile(by, K)
            direc = (mode >= 1) & (mode <= 8)
            delta = np.where(direc, rng.integers(-3, 4, n), 0)
            ief = np.where(direc, np.tile(rng.integers(1, 3, nb), K), 0)
            trm, blm = rng.integers(0, 1 << self.ntx, n), rng.integers(0, 1 << self.ntx, n)
            sc = np.zeros(n, INTRA_SPLIT_CAND)
            sc["x"], sc["y"], sc["mode"], sc["angle_delta"], sc["ief"], sc["tr_mask"], sc["bl_mask"] = x, y, mode, delta, ief, trm, blm
            self.d_split = dev(sc)
            self.scales = scales if kind else None
            carea = t * t
            self.a_out = {"eob": torch.empty((n, 1, self.ntx), dtype=torch.int16, device="cuda"),
                          "dist": torch.empty((n, 1, self.ntx) if kind == 0 else (n, 1), dtype=torch.int64, device="cuda")}
            # ---- the composition's per-step descriptors
            self.steps = []
            for k in range(self.ntx):
                xk, yk = x + (k % g) * t, y + (k // g) * t
                ec = np.zeros(n, INTRA_EDGE_CAND)
                ec["x"], ec["y"], ec["mode"], ec["angle_delta"] = xk, yk, mode, delta
                ec["flags"] = 1 | (((trm >> k) & 1) << 1) | (((blm >> k) & 1) << 2)
                var = np.where((xk == 0) & (yk == 0), 0, np.where(yk == 0, 1, np.where(xk == 0, 2, 3)))
                pa = mode == 12
                pm = np.where(pa & (var == 0), 0, np.where(pa & (var == 2), 1, np.where(pa & (var == 1), 2, mode)))
                ic = np.zeros(n, INTRA_CAND)
                ic["mode"], ic["variant"], ic["angle"], ic["ief"] = pm, var, base_angle[pm] + 3 * delta, ief
                ic["avail_w"], ic["avail_h"] = np.minimum(t, fw - xk), np.minimum(t, fh - yk)
                pos = torch.from_numpy(np.stack([xk, yk], 1).astype(np.int16)).cuda()
                self.steps.append((dev(ec), dev(ic), pos, (k % g) * t, (k // g) * t))
            self.edges = torch.empty((n, EDGE_LEN), dtype=_pix_dtype(bpp), device="cuda")
            self.lens = torch.empty((n, 2), dtype=torch.uint8, device="cuda")
            self.b_eob = torch.empty((n, self.ntx), dtype=torch.int16, device="cuda")
            self.b_dist = torch.empty((n, self.ntx) if kind == 0 else (n,), dtype=torch.int64, device="cuda")
            self.c_out = {"eob": torch.empty((n, 1), dtype=torch.int16, device="cuda"),
                          "dist": torch.empty((n, 1), dtype=torch.int64, device="cuda")}
            if kind == 0:
                self.c_out["qcoeffs"] = torch.empty((n, 1, carea), dtype=_coeff_dtype(bpp), device="cuda")
                self.c_out["pred"] = torch.empty((n, t, t), dtype=_pix_dtype(bpp), device="cuda")
                self.b_rec = torch.empty((n, t, t), dtype=_pix_dtype(bpp), device="cuda")
            else:
                self.c_out["rec"] = torch.empty((n, 1, t, t), dtype=_pix_dtype(bpp), device="cuda")
            dc = np.zeros(nb, DIST_CAND)
            dc["ox"], dc["oy"], dc["rx"], dc["ry"] = bx, by, bx, by
            self.d_dist = dev(dc)
            # the blocks of scratch plane m as (nby, pitch, nbx, pitch) tiles of its visible area
            yo, xo = rec.yorigin, rec.xorigin
            self.tiles = [p.data[yo:yo + self.nby * pitch, xo:xo + self.nbx * pitch]
                          .unflatten(0, (self.nby, pitch)).unflatten(2, (self.nbx, pitch)) for p in scratch]
            self.edge_stride_bytes = EDGE_LEN * bpp

        def one_launch(self, want_rec=False):
            return ctx.rdo_intra_split_batch(self.org, self.rec, tile, self.s, self.s, self.ts, self.d_split, 1,
                                             args.qindex, self.kind, scales=self.scales, n=self.n,
                                             outs=dict(self.a_out), want_rec=want_rec)

        def composition(self):
            nb, t, kind, st = self.nb, self.t, self.kind, _stream_ptr()
            for p in self.scratch:
                p.data.copy_(self.rec.data)
            for k, (d_ec, d_ic, pos, ox, oy) in enumerate(self.steps):
                for m, p in enumerate(self.scratch):
                    pr = p.cstruct()
                    rc = ctx.lib.r1_intra_edges_batch(ctx.h, C.byref(pr), 0, 0, fw, fh, self.ts,
                                                      d_ec.data_ptr() + m * nb * INTRA_EDGE_CAND.itemsize, nb,
                                                      self.edges.data_ptr() + m * nb * self.edge_stride_bytes, EDGE_LEN,
                                                      self.lens.data_ptr() + m * nb * 2, st)
                    assert rc == 0
                ctx.rdo_intra_cand_batch(self.org, t, t, d_ic, pos, self.edges, self.lens, 1, args.qindex,
                                         0 if kind == 0 else 2, edge_group=1, n=self.n, outs=self.c_out)
                self.b_eob[:, k] = self.c_out["eob"][:, 0]
                if kind == 0:
                    self.b_dist[:, k] = self.c_out["dist"][:, 0]
                    rco = ctx.dequantize_batch(self.c_out["qcoeffs"][:, 0], self.ts, args.qindex, self.bd)
                    ctx.inverse_transform_add_batch(rco, self.c_out["pred"], self.ts, 0, self.bd, out=self.b_rec)
                    rec_k = self.b_rec
                else:
                    rec_k = self.c_out["rec"][:, 0]
                rec_k = rec_k.view(K, self.nby, self.nbx, t, t).permute(0, 1, 3, 2, 4)
                for m in range(K):
                    self.tiles[m][:, oy:oy + t, :, ox:ox + t].copy_(rec_k[m])
            if kind:
                for m, p in enumerate(self.scratch):
                    ctx.dist_scaled_batch(kind, self.org, p, self.s, self.s, self.d_dist, scales=self.scales, n=nb,
                                          out=self.b_dist[m * nb:(m + 1) * nb])

        def block_recs(self):
            """(n, s, s): the blocks of the scratch planes behind the composition"""
            s = self.s
            return torch.stack([tl[:, :s, :, :s].permute(0, 2, 1, 3).reshape(self.nb, s, s) for tl in self.tiles]) \
                .reshape(self.n, s, s)

    for bd in (int(b) for b in args.bit_depths.split(",")):
        rec = Plane.from_numpy(W.random_plane_array(fw, fh, bd, 1), fw, fh, bd, 88, 88)
        org = Plane.from_numpy(W.random_plane_array(fw, fh, bd, 2), fw, fh, bd, 88, 88)
        scratch = [Plane(fw, fh, bd, 88, 88) for _ in range(K)]
        scales = torch.from_numpy(np.random.default_rng(5).integers(1 << 12, 1 << 16, ((fh + 7) // 8, (fw + 7) // 8))
                                  .astype(np.int32)).cuda()
        for s in (int(v) for v in args.sizes.split(",")):
            for depth in (int(v) for v in args.depths.split(",")):
                ts = TxSize.by_dims(s, s)
                for _ in range(depth):
                    ts = sub_tx_size(ts)
                t = ts.dims[0]
                for kind in (int(v) for v in args.kinds.split(",")):
                    # ---- parity where both routes mean the same: blocks that cannot see each other
                    chk = Setup(org, rec, scratch, s, t, bd, kind, 2 * s, 100 + s + depth)
                    oa = chk.one_launch(want_rec=bool(kind))
                    chk.composition()
                    torch.cuda.synchronize()
                    same = bool(torch.equal(oa["eob"][:, 0], chk.b_eob) and
                                torch.equal(oa["dist"][:, 0], chk.b_dist) and
                                (not kind or torch.equal(oa["rec"][:, 0], chk.block_recs())))
                    nz = float((chk.b_eob != 0).float().mean())
                    n_chk = chk.n
                    del chk, oa
                    if not same:
                        emit({"block": s, "tx": t, "depth": depth, "bd": bd, "dist_kind": kind, "identical": False})
                        raise SystemExit("the one launch and the composition disagree at %dx%d / %dx%d" % (s, s, t, t))
                    # ---- timing: every block
                    run = Setup(org, rec, scratch, s, t, bd, kind, s, 200 + s + depth)
                    runs = {"one_launch": [], "composition": []}
                    for _ in range(2):
                        runs["one_launch"].append(timed(run.one_launch))
                        runs["composition"].append(timed(run.composition))
                    ms = {k: min(v) for k, v in runs.items()}
                    emit({"block": s, "tx": t, "depth": depth, "ntx": run.ntx, "bd": bd, "dist_kind": kind, "n": run.n,
                          "k": K, "identical_on_isolated_blocks": same, "n_checked": n_chk,
                          "nonzero_eob_share": round(nz, 3),
                          "launches_composition": run.ntx * (K + 1 + (2 if kind == 0 else 0)) + (K if kind else 0),
                          "ms": {k: round(v, 4) for k, v in ms.items()},
                          "ms_runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                          "ratio_one_launch_vs_composition": round(ms["one_launch"] / ms["composition"], 4),
                          "trials_per_s_one_launch": round(run.n / (ms["one_launch"] * 1e-3))})
                    del run
    ctx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The three-depth intra decision with the pick and the commit on the stream, against the route there was without
them, same process, same inputs:

    python tools/bench_rd_pick.py [--bit-depths 8,10] [--reps 10] [--out F]

Every 16x16 block of a 3840x2160 luma plane (padding 88; noise, an 8x8 and a 4x4 checkerboard in 32-pixel bands, so
that each depth wins about a third of the blocks) x K = 4 intra modes (DC, V, H, SMOOTH).  Both routes run
the same six launches first -- r1_rdo_intra_cand_batch (16x16, the 7 types), r1_rdo_intra_split_batch at 8x8 and at
4x4 (7 types each), each followed by r1_coeff_rate_chain_batch -- and then decide:
  (a) device   r1_rd_pick_batch (R1_PICK_TX_TYPE, call_id 0 / 1 / 2 on one state per (block, mode)) behind each rate
               launch, a gather of the mode states' rate / distortion, r1_rd_pick_batch (R1_PICK_FIRST_MIN over the K
               modes with a rate_add), the winners' states, three r1_rd_commit_batch: nothing is read by the host.
  (b) host     synchronise, download rate + dist of the three depths, the same rules as one NumPy statement per depth
               (vectorised; not the per-slot Python model), upload the winners' indices, gather eob / coefficients /
               contexts and scatter the reconstructions with torch indexing.
The NumPy statement rounds lambda * (rate / 8) + dist twice; lambda is a small dyadic number here (203.25), so the
product is exact and both routes cost alike.  Parity of the two routes (states' decisions, eob_win, qcoeffs_win,
side_win and the destination plane) is checked before anything is timed.  Timing: HIP events around the whole route
for (a); wall clock between synchronisations for (b), which has the host in it; a sustain window before every series,
median of --reps, both sides alternately, best of two rounds.  `decide_only` rows time the routes WITHOUT the six
search / rate launches (their outputs kept from a previous pass): what the decision itself costs.  One JSON line per
point."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rd_chain_util import DEPTH_NTX, S, Chain           # the device route: tests/rd_chain_util.py, held to the host statements


class BenchChain(Chain):
    """the chain of tests/rd_chain_util.py (route (a)) with route (b) on the same buffers"""

    # ---- (b)
    def host_decide(self, rates, dists, adds):
        """the same rules, one NumPy statement per depth: -> (depth, mode, slot, rd) per block"""
        n, K = self.n, self.K
        best_rd = np.full(n, sys.float_info.max)
        best_rate, best_dist = np.zeros(n, np.int64), np.zeros(n, np.uint64)
        best_slot, best_depth = np.full(n, -1), np.full(n, -1)
        rows = np.arange(n)
        for d in range(3):
            r, ds = rates[d].astype(np.int64), dists[d]
            rd = self.lam * (r / 8.0) + ds.astype(np.float64)
            rd[r >= 0xFFFFFFFF] = np.inf
            j = rd.argmin(1)                                         # the first of equal minima
            keep = ~(rd[:, 0] > best_rd) & (rd[rows, j] < best_rd)   # the early exit, then rdo.rs:780
            best_rd = np.where(keep, rd[rows, j], best_rd)
            best_rate, best_dist = np.where(keep, r[rows, j], best_rate), np.where(keep, ds[rows, j], best_dist)
            best_slot, best_depth = np.where(keep, j, best_slot), np.where(keep, d, best_depth)
        rm = self.lam * ((best_rate + adds) / 8.0) + best_dist.astype(np.float64)
        rm[best_depth < 0] = np.inf                                  # a mode that kept nothing: the invalid rate
        rm = rm.reshape(-1, K)
        m = rm.argmin(1)
        b = np.arange(self.nb)
        c = b * K + m
        return best_depth[c], m, best_slot[c], rm[b, m]

    def host_route(self, search=True, wins=None):
        torch, K, nt = self.torch, self.K, self.nt
        if search:
            for d in range(3):
                self.launches(d)
        torch.cuda.synchronize()
        rates = [self.rate[d]["rate"].cpu().numpy().view(np.uint32).reshape(self.n, nt) for d in range(3)]
        dists = [self.search[d]["dist"].cpu().numpy().view(np.uint64).reshape(self.n, nt) for d in range(3)]
        depth, m, slot, rd = self.host_decide(rates, dists, self.rate_add_host)
        t = torch.from_numpy(((np.arange(self.nb) * K + m) * nt + slot).astype(np.int64)).cuda()
        dep = torch.from_numpy(depth.astype(np.int64)).cuda()
        o = wins if wins is not None else self.new_wins()
        yo, xo = self.dst.yorigin, self.dst.xorigin
        for d in range(3):
            sel = (dep == d).nonzero().ravel()
            td = t[sel]
            ntx = DEPTH_NTX[d]
            o["eob_win"][sel, :ntx] = self.search[d]["eob"].view(-1, ntx)[td]
            o["qcoeffs_win"][sel] = self.search[d]["qcoeffs"].view(-1, S * S)[td]
            o["side_win"][sel] = self.rate[d]["ctx"].view(-1, 32)[td]
            yy = (yo + self.pos[sel, 1].to(torch.int64))[:, None, None] + self.ar16[None, :, None]
            xx = (xo + self.pos[sel, 0].to(torch.int64))[:, None, None] + self.ar16[None, None, :]
            self.dst.data[yy, xx] = self.search[d]["rec"].view(-1, S, S)[td]
        return depth, m, slot, rd, o

    @property
    def rate_add_host(self):
        if not hasattr(self, "_adds"):
            self._adds = self.rate_add.cpu().numpy().astype(np.int64)
        return self._adds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bit-depths", default="8,10")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    from rav1e_amd import workload as W
    from rav1e_amd.api import Context, Plane
    from rav1e_amd.types import RD_PICK
    assert torch.cuda.is_available(), "bench_rd_pick.py measures on a GPU; there is nothing to report without one"
    ctx = Context(0)
    fw, fh = args.width, args.height

    def timed(f, events):
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.sustain_ms:
            f()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            else:
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
        return sorted(ms)[len(ms) // 2]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for bd in (int(b) for b in args.bit_depths.split(",")):
        # the source in 96-pixel periods -- 32 columns of noise (the 16x16 transform wins there), 32 of an 8x8
        # checkerboard, 32 of a 4x4 one (flat transform blocks one and two depths down) -- so that every depth wins a
        # share of the blocks and every commit has winners to move; the reconstruction: the source, slightly off
        a_org = W.random_plane_array(fw, fh, bd, 2)
        lay = W.plane_layout(fw, fh, bd, 88, 88)
        yy, xx = np.mgrid[0:a_org.shape[0], 0:a_org.shape[1]]
        xv = xx - lay["xorigin"]
        for lo, cell in ((32, 8), (64, 4)):
            band = (xv % 96 >= lo) & (xv % 96 < lo + 32)
            a_org[band] = ((50 + 125 * ((xv // cell + yy // cell) % 2)) << (bd - 8))[band]
        a_rec = np.clip(a_org.astype(np.int64) + np.random.default_rng(1).integers(-2, 3, a_org.shape), 0,
                        (1 << bd) - 1).astype(a_org.dtype)
        del yy, xx, xv
        rec = Plane.from_numpy(a_rec, fw, fh, bd, 88, 88)
        org = Plane.from_numpy(a_org, fw, fh, bd, 88, 88)
        dst_a, dst_b = Plane(fw, fh, bd, 88, 88), Plane(fw, fh, bd, 88, 88)
        bx, by = np.meshgrid(np.arange(fw // S) * S, np.arange(fh // S) * S)
        ch = BenchChain(ctx, org, rec, dst_a, bx.ravel(), by.ravel(), qindex=args.qindex)
        # ---- parity
        wa = None
        ch.launches(0), ch.launches(1), ch.launches(2)
        wa = ch.new_wins()
        st, blk, win, wa = ch.device_route(search=False, wins=wa)
        ch.dst = dst_b
        depth, m, slot, rd, wb = ch.host_route(search=False, wins=ch.new_wins())
        torch.cuda.synchronize()
        hw = win.cpu().numpy().view(RD_PICK).ravel()
        hb = blk.cpu().numpy().view(RD_PICK).ravel()
        same = bool(np.array_equal(hw["best_call"], depth) and np.array_equal(hw["best_slot"], slot) and
                    np.array_equal(hb["best_row"], m) and np.array_equal(hb["best_rd"].view(np.uint64), rd.view(np.uint64)) and
                    all(torch.equal(wa[k], wb[k]) for k in wa) and torch.equal(dst_a.data, dst_b.data))
        shares = [round(float((depth == d).mean()), 3) for d in range(3)]
        if not same:
            emit({"bd": bd, "identical": False})
            raise SystemExit("the device route and the host route disagree")
        ch.dst = dst_a
        rows = {}
        for name, search in (("full", True), ("decide_only", False)):
            runs = {"device": [], "host": []}
            for _ in range(2):
                runs["device"].append(timed(lambda: ch.device_route(search=search), True))
                runs["host"].append(timed(lambda: ch.host_route(search=search, wins=wb), False))
            rows[name] = {k: min(v) for k, v in runs.items()}
            rows[name + "_runs"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        emit({"bench": "rd_pick", "bd": bd, "width": fw, "height": fh, "blocks": ch.nb, "modes": ch.K, "types": ch.nt,
              "trials_per_depth": ch.n * ch.nt, "identical": same, "depth_shares": shares,
              "ms_full": {k: round(v, 4) for k, v in rows["full"].items()},
              "ms_decide_only": {k: round(v, 4) for k, v in rows["decide_only"].items()},
              "ms_runs": {"full": rows["full_runs"], "decide_only": rows["decide_only_runs"]},
              "ratio_device_vs_host_full": round(rows["full"]["device"] / rows["full"]["host"], 4),
              "ratio_device_vs_host_decide_only": round(rows["decide_only"]["device"] / rows["decide_only"]["host"], 4),
              "timing": "device: HIP events around the route; host: wall clock to the synchronisation behind it"})
        del ch, rec, org, dst_a, dst_b
    ctx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The partition decision of one quad-tree level with the pick and the selects on the stream, against the route there
was without them, same process, same inputs:

    python tools/bench_part_pick.py [--levels 64,16] [--reps 10] [--out F]

The nodes of ONE level of every superblock of a 3840x2160 frame: the 64x64 nodes over their 32x32 children (2 040
nodes; the last superblock row is cut by the frame) and the 16x16 nodes over their 8x8 children (32 400).  Each node
has four finished trials -- PARTITION_NONE (1 child cost), HORZ and VERT (2), SPLIT (4), the costs R1RdPick states of
integer values, the partition rates 1/8-bit integers, lambda a small dyadic number, so that every product and sum is
exact and both routes cost alike -- and behind each trial a snapshot of what it left: an R1CoeffCdfContext (7 872 B),
an R1CoeffNbrContext (3 120 B) and a luma plane.
  (a) device   four r1_rd_partition_pick_batch (R1_PART_BOTTOMUP, call_id 0..3, early exit on) on one state per node,
               r1_part_select_batch for the two contexts, r1_part_select_rect_batch for the node's rectangle: nothing
               is read by the host.
  (b) host     synchronise, download the children's costs, the same rule as one NumPy statement per trial (vectorised;
               the first nodes are also put through rdo_glue.partition_pick_bottomup), upload the choice, copy the
               winners' contexts and rectangles with torch indexing.
Both routes must leave the same decisions and the same three states before anything is timed.  Timing: HIP events
around the whole route for (a); wall clock between synchronisations for (b), which has the host in it -- the two
clocks compare as orders of magnitude only; a sustain window before every series, median of --reps, both sides
alternately, best of two rounds.  One JSON line per level."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MAX = sys.float_info.max
VISITED = (1, 2, 2, 4)
LAMBDA = 203.25


def host_decide(costs, rates, lam):
    """costs[p]: (n, VISITED[p]) f64, rates: (n, 4) -> (best_rd, best_partition) per node: encode_partition_bottomup's
    trials in order, every child present, no must_split, ref_rd_cost = f64::MAX, the early exit on"""
    n = len(rates)
    cost = lam * (rates / 8.0)
    best = costs[0][:, 0] + cost[:, 0]
    part = np.zeros(n, np.int8)
    for p in (1, 2, 3):
        rd, early = cost[:, p].copy(), np.zeros(n, bool)
        for k in range(VISITED[p]):
            rd = np.where(early, rd, rd + costs[p][:, k])
            early |= rd >= best
        keep = ~early & (rd < best)
        best, part = np.where(keep, rd, best), np.where(keep, p, part).astype(np.int8)
    return best, part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--levels", default="64,16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    from rav1e_amd import rdo_glue
    from rav1e_amd.api import Context, Plane
    from rav1e_amd.types import COEFF_CDF_CONTEXT, COEFF_NBR_CONTEXT, PART_BOTTOMUP, PART_PICK, RD_PICK
    assert torch.cuda.is_available(), "bench_part_pick.py measures on a GPU; there is nothing to report without one"
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

    for bs in (int(v) for v in args.levels.split(",")):
        rng = np.random.default_rng(bs)
        bx, by = np.meshgrid(np.arange((fw + bs - 1) // bs) * bs, np.arange((fh + bs - 1) // bs) * bs)
        n = bx.size
        pos = torch.from_numpy(np.stack([bx.ravel(), by.ravel()], 1).astype(np.int16)).cuda()
        # the children: per trial an array of R1RdPick states, a quarter costing about a quarter of the whole
        area = bs * bs
        hcost = [rng.integers(area * 40 // v, area * 60 // v, (n, v)).astype(np.float64) for v in VISITED]
        rates = rng.integers(8, 400, (n, 4)).astype(np.uint32)
        kids, kid_idx = [], []
        for p, v in enumerate(VISITED):
            a = np.zeros(n * v, RD_PICK)
            a["best_rd"] = hcost[p].ravel()
            kids.append(torch.from_numpy(a.view(np.uint8).reshape(n * v, RD_PICK.itemsize)).cuda())
            idx = np.full((n, 4), -1, np.int32)
            idx[:, :v] = np.arange(n * v, dtype=np.int32).reshape(n, v)
            kid_idx.append(torch.from_numpy(idx).cuda())
        drates = [torch.from_numpy(np.ascontiguousarray(rates[:, p]).view(np.int32)).cuda() for p in range(4)]
        init = ctx.part_pick_state(n)
        # what each trial left, and the live state of each route
        cdfs = [torch.randint(0, 256, (n, COEFF_CDF_CONTEXT.itemsize), dtype=torch.uint8, device="cuda") for _ in range(4)]
        nbrs = [torch.randint(0, 256, (n, COEFF_NBR_CONTEXT.itemsize), dtype=torch.uint8, device="cuda") for _ in range(4)]
        planes = [Plane(fw, fh, 8, 88, 88) for _ in range(4)]
        for p in planes:
            p.data.random_(0, 256)
        live = {r: (torch.zeros_like(cdfs[0]), torch.zeros_like(nbrs[0]), Plane(fw, fh, 8, 88, 88)) for r in "ab"}
        state = init.clone()
        ar = torch.arange(bs, device="cuda")

        def device_route():
            state.copy_(init)
            for p in range(4):
                ctx.rd_partition_pick_batch(state, p, p, PART_BOTTOMUP, LAMBDA, kids[p], kid_idx[p], part_rate=drates[p])
            cdf, nbr, plane = live["a"]
            ctx.part_select_batch(state, cdfs, cdf)
            ctx.part_select_batch(state, nbrs, nbr)
            ctx.part_select_rect_batch(state, planes, plane, pos, bs, bs)

        def host_route():
            torch.cuda.synchronize()
            costs = [k.cpu().numpy().reshape(-1).view(RD_PICK)["best_rd"].reshape(n, v) for k, v in zip(kids, VISITED)]
            best, part = host_decide(costs, rates, LAMBDA)
            choice = torch.from_numpy(part.astype(np.int64)).cuda()
            cdf, nbr, plane = live["b"]
            yo, xo = plane.yorigin, plane.xorigin
            for p in range(4):
                sel = (choice == p).nonzero().ravel()
                cdf[sel], nbr[sel] = cdfs[p][sel], nbrs[p][sel]
                yy = (yo + pos[sel, 1].to(torch.int64))[:, None, None] + ar[None, :, None]
                xx = (xo + pos[sel, 0].to(torch.int64))[:, None, None] + ar[None, None, :]
                yy, xx = torch.broadcast_tensors(yy, xx)
                ok = (yy < yo + fh) & (xx < xo + fw)                     # the frame cuts the last row of superblocks
                plane.data[yy[ok], xx[ok]] = planes[p].data[yy[ok], xx[ok]]
            return best, part

        # ---- parity, before anything is timed
        device_route()
        best, part = host_route()
        torch.cuda.synchronize()
        got = state.cpu().numpy().reshape(-1).view(PART_PICK)
        same = bool(np.array_equal(np.array(got["best_rd"]).view(np.uint64), best.view(np.uint64)) and
                    np.array_equal(got["best_partition"], part) and np.array_equal(got["best_call"], part) and
                    torch.equal(live["a"][0], live["b"][0]) and torch.equal(live["a"][1], live["b"][1]) and
                    torch.equal(live["a"][2].data, live["b"][2].data))
        for s in range(min(n, 256)):                                    # the NumPy statement is the glue's
            b, q = F64_MAX, -1
            for p in range(4):
                kept, rd, _e = rdo_glue.partition_pick_bottomup(b, p, LAMBDA, int(rates[s, p]), [float(v) for v in hcost[p][s]])
                b, q = (rd, p) if kept else (b, q)
            same = bool(same and b == best[s] and q == part[s])
        shares = [round(float((part == p).mean()), 3) for p in range(4)]
        if not same:
            emit({"bench": "part_pick", "level": bs, "identical": False})
            raise SystemExit("the device route and the host route disagree")
        runs = {"device": [], "host": []}
        for _ in range(2):
            runs["device"].append(timed(device_route, True))
            runs["host"].append(timed(host_route, False))
        ms = {k: round(min(v), 4) for k, v in runs.items()}
        emit({"bench": "part_pick", "level": "%d->%d" % (bs, bs // 2), "width": fw, "height": fh, "nodes": n, "trials": 4,
              "identical": same, "partition_shares": shares, "ms": ms,
              "ms_runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
              "ratio_device_vs_host": round(ms["device"] / ms["host"], 4),
              "timing": "device: HIP events around the route; host: wall clock to the synchronisation behind it"})
        del cdfs, nbrs, planes, live, kids
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

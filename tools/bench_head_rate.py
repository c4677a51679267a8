#!/usr/bin/env python3
"""The head rate and the head commit beside the coefficient-rate launch they stand in front of, and the host route they
remove, same process, same inputs:

    python tools/bench_head_rate.py [--points 16:8,32:8] [--reps 15] [--out FILE]

Every s x s block of a 3840x2160 frame (32 400 of 16x16, 8 040 of 32x32) at its place in a one-tile frame of 960 x 540
4x4 units, 4:2:0, with 4 luma modes x 2 chroma modes = 8 head trials per block, adjacent.  One R1HeadNbrContext and one
R1HeadCdfContext per block (seeded with what earlier blocks could have left), so that the commit's winners name distinct
contexts.  A point is block:transform.  Per point, alternating in one process after the same pre-warm:
  head_rate_ms    one r1_intra_head_rate_batch launch over all 8 n trials, the rng stored into the R1BlockRateTrial array
  head_commit_ms  one r1_intra_head_commit_batch launch over one winner per block (its own partition event and context
                  update with it)
  rate_ms         one r1_coeff_rate_block_batch launch over the same 8 n trials, LUMA ONLY: each trial reads the block's
                  coefficients from r1_rdo_intra_split_batch over a noise plane (the eight trials of a block share them).
                  With chroma it costs more, so the ratio below is the head's worst case
  d2h_ms, h2d_ms  COPIES ONLY of the route this removes: 24 B x n of winner states down to pinned host memory (the mode
                  and the depth the host's head contexts need) and 6 B x 8 n of rate_add and rng back up; route_wall_ms
                  is the wall clock of both copies with the synchronisation behind each
  host_python_ms  rdo_glue.head_symbols on the model's writer over the first 256 trials, scaled to 8 n: a Python
                  statement timed on the host, NOT rav1e's code -- reported apart and in no ratio
One JSON line per point: HIP-event medians after a sustained warm-up, best of two alternating rounds.  The first trials'
rate and rng and the first winners' contexts are checked against tests/head_model.py before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--points", default="16:8,32:8", help="block:transform, comma separated")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    import head_model as M
    from bench_coeff_cdf import random_context
    from rav1e_amd import rdo_glue as RG
    from rav1e_amd import workload as W
    from rav1e_amd.api import INTRA_SPLIT_CAND, Context, Plane
    from rav1e_amd.types import (BLOCK_CHAIN_CTX, BLOCK_RATE_TRIAL, COEFF_CDF_CONTEXT, HEAD_BLOCK, HEAD_CDF_CONTEXT, HEAD_COMMIT,
                                 HEAD_NBR_CONTEXT, HEAD_TRIAL, RD_PICK, TxSize)
    assert torch.cuda.is_available(), "this measures GPU time: no GPU, no number"
    ctx = Context(0)
    fw, fh, K = args.width, args.height, 8
    FX = M.load_fixture()

    def timed(f, reps=None):
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.sustain_ms:
            f()
            torch.cuda.synchronize()
        ev = []
        for _ in range(reps or args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(x.elapsed_time(y) for x, y in ev)
        return ms[len(ms) // 2]

    def wall(f, reps=9):
        f()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
        return sorted(out)[len(out) // 2]

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    org = Plane.from_numpy(W.random_plane_array(fw, fh, 8, 2), fw, fh, 8, 88, 88)
    rec = Plane.from_numpy(W.random_plane_array(fw, fh, 8, 1), fw, fh, 8, 88, 88)
    for point in args.points.split(","):
        s, t = (int(v) for v in point.split(":"))
        ts, bsize = int(TxSize.by_dims(t, t)), int(RG.block_size(s, s))
        rng = np.random.default_rng(2200 + s + t)
        bx, by = np.meshgrid(np.arange(fw // s) * s, np.arange(fh // s) * s)
        x, y = bx.ravel(), by.ravel()
        n = len(x)
        ntx, area = (s // t) ** 2, t * t
        # ---- the coefficients of every block: one r1_rdo_intra_split_batch launch
        sc = np.zeros(n, INTRA_SPLIT_CAND)
        sc["x"], sc["y"], sc["mode"] = x, y, rng.integers(0, 13, n)
        so = {"eob": torch.empty((n, 1, ntx), dtype=torch.int16, device="cuda"), "dist": torch.empty((n, 1, ntx), dtype=torch.int64, device="cuda"),
              "qcoeffs": torch.empty((n, 1, ntx, area), dtype=torch.int16, device="cuda")}
        ctx.rdo_intra_split_batch(org, rec, (0, 0, fw, fh), s, s, ts, dev(sc), 1, args.qindex, 0, n=n, want_qcoeffs=True, outs=so)
        # ---- the head's state: one seeded context pair per block, the block at its place in the frame
        seeds_n, seeds_c = FX["single_nbr"], FX["single_cdf"]
        host_n = np.ascontiguousarray(seeds_n[np.arange(n) % len(seeds_n)]).view(HEAD_NBR_CONTEXT).reshape(n)
        host_c = np.ascontiguousarray(seeds_c[np.arange(n) % len(seeds_c)]).view(HEAD_CDF_CONTEXT).reshape(n)
        dnbr, dcdf = dev(host_n).view(n, -1), dev(host_c).view(n, -1)
        blocks = np.zeros(n, HEAD_BLOCK)
        blocks["nbr"] = blocks["cdf"] = np.arange(n)
        blocks["bo_x"], blocks["bo_y"], blocks["mi_cols"], blocks["mi_rows"] = x >> 2, y >> 2, fw >> 2, fh >> 2
        blocks["bsize"], blocks["has_chroma"], blocks["tx_mode_select"] = bsize, 1, 1
        # a 2160-row frame ends inside its last 32x32 row: PARTITION_NONE is asserted against there, as in the reference
        inside = (x + s // 2 < fw) & (y + s // 2 < fh)
        trials = np.zeros(n * K, HEAD_TRIAL)
        trials["block"] = np.repeat(np.arange(n), K)
        ymodes = np.stack([rng.permutation(13)[:4] for _ in range(n)])                 # four luma modes per block
        trials["y_mode"] = np.repeat(ymodes, 2, axis=1).ravel()
        trials["uv_mode"] = np.where(np.arange(n * K) % 2 == 0, trials["y_mode"], 13)  # the luma mode again, and CFL
        trials["angle_y"], trials["angle_uv"] = rng.integers(-3, 4, n * K), rng.integers(-3, 4, n * K)
        trials["alpha_u"], trials["alpha_v"] = rng.integers(1, 17, n * K) * rng.choice([-1, 1], n * K), rng.integers(-16, 17, n * K)
        # depth 0 or depth 1 of the block
        trials["tx_size"] = np.where(rng.integers(0, 2, n * K) == 0, int(TxSize.by_dims(s, s)), int(TxSize.by_dims(s // 2, s // 2)))
        # ---- the coefficient rate over the same trials, luma only
        btr = np.zeros(n * K, BLOCK_RATE_TRIAL)
        btr["first_y"], btr["block"], btr["rng"] = np.repeat(np.arange(n) * ntx, K), np.repeat(np.arange(n), K), 0x8000
        bbl = np.zeros(n, BLOCK_CHAIN_CTX)
        for f in ("mi_w", "mi_h", "clip_w4", "clip_h4", "clip_uv_w4", "clip_uv_h4"):
            bbl[f] = 64
        bbl["y_mode"], bbl["cdf_sel"] = sc["mode"], np.arange(n) % 128
        base = dev(np.array([random_context(rng) for _ in range(4)], COEFF_CDF_CONTEXT)[np.arange(128) % 4]).view(128, -1)
        cdfs = ctx.coeff_cdf_slice_batch(base, ts, 0, False)
        dtr, dbl, dblocks, dtrials = dev(btr), dev(bbl), dev(blocks), dev(trials)
        qy, ey = so["qcoeffs"].view(n * ntx, area), so["eob"].view(n * ntx)
        ho = {"rate_add": torch.empty((n * K,), dtype=torch.int32, device="cuda")}
        bo = {"rate": torch.empty((n * K,), dtype=torch.int32, device="cuda"), "rng": torch.empty((n * K,), dtype=torch.int16, device="cuda")}
        state = np.zeros(n, RD_PICK)
        state["best_rd"], state["best_slot"] = 1.0, rng.integers(0, K, n)
        dstate = dev(state)
        commits = np.zeros(n, HEAD_COMMIT)
        commits["block"], commits["node_x"], commits["node_y"] = np.arange(n), x >> 2, y >> 2
        commits["node_bsize"], commits["part_type"], commits["subsize"] = bsize, np.where(inside, 0, 3), np.where(inside, bsize, 255)
        dcommits = dev(commits)
        head = lambda: ctx.intra_head_rate_batch(dnbr, dcdf, dblocks, dtrials, rng_into=dtr.view(n * K, -1), outs=ho)
        commit = lambda: ctx.intra_head_commit_batch(dnbr, dcdf, dblocks, dtrials, dcommits, dstate.view(n, -1), 0, 1, K)
        rate = lambda: ctx.coeff_rate_block_batch(qy, ey, 1, None, 1, dtr, s, s, ts, 1, 1, False, dbl, cdfs, want_plane_rate=False,
                                                  want_cul_level=False, want_ctx=False, outs=bo)
        host_down = torch.empty((n, 24), dtype=torch.uint8).pin_memory()
        host_up = torch.empty((n * K, 6), dtype=torch.uint8).pin_memory()
        up = torch.empty((n * K, 6), dtype=torch.uint8, device="cuda")
        d2h = lambda: host_down.copy_(dstate.view(n, 24), non_blocking=True)
        h2d = lambda: up.copy_(host_up, non_blocking=True)

        def route():
            d2h()
            torch.cuda.synchronize()
            h2d()
            torch.cuda.synchronize()
        print("# %dx%d / %dx%d: %d blocks, %d head trials" % (s, s, t, t, n, n * K), file=sys.stderr, flush=True)
        # exactness before speed: the first trials against the model, then ONE commit against it
        head()
        rate()
        torch.cuda.synchronize()
        k = 8
        got_rate = ho["rate_add"][:k * K].cpu().numpy().view(np.uint32)
        got_rng = dtr.view(n * K, -1)[:k * K].cpu().numpy().reshape(-1).view(BLOCK_RATE_TRIAL)["rng"]
        exact, refused = True, int((ho["rate_add"].cpu().numpy().view(np.uint32) == 0xFFFFFFFF).sum())
        blk_of = lambda i: tuple(int(blocks[i][f]) for f in ("bsize", "bo_x", "bo_y", "mi_cols", "mi_rows", "has_chroma", "tx_mode_select"))
        tr_of = lambda j: tuple(int(trials[j][f]) for f in ("y_mode", "uv_mode", "angle_y", "angle_uv", "alpha_u", "alpha_v", "tx_size"))
        for j in range(k * K):
            i = j // K
            want = M.head_rate(M.cdf_record(host_c[i:i + 1].view(np.uint16)), M.symbols(M.nbr_arrays(host_n[i].copy()), blk_of(i), tr_of(j)))
            exact = exact and (int(got_rate[j]), int(got_rng[j])) == want
        commit()
        torch.cuda.synchronize()
        got_n, got_c = dnbr[:k].cpu().numpy(), dcdf[:k].cpu().numpy()
        for i in range(k):
            cdf, rec_n = M.cdf_record(host_c[i:i + 1].view(np.uint16)), host_n[i].copy()
            nbr, tr = M.nbr_arrays(rec_n), tr_of(i * K + int(state["best_slot"][i]))
            M.partition_event(cdf, nbr, bsize, int(x[i]) >> 2, int(y[i]) >> 2, fw >> 2, fh >> 2, int(commits["part_type"][i]))
            M.head_commit(cdf, M.symbols(nbr, blk_of(i), tr, coded=True))
            RG.head_nbr_store(nbr, bsize, int(x[i]) >> 2, int(y[i]) >> 2, fw >> 2, fh >> 2, tr[0], tr[6], 1,
                              (int(x[i]) >> 2, int(y[i]) >> 2, bsize, bsize) if inside[i] else None)
            exact = exact and got_c[i].tobytes() == cdf.tobytes() and got_n[i].tobytes() == rec_n.tobytes()
        # the host statement in between, for scale only: Python, not rav1e
        m = min(n * K, 256)
        t0 = time.perf_counter()
        for j in range(m):
            i = j // K
            M.head_rate(M.cdf_record(host_c[i:i + 1].view(np.uint16)), M.symbols(M.nbr_arrays(host_n[i]), blk_of(i), tr_of(j)))
        host_ms = (time.perf_counter() - t0) * 1e3 * n * K / m
        runs = {"head": [], "commit": [], "rate": [], "d2h": [], "h2d": [], "route_wall": []}
        for _ in range(2):
            runs["head"].append(timed(head))
            runs["rate"].append(timed(rate))
            runs["commit"].append(timed(commit))
            runs["d2h"].append(timed(d2h, 5))
            runs["h2d"].append(timed(h2d, 5))
            runs["route_wall"].append(wall(route))
        ms = {k_: min(v) for k_, v in runs.items()}
        row = {"block": s, "tx": t, "n_blocks": n, "n_trials": n * K, "head_rate_ms": round(ms["head"], 4),
               "head_commit_ms": round(ms["commit"], 4), "rate_ms": round(ms["rate"], 4), "rate_is_luma_only": True,
               "d2h_states_ms": round(ms["d2h"], 4), "h2d_rate_add_rng_ms": round(ms["h2d"], 4), "route_wall_ms": round(ms["route_wall"], 4),
               "d2h_bytes": 24 * n, "h2d_bytes": 6 * n * K, "ms_runs": {k_: [round(v_, 4) for v_ in v] for k_, v in runs.items()},
               "head_rate_over_rate": round(ms["head"] / ms["rate"], 4),
               "head_rate_plus_commit_over_route_wall": round((ms["head"] + ms["commit"]) / ms["route_wall"], 4),
               "trials_refused_at_frame_edge": refused, "host_python_ms": round(host_ms, 1), "host_python_is_rav1e": False,
               "first_trials_equal_model": bool(exact), "copies_only": True}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        assert exact, "head rate / commit disagree with the model"
        del so, dnbr, dcdf, host_down, host_up, up
    ctx.close()


if __name__ == "__main__":
    main()

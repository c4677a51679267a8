#!/usr/bin/env python3
"""The neighbour-context gather and store beside the rate launch over the same trials, and the host route they remove,
same process, same inputs:

    python tools/bench_coeff_nbr.py [--bit-depths 8] [--points 16:8:8,16:8:0,32:8:0] [--reps 15] [--out FILE]

The 4K workloads of tools/bench_coeff_cdf.py, 4:2:0: every s x s block of a 3840x2160 luma noise plane through
r1_rdo_intra_split_batch (DCT_DCT, qcoeffs_out), the same over two 1920x1080 chroma noise planes.  One trial and ONE
R1CoeffNbrContext per block (seeded with what earlier blocks could have left), the block at its place in a one-tile frame.
A point is block:transform:n -- n = 0 takes every block (32 400 of 16x16, 8 040 of 32x32), n = 8 the launch-bound case of
one context per tile.  Per point, alternating in one process after the same pre-warm:
  gather_ms       one r1_coeff_nbr_gather_batch launch: the R1BlockChainCtx record of every block
  store_ms        one r1_coeff_nbr_store_batch launch from the rate call's ctx_out
  rate_ms         one r1_coeff_rate_block_batch launch over the same trials on the gathered records
  d2h_ms, h2d_ms  COPIES ONLY of the route this removes: 96 B x n of ctx_out to pinned host memory and 108 B x n of fresh
                  records back; route_wall_ms is the wall clock of both copies with the synchronisation behind each
  host_numpy_ms   rdo_glue.coeff_nbr_store + block_chain_ctx over the first 256 blocks, scaled to n: a NumPy / Python
                  statement timed on the host, NOT rav1e's code -- reported apart and in no ratio
One JSON line per point: HIP-event medians after a sustained warm-up, best of two alternating rounds.  The first records
and contexts are checked against rdo_glue.block_chain_ctx / coeff_nbr_store before anything is timed."""
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
    ap.add_argument("--bit-depths", default="8")
    ap.add_argument("--points", default="16:8:8,16:8:0,32:8:0", help="block:transform:n (0 = every block), comma separated")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    from bench_coeff_cdf import random_context
    from rav1e_amd import rdo_glue as RG
    from rav1e_amd import workload as W
    from rav1e_amd.api import INTRA_SPLIT_CAND, Context, Plane
    from rav1e_amd.types import BLOCK_CHAIN_CTX, BLOCK_RATE_TRIAL, COEFF_CDF_CONTEXT, COEFF_NBR_CONTEXT, NBR_BLOCK, TxSize
    assert torch.cuda.is_available(), "this measures GPU time: no GPU, no number"
    ctx = Context(0)
    fw, fh = args.width, args.height

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

    def split_launch(org, rec, w, h, s, ts, rng, bd):
        bx, by = np.meshgrid(np.arange(w // s) * s, np.arange(h // s) * s)
        x, y = bx.ravel(), by.ravel()
        n = len(x)
        t = TxSize(ts).dims[0]
        ntx, area = (s // t) ** 2, t * t
        mode = rng.integers(0, 13, n)
        direc = (mode >= 1) & (mode <= 8)
        sc = np.zeros(n, INTRA_SPLIT_CAND)
        sc["x"], sc["y"], sc["mode"] = x, y, mode
        sc["angle_delta"] = np.where(direc, rng.integers(-3, 4, n), 0)
        sc["ief"] = np.where(direc, rng.integers(1, 3, n), 0)
        sc["tr_mask"], sc["bl_mask"] = rng.integers(0, 1 << ntx, n), rng.integers(0, 1 << ntx, n)
        so = {"eob": torch.empty((n, 1, ntx), dtype=torch.int16, device="cuda"),
              "dist": torch.empty((n, 1, ntx), dtype=torch.int64, device="cuda"),
              "qcoeffs": torch.empty((n, 1, ntx, area), dtype=torch.int16 if bd == 8 else torch.int32, device="cuda")}
        ctx.rdo_intra_split_batch(org, rec, (0, 0, w, h), s, s, ts, dev(sc), 1, args.qindex, 0, n=n, want_qcoeffs=True, outs=so)
        return so, n, x, y, mode

    for bd in (int(b) for b in args.bit_depths.split(",")):
        planes = []
        for p, (w, h) in enumerate(((fw, fh), (fw // 2, fh // 2), (fw // 2, fh // 2))):
            planes.append((Plane.from_numpy(W.random_plane_array(w, h, bd, 2 + 2 * p), w, h, bd, 88, 88),
                           Plane.from_numpy(W.random_plane_array(w, h, bd, 1 + 2 * p), w, h, bd, 88, 88), w, h))
        for point in args.points.split(","):
            s, t, n_want = (int(v) for v in point.split(":"))
            ts = int(TxSize.by_dims(t, t))
            uv_ts, bw_uv, bh_uv = (int(v) for v in RG.chroma_tx_grid(RG.block_size(s, s), 1, 1))
            rng = np.random.default_rng(600 + s + t + bd)
            so, n_all, x, y, mode = split_launch(planes[0][0], planes[0][1], fw, fh, s, ts, rng, bd)
            n = n_want or n_all
            ntx, area, uv_area = (s // t) ** 2, t * t, (s // 2) ** 2
            uvo = []
            for p in (1, 2):
                a = split_launch(planes[p][0], planes[p][1], fw // 2, fh // 2, s, uv_ts, rng, bd)[0]
                b = split_launch(planes[p][1], planes[p][0], fw // 2, fh // 2, s, uv_ts, rng, bd)[0]
                uvo.append((torch.cat([a["qcoeffs"].view(-1, uv_area), b["qcoeffs"].view(-1, uv_area)])[:n].contiguous(),
                            torch.cat([a["eob"].view(-1), b["eob"].view(-1)])[:n].contiguous()))
            torch.cuda.synchronize()
            x, y, mode = x[:n], y[:n], mode[:n]
            descs = np.zeros(n, NBR_BLOCK)
            descs["nbr"], descs["bo_x"], descs["bo_y"] = np.arange(n), x >> 2, y >> 2
            descs["mi_width"] = descs["w_in_b"] = fw >> 2
            descs["mi_height"] = descs["h_in_b"] = fh >> 2
            descs["y_mode"], descs["cdf_sel"], descs["cdf_sel_uv"], descs["flags"] = mode, np.arange(n) % 128, 128 + np.arange(n) % 128, 1
            host_nbr = np.zeros(n, COEFF_NBR_CONTEXT)
            seed = rng.integers(0, 24, (64, 3, 1024)) | (rng.integers(0, 3, (64, 3, 1024)) << 6)
            host_nbr["above"] = seed[np.arange(n) % 64]
            host_nbr["left"] = seed[np.arange(n) % 64][:, :, :16]
            dnbr = dev(host_nbr).view(n, COEFF_NBR_CONTEXT.itemsize)
            trials = np.zeros(n, BLOCK_RATE_TRIAL)
            trials["first_y"], trials["first_u"], trials["first_v"] = np.arange(n) * ntx, np.arange(n), np.arange(n)
            trials["block"], trials["rng"] = np.arange(n), rng.integers(0x8000, 0x10000, n)
            trials["uv_tx_type"] = [RG.uv_tx_type_intra(int(m), uv_ts) for m in rng.integers(0, 14, n)]
            trials["do_chroma"] = 1
            base = dev(np.array([random_context(rng) for _ in range(4)], COEFF_CDF_CONTEXT)[np.arange(128) % 4]).view(128, -1)
            cdfs = torch.cat([ctx.coeff_cdf_slice_batch(base, ts, 0, False), ctx.coeff_cdf_slice_batch(base, uv_ts, 1, False)]).contiguous()
            dtr, ddesc = dev(trials), dev(descs)
            qy, ey = so["qcoeffs"].view(n_all * ntx, area)[:n * ntx].contiguous(), so["eob"].view(n_all * ntx)[:n * ntx].contiguous()
            chroma = (uvo[0][0], uvo[0][1], uvo[1][0], uvo[1][1])
            go = {"blocks": torch.empty((n, 108), dtype=torch.uint8, device="cuda")}
            bo = {"rate": torch.empty((n,), dtype=torch.int32, device="cuda"), "plane_rate": torch.empty((n, 3), dtype=torch.int32, device="cuda"),
                  "rng": torch.empty((n,), dtype=torch.int16, device="cuda"), "cul_level": torch.empty((n, 3, 16), dtype=torch.uint8, device="cuda"),
                  "ctx": torch.empty((n, 3, 2, 16), dtype=torch.uint8, device="cuda")}
            gather = lambda: ctx.coeff_nbr_gather_batch(dnbr, ddesc, s, s, 1, 1, outs=go)
            rate = lambda: ctx.coeff_rate_block_batch(qy, ey, 1, chroma, 1, dtr, s, s, ts, 1, 1, False, go["blocks"].view(-1), cdfs, outs=bo)
            store = lambda: ctx.coeff_nbr_store_batch(dnbr, ddesc, s, s, ts, 1, 1, ctx_in=bo["ctx"].view(-1))
            host_down = torch.empty((n, 96), dtype=torch.uint8).pin_memory()
            host_up = torch.empty((n, 108), dtype=torch.uint8).pin_memory()
            up = torch.empty((n, 108), dtype=torch.uint8, device="cuda")
            d2h = lambda: host_down.copy_(bo["ctx"].view(n, 96), non_blocking=True)
            h2d = lambda: up.copy_(host_up, non_blocking=True)

            def route():
                d2h()
                torch.cuda.synchronize()
                h2d()
                torch.cuda.synchronize()
            print("# %dx%d / %dx%d, %d-bit: %d blocks, one context each" % (s, s, t, t, bd, n), file=sys.stderr, flush=True)
            # exactness before speed: the first records and contexts behind ONE gather -> rate -> store
            gather()
            rate()
            store()
            torch.cuda.synchronize()
            k = min(n, 16)
            got_b = go["blocks"][:k].cpu().numpy().reshape(-1).view(BLOCK_CHAIN_CTX)
            got_n = dnbr[:k].cpu().numpy().reshape(-1).view(COEFF_NBR_CONTEXT)
            behind = bo["ctx"][:k].cpu().numpy()
            exact = bool((bo["rate"][:k].cpu().numpy().view(np.uint32) != 0xFFFFFFFF).all())
            for i in range(k):
                d = descs[i]
                want_b = np.array([RG.block_chain_ctx(host_nbr[i]["above"], host_nbr[i]["left"], int(d["bo_x"]), int(d["bo_y"]), RG.block_size(s, s),
                                                      1, 1, fw >> 2, fh >> 2, fw >> 2, fh >> 2, int(d["y_mode"]), int(d["cdf_sel"]),
                                                      int(d["cdf_sel_uv"]))], BLOCK_CHAIN_CTX)
                want_n = host_nbr[i:i + 1].copy()
                RG.coeff_nbr_store(want_n[0]["above"], want_n[0]["left"], int(d["bo_x"]), int(d["bo_y"]), RG.block_size(s, s), 1, 1, True, False, behind[i])
                exact = exact and want_b.tobytes() == got_b[i:i + 1].tobytes() and want_n.tobytes() == got_n[i:i + 1].tobytes()
            # the host statements in between, for scale only: NumPy / Python, not rav1e
            m = min(n, 256)
            t0 = time.perf_counter()
            for i in range(m):
                d = descs[i]
                RG.coeff_nbr_store(host_nbr[i]["above"], host_nbr[i]["left"], int(d["bo_x"]), int(d["bo_y"]), RG.block_size(s, s), 1, 1, True, False, behind[i % k])
                RG.block_chain_ctx(host_nbr[i]["above"], host_nbr[i]["left"], int(d["bo_x"]), int(d["bo_y"]), RG.block_size(s, s), 1, 1, fw >> 2, fh >> 2,
                                   fw >> 2, fh >> 2, 0, 0, 0)
            host_ms = (time.perf_counter() - t0) * 1e3 * n / m
            runs = {"gather": [], "store": [], "rate": [], "d2h": [], "h2d": [], "route_wall": []}
            for _ in range(2):
                runs["gather"].append(timed(gather))
                runs["rate"].append(timed(rate))
                runs["store"].append(timed(store))
                runs["d2h"].append(timed(d2h, 5))
                runs["h2d"].append(timed(h2d, 5))
                runs["route_wall"].append(wall(route))
            ms = {k_: min(v) for k_, v in runs.items()}
            row = {"block": s, "tx": t, "bd": bd, "n": n, "n_contexts": n, "gather_ms": round(ms["gather"], 4), "store_ms": round(ms["store"], 4),
                   "rate_ms": round(ms["rate"], 4), "d2h_ctx_ms": round(ms["d2h"], 4), "h2d_records_ms": round(ms["h2d"], 4),
                   "route_wall_ms": round(ms["route_wall"], 4), "d2h_bytes": 96 * n, "h2d_bytes": 108 * n,
                   "ms_runs": {k_: [round(v_, 4) for v_ in v] for k_, v in runs.items()},
                   "gather_plus_store_over_rate": round((ms["gather"] + ms["store"]) / ms["rate"], 4),
                   "gather_plus_store_over_route_wall": round((ms["gather"] + ms["store"]) / ms["route_wall"], 4),
                   "host_numpy_ms": round(host_ms, 2), "host_numpy_is_rav1e": False, "first_contexts_equal_model": bool(exact), "copies_only": True}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            assert exact, "gather / store disagree with the host statements"
            del so, uvo, bo, go, dnbr, host_down, host_up, up
    ctx.close()


if __name__ == "__main__":
    main()

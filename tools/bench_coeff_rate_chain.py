#!/usr/bin/env python3
"""The real coefficient rate across a block's transform blocks beside what it replaces, same process, same inputs:

    python tools/bench_coeff_rate_chain.py [--bit-depths 8,10] [--points 16:8,16:4,32:8] [--reps 15] [--out FILE]

Behind the 4K launches of tools/bench_intra_split.py: every s x s block of a 3840x2160 luma plane x K = 4 intra modes
through r1_rdo_intra_split_batch (DCT_DCT, transform-domain distortion, qcoeffs_out), which leaves eob / qcoeffs for
every (block, mode, transform block) in HBM.  Per point (block s : transform t, bit depth), alternating in one process:
  chain_ms        one r1_coeff_rate_chain_batch launch (order 0) on those buffers: n trials of ntx transform blocks each,
                  five CDF snapshots, random neighbour contexts, every output
  independent_ms  one r1_coeff_rate_batch launch over the SAME transform blocks as n * ntx independent slots: the same
                  symbol count at full parallelism, the WRONG rate (nothing carried) -- the cost floor of the symbols
  d2h_ms          the device-to-host copy of qcoeffs + eob into pinned memory that the device route removes (the host's
                  entropy coder behind it is NOT timed)
One JSON line per point: HIP-event medians after a sustained warm-up, best of two alternating rounds, the mean eob.  The
first trials are checked against the Python model of tests/coeff_rate_chain_model.py before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bit-depths", default="8,10")
    ap.add_argument("--points", default="16:8,16:4,32:8", help="block:transform, comma separated")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    import coeff_rate_model as M
    import coeff_rate_chain_model as CM
    from rav1e_amd import workload as W
    from rav1e_amd.api import INTRA_SPLIT_CAND, Context, Plane
    from rav1e_amd.types import TXB_CHAIN_CTX, TxSize
    assert torch.cuda.is_available(), "this measures GPU time: no GPU, no number"
    ctx = Context(0)
    fw, fh, K = args.width, args.height, args.k

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

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    for bd in (int(b) for b in args.bit_depths.split(",")):
        rec = Plane.from_numpy(W.random_plane_array(fw, fh, bd, 1), fw, fh, bd, 88, 88)
        org = Plane.from_numpy(W.random_plane_array(fw, fh, bd, 2), fw, fh, bd, 88, 88)
        for point in args.points.split(","):
            s, t = (int(v) for v in point.split(":"))
            ts = int(TxSize.by_dims(t, t))
            rng = np.random.default_rng(300 + s + t + bd)
            nbx, nby = fw // s, fh // s
            bx, by = np.meshgrid(np.arange(nbx) * s, np.arange(nby) * s)
            bx, by = bx.ravel(), by.ravel()
            nb = len(bx)
            n = nb * K
            ntx, area = (s // t) ** 2, t * t
            mode = np.argsort(rng.random((nb, 13)), axis=1)[:, :K].T.ravel()
            x, y = np.tile(bx, K), np.tile(by, K)
            direc = (mode >= 1) & (mode <= 8)
            sc = np.zeros(n, INTRA_SPLIT_CAND)
            sc["x"], sc["y"], sc["mode"] = x, y, mode
            sc["angle_delta"] = np.where(direc, rng.integers(-3, 4, n), 0)
            sc["ief"] = np.where(direc, np.tile(rng.integers(1, 3, nb), K), 0)
            sc["tr_mask"], sc["bl_mask"] = rng.integers(0, 1 << ntx, n), rng.integers(0, 1 << ntx, n)
            cdt = torch.int16 if bd == 8 else torch.int32
            so = {"eob": torch.empty((n, 1, ntx), dtype=torch.int16, device="cuda"),
                  "dist": torch.empty((n, 1, ntx), dtype=torch.int64, device="cuda"),
                  "qcoeffs": torch.empty((n, 1, ntx, area), dtype=cdt, device="cuda")}
            ctx.rdo_intra_split_batch(org, rec, (0, 0, fw, fh), s, s, ts, dev(sc), 1, args.qindex, 0, n=n, want_qcoeffs=True,
                                      outs=so)
            torch.cuda.synchronize()
            # the descriptors: neighbour contexts as a coded frame spreads them, the frame's own edges, five snapshots
            cdfs = M.random_cdfs(rng, 5, ts, 0, 0)
            chains = np.zeros(n, TXB_CHAIN_CTX)
            chains["above"] = rng.integers(0, 24, (n, 16)) | (rng.integers(0, 3, (n, 16)) << 6)
            chains["left"] = rng.integers(0, 24, (n, 16)) | (rng.integers(0, 3, (n, 16)) << 6)
            chains["mi_w"] = chains["clip_w4"] = np.minimum(255, (fw - x) >> 2)
            chains["mi_h"] = chains["clip_h4"] = np.minimum(255, (fh - y) >> 2)
            chains["y_mode"], chains["cdf_sel"] = mode, rng.integers(0, 5, n)
            ctxs = M.random_ctxs(rng, n * ntx, 5)
            dch, dcdf, dctx = dev(chains), dev(cdfs), dev(ctxs)
            co = {"rate": torch.empty((n, 1), dtype=torch.int32, device="cuda"),
                  "txb_rate": torch.empty((n, 1, ntx), dtype=torch.int32, device="cuda"),
                  "cul_level": torch.empty((n, 1, ntx), dtype=torch.uint8, device="cuda"),
                  "ctx": torch.empty((n, 1, 32), dtype=torch.uint8, device="cuda")}
            io = {"rate": torch.empty((n * ntx, 1), dtype=torch.int32, device="cuda"),
                  "cul_level": torch.empty((n * ntx, 1), dtype=torch.uint8, device="cuda")}
            q_flat, e_flat = so["qcoeffs"].view(n * ntx, 1, area), so["eob"].view(n * ntx, 1)
            chain = lambda: ctx.coeff_rate_chain_batch(so["qcoeffs"], so["eob"], 1, s, s, ts, 0, False, dch, dcdf, outs=co)
            indep = lambda: ctx.coeff_rate_batch(q_flat, e_flat, 1, ts, 0, False, dctx, dcdf, outs=io)
            hq = torch.empty((n, ntx, area), dtype=cdt).pin_memory()
            he = torch.empty((n, ntx), dtype=torch.int16).pin_memory()

            def d2h():
                hq.copy_(so["qcoeffs"].view(n, ntx, area), non_blocking=True)
                he.copy_(so["eob"].view(n, ntx), non_blocking=True)
            print("# %dx%d / %dx%d, %d-bit: %d trials x %d transform blocks" % (s, s, t, t, bd, n, ntx), file=sys.stderr, flush=True)
            chain()
            indep()
            torch.cuda.synchronize()
            # exactness before speed: the first trials against the model
            k = min(n, 48)
            qh = so["qcoeffs"][:k].cpu().numpy().reshape(k * ntx, -1)
            eh = so["eob"][:k].cpu().numpy().view(np.uint16).ravel()
            want = CM.coeff_rate_chain_batch(qh, eh, 1, s, s, ts, 0, 0, 0, chains[:k], cdfs)
            exact = bool(np.array_equal(co["rate"][:k].cpu().numpy().view(np.uint32).ravel(), want[0]) and
                         np.array_equal(co["txb_rate"][:k].cpu().numpy().view(np.uint32).reshape(k, ntx), want[1]) and
                         np.array_equal(co["cul_level"][:k].cpu().numpy().reshape(k, ntx), want[2]) and
                         np.array_equal(co["ctx"][:k].cpu().numpy().reshape(k, 32), want[3]))
            eobs_all = so["eob"].cpu().numpy().view(np.uint16)
            carried = float((co["rate"].view(-1).cpu().numpy().view(np.uint32).astype(np.int64) !=
                             io["rate"].view(n, ntx).cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=1)).mean())
            runs = {"chain": [], "independent": [], "d2h": []}
            for _ in range(2):
                runs["chain"].append(timed(chain))
                runs["independent"].append(timed(indep))
                runs["d2h"].append(timed(d2h, 5))
            ms = {k_: min(v) for k_, v in runs.items()}
            row = {"block": s, "tx": t, "ntx": ntx, "bd": bd, "n_trials": n, "k": K, "transform_blocks": n * ntx,
                   "mean_eob": round(float(eobs_all.mean()), 2), "max_eob": int(eobs_all.max()),
                   "nonzero_eob_share": round(float((eobs_all != 0).mean()), 3),
                   "chain_ms": round(ms["chain"], 4), "independent_ms": round(ms["independent"], 4),
                   "d2h_qcoeffs_eob_ms": round(ms["d2h"], 4), "d2h_bytes": int(hq.numel() * hq.element_size() + he.numel() * 2),
                   "ms_runs": {k_: [round(v_, 4) for v_ in v] for k_, v in runs.items()},
                   "chain_over_independent": round(ms["chain"] / ms["independent"], 4),
                   "chain_over_d2h": round(ms["chain"] / ms["d2h"], 4),
                   "trials_per_s": round(n / (ms["chain"] * 1e-3)),
                   "share_of_trials_whose_rate_differs_from_the_independent_sum": round(carried, 4),
                   "first_trials_equal_model": exact, "host_entropy_coder_timed": False}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            assert exact, "the chain launch disagrees with the model"
            del so, co, io, hq, he
    ctx.close()


if __name__ == "__main__":
    main()

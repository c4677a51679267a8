#!/usr/bin/env python3
"""The whole-block coefficient rate (luma, U, V on one writer) beside what the parent could do, same process, same inputs:

    python tools/bench_coeff_rate_block.py [--bit-depths 8,10] [--points 16:8,16:4,32:8] [--reps 15] [--out FILE]

Behind the 4K launches of tools/bench_coeff_rate_chain.py, in 4:2:0: every s x s block of a 3840x2160 luma noise plane x
K = 4 intra modes through r1_rdo_intra_split_batch (DCT_DCT, qcoeffs_out) leaves eob / qcoeffs of every (block, mode,
transform block) in HBM; the same launch over two 1920x1080 chroma noise planes with transforms of s / 2 leaves one
chroma transform block per trial and plane.  Per point (block s : luma transform t, bit depth), alternating in
one process after the same pre-warm:
  block_ms        (a) one r1_coeff_rate_block_batch launch: n trials of ntx luma + 1 U + 1 V transform blocks, ten CDF
                  snapshots (five luma, five chroma), random neighbour contexts and hand-over rng, every output
  parts_ms        (b) what the parent has: r1_coeff_rate_chain_batch on luma plus two r1_coeff_rate_batch launches on U
                  and V -- the cost floor, with the WRONG rate (three fresh writers, V not behind U)
  d2h_ms          (c) the device-to-host copy of the three planes' qcoeffs + eob into pinned memory that the device
                  route removes (the host's entropy coder behind it is NOT timed)
  luma_block_ms / luma_chain_ms   the same luma inputs through the new kernel (do_chroma = 0, rng = 0x8000) and through
                  r1_coeff_rate_chain_batch: the same body, so the ratio shows what the added planes cost a luma chain
One JSON line per point: HIP-event medians after a sustained warm-up, best of two alternating rounds.  The first trials
are checked against the Python model of tests/coeff_rate_block_model.py before anything is timed, and the luma-only
rates against the chain launch."""
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
    import coeff_rate_block_model as BM
    from rav1e_amd import rdo_glue as RG
    from rav1e_amd import workload as W
    from rav1e_amd.api import INTRA_SPLIT_CAND, Context, Plane
    from rav1e_amd.types import BLOCK_CHAIN_CTX, BLOCK_RATE_TRIAL, TXB_CHAIN_CTX, TxSize
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

    def split_launch(org, rec, w, h, s, ts, K_, rng, bd):
        """every s x s block of the plane x K_ modes through r1_rdo_intra_split_batch -> (outs, n, x, y, mode)"""
        nbx, nby = w // s, h // s
        bx, by = np.meshgrid(np.arange(nbx) * s, np.arange(nby) * s)
        bx, by = bx.ravel(), by.ravel()
        nb = len(bx)
        n = nb * K_
        t = TxSize(ts).dims[0]
        ntx, area = (s // t) ** 2, t * t
        mode = np.argsort(rng.random((nb, 13)), axis=1)[:, :K_].T.ravel()
        x, y = np.tile(bx, K_), np.tile(by, K_)
        direc = (mode >= 1) & (mode <= 8)
        sc = np.zeros(n, INTRA_SPLIT_CAND)
        sc["x"], sc["y"], sc["mode"] = x, y, mode
        sc["angle_delta"] = np.where(direc, rng.integers(-3, 4, n), 0)
        sc["ief"] = np.where(direc, np.tile(rng.integers(1, 3, nb), K_), 0)
        sc["tr_mask"], sc["bl_mask"] = rng.integers(0, 1 << ntx, n), rng.integers(0, 1 << ntx, n)
        cdt = torch.int16 if bd == 8 else torch.int32
        so = {"eob": torch.empty((n, 1, ntx), dtype=torch.int16, device="cuda"),
              "dist": torch.empty((n, 1, ntx), dtype=torch.int64, device="cuda"),
              "qcoeffs": torch.empty((n, 1, ntx, area), dtype=cdt, device="cuda")}
        ctx.rdo_intra_split_batch(org, rec, (0, 0, w, h), s, s, ts, dev(sc), 1, args.qindex, 0, n=n, want_qcoeffs=True, outs=so)
        return so, n, x, y, mode

    for bd in (int(b) for b in args.bit_depths.split(",")):
        planes = []
        for p, (w, h) in enumerate(((fw, fh), (fw // 2, fh // 2), (fw // 2, fh // 2))):
            planes.append((Plane.from_numpy(W.random_plane_array(w, h, bd, 2 + 2 * p), w, h, bd, 88, 88),
                           Plane.from_numpy(W.random_plane_array(w, h, bd, 1 + 2 * p), w, h, bd, 88, 88), w, h))
        for point in args.points.split(","):
            s, t = (int(v) for v in point.split(":"))
            ts = int(TxSize.by_dims(t, t))
            bsize = RG.block_size(s, s)
            uv_ts, bw_uv, bh_uv = (int(v) for v in RG.chroma_tx_grid(bsize, 1, 1))
            assert (bw_uv, bh_uv) == (1, 1) and TxSize(uv_ts).dims == (s // 2, s // 2)
            rng = np.random.default_rng(400 + s + t + bd)
            so, n, x, y, mode = split_launch(planes[0][0], planes[0][1], fw, fh, s, ts, K, rng, bd)
            ntx, area, uv_area = (s // t) ** 2, t * t, (s // 2) ** 2
            # chroma: blocks of s with transforms of s / 2 -- four chroma transform blocks per launch block; K modes over
            # a quarter as many blocks gives one chroma transform block per luma trial and plane
            # (one mode more: 1080 rows hold no whole number of blocks); the first n of them are used
            uvo = [split_launch(planes[p][0], planes[p][1], fw // 2, fh // 2, s, uv_ts, K + 1, rng, bd)[0] for p in (1, 2)]
            torch.cuda.synchronize()
            assert uvo[0]["eob"].numel() >= n, (uvo[0]["eob"].numel(), n)
            n_uv = n
            # the descriptors: neighbour contexts as a coded frame spreads them, the frame's own edges, ten snapshots
            cdfs = np.concatenate([M.random_cdfs(rng, 5, ts, 0, 0), M.random_cdfs(rng, 5, uv_ts, 0, 0)])
            blocks = np.zeros(n, BLOCK_CHAIN_CTX)
            blocks["ctx"] = rng.integers(0, 24, (n, 3, 2, 16)) | (rng.integers(0, 3, (n, 3, 2, 16)) << 6)
            blocks["mi_w"] = blocks["clip_w4"] = np.minimum(255, (fw - x) >> 2)
            blocks["mi_h"] = blocks["clip_h4"] = np.minimum(255, (fh - y) >> 2)
            blocks["clip_uv_w4"] = np.minimum(255, (fw - x) >> 3)
            blocks["clip_uv_h4"] = np.minimum(255, (fh - y) >> 3)
            blocks["y_mode"], blocks["cdf_sel"], blocks["cdf_sel_uv"] = mode, rng.integers(0, 5, n), rng.integers(5, 10, n)
            trials = np.zeros(n, BLOCK_RATE_TRIAL)
            trials["first_y"], trials["first_u"], trials["first_v"] = np.arange(n) * ntx, np.arange(n), np.arange(n)
            trials["block"], trials["rng"] = np.arange(n), rng.integers(0x8000, 0x10000, n)
            trials["uv_tx_type"] = [RG.uv_tx_type_intra(int(m), uv_ts) for m in rng.integers(0, 14, n)]
            trials["do_chroma"] = 1
            luma_trials = trials.copy()
            luma_trials["do_chroma"], luma_trials["rng"] = 0, 0x8000
            chains = np.zeros(n, TXB_CHAIN_CTX)
            chains["above"], chains["left"] = blocks["ctx"][:, 0, 0], blocks["ctx"][:, 0, 1]
            for f in ("mi_w", "mi_h", "clip_w4", "clip_h4", "y_mode", "cdf_sel"):
                chains[f] = blocks[f]
            uv_ctxs = [M.random_ctxs(rng, n_uv, 5) for _ in range(2)]
            for c_ in uv_ctxs:
                c_["txb_skip_ctx"] = rng.integers(7, 10, n_uv)
                c_["cdf_sel"] += 5
            dtr, dlt, dbl, dch, dcdf = dev(trials), dev(luma_trials), dev(blocks), dev(chains), dev(cdfs)
            dux = [dev(c_) for c_ in uv_ctxs]
            qy, ey = so["qcoeffs"].view(n * ntx, area), so["eob"].view(n * ntx)
            chroma = (uvo[0]["qcoeffs"].view(-1, uv_area)[:n], uvo[0]["eob"].view(-1)[:n], uvo[1]["qcoeffs"].view(-1, uv_area)[:n],
                      uvo[1]["eob"].view(-1)[:n])

            def outs_block():
                return {"rate": torch.empty((n,), dtype=torch.int32, device="cuda"),
                        "plane_rate": torch.empty((n, 3), dtype=torch.int32, device="cuda"),
                        "rng": torch.empty((n,), dtype=torch.int16, device="cuda"),
                        "cul_level": torch.empty((n, 3, 16), dtype=torch.uint8, device="cuda"),
                        "ctx": torch.empty((n, 3, 2, 16), dtype=torch.uint8, device="cuda")}
            bo, lo = outs_block(), outs_block()
            co = {"rate": torch.empty((n, 1), dtype=torch.int32, device="cuda"),
                  "txb_rate": torch.empty((n, 1, ntx), dtype=torch.int32, device="cuda"),
                  "cul_level": torch.empty((n, 1, ntx), dtype=torch.uint8, device="cuda"),
                  "ctx": torch.empty((n, 1, 32), dtype=torch.uint8, device="cuda")}
            io = [{"rate": torch.empty((n_uv, 1), dtype=torch.int32, device="cuda"),
                   "cul_level": torch.empty((n_uv, 1), dtype=torch.uint8, device="cuda")} for _ in range(2)]
            block = lambda: ctx.coeff_rate_block_batch(qy, ey, 1, chroma, 1, dtr, s, s, ts, 1, 1, False, dbl, dcdf, outs=bo)
            luma_block = lambda: ctx.coeff_rate_block_batch(qy, ey, 1, chroma, 1, dlt, s, s, ts, 1, 1, False, dbl, dcdf, outs=lo)
            chain = lambda: ctx.coeff_rate_chain_batch(so["qcoeffs"], so["eob"], 1, s, s, ts, 0, False, dch, dcdf, outs=co)

            def parts():
                chain()
                for p in range(2):
                    ctx.coeff_rate_batch(chroma[2 * p].view(n_uv, 1, uv_area), chroma[2 * p + 1].view(n_uv, 1), 1, uv_ts, 1 + p,
                                         False, dux[p], dcdf, outs=io[p])
            host = [torch.empty(tuple(t_.shape), dtype=t_.dtype).pin_memory() for t_ in (qy, ey) + chroma]

            def d2h():
                for h_, t_ in zip(host, (qy, ey) + chroma):
                    h_.copy_(t_, non_blocking=True)
            print("# %dx%d / %dx%d + 2 x %dx%d, %d-bit: %d trials x (%d + 2) transform blocks" % (s, s, t, t, s // 2, s // 2, bd, n, ntx),
                  file=sys.stderr, flush=True)
            block()
            luma_block()
            parts()
            torch.cuda.synchronize()
            # exactness before speed: the first trials against the model, the luma-only launch against the chain
            k = min(n, 32)
            hp = [(chroma[2 * p].cpu().numpy(), chroma[2 * p + 1].cpu().numpy().view(np.uint16)) for p in range(2)]
            want = BM.coeff_rate_block_batch([(qy.cpu().numpy(), ey.cpu().numpy().view(np.uint16)), hp[0], hp[1]], (1, 1), s, s, ts, 1, 1,
                                             0, 0, trials[:k], blocks, cdfs)
            exact = bool(np.array_equal(bo["rate"][:k].cpu().numpy().view(np.uint32), want[0]) and
                         np.array_equal(bo["plane_rate"][:k].cpu().numpy().view(np.uint32), want[1]) and
                         np.array_equal(bo["rng"][:k].cpu().numpy().view(np.uint16), want[2]) and
                         np.array_equal(bo["cul_level"][:k].cpu().numpy(), want[3]) and
                         np.array_equal(bo["ctx"][:k].cpu().numpy(), want[4]))
            luma_equal = bool(torch.equal(lo["rate"], co["rate"].view(-1)) and
                              torch.equal(lo["ctx"][:, 0].reshape(n, 32), co["ctx"].view(n, 32)))
            parts_sum = (co["rate"].view(-1).cpu().numpy().view(np.uint32).astype(np.int64) +
                         sum(io[p]["rate"].view(-1)[:n].cpu().numpy().view(np.uint32).astype(np.int64) for p in range(2)))
            differs = float((bo["rate"].cpu().numpy().view(np.uint32).astype(np.int64) != parts_sum).mean())
            eobs_y = ey.cpu().numpy().view(np.uint16)
            eobs_uv = np.concatenate([hp[0][1][:n], hp[1][1][:n]])
            runs = {"block": [], "parts": [], "d2h": [], "luma_block": [], "luma_chain": []}
            for _ in range(2):
                runs["block"].append(timed(block))
                runs["parts"].append(timed(parts))
                runs["d2h"].append(timed(d2h, 5))
                runs["luma_block"].append(timed(luma_block))
                runs["luma_chain"].append(timed(chain))
            ms = {k_: min(v) for k_, v in runs.items()}
            row = {"block": s, "tx": t, "uv_tx": s // 2, "ntx": ntx, "bd": bd, "n_trials": n, "k": K,
                   "transform_blocks": n * (ntx + 2), "mean_eob_y": round(float(eobs_y.mean()), 2),
                   "mean_eob_uv": round(float(eobs_uv.mean()), 2), "max_eob": int(max(eobs_y.max(), eobs_uv.max())),
                   "block_ms": round(ms["block"], 4), "parts_ms": round(ms["parts"], 4),
                   "d2h_qcoeffs_eob_ms": round(ms["d2h"], 4), "d2h_bytes": int(sum(h_.numel() * h_.element_size() for h_ in host)),
                   "luma_block_ms": round(ms["luma_block"], 4), "luma_chain_ms": round(ms["luma_chain"], 4),
                   "ms_runs": {k_: [round(v_, 4) for v_ in v] for k_, v in runs.items()},
                   "block_over_parts": round(ms["block"] / ms["parts"], 4), "block_over_d2h": round(ms["block"] / ms["d2h"], 4),
                   "luma_block_over_chain": round(ms["luma_block"] / ms["luma_chain"], 4),
                   "trials_per_s": round(n / (ms["block"] * 1e-3)),
                   "share_of_trials_whose_rate_differs_from_the_sum_of_parts": round(differs, 4),
                   "first_trials_equal_model": exact, "luma_only_equals_chain": luma_equal, "host_entropy_coder_timed": False}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            assert exact, "the block launch disagrees with the model"
            assert luma_equal, "the luma-only block launch disagrees with the chain launch"
            del so, uvo, bo, lo, co, io, host
    ctx.close()


if __name__ == "__main__":
    main()

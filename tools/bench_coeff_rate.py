#!/usr/bin/env python3
"""The real coefficient rate on the device beside the launch that feeds it, same box, same inputs:

    python tools/bench_coeff_rate.py [--k 4] [--reps 15] [--sizes 8,16,32] [--bit-depths 8,10] [--out FILE]

The type-search workload of tools/bench_txsearch.py: n = K predictions per block of a 3840x2160 plane (speed-6 ladder
candidates), mask = RAV1E_TX_TYPES cut by the inter tx set, cdef_dist distortion.  Per (size, bit depth), in one run:
  txsearch_ms   one r1_rdo_txsearch_batch launch with qcoeffs_out (the launch that feeds the rate; unchanged code)
  rate_ms       one r1_coeff_rate_batch launch on its (n, nt) slots, five CDF snapshots, random contexts
  d2h_ms        the device-to-host copy of qcoeffs + eob into pinned memory that the device route makes unnecessary --
                the only part of the host route measurable here: the host's entropy coder itself is NOT timed
One JSON line per (size, bit depth); medians of HIP-event times after a sustained warm-up.  The rates of the first 64
slots are checked against the Python model of tests/coeff_rate_model.py before anything is timed."""
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
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kind", type=int, default=3)
    ap.add_argument("--sizes", default="8,16,32")
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    import coeff_rate_model as M
    from rav1e_amd import rdo_glue as RG, workload as W
    from rav1e_amd.api import Context, Plane
    from rav1e_amd.types import COEFF_CDFS, TXB_CTX, TxSize
    assert torch.cuda.is_available(), "this measures GPU time: no GPU, no number"
    ctx = Context(0)
    fw, fh = args.width, args.height
    sizes = [int(s) for s in args.sizes.split(",")]

    def timed(f, reps=None):
        # warm up for sustain-ms of DEVICE time: a synchronise per call, so that a slow call (the 1 GB copy) cannot
        # pile thousands of enqueued repeats behind the clock the loop watches
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

    for bd in [int(b) for b in args.bit_depths.split(",")]:
        a = W.random_plane_array(fw, fh, bd, 1)
        b = np.clip(a.astype(np.int64) + np.random.default_rng(5).integers(-6 << (bd - 8), (6 << (bd - 8)) + 1, a.shape), 0,
                    (1 << bd) - 1).astype(a.dtype)
        org, ref = Plane.from_numpy(a, fw, fh, bd, 88, 88), Plane.from_numpy(b, fw, fh, bd, 88, 88)
        scales = torch.from_numpy(np.random.default_rng(9).integers(1 << 12, 1 << 16, ((fh + 7) // 8, (fw + 7) // 8)).astype(np.int32)).cuda()
        cands = W.speed6_ladder(fw, fh, args.k, mv_range=4, sizes=sizes)
        for s in sizes:
            c = cands[s]
            n = len(c)
            ts = int(TxSize.by_dims(s, s))
            mask = ctx.tx_type_mask(ts, True)
            types = RG.tx_type_slots(mask)
            nt = len(types)
            area = min(s, 32) ** 2
            rng = np.random.default_rng(100 + s + bd)
            # five snapshots: valid CDFs with adapted counters; contexts as a frame would spread them
            cdfs = M.random_cdfs(rng, 5, ts, 1, 0)
            ctxs = M.random_ctxs(rng, n, 5)
            dcdf = torch.from_numpy(cdfs.view(np.uint8).reshape(5, -1).copy()).cuda()
            dctx = torch.from_numpy(ctxs.view(np.uint8).reshape(n, 4).copy()).cuda()
            assert cdfs.dtype == COEFF_CDFS and ctxs.dtype == TXB_CTX
            dev = torch.from_numpy(c.view(np.uint8).reshape(-1).copy()).cuda()
            cdt = torch.int16 if bd == 8 else torch.int32
            fo = {"eob": torch.empty((n, nt), dtype=torch.int16, device="cuda"),
                  "dist": torch.empty((n, nt), dtype=torch.int64, device="cuda"),
                  "qcoeffs": torch.empty((n, nt, area), dtype=cdt, device="cuda")}
            ro = {"rate": torch.empty((n, nt), dtype=torch.int32, device="cuda"),
                  "cul_level": torch.empty((n, nt), dtype=torch.uint8, device="cuda")}
            sc = scales if args.kind else None
            search = lambda: ctx.rdo_txsearch_batch(org, ref, s, s, dev, mask, args.qindex, args.kind, scales=sc, n=n,
                                                    want_qcoeffs=True, outs=fo)
            rate = lambda: ctx.coeff_rate_batch(fo["qcoeffs"], fo["eob"], mask, ts, 0, True, dctx, dcdf, outs=ro)
            hq = torch.empty((n, nt, area), dtype=cdt).pin_memory()
            he = torch.empty((n, nt), dtype=torch.int16).pin_memory()

            def d2h():
                hq.copy_(fo["qcoeffs"], non_blocking=True)
                he.copy_(fo["eob"], non_blocking=True)
            print("# size %d, %d-bit: %d candidates x %d types" % (s, bd, n, nt), file=sys.stderr, flush=True)
            search()
            rate()
            torch.cuda.synchronize()
            # exactness before speed: the first slots against the model
            k = min(n, 64 // nt + 1)
            qh = fo["qcoeffs"][:k].cpu().numpy().reshape(k * nt, -1)
            eh = fo["eob"][:k].cpu().numpy().view(np.uint16).ravel()
            wr, wc = M.coeff_rate_batch(qh, eh, mask, ts, 0, 1, 0, ctxs[:k], cdfs)
            exact = bool(np.array_equal(ro["rate"][:k].cpu().numpy().view(np.uint32).ravel(), wr) and
                         np.array_equal(ro["cul_level"][:k].cpu().numpy().ravel(), wc))
            eobs_all = fo["eob"].cpu().numpy().view(np.uint16)
            ms_search = timed(search)
            ms_rate = timed(rate)
            ms_d2h = timed(d2h, 5)
            ms_search2 = timed(search)       # once more after the others: all saw the same clocks
            ms_rate2 = timed(rate)
            row = {"size": s, "bd": bd, "kind": args.kind, "n": n, "types": types, "slots": n * nt,
                   "mean_eob": round(float(eobs_all.mean()), 2), "max_eob": int(eobs_all.max()),
                   "txsearch_ms": round(min(ms_search, ms_search2), 4), "txsearch_ms_runs": [round(ms_search, 4), round(ms_search2, 4)],
                   "rate_ms": round(min(ms_rate, ms_rate2), 4), "rate_ms_runs": [round(ms_rate, 4), round(ms_rate2, 4)],
                   "rate_over_txsearch": round(min(ms_rate, ms_rate2) / min(ms_search, ms_search2), 4),
                   "d2h_qcoeffs_eob_ms": round(ms_d2h, 4), "d2h_bytes": int(hq.numel() * hq.element_size() + he.numel() * 2),
                   "slots_per_s": round(n * nt / (min(ms_rate, ms_rate2) * 1e-3)), "first_slots_equal_model": exact,
                   "host_entropy_coder_timed": False}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            assert exact, "the rate launch disagrees with the model"
    ctx.close()


if __name__ == "__main__":
    main()

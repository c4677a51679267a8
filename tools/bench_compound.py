#!/usr/bin/env python3
"""The compound (two-reference) candidate in one launch against what the library offered before it, same
process, same inputs:

    python tools/bench_compound.py [--bit-depth 8|10] [--sizes 16,8,32,64] [--k 8] [--reps 20]

For every size: every s x s block of a 3840x2160 plane (BASELINE.json configs[3], padding 88) x K = 8 compound
candidates -- the eight RAV1E_INTER_COMPOUND_MODES of the inter pre-screen on one reference pair; each
reference's motion vectors drawn as workload.speed6_ladder draws them (uniform full pels, 1/16-pel fractions).
  (a) compound     ONE r1_rdo_compound_cand_batch launch: satd_out only (the pre-screen), satd_out + pred_out
                   (a survivor), pred_out only (predict_inter_compound alone)
  (b) three-launch r1_mc_prep_batch x 2 -> r1_mc_avg_batch for the prediction (two int16 intermediates and the
                   prediction through HBM), then the CHEAPEST existing route to the SATD of a dense prediction:
                   r1_rdo_pred_cand_batch with dist_kind 0 (transform-domain distortion, no inverse transform,
                   SAD off) -- a quantizing kernel, because nothing else takes a dense prediction.  (r1_dist_batch
                   could read the buffer as a plane of stride s, but its int16 ry addresses 32767 / s blocks per
                   launch: over a hundred launches per size here.  Not a route a caller would take.)
Both legs are checked for identical predictions and SATDs first, then timed alternately (a, b, a, b; HIP events on
the launch stream, warm-up and a sustain window before every timed series, median of --reps).  One JSON line per
size: the times of every leg and run, the ratios, and the bytes each leg moves (counted from the shapes:
descriptors, windows, source blocks, intermediates, outputs)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg_bytes(s, bpp, n):
    """bytes per leg from the shapes: what each launch has to read and write at least once"""
    win, blk = (s + 7) * (s + 7) * bpp, s * s * bpp
    a_satd = 20 + 2 * win + blk + 4
    b_pred = 2 * (8 + win + 2 * s * s) + (2 * 2 * s * s + blk)         # prep x 2 (window in, int16 out), avg
    b_satd = 16 + 2 * blk + 2 + 8 + 4                                  # prediction + source in; eob, dist, satd out
    return {"compound_satd": n * a_satd, "compound_satd_pred": n * (a_satd + blk), "compound_pred": n * (20 + 2 * win + blk),
            "three_launch_pred": n * b_pred, "three_launch_pred_satd": n * (b_pred + b_satd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bit-depth", type=int, default=10)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="16,8,32,64")
    ap.add_argument("--mv-range", type=int, default=32)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    args = ap.parse_args()
    import time
    import torch
    from rav1e_amd import workload as W
    from rav1e_amd.api import COMPOUND_CAND, MC_CAND, RDO_CAND, Context, Plane, _pix_dtype
    assert torch.cuda.is_available(), "bench_compound.py measures on a GPU; there is nothing to report without one"
    ctx = Context(0)
    fw, fh, bd = args.width, args.height, args.bit_depth
    bpp = 1 if bd == 8 else 2
    planes = [Plane.from_numpy(W.random_plane_array(fw, fh, bd, seed), fw, fh, bd, 88, 88) for seed in (1, 2, 3)]
    org, ref0, ref1 = planes
    sizes = [int(s) for s in args.sizes.split(",")]
    mv = [W.speed6_ladder(fw, fh, args.k, seed=sd, mv_range=args.mv_range, sizes=sizes) for sd in (3, 4)]

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

    for s in sizes:
        c0, c1 = mv[0][s], mv[1][s]
        n = len(c0)
        cc, mcs = np.zeros(n, COMPOUND_CAND), []
        cc["ox"], cc["oy"] = c0["ox"], c0["oy"]
        for i, c in enumerate((c0, c1)):
            m = np.zeros(n, MC_CAND)
            for f in ("rx", "ry", "col_frac", "row_frac"):
                cc[f + str(i)] = m[f] = c[f]
            mcs.append(dev(m))
        rc = np.zeros(n, RDO_CAND)
        rc["ox"], rc["oy"] = c0["ox"], c0["oy"]
        d_cc, d_rc = dev(cc), dev(rc)
        # outputs of both legs, allocated once
        a_satd = {"satd": torch.empty(n, dtype=torch.int32, device="cuda")}
        a_both = {"satd": torch.empty(n, dtype=torch.int32, device="cuda"),
                  "pred": torch.empty((n, s, s), dtype=_pix_dtype(bpp), device="cuda")}
        tmp = [torch.empty((n, s, s), dtype=torch.int16, device="cuda") for _ in range(2)]
        b_pred = torch.empty((n, s, s), dtype=_pix_dtype(bpp), device="cuda")
        b_out = {"eob": torch.empty(n, dtype=torch.int16, device="cuda"), "dist": torch.empty(n, dtype=torch.int64, device="cuda"),
                 "satd": torch.empty(n, dtype=torch.int32, device="cuda")}

        def leg_a_satd():
            ctx.rdo_compound_cand_batch(org, ref0, ref1, s, s, d_cc, n=n, outs=a_satd)

        def leg_a_both():
            ctx.rdo_compound_cand_batch(org, ref0, ref1, s, s, d_cc, n=n, want_pred=True, outs=a_both)

        def leg_a_pred():
            ctx.rdo_compound_cand_batch(org, ref0, ref1, s, s, d_cc, n=n, want_satd=False, want_pred=True, outs=a_both)

        def leg_b_pred():
            ctx.prep_8tap_batch(ref0, s, s, mcs[0], n=n, out=tmp[0])
            ctx.prep_8tap_batch(ref1, s, s, mcs[1], n=n, out=tmp[1])
            ctx.mc_avg_batch(tmp[0], tmp[1], s, s, bd, out=b_pred)

        def leg_b():
            leg_b_pred()
            ctx.rdo_pixel_cand_batch(org, None, s, s, d_rc, args.qindex, 0, n=n, want_sad=False, want_satd=True,
                                     outs=b_out, pred=b_pred)

        # the two legs compute the same thing
        leg_a_satd()
        leg_a_both()
        leg_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(a_both["pred"], b_pred) and torch.equal(a_both["satd"], b_out["satd"]) and
                    torch.equal(a_satd["satd"], b_out["satd"]))
        if not same:
            print(json.dumps({"size": s, "bd": bd, "n": n, "identical": False}), flush=True)
            raise SystemExit("the compound launch and the three-launch route disagree at %dx%d" % (s, s))
        runs = {"compound_satd": [], "compound_satd_pred": [], "compound_pred": [], "three_launch_pred": [],
                "three_launch_pred_satd": []}
        for _ in range(2):      # alternate: both sides see the same clocks and neighbours
            runs["compound_satd"].append(timed(leg_a_satd))
            runs["three_launch_pred_satd"].append(timed(leg_b))
            runs["compound_satd_pred"].append(timed(leg_a_both))
            runs["three_launch_pred"].append(timed(leg_b_pred))
            runs["compound_pred"].append(timed(leg_a_pred))
        ms = {k: min(v) for k, v in runs.items()}
        print(json.dumps({
            "size": s, "bd": bd, "n": n, "k": args.k, "identical": same,
            "satd_route_three_launch": "r1_rdo_pred_cand_batch dist_kind 0, SAD off",
            "ms": {k: round(v, 4) for k, v in ms.items()},
            "ms_runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
            "bytes": leg_bytes(s, bpp, n),
            "ratio_satd_vs_three_launch": round(ms["compound_satd"] / ms["three_launch_pred_satd"], 4),
            "ratio_satd_pred_vs_three_launch": round(ms["compound_satd_pred"] / ms["three_launch_pred_satd"], 4),
            "ratio_pred_vs_three_launch_pred": round(ms["compound_pred"] / ms["three_launch_pred"], 4),
            "cands_per_s_satd": round(n / (ms["compound_satd"] * 1e-3))}), flush=True)
        del a_satd, a_both, tmp, b_pred, b_out
    ctx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The intra candidate in one launch against the route it replaces, same process, same inputs:

    python tools/bench_intra_cand.py [--bit-depths 8,10] [--sizes 8,16,32] [--kinds 3,0] [--k 4] [--reps 20] [--out F]

For every (size, bit depth, dist_kind): every s x s block of a 3840x2160 luma plane (padding 88) x K = 4 intra modes
-- what survives the SATD pre-screen (num_modes_rdo, src/rdo.rs:1507-1600) -- with the block's intra transform-type
set (r1_tx_type_mask(tx_size, 0, 0, 1)).  The edge sets are built once, outside the timed region, for both sides.
  (a) fused       ONE r1_rdo_intra_cand_batch launch (two at 32x32 would be one per type; its intra set is DCT_DCT
                  alone): the prediction is made on the CU.  Timed with edge_group = K (the K modes of a block share
                  the pre-screen's edge set) and with edge_group = 1 (one set per candidate, the reference's shape).
                  "fused" is whatever the entry point runs: at the (size, bit depth, kind) points where the one
                  launch lost (r1_intra_two_launch, csrc/rdo_cand_plan.hpp) it runs two launches itself.
  (b) two-launch  r1_predict_intra_batch (n dense s x s blocks to HBM) -> r1_rdo_txsearch_batch(pred = ...) reading
                  them back: the parent's code, untouched by the fused route.
Both sides are checked for identical eob / dist / sad / satd (and predictions) first, then timed alternately (a, b,
a, b; HIP events on the launch stream, warm-up and a sustain window before every timed series, median of --reps,
best of the two rounds).  One JSON line per point: both times, their ratio, the HBM traffic the fused launch removes
(2 n s s bpp: the prediction written and read back)."""
import argparse
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
    ap.add_argument("--sizes", default="8,16,32")
    ap.add_argument("--kinds", default="3,0")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import time
    import torch
    from rav1e_amd import workload as W
    from rav1e_amd.api import INTRA_CAND, INTRA_EDGE_CAND, RDO_CAND, Context, Plane, _pix_dtype
    from rav1e_amd.types import TxSize
    assert torch.cuda.is_available(), "bench_intra_cand.py measures on a GPU; there is nothing to report without one"
    ctx = Context(0)
    fw, fh, K = args.width, args.height, args.k

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

    for bd in (int(b) for b in args.bit_depths.split(",")):
        bpp = 1 if bd == 8 else 2
        rec = Plane.from_numpy(W.random_plane_array(fw, fh, bd, 1), fw, fh, bd, 88, 88)
        org = Plane.from_numpy(W.random_plane_array(fw, fh, bd, 2), fw, fh, bd, 88, 88)
        scales = torch.from_numpy(np.random.default_rng(5).integers(1 << 12, 1 << 16, ((fh + 7) // 8, (fw + 7) // 8))
                                  .astype(np.int32)).cuda()
        for s in (int(v) for v in args.sizes.split(",")):
            ts = int(TxSize.by_dims(s, s))
            rng = np.random.default_rng(100 + s)
            bx, by = np.meshgrid(np.arange(0, fw - s + 1, s), np.arange(0, fh - s + 1, s))
            bx, by = bx.ravel(), by.ravel()
            nb = len(bx)
            n = nb * K
            # one edge set per block, no mode (what the pre-screen shares), intra edge filter on
            ec = np.zeros(nb, INTRA_EDGE_CAND)
            ec["x"], ec["y"], ec["mode"], ec["flags"] = bx, by, -1, 1 | 2 * rng.integers(0, 2, nb) | 4 * rng.integers(0, 2, nb)
            edges, lens = ctx.intra_edges_batch(rec, (0, 0, fw, fh), ts, ec)
            # K distinct luma modes per block, after predict_intra's PAETH remap
            mode = np.argsort(rng.random((nb, 13)), axis=1)[:, :K].ravel()
            x, y = np.repeat(bx, K), np.repeat(by, K)
            var = np.where((x == 0) & (y == 0), 0, np.where(y == 0, 1, np.where(x == 0, 2, 3)))
            pa = mode == 12
            mode = np.where(pa & (var == 0), 0, np.where(pa & (var == 2), 1, np.where(pa & (var == 1), 2, mode)))
            delta = np.where((mode >= 1) & (mode <= 8), rng.integers(-3, 4, n), 0)
            ic = np.zeros(n, INTRA_CAND)
            ic["mode"], ic["variant"] = mode, var
            ic["angle"] = np.array([0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0])[mode] + 3 * delta
            ic["ief"] = rng.integers(1, 3, n)
            ic["avail_w"], ic["avail_h"] = s, s
            rc = np.zeros(n, RDO_CAND)
            rc["ox"], rc["oy"] = x, y
            d_ic, d_rc = dev(ic), dev(rc)
            pos = torch.from_numpy(np.stack([bx, by], 1).astype(np.int16)).cuda()
            # the two-launch route and edge_group = 1 take one set per candidate
            edges1, lens1 = edges.repeat_interleave(K, 0), lens.repeat_interleave(K, 0)
            pos1 = pos.repeat_interleave(K, 0)
            mask = ctx.tx_type_mask(ts, False)
            nt = bin(mask).count("1")
            for kind in (int(v) for v in args.kinds.split(",")):
                sc = scales if kind else None

                def outs():
                    return {"eob": torch.empty((n, nt), dtype=torch.int16, device="cuda"),
                            "dist": torch.empty((n, nt), dtype=torch.int64, device="cuda")}
                o_a, o_a1, o_b = outs(), outs(), outs()
                b_pred = torch.empty((n, s, s), dtype=_pix_dtype(bpp), device="cuda")

                def leg_a(o=o_a, **kw):
                    ctx.rdo_intra_cand_batch(org, s, s, d_ic, pos, edges, lens, mask, args.qindex, kind, edge_group=K,
                                             scales=sc, n=n, outs=o, **kw)

                def leg_a1():
                    ctx.rdo_intra_cand_batch(org, s, s, d_ic, pos1, edges1, lens1, mask, args.qindex, kind,
                                             edge_group=1, scales=sc, n=n, outs=o_a1)

                def leg_b(o=o_b, **kw):
                    ctx.predict_intra_batch(ts, d_ic, edges1, lens1, bd, n=n, out=b_pred)
                    ctx.rdo_txsearch_batch(org, None, s, s, d_rc, mask, args.qindex, kind, scales=sc, is_intra=1, n=n,
                                           outs=o, pred=b_pred, **kw)

                # parity of what both sides leave in HBM, with every scalar and the prediction
                fa, fb = outs(), outs()
                leg_a(fa, want_sad=True, want_satd=True, want_pred=True)
                leg_b(fb, want_sad=True, want_satd=True)
                leg_a()
                leg_a1()
                leg_b()
                torch.cuda.synchronize()
                same = bool(all(torch.equal(fa[k], fb[k]) for k in ("eob", "dist", "sad", "satd")) and
                            torch.equal(fa["pred"], b_pred) and
                            all(torch.equal(o_a[k], o_b[k]) and torch.equal(o_a1[k], o_b[k]) for k in ("eob", "dist")))
                del fa, fb
                if not same:
                    emit({"size": s, "bd": bd, "dist_kind": kind, "n": n, "identical": False})
                    raise SystemExit("the fused launch and the two-launch route disagree at %dx%d" % (s, s))
                runs = {"fused": [], "fused_group1": [], "two_launch": []}
                for _ in range(2):      # alternate: both sides see the same clocks and neighbours
                    runs["fused"].append(timed(leg_a))
                    runs["two_launch"].append(timed(leg_b))
                    runs["fused_group1"].append(timed(leg_a1))
                ms = {k: min(v) for k, v in runs.items()}
                emit({"size": s, "bd": bd, "dist_kind": kind, "n": n, "k": K, "tx_type_mask": hex(mask),
                      "identical": same, "ms": {k: round(v, 4) for k, v in ms.items()},
                      "ms_runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                      "ratio_fused_vs_two_launch": round(ms["fused"] / ms["two_launch"], 4),
                      "ratio_fused_group1_vs_two_launch": round(ms["fused_group1"] / ms["two_launch"], 4),
                      "hbm_bytes_removed": 2 * n * s * s * bpp,
                      "cands_per_s_fused": round(n / (ms["fused"] * 1e-3))})
                del o_a, o_a1, o_b, b_pred
    ctx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The frame's scale maps and segmentation inputs made on the device against the only route there was before:

    python tools/bench_scales.py [--reps 30] [--out profiles/scales_bench.jsonl]

For 4K (480 x 270 importance blocks) and 1080p (240 x 135), tune Psychovisual (activity scales) and Psnr (none);
the lookahead's maps (intra costs, block importances) and the activity scales are in HBM, as the stages before
leave them.
  (a) device  r1_frame_scales -> r1_scale_kmeans -> the 96-byte download of the centroids (the one
              synchronisation) -> r1_segmentation_from_centroids on the host -> r1_spatiotemporal_scale_batch over
              every 16x16 block of the frame
  (b) host    download the maps, run tests/scales_model.py's vectorised NumPy (a MODEL of the reference's
              arithmetic, not rav1e's Rust: a compiled host loop would be faster than it), upload the grid (and the
              scores' scales per 16x16 block)
Both legs end with the results where the RDO launches read them and are checked for identical results first.  They
are timed alternately on the wall clock from first call to the final synchronisation (both legs contain host work
and a synchronisation, so device events would miss what is being compared), after a warm-up and a sustain window,
median of --reps.  The device leg's launches alone (events, no download) are reported next to it.  No threshold:
these are launch-bound stages; what the device route removes is the round trip of the maps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_block_scales(M, dist, act, w, h):
    """spatiotemporal_scale of every 16x16 block (2 x 2 importance blocks, clipped), vectorised"""
    prod = dist.astype(np.uint64).reshape(h, w) * (act.astype(np.uint64).reshape(h, w) if act is not None else
                                                  np.uint64(M.ONE))
    s = np.add.reduceat(np.add.reduceat(prod, np.arange(0, h, 2), axis=0), np.arange(0, w, 2), axis=1)
    cnt = np.add.reduceat(np.add.reduceat(np.ones((h, w), np.uint64), np.arange(0, h, 2), axis=0),
                          np.arange(0, w, 2), axis=1)
    den = cnt << np.uint64(M.SHIFT)
    return ((s + (den >> np.uint64(1))) // den).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import scales_model as M
    from rav1e_amd.api import SCALE_BLOCK, Context
    assert torch.cuda.is_available(), "bench_scales.py measures on a GPU; there is nothing to report without one"
    ctx = Context(0)
    ac_q = None
    lines = []

    def wall(f):
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.sustain_ms:
            f()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    def events(f):
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

    for (label, w, h) in (("4k", 480, 270), ("1080p", 240, 135)):
        for tune in (True, False):
            rng = np.random.default_rng(w + int(tune))
            n = w * h
            intra = rng.integers(200, 60000, n).astype(np.uint32)
            imp = (intra * rng.random(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
            imp[~M.pow_guard(imp, intra)] = 0
            act = (16384 * 2.0 ** rng.uniform(-2, 2, n)).astype(np.uint32) if tune else None
            d_intra = torch.from_numpy(intra.view(np.int32)).cuda().reshape(h, w)
            d_imp = torch.from_numpy(imp).cuda().reshape(h, w)
            d_act = torch.from_numpy(act.view(np.int32)).cuda().reshape(h, w) if tune else None
            xs, ys = np.meshgrid(np.arange(0, 2 * w, 4), np.arange(0, 2 * h, 4))
            blocks = np.zeros(xs.size, SCALE_BLOCK)
            blocks["bo_x"], blocks["bo_y"], blocks["bsize"] = xs.ravel(), ys.ravel(), 6      # BLOCK_16X16
            res = {}

            def device_launches():
                d, s, st = ctx.frame_scales(d_intra, d_imp, d_act)
                res["d"], res["cent"] = d, ctx.scale_kmeans(s)

            def device_leg():
                device_launches()
                seg = ctx.segmentation_from_centroids(res["cent"], 128, 8)       # downloads the 96 bytes
                res["seg"] = seg
                res["scale"], res["sidx"] = ctx.spatiotemporal_scale_batch(res["d"], d_act, blocks, seg["threshold"], 0)

            def host_leg():
                hi, hp = d_intra.cpu().numpy().view(np.uint32).ravel(), d_imp.cpu().numpy().ravel()
                ha = d_act.cpu().numpy().view(np.uint32).ravel() if tune else None
                dist, scores, _ = M.frame_scales(hi, hp, ha)
                cent = M.scale_kmeans(scores)
                seg = M.segmentation_from_centroids(res["ac_q"], cent, 128, 8)
                bs = host_block_scales(M, dist, ha, w, h)
                thr = np.array(seg["threshold"], np.uint32)
                sidx = np.minimum((bs[..., None] < thr).cumprod(axis=-1).sum(axis=-1), 7).astype(np.uint8)
                res["h_d"] = torch.from_numpy(dist.view(np.int32)).cuda()
                res["h_scale"] = torch.from_numpy(bs.view(np.int32)).cuda()
                res["h_sidx"] = torch.from_numpy(sidx).cuda()
                res["h_seg"] = seg

            if ac_q is None:
                ac_q = np.load(os.path.join(ROOT, "tests", "golden", "scales_ref.npz"))["ac_q"]
            res["ac_q"] = ac_q
            device_leg()
            host_leg()
            torch.cuda.synchronize()
            same = bool(torch.equal(res["d"].ravel(), res["h_d"]) and
                        torch.equal(res["scale"], res["h_scale"].ravel()) and
                        torch.equal(res["sidx"], res["h_sidx"].ravel()) and
                        res["seg"]["seg_delta"].tolist() == res["h_seg"]["data"])
            if not same:
                raise SystemExit("the device route and the host model disagree at %s tune=%s" % (label, tune))
            runs = {"device": [], "host_model": [], "device_launches_only": []}
            for _ in range(2):      # alternate: both sides see the same clocks and neighbours
                runs["device"].append(wall(device_leg))
                runs["host_model"].append(wall(host_leg))
                runs["device_launches_only"].append(events(device_launches))
            ms = {k: min(v) for k, v in runs.items()}
            line = {"frame": label, "w_in_imp_b": w, "h_in_imp_b": h, "tune_psychovisual": tune,
                    "blocks_16x16": int(len(blocks)), "identical": same,
                    "ms": {k: round(v, 4) for k, v in ms.items()},
                    "ms_runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                    "host_leg": "NumPy model of the reference's arithmetic (tests/scales_model.py), not rav1e's Rust",
                    "bytes_down_host_route": n * 4 * (3 if tune else 2), "bytes_up_host_route": n * 4 + len(blocks) * 5,
                    "bytes_down_device_route": 96, "bytes_up_device_route": int(blocks.nbytes)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

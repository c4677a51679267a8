#!/usr/bin/env python3
"""The winner's replay on a device-resident CDF context beside the rate launch over the same trials, and the host
route it removes, same process, same inputs:

    python tools/bench_coeff_cdf.py [--bit-depths 8,10] [--points 16:8,32:8] [--reps 15] [--out FILE]

The 4K workloads of tools/bench_coeff_rate_block.py, 4:2:0: every s x s block of a 3840x2160 luma noise plane through
r1_rdo_intra_split_batch (DCT_DCT, qcoeffs_out), the same over two 1920x1080 chroma noise planes with transforms of
s / 2.  ONE winner per block (the block's first mode) and one R1CoeffCdfContext per block.  Per point, alternating in
one process after the same pre-warm:
  adapt_ms        one r1_coeff_cdf_adapt_batch launch over the winners: the slices gathered from the contexts, the
                  block walked, the adapted rows scattered back (at most 2 x 1088 bytes each way per trial), every output
  rate_ms         one r1_coeff_rate_block_batch launch over the same trials on slices r1_coeff_cdf_slice_batch cut
                  (the call takes at most 256 snapshots: the slices of the first 128 contexts, luma and chroma, in turn)
  slice_ms        the two r1_coeff_cdf_slice_batch launches (luma and chroma) over every context
  d2h_ms, h2d_ms  COPIES ONLY of the route this removes: the winners' qcoeffs + eob to pinned host memory, and fresh
                  luma + chroma slices for every block back (the host's entropy coder between them is NOT timed)
One JSON line per point: HIP-event medians after a sustained warm-up, best of two alternating rounds.  The first
contexts are checked against the model of tests/coeff_cdf_model.py behind the first adapt launch, before anything is
timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def random_context(rng):
    """one valid context: every CDF strictly descending inside (64, 32704), counters 0..32"""
    from rav1e_amd.types import COEFF_CDF_CONTEXT
    rec = np.zeros(1, COEFF_CDF_CONTEXT)[0]
    for name in COEFF_CDF_CONTEXT.names:
        if name == "pad":
            continue
        a = rec[name]
        n = a.shape[-1]
        rows = a.reshape(-1, n)
        for r in rows:
            r[:n - 1] = np.sort(rng.choice(np.arange(64, 32704), n - 1, replace=False))[::-1]
            r[n - 1] = rng.integers(0, 33)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bit-depths", default="8,10")
    ap.add_argument("--points", default="16:8,32:8", help="block:transform, comma separated")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    import coeff_cdf_model as DM
    from rav1e_amd import rdo_glue as RG
    from rav1e_amd import workload as W
    from rav1e_amd.api import INTRA_SPLIT_CAND, Context, Plane
    from rav1e_amd.types import BLOCK_CHAIN_CTX, BLOCK_RATE_TRIAL, COEFF_CDF_CONTEXT, TxSize
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

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    def split_launch(org, rec, w, h, s, ts, rng, bd):
        """every s x s block of the plane, one mode, through r1_rdo_intra_split_batch -> (outs, n, x, y, mode)"""
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
            s, t = (int(v) for v in point.split(":"))
            ts = int(TxSize.by_dims(t, t))
            uv_ts, bw_uv, bh_uv = (int(v) for v in RG.chroma_tx_grid(RG.block_size(s, s), 1, 1))
            assert (bw_uv, bh_uv) == (1, 1) and TxSize(uv_ts).dims == (s // 2, s // 2)
            rng = np.random.default_rng(500 + s + t + bd)
            so, n, x, y, mode = split_launch(planes[0][0], planes[0][1], fw, fh, s, ts, rng, bd)
            ntx, area, uv_area = (s // t) ** 2, t * t, (s // 2) ** 2
            # chroma: blocks of s with transforms of s / 2 give four chroma transform blocks per launch block; the first n
            # of each plane are the winners' (1080 rows hold no whole number of blocks: a second launch fills the rest)
            uvo = []
            for p in (1, 2):
                a = split_launch(planes[p][0], planes[p][1], fw // 2, fh // 2, s, uv_ts, rng, bd)[0]
                b = split_launch(planes[p][1], planes[p][0], fw // 2, fh // 2, s, uv_ts, rng, bd)[0]
                uvo.append((torch.cat([a["qcoeffs"].view(-1, uv_area), b["qcoeffs"].view(-1, uv_area)])[:n].contiguous(),
                            torch.cat([a["eob"].view(-1), b["eob"].view(-1)])[:n].contiguous()))
            torch.cuda.synchronize()
            assert uvo[0][1].numel() == n, (uvo[0][1].numel(), n)
            blocks = np.zeros(n, BLOCK_CHAIN_CTX)
            blocks["ctx"] = rng.integers(0, 24, (n, 3, 2, 16)) | (rng.integers(0, 3, (n, 3, 2, 16)) << 6)
            blocks["mi_w"] = blocks["clip_w4"] = np.minimum(255, (fw - x) >> 2)
            blocks["mi_h"] = blocks["clip_h4"] = np.minimum(255, (fh - y) >> 2)
            blocks["clip_uv_w4"] = np.minimum(255, (fw - x) >> 3)
            blocks["clip_uv_h4"] = np.minimum(255, (fh - y) >> 3)
            blocks["y_mode"], blocks["cdf_sel"], blocks["cdf_sel_uv"] = mode, np.arange(n) % 128, 128 + np.arange(n) % 128
            trials = np.zeros(n, BLOCK_RATE_TRIAL)
            trials["first_y"], trials["first_u"], trials["first_v"] = np.arange(n) * ntx, np.arange(n), np.arange(n)
            trials["block"], trials["rng"] = np.arange(n), rng.integers(0x8000, 0x10000, n)
            trials["uv_tx_type"] = [RG.uv_tx_type_intra(int(m), uv_ts) for m in rng.integers(0, 14, n)]
            trials["do_chroma"] = 1
            base = np.array([random_context(rng) for _ in range(4)], COEFF_CDF_CONTEXT)
            host_ctx = base[np.arange(n) % 4]
            dctx = dev(host_ctx).view(n, COEFF_CDF_CONTEXT.itemsize)
            dtr, dbl = dev(trials), dev(blocks)
            qy, ey = so["qcoeffs"].view(n * ntx, area), so["eob"].view(n * ntx)
            chroma = (uvo[0][0], uvo[0][1], uvo[1][0], uvo[1][1])
            ao = {"rate": torch.empty((n,), dtype=torch.int32, device="cuda"), "rng": torch.empty((n,), dtype=torch.int16, device="cuda"),
                  "ctx": torch.empty((n, 3, 2, 16), dtype=torch.uint8, device="cuda")}
            bo = {"rate": torch.empty((n,), dtype=torch.int32, device="cuda"), "plane_rate": torch.empty((n, 3), dtype=torch.int32, device="cuda"),
                  "rng": torch.empty((n,), dtype=torch.int16, device="cuda"), "cul_level": torch.empty((n, 3, 16), dtype=torch.uint8, device="cuda"),
                  "ctx": torch.empty((n, 3, 2, 16), dtype=torch.uint8, device="cuda")}
            sl = [torch.empty((n, 1088), dtype=torch.uint8, device="cuda") for _ in range(2)]

            def slices():
                ctx.coeff_cdf_slice_batch(dctx, ts, 0, False, out=sl[0])
                ctx.coeff_cdf_slice_batch(dctx, uv_ts, 1, False, out=sl[1])
            slices()
            cdfs = torch.cat([sl[0][:128], sl[1][:128]]).contiguous()
            adapt = lambda: ctx.coeff_cdf_adapt_batch(qy, ey, 1, chroma, 1, dtr, s, s, ts, 1, 1, False, dbl, dctx, outs=ao)
            rate = lambda: ctx.coeff_rate_block_batch(qy, ey, 1, chroma, 1, dtr, s, s, ts, 1, 1, False, dbl, cdfs, outs=bo)
            win = (qy, ey) + chroma
            host_w = [torch.empty(tuple(t_.shape), dtype=t_.dtype).pin_memory() for t_ in win]
            host_s = [torch.empty((n, 1088), dtype=torch.uint8).pin_memory() for _ in range(2)]
            up = [torch.empty((n, 1088), dtype=torch.uint8, device="cuda") for _ in range(2)]

            def d2h():
                for h_, t_ in zip(host_w, win):
                    h_.copy_(t_, non_blocking=True)

            def h2d():
                for h_, t_ in zip(host_s, up):
                    t_.copy_(h_, non_blocking=True)
            print("# %dx%d / %dx%d + 2 x %dx%d, %d-bit: %d winners x (%d + 2) transform blocks, %d contexts" %
                  (s, s, t, t, s // 2, s // 2, bd, n, ntx, n), file=sys.stderr, flush=True)
            # exactness before speed: the first contexts behind ONE adapt launch against the model
            adapt()
            torch.cuda.synchronize()
            k = 16
            got = dctx[:k].cpu().numpy().reshape(-1).view(COEFF_CDF_CONTEXT)
            hq = [a.cpu().numpy() for a in (qy, chroma[0], chroma[2])]
            he = [a.cpu().numpy().view(np.uint16) for a in (ey, chroma[1], chroma[3])]
            exact = True
            for i in range(k):
                want = host_ctx[i:i + 1].copy()
                r = DM.adapt(want[0], [hq[0][i * ntx:(i + 1) * ntx], hq[1][i:i + 1], hq[2][i:i + 1]],
                             [he[0][i * ntx:(i + 1) * ntx], he[1][i:i + 1], he[2][i:i + 1]], s, s, ts, 1, 1, 0, 0, trials[i], blocks[i])
                exact = exact and want.tobytes() == got[i:i + 1].tobytes() and int(ao["rate"][i].item()) & 0xFFFFFFFF == r["rate"]
            runs = {"adapt": [], "rate": [], "slice": [], "d2h": [], "h2d": []}
            for _ in range(2):
                runs["adapt"].append(timed(adapt))
                runs["rate"].append(timed(rate))
                runs["slice"].append(timed(slices))
                runs["d2h"].append(timed(d2h, 5))
                runs["h2d"].append(timed(h2d, 5))
            ms = {k_: min(v) for k_, v in runs.items()}
            eobs = ey.cpu().numpy().view(np.uint16)
            row = {"block": s, "tx": t, "uv_tx": s // 2, "ntx": ntx, "bd": bd, "n_winners": n, "n_contexts": n,
                   "mean_eob_y": round(float(eobs.mean()), 2), "adapt_ms": round(ms["adapt"], 4), "rate_ms": round(ms["rate"], 4),
                   "slice_ms": round(ms["slice"], 4), "d2h_winners_ms": round(ms["d2h"], 4), "h2d_slices_ms": round(ms["h2d"], 4),
                   "d2h_bytes": int(sum(h_.numel() * h_.element_size() for h_ in host_w)), "h2d_bytes": 2 * n * 1088,
                   "ms_runs": {k_: [round(v_, 4) for v_ in v] for k_, v in runs.items()},
                   "adapt_over_rate": round(ms["adapt"] / ms["rate"], 4),
                   "adapt_plus_slice_over_copies": round((ms["adapt"] + ms["slice"]) / (ms["d2h"] + ms["h2d"]), 4),
                   "winners_per_s": round(n / (ms["adapt"] * 1e-3)), "first_contexts_equal_model": bool(exact),
                   "copies_only": True, "host_entropy_coder_timed": False}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            assert exact, "the adapt launch disagrees with the model"
            del so, uvo, ao, bo, sl, host_w, host_s, up, dctx
    ctx.close()


if __name__ == "__main__":
    main()

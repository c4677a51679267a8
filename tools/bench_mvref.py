#!/usr/bin/env python3
"""The MV reference stack on the device beside the host route it removes, same process, same inputs:

    python tools/bench_mvref.py [--reps 15] [--out FILE]

A 3840x2160 frame as 8 tiles (4 x 2) of 240 x 270 4x4 units, every 16x16 block coded with a seeded winner (two thirds
inter over three references and one compound pair, vectors from a small pool so that neighbours match), each tile's
blocks array on the device.  Two points, one JSON line each: HIP-event medians after a sustained warm-up.
  chain_step   what one step of the block chain enqueues for an inter frame: the next block of each of the 8 tiles
               (one in the middle of its tile) x 4 queries (three single references, one compound pair):
                 stack_ms  one r1_mvref_stack_batch launch (8 blocks, 32 queries)
                 pmv_ms    one r1_mvref_pmv_batch launch over the 32 stacks
                 store_ms  one r1_tile_blocks_store_batch launch (8 winners, gated by an R1RdPick array)
               and the route this replaces on the same box -- download the winners, run the host statement, upload:
                 d2h_ms, h2d_ms   COPIES ONLY: 8 x 24 B of winner states down to pinned host memory, 32 x 112 B of stacks
                                  back up; route_wall_ms is the wall clock of both with the synchronisation behind each
                 host_python_ms   rdo_glue.tile_blocks_store + find_mvrefs for the same 8 blocks x 4 queries: a Python
                                  statement timed on the host, NOT rav1e's code -- reported apart and in no ratio
  whole_frame  every 16x16 block of the frame x 4 queries in ONE launch (32 400 blocks, 129 600 queries): the batch form,
               and what the staging costs per block when the device is full.
The first blocks' stacks are checked against rdo_glue.find_mvrefs before anything is timed."""
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sustain-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    from rav1e_amd import rdo_glue as G
    from rav1e_amd.api import Context
    from rav1e_amd.types import MV_BLOCK, MV_QUERY, MV_STACK, MV_TRIAL, RD_PICK, TILE_BLOCK
    assert torch.cuda.is_available(), "this measures GPU time: no GPU, no number"
    ctx = Context(0)
    FC, FR, TC, TR = 960, 540, 240, 270
    QUERIES = ((1, 8, 0), (4, 8, 0), (7, 8, 0), (1, 7, 1))
    SIGN_BIAS = (0, 0, 0, 0, 1, 1, 1, 0)
    rng = np.random.default_rng(23)
    pool = np.array([(8, -16), (-40, 24), (0, 0), (12, 12), (-3, 5), (64, -64), (9, -16), (100, 3)], np.int16)

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

    def wall(f, reps=9):
        f()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    def coded_tile():
        """every 16x16 block of a tile coded: cells as tile_blocks_store leaves them (whole blocks: nothing to clip but
        the last row of blocks, which for_each cuts at the tile)"""
        bw, bh = (TC + 3) // 4, (TR + 3) // 4
        kind = rng.integers(0, 3, (bh, bw))                               # 0 intra, 1 single, 2 compound
        per = np.zeros((bh, bw), TILE_BLOCK)
        per["n4_w"], per["n4_h"], per["bsize"] = 4, 4, 6
        per["mode"] = np.where(kind == 0, rng.integers(0, 13, (bh, bw)), np.where(kind == 1, rng.choice([14, 15, 19], (bh, bw)),
                                                                                  rng.choice([20, 24, 33], (bh, bw))))
        per["ref_frames"][..., 0] = np.where(kind == 0, 0, np.where(kind == 1, rng.choice([1, 4, 7], (bh, bw)), 1))
        per["ref_frames"][..., 1] = np.where(kind == 2, 7, 8)
        mv = pool[rng.integers(0, len(pool), (bh, bw, 2))]
        mv[kind == 0] = 0
        mv[kind == 1, 1] = 0
        per["mv"] = mv
        return np.ascontiguousarray(np.repeat(np.repeat(per, 4, axis=0), 4, axis=1)[:TR, :TC])

    host, tiles = [], []
    for ty in range(2):
        for tx in range(4):
            cells = coded_tile()
            host.append({"cells": cells, "tile_x": tx * TC, "tile_y": ty * TR, "frame_cols": FC, "frame_rows": FR})
            dev = torch.from_numpy(cells.view(np.uint8).reshape(-1)).cuda()
            tiles.append(ctx.tile_blocks(TC, TR, tx * TC, ty * TR, FC, FR, cells=dev))

    def records(places):
        blocks, queries = np.zeros(len(places), MV_BLOCK), np.zeros(4 * len(places), MV_QUERY)
        for b, (t, x, y) in enumerate(places):
            blocks[b] = (t, x, y, 6, 4, 0, 4 * b)
            for q, (r0, r1, comp) in enumerate(QUERIES):
                queries[4 * b + q] = (b, (r0, r1), comp, 0)
        return blocks, queries

    def check(places, out, n):
        got = out.cpu().numpy().view(MV_STACK)
        for b, (t, x, y) in enumerate(places[:n]):
            for q, (r0, r1, comp) in enumerate(QUERIES):
                ctxv, st = G.find_mvrefs(host[t], x, y, 6, (r0, r1), comp, SIGN_BIAS)
                g = got[4 * b + q]
                assert int(g["count"]) == len(st) and int(g["mode_context"]) == ctxv, (t, x, y, q)
                for k, e in enumerate(st):
                    assert tuple(g["cand"][k]["this_mv"]) + tuple(g["cand"][k]["comp_mv"]) + (int(g["cand"][k]["weight"]),) == e

    lines = []
    # ---- (i) one chain step: the next block of each tile
    places = [(t, 120, 132) for t in range(8)]
    blocks, queries = records(places)
    db = torch.from_numpy(blocks.view(np.uint8).reshape(-1)).cuda()
    dq = torch.from_numpy(queries.view(np.uint8).reshape(-1)).cuda()
    out = torch.empty(len(queries) * MV_STACK.itemsize, dtype=torch.uint8, device="cuda")
    ctx.mvref_stack_batch(tiles, db, dq, SIGN_BIAS, out=out, max_queries=4)
    check(places, out, 8)
    trials = np.zeros(8, MV_TRIAL)
    for b in range(8):
        trials[b] = (b, 19, (1, 8), 0, ((5, -7), (0, 0)))
    dt = torch.from_numpy(trials.view(np.uint8).reshape(-1)).cuda()
    st = np.zeros(8, RD_PICK)
    st["best_rd"], st["best_row"], st["best_slot"], st["best_call"] = 1.0, 0, 0, 0
    dst = torch.from_numpy(st.view(np.uint8).reshape(-1)).cuda()
    cands = torch.zeros(len(queries) * 16, dtype=torch.uint8, device="cuda")
    stack_ms = timed(lambda: ctx.mvref_stack_batch(tiles, db, dq, SIGN_BIAS, out=out, max_queries=4))
    pmv_ms = timed(lambda: ctx.mvref_pmv_batch(out, cands, 16, offset=8))
    store_ms = timed(lambda: ctx.tile_blocks_store_batch(tiles, db, dt, state=dst))
    step_ms = timed(lambda: (ctx.mvref_stack_batch(tiles, db, dq, SIGN_BIAS, out=out, max_queries=4),
                             ctx.mvref_pmv_batch(out, cands, 16, offset=8), ctx.tile_blocks_store_batch(tiles, db, dt, state=dst)))
    pin_st = torch.empty(8 * RD_PICK.itemsize, dtype=torch.uint8).pin_memory()
    pin_out = torch.zeros(len(queries) * MV_STACK.itemsize, dtype=torch.uint8).pin_memory()
    d2h_ms = timed(lambda: pin_st.copy_(dst, non_blocking=True))
    h2d_ms = timed(lambda: out.copy_(pin_out, non_blocking=True))

    def route():
        pin_st.copy_(dst, non_blocking=True)
        torch.cuda.synchronize()
        out.copy_(pin_out, non_blocking=True)
        torch.cuda.synchronize()

    def host_step():
        for b, (t, x, y) in enumerate(places):
            G.tile_blocks_store(host[t], x, y, 6, 19, (1, 8), ((5, -7), (0, 0)), 0)
            for (r0, r1, comp) in QUERIES:
                G.find_mvrefs(host[t], x + 4, y, 6, (r0, r1), comp, SIGN_BIAS)

    def step_wall():
        ctx.mvref_stack_batch(tiles, db, dq, SIGN_BIAS, out=out, max_queries=4)
        ctx.mvref_pmv_batch(out, cands, 16, offset=8)
        ctx.tile_blocks_store_batch(tiles, db, dt, state=dst)
        torch.cuda.synchronize()
    lines.append({"point": "chain_step", "tiles": 8, "blocks": 8, "queries": len(queries), "stack_ms": round(stack_ms, 5),
                  "pmv_ms": round(pmv_ms, 5), "store_ms": round(store_ms, 5), "step_ms": round(step_ms, 5),
                  "step_wall_ms": round(wall(step_wall), 5), "d2h_ms": round(d2h_ms, 5), "h2d_ms": round(h2d_ms, 5),
                  "route_wall_ms": round(wall(route), 5), "host_python_ms": round(wall(host_step, 5), 4)})
    # ---- (ii) the whole frame in one launch
    places = [(t, x, y) for t in range(8) for y in range(0, TR, 4) for x in range(0, TC, 4)]
    blocks, queries = records(places)
    db = torch.from_numpy(blocks.view(np.uint8).reshape(-1)).cuda()
    dq = torch.from_numpy(queries.view(np.uint8).reshape(-1)).cuda()
    out = torch.empty(len(queries) * MV_STACK.itemsize, dtype=torch.uint8, device="cuda")
    ctx.mvref_stack_batch(tiles, db, dq, SIGN_BIAS, out=out, max_queries=4)
    check(places, out, 64)
    frame_ms = timed(lambda: ctx.mvref_stack_batch(tiles, db, dq, SIGN_BIAS, out=out, max_queries=4))
    lines.append({"point": "whole_frame", "tiles": 8, "blocks": len(places), "queries": len(queries), "stack_ms": round(frame_ms, 5),
                  "ns_per_block": round(frame_ms * 1e6 / len(places), 2), "out_mb": round(len(queries) * MV_STACK.itemsize / 1e6, 2)})
    for ln in lines:
        ln.update({"width": 3840, "height": 2160, "reps": args.reps})
        s = json.dumps(ln)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

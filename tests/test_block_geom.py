"""The block geometry and the transform sets the host halves share (rav1e_amd/csrc/block_geom.hpp), without a device: a
host program (tests/c/block_geom_list.cpp, the host compiler alone -- which is also the proof that the header stands
without HIP) lists what the header says at every block size, subsampling and transform size; every line is held against
the host statements the fixtures pin to the reference -- types.BlockSize, rdo_glue (largest_chroma_tx_size,
chroma_tx_grid, coeff_nbr_store, txb_ctx, uv_tx_type_inter), the tables tests/golden/coeff_rate_ref.npz stores, the
executed subsampled_size sweep of tests/golden/coeff_rate_block_ref.npz, coeff_rate_model.tx_set / txs_ctx."""
import os
import subprocess

import numpy as np
import pytest

import coeff_rate_chain_model as CM
import coeff_rate_model as M
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import BlockSize, TxSize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIDES = (2, 4, 8, 12, 16, 32, 64, 128)
FORMATS = ((0, 0), (1, 0), (1, 1))            # 4:4:4, 4:2:2, 4:2:0
GEOM = ("bw4", "bh4", "sub_w4", "sub_h4", "uv_tx_size", "uw", "uh", "bw_uv", "bh_uv", "uv_w4", "uv_h4", "adj_x", "adj_y",
        "uv_skip_off", "skip_all_planes")


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    """{"B": {(bw, bh, xdec, ydec): [ints]}, "L": {(bw, bh, tx_size): [ints]}, "T": {(tx_size, inter, reduced): [ints]}}"""
    exe = str(tmp_path_factory.mktemp("block_geom") / "block_geom_list")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rav1e_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "block_geom_list.cpp")])
    out = {"B": {}, "L": {}, "T": {}}
    nkey = {"B": 4, "L": 3, "T": 3}
    lines = subprocess.check_output([exe], text=True).splitlines()
    for line in lines:
        kind, *v = line.split()
        v = [int(e) for e in v]
        key = tuple(v[:nkey[kind]])
        assert key not in out[kind], line
        out[kind][key] = v[nkey[kind]:]
    assert len(lines) == sum(len(d) for d in out.values())
    return out


def is_block_size(bw, bh):
    return "BLOCK_%dX%d" % (bw, bh) in BlockSize.__members__ and max(bw, bh) <= 64


@pytest.fixture(scope="module")
def refused_422():
    """the (bw, bh) at which the reference's subsampled_size(1, 0) refuses, executed (all 22 sizes)"""
    G = np.load(os.path.join(GOLDEN, "coeff_rate_block_ref.npz"))
    rows = G["sweep_rows"].tolist()
    assert {r[0] for r in rows} == set(range(22))
    assert all(r[6] >= 0 for r in rows if (r[1], r[2]) != (1, 0))        # no other format refuses anything
    return {BlockSize(r[0]).dims for r in rows if (r[1], r[2]) == (1, 0) and r[6] < 0}


def test_checks_of_every_pair_and_subsampling(listed, refused_422):
    B = listed["B"]
    assert set(B) == {(bw, bh, x, y) for bw in SIDES for bh in SIDES for x in (0, 1) for y in (0, 1)}
    sizes = set()
    for (bw, bh, xdec, ydec), v in B.items():
        size_ok, sub_ok, admits = v[:3]
        assert size_ok == is_block_size(bw, bh), (bw, bh)
        assert sub_ok == ((xdec, ydec) in FORMATS), (xdec, ydec)
        if size_ok:
            sizes.add((bw, bh))
            if sub_ok:
                assert admits == ((xdec, ydec) != (1, 0) or (bw, bh) not in refused_422), (bw, bh, xdec, ydec)
        assert len(v) == (3 + len(GEOM) if size_ok and sub_ok and admits else 3), (bw, bh, xdec, ydec)
    assert len(sizes) == 19
    # 4:2:2 refuses the seven sizes that are taller than wide
    assert len({bs for bs in refused_422 if max(bs) <= 64}) == 7
    assert sum(len(v) > 3 for v in B.values()) == 19 * 3 - 7 == 50


def spans(rows, fill):
    """per row: (first changed entry, changed entries), None where nothing changed; the changed entries are one run"""
    out = []
    for r in rows:
        at = [k for k, e in enumerate(r) if e != fill]
        assert at == list(range(at[0], at[0] + len(at))) if at else True
        out.append((at[0], len(at)) if at else None)
    return out


def test_geometry_of_every_admitted_block(listed):
    n = 0
    for (bw, bh, xdec, ydec), v in listed["B"].items():
        if len(v) == 3:
            continue
        n += 1
        g = dict(zip(GEOM, v[3:]))
        key = (bw, bh, xdec, ydec)
        bsize = RG.block_size(bw, bh)
        assert (g["bw4"], g["bh4"]) == (bw // 4, bh // 4), key
        uv = RG.largest_chroma_tx_size(bsize, xdec, ydec)
        assert (g["uv_tx_size"], (g["uw"], g["uh"])) == (int(uv), TxSize(uv).dims), key
        # one grid, whichever of write_tx_blocks / write_tx_tree walks it
        for is_inter in (False, True):
            assert tuple(int(e) for e in RG.chroma_tx_grid(bsize, xdec, ydec, is_inter)) == \
                (g["uv_tx_size"], g["bw_uv"], g["bh_uv"]), (key, is_inter)
        assert (g["adj_x"], g["adj_y"]) == ((bw == 4) * xdec, (bh == 4) * ydec), key
        plane_bsize = RG.block_size(max(4, bw >> xdec), max(4, bh >> ydec))
        assert g["uv_skip_off"] == RG.txb_ctx([0], [0], 1, plane_bsize, uv)[0], key
        # the spans rdo_glue.coeff_nbr_store writes, at an offset where the chroma origin of a 4-wide / 4-high block exists
        bo_x, bo_y = 32 + (bw == 4), 16 + (bh == 4)
        fresh = lambda: ([[0xEE] * 64 for _ in range(3)], [[0xEE] * 16 for _ in range(3)])
        above, left = fresh()
        assert RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, True, True)
        assert spans(above, 0xEE) == [(bo_x, g["bw4"])] + [(bo_x >> xdec, g["sub_w4"])] * 2, key
        assert spans(left, 0xEE) == [(bo_y % 16, g["bh4"])] + [((bo_y % 16) >> ydec, g["sub_h4"])] * 2, key
        above, left = fresh()
        assert RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, False, True)
        assert [s is not None for s in spans(above, 0xEE)] == [True] + [bool(g["skip_all_planes"])] * 2, key
        above, left = fresh()
        behind = [[[7] * 16 for _ in range(2)] for _ in range(3)]
        assert RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, True, False, behind)
        ux, uy = bo_x - g["adj_x"], (bo_y - g["adj_y"]) % 16
        assert spans(above, 0xEE) == [(bo_x, g["bw4"])] + [(ux >> xdec, g["uv_w4"]) if g["uv_w4"] else None] * 2, key
        assert spans(left, 0xEE) == [(bo_y % 16, g["bh4"])] + [(uy >> ydec, g["uv_h4"]) if g["uv_h4"] else None] * 2, key
        assert (g["uv_w4"] == 0) == (g["uv_h4"] == 0) == (g["bw_uv"] * g["bh_uv"] == 0), key
    assert n == 50


def test_luma_grid_of_every_block_size_and_transform_size(listed):
    L = listed["L"]
    assert set(L) == {(bw, bh, ts) for bw in SIDES for bh in SIDES if is_block_size(bw, bh) for ts in range(19)}
    assert len(L) == 19 * 19
    for (bw, bh, ts), (ntx, gw, tw4, th4, divides) in L.items():
        tw, th = TxSize(ts).dims
        assert (tw4, th4) == (tw // 4, th // 4), ts
        assert divides == (bw % tw == 0 and bh % th == 0), (bw, bh, ts)
        if divides:
            assert (ntx, gw, tw4, th4) == CM.luma_grid(bw, bh, ts)[:4] == ((bw // tw) * (bh // th), bw // tw, tw4, th4)


def test_transform_sets_of_every_size(listed):
    G = np.load(os.path.join(GOLDEN, "coeff_rate_ref.npz"))
    used, num, ind = G["tab_av1_tx_used"], G["tab_num_tx_set"], G["tab_av1_tx_ind"]
    T = listed["T"]
    assert set(T) == {(ts, i, r) for ts in range(19) for i in (0, 1) for r in (0, 1)}
    for (ts, inter, reduced), v in T.items():
        s, mask, n, rule, txs_ctx, sqr, sqr_up = v[:7]
        key = (ts, inter, reduced)
        assert s == M.tx_set(ts, inter, reduced) == int(G["tab_tx_set"][ts, inter, reduced]), key
        assert mask == sum(int(used[s][t]) << t for t in range(16)), key
        assert n == int(num[s]) == bin(mask).count("1"), key
        assert v[7:] == [int(e) for e in ind[s]], key
        assert txs_ctx == M.txs_ctx(ts) == int(G["tab_txs_ctx"][ts]), key
        tw, th = TxSize(ts).dims
        assert (4 << sqr, 4 << sqr_up) == (min(tw, th), max(tw, th)), key
        # WinnerArgs::uv_rule as k_rd_winner_tx_type applies it, against TxType::uv_inter
        assert rule in (0, 1, 2), key
        for t in range(16):
            got = (9 if t == 9 else 0) if rule == 1 else (0 if rule == 2 and t >= 12 else t)
            assert got == RG.uv_tx_type_inter(t, ts, True), (key, t)

"""tests/golden/tile_chain_ref.npz without a GPU: the carried intra decision loop of a tile -- the oracle's pixel
composition on a plane the loop writes winners into, the coefficient models, the product's host glue
(tests/tile_chain_util.host_chain) -- reproduces every array the reference left when its own text was executed block
after block on one tile state, one BlockContext and one `fc`; and each of the three carries is visible: taken out, it moves
the blocks it should and no others.  No tolerance anywhere."""
import numpy as np
import pytest

import tile_chain_util as TC

N_CASES = 5
MUTATED = (0, 1, 3)                 # 16x16 8-bit, 8x8 10-bit, the two superblock rows


@pytest.fixture(scope="module")
def cases():
    return TC.load()


@pytest.fixture(scope="module")
def chains(cases, oracle):
    memo = {}

    def run(i):
        if i not in memo:
            memo[i] = TC.host_chain(cases[i], oracle)
        return memo[i]
    return run


def test_fixture_holds_the_conditions_it_records(cases):
    assert len(cases) == N_CASES
    geo = [(c.bd, c.w, c.h, c.bs, TC.SU.TX_SIDE[c.ts0], TC.SU.TX_SIDE[c.ts1], c.k) for c in cases]
    assert geo[:4] == [(8, 64, 32, 16, 16, 8, 4), (10, 32, 32, 8, 8, 4, 3), (8, 64, 64, 32, 32, 16, 2), (8, 64, 128, 32, 32, 16, 2)]
    assert geo[4] == geo[1]                                     # the second tile of the two-tile run
    first = cases[0]
    assert {3, 8} & set(first.modes.tolist()) and 7 in first.modes.tolist()        # top-right and bottom-left are read
    assert first.counts["distinct_modes"] >= 3 and first.counts["distinct_types"] >= 2
    assert sum(c.counts["depth0_wins"] for c in cases) >= 1 and sum(c.counts["depth1_wins"] for c in cases) >= 1
    assert sum(c.counts["runner_up_within_1pct"] for c in cases) >= 1
    for c in cases:
        # the counts are the arrays' own
        assert c.counts["depth0_wins"] == int((c.win[:, 1] == 0).sum()) and c.counts["depth1_wins"] == int((c.win[:, 1] == 1).sum())
        assert c.counts["distinct_modes"] == len(set(c.win[:, 0].tolist())) and c.counts["carry_visible"] == int(c.carry.sum())
        changed = sum(bool(c.ctx_in[k].any()) and not np.array_equal(c.ctx_in[k], c.ctx_in[k - 1]) for k in range(1, c.nblocks))
        assert c.counts["ctx_nonzero_and_changed"] == changed >= 1 and c.counts["carry_visible"] >= 1
        assert c.nblocks == (c.w // c.bs) * (c.h // c.bs) == len(c.blocks)
        assert not set(c.modes.tolist()) & {9, 10, 11}          # no SMOOTH mode: the edge filter's smooth flag is constant
        assert c.blocks[0].tolist() == [0, 0, 1] and not c.ctx_in[0].any()
        # every block lies whole inside the tile, each once; a left reset stands in front of every superblock row
        assert sorted((x, y) for x, y, _ in c.blocks.tolist()) == sorted((x, y) for y in range(0, c.h, c.bs) for x in range(0, c.w, c.bs))
        assert [i for i, b in enumerate(c.blocks.tolist()) if b[2]] == [i for i, b in enumerate(c.blocks.tolist()) if b[0] == 0 and b[1] % 64 == 0]
        # the final plane is the blocks' reconstructions
        for (x, y, _), r in zip(c.blocks.tolist(), c.rec):
            assert np.array_equal(c.final[y:y + c.bs, x:x + c.bs], r)
    # exact ties between two modes at the minimum (the rate_add the generator set): `<` kept the earlier mode
    ties = 0
    for c in cases:
        tied = [b for b in range(c.nblocks) if int((c.mode_rd[b] == c.mode_rd[b].min()).sum()) == 2]
        assert len(tied) == c.counts["mode_ties"] and all(int(c.win[b, 0]) == int(np.argmin(c.mode_rd[b])) for b in tied)
        assert all(np.array(c.mode_rd[b].min(), np.float64).view(np.uint64) == c.best_rd[b] for b in range(c.nblocks))
        ties += len(tied)
    assert ties >= 2 and cases[0].counts["mode_ties"] >= 1
    rows = cases[3]
    assert sum(int(b[2]) for b in rows.blocks.tolist()) == 2 and rows.blocks[4].tolist() == [0, 64, 1]
    assert rows.left[3].any() and not rows.ctx_in[4].reshape(3, 2, 16)[:, 1].any() and rows.ctx_in[4].reshape(3, 2, 16)[0, 0].any()


def test_coding_order_is_the_quad_tree(cases):
    """the 16x16 blocks of a 64x32 tile: the z-order inside the 32x32 quadrants; the availability answers in that order
    (rdo_glue.intra_split_masks) let block 2 read block 1 as its top-right and block 4, the first of the right quadrant, read
    block 3 below-left of it; the first 8x8 transform block of block 1 has block 0's lower half below-left of it"""
    c = cases[0]
    assert [tuple(b[:2]) for b in c.blocks.tolist()] == [(0, 0), (16, 0), (0, 16), (16, 16), (32, 0), (48, 0), (32, 16), (48, 16)]
    tr = [TC.RG.intra_split_masks(16, 16, c.ts0, x >> 2, y >> 2, x, y, c.w, c.h)[0] for x, y, _ in c.blocks.tolist()]
    bl = [TC.RG.intra_split_masks(16, 16, c.ts0, x >> 2, y >> 2, x, y, c.w, c.h)[1] for x, y, _ in c.blocks.tolist()]
    assert tr == [0, 0, 1, 0, 0, 0, 1, 0] and bl == [0, 0, 0, 0, 1, 0, 0, 0]
    assert TC.RG.intra_split_masks(16, 16, c.ts1, 4, 0, 16, 0, c.w, c.h) == (0b0100, 0b0001)


@pytest.mark.parametrize("i", range(N_CASES))
def test_host_chain_reproduces_the_fixture(cases, chains, i):
    """every recorded array of every block: the trials' eob, qcoeffs, rate, distortion and rd; the decisions; the context
    bytes, the packed CDF context, both neighbour arrays and the reconstruction behind every block; the final plane"""
    c, got = cases[i], chains(i)
    m = TC.moved(c, got)
    assert not any(m.values()), (c.name, {k: v for k, v in m.items() if v})
    assert np.array_equal(got["final"], c.final), c.name


@pytest.mark.parametrize("i", MUTATED)
def test_without_the_reconstruction_carry(cases, oracle, i):
    """the winner's pixels are not written back: block 0 keeps every trial and decision; every later block has a coded
    neighbour that each of the case's modes reads an edge from, so its distortions move; no block's plane content is the
    fixture's"""
    c = cases[i]
    m = TC.moved(c, TC.host_chain(c, oracle, write_back=False))
    later = list(range(1, c.nblocks))
    assert m["dist"] == later and m["rd"] == later and m["best_rd"] == later, (c.name, m)
    assert all(0 not in m[k] for k in TC.TRIAL_ARRAYS + TC.DECISION_ARRAYS + ("ctx_in", "ctx_out", "cdf", "above", "left")), (c.name, m)
    assert m["rec"] == list(range(c.nblocks)), (c.name, m)


@pytest.mark.parametrize("i", MUTATED)
def test_without_the_cdf_carry(cases, oracle, i):
    """the winner's adapted CDFs are dropped: the context behind every block moves; block 0 is measured against the same
    start and keeps its rates, every later block's rates move; pixels move only behind the first changed decision"""
    c = cases[i]
    m = TC.moved(c, TC.host_chain(c, oracle, cdf_carry=False))
    assert m["cdf"] == list(range(c.nblocks)) and m["rate"] == list(range(1, c.nblocks)), (c.name, m)
    assert all(0 not in m[k] for k in TC.TRIAL_ARRAYS + TC.DECISION_ARRAYS + ("ctx_in", "ctx_out", "above", "left", "rec")), (c.name, m)
    first_win = min(m["win"]) if m["win"] else c.nblocks
    assert all(b > first_win for k in ("eob", "qc", "dist") for b in m[k]) and all(b >= first_win for b in m["rec"]), (c.name, m)


@pytest.mark.parametrize("i", MUTATED)
def test_without_the_neighbour_store(cases, oracle, i):
    """the winner's context spans are dropped: the gathered bytes move exactly where the fixture's are non-zero, and so do
    the rates there; pixels move only behind the first changed decision"""
    c = cases[i]
    m = TC.moved(c, TC.host_chain(c, oracle, nbr_store=False))
    nonzero = [b for b in range(c.nblocks) if c.ctx_in[b].any()]
    assert nonzero == list(range(1, c.nblocks))
    assert m["ctx_in"] == nonzero and m["rate"] == nonzero, (c.name, m)
    assert m["above"] == list(range(c.nblocks)), (c.name, m)
    assert all(0 not in m[k] for k in TC.TRIAL_ARRAYS + TC.DECISION_ARRAYS + ("ctx_in", "ctx_out", "cdf", "rec")), (c.name, m)
    first_win = min(m["win"]) if m["win"] else c.nblocks
    assert all(b > first_win for k in ("eob", "qc", "dist") for b in m[k]) and all(b >= first_win for b in m["rec"]), (c.name, m)

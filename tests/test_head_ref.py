"""tests/golden/head_ref.npz (gen_head_ref.py: the reference's head-symbol writers executed through tools/rustlite on a
real 2-D blocks array) against the host statements of rdo_glue (head_symbols, partition_symbol, tx_size_symbol,
head_nbr_store, head_nbr_reset_left) through tests/head_model.py: every rate, every rng, every adapted CDF and every
context array of the fixture, bit for bit.  Then one sensitivity test per trap of the reference's head: the behaviour is
turned off in the model and NAMED fixture cases must move -- a trap no case notices is a hole in the fixture."""
import numpy as np
import pytest

import head_model as M
from rav1e_amd import rdo_glue as G
from rav1e_amd.types import HEAD_CDF_CONTEXT, HEAD_NBR_CONTEXT, BlockSize, TxSize

FX = M.load_fixture()
SINGLES = M.Rows(FX, "single_rows", "single_cols")
SEQS = M.Rows(FX, "seq_rows", "seq_cols")
EVS = M.Rows(FX, "ev_rows", "ev_cols")
TRIALS = M.Rows(FX, "trial_rows", "trial_cols")
PARTS = M.Rows(FX, "part_rows", "part_cols")
PCASES = M.Rows(FX, "part_case_rows", "part_case_cols")
SINGLE_NAMES = [str(n) for n in FX["single_names"]]


@pytest.fixture(autouse=True)
def _nothing_off():
    M.OFF.clear()
    yield
    M.OFF.clear()


def single_results():
    cdfs = [M.cdf_record(r) for r in FX["single_cdf"]]
    nbrs = [M.nbr_arrays(M.nbr_record(r)) for r in FX["single_nbr"]]
    out = []
    for k in range(len(SINGLES)):
        r = SINGLES(k)
        syms = M.symbols(nbrs[r["ctx"]], M.blk_of(r), M.trial_of(r))
        out.append(M.head_rate(cdfs[r["ctx"]], syms))
    return out


def part_case_results():
    cdfs = [M.cdf_record(r) for r in FX["single_cdf"]]
    nbrs = [M.nbr_arrays(M.nbr_record(r)) for r in FX["single_nbr"]]
    return [M.partition_rate(cdfs[r["ctx"]], nbrs[r["ctx"]], r["bsize"], r["bo_x"], r["bo_y"], r["mi_cols"], r["mi_rows"],
                             r["ptype"], r["rng0"]) for r in (PCASES(k) for k in range(len(PCASES)))]


def run_sequence(si):
    """-> per event: ([(rate, rng) per trial], packed cdf behind, packed nbr behind), the model's"""
    seq = SEQS(si)
    cdf, rec = M.cdf_record(FX["seq_cdf0"][si]), M.nbr_record(FX["seq_nbr0"][si])
    nbr = M.nbr_arrays(rec)
    out = []
    for e in (k for k in range(len(EVS)) if EVS(k)["seq"] == si):
        ev = EVS(e)
        res = []
        if ev["kind"] == 1:
            G.head_nbr_reset_left(nbr)
        else:
            for p in range(ev["part_off"], ev["part_off"] + ev["n_parts"]):
                pr = PARTS(p)
                M.partition_event(cdf, nbr, pr["bsize"], pr["bo_x"], pr["bo_y"], seq["mi_cols"], seq["mi_rows"], pr["ptype"])
            blk = M.blk_of(ev, seq)
            trs = [M.trial_of(TRIALS(t)) for t in range(ev["trial_off"], ev["trial_off"] + ev["n_trials"])]
            res = [M.head_rate(cdf, M.symbols(nbr, blk, tr)) for tr in trs]
            win = trs[ev["winner"]]
            M.head_commit(cdf, M.symbols(nbr, blk, win, coded=True))
            node = (ev["upc_x"], ev["upc_y"], ev["upc_bsize"], ev["upc_subsize"]) if ev["upc_subsize"] >= 0 else None
            G.head_nbr_store(nbr, ev["bsize"], ev["bo_x"], ev["bo_y"], seq["mi_cols"], seq["mi_rows"], win[0], win[6],
                             seq["tx_mode_select"], node)
        out.append((e, res, cdf.copy().reshape(1).view(np.uint16).copy(), rec.copy().reshape(1).view(np.uint8).copy()))
    return out


def sequence_moves(si):
    """the names of the events of sequence si where the model leaves the fixture"""
    moved = []
    for (e, res, cdf, nbr) in run_sequence(si):
        ev = EVS(e)
        want = [(TRIALS(t)["rate"], TRIALS(t)["rng"]) for t in range(ev["trial_off"], ev["trial_off"] + ev["n_trials"])] \
            if ev["kind"] == 0 else []
        if res != want or not np.array_equal(cdf, FX["ev_cdf"][e]) or not np.array_equal(nbr, FX["ev_nbr"][e]):
            moved.append(str(FX["ev_names"][e]))
    return moved


def test_layout():
    assert FX["single_cdf"].shape[1] * 2 == HEAD_CDF_CONTEXT.itemsize and FX["single_nbr"].shape[1] == HEAD_NBR_CONTEXT.itemsize
    names = [str(f).replace("_cdfs", "").replace("_cdf", "") for f in FX["cdf_fields"]]
    assert names == [n for n in HEAD_CDF_CONTEXT.names if n != "pad"]


def test_tables():
    """what the statements restate of the reference's tables, at every block and transform size"""
    for b in range(22):
        w, h = FX["block_wh"][0][b], FX["block_wh"][1][b]
        assert BlockSize(b).dims == (w, h)
        assert list(FX["tab_partition_context"][b]) == [31 & ~((w >> 2) - 1), 31 & ~((h >> 2) - 1)]
        assert FX["tab_cfl_allowed"][b] == int(b <= 9) and FX["tab_is_sqr"][b] == int(w == h)
        if max(w, h) <= 64:
            assert TxSize(int(FX["tab_max_txsize_rect"][b])).dims == (w, h)
    assert [int(G.sub_tx_size(t)) for t in range(19)] == [int(v) for v in FX["tab_sub_tx_size"]]
    assert [int(v) for v in FX["tab_is_directional"]] == [int(1 <= m <= 8) for m in range(14)]


def test_single_trials():
    got = single_results()
    bad = [SINGLE_NAMES[k] for k in range(len(SINGLES)) if got[k] != (SINGLES(k)["rate"], SINGLES(k)["rng"])]
    assert not bad, bad[:10]


def test_partition_cases():
    got = part_case_results()
    bad = [k for k in range(len(PCASES)) if got[k] != (PCASES(k)["rate"], PCASES(k)["rng"])]
    assert not bad, [(PCASES(k), got[k]) for k in bad[:5]]


@pytest.mark.parametrize("si", range(len(SEQS)), ids=[str(n) for n in FX["seq_names"]])
def test_sequence(si):
    assert sequence_moves(si) == []


# ---- one sensitivity test per trap
def singles_moved():
    got = single_results()
    return {SINGLE_NAMES[k] for k in range(len(SINGLES)) if got[k] != (SINGLES(k)["rate"], SINGLES(k)["rng"])}


def seq_index(name):
    return [str(n) for n in FX["seq_names"]].index(name)


def test_trap_angle_deltas_share_a_row():
    M.OFF.add("angle_shared_row")
    moved = singles_moved()
    assert {"angle same row y=uv D45", "angle same row y=uv V", "rect 16x8 no partition depth 1"} <= moved
    assert "angle two rows" not in moved


def test_trap_cfl_alphas_share_a_row():
    M.OFF.add("cfl_shared_row")
    moved = singles_moved()
    assert {"cfl same row NEG NEG", "cfl same row POS POS"} <= moved
    assert not {"cfl two rows NEG POS", "cfl one alpha ZERO POS", "cfl one alpha NEG ZERO"} & moved


def test_trap_small_block_rows():
    """8x8 on partition_w8_cdf and tx_size_8x8_cdf (rectangles below 16 on tx_size_8x8_cdf too); 64x64 on tx_size_cdf[2]"""
    M.OFF.add("small_rows")
    moved = singles_moved()
    assert {"8x8 w8 rows depth 0", "8x8 w8 rows depth 1", "8x4 no angle depth 1", "cfl same row POS POS"} <= moved
    assert {"64x64 cat 3 depth 0", "64x64 cat 3 depth 2", "rect 64x16 depth 1 no cfl"} <= moved
    assert not {"rect 16x8 no partition depth 1", "tile left edge", "cfl same row NEG NEG"} & moved      # 16x16 and 16x8: cat 1
    assert sequence_moves(seq_index("mixed 420"))


def test_trap_rectangles_write_no_partition_symbol():
    M.OFF.add("rect_partition")
    moved = singles_moved()
    assert {"rect 16x8 no partition depth 1", "rect 8x32 no partition depth 2", "rect 64x16 depth 1 no cfl",
            "4x16 angle delta no partition"} <= moved
    assert not {"8x8 w8 rows depth 0", "64x64 cat 3 depth 0", "4x4 no partition no angle no tx", "4x8 no angle"} & moved
    assert sequence_moves(seq_index("rect 420")) and not sequence_moves(seq_index("sb32 420"))


def test_size_categories_and_rectangle_depths_as_symbols():
    """64x64 on tx_size_cdf[2]; a rectangle writes no partition symbol and a depth through sub_tx_size_map: the named
    cases hold those symbols, and the fixture's rates follow from them"""
    nbr = M.nbr_arrays(M.nbr_record(FX["single_nbr"][0]))
    for k, name in enumerate(SINGLE_NAMES):
        r = SINGLES(k)
        syms = M.symbols(M.nbr_arrays(M.nbr_record(FX["single_nbr"][r["ctx"]])), M.blk_of(r), M.trial_of(r))
        fields = [s[0] for s in syms]
        if name.startswith("64x64 cat 3"):
            assert syms[-1][0] == "tx_size" and syms[-1][1][0] == 2 and fields[0] == "partition"
        if name.startswith("rect "):
            assert "partition" not in fields and "partition_w8" not in fields and fields[-1] in ("tx_size", "tx_size_8x8")
        if name == "rect 8x32 no partition depth 2":
            assert syms[-1][:2] + syms[-1][3:4] == ("tx_size", (1, syms[-1][1][1]), 2)
    assert nbr is not None


def test_trap_below_8x8():
    M.OFF.add("sub8")
    moved = singles_moved()
    assert {"4x4 no partition no angle no tx", "4x4 even column", "4x8 no angle", "8x4 no angle depth 1"} <= moved
    assert not {"4x16 angle delta no partition", "16x4 angle delta"} & moved      # they write one: not below 8x8 in the enum
    M.OFF.clear()
    for k, name in enumerate(SINGLE_NAMES):
        r = SINGLES(k)
        if r["bsize"] < 3 or name.startswith("4x16"):
            syms = M.symbols(M.nbr_arrays(M.nbr_record(FX["single_nbr"][r["ctx"]])), M.blk_of(r), M.trial_of(r))
            fields = [s[0] for s in syms]
            assert not fields[0].startswith("partition")
            assert ("uv_mode" in fields or "uv_mode_cfl" in fields) == bool(r["has_chroma"])
    # both arms of has_chroma are in the fixture below 8x8
    assert {SINGLES(k)["has_chroma"] for k in range(len(SINGLES)) if SINGLES(k)["bsize"] == 0} == {0, 1}


def test_trap_tile_relative_neighbours():
    M.OFF.add("tile_relative")
    moved = singles_moved()
    assert "tile left edge" in moved
    top_row = {SINGLE_NAMES[k] for k in range(len(SINGLES)) if SINGLES(k)["bo_y"] == 0}
    assert len(moved & top_row) >= 5


def test_trap_edge_partition():
    M.OFF.add("edge_gather")
    got = part_case_results()
    edge = [k for k in range(len(PCASES)) if not (PCASES(k)["bo_x"] + (FX["block_wh"][0][PCASES(k)["bsize"]] >> 3) < PCASES(k)["mi_cols"] and
                                                  PCASES(k)["bo_y"] + (FX["block_wh"][0][PCASES(k)["bsize"]] >> 3) < PCASES(k)["mi_rows"])]
    written = [k for k in edge if PCASES(k)["rate"] != 0 or PCASES(k)["rng"] != PCASES(k)["rng0"]]
    assert len(edge) >= 20 and len(written) >= 12 and len(written) < len(edge)     # the corner arm writes nothing
    assert all(got[k] != (PCASES(k)["rate"], PCASES(k)["rng"]) for k in written)
    assert all(got[k] == (PCASES(k)["rate"], PCASES(k)["rng"]) for k in range(len(PCASES)) if k not in edge)
    assert sequence_moves(seq_index("edge 420")) and sequence_moves(seq_index("edge 444"))     # nothing adapts there


def test_refusals_of_the_statement():
    nbr = M.nbr_arrays(M.nbr_record(FX["single_nbr"][0]))
    ok = (6, 8, 0, 64, 64, 1, 1)
    assert M.symbols(nbr, ok, (3, 3, 0, 0, 0, 0, 2)) != G.HEAD_REFUSED
    for blk, tr in ((ok, (13, 0, 0, 0, 0, 0, 2)), (ok, (3, 14, 0, 0, 0, 0, 2)), (ok, (3, 13, 0, 0, 0, 0, 2)),
                    (ok, (3, 3, 4, 0, 0, 0, 2)), (ok, (3, 3, 0, -4, 0, 0, 2)), (ok, (3, 3, 0, 0, 0, 0, 3)),
                    ((9, 8, 0, 64, 64, 1, 1), (3, 3, 0, 0, 0, 0, 0)), ((18, 8, 0, 64, 64, 1, 1), (0, 13, 0, 0, 1, 1, 15)),
                    ((15, 0, 0, 64, 64, 1, 1), (0, 0, 0, 0, 0, 0, 4)), ((6, 64, 0, 64, 64, 1, 1), (0, 0, 0, 0, 0, 0, 2)),
                    ((6, 62, 0, 64, 64, 1, 1), (0, 0, 0, 0, 0, 0, 2))):
        assert M.symbols(nbr, blk, tr) == G.HEAD_REFUSED, (blk, tr)

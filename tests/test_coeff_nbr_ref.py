"""The device-resident coefficient neighbour contexts without a GPU: tests/golden/coeff_nbr_ref.npz (the reference's
write_coeffs_lv_map, reset_skip_context and reset_left_contexts executed over sequences of blocks at real tile positions
on ONE BlockContext and ONE fc, gen_coeff_nbr_ref.py) against the host statements the GPU tests hold the kernels to --
rdo_glue.block_chain_ctx chained with coeff_nbr_store / coeff_nbr_reset_left, winner_tx_type / uv_tx_type_inter -- the
struct layouts against the header compiled as C, and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coeff_cdf_model as DM
import coeff_nbr_model as NM
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import COEFF_NBR_CONTEXT, NBR_BLOCK, BlockSize, TxSize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return NM.load_fixture()


def test_fixture_holds_the_sequences_the_issue_names(fixture):
    G, seqs = fixture
    assert len(seqs) >= 24 and all(len(s.rows) <= 12 for s in seqs)
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "coeff_nbr_ref.npz")) < os.path.getsize(os.path.join(golden, "coeff_cdf_ref.npz"))
    rows = [c for s in seqs for c in s.rows]
    blocks = [c for c in rows if c.kind == 0]
    assert {c.cb for c in blocks} == {2, 4} and {c.inter for c in blocks} == {0, 1}
    assert {(c.xdec, c.ydec) for c in blocks} == {(1, 1), (1, 0), (0, 0)}
    for prefix in ("sb32", "sbrow", "mixed", "sub8", "4x16", "skip", "edge", "far", "zero"):
        assert any(s.name.startswith(prefix) for s in seqs), prefix
    assert G["case_above"].shape[1:] == (3, 1024) and G["case_left"].shape[1:] == (3, 16)
    assert any(c.kind == 1 for c in rows)
    # a skipped 4x16 in 4:2:0 at an even offset; sub-8x8 blocks that carry the chroma and that do not
    assert any(c.skip and (c.bw, c.bh, c.xdec, c.ydec) == (4, 16, 1, 1) and c.bo_x % 2 == 0 for c in blocks)
    assert {c.do_chroma for c in blocks if c.bw == 4 and c.bh == 4 and c.xdec} == {0, 1}
    # an empty chroma grid, a block the tile cuts, a window that meets entry 1023, all-zero eobs
    assert any(c.do_chroma and c.ntx[1] == 0 and not c.skip for c in blocks)
    assert any(c.bo_x + c.bw // 4 > c.mi_width for c in blocks) and any(c.bo_y + c.bh // 4 > c.mi_height for c in blocks)
    assert any(c.bo_x >= 1008 and c.bo_x + 16 > 1024 for c in blocks)
    assert any(not c.skip and not any(int(e) for p in range(3) for e in c.eobs[p]) for c in blocks)
    # `left` is consumed across a superblock boundary: a block at x >= 16 reads left entries an earlier block wrote
    assert all(int(v) == 0 for s in seqs if s.name == "sb32 420" for v in s.above0.ravel())


def test_host_statements_reproduce_every_stored_state(fixture):
    """every sequence replayed on one pair of arrays and one CDF context: block_chain_ctx on the arrays in front equals
    the stored record, the model's rate, rng and 96 bytes equal the reference's, and coeff_nbr_store / coeff_nbr_reset_left
    leave the WHOLE arrays as the reference did, behind every row"""
    _, seqs = fixture
    carried = 0
    for s in seqs:
        def check(c, above, left, blk, res, s=s):
            key = (s.name, c.step, c.name)
            if blk is not None:
                assert blk.tobytes() == c.block.tobytes(), key
                assert (res["rate"], res["rng"]) == (c.rate, c.rng_out), key
                assert res["ctx"] == c.ctx_out.tolist(), key
            assert np.array_equal(above, c.above), (key, np.argwhere(above != c.above)[:6].tolist())
            assert np.array_equal(left, c.left), (key, np.argwhere(left != c.left)[:6].tolist())
        _above, _left, cdf = NM.replay(s, check=check)
        assert np.array_equal(DM.packed_of(cdf), s.packed[1]), s.name
        carried += any(c.kind == 0 and not c.skip and c.step > 0 and c.ctx_in.any() for c in s.rows)
    assert carried >= 20


def test_wrong_stores_move_the_named_sequences(fixture):
    """two wrong scatters the fixture is there to catch: the chroma span stored at the luma offset (no >> xdec) moves
    the subsampled sequences and only them; the skip's chroma origin taken at bo_x (reset_skip_context's `>> xdec2`
    dropped) moves exactly the subsampled sequences that hold a skipped block with chroma"""
    _, seqs = fixture

    def no_shift(above, left, bo_x, bo_y, bsize, xdec, ydec, do_chroma, skip, ctx_behind=None):
        if skip or not xdec:
            return RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, do_chroma, skip, ctx_behind)
        lum = [above[0].copy(), left[0].copy()]
        RG.coeff_nbr_store(above, left, bo_x * 2, bo_y, bsize, xdec, ydec, do_chroma, skip, ctx_behind)
        above[0], left[0] = lum
        return RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, False, skip, ctx_behind)

    def skip_no_shift(above, left, bo_x, bo_y, bsize, xdec, ydec, do_chroma, skip, ctx_behind=None):
        if not skip or not xdec:
            return RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, do_chroma, skip, ctx_behind)
        lum = above[0].copy()
        RG.coeff_nbr_store(above, left, bo_x * 2, bo_y, bsize, xdec, ydec, do_chroma, skip)
        above[0] = lum
        return RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, xdec, ydec, False, skip)

    for wrong, expect in ((no_shift, lambda s: s.rows[0].xdec == 1 and "far" not in s.name),
                          (skip_no_shift, lambda s: s.rows[0].xdec == 1 and any(c.skip for c in s.rows))):
        moved = set()
        for s in seqs:
            try:
                above, left, _ = NM.replay(s, store=wrong)
            except AssertionError:          # the wrong span left the arrays
                moved.add(s.name)
                continue
            last = s.rows[-1]
            if not (np.array_equal(above, last.above) and np.array_equal(left, last.left)):
                moved.add(s.name)
        want = {s.name for s in seqs if expect(s)}
        assert want <= moved and not any(s.rows[0].xdec == 0 and s.name in moved for s in seqs), (sorted(moved ^ want))


def test_store_refuses_spans_that_leave_the_arrays():
    above, left = np.full((3, 1024), 7, np.uint8), np.full((3, 16), 7, np.uint8)
    ctx = np.full((3, 2, 16), 9, np.uint8)
    for bo_x, bo_y, bsize in ((1020, 0, BlockSize.BLOCK_32X32), (0, 12, BlockSize.BLOCK_32X32), (0, 30, BlockSize.BLOCK_16X16),
                              (0, 1, BlockSize.BLOCK_4X4)):
        for skip in (False, True):
            if skip and bsize == BlockSize.BLOCK_4X4:
                continue                    # a skipped block has no shifted chroma origin
            assert not RG.coeff_nbr_store(above, left, bo_x, bo_y, bsize, 1, 1, True, skip, ctx), (bo_x, bo_y, bsize, skip)
    assert (above == 7).all() and (left == 7).all()
    assert RG.coeff_nbr_store(above, left, 1016, 8, BlockSize.BLOCK_32X32, 1, 1, True, False, ctx)
    assert (above[0, 1016:] == 9).all() and (above[0, :1016] == 7).all() and (above[1, 508:512] == 9).all()
    assert (left[0, 8:] == 9).all() and (left[1, 4:8] == 9).all() and (left[1, :4] == 7).all() and (left[1, 8:] == 7).all()


def test_winner_tx_type_and_uv_tx_type_inter(fixture):
    """uv_tx_type_inter against the tt / uv_tt / uv_ts columns of the inter rows of both fixtures (TxType::uv_inter and
    write_tx_tree's rule executed there); winner_tx_type is the slot's type and that rule"""
    _, seqs = fixture
    _, cdf_seqs = DM.load_fixture()
    rows = [c for s in seqs for c in s.rows if c.kind == 0 and not c.skip] + [c for s in cdf_seqs for c in s.blocks]
    inter = [c for c in rows if c.inter]
    assert len(inter) >= 100
    seen = set()
    for c in inter:
        coded = [int(e) for k, e in enumerate(c.eobs[0])]
        if hasattr(c, "mi_width"):          # only transform blocks inside the tile are coded
            gw = c.bw // TxSize(c.ts).dims[0]
            tw4, th4 = TxSize(c.ts).dims[0] // 4, TxSize(c.ts).dims[1] // 4
            coded = [e for k, e in enumerate(coded) if c.bo_x + (k % gw) * tw4 < c.mi_width and c.bo_y + (k // gw) * th4 < c.mi_height]
        has = any(coded)
        assert RG.uv_tx_type_inter(c.tt, c.uv_ts, has) == c.uv_tt, c.name
        mask = 0xFFFF
        assert RG.winner_tx_type(c.tt, mask, 1, c.uv_ts, coded) == (c.tt, c.uv_tt), c.name
        seen.add((c.tt, has, max(TxSize(c.uv_ts).dims), min(TxSize(c.uv_ts).dims)))
    assert {k[1] for k in seen} == {True, False} and {k[2] for k in seen} >= {4, 8, 16, 32}
    assert RG.winner_tx_type(2, 0x0E0F, 0) == (2, None) and RG.winner_tx_type(4, 0x0E0F, 0) == (9, None)
    assert RG.winner_tx_type(7, 0x0E0F, 0) == (None, None) and RG.winner_tx_type(-1, 0x0E0F, 1, 0, [1]) == (None, None)


@pytest.mark.parametrize("name,dt,size", [("R1CoeffNbrContext", COEFF_NBR_CONTEXT, 3120), ("R1NbrBlock", NBR_BLOCK, 20)])
def test_struct_layout_equals_the_header_compiled_as_c(tmp_path, name, dt, size):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rav1e_amd.h"', 'int main(void) {',
             '  printf("%s.size %%zu 0\\n", sizeof(%s));' % (name, name)]
    for f in dt.names:
        lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    lines += ['  printf("width %d 0\\n", R1_COEFF_NBR_WIDTH);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in out if l}
    assert dt.itemsize == size and got[name + ".size"] == [size, 0] and got["width"] == [1024, 0]
    assert len(got) == len(dt.names) + 2
    for f in dt.names:
        assert got[name + "." + f] == [dt.fields[f][1], dt.fields[f][0].itemsize], (f, got[name + "." + f])


def test_library_exports_the_neighbour_context_calls():
    from rav1e_amd import _lib
    L = _lib.load()
    for sym, nargs in (("r1_coeff_nbr_gather_batch", 12), ("r1_coeff_nbr_store_batch", 14), ("r1_coeff_nbr_reset_left_batch", 7),
                       ("r1_rd_winner_tx_type_batch", 11)):
        assert hasattr(L, sym) and sym in _lib.SYMBOLS and len(getattr(L, sym).argtypes) == nargs
    assert L.r1_rd_winner_tx_type_batch.argtypes[4] is C.c_uint32
    assert L.r1_abi_version() == 7

"""The coefficient rate across a block's transform blocks without a GPU: tests/golden/coeff_rate_chain_ref.npz (the
reference's write_coeffs_lv_map executed once per coded transform block on ONE ContextWriter / BlockContext /
WriterCounter through tools/rustlite, gen_coeff_rate_chain_ref.py) against the Python model the GPU tests use
(tests/coeff_rate_chain_model.py), what each carried mechanism is worth, the host refusals of the new entry point, the
new struct layout against the header compiled as C, the host glue and the export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coeff_rate_model as M
import coeff_rate_chain_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return CM.load_fixture()


def test_model_reproduces_every_fixture_case(fixture):
    """total rate, tell_frac behind every block, cul_level per block and both context arrays at the end; the snapshot a
    case read is left as it was"""
    _, cases = fixture
    assert len(cases) >= 66
    for c in cases:
        before = c.cdfs.copy()
        r = c.model()
        key = (c.k, c.name)
        assert r["rate"] == c.rate, key
        assert r["tell"] == c.tell.tolist(), key
        assert r["cul"] == c.cul.tolist(), key
        assert r["ctx"] == c.ctx_out.tolist(), key
        assert sum(r["txb_rate"]) == c.rate, key
        assert before.tobytes() == c.cdfs.tobytes(), key


def test_fixture_covers_what_the_issue_lists(fixture):
    _, cases = fixture
    synth = [c for c in cases if "/" in c.name]
    shapes = {(c.bw, c.bh, c.ts) for c in synth}
    assert shapes == {(8, 8, 0), (16, 16, 0), (64, 64, 2), (16, 4, 0), (4, 16, 0), (32, 8, 8), (16, 64, 9), (64, 64, 3),
                      (64, 64, 4), (8, 8, 1)}
    assert any(c.eobs.max() > 256 for c in synth if (c.bw, c.ts) == (64, 3))
    assert {(c.inter, c.red) for c in synth} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c.y_mode for c in cases if not c.inter} == set(range(13))
    assert {0, 9, 10, 11} <= {c.tt for c in synth} and {c.cb for c in synth} == {2, 4}
    for v in (127, 128, 32767, (1 << 20) - 1):
        assert any((np.abs(c.qc) == v).any() for c in synth), v
    # eob == 0 first, in the middle, last, everywhere
    where = set()
    for c in synth:
        z = [int(c.eobs[k]) == 0 for k in c.coded()]
        if len(z) > 2 and any(z):
            where |= {"first"} if z[0] and not all(z) else set()
            where |= {"last"} if z[-1] and not all(z) else set()
            where |= {"middle"} if any(z[1:-1]) and not all(z) else set()
            where |= {"all"} if all(z) else set()
    assert where == {"first", "middle", "last", "all"}
    # DC of every sign; neighbour sums at the 63 clamp; non-zero starting contexts
    assert {int(np.sign(c.qc[k][0])) for c in synth for k in range(c.ntx) if c.eobs[k]} == {-1, 0, 1}
    assert any((c.cul & 63 == 63).any() for c in synth)
    assert any(c.ctx_in.any() for c in synth) and any(not c.ctx_in.any() for c in synth)
    # edges: last column, last row, both skipped; a coded block with a clipped span
    tw4 = lambda c: M.TX_W[c.ts] >> 2
    th4 = lambda c: M.TX_H[c.ts] >> 2
    assert any(c.mi_w < c.bw >> 2 and c.mi_w % tw4(c) == 0 and c.mi_h >= c.bh >> 2 for c in synth)
    assert any(c.mi_h < c.bh >> 2 and c.mi_h % th4(c) == 0 and c.mi_w >= c.bw >> 2 for c in synth)
    assert any(c.mi_w < c.bw >> 2 and c.mi_h < c.bh >> 2 for c in synth)
    assert any(c.clip_w4 < c.bw >> 2 and c.clip_w4 % tw4(c) for c in synth)
    assert any(c.mi_w < c.clip_w4 < 255 for c in synth)
    # counters on either side of update_cdf's rate steps
    counters = set()
    for c in synth:
        counters |= set(c.cdfs[0]["coeff_base"][:, 3].tolist()) | set(c.cdfs[0]["txb_skip"][:, 1].tolist())
    assert {0, 15, 16, 31, 32} <= counters
    assert sum(c.name.startswith("intra_split") for c in cases) >= 8 and sum(c.name.startswith("tx_tree") for c in cases) >= 8
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "coeff_rate_chain_ref.npz")) <= 512 * 1024


def test_one_transform_block_is_the_single_block_rate(fixture):
    """ntx == 1: the numbers of coeff_rate_model.coeff_rate with txb_skip_ctx 0 and the block's dc_sign_ctx"""
    from rav1e_amd import rdo_glue as RG
    _, cases = fixture
    ones = [c for c in cases if c.ntx == 1]
    assert len(ones) >= 10 and {c.ts for c in ones} >= {1, 4}
    for c in ones:
        sw, sh = min(M.TX_W[c.ts] >> 2, c.clip_w4), min(M.TX_H[c.ts] >> 2, c.clip_h4)
        skip_ctx, sign_ctx = RG.txb_ctx(c.ctx_in[:sw], c.ctx_in[16:16 + sh], 0, CM.BLOCK_DIMS[(c.bw, c.bh)], c.ts)
        assert skip_ctx == 0
        r = M.coeff_rate(c.qc[0], int(c.eobs[0]), c.ts, c.tt, 0, c.inter, c.red, 0, sign_ctx, c.y_mode, c.cdfs[0])
        assert (r[0], r[1]) == (c.rate, int(c.cul[0])), (c.k, c.name)
        assert c.indep == c.rate


def _moved(cases, **switch):
    return [c.name for c in cases if c.model(**switch)["rate"] != c.rate]


def test_every_carried_mechanism_moves_named_cases(fixture):
    """each of the four switched off in the model changes at least one case, and only cases where it can matter"""
    _, cases = fixture
    by_name = {c.name: c for c in cases}
    # the CDF carry: needs two coded blocks
    moved = _moved(cases, carry_cdfs=False)
    assert "8x8/4x4 r0 e0 p0 c0" in moved and len(moved) >= 40
    assert all(len(by_name[n].coded()) > 1 for n in moved)
    # set_coeff_context: needs a later block inside the block and a stored value that differs from the one in front
    # (a non-zero cul_level, or the 0 of an eob == 0 block over a non-zero starting context)
    moved = _moved(cases, set_context=False)
    assert "16x16/4x4 r0 e1 p1 c1" in moved and len(moved) >= 30
    assert all(by_name[n].ntx > 1 and (by_name[n].cul.any() or by_name[n].ctx_in.any()) for n in moved)
    # the clipped span of get_txb_ctx: needs clip_w4 / clip_h4 inside a coded transform block
    moved = _moved(cases, clipped_span=False)
    assert moved and all(by_name[n].clip_w4 < by_name[n].bw >> 2 or by_name[n].clip_h4 < by_name[n].bh >> 2 for n in moved)
    # the skip test: needs a block beyond mi_w / mi_h
    moved = _moved(cases, skip_test=False)
    assert moved and all(by_name[n].mi_w < by_name[n].bw >> 2 or by_name[n].mi_h < by_name[n].bh >> 2 for n in moved)
    # and the chain as a whole against the sum of independent single-block rates
    assert sum(c.indep != c.rate for c in cases) >= 60


def test_model_marks_bad_device_data(fixture):
    _, cases = fixture
    c = next(c for c in cases if c.name.startswith("16x16/4x4") and c.mi_w == 255 and c.mi_h == 255)
    for f, v in (("y_mode", 13), ("cdf_sel", 1), ("mi_w", 5), ("mi_h", 200)):
        ch = c.chain.copy()
        ch[f] = v
        if f.startswith("mi"):
            ch["clip_w4"], ch["clip_h4"] = 4, 199
        r = CM.coeff_rate_chain(c.qc, c.eobs, c.bw, c.bh, c.ts, c.tt, c.inter, c.red, ch, c.cdfs)
        assert r["rate"] == CM.INVALID and not any(r["txb_rate"]) and not any(r["cul"]) and not any(r["ctx"]), f
    e = c.eobs.copy()
    e[7] = 17
    assert CM.coeff_rate_chain(c.qc, e, c.bw, c.bh, c.ts, c.tt, c.inter, c.red, c.chain, c.cdfs)["rate"] == CM.INVALID
    ch = c.chain.copy()
    ch["mi_w"] = ch["clip_w4"] = 3                      # block 7 is no longer coded: its eob is not looked at
    assert CM.coeff_rate_chain(c.qc, e, c.bw, c.bh, c.ts, c.tt, c.inter, c.red, ch, c.cdfs)["rate"] != CM.INVALID


def test_glue_builds_the_fixture_descriptors(fixture):
    from rav1e_amd import rdo_glue as RG
    from rav1e_amd.types import TXB_CHAIN_CTX
    G, cases = fixture
    assert TXB_CHAIN_CTX == CM.CHAIN_DTYPE
    for c in cases:
        bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b = (int(v) for v in G["case_geom"][c.k])
        d = np.array([RG.txb_chain_ctx(G["case_above"][c.k], G["case_left"][c.k], bo_x, bo_y, c.bw, c.bh, mi_width, mi_height,
                                       w_in_b, h_in_b, c.y_mode, 0)], TXB_CHAIN_CTX)[0]
        assert d.tobytes() == c.chain.tobytes(), (c.k, c.name)


# ---- host refusals, in the manner of tests/test_entry_refusals.py (same harness: a zeroed stand-in context, host memory)


def _table():
    from test_entry_refusals import BUF as B
    base = dict(qcoeffs=B, coeff_bytes=2, eobs=B, n=0, tx_type_mask=1, bw=16, bh=16, tx_size=1, order=0, is_inter=0,
                use_reduced_tx_set=0, chains=B, cdfs=B, n_cdfs=1, rate_out=B, txb_rate_out=None, cul_level_out=None, ctx_out=None)
    rows = [
        (dict(), 0),
        (dict(txb_rate_out=B, cul_level_out=B, ctx_out=B), 0),
        (dict(order=1), 0),
        (dict(bw=8, bh=8), 0),                           # ntx 1
        (dict(bw=64, bh=64, tx_size=2), 0),              # ntx 16
        (dict(bw=64, bh=16, tx_size=18), 0),             # TX_64X16 on 64x16
        (dict(bw=16, bh=64, tx_size=9), 0),              # TX_16X32 on 16x64
        (dict(coeff_bytes=4), 0),
        # everything r1_coeff_rate_batch refuses
        (dict(coeff_bytes=1), -1), (dict(coeff_bytes=3), -1), (dict(coeff_bytes=8), -1),
        (dict(tx_size=19), -1), (dict(tx_size=-1), -1),
        (dict(tx_type_mask=0), -1), (dict(tx_type_mask=1 << 16), -1), (dict(tx_type_mask=0x0203, is_inter=1, use_reduced_tx_set=1), -1),
        (dict(tx_type_mask=0x0201, bw=64, bh=64, tx_size=3), -1),        # 32x32 intra: DCT only
        (dict(tx_type_mask=0x0201, bw=64, bh=64, tx_size=3, is_inter=1), 0),
        (dict(n_cdfs=0), -1), (dict(n_cdfs=257), -1), (dict(n_cdfs=-1), -1),
        (dict(qcoeffs=None), -1), (dict(eobs=None), -1), (dict(chains=None), -1), (dict(cdfs=None), -1), (dict(rate_out=None), -1),
        (dict(qcoeffs=None, n=1), -1), (dict(chains=None, n=1), -1),
        # the grid
        (dict(tx_size=2, bw=8, bh=8), -1),               # a transform larger than the block
        (dict(tx_size=8, bw=16, bh=4), -1),              # 16x8 does not divide 16x4
        (dict(tx_size=5, bw=8, bh=4), -1),
        (dict(tx_size=0, bw=32, bh=32), -1),             # ntx 64
        (dict(tx_size=0, bw=32, bh=16), -1),             # ntx 32
        (dict(tx_size=1, bw=64, bh=64), -1),             # ntx 64
        (dict(order=2), -1), (dict(order=-1), -1),
        # no block size
        (dict(bw=12, bh=16, tx_size=0), -1), (dict(bw=16, bh=24, tx_size=0), -1), (dict(bw=128, bh=128, tx_size=4), -1),
        (dict(bw=64, bh=8, tx_size=1), -1), (dict(bw=4, bh=32, tx_size=0), -1), (dict(bw=0, bh=16), -1), (dict(bw=16, bh=-16), -1),
        (dict(bw=2, bh=2, tx_size=0), -1),
    ]
    return base, rows


@pytest.fixture(scope="module")
def harness():
    from test_entry_refusals import Harness
    return Harness()


@pytest.mark.parametrize("row", range(len(_table()[1])))
def test_host_refusals(harness, row):
    base, rows = _table()
    over, status = rows[row]
    assert harness.call("r1_coeff_rate_chain_batch", base, over) == status, over


def test_struct_layout_equals_the_header_compiled_as_c(tmp_path):
    """R1TxbChainCtx: size 40 and every field offset, include/rav1e_amd.h compiled by gcc as C against the NumPy dtype"""
    from rav1e_amd.types import TXB_CHAIN_CTX as dt
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rav1e_amd.h"', 'int main(void) {',
             '  printf("size %zu 0\\n", sizeof(R1TxbChainCtx));']
    for f in dt.names:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(R1TxbChainCtx, %s), sizeof(((R1TxbChainCtx *)0)->%s));' % (f, f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in out if l}
    assert dt.itemsize == 40 and got["size"] == [40, 0]
    assert len(dt.names) == 9
    for f in dt.names:
        assert got[f] == [dt.fields[f][1], dt.fields[f][0].itemsize], (f, got[f])


def test_library_exports_the_chain():
    from rav1e_amd import _lib
    L = _lib.load()
    assert hasattr(L, "r1_coeff_rate_chain_batch") and "r1_coeff_rate_chain_batch" in _lib.SYMBOLS
    assert L.r1_coeff_rate_chain_batch.argtypes[5] is C.c_uint32 and len(L.r1_coeff_rate_chain_batch.argtypes) == 20
    assert L.r1_abi_version() == 7

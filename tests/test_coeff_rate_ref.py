"""The coefficient rate without a GPU: tests/golden/coeff_rate_ref.npz (the reference's write_coeffs_lv_map executed on
a WriterCounter through tools/rustlite, gen_coeff_rate_ref.py) against the Python model the GPU tests use
(tests/coeff_rate_model.py), the host glue (rdo_glue.txb_ctx, rdo_glue.pick_tx_type), the two new struct layouts
against the header compiled as C, and the export."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import coeff_rate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return M.load_fixture()


def test_model_reproduces_every_fixture_case(fixture):
    """rate, cul_level, the writer's final (bits, rng) and the (cdf id, symbol) list of all cases; the snapshot a case
    read is left as it was"""
    _, cases = fixture
    assert len(cases) >= 300
    for c in cases:
        before = c.cdfs.copy()
        rate, cul, bits, rng, syms = M.coeff_rate(c.qc, c.eob, c.ts, c.tt, c.plane, c.inter, c.red, c.txb_skip_ctx,
                                                  c.dc_sign_ctx, c.y_mode, c.cdfs)
        key = (c.k, c.ts, c.tt, c.plane, c.inter, c.eob)
        if syms != c.syms:
            first = next((i for i, (a, b) in enumerate(zip(syms, c.syms)) if a != b), min(len(syms), len(c.syms)))
            raise AssertionError((key, "symbol list differs at", first, syms[first:first + 3], c.syms[first:first + 3]))
        assert (rate, cul, bits, rng) == (c.rate, c.cul, c.bits, c.rng), key
        assert before.tobytes() == c.cdfs.tobytes(), key


def test_fixture_covers_what_the_issue_lists(fixture):
    _, cases = fixture
    assert {c.ts for c in cases} == set(range(19))
    assert {c.tt for c in cases} == {0, 1, 2, 3, 9, 10, 11}
    assert {c.txb_skip_ctx for c in cases} == set(range(13)) and {c.dc_sign_ctx for c in cases} == {0, 1, 2}
    assert {c.plane for c in cases} == {0, 1, 2} and {c.cb for c in cases} == {2, 4} and {c.kind for c in cases} == {0, 1, 2}
    assert {(c.inter, c.red) for c in cases if c.plane == 0} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert len({c.y_mode for c in cases if c.plane == 0 and not c.inter}) >= 8
    for ts in range(19):
        W, H = M.coded_dims(ts)
        eobs = {c.eob for c in cases if c.ts == ts}
        want = {0, 1, 2, W * H // 8, W * H // 8 + 1, W * H // 4, W * H // 4 + 1, W * H}
        want |= {g for g in M.K_EOB_GROUP_START if 0 < g <= W * H}
        assert want <= eobs, (ts, sorted(want - eobs))
    mags = set()
    for c in cases:
        mags |= set(np.abs(c.qc).tolist())
    assert {1, 2, 3, 14, 15, 127, 128, 32767, (1 << 20) - 1} <= mags
    assert any(c.eob > 1 and c.qc[0] < 0 for c in cases) and any(c.eob > 1 and c.qc[0] == 0 for c in cases)
    assert any((c.cul & 63) == 63 for c in cases) and any(0 < (c.cul & 63) < 63 for c in cases)
    counters = set()
    for c in cases:
        if c.kind == 2:
            counters |= set(c.cdfs["coeff_base"][:, 3].tolist())
    assert {0, 15, 16, 31, 32} <= counters
    # one context row hit hundreds of times
    assert max(max(np.bincount([i for i, _ in c.syms])) for c in cases if c.syms) >= 300


def test_restated_tables_equal_the_executed_text(fixture):
    """everything the model and the kernel restate from the reference: the dimension constants (also against the
    header's R1_ macros and types.py), the tx-set tables, the eob token tables as closed forms, the context offset
    tables by their rules, the scan orders"""
    G, _ = fixture
    from rav1e_amd import types as T
    names = ("TXB_SKIP_CONTEXTS", "EOB_COEF_CONTEXTS", "SIG_COEF_CONTEXTS_EOB", "SIG_COEF_CONTEXTS", "LEVEL_CONTEXTS",
             "BR_CDF_SIZE", "DC_SIGN_CONTEXTS", "INTRA_MODES")
    hdr = open(os.path.join(ROOT, "include", "rav1e_amd.h")).read()
    for n, v in zip(names, G["dims"]):
        assert getattr(M, n) == int(v) and getattr(T, n) == int(v), n
        assert int(re.search(r"#define R1_%s (\d+)" % n, hdr).group(1)) == int(v), n
    assert T.COEFF_CDFS == M.CDFS_DTYPE and T.TXB_CTX == M.TXB_CTX_DTYPE
    assert np.array_equal(G["tx_wh"], np.array([M.TX_W, M.TX_H, [M.coded_dims(t)[0] for t in range(19)],
                                                 [M.coded_dims(t)[1] for t in range(19)]]))
    assert np.array_equal(G["tab_av1_tx_ind"], np.array(M.AV1_TX_IND))
    assert np.array_equal(G["tab_num_tx_set"], np.array(M.NUM_TX_SET))
    used = G["tab_av1_tx_used"]
    assert [sum(int(used[s][t]) << t for t in range(16)) for s in range(6)] == list(M.TX_USED_MASK)
    assert [M.tx_class(t) for t in range(16)] == G["tab_tx_type_to_class"].tolist()
    assert [M.txs_ctx(t) for t in range(19)] == G["tab_txs_ctx"].tolist()
    for ts in range(19):
        for i in (0, 1):
            for r in (0, 1):
                assert M.tx_set(ts, i, r) == int(G["tab_tx_set"][ts, i, r]), (ts, i, r)
    assert list(M.K_EOB_GROUP_START) == G["tab_k_eob_group_start"].tolist()
    assert list(M.K_EOB_OFFSET_BITS) == G["tab_k_eob_offset_bits"].tolist()
    small, large, start = G["tab_eob_to_pos_small"], G["tab_eob_to_pos_large"], G["tab_k_eob_group_start"]
    for eob in range(1, 1025):
        t = int(small[eob]) if eob < 33 else int(large[min((eob - 1) >> 5, 16)])
        assert M.eob_pos_token(eob) == (t, eob - int(start[t])), eob
        # the kernel's closed forms
        pt = eob if eob < 3 else (eob - 1).bit_length() + 1
        assert pt == t and (pt if pt < 3 else (1 << (pt - 2)) + 1) == int(start[t])
        assert (0 if pt < 3 else pt - 2) == int(G["tab_k_eob_offset_bits"][t])
    assert [26 + (0 if i == 0 else (5 if i == 1 else 10)) for i in range(32)] == G["tab_nz_map_ctx_offset_1d"].tolist()
    tab = G["tab_av1_nz_map_ctx_offset"]
    for ts in range(19):
        W, H = M.coded_dims(ts)
        for row in range(min(H, 5)):
            for col in range(min(W, 5)):
                assert M.nz_map_ctx_offset(ts, row, col) == int(tab[ts][row][col]), (ts, row, col)
    for ts in range(19):
        W, H = M.coded_dims(ts)
        for tt in range(16):
            o = int(G["scan_off"][ts, tt])
            assert M.scan_order(ts, tt) == G["scan_all"][o:o + W * H].tolist(), (ts, tt)


def test_txb_ctx_matches_the_executed_get_txb_ctx(fixture):
    G, _ = fixture
    from rav1e_amd import rdo_glue as RG
    rows = G["txb_rows"]
    assert len(rows) == 200
    seen = set()
    for r in rows:
        above, left, (plane, bsize, ts, want_skip, want_sign) = r[:16], r[16:32], [int(v) for v in r[32:]]
        got = RG.txb_ctx(above[:M.TX_W[ts] >> 2], left[:M.TX_H[ts] >> 2], plane, bsize, ts)
        assert got == (want_skip, want_sign), r.tolist()
        seen.add(want_skip)
    assert seen == set(range(13))


def test_pick_tx_type():
    from rav1e_amd import rdo_glue as RG
    lam = 0.37
    cost = lambda r, d: RG.compute_rd_cost(lam, r, d)
    # the cheapest slot wins
    assert RG.pick_tx_type([800, 640, 900], [1000, 1010, 400], lam, 1e30) == (2, cost(900, 400))
    # a tie keeps the first of the two (strict <)
    assert RG.pick_tx_type([800, 800, 800], [500, 500, 500], lam, 1e30) == (0, cost(800, 500))
    assert RG.pick_tx_type([900, 800, 800], [500, 400, 400], lam, 1e30) == (1, cost(800, 400))
    # the early exit: the first cost above cur_best_rd ends the loop with the initial (DCT_DCT, f64::MAX)
    assert RG.pick_tx_type([800, 8, 8], [500, 1, 1], lam, cost(800, 500) - 1e-6) == (None, sys.float_info.max)
    # equal to cur_best_rd is not above it; later types are not subject to the exit
    assert RG.pick_tx_type([800, 80000], [500, 1], lam, cost(800, 500)) == (0, cost(800, 500))
    assert RG.pick_tx_type([800, 8], [500, 1], lam, cost(800, 500)) == (1, cost(8, 1))
    # one rounding: lambda * rate / 8 + distortion as a fused multiply-add
    assert RG.pick_tx_type([3], [(1 << 53) + 1], 1.0, 1e30)[1] == float((1 << 53) + 2)


def test_new_struct_layouts_equal_the_header_compiled_as_c(tmp_path):
    """R1CoeffCdfs / R1TxbCtx: sizeof and every field offset, include/rav1e_amd.h compiled by gcc as C against the
    NumPy dtypes of rav1e_amd/types.py"""
    from rav1e_amd import types as T
    pairs = {"R1CoeffCdfs": T.COEFF_CDFS, "R1TxbCtx": T.TXB_CTX}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rav1e_amd.h"', 'int main(void) {']
    for cname, dt in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, f, cname, f, cname, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): [int(v) for v in l.split()[2:]] for l in out if l}
    assert T.COEFF_CDFS.itemsize == 1088 and T.TXB_CTX.itemsize == 4
    for cname, dt in pairs.items():
        assert got[(cname, "size")] == [dt.itemsize], cname
        for f in dt.names:
            sub, off = dt.fields[f][0], dt.fields[f][1]
            assert got[(cname, f)] == [off, sub.itemsize], (cname, f, got[(cname, f)], off, sub.itemsize)


def test_library_exports_the_coefficient_rate():
    from rav1e_amd import _lib
    L = _lib.load()
    assert hasattr(L, "r1_coeff_rate_batch") and "r1_coeff_rate_batch" in _lib.SYMBOLS
    assert L.r1_coeff_rate_batch.argtypes[5] is C.c_uint32 and len(L.r1_coeff_rate_batch.argtypes) == 16
    assert L.r1_abi_version() == 7

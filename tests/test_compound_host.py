"""The compound (two-reference) candidate without a device: descriptor layout, the exported symbol, the host
arithmetic of rdo_glue.compound_cands against the reference-executed vectors, and the NULL-context refusal."""
import ctypes as C

import numpy as np


def test_compound_cand_layout():
    """R1CompoundCand as include/rav1e_amd.h declares it, field by field: six int16 and eight bytes = 20 bytes (the
    fields of the declaration add up to 20, not to the 16 its first draft's comment said), the ctypes struct and the
    numpy dtype agreeing on every offset"""
    from rav1e_amd import _lib
    from rav1e_amd.api import COMPOUND_CAND
    want = [("ox", 0), ("oy", 2), ("rx0", 4), ("ry0", 6), ("rx1", 8), ("ry1", 10), ("col_frac0", 12),
            ("row_frac0", 13), ("col_frac1", 14), ("row_frac1", 15), ("mode_x", 16), ("mode_y", 17), ("reserved", 18)]
    assert C.sizeof(_lib.R1CompoundCand) == 20 == COMPOUND_CAND.itemsize
    assert [(n, getattr(_lib.R1CompoundCand, n).offset) for n, _ in _lib.R1CompoundCand._fields_] == want
    assert [(n, COMPOUND_CAND.fields[n][1]) for n in COMPOUND_CAND.names] == want
    for n, _ in want[:-1]:
        assert getattr(_lib.R1CompoundCand, n).size == COMPOUND_CAND.fields[n][0].itemsize, n
    assert _lib.R1CompoundCand.reserved.size == 2 == COMPOUND_CAND.fields["reserved"][0].itemsize


def test_library_exports_compound_symbol():
    from rav1e_amd import _lib
    assert "r1_rdo_compound_cand_batch" in _lib.SYMBOLS
    L = _lib.load()
    f = L.r1_rdo_compound_cand_batch
    assert f.restype is C.c_int and len(f.argtypes) == 12
    assert L.r1_abi_version() == 7


def test_compound_cands_match_reference_rows():
    """rdo_glue.compound_cands against every executed predict_inter_compound case of rdo_glue_ref.npz: the
    (px, py, col_frac, row_frac) pairs are the ones rdo_glue_cases.check_compound derives for the same row"""
    import rdo_glue_cases as RC
    from rav1e_amd import rdo_glue as RG
    G = np.load(RC.GOLD)
    n = 0
    for k in [str(k) for k in G["pic_keys"]]:
        filt = {"REGULAR": 0, "SHARP": 2}[k.split("_")[1]]
        rows = [[int(v) for v in row] for row in G["pic_rows_" + k]]
        for (w, h, x, y, r0, c0, r1, c1, _) in rows:
            want = []
            for (mr, mc) in ((r0, c0), (r1, c1)):          # as check_compound
                rf, cf, px, py = RG.get_mv_params(mr, mc, x, y)
                want.append((px, py, cf, rf))
            c = RG.compound_cands(x, y, [(r0, c0)], [(r1, c1)], filt)
            assert len(c) == 1 and (int(c["ox"][0]), int(c["oy"][0])) == (x, y)
            got = [tuple(int(c[f % i][0]) for f in ("rx%d", "ry%d", "col_frac%d", "row_frac%d")) for i in (0, 1)]
            assert got == want, (k, w, h, x, y, got, want)
            assert (int(c["mode_x"][0]), int(c["mode_y"][0])) == (filt, filt)
            n += 1
        # and as ONE list per block position: the i-th entry pairs mvs0[i] with mvs1[i]
        x, y = rows[0][2], rows[0][3]
        c = RG.compound_cands(x, y, [(r[4], r[5]) for r in rows], [(r[6], r[7]) for r in rows], filt)
        for i, r in enumerate(rows):
            one = RG.compound_cands(x, y, [(r[4], r[5])], [(r[6], r[7])], filt)
            assert c[i] == one[0]
    assert n == 3 * 2 * 21
    # decimated planes shift like get_mv_params does
    c = RG.compound_cands(10, 6, [(-13, 27)], [(5, -9)], 1, xdec=1, ydec=1)
    assert tuple(int(c[f][0]) for f in ("row_frac0", "col_frac0", "rx0", "ry0")) == RG.get_mv_params(-13, 27, 10, 6, 1, 1)
    assert tuple(int(c[f][0]) for f in ("row_frac1", "col_frac1", "rx1", "ry1")) == RG.get_mv_params(5, -9, 10, 6, 1, 1)


def test_compound_null_context_is_einval():
    """argument checks come before anything touches a device"""
    from rav1e_amd import _lib
    L = _lib.load()
    pl = _lib.R1Plane(None, 64, 64, 16, 16, 0, 0, 1, 8)
    cands = (_lib.R1CompoundCand * 1)()
    out = (C.c_uint32 * 1)(0xdeadbeef)
    rc = L.r1_rdo_compound_cand_batch(None, C.byref(pl), C.byref(pl), C.byref(pl), 8, 8,
                                      C.cast(cands, C.c_void_p), 1, None, C.cast(out, C.c_void_p), None, None)
    assert rc == -1 and out[0] == 0xdeadbeef

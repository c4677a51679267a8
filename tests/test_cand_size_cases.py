"""The case tables of tests/cand_size_cases.py against the kernels they are there to launch, without a device: the
host compiler says which k_rdo_cand<.., PS = 1> the plan names (tests/c/rdo_plan_list.cpp) and which route an
r1_rdo_intra_cand_batch call takes (tests/c/rdo_intra_route_list.cpp); every table row is mapped to the kernel it
launches, and the set reached must be the 105 exactly.  Likewise the compound table and the 19 x 3 k_compound_fast."""
import os
import subprocess

import pytest

import cand_size_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FANOUT, PER_TYPE, TWO_LAUNCH = 0, 1, 2      # RdoIntraRoute


def _host_rows(tmp, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "rav1e_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", name + ".cpp")])
    return [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe], text=True).splitlines()]


@pytest.fixture(scope="module")
def intra_kernels(tmp_path_factory):
    """the (BD, WL, HL, QM, MT) of every PS = 1 instantiation the plan names"""
    rows = _host_rows(tmp_path_factory.mktemp("plan"), "rdo_plan_list")
    keys = {r[:5] for r in rows if r[5] == 1}
    assert len(keys) == 105
    return keys


@pytest.fixture(scope="module")
def intra_route(tmp_path_factory):
    """{(BD, WL, HL, QM): route}"""
    rows = _host_rows(tmp_path_factory.mktemp("route"), "rdo_intra_route_list")
    assert len(rows) == 3 * 19 * 2
    return {r[:4]: r[4] for r in rows}


def reached(rows, route):
    """the PS = 1 kernels the (TxSize id, bit depth, dist_kind) rows launch: dist_kind 0 is QM 1 and a pixel kind QM 2;
    route 0 launches the MT form, route 1 the plain form, route 2 (the two launches) no PS = 1 kernel"""
    out = set()
    for ts, bd, kind in rows:
        w, h = K.TX_DIMS[ts]
        wl, hl, qm = w.bit_length() - 1, h.bit_length() - 1, 1 if kind == 0 else 2
        r = route[bd, wl, hl, qm]
        assert r in (FANOUT, PER_TYPE, TWO_LAUNCH)
        if r != TWO_LAUNCH:
            out.add((bd, wl, hl, qm, int(r == FANOUT)))
    return out


def test_the_tables_are_the_ones_the_gpu_tests_parametrise_over():
    import test_gpu_compound as CP
    import test_gpu_depth12 as D12
    import test_gpu_rdo_intra as RI
    assert RI.CASES is K.INTRA_CASES and RI.TX_DIMS is K.TX_DIMS
    assert D12.INTRA_SIZES is K.DEPTH12_INTRA_SIZES and D12.KINDS is K.INTRA_KINDS and D12.BD == 12
    assert CP.SIZES is K.COMPOUND_SIZES
    assert len(K.TX_DIMS) == 19 == len(set(K.TX_DIMS))
    assert 0 in K.INTRA_KINDS and any(k != 0 for k in K.INTRA_KINDS)


def test_no_intra_row_twice():
    pairs = K.INTRA_CASES + [(ts, 12) for ts in K.DEPTH12_INTRA_SIZES]
    assert len(pairs) == len(set(pairs)) == 19 * 3
    assert set(K.INTRA_CASES_SEEDED).isdisjoint(K.INTRA_CASES_EOB)


def test_intra_rows_launch_every_ps1_kernel_of_the_plan(intra_kernels, intra_route):
    got = reached(K.intra_rows(), intra_route)
    assert sorted(intra_kernels - got) == [], "(BD, WL, HL, QM, MT) instantiated and launched by no row"
    assert sorted(got - intra_kernels) == [], "a row maps to a kernel the plan does not name"
    assert len(got) == 105


def test_every_intra_row_is_needed(intra_kernels, intra_route):
    """the check above is not vacuous: without any one (size, depth) pair that has a fused point a kernel is missed"""
    rows = K.intra_rows()
    for pair in sorted({r[:2] for r in rows}):
        rest = reached([r for r in rows if r[:2] != pair], intra_route)
        lost = intra_kernels - rest
        assert lost == reached([r for r in rows if r[:2] == pair], intra_route), pair
    # (16x16 at 10 and 12 bits takes the two launches for every kind: those pairs launch no PS = 1 kernel)
    none = sorted({r[:2] for r in rows if not reached([q for q in rows if q[:2] == r[:2]], intra_route)})
    assert none == [(2, 10), (2, 12)], none


def test_compound_table_holds_every_size_at_every_depth():
    """k_compound_fast<BD, WL, HL>: one `case` per R1_TX_SIZES entry and depth in mc_compound.hip"""
    fast = {(bd, w, h) for (w, h) in K.COMPOUND_SIZES for bd in K.COMPOUND_DEPTHS if (w, h) in K.TX_DIMS}
    assert fast == {(bd, w, h) for (w, h) in K.TX_DIMS for bd in (8, 10, 12)} and len(fast) == 57
    assert len(K.COMPOUND_SIZES) == len(set(K.COMPOUND_SIZES))
    # and the slab kernel keeps its two- and four-slab block sizes
    assert {(128, 64), (128, 128)} <= set(K.COMPOUND_SIZES)

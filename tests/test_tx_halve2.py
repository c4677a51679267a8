"""The two-instruction halving of the fused kernels' forward networks (namespace m24h of rav1e_amd/csrc/tx_common.hpp):

    TX_RSHIFT1(a) = (a + (a < 0)) >> 1      ==      (a - (a >> 24)) >> 1        while |a| < 2^24

on the host.  The bound of every halving operand (tools/tx_range.py halving_bounds(): column pass, then the row pass
fed with the column outputs after shift[1], residuals from pixels) against 2^24 for every (size, type, bit depth)
the form may be enabled for; the NumPy networks (oracle/fwd_tx_np.py) run whole with either halving -- every one of
them, those the rotation kernels bound at import included, counted against the generator's trace -- on random
residual blocks and on the full-scale sign patterns of tests/golden/fwd_tx_ref.npz; the identity at and just past the
bound; and the header's text: the macro m24h compiles is the form tested here, and rdo_halve2 (rdo_cand_plan.hpp)
names no instantiation outside what this file covers."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rav1e_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_tx1d as G  # noqa: E402
import tx_range as R  # noqa: E402
import fwd_tx_ref_util as U  # noqa: E402

F = G.F
I32 = np.int32
LIMIT = 1 << 24
# the instantiations rdo_halve2 may name: the coefficient kernels of the square sizes 8x8 .. 64x64 at 8 and 10 bits
SIZES = {1: 8, 2: 16, 3: 32, 4: 64}          # TxSize id -> side
CASES = [(bd, ts, tt) for bd in (8, 10) for ts in SIZES for tt in range(16) if F.valid_av1_transform(ts, tt)]


def halve_old(a):
    return (a + (a < 0).astype(I32)) >> I32(1)


def halve_new(a):
    return (a - (a >> I32(24))) >> I32(1)


def forward(res, ts, tt, bd, halve):
    """F.forward_transform with EVERY halving of the networks replaced -> (coefficients, [largest |operand| of each
    halving, in execution order]).  The module calls the halving under three names: `rshift1` itself, and the copies
    the rotation kernels RotateAddShift / RotateSubShift bound as `SHIFT` when they were made -- most of the halvings
    of the larger networks.  All three go through the spy; tape_halvings() below counts that none is left out."""
    seen = []
    orig = F.rshift1
    assert F.RotateAddShift.SHIFT is orig and F.RotateSubShift.SHIFT is orig

    def spy(a):
        seen.append(int(np.abs(a.astype(np.int64)).max()))
        return halve(a)
    F.rshift1 = F.RotateAddShift.SHIFT = F.RotateSubShift.SHIFT = spy
    try:
        return F.forward_transform(res, ts, tt, bd), seen
    finally:
        F.rshift1 = F.RotateAddShift.SHIFT = F.RotateSubShift.SHIFT = orig


def tape_halvings(t):
    """[is it live?] for every TX_RSHIFT1 of 1-D network `t` in execution order: the symbolic trace the generator
    makes, before its dead-code elimination (a numeric run executes the dead ones too; the device code is the live
    ones, tools/gen_tx1d.py trace_ops)"""
    if G.NAMES[t] is None:
        return []
    n = F.TXFM_LEN[t]
    tape = []
    F.TXFM_FUNCS[t]([F.Sym("c%d" % i, tape) for i in range(n)])
    live = set(name for name, expr in G.trace_ops(t)[1] if expr.startswith("TX_RSHIFT1("))
    flags = [name in live for name, expr in tape if expr.startswith("TX_RSHIFT1(")]
    assert sum(flags) == len(live)
    return flags


def chain_halvings(ts, tt):
    """the halvings of the column network, then those of the row network, as forward_transform executes them"""
    w, h = F.TX_DIMS[ts]
    tcol = F.TXFM_TYPE_LS[h.bit_length() - 3][F.VTX_TAB[tt]]
    trow = F.TXFM_TYPE_LS[w.bit_length() - 3][F.HTX_TAB[tt]]
    return tape_halvings(tcol) + tape_halvings(trow)


@pytest.fixture(scope="module")
def bounds():
    return R.halving_bounds()


def test_bound_of_every_halving_operand(bounds):
    """below 2^24 wherever the form may be enabled -- and, as it happens, at every size, type and bit depth"""
    for key in CASES:
        assert bounds[key] < LIMIT, (key, bounds[key])
    assert set(bounds) >= set(CASES)
    worst = max(bounds.values())
    assert worst < LIMIT and worst < (1 << 19), worst
    # the generator's own assertion covers the column family
    assert G.HALVE2_LIMIT == LIMIT
    G.col_family()


def test_identity_inside_the_bound_and_where_it_ends():
    """(a - (a >> 24)) >> 1 is the halving toward zero exactly while a >> 24 is the sign, 0 or -1: |a| < 2^24.  The
    first value past the bound, a = 2^24, already differs (a >> 24 = 1): the bound is the condition, not a margin.
    On the negative side a = -2^24 still has a >> 24 = -1; a = -2^24 - 1 has a >> 24 = -2 but is odd, where one more
    unit before the shift changes nothing, so the first negative value that differs is -2^24 - 2."""
    edge = np.array([0, 1, -1, 2, -2, 3, -3, LIMIT - 1, LIMIT - 2, -(LIMIT - 1), -(LIMIT - 2), -LIMIT], I32)
    assert np.array_equal(halve_old(edge), halve_new(edge))
    rng = np.random.default_rng(24)
    a = rng.integers(-(LIMIT - 1), LIMIT, 1 << 20, dtype=I32)
    assert np.array_equal(halve_old(a), halve_new(a))
    for a, same in ((LIMIT, False), (LIMIT + 1, True), (-LIMIT - 1, True), (-LIMIT - 2, False), (LIMIT + 2, False)):
        x = np.array([a], I32)
        assert (halve_old(x)[0] == halve_new(x)[0]) == same, a
    # toward zero, both signs
    assert halve_new(np.array([-3, 3, -1, 1], I32)).tolist() == [-1, 1, 0, 0]


@pytest.fixture(scope="module")
def golden():
    return {(c.bd, c.ts, c.tt): c for bd in (8, 10) for c in U.load()[bd]}


@pytest.mark.parametrize("bd,ts,tt", CASES, ids=["%d_%dx%d_t%d" % (c[0], SIZES[c[1]], SIZES[c[1]], c[2]) for c in CASES])
def test_networks_agree_with_either_halving(bounds, golden, bd, ts, tt):
    n = SIZES[ts]
    mx = (1 << bd) - 1
    rng = np.random.default_rng(2400 + 100 * bd + 16 * ts + tt)
    nb = -(-100000 // n)                       # 10^5 residual columns
    sets = {"random": rng.integers(-mx, mx + 1, (nb, n, n)).astype(np.int16),
            "random small": rng.integers(-3, 4, (64, n, n)).astype(np.int16)}
    case = golden.get((bd, ts, tt))
    assert case is not None, "fwd_tx_ref.npz has every square size and type"
    sg = np.where(case.res >= 0, 1, -1).astype(np.int16)
    sets["full-scale sign patterns"] = np.concatenate([sg * mx, -sg * mx, sg.transpose(0, 2, 1) * mx])
    live = chain_halvings(ts, tt)
    for name, res in sets.items():
        old, seen_old = forward(res, ts, tt, bd, halve_old)
        new, seen_new = forward(res, ts, tt, bd, halve_new)
        assert np.array_equal(old, new), (name, bd, ts, tt)
        assert seen_old == seen_new
        # every halving of both networks went through the replaced form, none more, none less
        assert len(seen_new) == len(live), (name, len(seen_new), len(live))
        # the bound is a bound: no operand of a halving the device code executes exceeds it
        met = [v for v, lv in zip(seen_new, live) if lv]
        assert not met or max(met) <= bounds[bd, ts, tt], (name, max(met), bounds[bd, ts, tt])
        assert max(seen_new, default=0) < LIMIT
    # the golden coefficients, executed from the reference's text, through the new form
    new, seen = forward(case.res, ts, tt, bd, halve_new)
    assert np.array_equal(new.astype(case.coef.dtype), case.coef) and len(seen) == len(live)


def test_the_spy_meets_every_traced_halving():
    """the counts the replaced form must be called with are the generator's: per network, the TX_RSHIFT1 of the traced
    SSA (live ones = the statements of fwd_tx_1d.inc), and a DCT / ADST chain of any size here has some"""
    inc = open(os.path.join(CSRC, "fwd_tx_1d.inc")).read()
    for t, nm in enumerate(G.NAMES):
        if nm is None:
            continue
        body = inc[inc.index("void r1_%s(T *c) {" % nm):]
        body = body[:body.index("\n}")]
        assert body.count("TX_RSHIFT1(") == sum(tape_halvings(t)), nm
    assert sum(tape_halvings(1)) == 8 and sum(tape_halvings(4)) == 114      # fdct8, fdct64 (fwd_tx_1d.inc)
    for bd, ts, tt in CASES:
        if tt != 9:                                   # IDTX: both passes are the identity
            assert sum(chain_halvings(ts, tt)) > 0, (ts, tt)


def test_header_compiles_the_form_tested_here():
    txt = open(os.path.join(CSRC, "tx_common.hpp")).read()
    body = txt[txt.index("namespace m24h {"):txt.index("}  // namespace m24h")]
    m = re.findall(r"#define TX_RSHIFT1\(a\) (.*)", body)
    assert m[0] == "(TX_SUB((a), (a) >> 24) >> 1)"                 # what m24h's networks see
    assert m[1] == "(TX_ADD((a), (T)((a) < 0)) >> 1)"               # put back for whoever includes the header
    assert body.count('#include "fwd_tx_1d.inc"') == 1 and body.count('#include "fwd_tx_1d_col.inc"') == 1


PLAN_MAIN = r"""
#include <cstdio>
#include "rdo_cand_plan.hpp"
int main() {
  for (int bd = 8; bd <= 12; bd += 2) for (int wl = 2; wl <= 6; wl++) for (int hl = 2; hl <= 6; hl++)
    for (int qm = 0; qm < 3; qm++) for (int mt = 0; mt < 2; mt++) for (int ps = 0; ps < 2; ps++)
      if (rdo_halve2(bd, wl, hl, qm, mt, ps) || rdo_mc_pack4(bd, wl, hl, qm, mt, ps))
        std::printf("%d %d %d %d %d %d %d %d\n", bd, wl, hl, qm, mt, ps, (int)rdo_halve2(bd, wl, hl, qm, mt, ps),
                    (int)rdo_mc_pack4(bd, wl, hl, qm, mt, ps));
}
"""


def test_plan_enables_only_what_is_covered(tmp_path):
    """the plan header, compiled on the host: the instantiations that take the halving are coefficient kernels (QM 0,
    no type search, no intra source) of square sizes among this file's CASES -- exactly the ones measured faster --
    and the shift-free pack goes to 8-bit ones only"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "a host C++ compiler is needed"
    (tmp_path / "p.cpp").write_text(PLAN_MAIN)
    exe = str(tmp_path / "p")
    subprocess.check_call([cxx, "-std=c++17", "-I" + CSRC, "-o", exe, str(tmp_path / "p.cpp")])
    rows = [tuple(int(v) for v in ln.split()) for ln in subprocess.check_output([exe], text=True).splitlines()]
    covered = set((bd, SIZES[ts]) for bd, ts, _ in CASES)
    for bd, wl, hl, qm, mt, ps, halve, pack in rows:
        assert (qm, mt, ps) == (0, 0, 0) and wl == hl, (bd, wl, hl, qm, mt, ps)
        assert not halve or (bd, 1 << wl) in covered
        assert not pack or bd == 8
    assert sorted((bd, 1 << wl) for bd, wl, *_r, halve, _p in rows if halve) == \
        [(8, 8), (8, 16), (8, 32), (8, 64), (10, 16), (10, 64)]
    assert sorted((bd, 1 << wl) for bd, wl, *_r, pack in rows if pack) == [(8, 8), (8, 16), (8, 32)]

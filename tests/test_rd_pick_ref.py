"""The RD decision without a GPU: tests/golden/rd_pick_ref.npz -- compute_rd_cost, rdo_tx_type_decision and
rdo_tx_size_type executed from the reference's text (tests/golden/gen_rd_pick_ref.py) -- against the host statements
r1_rd_pick_batch is held to (rdo_glue.compute_rd_cost, pick_tx_type, pick_first_min, tx_size_type_decision); the
layout of R1RdPick; what the two entry points answer to a bad argument.

The reference converts the distortion to f64 BEFORE its fused multiply-add (`distortion.0 as f64`); compute_rd_cost and
pick_tx_type add the integer they are given exactly, so they are handed rdo_glue.dist_as_f64(dist) here, as
pick_first_min and tx_size_type_decision hand it themselves.  Below 2^53 that is dist itself."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from rav1e_amd import rdo_glue
from rav1e_amd.types import RD_PICK
from test_entry_refusals import BUF, Harness, P, fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_MAX = sys.float_info.max


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "rd_pick_ref.npz"))


def bits(v):
    return np.array(v, np.float64).view(np.uint64)


# ---------------------------------------------------------------- the fixture through the host statements
def test_fixture_holds_the_cases_the_feature_is_about(ref):
    assert int(ref["n_fused_differs"]) >= 50 and int((ref["cost_kind"] == 1).sum()) == int(ref["n_fused_differs"])
    assert {int(v) for v in ref["tt_nt"]} == {1, 2, 5, 7, 16}
    assert {int(v) for v in ref["sz_depth"]} == {0, 1, 2}
    assert {0, 1, 7, 8, 2 ** 32 - 2} <= {int(v) for v in ref["cost_rate"]}
    assert {2 ** 53 + 1, 2 ** 53 + 3, 2 ** 63 + 2 ** 10 + 1, 2 ** 64 - 1} <= {int(v) for v in ref["cost_dist"]}
    assert 0.0 in ref["cost_lam"] and 8.0 in ref["cost_lam"]
    assert (ref["tt_slot"] == -1).any() and (ref["tt_evals"][ref["tt_slot"] == -1] == 1).all()
    # the tuples of kind 1 are those where a multiply and an add round differently from the fused form
    k1 = ref["cost_kind"] == 1
    twice = ref["cost_lam"][k1] * (ref["cost_rate"][k1] / 8.0) + ref["cost_dist"][k1].astype(np.float64)
    assert (bits(twice) != bits(ref["cost_rd"][k1])).all()


def test_compute_rd_cost_bit_for_bit(ref):
    got = [rdo_glue.compute_rd_cost(float(l), int(r), rdo_glue.dist_as_f64(d)) for l, r, d in zip(ref["cost_lam"], ref["cost_rate"], ref["cost_dist"])]
    assert np.array_equal(bits(got), bits(ref["cost_rd"]))


def type_case(ref, i):
    nt = int(ref["tt_nt"][i])
    return [int(v) for v in ref["tt_rate"][i, :nt]], [rdo_glue.dist_as_f64(v) for v in ref["tt_dist"][i, :nt]], float(ref["tt_lam"][i]), float(ref["tt_cur"][i])


def test_pick_tx_type_reproduces_rdo_tx_type_decision(ref):
    for i, name in enumerate(ref["tt_names"]):
        slot, rd = rdo_glue.pick_tx_type(*type_case(ref, i))
        assert (-1 if slot is None else slot) == int(ref["tt_slot"][i]), name
        assert bits(rd) == bits(ref["tt_rd"][i]), name


def size_case(ref, i):
    nd = int(ref["sz_ndepth"][i])
    rates = [[int(v) for v in ref["sz_rate"][i, d, :ref["sz_nt"][i, d]]] for d in range(nd)]
    dists = [[int(v) for v in ref["sz_dist"][i, d, :ref["sz_nt"][i, d]]] for d in range(nd)]
    return rates, dists, float(ref["sz_lam"][i])


def test_tx_size_type_decision_reproduces_rdo_tx_size_type(ref):
    for i, name in enumerate(ref["sz_names"]):
        depth, slot, rd = rdo_glue.tx_size_type_decision(*size_case(ref, i))
        assert (depth, slot) == (int(ref["sz_depth"][i]), int(ref["sz_slot"][i])), name
        assert bits(rd) == bits(ref["sz_rd"][i]), name


def test_pick_first_min_reproduces_the_mode_loop(ref):
    for i, name in enumerate(ref["fm_names"]):
        n = int(ref["fm_n"][i])
        best_in = float(ref["fm_best_in"][i])
        idx, rd, rate, dist = rdo_glue.pick_first_min(ref["fm_rate"][i, :n], ref["fm_dist"][i, :n], float(ref["fm_lam"][i]),
                                                      best=(None, best_in, 0, 0), rate_adds=ref["fm_add"][i, :n])
        want = int(ref["fm_idx"][i])
        assert (-1 if idx is None else idx) == want, name
        assert bits(rd) == bits(ref["fm_rd"][i, want] if want >= 0 else best_in), name
        if want >= 0:
            assert (rate, dist) == (int(ref["fm_rate"][i, want]) + int(ref["fm_add"][i, want]), int(ref["fm_dist"][i, want])), name


def test_pick_first_min_costs_an_invalid_rate_infinity():
    inv = rdo_glue.RATE_INVALID
    assert rdo_glue.pick_first_min([inv, 8], [0, 10 ** 15], 1.0)[0] == 1
    assert rdo_glue.pick_first_min([8, 8], [0, 0], 1.0, rate_adds=[inv - 8, 1])[0] == 1
    assert rdo_glue.pick_first_min([inv], [0], 0.0) == (None, F64_MAX, 0, 0)


# ---------------------------------------------------------------- a local copy of the model with its two decisions switchable
def model_tx_type(rates, dists, lam, cur_best_rd, early_exit=True, strict=True):
    best, best_rd = None, F64_MAX
    for j, (rate, dist) in enumerate(zip(rates, dists)):
        rd = rdo_glue.compute_rd_cost(lam, rate, dist)
        if early_exit and j == 0 and rd > cur_best_rd:
            break
        if rd < best_rd or (not strict and rd <= best_rd):
            best, best_rd = j, rd
    return best, best_rd


def moved(ref, **kw):
    out = set()
    for i, name in enumerate(ref["tt_names"]):
        slot, rd = model_tx_type(*type_case(ref, i), **kw)
        if (-1 if slot is None else slot) != int(ref["tt_slot"][i]) or bits(rd) != bits(ref["tt_rd"][i]):
            out.add(str(name))
    return out


def test_the_model_copy_is_the_model(ref):
    assert moved(ref) == set()


def test_without_the_early_exit_the_exit_cases_move(ref):
    m = moved(ref, early_exit=False)
    assert m == {"exit_slot0_above_later_below", "exit_slot0_above_later_below_7", "exit_nt1", "lambda0_exit", "dist_u64_max_exit"}


def test_without_strictness_the_tie_cases_move(ref):
    m = moved(ref, strict=False)
    assert {"tie_rate8_dist0_vs_rate0_dist8", "tie_rate0_dist8_vs_rate8_dist0", "tie_slots_0_and_3", "tie_all_equal_16",
            "dist_2p53_plus1_ties_to_even", "dist_2p53_plus1_converted_before_fma"} <= m
    assert not any(n.startswith("exit_") for n in m)


# ---------------------------------------------------------------- R1RdPick as C sees it
def test_rd_pick_layout_equals_the_header_compiled_as_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rav1e_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(R1RdPick));']
    lines += ['  printf("%s %%zu\\n", offsetof(R1RdPick, %s));' % (f, f) for f in RD_PICK.names]
    lines += ['  printf("rules %d %d\\n", R1_PICK_FIRST_MIN, R1_PICK_TX_TYPE);', '  return 0;', '}']
    src, exe = tmp_path / "rd_pick_layout.c", tmp_path / "rd_pick_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == RD_PICK.itemsize == 24
    assert RD_PICK.names == ("best_rd", "best_dist", "best_rate", "best_row", "best_slot", "best_call")
    for f in RD_PICK.names:
        assert int(got[f]) == RD_PICK.fields[f][1], f
    assert [RD_PICK.fields[f][1] for f in RD_PICK.names] == [0, 8, 16, 20, 22, 23]
    from rav1e_amd.types import PICK_FIRST_MIN, PICK_TX_TYPE
    assert got["rules"].split() == [str(PICK_FIRST_MIN), str(PICK_TX_TYPE)] == ["0", "1"]


# ---------------------------------------------------------------- refusals
class _DoublesByBits:
    """the library with every `double` parameter taken as the 64-bit pattern of the value"""

    def __init__(self, lib, symbols):
        self._lib, self._symbols = lib, symbols

    def __getattr__(self, name):
        f, types = getattr(self._lib, name), self._symbols[name][1]
        return lambda *args: f(*[struct.unpack("<d", struct.pack("<Q", a))[0] if t is C.c_double else a
                                 for a, t in zip(args, types)])


class BufPlus:
    """BUF (16-byte aligned, as every allocation of its size is) `off` bytes in: a pointer of a chosen misalignment"""

    def __init__(self, off):
        self.off = off

    def __repr__(self):
        return "BUF+%d" % self.off


class FloatHarness(Harness):
    """the imported harness, whose call() passes integers and pointers: a Python float of the table (lambda) travels
    through it as its bit pattern and becomes a `double` again at the library"""

    def __init__(self):
        super().__init__()
        self.L = _DoublesByBits(self.L, self._lib.SYMBOLS)

    def value(self, v, keep):
        if isinstance(v, BufPlus):
            return C.addressof(self.mem[2]) + v.off
        return struct.unpack("<Q", struct.pack("<d", v))[0] if isinstance(v, float) else super().value(v, keep)


PICK = dict(rate=BUF, rate_add=None, dist=BUF, n_states=0, group=1, nt=7, lambda_=8.0, rule=1, call_id=0, state=BUF,
            invalid_out=None)
COMMIT = dict(state=BUF, n_states=0, call_id=0, group=1, nt=7, ntx=4, order=0, coded_area=64, coeff_bytes=2, eobs=BUF,
              qcoeffs=BUF, side=BUF, side_bytes=32, rec_trials=BUF, bw=16, bh=16, rec=P(2, 10), pos_xy=BUF, store_w=64,
              store_h=64, eob_win=BUF, qcoeffs_win=BUF, win_stride=256, side_win=BUF)
NO_TX = dict(eobs=None, qcoeffs=None, eob_win=None, qcoeffs_win=None)
NO_REC = dict(rec_trials=None, rec=None, pos_xy=None)
TABLE = [
    ("r1_rd_pick_batch", PICK, [
        (dict(), 0),
        (dict(rate_add=BUF, invalid_out=BUF), 0),
        (dict(rule=0, group=4096, nt=1), 0),
        (dict(rule=0, group=256, nt=16), 0),
        (dict(lambda_=0.0), 0),
        (dict(call_id=127), 0),
        (dict(rate=None), -1),
        (dict(dist=None), -1),
        (dict(state=None), -1),
        (dict(n_states=-1), -1),
        (dict(rule=0, group=0), -1),
        (dict(rule=0, group=4097, nt=1), -1),
        (dict(nt=0), -1),
        (dict(nt=17), -1),
        (dict(rule=0, group=257, nt=16), -1),
        (dict(rule=-1), -1),
        (dict(rule=2), -1),
        (dict(rule=1, group=2), -1),
        (dict(call_id=-1), -1),
        (dict(call_id=128), -1),
        (dict(lambda_=-1.0), -1),
        (dict(lambda_=float("inf")), -1),
        (dict(lambda_=float("nan")), -1),
    ]),
    ("r1_rd_commit_batch", COMMIT, [
        (dict(), 0),
        (dict(order=1), 0),
        (dict(coeff_bytes=4, coded_area=1024, ntx=16, win_stride=16384), 0),
        (NO_TX, 0),
        (dict(side=None, side_win=None), 0),
        (NO_REC, 0),
        (dict(NO_TX, **NO_REC), 0),
        (dict(rec=P(1, 8), bw=4, bh=4), 0),
        (dict(bw=64, bh=16, store_w=0, store_h=0), 0),
        (dict(rec_trials=BufPlus(16)), 0),
        (dict(qcoeffs=BufPlus(2), qcoeffs_win=BufPlus(6)), 0),
        (dict(coeff_bytes=4, qcoeffs=BufPlus(4), qcoeffs_win=BufPlus(12)), 0),
        (dict(win_stride=2 ** 31 - 1), 0),
        (dict(rec_trials=BufPlus(1)), -1),
        (dict(rec_trials=BufPlus(8)), -1),
        (dict(qcoeffs=BufPlus(1)), -1),
        (dict(qcoeffs_win=BufPlus(1)), -1),
        (dict(coeff_bytes=4, qcoeffs=BufPlus(2)), -1),
        (dict(coeff_bytes=4, qcoeffs_win=BufPlus(2)), -1),
        (dict(state=None), -1),
        (dict(n_states=-1), -1),
        (dict(call_id=128), -1),
        (dict(group=0), -1),
        (dict(nt=17), -1),
        (dict(eobs=None), -1),
        (dict(qcoeffs=None), -1),
        (dict(eob_win=None), -1),
        (dict(qcoeffs_win=None), -1),
        (dict(side=None), -1),
        (dict(side_win=None), -1),
        (dict(rec_trials=None), -1),
        (dict(rec=None), -1),
        (dict(pos_xy=None), -1),
        (dict(ntx=0), -1),
        (dict(ntx=17), -1),
        (dict(order=2), -1),
        (dict(order=-1), -1),
        (dict(order=1, group=2), -1),
        (dict(coeff_bytes=1), -1),
        (dict(coeff_bytes=8), -1),
        (dict(coded_area=15), -1),
        (dict(coded_area=1025), -1),
        (dict(win_stride=255), -1),
        (dict(side_bytes=0), -1),
        (dict(side_bytes=129), -1),
        (dict(bw=12), -1),
        (dict(bw=128, bh=128), -1),
        (dict(bw=64, bh=8), -1),
        (dict(bw=2, bh=4), -1),
        (dict(rec=P(3, 8)), -1),
        (dict(rec=P(1, 10)), -1),
        (dict(rec=P(2, 8)), -1),
        (dict(rec=P(2, 9)), -1),
        (dict(store_w=65), -1),
        (dict(store_h=65), -1),
        (dict(store_w=-1), -1),
        (dict(store_h=-1), -1),
    ]),
]


@pytest.fixture(scope="module")
def harness():
    return FloatHarness()


def _rows():
    for name, base, cases in TABLE:
        for over, status in cases:
            yield pytest.param(name, base, over, status, id="%s-%s" % (name, fmt(over)[5:-1] or "valid"))


@pytest.mark.parametrize("name,base,over,status", _rows())
def test_status(harness, name, base, over, status):
    assert harness.call(name, base, over) == status

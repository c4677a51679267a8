"""The column family of the forward 1-D networks (rav1e_amd/csrc/fwd_tx_1d_col.inc, tools/gen_tx1d.py fold()) against
the plain networks between their shifts, on the host: for every network and every (K0, S) the column pass meets,

    r1_<net>_col<K0, S>(c)  ==  round_shift(r1_<net>(c << K0), S)

bit for bit.  Both families are compiled with the host compiler from the device tree's generated text, with plain-C
macros for TX_*; the macros of the 24-bit mads (TX_MULK, TX_SHL_SUBR) sign-extend their factor from 24 bits as
v_mad_i32_i24 does, so an input outside that range would show.  Inputs: full-scale columns in every sign pattern a
block of tests/golden/fwd_tx_ref.npz produces (both orientations: the up-down flip is a permutation in front of the
network), columns of -1 / -3 / +1, impulses, and 10^5 random columns of the pixel-residual range."""
import ctypes
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
import fwd_tx_ref_util as U  # noqa: E402

MACROS = r"""
#include <stdint.h>
typedef int32_t T;
#define TX1D_FN static inline
#define I24(a) ((T)((uint32_t)(a) << 8) >> 8)
#define TX_ADD(a, b) ((T)((uint32_t)(a) + (uint32_t)(b)))
#define TX_SUB(a, b) ((T)((uint32_t)(a) - (uint32_t)(b)))
#define TX_MUL(a, m, s) ((T)((uint32_t)(a) * (uint32_t)(m) + (uint32_t)((1 << (s)) >> 1)) >> (s))
#define TX_RSHIFT1(a) (TX_ADD((a), (T)((a) < 0)) >> 1)
#define TX_ADD_AVG(a, b) (TX_ADD(a, b) >> 1)
#define TX_SUB_AVG(a, b) (TX_SUB(a, b) >> 1)
#define TX_MULK(a, m, s, k) ((T)((uint32_t)I24(a) * (uint32_t)(m) + (uint32_t)(1 << ((s) - 1 - (k)))) >> ((s) - (k)))
#define TX_SHL(a, d) ((T)((uint32_t)(a) << (d)))
#define TX_SHL_ADD(a, d, b) ((T)(((uint32_t)(a) << (d)) + (uint32_t)(b)))
#define TX_SHL_SUBR(b, d, a) ((T)((uint32_t)(a) - ((uint32_t)I24(b) << (d))))
#define TX_RND(a, s) (((a) + (1 << ((s) - 1))) >> (s))
#include "fwd_tx_1d.inc"
#undef TX1D_FN
#define TX1D_FN inline   /* an explicit specialization takes no storage class */
#include "fwd_tx_1d_col.inc"
"""

CASE = r"""
    case %(id)d:
      for (long i = 0; i < ncols; i++) {
        T p[%(n)d], q[%(n)d];
        for (int r = 0; r < %(n)d; r++) { q[r] = x[i * %(n)d + r]; p[r] = (T)((uint32_t)q[r] << %(k0)d); }
        r1_%(net)s(p);
        r1_%(net)s_col<%(k0)d, %(s)d>(q);
        for (int r = 0; r < %(n)d; r++) {
          plain[i * %(n)d + r] = %(s)d ? (p[r] + ((1 << %(s)d) >> 1)) >> %(s)d : p[r];
          folded[i * %(n)d + r] = q[r];
        }
      }
      return 0;
"""


def members():
    """[(net, n, K0, S)] of the committed column family, in file order"""
    txt = open(os.path.join(CSRC, "fwd_tx_1d_col.inc")).read()
    lens = {nm: G.F.TXFM_LEN[t] for t, nm in enumerate(G.NAMES) if nm}
    return [(m[0], lens[m[0]], int(m[1]), int(m[2]))
            for m in re.findall(r"template <> TX1D_FN void r1_(\w+)_col<(\d+), (\d+)>", txt)]


MEMBERS = members()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "a host C++ compiler is needed"
    d = tmp_path_factory.mktemp("txcol")
    src = MACROS + 'extern "C" int run(int id, const T *x, T *plain, T *folded, long ncols) {\n  switch (id) {' + \
        "".join(CASE % dict(id=i, net=net, n=n, k0=k0, s=s) for i, (net, n, k0, s) in enumerate(MEMBERS)) + \
        "  }\n  return 1;\n}\n"
    (d / "h.cpp").write_text(src)
    so = str(d / "h.so")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-fwrapv", "-I", CSRC, str(d / "h.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]

    def run(i, cols):
        cols = np.ascontiguousarray(cols, np.int32)
        a, b = np.empty_like(cols), np.empty_like(cols)
        assert lib.run(i, cols.ctypes.data, a.ctypes.data, b.ctypes.data, len(cols)) == 0
        return a, b
    return run


@pytest.fixture(scope="module")
def sign_patterns():
    """{(bit depth, column length): unique +-1 column patterns of the golden blocks, both orientations}"""
    out = {}
    for bd in (8, 10):
        acc = {}
        for case in U.load()[bd]:
            sg = np.where(case.res >= 0, 1, -1).astype(np.int8)          # (nb, h, w)
            cols = sg.transpose(0, 2, 1).reshape(-1, case.h)
            acc.setdefault(case.h, []).append(np.unique(cols, axis=0))
        for h, lst in acc.items():
            u = np.unique(np.concatenate(lst), axis=0)
            out[bd, h] = np.unique(np.concatenate([u, u[:, ::-1]]), axis=0).astype(np.int32)
    return out


def bit_depth(k0):
    return 10 if k0 == 2 else 8     # shift[0] is 3 / 4 at 8 bits, 2 at 10 bits (FWD_TXFM_SHIFT_LS)


def test_family_is_the_generators_and_complete():
    """the committed files are what the generator writes, and the family has every (network, K0, S) the column pass
    dispatches: DCT 4..64, ADST 4 / 8 / 16 (the flip is a permutation), over the 19 sizes at 8 / 10 bits"""
    text, _table = G.col_family()
    assert text == open(os.path.join(CSRC, "fwd_tx_1d_col.inc")).read()
    assert open(os.path.join(CSRC, "fwd_tx_1d.inc")).read() == open(os.path.join(ROOT, "oracle", "fwd_tx_1d.inc")).read()
    pairs = G.col_pairs()
    assert sorted(pairs) == [4, 8, 16, 32, 64]
    want = set()
    for net, n in (("fdct4", 4), ("fdst_vii_4", 4), ("fdct8", 8), ("fdst8", 8), ("fdct16", 16), ("fdst16", 16),
                   ("fdct32", 32), ("fdct64", 64)):
        for k0, s, inmax in pairs[n]:
            assert inmax == (1 << bit_depth(k0)) - 1
            want.add((net, n, k0, s))
    assert set(MEMBERS) == want and len(MEMBERS) == len(want)
    # what fwd_shift_ct yields: 8 bits (3, 0) at 4x4, (4, 1) / (4, 2) elsewhere; 10 bits (2, 0)
    assert set((k0, s) for _, _, k0, s in MEMBERS) == {(3, 0), (4, 1), (4, 2), (2, 0)}


def test_mad_input_bound_not_above_plain():
    """the factor of every 24-bit mad of a folded network is bounded by the plain network's (and by 2^23)"""
    for t, nm in enumerate(G.NAMES):
        if nm is None or nm == "fwht4":
            continue
        n, ops, outs = G.trace_ops(t)
        for k0, s, inmax in G.col_pairs()[n]:
            _lines, _cnt, fold_mad, plain_mad = G.fold(n, ops, outs, k0, s, inmax)
            assert fold_mad <= plain_mad < (1 << 23), (nm, k0, s, fold_mad, plain_mad)


@pytest.mark.parametrize("i", range(len(MEMBERS)), ids=["%s_%d_%d" % (m[0], m[2], m[3]) for m in MEMBERS])
def test_folded_equals_plain(host, sign_patterns, i):
    net, n, k0, s = MEMBERS[i]
    bd = bit_depth(k0)
    mx = (1 << bd) - 1
    rng = np.random.default_rng(1000 + i)
    sets = {
        "full-scale sign patterns": sign_patterns[bd, n] * mx,
        "constant columns": np.array([[-1] * n, [-3] * n, [1] * n, [mx] * n, [-mx] * n], np.int32),
        "impulses": np.concatenate([np.eye(n, dtype=np.int32) * a for a in (1, -1, 3, -3, mx, -mx)]),
        "random": rng.integers(-mx, mx + 1, (100000, n), dtype=np.int32),
        "random small": rng.integers(-4, 5, (20000, n), dtype=np.int32),
    }
    assert len(sets["full-scale sign patterns"]) > 0
    for name, cols in sets.items():
        plain, folded = host(i, cols)
        bad = np.flatnonzero((plain != folded).any(axis=1))
        assert bad.size == 0, (net, k0, s, name, cols[bad[0]].tolist(), plain[bad[0]].tolist(), folded[bad[0]].tolist())

"""The high-word multiply of the fused kernels' forward networks (namespace m24w of rav1e_amd/csrc/tx_common.hpp,
networks rav1e_amd/csrc/fwd_tx_1d_hw.inc):

    (a M + 2^(s-1)) >> s      ==      (a (M << (16 - s)) + 2^15) >> 16        while |a| (M << (16 - s)) + 2^15 < 2^31

on the host.  The identity for every (M, s) the networks hold, at and just past its bound; the generated text itself,
interpreted in NumPy with wrapping int32 arithmetic -- a multiply takes the scaled form exactly where the text's QB
admits the call's bound B -- against the plain networks: every (size, type) the gate names at 8 bits, column pass
(column family on the unshifted residual AND the plain network on residual << shift[0]) then the row pass fed with the
column outputs after shift[1], on random residual blocks and on the full-scale sign patterns of
tests/golden/fwd_tx_ref.npz; every multiply counted against the generator's trace; the largest |a| met at each node
against the bound the generator used; and the header's text and the plan's gate (tests/c/mul_hiword_list.cpp)."""
import os
import re
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
BD = 8
SIZES = {1: 8, 2: 16, 3: 32, 4: 64}          # TxSize id -> side: the instantiations rdo_mul_hiword_built names
CASES = [(ts, tt) for ts in SIZES for tt in range(16) if F.valid_av1_transform(ts, tt)]
SHIPPED = {8: True, 16: True, 32: True, 64: True}   # side -> rdo_mul_hiword (8 bits, QM 0, plain)


# ---- the two forms ----
def mul_old(a, m, s):
    return (a * I32(m) + I32((1 << s) >> 1)) >> I32(s)


def mul_new(a, m, s):
    """what mul_rsw<M, s, true> computes: the mad's 32-bit sum (wrapping), then >> 16"""
    with np.errstate(over="ignore"):
        return (a * I32(m << (16 - s)) + I32(1 << 15)) >> I32(16)


# ---- the generated text, interpreted ----
_STMT = re.compile(r"\s*(?:const T (\w+)|c\[(\d+)\]) = (.*);$")
_CALL = re.compile(r"(TX_\w+)\((.*)\)$")


class Net:
    """one function of fwd_tx_1d_hw.inc: name -> statements (per (K0, S) block for the column form)"""

    def __init__(self, text):
        self.plain, self.col = {}, {}
        for m in re.finditer(r"template <([^>]*)> TX1D_FN void r1_(\w+)\(T \*c\) \{\n(.*?)\n\}\n", text, re.S):
            params, name, body = m.groups()
            if name.endswith("_col"):
                assert params == "int K0, int S, int B"
                for b in re.finditer(r"  if constexpr \(K0 == (\d+) && S == (\d+)\) \{\n(.*?)\n  \}", body, re.S):
                    self.col[name[:-4], int(b.group(1)), int(b.group(2))] = b.group(3).splitlines()
            else:
                assert params == "int B"
                self.plain[name] = [ln for ln in body.splitlines() if not ln.startswith("  const T c0 = c[0]")]


@pytest.fixture(scope="module")
def nets():
    return Net(open(os.path.join(CSRC, "fwd_tx_1d_hw.inc")).read())


def run(stmts, cin, bound, spy):
    """the statements on int32 lanes cin[i]; a multiply marked QB takes the scaled form iff bound <= QB.  spy gets
    (largest |a|, M, shift executed, QB, scaled?) per multiply, in order."""
    v = {"c%d" % i: x for i, x in enumerate(cin)}
    out = {}

    def val(e):
        e = e.strip()
        m = _CALL.match(e)
        if not m:
            return v[e]
        op, a = m.group(1), [x.strip() for x in m.group(2).split(",")]
        if op in ("TX_MULW", "TX_MULKW"):
            x, mul, s = v[a[0]], int(a[1]), int(a[2])
            k = int(a[3]) if op == "TX_MULKW" else 0
            qb = int(a[-1])
            hw = bound <= qb
            spy.append((int(np.abs(x.astype(np.int64)).max()), mul, s - k, qb, hw))
            if hw:
                return mul_new(x, mul, s - k)
            return (x * I32(mul) + I32(1 << (s - 1 - k))) >> I32(s - k)       # mul_rs / mul_rk
        if op == "TX_ADD":
            return v[a[0]] + v[a[1]]
        if op == "TX_SUB":
            return v[a[0]] - v[a[1]]
        if op in ("TX_RSHIFT1", "TX_RSHIFT1W"):
            return (v[a[0]] - (v[a[0]] >> I32(24))) >> I32(1)               # m24h's halving, which m24w keeps
        if op == "TX_ADD_AVG":
            return (v[a[0]] + v[a[1]]) >> I32(1)
        if op == "TX_SUB_AVG":
            return (v[a[0]] - v[a[1]]) >> I32(1)
        if op == "TX_SHL":
            return v[a[0]] << I32(int(a[1]))
        if op == "TX_SHL_ADD":
            return (v[a[0]] << I32(int(a[1]))) + v[a[2]]
        if op == "TX_SHL_SUBR":                                              # a - (b << d)
            return v[a[2]] - (v[a[0]] << I32(int(a[1])))
        if op in ("TX_RND", "TX_RNDW"):
            return (v[a[0]] + I32(1 << (int(a[1]) - 1))) >> I32(int(a[1]))
        raise ValueError(e)

    for ln in stmts:
        m = _STMT.match(ln)
        assert m, ln
        if m.group(1):
            v[m.group(1)] = val(m.group(3))
        else:
            out[int(m.group(2))] = val(m.group(3))
    return [out[i] for i in range(len(cin))]


def rshift(c, s):
    return (c + I32((1 << s) >> 1)) >> I32(s) if s > 0 else c << I32(-s)


def chain(nets, res, ts, tt, family, cb, rb):
    """forward_transform (oracle/fwd_tx_np.py) with both passes on the interpreted text.  family "colk": the column
    form on the unshifted residual; "col": shift[0], the plain form, shift[1].  -> (coefficients, column spy, row spy,
    largest |row input|)"""
    w, h = F.TX_DIMS[ts]
    res = np.asarray(res).astype(I32).reshape((-1, h, w))
    n = res.shape[0]
    tcol = F.TXFM_TYPE_LS[h.bit_length() - 3][F.VTX_TAB[tt]]
    trow = F.TXFM_TYPE_LS[w.bit_length() - 3][F.HTX_TAB[tt]]
    sh = [int(x) for x in F.FWD_SHIFT[ts][(BD - 8) // 2]]
    src = res[:, ::-1, :] if tt in F.UD_FLIP else res
    cols = [np.ascontiguousarray(src[:, r, :]).reshape(-1) for r in range(h)]
    cspy, rspy = [], []
    if G.NAMES[tcol] is None:                   # the identity: shift[0] then shift[1] (shift_col_ident)
        cols = [rshift(c << I32(sh[0]), -sh[1]) for c in cols]
    elif family == "colk":
        cols = run(nets.col[G.NAMES[tcol], sh[0], -sh[1]], cols, cb, cspy)
    else:
        cols = [rshift(c, -sh[1]) for c in run(nets.plain[G.NAMES[tcol]], [c << I32(sh[0]) for c in cols], cb, cspy)]
    buf = np.stack([c.reshape(n, w) for c in cols], axis=1)
    if tt in F.LR_FLIP:
        buf = buf[:, :, ::-1]
    rin = int(np.abs(buf).max())
    rows = [np.ascontiguousarray(buf[:, :, c]).reshape(-1) for c in range(w)]
    if G.NAMES[trow] is not None:
        rows = run(nets.plain[G.NAMES[trow]], rows, rb, rspy)
    rows = [rshift(c, -sh[2]) for c in rows]
    out2d = np.stack([c.reshape(n, h) for c in rows], axis=2)
    out = np.zeros((n, w * h), dtype=I32)
    ostride = min(h, 32)
    for r in range(h):
        base = (r >= 32) * ostride * min(w, 32)
        for cg in range(0, w, 32):
            for c in range(min(w, 32)):
                out[:, base + h * cg + c * ostride + (r & 31)] = out2d[:, r, c + cg]
    return out, cspy, rspy, rin


# ---- what the plan says ----
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mul_hiword") / "mul_hiword_list")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "c", "mul_hiword_list.cpp")])
    keys = ("bd", "wl", "hl", "qm", "mt", "ps", "built", "on", "halve2", "col_fold", "cb", "rb")
    return [dict(zip(keys, (int(x) for x in ln.split()))) for ln in subprocess.check_output([exe], text=True).splitlines()]


def row_of(plan, n):
    (r,) = [p for p in plan if 1 << p["wl"] == n]
    return r


def test_plan_names_only_what_is_covered(plan):
    """built: the 8-bit coefficient kernels (QM 0, no type search, no intra source) of the four square sizes, all on
    m24h's halving; on: a subset of them; the bounds the passes hand over are tools/tx_range.py's"""
    assert sorted((p["bd"], 1 << p["wl"]) for p in plan if p["built"]) == [(BD, n) for n in sorted(SIZES.values())]
    for p in plan:
        assert p["built"] and p["halve2"] and (p["qm"], p["mt"], p["ps"]) == (0, 0, 0) and p["wl"] == p["hl"], p
        assert bool(p["on"]) == SHIPPED[1 << p["wl"]], p
        ts = p["wl"] - 2
        types = [tt for tt in range(16) if F.valid_av1_transform(ts, tt)]
        b0 = set(R.chain_input_bounds(BD, ts, tt)[0] for tt in types)
        assert b0 == {255 << 4}
        assert p["cb"] == (255 if p["col_fold"] else 255 << 4)
        assert p["rb"] == max(R.chain_input_bounds(BD, ts, tt)[1] for tt in types), p
    assert [row_of(plan, n)["rb"] for n in (8, 16, 32, 64)] == [5774, 8164, 5776, 16334]


def test_file_is_what_the_generator_emits(nets):
    text, marks = G.hiword_family()
    assert text == open(os.path.join(CSRC, "fwd_tx_1d_hw.inc")).read()
    # the text carries the generator's QB at every multiply, in trace order, and nothing but marked multiplies
    assert not re.search(r"TX_MULK?\(", text)
    for (nm, k0, s), qbs in marks.items():
        stmts = nets.plain[nm] if k0 is None else nets.col[nm, k0, s]
        got = [int(m.group(1)) for ln in stmts for m in [re.search(r"TX_MULK?W\(.*, (\d+)\);$", ln)] if m]
        assert got == qbs, (nm, k0, s)
    assert set(nm for nm, _k, _s in marks) == set(G.HW_NAMES)
    # the other two families are still the generator's text, byte for byte
    assert G.col_family()[0] == open(os.path.join(CSRC, "fwd_tx_1d_col.inc")).read()


def pairs_that_occur():
    """{(M, shift executed)} over every multiply of both families"""
    res = set()
    for t, nm in enumerate(G.NAMES):
        if nm not in G.HW_NAMES:
            continue
        res.update((m, s) for _n, _b, m, s, _l, _e, _k in G.mul_nodes(t, 0))
        for k0, _s, inmax in G.col_pairs()[F.TXFM_LEN[t]]:
            res.update((m, s) for _n, _b, m, s, _l, _e, _k in G.mul_nodes(t, inmax, k0))
    return sorted(res)


def test_identity_at_and_past_its_bound():
    """for every (M, s): equal on [-amax, amax], amax the largest |a| with |a| Ms + 2^15 < 2^31; at amax + 1 the sum
    reaches 2^31, wraps negative, and the forms differ -- the bound is the condition, not a margin.  A pair whose
    scaled multiplier is no 24-bit operand never qualifies."""
    rng = np.random.default_rng(16)
    prs = pairs_that_occur()
    assert len(prs) > 100 and all(1 <= s <= 16 and m > 0 for m, s in prs)
    wide = 0
    for m, s in prs:
        ms = m << (16 - s)
        if ms >= 1 << 23:
            assert not G.hiword_ok(0, m, s)
            wide += 1
            continue
        amax = ((1 << 31) - (1 << 15) - 1) // ms
        assert G.hiword_ok(amax, m, s) and not G.hiword_ok(amax + 1, m, s)
        a = np.concatenate([rng.integers(-amax, amax + 1, 1 << 14), np.array([0, 1, -1, amax, amax - 1, -amax, 1 - amax]),
                            rng.integers(-300, 301, 1 << 10)]).astype(I32)
        assert np.array_equal(mul_old(a, m, s), mul_new(a, m, s)), (m, s)
        past = np.array([amax + 1], I32)
        assert mul_new(past, m, s)[0] < 0 < mul_old(past, m, s)[0], (m, s)
    assert wide == 0 or wide < len(prs)


def test_qb_is_where_a_node_stops_qualifying():
    """QB of every multiply: at B = QB the node's bound (L1 gain, rounding, pending scale) qualifies, at QB + 1 it does
    not; and at the bounds the plan passes, the nodes that take the form are those tools/tx_range.py mul_bounds()
    admits"""
    import math
    _text, marks = G.hiword_family()
    for t, nm in enumerate(G.NAMES):
        if nm not in G.HW_NAMES:
            continue
        fams = [(None, None, 0)] + [(k0, s, k0) for k0, s, _m in G.col_pairs()[F.TXFM_LEN[t]]]
        for k0, s, sh in fams:
            for (_n, _b, m, se, l1, e, ka), qb in zip(G.mul_nodes(t, 0, k0), marks[nm, k0, s]):
                def bound(b):
                    return int(math.ceil((b << sh) * l1 + e)) >> ka
                assert qb == 0 or G.hiword_ok(bound(qb), m, se)
                assert qb >= 1 << 24 or not G.hiword_ok(bound(qb + 1), m, se)
    mb = R.mul_bounds()
    took = {}
    for ts, tt in CASES:
        for ps in ("col", "colk", "row"):
            took[SIZES[ts], tt, ps] = (sum(G.hiword_ok(*x) for x in mb[BD, ts, tt, ps]), len(mb[BD, ts, tt, ps]))
    # DCT_DCT: the counts rdo_cand_plan.hpp quotes
    assert [took[n, 0, "colk"] for n in (8, 16, 32)] == [(13, 13), (31, 31), (81, 81)]
    assert took[64, 0, "col"] == (167, 191)
    assert [took[n, 0, "row"] for n in (8, 16, 32, 64)] == [(13, 13), (27, 31), (70, 81), (87, 191)]
    assert took[16, 3, "row"] == (42, 48) and took[8, 3, "row"] == (20, 20)


@pytest.fixture(scope="module")
def golden():
    return {(c.ts, c.tt): c for c in U.load()[BD]}


@pytest.mark.parametrize("ts,tt", CASES, ids=["%dx%d_t%d" % (SIZES[c[0]], SIZES[c[0]], c[1]) for c in CASES])
def test_networks_agree_with_the_scaled_products(nets, plan, golden, ts, tt):
    n = SIZES[ts]
    mx = (1 << BD) - 1
    p = row_of(plan, n)
    rng = np.random.default_rng(1600 + 16 * ts + tt)
    nb = -(-50000 // n)
    case = golden[ts, tt]
    sg = np.where(case.res >= 0, 1, -1).astype(np.int16)
    sets = {"random": rng.integers(-mx, mx + 1, (nb, n, n)).astype(np.int16),
            "random small": rng.integers(-3, 4, (64, n, n)).astype(np.int16),
            "full-scale sign patterns": np.concatenate([sg * mx, -sg * mx, sg.transpose(0, 2, 1) * mx]),
            "golden": case.res}
    sh0 = int(F.FWD_SHIFT[ts][0][0])
    tcol = F.TXFM_TYPE_LS[n.bit_length() - 3][F.VTX_TAB[tt]]
    trow = F.TXFM_TYPE_LS[n.bit_length() - 3][F.HTX_TAB[tt]]
    # (family, the bound its column pass is called with): the one the kernel runs first, then the other
    fams = {"colk": mx, "col": mx << sh0}
    assert p["cb"] == fams["colk" if p["col_fold"] else "col"]
    rb = p["rb"]
    scaled = 0
    for fam, cb in fams.items():
        if G.NAMES[tcol] is None:
            want_c = []
        else:
            want_c = G.mul_nodes(tcol, mx, sh0) if fam == "colk" else G.mul_nodes(tcol, mx << sh0)
        want_r = G.mul_nodes(trow, rb) if G.NAMES[trow] else []
        for name, res in sets.items():
            got, cspy, rspy, rin = chain(nets, res, ts, tt, fam, cb, rb)
            assert np.array_equal(got, F.forward_transform(res, ts, tt, BD)), (name, fam, ts, tt)
            assert rin <= rb, (name, rin, rb)                   # the row bound is a bound
            # every multiply of both networks went through the interpreter's marked form, none more, none less
            assert len(cspy) == len(want_c) and len(rspy) == len(want_r), (name, fam)
            for spy, want in ((cspy, want_c), (rspy, want_r)):
                for (amax, m, s, qb, hw), (_nm, b, wm, ws, _l, _e, _k) in zip(spy, want):
                    assert (m, s) == (wm, ws)
                    assert amax <= b, (name, fam, amax, b)     # the generator's bound of the node is a bound
                    assert hw == G.hiword_ok(b, m, s), (name, fam, m, s, b, qb)
                    if hw:
                        assert b * (m << (16 - s)) + (1 << 15) < 1 << 31 and (m << (16 - s)) < 1 << 23
                        scaled += 1
        got, _c, _r, _i = chain(nets, case.res, ts, tt, fam, cb, rb)
        assert np.array_equal(got.astype(case.coef.dtype), case.coef)      # reference-executed coefficients
    if tt != 9:
        assert scaled > 0


def test_a_bound_too_small_breaks_the_networks(nets):
    """the interpreter models the wrap: called with B far below the real input bound, nodes take the form that
    must not, and full-scale input no longer gives the plain network's outputs"""
    rng = np.random.default_rng(7)
    x = [rng.integers(-16334, 16335, 4096).astype(I32) for _ in range(64)]
    want = F.TXFM_FUNCS[4]([c.copy() for c in x])
    assert all(np.array_equal(a, b) for a, b in zip(run(nets.plain["fdct64"], x, 16334, []), want))
    assert not all(np.array_equal(a, b) for a, b in zip(run(nets.plain["fdct64"], x, 1, []), want))


def test_header_compiles_the_form_tested_here():
    txt = open(os.path.join(CSRC, "tx_common.hpp")).read()
    body = txt[txt.index("namespace m24w {"):txt.index("}  // namespace m24w")]
    assert body.count('#include "fwd_tx_1d_hw.inc"') == 1 and "#include" not in body.replace('#include "fwd_tx_1d_hw.inc"', "")
    assert '"s"(M * (1 << (16 - S))), "v"(1 << 15));\n    return r >> 16;' in body
    assert "return mul_rs<M, S>(a);" in body and "else return mul_rk<M, S, K>(a);" in body
    assert "if constexpr (HW) return mul_rsw<M, S - K, true>(a);" in body
    assert "#define TX_MULW(a, m, s, qb) (mul_rsw<(m), (s), (B <= (qb))>(a))" in body
    assert "#define TX_MULKW(a, m, s, k, qb) (mul_rkw<(m), (s), (k), (B <= (qb))>(a))" in body
    m = re.findall(r"#define TX_RSHIFT1\(a\) (.*)", body)
    assert m == ["(TX_SUB((a), (a) >> 24) >> 1)", "(TX_ADD((a), (T)((a) < 0)) >> 1)"]
    assert "return TX_SUB(a, a >> 24) >> 1;" in body and "return (a + (1 << (S - 1))) >> S;" in body
    # no SDWA and no sub-dword destination by hand: the selects are the compiler's
    assert "sdwa" not in "".join(re.findall(r'asm\((.*?)\);', body, re.S))
    assert "dst_sel" not in body
    kern = open(os.path.join(CSRC, "rdo_cand_kernel.hpp")).read()
    assert kern.count("_m24w") == 6         # phases C (column family, plain) and D, scalar and per-lane arm each

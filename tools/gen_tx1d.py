#!/usr/bin/env python3
"""Emit the forward 1-D transform networks as straight-line SSA C.

Source of truth: oracle/fwd_tx_np.py (our restatement of
src/transform/forward_shared.rs:398-1796, pinned bit-exact by
tests/golden/fwd_tx_golden.npz).  Each network is traced once with symbolic
lanes; every primitive op (TX_MUL / TX_ADD / TX_SUB / TX_RSHIFT1 /
TX_ADD_AVG / TX_SUB_AVG) becomes one `const T tN = ...;` statement, dead
values (unused half outputs) are dropped.  The including file defines `T`,
`TX1D_FN` (function qualifiers) and the TX_* macros, so the same text serves

  oracle/fwd_tx_1d.inc              (plain C, host oracle / CPU baseline)
  rav1e_amd/csrc/fwd_tx_1d.inc      (HIP device code, register arrays)

The two files are written separately so that the product tree never includes
anything under oracle/.

A second family, rav1e_amd/csrc/fwd_tx_1d_col.inc, serves the COLUMN pass of
the fused kernels: `r1_<net>_col<K0, S>(T *c)` takes the residuals unshifted
and returns the outputs after the rounding shift by S, i.e. it computes

  c[i] = round_shift(r1_<net>(c[] << K0)[i], S)

bit for bit, with the left shift never executed: every SSA value is carried as
(reg, k), value = reg * 2^k (fold(), below).
"""
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fwd_tx_np as F  # noqa: E402

NAMES = ["fdct4", "fdct8", "fdct16", "fdct32", "fdct64", "fdst_vii_4", "fdst8",
         "fdst16", None, None, None, None, "fwht4"]


def trace_ops(t):
    """-> (n, [(name, expr)] live statements in order, [output names])"""
    n = F.TXFM_LEN[t]
    tape = []
    ins = [F.Sym("c%d" % i, tape) for i in range(n)]
    outs = F.TXFM_FUNCS[t](ins)
    # dead-code elimination
    live = set(o.name for o in outs)
    for name, expr in reversed(tape):
        if name in live:
            for tok in re.findall(r"\b[ct]\d+\b", expr):
                live.add(tok)
    return n, [(name, expr) for name, expr in tape if name in live], [o.name for o in outs]


def trace(t):
    n, ops, outs = trace_ops(t)
    lines = ["TX1D_FN void r1_%s(T *c) {" % NAMES[t]]
    lines.append("  const T " + ", ".join("c%d = c[%d]" % (i, i) for i in range(n)) + ";")
    for name, expr in ops:
        lines.append("  const T %s = %s;" % (name, expr))
    for i, o in enumerate(outs):
        lines.append("  c[%d] = %s;" % (i, o))
    lines.append("}")
    return "\n".join(lines), len(ops)


# ---- the column family: pending power-of-two scales ----
# The column pass of the fused kernels feeds a network with residual << K0 (K0 = shift[0] of
# FWD_TXFM_SHIFT_LS) and rounds its outputs by S = -shift[1].  The networks then spend their first levels halving
# multiples of 2^k with TX_RSHIFT1, whose sign correction does nothing on an even number.  fold() carries every SSA
# value as (reg, k) with value = reg * 2^k exactly:
#   input                          (residual, K0): no shift
#   ADD / SUB, equal k             the op on the regs
#   ADD, unequal k                 (ra << d) + rb                                  TX_SHL_ADD  (v_lshl_add_u32)
#   SUB, larger k on subtrahend    ra - (rb << d)                                  TX_SHL_SUBR (v_mad_i32_i24 by -2^d)
#   SUB, larger k on minuend       TX_SHL, then TX_SUB
#   RSHIFT1, k >= 1                (reg, k - 1): nothing
#   ADD_AVG / SUB_AVG, k >= 1      the add / sub alone, result at k - 1
#   MUL(a, M, S), k <= S - 1       (reg * M + 2^(S-1-k)) >> (S - k), result at k = 0   TX_MULK
#                                  [floor((X 2^k + 2^(S-1)) / 2^S) = floor((X + 2^(S-1-k)) / 2^(S-k))]
#   output, k >= S                 reg << (k - S): the rounding term cannot carry
#   output, k < S                  (reg + 2^(S-1-k)) >> (S - k)                    TX_RND (same identity)
# A value that several consumers want at one lower k is shifted there once (a copy `<name>_k<k'>`) when that is
# cheaper than the sum of their alignment costs at the issue prices below.
FAST, SLOW = 2.5, 4.5   # cycles per wave instruction: add / sub / compare / arithmetic shift right; left shift,
                        # shift-add and 24-bit mad (tools/ubench/valu_rate*.hip)
_OP = re.compile(r"TX_(\w+)\((.*)\)$")


def _parse(expr):
    m = _OP.match(expr)
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def value_gains(n, ops):
    """{SSA name of the PLAIN network: (L1 norm of the value's response to the inputs, accumulated rounding error)}:
    the networks are linear up to rounding, so |value| <= |input| bound * L1 + error"""
    vec = {"c%d" % i: [float(j == i) for j in range(n)] for i in range(n)}
    err = {"c%d" % i: 0.0 for i in range(n)}
    for name, expr in ops:
        op, a = _parse(expr)
        if op in ("ADD", "SUB", "ADD_AVG", "SUB_AVG"):
            sg = 1.0 if op.startswith("ADD") else -1.0
            h = 0.5 if op.endswith("AVG") else 1.0
            vec[name] = [(x + sg * y) * h for x, y in zip(vec[a[0]], vec[a[1]])]
            err[name] = (err[a[0]] + err[a[1]]) * h + (0.5 if h < 1 else 0.0)
        elif op == "RSHIFT1":
            vec[name] = [x * 0.5 for x in vec[a[0]]]
            err[name] = err[a[0]] * 0.5 + 0.5
        elif op == "MUL":
            g = int(a[1]) / float(1 << int(a[2]))
            vec[name] = [x * g for x in vec[a[0]]]
            err[name] = err[a[0]] * abs(g) + 0.5
        else:
            raise ValueError(expr)
    return {k: (sum(abs(x) for x in v), err[k]) for k, v in vec.items()}


def value_bounds(n, ops, inmax):
    """|value| bound of every SSA name of the PLAIN network fed with |input| <= inmax: inmax * L1 norm of the value's
    response to the inputs (the networks are linear up to rounding) + the accumulated rounding error."""
    return {k: int(math.ceil(inmax * l1 + e)) for k, (l1, e) in value_gains(n, ops).items()}


def halving_bound(n, ops, outs, inmax):
    """(largest |operand| of a TX_RSHIFT1, largest |output|) of the network fed with |input| <= inmax.  The column
    family executes a halving only on a value with no pending scale (k = 0), whose register IS the plain network's
    value when that is fed with inmax << K0: the bound of the plain network covers both."""
    vb = value_bounds(n, ops, inmax)
    hs = [vb[a[0]] for op, a in (_parse(expr) for _, expr in ops) if op == "RSHIFT1"]
    return (max(hs) if hs else 0), max(vb[o] for o in outs)


# (a - (a >> 24)) >> 1, the halving of m24h (csrc/tx_common.hpp), is TX_RSHIFT1 while a >> 24 is the sign
HALVE2_LIMIT = 1 << 24


def plain_counts(n, ops, k0, s):
    """(fast, slow) instructions of shift[0], the plain network and shift[1]"""
    fast, slow = (2 * n if s > 0 else 0), (n if k0 > 0 else 0)
    for _, expr in ops:
        op, _a = _parse(expr)
        if op in ("ADD", "SUB"):
            fast += 1
        elif op == "RSHIFT1":
            fast += 3
        elif op in ("ADD_AVG", "SUB_AVG"):
            fast += 2
        else:
            fast += 1
            slow += 1
    return fast, slow


def pending_scales(n, parsed, k0):
    """pass 1 of fold(): the pending scale k of every value, value = reg * 2^k (independent of how operands get
    aligned)"""
    k = {"c%d" % i: k0 for i in range(n)}
    for name, op, a in parsed:
        if op in ("ADD", "SUB"):
            k[name] = min(k[a[0]], k[a[1]])
        elif op == "RSHIFT1":
            k[name] = max(k[a[0]] - 1, 0)
        elif op in ("ADD_AVG", "SUB_AVG"):
            k[name] = max(min(k[a[0]], k[a[1]]) - 1, 0)
        else:
            assert k[a[0]] <= int(a[2]) - 1, (name, a)
            k[name] = 0
    return k


def fold(n, ops, outs, k0, s, inmax):
    """-> (body lines, (fast, slow), mad-input bound folded, mad-input bound plain)"""
    vb = value_bounds(n, ops, inmax << k0)
    parsed = [(name,) + tuple(_parse(expr)) for name, expr in ops]
    plain_mad = max(vb[a[0]] for _, op, a in parsed if op == "MUL")
    k = pending_scales(n, parsed, k0)

    def mad_ok(b):   # may `b` be the 24-bit factor of a v_mad_i32_i24?
        return (vb[b] >> k[b]) <= plain_mad

    # pass 2: what aligning the higher-k operand costs each consumer beyond the aligned op; shift once where cheaper
    want = {}   # (name, k') -> summed extra cost
    for name, op, a in parsed:
        if op == "MUL" or op == "RSHIFT1":
            continue
        ka, kb = k[a[0]], k[a[1]]
        if ka == kb:
            continue
        m = min(ka, kb)
        hi = a[0] if ka > kb else a[1]
        if op.endswith("AVG") and m == 0:
            extra = SLOW                      # materialise, then the plain average
        elif op.startswith("ADD"):
            extra = SLOW - FAST               # shift-add for add
        elif hi == a[1] and mad_ok(hi):
            extra = SLOW - FAST               # mad for sub
        else:
            extra = SLOW                      # shift, then sub
        want[(hi, m)] = want.get((hi, m), 0.0) + extra
    copies = set(key for key, cost in want.items() if cost > SLOW)

    lines, fast, slow = [], 0, 0
    fold_mad = 0
    made = set()

    def at(name, kk):
        """the operand `name` brought to scale kk by a shared copy, or None"""
        nonlocal slow
        if (name, kk) not in copies:
            return None
        cp = "%s_k%d" % (name, kk)
        if cp not in made:
            made.add(cp)
            lines.append("  const T %s = TX_SHL(%s, %d);" % (cp, name, k[name] - kk))
            slow += 1
        return cp

    for name, op, a in parsed:
        if op == "MUL":
            ka = k[a[0]]
            fold_mad = max(fold_mad, vb[a[0]] >> ka)
            if ka == 0:
                e = "TX_MUL(%s, %s, %s)" % (a[0], a[1], a[2])
            else:
                e = "TX_MULK(%s, %s, %s, %d)" % (a[0], a[1], a[2], ka)
            fast += 1
            slow += 1
        elif op == "RSHIFT1":
            if k[a[0]] >= 1:
                e = a[0]                      # (reg, k - 1)
            else:
                e = "TX_RSHIFT1(%s)" % a[0]
                fast += 3
        else:
            ka, kb = k[a[0]], k[a[1]]
            m = min(ka, kb)
            avg = op.endswith("AVG")
            base = op[:3]
            x, y = a[0], a[1]
            if ka != kb:
                hi = x if ka > kb else y
                cp = at(hi, m)
                if cp is not None:
                    x, y = (cp, y) if hi == x else (x, cp)
                    ka = kb = m
            if ka == kb:
                if avg and m == 0:
                    e = "TX_%s_AVG(%s, %s)" % (base, x, y)
                    fast += 2
                else:
                    e = "TX_%s(%s, %s)" % (base, x, y)
                    fast += 1
            else:
                d = abs(ka - kb)
                if avg and m == 0:
                    lines.append("  const T %s_m = TX_SHL(%s, %d);" % (name, hi, d))
                    slow += 1
                    x, y = ("%s_m" % name, y) if hi == x else (x, "%s_m" % name)
                    e = "TX_%s_AVG(%s, %s)" % (base, x, y)
                    fast += 2
                elif base == "ADD":
                    lo = y if hi == x else x
                    e = "TX_SHL_ADD(%s, %d, %s)" % (hi, d, lo)
                    slow += 1
                elif hi == y and mad_ok(hi):
                    fold_mad = max(fold_mad, vb[hi] >> k[hi])
                    e = "TX_SHL_SUBR(%s, %d, %s)" % (hi, d, x)
                    slow += 1
                else:
                    lines.append("  const T %s_m = TX_SHL(%s, %d);" % (name, hi, d))
                    slow += 1
                    x, y = ("%s_m" % name, y) if hi == x else (x, "%s_m" % name)
                    e = "TX_SUB(%s, %s)" % (x, y)
                    fast += 1
        lines.append("  const T %s = %s;" % (name, e))
    for i, o in enumerate(outs):
        ko = k[o]
        if ko > s:
            e = "TX_SHL(%s, %d)" % (o, ko - s)
            slow += 1
        elif ko == s:
            e = o
        else:
            e = "TX_RND(%s, %d)" % (o, s - ko)
            fast += 2
        lines.append("  c[%d] = %s;" % (i, e))
    return lines, (fast, slow), fold_mad, plain_mad


def col_pairs():
    """{column length: sorted (K0, S, input bound) the column pass meets}: shift[0] and -shift[1] of FWD_TXFM_SHIFT_LS
    over the 19 sizes at 8 / 10 / 12 bits.  K0 = 0 (12 bits) keeps the plain network and has no member here."""
    res = {}
    for ts, (_w, h) in enumerate(F.TX_DIMS):
        for bi, bd in enumerate((8, 10, 12)):
            sh = F.FWD_SHIFT[ts][bi]
            if sh[0] > 0:
                res.setdefault(h, set()).add((int(sh[0]), int(-sh[1]), (1 << bd) - 1))
    return {h: sorted(v) for h, v in res.items()}


def col_family():
    """-> (text of fwd_tx_1d_col.inc, count table lines)"""
    pairs = col_pairs()
    body, table = [], []
    table.append("network K0 S | plain fast/slow | folded fast/slow | instructions | cycles | mad input plain/folded")
    for t, nm in enumerate(NAMES):
        if nm is None or nm == "fwht4":
            continue
        n, ops, outs = trace_ops(t)
        body.append("template <int K0, int S> TX1D_FN void r1_%s_col(T *c);" % nm)
        for k0, s, inmax in pairs[n]:
            lines, (ff, fs), fm, pm = fold(n, ops, outs, k0, s, inmax)
            pf, ps = plain_counts(n, ops, k0, s)
            assert fm <= pm and pm < (1 << 23), (nm, k0, s, fm, pm)
            hb, _ = halving_bound(n, ops, outs, inmax << k0)
            assert hb < HALVE2_LIMIT, (nm, k0, s, hb)
            body.append("template <> TX1D_FN void r1_%s_col<%d, %d>(T *c) {\n" % (nm, k0, s) +
                        "  const T " + ", ".join("c%d = c[%d]" % (i, i) for i in range(n)) + ";\n" +
                        "\n".join(lines) + "\n}")
            table.append("%s %d %d | %d/%d | %d/%d | %+.1f%% | %+.1f%% | %d/%d" % (
                nm, k0, s, pf, ps, ff, fs, 100.0 * (ff + fs - pf - ps) / (pf + ps),
                100.0 * (ff * FAST + fs * SLOW - pf * FAST - ps * SLOW) / (pf * FAST + ps * SLOW), pm, fm))
    hdr = ("/* GENERATED by tools/gen_tx1d.py from oracle/fwd_tx_np.py -- do not edit.\n"
           " * Column-pass family of the forward 1-D networks: r1_<net>_col<K0, S>(c) computes\n"
           " * round_shift(r1_<net>(c << K0), S) bit for bit on unshifted inputs, every SSA value carried\n"
           " * as (reg, k), value = reg * 2^k (tools/gen_tx1d.py, fold()).  Instructions at 2.5 (fast) / 4.5 (slow)\n"
           " * cycles, shift[0] and shift[1] included; `mad input` is the bound of the 24-bit multiply's factor:\n"
           " * " + "\n * ".join(table) + " */\n")
    return hdr + "\n\n".join(body) + "\n", table


# ---- the high-word family: products kept at scale 2^16 ----
#   (a M + 2^(s-1)) >> s  ==  (a (M << (16 - s)) + 2^15) >> 16        s <= 16
# exact while the scaled product plus 2^15 fits an i32 and M << (16 - s) stays a 24-bit operand; s is the shift the
# multiply EXECUTES (S of the plain family, S - k of the column family).  With the value stated as P >> 16 a consumer
# `x +- (P >> 16)` is one add / sub that reads the product's high word (src_sel:WORD_1, sign-extended): the shift of a
# product that only feeds adds and subs is never executed.  fwd_tx_1d_hw.inc states every multiply of the networks of
# 8 points and more, both families, as TX_MULW(a, M, S, QB) / TX_MULKW(a, M, S, k, QB): QB is the largest bound of the
# network's INPUTS (the unshifted residual for the column family) at which the node still qualifies, and the
# functions take the bound of the call, B, as a template parameter -- a node is scaled where B <= QB and is the
# plain family's mul_rs / mul_rk otherwise (csrc/tx_common.hpp, m24w).
HIWORD = 16
HW_NAMES = ("fdct8", "fdct16", "fdct32", "fdct64", "fdst8", "fdst16")
_GAINS = {}


def net(t):
    """(n, ops, outs, gains) of network t, traced once"""
    if t not in _GAINS:
        n, ops, outs = trace_ops(t)
        _GAINS[t] = (n, ops, outs, value_gains(n, ops))
    return _GAINS[t]


def hiword_ok(bound, m, s):
    """may a multiply by m, rounding shift s, whose factor is bounded by `bound`, keep its product at scale 2^16?"""
    if s < 1 or s > HIWORD:
        return False
    ms = abs(m) << (HIWORD - s)
    return ms < (1 << 23) and bound * ms + (1 << 15) < (1 << 31)


def mul_nodes(t, inmax, k0=None):
    """[(name, |factor| bound, M, shift executed, L1 gain, rounding error, k)] for every live multiply of network t in
    trace order, inputs bounded by inmax.  k0 None: the plain family.  Otherwise the column family on unshifted
    inputs at pending scale k0: the factor is the register, plain value >> k, and the shift executed is S - k."""
    n, ops, _outs, gains = net(t)
    parsed = [(name,) + tuple(_parse(expr)) for name, expr in ops]
    k = pending_scales(n, parsed, k0) if k0 is not None else None
    res = []
    for name, op, a in parsed:
        if op != "MUL":
            continue
        l1, e = gains[a[0]]
        ka = k[a[0]] if k is not None else 0
        b = int(math.ceil((inmax << (k0 or 0)) * l1 + e)) >> ka
        res.append((name, b, int(a[1]), int(a[2]) - ka, l1, e, ka))
    return res


def hiword_qb(l1, e, m, s, k0, ka):
    """the largest input bound at which the node qualifies (0: never)"""
    def ok(b):
        return hiword_ok(int(math.ceil((b << k0) * l1 + e)) >> ka, m, s)
    lo, hi = 0, 1 << 24          # ok(lo) or lo == 0; not ok(hi) unless capped
    if ok(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


def _halve_w(text, prods):
    """a halving whose operand is a product is stated as TX_RSHIFT1W: its operand is materialised (see m24w)"""
    m = re.search(r"TX_RSHIFT1\((\w+)\)", text)
    return text.replace("TX_RSHIFT1(", "TX_RSHIFT1W(") if m and m.group(1) in prods else text


def _rnd_w(text, prods, defs):
    """an output (x +- y + 1) >> 1 of two products is stated as TX_RNDW: its operand is materialised (see m24w)"""
    m = re.match(r"  c\[\d+\] = TX_RND\((\w+), 1\);$", text)
    if m:
        d = re.match(r"  const T \w+ = TX_(ADD|SUB)\((\w+), (\w+)\);$", defs.get(m.group(1), ""))
        if d and d.group(2) in prods and d.group(3) in prods:
            return text.replace("TX_RND(", "TX_RNDW(")
    return text


def hiword_family():
    """-> (text of fwd_tx_1d_hw.inc, {(name, k0, s): [QB per multiply in trace order]}); k0 = s = None: plain"""
    pairs = col_pairs()
    body, marks = [], {}
    for t, nm in enumerate(NAMES):
        if nm not in HW_NAMES:
            continue
        n, ops, outs, _g = net(t)
        ins = "  const T " + ", ".join("c%d = c[%d]" % (i, i) for i in range(n)) + ";"
        qbs = [hiword_qb(l1, e, m, s, 0, 0) for _nm, _b, m, s, l1, e, _k in mul_nodes(t, 0)]
        marks[nm, None, None] = qbs
        it = iter(qbs)
        lines = ["template <int B> TX1D_FN void r1_%s(T *c) {" % nm, ins]
        prods = set(name for name, expr in ops if expr.startswith("TX_MUL("))
        for name, expr in ops:
            if expr.startswith("TX_MUL("):
                qb = next(it)
                assert hiword_ok(0, *[int(v) for v in _parse(expr)[1][1:]]) or qb == 0
                expr = "TX_MULW(%s, %d)" % (expr[len("TX_MUL("):-1], qb)
            lines.append("  const T %s = %s;" % (name, _halve_w(expr, prods)))
        lines += ["  c[%d] = %s;" % (i, o) for i, o in enumerate(outs)]
        lines.append("}")
        body.append("\n".join(lines))
        # the column family: fold()'s text, its multiplies marked
        lines = ["template <int K0, int S, int B> TX1D_FN void r1_%s_col(T *c) {" % nm,
                 "  static_assert(%s, \"a (shift[0], -shift[1]) pair the column pass meets\");" %
                 " || ".join("(K0 == %d && S == %d)" % (k0, s) for k0, s, _m in pairs[n]), ins]
        for k0, s, inmax in pairs[n]:
            flines, _cnt, _fm, _pm = fold(n, ops, outs, k0, s, inmax)
            nodes = mul_nodes(t, inmax, k0)
            qbs = [hiword_qb(l1, e, m, se, k0, ka) for _nm, _b, m, se, l1, e, ka in nodes]
            marks[nm, k0, s] = qbs
            it = iter(zip(nodes, qbs))
            lines.append("  if constexpr (K0 == %d && S == %d) {" % (k0, s))
            defs = {}
            for ln in flines:
                mm = re.match(r"  const T (\w+) = TX_MUL(K?)\((.*)\);$", ln)
                if mm:
                    nd, qb = next(it)
                    a = [v.strip() for v in mm.group(3).split(",")]
                    ka = int(a[3]) if mm.group(2) else 0
                    assert nd[0] == mm.group(1) and nd[2] == int(a[1]) and nd[3] == int(a[2]) - ka and nd[6] == ka
                    # what the generator asserts for every node it emits in the new form: at its QB the node qualifies,
                    # one past it no longer does
                    assert qb == 0 or hiword_ok(int(math.ceil((qb << k0) * nd[4] + nd[5])) >> ka, nd[2], nd[3])
                    ln = "  const T %s = TX_MUL%sW(%s, %d);" % (mm.group(1), mm.group(2), mm.group(3), qb)
                defs[mm.group(1) if mm else ln.split(" = ")[0].split()[-1]] = ln
                lines.append("  " + _rnd_w(_halve_w(ln, prods), prods, defs))
            assert next(it, None) is None
            lines.append("  }")
        lines.append("}")
        body.append("\n".join(lines))
    hdr = ("/* GENERATED by tools/gen_tx1d.py from oracle/fwd_tx_np.py -- do not edit.\n"
           " * High-word family of the forward 1-D networks of 8 points and more, plain and column form: the text of\n"
           " * fwd_tx_1d.inc / fwd_tx_1d_col.inc with every multiply stated as TX_MULW(a, M, S, QB) /\n"
           " * TX_MULKW(a, M, S, k, QB).  QB = the largest bound of the network's inputs (column form: of the unshifted\n"
           " * residual) at which |a| * (M << (16 - s)) + 2^15 < 2^31 and M << (16 - s) < 2^23, s the shift the multiply\n"
           " * executes; B = the bound of the call.  Where B <= QB the product stays at scale 2^16 and the value is\n"
           " * P >> 16 (tools/gen_tx1d.py, hiword_family()). */\n")
    return hdr + "\n\n".join(body) + "\n", marks


def main():
    body = []
    stats = []
    for t, nm in enumerate(NAMES):
        if nm is None:
            continue
        txt, nops = trace(t)
        body.append(txt)
        stats.append("%s:%d" % (nm, nops))
    hdr = ("/* GENERATED by tools/gen_tx1d.py from oracle/fwd_tx_np.py -- do not edit.\n"
           " * Forward 1-D transform networks (restating the reference's\n"
           " * src/transform/forward_shared.rs:398-1796) as straight-line SSA.\n"
           " * primitive ops per network: %s */\n" % " ".join(stats))
    text = hdr + "\n\n".join(body) + "\n"
    for rel in ("oracle/fwd_tx_1d.inc", "rav1e_amd/csrc/fwd_tx_1d.inc"):
        with open(os.path.join(ROOT, rel), "w") as f:
            f.write(text)
        print("wrote", rel, len(text), "bytes")
    print(" ".join(stats))
    text, table = col_family()
    rel = "rav1e_amd/csrc/fwd_tx_1d_col.inc"
    with open(os.path.join(ROOT, rel), "w") as f:
        f.write(text)
    print("wrote", rel, len(text), "bytes")
    print("\n".join(table))
    text, _marks = hiword_family()
    rel = "rav1e_amd/csrc/fwd_tx_1d_hw.inc"
    with open(os.path.join(ROOT, rel), "w") as f:
        f.write(text)
    print("wrote", rel, len(text), "bytes")


if __name__ == "__main__":
    import tx_range   # column and row pass in their chain: every halving operand the fused kernels meet
    for (bd, ts, tt), hb in sorted(tx_range.halving_bounds().items()):
        assert hb < HALVE2_LIMIT, (bd, ts, tt, hb)
    main()

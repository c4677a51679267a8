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


def value_bounds(n, ops, inmax):
    """|value| bound of every SSA name of the PLAIN network fed with |input| <= inmax: inmax * L1 norm of the value's
    response to the inputs (the networks are linear up to rounding) + the accumulated rounding error."""
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
    return {k: int(math.ceil(inmax * sum(abs(x) for x in v) + err[k])) for k, v in vec.items()}


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


def fold(n, ops, outs, k0, s, inmax):
    """-> (body lines, (fast, slow), mad-input bound folded, mad-input bound plain)"""
    vb = value_bounds(n, ops, inmax << k0)
    parsed = [(name,) + tuple(_parse(expr)) for name, expr in ops]
    plain_mad = max(vb[a[0]] for _, op, a in parsed if op == "MUL")
    # pass 1: the pending scale of every value (independent of how operands get aligned)
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


if __name__ == "__main__":
    import tx_range   # column and row pass in their chain: every halving operand the fused kernels meet
    for (bd, ts, tt), hb in sorted(tx_range.halving_bounds().items()):
        assert hb < HALVE2_LIMIT, (bd, ts, tt, hb)
    main()

#!/usr/bin/env python3
"""Worst-case magnitude of every multiplier input of the forward transform.

Each 1-D network is (up to rounding) linear, so the worst-case |a| at a
multiplier fed by inputs bounded by B is B * (L1 norm of that node's impulse
responses) + a small rounding slack.  We measure the impulse responses by
running the NumPy restatement on scaled unit impulses, one lane per impulse,
and intercepting tx_mul.  Used to justify v_mul_i32_i24 (needs |a| < 2^23) in
the fused kernel, where the residual is bounded by the pixel range.
"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fwd_tx_np as F

AMP = 1 << 14   # impulse amplitude (keeps relative rounding error ~1e-4)


def l1_gain(ttype):
    """-> (max L1 gain over all tx_mul inputs, max L1 gain over outputs)"""
    n = F.TXFM_LEN[ttype]
    rec = []
    orig = F.tx_mul

    def spy(a, mul, shift):
        rec.append(np.abs(a.astype(np.float64)).sum() / AMP)
        return orig(a, mul, shift)
    F.tx_mul = spy
    try:
        x = (np.eye(n, dtype=np.int32) * AMP)
        outs = F.TXFM_FUNCS[ttype]([np.ascontiguousarray(x[:, i]) for i in range(n)])
    finally:
        F.tx_mul = orig
    og = max(np.abs(o.astype(np.float64)).sum() / AMP for o in outs)
    return (max(rec) if rec else 0.0), og


def analyse():
    rows = []
    for bd in (8, 10, 12):
        for ts, (w, h) in enumerate(F.TX_DIMS):
            for tt in range(16):
                if not F.valid_av1_transform(ts, tt):
                    continue
                sh = F.FWD_SHIFT[ts][(bd - 8) // 2]
                wi, hi = w.bit_length() - 3, h.bit_length() - 3
                tcol = F.TXFM_TYPE_LS[hi][F.VTX_TAB[tt]]
                trow = F.TXFM_TYPE_LS[wi][F.HTX_TAB[tt]]
                b0 = ((1 << bd) - 1) * (1 << sh[0])          # column input bound
                gm, go = l1_gain(tcol)
                col_mul = b0 * gm + 64
                col_out = b0 * go + 64
                b1 = col_out * 2.0 ** sh[1] + 1                 # after shift[1]
                gm2, go2 = l1_gain(trow)
                row_mul = b1 * gm2 + 64
                rows.append((bd, ts, tt, max(col_mul, row_mul, b0, b1)))
    return rows


def shifted_coefficient_bound():
    """{bit depth: max over sizes / types of |c << log_tx_scale| for residuals that come from pixels}: the magnitude
    the quantizer divides (quantize/mod.rs:296-318) -- what lets the fused kernels' quantizer run on 24-bit multipliers
    (csrc/quant_common.hpp, QParams::ac_m22: a + ac_offset < 2^22)"""
    worst = {8: 0.0, 10: 0.0, 12: 0.0}
    for bd in worst:
        for ts, (w, h) in enumerate(F.TX_DIMS):
            for tt in range(16):
                if not F.valid_av1_transform(ts, tt):
                    continue
                sh = F.FWD_SHIFT[ts][(bd - 8) // 2]
                tcol = F.TXFM_TYPE_LS[h.bit_length() - 3][F.VTX_TAB[tt]]
                trow = F.TXFM_TYPE_LS[w.bit_length() - 3][F.HTX_TAB[tt]]
                b0 = ((1 << bd) - 1) * (1 << sh[0])
                _, go = l1_gain(tcol)
                b1 = (b0 * go + 64) * 2.0 ** sh[1] + 1
                _, go2 = l1_gain(trow)
                out = (b1 * go2 + 64) * 2.0 ** sh[2] + 1
                lts = (w * h > 256) + (w * h > 1024)
                worst[bd] = max(worst[bd], out * (1 << lts))
    return worst


def halving_bounds():
    """{(bit depth, tx_size, tx_type): largest |operand| of a TX_RSHIFT1 in the column pass and the row pass of a
    fused kernel}, residuals from pixels: the plain networks fed with residual << shift[0], or the column family on
    the unshifted residual (the same values, tools/gen_tx1d.py halving_bound), then the row network fed with the
    column outputs after shift[1].  The two-instruction halving of m24h (csrc/tx_common.hpp) needs them below
    2^24.  Bounds are L1 norms of the SSA values' responses plus the accumulated rounding, as for the 24-bit mads.
    The composition is forward_transform's (oracle/fwd_tx_np.py, forward.rs:71-161) for all 19 sizes: that function
    has no step of its own for rectangles (the daala networks carry their scaling), and its identity is a no-op
    (forward_shared.rs:1775).  The form is enabled, and run numerically by tests/test_tx_halve2.py, only for the
    square sizes 8x8 .. 64x64; for the other sizes this is the bound alone."""
    import math
    import gen_tx1d as G
    nets = {}

    def bound(t, inmax):
        if G.NAMES[t] is None:    # the identity: no halving, outputs = inputs (tx_type < 16: the WHT is never met)
            return 0, inmax
        if t not in nets:
            nets[t] = G.trace_ops(t)
        n, ops, outs = nets[t]
        return G.halving_bound(n, ops, outs, inmax)
    res = {}
    for bd in (8, 10, 12):
        for ts, (w, h) in enumerate(F.TX_DIMS):
            for tt in range(16):
                if not F.valid_av1_transform(ts, tt):
                    continue
                sh = F.FWD_SHIFT[ts][(bd - 8) // 2]
                tcol = F.TXFM_TYPE_LS[h.bit_length() - 3][F.VTX_TAB[tt]]
                trow = F.TXFM_TYPE_LS[w.bit_length() - 3][F.HTX_TAB[tt]]
                hcol, ocol = bound(tcol, ((1 << bd) - 1) << sh[0])
                hrow, _ = bound(trow, int(math.ceil(ocol * 2.0 ** sh[1])) + 1)
                res[bd, ts, tt] = max(hcol, hrow)
    return res


def chain_input_bounds(bd, ts, tt):
    """(|input| bound of the column network = pixel range << shift[0], |input| bound of the row network = the column
    outputs after shift[1]) of a fused kernel's chain, residuals from pixels; the composition is halving_bounds()'s"""
    import math
    import gen_tx1d as G
    w, h = F.TX_DIMS[ts]
    sh = F.FWD_SHIFT[ts][(bd - 8) // 2]
    tcol = F.TXFM_TYPE_LS[h.bit_length() - 3][F.VTX_TAB[tt]]
    b0 = ((1 << bd) - 1) << sh[0]
    if G.NAMES[tcol] is None:            # the identity
        ocol = b0
    else:
        n, ops, outs, gains = G.net(tcol)
        ocol = max(int(math.ceil(b0 * gains[o][0] + gains[o][1])) for o in outs)
    return b0, int(math.ceil(ocol * 2.0 ** sh[1])) + 1


def mul_bounds():
    """{(bit depth, tx_size, tx_type, pass): [(worst-case |a|, M, shift executed)] for every multiply of the pass's
    network in trace order}, residuals from pixels.  pass: "col" = the plain network fed with residual << shift[0];
    "colk" = the column family on the unshifted residual (tools/gen_tx1d.py fold(): the factor is the register,
    the plain value >> k, and the multiply shifts by S - k), where shift[0] > 0; "row" = the plain network fed with the
    column outputs after shift[1].  |a| = the input bound times the node's L1 gain plus the accumulated rounding, as
    for the 24-bit mads and the halvings.  A product may stay at scale 2^16 (m24w, csrc/tx_common.hpp) where
    gen_tx1d.hiword_ok(|a|, M, shift) holds."""
    import gen_tx1d as G
    res = {}
    for bd in (8, 10, 12):
        for ts, (w, h) in enumerate(F.TX_DIMS):
            for tt in range(16):
                if not F.valid_av1_transform(ts, tt):
                    continue
                sh = F.FWD_SHIFT[ts][(bd - 8) // 2]
                tcol = F.TXFM_TYPE_LS[h.bit_length() - 3][F.VTX_TAB[tt]]
                trow = F.TXFM_TYPE_LS[w.bit_length() - 3][F.HTX_TAB[tt]]
                b0, b1 = chain_input_bounds(bd, ts, tt)

                def nodes(t, inmax, k0=None):
                    if G.NAMES[t] is None:
                        return []
                    return [(b, m, s) for _n, b, m, s, _l, _e, _k in G.mul_nodes(t, inmax, k0)]
                res[bd, ts, tt, "col"] = nodes(tcol, b0)
                if sh[0] > 0:
                    res[bd, ts, tt, "colk"] = nodes(tcol, (1 << bd) - 1, int(sh[0]))
                res[bd, ts, tt, "row"] = nodes(trow, b1)
    return res


if __name__ == "__main__":
    hb = halving_bounds()
    for bd in (8, 10, 12):
        print("bd %d: halving operands < 2^%.2f" % (bd, np.log2(max(v for k, v in hb.items() if k[0] == bd))))
    rows = analyse()
    worst = max(rows, key=lambda r: r[3])
    print("worst multiplier input: bd=%d tx_size=%d tx_type=%d |a| <= %.0f = 2^%.2f"
          % (worst[0], worst[1], worst[2], worst[3], np.log2(worst[3])))
    for bd in (8, 10, 12):
        m = max(r[3] for r in rows if r[0] == bd)
        print("bd %d: 2^%.2f" % (bd, np.log2(m)))

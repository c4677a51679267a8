"""What every entry point answers to a bad argument, as a table: entry point, a valid argument set, and overrides
applied one at a time, each with the status it returns (0 = accepted, -1 = R1_EINVAL).  Nothing here touches a
device: the context is a zeroed stand-in, the buffers are host memory, and every row either fails a check or leaves
through the `n <= 0` early-out (for the lookahead entry points: an empty plane) that follows the checks.

The table pins what the library does, its inconsistencies included -- a 0 where a sibling answers -1 (r1_dist_batch
takes one-byte pixels with bit_depth = 10, r1_activity_scales does not) is as much a row as a refusal is.

Not in the table, because a HIP call can come before the last argument check:
  r1_estimate_tile_motion_batch, r1_me_status            (device guard first)
  r1_rdo_intra_cand_batch                                (hipPointerGetAttributes before the CFL check;
                                                          its refusals are tests/test_rdo_intra_host.py)
  r1_comm_*, r1_push_rects, r1_ipc_*                     (need a communicator / a device)
Entry points without an early-out (r1_plane_pad, r1_cdef_*frame*, r1_cdef_strength_search, r1_lrf_sgrproj_plane,
r1_deblock_sse_*, ...) have refusals only: an accepted set would launch.
"""
import collections
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class P(collections.namedtuple("P", "bpp bd w h buf stride", defaults=(64, 64, 0, 64))):
    """an R1Plane on host memory: bytes per pixel, bit depth, size, which of two backing buffers, stride"""

    def __repr__(self):
        v = list(self)
        while len(v) > 2 and v[-1] == P._field_defaults[P._fields[len(v) - 1]]:
            v.pop()
        return "P(%s)" % ", ".join(map(str, v))


def _spec(name, fields):
    return collections.namedtuple(name, fields)


QP = _spec("QP", "bd")                       # R1QuantParams of that bit depth
CDEFP = _spec("CDEFP", "bd")                 # R1CdefParams
CSP = _spec("CSP", "bd planes xdec ydec")    # R1CdefSearchParams of a 64 x 64 frame
MEP = _spec("MEP", "bd")                     # R1MeParams
MEJOB = _spec("MEJOB", "org ref")            # R1MeJob whose source / reference planes are all `org` / `ref`


def PL3(a, b=None, c=None):
    """R1Plane[3]"""
    return (a, b if b is not None else a, c if c is not None else a)


class _Buf:
    def __repr__(self):
        return "BUF"


BUF = _Buf()                                 # any non-NULL array: zeroed host memory


def fmt(d):
    return "dict(%s)" % ", ".join("%s=%r" % kv for kv in d.items())


class Harness:
    def __init__(self, path=None):
        from rav1e_amd import _lib
        self._lib = _lib
        if path is None:
            self.L = _lib.load()
        else:
            self.L = C.CDLL(path)
            for name, (res, args) in _lib.SYMBOLS.items():
                f = getattr(self.L, name)
                f.restype, f.argtypes = res, args
        self.fake_ctx = (C.c_uint8 * 65536)()
        self.mem = [(C.c_uint8 * (1 << 16))() for _ in range(3)]     # two plane buffers and BUF
        text = open(os.path.join(ROOT, "include", "rav1e_amd.h")).read()
        self.params = {}
        for name in _lib.SYMBOLS:
            m = re.search(r"\b%s\((.*?)\);" % name, text, re.S)
            if m:
                self.params[name] = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]

    def plane(self, p):
        return self._lib.R1Plane(C.addressof(self.mem[p.buf]), p.stride, 64, p.w, p.h, 0, 0, p.bpp, p.bd)

    def value(self, v, keep):
        """a table value as a ctypes argument; `keep` holds what the pointers point to until the call returns"""
        L = self._lib
        if v is None or isinstance(v, int):
            return v
        if v is BUF:
            return C.addressof(self.mem[2])
        if isinstance(v, P):
            o = self.plane(v)
        elif isinstance(v, tuple) and isinstance(v[0], P) and not hasattr(v, "_fields"):
            o = (L.R1Plane * 3)(*[self.plane(p) for p in v])
        elif isinstance(v, QP):
            o = L.R1QuantParams(qindex=60, bit_depth=v.bd)
        elif isinstance(v, CDEFP):
            o = L.R1CdefParams(damping=3, bit_depth=v.bd)
        elif isinstance(v, CSP):
            o = L.R1CdefSearchParams(damping=3, bit_depth=v.bd, n_idx=1, planes=v.planes, xdec=v.xdec, ydec=v.ydec,
                                     crop_w=64, crop_h=64, area_sb_w=1, area_sb_h=1)
        elif isinstance(v, MEP):
            o = L.R1MeParams(w_in_b=16, h_in_b=16, stats_cols=16, stats_rows=16, bit_depth=v.bd)
        elif isinstance(v, MEJOB):
            o = L.R1MeJob(stats=C.addressof(self.mem[2]), tile_w=64, tile_h=64)
            for k in range(3):
                o.org[k], o.ref[k] = self.plane(v.org), self.plane(v.ref)
        else:
            raise TypeError(v)
        keep.append(o)
        return C.pointer(o)

    def call(self, name, base, over):
        names = self.params[name]
        v = dict(ctx=C.addressof(self.fake_ctx), stream=None)
        v.update({k.rstrip("_"): x for k, x in base.items()})
        assert {k.rstrip("_") for k in over} <= set(v), (name, over)
        v.update({k.rstrip("_"): x for k, x in over.items()})
        assert set(v) - {"ctx", "stream"} <= set(names), (name, set(v) - set(names))
        keep = []
        args = []
        for k, t in zip(names, self._lib.SYMBOLS[name][1]):
            a = self.value(v[k], keep)
            if isinstance(a, int) and hasattr(t, "contents"):      # an address for a typed pointer parameter
                a = C.c_void_p(a)
            args.append(a if a is None or isinstance(a, int) else C.cast(a, t))
        return getattr(self.L, name)(*args)


P8, P10 = P(1, 8), P(2, 10)

# (entry point, valid arguments, [(override, status), ...]); dict() is the valid set itself
TABLE = [
    ("r1_dist_batch", dict(kind=0, org=P(1, 8), ref=P(1, 8), w=8, h=8, cands=BUF, n=0, out=BUF), [
        (dict(), 0),
        (dict(org=P(3, 8), ref=P(3, 8)), -1),
        (dict(org=P(1, 10), ref=P(1, 10)), 0),
        (dict(org=P(2, 8), ref=P(2, 8)), 0),
        (dict(ref=P(2, 10)), -1),
        (dict(ref=P(1, 10)), 0),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(out=None, n=0), 0),
        (dict(out=None, n=1), -1),
    ]),
    ("r1_dist_scaled_batch", dict(kind=2, org=P(1, 8), ref=P(1, 8), w=8, h=8, cands=BUF, n=0, scales=None, scale_stride=0, xdec=0, ydec=0, out=BUF), [
        (dict(), 0),
        (dict(org=P(3, 8), ref=P(3, 8)), -1),
        (dict(org=P(1, 10), ref=P(1, 10)), 0),
        (dict(org=P(2, 8), ref=P(2, 8)), 0),
        (dict(ref=P(2, 10)), -1),
        (dict(ref=P(1, 10)), 0),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(out=None, n=0), 0),
        (dict(out=None, n=1), -1),
    ]),
    ("r1_plane_pad", dict(plane=P(1, 8), w=8, h=8, xdec=0, ydec=0), [
        (dict(plane=P(3, 8)), -1),
        (dict(plane=None), -1),
        (dict(xdec=3), -1),
        (dict(ydec=-1), -1),
    ]),
    ("r1_plane_downsample", dict(src=P(1, 8), dst=P(1, 8, 32, 32, 1), frame_w=64, frame_h=64, dst_xdec=1, dst_ydec=1), [
        (dict(src=P(3, 8), dst=P(3, 8, 32, 32, 1)), -1),
        (dict(dst=P(2, 10, 32, 32, 1)), -1),
        (dict(src=None), -1),
        (dict(dst=None), -1),
        (dict(dst_xdec=3), -1),
        (dict(dst_ydec=0), -1),
    ]),
    ("r1_fwd_txfm_batch", dict(residual=BUF, coeffs=BUF, n=0, tx_size=1, tx_type=0, bit_depth=8, coeff_bytes=2), [
        (dict(), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(bit_depth=9), -1),
        (dict(residual=None, n=0), 0),
        (dict(residual=None, n=1), -1),
        (dict(coeffs=None, n=0), 0),
        (dict(coeffs=None, n=1), -1),
    ]),
    ("r1_inv_txfm_add_batch", dict(coeffs=BUF, coeff_stride=64, pred=BUF, rec=BUF, n=0, tx_size=1, tx_type=0, bit_depth=8, bytes_per_px=1), [
        (dict(), 0),
        (dict(bytes_per_px=3), -1),
        (dict(bit_depth=10), -1),
        (dict(bytes_per_px=2), -1),
        (dict(bytes_per_px=2, bit_depth=10), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(bit_depth=9), -1),
        (dict(coeffs=None, n=0), 0),
        (dict(coeffs=None, n=1), -1),
        (dict(pred=None, n=0), 0),
        (dict(pred=None, n=1), -1),
        (dict(rec=None, n=0), 0),
        (dict(rec=None, n=1), -1),
    ]),
    ("r1_quantize_batch", dict(coeffs=BUF, coeff_stride=64, n=0, tx_size=1, tx_type=0, params=QP(bd=8), coeff_bytes=2, qcoeffs=BUF, eobs=BUF, rcoeffs=BUF), [
        (dict(), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(params=QP(bd=9)), -1),
        (dict(params=None), -1),
        (dict(coeffs=None, n=0), 0),
        (dict(coeffs=None, n=1), -1),
        (dict(qcoeffs=None, n=0), 0),
        (dict(qcoeffs=None, n=1), -1),
        (dict(eobs=None, n=0), 0),
        (dict(eobs=None, n=1), -1),
    ]),
    ("r1_quantize_rdo_batch", dict(coeffs=BUF, coeff_stride=64, n=0, tx_size=1, tx_type=0, params=QP(bd=8), coeff_bytes=2, qcoeffs=BUF, eobs=BUF, rcoeffs=BUF, tx_dist=BUF, est_rate=BUF), [
        (dict(), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(params=QP(bd=9)), -1),
        (dict(params=None), -1),
        (dict(coeffs=None, n=0), 0),
        (dict(coeffs=None, n=1), -1),
        (dict(qcoeffs=None, n=0), 0),
        (dict(qcoeffs=None, n=1), -1),
        (dict(eobs=None, n=0), 0),
        (dict(eobs=None, n=1), -1),
        (dict(tx_dist=None, n=0), 0),
        (dict(tx_dist=None, n=1), -1),
    ]),
    ("r1_dequantize_batch", dict(qcoeffs=BUF, n=0, tx_size=1, params=QP(bd=8), coeff_bytes=2, rcoeffs=BUF), [
        (dict(), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(params=QP(bd=9)), -1),
        (dict(params=None), -1),
        (dict(qcoeffs=None, n=0), 0),
        (dict(qcoeffs=None, n=1), -1),
        (dict(rcoeffs=None, n=0), 0),
        (dict(rcoeffs=None, n=1), -1),
    ]),
    ("r1_intra_edges_batch", dict(rec=P(1, 8), tile_x=0, tile_y=0, tile_w=64, tile_h=64, tx_size=1, cands=BUF, n=0, edges=BUF, edge_stride=257, lens=BUF), [
        (dict(), 0),
        (dict(rec=P(3, 8)), -1),
        (dict(rec=P(1, 10)), 0),
        (dict(rec=P(2, 8)), 0),
        (dict(rec=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(edges=None, n=0), 0),
        (dict(edges=None, n=1), -1),
        (dict(lens=None, n=0), 0),
        (dict(lens=None, n=1), -1),
    ]),
    ("r1_predict_intra_batch", dict(tx_size=1, cands=BUF, n=0, edges=BUF, edge_stride=257, lens=BUF, ac=None, bit_depth=8, bytes_per_px=1, dst=BUF), [
        (dict(), 0),
        (dict(bytes_per_px=3), -1),
        (dict(bit_depth=10), -1),
        (dict(bytes_per_px=2), -1),
        (dict(bytes_per_px=2, bit_depth=10), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(bit_depth=9), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(edges=None, n=0), 0),
        (dict(edges=None, n=1), -1),
        (dict(lens=None, n=0), 0),
        (dict(lens=None, n=1), -1),
        (dict(dst=None, n=0), 0),
        (dict(dst=None, n=1), -1),
    ]),
    ("r1_intra_satd_batch", dict(src=P(1, 8), tx_size=1, cands=BUF, n=0, group=1, pos_xy=BUF, edges=BUF, edge_stride=257, lens=BUF, ac=None, satd_out=BUF), [
        (dict(), 0),
        (dict(src=P(3, 8)), -1),
        (dict(src=P(1, 10)), -1),
        (dict(src=P(2, 8)), -1),
        (dict(src=None), -1),
        (dict(src=P(1, 9)), -1),
        (dict(src=P(2, 10)), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(edges=None, n=0), 0),
        (dict(edges=None, n=1), -1),
        (dict(lens=None, n=0), 0),
        (dict(lens=None, n=1), -1),
        (dict(pos_xy=None, n=0), 0),
        (dict(pos_xy=None, n=1), -1),
        (dict(satd_out=None, n=0), 0),
        (dict(satd_out=None, n=1), -1),
    ]),
    ("r1_cfl_ac_batch", dict(luma=P(1, 8), bw=8, bh=8, xdec=1, ydec=1, cands=BUF, n=0, ac=BUF), [
        (dict(), 0),
        (dict(luma=P(3, 8)), -1),
        (dict(luma=P(1, 10)), 0),
        (dict(luma=P(2, 8)), 0),
        (dict(luma=None), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(xdec=0, ydec=1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(ac=None, n=0), 0),
        (dict(ac=None, n=1), -1),
    ]),
    ("r1_cfl_alpha_search_batch", dict(src=P(1, 8), tx_size=1, cands=BUF, n=0, edges=BUF, edge_stride=257, lens=BUF, ac=BUF, alpha_out=BUF, cost_out=None), [
        (dict(), 0),
        (dict(src=P(3, 8)), -1),
        (dict(src=P(1, 10)), -1),
        (dict(src=P(2, 8)), -1),
        (dict(src=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(tx_size=4), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(edges=None, n=0), 0),
        (dict(edges=None, n=1), -1),
        (dict(lens=None, n=0), 0),
        (dict(lens=None, n=1), -1),
        (dict(ac=None, n=0), 0),
        (dict(ac=None, n=1), -1),
        (dict(alpha_out=None, n=0), 0),
        (dict(alpha_out=None, n=1), -1),
    ]),
    ("r1_cdef_find_dir_batch", dict(luma=P(1, 8), cands=BUF, n=0, dir_out=BUF, var_out=BUF), [
        (dict(), 0),
        (dict(luma=P(3, 8)), -1),
        (dict(luma=P(1, 10)), 0),
        (dict(luma=P(2, 8)), 0),
        (dict(luma=None), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(dir_out=None, n=0), 0),
        (dict(dir_out=None, n=1), -1),
        (dict(var_out=None, n=0), 0),
        (dict(var_out=None, n=1), -1),
    ]),
    ("r1_cdef_filter_block_batch", dict(in_=P(1, 8), out=P(1, 8, 64, 64, 1), xdec=0, ydec=0, cands=BUF, n=0), [
        (dict(), 0),
        (dict(in_=P(3, 8), out=P(3, 8, 64, 64, 1)), -1),
        (dict(in_=P(1, 10), out=P(1, 10, 64, 64, 1)), 0),
        (dict(in_=P(2, 8), out=P(2, 8, 64, 64, 1)), 0),
        (dict(out=P(2, 10, 64, 64, 1)), -1),
        (dict(out=P(1, 10, 64, 64, 1)), 0),
        (dict(out=P(1, 8)), -1),
        (dict(in_=None), -1),
        (dict(out=None), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
    ]),
    ("r1_cdef_analyze_frame", dict(luma=P(1, 8), tile_w=64, tile_h=64, mi_cols=16, mi_rows=16, dir_out=BUF, var_out=BUF), [
        (dict(luma=P(3, 8)), -1),
        (dict(luma=P(1, 9)), -1),
        (dict(luma=None), -1),
        (dict(dir_out=None), -1),
        (dict(var_out=None), -1),
    ]),
    ("r1_cdef_filter_frame_plane", dict(luma=P(1, 8), in_=P(1, 8), out=P(1, 8, 64, 64, 1), p=0, xdec=0, ydec=0, tile_w=64, tile_h=64, skip_mi=BUF, mi_stride=16, mi_cols=16, mi_rows=16, cdef_index_sb=BUF, sb_stride=1, params=CDEFP(bd=8)), [
        (dict(in_=P(3, 8), out=P(3, 8, 64, 64, 1)), -1),
        (dict(out=P(2, 10, 64, 64, 1)), -1),
        (dict(out=P(1, 8)), -1),
        (dict(p=1, xdec=2), -1),
        (dict(p=1, ydec=-1), -1),
        (dict(xdec=1), -1),
        (dict(params=CDEFP(bd=9)), -1),
        (dict(params=None), -1),
        (dict(in_=None), -1),
        (dict(out=None), -1),
        (dict(skip_mi=None), -1),
        (dict(cdef_index_sb=None), -1),
        (dict(luma=P(3, 8), in_=P(3, 8), out=P(3, 8, 64, 64, 1)), -1),
        (dict(luma=P(2, 10)), -1),
        (dict(luma=P(1, 10)), -1),
        (dict(luma=None), -1),
    ]),
    ("r1_cdef_filter_frame_plane_dirs", dict(dirs=BUF, vars=BUF, in_=P(1, 8), out=P(1, 8, 64, 64, 1), p=0, xdec=0, ydec=0, tile_w=64, tile_h=64, skip_mi=BUF, mi_stride=16, mi_cols=16, mi_rows=16, cdef_index_sb=BUF, sb_stride=1, params=CDEFP(bd=8)), [
        (dict(in_=P(3, 8), out=P(3, 8, 64, 64, 1)), -1),
        (dict(out=P(2, 10, 64, 64, 1)), -1),
        (dict(out=P(1, 8)), -1),
        (dict(p=1, xdec=2), -1),
        (dict(p=1, ydec=-1), -1),
        (dict(xdec=1), -1),
        (dict(params=CDEFP(bd=9)), -1),
        (dict(params=None), -1),
        (dict(in_=None), -1),
        (dict(out=None), -1),
        (dict(skip_mi=None), -1),
        (dict(cdef_index_sb=None), -1),
        (dict(dirs=None), -1),
        (dict(vars=None), -1),
        (dict(tile_w=60), -1),
    ]),
    ("r1_cdef_strength_search", dict(err_out=BUF, best_out=BUF, scratch=BUF, rec=(P(1, 8), P(1, 8), P(1, 8)), src=(P(1, 8), P(1, 8), P(1, 8)), skip_mi=BUF, mi_stride=16, mi_cols=16, mi_rows=16, scales=None, scale_stride=0, params=CSP(bd=8, planes=3, xdec=1, ydec=1)), [
        (dict(rec=(P(3, 8), P(3, 8), P(3, 8)), src=(P(3, 8), P(3, 8), P(3, 8))), -1),
        (dict(params=CSP(bd=10, planes=3, xdec=1, ydec=1)), -1),
        (dict(params=CSP(bd=9, planes=3, xdec=1, ydec=1)), -1),
        (dict(rec=(P(2, 8), P(2, 8), P(2, 8)), src=(P(2, 8), P(2, 8), P(2, 8))), -1),
        (dict(src=(P(1, 8), P(1, 8), P(2, 10))), -1),
        (dict(rec=(P(1, 8), P(2, 10), P(1, 8))), -1),
        (dict(params=CSP(bd=8, planes=3, xdec=0, ydec=1)), -1),
        (dict(params=CSP(bd=8, planes=3, xdec=2, ydec=1)), -1),
        (dict(params=None), -1),
        (dict(rec=None), -1),
        (dict(src=None), -1),
        (dict(skip_mi=None), -1),
        (dict(err_out=None), -1),
        (dict(best_out=None), -1),
        (dict(scratch=None), -1),
    ]),
    ("r1_cdef_lrf_trial_batch", dict(cdef_cur=(P(1, 8), P(1, 8), P(1, 8)), units=BUF, n_units=BUF, sb_sel=None, err_out=BUF, err_planes_out=None, best_out=BUF, scratch=BUF, rec=(P(1, 8), P(1, 8), P(1, 8)), src=(P(1, 8), P(1, 8), P(1, 8)), skip_mi=BUF, mi_stride=16, mi_cols=16, mi_rows=16, scales=None, scale_stride=0, params=CSP(bd=8, planes=3, xdec=1, ydec=1)), [
        (dict(rec=(P(3, 8), P(3, 8), P(3, 8)), src=(P(3, 8), P(3, 8), P(3, 8))), -1),
        (dict(params=CSP(bd=10, planes=3, xdec=1, ydec=1)), -1),
        (dict(params=CSP(bd=9, planes=3, xdec=1, ydec=1)), -1),
        (dict(rec=(P(2, 8), P(2, 8), P(2, 8)), src=(P(2, 8), P(2, 8), P(2, 8))), -1),
        (dict(src=(P(1, 8), P(1, 8), P(2, 10))), -1),
        (dict(rec=(P(1, 8), P(2, 10), P(1, 8))), -1),
        (dict(params=CSP(bd=8, planes=3, xdec=0, ydec=1)), -1),
        (dict(params=CSP(bd=8, planes=3, xdec=2, ydec=1)), -1),
        (dict(params=None), -1),
        (dict(rec=None), -1),
        (dict(src=None), -1),
        (dict(skip_mi=None), -1),
        (dict(err_out=None), -1),
        (dict(best_out=None), -1),
        (dict(scratch=None), -1),
        (dict(n_units=None), -1),
    ]),
    ("r1_cdef_apply_area", dict(out=(P(1, 8, 64, 64, 1), P(1, 8, 64, 64, 1), P(1, 8, 64, 64, 1)), index_sb=BUF, scratch=BUF, rec=(P(1, 8), P(1, 8), P(1, 8)), skip_mi=BUF, mi_stride=16, mi_cols=16, mi_rows=16, params=CSP(bd=8, planes=3, xdec=1, ydec=1)), [
        (dict(params=CSP(bd=10, planes=3, xdec=1, ydec=1)), -1),
        (dict(params=CSP(bd=9, planes=3, xdec=1, ydec=1)), -1),
        (dict(rec=(P(1, 8), P(2, 10), P(1, 8))), -1),
        (dict(params=CSP(bd=8, planes=3, xdec=0, ydec=1)), -1),
        (dict(params=CSP(bd=8, planes=3, xdec=2, ydec=1)), -1),
        (dict(params=None), -1),
        (dict(rec=None), -1),
        (dict(skip_mi=None), -1),
        (dict(out=(P(2, 10, 64, 64, 1), P(2, 10, 64, 64, 1), P(2, 10, 64, 64, 1))), -1),
        (dict(out=(P(1, 8), P(1, 8), P(1, 8))), -1),
        (dict(out=None), -1),
        (dict(index_sb=None), -1),
        (dict(scratch=None), -1),
    ]),
    ("r1_estimate_intra_costs", dict(luma=P(1, 8, 0, 0), costs=BUF), [
        (dict(), 0),
        (dict(luma=P(3, 8, 0, 0)), -1),
        (dict(luma=P(1, 10, 0, 0)), 0),
        (dict(luma=P(2, 8, 0, 0)), 0),
        (dict(luma=None), -1),
        (dict(costs=None), -1),
    ]),
    ("r1_estimate_inter_costs", dict(org=P(1, 8, 0, 0), ref=P(1, 8, 0, 0), mvs=BUF, costs=BUF), [
        (dict(), 0),
        (dict(org=P(3, 8, 0, 0), ref=P(3, 8, 0, 0)), -1),
        (dict(org=P(1, 10, 0, 0)), 0),
        (dict(org=P(2, 8, 0, 0), ref=P(2, 8, 0, 0)), 0),
        (dict(ref=P(2, 10, 0, 0)), -1),
        (dict(ref=P(1, 10, 0, 0)), 0),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(mvs=None), -1),
        (dict(costs=None), -1),
    ]),
    ("r1_importance_block_difference", dict(org=P(1, 8, 0, 0), ref=P(1, 8, 0, 0), sum_out=BUF), [
        (dict(org=P(3, 8, 0, 0), ref=P(3, 8, 0, 0)), -1),
        (dict(ref=P(2, 10, 0, 0)), -1),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(sum_out=None), -1),
    ]),
    ("r1_activity_scales", dict(luma=P(1, 8, 0, 0), variances=BUF, scales=BUF), [
        (dict(), 0),
        (dict(luma=P(3, 8, 0, 0)), -1),
        (dict(luma=P(1, 10, 0, 0)), -1),
        (dict(luma=P(2, 8, 0, 0)), -1),
        (dict(luma=P(2, 10, 0, 0)), 0),
        (dict(luma=None), -1),
        (dict(variances=None), 0),
        (dict(variances=None, scales=None), -1),
    ]),
    ("r1_mc_put_batch", dict(ref=P(1, 8), w=8, h=8, cands=BUF, n=0, dst=BUF), [
        (dict(), 0),
        (dict(ref=P(3, 8)), -1),
        (dict(ref=P(1, 10)), 0),
        (dict(ref=P(2, 8)), 0),
        (dict(ref=None), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(dst=None, n=0), 0),
        (dict(dst=None, n=1), -1),
    ]),
    ("r1_mc_prep_batch", dict(ref=P(1, 8), w=8, h=8, cands=BUF, n=0, tmp=BUF), [
        (dict(), 0),
        (dict(ref=P(3, 8)), -1),
        (dict(ref=P(1, 10)), 0),
        (dict(ref=P(2, 8)), 0),
        (dict(ref=None), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(tmp=None, n=0), 0),
        (dict(tmp=None, n=1), -1),
    ]),
    ("r1_mc_avg_batch", dict(tmp1=BUF, tmp2=BUF, w=8, h=8, n=0, bit_depth=8, bytes_per_px=1, dst=BUF), [
        (dict(), 0),
        (dict(bytes_per_px=3), -1),
        (dict(bit_depth=10), 0),
        (dict(bytes_per_px=2), 0),
        (dict(bytes_per_px=2, bit_depth=10), 0),
        (dict(bit_depth=9), -1),
        (dict(tmp1=None, n=0), 0),
        (dict(tmp1=None, n=1), -1),
        (dict(tmp2=None, n=0), 0),
        (dict(tmp2=None, n=1), -1),
        (dict(dst=None, n=0), 0),
        (dict(dst=None, n=1), -1),
    ]),
    ("r1_rdo_cand_batch", dict(sad_out=BUF, satd_out=BUF, coeffs=BUF, pred_out=None, org=P(1, 8), ref=P(1, 8), w=8, h=8, tx_size=1, cands=BUF, n=0), [
        (dict(), 0),
        (dict(org=P(3, 8), ref=P(3, 8)), -1),
        (dict(org=P(1, 10), ref=P(1, 10)), -1),
        (dict(org=P(2, 8), ref=P(2, 8)), -1),
        (dict(ref=P(2, 10)), -1),
        (dict(ref=P(1, 10)), -1),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
    ]),
    ("r1_rdo_full_cand_batch", dict(params=QP(bd=8), sad_out=BUF, satd_out=BUF, eob_out=BUF, tx_dist_out=BUF, est_rate_out=None, qcoeffs_out=None, coeffs=None, org=P(1, 8), ref=P(1, 8), w=8, h=8, tx_size=1, cands=BUF, n=0), [
        (dict(), 0),
        (dict(org=P(3, 8), ref=P(3, 8)), -1),
        (dict(org=P(1, 10), ref=P(1, 10)), -1),
        (dict(org=P(2, 8), ref=P(2, 8)), -1),
        (dict(ref=P(2, 10)), -1),
        (dict(ref=P(1, 10)), -1),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(params=QP(bd=10)), -1),
        (dict(params=None), -1),
        (dict(eob_out=None), -1),
        (dict(tx_dist_out=None), -1),
    ]),
    ("r1_rdo_pixel_cand_batch", dict(org=P(1, 8), ref=P(1, 8), w=8, h=8, tx_size=1, cands=BUF, n=0, params=QP(bd=8), dist_kind=2, scales=None, scale_stride=0, xdec=0, ydec=0, sad_out=None, satd_out=None, eob_out=BUF, dist_out=BUF, qcoeffs_out=None, rec_out=None), [
        (dict(), 0),
        (dict(org=P(3, 8), ref=P(3, 8)), -1),
        (dict(org=P(1, 10), ref=P(1, 10)), -1),
        (dict(org=P(2, 8), ref=P(2, 8)), -1),
        (dict(ref=P(2, 10)), -1),
        (dict(ref=P(1, 10)), -1),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(params=QP(bd=10)), -1),
        (dict(params=None), -1),
        (dict(eob_out=None), -1),
        (dict(dist_out=None), -1),
    ]),
    ("r1_rdo_pred_cand_batch", dict(pred=BUF, org=P(1, 8), w=8, h=8, tx_size=1, cands=BUF, n=0, params=QP(bd=8), dist_kind=2, scales=None, scale_stride=0, xdec=0, ydec=0, sad_out=None, satd_out=None, eob_out=BUF, dist_out=BUF, qcoeffs_out=None, rec_out=None), [
        (dict(), 0),
        (dict(org=P(3, 8)), -1),
        (dict(org=P(1, 10)), -1),
        (dict(org=P(2, 8)), -1),
        (dict(org=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(params=QP(bd=10)), -1),
        (dict(params=None), -1),
        (dict(eob_out=None), -1),
        (dict(dist_out=None), -1),
        (dict(pred=None), -1),
    ]),
    ("r1_rdo_txsearch_batch", dict(pred=None, tx_type_mask=1, est_rate_out=None, org=P(1, 8), ref=P(1, 8), w=8, h=8, tx_size=1, cands=BUF, n=0, params=QP(bd=8), dist_kind=2, scales=None, scale_stride=0, xdec=0, ydec=0, sad_out=None, satd_out=None, eob_out=BUF, dist_out=BUF, qcoeffs_out=None, rec_out=None), [
        (dict(), 0),
        (dict(org=P(3, 8), ref=P(3, 8)), -1),
        (dict(org=P(1, 10), ref=P(1, 10)), -1),
        (dict(org=P(2, 8), ref=P(2, 8)), -1),
        (dict(ref=P(2, 10)), -1),
        (dict(ref=P(1, 10)), -1),
        (dict(org=None), -1),
        (dict(ref=None), -1),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(params=QP(bd=10)), -1),
        (dict(params=None), -1),
        (dict(eob_out=None), -1),
        (dict(dist_out=None), -1),
        (dict(pred=BUF), -1),
        (dict(ref=None, pred=BUF), 0),
        (dict(ref=None, pred=BUF, org=P(1, 10)), -1),
    ]),
    ("r1_rdo_compound_cand_batch", dict(org=P(1, 8), ref0=P(1, 8), ref1=P(1, 8), w=8, h=8, cands=BUF, n=0, sad_out=BUF, satd_out=None, pred_out=None), [
        (dict(), 0),
        (dict(org=P(3, 8), ref0=P(3, 8), ref1=P(3, 8)), -1),
        (dict(org=P(1, 10), ref0=P(1, 10), ref1=P(1, 10)), -1),
        (dict(org=P(2, 8), ref0=P(2, 8), ref1=P(2, 8)), -1),
        (dict(ref0=P(2, 10)), -1),
        (dict(ref0=P(1, 10)), -1),
        (dict(ref1=P(2, 10)), -1),
        (dict(ref1=P(1, 10)), -1),
        (dict(org=None), -1),
        (dict(ref0=None), -1),
        (dict(ref1=None), -1),
        (dict(org=P(1, 9), ref0=P(1, 9), ref1=P(1, 9)), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
    ]),
    ("r1_lrf_sgrproj_plane", dict(cdeffed=P(1, 8), deblocked=P(1, 8), out=P(1, 8, 64, 64, 1), ydec=0, crop_w=64, crop_h=64, frame_height=64, unit_size=64, unit_cols=1, unit_rows=1, stripe_height=64, units=BUF), [
        (dict(cdeffed=P(3, 8), deblocked=P(3, 8), out=P(3, 8, 64, 64, 1)), -1),
        (dict(cdeffed=P(1, 10), deblocked=P(1, 10), out=P(1, 10, 64, 64, 1)), -1),
        (dict(cdeffed=P(2, 8), deblocked=P(2, 8), out=P(2, 8, 64, 64, 1)), -1),
        (dict(deblocked=P(2, 10)), -1),
        (dict(out=P(2, 10, 64, 64, 1)), -1),
        (dict(out=P(1, 8)), -1),
        (dict(ydec=-1), -1),
        (dict(ydec=2), -1),
        (dict(cdeffed=None), -1),
        (dict(deblocked=None), -1),
        (dict(out=None), -1),
        (dict(units=None), -1),
        (dict(cdeffed=P(1, 8, 64, 64, 0, 16777216)), -1),
    ]),
    ("r1_sgrproj_solve_batch", dict(cdeffed=P(1, 8), input=P(1, 8), units=BUF, n=0, max_w=64, max_h=64, moments_scratch=BUF, xqd_out=BUF), [
        (dict(), 0),
        (dict(cdeffed=P(3, 8), input=P(3, 8)), -1),
        (dict(cdeffed=P(1, 10), input=P(1, 10)), -1),
        (dict(cdeffed=P(2, 8), input=P(2, 8)), -1),
        (dict(input=P(2, 10)), -1),
        (dict(input=P(1, 10)), -1),
        (dict(cdeffed=None), -1),
        (dict(input=None), -1),
        (dict(input=P(1, 8, 64, 64, 0, 16777216)), -1),
        (dict(units=None, n=0), 0),
        (dict(units=None, n=1), -1),
        (dict(moments_scratch=None, n=0), 0),
        (dict(moments_scratch=None, n=1), -1),
        (dict(xqd_out=None, n=0), 0),
        (dict(xqd_out=None, n=1), -1),
    ]),
    ("r1_lrf_search_batch", dict(lrf_in=P(1, 8), src=P(1, 8), units=BUF, n=0, max_w=64, max_h=64, is_chroma=1, xdec=0, ydec=0, scales=None, scale_stride=0, dist_scale=16384, scratch=BUF, xqd_out=BUF, err_out=BUF), [
        (dict(), 0),
        (dict(lrf_in=P(3, 8), src=P(3, 8)), -1),
        (dict(lrf_in=P(1, 10), src=P(1, 10)), -1),
        (dict(lrf_in=P(2, 8), src=P(2, 8)), -1),
        (dict(src=P(2, 10)), -1),
        (dict(src=P(1, 10)), -1),
        (dict(lrf_in=None), -1),
        (dict(src=None), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(is_chroma=0, xdec=1), -1),
        (dict(src=P(1, 8, 64, 64, 0, 16777216)), -1),
        (dict(units=None, n=0), 0),
        (dict(units=None, n=1), -1),
        (dict(scratch=None, n=0), 0),
        (dict(scratch=None, n=1), -1),
        (dict(xqd_out=None, n=0), 0),
        (dict(xqd_out=None, n=1), -1),
        (dict(err_out=None, n=0), 0),
        (dict(err_out=None, n=1), -1),
    ]),
    ("r1_deblock_plane", dict(state=BUF, plane=P(1, 8), pli=0, xdec=0, ydec=0, blocks=BUF, blocks_stride=16, blocks_cols=16, blocks_rows=16, crop_w=64, crop_h=64), [
        (dict(), 0),
        (dict(plane=P(3, 8)), -1),
        (dict(plane=P(1, 10)), -1),
        (dict(plane=P(2, 8)), -1),
        (dict(plane=None), -1),
        (dict(pli=1, xdec=2), -1),
        (dict(pli=1, ydec=-1), -1),
        (dict(xdec=1), -1),
        (dict(state=None), -1),
        (dict(blocks=None), -1),
    ]),
    ("r1_deblock_sse_plane", dict(rec=P(1, 8), src=P(1, 8), pli=0, v_tally=BUF, h_tally=BUF, xdec=0, ydec=0, blocks=BUF, blocks_stride=16, blocks_cols=16, blocks_rows=16, crop_w=64, crop_h=64), [
        (dict(rec=P(3, 8), src=P(3, 8)), -1),
        (dict(rec=P(1, 10), src=P(1, 10)), -1),
        (dict(rec=P(2, 8), src=P(2, 8)), -1),
        (dict(src=P(2, 10)), -1),
        (dict(src=P(1, 10)), -1),
        (dict(rec=None), -1),
        (dict(src=None), -1),
        (dict(pli=1, xdec=2), -1),
        (dict(pli=1, ydec=-1), -1),
        (dict(blocks=None), -1),
        (dict(v_tally=None), -1),
        (dict(h_tally=None), -1),
    ]),
    ("r1_deblock_frame", dict(state=BUF, planes=(P(1, 8), P(1, 8), P(1, 8)), xdec=0, ydec=0, blocks=BUF, blocks_stride=16, blocks_cols=16, blocks_rows=16, crop_w=64, crop_h=64), [
        (dict(), 0),
        (dict(planes=(P(3, 8), P(3, 8), P(3, 8))), -1),
        (dict(planes=(P(1, 10), P(1, 10), P(1, 10))), -1),
        (dict(planes=(P(2, 8), P(2, 8), P(2, 8))), -1),
        (dict(planes=(P(1, 8), P(2, 10), P(1, 8))), -1),
        (dict(planes=(P(1, 8), P(1, 8), P(1, 10))), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(state=None), -1),
        (dict(planes=None), -1),
        (dict(blocks=None), -1),
    ]),
    ("r1_deblock_sse_frame", dict(rec=(P(1, 8), P(1, 8), P(1, 8)), src=(P(1, 8), P(1, 8), P(1, 8)), tallies=BUF, xdec=0, ydec=0, blocks=BUF, blocks_stride=16, blocks_cols=16, blocks_rows=16, crop_w=64, crop_h=64), [
        (dict(rec=(P(3, 8), P(3, 8), P(3, 8)), src=(P(3, 8), P(3, 8), P(3, 8))), -1),
        (dict(rec=(P(1, 10), P(1, 10), P(1, 10)), src=(P(1, 10), P(1, 10), P(1, 10))), -1),
        (dict(rec=(P(2, 8), P(2, 8), P(2, 8)), src=(P(2, 8), P(2, 8), P(2, 8))), -1),
        (dict(src=(P(1, 8), P(2, 10), P(1, 8))), -1),
        (dict(src=(P(1, 8), P(1, 8), P(1, 10))), -1),
        (dict(rec=(P(1, 8), P(2, 10), P(1, 8)), src=(P(1, 8), P(2, 10), P(1, 8))), -1),
        (dict(xdec=2), -1),
        (dict(ydec=-1), -1),
        (dict(rec=None), -1),
        (dict(src=None), -1),
        (dict(tallies=None), -1),
        (dict(blocks=None), -1),
    ]),
    ("r1_estimate_motion_batch", dict(tile=MEJOB(org=P(1, 8), ref=P(1, 8)), params=MEP(bd=8), cands=BUF, n=0, max_w=8, max_h=8, use_satd=0, filter_mode=0, out=BUF), [
        (dict(), 0),
        (dict(tile=MEJOB(org=P(3, 8), ref=P(3, 8))), -1),
        (dict(tile=MEJOB(org=P(1, 10), ref=P(1, 10))), 0),
        (dict(tile=MEJOB(org=P(2, 8), ref=P(2, 8))), 0),
        (dict(tile=MEJOB(org=P(1, 8), ref=P(2, 10))), -1),
        (dict(tile=MEJOB(org=P(1, 8), ref=P(1, 10))), 0),
        (dict(params=MEP(bd=9)), -1),
        (dict(tile=None), -1),
        (dict(params=None), -1),
        (dict(cands=None, n=0), 0),
        (dict(cands=None, n=1), -1),
        (dict(out=None, n=0), 0),
        (dict(out=None, n=1), -1),
    ]),
    ("r1_coeff_rate_batch", dict(qcoeffs=BUF, coeff_bytes=2, eobs=BUF, n=0, tx_type_mask=1, tx_size=1, plane=0, is_inter=0, use_reduced_tx_set=0, ctxs=BUF, cdfs=BUF, n_cdfs=1, rate_out=BUF, cul_level_out=None), [
        (dict(), 0),
        (dict(tx_size=19), -1),
        (dict(tx_size=-1), -1),
        (dict(qcoeffs=None, n=0), -1),
        (dict(qcoeffs=None, n=1), -1),
        (dict(eobs=None, n=0), -1),
        (dict(eobs=None, n=1), -1),
        (dict(ctxs=None, n=0), -1),
        (dict(ctxs=None, n=1), -1),
        (dict(cdfs=None, n=0), -1),
        (dict(cdfs=None, n=1), -1),
        (dict(rate_out=None, n=0), -1),
        (dict(rate_out=None, n=1), -1),
    ]),
    ("r1_segmentation_from_centroids", dict(centroids=BUF, base_q_idx=100, bit_depth=8, out=BUF), [
        (dict(), 0),
        (dict(bit_depth=9), -1),
        (dict(centroids=None), -1),
        (dict(out=None), -1),
    ]),
]


@pytest.fixture(scope="module")
def harness():
    return Harness()


def _rows():
    for name, base, cases in TABLE:
        for over, status in cases:
            yield pytest.param(name, base, over, status, id="%s-%s" % (name, fmt(over)[5:-1] or "valid"))


@pytest.mark.parametrize("name,base,over,status", _rows())
def test_status(harness, name, base, over, status):
    assert harness.call(name, base, over) == status


def test_table_covers_the_entry_points():
    names = [t[0] for t in TABLE]
    assert len(names) == len(set(names)) >= 40
    # every entry point with an early-out behind its checks has its valid set in the table
    assert sum(1 for _, _, cases in TABLE if cases and cases[0] == (dict(), 0)) >= 25

"""Host-side mirror of the reference's kernel interface over the batch C ABI.

Function names and argument meaning follow the reference (src/dist.rs,
src/mc.rs, src/transform/forward.rs); the difference is that every call takes a
whole candidate list.  All tensors live on the GPU (torch is the allocator and
stream provider only); descriptors are packed as the C structs of
include/rav1e_amd.h.
"""
import ctypes as C
from operator import itemgetter

import numpy as np
import torch

from . import _lib
from .types import (BLOCK_CHAIN_CTX, BLOCK_RATE_TRIAL, COEFF_CDF_CONTEXT, COEFF_CDFS, COEFF_RATE_INVALID, PICK_FIRST_MIN, PICK_TX_TYPE,  # noqa: F401
                    COEFF_NBR_CONTEXT, HEAD_BLOCK, HEAD_CDF_CONTEXT, HEAD_COMMIT, HEAD_NBR_CONTEXT, HEAD_TRIAL, MV_BLOCK, MV_QUERY, MV_STACK, MV_TRIAL, MVREF_MAX_QUERIES, MVREF_MAX_TILES, NBR_BLOCK, PART_BOTTOMUP, PART_PICK, PART_TOPDOWN, RD_PICK, TILE_BLOCK, TILE_BLOCKS, TX_DIMS, TXB_CHAIN_CTX, TXB_CTX, TxSize, valid_av1_transform)

DIST_CAND = np.dtype([("ox", "<i2"), ("oy", "<i2"), ("rx", "<i2"), ("ry", "<i2")])
MC_CAND = np.dtype([("rx", "<i2"), ("ry", "<i2"), ("col_frac", "u1"), ("row_frac", "u1"),
                    ("mode_x", "u1"), ("mode_y", "u1")])
INTRA_EDGE_CAND = np.dtype([("x", "<i2"), ("y", "<i2"), ("mode", "i1"), ("angle_delta", "i1"),
                            ("flags", "u1"), ("reserved", "u1")])
INTRA_CAND = np.dtype([("mode", "u1"), ("variant", "u1"), ("angle", "<i2"), ("ief", "u1"),
                       ("avail_w", "u1"), ("avail_h", "u1"), ("reserved", "u1")])
# R1IntraSplitCand: one intra block of r1_rdo_intra_split_batch
INTRA_SPLIT_CAND = np.dtype([("x", "<i2"), ("y", "<i2"), ("mode", "u1"), ("angle_delta", "i1"), ("ief", "u1"),
                             ("reserved", "u1"), ("tr_mask", "<u2"), ("bl_mask", "<u2")])
assert INTRA_SPLIT_CAND.itemsize == 12
CFL_AC_CAND = np.dtype([("x", "<i2"), ("y", "<i2"), ("w_pad", "u1"), ("h_pad", "u1"),
                        ("reserved", "u1", (2,))])
CDEF_DIR_CAND = np.dtype([("x", "<i2"), ("y", "<i2")])
CDEF_BLOCK_CAND = np.dtype([("x", "<i2"), ("y", "<i2"), ("pri_strength", "<i2"),
                            ("sec_strength", "<i2"), ("dir", "u1"), ("damping", "u1"),
                            ("edges", "u1"), ("reserved", "u1")])
EDGE_LEN = 257
RDO_CAND = np.dtype([("ox", "<i2"), ("oy", "<i2"), ("rx", "<i2"), ("ry", "<i2"),
                     ("col_frac", "u1"), ("row_frac", "u1"), ("mode_x", "u1"), ("mode_y", "u1"),
                     ("tx_type", "u1"), ("reserved", "u1", (3,))])
# R1CompoundCand: one two-reference candidate (r1_rdo_compound_cand_batch)
COMPOUND_CAND = np.dtype([("ox", "<i2"), ("oy", "<i2"), ("rx0", "<i2"), ("ry0", "<i2"), ("rx1", "<i2"), ("ry1", "<i2"),
                          ("col_frac0", "u1"), ("row_frac0", "u1"), ("col_frac1", "u1"), ("row_frac1", "u1"),
                          ("mode_x", "u1"), ("mode_y", "u1"), ("reserved", "u1", (2,))])
assert COMPOUND_CAND.itemsize == C.sizeof(_lib.R1CompoundCand)
# R1ScaleBlock: a coded block of r1_spatiotemporal_scale_batch (origin in 4x4 units, BlockSize)
SCALE_BLOCK = np.dtype([("bo_x", "<i4"), ("bo_y", "<i4"), ("bsize", "<i4")])
assert SCALE_BLOCK.itemsize == C.sizeof(_lib.R1ScaleBlock)


class R1Error(RuntimeError):
    pass


class Plane:
    """Plane<T> with v_frame 0.3.9's PlaneConfig layout, resident in HBM.

    xorigin / stride are rounded so row starts are 64-byte aligned; element
    (x, y) is data[(yorigin + y) * stride + xorigin + x]
    (src/tiling/plane_region.rs:185).  rav1e luma planes use 88 px of padding
    (src/frame/mod.rs:22-23)."""

    def __init__(self, width, height, bit_depth=8, xpad=88, ypad=88, device="cuda"):
        self.bpp = 1 if bit_depth == 8 else 2
        al = 64 // self.bpp
        self.width, self.height, self.bit_depth = width, height, bit_depth
        self.xpad, self.ypad = xpad, ypad
        self.xorigin = (xpad + al - 1) // al * al
        self.yorigin = ypad
        self.stride = (self.xorigin + width + xpad + al - 1) // al * al
        self.alloc_height = self.yorigin + height + ypad
        self.data = torch.zeros((self.alloc_height, self.stride), dtype=_pix_dtype(self.bpp), device=device)

    @classmethod
    def from_numpy(cls, arr, width, height, bit_depth, xpad, ypad, device="cuda"):
        """arr: the full (alloc_height, stride) host array of a HostPlane-style layout."""
        p = cls(width, height, bit_depth, xpad, ypad, device)
        assert arr.shape == (p.alloc_height, p.stride), (arr.shape, p.alloc_height, p.stride)
        src = arr if p.bpp == 1 else arr.view(np.int16)
        p.data.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        return p

    def cstruct(self):
        return _lib.R1Plane(self.data.data_ptr(), self.stride, self.alloc_height, self.width,
                            self.height, self.xorigin, self.yorigin, self.bpp, self.bit_depth)


ME_BLOCK_CAND = np.dtype([("bx", "<i2"), ("by", "<i2"), ("w", "u1"), ("h", "u1"), ("corner", "u1"),
                          ("reserved", "u1"), ("pmv", "<i2", (2, 2))])
ME_RESULT = np.dtype([("row", "<i2"), ("col", "<i2"), ("sad", "<u4"), ("cost", "<u8")])
assert ME_BLOCK_CAND.itemsize == 16 and ME_RESULT.itemsize == 16


CFL_ALPHA_CAND = np.dtype([("x", "<i2"), ("y", "<i2"), ("variant", "u1"), ("vis_w", "u1"), ("vis_h", "u1"),
                           ("reserved", "u1")])
SGR_SOLVE_UNIT = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "<i2"), ("h", "<i2"), ("set", "u1"), ("edges", "u1"),
                           ("reserved", "u1", (2,))])
SGR_EDGE_LEFT, SGR_EDGE_ABOVE = 1, 2   # R1_SGR_EDGE_*: see include/rav1e_amd.h, R1SgrSolveUnit
assert SGR_SOLVE_UNIT.itemsize == 12
# R1TrialUnit: a superblock whose restoration unit holds a self-guided choice (r1_cdef_lrf_trial_batch)
TRIAL_UNIT = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "<i2"), ("h", "<i2"), ("set", "u1"), ("edges", "u1"),
                       ("xqd", "i1", (2,)), ("sb", "<i4")])
assert TRIAL_UNIT.itemsize == 16


def me_lambdas(me_lambda):
    """lambda of the three ME passes by ssdec (src/me.rs:175-177): fi.me_lambda = sqrt(fi.lambda)."""
    return [int(me_lambda * 256.0 / (1 << (2 * ss)) * (0.5 if ss == 0 else 0.125)) for ss in range(3)]


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_cands(cands, dtype, n=None):
    """numpy structured array (or device uint8 tensor) -> (device byte tensor, n); n defaults to every
    record of the list"""
    if isinstance(cands, torch.Tensor):
        dc = cands
    else:
        a = np.ascontiguousarray(cands, dtype=dtype)
        dc = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
    return dc, dc.numel() // dtype.itemsize if n is None else n


def _scales_arg(scales):
    """an optional DistortionScale grid -> (pointer, row stride in elements) of the C calls"""
    return (None, 0) if scales is None else (scales.data_ptr(), scales.stride(0))


def _plane3(planes):
    """a list of 1 or 3 Planes -> the R1Plane[3] of the C calls (a single plane fills all three entries)"""
    return (_lib.R1Plane * 3)(*[(planes[k] if k < len(planes) else planes[0]).cstruct() for k in range(3)])


def _blocks_stride(blocks):
    """row stride, in R1DeblockBlock records, of a (rows, cols, 8) uint8 tensor of them (rows may be views)"""
    assert blocks.stride(2) == 1 and blocks.stride(1) == 8 and blocks.stride(0) % 8 == 0
    return blocks.stride(0) // 8


def _pix_dtype(bpp):
    """torch dtype of a pixel of `bpp` bytes (16-bit pixels are stored raw as int16)"""
    return torch.uint8 if bpp == 1 else torch.int16


def _coeff_dtype(bpp):
    """torch dtype of a transform coefficient of a plane of `bpp` bytes per pixel"""
    return torch.int16 if bpp == 1 else torch.int32


def _out_spec(*outs):
    """(key, shape letters, dtype) per output -> (key, shape getter, dtype); the getter maps a call's sizes to an
    int (one letter: torch.empty's fastest form) or a tuple"""
    return tuple((k, itemgetter(*shape), dtype) for k, shape, dtype in outs)


# The outputs of the fused-candidate wrappers in the order they are allocated.  Shape letters: n candidates, t the
# slots of the transform types (rdo_txsearch_batch), a the coded area min(w, 32) * min(h, 32), x = w * h, h and w the
# block; a dtype given as a function takes the plane's bytes per pixel.
_CAND_OUTS = _out_spec(("sad", "n", torch.int32), ("satd", "n", torch.int32), ("coeffs", "nx", _coeff_dtype),
                       ("pred", "nhw", _pix_dtype))
_COMPOUND_OUTS = _out_spec(("sad", "n", torch.int32), ("satd", "n", torch.int32), ("pred", "nhw", _pix_dtype))
_FULL_CAND_OUTS = _out_spec(("eob", "n", torch.int16), ("tx_dist", "n", torch.int64), ("sad", "n", torch.int32),
                            ("satd", "n", torch.int32), ("est_rate", "n", torch.int64),
                            ("qcoeffs", "na", _coeff_dtype), ("coeffs", "nx", _coeff_dtype))
_PIXEL_CAND_OUTS = _out_spec(("eob", "n", torch.int16), ("dist", "n", torch.int64), ("sad", "n", torch.int32),
                             ("satd", "n", torch.int32), ("qcoeffs", "na", _coeff_dtype), ("rec", "nhw", _pix_dtype))
_TXSEARCH_OUTS = _out_spec(("eob", "nt", torch.int16), ("dist", "nt", torch.int64), ("sad", "n", torch.int32),
                           ("satd", "n", torch.int32), ("est_rate", "nt", torch.int64),
                           ("qcoeffs", "nta", _coeff_dtype), ("rec", "nthw", _pix_dtype))

_INTRA_CAND_OUTS = _TXSEARCH_OUTS + _out_spec(("pred", "nhw", _pix_dtype))


_CUDA = torch.device("cuda")   # the current device, like "cuda", without parsing the string per allocation


def _bind_outs(outs, spec, wants, bpp, n, w, h, nt=1):
    """outs (a new dict if None) with every output of `spec` allocated that is wanted (wants[i] for spec[i]) and
    not in it yet"""
    o = outs if outs is not None else {}
    size = None
    for (k, shape, dtype), want in zip(spec, wants):
        if want and k not in o:
            size = size or {"n": n, "t": nt, "a": min(w, 32) * min(h, 32), "x": w * h, "h": h, "w": w}
            o[k] = torch.empty(shape(size), dtype=dtype(bpp) if callable(dtype) else dtype, device=_CUDA)
    return o


def _ptrs(o, *keys):
    """data pointers of o[k] for the keys, None where o has no such key"""
    return [o[k].data_ptr() if k in o else None for k in keys]


def _check_coeffs(qcoeffs, eobs, dtype=None):
    """a (qcoeffs, eobs) pair of the coefficient-rate calls: contiguous device tensors, int16 / int32 (or `dtype`) and
    two bytes per entry"""
    assert qcoeffs.is_cuda and qcoeffs.is_contiguous() and qcoeffs.dtype in ((dtype,) if dtype else (torch.int16, torch.int32))
    assert eobs.is_cuda and eobs.is_contiguous() and eobs.element_size() == 2


def _block_coeffs(qcoeffs_y, eobs_y, chroma, trials, blocks, bw, bh, tx_size, xdec, ydec):
    """The coefficient, trial and block arguments coeff_rate_block_batch and coeff_cdf_adapt_batch share: the arrays
    checked against the luma and the chroma transform size, the records on the device.
    -> (the four chroma pointers -- None each without chroma --, chroma transform blocks per plane, trials, n, blocks,
    n_blocks)"""
    from . import rdo_glue
    tw, th = TxSize(tx_size).dims
    _check_coeffs(qcoeffs_y, eobs_y)
    area = min(tw, 32) * min(th, 32)
    assert qcoeffs_y.numel() == eobs_y.numel() * area, (qcoeffs_y.numel(), eobs_y.numel(), area)
    uv_ptrs, n_uv = [None] * 4, 0
    if chroma is not None:
        qu, eu, qv, ev = chroma
        uw, uh = TxSize(rdo_glue.largest_chroma_tx_size(rdo_glue.block_size(bw, bh), xdec, ydec)).dims
        for q, e in ((qu, eu), (qv, ev)):
            _check_coeffs(q, e, qcoeffs_y.dtype)
            assert q.numel() == e.numel() * uw * uh and e.numel() == eu.numel(), (q.numel(), e.numel(), uw, uh)
        uv_ptrs, n_uv = [t.data_ptr() for t in (qu, eu, qv, ev)], eu.numel()
    dtr, n = _dev_cands(trials, BLOCK_RATE_TRIAL)
    dbl, n_blocks = _dev_cands(blocks, BLOCK_CHAIN_CTX)
    return uv_ptrs, n_uv, dtr, n, dbl, n_blocks


def _rd_pick_states(state, n=None):
    """state: a uint8 device tensor of RD_PICK records, n of them where the caller knows the count -> the count"""
    assert state.is_cuda and state.is_contiguous() and state.element_size() == 1
    assert n is None or state.numel() == n * RD_PICK.itemsize
    return state.numel() // RD_PICK.itemsize


def _bind_wanted(outs, spec, dev):
    """(a copy of outs with every wanted output of spec = {key: (want, shape, dtype)} allocated on dev that is not in
    it yet, the data pointers by key: None for an output that is not wanted, handed in or not)"""
    o = dict(outs) if outs else {}
    ptr = {}
    for k, (want, shape, dtype) in spec.items():
        if want and k not in o:
            o[k] = torch.empty(shape, dtype=dtype, device=dev)
        ptr[k] = o[k].data_ptr() if want else None
    return o, ptr


def segmentation_from_centroids(centroids, base_q_idx, bit_depth, lib=None):
    """r1_segmentation_from_centroids: a host function of the library (no context, no GPU); see
    Context.segmentation_from_centroids"""
    lib = lib or _lib.load()
    c = centroids.cpu().numpy() if isinstance(centroids, torch.Tensor) else centroids
    c = np.ascontiguousarray(c, dtype=np.int16)
    assert c.size == 48
    out = _lib.R1SegmentationData()
    rc = lib.r1_segmentation_from_centroids(c.ctypes.data, int(base_q_idx), int(bit_depth), C.byref(out))
    if rc != 0:
        raise R1Error("r1_segmentation_from_centroids failed (%d): %s" % (rc, lib.r1_last_error().decode()))
    return {"seg_delta": np.array(out.seg_delta[:], np.int16), "threshold": np.array(out.threshold[:], np.uint32),
            "min_segment": out.min_segment, "max_segment": out.max_segment, "k": out.k, "position": out.position}


class Context:
    """r1_ctx handle (one per process/GPU).  Thread-safe in the library."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise R1Error("rav1e_amd needs a HIP device; there is no CPU fallback")
        h = C.c_void_p()
        rc = self.lib.r1_ctx_create(device, C.byref(h))
        if rc != 0:
            raise R1Error("r1_ctx_create: %s" % self.lib.r1_last_error().decode())
        self.h = h

    def close(self):
        if self.h:
            self.lib.r1_ctx_destroy(self.h)
            self.h = None

    def _check(self, rc, what):
        if rc != 0:
            raise R1Error("%s failed (%d): %s" % (what, rc, self.lib.r1_last_error().decode()))

    # ---- dist:: ----
    def dist_batch(self, kind, org, ref, w, h, cands, n=None, out=None):
        """get_sad / get_satd (src/dist.rs:31,156) over a candidate list."""
        dc, n = _dev_cands(cands, DIST_CAND, n)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device="cuda")
        po, pr = org.cstruct(), ref.cstruct()
        self._check(self.lib.r1_dist_batch(self.h, int(kind), C.byref(po), C.byref(pr), w, h,
                                           dc.data_ptr(), n, out.data_ptr(), _stream_ptr()),
                    "r1_dist_batch")
        return out

    def dist_scaled_batch(self, kind, org, ref, w, h, cands, scales=None, xdec=0, ydec=0,
                          n=None, out=None):
        """sse_wxh (kind 2) / cdef_dist_wxh (kind 3) of src/rdo.rs:142-224 over a
        candidate list; scales: (rows, stride) int32 device tensor of Q14
        DistortionScale per 8x8 luma importance block, or None."""
        dc, n = _dev_cands(cands, DIST_CAND, n)
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device="cuda")
        po, pr = org.cstruct(), ref.cstruct()
        self._check(self.lib.r1_dist_scaled_batch(
            self.h, int(kind), C.byref(po), C.byref(pr), w, h, dc.data_ptr(), n, *_scales_arg(scales), xdec,
            ydec, out.data_ptr(), _stream_ptr()), "r1_dist_scaled_batch")
        return out

    # ---- transform::forward ----
    def forward_transform_batch(self, residual, tx_size, tx_type, bit_depth, coeff_bytes=None,
                                out=None):
        """forward_transform (src/transform/forward.rs:71) over n dense blocks.
        residual: int16 device tensor (n, h, w)."""
        w, h = TX_DIMS[int(tx_size)]
        n = residual.numel() // (w * h)
        if coeff_bytes is None:
            coeff_bytes = 2 if bit_depth == 8 else 4
        if out is None:
            out = torch.empty((n, w * h), dtype=torch.int16 if coeff_bytes == 2 else torch.int32,
                              device="cuda")
        self._check(self.lib.r1_fwd_txfm_batch(self.h, residual.data_ptr(), out.data_ptr(), n,
                                               int(tx_size), int(tx_type), bit_depth, coeff_bytes,
                                               _stream_ptr()), "r1_fwd_txfm_batch")
        return out

    # ---- transform::inverse ----
    def inverse_transform_add_batch(self, coeffs, pred, tx_size, tx_type, bit_depth, out=None):
        """inverse_transform_add (src/transform/inverse.rs:1633) over n blocks.
        coeffs: (n, stride) int16/int32 device tensor (stride >= coded area);
        pred: (n, h, w) pixels; returns the reconstruction (pass out=pred for
        the reference's in-place behaviour)."""
        w, h = TX_DIMS[int(tx_size)]
        n = pred.numel() // (w * h)
        bpp = 1 if bit_depth == 8 else 2
        if out is None:
            out = torch.empty_like(pred)
        self._check(self.lib.r1_inv_txfm_add_batch(
            self.h, coeffs.data_ptr(), coeffs.stride(0) if coeffs.dim() > 1 else coeffs.numel() // n,
            pred.data_ptr(), out.data_ptr(), n, int(tx_size), int(tx_type), bit_depth, bpp,
            _stream_ptr()), "r1_inv_txfm_add_batch")
        return out

    # ---- quantize:: ----
    @staticmethod
    def _qparams(qindex, bit_depth, is_intra, dc_delta_q=0, ac_delta_q=0):
        return _lib.R1QuantParams(int(qindex), int(bit_depth), int(bool(is_intra)), int(dc_delta_q),
                                  int(ac_delta_q))

    def quantize_batch(self, coeffs, tx_size, tx_type, qindex, bit_depth, is_intra,
                       dc_delta_q=0, ac_delta_q=0, want_rcoeffs=True):
        """QuantizationContext::quantize (+ dequantize) over n blocks
        (src/quantize/mod.rs:268-384).  coeffs: (n, stride) device tensor.
        -> dict(qcoeffs, eobs, rcoeffs) over the coded area."""
        w, h = TX_DIMS[int(tx_size)]
        area = min(w, 32) * min(h, 32)
        n = coeffs.shape[0]
        cb = coeffs.element_size()
        q = torch.empty((n, area), dtype=coeffs.dtype, device="cuda")
        r = torch.empty((n, area), dtype=coeffs.dtype, device="cuda") if want_rcoeffs else None
        eobs = torch.empty(n, dtype=torch.int16, device="cuda")
        qp = self._qparams(qindex, bit_depth, is_intra, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_quantize_batch(
            self.h, coeffs.data_ptr(), coeffs.stride(0), n, int(tx_size), int(tx_type), C.byref(qp),
            cb, q.data_ptr(), eobs.data_ptr(), r.data_ptr() if r is not None else None,
            _stream_ptr()), "r1_quantize_batch")
        return {"qcoeffs": q, "eobs": eobs, "rcoeffs": r}

    def quantize_rdo_batch(self, coeffs, tx_size, tx_type, qindex, bit_depth, is_intra,
                           dc_delta_q=0, ac_delta_q=0, want_rate=True):
        """quantize + dequantize + transform-domain distortion + estimate_rate
        (src/encoder.rs:1556-1650, src/rdo.rs:127-139) over n blocks; coeffs must
        hold the full w*h forward-transform output per block."""
        w, h = TX_DIMS[int(tx_size)]
        area = min(w, 32) * min(h, 32)
        n = coeffs.shape[0]
        q = torch.empty((n, area), dtype=coeffs.dtype, device="cuda")
        r = torch.empty((n, area), dtype=coeffs.dtype, device="cuda")
        eobs = torch.empty(n, dtype=torch.int16, device="cuda")
        dist = torch.empty(n, dtype=torch.int64, device="cuda")
        rate = torch.empty(n, dtype=torch.int64, device="cuda") if want_rate else None
        qp = self._qparams(qindex, bit_depth, is_intra, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_quantize_rdo_batch(
            self.h, coeffs.data_ptr(), coeffs.stride(0), n, int(tx_size), int(tx_type), C.byref(qp),
            coeffs.element_size(), q.data_ptr(), eobs.data_ptr(), r.data_ptr(), dist.data_ptr(),
            rate.data_ptr() if rate is not None else None, _stream_ptr()), "r1_quantize_rdo_batch")
        return {"qcoeffs": q, "eobs": eobs, "rcoeffs": r, "tx_dist": dist, "est_rate": rate}

    def dequantize_batch(self, qcoeffs, tx_size, qindex, bit_depth, dc_delta_q=0, ac_delta_q=0):
        """rust::dequantize (src/quantize/mod.rs:363-384) over n coded-area blocks."""
        n = qcoeffs.shape[0]
        r = torch.empty_like(qcoeffs)
        qp = self._qparams(qindex, bit_depth, 0, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_dequantize_batch(self.h, qcoeffs.data_ptr(), n, int(tx_size),
                                                 C.byref(qp), qcoeffs.element_size(),
                                                 r.data_ptr(), _stream_ptr()),
                    "r1_dequantize_batch")
        return r

    # ---- predict:: ----
    def intra_edges_batch(self, rec, tile, tx_size, cands, n=None):
        """get_intra_edges (src/partition.rs:639-898) for n transform blocks of
        one tile.  tile = (x, y, w, h) in plane pixels.  -> (edges (n, 257), lens (n, 2))"""
        dc, n = _dev_cands(cands, INTRA_EDGE_CAND, n)
        edges = torch.empty((n, EDGE_LEN), dtype=_pix_dtype(rec.bpp), device="cuda")
        lens = torch.empty((n, 2), dtype=torch.uint8, device="cuda")
        pr = rec.cstruct()
        self._check(self.lib.r1_intra_edges_batch(self.h, C.byref(pr), tile[0], tile[1], tile[2],
                                                  tile[3], int(tx_size), dc.data_ptr(), n,
                                                  edges.data_ptr(), EDGE_LEN, lens.data_ptr(),
                                                  _stream_ptr()), "r1_intra_edges_batch")
        return edges, lens

    def predict_intra_batch(self, tx_size, cands, edges, lens, bit_depth, ac=None, n=None, out=None):
        """dispatch_predict_intra (src/predict.rs:705-784) for n blocks -> (n, h, w) pixels (into `out` if given)."""
        w, h = TX_DIMS[int(tx_size)]
        dc, n = _dev_cands(cands, INTRA_CAND, n)
        bpp = 1 if bit_depth == 8 else 2
        if out is None:
            out = torch.empty((n, h, w), dtype=_pix_dtype(bpp), device="cuda")
        self._check(self.lib.r1_predict_intra_batch(
            self.h, int(tx_size), dc.data_ptr(), n, edges.data_ptr(), edges.stride(0),
            lens.data_ptr(), ac.data_ptr() if ac is not None else None, bit_depth, bpp,
            out.data_ptr(), _stream_ptr()), "r1_predict_intra_batch")
        return out

    def intra_satd_batch(self, src, tx_size, cands, group, pos_xy, edges, lens, ac=None, n=None):
        """the intra mode pre-screen (src/rdo.rs:1434-1506): predict `group` modes per block from
        one edge set, get_satd against the source block at pos_xy -> (n,) int32"""
        dc, n = _dev_cands(cands, INTRA_CAND, n)
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        ps = src.cstruct()
        self._check(self.lib.r1_intra_satd_batch(
            self.h, C.byref(ps), int(tx_size), dc.data_ptr(), n, group, pos_xy.data_ptr(),
            edges.data_ptr(), edges.stride(0), lens.data_ptr(),
            ac.data_ptr() if ac is not None else None, out.data_ptr(), _stream_ptr()),
            "r1_intra_satd_batch")
        return out

    def update_block_importances(self, intra_costs, future_importances, inter_costs, mvs, w, h, length,
                                 ref_importances):
        """update_block_importances after its SATD map (src/api/internal.rs:911-1068); device
        tensors: int32 (w*h) costs, float32 importances, int16 (w*h, 2) (row, col) motion vectors;
        ref_importances (float32) is updated in place"""
        need = self.lib.r1_update_block_importances_scratch_bytes(w, h) if w * h else 0
        if need < 0:
            raise R1Error("r1_update_block_importances_scratch_bytes failed")
        scratch = torch.empty(max(int(need), 256), dtype=torch.uint8, device="cuda")
        self._check(self.lib.r1_update_block_importances(
            self.h, intra_costs.data_ptr(), future_importances.data_ptr(), inter_costs.data_ptr(),
            mvs.data_ptr(), w, h, length, ref_importances.data_ptr(), scratch.data_ptr(),
            scratch.numel(), _stream_ptr()), "r1_update_block_importances")
        return ref_importances

    def frame_scales(self, intra_costs, block_importances, activity_scales=None):
        """distortion_scale_for per importance block + compute_spatiotemporal_scores (activity_scales given) or
        compute_temporal_scores (None) (src/api/internal.rs:1211-1230, src/encoder.rs:744-777).  Device tensors:
        int32 intra costs, float32 importances, int32 Q14 activity scales, all of one shape.  -> (distortion
        scales, spatiotemporal scores, stats): int32 tensors of that shape -- the first is the `scales` grid of the
        distortion entry points -- and a 24-byte uint8 tensor holding an R1ScaleStats (scale_stats reads it)"""
        n = intra_costs.numel()
        dist = torch.empty(intra_costs.shape, dtype=torch.int32, device="cuda")
        scores = torch.empty(intra_costs.shape, dtype=torch.int32, device="cuda")
        stats = torch.empty(C.sizeof(_lib.R1ScaleStats), dtype=torch.uint8, device="cuda")
        need = self.lib.r1_frame_scales_scratch_bytes(n)
        if need < 0:
            raise R1Error("r1_frame_scales_scratch_bytes failed")
        scratch = torch.empty(max(int(need), 256), dtype=torch.uint8, device="cuda")
        self._check(self.lib.r1_frame_scales(
            self.h, intra_costs.data_ptr(), block_importances.data_ptr(),
            activity_scales.data_ptr() if activity_scales is not None else None, n, dist.data_ptr(),
            scores.data_ptr(), stats.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream_ptr()),
            "r1_frame_scales")
        return dist, scores, stats

    @staticmethod
    def scale_stats(stats):
        """the R1ScaleStats of frame_scales on the host (synchronises): (log_sum_q11, inv_mean,
        log_isqrt_mean_scale)"""
        s = _lib.R1ScaleStats.from_buffer_copy(stats.cpu().numpy().tobytes())
        return s.log_sum_q11, s.inv_mean, s.log_isqrt_mean_scale

    def scale_kmeans(self, spatiotemporal):
        """the k-means of blog16(score) for k = 8 ... 3 (src/segmentation.rs:84-94, src/util/kmeans.rs) ->
        (6, 8) int16 device tensor, row r = k = 8 - r, unused entries 0"""
        n = spatiotemporal.numel()
        need = self.lib.r1_scale_kmeans_scratch_bytes(n)
        if need < 0:
            raise R1Error("r1_scale_kmeans_scratch_bytes failed")
        scratch = torch.empty(int(need), dtype=torch.uint8, device="cuda")
        out = torch.empty((6, 8), dtype=torch.int16, device="cuda")
        self._check(self.lib.r1_scale_kmeans(self.h, spatiotemporal.data_ptr(), n, out.data_ptr(),
                                             scratch.data_ptr(), scratch.numel(), _stream_ptr()), "r1_scale_kmeans")
        return out

    def segmentation_from_centroids(self, centroids, base_q_idx, bit_depth):
        """the rest of segmentation_optimize_inner + update_threshold (src/segmentation.rs:96-160,
        src/encoder.rs:566-580) on the host; centroids: the (6, 8) table (a device tensor is downloaded: the one
        synchronisation of the chain).  -> dict(seg_delta int16[8], threshold uint32[7], min_segment,
        max_segment, k, position)"""
        return segmentation_from_centroids(centroids, base_q_idx, bit_depth, self.lib)

    def spatiotemporal_scale_batch(self, distortion_scales, activity_scales, blocks, thresholds=None, min_segment=0):
        """spatiotemporal_scale + segment_idx_from_distortion (src/rdo.rs:464-504, src/segmentation.rs:180-196)
        per coded block.  distortion_scales / activity_scales (or None = 1.0): (h_in_imp_b, w_in_imp_b) int32
        device tensors; blocks: host SCALE_BLOCK records; thresholds: seven host values or None.
        -> (scale int32[n], sidx uint8[n]) device tensors"""
        h, w = distortion_scales.shape
        b = np.ascontiguousarray(blocks, dtype=SCALE_BLOCK)
        n = len(b)
        scale = torch.empty(n, dtype=torch.int32, device="cuda")
        sidx = torch.empty(n, dtype=torch.uint8, device="cuda")
        thr = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.uint32)
        assert thr is None or thr.size == 7
        self._check(self.lib.r1_spatiotemporal_scale_batch(
            self.h, distortion_scales.data_ptr(), activity_scales.data_ptr() if activity_scales is not None else None,
            w, h, b.ctypes.data, n, thr.ctypes.data if thr is not None else None, min_segment, scale.data_ptr(),
            sidx.data_ptr(), _stream_ptr()), "r1_spatiotemporal_scale_batch")
        return scale, sidx

    def prescreen_select_batch(self, keys, group, keep_head, k):
        """the selection step of the mode pre-screens (src/rdo.rs:1352-1357, 1504-1509): keys
        (n_groups * group,) int32 SATDs in the caller's candidate order -> (n_groups, k) uint8
        indices: the first keep_head candidates stay, the rest stably sorted by key, take k"""
        n_groups = keys.numel() // group
        out = torch.empty((n_groups, k), dtype=torch.uint8, device="cuda")
        self._check(self.lib.r1_prescreen_select_batch(self.h, keys.data_ptr(), n_groups, group,
                                                       keep_head, k, out.data_ptr(), _stream_ptr()),
                    "r1_prescreen_select_batch")
        return out

    def cfl_alpha_search_batch(self, src, tx_size, cands, edges, lens, ac, n=None):
        """rdo_cfl_alpha (src/rdo.rs:1593-1688) for one chroma plane -> (alpha int16, sse int64)"""
        dc, n = _dev_cands(cands, CFL_ALPHA_CAND, n)
        alpha = torch.empty(n, dtype=torch.int16, device="cuda")
        cost = torch.empty(n, dtype=torch.int64, device="cuda")
        ps = src.cstruct()
        self._check(self.lib.r1_cfl_alpha_search_batch(
            self.h, C.byref(ps), int(tx_size), dc.data_ptr(), n, edges.data_ptr(), edges.stride(0),
            lens.data_ptr(), ac.data_ptr(), alpha.data_ptr(), cost.data_ptr(), _stream_ptr()),
            "r1_cfl_alpha_search_batch")
        return alpha, cost

    def cfl_ac_batch(self, luma, bw, bh, xdec, ydec, cands, n=None):
        """pred_cfl_ac (src/predict.rs:1020-1063) -> (n, bh*bw) int16"""
        dc, n = _dev_cands(cands, CFL_AC_CAND, n)
        ac = torch.empty((n, bw * bh), dtype=torch.int16, device="cuda")
        pl = luma.cstruct()
        self._check(self.lib.r1_cfl_ac_batch(self.h, C.byref(pl), bw, bh, xdec, ydec, dc.data_ptr(),
                                             n, ac.data_ptr(), _stream_ptr()), "r1_cfl_ac_batch")
        return ac

    # ---- cdef:: ----
    def cdef_find_dir_batch(self, luma, cands, n=None):
        """cdef_find_dir (src/cdef.rs:84-143) -> (dir uint8, var int32)"""
        dc, n = _dev_cands(cands, CDEF_DIR_CAND, n)
        d = torch.empty(n, dtype=torch.uint8, device="cuda")
        v = torch.empty(n, dtype=torch.int32, device="cuda")
        pl = luma.cstruct()
        self._check(self.lib.r1_cdef_find_dir_batch(self.h, C.byref(pl), dc.data_ptr(), n,
                                                    d.data_ptr(), v.data_ptr(), _stream_ptr()),
                    "r1_cdef_find_dir_batch")
        return d, v

    def cdef_filter_block_batch(self, src, dst, xdec, ydec, cands, n=None):
        """cdef_filter_block (src/cdef.rs:198-298) for n blocks, src plane -> dst plane"""
        dc, n = _dev_cands(cands, CDEF_BLOCK_CAND, n)
        a, b = src.cstruct(), dst.cstruct()
        self._check(self.lib.r1_cdef_filter_block_batch(self.h, C.byref(a), C.byref(b), xdec, ydec,
                                                        dc.data_ptr(), n, _stream_ptr()),
                    "r1_cdef_filter_block_batch")

    @staticmethod
    def _cdef_params(y_strengths, uv_strengths, damping, bit_depth):
        prm = _lib.R1CdefParams()
        for i in range(8):
            prm.y_strengths[i] = int(y_strengths[i])
            prm.uv_strengths[i] = int(uv_strengths[i])
        prm.damping, prm.bit_depth = int(damping), int(bit_depth)
        return prm

    def cdef_filter_frame_plane(self, luma, src, dst, p, xdec, ydec, tile_w, tile_h, skip_mi,
                                cdef_index_sb, y_strengths, uv_strengths, damping, bit_depth):
        """cdef_filter_tile (src/cdef.rs:600-625) for plane p of the whole frame.
        skip_mi: (mi_rows, mi_cols) uint8 device tensor; cdef_index_sb: (sb_rows, sb_cols)."""
        prm = self._cdef_params(y_strengths, uv_strengths, damping, bit_depth)
        l, a, b = luma.cstruct(), src.cstruct(), dst.cstruct()
        self._check(self.lib.r1_cdef_filter_frame_plane(
            self.h, C.byref(l), C.byref(a), C.byref(b), p, xdec, ydec, tile_w, tile_h,
            skip_mi.data_ptr(), skip_mi.stride(0), skip_mi.shape[1], skip_mi.shape[0],
            cdef_index_sb.data_ptr(), cdef_index_sb.stride(0), C.byref(prm), _stream_ptr()),
            "r1_cdef_filter_frame_plane")

    def cdef_analyze_frame(self, luma, tile_w, tile_h, mi_cols, mi_rows):
        """cdef_analyze_superblock (src/cdef.rs:340-373) for every 8x8 luma block of the frame ->
        (dir uint8 [nby, nbx], var int32 [nby, nbx]); blocks outside mi_cols x mi_rows stay 0"""
        nbx, nby = ((tile_w + 63) // 64) * 8, ((tile_h + 63) // 64) * 8
        assert self.lib.r1_cdef_analyze_blocks(tile_w, tile_h) == nbx * nby
        d = torch.zeros((nby, nbx), dtype=torch.uint8, device="cuda")
        v = torch.zeros((nby, nbx), dtype=torch.int32, device="cuda")
        l = luma.cstruct()
        self._check(self.lib.r1_cdef_analyze_frame(self.h, C.byref(l), tile_w, tile_h, mi_cols, mi_rows,
                                                   d.data_ptr(), v.data_ptr(), _stream_ptr()),
                    "r1_cdef_analyze_frame")
        return d, v

    def cdef_filter_frame_plane_dirs(self, dirs, variances, src, dst, p, xdec, ydec, tile_w, tile_h,
                                     skip_mi, cdef_index_sb, y_strengths, uv_strengths, damping, bit_depth):
        """cdef_filter_superblock over the frame for plane p with the analysis of cdef_analyze_frame"""
        prm = self._cdef_params(y_strengths, uv_strengths, damping, bit_depth)
        a, b = src.cstruct(), dst.cstruct()
        self._check(self.lib.r1_cdef_filter_frame_plane_dirs(
            self.h, dirs.data_ptr(), variances.data_ptr(), C.byref(a), C.byref(b), p, xdec, ydec,
            tile_w, tile_h, skip_mi.data_ptr(), skip_mi.stride(0), skip_mi.shape[1], skip_mi.shape[0],
            cdef_index_sb.data_ptr(), cdef_index_sb.stride(0), C.byref(prm), _stream_ptr()),
            "r1_cdef_filter_frame_plane_dirs")

    def cdef_strength_search(self, rec, src, skip_mi, y_strengths, uv_strengths, damping, bit_depth,
                             n_idx, xdec, ydec, crop_w, crop_h, area_sb=(1, 1), scales=None,
                             dist_scale=(1 << 14, 1 << 14, 1 << 14)):
        """the CDEF leg of rdo_loop_decision (src/rdo.rs:2104-2560, no restoration filter): for
        every superblock and cdef_index < n_idx the ScaledDistortion of the filtered superblock
        against the source, and the first index of smallest cost.
        rec / src: lists of 1 or 3 Planes (whole frame; rec deblocked); skip_mi: (mi_rows, mi_cols)
        uint8 device tensor; scales: (h/8, w/8) int32 device tensor (Q14) or None.
        -> (err (n_sby, n_sbx, 8) int64 holding u64, best (n_sby, n_sbx) int8, -1 = skipped)"""
        prm = self._cdef_search_params(len(rec), y_strengths, uv_strengths, damping, bit_depth, n_idx, xdec, ydec, crop_w,
                                       crop_h, area_sb, dist_scale)
        mi_rows, mi_cols = skip_mi.shape
        n_sbx, n_sby = (mi_cols + 15) // 16, (mi_rows + 15) // 16
        pr = _plane3(rec)
        ps = _plane3(src)
        err = torch.empty((n_sby, n_sbx, 8), dtype=torch.int64, device="cuda")
        best = torch.empty((n_sby, n_sbx), dtype=torch.int8, device="cuda")
        scratch = torch.empty(self.lib.r1_cdef_strength_search_scratch_bytes(mi_cols, mi_rows),
                              dtype=torch.uint8, device="cuda")
        self._check(self.lib.r1_cdef_strength_search(
            self.h, pr, ps, skip_mi.data_ptr(), skip_mi.stride(0), mi_cols, mi_rows, *_scales_arg(scales),
            C.byref(prm), err.data_ptr(), best.data_ptr(), scratch.data_ptr(), _stream_ptr()),
            "r1_cdef_strength_search")
        return err, best

    def _cdef_search_params(self, n_planes, y_strengths, uv_strengths, damping, bit_depth, n_idx, xdec, ydec, crop_w,
                            crop_h, area_sb, dist_scale):
        prm = _lib.R1CdefSearchParams()
        for i in range(8):
            prm.y_strengths[i] = int(y_strengths[i])
            prm.uv_strengths[i] = int(uv_strengths[i])
        prm.damping, prm.bit_depth, prm.n_idx, prm.planes = int(damping), int(bit_depth), int(n_idx), n_planes
        prm.xdec, prm.ydec, prm.crop_w, prm.crop_h = int(xdec), int(ydec), int(crop_w), int(crop_h)
        prm.area_sb_w, prm.area_sb_h = int(area_sb[0]), int(area_sb[1])
        for i in range(3):
            prm.dist_scale[i] = int(dist_scale[i])
        return prm

    def cdef_lrf_trial_scratch(self, rec, skip_mi, n_idx, xdec, ydec):
        """the scratch of cdef_lrf_trial_batch (it holds every index' trial output as whole planes), to allocate once"""
        mi_rows, mi_cols = skip_mi.shape
        nb = self.lib.r1_cdef_lrf_trial_scratch_bytes(mi_cols, mi_rows, xdec if len(rec) == 3 else 0,
                                                      ydec if len(rec) == 3 else 0, rec[0].bpp, n_idx, len(rec))
        return torch.empty(nb, dtype=torch.uint8, device="cuda")

    def cdef_lrf_trial_batch(self, rec, cdef_cur, src, skip_mi, units, y_strengths, uv_strengths, damping, bit_depth,
                             n_idx, xdec, ydec, crop_w, crop_h, area_sb=(1, 1), scales=None,
                             dist_scale=(1 << 14, 1 << 14, 1 << 14), sb_sel=None, scratch=None, outs=None):
        """a later pass of rdo_loop_decision's CDEF leg (src/rdo.rs:2377-2560): every (superblock, cdef_index) trial
        with the restoration units' CURRENT choices applied to the trial's output before the error is taken.
        units: three TRIAL_UNIT arrays (Y, U, V; may be empty) -- the superblocks under a self-guided choice;
        cdef_cur: the working copy (cdef_apply_area) or None when no unit carries an edge flag.
        -> (err (n_sby, n_sbx, 8) int64, err_planes (n_sby, n_sbx, 8, 3) int64, best (n_sby, n_sbx) int8)"""
        prm = self._cdef_search_params(len(rec), y_strengths, uv_strengths, damping, bit_depth, n_idx, xdec, ydec, crop_w,
                                       crop_h, area_sb, dist_scale)
        mi_rows, mi_cols = skip_mi.shape
        n_sbx, n_sby = (mi_cols + 15) // 16, (mi_rows + 15) // 16
        cur = cdef_cur if cdef_cur is not None else rec
        pr = _plane3(rec)
        pc = _plane3(cur)
        ps = _plane3(src)
        if isinstance(units, tuple):          # (device byte tensor or None, (n_y, n_u, n_v)): uploaded once by the caller
            du, counts = units
            n_units = (C.c_int32 * 3)(*[int(v) for v in counts])
        else:
            us = [np.ascontiguousarray(u, TRIAL_UNIT) for u in units] + [np.zeros(0, TRIAL_UNIT)] * (3 - len(units))
            n_units = (C.c_int32 * 3)(*[len(u) for u in us])
            allu = np.concatenate(us)
            du = _dev_cands(allu, TRIAL_UNIT)[0] if len(allu) else None
        o = outs if outs is not None else {}
        if "err" not in o:
            o["err"] = torch.empty((n_sby, n_sbx, 8), dtype=torch.int64, device="cuda")
        if "err_planes" not in o:
            o["err_planes"] = torch.empty((n_sby, n_sbx, 8, 3), dtype=torch.int64, device="cuda")
        if "best" not in o:
            o["best"] = torch.empty((n_sby, n_sbx), dtype=torch.int8, device="cuda")
        err, errp, best = o["err"], o["err_planes"], o["best"]
        nb = self.lib.r1_cdef_lrf_trial_scratch_bytes(mi_cols, mi_rows, xdec if len(rec) == 3 else 0,
                                                      ydec if len(rec) == 3 else 0, rec[0].bpp, n_idx, len(rec))
        if scratch is None or scratch.numel() < nb:
            scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
        self._check(self.lib.r1_cdef_lrf_trial_batch(
            self.h, pr, pc, ps, skip_mi.data_ptr(), skip_mi.stride(0), mi_cols, mi_rows, *_scales_arg(scales),
            C.byref(prm), du.data_ptr() if du is not None else None, n_units,
            sb_sel.data_ptr() if sb_sel is not None else None, err.data_ptr(), errp.data_ptr(), best.data_ptr(),
            scratch.data_ptr(), _stream_ptr()), "r1_cdef_lrf_trial_batch")
        return err, errp, best

    def cdef_apply_area(self, rec, out, skip_mi, index_sb, y_strengths, uv_strengths, damping, bit_depth, n_idx, xdec,
                        ydec, crop_w, crop_h, area_sb=(1, 1)):
        """the CDEF working copy of every analysis area (src/rdo.rs:2546-2560): cdef_filter_superblock with
        index_sb[sby, sbx] (int8 device tensor; < 0 = unfiltered) from rec into out (lists of 1 or 3 Planes)"""
        prm = self._cdef_search_params(len(rec), y_strengths, uv_strengths, damping, bit_depth, n_idx, xdec, ydec, crop_w,
                                       crop_h, area_sb, (1 << 14,) * 3)
        mi_rows, mi_cols = skip_mi.shape
        pr = _plane3(rec)
        po = _plane3(out)
        scratch = torch.empty(self.lib.r1_cdef_strength_search_scratch_bytes(mi_cols, mi_rows),
                              dtype=torch.uint8, device="cuda")
        assert index_sb.dtype == torch.int8 and index_sb.is_contiguous()
        self._check(self.lib.r1_cdef_apply_area(
            self.h, pr, po, skip_mi.data_ptr(), skip_mi.stride(0), mi_cols, mi_rows, C.byref(prm),
            index_sb.data_ptr(), scratch.data_ptr(), _stream_ptr()), "r1_cdef_apply_area")
        return out

    # ---- frame glue ----
    def plane_pad(self, plane, w, h, xdec=0, ydec=0):
        """Plane::pad(w, h) in place (FramePad::pad, src/frame/mod.rs:76-86); w, h: frame size"""
        pl = plane.cstruct()
        self._check(self.lib.r1_plane_pad(self.h, C.byref(pl), w, h, xdec, ydec, _stream_ptr()),
                    "r1_plane_pad")
        return plane

    def plane_downsample(self, src, frame_w, frame_h, dec):
        """Plane::downsampled(frame_w, frame_h) (src/encoder.rs:476-477) -> new padded Plane of
        half the size and half the padding; dec: the NEW plane's decimation (1 half, 2 quarter)"""
        dst = Plane((src.width + 1) // 2, (src.height + 1) // 2, src.bit_depth, src.xpad // 2, src.ypad // 2)
        a, b = src.cstruct(), dst.cstruct()
        self._check(self.lib.r1_plane_downsample(self.h, C.byref(a), C.byref(b), frame_w, frame_h, dec, dec,
                                                 _stream_ptr()), "r1_plane_downsample")
        return dst

    # ---- lookahead cost maps ----
    def estimate_intra_costs(self, luma):
        """estimate_intra_costs (src/api/lookahead.rs:30-123) -> (h/8, w/8) int32"""
        hb, wb = luma.height // 8, luma.width // 8
        out = torch.empty((hb, wb), dtype=torch.int32, device="cuda")
        pl = luma.cstruct()
        self._check(self.lib.r1_estimate_intra_costs(self.h, C.byref(pl), out.data_ptr(),
                                                     _stream_ptr()), "r1_estimate_intra_costs")
        return out

    def estimate_inter_costs(self, org, ref, mvs):
        """SATD map of estimate_inter_costs (lookahead.rs:226-268); mvs: (h/8, w/8, 2)
        int16 device tensor of (row, col) in 1/8 pel"""
        hb, wb = org.height // 8, org.width // 8
        out = torch.empty((hb, wb), dtype=torch.int32, device="cuda")
        a, b = org.cstruct(), ref.cstruct()
        self._check(self.lib.r1_estimate_inter_costs(self.h, C.byref(a), C.byref(b), mvs.data_ptr(),
                                                     out.data_ptr(), _stream_ptr()),
                    "r1_estimate_inter_costs")
        return out

    def activity_scales(self, luma):
        """ActivityMask::from_plane + fill_scales (src/activity.rs:21-66) -> (variances, scales),
        uint32-valued int32 tensors (ceil(h/8), ceil(w/8))"""
        hb, wb = (luma.height + 7) // 8, (luma.width + 7) // 8
        var = torch.empty((hb, wb), dtype=torch.int32, device="cuda")
        sc = torch.empty((hb, wb), dtype=torch.int32, device="cuda")
        pl = luma.cstruct()
        self._check(self.lib.r1_activity_scales(self.h, C.byref(pl), var.data_ptr(), sc.data_ptr(),
                                                _stream_ptr()), "r1_activity_scales")
        return var, sc

    def importance_block_difference(self, org, ref):
        """estimate_importance_block_difference (lookahead.rs:125-180) -> f64"""
        out = torch.zeros(1, dtype=torch.int64, device="cuda")
        a, b = org.cstruct(), ref.cstruct()
        self._check(self.lib.r1_importance_block_difference(self.h, C.byref(a), C.byref(b),
                                                            out.data_ptr(), _stream_ptr()),
                    "r1_importance_block_difference")
        n = (org.height // 8) * (org.width // 8)
        return float(out.item()) / n

    # ---- mc:: ----
    def put_8tap_batch(self, ref, w, h, cands, n=None, out=None):
        dc, n = _dev_cands(cands, MC_CAND, n)
        if out is None:
            out = torch.empty((n, h, w), dtype=_pix_dtype(ref.bpp), device="cuda")
        pr = ref.cstruct()
        self._check(self.lib.r1_mc_put_batch(self.h, C.byref(pr), w, h, dc.data_ptr(), n,
                                             out.data_ptr(), _stream_ptr()), "r1_mc_put_batch")
        return out

    def prep_8tap_batch(self, ref, w, h, cands, n=None, out=None):
        dc, n = _dev_cands(cands, MC_CAND, n)
        if out is None:
            out = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
        pr = ref.cstruct()
        self._check(self.lib.r1_mc_prep_batch(self.h, C.byref(pr), w, h, dc.data_ptr(), n,
                                              out.data_ptr(), _stream_ptr()), "r1_mc_prep_batch")
        return out

    def mc_batch_mfma(self, ref, w, h, cands, prep=False, n=None, out=None):
        """put_8tap / prep_8tap with the horizontal pass on the matrix cores (csrc/mc_mfma.hip)"""
        dc, n = _dev_cands(cands, MC_CAND, n)
        if out is None:
            out = torch.empty((n, h, w), dtype=torch.int16 if prep else torch.uint8, device="cuda")
        pr = ref.cstruct()
        self._check(self.lib.r1_mc_batch_mfma(self.h, int(prep), C.byref(pr), w, h, dc.data_ptr(), n,
                                              out.data_ptr(), _stream_ptr()), "r1_mc_batch_mfma")
        return out

    def mc_avg_batch(self, tmp1, tmp2, w, h, bit_depth, out=None):
        n = tmp1.numel() // (w * h)
        bpp = 1 if bit_depth == 8 else 2
        if out is None:
            out = torch.empty((n, h, w), dtype=_pix_dtype(bpp), device="cuda")
        self._check(self.lib.r1_mc_avg_batch(self.h, tmp1.data_ptr(), tmp2.data_ptr(), w, h, n,
                                             bit_depth, bpp, out.data_ptr(), _stream_ptr()),
                    "r1_mc_avg_batch")
        return out

    def _bind_launch(self, name, args, keep):
        """entry point `name` bound to args: the returned closure is one ctypes call (args + the current
        stream) and an rc check; it keeps `keep` -- what args point into -- alive"""
        f = getattr(self.lib, name)

        def launch():
            rc = f(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            if rc != 0:
                self._check(rc, name)
            return keep
        return launch

    def prepare_rdo_cand(self, org, ref, w, h, dcands, n, outs):
        """Bind one fused-candidate launch once (descriptor and output tensors
        stay alive in the returned closure): the per-step host cost is then one
        ctypes call -- what a native caller of the C ABI pays -- instead of
        rebuilding the argument structs in Python every step."""
        po, pr = org.cstruct(), ref.cstruct()
        return self._bind_launch("r1_rdo_cand_batch", [
            self.h, C.byref(po), C.byref(pr), w, h, int(TxSize.by_dims(w, h)), dcands.data_ptr(), n,
            outs["sad"].data_ptr(), outs["satd"].data_ptr(), outs["coeffs"].data_ptr(), None], (po, pr, dcands, outs))

    def prepare_rdo_full_cand(self, org, ref, w, h, dcands, n, qindex, outs, is_intra=0):
        """prepare_rdo_cand for r1_rdo_full_cand_batch (outs: sad, satd, eob, tx_dist, est_rate)."""
        po, pr = org.cstruct(), ref.cstruct()
        qp = self._qparams(qindex, org.bit_depth, is_intra, 0, 0)
        return self._bind_launch("r1_rdo_full_cand_batch", [
            self.h, C.byref(po), C.byref(pr), w, h, int(TxSize.by_dims(w, h)), dcands.data_ptr(), n, C.byref(qp),
            outs["sad"].data_ptr(), outs["satd"].data_ptr(), outs["eob"].data_ptr(), outs["tx_dist"].data_ptr(),
            outs["est_rate"].data_ptr(), None, None], (po, pr, qp, dcands, outs))

    def rdo_full_cand_batch(self, org, ref, w, h, cands, qindex, is_intra=0, dc_delta_q=0,
                            ac_delta_q=0, n=None, want_sad=True, want_satd=True, want_rate=True,
                            want_qcoeffs=False, want_coeffs=False, outs=None):
        """mc -> sad/satd -> diff -> forward_transform -> quantize -> dequantize ->
        tx-domain distortion -> estimate_rate for every candidate, one launch."""
        tx_size = int(TxSize.by_dims(w, h))
        dc, n = _dev_cands(cands, RDO_CAND, n)
        o = _bind_outs(outs, _FULL_CAND_OUTS, (True, True, want_sad, want_satd, want_rate, want_qcoeffs, want_coeffs),
                       org.bpp, n, w, h)
        po, pr = org.cstruct(), ref.cstruct()
        qp = self._qparams(qindex, org.bit_depth, is_intra, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_rdo_full_cand_batch(
            self.h, C.byref(po), C.byref(pr), w, h, tx_size, dc.data_ptr(), n, C.byref(qp),
            *_ptrs(o, "sad", "satd", "eob", "tx_dist", "est_rate", "qcoeffs", "coeffs"), _stream_ptr()),
            "r1_rdo_full_cand_batch")
        return o

    # ---- me:: ----
    def estimate_tile_motion(self, jobs, w_in_b, h_in_b, bit_depth, lambdas, allow_hp=True,
                             allow_full_search=False, me_range_scale=1, launch_mode=0):
        """estimate_tile_motion (src/me.rs:153-218) for a list of independent
        (tile, reference frame) jobs.  Each job: dict(org=[Plane x3], ref=[Plane x3]
        (full, half, quarter resolution), stats=int32 tensor (rows, cols, 2) viewing the
        FrameMEStats array [(row | col << 16), normalized_sad], prev=tensor or None,
        tile=(x, y, w, h) luma px).  lambdas: per ssdec (see me_lambdas)."""
        n = len(jobs)
        arr = (_lib.R1MeJob * n)()
        rows, cols = jobs[0]["stats"].shape[:2]
        for j, job in enumerate(jobs):
            st = job["stats"]
            assert st.dtype == torch.int32 and st.shape == (rows, cols, 2) and st.is_contiguous()
            for l in range(3):
                arr[j].org[l] = job["org"][l].cstruct()
                arr[j].ref[l] = job["ref"][l].cstruct()
            arr[j].stats = st.data_ptr()
            pv = job.get("prev")
            arr[j].prev = pv.data_ptr() if pv is not None else None
            arr[j].tile_x, arr[j].tile_y, arr[j].tile_w, arr[j].tile_h = job["tile"]
        p = _lib.R1MeParams(w_in_b, h_in_b, cols, rows, bit_depth, int(allow_hp),
                            int(allow_full_search), me_range_scale,
                            (C.c_uint32 * 3)(*[int(v) for v in lambdas]), int(launch_mode))
        self._check(self.lib.r1_estimate_tile_motion_batch(self.h, arr, n, C.byref(p), _stream_ptr()),
                    "r1_estimate_tile_motion_batch")

    def estimate_frame_motion(self, jobs, w_in_b, h_in_b, bit_depth, lambdas, **kw):
        """The frame-level caller of estimate_tile_motion: enqueue, wait, and acknowledge.  If the
        persistent launch flagged a timed-out dependency wait (r1_me_status -> R1_ETIMEDOUT) the
        statistics are recomputed with launch_mode 1 (launch boundaries, no waits) -- the
        automatic fallback include/rav1e_amd.h describes.  `prev` of the jobs is untouched by a
        search, and a search overwrites every entry of its tile, so the re-issue is idempotent.
        -> the launch mode that produced the statistics."""
        mode = int(kw.pop("launch_mode", 0))
        self.estimate_tile_motion(jobs, w_in_b, h_in_b, bit_depth, lambdas, launch_mode=mode, **kw)
        ok, _, _ = self.me_status(wait=True)
        if ok:
            return mode
        if mode == 1:
            raise R1Error("r1_me_status flagged a launch_mode 1 call: " + self.lib.r1_last_error().decode())
        self.estimate_tile_motion(jobs, w_in_b, h_in_b, bit_depth, lambdas, launch_mode=1, **kw)
        ok, _, _ = self.me_status(wait=True)
        assert ok
        return 1

    def me_status(self, wait=True):
        """r1_me_status: (ok, first_failed_call, calls) -- the statistics of the persistent tile-ME
        launches are valid once this has reported ok after them (include/rav1e_amd.h)."""
        first, calls = C.c_ulonglong(0), C.c_ulonglong(0)
        rc = self.lib.r1_me_status(self.h, int(wait), C.byref(first), C.byref(calls))
        if rc not in (0, -5):
            self._check(rc, "r1_me_status")
        return rc == 0, int(first.value), int(calls.value)

    def estimate_motion_batch(self, job, cands, w_in_b, h_in_b, bit_depth, lambdas, max_w=64,
                              max_h=64, use_satd=True, filter_mode=0, allow_hp=True, n=None):
        """estimate_motion(.., Some(pmv), ..) of src/rdo.rs:1183-1196 for independent
        blocks (ME_BLOCK_CAND array) of one (tile, reference) job -> ME_RESULT tensor bytes."""
        arr = (_lib.R1MeJob * 1)()
        st = job["stats"]
        rows, cols = st.shape[:2]
        for l in range(3):
            arr[0].org[l] = job["org"][l].cstruct()
            arr[0].ref[l] = job["ref"][l].cstruct()
        arr[0].stats = st.data_ptr()
        pv = job.get("prev")
        arr[0].prev = pv.data_ptr() if pv is not None else None
        arr[0].tile_x, arr[0].tile_y, arr[0].tile_w, arr[0].tile_h = job["tile"]
        p = _lib.R1MeParams(w_in_b, h_in_b, cols, rows, bit_depth, int(allow_hp), 0, 1,
                            (C.c_uint32 * 3)(*[int(v) for v in lambdas]), 0)
        dc, n = _dev_cands(cands, ME_BLOCK_CAND, n)
        out = torch.empty(n * ME_RESULT.itemsize, dtype=torch.uint8, device="cuda")
        self._check(self.lib.r1_estimate_motion_batch(self.h, arr, C.byref(p), dc.data_ptr(), n, max_w,
                                                      max_h, int(use_satd), filter_mode,
                                                      out.data_ptr(), _stream_ptr()),
                    "r1_estimate_motion_batch")
        return out

    # ---- deblock:: ----
    def deblock_plane(self, state, plane, pli, xdec, ydec, blocks, crop_w, crop_h):
        """deblock_plane (src/deblock.rs:1294-1459), in place.  state: 24-byte R1DeblockState
        (numpy, host); blocks: uint8 device tensor (mi_rows, mi_cols, 8) of R1DeblockBlock."""
        pc = plane.cstruct()
        st = np.ascontiguousarray(state).view(np.uint8)
        assert st.size == 24 and blocks.dtype == torch.uint8 and blocks.shape[2] == 8
        self._check(self.lib.r1_deblock_plane(self.h, st.ctypes.data, C.byref(pc), pli, xdec, ydec,
                                              blocks.data_ptr(), _blocks_stride(blocks), blocks.shape[1],
                                              blocks.shape[0], crop_w, crop_h, _stream_ptr()),
                    "r1_deblock_plane")

    def deblock_sse_plane(self, rec, src, pli, xdec, ydec, blocks, crop_w, crop_h, tallies=None):
        """sse_plane (src/deblock.rs:1461-1542) -> int64 device tensor (2, 65): vertical, horizontal"""
        if tallies is None:
            tallies = torch.zeros((2, 65), dtype=torch.int64, device="cuda")
        pr, ps = rec.cstruct(), src.cstruct()
        self._check(self.lib.r1_deblock_sse_plane(self.h, C.byref(pr), C.byref(ps), pli, xdec, ydec,
                                                  blocks.data_ptr(), _blocks_stride(blocks), blocks.shape[1],
                                                  blocks.shape[0], crop_w, crop_h,
                                                  tallies[0].data_ptr(), tallies[1].data_ptr(),
                                                  _stream_ptr()), "r1_deblock_sse_plane")
        return tallies

    def deblock_frame(self, state, planes, xdec, ydec, blocks, crop_w, crop_h):
        """deblock_filter_frame (src/deblock.rs:1544-1551): the three planes in place, two launches"""
        arr = (_lib.R1Plane * 3)(*[p.cstruct() for p in planes])
        st = np.ascontiguousarray(state).view(np.uint8)
        assert st.size == 24 and blocks.dtype == torch.uint8 and blocks.shape[2] == 8
        self._check(self.lib.r1_deblock_frame(self.h, st.ctypes.data, arr, xdec, ydec, blocks.data_ptr(),
                                              _blocks_stride(blocks), blocks.shape[1], blocks.shape[0], crop_w,
                                              crop_h, _stream_ptr()), "r1_deblock_frame")

    def deblock_sse_frame(self, rec, src, xdec, ydec, blocks, crop_w, crop_h, tallies=None):
        """the level search of all planes and directions in one launch -> int64 (3, 2, 65)"""
        if tallies is None:
            tallies = torch.zeros((3, 2, 65), dtype=torch.int64, device="cuda")
        ra = (_lib.R1Plane * 3)(*[p.cstruct() for p in rec])
        sa = (_lib.R1Plane * 3)(*[p.cstruct() for p in src])
        self._check(self.lib.r1_deblock_sse_frame(self.h, ra, sa, xdec, ydec, blocks.data_ptr(),
                                                  _blocks_stride(blocks), blocks.shape[1], blocks.shape[0],
                                                  crop_w, crop_h, tallies.data_ptr(), _stream_ptr()),
                    "r1_deblock_sse_frame")
        return tallies

    def deblock_pick_levels(self, tallies, pli):
        """sse_optimize's tail on host copies of the tallies -> levels (2 for luma, 1 for chroma)"""
        t = np.ascontiguousarray(tallies.cpu().numpy())
        out = np.zeros(2, np.uint8)
        self._check(self.lib.r1_deblock_pick_levels(t[0].ctypes.data, t[1].ctypes.data, pli,
                                                    out.ctypes.data), "r1_deblock_pick_levels")
        return out[:2] if pli == 0 else out[:1]

    def rdo_pixel_cand_batch(self, org, ref, w, h, cands, qindex, dist_kind, scales=None, xdec=0,
                             ydec=0, is_intra=0, dc_delta_q=0, ac_delta_q=0, n=None, want_sad=True,
                             want_satd=True, want_qcoeffs=False, want_rec=False, outs=None, pred=None):
        """mc -> sad/satd -> diff -> forward_transform -> quantize -> dequantize -> inverse
        transform -> reconstruction -> weighted SSE / cdef_dist against the source, one launch.
        pred (dense (n, h, w) device tensor): r1_rdo_pred_cand_batch -- the prediction comes
        from that buffer instead of put_8tap(ref); dist_kind 0 = transform-domain distortion."""
        tx_size = int(TxSize.by_dims(w, h))
        dc, n = _dev_cands(cands, RDO_CAND, n)
        o = _bind_outs(outs, _PIXEL_CAND_OUTS, (True, True, want_sad, want_satd, want_qcoeffs, want_rec), org.bpp, n,
                       w, h)
        po = org.cstruct()
        qp = self._qparams(qindex, org.bit_depth, is_intra, dc_delta_q, ac_delta_q)
        # the two entry points differ in the prediction source only
        if pred is not None:
            name, src = "r1_rdo_pred_cand_batch", pred.data_ptr()
        else:
            name, src = "r1_rdo_pixel_cand_batch", C.byref(ref.cstruct())
        self._check(getattr(self.lib, name)(
            self.h, C.byref(po), src, w, h, tx_size, dc.data_ptr(), n, C.byref(qp), dist_kind, *_scales_arg(scales),
            xdec, ydec, *_ptrs(o, "sad", "satd", "eob", "dist", "qcoeffs", "rec"), _stream_ptr()), name)
        return o

    def tx_type_mask(self, tx_size, is_inter, use_reduced_set=False, rav1e_types_only=True):
        """av1_tx_used[get_tx_set(..)] (src/context/transform_unit.rs:37-44, 123-148) as a TxType bit
        mask, by default cut down to RAV1E_TX_TYPES (src/transform/mod.rs:28-44)"""
        return int(self.lib.r1_tx_type_mask(int(tx_size), int(bool(is_inter)), int(bool(use_reduced_set)),
                                            int(bool(rav1e_types_only))))

    def rdo_txsearch_batch(self, org, ref, w, h, cands, tx_type_mask, qindex, dist_kind, scales=None, xdec=0,
                           ydec=0, is_intra=0, dc_delta_q=0, ac_delta_q=0, n=None, want_sad=False,
                           want_satd=False, want_est_rate=False, want_qcoeffs=False, want_rec=False,
                           outs=None, pred=None):
        """r1_rdo_txsearch_batch: rdo_tx_type_decision's per-type loop (src/rdo.rs:1701-1817) on one
        prediction per candidate -- put_8tap(ref), or the dense `pred` (n, h, w) tensor when ref is None.
        eob / dist (/ est_rate): (n, nt); qcoeffs: (n, nt, coded area); rec: (n, nt, h, w); slot j = the
        j-th set bit of tx_type_mask."""
        tx_size = int(TxSize.by_dims(w, h))
        dc, n = _dev_cands(cands, RDO_CAND, n)
        o = _bind_outs(outs, _TXSEARCH_OUTS, (True, True, want_sad, want_satd, want_est_rate, want_qcoeffs, want_rec),
                       org.bpp, n, w, h, bin(int(tx_type_mask)).count("1"))
        po = org.cstruct()
        pr = ref.cstruct() if ref is not None else None
        qp = self._qparams(qindex, org.bit_depth, is_intra, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_rdo_txsearch_batch(
            self.h, C.byref(po), C.byref(pr) if pr is not None else None,
            pred.data_ptr() if pred is not None else None, w, h, tx_size, dc.data_ptr(), n, int(tx_type_mask),
            C.byref(qp), dist_kind, *_scales_arg(scales), xdec, ydec,
            *_ptrs(o, "sad", "satd", "eob", "dist", "est_rate", "qcoeffs", "rec"), _stream_ptr()),
            "r1_rdo_txsearch_batch")
        return o

    def rdo_intra_cand_batch(self, org, w, h, cands, pos_xy, edges, lens, tx_type_mask, qindex, dist_kind,
                             edge_group=1, ac=None, scales=None, xdec=0, ydec=0, is_intra=1, dc_delta_q=0,
                             ac_delta_q=0, n=None, want_sad=False, want_satd=False, want_est_rate=False,
                             want_qcoeffs=False, want_rec=False, want_pred=False, outs=None):
        """r1_rdo_intra_cand_batch: predict_intra_batch -> rdo_txsearch_batch(pred=...) in one launch, the prediction
        made on the CU.  cands: INTRA_CAND list; candidate i uses edge set / lens pair / pos_xy pair i // edge_group
        (edges, lens: intra_edges_batch's outputs; pos_xy: (n // edge_group, 2) int16 device tensor, the block
        positions in org) and AC block i of `ac`.  Outputs as rdo_txsearch_batch, + pred: (n, h, w)."""
        tx_size = int(TxSize.by_dims(w, h))
        # the library refuses UV_CFL_PRED without `ac` only where it can read the descriptors: before the upload
        if ac is None and isinstance(cands, np.ndarray) and (cands["mode"][:n] == 13).any():
            raise R1Error("r1_rdo_intra_cand_batch: a UV_CFL_PRED candidate needs `ac`")
        dc, n = _dev_cands(cands, INTRA_CAND, n)
        o = _bind_outs(outs, _INTRA_CAND_OUTS,
                       (True, True, want_sad, want_satd, want_est_rate, want_qcoeffs, want_rec, want_pred),
                       org.bpp, n, w, h, bin(int(tx_type_mask)).count("1"))
        po = org.cstruct()
        qp = self._qparams(qindex, org.bit_depth, is_intra, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_rdo_intra_cand_batch(
            self.h, C.byref(po), w, h, tx_size, dc.data_ptr(), n, int(edge_group), pos_xy.data_ptr(), edges.data_ptr(),
            edges.stride(0), lens.data_ptr(), ac.data_ptr() if ac is not None else None, int(tx_type_mask),
            C.byref(qp), dist_kind, *_scales_arg(scales), xdec, ydec,
            *_ptrs(o, "sad", "satd", "eob", "dist", "est_rate", "qcoeffs", "rec", "pred"), _stream_ptr()),
            "r1_rdo_intra_cand_batch")
        return o

    def rdo_intra_split_batch(self, org, rec, tile, bw, bh, tx_size, cands, tx_type_mask, qindex, dist_kind,
                              enable_intra_edge_filter=True, scales=None, is_intra=1, dc_delta_q=0, ac_delta_q=0,
                              n=None, want_est_rate=False, want_qcoeffs=False, want_rec=False, outs=None):
        """r1_rdo_intra_split_batch: write_tx_blocks' loop over the transform blocks of an intra block coded with
        tx_size < block size (rdo_tx_size_type's split depths), one launch, the working reconstruction on the CU.
        cands: INTRA_SPLIT_CAND list (rdo_glue.intra_split_cands), positions relative to tile = (x, y, w, h).
        Outputs, ntx = transform blocks per block, nt = set bits of tx_type_mask: eob (n, nt, ntx); dist (n, nt, ntx)
        under dist_kind 0 (with est_rate), else (n, nt); qcoeffs (n, nt, ntx, coded area); rec (n, nt, bh, bw)."""
        tw, th = TxSize(tx_size).dims
        ntx = max(1, bw // tw) * max(1, bh // th)
        # the library checks the descriptors only where it can read them: before the upload
        if isinstance(cands, np.ndarray):
            c = cands[:n]
            if (c["mode"] > 12).any() or ((c["x"] | c["y"]) & 3).any() or (c["x"] < 0).any() or (c["y"] < 0).any():
                raise R1Error("r1_rdo_intra_split_batch: a mode above 12 or a position that is no multiple of 4")
        dc, n = _dev_cands(cands, INTRA_SPLIT_CAND, n)
        nt = bin(int(tx_type_mask)).count("1")
        o = outs if outs is not None else {}
        spec = {"eob": ((n, nt, ntx), torch.int16), "dist": ((n, nt, ntx) if dist_kind == 0 else (n, nt), torch.int64)}
        if want_est_rate:
            spec["est_rate"] = ((n, nt, ntx), torch.int64)
        if want_qcoeffs:
            spec["qcoeffs"] = ((n, nt, ntx, min(tw, 32) * min(th, 32)), _coeff_dtype(org.bpp))
        if want_rec:
            spec["rec"] = ((n, nt, bh, bw), _pix_dtype(org.bpp))
        for k, (shape, dtype) in spec.items():
            if k not in o:
                o[k] = torch.empty(shape, dtype=dtype, device=_CUDA)
        po, pr = org.cstruct(), rec.cstruct()
        qp = self._qparams(qindex, org.bit_depth, is_intra, dc_delta_q, ac_delta_q)
        self._check(self.lib.r1_rdo_intra_split_batch(
            self.h, C.byref(po), C.byref(pr), *[int(v) for v in tile], bw, bh, int(tx_size), dc.data_ptr(), n,
            int(bool(enable_intra_edge_filter)), int(tx_type_mask), C.byref(qp), dist_kind, *_scales_arg(scales),
            *_ptrs(o, "eob", "dist", "est_rate", "qcoeffs", "rec"), _stream_ptr()), "r1_rdo_intra_split_batch")
        return o

    def coeff_rate_batch(self, qcoeffs, eobs, tx_type_mask, tx_size, plane, is_inter, ctxs, cdfs,
                         use_reduced_tx_set=False, want_cul_level=True, outs=None):
        """r1_coeff_rate_batch: the real rate of every (candidate, type) slot -- write_coeffs_lv_map
        (src/context/block_unit.rs:1783-2016) on a fresh WriterCounter against an unadapted copy of the slot's CDF
        snapshot, as rdo_tx_type_decision measures it (src/rdo.rs:1744-1799).
        qcoeffs / eobs: the (n, nt, coded area) int16 / int32 and (n, nt) uint16 device tensors the candidate calls
        write (rdo_txsearch_batch(want_qcoeffs=True), ...): chained on the current stream, no copy.
        ctxs: n TXB_CTX (NumPy array, or a uint8 device tensor (n, 4)); cdfs: COEFF_CDFS array (or a uint8 device tensor
        (n_cdfs, 1088)) of 1..256 snapshots.  -> {"rate": (n, nt) int32 holding uint32 1/8 bits (COEFF_RATE_INVALID
        for a slot with out-of-range device inputs), "cul_level": (n, nt) uint8}"""
        nt = bin(int(tx_type_mask)).count("1")
        _check_coeffs(qcoeffs, eobs)
        dctx, n = _dev_cands(ctxs, TXB_CTX)
        dcdf, n_cdfs = _dev_cands(cdfs, COEFF_CDFS)
        assert eobs.numel() == n * nt or nt == 0, (eobs.numel(), n, nt)      # (an empty mask: the library refuses it)
        o, ptr = _bind_wanted(outs, {"rate": (True, (n, nt), torch.int32),
                                     "cul_level": (want_cul_level, (n, nt), torch.uint8)}, qcoeffs.device)
        self._check(self.lib.r1_coeff_rate_batch(
            self.h, qcoeffs.data_ptr(), qcoeffs.element_size(), eobs.data_ptr(), n, int(tx_type_mask), int(tx_size),
            int(plane), int(bool(is_inter)), int(bool(use_reduced_tx_set)), dctx.data_ptr(), dcdf.data_ptr(),
            n_cdfs, ptr["rate"], ptr["cul_level"], _stream_ptr()), "r1_coeff_rate_batch")
        return o

    def coeff_rate_chain_batch(self, qcoeffs, eobs, tx_type_mask, bw, bh, tx_size, order, is_inter, chains, cdfs,
                               use_reduced_tx_set=False, want_txb_rate=True, want_cul_level=True, want_ctx=True,
                               outs=None):
        """r1_coeff_rate_chain_batch: the real luma coefficient rate of every (block, type) trial across the block's
        ntx = (bw / tw) * (bh / th) transform blocks in raster order -- write_coeffs_lv_map once per coded transform
        block on one WriterCounter, the CDFs and the neighbour contexts carried, as rdo_tx_size_type measures a
        transform depth (src/rdo.rs:725-802).
        qcoeffs / eobs: the int16 / int32 and 2-byte device tensors of n * nt * ntx transform blocks the candidate
        calls wrote, chained on the current stream, no copy: order 0 = [block][type][transform block]
        (rdo_intra_split_batch), order 1 = [block][transform block][type] (rdo_txsearch_batch over the blocks'
        transform blocks).  chains: n TXB_CHAIN_CTX (rdo_glue.txb_chain_ctx; NumPy array or a uint8 device tensor
        (n, 40)); cdfs: as coeff_rate_batch.
        -> {"rate": (n, nt) int32 holding uint32 1/8 bits (COEFF_RATE_INVALID for a trial with out-of-range device
        inputs), "txb_rate": (n, nt, ntx) int32, "cul_level": (n, nt, ntx) uint8, "ctx": (n, nt, 32) uint8 -- above[16],
        left[16] behind the last transform block}; the three side outputs are optional."""
        nt = bin(int(tx_type_mask)).count("1")
        tw, th = TxSize(tx_size).dims
        ntx = max(1, bw // tw) * max(1, bh // th)
        _check_coeffs(qcoeffs, eobs)
        dch, n = _dev_cands(chains, TXB_CHAIN_CTX)
        dcdf, n_cdfs = _dev_cands(cdfs, COEFF_CDFS)
        assert eobs.numel() == n * nt * ntx or nt == 0, (eobs.numel(), n, nt, ntx)
        o, ptr = _bind_wanted(outs, {
            "rate": (True, (n, nt), torch.int32), "txb_rate": (want_txb_rate, (n, nt, ntx), torch.int32),
            "cul_level": (want_cul_level, (n, nt, ntx), torch.uint8), "ctx": (want_ctx, (n, nt, 32), torch.uint8)},
            qcoeffs.device)
        self._check(self.lib.r1_coeff_rate_chain_batch(
            self.h, qcoeffs.data_ptr(), qcoeffs.element_size(), eobs.data_ptr(), n, int(tx_type_mask), int(bw), int(bh),
            int(tx_size), int(order), int(bool(is_inter)), int(bool(use_reduced_tx_set)), dch.data_ptr(),
            dcdf.data_ptr(), n_cdfs, ptr["rate"], ptr["txb_rate"], ptr["cul_level"], ptr["ctx"], _stream_ptr()),
            "r1_coeff_rate_chain_batch")
        return o

    def coeff_rate_block_batch(self, qcoeffs_y, eobs_y, step_y, chroma, step_uv, trials, bw, bh, tx_size, xdec, ydec,
                               is_inter, blocks, cdfs, use_reduced_tx_set=False, want_plane_rate=True, want_rng=True,
                               want_cul_level=True, want_ctx=True, outs=None):
        """r1_coeff_rate_block_batch: the real coefficient rate of a whole block per trial -- write_coeffs_lv_map over
        the luma transform blocks, then U's, then V's, on ONE counter that starts at the trial's handed-over rng, as
        write_tx_blocks / write_tx_tree with luma_only = false code them behind the head symbols of
        luma_chroma_mode_rdo (src/rdo.rs:855-945, src/encoder.rs:2202-2240).
        qcoeffs_y / eobs_y: the int16 / int32 and 2-byte device tensors of luma transform blocks a candidate call
        wrote; transform block k of a trial lies at first_y + k * step_y.  chroma: None (no trial has do_chroma) or
        (qcoeffs_u, eobs_u, qcoeffs_v, eobs_v), all of the chroma transform size and as many blocks each, at
        first_u / first_v + k * step_uv.  trials: n BLOCK_RATE_TRIAL (rdo_glue.block_rate_trial); blocks:
        BLOCK_CHAIN_CTX (rdo_glue.block_chain_ctx); cdfs: COEFF_CDFS, the luma and chroma slices -- each a NumPy array
        or a uint8 device tensor of the struct's bytes.
        -> {"rate": (n,) int32 holding uint32 1/8 bits (COEFF_RATE_INVALID for a trial with out-of-range device
        inputs), "plane_rate": (n, 3) int32, "rng": (n,) int16 holding uint16, "cul_level": (n, 3, 16) uint8,
        "ctx": (n, 3, 2, 16) uint8}; the four side outputs are optional."""
        uv_ptrs, n_uv, dtr, n, dbl, n_blocks = _block_coeffs(qcoeffs_y, eobs_y, chroma, trials, blocks, bw, bh, tx_size,
                                                             xdec, ydec)
        dcdf, n_cdfs = _dev_cands(cdfs, COEFF_CDFS)
        o, ptr = _bind_wanted(outs, {
            "rate": (True, (n,), torch.int32), "plane_rate": (want_plane_rate, (n, 3), torch.int32),
            "rng": (want_rng, (n,), torch.int16), "cul_level": (want_cul_level, (n, 3, 16), torch.uint8),
            "ctx": (want_ctx, (n, 3, 2, 16), torch.uint8)}, qcoeffs_y.device)
        self._check(self.lib.r1_coeff_rate_block_batch(
            self.h, qcoeffs_y.data_ptr(), eobs_y.data_ptr(), eobs_y.numel(), int(step_y), *uv_ptrs, n_uv, int(step_uv),
            qcoeffs_y.element_size(), dtr.data_ptr(), n, int(bw), int(bh), int(tx_size), int(xdec), int(ydec),
            int(bool(is_inter)), int(bool(use_reduced_tx_set)), dbl.data_ptr(), n_blocks, dcdf.data_ptr(), n_cdfs,
            ptr["rate"], ptr["plane_rate"], ptr["rng"], ptr["cul_level"], ptr["ctx"], _stream_ptr()),
            "r1_coeff_rate_block_batch")
        return o

    def coeff_cdf_slice_batch(self, contexts, tx_size, plane_type, is_inter, use_reduced_tx_set=False, out=None):
        """r1_coeff_cdf_slice_batch: the COEFF_CDFS slice of every context that the rate calls take for (tx_size,
        plane_type, is_inter, reduced set), cut on the device.  contexts: (n, 7872) uint8 device tensor of
        COEFF_CDF_CONTEXT records (rdo_glue.coeff_cdf_context), or a NumPy array of them.
        -> (n, 1088) uint8 device tensor: hand it to a rate call as `cdfs`, cdf_sel = the context's index"""
        dctx, n = _dev_cands(contexts, COEFF_CDF_CONTEXT)
        if out is None:
            out = torch.empty((n, COEFF_CDFS.itemsize), dtype=torch.uint8, device=dctx.device)
        assert out.is_cuda and out.is_contiguous() and out.element_size() == 1 and out.numel() == n * COEFF_CDFS.itemsize
        self._check(self.lib.r1_coeff_cdf_slice_batch(
            self.h, dctx.data_ptr(), n, int(tx_size), int(plane_type), int(bool(is_inter)), int(bool(use_reduced_tx_set)),
            out.data_ptr(), _stream_ptr()), "r1_coeff_cdf_slice_batch")
        return out

    def coeff_cdf_adapt_batch(self, qcoeffs_y, eobs_y, step_y, chroma, step_uv, trials, bw, bh, tx_size, xdec, ydec,
                              is_inter, blocks, contexts, use_reduced_tx_set=False, state=None, call_id=0,
                              want_rate=True, want_rng=True, want_ctx=True, outs=None):
        """r1_coeff_cdf_adapt_batch: the winner's replay -- what coeff_rate_block_batch does for every trial, on the
        slices of contexts[t], which is left adapted in place.  The coefficient, trial and block arguments are
        coeff_rate_block_batch's (trial arrays, or rd_commit_batch's winner arrays: first_y = s * 16, step 1 with
        win_stride = 16 * coded area).  contexts: (n, 7872) uint8 device tensor, one COEFF_CDF_CONTEXT per trial.
        state / call_id: the optional gate -- (n, 24) uint8 device tensor of RD_PICK; trial t acts only when
        state[t].best_call == call_id, else nothing of it is written.
        -> {"rate": (n,) int32 holding uint32, "rng": (n,) int16 holding uint16, "ctx": (n, 3, 2, 16) uint8}, all
        optional"""
        uv_ptrs, n_uv, dtr, n, dbl, n_blocks = _block_coeffs(qcoeffs_y, eobs_y, chroma, trials, blocks, bw, bh, tx_size,
                                                             xdec, ydec)
        assert isinstance(contexts, torch.Tensor) and contexts.is_cuda and contexts.is_contiguous() and \
            contexts.element_size() == 1 and contexts.numel() == n * COEFF_CDF_CONTEXT.itemsize, "one context per trial"
        if state is not None:
            _rd_pick_states(state, n)
        o, ptr = _bind_wanted(outs, {"rate": (want_rate, (n,), torch.int32), "rng": (want_rng, (n,), torch.int16),
                                     "ctx": (want_ctx, (n, 3, 2, 16), torch.uint8)}, qcoeffs_y.device)
        self._check(self.lib.r1_coeff_cdf_adapt_batch(
            self.h, qcoeffs_y.data_ptr(), eobs_y.data_ptr(), eobs_y.numel(), int(step_y), *uv_ptrs, n_uv, int(step_uv),
            qcoeffs_y.element_size(), dtr.data_ptr(), n, int(bw), int(bh), int(tx_size), int(xdec), int(ydec),
            int(bool(is_inter)), int(bool(use_reduced_tx_set)), dbl.data_ptr(), n_blocks, contexts.data_ptr(),
            state.data_ptr() if state is not None else None, int(call_id), ptr["rate"], ptr["rng"], ptr["ctx"],
            _stream_ptr()), "r1_coeff_cdf_adapt_batch")
        o["contexts"] = contexts
        return o

    @staticmethod
    def rd_pick_state(n):
        """n initial R1RdPick states -- (f64::MAX, 0, 0, -1, -1, -1): nothing kept yet -- as an (n, 24) uint8 device
        tensor (RD_PICK records; .cpu().numpy().view(RD_PICK) reads them)"""
        import sys
        st = np.zeros(n, RD_PICK)
        st["best_rd"], st["best_row"], st["best_slot"], st["best_call"] = sys.float_info.max, -1, -1, -1
        return torch.from_numpy(st.view(np.uint8).reshape(n, RD_PICK.itemsize)).cuda()

    def rd_pick_batch(self, rate, dist, state, group, nt, lam, rule=PICK_FIRST_MIN, call_id=0, rate_add=None,
                      want_invalid=False, outs=None):
        """r1_rd_pick_batch: compute_rd_cost (src/rdo.rs:718-723) of every trial and the reference's comparison, on
        the current stream behind the launches that made `rate` and `dist`, no copy.
        rate / rate_add: 4-byte device tensors of n_states * group * nt entries (uint32 1/8 bits; the rate calls'
        outputs as they lie), dist: 8-byte (uint64).  state: (n_states, 24) uint8 device tensor (rd_pick_state),
        updated in place.  rule: PICK_FIRST_MIN, or PICK_TX_TYPE (group == 1: rdo_tx_type_decision's loop with its
        early exit).  -> {"state": state, "invalid": (n_states,) uint8 when wanted}"""
        n = _rd_pick_states(state)
        for t, size in ((rate, 4), (dist, 8)) + (((rate_add, 4),) if rate_add is not None else ()):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == size and t.numel() == n * group * nt, \
                (t.shape, t.dtype, n, group, nt)
        o, ptr = _bind_wanted(outs, {"invalid": (want_invalid, (n,), torch.uint8)}, state.device)
        o["state"] = state
        self._check(self.lib.r1_rd_pick_batch(
            self.h, rate.data_ptr(), rate_add.data_ptr() if rate_add is not None else None, dist.data_ptr(), n,
            int(group), int(nt), float(lam), int(rule), int(call_id), state.data_ptr(), ptr["invalid"], _stream_ptr()),
            "r1_rd_pick_batch")
        return o

    def rd_commit_batch(self, state, call_id, group, nt, coeffs=None, ntx=1, order=0, side=None, rec_trials=None,
                        rec=None, pos_xy=None, store_w=None, store_h=None, outs=None):
        """r1_rd_commit_batch: for every state the call `call_id` won, the winner's results where the next step
        reads them; states won by another call or by none keep what `outs` holds.
        coeffs: (eobs, qcoeffs) as the candidate calls wrote them -- transform block k of trial t at t * ntx + k
        (order 0) or, group == 1, at (s * ntx + k) * nt + slot (order 1) -> outs["eob_win"] (n, 16) int16,
        outs["qcoeffs_win"] (n, win_stride) in the coefficients' type (allocated (n, ntx * coded area) when not handed
        in; the commits of several depths share one of the largest depth's stride).
        side: (trials, side_bytes) uint8 -> outs["side_win"] (n, side_bytes).
        rec_trials: (trials, bh, bw) dense blocks in the plane's pixel type -> `rec` (a Plane) at pos_xy ((n, 2) int16
        device tensor), clipped to store_w x store_h (the plane's visible size by default); blocks must not overlap."""
        n = _rd_pick_states(state)
        o = dict(outs) if outs else {}
        eobs = qc = None
        area = cbytes = stride = 0
        if coeffs is not None:
            eobs, qc = coeffs
            _check_coeffs(qc, eobs)
            assert qc.numel() % eobs.numel() == 0 and eobs.numel() == n * group * nt * ntx, (eobs.shape, n, group, nt, ntx)
            area, cbytes = qc.numel() // eobs.numel(), qc.element_size()
            if "eob_win" not in o:
                o["eob_win"] = torch.zeros((n, 16), dtype=torch.int16, device=state.device)
            if "qcoeffs_win" not in o:
                o["qcoeffs_win"] = torch.zeros((n, ntx * area), dtype=qc.dtype, device=state.device)
            qw = o["qcoeffs_win"]
            assert qw.dtype == qc.dtype and qw.dim() == 2 and qw.shape[0] == n and qw.stride(1) == 1, qw.shape
            assert o["eob_win"].is_contiguous() and o["eob_win"].numel() == n * 16 and o["eob_win"].element_size() == 2
            stride = qw.stride(0)
        side_bytes = 0
        if side is not None:
            assert side.is_cuda and side.is_contiguous() and side.element_size() == 1 and side.numel() % (n * group * nt) == 0
            side_bytes = side.numel() // (n * group * nt)
            if "side_win" not in o:
                o["side_win"] = torch.zeros((n, side_bytes), dtype=torch.uint8, device=state.device)
            assert o["side_win"].is_contiguous() and o["side_win"].numel() == n * side_bytes
        bw = bh = 0
        pr = None
        if rec_trials is not None:
            assert rec_trials.is_cuda and rec_trials.is_contiguous() and rec_trials.element_size() == rec.bpp
            bh, bw = rec_trials.shape[-2:]
            assert rec_trials.numel() == n * group * nt * bw * bh, (rec_trials.shape, n, group, nt)
            assert pos_xy.is_cuda and pos_xy.is_contiguous() and pos_xy.element_size() == 2 and pos_xy.numel() == 2 * n
            pr = rec.cstruct()
            store_w = rec.width if store_w is None else store_w
            store_h = rec.height if store_h is None else store_h
        self._check(self.lib.r1_rd_commit_batch(
            self.h, state.data_ptr(), n, int(call_id), int(group), int(nt), int(ntx), int(order), int(area), int(cbytes),
            eobs.data_ptr() if eobs is not None else None, qc.data_ptr() if qc is not None else None,
            side.data_ptr() if side is not None else None, int(side_bytes),
            rec_trials.data_ptr() if rec_trials is not None else None, int(bw), int(bh),
            C.byref(pr) if pr is not None else None, pos_xy.data_ptr() if rec_trials is not None else None,
            int(store_w or 0), int(store_h or 0), o["eob_win"].data_ptr() if eobs is not None else None,
            o["qcoeffs_win"].data_ptr() if eobs is not None else None, int(stride),
            o["side_win"].data_ptr() if side is not None else None, _stream_ptr()), "r1_rd_commit_batch")
        return o

    # ---- the partition decision on the device ----
    @staticmethod
    def part_pick_state(n, best_rd=None):
        """n initial R1PartPick states -- (f64::MAX, PARTITION_INVALID, -1, 0): nothing kept -- as an (n, 16) uint8
        device tensor (PART_PICK records; .cpu().numpy().view(PART_PICK) reads them).  best_rd: the costs a top-down
        node starts from (cached_block.rd_cost), per node"""
        import sys
        st = np.zeros(n, PART_PICK)
        st["best_rd"] = sys.float_info.max if best_rd is None else best_rd
        st["best_partition"], st["best_call"] = -1, -1
        return torch.from_numpy(st.view(np.uint8).reshape(n, PART_PICK.itemsize)).cuda()

    def rd_partition_pick_batch(self, state, partition, call_id, rule, lam, children, child_idx, enable_early_exit=True,
                                part_rate=None, must_split=None, parent=None, parent_idx=None):
        """r1_rd_partition_pick_batch: one partition type tried at every node of `state` ((n, 16) uint8 device tensor,
        part_pick_state; updated in place), on the current stream behind the children's chains, no copy.
        children: a 2-D uint8 device tensor of R1RdPick or R1PartPick records, one per row (a row begins with the
        child's best_rd; rows may be strided); child_idx: (n, 4) int32 device tensor of rows, -1 = absent.
        part_rate: (n,) 4-byte device tensor (uint32 1/8 bits) or None (the reference's 0.0 arm); must_split: (n,)
        uint8 or None; parent / parent_idx: the R1PartPick records whose best_rd is the nodes' ref_rd_cost and (n,)
        int32 rows into them, or None (f64::MAX).  Nothing is allocated.  -> state"""
        assert state.is_cuda and state.is_contiguous() and state.element_size() == 1 and state.numel() % PART_PICK.itemsize == 0
        n = state.numel() // PART_PICK.itemsize
        assert children.is_cuda and children.dim() == 2 and children.element_size() == 1 and children.stride(1) == 1
        assert child_idx.is_cuda and child_idx.is_contiguous() and child_idx.dtype == torch.int32 and child_idx.numel() == 4 * n
        for t, size in ((part_rate, 4), (must_split, 1), (parent_idx, 4)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.element_size() == size and t.numel() == n), t
        n_parent = 0
        if parent is not None:
            assert parent.is_cuda and parent.is_contiguous() and parent.element_size() == 1 and parent_idx is not None
            n_parent = parent.numel() // PART_PICK.itemsize
        self._check(self.lib.r1_rd_partition_pick_batch(
            self.h, state.data_ptr(), n, int(partition), int(call_id), int(rule), float(lam), int(bool(enable_early_exit)),
            part_rate.data_ptr() if part_rate is not None else None, children.data_ptr(), int(children.stride(0)),
            int(children.shape[0]), child_idx.data_ptr(), must_split.data_ptr() if must_split is not None else None,
            parent.data_ptr() if parent is not None else None, n_parent,
            parent_idx.data_ptr() if parent_idx is not None else None, _stream_ptr()), "r1_rd_partition_pick_batch")
        return state

    def part_select_batch(self, state, srcs, dst):
        """r1_part_select_batch: for every node whose best_call names one of `srcs` (a list of up to four 2-D device
        tensors, one row per node, or None; entry c belongs to call_id c), that row goes to the node's row of `dst`;
        every other row of dst stays.  A source that IS dst copies nothing.  Rows are multiples of 4 bytes.  -> dst"""
        assert state.is_cuda and state.is_contiguous() and state.element_size() == 1
        n = state.numel() // PART_PICK.itemsize
        assert dst.is_cuda and dst.dim() == 2 and dst.shape[0] == n and dst.stride(1) == 1
        row = dst.shape[1] * dst.element_size()
        live = [t for t in srcs if t is not None]
        for t in live:
            assert t.is_cuda and t.dim() == 2 and t.shape == dst.shape and t.dtype == dst.dtype and t.stride(1) == 1 and \
                t.stride(0) == live[0].stride(0), (t.shape, t.stride())
        ptrs = (C.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in srcs])
        src_stride = live[0].stride(0) * dst.element_size() if live else 0
        self._check(self.lib.r1_part_select_batch(
            self.h, state.data_ptr(), n, len(srcs), ptrs, src_stride, dst.data_ptr(), dst.stride(0) * dst.element_size(),
            row, _stream_ptr()), "r1_part_select_batch")
        return dst

    def part_select_rect_batch(self, state, src_planes, dst_plane, pos_xy, bw, bh, store_w=None, store_h=None):
        """r1_part_select_rect_batch: the node's bw x bh rectangle at pos_xy ((n, 2) int16 device tensor) from the plane
        of the winning trial (src_planes: a list of up to four Planes of dst_plane's geometry, or None; entry c belongs
        to call_id c) into dst_plane, clipped to store_w x store_h (the visible size by default).  Rectangles must not
        overlap.  -> dst_plane"""
        assert state.is_cuda and state.is_contiguous() and state.element_size() == 1
        n = state.numel() // PART_PICK.itemsize
        assert pos_xy.is_cuda and pos_xy.is_contiguous() and pos_xy.element_size() == 2 and pos_xy.numel() == 2 * n
        planes = (_lib.R1Plane * 4)(*[p.cstruct() if p is not None else _lib.R1Plane() for p in src_planes])
        pd = dst_plane.cstruct()
        self._check(self.lib.r1_part_select_rect_batch(
            self.h, state.data_ptr(), n, len(src_planes), planes, C.byref(pd), pos_xy.data_ptr(), int(bw), int(bh),
            int(dst_plane.width if store_w is None else store_w), int(dst_plane.height if store_h is None else store_h),
            _stream_ptr()), "r1_part_select_rect_batch")
        return dst_plane

    # ---- the coefficient neighbour contexts carried on the device ----
    @staticmethod
    def coeff_nbr_contexts(n):
        """n fresh R1CoeffNbrContext (BlockContext::new: all zero) as an (n, 3120) uint8 device tensor
        (COEFF_NBR_CONTEXT records; .cpu().numpy().view(COEFF_NBR_CONTEXT) reads them)"""
        return torch.zeros((n, COEFF_NBR_CONTEXT.itemsize), dtype=torch.uint8, device="cuda")

    @staticmethod
    def _nbr_contexts(contexts):
        assert isinstance(contexts, torch.Tensor) and contexts.is_cuda and contexts.is_contiguous() and \
            contexts.element_size() == 1 and contexts.numel() % COEFF_NBR_CONTEXT.itemsize == 0, "(n, 3120) uint8 on the device"
        return contexts.numel() // COEFF_NBR_CONTEXT.itemsize

    def coeff_nbr_gather_batch(self, contexts, descs, bw, bh, xdec, ydec, want_blocks=True, want_chains=False, outs=None):
        """r1_coeff_nbr_gather_batch: the BLOCK_CHAIN_CTX (and / or TXB_CHAIN_CTX) record of every desc, cut from
        contexts[desc.nbr] on the device -- rdo_glue.block_chain_ctx / txb_chain_ctx.  contexts: (n_contexts, 3120)
        uint8 device tensor; descs: NBR_BLOCK records (rdo_glue.nbr_block), a NumPy array or a uint8 device tensor.
        -> {"blocks": (n, 108) uint8, "chains": (n, 40) uint8}: hand them to the rate calls as `blocks` / `chains`"""
        n_ctx = self._nbr_contexts(contexts)
        dd, n = _dev_cands(descs, NBR_BLOCK)
        o, ptr = _bind_wanted(outs, {"blocks": (want_blocks, (n, BLOCK_CHAIN_CTX.itemsize), torch.uint8),
                                     "chains": (want_chains, (n, TXB_CHAIN_CTX.itemsize), torch.uint8)}, contexts.device)
        self._check(self.lib.r1_coeff_nbr_gather_batch(
            self.h, contexts.data_ptr(), n_ctx, dd.data_ptr(), n, int(bw), int(bh), int(xdec), int(ydec), ptr["blocks"],
            ptr["chains"], _stream_ptr()), "r1_coeff_nbr_gather_batch")
        return o

    def coeff_nbr_store_batch(self, contexts, descs, bw, bh, tx_size, xdec, ydec, ctx_in=None, state=None, call_id=0):
        """r1_coeff_nbr_store_batch: what every coded or skipped desc leaves on contexts[desc.nbr], in place --
        rdo_glue.coeff_nbr_store.  ctx_in: (n, 96) uint8 device bytes, the `ctx` output of coeff_rate_block_batch /
        coeff_cdf_adapt_batch or rd_commit_batch's side_win (None when every desc is skipped).  state / call_id: the
        optional gate, as coeff_cdf_adapt_batch.  Acting descs must name distinct contexts.  -> contexts"""
        n_ctx = self._nbr_contexts(contexts)
        dd, n = _dev_cands(descs, NBR_BLOCK)
        if ctx_in is not None:
            assert ctx_in.is_cuda and ctx_in.is_contiguous() and ctx_in.element_size() == 1 and ctx_in.numel() == n * 96
        if state is not None:
            _rd_pick_states(state, n)
        self._check(self.lib.r1_coeff_nbr_store_batch(
            self.h, dd.data_ptr(), n, int(bw), int(bh), int(tx_size), int(xdec), int(ydec),
            ctx_in.data_ptr() if ctx_in is not None else None, state.data_ptr() if state is not None else None,
            int(call_id), contexts.data_ptr(), n_ctx, _stream_ptr()), "r1_coeff_nbr_store_batch")
        return contexts

    def coeff_nbr_reset_left_batch(self, contexts, sel, planes=3):
        """r1_coeff_nbr_reset_left_batch: left[p][*] = 0, p < planes, on contexts[sel[i]] (reset_left_contexts'
        coefficient part at the start of a superblock row).  sel: indices, a sequence or an int32 device tensor."""
        n_ctx = self._nbr_contexts(contexts)
        if not isinstance(sel, torch.Tensor):
            sel = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(contexts.device)
        assert sel.is_cuda and sel.is_contiguous() and sel.element_size() == 4
        self._check(self.lib.r1_coeff_nbr_reset_left_batch(
            self.h, contexts.data_ptr(), n_ctx, sel.data_ptr(), sel.numel(), int(planes), _stream_ptr()),
            "r1_coeff_nbr_reset_left_batch")
        return contexts

    def rd_winner_tx_type_batch(self, state, call_id, tx_type_mask, is_inter, uv_tx_size, trials, eob_win=None, ntx=1):
        """r1_rd_winner_tx_type_batch: for every state the call `call_id` won, trials[s].tx_type = the best_slot-th type
        of tx_type_mask and, with is_inter, trials[s].uv_tx_type = rdo_glue.uv_tx_type_inter of it (DCT_DCT when the
        winner's ntx eobs in eob_win, rd_commit_batch's (n, 16), are all zero).  trials: (n, 24) uint8 device tensor of
        BLOCK_RATE_TRIAL, updated in place.  -> trials"""
        n = _rd_pick_states(state)
        assert isinstance(trials, torch.Tensor) and trials.is_cuda and trials.is_contiguous() and \
            trials.element_size() == 1 and trials.numel() == n * BLOCK_RATE_TRIAL.itemsize
        if eob_win is not None:
            assert eob_win.is_cuda and eob_win.is_contiguous() and eob_win.element_size() == 2 and eob_win.numel() == n * 16
        self._check(self.lib.r1_rd_winner_tx_type_batch(
            self.h, state.data_ptr(), n, int(call_id), int(tx_type_mask), int(bool(is_inter)), int(uv_tx_size),
            eob_win.data_ptr() if eob_win is not None else None, int(ntx), trials.data_ptr(), _stream_ptr()),
            "r1_rd_winner_tx_type_batch")
        return trials

    # ---- the intra head symbols on the device ----
    @staticmethod
    def head_nbr_contexts(n):
        """n fresh R1HeadNbrContext (BlockContext::new and a blocks array of DC_PRED: all zero) as an (n, 3640) uint8
        device tensor (HEAD_NBR_CONTEXT records; .cpu().numpy().view(HEAD_NBR_CONTEXT) reads them)"""
        return torch.zeros((n, HEAD_NBR_CONTEXT.itemsize), dtype=torch.uint8, device="cuda")

    @staticmethod
    def _head_contexts(nbrs, cdfs):
        for t, dt in ((nbrs, HEAD_NBR_CONTEXT), (cdfs, HEAD_CDF_CONTEXT)):
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.element_size() == 1 and \
                t.numel() % dt.itemsize == 0 and t.data_ptr() % 2 == 0, "(n, %d) uint8 on the device" % dt.itemsize
        return nbrs.numel() // HEAD_NBR_CONTEXT.itemsize, cdfs.numel() // HEAD_CDF_CONTEXT.itemsize

    @staticmethod
    def _head_decided(n, depth_state, tx_sizes, cfl_alpha):
        """the two optional inputs that carry what the device decided -> (depth_state pointer, host table, alpha pointer)"""
        assert (depth_state is None) == (tx_sizes is None)
        table = None
        if depth_state is not None:
            _rd_pick_states(depth_state, n)
            table = (C.c_uint8 * 3)(*[int(t) for t in tx_sizes])
        if cfl_alpha is not None:
            assert cfl_alpha.is_cuda and cfl_alpha.is_contiguous() and cfl_alpha.element_size() == 2 and cfl_alpha.numel() == 2 * n
        return (depth_state.data_ptr() if depth_state is not None else None, table,
                cfl_alpha.data_ptr() if cfl_alpha is not None else None)

    def intra_head_rate_batch(self, nbrs, cdfs, blocks, trials, depth_state=None, tx_sizes=None, cfl_alpha=None,
                              rng_into=None, outs=None):
        """r1_intra_head_rate_batch: what every intra mode trial writes in front of its coefficients, as rate_add of
        rd_pick_batch, on the current stream -- rdo_glue.head_symbols on the device.  nbrs: (n_nbrs, 3640) uint8 device
        tensor of HEAD_NBR_CONTEXT, cdfs: (n_cdfs, 2192) uint8 of HEAD_CDF_CONTEXT; blocks / trials: HEAD_BLOCK /
        HEAD_TRIAL records, NumPy arrays or uint8 device tensors.  depth_state / tx_sizes: (n, 24) RD_PICK states and
        the three TxSize of their call ids, in place of the trials' tx_size; cfl_alpha: (n, 2) int16 device tensor in
        place of their alphas.  rng_into: an (n, 24) uint8 device tensor of BLOCK_RATE_TRIAL whose rng fields take the
        writer's rng behind the head; otherwise the rng comes back as "rng" (n,) int16.
        -> {"rate_add": (n,) int32 (uint32 1/8 bits, 0xFFFFFFFF = refused), "rng": ...}"""
        n_nbrs, n_cdfs = self._head_contexts(nbrs, cdfs)
        db, n_blocks = _dev_cands(blocks, HEAD_BLOCK)
        dt, n = _dev_cands(trials, HEAD_TRIAL)
        ds, table, da = self._head_decided(n, depth_state, tx_sizes, cfl_alpha)
        o, ptr = _bind_wanted(outs, {"rate_add": (True, (n,), torch.int32), "rng": (rng_into is None, (n,), torch.int16)},
                              nbrs.device)
        rng_ptr, stride = ptr["rng"], 2
        if rng_into is not None:
            assert rng_into.is_cuda and rng_into.is_contiguous() and rng_into.element_size() == 1 and \
                rng_into.numel() == n * BLOCK_RATE_TRIAL.itemsize
            rng_ptr, stride = rng_into.data_ptr() + BLOCK_RATE_TRIAL.fields["rng"][1], BLOCK_RATE_TRIAL.itemsize
        self._check(self.lib.r1_intra_head_rate_batch(
            self.h, nbrs.data_ptr(), n_nbrs, cdfs.data_ptr(), n_cdfs, db.data_ptr(), n_blocks, dt.data_ptr(), n, ds, table,
            da, ptr["rate_add"], rng_ptr, stride, _stream_ptr()), "r1_intra_head_rate_batch")
        return o

    def partition_rate_batch(self, nbrs, cdfs, nodes, partitions, rng_in=None, want_rng=False, outs=None):
        """r1_partition_rate_batch: write_partition alone at every node (HEAD_BLOCK records whose bsize is the node's),
        partitions: (n,) uint8 PartitionType, rng_in: (n,) 2-byte device tensor or None (0x8000) -- rdo_glue.
        partition_symbol on the device.  -> {"part_rate": (n,) int32, what rd_partition_pick_batch takes as part_rate,
        "rng": (n,) int16 when wanted}"""
        n_nbrs, n_cdfs = self._head_contexts(nbrs, cdfs)
        dn, n = _dev_cands(nodes, HEAD_BLOCK)
        if not isinstance(partitions, torch.Tensor):
            partitions = torch.from_numpy(np.ascontiguousarray(partitions, dtype=np.uint8)).to(nbrs.device)
        assert partitions.is_cuda and partitions.is_contiguous() and partitions.element_size() == 1 and partitions.numel() == n
        if rng_in is not None:
            assert rng_in.is_cuda and rng_in.is_contiguous() and rng_in.element_size() == 2 and rng_in.numel() == n
        o, ptr = _bind_wanted(outs, {"part_rate": (True, (n,), torch.int32), "rng": (want_rng, (n,), torch.int16)}, nbrs.device)
        self._check(self.lib.r1_partition_rate_batch(
            self.h, nbrs.data_ptr(), n_nbrs, cdfs.data_ptr(), n_cdfs, dn.data_ptr(), partitions.data_ptr(), n,
            rng_in.data_ptr() if rng_in is not None else None, ptr["part_rate"], ptr["rng"], _stream_ptr()),
            "r1_partition_rate_batch")
        return o

    def intra_head_commit_batch(self, nbrs, cdfs, blocks, trials, commits, state, call_id, group, nt, depth_state=None,
                                tx_sizes=None, cfl_alpha=None):
        """r1_intra_head_commit_batch: for every state the call `call_id` won, the winner's head symbols adapt its
        HEAD_CDF_CONTEXT and its mode, skip, transform size and partition context go to its HEAD_NBR_CONTEXT, both in
        place -- rdo_glue.head_symbols / head_nbr_store on the device.  commits: HEAD_COMMIT records, one per state;
        trials: the array the rate call read (trial (s * group + best_row) * nt + best_slot is the winner); the
        decided inputs as there.  Acting states must name distinct contexts.  -> (nbrs, cdfs)"""
        n_nbrs, n_cdfs = self._head_contexts(nbrs, cdfs)
        db, n_blocks = _dev_cands(blocks, HEAD_BLOCK)
        dt, n_trials = _dev_cands(trials, HEAD_TRIAL)
        dc, n = _dev_cands(commits, HEAD_COMMIT)
        _rd_pick_states(state, n)
        ds, table, da = self._head_decided(n_trials, depth_state, tx_sizes, cfl_alpha)
        self._check(self.lib.r1_intra_head_commit_batch(
            self.h, nbrs.data_ptr(), n_nbrs, cdfs.data_ptr(), n_cdfs, db.data_ptr(), n_blocks, dt.data_ptr(), n_trials,
            dc.data_ptr(), state.data_ptr(), n, int(call_id), int(group), int(nt), ds, table, da, _stream_ptr()),
            "r1_intra_head_commit_batch")
        return nbrs, cdfs

    def head_nbr_reset_left_batch(self, nbrs, sel):
        """r1_head_nbr_reset_left_batch: left_partition and left_tx of nbrs[sel[i]] = 0 (the head part of
        reset_left_contexts at the start of a superblock row; left_mode / left_skip stay).  sel: indices, a sequence or
        an int32 device tensor."""
        assert nbrs.is_cuda and nbrs.is_contiguous() and nbrs.element_size() == 1 and nbrs.numel() % HEAD_NBR_CONTEXT.itemsize == 0
        if not isinstance(sel, torch.Tensor):
            sel = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(nbrs.device)
        assert sel.is_cuda and sel.is_contiguous() and sel.element_size() == 4
        self._check(self.lib.r1_head_nbr_reset_left_batch(
            self.h, nbrs.data_ptr(), nbrs.numel() // HEAD_NBR_CONTEXT.itemsize, sel.data_ptr(), sel.numel(), _stream_ptr()),
            "r1_head_nbr_reset_left_batch")
        return nbrs

    # ---- the MV reference stack and the tile's blocks array ----
    @staticmethod
    def tile_blocks(cols, rows, tile_x=0, tile_y=0, frame_cols=None, frame_rows=None, stride=None, cells=None):
        """One tile's (or branch's) blocks array: a dict with `cells`, a uint8 device tensor of rows * stride TILE_BLOCK
        records -- NOT initialised (tile_blocks_reset_batch) unless handed in -- and the fields of R1TileBlocks."""
        stride = cols if stride is None else int(stride)
        if cells is None:
            cells = torch.empty(rows * stride * TILE_BLOCK.itemsize, dtype=torch.uint8, device="cuda")
        return {"cells": cells, "stride": stride, "cols": int(cols), "rows": int(rows), "tile_x": int(tile_x),
                "tile_y": int(tile_y), "frame_cols": int(tile_x + cols if frame_cols is None else frame_cols),
                "frame_rows": int(tile_y + rows if frame_rows is None else frame_rows)}

    @staticmethod
    def _tile_descs(tiles):
        """tile_blocks dicts -> the HOST R1TileBlocks array of the C calls"""
        if len(tiles) > MVREF_MAX_TILES:
            raise ValueError("at most %d blocks arrays per call" % MVREF_MAX_TILES)
        d = np.zeros(len(tiles), TILE_BLOCKS)
        for k, t in enumerate(tiles):
            c = t["cells"]
            assert c.is_cuda and c.is_contiguous() and c.element_size() == 1
            assert c.numel() >= t["rows"] * t["stride"] * TILE_BLOCK.itemsize
            d[k] = (c.data_ptr(), t["stride"], t["cols"], t["rows"], t["tile_x"], t["tile_y"], t["frame_cols"],
                    t["frame_rows"], 0)
        return d

    def tile_blocks_reset_batch(self, tiles, sel=None):
        """r1_tile_blocks_reset_batch: Block::default() over the whole arrays tiles[sel[i]] (every one without sel) --
        rdo_glue.tile_blocks_default on the device"""
        d = self._tile_descs(tiles)
        s = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
        self._check(self.lib.r1_tile_blocks_reset_batch(
            self.h, d.ctypes.data, len(d), None if s is None else s.ctypes.data, len(d) if s is None else s.size,
            _stream_ptr()), "r1_tile_blocks_reset_batch")
        return tiles

    def tile_blocks_store_batch(self, tiles, blocks, trials, state=None, call_id=0, group=1, nt=1, n=None):
        """r1_tile_blocks_store_batch: what the winners leave in their arrays -- rdo_glue.tile_blocks_store on the device.
        blocks: MV_BLOCK records; trials: MV_TRIAL records; state: RD_PICK records (state s acts when its best_call ==
        call_id, on trial (s * group + best_row) * nt + best_slot), or None: desc s acts on trial s."""
        d = self._tile_descs(tiles)
        db, n_blocks = _dev_cands(blocks, MV_BLOCK)
        dt, n_trials = _dev_cands(trials, MV_TRIAL)
        if state is not None:
            n = _rd_pick_states(state, n)
        elif n is None:
            n = n_trials
        self._check(self.lib.r1_tile_blocks_store_batch(
            self.h, d.ctypes.data, len(d), db.data_ptr(), n_blocks, dt.data_ptr(), n_trials,
            None if state is None else state.data_ptr(), n, int(call_id), int(group), int(nt), _stream_ptr()),
            "r1_tile_blocks_store_batch")
        return tiles

    def mvref_stack_batch(self, tiles, blocks, queries, sign_bias, out=None, max_queries=None):
        """r1_mvref_stack_batch: find_mvrefs for every query of every block -- rdo_glue.find_mvrefs on the device, one
        wave per block.  blocks: MV_BLOCK records (query_off / n_queries name each block's run of `queries`, MV_QUERY
        records); sign_bias: fi.ref_frame_sign_bias, entry r - 1 for reference r.  Host arrays are checked here: a block
        with more than 64 queries is refused (ValueError); device arrays need max_queries.
        -> a uint8 device tensor of MV_STACK records, one per query (count 0xFF: the device refused the query)"""
        d = self._tile_descs(tiles)
        if not isinstance(blocks, torch.Tensor):
            blocks = np.ascontiguousarray(blocks, dtype=MV_BLOCK)
            most = int(blocks["n_queries"].max()) if blocks.size else 1
            if most > MVREF_MAX_QUERIES:
                raise ValueError("a block has %d queries: at most %d (one lane each)" % (most, MVREF_MAX_QUERIES))
            if max_queries is None:
                max_queries = max(most, 1)
        if max_queries is None:
            max_queries = MVREF_MAX_QUERIES
        db, n_blocks = _dev_cands(blocks, MV_BLOCK)
        dq, n_queries = _dev_cands(queries, MV_QUERY)
        if out is None:
            out = torch.empty(n_queries * MV_STACK.itemsize, dtype=torch.uint8, device="cuda")
        assert out.is_cuda and out.is_contiguous() and out.numel() >= n_queries * MV_STACK.itemsize
        bias = np.zeros(8, np.uint8)
        sb = np.asarray(sign_bias).astype(np.uint8).reshape(-1)
        bias[:min(sb.size, 8)] = sb[:8]
        self._check(self.lib.r1_mvref_stack_batch(
            self.h, d.ctypes.data, len(d), db.data_ptr(), n_blocks, dq.data_ptr(), n_queries, int(max_queries),
            bias.ctypes.data, out.data_ptr(), _stream_ptr()), "r1_mvref_stack_batch")
        return out

    def mvref_pmv_batch(self, stacks, pmv_out, stride, offset=0, n=None):
        """r1_mvref_pmv_batch: pmv[0], pmv[1] of stack q (rdo_glue.mvref_pmv) at byte offset + q * stride of the uint8
        device tensor pmv_out -- offset 8 and stride 16 fill the pmv of an ME_BLOCK_CAND array.  A refused stack writes
        nothing."""
        assert stacks.is_cuda and stacks.is_contiguous() and stacks.element_size() == 1
        assert pmv_out.is_cuda and pmv_out.is_contiguous() and pmv_out.element_size() == 1
        if n is None:
            n = stacks.numel() // MV_STACK.itemsize
        assert n == 0 or (offset >= 0 and offset + (n - 1) * stride + 8 <= pmv_out.numel())
        self._check(self.lib.r1_mvref_pmv_batch(self.h, stacks.data_ptr(), n, pmv_out.data_ptr() + int(offset), int(stride),
                                                _stream_ptr()), "r1_mvref_pmv_batch")
        return pmv_out

    # ---- lrf:: ----
    def lrf_sgrproj_plane(self, cdeffed, deblocked, out, ydec, crop_w, crop_h, frame_height, unit_size,
                          units, stripe_height):
        """lrf_filter_frame's Sgrproj arm for one plane (src/lrf.rs:1482-1585); units: uint8 device
        tensor (unit_rows, unit_cols, 4) of R1LrfUnit; `out` must already hold the CDEF output."""
        pc, pd, po = cdeffed.cstruct(), deblocked.cstruct(), out.cstruct()
        assert units.dtype == torch.uint8 and units.shape[2] == 4 and units.is_contiguous()
        self._check(self.lib.r1_lrf_sgrproj_plane(self.h, C.byref(pc), C.byref(pd), C.byref(po), ydec,
                                                  crop_w, crop_h, frame_height, unit_size,
                                                  units.shape[1], units.shape[0], stripe_height,
                                                  units.data_ptr(), _stream_ptr()),
                    "r1_lrf_sgrproj_plane")

    def sgrproj_solve_batch(self, cdeffed, inp, units, max_w=256, max_h=256):
        """sgrproj_solve (src/lrf.rs:847-1096) for (unit, set) pairs; units: SGR_SOLVE_UNIT array (`edges`: SGR_EDGE_* --
        the unit's place in its rdo_loop_decision area, rdo_glue.restoration_unit_edges) -> (n, 2) int8 xqd"""
        dc, n = _dev_cands(units, SGR_SOLVE_UNIT)
        scratch = torch.empty(n * 5, dtype=torch.int64, device="cuda")
        out = torch.empty((n, 2), dtype=torch.int8, device="cuda")
        pc, pi = cdeffed.cstruct(), inp.cstruct()
        self._check(self.lib.r1_sgrproj_solve_batch(self.h, C.byref(pc), C.byref(pi), dc.data_ptr(), n,
                                                    max_w, max_h, scratch.data_ptr(), out.data_ptr(),
                                                    _stream_ptr()), "r1_sgrproj_solve_batch")
        return out

    def lrf_search_batch(self, lrf_in, src, units, is_chroma=False, xdec=0, ydec=0, scales=None, dist_scale=1 << 14,
                         max_w=256, max_h=256):
        """the restoration leg of rdo_loop_decision for one plane (src/rdo.rs:2575-2763) but the rate:
        units: SGR_SOLVE_UNIT array (set 255 = the no-filter option; `edges` from rdo_glue.restoration_unit_edges, 0 for
        one unit per plane and area; list the sets of a unit next to each other); scales: 2-D int32/uint32 device
        tensor (one DistortionScale per 8x8 luma block) or None -> ((n, 2) int8 xqd, (n,) int64 err)"""
        dc, n = _dev_cands(units, SGR_SOLVE_UNIT)
        scratch = torch.empty(n * 6, dtype=torch.int64, device="cuda")
        xqd = torch.empty((n, 2), dtype=torch.int8, device="cuda")
        err = torch.empty(n, dtype=torch.int64, device="cuda")
        pc, ps = lrf_in.cstruct(), src.cstruct()
        self._check(self.lib.r1_lrf_search_batch(self.h, C.byref(pc), C.byref(ps), dc.data_ptr(), n, max_w, max_h,
                                                 int(bool(is_chroma)), xdec, ydec,
                                                 *_scales_arg(scales), int(dist_scale),
                                                 scratch.data_ptr(), xqd.data_ptr(), err.data_ptr(), _stream_ptr()),
                    "r1_lrf_search_batch")
        return xqd, err

    # ---- fused candidate ----
    def rdo_cand_batch(self, org, ref, w, h, cands, n=None, want_sad=True, want_satd=True,
                       want_coeffs=True, want_pred=False, outs=None):
        """mc -> sad/satd -> diff -> forward_transform for every candidate."""
        tx_size = int(TxSize.by_dims(w, h))
        dc, n = _dev_cands(cands, RDO_CAND, n)
        o = _bind_outs(outs, _CAND_OUTS, (want_sad, want_satd, want_coeffs, want_pred), org.bpp, n, w, h)
        po, pr = org.cstruct(), ref.cstruct()

        def p(k, want):   # unlike the other fused wrappers: NULL for an unwanted output even if outs holds it
            return o[k].data_ptr() if want else None
        self._check(self.lib.r1_rdo_cand_batch(self.h, C.byref(po), C.byref(pr), w, h, tx_size,
                                               dc.data_ptr(), n, p("sad", want_sad),
                                               p("satd", want_satd), p("coeffs", want_coeffs),
                                               p("pred", want_pred), _stream_ptr()),
                    "r1_rdo_cand_batch")
        return o

    def rdo_compound_cand_batch(self, org, ref0, ref1, w, h, cands, n=None, want_sad=False, want_satd=True,
                                want_pred=False, outs=None):
        """prep_8tap(ref0), prep_8tap(ref1) -> mc_avg -> sad / satd against the source for every two-reference
        candidate (COMPOUND_CAND), one launch; pred: (n, h, w) pixels, the `pred` input of rdo_pixel_cand_batch /
        rdo_txsearch_batch.  An output that is not wanted is a NULL pointer even if outs holds it."""
        dc, n = _dev_cands(cands, COMPOUND_CAND, n)
        wants = (want_sad, want_satd, want_pred)
        o = _bind_outs(outs, _COMPOUND_OUTS, wants, org.bpp, n, w, h)
        po, p0, p1 = org.cstruct(), ref0.cstruct(), ref1.cstruct()
        ptrs = [o[k].data_ptr() if want else None for k, want in zip(("sad", "satd", "pred"), wants)]
        self._check(self.lib.r1_rdo_compound_cand_batch(self.h, C.byref(po), C.byref(p0), C.byref(p1), w, h,
                                                        dc.data_ptr(), n, *ptrs, _stream_ptr()),
                    "r1_rdo_compound_cand_batch")
        return o

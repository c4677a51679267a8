"""Plane layouts and array strides the ABI admits but oracle_lib.HostPlane / api.Plane never produce.

include/rav1e_amd.h states no alignment for R1Plane: element (x, y) is data[(yorigin + y) * stride + xorigin + x].
relayout() rebuilds a HostPlane in one of two layouts, on the host (for the oracle) and on the device (for the
library), with the same visible pixels and the same padding content:

  "odd"    xorigin = xpad | 1, yorigin = ypad + 1, stride = the smallest odd number >= xorigin + width + xpad,
           and the device plane starts ONE ELEMENT past a 256-byte boundary: no row start is aligned to more
           than the element, and an 8-bit plane's rows start at odd byte addresses.
  "tight"  xorigin = xpad, yorigin = ypad, stride = xorigin + width + xpad; nothing rounded, base offset 0.

strided() does the same for the 2-D arrays that the ABI takes with a stride argument.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

GUARD = 256          # guard bytes before and behind a device plane
GUARD_BYTE = 0x5A
KINDS = ("odd", "tight")


def _torch_view(a):
    """numpy array -> an array of a dtype torch can hold (unsigned 16/32/64-bit as the signed type)"""
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return a.view(signed[a.dtype]) if a.dtype in signed else a


class DevicePlane:
    """What api.py reads of a Plane (data, cstruct(), bpp, geometry), over a byte buffer with guards."""

    def __init__(self, host, base_off):
        import torch
        self.bpp, self.bit_depth = host.bpp, host.bit_depth
        self.width, self.height = host.width, host.height
        self.xpad, self.ypad = host.xpad, host.ypad
        self.xorigin, self.yorigin = host.xorigin, host.yorigin
        self.stride, self.alloc_height = host.stride, host.alloc_height
        self.nbytes = self.alloc_height * self.stride * self.bpp
        self.off = GUARD + base_off * self.bpp
        self.buf = torch.full((self.off + self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        body = self.buf[self.off:self.off + self.nbytes]
        self.data = (body if self.bpp == 1 else body.view(torch.int16)).view(self.alloc_height, self.stride)
        self.upload(host)

    def upload(self, host):
        import torch
        self.data.copy_(torch.from_numpy(_torch_view(np.ascontiguousarray(host.data))))

    def cstruct(self):
        from rav1e_amd import _lib
        return _lib.R1Plane(self.data.data_ptr(), self.stride, self.alloc_height, self.width, self.height,
                            self.xorigin, self.yorigin, self.bpp, self.bit_depth)

    def host(self):
        """the whole allocation, padding and the bytes between rows included, as the host plane's dtype"""
        a = self.data.cpu().numpy()
        return a if self.bpp == 1 else a.view(np.uint16)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.off] == GUARD_BYTE).all() and (b[self.off + self.nbytes:] == GUARD_BYTE).all())


def guards_intact(*planes):
    return all(p.guards_intact() for p in planes)


def host_relayout(hp, kind, xpad, ypad):
    """the host half of relayout(): a HostPlane in layout `kind` holding hp's visible pixels and xpad x ypad of
    its padding; what the layout adds beyond that (a column, a row, the end of each row) holds seeded noise"""
    assert kind in KINDS
    assert xpad <= hp.xorigin and ypad <= hp.yorigin
    assert hp.xorigin + hp.width + xpad <= hp.stride and hp.yorigin + hp.height + ypad <= hp.alloc_height
    p = O.HostPlane.__new__(O.HostPlane)
    p.bpp, p.bit_depth, p.width, p.height = hp.bpp, hp.bit_depth, hp.width, hp.height
    p.xpad, p.ypad = xpad, ypad
    if kind == "odd":
        p.xorigin, p.yorigin = xpad | 1, ypad + 1
        p.stride = (p.xorigin + p.width + xpad) | 1
    else:
        p.xorigin, p.yorigin = xpad, ypad
        p.stride = p.xorigin + p.width + xpad
    p.alloc_height = p.yorigin + p.height + ypad
    rng = np.random.default_rng(p.stride * 131 + p.alloc_height)
    p.data = rng.integers(0, 1 << p.bit_depth, size=(p.alloc_height, p.stride), dtype=hp.data.dtype)
    p.data[p.yorigin - ypad:p.yorigin + p.height + ypad, p.xorigin - xpad:p.xorigin + p.width + xpad] = \
        hp.data[hp.yorigin - ypad:hp.yorigin + hp.height + ypad, hp.xorigin - xpad:hp.xorigin + hp.width + xpad]
    return p


def relayout(hp, kind, xpad, ypad):
    """HostPlane -> (host plane, device plane) in layout `kind` (see the module text)"""
    p = host_relayout(hp, kind, xpad, ypad)
    return p, DevicePlane(p, 1 if kind == "odd" else 0)


def device_like(hp):
    """a guarded device plane in hp's own layout (for the plane of a call that keeps the HostPlane layout)"""
    return DevicePlane(hp, 0)


def host_strided(a, extra, poison):
    """(rows, cols, ...) array -> a view of it inside a (rows, cols + extra, ...) array whose other columns hold
    `poison`; `.base` is the whole array.  The row stride of the view is cols + extra entries."""
    a = np.asarray(a)
    assert a.ndim >= 2 and extra > 0
    big = np.empty((a.shape[0], a.shape[1] + extra) + a.shape[2:], a.dtype)
    big[...] = poison
    big[:, :a.shape[1]] = a
    v = big[:, :a.shape[1]]
    assert v.base is big
    return v


def strided(a, extra, poison):
    """host_strided() and a device tensor view of the same bytes -> (host view, device view)"""
    import torch
    v = host_strided(a, extra, poison)
    dbig = torch.from_numpy(_torch_view(v.base)).cuda()
    return v, dbig[:, :a.shape[1]]


def strided_out(rows, cols, extra, dtype):
    """a device output of `rows` records of `cols` entries, `extra` guard entries of 0x5A bytes behind each ->
    (device view (rows, cols), the whole device tensor (rows, cols + extra))"""
    import torch
    big = torch.empty((rows, cols + extra), dtype=dtype, device="cuda")
    big.view(torch.uint8).fill_(GUARD_BYTE)
    return big[:, :cols], big


def gap_intact(big, cols):
    """the guard entries of a strided_out() tensor still hold 0x5A bytes"""
    g = np.ascontiguousarray(big[:, cols:].cpu().numpy())
    return bool((g.view(np.uint8) == GUARD_BYTE).all())


# ---- the oracle calls both layout modules make (host planes in any layout, arrays dense or host_strided) ----
def window(hp, xpad=0, ypad=0):
    """the visible area of a host plane and xpad x ypad of its padding: what two layouts of one plane share"""
    return hp.data[hp.yorigin - ypad:hp.yorigin + hp.height + ypad, hp.xorigin - xpad:hp.xorigin + hp.width + xpad]


def row_stride(a):
    """row stride of a 2-D (or (rows, cols, k) record) host array in entries of its second axis"""
    assert a.strides[0] % a.strides[1] == 0
    return a.strides[0] // a.strides[1]


def planes3(planes):
    return (O.Plane * 3)(*[planes[min(k, len(planes) - 1)].cstruct() for k in range(3)])


def o_dist(L, kind, a, b, w, h, c):
    out = np.zeros(len(c), np.uint32)
    pa, pb = a.cstruct(), b.cstruct()
    assert L.r1o_dist_batch(kind, C.byref(pa), C.byref(pb), w, h, O.ptr(c), len(c), O.ptr(out)) == 0
    return out


def o_dist_scaled(L, kind, a, b, w, h, c, scales, xdec=0, ydec=0):
    out = np.zeros(len(c), np.uint64)
    pa, pb = a.cstruct(), b.cstruct()
    assert L.r1o_dist_scaled_batch(kind, C.byref(pa), C.byref(pb), w, h, O.ptr(c), len(c), scales.ctypes.data,
                                   row_stride(scales), xdec, ydec, O.ptr(out)) == 0
    return out


def o_mc(L, a, w, h, c):
    """-> (put, prep)"""
    put = np.zeros((len(c), h, w), a.data.dtype)
    prep = np.zeros((len(c), h, w), np.int16)
    pa = a.cstruct()
    assert L.r1o_mc_put_batch(C.byref(pa), w, h, O.ptr(c), len(c), O.ptr(put)) == 0
    assert L.r1o_mc_prep_batch(C.byref(pa), w, h, O.ptr(c), len(c), O.ptr(prep)) == 0
    return put, prep


def o_cdef_plane(L, luma, src, dst, p, xdec, ydec, w, h, skip, ci, ystr, uvstr, damping, bd):
    """r1o_cdef_filter_tile_plane into dst (a host plane, written in place)"""
    l, a, b = luma.cstruct(), src.cstruct(), dst.cstruct()
    ys, us = np.ascontiguousarray(ystr, np.uint8), np.ascontiguousarray(uvstr, np.uint8)
    L.r1o_cdef_filter_tile_plane(C.byref(l), C.byref(a), C.byref(b), p, xdec, ydec, w, h, skip.ctypes.data,
                                 row_stride(skip), skip.shape[1], skip.shape[0], ci.ctypes.data, row_stride(ci),
                                 O.ptr(ys), O.ptr(us), damping, bd)


def o_cdef_search(L, rec, src, skip, scales, prm):
    mi_rows, mi_cols = skip.shape
    n_sbx, n_sby = (mi_cols + 15) // 16, (mi_rows + 15) // 16
    err, best = np.zeros((n_sby, n_sbx, 8), np.uint64), np.zeros((n_sby, n_sbx), np.int8)
    assert L.r1o_cdef_strength_search(planes3(rec), planes3(src), skip.ctypes.data, row_stride(skip), mi_cols,
                                      mi_rows, scales.ctypes.data if scales is not None else None,
                                      row_stride(scales) if scales is not None else 0, C.byref(prm),
                                      err.ctypes.data, best.ctypes.data) == 0
    return err, best


def o_deblock(L, state, hp, pli, xd, yd, blocks, cw, ch, bd):
    """r1o_deblock_plane in place; blocks: (rows, cols, 8) uint8 records, dense or host_strided"""
    pc = hp.cstruct()
    assert L.r1o_deblock_plane(state.ctypes.data, C.byref(pc), pli, xd, yd, blocks.ctypes.data,
                               blocks.strides[0] // 8, blocks.shape[1], blocks.shape[0], cw, ch, bd) == 0


def o_deblock_sse(L, rec, src, pli, xd, yd, blocks, cw, ch, bd):
    t = np.zeros((2, 65), np.int64)
    pc, sc = rec.cstruct(), src.cstruct()
    assert L.r1o_deblock_sse_plane(C.byref(pc), C.byref(sc), pli, xd, yd, blocks.ctypes.data,
                                   blocks.strides[0] // 8, blocks.shape[1], blocks.shape[0], cw, ch, bd,
                                   t[0].ctypes.data, t[1].ctypes.data) == 0
    return t


def o_lrf_plane(L, cdef, debl, out, ydec, w, h, fh, us, sh, units, bd):
    cc, cd, co = cdef.cstruct(), debl.cstruct(), out.cstruct()
    assert L.r1o_lrf_filter_plane(C.byref(cc), C.byref(cd), C.byref(co), ydec, w, h, fh, us, units.shape[1],
                                  units.shape[0], sh, units.ctypes.data, bd) == 0


def o_sgr_solve(L, cdef, src, u, bd):
    cc, cs = cdef.cstruct(), src.cstruct()
    out = np.zeros((len(u), 2), np.int8)
    for i in range(len(u)):
        L.r1o_sgrproj_solve(C.byref(cc), C.byref(cs), int(u["x"][i]), int(u["y"][i]), int(u["w"][i]),
                            int(u["h"][i]), int(u["set"][i]), int(u["edges"][i]), bd, out[i].ctypes.data)
    return out


def o_lrf_search(L, lrf_in, src, u, chroma, xd, yd, scales, dist_scale, bd):
    ci, cs = lrf_in.cstruct(), src.cstruct()
    wx, we = np.zeros((len(u), 2), np.int8), np.zeros(len(u), np.uint64)
    for i in range(len(u)):
        assert L.r1o_lrf_search_unit(C.byref(ci), C.byref(cs), int(u["x"][i]), int(u["y"][i]), int(u["w"][i]),
                                     int(u["h"][i]), int(u["set"][i]), int(u["edges"][i]), int(chroma), xd, yd,
                                     scales.ctypes.data, row_stride(scales), dist_scale, bd, wx[i].ctypes.data,
                                     we[i:].ctypes.data) == 0
    return wx, we


def o_pad(L, hp, fw, fh):
    pc = hp.cstruct()
    L.r1o_plane_pad(C.byref(pc), fw, fh, 0, 0)


def o_downsample(L, src, dst, fw, fh, dec):
    a, b = src.cstruct(), dst.cstruct()
    assert L.r1o_plane_downsample(C.byref(a), C.byref(b), fw, fh, dec, dec) == 0


# ---- the cases both layout modules run (base planes in the HostPlane layout; relayout them per test) ----
CDEF_PAD = 4       # k_cdef_frame stages its halo from inside the picture only; the search reads 2 px around a block
DEBLOCK_PAD = 8    # a filter line at the bottom of the frame may read up to 7 rows of padding (rav1e_amd.h)
LRF_PAD = 8        # a unit at x < 4 (y < 2) needs that much origin padding (rav1e_amd.h)


def noise_padded(img, bd, pad):
    """HostPlane of an image with seeded noise (not replicated edges) in its padding"""
    h, w = img.shape
    hp = O.HostPlane(w, h, bd, pad, pad, rng=np.random.default_rng(w * 3 + h + bd))
    hp.view()[:] = img
    return hp


def flip_poison(skip):
    """poison for the gap of a skip-flag grid: the opposite of the majority, so a row read with the dense stride
    (which walks into the gap) sees flags that change the result"""
    return 0 if skip.mean() > 0.5 else 1


def lay(hp, kind, xpad, ypad):
    """hp in layout `kind`; None = a copy in the HostPlane layout.  The result remembers its kind for dev()."""
    if kind is None:
        p = O.HostPlane.__new__(O.HostPlane)
        p.__dict__.update(hp.__dict__)
        p.data = hp.data.copy()
    else:
        p = host_relayout(hp, kind, xpad, ypad)
    p.kind = kind
    return p


def dev(p):
    """the guarded device plane of a host plane made by lay()"""
    return DevicePlane(p, 1 if p.kind == "odd" else 0)


def cdef_case(bd, w=136, h=72):
    """136 x 72, 4:2:0: three superblock columns, the last 8 pixels wide; two rows, the last 8 high"""
    rng = np.random.default_rng(500 + bd)
    yy, xx = np.mgrid[0:h, 0:w]
    Y = np.clip((np.sin(xx / 6.0) + np.cos((yy + 2 * xx) / 9.0)) * 45 + 128 + rng.integers(-5, 6, (h, w)), 0, 255)
    Y = Y.astype(np.int64) << (bd - 8)
    U = rng.integers(0, 1 << bd, (h // 2, w // 2)) // 4 + (1 << (bd - 2))
    V = np.clip(Y[::2, ::2] // 2 + (30 << (bd - 8)), 0, (1 << bd) - 1)
    src_i = [Y, U, V]
    rec_i = [np.clip(s + rng.integers(-12 << (bd - 8), (12 << (bd - 8)) + 1, s.shape) * (rng.random(s.shape) < 0.3),
                     0, (1 << bd) - 1) for s in src_i]
    mi_cols, mi_rows = 2 * ((w + 7) // 8), 2 * ((h + 7) // 8)
    skip = (rng.random((mi_rows, mi_cols)) < 0.3).astype(np.uint8)
    skip[:4, 8:16] = 1
    skip[16:, 16:32] = 1       # one superblock skipped whole: the search leaves it out (-1)
    n_sbx, n_sby = (mi_cols + 15) // 16, (mi_rows + 15) // 16
    ystr, uvstr = rng.integers(1, 64, 8).astype(np.uint8), rng.integers(1, 64, 8).astype(np.uint8)
    ystr[0] = uvstr[0] = 0
    return {"bd": bd, "w": w, "h": h, "src": [noise_padded(a, bd, 16) for a in src_i],
            "rec": [noise_padded(a, bd, 16) for a in rec_i], "skip": skip,
            "ci": rng.integers(0, 8, (n_sby, n_sbx)).astype(np.uint8),
            "scales": rng.integers(1 << 11, 1 << 17, ((h + 7) // 8, (w + 7) // 8)).astype(np.uint32),
            "ystr": ystr, "uvstr": uvstr, "damping": 5,
            "dst": [O.HostPlane(p.shape[1], p.shape[0], bd, 16, 16, rng=np.random.default_rng(9 + i))
                    for i, p in enumerate(src_i)]}


def cdef_filter_planes(case, ksrc, kdst, strided):
    """the inputs of the frame filter of cdef_case in the given layouts -> (src, dst host planes, skip, ci)"""
    src = [lay(p, k, CDEF_PAD, CDEF_PAD) for p, k in zip(case["rec"], ksrc)]
    dst = [lay(p, k, CDEF_PAD, CDEF_PAD) for p, k in zip(case["dst"], kdst)]
    skip, ci = case["skip"], case["ci"]
    if strided:
        skip, ci = host_strided(skip, 3, flip_poison(skip)), host_strided(ci, 1, 7 - ci[:, -1:])
    return src, dst, skip, ci


def cdef_filter_oracle(L, case, ksrc, kdst, strided):
    src, dst, skip, ci = cdef_filter_planes(case, ksrc, kdst, strided)
    for p in range(3):
        xd = yd = 0 if p == 0 else 1
        o_cdef_plane(L, src[0], src[p], dst[p], p, xd, yd, case["w"], case["h"], skip, ci, case["ystr"],
                     case["uvstr"], case["damping"], case["bd"])
    return dst


def cdef_search_params(case, n_idx=8, area=(2, 1)):
    prm = O.CdefSearchParams()
    prm.y_strengths[:] = [int(v) for v in case["ystr"]]
    prm.uv_strengths[:] = [int(v) for v in case["uvstr"]]
    prm.damping, prm.bit_depth, prm.n_idx, prm.planes = case["damping"], case["bd"], n_idx, 3
    prm.xdec, prm.ydec, prm.crop_w, prm.crop_h = 1, 1, case["w"], case["h"]
    prm.area_sb_w, prm.area_sb_h = area
    prm.dist_scale[:] = [21000, 9000, 40000]
    return prm


def deblock_case(bd, w=128, h=64):
    """128 x 64, 4:2:0, cropped to 124 x 60 -> state, blocks as (rows, cols, 8) uint8 records, (rec, src) per plane"""
    import deblock_util as D
    from test_gpu_parity import _deblock_planes
    rng = np.random.default_rng(600 + bd)
    blocks = D.random_blocks(rng, w // 4, h // 4, 1, 1, deltas=True)
    state = D.make_state([int(v) for v in rng.integers(8, 50, 4)], rng, True, True)
    imgs = _deblock_planes(rng, w, h, bd, 1, 1, blocks)
    return {"state": state, "blocks": blocks.view(np.uint8).reshape(blocks.shape + (8,)).copy(), "cw": w - 4, "ch": h - 4,
            "planes": [(noise_padded(r, bd, 16), noise_padded(s, bd, 16)) for r, s in imgs]}


SGR_SOLVE_UNIT = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "<i2"), ("h", "<i2"), ("set", "u1"), ("edges", "u1"),
                           ("reserved", "u1", (2,))])


def lrf_case(bd, w, h=64):
    """w / 64 restoration units of 64 x 64 in one row: the filter's units, (unit, set) pairs for the solver and, with
    the no-filter option (set 255), for the search"""
    rng = np.random.default_rng(700 + bd + w)
    yy, xx = np.mgrid[0:h, 0:w]
    src = np.clip((np.sin(xx / 7.0) + np.cos(yy / 5.0) + 2) / 4 * ((1 << bd) - 1), 0, (1 << bd) - 1).astype(np.int64)
    debl = np.clip(src + rng.integers(-8, 9, (h, w)) * (1 << (bd - 8)), 0, (1 << bd) - 1)
    cdef = np.clip(debl + rng.integers(-2, 3, (h, w)) * (1 << (bd - 8)), 0, (1 << bd) - 1)
    cols = w // 64
    units = np.zeros((1, cols), O.LRF_UNIT)
    units["filter"] = 3
    units["set"] = rng.integers(0, 16, (1, cols))
    units["xqd"][..., 0] = rng.integers(-96, 32, (1, cols))
    units["xqd"][..., 1] = rng.integers(-32, 96, (1, cols))
    solve = np.array([(64 * c, 0, 64, 64, s, (c + s) & 3, (0, 0)) for c in range(cols) for s in (0, 5, 11, 14)],
                     SGR_SOLVE_UNIT)
    search = np.array([(64 * c, 0, 64, 64, s, (c + s) & 3, (0, 0)) for c in range(cols) for s in (255, 2, 11, 14, 9)],
                      SGR_SOLVE_UNIT)
    return {"src": noise_padded(src, bd, 16), "debl": noise_padded(debl, bd, 16), "cdef": noise_padded(cdef, bd, 16),
            "units": units, "solve": solve, "search": search,
            "scales": rng.integers(1 << 12, 1 << 16, (h // 8, w // 8)).astype(np.uint32)}

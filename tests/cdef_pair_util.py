"""One picture through both statements of cdef_filter_superblock: the frame filter (r1o_cdef_filter_tile_plane /
r1_cdef_filter_frame_plane) and the working copy of rdo_loop_decision (r1o_cdef_apply_area / r1_cdef_apply_area)
with ONE analysis area over the frame and the frame filter's cdef_index map as its index map.  With the frame a
multiple of 8 both ways the two agree pixel for pixel: the area's borders are the picture's, every block is whole."""
import ctypes as C

import numpy as np

import layout_util as LU
import loop_decision_util as U
import oracle_lib as O

# (bit depth, xdec, ydec): 4:2:0 at 8 / 10 / 12 bits, 4:2:2 (Cdef_Uv_Dir) and 4:4:4
FORMATS = [(8, 1, 1), (10, 1, 1), (12, 1, 1), (12, 1, 0), (10, 0, 0)]
_CACHE = {}


def case(bd, xdec, ydec, w=136, h=72):
    """136 x 72: three superblock columns, the last 8 pixels wide; two rows, the last 8 high; one superblock skipped
    whole.  Index 0 has strength 0; index 1 (luma) / 2 (chroma) primary strength 0 with a secondary one: the
    direction-0 tap set."""
    assert w % 8 == 0 and h % 8 == 0
    rng = np.random.default_rng(900 + bd + 2 * xdec + ydec)
    yy, xx = np.mgrid[0:h, 0:w]
    Y = np.clip((np.sin(xx / 6.0) + np.cos((yy + 2 * xx) / 9.0)) * 45 + 128 + rng.integers(-5, 6, (h, w)), 0, 255)
    Y = Y.astype(np.int64) << (bd - 8)
    cw, ch = w >> xdec, h >> ydec
    U_ = rng.integers(0, 1 << bd, (ch, cw)) // 4 + (1 << (bd - 2))
    V = np.clip(Y[::1 << ydec, ::1 << xdec] // 2 + (30 << (bd - 8)), 0, (1 << bd) - 1)
    rec = [np.clip(s + rng.integers(-12 << (bd - 8), (12 << (bd - 8)) + 1, s.shape) * (rng.random(s.shape) < 0.3),
                   0, (1 << bd) - 1) for s in (Y, U_, V)]
    mi_cols, mi_rows = w // 4, h // 4
    skip = (rng.random((mi_rows, mi_cols)) < 0.3).astype(np.uint8)
    skip[:4, 8:16] = 1
    skip[16:, 16:32] = 1
    n_sbx, n_sby = (mi_cols + 15) // 16, (mi_rows + 15) // 16
    ystr, uvstr = rng.integers(4, 64, 8).astype(np.uint8), rng.integers(4, 64, 8).astype(np.uint8)
    ystr[0] = uvstr[0] = 0
    ystr[1], uvstr[2] = 2, 3
    ci = rng.integers(3, 8, (n_sby, n_sbx)).astype(np.uint8)
    ci.flat[:3] = [0, 1, 2]
    return {"bd": bd, "xdec": xdec, "ydec": ydec, "w": w, "h": h, "skip": skip, "ci": ci, "ystr": ystr, "uvstr": uvstr,
            "damping": 5, "rec": [LU.noise_padded(a, bd, 16) for a in rec]}


def params(c):
    """the search parameters that make r1_cdef_apply_area the frame filter: one area over the frame"""
    prm = O.CdefSearchParams()
    prm.y_strengths[:] = [int(v) for v in c["ystr"]]
    prm.uv_strengths[:] = [int(v) for v in c["uvstr"]]
    prm.damping, prm.bit_depth, prm.n_idx, prm.planes = c["damping"], c["bd"], 8, 3
    prm.xdec, prm.ydec, prm.crop_w, prm.crop_h = c["xdec"], c["ydec"], c["w"], c["h"]
    prm.area_sb_h, prm.area_sb_w = c["ci"].shape
    return prm


def blank(c):
    return [O.HostPlane(p.width, p.height, c["bd"], 16, 16, rng=np.random.default_rng(9 + i))
            for i, p in enumerate(c["rec"])]


def oracle_pair(L, bd, xdec, ydec, w=136, h=72):
    """-> (case, visible planes of the frame filter, of the working copy), computed once per format"""
    key = (bd, xdec, ydec, w, h)
    if key not in _CACHE:
        U.sigs(L)
        c = case(bd, xdec, ydec, w, h)
        frame, area = blank(c), blank(c)
        for p in range(3):
            LU.o_cdef_plane(L, c["rec"][0], c["rec"][p], frame[p], p, xdec if p else 0, ydec if p else 0, w, h,
                            c["skip"], c["ci"], c["ystr"], c["uvstr"], c["damping"], bd)
        prm, idx = params(c), c["ci"].astype(np.int8)
        assert L.r1o_cdef_apply_area(LU.planes3(c["rec"]), LU.planes3(area), c["skip"].ctypes.data, c["skip"].shape[1],
                                     c["skip"].shape[1], c["skip"].shape[0], C.byref(prm), idx.ctypes.data) == 0
        _CACHE[key] = (c, [LU.window(p).copy() for p in frame], [LU.window(p).copy() for p in area])
    return _CACHE[key]

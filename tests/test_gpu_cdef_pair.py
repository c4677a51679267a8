"""k_cdef_frame and MODE 2 of k_cdef_search_pk both compute cdef_filter_superblock on the shared steps of
cdef_common.hpp; the other GPU tests hold each against its own oracle function only.  Here the two kernels are held
against each other: r1_cdef_apply_area with one analysis area over the frame and the frame filter's index map against
r1_cdef_filter_frame_plane (the statement tests/test_oracle_cdef.py proves for the oracle pair)."""
import numpy as np
import pytest

import cdef_pair_util as P
import layout_util as LU

pytestmark = pytest.mark.gpu


def _visible(d):
    return d.host()[d.yorigin:d.yorigin + d.height, d.xorigin:d.xorigin + d.width]


@pytest.mark.parametrize("fmt", [(8, 1, 1), (10, 1, 1), (12, 1, 0), (10, 0, 0)])
def test_apply_area_equals_frame_filter_on_the_device(ctx, oracle, fmt):
    """136 x 72: three superblock columns, the last 8 pixels wide, two rows, the last 8 high -- every picture-edge
    case of both tiles -- with one superblock skipped whole, an index of strength 0 and, per plane kind, one with
    primary strength 0 and a secondary one (the direction-0 tap set)"""
    import torch
    bd, xdec, ydec = fmt
    c, want_frame, want_area = P.oracle_pair(oracle, bd, xdec, ydec)
    w, h, (n_sby, n_sbx) = c["w"], c["h"], c["ci"].shape
    ystr, uvstr = [int(v) for v in c["ystr"]], [int(v) for v in c["uvstr"]]
    drec = [LU.dev(LU.lay(p, None, 0, 0)) for p in c["rec"]]
    d_area, d_frame = ([LU.dev(LU.lay(p, None, 0, 0)) for p in P.blank(c)] for _ in range(2))
    dskip, dci = torch.from_numpy(c["skip"]).cuda(), torch.from_numpy(c["ci"]).cuda()
    ctx.cdef_apply_area(drec, d_area, dskip, torch.from_numpy(c["ci"].astype(np.int8)).cuda(), ystr, uvstr,
                        c["damping"], bd, 8, xdec, ydec, w, h, area_sb=(n_sbx, n_sby))
    for p in range(3):
        ctx.cdef_filter_frame_plane(drec[0], drec[p], d_frame[p], p, xdec if p else 0, ydec if p else 0, w, h, dskip,
                                    dci, ystr, uvstr, c["damping"], bd)
    for p in range(3):
        area, frame = _visible(d_area[p]), _visible(d_frame[p])
        bad = np.argwhere(area != frame)
        assert len(bad) == 0, (fmt, p, len(bad), bad[:4])
        assert np.array_equal(frame, want_frame[p]) and np.array_equal(area, want_area[p]), (fmt, p)
        assert (frame != LU.window(c["rec"][p])).sum() > 500, (fmt, p)
    assert LU.guards_intact(*drec, *d_area, *d_frame)

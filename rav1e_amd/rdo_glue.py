"""Host-side glue of the RDO path: the small pieces of encoder logic that sit between the
reference's callers and the batch entry points -- descriptor arithmetic, no pixels.  Each function
restates a reference function (file:line); tests/golden/rdo_glue_ref.npz pins them together with
the kernels by executing the reference's own text (tests/golden/gen_rdo_glue_ref.py).

  get_mv_params              src/predict.rs:284-297   (MV -> integer offset + 1/16-pel fractions)
  compound_cands             src/predict.rs:339-382   (two MV lists -> the descriptors of the compound launch)
  clip_visible_bsize         src/rdo.rs:228-251
  luma_ac_pads               src/predict.rs:644-688   (luma_ac's w_pad / h_pad and its luma offset)
  largest_chroma_tx_size     src/partition.rs:385-393
  chroma_dist_dims           src/rdo.rs:404-413       (chroma_w / chroma_h of compute_tx_distortion)
  scale_distortion           src/rdo.rs:613-615,674-695   (RawDistortion * DistortionScale -> mul_u64)
  compute_tx_distortion      src/rdo.rs:349-434       (composition; the SSE comes from a callable:
                                                       Context.dist_scaled_batch on the GPU)
  compute_distortion         src/rdo.rs:254-347       (composition: luma by tune, chroma sse_wxh per plane)
  rav1e_tx_types / tx_type_slots   src/transform/mod.rs:28-44, src/rdo.rs:1731-1736
                                                      (which slot of r1_rdo_txsearch_batch holds which TxType)
  txb_ctx                    src/context/block_unit.rs:442-526   (BlockContext::get_txb_ctx: the two neighbour
                                                       contexts r1_coeff_rate_batch takes per candidate)
  txb_chain_ctx              src/encoder.rs:2282, 2446, 1561-1566  (a block's contexts and edges in front of its transform
                                                       blocks: the descriptor of r1_coeff_rate_chain_batch; pinned by
                                                       tests/golden/coeff_rate_chain_ref.npz)
  sub_tx_size                src/context/transform_unit.rs:85-105  (sub_tx_size_map: the next transform depth)
  has_chroma                 src/context/transform_unit.rs:108-121
  chroma_tx_grid             src/encoder.rs:2327-2338, 2492-2505  (uv_tx_size and the chroma transform-block grid of
                                                       write_tx_blocks / write_tx_tree, the integer arithmetic literally)
  uv_tx_type_intra / uv_tx_type_inter   src/encoder.rs:2346-2350, 2507-2511; src/context/transform_unit.rs:162-197;
                                                       src/transform/mod.rs:81-97
  block_chain_ctx / block_rate_trial    src/encoder.rs:2364-2369, 2525-2530, 1441, 1561-1566  (a block's three planes'
                                                       contexts and edges, and one trial: the descriptors of
                                                       r1_coeff_rate_block_batch; all pinned by
                                                       tests/golden/coeff_rate_block_ref.npz)
  intra_split_cands          src/encoder.rs:2276-2311  (write_tx_blocks' transform-block grid -> the descriptors of
                                                       r1_rdo_intra_split_batch)
  has_top_right / has_bottom_left   src/recon_intra.rs:174-243, 374-450   (luma, blocks up to 64x64; the reference's
                                                       availability tables are replaced by the coding order they
                                                       encode, computed)
  intra_split_masks          src/partition.rs:766-848  (the questions get_intra_edges asks per transform block)
                             pinned by tests/golden/rdo_intra_split_ref.npz / tests/test_rdo_intra_split_ref.py
  pick_tx_type               src/rdo.rs:1801-1818     (the tail of rdo_tx_type_decision's loop on the device's rates)
                             both pinned by tests/golden/coeff_rate_ref.npz / tests/test_coeff_rate_ref.py
  pick_first_min             src/rdo.rs:923-938, 780-784   (`rd < best.rd_cost`: the mode loop and the depth carry)
  tx_size_type_decision      src/rdo.rs:748-799       (rdo_tx_size_type's loop over the depths, over pick_tx_type)
  dist_as_f64                src/rdo.rs:722           (`distortion.0 as f64`, applied by the two above before they cost)
                             the host statements of r1_rd_pick_batch; pinned by tests/golden/rd_pick_ref.npz /
                             tests/test_rd_pick_ref.py
  coeff_nbr_store            src/context/block_unit.rs:333-348, src/context/partition_unit.rs:434-469  (what a coded or a
                                                       skipped block leaves in the coefficient neighbour contexts)
  coeff_nbr_reset_left       src/context/block_unit.rs:350-354, 394-397
  winner_tx_type             src/encoder.rs:2507-2511  (the winner's slot as the adapt trial's tx_type / uv_tx_type)
                             the host statements of r1_coeff_nbr_store_batch, r1_coeff_nbr_reset_left_batch and
                             r1_rd_winner_tx_type_batch; pinned by tests/golden/coeff_nbr_ref.npz /
                             tests/test_coeff_nbr_ref.py
  head_symbols               src/rdo.rs:870-877, src/encoder.rs:1913, 2086-2102, 2132-2136  (the head of an intra mode
                                                       trial as a list of (CDF row, symbol))
  partition_symbol / partition_context   src/context/partition_unit.rs:267-357, 416-429, 131-193
  tx_size_symbol             src/context/transform_unit.rs:576-667
  head_nbr_store             src/tiling/tile_blocks.rs:206-256, src/context/block_unit.rs:362-386,
                             src/context/partition_unit.rs:480-503  (what the coded block leaves)
  head_nbr_reset_left        src/context/block_unit.rs:356-360, 388-401
                             the host statements of r1_intra_head_rate_batch, r1_partition_rate_batch,
                             r1_intra_head_commit_batch and r1_head_nbr_reset_left_batch; pinned by
                             tests/golden/head_ref.npz / tests/test_head_ref.py
  find_mvrefs                src/context/block_unit.rs:795-1442 (setup_mvref_list and everything it calls)
  has_tr                     src/partition.rs:900-955 (has_top_right above is the intra edge rule: another rule)
  tile_blocks_store / tile_blocks_default   src/tiling/tile_blocks.rs:206-277, src/context/block_unit.rs:194-211
  mvref_pmv                  src/rdo.rs:1175-1181
                             the host statements of r1_mvref_stack_batch, r1_tile_blocks_store_batch,
                             r1_tile_blocks_reset_batch and r1_mvref_pmv_batch; pinned by
                             tests/golden/mvref_ref.npz / tests/test_mvref_ref.py
"""
import numpy as np

from .types import TILE_BLOCK, BlockSize, TxSize

MI_SIZE_LOG2 = 2
DIST_SCALE_SHIFT = 14


def get_mv_params(mv_row, mv_col, po_x, po_y, xdec=0, ydec=0):
    """-> (row_frac, col_frac, x, y): put_8tap / prep_8tap read the block whose top-left pixel is
    (x, y) (the reference slices at (x - 3, y - 3) and steps 3 in: the filter's own margin)"""
    row_offset = mv_row >> (3 + ydec)
    col_offset = mv_col >> (3 + xdec)
    row_frac = (mv_row << (1 - ydec)) & 0xf
    col_frac = (mv_col << (1 - xdec)) & 0xf
    return row_frac, col_frac, po_x + col_offset, po_y + row_offset


def compound_cands(x, y, mvs0, mvs1, filter_mode, xdec=0, ydec=0):
    """The descriptors of r1_rdo_compound_cand_batch for one block at plane position (x, y): candidate i pairs
    mvs0[i] on the first reference with mvs1[i] on the second, each (row, col) in 1/8 pel -- get_mv_params per
    reference as predict_inter_compound does (src/predict.rs:339-382), fi.default_filter for both.
    -> numpy array of api.COMPOUND_CAND"""
    import numpy as np
    from .api import COMPOUND_CAND
    assert len(mvs0) == len(mvs1)
    c = np.zeros(len(mvs0), COMPOUND_CAND)
    c["ox"], c["oy"], c["mode_x"], c["mode_y"] = x, y, int(filter_mode), int(filter_mode)
    for i, pair in enumerate(zip(mvs0, mvs1)):
        for k, (mv_row, mv_col) in enumerate(pair):
            rf, cf, px, py = get_mv_params(int(mv_row), int(mv_col), x, y, xdec, ydec)
            c["rx%d" % k][i], c["ry%d" % k][i], c["col_frac%d" % k][i], c["row_frac%d" % k][i] = px, py, cf, rf
    return c


def clip_visible_bsize(frame_w, frame_h, blk_w, blk_h, x, y):
    vw = blk_w if x + blk_w <= frame_w else (0 if x >= frame_w else frame_w - x)
    vh = blk_h if y + blk_h <= frame_h else (0 if y >= frame_h else frame_h - y)
    return vw, vh


def largest_chroma_tx_size(bsize, xdec, ydec):
    """TxSize of the chroma transform block of a luma partition: the subsampled block size, its
    largest rectangular transform, 64-point sides coded as 32 (av1_get_coded_tx_size)"""
    w, h = BlockSize(bsize).dims
    cw, ch = max(4, w >> xdec), max(4, h >> ydec)     # subsampled_size: sub-8x8 blocks share a 4x4
    return TxSize.by_dims(min(cw, 32), min(ch, 32))


def luma_ac_pads(bsize, luma_tx_size, bo_x, bo_y, w_in_b, h_in_b, xdec, ydec):
    """luma_ac: (w_pad, h_pad, luma_x, luma_y) -- pads in 4-pixel units of the chroma block, and the
    luma position pred_cfl_ac reads (sub-8x8 partitions read from the 8x8 that contains them)"""
    bw, bh = BlockSize(bsize).dims
    if (xdec and bw == 4) or (ydec and bh == 4):          # is_sub8x8 -> sub8x8_offset
        bo_x += -1 if (xdec and bw == 4) else 0
        bo_y += -1 if (ydec and bh == 4) else 0
    clipped_bw = min((w_in_b - bo_x) << MI_SIZE_LOG2, bw)
    clipped_bh = min((h_in_b - bo_y) << MI_SIZE_LOG2, bh)
    tw, th = TxSize(luma_tx_size).dims
    max_luma_w = ((clipped_bw + tw - 1) // tw) * tw if bw > 8 else bw
    max_luma_h = ((clipped_bh + th - 1) // th) * th if bh > 8 else bh
    return (bw - max_luma_w) >> (2 + xdec), (bh - max_luma_h) >> (2 + ydec), bo_x << MI_SIZE_LOG2, bo_y << MI_SIZE_LOG2


def chroma_dist_dims(bsize, visible_w, visible_h, xdec, ydec):
    bw, bh = BlockSize(bsize).dims
    cw = (visible_w + xdec) >> xdec if (bw >= 8 or xdec == 0) else (4 + visible_w + xdec) >> xdec
    ch = (visible_h + ydec) >> ydec if (bh >= 8 or ydec == 0) else (4 + visible_h + ydec) >> ydec
    return cw, ch


def scale_distortion(dist, scale_q14):
    """Distortion * DistortionScale (mul_u64): (scale * dist + 2^13) >> 14"""
    return (int(scale_q14) * int(dist) + (1 << DIST_SCALE_SHIFT >> 1)) >> DIST_SCALE_SHIFT


def compute_tx_distortion(sse_wxh, frame_w, frame_h, bsize, is_chroma_block, bo_x, bo_y, tx_dist, skip,
                          luma_only, dist_scale, xdec=1, ydec=1, monochrome=False):
    """compute_tx_distortion for one block.  sse_wxh(plane_index, x, y, w, h) -> the RawDistortion
    of sse_wxh on that plane at plane position (x, y) (r1_dist_scaled_batch, kind WSSE; the per-
    block bias of temporal RDO is inside it).  tx_dist: the ScaledDistortion the transform blocks
    accumulated.  dist_scale: fi.dist_scale (three Q14 values)."""
    bw, bh = BlockSize(bsize).dims
    if not skip:
        vw, vh = bw, bh
    else:
        vw, vh = clip_visible_bsize(frame_w, frame_h, bw, bh, bo_x << MI_SIZE_LOG2, bo_y << MI_SIZE_LOG2)
    if vw == 0 or vh == 0:
        return 0
    x, y = bo_x << MI_SIZE_LOG2, bo_y << MI_SIZE_LOG2
    dist = scale_distortion(sse_wxh(0, x, y, vw, vh), dist_scale[0]) if skip else int(tx_dist)
    if is_chroma_block and not luma_only and skip and not monochrome:
        cw, ch = chroma_dist_dims(bsize, vw, vh, xdec, ydec)
        # Area::BlockStartingAt on a decimated plane: (bo >> dec) << 2 (tiling/plane_region.rs:100-108)
        cx, cy = (bo_x >> xdec) << MI_SIZE_LOG2, (bo_y >> ydec) << MI_SIZE_LOG2
        for p in (1, 2):
            dist += scale_distortion(sse_wxh(p, cx, cy, cw, ch), dist_scale[p])
    return dist


def compute_distortion(dist_wxh, frame_w, frame_h, bsize, is_chroma_block, bo_x, bo_y, luma_only, dist_scale,
                       tune_psychovisual, xdec=1, ydec=1, monochrome=False):
    """compute_distortion for one block.  dist_wxh(kind, plane_index, x, y, w, h) -> the RawDistortion of
    sse_wxh (kind 2) / cdef_dist_wxh (kind 3) on that plane at plane position (x, y) over the VISIBLE w x h
    (r1_dist_scaled_batch; the per-importance-block bias of temporal RDO is inside it).  Luma: cdef_dist_wxh
    under Tune::Psychovisual, sse_wxh under Tune::Psnr, times fi.dist_scale[0]; chroma (is_chroma_block and
    not luma_only): sse_wxh per plane on the decimated planes, times fi.dist_scale[p]."""
    bw, bh = BlockSize(bsize).dims
    x, y = bo_x << MI_SIZE_LOG2, bo_y << MI_SIZE_LOG2
    vw, vh = clip_visible_bsize(frame_w, frame_h, bw, bh, x, y)
    if vw == 0 or vh == 0:
        return 0
    dist = scale_distortion(dist_wxh(3 if tune_psychovisual else 2, 0, x, y, vw, vh), dist_scale[0])
    if is_chroma_block and not luma_only and not monochrome:
        cw, ch = chroma_dist_dims(bsize, vw, vh, xdec, ydec)
        cx, cy = (bo_x >> xdec) << MI_SIZE_LOG2, (bo_y >> ydec) << MI_SIZE_LOG2
        for p in (1, 2):
            dist += scale_distortion(dist_wxh(2, p, cx, cy, cw, ch), dist_scale[p])
    return dist


RAV1E_TX_TYPES = (0, 1, 2, 3, 9, 10, 11)   # DCT_DCT, ADST_DCT, DCT_ADST, ADST_ADST, IDTX, V_DCT, H_DCT


def tx_type_slots(tx_type_mask):
    """slot j of r1_rdo_txsearch_batch's outputs -> TxType: the set bits of the mask in ascending order,
    which is also the order of RAV1E_TX_TYPES (the loop order of rdo_tx_type_decision)"""
    return [t for t in range(16) if (int(tx_type_mask) >> t) & 1]


def sub_tx_size(tx_size):
    """sub_tx_size_map: the transform size one split depth down (rdo_tx_size_type, src/rdo.rs:735, 792).  A square
    halves both sides (4x4 stays), a 2:1 rectangle becomes the square of its short side, a 4:1 rectangle halves its
    long side."""
    w, h = TxSize(tx_size).dims
    if w == h:
        return TxSize.by_dims(max(4, w // 2), max(4, h // 2))
    if max(w, h) == 2 * min(w, h):
        return TxSize.by_dims(min(w, h), min(w, h))
    return TxSize.by_dims(w // 2, h) if w > h else TxSize.by_dims(w, h // 2)


SB_MI = 16   # a 64x64 superblock in 4x4 units


def _coding_rank(r, c, w_mi, h_mi):
    """The place of block (row r, column c) of a superblock cut into uniform w_mi x h_mi blocks, in coding order:
    the z-order of the square of side max(w, h) that holds it, then its place inside that square (halves or quarters
    of a HORZ / VERT / HORZ_4 / VERT_4 partition, top to bottom or left to right).  This is what the reference's
    has_tr_* / has_bl_* tables (src/recon_intra.rs) tabulate: `the neighbour is coded before this block`."""
    s = max(w_mi, h_mi)
    rs, cs = r * h_mi // s, c * w_mi // s
    z = 0
    for bit in range(5):
        z |= ((cs >> bit) & 1) << (2 * bit) | ((rs >> bit) & 1) << (2 * bit + 1)
    return z * 4 + (c * w_mi % s) // w_mi + (r * h_mi % s) // h_mi


def has_top_right(bw, bh, mi_col, mi_row, top_available, right_available, tx_w, row_off, col_off):
    """has_top_right (src/recon_intra.rs:174-243) for a luma block of bw x bh pixels (<= 64) at 4x4-unit position
    (mi_col, mi_row) and the transform block of width tx_w at (row_off, col_off) 4x4 units inside it."""
    if not top_available or not right_available:
        return False
    bw_unit, count = bw >> 2, tx_w >> 2
    if row_off > 0:
        return col_off + count < bw_unit             # just: enough pixels on the right, inside the block
    if col_off + count < bw_unit:
        return True                                  # all in the block above
    w_mi, h_mi = bw >> 2, bh >> 2
    r, c = (mi_row & (SB_MI - 1)) // h_mi, (mi_col & (SB_MI - 1)) // w_mi
    if r == 0:
        return True                                  # top row of the superblock: the superblocks above are coded
    if (c + 1) * w_mi >= SB_MI:
        return False                                 # rightmost column: the superblock to the right is not
    return _coding_rank(r - 1, c + 1, w_mi, h_mi) < _coding_rank(r, c, w_mi, h_mi)


def has_bottom_left(bw, bh, mi_col, mi_row, bottom_available, left_available, tx_h, row_off, col_off):
    """has_bottom_left (src/recon_intra.rs:374-450), as has_top_right"""
    if not bottom_available or not left_available:
        return False
    if col_off > 0:
        return False                                 # inside the block: that transform block is not coded yet
    bh_unit, count = bh >> 2, tx_h >> 2
    if row_off + count < bh_unit:
        return True                                  # all in the block to the left
    w_mi, h_mi = bw >> 2, bh >> 2
    r, c = (mi_row & (SB_MI - 1)) // h_mi, (mi_col & (SB_MI - 1)) // w_mi
    if c == 0:
        return r * h_mi + row_off + count < SB_MI    # leftmost column: only the left superblock is coded
    if (r + 1) * h_mi >= SB_MI:
        return False                                 # bottom row: the superblock below is not coded
    # the block that holds the pixel below-left of this block's bottom-left corner
    return _coding_rank((r + 1), c - 1, w_mi, h_mi) < _coding_rank(r, c, w_mi, h_mi)


def intra_split_masks(bw, bh, tx_size, mi_col, mi_row, x, y, rect_w, rect_h):
    """(tr_mask, bl_mask) of R1IntraSplitCand for the block at tile position (x, y) pixels / (mi_col, mi_row) 4x4 units:
    bit k = has_top_right / has_bottom_left as get_intra_edges asks them for transform block k (src/partition.rs:766-848:
    have_top = by4 != 0 || the block is not in the tile's first row, right_available = x_k + tw < rect_w, ...).
    rect_w / rect_h: the tile clipped to the plane."""
    tw, th = TxSize(tx_size).dims
    gw, gh = bw // tw, bh // th
    tr = bl = 0
    for by in range(gh):
        for bx in range(gw):
            k, xk, yk, bx4, by4 = by * gw + bx, x + bx * tw, y + by * th, bx * (tw >> 2), by * (th >> 2)
            if has_top_right(bw, bh, mi_col, mi_row, by4 != 0 or mi_row > 0, xk + tw < rect_w, tw, by4, bx4):
                tr |= 1 << k
            if has_bottom_left(bw, bh, mi_col, mi_row, yk + th < rect_h, bx4 != 0 or mi_col > 0, th, by4, bx4):
                bl |= 1 << k
    return tr, bl


def intra_split_cands(blocks, bw, bh, tx_size):
    """The descriptors of r1_rdo_intra_split_batch for intra blocks of bw x bh pixels coded with tx_size transforms.
    blocks: one (x, y, mode, angle_delta, ief, has_tr, has_bl) per block -- the position relative to the tile, the luma
    mode as write_tx_blocks receives it (no Paeth remap), the block's ief (0 none, 1 plain, 2 smooth neighbour; it is
    taken as 0 for a mode that is not directional, as encode_tx_block does, src/encoder.rs:1458) and has_tr / has_bl:
    the answers of has_top_right / has_bottom_left per transform block, indexed by the block's raster index in the
    bw/tw x bh/th grid (sequences of ntx truth values, or ready bit masks).  -> numpy array of api.INTRA_SPLIT_CAND"""
    import numpy as np
    from .api import INTRA_SPLIT_CAND
    tw, th = TxSize(tx_size).dims
    assert bw % tw == 0 and bh % th == 0
    ntx = (bw // tw) * (bh // th)
    assert 2 <= ntx <= 16

    def mask(v):
        if isinstance(v, (int, np.integer)):
            assert 0 <= int(v) < (1 << ntx)
            return int(v)
        assert len(v) == ntx
        return sum(1 << k for k, b in enumerate(v) if b)
    c = np.zeros(len(blocks), INTRA_SPLIT_CAND)
    for i, (x, y, mode, delta, ief, tr, bl) in enumerate(blocks):
        assert x >= 0 and y >= 0 and x % 4 == 0 and y % 4 == 0 and 0 <= mode <= 12
        directional = 1 <= mode <= 8
        c[i] = (x, y, mode, delta if directional else 0, ief if directional else 0, 0, mask(tr), mask(bl))
    return c


RESTORATION_TILESIZE_MAX_LOG2 = 8


def tx_split_blocks(bx, by, bw, bh, tw, th, mi_width, mi_height):
    """The transform blocks write_tx_tree (src/encoder.rs:2440-2476) visits for a block at 4x4-unit position (bx, by) of
    bw x bh pixels coded with tw x th transforms: raster order, blocks that START outside the tile's 4x4 grid skipped.
    -> [(index in the bw/tw x bh/th grid, pixel x, pixel y)].  For an inter block these are the candidates of the next
    transform depth (rdo_tx_size_type, src/rdo.rs:745-815): one r1_rdo_txsearch_batch launch in its dense-prediction
    form, the block's prediction cut into the same rectangles."""
    out = []
    for j in range(bh // th):
        for i in range(bw // tw):
            tx, ty = bx + i * (tw // 4), by + j * (th // 4)
            if tx >= mi_width or ty >= mi_height:
                continue
            out.append((j * (bw // tw) + i, tx * 4, ty * 4))
    return out


def restoration_plane_configs(width, height, xdec, ydec, base_q_idx, enable_large_lru=True, enable_restoration=True,
                              use_128x128_superblock=False, tiling=(1, 1, 0, 0)):
    """RestorationState::new (src/lrf.rs:1321-1480): the restoration-unit geometry of the three planes of a frame --
    per plane dict(unit_size, sb_h_shift, sb_v_shift, stripe_height, cols, rows).  tiling = (cols, rows,
    tile_width_sb, tile_height_sb).  cols / rows follow the specification's last-unit rule (a remainder of less than
    half a unit stretches the last unit instead of starting a new one)."""
    stripe_uv_decimate = 1 if (xdec > 0 and ydec > 0) else 0
    y_sb_log2 = 7 if use_128x128_superblock else 6
    uv_sb_h_log2, uv_sb_v_log2 = y_sb_log2 - xdec, y_sb_log2 - ydec
    if enable_large_lru and enable_restoration:
        assert width > 1 and height > 1
        lrf_base_shift = 0 if base_q_idx > 200 else (1 if base_q_idx > 160 else 2)
        if stripe_uv_decimate:
            if lrf_base_shift == 2:
                lrf_chroma_shift = 1
            else:
                us = 1 << (RESTORATION_TILESIZE_MAX_LOG2 - lrf_base_shift)
                unshifted = ((width >> xdec) - 1) % us <= us // 2 or ((height >> ydec) - 1) % us <= us // 2
                shifted = ((width >> xdec) - 1) % (us >> 1) <= us // 4 or ((height >> ydec) - 1) % (us >> 1) <= us // 4
                lrf_chroma_shift = 1 if (unshifted and not shifted) else 0
        else:
            lrf_chroma_shift = 0
        lrf_y_shift, lrf_uv_shift = lrf_base_shift, lrf_base_shift + lrf_chroma_shift
    else:
        lrf_y_shift = 1 if use_128x128_superblock else 2
        lrf_uv_shift = lrf_y_shift + stripe_uv_decimate
    y_unit = 1 << (RESTORATION_TILESIZE_MAX_LOG2 - lrf_y_shift)
    uv_unit = 1 << (RESTORATION_TILESIZE_MAX_LOG2 - lrf_uv_shift)
    t_cols, t_rows, tw_sb, th_sb = tiling
    if t_cols > 1 or t_rows > 1:
        tz = lambda v: (v & -v).bit_length() - 1 if v else 64     # usize::trailing_zeros (0 -> the type's width)
        hz, vz = tz(tw_sb), tz(th_sb)
        y_unit = min(y_unit, 1 << (y_sb_log2 + min(hz, vz)))
        uv_unit = min(uv_unit, min(1 << (uv_sb_h_log2 + hz), 1 << (uv_sb_v_log2 + vz)))
    if ydec == 0 and y_unit != uv_unit:
        y_unit = min(uv_unit, y_unit)
        uv_unit = y_unit
    y_log2, uv_log2 = y_unit.bit_length() - 1, uv_unit.bit_length() - 1
    y_cols = max((width + (y_unit >> 1)) // y_unit, 1)
    y_rows = max((height + (y_unit >> 1)) // y_unit, 1)
    uv_cols = max((((width + (1 << xdec >> 1)) >> xdec) + (uv_unit >> 1)) // uv_unit, 1)
    uv_rows = max((((height + (1 << ydec >> 1)) >> ydec) + (uv_unit >> 1)) // uv_unit, 1)
    y = dict(unit_size=y_unit, sb_h_shift=y_log2 - y_sb_log2, sb_v_shift=y_log2 - y_sb_log2, stripe_height=64, cols=y_cols,
             rows=y_rows)
    uv = dict(unit_size=uv_unit, sb_h_shift=uv_log2 - uv_sb_h_log2, sb_v_shift=uv_log2 - uv_sb_v_log2,
              stripe_height=64 >> stripe_uv_decimate, cols=uv_cols, rows=uv_rows)
    return [y, dict(uv), dict(uv)]


def restoration_search_units(cfg, crop_w, crop_h, dec_x=0, dec_y=0):
    """The (x, y, vis_w, vis_h) rectangles the restoration leg of rdo_loop_decision solves and filters, for a WHOLE
    plane: one per restoration unit (x, y) < (cfg.cols, cfg.rows) -- has_restoration_unit(.., stretch = false) -- at
    loop_sbo.plane_offset = unit index x unit_size, clipped to the visible plane: vis = min(unit_size, (crop >> dec) -
    offset) (src/rdo.rs:2645-2654; the stretched remainder of a last unit is filtered at frame time, not searched).
    This is the `units` list of r1_lrf_search_batch (one entry per parameter set each)."""
    us, out = cfg["unit_size"], []
    pw, ph = crop_w >> dec_x, crop_h >> dec_y
    for uy in range(cfg["rows"]):
        for ux in range(cfg["cols"]):
            x, y = ux * us, uy * us
            if x < pw and y < ph:
                out.append((x, y, min(us, pw - x), min(us, ph - y)))
    return out


def restoration_area_sb(cfgs):
    """The area one rdo_loop_decision call decides, in superblocks: the largest restoration unit of the planes
    (src/rdo.rs:2119-2141).  cfgs: restoration_plane_configs(..)."""
    return (max(1 << c["sb_h_shift"] for c in cfgs), max(1 << c["sb_v_shift"] for c in cfgs))


SGR_EDGE_LEFT, SGR_EDGE_ABOVE = 1, 2


def restoration_unit_edges(x, y, dec_x, dec_y, area_sb, sb_log2=6):
    """R1SgrSolveUnit.edges of the unit at plane pixel (x, y): rdo_loop_decision filters on a scratch copy of the
    area (src/rdo.rs:2277-2296), so setup_integral_image (src/lrf.rs: `cdeffed.x == 0`, `clamp(y, 0, ..)`) finds
    pixels left of / above the unit exactly when the unit does not start the area's first unit column / row."""
    aw, ah = (area_sb[0] << sb_log2) >> dec_x, (area_sb[1] << sb_log2) >> dec_y
    return (SGR_EDGE_LEFT if x % aw else 0) | (SGR_EDGE_ABOVE if y % ah else 0)


def compute_rd_cost(lam, rate, distortion):
    """compute_rd_cost (src/rdo.rs:718-723): fi.lambda.mul_add(rate / 8, distortion) -- ONE rounding (f64 fused
    multiply-add), reproduced here through exact rationals"""
    from fractions import Fraction
    return float(Fraction(float(lam)) * Fraction(int(rate), 8) + Fraction(int(distortion)))


def dist_as_f64(distortion):
    """`distortion.0 as f64` (src/rdo.rs:722): the u64 distortion rounded to the nearest f64, ties to even, returned
    as the integer that f64 holds.  The reference converts BEFORE its fused multiply-add, so from 2^53 on its cost
    has two roundings; compute_rd_cost above adds the integer it is given exactly.  The statements r1_rd_pick_batch
    is held to (pick_first_min, tx_size_type_decision) therefore hand compute_rd_cost / pick_tx_type
    dist_as_f64(dist): below 2^53 that is dist itself"""
    return int(float(int(distortion)))


def pick_restoration_filter(options, lam, best_cost=-1.0):
    """The choice of one restoration unit (src/rdo.rs:2617-2745).  options: [(rate, err)] in the order the leg tries
    them -- the no-filter option first, then one per parameter set, err = what r1_lrf_search_batch returned, rate =
    cw.fc.count_lrf_switchable for that option.  Returns (index into options or None when nothing beat best_cost,
    the cost kept).  First smallest cost wins; the no-filter option also wins when no cost was kept before."""
    pick = None
    for i, (rate, err) in enumerate(options):
        cost = compute_rd_cost(lam, rate, err)
        if (i == 0 and best_cost < 0.0) or cost < best_cost:
            best_cost, pick = cost, i
    return pick, best_cost



COEFF_CONTEXT_BITS = 6
_DC_SIGNS = (0, -1, 1)
# skip_contexts[min][max] (block_unit.rs:492-498)
_SKIP_CONTEXTS = ((1, 2, 2, 2, 3), (1, 4, 4, 4, 5), (1, 4, 4, 4, 5), (1, 4, 4, 4, 5), (1, 4, 4, 4, 6))


def txb_ctx(above_ctxs, left_ctxs, plane, plane_bsize, tx_size):
    """BlockContext::get_txb_ctx (src/context/block_unit.rs:442-526) -> (txb_skip_ctx, dc_sign_ctx).
    above_ctxs / left_ctxs: the entries of above_coeff_context[plane] / left_coeff_context[plane] the transform block
    covers (frame_clipped_txw >> 2 and frame_clipped_txh >> 2 of them), each the cul_level byte a coded neighbour
    left there (r1_coeff_rate_batch's cul_level_out)."""
    above, left = [int(v) for v in above_ctxs], [int(v) for v in left_ctxs]
    dc_sign = sum(_DC_SIGNS[v >> COEFF_CONTEXT_BITS] for v in above + left)
    dc_sign_ctx = 0 if dc_sign == 0 else (1 if dc_sign < 0 else 2)
    top = left_ = 0
    for v in above:
        top |= v
    for v in left:
        left_ |= v
    tw, th = TxSize(tx_size).dims
    bw, bh = BlockSize(plane_bsize).dims
    if plane == 0:
        if (bw, bh) == (tw, th):
            return 0, dc_sign_ctx
        top, left_ = top & 63, left_ & 63
        return _SKIP_CONTEXTS[min(min(top, left_), 4)][min(top | left_, 4)], dc_sign_ctx
    # num_pels_log2_lookup[plane_bsize] > num_pels_log2_lookup[tx_size.block_size()]
    return (top != 0) + (left_ != 0) + (10 if bw * bh > tw * th else 7), dc_sign_ctx


def txb_chain_ctx(above_row, left_col, bo_x, bo_y, bw, bh, mi_width, mi_height, w_in_b, h_in_b, y_mode, cdf_sel):
    """The R1TxbChainCtx of r1_coeff_rate_chain_batch for a bw x bh luma block at tile block offset (bo_x, bo_y), as a
    tuple in the field order of types.TXB_CHAIN_CTX.  above_row / left_col: above_coeff_context[0] (indexed by bo.x)
    and left_coeff_context[0] (indexed by bo.y_in_sb() = bo_y % 16) as they stand in front of the block; mi_width /
    mi_height: the tile's (the skip test of encoder.rs:2282, 2446); w_in_b / h_in_b: fi.w_in_b / fi.h_in_b less the
    tile's own block offset in the frame, so that w_in_b - bo_x is fi.w_in_b - frame_bo.x (encoder.rs:1561-1566)."""
    assert 4 <= bw <= 64 and 4 <= bh <= 64
    y_sb = bo_y % 16
    # the block covers the first bw / 4 and bh / 4 entries; the rest (as far as the arrays go) passes through to ctx_out
    above = [int(v) for v in above_row[bo_x:bo_x + 16]]
    left = [int(v) for v in left_col[y_sb:y_sb + 16]]
    pad = lambda v: tuple(v + [0] * (16 - len(v)))
    return (pad(above), pad(left), min(255, mi_width - bo_x), min(255, mi_height - bo_y), min(255, w_in_b - bo_x),
            min(255, h_in_b - bo_y), int(y_mode), int(cdf_sel), (0, 0))


def block_size(bw, bh):
    """the BlockSize of bw x bh luma pixels"""
    return BlockSize["BLOCK_%dX%d" % (bw, bh)]


def has_chroma(bo_x, bo_y, bsize, xdec, ydec, monochrome=False):
    """has_chroma (src/context/transform_unit.rs:108-121): whether the block at tile block offset (bo_x, bo_y) carries
    the chroma of its 8x8 -- with subsampling, a 4-wide / 4-high block does at odd offsets only.  monochrome: Cs400."""
    if monochrome:
        return False
    w, h = BlockSize(bsize).dims
    bw, bh = w >> MI_SIZE_LOG2, h >> MI_SIZE_LOG2
    return ((bo_x & 1) == 1 or (bw & 1) == 0 or xdec == 0) and ((bo_y & 1) == 1 or (bh & 1) == 0 or ydec == 0)


def chroma_tx_grid(bsize, xdec, ydec, is_inter=False):
    """-> (uv_tx_size, bw_uv, bh_uv): the chroma transform size and the grid write_tx_blocks (src/encoder.rs:2327-2338)
    or write_tx_tree (2492-2505) loops over per chroma plane, the integer arithmetic as it stands -- either side 0
    makes both 1 BEFORE the division by the transform's width_mi / height_mi, so BLOCK_4X16 and BLOCK_16X4 in 4:2:0
    come out with an empty grid."""
    w, h = BlockSize(bsize).dims
    uv_tx_size = largest_chroma_tx_size(bsize, xdec, ydec)
    if is_inter:      # max_txsize_rect_lookup[bsize].width_mi(), height_mi(): 64 at most
        w_mi, h_mi = min(w, 64) >> MI_SIZE_LOG2, min(h, 64) >> MI_SIZE_LOG2
    else:             # bw * tx_size.width_mi() with bw = bsize.width_mi() / tx_size.width_mi()
        w_mi, h_mi = w >> MI_SIZE_LOG2, h >> MI_SIZE_LOG2
    bw_uv, bh_uv = w_mi >> xdec, h_mi >> ydec
    if bw_uv == 0 or bh_uv == 0:
        bw_uv = bh_uv = 1
    uw, uh = TxSize(uv_tx_size).dims
    return uv_tx_size, bw_uv // (uw >> MI_SIZE_LOG2), bh_uv // (uh >> MI_SIZE_LOG2)


# intra_mode_to_tx_type_context over uv2y (src/context/transform_unit.rs:162-193): DC .. PAETH, then UV_CFL -> DC
_INTRA_MODE_TX_TYPE = (0, 1, 2, 0, 3, 1, 2, 2, 1, 3, 1, 2, 3, 0)


def uv_tx_type_intra(chroma_mode, uv_tx_size):
    """the uv_tx_type of write_tx_blocks (src/encoder.rs:2346-2350); chroma_mode: DC_PRED 0 .. PAETH_PRED 12, UV_CFL_PRED 13"""
    uw, uh = TxSize(uv_tx_size).dims
    return 0 if uw >= 32 or uh >= 32 else _INTRA_MODE_TX_TYPE[int(chroma_mode)]


def uv_tx_type_inter(tx_type, uv_tx_size, partition_has_coeff):
    """the uv_tx_type of write_tx_tree (src/encoder.rs:2507-2511): TxType::uv_inter (src/transform/mod.rs:81-97) of the
    luma type, DCT_DCT when no luma transform block had a coefficient"""
    if not partition_has_coeff:
        return 0
    uw, uh = TxSize(uv_tx_size).dims
    tx_type = int(tx_type)
    if max(uw, uh) == 32:                  # sqr_up() == TX_32X32
        return 9 if tx_type == 9 else 0
    if min(uw, uh) == 16:                  # sqr() == TX_16X16
        return 0 if tx_type in (12, 13, 14, 15) else tx_type
    return tx_type


def block_chain_ctx(above_rows, left_cols, bo_x, bo_y, bsize, xdec, ydec, mi_width, mi_height, w_in_b, h_in_b, y_mode,
                    cdf_sel, cdf_sel_uv):
    """The R1BlockChainCtx of r1_coeff_rate_block_batch for the block at tile block offset (bo_x, bo_y), as a tuple in the
    field order of types.BLOCK_CHAIN_CTX.  above_rows[p] / left_cols[p]: above_coeff_context[p] (indexed by x >> xdec
    for chroma) and left_coeff_context[p] (by y_in_sb() >> ydec) in front of the block; the rest as txb_chain_ctx.
    The chroma arrays and the chroma clip start at the first chroma transform block's tx_bo: the block's offset less
    one unit where the block is 4 wide / high and the plane is subsampled (src/encoder.rs:2364-2369, 2525-2530)."""
    bw, bh = BlockSize(bsize).dims
    assert 4 <= bw <= 64 and 4 <= bh <= 64
    ux, uy = bo_x - (bw == 4) * xdec, bo_y - (bh == 4) * ydec
    pad = lambda v: [int(e) for e in v] + [0] * (16 - len(v))
    ctx = []
    for p in range(3):
        x0, y0 = (bo_x, bo_y % 16) if p == 0 else (ux >> xdec, (uy % 16) >> ydec)
        ctx.append((pad(above_rows[p][x0:x0 + 16]), pad(left_cols[p][y0:y0 + 16])))
    clip_uv = lambda edge, o, dec: min(255, max(0, (((edge - o) << MI_SIZE_LOG2) >> dec) >> 2))
    return (ctx, min(255, mi_width - bo_x), min(255, mi_height - bo_y), min(255, w_in_b - bo_x), min(255, h_in_b - bo_y),
            clip_uv(w_in_b, ux, xdec), clip_uv(h_in_b, uy, ydec), int(y_mode), int(cdf_sel), int(cdf_sel_uv), (0, 0, 0))


def block_rate_trial(first_y, first_u, first_v, block, tx_type, uv_tx_type, do_chroma, rng=0x8000):
    """One R1BlockRateTrial, in the field order of types.BLOCK_RATE_TRIAL.  rng: the host counter's `rng` behind the
    last head symbol (0x8000: a fresh WriterCounter); the reference's rate is then the call's rate_out plus the host's
    tell_frac at that point less the fresh counter's."""
    assert 0x8000 <= int(rng) <= 0xFFFF
    return (int(first_y), int(first_u), int(first_v), int(block), int(rng), int(tx_type), int(uv_tx_type),
            int(bool(do_chroma)), (0, 0, 0))


def coeff_cdf_context(fields):
    """One R1CoeffCdfContext (a types.COEFF_CDF_CONTEXT record) from a dict of the reference's CDFContext field arrays
    (src/context/cdf_context.rs:23-96), keyed by the reference's names with or without the `_cdf` in them
    (`txb_skip_cdf`, `eob_flag_cdf16`, `intra_tx_1_cdf`, ... or the struct's `txb_skip`, `eob_flag16`, `intra_tx_1`):
    every coefficient field must be there, in the reference's shape; the padding is zero."""
    import numpy as np
    from .types import COEFF_CDF_CONTEXT
    rec = np.zeros(1, COEFF_CDF_CONTEXT)[0]
    for name in COEFF_CDF_CONTEXT.names:
        if name == "pad":
            continue
        if name.startswith("eob_flag"):
            ref = "eob_flag_cdf" + name[len("eob_flag"):]
        else:
            ref = name + "_cdf"
        v = fields[ref] if ref in fields else fields[name]
        a = np.asarray(v)
        assert a.shape == rec[name].shape, (name, a.shape, rec[name].shape)
        assert a.min() >= 0 and a.max() <= 0xFFFF, name
        rec[name] = a
    return rec


def nbr_block(nbr, bo_x, bo_y, mi_width, mi_height, w_in_b, h_in_b, y_mode=0, cdf_sel=0, cdf_sel_uv=0, do_chroma=True,
              skip=False):
    """One R1NbrBlock, in the field order of types.NBR_BLOCK: a block's place on the device-resident neighbour context
    `nbr`; the geometry arguments as block_chain_ctx takes them."""
    return (int(nbr), int(bo_x), int(bo_y), int(mi_width), int(mi_height), int(w_in_b), int(h_in_b), int(y_mode),
            int(cdf_sel), int(cdf_sel_uv), int(bool(do_chroma)) | int(bool(skip)) << 1)


def coeff_nbr_store(above_rows, left_cols, bo_x, bo_y, bsize, xdec, ydec, do_chroma, skip, ctx_behind=None):
    """What a block leaves in above_coeff_context / left_coeff_context, IN PLACE (the statement of
    r1_coeff_nbr_store_batch).  above_rows[p] / left_cols[p]: the arrays as block_chain_ctx indexes them.
    Coded (skip false): ctx_behind, the [3][2][16] R1BlockChainCtx.ctx behind the block (the rate call's ctx_out), goes
    back over the block's spans -- luma bw / 4 and bh / 4 entries at (bo_x, bo_y % 16); with do_chroma the chroma
    transform grid's span (chroma_tx_grid) at block_chain_ctx's chroma origin.  That is every set_coeff_context
    (src/context/block_unit.rs:333-348) of the block's transform blocks: ctx_out passes through what none of them wrote.
    Skipped: reset_skip_context (src/context/partition_unit.rs:434-469) -- zeros over bsize.subsampled_size(xdec, ydec) at
    (bo_x >> xdec, (bo_y % 16) >> ydec); chroma with do_chroma and, whatever the flag, for BLOCK_4X16 / BLOCK_16X4: they
    are not below BLOCK_8X8 in the enum's order, so the reference resets three planes there even where has_chroma says no
    (every other size at or above BLOCK_8X8 has has_chroma true, and do_chroma false then means Cs400: one plane).
    -> False, nothing written, where a span leaves the arrays (the device's refusal), else True"""
    bw, bh = BlockSize(bsize).dims
    bw4, bh4 = bw >> MI_SIZE_LOG2, bh >> MI_SIZE_LOG2
    y_sb = bo_y % 16
    width = len(above_rows[0])
    if bo_x + bw4 > width or y_sb + bh4 > 16:
        return False
    if skip:
        chroma = bool(do_chroma) or (bw, bh) in ((4, 16), (16, 4))
        cx, cy = bo_x >> xdec, y_sb >> ydec
        cw, ch = max(bw >> xdec, 4) >> MI_SIZE_LOG2, max(bh >> ydec, 4) >> MI_SIZE_LOG2
    else:
        uv_tx_size, bw_uv, bh_uv = chroma_tx_grid(bsize, xdec, ydec)
        uw, uh = TxSize(uv_tx_size).dims
        chroma = bool(do_chroma) and bw_uv * bh_uv > 0
        ux, uy = bo_x - (bw == 4) * xdec, bo_y - (bh == 4) * ydec
        if chroma and (ux < 0 or uy < 0):
            return False
        cx, cy = ux >> xdec, (uy % 16) >> ydec
        cw, ch = bw_uv * (uw >> MI_SIZE_LOG2), bh_uv * (uh >> MI_SIZE_LOG2)
    if chroma and (cx + cw > width or cy + ch > 16):
        return False
    value = (lambda p, a, k: 0) if skip else (lambda p, a, k: int(ctx_behind[p][a][k]))
    for p in range(3 if chroma else 1):
        x0, y0, w, h = (bo_x, y_sb, bw4, bh4) if p == 0 else (cx, cy, cw, ch)
        for k in range(w):
            above_rows[p][x0 + k] = value(p, 0, k)
        for k in range(h):
            left_cols[p][y0 + k] = value(p, 1, k)
    return True


def coeff_nbr_reset_left(left_cols, planes=3):
    """reset_left_contexts' coefficient part (src/context/block_unit.rs:350-354, 394-397), IN PLACE: the statement of
    r1_coeff_nbr_reset_left_batch"""
    for p in range(planes):
        for k in range(len(left_cols[p])):
            left_cols[p][k] = 0


def winner_tx_type(best_slot, tx_type_mask, is_inter, uv_tx_size=None, eobs=None):
    """The statement of r1_rd_winner_tx_type_batch: -> (tx_type, uv_tx_type or None).  tx_type: the best_slot-th type of
    the mask (tx_type_slots); None, None when best_slot lies outside it.  uv_tx_type: for inter, uv_tx_type_inter with
    partition_has_coeff = any(eobs) over the winner's luma transform blocks (src/encoder.rs:2507-2511); for intra None --
    it belongs to the chroma mode (uv_tx_type_intra)."""
    slots = tx_type_slots(tx_type_mask)
    if not 0 <= int(best_slot) < len(slots):
        return None, None
    tx_type = slots[int(best_slot)]
    if not is_inter:
        return tx_type, None
    return tx_type, uv_tx_type_inter(tx_type, uv_tx_size, any(int(e) != 0 for e in eobs))


def pick_tx_type(rates, dists, lam, cur_best_rd):
    """The tail of rdo_tx_type_decision's loop (src/rdo.rs:1801-1818) over the slots of one candidate, in slot order
    (tx_type_slots): rd = compute_rd_cost(rate, distortion); after the FIRST type the loop ends when rd > cur_best_rd;
    a type is kept on strict `<`, so a tie keeps the earlier one.  rates: r1_coeff_rate_batch's (1/8 bit), dists: the
    candidate call's.  -> (slot kept, its rd); (None, f64::MAX) when the early exit left the reference's initial
    (DCT_DCT, f64::MAX)."""
    import sys
    best, best_rd = None, sys.float_info.max
    for j, (rate, dist) in enumerate(zip(rates, dists)):
        rd = compute_rd_cost(lam, rate, dist)
        if j == 0 and rd > cur_best_rd:
            break
        if rd < best_rd:
            best, best_rd = j, rd
    return best, best_rd


RATE_INVALID = 0xFFFFFFFF   # the rate calls' refusal value; r1_rd_pick_batch costs such a slot +infinity


def pick_first_min(rates, dists, lam, best=None, rate_adds=None):
    """`rd < best.rd_cost` over trials in order (luma_chroma_mode_rdo, src/rdo.rs:923-938; the carry across depths of
    rdo_tx_size_type, 780-784): a trial is kept on strict `<`, so a tie keeps the earlier one -- one kept before
    included.  best: (index, rd, rate, dist) carried in, None = (None, f64::MAX, 0, 0).  rate_adds: what the host adds
    per trial (the head's tell_frac difference).  A rate of RATE_INVALID, or a sum that reaches it, costs +infinity.
    -> (index kept or the one carried in, its rd, its rate with the addition, its dist)"""
    import sys
    idx, best_rd, best_rate, best_dist = best if best is not None else (None, sys.float_info.max, 0, 0)
    for i, (rate, dist) in enumerate(zip(rates, dists)):
        rate = int(rate) + (int(rate_adds[i]) if rate_adds is not None else 0)
        rd = float("inf") if rate >= RATE_INVALID else compute_rd_cost(lam, rate, dist_as_f64(dist))
        if rd < best_rd:
            idx, best_rd, best_rate, best_dist = i, rd, rate, int(dist)
    return idx, best_rd, best_rate, best_dist


def tx_size_type_decision(per_depth_rates, per_depth_dists, lam):
    """rdo_tx_size_type's loop over the transform depths (src/rdo.rs:748-799): depth d runs rdo_tx_type_decision with
    cur_best_rd = the rd kept so far -- pick_tx_type, early exit included -- and its result replaces what is kept when
    its rd is strictly below (780).  per_depth_rates[d] / per_depth_dists[d]: the slots of depth d in slot order.
    -> (depth kept, slot kept, rd); (None, None, f64::MAX) when no depth kept anything"""
    import sys
    best_depth, best_slot, best_rd = None, None, sys.float_info.max
    for depth, (rates, dists) in enumerate(zip(per_depth_rates, per_depth_dists)):
        slot, rd = pick_tx_type(rates, [dist_as_f64(d) for d in dists], lam, best_rd)
        if slot is not None and rd < best_rd:
            best_depth, best_slot, best_rd = depth, slot, rd
    return best_depth, best_slot, best_rd


F64_MAX = 1.7976931348623157e308      # f64::MAX: "no cost" of the partition search


def _partition_children(partition):
    """how many entries of a node's four children a partition type visits (get_sub_partitions, src/rdo.rs:1825-1846)"""
    return {0: 1, 1: 2, 2: 2, 3: 4}[int(partition)]


def partition_pick_bottomup(best_rd, partition, lam, rate, children, must_split=False, ref_rd=F64_MAX,
                            enable_early_exit=True):
    """One trial of encode_partition_bottomup (src/encoder.rs:2683-2843) -- the statement r1_rd_partition_pick_batch is
    held to under R1_PART_BOTTOMUP.  best_rd: what the node holds (f64::MAX: nothing); rate: the partition symbol's
    tell_frac difference in 1/8 bit, None for the reference's 0.0 arm; children: up to four costs, None = absent.
    Python floats add as the reference's f64: cost + c0, then + c1, ... each rounded on its own.
    -> (kept, rd, early_exit): kept says whether best_rd becomes rd and best_partition the trial's."""
    cost = 0.0 if rate is None else compute_rd_cost(lam, rate, 0)
    kids = list(children)[:_partition_children(partition)]
    if int(partition) == 0:
        if not kids or kids[0] is None:
            return False, 0.0, False
        return True, kids[0] + cost, False                                 # 2708-2711: unconditionally
    rd = cost
    for c in kids:
        if c is None or c == F64_MAX:                                      # 2802, 2820
            continue
        rd = rd + c
        if not must_split and enable_early_exit and (rd >= best_rd or rd >= ref_rd):   # 2822-2828
            return False, rd, True
    return rd < best_rd, rd, False                                         # 2835


def partition_pick_topdown(best_rd, partition, lam, rate, children, enable_early_exit=True):
    """One trial of rdo_partition_decision (src/rdo.rs:1849-2024; rdo_partition_none / rdo_partition_simple) -- the
    statement of R1_PART_TOPDOWN.  best_rd: cached_block.rd_cost or what an earlier trial left.  The children are summed
    from 0.0 and the partition cost is added to the sum LAST; the early exit looks at the sum without the cost.
    -> (kept, rd, early_exit); a refused trial (an absent child, or the early exit) keeps nothing."""
    kids = list(children)[:_partition_children(partition)]
    if int(partition) == 0:
        if not kids or kids[0] is None:
            return False, 0.0, False
        return kids[0] < best_rd, kids[0], False                           # 1856-1861, 2006: no partition symbol
    cost = 0.0 if rate is None else compute_rd_cost(lam, rate, 0)
    total = 0.0
    for c in kids + [None] * (_partition_children(partition) - len(kids)):
        if c is None:                                                      # 1933-1936
            return False, total, False
        total = total + c
        if enable_early_exit and total > best_rd:                          # 1912
            return False, total, True
    rd = cost + total                                                      # 1939
    return rd < best_rd, rd, False


# ---- the head symbols of an intra block of an intra frame (r1_intra_head_rate_batch, r1_partition_rate_batch,
# r1_intra_head_commit_batch); pinned by tests/golden/head_ref.npz / tests/test_head_ref.py
HEAD_REFUSED = "refused"    # what the device answers with rate 0xFFFFFFFF (the reference would assert! or index out of range)
_INTRA_MODE_CONTEXT = (0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0)     # write_intra_mode_kf, src/context/block_unit.rs:703-704
_PARTITION_GATHER = {2: (2, 3, 4, 6, 7, 9),      # partition_gather_vert_alike (partition_unit.rs:163-193): VERT, SPLIT,
                     1: (1, 3, 4, 5, 6, 8)}      # HORZ_A, VERT_A, VERT_B, VERT_4; _horz_alike (131-161): HORZ, SPLIT, ..
_BLOCK_8X8, _BLOCK_32X32 = 3, 9


def _head_block_ok(bsize, bo_x, bo_y, mi_cols, mi_rows):
    return (0 <= int(bsize) < 22 and max(BlockSize(bsize).dims) <= 64 and 0 <= bo_x < mi_cols <= 1024 and
            0 <= bo_y < mi_rows)


def partition_context(above_partition, left_partition, bo_x, bo_y, bsize):
    """partition_plane_context (src/context/partition_unit.rs:416-429) of a square block of 8x8 and up"""
    w, h = BlockSize(bsize).dims
    assert w == h and w >= 8
    bsl = w.bit_length() - 4
    above = (int(above_partition[bo_x >> 1]) >> bsl) & 1
    left = (int(left_partition[(bo_y % 16) >> 1]) >> bsl) & 1
    return left * 2 + above + bsl * 4


def partition_symbol(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, partition):
    """write_partition (src/context/partition_unit.rs:267-357) as one symbol: None where it writes nothing (neither rows
    nor columns), HEAD_REFUSED where it asserts (a block below 8x8 or not square, a type the edge does not admit, an 8x8
    at an edge) or where the device refuses (a 128-point size, a place outside the tile), else
    (field, row, n, symbol, gather): field / row name the CDF row -- `partition_w8` for ctx < 4, else `partition`[ctx - 4];
    n its symbol count; gather 0 for a symbol written with its update, 2 / 1 for the two-entry CDF of
    partition_gather_vert_alike / _horz_alike written with w.symbol alone: nothing adapts."""
    if not _head_block_ok(bsize, bo_x, bo_y, mi_cols, mi_rows) or not 0 <= int(partition) <= 3:
        return HEAD_REFUSED
    w, h = BlockSize(bsize).dims
    if w != h or w < 8:
        return HEAD_REFUSED
    hbs = (w >> MI_SIZE_LOG2) // 2
    has_cols, has_rows = bo_x + hbs < mi_cols, bo_y + hbs < mi_rows
    ctx = partition_context(nbr["above_partition"], nbr["left_partition"], bo_x, bo_y, bsize)
    if not has_rows and not has_cols:
        return None
    field, row, n = ("partition_w8", ctx, 4) if ctx < 4 else ("partition", ctx - 4, 10)
    if has_rows and has_cols:
        return field, row, n, int(partition), 0
    if int(partition) not in ((3, 1) if has_cols else (3, 2)) or int(bsize) <= _BLOCK_8X8:
        return HEAD_REFUSED
    return field, row, n, int(int(partition) == 3), 2 if has_cols else 1


def tx_size_symbol(nbr, bsize, bo_x, bo_y, tx_size):
    """write_tx_size_intra (src/context/transform_unit.rs:576-667) for an intra frame: -> (field, row, n, depth) or
    HEAD_REFUSED where tx_size is no depth 0..2 of the block.  above_tx_context / left_tx_context are read raw; has_above
    / has_left are the tile's."""
    mw, mh = BlockSize(bsize).dims                       # max_txsize_rect_lookup: the block itself up to 64x64
    t = TxSize.by_dims(mw, mh)
    depth = 0
    while int(t) != int(tx_size):
        if depth == 2 or sub_tx_size(t) == t:
            return HEAD_REFUSED
        t, depth = sub_tx_size(t), depth + 1
    t, steps = TxSize.by_dims(mw, mh), 0
    while int(t) != 0:
        t, steps = sub_tx_size(t), steps + 1
    above = int(int(nbr["above_tx"][bo_x]) >= mw)
    left = int(int(nbr["left_tx"][bo_y % 16]) >= mh)
    ctx = (above if bo_y > 0 else 0) + (left if bo_x > 0 else 0)
    if steps - 1 > 0:
        return ("tx_size", (steps - 2, ctx), 3, depth)
    return ("tx_size_8x8", ctx, 2, depth)


def head_symbols(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma_, tx_mode_select, y_mode, uv_mode, angle_y,
                 angle_uv, alpha_u, alpha_v, tx_size, coded=False):
    """What one intra mode trial of an intra frame writes in front of its coefficients (src/rdo.rs:870-877 and
    encode_block_pre_cdef / encode_block_post_cdef, src/encoder.rs:1913, 2086-2102, 2132-2136), skip = false: the
    statement of r1_intra_head_rate_batch.  nbr: the arrays of a types.HEAD_NBR_CONTEXT record (never written).
    -> HEAD_REFUSED, or the list of (field, row, n, symbol, gather) in coding order, as partition_symbol returns them:
    partition (PARTITION_NONE, for a square block of 8x8 and up), skip, kf_y, angle_delta (directional, bsize >= BLOCK_8X8
    IN THE ENUM'S ORDER: 4x16 and 16x4 write one), uv_mode_cfl / uv_mode, cfl_sign and cfl_alpha, angle_delta again,
    tx_size_8x8 / tx_size.  Two symbols may name one row (equal directional modes; equal CFL signs): the second is
    written on what the first adapted.
    coded=True: the block as it is coded for real (encode_block_pre_cdef / encode_block_post_cdef alone), the symbols
    r1_intra_head_commit_batch replays: without the trial's PARTITION_NONE -- the real partition symbol is the walker's
    (src/encoder.rs:2688, 2781, 2862), the commit's partition event."""
    if not _head_block_ok(bsize, bo_x, bo_y, mi_cols, mi_rows):
        return HEAD_REFUSED
    bsize, y_mode, uv_mode = int(bsize), int(y_mode), int(uv_mode)
    if not 0 <= y_mode < 13:
        return HEAD_REFUSED
    w, h = BlockSize(bsize).dims
    syms = []
    if not coded and bsize >= _BLOCK_8X8 and w == h:
        p = partition_symbol(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, 0)
        if p == HEAD_REFUSED:
            return HEAD_REFUSED
        if p is not None:
            syms.append(p)
    above_skip = bo_y > 0 and bool(nbr["above_skip"][bo_x])
    left_skip = bo_x > 0 and bool(nbr["left_skip"][bo_y % 16])
    syms.append(("skip", int(above_skip) + int(left_skip), 2, 0, 0))
    above_mode = int(nbr["above_mode"][bo_x]) if bo_y > 0 else 0
    left_mode = int(nbr["left_mode"][bo_y % 16]) if bo_x > 0 else 0
    if above_mode >= 13 or left_mode >= 13:
        return HEAD_REFUSED
    syms.append(("kf_y", (_INTRA_MODE_CONTEXT[above_mode], _INTRA_MODE_CONTEXT[left_mode]), 13, y_mode, 0))
    directional = lambda m: 1 <= m <= 8                  # V_PRED ..= D67_PRED (src/predict.rs:262-264)
    if directional(y_mode) and bsize >= _BLOCK_8X8:
        if not -3 <= int(angle_y) <= 3:
            return HEAD_REFUSED
        syms.append(("angle_delta", y_mode - 1, 7, int(angle_y) + 3, 0))
    if has_chroma_:
        cfl_allowed = bsize <= _BLOCK_32X32              # BlockSize::cfl_allowed (src/partition.rs:228-231), enum order
        if not 0 <= uv_mode < (14 if cfl_allowed else 13):
            return HEAD_REFUSED
        syms.append(("uv_mode_cfl" if cfl_allowed else "uv_mode", y_mode, 14 if cfl_allowed else 13, uv_mode, 0))
        if uv_mode == 13:
            au, av = int(alpha_u), int(alpha_v)
            if (au == 0 and av == 0) or not (-16 <= au <= 16 and -16 <= av <= 16):
                return HEAD_REFUSED
            sign = [1 if a < 0 else (2 if a > 0 else 0) for a in (au, av)]      # CFLSign::from_alpha
            syms.append(("cfl_sign", (), 8, sign[0] * 3 + sign[1] - 1, 0))
            for uv, a in enumerate((au, av)):
                if sign[uv]:
                    syms.append(("cfl_alpha", (sign[uv] - 1) * 3 + sign[1 - uv], 16, abs(a) - 1, 0))
        if directional(uv_mode) and bsize >= _BLOCK_8X8:
            if not -3 <= int(angle_uv) <= 3:
                return HEAD_REFUSED
            syms.append(("angle_delta", uv_mode - 1, 7, int(angle_uv) + 3, 0))
    if tx_mode_select and bsize > 0:
        t = tx_size_symbol(nbr, bsize, bo_x, bo_y, tx_size)
        if t == HEAD_REFUSED:
            return HEAD_REFUSED
        syms.append(t + (0,))
    elif not 0 <= int(tx_size) < 19:
        return HEAD_REFUSED
    return syms


def head_nbr_store(nbr, bsize, bo_x, bo_y, mi_cols, mi_rows, y_mode, tx_size, tx_mode_select, node=None):
    """What a coded intra block (skip = false) leaves in the arrays of a types.HEAD_NBR_CONTEXT record, IN PLACE -- the
    stores of r1_intra_head_commit_batch: set_skip / set_mode over the block's extent clipped to the tile as
    TileBlocksMut::for_each clips (src/tiling/tile_blocks.rs:206-224), as row buffers: above_mode / above_skip [bo_x ..],
    left_mode / left_skip [bo_y % 16 ..]; with tx_mode_select update_tx_size_context (src/context/block_unit.rs:362-386):
    the transform's width over above_tx[bo_x .. bo_x + bw / 4], its height over left_tx[bo_y % 16 ..], clipped to the
    arrays; node = (node_x, node_y, node_bsize, subsize): update_partition_context (partition_unit.rs:480-503) of the
    walker's node."""
    w, h = BlockSize(bsize).dims
    bw4, bh4 = w >> MI_SIZE_LOG2, h >> MI_SIZE_LOG2
    cw = mi_cols - bo_x if bo_x + bw4 >= mi_cols else bw4
    for k in range(cw):
        nbr["above_mode"][bo_x + k], nbr["above_skip"][bo_x + k] = int(y_mode), 0
    for k in range(bh4):
        if bo_y + k < mi_rows:
            nbr["left_mode"][(bo_y + k) % 16], nbr["left_skip"][(bo_y + k) % 16] = int(y_mode), 0
    if tx_mode_select:
        tw, th = TxSize(tx_size).dims
        for k in range(bw4):
            if bo_x + k < len(nbr["above_tx"]):
                nbr["above_tx"][bo_x + k] = tw
        for k in range(bh4):
            if bo_y % 16 + k < 16:
                nbr["left_tx"][bo_y % 16 + k] = th
    if node is not None:
        node_x, node_y, node_bsize, subsize = node
        nw, nh = BlockSize(node_bsize).dims
        sw, sh = BlockSize(subsize).dims
        # partition_context_lookup[subsize]: the bits of the sizes the sub-block is smaller than (partition_unit.rs:15-38)
        above, left = 31 & ~((sw >> 2) - 1), 31 & ~((sh >> 2) - 1)
        for k in range((nw >> 2) >> 1):
            if (node_x >> 1) + k < len(nbr["above_partition"]):
                nbr["above_partition"][(node_x >> 1) + k] = above
        for k in range((nh >> 2) >> 1):
            if ((node_y % 16) >> 1) + k < 8:
                nbr["left_partition"][((node_y % 16) >> 1) + k] = left


def head_nbr_reset_left(nbr):
    """The head part of reset_left_contexts (src/context/block_unit.rs:356-360, 388-401), IN PLACE: the statement of
    r1_head_nbr_reset_left_batch.  left_mode / left_skip stay: the reference's blocks array is not reset."""
    for name in ("left_partition", "left_tx"):
        for k in range(len(nbr[name])):
            nbr[name][k] = 0


# ---- the MV reference stack of an inter block (r1_mvref_stack_batch, r1_mvref_pmv_batch) and the tile's blocks array it
# is built from (r1_tile_blocks_reset_batch, r1_tile_blocks_store_batch); pinned by tests/golden/mvref_ref.npz /
# tests/test_mvref_ref.py.  A tile is a dict: `cells`, a (rows, cols) array of types.TILE_BLOCK, and tile_x, tile_y,
# frame_cols, frame_rows in 4x4 units.
MV_REFUSED = "refused"      # what the device answers with count 0xFF (the reference would panic, or the ABI is left)
INTRA_FRAME, NONE_FRAME = 0, 8
NEARESTMV = 14              # Block::is_inter: mode >= NEARESTMV (src/context/block_unit.rs:186-188)
REF_CAT_LEVEL = 640
MAX_REF_MV_STACK_SIZE = 8
_NEWMV_MODES = frozenset((19, 24, 25, 26, 27, 28, 29, 30, 31, 33))      # PredictionMode::has_newmv (src/predict.rs:173-184)
_BLOCK_64X64 = 12


def tile_blocks_default(rows, cols):
    """Block::default() (src/context/block_unit.rs:194-211) over a fresh array: the statement of
    r1_tile_blocks_reset_batch"""
    cells = np.zeros((rows, cols), TILE_BLOCK)
    cells["n4_w"], cells["n4_h"], cells["bsize"] = 16, 16, _BLOCK_64X64
    return cells


def tile_blocks_store(tile, bo_x, bo_y, bsize, mode, ref_frames, mvs, skip):
    """What a coded block leaves in the tile's blocks array, IN PLACE: set_skip, set_block_size, set_mode, set_ref_frames
    and set_motion_vectors (src/encoder.rs:1900, 1968-1972) over the block's extent clipped as TileBlocksMut::for_each
    clips it (src/tiling/tile_blocks.rs:206-224): the width is cut to the tile where bo_x + bw >= cols, rows past the tile
    are left out.  An intra winner (mode < NEARESTMV) stores {INTRA_FRAME, NONE_FRAME} and zero vectors.  The statement
    of r1_tile_blocks_store_batch."""
    cells = tile["cells"]
    rows, cols = cells.shape
    w, h = BlockSize(bsize).dims
    bw, bh = w >> MI_SIZE_LOG2, h >> MI_SIZE_LOG2
    if int(mode) < NEARESTMV:
        ref_frames, mvs = (INTRA_FRAME, NONE_FRAME), ((0, 0), (0, 0))
    cw = cols - bo_x if bo_x + bw >= cols else bw
    for y in range(bo_y, bo_y + bh):
        if y >= rows:
            continue
        for x in range(bo_x, bo_x + cw):
            c = cells[y, x]
            c["mv"], c["ref_frames"], c["mode"] = mvs, ref_frames, int(mode)
            c["n4_w"], c["n4_h"], c["bsize"], c["skip"] = bw, bh, int(bsize), int(bool(skip))


def has_tr(bo_x, bo_y, bsize):
    """has_tr (src/partition.rs:900-955): whether the block's top-right neighbour is coded before it, by its place in a
    64x64 superblock.  (has_top_right above is the intra edge rule: another rule.)"""
    w, h = BlockSize(bsize).dims
    n4_w, n4_h = w >> MI_SIZE_LOG2, h >> MI_SIZE_LOG2
    mask_row, mask_col = bo_y & (SB_MI - 1), bo_x & (SB_MI - 1)
    bs = max(n4_w, n4_h)
    if bs > SB_MI:
        return False
    tr = not ((mask_row & bs) != 0 and (mask_col & bs) != 0)
    while bs < SB_MI:
        if (mask_col & bs) == 0:
            break
        if (mask_col & (2 * bs)) != 0 and (mask_row & (2 * bs)) != 0:
            tr = False
            break
        bs <<= 1
    if n4_w < n4_h and (bo_x & n4_w) == 0:      # the left of two vertical rectangles
        tr = True
    if n4_w > n4_h and (bo_y & n4_h) != 0:      # the bottom of two horizontal rectangles
        tr = False
    return tr


class _MvRefused(Exception):
    pass


def find_mvrefs(tile, bo_x, bo_y, bsize, ref_frames, is_compound, sign_bias):
    """find_mvrefs / setup_mvref_list (src/context/block_unit.rs:795-1442): the statement of r1_mvref_stack_batch.
    sign_bias: fi.ref_frame_sign_bias, entry r - 1 for reference r (RefType::to_index).
    -> MV_REFUSED, or (mode_context, [(this_row, this_col, comp_row, comp_col, weight), ..]) sorted by descending weight,
    ties in insertion order, at most 9 entries, the vectors clamped around the block's place IN THE FRAME."""
    cells = tile["cells"]
    rows, cols = cells.shape
    r0, r1 = int(ref_frames[0]), int(ref_frames[1])
    is_compound = bool(is_compound)
    if not 0 <= int(bsize) < 22 or max(BlockSize(bsize).dims) > 64 or not (0 <= bo_x < cols <= 1024 and 0 <= bo_y < rows):
        return MV_REFUSED
    if r0 == NONE_FRAME or r0 > NONE_FRAME or r1 > NONE_FRAME or (is_compound and r1 in (INTRA_FRAME, NONE_FRAME)):
        return MV_REFUSED
    if r0 == INTRA_FRAME:
        return 0, []
    w, h = BlockSize(bsize).dims
    n4_w, n4_h = w >> MI_SIZE_LOG2, h >> MI_SIZE_LOG2
    stack = []                                   # [this_row, this_col, comp_row, comp_col, weight]
    st = {"rows": 0, "cols": 0, "newmv": 0}
    wrap = lambda v: ((v + 0x8000) & 0xFFFF) - 0x8000                           # i16, as the device negates
    neg = lambda mv: (wrap(-mv[0]), wrap(-mv[1]))

    def cell(x, y):
        if not (0 <= x < cols and 0 <= y < rows):
            raise _MvRefused                     # the reference indexes past the row (it panics)
        c = cells[y, x]
        if int(c["n4_w"]) not in (1, 2, 4, 8, 16) or int(c["n4_h"]) not in (1, 2, 4, 8, 16):
            raise _MvRefused
        return c

    def add_ref_mv_candidate(c, weight, count_key):
        if int(c["mode"]) < NEARESTMV:
            return False
        refs = (int(c["ref_frames"][0]), int(c["ref_frames"][1]))
        mvs = [(int(c["mv"][i][0]), int(c["mv"][i][1])) for i in range(2)]
        newmv = int(c["mode"]) in _NEWMV_MODES
        if is_compound:
            if refs != (r0, r1):
                return False
            keys = [mvs[0] + mvs[1]]
        else:
            keys = [mvs[i] + (0, 0) for i in range(2) if refs[i] == r0]
        for key in keys:
            n = 4 if is_compound else 2          # a single search compares this_mv alone
            for e in stack:
                if tuple(e[:n]) == key[:n]:
                    e[4] += weight
                    break
            else:
                if len(stack) < MAX_REF_MV_STACK_SIZE:
                    stack.append(list(key) + [weight])
            if newmv and count_key:
                st[count_key] += 1
        return bool(keys)

    def scan(horizontal, offset, max_offs, count_key):
        """scan_row_mbmi (horizontal) / scan_col_mbmi: 967-1097"""
        target, other_n4 = (n4_w, "n4_h") if horizontal else (n4_h, "n4_w")
        along_n4 = "n4_w" if horizontal else "n4_h"
        pos, room = (bo_x, cols - bo_x) if horizontal else (bo_y, rows - bo_y)
        end_mi = min(target, room, 16)
        shift = 0
        if abs(offset) > 1:
            shift = 1
            if (pos & 1) and target < 2:
                shift -= 1
        found = False
        i = 0
        while i < end_mi:
            c = cell(bo_x + shift + i, bo_y + offset) if horizontal else cell(bo_x + offset, bo_y + shift + i)
            n4 = int(c[along_n4])
            length = min(target, n4)
            if target >= 16:
                length = max(4, length)
            elif abs(offset) > 1:
                length = max(length, 2)
            weight = 2
            if 2 <= target <= n4:
                inc = min(-max_offs + offset + 1, int(c[other_n4]))
                if inc < 0:
                    raise _MvRefused             # assert!(inc >= 0)
                weight = max(weight, inc)
                st["rows" if horizontal else "cols"] = inc - offset - 1
            if add_ref_mv_candidate(c, length * weight, count_key):
                found = True
            i += length
        return found

    def scan_blk(x, y, count_key):
        if x >= cols or y >= rows:
            return False
        return add_ref_mv_candidate(cell(x, y), 4, count_key)

    try:
        row_adj, col_adj = int(n4_h < 2 and (bo_y & 1)), int(n4_w < 2 and (bo_x & 1))
        up_avail, left_avail = bo_y > 0, bo_x > 0
        max_row_offs = max_col_offs = 0
        if up_avail:
            max_row_offs = (-4 if n4_h < 2 else -6) + row_adj
            max_row_offs = min(max(max_row_offs, -bo_y), rows - bo_y - 1)       # find_valid_row_offs
        if left_avail:
            max_col_offs = (-4 if n4_w < 2 else -6) + col_adj
            max_col_offs = min(max(max_col_offs, -bo_x), cols - bo_x - 1)
        row_match = col_match = False
        if abs(max_row_offs) >= 1:
            row_match |= scan(True, -1, max_row_offs, "newmv")
        if abs(max_col_offs) >= 1:
            col_match |= scan(False, -1, max_col_offs, "newmv")
        if has_tr(bo_x, bo_y, bsize) and bo_y > 0:
            row_match |= scan_blk(bo_x + n4_w, bo_y - 1, "newmv")
        nearest_match = int(row_match) + int(col_match)
        for e in stack:                                                        # add_offset
            e[4] += REF_CAT_LEVEL
        if bo_x > 0 and bo_y > 0:
            row_match |= scan_blk(bo_x - 1, bo_y - 1, None)
        for idx in (2, 3):
            row_offset, col_offset = -2 * idx + 1 + row_adj, -2 * idx + 1 + col_adj
            if abs(row_offset) <= abs(max_row_offs) and abs(row_offset) > st["rows"]:
                row_match |= scan(True, row_offset, max_row_offs, None)
            if abs(col_offset) <= abs(max_col_offs) and abs(col_offset) > st["cols"]:
                col_match |= scan(False, col_offset, max_col_offs, None)
        total_match = int(row_match) + int(col_match)
        newmv = min(st["newmv"], 1)
        if nearest_match == 0:
            mode_context = min(total_match, 1) + (total_match << 4)
        elif nearest_match == 1:
            mode_context = 3 - newmv + ((2 + total_match) << 4)
        else:
            mode_context = 5 - newmv + (5 << 4)
        stack.sort(key=lambda e: -e[4])                                        # sort_by: stable, descending weight
        if len(stack) < 2:                                                     # 7.10.2.12, the extra search
            num4x4 = min(n4_w, 16, cols - bo_x, n4_h, rows - bo_y)
            id_mvs, diff_mvs = ([], []), ([], [])
            for pas in range(int(not up_avail), int(left_avail) + 1):
                idx = 0
                while idx < num4x4 and len(stack) < 2:
                    c = cell(bo_x + idx, bo_y - 1) if pas == 0 else cell(bo_x - 1, bo_y + idx)
                    for k in range(2):
                        cand_ref = int(c["ref_frames"][k])
                        if cand_ref in (INTRA_FRAME, NONE_FRAME):
                            continue
                        if cand_ref > NONE_FRAME:
                            raise _MvRefused                                   # to_index past ref_frame_sign_bias
                        mv = (int(c["mv"][k][0]), int(c["mv"][k][1]))
                        if is_compound:
                            for lst, want in enumerate((r0, r1)):
                                if cand_ref == want and len(id_mvs[lst]) < 2:
                                    id_mvs[lst].append(mv)
                                elif len(diff_mvs[lst]) < 2:
                                    flip = bool(sign_bias[cand_ref - 1]) != bool(sign_bias[want - 1])
                                    diff_mvs[lst].append(neg(mv) if flip else mv)
                        else:
                            if bool(sign_bias[cand_ref - 1]) != bool(sign_bias[r0 - 1]):
                                mv = neg(mv)
                            if all((e[0], e[1]) != mv for e in stack):
                                stack.append([mv[0], mv[1], 0, 0, 2])
                    idx += int(c["n4_w"]) if pas == 0 else int(c["n4_h"])
            if is_compound:
                combined = [[(0, 0), (0, 0)], [(0, 0), (0, 0)]]
                for lst in range(2):
                    both = (id_mvs[lst] + diff_mvs[lst])[:2]
                    for k, mv in enumerate(both):
                        combined[k][lst] = mv
                if len(stack) == 1:
                    first = combined[0][0] + combined[0][1]
                    pick = combined[1] if tuple(stack[0][:4]) == first else combined[0]
                    stack.append(list(pick[0] + pick[1]) + [2])
                else:
                    for k in range(2):
                        stack.append(list(combined[k][0] + combined[k][1]) + [2])
    except _MvRefused:
        return MV_REFUSED
    fx, fy = int(tile["tile_x"]) + bo_x, int(tile["tile_y"]) + bo_y            # the clamp is on the frame's coordinates
    border_w, border_h = 128 + w * 8, 128 + h * 8
    x_min, x_max = -fx * 32 - border_w, (int(tile["frame_cols"]) - fx - n4_w) * 32 + border_w
    y_min, y_max = -fy * 32 - border_h, (int(tile["frame_rows"]) - fy - n4_h) * 32 + border_h
    out = []
    for e in stack:
        out.append((min(max(e[0], y_min), y_max), min(max(e[1], x_min), x_max),
                    min(max(e[2], y_min), y_max), min(max(e[3], x_min), x_max), e[4]))
    return mode_context, out


def mvref_pmv(stack):
    """pmv of estimate_motion from a stack (src/rdo.rs:1175-1181): the statement of r1_mvref_pmv_batch"""
    return tuple((stack[k][0], stack[k][1]) if len(stack) > k else (0, 0) for k in range(2))

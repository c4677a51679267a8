"""Enums with the reference's integer values (they index its dispatch tables).

BlockSize   src/partition.rs:130-153      TxSize  src/transform/mod.rs:101-123
TxType      src/transform/mod.rs:56-74    FilterMode  src/mc.rs:100-106

COEFF_CDFS / TXB_CTX: the NumPy mirrors of R1CoeffCdfs / R1TxbCtx (include/rav1e_amd.h, r1_coeff_rate_batch); the
dimensions are the reference's (src/context/transform_unit.rs:27, 200-219).  TXB_CHAIN_CTX: R1TxbChainCtx
(r1_coeff_rate_chain_batch).  BLOCK_CHAIN_CTX / BLOCK_RATE_TRIAL: R1BlockChainCtx / R1BlockRateTrial
(r1_coeff_rate_block_batch).  COEFF_CDF_CONTEXT: R1CoeffCdfContext (r1_coeff_cdf_slice_batch, r1_coeff_cdf_adapt_batch).
COEFF_NBR_CONTEXT / NBR_BLOCK: R1CoeffNbrContext / R1NbrBlock (r1_coeff_nbr_gather_batch, r1_coeff_nbr_store_batch).
PartitionType  src/partition.rs:114-126; PART_PICK: R1PartPick (r1_rd_partition_pick_batch, r1_part_select_batch).
HEAD_CDF_CONTEXT / HEAD_NBR_CONTEXT / HEAD_BLOCK / HEAD_TRIAL / HEAD_COMMIT: R1HeadCdfContext / R1HeadNbrContext /
R1HeadBlock / R1HeadTrial / R1HeadCommit (r1_intra_head_rate_batch, r1_partition_rate_batch, r1_intra_head_commit_batch).
TILE_BLOCK / TILE_BLOCKS / MV_BLOCK / MV_QUERY / CANDIDATE_MV / MV_STACK / MV_TRIAL: R1TileBlock / R1TileBlocks / R1MvBlock /
R1MvQuery / R1CandidateMv / R1MvStack / R1MvTrial (r1_tile_blocks_*_batch, r1_mvref_stack_batch, r1_mvref_pmv_batch).
"""
import enum

import numpy as np


class BlockSize(enum.IntEnum):
    BLOCK_4X4 = 0
    BLOCK_4X8 = 1
    BLOCK_8X4 = 2
    BLOCK_8X8 = 3
    BLOCK_8X16 = 4
    BLOCK_16X8 = 5
    BLOCK_16X16 = 6
    BLOCK_16X32 = 7
    BLOCK_32X16 = 8
    BLOCK_32X32 = 9
    BLOCK_32X64 = 10
    BLOCK_64X32 = 11
    BLOCK_64X64 = 12
    BLOCK_64X128 = 13
    BLOCK_128X64 = 14
    BLOCK_128X128 = 15
    BLOCK_4X16 = 16
    BLOCK_16X4 = 17
    BLOCK_8X32 = 18
    BLOCK_32X8 = 19
    BLOCK_16X64 = 20
    BLOCK_64X16 = 21

    @property
    def dims(self):
        w, h = self.name.split("_")[1].split("X")
        return int(w), int(h)


class TxSize(enum.IntEnum):
    TX_4X4 = 0
    TX_8X8 = 1
    TX_16X16 = 2
    TX_32X32 = 3
    TX_64X64 = 4
    TX_4X8 = 5
    TX_8X4 = 6
    TX_8X16 = 7
    TX_16X8 = 8
    TX_16X32 = 9
    TX_32X16 = 10
    TX_32X64 = 11
    TX_64X32 = 12
    TX_4X16 = 13
    TX_16X4 = 14
    TX_8X32 = 15
    TX_32X8 = 16
    TX_16X64 = 17
    TX_64X16 = 18

    @property
    def dims(self):
        w, h = self.name.split("_")[1].split("X")
        return int(w), int(h)

    @staticmethod
    def by_dims(w, h):
        return TxSize["TX_%dX%d" % (w, h)]


TX_DIMS = [t.dims for t in TxSize]


class TxType(enum.IntEnum):
    DCT_DCT = 0
    ADST_DCT = 1
    DCT_ADST = 2
    ADST_ADST = 3
    FLIPADST_DCT = 4
    DCT_FLIPADST = 5
    FLIPADST_FLIPADST = 6
    ADST_FLIPADST = 7
    FLIPADST_ADST = 8
    IDTX = 9
    V_DCT = 10
    H_DCT = 11
    V_ADST = 12
    H_ADST = 13
    V_FLIPADST = 14
    H_FLIPADST = 15
    WHT_WHT = 16


class FilterMode(enum.IntEnum):
    REGULAR = 0
    SMOOTH = 1
    SHARP = 2
    BILINEAR = 3


class PartitionType(enum.IntEnum):
    """the four the encoder tries (RAV1E_PARTITION_TYPES) with the reference's discriminants; PARTITION_INVALID is the
    device state's "nothing kept", -1 (the reference's own discriminant, 10, indexes nothing)"""
    PARTITION_NONE = 0
    PARTITION_HORZ = 1
    PARTITION_VERT = 2
    PARTITION_SPLIT = 3
    PARTITION_INVALID = -1


class DistKind(enum.IntEnum):
    SAD = 0
    SATD = 1


def valid_av1_transform(tx_size, tx_type):
    """src/transform/mod.rs:405-417 (+ WHT exists only at 4x4)."""
    w, h = TX_DIMS[int(tx_size)]
    m = max(w, h)
    if int(tx_type) == 16:
        return (w, h) == (4, 4)
    if m == 64:
        return int(tx_type) == 0
    if m == 32:
        return int(tx_type) in (0, 9)
    return True


# ---- r1_coeff_rate_batch: the (txs_ctx, plane_type) slice of the reference's CDFContext, and a block's contexts
TXB_SKIP_CONTEXTS, EOB_COEF_CONTEXTS, SIG_COEF_CONTEXTS_EOB, SIG_COEF_CONTEXTS = 13, 9, 4, 42
LEVEL_CONTEXTS, BR_CDF_SIZE, DC_SIGN_CONTEXTS, INTRA_MODES = 21, 4, 3, 13
COEFF_CDFS = np.dtype([("txb_skip", "<u2", (TXB_SKIP_CONTEXTS, 2)), ("eob_flag", "<u2", (2, 11)),
                       ("eob_extra", "<u2", (EOB_COEF_CONTEXTS, 2)),
                       ("coeff_base_eob", "<u2", (SIG_COEF_CONTEXTS_EOB, 3)),
                       ("coeff_base", "<u2", (SIG_COEF_CONTEXTS, 4)), ("coeff_br", "<u2", (LEVEL_CONTEXTS, BR_CDF_SIZE)),
                       ("dc_sign", "<u2", (DC_SIGN_CONTEXTS, 2)), ("tx_type", "<u2", (INTRA_MODES, 16))])
TXB_CTX = np.dtype([("txb_skip_ctx", "u1"), ("dc_sign_ctx", "u1"), ("y_mode", "u1"), ("cdf_sel", "u1")])
COEFF_RATE_INVALID = 0xFFFFFFFF      # the rate of a slot whose device-resident inputs are out of range
# R1TxbChainCtx (r1_coeff_rate_chain_batch): a block's neighbour contexts and edges in front of its transform blocks
TXB_CHAIN_CTX = np.dtype([("above", "u1", (16,)), ("left", "u1", (16,)), ("mi_w", "u1"), ("mi_h", "u1"),
                          ("clip_w4", "u1"), ("clip_h4", "u1"), ("y_mode", "u1"), ("cdf_sel", "u1"),
                          ("reserved", "u1", (2,))])
# R1BlockChainCtx / R1BlockRateTrial (r1_coeff_rate_block_batch): the same for luma, U and V -- ctx[plane][0: above,
# 1: left][16] -- and one trial's place in the coefficient arrays, its transform types and the writer's rng in front
BLOCK_CHAIN_CTX = np.dtype([("ctx", "u1", (3, 2, 16)), ("mi_w", "u1"), ("mi_h", "u1"), ("clip_w4", "u1"),
                            ("clip_h4", "u1"), ("clip_uv_w4", "u1"), ("clip_uv_h4", "u1"), ("y_mode", "u1"),
                            ("cdf_sel", "u1"), ("cdf_sel_uv", "u1"), ("reserved", "u1", (3,))])
BLOCK_RATE_TRIAL = np.dtype([("first_y", "<u4"), ("first_u", "<u4"), ("first_v", "<u4"), ("block", "<u4"), ("rng", "<u2"),
                             ("tx_type", "u1"), ("uv_tx_type", "u1"), ("do_chroma", "u1"), ("reserved", "u1", (3,))])
# R1RdPick (r1_rd_pick_batch / r1_rd_commit_batch): the decision state of one block, carried from call to call
RD_PICK = np.dtype([("best_rd", "<f8"), ("best_dist", "<u8"), ("best_rate", "<u4"), ("best_row", "<i2"),
                    ("best_slot", "i1"), ("best_call", "i1")])
assert RD_PICK.itemsize == 24
# R1CoeffCdfContext (r1_coeff_cdf_slice_batch / r1_coeff_cdf_adapt_batch): the coefficient side of the reference's
# CDFContext in its own shapes (src/context/cdf_context.rs:23-96), padded to a multiple of 16 bytes
TX_SIZES, PLANE_TYPES, TX_SIZE_SQR_CONTEXTS = 5, 2, 4
COEFF_CDF_CONTEXT = np.dtype(
    [("txb_skip", "<u2", (TX_SIZES, TXB_SKIP_CONTEXTS, 2)),
     ("eob_extra", "<u2", (TX_SIZES, PLANE_TYPES, EOB_COEF_CONTEXTS, 2)),
     ("coeff_base_eob", "<u2", (TX_SIZES, PLANE_TYPES, SIG_COEF_CONTEXTS_EOB, 3)),
     ("coeff_base", "<u2", (TX_SIZES, PLANE_TYPES, SIG_COEF_CONTEXTS, 4)),
     ("coeff_br", "<u2", (TX_SIZES, PLANE_TYPES, LEVEL_CONTEXTS, BR_CDF_SIZE)),
     ("dc_sign", "<u2", (PLANE_TYPES, DC_SIGN_CONTEXTS, 2))]
    + [("eob_flag%d" % (16 << k), "<u2", (PLANE_TYPES, 2, 5 + k)) for k in range(7)]
    + [("intra_tx_1", "<u2", (TX_SIZE_SQR_CONTEXTS, INTRA_MODES, 7)), ("intra_tx_2", "<u2", (TX_SIZE_SQR_CONTEXTS, INTRA_MODES, 5)),
       ("inter_tx_1", "<u2", (TX_SIZE_SQR_CONTEXTS, 16)), ("inter_tx_2", "<u2", (TX_SIZE_SQR_CONTEXTS, 12)),
       ("inter_tx_3", "<u2", (TX_SIZE_SQR_CONTEXTS, 2)), ("pad", "<u2", (6,))])
assert COEFF_CDF_CONTEXT.itemsize == 7872 and COEFF_CDF_CONTEXT.itemsize % 16 == 0
PICK_FIRST_MIN, PICK_TX_TYPE = 0, 1   # R1_PICK_*
# R1CoeffNbrContext / R1NbrBlock (r1_coeff_nbr_gather_batch, r1_coeff_nbr_store_batch, r1_coeff_nbr_reset_left_batch):
# above_coeff_context / left_coeff_context of one tile (src/context/block_unit.rs:237-238), and a block's place in it
COEFF_NBR_WIDTH = 1024                # COEFF_CONTEXT_MAX_WIDTH
COEFF_NBR_CONTEXT = np.dtype([("above", "u1", (3, COEFF_NBR_WIDTH)), ("left", "u1", (3, 16))])
NBR_BLOCK = np.dtype([("nbr", "<u4"), ("bo_x", "<u2"), ("bo_y", "<u2"), ("mi_width", "<u2"), ("mi_height", "<u2"),
                      ("w_in_b", "<u2"), ("h_in_b", "<u2"), ("y_mode", "u1"), ("cdf_sel", "u1"), ("cdf_sel_uv", "u1"),
                      ("flags", "u1")])
assert COEFF_NBR_CONTEXT.itemsize == 3120 and NBR_BLOCK.itemsize == 20
NBR_DO_CHROMA, NBR_SKIP = 1, 2        # R1NbrBlock.flags
# R1PartPick (r1_rd_partition_pick_batch / r1_part_select_batch / r1_part_select_rect_batch): the decision state of one
# node of the partition quad-tree, carried from call to call; best_rd leads it as it leads RD_PICK
PART_PICK = np.dtype([("best_rd", "<f8"), ("best_partition", "i1"), ("best_call", "i1"), ("early_exit", "u1"),
                      ("reserved", "u1", (5,))])
assert PART_PICK.itemsize == 16
PART_BOTTOMUP, PART_TOPDOWN = 0, 1    # R1_PART_*
# R1HeadCdfContext (r1_intra_head_rate_batch / r1_partition_rate_batch / r1_intra_head_commit_batch): the head fields of
# the reference's CDFContext in its own shapes (src/context/cdf_context.rs:42-92), padded to a multiple of 16 bytes
HEAD_CDF_CONTEXT = np.dtype(
    [("partition_w8", "<u2", (4, 4)), ("partition", "<u2", (12, 10)), ("partition_w128", "<u2", (4, 8)),
     ("skip", "<u2", (3, 2)), ("kf_y", "<u2", (5, 5, INTRA_MODES)), ("y_mode", "<u2", (4, INTRA_MODES)),
     ("uv_mode", "<u2", (INTRA_MODES, INTRA_MODES)), ("uv_mode_cfl", "<u2", (INTRA_MODES, 14)),
     ("angle_delta", "<u2", (8, 7)), ("cfl_sign", "<u2", (8,)), ("cfl_alpha", "<u2", (6, 16)),
     ("tx_size_8x8", "<u2", (3, 2)), ("tx_size", "<u2", (3, 3, 3)), ("pad", "<u2", (1,))])
# R1HeadNbrContext: what the head contexts read of BlockContext (src/context/block_unit.rs:233-236) and, as row buffers,
# of blocks.above_of / left_of -- one per tile or speculative branch, beside COEFF_NBR_CONTEXT; a fresh tile is zeros
HEAD_NBR_CONTEXT = np.dtype(
    [("above_partition", "u1", (COEFF_NBR_WIDTH // 2,)), ("left_partition", "u1", (8,)),
     ("above_tx", "u1", (COEFF_NBR_WIDTH,)), ("left_tx", "u1", (16,)), ("above_mode", "u1", (COEFF_NBR_WIDTH,)),
     ("left_mode", "u1", (16,)), ("above_skip", "u1", (COEFF_NBR_WIDTH,)), ("left_skip", "u1", (16,))])
assert HEAD_CDF_CONTEXT.itemsize == 2192 and HEAD_CDF_CONTEXT.itemsize % 16 == 0 and HEAD_NBR_CONTEXT.itemsize == 3640
# R1HeadBlock / R1HeadTrial / R1HeadCommit: a block's static geometry, one mode trial of it, and what the winner's commit
# is told of the partition walker
HEAD_BLOCK = np.dtype([("nbr", "<u4"), ("cdf", "<u4"), ("bo_x", "<u2"), ("bo_y", "<u2"), ("mi_cols", "<u2"),
                       ("mi_rows", "<u2"), ("bsize", "u1"), ("has_chroma", "u1"), ("tx_mode_select", "u1"),
                       ("reserved", "u1")])
HEAD_TRIAL = np.dtype([("block", "<u4"), ("y_mode", "u1"), ("uv_mode", "u1"), ("angle_y", "i1"), ("angle_uv", "i1"),
                       ("alpha_u", "<i2"), ("alpha_v", "<i2"), ("tx_size", "u1"), ("reserved", "u1", (3,))])
HEAD_COMMIT = np.dtype([("block", "<u4"), ("node_x", "<u2"), ("node_y", "<u2"), ("node_bsize", "u1"),
                        ("part_type", "i1"), ("subsize", "u1"), ("flags", "u1"), ("reserved", "u1", (4,))])
assert HEAD_BLOCK.itemsize == 20 and HEAD_TRIAL.itemsize == 16 and HEAD_COMMIT.itemsize == 16
HEAD_NO_SUBSIZE = 255                 # R1HeadCommit.subsize: no update_partition_context
HEAD_EVENT_ONLY = 1                   # R1HeadCommit.flags bit 0: the partition event alone, no block
UV_CFL_PRED = 13                      # PredictionMode::UV_CFL_PRED (src/predict.rs)

# R1TileBlock: one 4x4 unit of a tile's blocks array (Block, src/context/block_unit.rs:159-183, as far as find_mvrefs and
# the inter head contexts read it); R1TileBlocks: the host descriptor of one array; the records of r1_mvref_stack_batch
TILE_BLOCK = np.dtype([("mv", "<i2", (2, 2)), ("ref_frames", "u1", (2,)), ("mode", "u1"), ("n4_w", "u1"), ("n4_h", "u1"),
                       ("bsize", "u1"), ("skip", "u1"), ("reserved", "u1")])
TILE_BLOCKS = np.dtype([("cells", "<u8"), ("stride", "<i4"), ("cols", "<i4"), ("rows", "<i4"), ("tile_x", "<i4"),
                        ("tile_y", "<i4"), ("frame_cols", "<i4"), ("frame_rows", "<i4"), ("reserved", "<i4")])
MV_BLOCK = np.dtype([("tile", "<u4"), ("bo_x", "<u2"), ("bo_y", "<u2"), ("bsize", "u1"), ("n_queries", "u1"),
                     ("reserved", "<u2"), ("query_off", "<u4")])
MV_QUERY = np.dtype([("block", "<u4"), ("ref_frames", "u1", (2,)), ("is_compound", "u1"), ("reserved", "u1")])
CANDIDATE_MV = np.dtype([("this_mv", "<i2", (2,)), ("comp_mv", "<i2", (2,)), ("weight", "<u4")])
MV_STACK = np.dtype([("count", "u1"), ("reserved", "u1"), ("mode_context", "<u2"), ("cand", CANDIDATE_MV, (9,))])
MV_TRIAL = np.dtype([("block", "<u4"), ("mode", "u1"), ("ref_frames", "u1", (2,)), ("skip", "u1"), ("mv", "<i2", (2, 2))])
assert TILE_BLOCK.itemsize == 16 and TILE_BLOCKS.itemsize == 40 and MV_BLOCK.itemsize == 16 and MV_QUERY.itemsize == 8
assert CANDIDATE_MV.itemsize == 12 and MV_STACK.itemsize == 112 and MV_TRIAL.itemsize == 16
MVREF_MAX_TILES = 64                  # R1_MVREF_MAX_TILES: descriptors per call
MVREF_MAX_QUERIES = 64                # R1_MVREF_MAX_QUERIES: queries per block
MVREF_REFUSED = 0xFF                  # R1MvStack.count of a refused query

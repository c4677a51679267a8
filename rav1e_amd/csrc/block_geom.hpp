// block_geom.hpp -- what the reference says of a block that decides which bytes of the carried contexts
// (R1CoeffNbrContext, R1CoeffCdfContext) a launch reads and writes, stated once: what a block size is, which chroma
// subsamplings exist, the chroma side of a block, the luma transform grid, the transform sets.  The host halves of
// coeff_rate.hip, coeff_nbr.hip, rd_pick.hip, rdo_intra_split.hip and rdo_cand.hip read it.
// No device code and nothing of HIP: a host compiler accepts this header alone, and tests/test_block_geom.py
// (tests/c/block_geom_list.cpp) holds every answer, at every block size, subsampling and transform size, against the
// host statements that the fixtures pin to the reference (rdo_glue.py, tests/golden/coeff_rate_ref.npz).
// Pure arithmetic: the entry points make the checks (R1_REQUIRE) and ask for the geometry of what passed.
#pragma once
#include "entry.hpp"

// ---- block sizes and subsamplings ----
// A block size (BlockSize, src/partition.rs): sides 4 .. 64 here (the 128-point sizes are not launched), powers of
// two, at most 4 : 1.  19 pairs.
inline bool r1_block_size_ok(int bw, int bh) {
  return r1_is_pow2(bw) && r1_is_pow2(bh) && bw >= 4 && bh >= 4 && bw <= 64 && bh <= 64 && bw <= 4 * bh && bh <= 4 * bw;
}
// 4:2:0, 4:2:2, 4:4:4 -- (0, 1) is no format
inline bool r1_subsampling_ok(int xdec, int ydec) { return r1_dec_ok(xdec, ydec) && xdec >= ydec; }
// subsampled_size (partition.rs:337-379): what 4:2:2 admits
inline bool r1_subsampling_admits(int xdec, int ydec, int bw, int bh) { return !(xdec == 1 && ydec == 0) || bw >= bh; }

// ---- the chroma side of a block ----
struct R1BlockGeom {
  int bw4, bh4;               // the block in 4x4 units
  int sub_w4, sub_h4;         // bsize.subsampled_size(xdec, ydec) in 4x4 units: what a skipped block resets per chroma plane
  int uv_tx_size, uw, uh;     // largest_chroma_tx_size and its sides in pixels
  int bw_uv, bh_uv;           // the chroma transform grid; one of them 0 where the reference's loop is empty
  int uv_w4, uv_h4;           // what a coded block's grid spans per chroma plane, 4x4 units -- 0 where the grid is empty
  int adj_x, adj_y;           // the one-unit shift of a 4-wide / 4-high block's chroma origin (encoder.rs:2364-2369)
  int uv_skip_off;            // get_txb_ctx, chroma: 10 when the plane's block has more pixels than the transform, else 7
  int skip_all_planes;        // reset_skip_context (partition_unit.rs:434-469): BLOCK_4X16 / BLOCK_16X4 are not below
                              // BLOCK_8X8 in the enum's order, so three planes are reset whatever has_chroma says
};
// bw x bh is a block size that the subsampling admits
inline R1BlockGeom r1_block_geom(int bw, int bh, int xdec, int ydec) {
  R1BlockGeom g = {};
  g.bw4 = bw >> 2, g.bh4 = bh >> 2;
  g.adj_x = (bw == 4) * xdec, g.adj_y = (bh == 4) * ydec;
  // subsampled_size, then largest_chroma_tx_size (partition.rs:385-393): the subsampled block, its largest transform,
  // 64-point sides coded as 32 -- always one of the 19
  const int pw = (bw >> xdec) > 4 ? bw >> xdec : 4, ph = (bh >> ydec) > 4 ? bh >> ydec : 4;
  g.sub_w4 = pw >> 2, g.sub_h4 = ph >> 2;
  g.uw = pw < 32 ? pw : 32, g.uh = ph < 32 ? ph : 32;
  while (g.uv_tx_size < 19 && ((1 << r1tx::kTxWLog2[g.uv_tx_size]) != g.uw || (1 << r1tx::kTxHLog2[g.uv_tx_size]) != g.uh))
    g.uv_tx_size++;
  // the chroma grid, literally (write_tx_blocks, encoder.rs:2327-2338; write_tx_tree, 2492-2505, has
  // max_txsize_rect_lookup[bsize] in place of the block, the same dimensions up to 64x64): either side 0 makes both 1
  // BEFORE the division, so 4x16 and 16x4 have an empty grid in 4:2:0
  g.bw_uv = g.bw4 >> xdec, g.bh_uv = g.bh4 >> ydec;
  if (g.bw_uv == 0 || g.bh_uv == 0) g.bw_uv = 1, g.bh_uv = 1;
  g.bw_uv /= g.uw >> 2, g.bh_uv /= g.uh >> 2;
  const bool coded = g.bw_uv * g.bh_uv != 0;
  g.uv_w4 = coded ? g.bw_uv * (g.uw >> 2) : 0;
  g.uv_h4 = coded ? g.bh_uv * (g.uh >> 2) : 0;
  g.uv_skip_off = pw * ph > g.uw * g.uh ? 10 : 7;
  g.skip_all_planes = (bw == 4 && bh == 16) || (bw == 16 && bh == 4);
  return g;
}

// ---- the luma grid of a block under transforms of one size (tx_size is valid) ----
struct R1LumaGrid {
  int ntx, gw;       // transform blocks per block and per row
  int tw4, th4;      // the transform in 4x4 units
  bool divides;      // the transform's sides divide the block's; ntx and gw mean nothing otherwise
};
inline R1LumaGrid r1_luma_grid(int bw, int bh, int tx_size) {
  const int tw = 1 << r1tx::kTxWLog2[tx_size], th = 1 << r1tx::kTxHLog2[tx_size];
  return {(bw / tw) * (bh / th), bw / tw, tw >> 2, th >> 2, bw % tw == 0 && bh % th == 0};
}

// ---- the transform sets (tx_size is valid; the flags are read as true / false) ----
// TxSize::sqr / sqr_up as TX_4X4 = 0 .. TX_64X64 = 4
inline int r1_txsize_sqr_log2(int t) { return (r1tx::kTxWLog2[t] < r1tx::kTxHLog2[t] ? r1tx::kTxWLog2[t] : r1tx::kTxHLog2[t]) - 2; }
inline int r1_txsize_sqr_up_log2(int t) { return (r1tx::kTxWLog2[t] > r1tx::kTxHLog2[t] ? r1tx::kTxWLog2[t] : r1tx::kTxHLog2[t]) - 2; }
// get_tx_set (src/context/transform_unit.rs:123-148) -> 0 .. 5 in TxSet order: TX_SET_DCTONLY, TX_SET_INTER_3,
// TX_SET_INTRA_2, TX_SET_INTRA_1, TX_SET_INTER_2, TX_SET_INTER_1
inline int r1_tx_set(int tx_size, int is_inter, int reduced) {
  const int up = r1_txsize_sqr_up_log2(tx_size), dn = r1_txsize_sqr_log2(tx_size);
  if (up > 3) return 0;
  if (is_inter) return (reduced || up == 3) ? 1 : (dn == 2 ? 4 : 5);
  if (up == 3) return 0;
  return (reduced || dn == 2) ? 2 : 3;
}
namespace r1tx {
// av1_tx_used as a bit mask over TxType, num_tx_set, av1_tx_ind (transform_unit.rs:36-58): rows in TxSet order
static const uint32_t kTxUsed[6] = {0x0001, 0x0201, 0x020F, 0x0E0F, 0x0FFF, 0xFFFF};
static const uint8_t kNumTxSet[6] = {1, 2, 5, 7, 12, 16};
static const uint8_t kTxInd[6][16] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                      {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                      {1, 3, 4, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                      {1, 5, 6, 4, 0, 0, 0, 0, 0, 0, 2, 3, 0, 0, 0, 0},
                                      {3, 4, 5, 8, 6, 7, 9, 10, 11, 0, 1, 2, 0, 0, 0, 0},
                                      {7, 8, 9, 12, 10, 11, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6}};
}  // namespace r1tx
// TxType::uv_inter (src/transform/mod.rs:81-97) as WinnerArgs::uv_rule has it: 1 -- sqr_up() == TX_32X32 keeps IDTX
// alone (else DCT_DCT); 2 -- sqr() == TX_16X16 drops the 1-D ADSTs; 0 -- the luma type
inline int r1_uv_inter_rule(int uv_tx_size) {
  return r1_txsize_sqr_up_log2(uv_tx_size) == 3 ? 1 : (r1_txsize_sqr_log2(uv_tx_size) == 2 ? 2 : 0);
}
// get_txsize_entropy_ctx
inline int r1_txs_ctx(int tx_size) { return (r1_txsize_sqr_log2(tx_size) + r1_txsize_sqr_up_log2(tx_size) + 1) >> 1; }

// mvref_kernel.hpp -- the device half of the MV-stack unit (its entry points: mvref.hip): the tile's blocks array on
// the device and find_mvrefs / setup_mvref_list (src/context/block_unit.rs:795-1442, has_tr of src/partition.rs:900-955)
// over it.
//   k_tile_blocks_reset  Block::default() over whole arrays
//   k_tile_blocks_store  what a coded block leaves: one wave per state, a 16-byte cell per lane and store
//   k_mvref_stack        one WAVE per block.  The walk is serial and its addresses depend on data (the next index is
//                        i += len with len from the cell just read): one lane per query on global memory would be a chain
//                        of 20 .. 60 dependent loads.  Every query of a block (its reference sets) reads the same
//                        neighbourhood, so the wave stages it in LDS in one round trip -- one 16-byte cell per lane and
//                        load, three loads at most -- and lane q walks query q from there.  The queries of a block have
//                        the block's geometry, so the lanes of a wave run the same loops and differ in what matches.
//   k_mvref_pmv          the stack's first two vectors to where r1_estimate_motion_batch reads pmv
// The neighbourhood (kNbrCells slots): rows -1 .. -5 over columns 0 .. n4_w (one to the right: the far rows start one
// column in, the top-right cell is (n4_w, -1)), columns -1 .. -5 over rows 0 .. n4_h, and the top-left cell.  A position
// outside the tile is not loaded and never read: the walk checks the tile before every read and refuses where the
// reference would index past the array.
// A lane's stack lives in LDS, entry-major and lane-minor (conflict-free): it is indexed by data (find a match, push at
// len, sort), which registers cannot be without scratch.  No scratch, no atomics, no spin-waits; every loop is bounded by
// 16 steps, by the stack's 8 entries, or by 2 passes.  sort_by (stable) is an insertion sort by descending weight that
// moves an entry only past strictly smaller ones, so ties keep insertion order.
// Restated from the reference (pinned by tests/golden/mvref_ref.npz): the sides of the 22 block sizes, has_newmv as a
// mode set, REF_CAT_LEVEL, MVREF_ROW_COLS = 3 as the two far offsets, REFMV_OFFSET = 4.
#pragma once
#include <stddef.h>

#include "common.hpp"

namespace {
static_assert(sizeof(R1TileBlock) == 16 && sizeof(R1TileBlocks) == 40 && sizeof(R1MvBlock) == 16, "ABI layout");
static_assert(sizeof(R1MvQuery) == 8 && sizeof(R1CandidateMv) == 12 && sizeof(R1MvStack) == 112, "ABI layout");
static_assert(sizeof(R1MvTrial) == 16 && offsetof(R1MeBlockCand, pmv) == 8 && sizeof(R1MeBlockCand) == 16, "ABI layout");

constexpr int kNbrRow = 17;                      // a far row or column: the block's 16 units and one more
constexpr int kNbrCells = 2 * 5 * kNbrRow + 1;   // 171
constexpr int kNbrTopLeft = kNbrCells - 1;
constexpr int kStackMax = 8;                     // MAX_REF_MV_STACK_SIZE: the extra search pushes only below 2
constexpr uint32_t kRefCatLevel = 640;
constexpr int kMvLanes = 64;

// log2 of the sides of BlockSize 0 .. 21 in the enum's order (src/partition.rs:130-153); 7: the 128-point sizes
__device__ const uint8_t kMvBsWL[22] = {2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6, 7, 7, 2, 4, 3, 5, 4, 6};
__device__ const uint8_t kMvBsHL[22] = {2, 3, 2, 3, 4, 3, 4, 5, 4, 5, 6, 5, 6, 7, 6, 7, 4, 2, 5, 3, 6, 4};

struct MvTiles {
  R1TileBlocks t[R1_MVREF_MAX_TILES];
};

struct TileResetArgs {
  MvTiles tiles;
  uint8_t sel[R1_MVREF_MAX_TILES];
};

struct TileStoreArgs {
  MvTiles tiles;
  const R1MvBlock *blocks;
  const R1MvTrial *trials;
  const R1RdPick *state;
  int n, n_tiles, n_blocks, n_trials, call_id, group, nt;
};

struct MvStackArgs {
  MvTiles tiles;
  const R1MvBlock *blocks;
  const R1MvQuery *queries;
  R1MvStack *out;
  int n_blocks, n_queries, n_tiles, max_queries;
  uint8_t sign_bias[8];
};

struct MvPmvArgs {
  const R1MvStack *stacks;
  uint8_t *pmv_out;
  long long stride;
  int n;
};

__device__ __forceinline__ uint4 mv_default_cell() {
  // zero vectors; INTRA_FRAME, INTRA_FRAME, DC_PRED, n4_w 16; n4_h 16, BLOCK_64X64, skip 0
  return make_uint4(0u, 0u, 16u << 24, 16u | (12u << 8));
}

// One descriptor per blockIdx.y, every cell of rows x stride
__global__ __launch_bounds__(256) void k_tile_blocks_reset(const TileResetArgs a) {
  const R1TileBlocks &t = a.tiles.t[a.sel[blockIdx.y]];
  const long long cells = (long long)t.rows * t.stride;
  uint4 *p = (uint4 *)t.cells;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long long)gridDim.x * 256) p[i] = mv_default_cell();
}

// the block of a store or a stack: its descriptor, its sides, its place -> false: the device refuses it
struct MvPlace {
  int tile, cols, rows, stride, bo_x, bo_y, n4_w, n4_h;
};
__device__ __forceinline__ bool mv_place(const MvTiles &tiles, int n_tiles, const R1MvBlock &b, MvPlace &p) {
  if (b.tile >= (uint32_t)n_tiles || b.bsize >= 22) return false;
  const int wl = kMvBsWL[b.bsize], hl = kMvBsHL[b.bsize];
  if (wl > 6 || hl > 6) return false;
  const R1TileBlocks &t = tiles.t[b.tile];
  p.tile = (int)b.tile, p.cols = t.cols, p.rows = t.rows, p.stride = t.stride;
  p.bo_x = b.bo_x, p.bo_y = b.bo_y, p.n4_w = 1 << (wl - 2), p.n4_h = 1 << (hl - 2);
  return p.bo_x < p.cols && p.bo_y < p.rows;
}

// One wave per state: everything of a state is checked before anything of it is written
__global__ __launch_bounds__(kMvLanes) void k_tile_blocks_store(const TileStoreArgs a) {
  const long long s = blockIdx.x;
  long long t = s;
  if (a.state) {
    const R1RdPick st = a.state[s];
    if (st.best_call != a.call_id) return;
    if (st.best_row < 0 || st.best_row >= a.group || st.best_slot < 0 || st.best_slot >= a.nt) return;
    t = (s * a.group + st.best_row) * a.nt + st.best_slot;
  }
  if (t >= a.n_trials) return;
  const R1MvTrial tr = a.trials[t];
  if (tr.block >= (uint32_t)a.n_blocks || tr.mode > 33) return;
  const R1MvBlock b = a.blocks[tr.block];
  MvPlace p;
  if (!mv_place(a.tiles, a.n_tiles, b, p)) return;
  const bool inter = tr.mode >= R1_NEARESTMV;
  uint4 c;
  c.x = inter ? (uint32_t)(uint16_t)tr.mv[0][0] | ((uint32_t)(uint16_t)tr.mv[0][1] << 16) : 0u;
  c.y = inter ? (uint32_t)(uint16_t)tr.mv[1][0] | ((uint32_t)(uint16_t)tr.mv[1][1] << 16) : 0u;
  const uint32_t r0 = inter ? tr.ref_frames[0] : R1_INTRA_FRAME, r1 = inter ? tr.ref_frames[1] : R1_NONE_FRAME;
  c.z = r0 | (r1 << 8) | ((uint32_t)tr.mode << 16) | ((uint32_t)p.n4_w << 24);
  c.w = (uint32_t)p.n4_h | ((uint32_t)b.bsize << 8) | ((tr.skip ? 1u : 0u) << 16);
  // for_each (tile_blocks.rs:206-224): the width cut to the tile, rows past it left out
  const int cw = p.bo_x + p.n4_w >= p.cols ? p.cols - p.bo_x : p.n4_w;
  uint4 *cells = (uint4 *)a.tiles.t[p.tile].cells;
  const int wl4 = __ffs(p.n4_w) - 1;
  for (int idx = threadIdx.x; idx < p.n4_w * p.n4_h; idx += kMvLanes) {
    const int dx = idx & (p.n4_w - 1), dy = idx >> wl4;
    if (dx < cw && p.bo_y + dy < p.rows) cells[(long long)(p.bo_y + dy) * p.stride + p.bo_x + dx] = c;
  }
}

// ---- the walk of one query, one lane ----
__device__ __forceinline__ uint32_t mv_neg(uint32_t mv) {      // (-row, -col), each wrapping as i16
  return ((0u - (mv & 0xFFFFu)) & 0xFFFFu) | ((0u - (mv >> 16)) << 16);
}
__device__ __forceinline__ bool mv_n4_ok(uint32_t v) { return v >= 1 && v <= 16 && (v & (v - 1)) == 0; }
__device__ __forceinline__ int mv_abs(int v) { return v < 0 ? -v : v; }

struct MvWalk {
  const uint4 *nbr;       // the staged neighbourhood
  uint32_t *stk;          // this lane's stack: entry e, field f at stk[(e * 3 + f) * kMvLanes]
  int cols, rows, bo_x, bo_y, n4_w, n4_h;
  uint32_t r0, r1;
  bool comp, refused;
  int len, newmv, proc_rows, proc_cols;

  // the cell at (dx, dy) from the block's origin -> false (and refused): outside the tile, or its sides are no block's
  __device__ __forceinline__ bool cell(int dx, int dy, uint4 &c) {
    const int x = bo_x + dx, y = bo_y + dy;
    if (x < 0 || x >= cols || y < 0 || y >= rows) {
      refused = true;
      return false;
    }
    int slot = dy < 0 ? (dx < 0 ? kNbrTopLeft : (-dy - 1) * kNbrRow + dx) : 5 * kNbrRow + (-dx - 1) * kNbrRow + dy;
    slot = slot < 0 ? 0 : (slot > kNbrTopLeft ? kNbrTopLeft : slot);
    c = nbr[slot];
    if (!mv_n4_ok(c.z >> 24) || !mv_n4_ok(c.w & 255)) {
      refused = true;
      return false;
    }
    return true;
  }
  __device__ __forceinline__ uint32_t &at(int e, int f) { return stk[(e * 3 + f) * kMvLanes]; }

  // find_matching_*_and_update_weight, then the push below MAX_REF_MV_STACK_SIZE
  __device__ __forceinline__ void add(uint32_t this_mv, uint32_t comp_mv, uint32_t weight) {
    bool found = false;
    for (int e = 0; e < kStackMax; e++)
      if (!found && e < len && at(e, 0) == this_mv && (!comp || at(e, 1) == comp_mv)) {
        at(e, 2) += weight;
        found = true;
      }
    if (!found && len < kStackMax) {
      at(len, 0) = this_mv, at(len, 1) = comp ? comp_mv : 0u, at(len, 2) = weight;
      len++;
    }
  }
  // add_ref_mv_candidate (853-911)
  __device__ __forceinline__ bool add_ref(const uint4 &c, uint32_t weight, bool count) {
    const uint32_t mode = (c.z >> 16) & 255;
    if (mode < R1_NEARESTMV) return false;
    const uint32_t ref0 = c.z & 255, ref1 = (c.z >> 8) & 255;
    const int newmv_inc = (count && (mode == 19 || (mode >= 24 && mode <= 31) || mode == 33)) ? 1 : 0;
    if (comp) {
      if (ref0 != r0 || ref1 != r1) return false;
      add(c.x, c.y, weight);
      newmv += newmv_inc;
      return true;
    }
    bool found = false;
    if (ref0 == r0) add(c.x, 0u, weight), newmv += newmv_inc, found = true;
    if (ref1 == r0) add(c.y, 0u, weight), newmv += newmv_inc, found = true;
    return found;
  }
  // scan_row_mbmi (horizontal) / scan_col_mbmi (967-1097)
  __device__ __forceinline__ bool scan(bool horizontal, int offset, int max_offs, bool count) {
    const int target = horizontal ? n4_w : n4_h;
    const int pos = horizontal ? bo_x : bo_y, room = horizontal ? cols - bo_x : rows - bo_y;
    int end_mi = target < room ? target : room;
    end_mi = end_mi < 16 ? end_mi : 16;
    const bool far = mv_abs(offset) > 1;
    const int shift = far && !((pos & 1) && target < 2) ? 1 : 0;
    bool found = false;
    int i = 0;
    for (int step = 0; step < 16 && i < end_mi && !refused; step++) {
      uint4 c;
      if (!(horizontal ? cell(shift + i, offset, c) : cell(offset, shift + i, c))) break;
      const int cw = (int)(c.z >> 24), ch = (int)(c.w & 255);
      const int n4 = horizontal ? cw : ch, other = horizontal ? ch : cw;
      int length = target < n4 ? target : n4;
      if (target >= 16)
        length = length > 4 ? length : 4;
      else if (far)
        length = length > 2 ? length : 2;
      int weight = 2;
      if (target >= 2 && target <= n4) {
        int inc = -max_offs + offset + 1;
        inc = inc < other ? inc : other;
        if (inc < 0) {                        // assert!(inc >= 0)
          refused = true;
          break;
        }
        weight = weight > inc ? weight : inc;
        if (horizontal)
          proc_rows = inc - offset - 1;
        else
          proc_cols = inc - offset - 1;
      }
      if (add_ref(c, (uint32_t)(length * weight), count)) found = true;
      i += length;
    }
    return found;
  }
  // scan_blk_mbmi (1099-1118)
  __device__ __forceinline__ bool scan_blk(int dx, int dy, bool count) {
    if (bo_x + dx >= cols || bo_y + dy >= rows) return false;
    uint4 c;
    if (!cell(dx, dy, c)) return false;
    return add_ref(c, 4u, count);
  }
};

// has_tr (src/partition.rs:900-955)
__device__ __forceinline__ bool mv_has_tr(int bo_x, int bo_y, int n4_w, int n4_h) {
  const int mask_row = bo_y & 15, mask_col = bo_x & 15;
  int bs = n4_w > n4_h ? n4_w : n4_h;
  bool tr = !((mask_row & bs) != 0 && (mask_col & bs) != 0);
  for (int k = 0; k < 4 && bs < 16; k++) {
    if ((mask_col & bs) == 0) break;
    if ((mask_col & (2 * bs)) != 0 && (mask_row & (2 * bs)) != 0) {
      tr = false;
      break;
    }
    bs <<= 1;
  }
  if (n4_w < n4_h && (bo_x & n4_w) == 0) tr = true;
  if (n4_w > n4_h && (bo_y & n4_h) != 0) tr = false;
  return tr;
}

__device__ __forceinline__ uint32_t mv_clamp(uint32_t mv, int y_min, int y_max, int x_min, int x_max) {
  int row = (int)(int16_t)(mv & 0xFFFFu), col = (int)(int16_t)(mv >> 16);
  row = row < y_min ? y_min : (row > y_max ? y_max : row);
  col = col < x_min ? x_min : (col > x_max ? x_max : col);
  return (uint32_t)(uint16_t)row | ((uint32_t)(uint16_t)col << 16);
}

__global__ __launch_bounds__(kMvLanes) void k_mvref_stack(const MvStackArgs a) {
  __shared__ uint4 nbr[kNbrCells + 1];
  __shared__ uint32_t stk[(kStackMax + 1) * 3 * kMvLanes];
  const int lane = threadIdx.x;
  const uint32_t bi = blockIdx.x;
  const R1MvBlock b = a.blocks[bi];
  MvPlace p = {};
  const bool ok = mv_place(a.tiles, a.n_tiles, b, p) && (int)b.n_queries <= a.max_queries;
  if (ok) {
    const uint4 *cells = (const uint4 *)a.tiles.t[p.tile].cells;
    for (int slot = lane; slot < kNbrCells; slot += kMvLanes) {
      int dx, dy;
      bool want;
      if (slot == kNbrTopLeft) {
        dx = -1, dy = -1, want = true;
      } else if (slot < 5 * kNbrRow) {
        dy = -(slot / kNbrRow) - 1, dx = slot % kNbrRow, want = dx <= p.n4_w;
      } else {
        dx = -((slot - 5 * kNbrRow) / kNbrRow) - 1, dy = (slot - 5 * kNbrRow) % kNbrRow, want = dy <= p.n4_h;
      }
      const int x = p.bo_x + dx, y = p.bo_y + dy;
      if (want && x >= 0 && x < p.cols && y >= 0 && y < p.rows) nbr[slot] = cells[(long long)y * p.stride + x];
    }
  }
  __syncthreads();
  if (lane >= (int)b.n_queries) return;
  const long long qi = (long long)b.query_off + lane;
  if (qi >= a.n_queries) return;
  R1MvStack *o = a.out + qi;
  if (!ok) {
    o->count = R1_MVREF_REFUSED;
    return;
  }
  const R1MvQuery q = a.queries[qi];
  MvWalk w;
  w.nbr = nbr, w.stk = stk + lane;
  w.cols = p.cols, w.rows = p.rows, w.bo_x = p.bo_x, w.bo_y = p.bo_y, w.n4_w = p.n4_w, w.n4_h = p.n4_h;
  w.r0 = q.ref_frames[0], w.r1 = q.ref_frames[1], w.comp = q.is_compound != 0, w.refused = false;
  w.len = 0, w.newmv = 0, w.proc_rows = 0, w.proc_cols = 0;
  if (q.block != bi || w.r0 >= R1_NONE_FRAME || w.r1 > R1_NONE_FRAME ||
      (w.comp && (w.r1 == R1_INTRA_FRAME || w.r1 == R1_NONE_FRAME))) {
    o->count = R1_MVREF_REFUSED;
    return;
  }
  uint32_t *od = (uint32_t *)o;
  if (w.r0 == R1_INTRA_FRAME) {                      // find_mvrefs returns 0 on an empty stack
    for (int k = 0; k < 28; k++) od[k] = 0u;
    return;
  }
  // setup_mvref_list (1127-1418)
  const int row_adj = (p.n4_h < 2 && (p.bo_y & 1)) ? 1 : 0, col_adj = (p.n4_w < 2 && (p.bo_x & 1)) ? 1 : 0;
  const bool up_avail = p.bo_y > 0, left_avail = p.bo_x > 0;
  int max_row_offs = 0, max_col_offs = 0;
  if (up_avail) {
    max_row_offs = (p.n4_h < 2 ? -4 : -6) + row_adj;
    max_row_offs = max_row_offs > -p.bo_y ? max_row_offs : -p.bo_y;                            // find_valid_row_offs
    max_row_offs = max_row_offs < p.rows - p.bo_y - 1 ? max_row_offs : p.rows - p.bo_y - 1;
  }
  if (left_avail) {
    max_col_offs = (p.n4_w < 2 ? -4 : -6) + col_adj;
    max_col_offs = max_col_offs > -p.bo_x ? max_col_offs : -p.bo_x;
    max_col_offs = max_col_offs < p.cols - p.bo_x - 1 ? max_col_offs : p.cols - p.bo_x - 1;
  }
  bool row_match = false, col_match = false;
  if (mv_abs(max_row_offs) >= 1) row_match |= w.scan(true, -1, max_row_offs, true);
  if (mv_abs(max_col_offs) >= 1) col_match |= w.scan(false, -1, max_col_offs, true);
  if (mv_has_tr(p.bo_x, p.bo_y, p.n4_w, p.n4_h) && up_avail) row_match |= w.scan_blk(p.n4_w, -1, true);
  const int nearest_match = (int)row_match + (int)col_match;
  for (int e = 0; e < kStackMax; e++)                                                          // add_offset
    if (e < w.len) w.at(e, 2) += kRefCatLevel;
  if (left_avail && up_avail) row_match |= w.scan_blk(-1, -1, false);
  for (int idx = 2; idx <= 3; idx++) {
    const int row_offset = -2 * idx + 1 + row_adj, col_offset = -2 * idx + 1 + col_adj;
    if (mv_abs(row_offset) <= mv_abs(max_row_offs) && mv_abs(row_offset) > w.proc_rows)
      row_match |= w.scan(true, row_offset, max_row_offs, false);
    if (mv_abs(col_offset) <= mv_abs(max_col_offs) && mv_abs(col_offset) > w.proc_cols)
      col_match |= w.scan(false, col_offset, max_col_offs, false);
  }
  const int total_match = (int)row_match + (int)col_match;
  const int newmv = w.newmv < 1 ? w.newmv : 1;
  int mode_context;
  if (nearest_match == 0)
    mode_context = (total_match < 1 ? total_match : 1) + (total_match << 4);
  else if (nearest_match == 1)
    mode_context = 3 - newmv + ((2 + total_match) << 4);
  else
    mode_context = 5 - newmv + (5 << 4);
  // 7.10.2.11: stable, descending weight
  for (int i = 1; i < kStackMax; i++) {
    if (i >= w.len) break;
    const uint32_t k0 = w.at(i, 0), k1 = w.at(i, 1), k2 = w.at(i, 2);
    int j = i;
    for (int s = 0; s < kStackMax && j > 0 && w.at(j - 1, 2) < k2; s++, j--)
      w.at(j, 0) = w.at(j - 1, 0), w.at(j, 1) = w.at(j - 1, 1), w.at(j, 2) = w.at(j - 1, 2);
    w.at(j, 0) = k0, w.at(j, 1) = k1, w.at(j, 2) = k2;
  }
  if (w.len < 2 && !w.refused) {                                                               // 7.10.2.12
    int num4x4 = p.n4_w < p.n4_h ? p.n4_w : p.n4_h;
    num4x4 = num4x4 < p.cols - p.bo_x ? num4x4 : p.cols - p.bo_x;
    num4x4 = num4x4 < p.rows - p.bo_y ? num4x4 : p.rows - p.bo_y;
    uint32_t id0[2] = {0u, 0u}, id1[2] = {0u, 0u}, df0[2] = {0u, 0u}, df1[2] = {0u, 0u};      // [list]: first, second
    int idc[2] = {0, 0}, dfc[2] = {0, 0};
    for (int pass = up_avail ? 0 : 1; pass <= (left_avail ? 1 : 0); pass++) {
      int idx = 0;
      for (int step = 0; step < 16 && idx < num4x4 && w.len < 2 && !w.refused; step++) {
        uint4 c;
        if (!(pass == 0 ? w.cell(idx, -1, c) : w.cell(-1, idx, c))) break;
#pragma unroll
        for (int k = 0; k < 2; k++) {
          const uint32_t cand_ref = (c.z >> (8 * k)) & 255;
          if (cand_ref == R1_INTRA_FRAME || cand_ref == R1_NONE_FRAME) continue;
          if (cand_ref > R1_NONE_FRAME) {                      // to_index past ref_frame_sign_bias
            w.refused = true;
            continue;
          }
          const uint32_t mv = k == 0 ? c.x : c.y;
          if (w.comp) {
#pragma unroll
            for (int lst = 0; lst < 2; lst++) {
              const uint32_t want = lst == 0 ? w.r0 : w.r1;
              if (cand_ref == want && idc[lst] < 2) {
                if (idc[lst] == 0) id0[lst] = mv; else id1[lst] = mv;
                idc[lst]++;
              } else if (dfc[lst] < 2) {
                const uint32_t m = a.sign_bias[cand_ref - 1] != a.sign_bias[want - 1] ? mv_neg(mv) : mv;
                if (dfc[lst] == 0) df0[lst] = m; else df1[lst] = m;
                dfc[lst]++;
              }
            }
          } else {
            const uint32_t m = a.sign_bias[cand_ref - 1] != a.sign_bias[w.r0 - 1] ? mv_neg(mv) : mv;
            bool found = false;
            for (int e = 0; e < 2; e++)
              if (e < w.len && w.at(e, 0) == m) found = true;
            if (!found && !w.refused) {
              w.at(w.len, 0) = m, w.at(w.len, 1) = 0u, w.at(w.len, 2) = 2u;
              w.len++;
            }
          }
        }
        idx += pass == 0 ? (int)(c.z >> 24) : (int)(c.w & 255);
      }
    }
    if (w.comp && !w.refused) {
      uint32_t c0[2], c1[2];                                   // combined_mvs[0][list], [1][list]
#pragma unroll
      for (int lst = 0; lst < 2; lst++) {
        c0[lst] = idc[lst] > 0 ? id0[lst] : (dfc[lst] > 0 ? df0[lst] : 0u);
        c1[lst] = idc[lst] > 1 ? id1[lst] : (idc[lst] == 1 ? (dfc[lst] > 0 ? df0[lst] : 0u) : (dfc[lst] > 1 ? df1[lst] : 0u));
      }
      if (w.len == 1) {
        const bool same = w.at(0, 0) == c0[0] && w.at(0, 1) == c0[1];
        w.at(1, 0) = same ? c1[0] : c0[0], w.at(1, 1) = same ? c1[1] : c0[1], w.at(1, 2) = 2u;
      } else {
        w.at(0, 0) = c0[0], w.at(0, 1) = c0[1], w.at(0, 2) = 2u;
        w.at(1, 0) = c1[0], w.at(1, 1) = c1[1], w.at(1, 2) = 2u;
      }
      w.len = 2;
    }
  }
  if (w.refused) {
    o->count = R1_MVREF_REFUSED;
    return;
  }
  // the clamp, around the block's place in the FRAME (1385-1415)
  const R1TileBlocks &t = a.tiles.t[p.tile];
  const int fx = t.tile_x + p.bo_x, fy = t.tile_y + p.bo_y;
  const int border_w = 128 + p.n4_w * 32, border_h = 128 + p.n4_h * 32;
  const int x_min = -fx * 32 - border_w, x_max = (t.frame_cols - fx - p.n4_w) * 32 + border_w;
  const int y_min = -fy * 32 - border_h, y_max = (t.frame_rows - fy - p.n4_h) * 32 + border_h;
  od[0] = (uint32_t)w.len | ((uint32_t)mode_context << 16);
  for (int e = 0; e < 9; e++) {
    const bool live = e < w.len;
    const int ee = e < kStackMax ? e : kStackMax;
    od[1 + 3 * e] = live ? mv_clamp(w.at(ee, 0), y_min, y_max, x_min, x_max) : 0u;
    od[2 + 3 * e] = live ? mv_clamp(w.at(ee, 1), y_min, y_max, x_min, x_max) : 0u;
    od[3 + 3 * e] = live ? w.at(ee, 2) : 0u;
  }
}

// One lane per stack
__global__ __launch_bounds__(256) void k_mvref_pmv(const MvPmvArgs a) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.n) return;
  const R1MvStack *s = a.stacks + q;
  const int count = s->count;
  if (count == R1_MVREF_REFUSED) return;
  int16_t *out = (int16_t *)(a.pmv_out + q * a.stride);
  out[0] = count > 0 ? s->cand[0].this_mv[0] : (int16_t)0;
  out[1] = count > 0 ? s->cand[0].this_mv[1] : (int16_t)0;
  out[2] = count > 1 ? s->cand[1].this_mv[0] : (int16_t)0;
  out[3] = count > 1 ? s->cand[1].this_mv[1] : (int16_t)0;
}
}  // namespace

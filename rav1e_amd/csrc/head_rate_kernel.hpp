// head_rate_kernel.hpp -- the device half of the head-symbol unit (its entry points: head_rate.hip): what an intra mode
// trial of an intra frame writes in front of its coefficients (src/rdo.rs:870-877, src/encoder.rs:1913, 2086-2102,
// 2132-2136), stated ONCE as head_walk over a sink, and run three ways:
//   k_intra_head_rate    RateSink on the counting writer of coeff_rate_kernel.hpp: the trial's tell_frac difference and the
//                        rng behind it; contexts are read, never written
//   k_intra_head_commit  a checking pass (NullSink), then CommitSink: the winner's symbols adapt its R1HeadCdfContext in
//                        place (update_cdf's three steps, coeff_rate_kernel.hpp), then the stores of set_mode / set_skip,
//                        update_tx_size_context and update_partition_context on its R1HeadNbrContext
//   k_partition_rate     write_partition alone (src/context/partition_unit.rs:267-357), any of the four types
//
// One LANE per trial (per winner, per node).  A head is at most ten dependent symbols, each two or three 2-byte loads from
// a row of at most 16 entries and a dozen integer instructions of the range coder: nothing to share between lanes, and a
// wave per trial -- the coefficient kernels' mapping -- would idle 63 of them.  The trials of a block lie next to each
// other, so neighbouring lanes read the same context bytes and, mode for mode, the same or neighbouring CDF rows.
// No LDS, no scratch: the symbols are never held in an array, each is written where it is decided.  Two symbols of one
// head can name one row (the two angle deltas when the chroma mode equals the luma mode; the two CFL alphas when both
// signs are equal): the rate sink is told the earlier symbol and adapts the two entries it reads; the commit sink writes
// memory and reads it back.  Every loop is bounded by 16; no atomics, no spin-waits.
//
// Restated from the reference (pinned by tests/golden/head_ref.npz through every fixture case): intra_mode_context
// (block_unit.rs:703-704), the sides of the 22 block sizes, sub_tx_size_map and max_txsize_rect_lookup as arithmetic on
// log2 sides (transform_unit.rs:60-105), partition_context_lookup as 31 & ~(side / 4 - 1) (partition_unit.rs:15-38).
#pragma once
#include <stddef.h>

#include "coeff_rate_kernel.hpp"

namespace {
static_assert(sizeof(R1HeadCdfContext) == 2192 && sizeof(R1HeadCdfContext) % 16 == 0, "ABI layout");
static_assert(sizeof(R1HeadNbrContext) == 3640, "ABI layout");
static_assert(sizeof(R1HeadBlock) == 20 && sizeof(R1HeadTrial) == 16 && sizeof(R1HeadCommit) == 16, "ABI layout");
static_assert(offsetof(R1BlockRateTrial, rng) == 16, "where the head's rng lands with stride 24");

constexpr uint32_t kHeadInvalid = 0xFFFFFFFFu;
constexpr int kBlock8x8 = 3, kBlock32x32 = 9, kUvCfl = 13;
// a row's place in R1HeadCdfContext, in uint16 entries
#define R1_HEAD_OFF(field) ((int)(offsetof(R1HeadCdfContext, field) / 2))

// log2 of the sides of BlockSize 0 .. 21 in the enum's order (src/partition.rs:130-153); 7: the 128-point sizes
__device__ const uint8_t kBsWL[22] = {2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6, 7, 7, 2, 4, 3, 5, 4, 6};
__device__ const uint8_t kBsHL[22] = {2, 3, 2, 3, 4, 3, 4, 5, 4, 5, 6, 5, 6, 7, 6, 7, 4, 2, 5, 3, 6, 4};
#define R1_TX_WL(ID, WL, HL) WL,
#define R1_TX_HL(ID, WL, HL) HL,
__device__ const uint8_t kHeadTxWL[19] = {R1_TX_SIZES(R1_TX_WL)};
__device__ const uint8_t kHeadTxHL[19] = {R1_TX_SIZES(R1_TX_HL)};
#undef R1_TX_WL
#undef R1_TX_HL

// intra_mode_context[mode], a nibble per mode: 0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0
__device__ __forceinline__ int intra_mode_ctx(int mode) { return (int)((0x0210344443210ull >> (4 * mode)) & 15); }
// PredictionMode::is_directional: V_PRED ..= D67_PRED
__device__ __forceinline__ bool directional(int mode) { return mode >= 1 && mode <= 8; }
// sub_tx_size_map on log2 sides: a square halves both (4x4 stays), a rectangle halves its long side
// (two selects: written as branches that decrement one of two references, the pair becomes an indexed array in scratch)
__device__ __forceinline__ void sub_tx(int &wl, int &hl) {
  const int dw = wl >= hl && wl > 2, dh = hl >= wl && hl > 2;
  wl -= dw, hl -= dh;
}

// One block and one trial of it, as the walk reads them
struct HeadIn {
  int bsize, bo_x, bo_y, mi_cols, mi_rows, has_chroma, tx_mode_select;
  int y_mode, uv_mode, angle_y, angle_uv, alpha_u, alpha_v, tx_size;
};

__device__ __forceinline__ void head_in_block(HeadIn &h, const R1HeadBlock &b) {
  h.bsize = b.bsize, h.bo_x = b.bo_x, h.bo_y = b.bo_y, h.mi_cols = b.mi_cols, h.mi_rows = b.mi_rows;
  h.has_chroma = b.has_chroma != 0, h.tx_mode_select = b.tx_mode_select != 0;
}
__device__ __forceinline__ void head_in_trial(HeadIn &h, const R1HeadTrial &t) {
  h.y_mode = t.y_mode, h.uv_mode = t.uv_mode, h.angle_y = t.angle_y, h.angle_uv = t.angle_uv;
  h.alpha_u = t.alpha_u, h.alpha_v = t.alpha_v, h.tx_size = t.tx_size;
}

// What the device refuses of a block's place whatever is written there: a size past the enum or with a 128-point side,
// a tile wider than the context arrays, a place outside the tile
__device__ __forceinline__ bool head_place_ok(int bsize, int bo_x, int bo_y, int mi_cols, int mi_rows) {
  return bsize < 22 && kBsWL[bsize] <= 6 && kBsHL[bsize] <= 6 && mi_cols <= R1_HEAD_NBR_WIDTH && bo_x < mi_cols &&
         bo_y < mi_rows;
}

// write_partition (partition_unit.rs:267-357) for a square block of log2 side wl in 3 .. 6 at a place head_place_ok
// passed.  -> -1: the reference asserts; 0: nothing is written (neither rows nor columns); 1: symbol s on the row at
// `off` of n symbols, with its update; 2 / 3: symbol s on the two-entry CDF of partition_gather_vert_alike /
// _horz_alike over that row, written with w.symbol alone.  ctx < 16: partition_w128_cdf belongs to the 128-point sizes.
__device__ __forceinline__ int partition_sym(const R1HeadNbrContext *nb, int wl, int bo_x, int bo_y, int mi_cols,
                                             int mi_rows, int p, int &off, int &n, int &s) {
  const int hbs = 1 << (wl - 3), bsl = wl - 3;
  const bool has_cols = bo_x + hbs < mi_cols, has_rows = bo_y + hbs < mi_rows;
  const int above = (nb->above_partition[bo_x >> 1] >> bsl) & 1;
  const int left = (nb->left_partition[(bo_y & 15) >> 1] >> bsl) & 1;
  const int ctx = left * 2 + above + bsl * 4;
  if (!has_rows && !has_cols) return 0;
  off = ctx < 4 ? R1_HEAD_OFF(partition_w8) + ctx * 4 : R1_HEAD_OFF(partition) + (ctx - 4) * 10;
  n = ctx < 4 ? 4 : 10;
  if (has_rows && has_cols) {
    s = p;
    return 1;
  }
  if (wl == 3) return -1;                                            // assert!(bsize > BlockSize::BLOCK_8X8)
  if (p != R1_PARTITION_SPLIT && p != (has_cols ? R1_PARTITION_HORZ : R1_PARTITION_VERT)) return -1;
  s = p == R1_PARTITION_SPLIT;
  return has_cols ? 2 : 3;
}

// out[0] of partition_gather_vert_alike (kVert) / _horz_alike over a ten-entry row: the sum of cdf_element_prob
// (cdf_context.rs:721-724) over VERT, SPLIT, HORZ_A, VERT_A, VERT_B, VERT_4 / HORZ, SPLIT, HORZ_A, HORZ_B, VERT_A, HORZ_4
template <bool kVert>
__device__ __forceinline__ uint32_t partition_gather(const uint16_t *r) {
  auto prob = [&](int e) { return (uint32_t)r[e - 1] - (e + 1 < 10 ? (uint32_t)r[e] : 0u); };     // e > 0 throughout
  const uint32_t sum = kVert ? prob(2) + prob(3) + prob(4) + prob(6) + prob(7) + prob(9)
                             : prob(1) + prob(3) + prob(4) + prob(5) + prob(6) + prob(8);
  return sum & 0xffffu;
}

// ---- the three sinks of head_walk: sym(off, n, s, poff, ps) is symbol s on the row of n symbols at entry `off`;
// poff == off says that this head wrote symbol ps on the same row before
struct NullSink {
  __device__ __forceinline__ void sym(int, int, int, int = -1, int = 0) {}
};

struct RateSink {
  const uint16_t *cdf;
  Counter w;
  __device__ __forceinline__ void sym(int off, int n, int s, int poff = -1, int ps = 0) {
    const uint16_t *r = cdf + off;
    uint32_t fl = s > 0 ? r[s - 1] : 32768u, fh = r[s];       // r[n - 1] is the counter: below 64, so it reads as 0
    if (poff == off) {                                        // the row as symbol ps left it
      const uint32_t cnt = r[n - 1], rate = cdf_rate(cnt, n);
      if (s > 0) fl = cdf_step(fl, s - 1 >= ps, rate);
      fh = s < n - 1 ? cdf_step(fh, s >= ps, rate) : cdf_count(cnt);
    }
    w.store(s > 0 ? fl >> 6 : 512u, fh >> 6, (uint32_t)(n - s));
  }
  // w.symbol(s, &[out0, 0]) of the edge arms: nothing adapts
  __device__ __forceinline__ void edge(uint32_t out0, int s) {
    if (s) w.store(out0 >> 6, 0u, 1u);
    else w.store(512u, out0 >> 6, 2u);
  }
};

struct CommitSink {
  uint16_t *cdf;
  __device__ __forceinline__ void sym(int off, int n, int s, int = -1, int = 0) {
    uint16_t *r = cdf + off;
    const uint32_t cnt = r[n - 1], rate = cdf_rate(cnt, n);
    for (int i = 0; i < 15; i++)                              // the longest row (cfl_alpha) has 15 entries and a counter
      if (i < n - 1) r[i] = (uint16_t)cdf_step(r[i], i >= s, rate);
    r[n - 1] = (uint16_t)cdf_count(cnt);
  }
};

// The head of one trial, in coding order.  -> false: the device refuses the trial (the sink may have been told symbols in
// front of the refusal: a caller that writes memory walks a NullSink first).  kTrial: a mode trial, which writes
// PARTITION_NONE itself; false: the block coded for real, whose partition symbol is the walker's (the commit's event).
template <bool kTrial, typename Sink>
__device__ __forceinline__ bool head_walk(Sink &k, const R1HeadNbrContext *nb, const HeadIn &h) {
  if (!head_place_ok(h.bsize, h.bo_x, h.bo_y, h.mi_cols, h.mi_rows)) return false;
  if (h.y_mode >= R1_INTRA_MODES || h.tx_size >= 19) return false;
  const int wl = kBsWL[h.bsize], hl = kBsHL[h.bsize], y_sb = h.bo_y & 15;
  const bool ge_8x8 = h.bsize >= kBlock8x8;        // in the enum's order: BLOCK_4X16 and BLOCK_16X4 are not below it
  // 1. write_partition(PARTITION_NONE) for a square block of 8x8 and up (rdo.rs:870-877)
  if (kTrial && ge_8x8 && wl == hl) {
    int off, n, s;
    const int arm = partition_sym(nb, wl, h.bo_x, h.bo_y, h.mi_cols, h.mi_rows, R1_PARTITION_NONE, off, n, s);
    if (arm < 0 || arm > 1) return false;          // at an edge the reference asserts against PARTITION_NONE
    if (arm == 1) k.sym(off, n, s);
  }
  // 2. write_skip(false): the neighbours' flags, each only inside the tile
  const int skip_ctx = (int)(h.bo_y > 0 && nb->above_skip[h.bo_x] != 0) + (int)(h.bo_x > 0 && nb->left_skip[y_sb] != 0);
  k.sym(R1_HEAD_OFF(skip) + skip_ctx * 2, 2, 0);
  // 3. write_intra_mode_kf: DC_PRED at the tile's top / left
  const int above_mode = h.bo_y > 0 ? nb->above_mode[h.bo_x] : 0, left_mode = h.bo_x > 0 ? nb->left_mode[y_sb] : 0;
  if (above_mode >= R1_INTRA_MODES || left_mode >= R1_INTRA_MODES) return false;
  k.sym(R1_HEAD_OFF(kf_y) + (intra_mode_ctx(above_mode) * 5 + intra_mode_ctx(left_mode)) * R1_INTRA_MODES, R1_INTRA_MODES,
        h.y_mode);
  // 4. the luma angle delta
  int angle_off = -1, angle_s = 0;
  if (directional(h.y_mode) && ge_8x8) {
    if (h.angle_y < -3 || h.angle_y > 3) return false;
    angle_off = R1_HEAD_OFF(angle_delta) + (h.y_mode - 1) * 7, angle_s = h.angle_y + 3;
    k.sym(angle_off, 7, angle_s);
  }
  // 5. chroma
  if (h.has_chroma) {
    const bool cfl_allowed = h.bsize <= kBlock32x32;   // BlockSize::cfl_allowed, the enum's order again
    const int n_uv = cfl_allowed ? 14 : 13;
    if (h.uv_mode >= n_uv) return false;
    k.sym(cfl_allowed ? R1_HEAD_OFF(uv_mode_cfl) + h.y_mode * 14 : R1_HEAD_OFF(uv_mode) + h.y_mode * 13, n_uv, h.uv_mode);
    if (h.uv_mode == kUvCfl) {
      const int au = h.alpha_u, av = h.alpha_v;
      if ((au == 0 && av == 0) || au < -16 || au > 16 || av < -16 || av > 16) return false;
      const int su = au < 0 ? 1 : (au > 0 ? 2 : 0), sv = av < 0 ? 1 : (av > 0 ? 2 : 0);   // CFLSign::from_alpha
      k.sym(R1_HEAD_OFF(cfl_sign), 8, su * 3 + sv - 1);
      const int off_u = R1_HEAD_OFF(cfl_alpha) + ((su - 1) * 3 + sv) * 16, s_u = (au < 0 ? -au : au) - 1;
      if (su) k.sym(off_u, 16, s_u);
      if (sv) k.sym(R1_HEAD_OFF(cfl_alpha) + ((sv - 1) * 3 + su) * 16, 16, (av < 0 ? -av : av) - 1, su ? off_u : -1, s_u);
    }
    if (directional(h.uv_mode) && ge_8x8) {
      if (h.angle_uv < -3 || h.angle_uv > 3) return false;
      k.sym(R1_HEAD_OFF(angle_delta) + (h.uv_mode - 1) * 7, 7, h.angle_uv + 3, angle_off, angle_s);
    }
  }
  // 6. write_tx_size_intra
  if (h.tx_mode_select && h.bsize > 0) {
    const int tw = kHeadTxWL[h.tx_size], th = kHeadTxHL[h.tx_size];
    int cw = wl, ch = hl, depth = 0;               // tx_size_to_depth from max_txsize_rect_lookup[bsize]: the block itself
    bool found = cw == tw && ch == th;
    for (int i = 0; i < 2; i++)
      if (!found) {
        sub_tx(cw, ch);
        depth++;
        found = cw == tw && ch == th;
      }
    if (!found) return false;
    int steps = 0;                                 // bsize_to_tx_size_cat: the splits down to TX_4X4, less one
    cw = wl, ch = hl;
    for (int i = 0; i < 4; i++)
      if (cw != 2 || ch != 2) {
        sub_tx(cw, ch);
        steps++;
      }
    // get_tx_size_context: the arrays raw, has_above / has_left the tile's
    const int above = nb->above_tx[h.bo_x] >= (1 << wl), left = nb->left_tx[y_sb] >= (1 << hl);
    const int ctx = (h.bo_y > 0 ? above : 0) + (h.bo_x > 0 ? left : 0);
    if (steps > 1) k.sym(R1_HEAD_OFF(tx_size) + ((steps - 2) * 3 + ctx) * 3, 3, depth);
    else k.sym(R1_HEAD_OFF(tx_size_8x8) + ctx * 2, 2, depth);
  }
  return true;
}

// ---- arguments
struct HeadRateArgs {
  const R1HeadNbrContext *nbrs;
  const R1HeadCdfContext *cdfs;
  const R1HeadBlock *blocks;
  const R1HeadTrial *trials;
  const R1RdPick *depth_state;
  const int16_t *cfl_alpha;
  uint32_t *rate_add;
  uint8_t *rng_out;
  long long rng_stride;
  int n, n_nbrs, n_cdfs, n_blocks;
  uint32_t tx_sizes;      // the host's table of three TxSize, a byte each: indexed by shifts, not through memory
};

struct HeadCommitArgs {
  R1HeadNbrContext *nbrs;
  R1HeadCdfContext *cdfs;
  const R1HeadBlock *blocks;
  const R1HeadTrial *trials;
  const R1HeadCommit *commits;
  const R1RdPick *state, *depth_state;
  const int16_t *cfl_alpha;
  int n_states, n_nbrs, n_cdfs, n_blocks, n_trials, call_id, group, nt;
  uint32_t tx_sizes;      // the host's table of three TxSize, a byte each: indexed by shifts, not through memory
};

struct PartRateArgs {
  const R1HeadNbrContext *nbrs;
  const R1HeadCdfContext *cdfs;
  const R1HeadBlock *nodes;
  const uint8_t *partitions;
  const uint16_t *rng_in;
  uint32_t *part_rate;
  uint16_t *rng_out;
  int n, n_nbrs, n_cdfs;
};

struct HeadResetArgs {
  R1HeadNbrContext *nbrs;
  const uint32_t *sel;
  int n, n_nbrs;
};

// What the device decided in front of this call, in place of the record's fields: the transform size of the depth the
// pick kept, the alphas the CFL search found.  -> false: best_call names no depth
__device__ __forceinline__ bool head_overrides(HeadIn &h, long long t, const R1RdPick *depth_state, uint32_t tx_sizes,
                                               const int16_t *cfl_alpha) {
  if (depth_state) {
    const int c = depth_state[t].best_call;
    if (c < 0 || c > 2) return false;
    h.tx_size = (int)((tx_sizes >> (8 * c)) & 255);
  }
  if (cfl_alpha) h.alpha_u = cfl_alpha[2 * t], h.alpha_v = cfl_alpha[2 * t + 1];
  return true;
}

__global__ __launch_bounds__(256) void k_intra_head_rate(const HeadRateArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n) return;
  const R1HeadTrial tr = a.trials[t];
  uint32_t rate = kHeadInvalid;
  RateSink k;
  if (tr.block < (uint32_t)a.n_blocks) {
    const R1HeadBlock b = a.blocks[tr.block];
    HeadIn h;
    head_in_block(h, b);
    head_in_trial(h, tr);
    if (b.nbr < (uint32_t)a.n_nbrs && b.cdf < (uint32_t)a.n_cdfs && head_overrides(h, t, a.depth_state, a.tx_sizes, a.cfl_alpha)) {
      k.cdf = (const uint16_t *)(a.cdfs + b.cdf);
      const uint32_t tell = k.w.tell_frac();
      if (head_walk<true>(k, a.nbrs + b.nbr, h)) rate = k.w.tell_frac() - tell;
    }
  }
  a.rate_add[t] = rate;
  if (rate != kHeadInvalid && a.rng_out) *(uint16_t *)(a.rng_out + t * a.rng_stride) = (uint16_t)k.w.rng;
}

__global__ __launch_bounds__(256) void k_partition_rate(const PartRateArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const R1HeadBlock b = a.nodes[i];
  const int p = a.partitions[i];
  const uint32_t rng = a.rng_in ? a.rng_in[i] : 0x8000u;
  uint32_t rate = kHeadInvalid;
  RateSink k;
  if (b.nbr < (uint32_t)a.n_nbrs && b.cdf < (uint32_t)a.n_cdfs && p <= R1_PARTITION_SPLIT && rng >= 0x8000u &&
      head_place_ok(b.bsize, b.bo_x, b.bo_y, b.mi_cols, b.mi_rows) && b.bsize >= kBlock8x8 && kBsWL[b.bsize] == kBsHL[b.bsize]) {
    k.cdf = (const uint16_t *)(a.cdfs + b.cdf);
    k.w.rng = rng;
    const uint32_t tell = k.w.tell_frac();
    int off = 0, n = 0, s = 0;
    const int arm = partition_sym(a.nbrs + b.nbr, kBsWL[b.bsize], b.bo_x, b.bo_y, b.mi_cols, b.mi_rows, p, off, n, s);
    if (arm == 1) k.sym(off, n, s);
    else if (arm == 2) k.edge(partition_gather<true>(k.cdf + off), s);
    else if (arm == 3) k.edge(partition_gather<false>(k.cdf + off), s);
    if (arm >= 0) rate = k.w.tell_frac() - tell;
  }
  a.part_rate[i] = rate;
  if (rate != kHeadInvalid && a.rng_out) a.rng_out[i] = (uint16_t)k.w.rng;
}

// One lane per state.  Everything of a desc is checked before anything of it is written.
__global__ __launch_bounds__(256) void k_intra_head_commit(const HeadCommitArgs a) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= a.n_states) return;
  const R1RdPick st = a.state[s];
  if (st.best_call != a.call_id) return;
  const R1HeadCommit c = a.commits[s];
  if (c.block >= (uint32_t)a.n_blocks) return;
  const R1HeadBlock b = a.blocks[c.block];
  if (b.nbr >= (uint32_t)a.n_nbrs || b.cdf >= (uint32_t)a.n_cdfs) return;
  R1HeadNbrContext *nb = a.nbrs + b.nbr;
  const bool event_only = (c.flags & R1_HEAD_EVENT_ONLY) != 0;
  const bool has_node = c.part_type >= 0 || c.subsize != R1_HEAD_NO_SUBSIZE;
  // the walker's node: square, 8x8 .. 64x64, inside the tile
  int node_wl = 0;
  if (has_node) {
    if (!head_place_ok(c.node_bsize, c.node_x, c.node_y, b.mi_cols, b.mi_rows)) return;
    node_wl = kBsWL[c.node_bsize];
    if (node_wl != kBsHL[c.node_bsize] || node_wl < 3) return;
  }
  int p_arm = 0, p_off = 0, p_n = 0, p_s = 0;
  if (c.part_type >= 0) {
    if (c.part_type > R1_PARTITION_SPLIT) return;
    p_arm = partition_sym(nb, node_wl, c.node_x, c.node_y, b.mi_cols, b.mi_rows, c.part_type, p_off, p_n, p_s);
    if (p_arm < 0) return;
  }
  if (c.subsize != R1_HEAD_NO_SUBSIZE && (c.subsize >= 22 || event_only)) return;
  HeadIn h;
  head_in_block(h, b);
  if (!event_only) {
    if (st.best_row < 0 || st.best_row >= a.group || st.best_slot < 0 || st.best_slot >= a.nt) return;
    const long long t = ((long long)s * a.group + st.best_row) * a.nt + st.best_slot;
    if (t >= a.n_trials) return;
    const R1HeadTrial tr = a.trials[t];
    if (tr.block != c.block) return;
    head_in_trial(h, tr);
    if (!head_overrides(h, t, a.depth_state, a.tx_sizes, a.cfl_alpha)) return;
    NullSink check;
    if (!head_walk<false>(check, nb, h)) return;
  }
  // ---- from here on the desc acts
  CommitSink k = {(uint16_t *)(a.cdfs + b.cdf)};
  if (p_arm == 1) k.sym(p_off, p_n, p_s);             // an edge arm adapts nothing
  if (event_only) return;
  head_walk<false>(k, nb, h);
  // set_mode / set_skip over the block's extent as TileBlocksMut::for_each clips it, as row buffers
  const int bw4 = 1 << (kBsWL[h.bsize] - 2), bh4 = 1 << (kBsHL[h.bsize] - 2), y_sb = h.bo_y & 15;
  const int cols = h.bo_x + bw4 >= h.mi_cols ? h.mi_cols - h.bo_x : bw4;
  for (int i = 0; i < 16; i++) {
    if (i < cols) nb->above_mode[h.bo_x + i] = (uint8_t)h.y_mode, nb->above_skip[h.bo_x + i] = 0;
    if (i < bh4 && h.bo_y + i < h.mi_rows) nb->left_mode[(y_sb + i) & 15] = (uint8_t)h.y_mode, nb->left_skip[(y_sb + i) & 15] = 0;
  }
  // update_tx_size_context (block_unit.rs:362-386), skip = false: the transform's sides over the block's spans
  if (h.tx_mode_select) {
    const uint8_t tx_w = (uint8_t)(1 << kHeadTxWL[h.tx_size]), tx_h = (uint8_t)(1 << kHeadTxHL[h.tx_size]);
    for (int i = 0; i < 16; i++) {
      if (i < bw4 && h.bo_x + i < R1_HEAD_NBR_WIDTH) nb->above_tx[h.bo_x + i] = tx_w;
      if (i < bh4 && y_sb + i < 16) nb->left_tx[y_sb + i] = tx_h;
    }
  }
  // update_partition_context (partition_unit.rs:480-503) over the node's spans
  if (c.subsize != R1_HEAD_NO_SUBSIZE) {
    const uint8_t above = (uint8_t)(31 & ~((1 << (kBsWL[c.subsize] - 2)) - 1));
    const uint8_t left = (uint8_t)(31 & ~((1 << (kBsHL[c.subsize] - 2)) - 1));
    const int n8 = 1 << (node_wl - 3), x8 = c.node_x >> 1, y8 = (c.node_y & 15) >> 1;
    for (int i = 0; i < 8; i++) {
      if (i < n8 && x8 + i < R1_HEAD_NBR_WIDTH / 2) nb->above_partition[x8 + i] = above;
      if (i < n8 && y8 + i < 8) nb->left_partition[y8 + i] = left;
    }
  }
}

// Thirty-two lanes per selected context: one byte of left_partition_context[8] or left_tx_context[16] each
__global__ __launch_bounds__(256) void k_head_nbr_reset_left(const HeadResetArgs a) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = tid >> 5;
  const int k = (int)(tid & 31);
  if (i >= a.n || k >= 24) return;
  const uint32_t s = a.sel[i];
  if (s >= (uint32_t)a.n_nbrs) return;
  if (k < 8) a.nbrs[s].left_partition[k] = 0;
  else a.nbrs[s].left_tx[k - 8] = 0;
}
}  // namespace

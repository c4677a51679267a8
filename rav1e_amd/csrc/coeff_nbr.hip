// coeff_nbr.hip -- the coefficient neighbour contexts carried from block to block on the device, and the winner's
// transform type where the adapt call reads it.
// r1_coeff_nbr_gather_batch: the R1BlockChainCtx / R1TxbChainCtx records the rate calls take, cut out of an
// R1CoeffNbrContext (BlockContext::above_coeff_context / left_coeff_context, src/context/block_unit.rs:237-238) for a
// block's place in its tile -- rdo_glue.block_chain_ctx / txb_chain_ctx on the device.
// r1_coeff_nbr_store_batch: what a coded block (set_coeff_context over its transform blocks, block_unit.rs:333-348, read
// off the rate call's ctx_out) or a skipped one (reset_skip_context, src/context/partition_unit.rs:434-469) leaves there.
// r1_coeff_nbr_reset_left_batch: the coefficient part of reset_left_contexts (block_unit.rs:394-401).
// r1_rd_winner_tx_type_batch: best_slot of an R1RdPick as the tx_type / uv_tx_type of an R1BlockRateTrial
// (write_tx_tree's rule for chroma, src/encoder.rs:2507-2511; TxType::uv_inter, src/transform/mod.rs:81-97).
// Byte movers: no LDS, no scratch, no atomics, no spin-waits; every loop is bounded by 16.  All enqueue on the caller's
// stream; nothing is read back.  Pinned by tests/golden/coeff_nbr_ref.npz.
#include "block_geom.hpp"
#include "common.hpp"

#include <stddef.h>

static_assert(sizeof(R1CoeffNbrContext) == 3120, "R1CoeffNbrContext is 3120 bytes");
static_assert(sizeof(R1NbrBlock) == 20, "R1NbrBlock is 20 bytes");
static_assert(offsetof(R1CoeffNbrContext, left) == 3 * R1_COEFF_NBR_WIDTH, "left follows above");
static_assert(sizeof(R1BlockChainCtx) == 108 && sizeof(R1TxbChainCtx) == 40 && sizeof(R1BlockRateTrial) == 24 &&
              sizeof(R1RdPick) == 24, "the records this unit writes byte by byte");

constexpr int kLeftLen = 16;       // MIB_SIZE: a superblock's 4x4 units
constexpr int kNbrLanes = 8;       // lanes per desc in the gather and the store: six 16-byte rows and two record tails

// What the host knows of a launch: the block's size in 4x4 units, the subsampling, the one-unit chroma shift of a
// 4-wide / 4-high block, and the spans a store covers per chroma plane
struct NbrGeom {
  int bw4, bh4, xdec, ydec, adj_x, adj_y;
  int uv_w4, uv_h4;       // coded: bw_uv * (uv_tw / 4), bh_uv * (uv_th / 4) -- 0 where the chroma grid is empty
  int sub_w4, sub_h4;     // skipped: bsize.subsampled_size(xdec, ydec) in 4x4 units
  int skip_all_planes;    // BLOCK_4X16 / BLOCK_16X4: `bsize >= BLOCK_8X8` holds for them in the enum's order
};

struct GatherArgs {
  const R1CoeffNbrContext *contexts;
  const R1NbrBlock *descs;
  uint8_t *blocks, *chains;
  int n, n_contexts;
  NbrGeom g;
};

struct StoreArgs {
  const R1NbrBlock *descs;
  const uint8_t *ctx_in;
  const R1RdPick *state;
  R1CoeffNbrContext *contexts;
  int n, n_contexts, call_id;
  NbrGeom g;
};

struct ResetArgs {
  R1CoeffNbrContext *contexts;
  const uint32_t *sel;
  int n, n_contexts, planes;
};

struct WinnerArgs {
  const R1RdPick *state;
  const uint16_t *eob_win;
  uint8_t *trials;
  int n_states, call_id, is_inter, ntx, uv_rule;   // uv_rule 0: the luma type, 1: IDTX or DCT_DCT, 2: no 1-D ADST
  uint32_t mask;
};

// The refusal cases the gather and the store share
__device__ __forceinline__ bool nbr_desc_ok(const R1NbrBlock &d, int n_contexts) {
  return d.nbr < (uint32_t)n_contexts && d.bo_x < R1_COEFF_NBR_WIDTH && d.y_mode < R1_INTRA_MODES && d.mi_width > d.bo_x &&
         d.mi_height > d.bo_y;
}

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Sixteen bytes of `arr` (len bytes, a multiple of 4) from entry `at`, zeros past its end; at < 0 gives zeros throughout
// (the slice of the host statement is empty there).  A4: the array is 4-byte aligned -- five aligned dwords and a byte
// shift; otherwise byte loads.
template <bool A4>
__device__ __forceinline__ void load_window(const uint8_t *arr, int len, int at, uint32_t w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0;
  if (at < 0 || at >= len) return;
  if constexpr (A4) {
    const int a0 = at & ~3, sh = (at & 3) * 8;
    uint32_t d[5];
#pragma unroll
    for (int k = 0; k < 5; k++) d[k] = a0 + 4 * k < len ? *(const uint32_t *)(arr + a0 + 4 * k) : 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> sh);
  } else {
#pragma unroll
    for (int c = 0; c < 16; c++)
      if (at + c < len) w[c >> 2] |= (uint32_t)arr[at + c] << ((c & 3) * 8);
  }
}

template <bool A4>
__device__ __forceinline__ void store_words(uint8_t *dst, const uint32_t *w, int n_words) {
  for (int k = 0; k < n_words; k++) {
    if constexpr (A4) {
      *(uint32_t *)(dst + 4 * k) = w[k];
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++) dst[4 * k + b] = (uint8_t)(w[k] >> (8 * b));
    }
  }
}

// Eight lanes per desc, so a wave covers eight: lanes 0-5 move the row ctx[plane][above / left] (lanes 0 and 1 also the
// chain record's above / left), lane 6 writes the block record's twelve trailing bytes, lane 7 the chain record's eight.
// A4: contexts, blocks and chains are 4-byte aligned (both records are multiples of 4 bytes).
template <bool A4>
__global__ __launch_bounds__(256) void k_coeff_nbr_gather(const GatherArgs a) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = tid / kNbrLanes;
  const int r = (int)(tid % kNbrLanes);
  if (i >= a.n) return;
  const R1NbrBlock d = a.descs[i];
  const NbrGeom &g = a.g;
  const bool ok = nbr_desc_ok(d, a.n_contexts);
  uint8_t *blk = a.blocks ? a.blocks + (size_t)i * sizeof(R1BlockChainCtx) : nullptr;
  uint8_t *chn = a.chains ? a.chains + (size_t)i * sizeof(R1TxbChainCtx) : nullptr;
  // the first chroma transform block's offset (encoder.rs:2364-2369): may be -1 where the reference never asks
  const int ux = (int)d.bo_x - g.adj_x, uy = (int)d.bo_y - g.adj_y;
  if (r < 6) {
    const int p = r >> 1, left = r & 1;
    uint32_t w[4] = {0, 0, 0, 0};
    if (ok) {
      const R1CoeffNbrContext *c = a.contexts + d.nbr;
      if (left) load_window<A4>(c->left[p], kLeftLen, p == 0 ? (d.bo_y & 15) : ((uy & 15) >> g.ydec), w);
      else load_window<A4>(c->above[p], R1_COEFF_NBR_WIDTH, p == 0 ? (int)d.bo_x : (ux >> g.xdec), w);
    }
    if (blk) store_words<A4>(blk + r * 16, w, 4);
    if (chn && p == 0) store_words<A4>(chn + r * 16, w, 4);
    return;
  }
  const int mi_w = clamp_u8((int)d.mi_width - d.bo_x), mi_h = clamp_u8((int)d.mi_height - d.bo_y);
  const int clip_w = clamp_u8((int)d.w_in_b - d.bo_x), clip_h = clamp_u8((int)d.h_in_b - d.bo_y);
  uint32_t w[3];
  if (r == 6) {
    if (!blk) return;
    // min(255, max(0, (((fi.w_in_b - frame_bo.x) << MI_SIZE_LOG2) >> xdec) >> 2)) at the first chroma transform block,
    // which is (w_in_b - ux) >> xdec clamped.  Clamped to [0, (256 << xdec) - 1] FIRST and shifted then: written as
    // shift-then-clamp, the pair is fused into one packed shift-and-saturate instruction of gfx950 whose upper result half
    // came back from the device holding the destination register's previous bits, which then landed in y_mode.
    const int vw = (int)d.w_in_b - ux, vh = (int)d.h_in_b - uy;
    const int hw = (256 << g.xdec) - 1, hh = (256 << g.ydec) - 1;
    const int cuw = (vw < 0 ? 0 : (vw > hw ? hw : vw)) >> g.xdec;
    const int cuh = (vh < 0 ? 0 : (vh > hh ? hh : vh)) >> g.ydec;
    w[0] = (uint32_t)mi_w | (uint32_t)mi_h << 8 | (uint32_t)clip_w << 16 | (uint32_t)clip_h << 24;
    w[1] = (uint32_t)cuw | (uint32_t)cuh << 8 | (uint32_t)d.y_mode << 16 | (uint32_t)d.cdf_sel << 24;
    w[2] = d.cdf_sel_uv;
    if (!ok) w[0] = 0, w[1] = 255u << 16, w[2] = 0;
    store_words<A4>(blk + 96, w, 3);
  } else {
    if (!chn) return;
    w[0] = (uint32_t)mi_w | (uint32_t)mi_h << 8 | (uint32_t)clip_w << 16 | (uint32_t)clip_h << 24;
    w[1] = (uint32_t)d.y_mode | (uint32_t)d.cdf_sel << 8;
    if (!ok) w[0] = 0, w[1] = 255u;
    store_words<A4>(chn + 32, w, 2);
  }
}

// Eight lanes per desc; lanes 0-5 own the row (plane, above / left) and write its span, lanes 6 and 7 idle.  A span is at
// most 16 bytes at any byte offset: whole dwords where offset and length allow it (A4: contexts and ctx_in are 4-byte
// aligned), bytes otherwise.  Acting descs name distinct contexts (the caller's to keep), so no two lanes write one byte.
template <bool A4>
__global__ __launch_bounds__(256) void k_coeff_nbr_store(const StoreArgs a) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = tid / kNbrLanes;
  const int r = (int)(tid % kNbrLanes);
  if (i >= a.n || r >= 6) return;
  if (a.state && a.state[i].best_call != a.call_id) return;
  const R1NbrBlock d = a.descs[i];
  const NbrGeom &g = a.g;
  if (!nbr_desc_ok(d, a.n_contexts)) return;
  const bool skip = (d.flags & 2) != 0, do_chroma = (d.flags & 1) != 0;
  if (!skip && !a.ctx_in) return;
  const int y_sb = d.bo_y & 15;
  // every span of the desc, checked whole before anything of it is written
  if ((int)d.bo_x + g.bw4 > R1_COEFF_NBR_WIDTH || y_sb + g.bh4 > kLeftLen) return;
  int cx, cy, cw, ch;
  bool chroma;
  if (skip) {
    // nplanes of reset_skip_context: three for every size at or above BLOCK_8X8 in the enum's order, else has_chroma
    chroma = do_chroma || g.skip_all_planes;
    cx = (int)d.bo_x >> g.xdec, cy = y_sb >> g.ydec, cw = g.sub_w4, ch = g.sub_h4;
  } else {
    const int ux = (int)d.bo_x - g.adj_x, uy = (int)d.bo_y - g.adj_y;
    chroma = do_chroma && g.uv_w4 > 0;
    if (chroma && (ux < 0 || uy < 0)) return;
    cx = ux >> g.xdec, cy = (uy & 15) >> g.ydec, cw = g.uv_w4, ch = g.uv_h4;
  }
  if (chroma && (cx + cw > R1_COEFF_NBR_WIDTH || cy + ch > kLeftLen)) return;
  const int p = r >> 1, left = r & 1;
  if (p != 0 && !chroma) return;
  R1CoeffNbrContext *c = a.contexts + d.nbr;
  uint8_t *dst = left ? c->left[p] + (p == 0 ? y_sb : cy) : c->above[p] + (p == 0 ? (int)d.bo_x : cx);
  const int len = p == 0 ? (left ? g.bh4 : g.bw4) : (left ? ch : cw);   // 1 .. 16
  uint32_t w[4] = {0, 0, 0, 0};
  if (!skip) load_window<A4>(a.ctx_in + (size_t)i * 96 + r * 16, 16, 0, w);
  const int at = (int)(dst - (uint8_t *)c);                              // the struct's rows start at multiples of 16
  if (A4 && ((at | len) & 3) == 0) {
    for (int k = 0; k < 4; k++)
      if (4 * k < len) *(uint32_t *)(dst + 4 * k) = w[k];
  } else {
    for (int k = 0; k < 16; k++)
      if (k < len) dst[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
  }
}

// Sixteen lanes per selected context, one per dword of left[3][16]; lanes past planes * 4 idle
template <bool A4>
__global__ __launch_bounds__(256) void k_coeff_nbr_reset_left(const ResetArgs a) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = tid >> 4;
  const int k = (int)(tid & 15);
  if (i >= a.n || k >= a.planes * 4) return;
  const uint32_t s = a.sel[i];
  if (s >= (uint32_t)a.n_contexts) return;
  const uint32_t zero = 0;
  store_words<A4>(&a.contexts[s].left[0][0] + 4 * k, &zero, 1);
}

// One lane per state: two byte stores at most
__global__ __launch_bounds__(256) void k_rd_winner_tx_type(const WinnerArgs a) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= a.n_states) return;
  const R1RdPick st = a.state[s];
  if (st.best_call != a.call_id) return;
  if (st.best_slot < 0 || st.best_slot >= __builtin_popcount(a.mask)) return;
  uint32_t m = a.mask;
  for (int j = 0; j < 16; j++)                      // drop the best_slot lowest set bits
    if (j < st.best_slot) m &= m - 1;
  const int tx_type = __builtin_ctz(m);
  uint8_t *t = a.trials + (size_t)s * sizeof(R1BlockRateTrial);
  t[offsetof(R1BlockRateTrial, tx_type)] = (uint8_t)tx_type;
  if (!a.is_inter) return;
  bool has_coeff = false;
  for (int k = 0; k < 16; k++)
    if (k < a.ntx) has_coeff |= a.eob_win[(size_t)s * 16 + k] != 0;
  int uv = tx_type;
  if (a.uv_rule == 1) uv = tx_type == 9 ? 9 : 0;
  else if (a.uv_rule == 2 && tx_type >= 12) uv = 0;
  t[offsetof(R1BlockRateTrial, uv_tx_type)] = (uint8_t)(has_coeff ? uv : 0);
}

static bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

// The checks of the block's size and subsampling the gather and the store share, and the geometry they decide
static int nbr_geom(int bw, int bh, int xdec, int ydec, NbrGeom &g) {
  R1_REQUIRE(r1_block_size_ok(bw, bh));
  R1_REQUIRE(r1_subsampling_ok(xdec, ydec));
  R1_REQUIRE(r1_subsampling_admits(xdec, ydec, bw, bh));
  const R1BlockGeom b = r1_block_geom(bw, bh, xdec, ydec);
  g = {b.bw4, b.bh4, xdec, ydec, b.adj_x, b.adj_y, b.uv_w4, b.uv_h4, b.sub_w4, b.sub_h4, b.skip_all_planes};
  return R1_OK;
}

static unsigned nbr_grid(long long n, int lanes) { return (unsigned)((n * lanes + 255) / 256); }

extern "C" int r1_coeff_nbr_gather_batch(r1_ctx *ctx, const R1CoeffNbrContext *contexts, int n_contexts,
                                         const R1NbrBlock *descs, int n, int bw, int bh, int xdec, int ydec,
                                         R1BlockChainCtx *blocks_out, R1TxbChainCtx *chains_out, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(contexts && descs);
  R1_REQUIRE(blocks_out || chains_out);
  R1_REQUIRE(n >= 0 && n_contexts >= 1);
  GatherArgs a = {};
  const int rc = nbr_geom(bw, bh, xdec, ydec, a.g);
  if (rc != R1_OK) return rc;
  if (n == 0) return R1_OK;
  a.contexts = contexts, a.descs = descs, a.blocks = (uint8_t *)blocks_out, a.chains = (uint8_t *)chains_out;
  a.n = n, a.n_contexts = n_contexts;
  R1DeviceGuard guard(ctx);
  r1_by_bool(aligned4(contexts) && aligned4(blocks_out) && aligned4(chains_out), [&](auto A) {
    hipLaunchKernelGGL(k_coeff_nbr_gather<A.value>, dim3(nbr_grid(n, kNbrLanes)), dim3(256), 0, (hipStream_t)stream, a);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_coeff_nbr_store_batch(r1_ctx *ctx, const R1NbrBlock *descs, int n, int bw, int bh, int tx_size, int xdec,
                                        int ydec, const uint8_t *ctx_in, const R1RdPick *state, int call_id,
                                        R1CoeffNbrContext *contexts, int n_contexts, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(contexts && descs);
  R1_REQUIRE(n >= 0 && n_contexts >= 1);
  R1_REQUIRE(!state || (call_id >= 0 && call_id <= 127));
  StoreArgs a = {};
  const int rc = nbr_geom(bw, bh, xdec, ydec, a.g);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(r1_luma_grid(bw, bh, tx_size).divides);
  if (n == 0) return R1_OK;
  a.descs = descs, a.ctx_in = ctx_in, a.state = state, a.contexts = contexts;
  a.n = n, a.n_contexts = n_contexts, a.call_id = call_id;
  R1DeviceGuard guard(ctx);
  r1_by_bool(aligned4(contexts) && aligned4(ctx_in), [&](auto A) {
    hipLaunchKernelGGL(k_coeff_nbr_store<A.value>, dim3(nbr_grid(n, kNbrLanes)), dim3(256), 0, (hipStream_t)stream, a);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_coeff_nbr_reset_left_batch(r1_ctx *ctx, R1CoeffNbrContext *contexts, int n_contexts, const uint32_t *sel,
                                             int n, int planes, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(contexts && sel);
  R1_REQUIRE(n >= 0 && n_contexts >= 1);
  R1_REQUIRE(planes >= 1 && planes <= 3);
  if (n == 0) return R1_OK;
  const ResetArgs a = {contexts, sel, n, n_contexts, planes};
  R1DeviceGuard guard(ctx);
  r1_by_bool(aligned4(contexts), [&](auto A) {
    hipLaunchKernelGGL(k_coeff_nbr_reset_left<A.value>, dim3(nbr_grid(n, 16)), dim3(256), 0, (hipStream_t)stream, a);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_rd_winner_tx_type_batch(r1_ctx *ctx, const R1RdPick *state, int n_states, int call_id,
                                          uint32_t tx_type_mask, int is_inter, int uv_tx_size, const uint16_t *eob_win,
                                          int ntx, R1BlockRateTrial *trials, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(state && trials);
  R1_REQUIRE(n_states >= 0);
  R1_REQUIRE(call_id >= 0 && call_id <= 127);
  is_inter = is_inter != 0;
  // the largest set of the prediction kind: TX_SET_ALL16 for inter, TX_SET_INTRA_1 for intra
  R1_REQUIRE(tx_type_mask != 0 && (tx_type_mask & ~r1_tx_type_mask(0, is_inter, 0, 0)) == 0);
  R1_REQUIRE(r1_tx_size_ok(uv_tx_size));
  R1_REQUIRE(ntx >= 1 && ntx <= 16);
  R1_REQUIRE(!is_inter || eob_win);
  if (n_states == 0) return R1_OK;
  const WinnerArgs a = {state, eob_win, (uint8_t *)trials, n_states, call_id, is_inter, ntx, r1_uv_inter_rule(uv_tx_size),
                        tx_type_mask};
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_rd_winner_tx_type, dim3(nbr_grid(n_states, 1)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

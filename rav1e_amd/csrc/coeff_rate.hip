// coeff_rate.hip -- r1_coeff_rate_batch: the real coefficient rate of one transform block per (candidate, type)
// slot, as rdo_tx_type_decision measures it (src/rdo.rs:1744-1799): a fresh WriterCounter (src/ec.rs:193-201,
// 317-319), tell_frac, write_coeffs_lv_map (src/context/block_unit.rs:1783-2016), tell_frac, CDFs rolled back.
// Every slot starts from an unadapted copy of its R1CoeffCdfs snapshot, so the slots are independent.
// r1_coeff_rate_chain_batch: the same over the luma transform blocks of a block in raster order, as rdo_tx_size_type
// measures a transform depth (src/rdo.rs:725-802): one counter, one adapting CDF copy and the block's 32 neighbour
// context bytes carried from transform block to transform block (k_coeff_rate_chain).
// r1_coeff_rate_block_batch: the same over the luma, U and V transform blocks of a block, as write_tx_blocks /
// write_tx_tree code them with luma_only = false behind the head symbols of the mode decision (src/rdo.rs:855-945,
// src/encoder.rs:2202-2240): one counter that starts at a handed-over rng, the luma snapshot and then the chroma one in
// the adapting copy, 96 context bytes (k_coeff_rate_block).
// r1_coeff_cdf_slice_batch / r1_coeff_cdf_adapt_batch: the CDF state carried from block to block on the device -- the
// snapshot the calls above take, cut out of an R1CoeffCdfContext, and the whole-block walk once more on the winner, with
// the adapted rows written back to the context (k_coeff_cdf_slice, k_coeff_cdf_adapt).
// This is the host half: checks, launch arguments, entry points; the kernels are coeff_rate_kernel.hpp, and what the
// reference says of a block and of the transform sets (av1_tx_ind / num_tx_set / av1_tx_used) is block_geom.hpp.
#include "block_geom.hpp"
#include "coeff_rate_kernel.hpp"
#include "quant_common.hpp"

// What the transform size and the set decide of the launch arguments (tx_size is valid, the flags are 0 / 1) -> the set
static int rate_shape(r1_ctx *ctx, int tx_size, int plane, int is_inter, int use_reduced_tx_set, RateArgs &a) {
  const int set = r1_tx_set(tx_size, is_inter, use_reduced_tx_set);
  const int wl = r1tx::kTxWLog2[tx_size], hl = r1tx::kTxHLog2[tx_size];
  for (int k = 0; k < 3; k++) a.scan[k] = ctx->scan_dev + ctx->scan_off[tx_size][k];
  a.plane = plane;
  a.w_coded = r1q::coded_dim(wl);
  a.hl = r1_ilog2(r1q::coded_dim(hl));
  a.area = a.w_coded << a.hl;
  a.shape = wl < hl ? 1 : (wl > hl ? 2 : 0);
  a.eob_flag_n = 5 + (wl + hl - 4 < 6 ? wl + hl - 4 : 6);   // eob_multi_size = area_log2 - 4; `_ =>`: eob_flag_cdf1024
  a.tx_n = r1tx::kNumTxSet[set] > 1 ? r1tx::kNumTxSet[set] : 0;
  a.is_inter = is_inter;
  return set;
}

// The checks every rate entry point shares -- the context, the coefficient width, the transform size (rate_common) --
// and those of the three that read snapshots: the snapshots, the output every call writes, the launch arguments they
// decide (rate_base)
static int rate_common(r1_ctx *ctx, int coeff_bytes, int tx_size) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(coeff_bytes == 2 || coeff_bytes == 4);
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  return R1_OK;
}
static int rate_base(r1_ctx *ctx, int coeff_bytes, int tx_size, const R1CoeffCdfs *cdfs, int n_cdfs, uint32_t *rate_out,
                     uint8_t *cul_level_out, RateArgs &a) {
  const int rc = rate_common(ctx, coeff_bytes, tx_size);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(n_cdfs >= 1 && n_cdfs <= 256);
  R1_REQUIRE(cdfs && rate_out);
  a = {};
  a.cdfs = cdfs, a.rate = rate_out, a.cul = cul_level_out, a.n_cdfs = n_cdfs;
  return R1_OK;
}

// The checks and the launch arguments the slot and chain entry points share: what the transform size, the type mask and
// the set decide.  `per_block`: slots per candidate beyond the types (1, or the chain's ntx) for the 2^31 bound.
static int rate_args(r1_ctx *ctx, const void *qcoeffs, int coeff_bytes, const uint16_t *eobs, int n, uint32_t tx_type_mask,
                     int tx_size, int plane, int is_inter, int use_reduced_tx_set, const R1CoeffCdfs *cdfs, int n_cdfs,
                     uint32_t *rate_out, uint8_t *cul_level_out, int per_block, RateArgs &a) {
  const int rc = rate_base(ctx, coeff_bytes, tx_size, cdfs, n_cdfs, rate_out, cul_level_out, a);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(plane >= 0 && plane <= 2);
  is_inter = is_inter != 0;
  use_reduced_tx_set = use_reduced_tx_set != 0;
  const uint32_t allowed = r1tx::kTxUsed[r1_tx_set(tx_size, is_inter, use_reduced_tx_set)];
  R1_REQUIRE(tx_type_mask != 0 && (tx_type_mask & ~allowed) == 0);
  R1_REQUIRE(qcoeffs && eobs);
  a.qc = qcoeffs, a.eobs = eobs;
  a.nt = __builtin_popcount(tx_type_mask);
  R1_REQUIRE((long long)(n > 0 ? n : 0) * a.nt * per_block <= 0x7fffffffLL);
  a.n_slots = (n > 0 ? n : 0) * a.nt;
  const int set = rate_shape(ctx, tx_size, plane, is_inter, use_reduced_tx_set, a);
  for (int t = 0, j = 0; t < 16; t++)
    if ((tx_type_mask >> t) & 1) a.type[j] = (uint8_t)t, a.tx_sym[j] = r1tx::kTxInd[set][t], j++;
  return R1_OK;
}

// A bw x bh block under transforms of tx_size: the luma grid of the chain and of the whole block
static int luma_grid(int bw, int bh, int tx_size, TxbGrid &g) {
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(r1_block_size_ok(bw, bh));
  const R1LumaGrid l = r1_luma_grid(bw, bh, tx_size);
  R1_REQUIRE(l.divides);
  g = {l.ntx, l.gw, l.tw4, l.th4, 0, 0, 0, 0};
  R1_REQUIRE(g.ntx >= 1 && g.ntx <= 16);
  return R1_OK;
}

// One wave per slot, four slots per workgroup: kernel(CT{}) is the instantiation for coefficients of type CT
template <class Args, class Kernel>
static int rate_launch(r1_ctx *ctx, int coeff_bytes, int n_slots, void *stream, const Args &args, Kernel kernel) {
  R1DeviceGuard guard(ctx);
  r1_by_value<4, 2>(coeff_bytes, [&](auto B) {
    using CT = std::conditional_t<B.value == 2, int16_t, int32_t>;
    hipLaunchKernelGGL(kernel(CT{}), dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, (hipStream_t)stream, args);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_coeff_rate_batch(r1_ctx *ctx, const void *qcoeffs, int coeff_bytes, const uint16_t *eobs, int n,
                                   uint32_t tx_type_mask, int tx_size, int plane, int is_inter,
                                   int use_reduced_tx_set, const R1TxbCtx *ctxs, const R1CoeffCdfs *cdfs, int n_cdfs,
                                   uint32_t *rate_out, uint8_t *cul_level_out, void *stream) {
  RateArgs a;
  const int rc = rate_args(ctx, qcoeffs, coeff_bytes, eobs, n, tx_type_mask, tx_size, plane, is_inter, use_reduced_tx_set,
                           cdfs, n_cdfs, rate_out, cul_level_out, 1, a);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(ctxs);
  if (n <= 0) return R1_OK;
  a.ctxs = ctxs;
  return rate_launch(ctx, coeff_bytes, a.n_slots, stream, a, [](auto ct) { return k_coeff_rate<decltype(ct)>; });
}

extern "C" int r1_coeff_rate_chain_batch(r1_ctx *ctx, const void *qcoeffs, int coeff_bytes, const uint16_t *eobs, int n,
                                         uint32_t tx_type_mask, int bw, int bh, int tx_size, int order, int is_inter,
                                         int use_reduced_tx_set, const R1TxbChainCtx *chains, const R1CoeffCdfs *cdfs,
                                         int n_cdfs, uint32_t *rate_out, uint32_t *txb_rate_out, uint8_t *cul_level_out,
                                         uint8_t *ctx_out, void *stream) {
  ChainArgs c = {};
  int rc = luma_grid(bw, bh, tx_size, c.g);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(order == 0 || order == 1);
  rc = rate_args(ctx, qcoeffs, coeff_bytes, eobs, n, tx_type_mask, tx_size, 0, is_inter, use_reduced_tx_set, cdfs, n_cdfs,
                 rate_out, cul_level_out, c.g.ntx, c.r);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(chains);
  if (n <= 0) return R1_OK;
  c.chains = chains, c.txb_rate = txb_rate_out, c.ctx_out = ctx_out, c.order = order;
  return rate_launch(ctx, coeff_bytes, c.r.n_slots, stream, c, [](auto ct) { return k_coeff_rate_chain<decltype(ct)>; });
}

// What r1_coeff_rate_block_batch and r1_coeff_cdf_adapt_batch share: the checks of the coefficient, trial and block
// arguments and everything of the launch arguments they decide.  c.r[0] holds the caller's part (the snapshots and the
// outputs) on entry.  -> the chroma transform size in uv_tx_size
static int block_args(r1_ctx *ctx, const void *qcoeffs_y, const uint16_t *eobs_y, int n_txb_y, int step_y,
                      const void *qcoeffs_u, const uint16_t *eobs_u, const void *qcoeffs_v, const uint16_t *eobs_v,
                      int n_txb_uv, int step_uv, const R1BlockRateTrial *trials, int n, int bw, int bh, int tx_size,
                      int xdec, int ydec, int is_inter, int use_reduced_tx_set, const R1BlockChainCtx *blocks,
                      int n_blocks, BlockArgs &c, int &uv_tx_size) {
  TxbGrid g;
  const int rc = luma_grid(bw, bh, tx_size, g);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(r1_subsampling_ok(xdec, ydec));
  R1_REQUIRE(r1_subsampling_admits(xdec, ydec, bw, bh));
  R1_REQUIRE(step_y >= 1 && step_uv >= 1 && n_txb_y >= 0 && n_txb_uv >= 0);
  R1_REQUIRE(n_blocks >= 1);
  R1_REQUIRE(qcoeffs_y && eobs_y && trials && blocks);
  const int n_uv_ptrs = (qcoeffs_u != nullptr) + (eobs_u != nullptr) + (qcoeffs_v != nullptr) + (eobs_v != nullptr);
  R1_REQUIRE(n_uv_ptrs == 0 || n_uv_ptrs == 4);
  const R1BlockGeom b = r1_block_geom(bw, bh, xdec, ydec);
  uv_tx_size = b.uv_tx_size;

  c.r[0].n_slots = n > 0 ? n : 0;
  c.r[1] = c.r[0];
  const int set = rate_shape(ctx, tx_size, 0, is_inter, use_reduced_tx_set, c.r[0]);
  rate_shape(ctx, uv_tx_size, 1, is_inter, use_reduced_tx_set, c.r[1]);
  for (int t = 0; t < 16; t++) {
    c.r[0].type[t] = c.r[1].type[t] = (uint8_t)t;
    c.r[0].tx_sym[t] = r1tx::kTxInd[set][t];
  }
  c.mask[0] = r1tx::kTxUsed[set];
  c.mask[1] = (b.uw == 32 || b.uh == 32) ? 0x0201u : 0xFFFFu;   // the scans av1_scan_orders holds for the size
  c.pl[0] = {qcoeffs_y, eobs_y, n_txb_y, step_y, g};
  c.pl[1] = {qcoeffs_u, eobs_u, n_txb_uv, step_uv,
             {b.bw_uv * b.bh_uv, b.bw_uv > 0 ? b.bw_uv : 1, b.uw >> 2, b.uh >> 2, xdec, ydec, b.adj_x, b.adj_y}};
  c.pl[2] = c.pl[1];
  c.pl[2].qc = qcoeffs_v, c.pl[2].eobs = eobs_v;
  c.trials = trials, c.blocks = blocks;
  c.n_blocks = n_blocks;
  c.uv_skip_off = b.uv_skip_off;
  return R1_OK;
}

extern "C" int r1_coeff_rate_block_batch(r1_ctx *ctx, const void *qcoeffs_y, const uint16_t *eobs_y, int n_txb_y, int step_y,
                                         const void *qcoeffs_u, const uint16_t *eobs_u, const void *qcoeffs_v,
                                         const uint16_t *eobs_v, int n_txb_uv, int step_uv, int coeff_bytes,
                                         const R1BlockRateTrial *trials, int n, int bw, int bh, int tx_size, int xdec,
                                         int ydec, int is_inter, int use_reduced_tx_set, const R1BlockChainCtx *blocks,
                                         int n_blocks, const R1CoeffCdfs *cdfs, int n_cdfs, uint32_t *rate_out,
                                         uint32_t *plane_rate_out, uint16_t *rng_out, uint8_t *cul_level_out,
                                         uint8_t *ctx_out, void *stream) {
  BlockArgs c = {};
  int rc = rate_base(ctx, coeff_bytes, tx_size, cdfs, n_cdfs, rate_out, cul_level_out, c.r[0]);
  if (rc != R1_OK) return rc;
  int uv_tx_size;
  rc = block_args(ctx, qcoeffs_y, eobs_y, n_txb_y, step_y, qcoeffs_u, eobs_u, qcoeffs_v, eobs_v, n_txb_uv, step_uv, trials, n,
                  bw, bh, tx_size, xdec, ydec, is_inter != 0, use_reduced_tx_set != 0, blocks, n_blocks, c, uv_tx_size);
  if (rc != R1_OK) return rc;
  if (n <= 0) return R1_OK;
  c.plane_rate = plane_rate_out, c.rng_out = rng_out, c.ctx_out = ctx_out;
  return rate_launch(ctx, coeff_bytes, c.r[0].n_slots, stream, c, [](auto ct) { return k_coeff_rate_block<decltype(ct)>; });
}

// ---- the device-resident coefficient CDF context: r1_coeff_cdf_slice_batch, r1_coeff_cdf_adapt_batch
// Where the R1CoeffCdfs slice of (tx_size, plane_type, is_inter, reduced) lies in an R1CoeffCdfContext: the gather rule
// of the header (tx_size is valid, the other three are 0 / 1)
static void cdf_map(int tx_size, int plane_type, int is_inter, int use_reduced_tx_set, CdfMap &m) {
  auto off = [](size_t bytes) { return (uint16_t)(bytes / 2); };
  const int wl = r1tx::kTxWLog2[tx_size], hl = r1tx::kTxHLog2[tx_size];
  const int txs_ctx = r1_txs_ctx(tx_size);
  const int ems = wl + hl - 4 < 6 ? wl + hl - 4 : 6;                           // eob_multi_size; `_ =>`: eob_flag_cdf1024
  const int tp = txs_ctx * 2 + plane_type, br = (txs_ctx < 3 ? txs_ctx : 3) * 2 + plane_type;
  static const size_t kEobFlag[7] = {offsetof(R1CoeffCdfContext, eob_flag16),  offsetof(R1CoeffCdfContext, eob_flag32),
                                     offsetof(R1CoeffCdfContext, eob_flag64),  offsetof(R1CoeffCdfContext, eob_flag128),
                                     offsetof(R1CoeffCdfContext, eob_flag256), offsetof(R1CoeffCdfContext, eob_flag512),
                                     offsetof(R1CoeffCdfContext, eob_flag1024)};
  const uint16_t nf = (uint16_t)(5 + ems);
  m = {};
  // txb_skip is shared by txs_ctx: luma adapts rows 0-6, chroma 7-12 (get_txb_ctx)
  m.seg[0] = {off(offsetof(R1CoeffCdfContext, txb_skip) + txs_ctx * sizeof(uint16_t[R1_TXB_SKIP_CONTEXTS][2])), 2, R1_TXB_SKIP_CONTEXTS, (uint16_t)(plane_type ? 7 : 0),
              (uint16_t)(plane_type ? R1_TXB_SKIP_CONTEXTS : 7)};
  m.seg[1] = {(uint16_t)(off(kEobFlag[ems]) + plane_type * 2 * nf), nf, 2, 0, 2};
  m.seg[2] = {off(offsetof(R1CoeffCdfContext, eob_extra) + tp * sizeof(uint16_t[R1_EOB_COEF_CONTEXTS][2])), 2, R1_EOB_COEF_CONTEXTS,
              0, R1_EOB_COEF_CONTEXTS};
  m.seg[3] = {off(offsetof(R1CoeffCdfContext, coeff_base_eob) + tp * sizeof(uint16_t[R1_SIG_COEF_CONTEXTS_EOB][3])), 3,
              R1_SIG_COEF_CONTEXTS_EOB, 0, R1_SIG_COEF_CONTEXTS_EOB};
  m.seg[4] = {off(offsetof(R1CoeffCdfContext, coeff_base) + tp * sizeof(uint16_t[R1_SIG_COEF_CONTEXTS][4])), 4, R1_SIG_COEF_CONTEXTS,
              0, R1_SIG_COEF_CONTEXTS};
  m.seg[5] = {off(offsetof(R1CoeffCdfContext, coeff_br) + br * sizeof(uint16_t[R1_LEVEL_CONTEXTS][R1_BR_CDF_SIZE])), R1_BR_CDF_SIZE,
              R1_LEVEL_CONTEXTS, 0, R1_LEVEL_CONTEXTS};
  m.seg[6] = {off(offsetof(R1CoeffCdfContext, dc_sign) + plane_type * sizeof(uint16_t[R1_DC_SIGN_CONTEXTS][2])), 2,
              R1_DC_SIGN_CONTEXTS, 0, R1_DC_SIGN_CONTEXTS};
  // write_tx_type (transform_unit.rs:530-574): the table of get_tx_set_index at tx_size.sqr(); sets in TxSet order
  const int set = r1_tx_set(tx_size, is_inter, use_reduced_tx_set);
  if (plane_type == 0 && r1tx::kNumTxSet[set] > 1) {
    const uint16_t n = r1tx::kNumTxSet[set];
    size_t at = 0;
    switch (set) {
      case 1: at = offsetof(R1CoeffCdfContext, inter_tx_3); break;   // TX_SET_INTER_3: index 3
      case 2: at = offsetof(R1CoeffCdfContext, intra_tx_2); break;   // TX_SET_INTRA_2: index 2
      case 3: at = offsetof(R1CoeffCdfContext, intra_tx_1); break;   // TX_SET_INTRA_1: index 1
      case 4: at = offsetof(R1CoeffCdfContext, inter_tx_2); break;   // TX_SET_INTER_2: index 2
      default: at = offsetof(R1CoeffCdfContext, inter_tx_1); break;  // TX_SET_INTER_1: index 1
    }
    const uint16_t rows = is_inter ? 1 : R1_INTRA_MODES;             // row 0 for inter, row y_mode for intra
    m.seg[7] = {(uint16_t)(off(at) + r1_txsize_sqr_log2(tx_size) * rows * n), n, rows, 0, rows};
  }
}

extern "C" int r1_coeff_cdf_slice_batch(r1_ctx *ctx, const R1CoeffCdfContext *contexts, int n, int tx_size, int plane_type,
                                        int is_inter, int use_reduced_tx_set, R1CoeffCdfs *slices_out, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(plane_type == 0 || plane_type == 1);
  R1_REQUIRE(n >= 0);
  R1_REQUIRE(contexts && slices_out);
  if (n == 0) return R1_OK;
  SliceArgs a = {contexts, slices_out, n, {}};
  cdf_map(tx_size, plane_type, is_inter != 0, use_reduced_tx_set != 0, a.map);
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_coeff_cdf_slice, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_coeff_cdf_adapt_batch(r1_ctx *ctx, const void *qcoeffs_y, const uint16_t *eobs_y, int n_txb_y, int step_y,
                                        const void *qcoeffs_u, const uint16_t *eobs_u, const void *qcoeffs_v,
                                        const uint16_t *eobs_v, int n_txb_uv, int step_uv, int coeff_bytes,
                                        const R1BlockRateTrial *trials, int n, int bw, int bh, int tx_size, int xdec,
                                        int ydec, int is_inter, int use_reduced_tx_set, const R1BlockChainCtx *blocks,
                                        int n_blocks, R1CoeffCdfContext *contexts, const R1RdPick *state, int call_id,
                                        uint32_t *rate_out, uint16_t *rng_out, uint8_t *ctx_out, void *stream) {
  AdaptArgs c = {};
  int rc = rate_common(ctx, coeff_bytes, tx_size);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(contexts);
  R1_REQUIRE(!state || (call_id >= 0 && call_id <= 127));
  c.b.r[0].rate = rate_out;
  is_inter = is_inter != 0, use_reduced_tx_set = use_reduced_tx_set != 0;
  int uv_tx_size;
  rc = block_args(ctx, qcoeffs_y, eobs_y, n_txb_y, step_y, qcoeffs_u, eobs_u, qcoeffs_v, eobs_v, n_txb_uv, step_uv, trials, n,
                  bw, bh, tx_size, xdec, ydec, is_inter, use_reduced_tx_set, blocks, n_blocks, c.b, uv_tx_size);
  if (rc != R1_OK) return rc;
  if (n <= 0) return R1_OK;
  c.b.rng_out = rng_out, c.b.ctx_out = ctx_out;
  c.io.contexts = contexts, c.io.state = state, c.io.call_id = call_id;
  cdf_map(tx_size, 0, is_inter, use_reduced_tx_set, c.io.map[0]);
  cdf_map(uv_tx_size, 1, is_inter, use_reduced_tx_set, c.io.map[1]);
  return rate_launch(ctx, coeff_bytes, c.b.r[0].n_slots, stream, c, [](auto ct) { return k_coeff_cdf_adapt<decltype(ct)>; });
}

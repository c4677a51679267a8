// rdo_cand.hip -- the host side of the fused RDO candidate kernel: the argument checks, the dispatch over the
// fifteen (bit depth, slice) objects (twelve more for the intra prediction source) and the C entry points.  The
// kernel itself is rdo_cand_kernel.hpp, compiled by rdo_cand_slice.hip; this unit sees only what it shares with
// the slices (rdo_cand_args.hpp, and through it the plan of rdo_cand_plan.hpp).
#include "block_geom.hpp"
#include "itx_common.hpp"   // kInvShift
#include "rdo_cand_args.hpp"

namespace {
// The source plane and the block of every entry point: pixel format against bit depth, w x h against tx_size.
int rdo_plane_checks(const R1Plane *org, int w, int h, int tx_size) {
  R1_REQUIRE(r1_px_ok(*org));
  R1_REQUIRE(r1_px_fits_depth(*org));
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE((1 << r1tx::kTxWLog2[tx_size]) == w && (1 << r1tx::kTxHLog2[tx_size]) == h);
  return R1_OK;
}

int rdo_dispatch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, int w, int h, int tx_size,
                 const R1RdoCand *cands, int n, uint32_t *sad_out, uint32_t *satd_out,
                 void *coeffs, void *pred_out, const RdoQuantArgs *qa, void *stream, bool mt = false) {
  const bool from_pred = qa && qa->pred_in;
  R1_REQUIRE(ctx && org && (ref || from_pred));
  const R1Plane no_ref = {};
  if (from_pred) ref = &no_ref;
  R1_REQUIRE(from_pred || r1_same_px(*org, *ref));
  R1_REQUIRE(from_pred || r1_same_depth(*org, *ref));
  if (const int rc = rdo_plane_checks(org, w, h, tx_size); rc != R1_OK) return rc;
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands);
  hipStream_t st = (hipStream_t)stream;
  // the per-candidate tx_type selects the 1-D kernels on the device; the
  // shifts depend only on (tx_size, bit depth) for every non-WHT type and are
  // compile-time constants of the instantiation
  const int bd = org->bit_depth;
  R1_REQUIRE(r1_depth_ok(bd));
  const int qm = !qa ? 0 : (qa->pix_dist ? 2 : 1);
  typedef int (*SliceFn)(R1_SLICE_ARGS);
#define R1_RDO_SLICE_ENTRY(B, Q) r1_rdo_slice_b##B##_q##Q,
  static const SliceFn kSlices[3][5] = {{R1_RDO_SLICE_ROW(R1_RDO_SLICE_ENTRY, 8)},
                                        {R1_RDO_SLICE_ROW(R1_RDO_SLICE_ENTRY, 10)},
                                        {R1_RDO_SLICE_ROW(R1_RDO_SLICE_ENTRY, 12)}};
#undef R1_RDO_SLICE_ENTRY
  R1_REQUIRE(!mt || (qa && qa->tx_mask != 0 && qm != 0 && !coeffs));
  return kSlices[(bd - 8) / 2][mt ? qm + 2 : qm](tx_size, *org, *ref, cands, n, sad_out, satd_out, coeffs, pred_out,
                                                 qa, st);
}

// The RdoQuantArgs of a quantizing entry point, every argument check written once: the quantizer (QM 1 and 2),
// then the distortion -- dist_kind 0 = the transform-domain distortion (QM 1, no reconstruction), R1_DIST_WSSE /
// R1_DIST_CDEF = the pixel-domain leg (QM 2).  The scale grid and the decimation are checked for every kind.
int rdo_quant_args(const r1_ctx *ctx, const R1Plane *org, int tx_size, const R1QuantParams *params, int dist_kind,
                   const uint32_t *scales, int scale_stride, int xdec, int ydec, uint16_t *eob_out,
                   uint64_t *dist_out, void *qcoeffs_out, void *rec_out, RdoQuantArgs &qa) {
  R1_REQUIRE(ctx && org && params && eob_out && dist_out);
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(params->bit_depth == org->bit_depth);
  R1_REQUIRE(dist_kind == 0 || dist_kind == R1_DIST_WSSE || dist_kind == R1_DIST_CDEF);
  R1_REQUIRE(r1_dec_ok(xdec, ydec));
  R1_REQUIRE(dist_kind != R1_DIST_CDEF || (xdec == 0 && ydec == 0));   // cdef_dist is luma-only
  R1_REQUIRE(!scales || scale_stride > 0);
  R1_REQUIRE(dist_kind != 0 || !rec_out);
  qa.qp = r1q::make_qparams(*params, tx_size, org->bytes_per_px == 1 ? 2 : 4);
  for (int k = 0; k < 3; k++) qa.scan[k] = ctx->scan_dev + ctx->scan_off[tx_size][k];
  qa.tx_size = tx_size;
  qa.q_bin = params->qindex / 32;   // RDO_QUANT_DIV
  qa.eob = eob_out;
  qa.qcoeffs = qcoeffs_out;
  if (dist_kind == 0) {
    qa.tx_dist = (unsigned long long *)dist_out;
    return R1_OK;
  }
  qa.dist_kind = dist_kind;
  qa.inv_shift = r1itx::kInvShift[tx_size];
  qa.scales = scales;
  qa.scale_stride = scale_stride;
  qa.xdec = xdec;
  qa.ydec = ydec;
  qa.pix_dist = (unsigned long long *)dist_out;
  qa.rec = rec_out;
  return R1_OK;
}

// The transform-type mask of a type-search entry point (after rdo_quant_args: tx_size is in range), checked and
// written into the kernel's argument block: one result slot per set bit.
int rdo_type_mask_args(int tx_size, uint32_t tx_type_mask, int dist_kind, uint64_t *est_rate_out, RdoQuantArgs &qa) {
  R1_REQUIRE(dist_kind == 0 || !est_rate_out);
  // WHT (16) has no scan order; the mask is over the 16 TxTypes of the tx sets
  R1_REQUIRE(tx_type_mask != 0 && tx_type_mask <= 0xFFFFu);
  // a 64-point side codes DCT_DCT only (TX_SET_DCTONLY)
  R1_REQUIRE((r1tx::kTxWLog2[tx_size] <= 5 && r1tx::kTxHLog2[tx_size] <= 5) || tx_type_mask == 1u);
  // every type of the mask must exist for the size: the inter sets are the largest (av1_tx_used; a 32-point side has
  // DCT_DCT and IDTX only -- the reference's 1-D tables have no other kernel there and would panic)
  R1_REQUIRE((tx_type_mask & ~r1_tx_type_mask(tx_size, 1, 0, 0)) == 0);
  qa.est_rate = (unsigned long long *)est_rate_out;
  qa.tx_mask = tx_type_mask;
  qa.nt = __builtin_popcount(tx_type_mask);
  return R1_OK;
}

// The type search of a size that does not fan out (a 32- or 64-point side, at most two types): one plain launch per
// type, the type forced, results into its slot; the first launch also writes what no type changes (sad, satd, pred).
template <typename Launch>
int rdo_launch_per_type(RdoQuantArgs &qa, uint32_t tx_type_mask, Launch launch) {
  int slot = 0;
  for (uint32_t m = tx_type_mask; m != 0; m &= m - 1, slot++) {
    qa.tx_mask = m & (0u - m);
    qa.slot = slot;
    const int rc = launch(slot == 0);
    if (rc != R1_OK) return rc;
  }
  return R1_OK;
}
}  // namespace

extern "C" int r1_rdo_cand_batch(r1_ctx *ctx, const R1Plane *org,
                                 const R1Plane *ref, int w, int h, int tx_size,
                                 const R1RdoCand *cands, int n,
                                 uint32_t *sad_out, uint32_t *satd_out,
                                 void *coeffs, void *pred_out, void *stream) {
  return rdo_dispatch(ctx, org, ref, w, h, tx_size, cands, n, sad_out, satd_out, coeffs, pred_out,
                      nullptr, stream);
}

extern "C" int r1_rdo_full_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, int w,
                                      int h, int tx_size, const R1RdoCand *cands, int n,
                                      const R1QuantParams *params, uint32_t *sad_out,
                                      uint32_t *satd_out, uint16_t *eob_out,
                                      uint64_t *tx_dist_out, uint64_t *est_rate_out,
                                      void *qcoeffs_out, void *coeffs, void *stream) {
  RdoQuantArgs qa = {};
  // dist_kind 0: tx_dist_out takes the transform-domain distortion
  const int rc = rdo_quant_args(ctx, org, tx_size, params, 0, nullptr, 0, 0, 0, eob_out, tx_dist_out, qcoeffs_out,
                                nullptr, qa);
  if (rc != R1_OK) return rc;
  qa.est_rate = (unsigned long long *)est_rate_out;
  return rdo_dispatch(ctx, org, ref, w, h, tx_size, cands, n, sad_out, satd_out, coeffs, nullptr,
                      &qa, stream);
}

extern "C" int r1_rdo_pixel_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, int w,
                                       int h, int tx_size, const R1RdoCand *cands, int n,
                                       const R1QuantParams *params, int dist_kind,
                                       const uint32_t *scales, int scale_stride, int xdec, int ydec,
                                       uint32_t *sad_out, uint32_t *satd_out, uint16_t *eob_out,
                                       uint64_t *dist_out, void *qcoeffs_out, void *rec_out,
                                       void *stream) {
  R1_REQUIRE(dist_kind != 0);   // the pixel-domain leg only: kind 0 is r1_rdo_full_cand_batch
  RdoQuantArgs qa = {};
  const int rc = rdo_quant_args(ctx, org, tx_size, params, dist_kind, scales, scale_stride, xdec, ydec, eob_out,
                                dist_out, qcoeffs_out, rec_out, qa);
  if (rc != R1_OK) return rc;
  return rdo_dispatch(ctx, org, ref, w, h, tx_size, cands, n, sad_out, satd_out, nullptr, nullptr,
                      &qa, stream);
}

extern "C" int r1_rdo_pred_cand_batch(r1_ctx *ctx, const R1Plane *org, const void *pred, int w, int h,
                                      int tx_size, const R1RdoCand *cands, int n,
                                      const R1QuantParams *params, int dist_kind,
                                      const uint32_t *scales, int scale_stride, int xdec, int ydec,
                                      uint32_t *sad_out, uint32_t *satd_out, uint16_t *eob_out,
                                      uint64_t *dist_out, void *qcoeffs_out, void *rec_out,
                                      void *stream) {
  R1_REQUIRE(pred);
  RdoQuantArgs qa = {};
  const int rc = rdo_quant_args(ctx, org, tx_size, params, dist_kind, scales, scale_stride, xdec, ydec, eob_out,
                                dist_out, qcoeffs_out, rec_out, qa);
  if (rc != R1_OK) return rc;
  qa.pred_in = pred;
  return rdo_dispatch(ctx, org, nullptr, w, h, tx_size, cands, n, sad_out, satd_out, nullptr, nullptr,
                      &qa, stream);
}
// av1_tx_used[get_tx_set(tx_size, is_inter, use_reduced_set)] (src/context/transform_unit.rs:37-44,
// 123-148) as a bit mask over TxType, optionally cut down to RAV1E_TX_TYPES (src/transform/mod.rs:28-44):
// the types the loop of rdo_tx_type_decision (src/rdo.rs:1732-1736) does not skip.
extern "C" uint32_t r1_tx_type_mask(int tx_size, int is_inter, int use_reduced_set, int rav1e_types_only) {
  if (!r1_tx_size_ok(tx_size)) return 0;
  const uint32_t m = r1tx::kTxUsed[r1_tx_set(tx_size, is_inter, use_reduced_set)];
  return rav1e_types_only ? (m & 0x0E0Fu) : m;
}

extern "C" int r1_rdo_txsearch_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, const void *pred,
                                     int w, int h, int tx_size, const R1RdoCand *cands, int n,
                                     uint32_t tx_type_mask, const R1QuantParams *params, int dist_kind,
                                     const uint32_t *scales, int scale_stride, int xdec, int ydec,
                                     uint32_t *sad_out, uint32_t *satd_out, uint16_t *eob_out,
                                     uint64_t *dist_out, uint64_t *est_rate_out, void *qcoeffs_out,
                                     void *rec_out, void *stream) {
  R1_REQUIRE((ref != nullptr) != (pred != nullptr));
  RdoQuantArgs qa = {};
  int rc = rdo_quant_args(ctx, org, tx_size, params, dist_kind, scales, scale_stride, xdec, ydec, eob_out, dist_out,
                          qcoeffs_out, rec_out, qa);
  if (rc != R1_OK) return rc;
  rc = rdo_type_mask_args(tx_size, tx_type_mask, dist_kind, est_rate_out, qa);
  if (rc != R1_OK) return rc;
  qa.pred_in = pred;
  if (rdo_type_fanout(r1tx::kTxWLog2[tx_size], r1tx::kTxHLog2[tx_size]))
    return rdo_dispatch(ctx, org, ref, w, h, tx_size, cands, n, sad_out, satd_out, nullptr, nullptr, &qa, stream, true);
  return rdo_launch_per_type(qa, tx_type_mask, [&](bool first) {
    return rdo_dispatch(ctx, org, ref, w, h, tx_size, cands, n, first ? sad_out : nullptr, first ? satd_out : nullptr,
                        nullptr, nullptr, &qa, stream, false);
  });
}

// ---- the intra candidate in one launch: the prediction is made inside the chain (k_rdo_cand with PS = 1) ----
extern "C" int r1_rdo_intra_cand_batch(r1_ctx *ctx, const R1Plane *org, int w, int h, int tx_size,
                                       const R1IntraCand *cands, int n, int edge_group, const int16_t *pos_xy,
                                       const void *edges, int edge_stride, const uint8_t *lens, const int16_t *ac,
                                       uint32_t tx_type_mask, const R1QuantParams *params, int dist_kind,
                                       const uint32_t *scales, int scale_stride, int xdec, int ydec,
                                       uint32_t *sad_out, uint32_t *satd_out, uint16_t *eob_out, uint64_t *dist_out,
                                       uint64_t *est_rate_out, void *qcoeffs_out, void *rec_out, void *pred_out,
                                       void *stream) {
  RdoQuantArgs qa = {};
  int rc = rdo_quant_args(ctx, org, tx_size, params, dist_kind, scales, scale_stride, xdec, ydec, eob_out, dist_out,
                          qcoeffs_out, rec_out, qa);
  if (rc != R1_OK) return rc;
  rc = rdo_type_mask_args(tx_size, tx_type_mask, dist_kind, est_rate_out, qa);
  if (rc != R1_OK) return rc;
  rc = rdo_plane_checks(org, w, h, tx_size);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(r1_depth_ok(org->bit_depth));
  // the intra source
  R1_REQUIRE(edge_stride >= R1_INTRA_EDGE_LEN && edge_group >= 1);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(n % edge_group == 0);
  R1_REQUIRE(cands && edges && lens && pos_xy);
  if (!ac) {
    // UV_CFL_PRED needs its AC block.  The descriptors are the caller's memory: where the host can read them
    // (ordinary or pinned host memory) they are checked here; descriptors in device memory cannot be seen without
    // a synchronising copy, and there the kernel predicts such a candidate's DC without touching `ac`.
    hipPointerAttribute_t at = {};
    const hipError_t e = hipPointerGetAttributes(&at, cands);
    // an unregistered pointer is hipErrorInvalidValue to older runtimes, and without a device nothing is device
    // memory; after any other failure the descriptors are left alone
    int ndev = 0;
    const bool host_readable =
        e == hipSuccess ? at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeHost
                        : e == hipErrorInvalidValue || hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0;
    (void)hipGetLastError();
    if (host_readable)
      for (int i = 0; i < n; i++) R1_REQUIRE(cands[i].mode != 13);
  }
  RdoIntraArgs ia = {cands, edges, lens, pos_xy, ac, edge_stride, edge_group};
  typedef int (*ISliceFn)(R1_INTRA_SLICE_ARGS);
#define R1_RDO_ISLICE_ENTRY(B, Q) r1_rdo_islice_b##B##_q##Q,
  static const ISliceFn kISlices[3][4] = {{R1_RDO_ISLICE_ROW(R1_RDO_ISLICE_ENTRY, 8)},
                                          {R1_RDO_ISLICE_ROW(R1_RDO_ISLICE_ENTRY, 10)},
                                          {R1_RDO_ISLICE_ROW(R1_RDO_ISLICE_ENTRY, 12)}};
#undef R1_RDO_ISLICE_ENTRY
  const ISliceFn *row = kISlices[(org->bit_depth - 8) / 2];
  const int qm = dist_kind == 0 ? 1 : 2;
  hipStream_t st = (hipStream_t)stream;
  const RdoIntraRoute route = rdo_intra_route(r1tx::kTxWLog2[tx_size], r1tx::kTxHLog2[tx_size], org->bit_depth, qm);
  if (route == RDO_INTRA_TWO_LAUNCH) {
    // predict to pred_out (or to the ring) and run the existing kernels on it: same slots, same results
    R1DeviceGuard guard(ctx);
    const size_t cand_bytes = ((size_t)n * sizeof(R1RdoCand) + 255) & ~(size_t)255;
    const size_t need = cand_bytes + (pred_out ? 0 : (size_t)n * w * h * org->bytes_per_px);
    void *scratch;
    rc = ctx->intra_ring.acquire(need, &scratch);
    if (rc != R1_OK) return rc;
    R1RdoCand *rc_dev = (R1RdoCand *)scratch;
    void *pred = pred_out ? pred_out : (void *)((uint8_t *)scratch + cand_bytes);
    rc = r1_predict_intra_route_launch(tx_size, cands, n, edges, edge_stride, lens, edge_group, pos_xy, rc_dev, ac,
                                       org->bit_depth, org->bytes_per_px, pred, st);
    if (rc == R1_OK)
      rc = r1_rdo_txsearch_batch(ctx, org, nullptr, pred, w, h, tx_size, rc_dev, n, tx_type_mask, params, dist_kind,
                                 scales, scale_stride, xdec, ydec, sad_out, satd_out, eob_out, dist_out, est_rate_out,
                                 qcoeffs_out, rec_out, stream);
    const int rel = ctx->intra_ring.release(st);
    return rel != R1_OK ? rel : rc;
  }
  if (route == RDO_INTRA_FANOUT)   // slices 3 / 4
    return row[qm + 1](tx_size, *org, n, sad_out, satd_out, pred_out, &qa, &ia, st);
  // each launch makes the prediction again on the CU, the first one writes sad / satd / pred_out
  return rdo_launch_per_type(qa, tx_type_mask, [&](bool first) {
    return row[qm - 1](tx_size, *org, n, first ? sad_out : nullptr, first ? satd_out : nullptr,
                       first ? pred_out : nullptr, &qa, &ia, st);
  });
}

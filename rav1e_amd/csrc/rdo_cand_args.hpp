// rdo_cand_args.hpp -- what the slices of the fused candidate kernel (rdo_cand_slice.hip: the kernel of
// rdo_cand_kernel.hpp, one (bit depth, slice) each) and the host unit (rdo_cand.hip: argument checks, dispatch,
// entry points) share: the kernel's quantizer argument block, the slice signature and the list of slices.  Which
// instantiations a slice holds and which route a call takes: rdo_cand_plan.hpp.
#pragma once
#include "quant_common.hpp"
#include "rdo_cand_plan.hpp"

// QUANT (the "full" candidate): the coefficients do not go to HBM
// (unless `coeffs` is also given) but through the quantizer in place --
// quantize + dequantize + transform-domain distortion + estimate_rate, i.e.
// encode_tx_block's RDOType::TxDistEstRate evaluation (src/encoder.rs:1533-1650)
// -- and only (eob, distortion, rate) leave the CU.
struct RdoQuantArgs {
  r1q::QParams qp;
  const uint16_t *scan[3];   // av1_scan_orders[tx_size]: default / mrow / mcol
  int tx_size, q_bin;
  uint16_t *eob;
  unsigned long long *tx_dist, *est_rate;
  void *qcoeffs;             // optional: dense coded-area blocks
  // QM == 2 (pixel-domain leg): dequantize -> inverse transform -> reconstruct ->
  // sse_wxh / cdef_dist_wxh against the source with the DistortionScale grid
  // (encode_tx_block with need_recon_pixel / compute_distortion, src/rdo.rs:254-340)
  int dist_kind, inv_shift;
  const uint32_t *scales;
  int scale_stride, xdec, ydec;
  unsigned long long *pix_dist;
  void *rec;                 // optional: dense w*h reconstructions
  // prediction from a dense buffer (n x h x w pixels: intra predictions, compound
  // averages) instead of put_8tap of the reference plane
  const void *pred_in;
  // MT (transform-type search fan-out, rdo_tx_type_decision src/rdo.rs:1701-1817): every candidate is
  // carried through the chain once per set bit of tx_mask (bit t = TxType t, ascending), on ONE
  // prediction / residual; result slot of (candidate i, j-th set bit) = i * nt + j, nt = popcount
  uint32_t tx_mask;
  int nt;
  // plain (non-MT) kernels: tx_mask != 0 forces the type of every candidate to its lowest set bit and the
  // results go to slot `slot` of nt (sizes with a 32-point side: one launch per type, see r1_rdo_txsearch_batch)
  int slot;
};

// The intra prediction source (k_rdo_cand with PS = 1, r1_rdo_intra_cand_batch): candidate i predicts from edge set
// i / edge_group (`edges`: edge_stride pixels each, `lens`: init_left / init_above pairs, as r1_intra_edges_batch
// leaves them) at the block position pos_xy[2 (i / edge_group)], +1 in the source plane; ac: dense w*h int16 per
// candidate (UV_CFL_PRED) or NULL.
struct RdoIntraArgs {
  const R1IntraCand *cands;
  const void *edges;
  const uint8_t *lens;
  const int16_t *pos_xy;
  const int16_t *ac;
  int edge_stride, edge_group;
};
struct RdoNoIntraArgs {};   // what the PS = 0 instantiations take in its place

#define R1_SLICE_ARGS                                                                         \
  int tx_size, const R1Plane &org, const R1Plane &ref, const R1RdoCand *cands, int n,         \
      uint32_t *sad, uint32_t *satd, void *coeffs, void *pred, const RdoQuantArgs *qa, hipStream_t st
// The slices, written once: X(bit depth, slice).  Slice numbers 0..2 = QM; 3 / 4 = the type-search (MT)
// instantiations of QM 1 / 2.  One object (rdo_cand_b<B>_q<Q>.o) and one function r1_rdo_slice_b<B>_q<Q> each.
#define R1_RDO_SLICE_ROW(X, B) X(B, 0) X(B, 1) X(B, 2) X(B, 3) X(B, 4)
#define R1_RDO_SLICES(X) R1_RDO_SLICE_ROW(X, 8) R1_RDO_SLICE_ROW(X, 10) R1_RDO_SLICE_ROW(X, 12)
#define R1_RDO_SLICE_DECL(B, Q) int r1_rdo_slice_b##B##_q##Q(R1_SLICE_ARGS);
R1_RDO_SLICES(R1_RDO_SLICE_DECL)
#undef R1_RDO_SLICE_DECL
// The intra slices (PS = 1): X(bit depth, slice), slices 1 / 2 = the plain form of QM 1 / 2 (the ten sizes with a
// 32- or 64-point side), 3 / 4 = the fan-out form (the nine sizes up to 16 x 16).  One object
// (rdo_cand_i_b<B>_q<Q>.o) and one function r1_rdo_islice_b<B>_q<Q> each, from the same rdo_cand_slice.hip.
#define R1_INTRA_SLICE_ARGS                                                                               \
  int tx_size, const R1Plane &org, int n, uint32_t *sad, uint32_t *satd, void *pred, const RdoQuantArgs *qa, \
      const RdoIntraArgs *ia, hipStream_t st
#define R1_RDO_ISLICE_ROW(X, B) X(B, 1) X(B, 2) X(B, 3) X(B, 4)
#define R1_RDO_ISLICES(X) R1_RDO_ISLICE_ROW(X, 8) R1_RDO_ISLICE_ROW(X, 10) R1_RDO_ISLICE_ROW(X, 12)
#define R1_RDO_ISLICE_DECL(B, Q) int r1_rdo_islice_b##B##_q##Q(R1_INTRA_SLICE_ARGS);
R1_RDO_ISLICES(R1_RDO_ISLICE_DECL)
#undef R1_RDO_ISLICE_DECL

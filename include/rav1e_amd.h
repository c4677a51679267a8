/*
 * rav1e_amd.h -- C ABI of librav1e_hip.so, the MI355X (gfx950) block-kernel
 * backend for rav1e's per-block RDO inner loop.
 *
 * This is the drop-in boundary: exactly what a new `CpuFeatureLevel::HIP`
 * row of rav1e's `src/asm` dispatch tables would bind over FFI
 * (reference dispatch surface: src/cpu_features/x86.rs:97-158; per-family
 * tables cited at each entry point below).  Two layers:
 *
 *  (1) BATCH API (the product).  The reference calls its kernels one block at
 *      a time (src/me.rs:1445-1454, src/rdo.rs:1328-1352, src/encoder.rs:
 *      1404-1661); a GPU wants thousands of independent candidates per
 *      launch, so the host enqueues descriptor arrays and flushes.  All
 *      pointers are DEVICE pointers unless stated; the caller owns every
 *      buffer; nothing is retained after a call returns; calls are
 *      asynchronous on `stream` (a hipStream_t passed as void*, NULL = the
 *      default stream).  Return value: 0 ok, negative R1_E* on error; results
 *      are undefined on error.  Thread-safe: no global mutable state (the one
 *      per-context resource, the job-descriptor ring of the tile ME, is
 *      serialised internally).
 *
 *  (2) PER-CALL COMPAT SHIMS with the reference's exact asm signatures
 *      (host pointers, byte strides, values returned directly).  They stage,
 *      launch and synchronise -- for plumbing / `check_asm`-style parity
 *      only, never fast.
 *
 * Enum integer values are the reference's (they index its dispatch tables):
 *   BlockSize  src/partition.rs:130-153      TxSize  src/transform/mod.rs:101-123
 *   TxType     src/transform/mod.rs:56-74    FilterMode  src/mc.rs:100-106
 */
#ifndef RAV1E_AMD_H
#define RAV1E_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R1_OK 0
#define R1_EINVAL (-1)   /* bad argument / descriptor (reference: assert! panic) */
#define R1_EHIP (-2)     /* HIP runtime error; see r1_last_error() */
#define R1_ECOMM (-3)    /* RCCL error (or no RCCL library to load); see r1_last_error() */
#define R1_ENOMEM (-4)
#define R1_ETIMEDOUT (-5) /* r1_me_status: a persistent tile-ME launch flagged a timed-out dependency wait */

/* ---- Plane<T> view (v_frame 0.3.9 PlaneConfig layout; reference use:
 * src/tiling/plane_region.rs:185 -- element (x,y) lives at
 * data[(yorigin + y) * stride + xorigin + x]).  `data` is a device pointer to
 * the start of the allocation; stride is in ELEMENTS.  No alignment beyond the
 * element's own (1 or 2 bytes) is required of `data`, `stride` or `xorigin`, and
 * the planes of one call may differ in all of them. */
typedef struct R1Plane {
  void *data;
  int32_t stride;
  int32_t alloc_height;
  int32_t width, height;     /* visible size */
  int32_t xorigin, yorigin;  /* padding left / above pixel (0,0) */
  int32_t bytes_per_px;      /* 1 (Pixel = u8) or 2 (Pixel = u16) */
  int32_t bit_depth;         /* 8, 10 or 12 */
} R1Plane;

/* rav1e FilterMode (src/mc.rs:100-106) */
enum { R1_FILTER_REGULAR = 0, R1_FILTER_SMOOTH = 1, R1_FILTER_SHARP = 2,
       R1_FILTER_BILINEAR = 3 };

/* distortion kinds of r1_dist_batch */
enum { R1_DIST_SAD = 0, R1_DIST_SATD = 1,
       /* r1_dist_scaled_batch: */ R1_DIST_WSSE = 2, R1_DIST_CDEF = 3 };

/* One distortion candidate: block of the launch's (w,h) at (ox,oy) in the
 * org plane against (rx,ry) in the ref plane (full-pel, plane coordinates;
 * may lie in the padding as the reference's MV clamp allows,
 * src/me.rs:339-362). */
typedef struct R1DistCand {
  int16_t ox, oy, rx, ry;
} R1DistCand;

/* One motion-compensation candidate: full-pel position of the block in the
 * ref plane plus 1/16-pel fractions, i.e. the outputs of get_mv_params
 * (src/predict.rs:284-297). */
typedef struct R1McCand {
  int16_t rx, ry;
  uint8_t col_frac, row_frac; /* 0..15 */
  uint8_t mode_x, mode_y;     /* FilterMode */
} R1McCand;

/* One fused RDO candidate (mc -> dist -> diff -> forward transform). */
typedef struct R1RdoCand {
  int16_t ox, oy;             /* block position in the org (source) plane */
  int16_t rx, ry;             /* full-pel position in the ref plane */
  uint8_t col_frac, row_frac; /* 0..15 */
  uint8_t mode_x, mode_y;     /* FilterMode */
  uint8_t tx_type;            /* TxType for the residual transform */
  uint8_t reserved[3];
} R1RdoCand;

typedef struct r1_ctx r1_ctx;

/* ---- context ---- */
int r1_ctx_create(int device, r1_ctx **out);
void r1_ctx_destroy(r1_ctx *ctx);
const char *r1_last_error(void);
/* ABI version, bumped on any incompatible change.
 * 4 (round 4): r1_estimate_tile_motion_batch refuses with R1_ETIMEDOUT while a flagged persistent launch
 *    has not been acknowledged through r1_me_status; r1_cdef_filter_frame_plane checks luma->bit_depth
 *    against params->bit_depth and the _dirs variant wants 8-aligned tile_w / tile_h; skip_mi bytes are
 *    bools (any non-zero value) in the CDEF filter and the strength search alike.
 * 5 (round 5): + r1_rdo_txsearch_batch, r1_tx_type_mask (additions only; nothing of 4 changed).
 * 6 (round 5): R1SgrSolveUnit.reserved[0] became `edges` (R1_SGR_EDGE_*): what r1_sgrproj_solve_batch /
 *    r1_lrf_search_batch see left of / above a unit is the caller's statement of the unit's place in its
 *    rdo_loop_decision area, no longer the unit's place in the frame (0 = nothing, the case of one unit per
 *    plane and area); the restoration entry points refuse planes of 4 GiB and more.  MIGRATION from 5: a
 *    caller that left reserved = 0 keeps its results only where a plane has ONE unit per area; with several
 *    units per area (64-pixel luma units under 128-pixel chroma units, qindex > 160) it must now set `edges`
 *     -- 0 means "the unit alone", no longer "as the unit lies in the frame".
 * 7 (round 6): + r1_cdef_lrf_trial_batch, r1_cdef_lrf_trial_scratch_bytes, r1_cdef_apply_area, R1TrialUnit,
 *    r1_comm_plane_pool_open / _close (additions only; nothing of 6 changed).
 * Additions never changed an existing signature: the peer-store entry points (r1_comm_push_*, round 4) and
 * r1_comm_push_frame (round 5) were added under versions 4 and 5 respectively, and the compound candidate
 * (r1_rdo_compound_cand_batch, R1CompoundCand) under version 7, as were the frame's scale maps and segmentation
 * inputs (r1_frame_scales, r1_scale_kmeans, r1_segmentation_from_centroids, r1_spatiotemporal_scale_batch) and the
 * intra candidate (r1_rdo_intra_cand_batch), the coefficient rate (r1_coeff_rate_batch, R1CoeffCdfs, R1TxbCtx), the
 * intra transform-split candidate (r1_rdo_intra_split_batch, R1IntraSplitCand), the coefficient rate across a
 * block's transform blocks (r1_coeff_rate_chain_batch, R1TxbChainCtx) and across its three planes on one writer
 * (r1_coeff_rate_block_batch, R1BlockChainCtx, R1BlockRateTrial), and the decision on the device (r1_rd_pick_batch,
 * r1_rd_commit_batch, R1RdPick), and the device-resident coefficient CDF context (r1_coeff_cdf_slice_batch,
 * r1_coeff_cdf_adapt_batch, R1CoeffCdfContext), and the device-resident coefficient neighbour contexts with the
 * winner's transform type (r1_coeff_nbr_gather_batch, r1_coeff_nbr_store_batch, r1_coeff_nbr_reset_left_batch,
 * r1_rd_winner_tx_type_batch, R1CoeffNbrContext, R1NbrBlock), and the partition decision on the device
 * (r1_rd_partition_pick_batch, r1_part_select_batch, r1_part_select_rect_batch, R1PartPick). */
int r1_abi_version(void);

/* ---- dist:: (reference: src/dist.rs get_sad 31, get_satd 156; dispatch
 * tables SAD_FNS/SATD_FNS/_HBD src/asm/x86/dist/mod.rs:483-729).
 * out[i] = get_sad/get_satd(org@cand[i], ref@cand[i], w, h).  w,h <= 128 and
 * multiples of 4 (SATD uses 4x4 Hadamards when min(w,h)==4 else 8x8). */
int r1_dist_batch(r1_ctx *ctx, int kind, const R1Plane *org,
                  const R1Plane *ref, int w, int h, const R1DistCand *cands,
                  int n, uint32_t *out, void *stream);

/* ---- candidate-level pixel-domain distortion with the DistortionScale bias
 * (reference: sse_wxh src/rdo.rs:177-224 -> get_weighted_sse src/dist.rs:234-283
 * [kind R1_DIST_WSSE]; cdef_dist_wxh src/rdo.rs:142-173 -> cdef_dist_kernel
 * src/dist.rs:302-372 + apply_ssim_boost src/activity.rs:159-186
 * [kind R1_DIST_CDEF]; x86 tables src/asm/x86/dist/{sse,cdef_dist}.rs).
 * scales: the frame's distortion_scales grid (src/rdo.rs:443-459), one Q14
 * u32 per 8x8 LUMA importance block, entry [(luma_y >> 3) * scale_stride +
 * (luma_x >> 3)] where luma_xy = (plane_xy << dec) of each 4x4 cell (WSSE) or
 * 8x8 kernel (CDEF) -- exactly what the compute_bias closure at
 * src/rdo.rs:283-303 looks up.  NULL = DistortionScale::default() (1 << 14).
 * out[i] = the reference's Distortion (u64), before `* fi.dist_scale[p]`.
 * w, h <= 128: the visible block size after frame clipping (clip_visible_bsize, src/rdo.rs:228-251),
 * any size >= 1.  R1_DIST_CDEF: the last kernel of a row / column is kernel_w x kernel_h < 8x8.
 * R1_DIST_WSSE: -- like get_weighted_sse, only whole 4x4 cells are measured (a
 * clipped chroma block may be 2 wide: its distortion is 0, as in the reference). */
int r1_dist_scaled_batch(r1_ctx *ctx, int kind, const R1Plane *org,
                         const R1Plane *ref, int w, int h,
                         const R1DistCand *cands, int n, const uint32_t *scales,
                         int scale_stride, int xdec, int ydec, uint64_t *out,
                         void *stream);

/* ---- transform::forward (reference: src/transform/forward.rs:71-161;
 * x86 entry src/asm/x86/transform/forward.rs:444-447).
 * residual: n dense blocks of w*h int16 (row-major, stride = tx width, the
 * only call site's layout, src/encoder.rs:1544-1552).
 * coeffs: n dense blocks of w*h coefficients in the reference's transposed,
 * 32x32-chunked order; int16 when coeff_bytes == 2 (Pixel = u8) or int32
 * when 4 (Pixel = u16).  Invalid (tx_size, tx_type) -> R1_EINVAL. */
int r1_fwd_txfm_batch(r1_ctx *ctx, const int16_t *residual, void *coeffs,
                      int n, int tx_size, int tx_type, int bit_depth,
                      int coeff_bytes, void *stream);

/* ---- transform::inverse (reference: inverse_transform_add,
 * src/transform/inverse.rs:1633-1705; InvTxfmFunc tables
 * src/asm/x86/transform/inverse.rs, wrapper src/asm/shared/transform/inverse.rs:30-36).
 * coeffs: block i at coeffs + i*coeff_stride (elements); only the first
 * min(w,32)*min(h,32) entries are read, in the forward transform's transposed
 * order (so the output of r1_fwd_txfm_batch / r1_quantize_batch's rcoeffs can
 * be passed unchanged).  int16 when bytes_per_px == 1, int32 when 2
 * (T::Coeff).  pred / rec: n dense w*h pixel blocks; rec may alias pred (the
 * reference adds in place). */
int r1_inv_txfm_add_batch(r1_ctx *ctx, const void *coeffs, int coeff_stride,
                          const void *pred, void *rec, int n, int tx_size,
                          int tx_type, int bit_depth, int bytes_per_px,
                          void *stream);

/* ---- quantize:: (reference: QuantizationContext::{update,quantize}
 * src/quantize/mod.rs:219-355, dequantize 363-384 with its dispatch
 * src/asm/x86/quantize.rs; scan orders src/scan_order.rs). */
typedef struct R1QuantParams {
  uint8_t qindex;       /* base_q_idx of the block */
  uint8_t bit_depth;    /* 8, 10, 12 */
  uint8_t is_intra;     /* selects the rounding biases (mod.rs:258-265) */
  int8_t dc_delta_q, ac_delta_q;
  uint8_t reserved[3];
} R1QuantParams;
/* block i reads coeffs + i*coeff_stride (>= coded area entries, the layout
 * r1_fwd_txfm_batch writes); qcoeffs / rcoeffs: dense coded-area blocks
 * (min(w,32)*min(h,32)), fully written (zeros beyond eob); eobs[i] = the
 * reference's return value.  rcoeffs may be NULL (no fused dequantize).
 * coeff_bytes 2 (T::Coeff = i16) or 4 (i32).  tx_type 16 (WHT) -> R1_EINVAL
 * (the reference's scan table has 16 columns). */
int r1_quantize_batch(r1_ctx *ctx, const void *coeffs, int coeff_stride, int n,
                      int tx_size, int tx_type, const R1QuantParams *params,
                      int coeff_bytes, void *qcoeffs, uint16_t *eobs,
                      void *rcoeffs, void *stream);
/* The RDO form of the same call (SURVEY.md 8f "N4", first step): additionally the
 * transform-domain distortion of encode_tx_block (src/encoder.rs:1616-1640;
 * coeffs must then hold the full w*h forward-transform output, coeff_stride >=
 * w*h) and, when est_rate is non-NULL, estimate_rate(qindex, tx_size, tx_dist)
 * from RDO_RATE_TABLE (src/rdo.rs:127-139) -- what RDOType::TxDistEstRate
 * uses to rank transform candidates without the entropy coder. */
int r1_quantize_rdo_batch(r1_ctx *ctx, const void *coeffs, int coeff_stride, int n,
                          int tx_size, int tx_type, const R1QuantParams *params,
                          int coeff_bytes, void *qcoeffs, uint16_t *eobs,
                          void *rcoeffs, uint64_t *tx_dist, uint64_t *est_rate,
                          void *stream);
int r1_dequantize_batch(r1_ctx *ctx, const void *qcoeffs, int n, int tx_size,
                        const R1QuantParams *params, int coeff_bytes,
                        void *rcoeffs, void *stream);

/* ---- mc:: (reference: src/mc.rs put_8tap 250, prep_8tap 360, mc_avg 454;
 * dispatch tables PUT_FNS/PREP_FNS/AVG_FNS src/asm/x86/mc.rs:17-78,371-382).
 * put: dst = n dense w*h pixel blocks (same pixel type as `ref`).
 * prep: tmp = n dense w*h int16 blocks.  avg: dst from two prep outputs.
 * w power of two in 2..128 (this ABI: >= 4), h even. */
int r1_mc_put_batch(r1_ctx *ctx, const R1Plane *ref, int w, int h,
                    const R1McCand *cands, int n, void *dst, void *stream);
int r1_mc_prep_batch(r1_ctx *ctx, const R1Plane *ref, int w, int h,
                     const R1McCand *cands, int n, int16_t *tmp, void *stream);
int r1_mc_avg_batch(r1_ctx *ctx, const int16_t *tmp1, const int16_t *tmp2,
                    int w, int h, int n, int bit_depth, int bytes_per_px,
                    void *dst, void *stream);
/* The same put_8tap / prep_8tap (prep != 0) with the horizontal 8-tap pass on the matrix
 * cores (banded-Toeplitz v_mfma_i32_16x16x32_i8; csrc/mc_mfma.hip): 8-bit planes, square
 * blocks 8 / 16 / 32 / 64.  Bit-identical to r1_mc_put_batch / r1_mc_prep_batch; kept as a
 * separate entry point so that both formulations can be timed side by side
 * (tools/bench_mc_mfma.py).  Other sizes / bit depths: R1_EINVAL. */
int r1_mc_batch_mfma(r1_ctx *ctx, int prep, const R1Plane *ref, int w, int h,
                     const R1McCand *cands, int n, void *dst, void *stream);

/* ---- predict:: (reference: get_intra_edges src/partition.rs:639-898,
 * PredictionMode::predict_intra src/predict.rs:205-249, dispatch_predict_intra
 * 705-784 with its kernels 786-1505, pred_cfl_ac 1020-1063; x86 dispatch
 * src/asm/x86/predict.rs).  PredictionMode values 0..13 are the reference's
 * (src/predict.rs:75-89). */
#define R1_INTRA_EDGE_LEN 257  /* IntraEdgeBuffer: 4 * MAX_TX_SIZE + 1 (partition.rs:600) */

/* Inputs of get_intra_edges for one transform block.  (x, y): position
 * relative to the tile (`po`).  flags: bit0 enable_intra_edge_filter, bit1 =
 * has_top_right(..), bit2 = has_bottom_left(..) -- those two are decisions on
 * the partition tree (encoder state, src/partition.rs:400-560) and stay on
 * the host.  mode < 0 = None (every edge is needed). */
typedef struct R1IntraEdgeCand {
  int16_t x, y;
  int8_t mode;
  int8_t angle_delta;   /* IntraParam::AngleDelta, else 0 */
  uint8_t flags;
  uint8_t reserved;
} R1IntraEdgeCand;
/* edges: n buffers of `edge_stride` (>= 257) pixels in the reference's layout:
 * left right-aligned ending at index 128 (bottom -> top), top-left at 128,
 * above from 129.  lens[2i], lens[2i+1] = init_left, init_above of
 * IntraEdge::new.  Tile = (tile_x, tile_y, tile_w, tile_h) in plane pixels. */
int r1_intra_edges_batch(r1_ctx *ctx, const R1Plane *rec, int tile_x, int tile_y,
                         int tile_w, int tile_h, int tx_size,
                         const R1IntraEdgeCand *cands, int n, void *edges,
                         int edge_stride, uint8_t *lens, void *stream);

/* Arguments of dispatch_predict_intra for one block (after predict_intra's
 * PAETH / CFL remaps, which depend only on the block position). */
typedef struct R1IntraCand {
  uint8_t mode;        /* PredictionMode 0..13 */
  uint8_t variant;     /* PredictionVariant: 0 NONE, 1 LEFT, 2 TOP, 3 BOTH */
  int16_t angle;       /* p_angle; alpha for UV_CFL_PRED */
  uint8_t ief;         /* ief_params: 0 None, 1 Some(no smooth neighbour), 2 Some(smooth) */
  uint8_t avail_w;     /* min(tx width, plane width - block x)  (predict.rs:1346) */
  uint8_t avail_h;     /* min(tx height, plane height - block y) */
  uint8_t reserved;
} R1IntraCand;
/* dst: n dense w*h pixel blocks.  ac: n dense w*h int16 (CFL only, else NULL). */
int r1_predict_intra_batch(r1_ctx *ctx, int tx_size, const R1IntraCand *cands, int n,
                           const void *edges, int edge_stride, const uint8_t *lens,
                           const int16_t *ac, int bit_depth, int bytes_per_px,
                           void *dst, void *stream);

/* pred_cfl_ac: (x, y) = luma position of the block in plane pixels; bw x bh =
 * chroma block size; w_pad / h_pad in 4-pixel units (luma_ac, predict.rs:667-702). */
typedef struct R1CflAcCand {
  int16_t x, y;
  uint8_t w_pad, h_pad;
  uint8_t reserved[2];
} R1CflAcCand;
int r1_cfl_ac_batch(r1_ctx *ctx, const R1Plane *luma, int bw, int bh, int xdec,
                    int ydec, const R1CflAcCand *cands, int n, int16_t *ac,
                    void *stream);

/* rdo_cfl_alpha (src/rdo.rs:1593-1688) for ONE chroma plane: the alpha in
 * -16 .. 16 minimising the SSE of UV_CFL_PRED against the source over the
 * visible part of the block, with the reference's search order and early exit.
 * (x, y): block position in `src` (the chroma INPUT plane); variant: the
 * PredictionVariant of the DC average (0 NONE, 1 LEFT, 2 TOP, 3 BOTH); vis_w /
 * vis_h: clip_visible_bsize.  edges / lens: r1_intra_edges_batch of the
 * reconstructed chroma plane (mode UV_CFL_PRED), ac: r1_cfl_ac_batch, one
 * entry per candidate.  alpha_out: int16 per candidate; cost_out (optional):
 * its SSE. */
typedef struct R1CflAlphaCand {
  int16_t x, y;
  uint8_t variant, vis_w, vis_h, reserved;
} R1CflAlphaCand;
int r1_cfl_alpha_search_batch(r1_ctx *ctx, const R1Plane *src, int tx_size,
                              const R1CflAlphaCand *cands, int n, const void *edges,
                              int edge_stride, const uint8_t *lens, const int16_t *ac,
                              int16_t *alpha_out, uint64_t *cost_out, void *stream);

/* ---- cdef:: (reference: cdef_find_dir src/cdef.rs:84-143, cdef_filter_block
 * 198-298, cdef_filter_superblock / cdef_filter_tile 405-625; x86 dispatch
 * src/asm/x86/cdef.rs:83-110).  Edge flags = the reference's CDEF_HAVE_*. */
enum { R1_CDEF_HAVE_LEFT = 1, R1_CDEF_HAVE_RIGHT = 2, R1_CDEF_HAVE_TOP = 4,
       R1_CDEF_HAVE_BOTTOM = 8, R1_CDEF_HAVE_ALL = 15 };
typedef struct R1CdefDirCand { int16_t x, y; } R1CdefDirCand;   /* 8x8 luma block, plane px */
int r1_cdef_find_dir_batch(r1_ctx *ctx, const R1Plane *luma, const R1CdefDirCand *cands,
                           int n, uint8_t *dir_out, int32_t *var_out, void *stream);
/* One cdef_filter_block call: block at (x, y) of plane `in` (size (8>>xdec) x
 * (8>>ydec)), written to the same position of `out` (a different plane). */
typedef struct R1CdefBlockCand {
  int16_t x, y;
  int16_t pri_strength, sec_strength;  /* already shifted / adjusted, as passed to the asm */
  uint8_t dir, damping, edges, reserved;
} R1CdefBlockCand;
int r1_cdef_filter_block_batch(r1_ctx *ctx, const R1Plane *in, const R1Plane *out,
                               int xdec, int ydec, const R1CdefBlockCand *cands, int n,
                               void *stream);
/* cdef_filter_tile for plane p of the whole frame (the reference's only call,
 * src/encoder.rs:3301-3321): skip test over the four 4x4 blocks of every 8x8,
 * direction search on luma, adjust_strength, chroma direction map, edge
 * flags, filter or copy.  skip_mi: Block::skip per 4x4 luma unit (TileBlocks), a bool per byte
 * (any non-zero value = skipped; the strength search reads it the same way);
 * cdef_index_sb: per 64x64 superblock; params = the FrameInvariants fields
 * cdef_filter_superblock reads.  luma->bit_depth must equal params->bit_depth (R1_EINVAL). */
typedef struct R1CdefParams {
  uint8_t y_strengths[8], uv_strengths[8];   /* fi.cdef_y_strengths / cdef_uv_strengths */
  uint8_t damping;                           /* fi.cdef_damping */
  uint8_t bit_depth;
  uint8_t reserved[2];
} R1CdefParams;
int r1_cdef_filter_frame_plane(r1_ctx *ctx, const R1Plane *luma, const R1Plane *in,
                               const R1Plane *out, int p, int xdec, int ydec,
                               int tile_w, int tile_h, const uint8_t *skip_mi,
                               int mi_stride, int mi_cols, int mi_rows,
                               const uint8_t *cdef_index_sb, int sb_stride,
                               const R1CdefParams *params, void *stream);

/* The same in two steps, as the reference does it per superblock (cdef_analyze_superblock once,
 * src/cdef.rs:340-373, then cdef_filter_superblock for each plane, 405-560): the analysis
 * writes (dir, var) of every 8x8 luma block, raster order over the grid of
 * nbx = 8*ceil(tile_w/64) by nby = 8*ceil(tile_h/64) blocks (r1_cdef_analyze_blocks() entries;
 * blocks outside mi_cols x mi_rows are not written; skipped blocks are analysed too, their
 * entries are never read), and three filter calls share it.  r1_cdef_filter_frame_plane is
 * analysis + one plane with stream-ordered scratch.  tile_w / tile_h here = the luma PLANE size as
 * v_frame pads it (multiples of 8; r1_cdef_filter_frame_plane_dirs has no luma plane to take the
 * picture limits from and rejects anything else with R1_EINVAL). */
long long r1_cdef_analyze_blocks(int tile_w, int tile_h);
int r1_cdef_analyze_frame(r1_ctx *ctx, const R1Plane *luma, int tile_w, int tile_h,
                          int mi_cols, int mi_rows, uint8_t *dir_out, int32_t *var_out,
                          void *stream);
int r1_cdef_filter_frame_plane_dirs(r1_ctx *ctx, const uint8_t *dirs, const int32_t *vars,
                                    const R1Plane *in, const R1Plane *out, int p, int xdec,
                                    int ydec, int tile_w, int tile_h, const uint8_t *skip_mi,
                                    int mi_stride, int mi_cols, int mi_rows,
                                    const uint8_t *cdef_index_sb, int sb_stride,
                                    const R1CdefParams *params, void *stream);

/* CDEF strength search: the CDEF leg of rdo_loop_decision (src/rdo.rs:2104-2560) when no
 * restoration filter is in play (RestorationFilter::None / no restoration unit,
 * rdo.rs:2432-2451, 2504-2520).  The reference cuts the deblocked reconstruction into
 * analysis areas of area_sb_w x area_sb_h superblocks (the largest restoration unit; 1 x 1
 * with restoration off), takes a scratch copy of each (rdo.rs:2277-2284: the AREA's borders are
 * picture edges for CDEF) and, for every superblock that is not completely skipped, tries
 * cdef_index 0 .. n_idx-1: cdef_filter_superblock (src/cdef.rs:405-560), then
 * rdo_loop_plane_error (rdo.rs:2027-2093: cdef_dist_kernel * bias per 8x8 luma block, sse_wxh
 * with the bias per chroma block, each plane's sum * fi.dist_scale[pli]) and keeps the first
 * index of smallest compute_rd_cost(rate 0, err).  One launch evaluates every (superblock,
 * index) of the frame; no filtered plane is written.
 *   rec / src: `planes` whole-frame planes (rec deblocked; areas at multiples of the area
 *   size), skip_mi: Block::skip per 4x4 luma unit, scales: coded_frame_data.distortion_scales
 *   (Q14, per 8x8 luma block; NULL = DistortionScale::default()).
 *   err_out: [n_sby][n_sbx][8] ScaledDistortion (0 for skipped superblocks / unused indices),
 *   best_out: [n_sby][n_sbx], -1 = skipped; n_sb* = ceil(mi / 16).  scratch: DEVICE,
 *   r1_cdef_strength_search_scratch_bytes() bytes (zeroed here).  All pointers DEVICE. */
typedef struct R1CdefSearchParams {
  uint8_t y_strengths[8], uv_strengths[8];   /* fi.cdef_y_strengths / cdef_uv_strengths */
  int32_t damping, bit_depth;                /* fi.cdef_damping, fi.sequence.bit_depth */
  int32_t n_idx;                             /* 1 << fi.cdef_bits */
  int32_t planes;                            /* 1 (Cs400) or 3 */
  int32_t xdec, ydec;                        /* chroma decimation: (1,1), (1,0) or (0,0) */
  int32_t crop_w, crop_h;                    /* fi.width, fi.height */
  int32_t area_sb_w, area_sb_h;
  uint32_t dist_scale[3];                    /* fi.dist_scale[pli] (DistortionScale, Q14) */
} R1CdefSearchParams;
long long r1_cdef_strength_search_scratch_bytes(int mi_cols, int mi_rows);
int r1_cdef_strength_search(r1_ctx *ctx, const R1Plane *rec, const R1Plane *src,
                            const uint8_t *skip_mi, int mi_stride, int mi_cols, int mi_rows,
                            const uint32_t *scales, int scale_stride,
                            const R1CdefSearchParams *params, uint64_t *err_out,
                            int8_t *best_out, void *scratch, void *stream);

/* ---- rdo_loop_decision with BOTH filters on: the later passes of its CDEF leg, and the working copy
 * (src/rdo.rs:2366-2574; BASELINE configs[3]: speed 4 enables cdef and lrf,
 * src/api/config/speedsettings.rs:78-79,168-171).  The reference alternates the two legs until no
 * choice changes.  From the second pass on a restoration unit may hold a self-guided choice, and every
 * CDEF trial of a superblock under it then goes (rdo.rs:2407-2530)
 *   cdef_filter_superblock(index)  ->  per plane: setup_integral_image on THAT SUPERBLOCK of the working
 *   copy (crop = the superblock: hard-clipped right and below; 4 columns left / 2 rows above from the
 *   working copy when the superblock is not first in its area) -> sgrproj_stripe_filter(set, xqd of the
 *   unit's current choice) -> rdo_loop_plane_error of the RESTORED superblock,
 * planes without such a choice as in the first pass (error of the CDEF output itself).
 *
 * r1_cdef_lrf_trial_batch: ONE call per pass for every (superblock, index) of the frame.
 *   rec / src / skip_mi / scales / params / err_out / best_out: as r1_cdef_strength_search (with no
 *     units the two calls return the same numbers);
 *   units (DEVICE): the superblocks whose restoration unit holds a self-guided choice -- n_units[0]
 *     luma entries, then n_units[1] of U, then n_units[2] of V (n_units: HOST, 3 ints).  (x, y, w, h):
 *     the superblock's visible rectangle in pixels of that plane (w = vis_width, h = vis_height,
 *     rdo.rs:2415-2428: what is filtered; the error is taken over every block of the grid it touches,
 *     see "frame sizes" below), set / xqd: the choice, edges: R1_SGR_EDGE_LEFT when the
 *     superblock is not in column 0 of its area, R1_SGR_EDGE_ABOVE when not in row 0, sb = fby * n_sbx + fbx;
 *   cdef_cur: the area working copies as r1_cdef_apply_area leaves them (read only where an edge flag is
 *     set; any valid planes otherwise);
 *   sb_sel (DEVICE, n_sb bytes, NULL = all): superblocks to evaluate.  In an area of several
 *     superblocks a trial reads its left / upper neighbours' CURRENT output, which the same pass may
 *     just have changed: such a host walks the area positions in raster order -- one call per position
 *     with that position selected, r1_cdef_apply_area in between; areas of one superblock (64-pixel
 *     luma units, every qindex <= 160) need one call;
 *   err_planes_out (optional): [n_sb][8][3] the per-plane ScaledDistortion terms of err_out;
 *   scratch: r1_cdef_lrf_trial_scratch_bytes() bytes -- it holds the trial output of every index as
 *     whole planes (n_idx x frame), which the restoration trial reads back.
 * The rate of a trial is the same for every index of a superblock (rdo.rs:2444-2456, 2499-2503): the
 * host adds it to err_out before comparing costs when it wants the reference's f64 rounding;
 * best_out compares the errors alone.
 *
 * r1_cdef_apply_area: cdef_filter_superblock with index_sb[sb] for every superblock into `out` -- the
 * CDEF working copy of every area at once (rdo.rs:2546-2560: "keep cdef output up to date"), the input
 * of the restoration leg (rdo.rs:2575-2582).  Superblocks with index < 0 or completely skipped, and
 * skipped 8x8 blocks, are copied from rec.  Areas' borders are picture edges as in the search.  Only
 * pixels of 8x8 blocks inside the block grid are written.  An index_sb entry outside [0, n_idx) means
 * "not filtered", like a negative one.  scratch: r1_cdef_strength_search_scratch_bytes().
 *
 * Frame sizes that are not multiples of 8 luma pixels.  rdo_loop_plane_error sums EVERY block of the
 * block grid (rdo.rs:2039-2043; mi_cols = 2 * ceil(crop_w / 8), mi_rows likewise), a last block that is
 * only partly visible included, whole.  Its pixels past the visible edge are: the source's and the
 * reconstruction's / CDEF output's own (both cut out of the 8-aligned allocation, rdo.rs:2277-2295),
 * and, on a plane restored inside a trial, R1_PLANE_NEW_FILL -- the restoration working copy is a fresh
 * Plane::new (rdo.rs:2331-2341) that the filter writes inside vis_width x vis_height only.  So every
 * plane handed to these calls must be ALLOCATED out to the block grid (width >= (mi_cols * 4) >> xdec,
 * height >= (mi_rows * 4) >> ydec, as Frame::new makes them) and carry real pixels there; crop_w /
 * crop_h stay the visible size.  Planes that do not reach the grid, or a grid that is not the crop's,
 * are R1_EINVAL; a unit whose blocks leave its planes is not evaluated.  With a subsampled plane
 * crop % 8 == 1 is not taken (the visible chroma extent no longer touches the last block column). */
typedef struct R1TrialUnit {
  int16_t x, y, w, h;
  uint8_t set, edges;
  int8_t xqd[2];
  int32_t sb;
} R1TrialUnit;
long long r1_cdef_lrf_trial_scratch_bytes(int mi_cols, int mi_rows, int xdec, int ydec,
                                          int bytes_per_px, int n_idx, int planes);
int r1_cdef_lrf_trial_batch(r1_ctx *ctx, const R1Plane *rec, const R1Plane *cdef_cur, const R1Plane *src,
                            const uint8_t *skip_mi, int mi_stride, int mi_cols, int mi_rows,
                            const uint32_t *scales, int scale_stride, const R1CdefSearchParams *params,
                            const R1TrialUnit *units, const int32_t *n_units, const uint8_t *sb_sel,
                            uint64_t *err_out, uint64_t *err_planes_out, int8_t *best_out, void *scratch,
                            void *stream);
int r1_cdef_apply_area(r1_ctx *ctx, const R1Plane *rec, const R1Plane *out, const uint8_t *skip_mi,
                       int mi_stride, int mi_cols, int mi_rows, const R1CdefSearchParams *params,
                       const int8_t *index_sb, void *scratch, void *stream);

/* ---- lookahead cost maps (SURVEY.md 8f "N1"; reference:
 * estimate_intra_costs src/api/lookahead.rs:30-123,
 * estimate_importance_block_difference 125-180, the SATD map of
 * estimate_inter_costs 226-268).  One launch per frame; the 8x8 importance
 * blocks are independent.  costs: (height/8) * (width/8) u32, row-major.
 * mvs: (row, col) int16 pairs in 1/8 pel per importance block
 * (stats[y*2][x*2].mv; the motion search itself is not part of this call).
 * sum_out: device u64 = sum over blocks of |mean(org) - mean(ref)| (the
 * reference divides by the block count in f64). */
int r1_estimate_intra_costs(r1_ctx *ctx, const R1Plane *luma, uint32_t *costs, void *stream);
int r1_estimate_inter_costs(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref,
                            const int16_t *mvs, uint32_t *costs, void *stream);
int r1_importance_block_difference(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref,
                                   uint64_t *sum_out, void *stream);

/* ---- frame glue: planes stay resident in HBM between the block stages ----
 * r1_plane_pad: Plane::pad(w, h) (v_frame 0.3.9) as FramePad::pad calls it per plane
 * (src/frame/mod.rs:76-86) on the reconstruction before it becomes a reference
 * (src/api/internal.rs:1436): the visible area of (w + xdec) >> xdec by (h + ydec) >> ydec
 * pixels is replicated over the whole allocation (left / right to the stride, above / below to
 * alloc_height).  w, h: FRAME size in luma pixels; xdec, ydec: the plane's decimation.
 * r1_plane_downsample: Plane::downsampled(frame_w, frame_h) (v_frame 0.3.9), the call that
 * makes FrameState::input_hres / input_qres (src/encoder.rs:476-477): dst (caller-allocated,
 * visible size ((src.width + 1) / 2, (src.height + 1) / 2), half the padding) receives the
 * rounded 2x2 box average, then dst.pad(frame_w, frame_h) with dst's decimation (1 for the
 * half-, 2 for the quarter-resolution plane) -- one launch for both.  src must be padded (odd
 * sizes read one pixel into its border), as in the reference. */
int r1_plane_pad(r1_ctx *ctx, const R1Plane *plane, int w, int h, int xdec, int ydec, void *stream);
int r1_plane_downsample(r1_ctx *ctx, const R1Plane *src, const R1Plane *dst, int frame_w, int frame_h,
                        int dst_xdec, int dst_ydec, void *stream);

/* ActivityMask::from_plane + fill_scales (src/activity.rs:21-66): the spatial
 * DistortionScale of every 8x8 luma block, ssim_boost(variance, variance) in
 * Q14 -- the producer of the `scales` grid r1_dist_scaled_batch and
 * r1_rdo_pixel_cand_batch consume (the encoder multiplies it with the
 * lookahead's spatiotemporal scale, src/api/internal.rs).  ceil(w/8) x
 * ceil(h/8) entries, row-major; either output may be NULL. */
int r1_activity_scales(r1_ctx *ctx, const R1Plane *luma, uint32_t *variances, uint32_t *scales,
                       void *stream);

/* update_block_importances (SURVEY.md 8f "N1"; src/api/internal.rs:911-1068)
 * after its SATD map, which is the map of r1_estimate_inter_costs with
 * mvs[i] = me_stats[2y][2x].mv: every 8x8 importance block i of the current
 * frame adds  (intra_cost + future_importance) * (1 - inter_cost / intra_cost) / len
 * (0 when intra_cost <= inter_cost), split by overlap area, to the importance
 * blocks of the reference frame under its motion-compensated position.  All
 * maps are w_in_imp_b x h_in_imp_b, row-major, DEVICE; ref_importances is
 * updated in place.  f32 throughout, one IEEE operation at a time and summed
 * in the reference's order (source blocks in raster order): the result is
 * bit-identical to the sequential loop.  scratch: DEVICE, 256-byte aligned,
 * at least r1_update_block_importances_scratch_bytes(w, h) bytes (pair lists,
 * per-destination counts / offsets: 76 bytes per importance block; < 0 on
 * error), caller-owned like every buffer. */
long long r1_update_block_importances_scratch_bytes(int w_in_imp_b, int h_in_imp_b);
int r1_update_block_importances(r1_ctx *ctx, const uint32_t *intra_costs,
                                const float *future_importances, const uint32_t *inter_costs,
                                const int16_t *mvs, int w_in_imp_b, int h_in_imp_b, int len,
                                float *ref_importances, void *scratch, long long scratch_bytes,
                                void *stream);

/* ---- temporal-RDO scale maps and segmentation inputs (SURVEY.md 8f "N1" -> "N4"): what the reference does once
 * per coded frame between the lookahead and the first RDO call.  All maps are n = w_in_imp_b * h_in_imp_b entries,
 * row-major, DEVICE; a DistortionScale is its Q14 u32.  Every result is the reference's integer arithmetic bit for
 * bit; the one float is the f64 pow(frac, 1/3) of distortion_scale_for, whose last bits do not reach the Q14
 * result except on a vanishing share of inputs (docs/PARITY.md).
 *
 * r1_frame_scales: distortion_scale_for(block_importances[i], intra_costs[i]) per block (src/api/internal.rs:
 * 1211-1230, src/rdo.rs:506-553; an intra cost of 0 gives 1.0), then CodedFrameData::compute_spatiotemporal_scores
 * (activity_scales given: score = d * a, both maps times inv_mean(scores)) or compute_temporal_scores
 * (activity_scales NULL, Tune::Psnr: both outputs are d * inv_mean(d)) (src/encoder.rs:744-777;
 * DistortionScale::inv_mean, Mul src/rdo.rs:585-630).  distortion_scales_out is the `scales` grid of
 * r1_dist_scaled_batch and the fused candidates as it stands; spatiotemporal_out feeds r1_scale_kmeans.
 * stats_out (DEVICE): the sum of blog32_q11 over the scores, inv_mean, and the functions' return value
 * inv_mean.blog64() >> 1 that rate control takes.  scratch: DEVICE, 256-byte aligned,
 * r1_frame_scales_scratch_bytes(n) bytes (< 0 on error). */
typedef struct R1ScaleStats {
  int64_t log_sum_q11;           /* sum of blog32_q11(score) */
  uint32_t inv_mean;             /* DistortionScale::inv_mean(scores).0 */
  uint32_t reserved;
  int64_t log_isqrt_mean_scale;  /* inv_mean.blog64() >> 1, Q57 */
} R1ScaleStats;
long long r1_frame_scales_scratch_bytes(int n);
int r1_frame_scales(r1_ctx *ctx, const uint32_t *intra_costs, const float *block_importances,
                    const uint32_t *activity_scales, int n, uint32_t *distortion_scales_out,
                    uint32_t *spatiotemporal_out, R1ScaleStats *stats_out, void *scratch,
                    long long scratch_bytes, void *stream);

/* r1_scale_kmeans: the k-means of blog16(score) that segmentation_optimize_inner runs for k = 3 ... 8
 * (src/segmentation.rs:84-94, src/util/kmeans.rs:11-102) from a histogram of the keys instead of the sorted
 * array -- the same centroids, thresholds that double-count, rounding and early stop included.
 * centroids_out: DEVICE, 6 x 8 int16, row r = k = 8 - r (the order of the reference's tuple), unused entries 0.
 * scratch: DEVICE, 256-byte aligned, r1_scale_kmeans_scratch_bytes(n) bytes (the bin tables; < 0 on error). */
long long r1_scale_kmeans_scratch_bytes(int n);
int r1_scale_kmeans(r1_ctx *ctx, const uint32_t *spatiotemporal, int n, int16_t *centroids_out, void *scratch,
                    long long scratch_bytes, void *stream);

/* r1_segmentation_from_centroids: the rest of segmentation_optimize_inner (src/segmentation.rs:96-160) and
 * SegmentationState::update_threshold (src/encoder.rs:566-580) on a HOST copy of the 96 bytes above; needs no GPU.
 * The k whose centroid spacing has the least variance (the last such k), compute_delta (blog64(ac_q), bexp64,
 * select_ac_qi(..).max(1) - base_q_idx, centroids in reverse, .max(1 - base_q_idx)) -> seg_delta[0 .. k), the
 * SEG_LVL_ALT_Q data; threshold[i] = DistortionScale::new(base_ac_q^2, q[i + 1] * q[i]), unused entries 0.
 * update_data / preskip / last_active_segid stay the caller's. */
typedef struct R1SegmentationData {
  int16_t seg_delta[8];
  uint32_t threshold[7];
  uint8_t min_segment, max_segment;
  uint8_t k;                     /* max_segment + 1 */
  uint8_t position;              /* row of the centroid table that was chosen: 8 - k */
} R1SegmentationData;
int r1_segmentation_from_centroids(const int16_t *centroids, int base_q_idx, int bit_depth,
                                   R1SegmentationData *out);

/* r1_spatiotemporal_scale_batch: spatiotemporal_scale (src/rdo.rs:464-504: the rounded mean of d * a over the
 * importance blocks a coded block covers, clipped to the map) and segment_idx_from_distortion with select_segment's
 * .max(min_segment) (src/segmentation.rs:180-196) for n coded blocks, one lane each.  blocks: HOST (the library
 * checks every entry -- a BlockSize outside the 22, or an origin outside the map, is R1_EINVAL -- and uploads the
 * list on `stream`); bo_x, bo_y in 4x4 units as a PlaneBlockOffset.  activity_scales NULL = 1.0.  thresholds:
 * HOST, seven entries that never increase (R1SegmentationData.threshold), NULL = segment index min_segment.
 * scale_out (u32) / sidx_out (u8): DEVICE, either may be NULL. */
typedef struct R1ScaleBlock {
  int32_t bo_x, bo_y;
  int32_t bsize;                 /* BlockSize */
} R1ScaleBlock;
int r1_spatiotemporal_scale_batch(r1_ctx *ctx, const uint32_t *distortion_scales,
                                  const uint32_t *activity_scales, int w_in_imp_b, int h_in_imp_b,
                                  const R1ScaleBlock *blocks, int n, const uint32_t *thresholds,
                                  int min_segment, uint32_t *scale_out, uint8_t *sidx_out, void *stream);

/* ---- intra mode pre-screen (SURVEY.md 8f "N1"; src/rdo.rs:1434-1506): for
 * every block the candidate modes are predicted from ONE edge set
 * (get_intra_edges with IntraParam::None) and ranked by get_satd against the
 * source block.  cands: n = blocks * group entries, the `group` modes of block
 * b at [b*group, (b+1)*group); edges / lens (r1_intra_edges_batch layout) and
 * pos_xy (x, y of the block in `src`, int16 pairs) have one entry per BLOCK.
 * The predictions stay in LDS; satd_out[n].  The probability ordering and the
 * final sort (rdo.rs:1424-1428, 1504) are entropy-coder state and stay with
 * the caller. */
int r1_intra_satd_batch(r1_ctx *ctx, const R1Plane *src, int tx_size, const R1IntraCand *cands,
                        int n, int group, const int16_t *pos_xy, const void *edges,
                        int edge_stride, const uint8_t *lens, const int16_t *ac,
                        uint32_t *satd_out, void *stream);

/* The selection step of both mode pre-screens (SURVEY.md 8f "N1": "returning
 * sorted candidate lists"): per group of `group` keys (the SATDs of one block's
 * candidates, in the caller's order -- for the intra pre-screen that is the
 * probability order of src/rdo.rs:1424-1428) the first `keep_head` candidates
 * keep their places, the rest are STABLY sorted by key, and the first k of the
 * resulting list are returned as indices into the group:
 *   intra  modes[num_modes_rdo / 2..].sort_by_key(satd); take(num_modes_rdo)
 *          (src/rdo.rs:1504-1509): keep_head = num_modes_rdo / 2, k = num_modes_rdo
 *   inter  sorted.sort_by_key(satd); take(num_modes_rdo) (src/rdo.rs:1352-1357):
 *          keep_head = 0
 * keys: n_groups * group (device), idx_out: n_groups * k bytes (device).
 * 1 <= k <= group <= 64, 0 <= keep_head <= k. */
int r1_prescreen_select_batch(r1_ctx *ctx, const uint32_t *keys, int n_groups, int group,
                              int keep_head, int k, uint8_t *idx_out, void *stream);

/* ---- hierarchical motion estimation of whole tiles (SURVEY.md 8f "N2").
 * Replaces estimate_tile_motion (src/me.rs:153-218) for one (tile, reference
 * frame) pair per job: the three passes (quarter, half, full resolution) of
 * estimate_sb_motion / refine_subsampled_sb_motion with full_pixel_me
 * (predictor subsets, diamond search; at the first pass the thresholded
 * subset / uneven-multi-hexagon / optional full search cascade), writing the
 * reference's FrameMEStats.  Jobs are independent (the reference runs tiles on
 * rayon workers, src/encoder.rs encode_tile_group, and loops the reference
 * frames inside, me.rs:190-199) and execute concurrently; inside a job the
 * superblocks go in anti-diagonal wavefronts -- the exact dependence order of
 * the reference's raster walk (see rav1e_amd/csrc/me_search.hpp).
 *
 * R1MeStats = MEStats (src/me.rs:31-35): mv in 1/8 pel, SAD normalised to a
 * 128x128 block.  stats: the FrameMEStats array of this reference frame
 * (stats_cols x stats_rows entries, one per 4x4 luma block, device memory,
 * in/out: the first pass reads what the previous frame left there exactly as
 * the reference does); prev: the previous frame's array for the same
 * reference index (EPZS subset C, me.rs:477-514) or NULL.
 * org / ref: [0] full, [1] half, [2] quarter resolution luma (FrameState
 * input_hres / input_qres, src/encoder.rs:412-413; ReferenceFrame input_hres /
 * input_qres): device planes with the reference's padding (>= 16 px + block
 * at each resolution, which the MV range of me.rs:339-362 assumes).
 * lambda[ssdec]: (fi.me_lambda * 256 / (1 << 2*ssdec) * (ssdec == 0 ? 0.5 :
 * 0.125)) as u32, me.rs:175-177 -- f64 arithmetic, evaluated by the host.
 * `jobs` is HOST memory (pointers inside are device pointers) and is consumed
 * before the call returns; the work itself is only ENQUEUED on `stream`
 * as ONE persistent launch whose waves walk block rows and hand results over
 * through progress words in memory (two waves per SIMD).  launch_mode 2: every job
 * is pinned to one XCD so that the hand-overs stay in that XCD's L2 -- wants >= 8
 * jobs to use the chip and a device whose launches spread over 8 XCDs (probed once
 * per context; forcing mode 2 elsewhere is R1_EINVAL).  launch_mode 3: not pinned
 * -- any wave takes any row, results written through at agent scope.  launch_mode 1:
 * the launch-boundary version (superblock columns + rows + 3 launches replayed as
 * one hipGraph, the three passes skewed inside them), kept as the cross-check.
 * launch_mode 0 takes 2 from 8 jobs on, else 3.  A dependency wait of a persistent
 * launch that runs out of patience is not a hang: the call is flagged (r1_me_status,
 * below), and once a flagged launch has finished every following call of this
 * function returns R1_ETIMEDOUT -- nothing enqueued -- until r1_me_status has
 * reported the flag.  At most 256 jobs per call (tiles x reference frames of
 * one frame).  The context keeps one scratch MEStats frame per distinct
 * `stats` array of a call (the refinements of a pass are computed one diagonal
 * ahead of its searches and must stay invisible to them until then). */
typedef struct R1MeStats {
  int16_t row, col;
  uint32_t normalized_sad;
} R1MeStats;
typedef struct R1MeParams {
  int32_t w_in_b, h_in_b;            /* fi.w_in_b, fi.h_in_b (4x4 units) */
  int32_t stats_cols, stats_rows;    /* FrameMEStats::cols, rows */
  int32_t bit_depth;
  int32_t allow_hp;                  /* fi.allow_high_precision_mv */
  int32_t allow_full_search;         /* speed_settings.motion.me_allow_full_search */
  int32_t me_range_scale;            /* fi.me_range_scale */
  uint32_t lambda[3];
  int32_t launch_mode;               /* r1_estimate_tile_motion_batch: 0 = choose (below), 1 = one
                                      * launch per superblock diagonal, 2 / 3 = one persistent launch,
                                      * jobs pinned to an XCD each / not pinned */
} R1MeParams;
typedef struct R1MeJob {
  R1Plane org[3], ref[3];
  R1MeStats *stats;
  const R1MeStats *prev;
  int32_t tile_x, tile_y;            /* luma px, multiples of 64 */
  int32_t tile_w, tile_h;            /* luma px, multiples of 4 */
} R1MeJob;
int r1_estimate_tile_motion_batch(r1_ctx *ctx, const R1MeJob *jobs, int n_jobs,
                                  const R1MeParams *params, void *stream);
/* The persistent launches (launch_mode 2 / 3) hand results between waves through memory; a wave
 * whose dependency wait runs out of patience (a bounded spin: nothing can hang the GPU) carries on
 * with stale predictors and flags the CALL.  The statistics of a call are valid once r1_me_status
 * has returned R1_OK after it: wait != 0 first waits for every launch enqueued so far (wait == 0
 * only looks at launches that have finished).  R1_ETIMEDOUT: *first_failed_call (optional) is the
 * 1-based index, per context, of the first flagged r1_estimate_tile_motion_batch call -- re-issue
 * it with launch_mode = 1 (launch boundaries instead of waits).  Flags are consumed by the report;
 * while one is pending, r1_estimate_tile_motion_batch refuses with R1_ETIMEDOUT (a caller that never
 * polls cannot go on consuming non-reference statistics silently).  *calls (optional): calls made on this context so far. */
int r1_me_status(r1_ctx *ctx, int wait, unsigned long long *first_failed_call,
                 unsigned long long *calls);

/* estimate_motion with a predicted MV (the RDO-time call, src/rdo.rs:1183-1196:
 * estimate_motion(fi, ts, w, h, tile_bo, ref, Some(pmv), corner, false, 0, None),
 * src/me.rs:536-632) over n independent blocks of one (tile, reference) pair:
 * full_pixel_me at full resolution from the tile's MEStats (read only),
 * get_fullpel_mv_rd with SATD when use_satd (speed_settings.motion
 * .use_satd_subpel), then subpel_diamond_search (1/2 -> 1/4 -> 1/8 pel when
 * allow_hp; put_8tap of fi.default_filter = filter_mode + get_satd / get_sad).
 * tile: HOST descriptor (planes [0] are used; stats / prev as above).
 * cands, out: DEVICE arrays.  bx, by: tile-relative position in 4x4 units;
 * w, h: a BlockSize up to 64x64; corner: 0 = MVSamplingMode::INIT, else
 * 1 | right << 1 | bottom << 2; pmv[k] = (row, col) in 1/8 pel.
 * max_w, max_h: the largest block of the batch (sizes the LDS of the launch;
 * a candidate that exceeds it, or is not a power-of-two BlockSize, returns the
 * reference's MotionSearchResult::empty(): cost = u64::MAX, sad = u32::MAX).
 * out[i] = MotionSearchResult { mv, rd { cost, sad } }. */
typedef struct R1MeBlockCand {
  int16_t bx, by;
  uint8_t w, h, corner, reserved;
  int16_t pmv[2][2];
} R1MeBlockCand;
typedef struct R1MeResult {
  int16_t row, col;
  uint32_t sad;
  uint64_t cost;
} R1MeResult;
int r1_estimate_motion_batch(r1_ctx *ctx, const R1MeJob *tile, const R1MeParams *params,
                             const R1MeBlockCand *cands, int n, int max_w, int max_h,
                             int use_satd, int filter_mode, R1MeResult *out, void *stream);

/* ---- deblocking filter and its level search (SURVEY.md 8f "N3"; reference
 * src/deblock.rs: deblock_plane 1294-1459 / deblock_filter_frame 1544-1551,
 * sse_plane 1461-1542, sse_optimize 1553-1617, deblock_filter_optimize 1620).
 * R1DeblockBlock: what the filter reads from the reference's per-4x4 `Block`
 * (src/context/block_unit.rs), one entry per 4x4 luma block of the frame,
 * row-major with `blocks_stride` entries per row, DEVICE memory:
 *   tx_log2   = log2(txsize.width_mi()) | log2(txsize.height_mi()) << 3
 *   uvtx_log2 = the same for bsize.largest_chroma_tx_size(xdec, ydec)
 *   n4_log2   = log2(n4_w) | log2(n4_h) << 3
 *   flags     = skip | (ref_frames[0] == INTRA_FRAME) << 1
 *               | (mode >= NEARESTMV && mode != GLOBALMV && mode != GLOBAL_GLOBALMV) << 2
 *               | ref_frames[0].to_index() << 3
 *   deltas    = deblock_deltas
 * R1DeblockState = DeblockState (levels: Y vertical, Y horizontal, U, V).
 * r1_deblock_plane filters `plane` IN PLACE (pli 0..2; luma: xdec = ydec = 0),
 * crop_w / crop_h in luma pixels as the reference's callers pass them
 * (fi.width, fi.height).
 * r1_deblock_sse_plane ADDS the level-search tallies of one plane into
 * v_tally / h_tally (device, MAX_LOOP_FILTER + 2 = 65 int64 each, zeroed by
 * the caller); r1_deblock_pick_levels is sse_optimize's tail on HOST copies of
 * them: luma -> levels_out[0..1] = (vertical, horizontal), chroma ->
 * levels_out[0].  Like the reference's sse_h_edge (deblock.rs:1258) the
 * horizontal tallies size their filters from transform WIDTHS; near the top and
 * bottom of the frame such a line may read up to 7 rows of the planes' padding. */
typedef struct R1DeblockBlock {
  uint8_t tx_log2, uvtx_log2, n4_log2, flags;
  int8_t deltas[4];
} R1DeblockBlock;
typedef struct R1DeblockState {
  uint8_t levels[4];
  uint8_t sharpness;            /* carried; the reference's filters never read it */
  uint8_t deltas_enabled, block_deltas_enabled, block_delta_shift, block_delta_multi;
  int8_t ref_deltas[8], mode_deltas[2];
  uint8_t reserved[5];
} R1DeblockState;
int r1_deblock_plane(r1_ctx *ctx, const R1DeblockState *state, const R1Plane *plane, int pli,
                     int xdec, int ydec, const R1DeblockBlock *blocks, int blocks_stride,
                     int blocks_cols, int blocks_rows, int crop_w, int crop_h, void *stream);
int r1_deblock_sse_plane(r1_ctx *ctx, const R1Plane *rec, const R1Plane *src, int pli, int xdec,
                         int ydec, const R1DeblockBlock *blocks, int blocks_stride, int blocks_cols,
                         int blocks_rows, int crop_w, int crop_h, int64_t *v_tally,
                         int64_t *h_tally, void *stream);
int r1_deblock_pick_levels(const int64_t *v_tally, const int64_t *h_tally, int pli,
                           uint8_t *levels_out);
/* The same for all three planes of a 4:x:x frame at once (deblock_filter_frame /
 * deblock_filter_optimize, src/deblock.rs:1544-1551, 1620-1668): planes / rec /
 * src point at THREE R1Plane structs (Y, U, V; host memory), chroma decimation
 * xdec / ydec.  r1_deblock_frame: two launches (all vertical edges of the three
 * planes, then all horizontal ones) instead of six.  r1_deblock_sse_frame: one
 * launch for the six (plane, direction) tallies; `tallies` = 6 x 65 int64
 * (DEVICE, zeroed by the caller), entry 2 * pli + (0 vertical, 1 horizontal),
 * each as r1_deblock_sse_plane fills it. */
int r1_deblock_frame(r1_ctx *ctx, const R1DeblockState *state, const R1Plane *planes, int xdec,
                     int ydec, const R1DeblockBlock *blocks, int blocks_stride, int blocks_cols,
                     int blocks_rows, int crop_w, int crop_h, void *stream);
int r1_deblock_sse_frame(r1_ctx *ctx, const R1Plane *rec, const R1Plane *src, int xdec, int ydec,
                         const R1DeblockBlock *blocks, int blocks_stride, int blocks_cols,
                         int blocks_rows, int crop_w, int crop_h, int64_t *tallies, void *stream);

/* ---- loop restoration, self-guided filter (SURVEY.md 8f "N3", last stage of
 * the post-filter chain; reference RestorationState::lrf_filter_frame
 * src/lrf.rs:1482-1585 -> setup_integral_image 530 + sgrproj_stripe_filter
 * 630; the encoder never selects Wiener, src/rdo.rs:2508).  One plane per call:
 * cdeffed = the CDEF output, deblocked = the frame before CDEF (rows outside a
 * 64-row stripe are taken from it, as the decoder does), out = a plane that
 * already holds a copy of the CDEF output (units without a filter are left as
 * they are; must not alias cdeffed).  crop_w / crop_h: visible size of THIS
 * plane ((fi.width + xdec_round) >> xdec ..), frame_height: fi.height (luma;
 * sets the stripe count), ydec: the plane's vertical decimation, unit_size /
 * unit_cols / unit_rows / stripe_height: RestorationPlaneConfig, units:
 * unit_rows x unit_cols entries (DEVICE), filter = RESTORE_NONE 0 or
 * RESTORE_SGRPROJ 3, set = index into SGRPROJ_PARAMS_S, xqd as coded.
 * A unit with R1_SGR_EDGE_LEFT reads 4 columns left of its x, one with R1_SGR_EDGE_ABOVE 2 rows above its y:
 * such a unit must lie at x >= 4 (y >= 2) or the plane must carry that much origin padding (xorigin >= 4,
 * yorigin >= 2; rav1e's planes carry 88 / 44) -- the kernels clamp the read to the allocation's first
 * column / row otherwise, which is not what the reference reads.
 * All three restoration entry points address pixels with 32-bit byte offsets:
 * R1_EINVAL for an input plane whose allocation (stride * alloc_height *
 * bytes_per_px) reaches 4 GiB or whose stride / alloc_height reach 2^24. */
typedef struct R1LrfUnit {
  uint8_t filter, set;
  int8_t xqd[2];
} R1LrfUnit;
int r1_lrf_sgrproj_plane(r1_ctx *ctx, const R1Plane *cdeffed, const R1Plane *deblocked,
                         const R1Plane *out, int ydec, int crop_w, int crop_h, int frame_height,
                         int unit_size, int unit_cols, int unit_rows, int stripe_height,
                         const R1LrfUnit *units, void *stream);
/* sgrproj_solve (src/lrf.rs:847-1096) as the restoration search calls it
 * (rdo_loop_decision, src/rdo.rs:2651-2676): for each (restoration unit,
 * parameter set) pair the least-squares projection weights xqd of the
 * self-guided filter of `cdeffed` towards `input` (the source frame), the
 * unit hard-clipped at its right / bottom edge, its left / upper neighbourhood
 * as the unit's `edges` say (below), no stripes.  units (DEVICE):
 * (x, y, w, h) in plane pixels, w <= max_w, h <= max_h (<= 384); xqd_out:
 * 2 int8 per pair; moments_scratch: 5 int64 per pair (device; zeroed here).
 * The moments are exact integers, the 2x2 solve is done in IEEE doubles with
 * the reference's operation order (including its two fused multiply-adds),
 * so the weights are bit-identical. */
typedef struct R1SgrSolveUnit {
  int16_t x, y, w, h;
  uint8_t set;
  uint8_t edges;      /* R1_SGR_EDGE_* (ABI 6; was reserved = 0) */
  uint8_t reserved[2];
} R1SgrSolveUnit;
/* What setup_integral_image (src/lrf.rs:530-630) sees outside the unit.  rdo_loop_decision filters
 * a unit on its scratch copy of the AREA it is deciding -- the largest restoration unit of the three
 * planes, in superblocks (src/rdo.rs:2119-2141, 2277-2296) -- and that copy has no pixels outside the
 * area.  The right and bottom edges are always clipped to the unit (crop = the unit).  On the left
 * the filter reads 4 real columns, above 2 real rows, IF the unit's slice does not start in column 0
 * / row 0 of the area copy, i.e. if the plane has more than one unit per area (a 64-pixel luma unit
 * beside 128-pixel chroma units) and this is not the first:
 *   edges = (unit x in plane pixels) % (area width in plane pixels) != 0 ? R1_SGR_EDGE_LEFT : 0
 *         | (unit y ...) % (area height ...) != 0 ? R1_SGR_EDGE_ABOVE : 0
 * 0 (every unit of the 64 / 32-pixel configuration: one unit per plane and area) = the unit alone.
 * A flag is ignored at the plane's own left / top edge.  Found by executing rdo_loop_decision itself
 * (tests/golden/gen_loop_decision_ref.py); up to ABI 5 the kernels decided from the unit's position
 * in the FRAME, which matches the reference only for areas at the frame's left / top edge. */
enum { R1_SGR_EDGE_LEFT = 1, R1_SGR_EDGE_ABOVE = 2 };
/* What a pixel of rdo_loop_decision's restoration working copy holds where no filter wrote: the fill
 * of v_frame's Plane::new, for every bit depth.  v_frame is not part of the reference tree: the value
 * restates it (docs/PARITY.md).  One constant for product, oracle (R1O_PLANE_NEW_FILL), the fixture
 * generator and the host driver (rav1e_amd.loop_decision.PLANE_NEW_FILL). */
#define R1_PLANE_NEW_FILL 128
int r1_sgrproj_solve_batch(r1_ctx *ctx, const R1Plane *cdeffed, const R1Plane *input,
                           const R1SgrSolveUnit *units, int n, int max_w, int max_h,
                           int64_t *moments_scratch, int8_t *xqd_out, void *stream);
/* The restoration-filter leg of rdo_loop_decision for ONE plane, everything but the entropy coder's
 * rate (src/rdo.rs:2575-2763).  For each (restoration unit, parameter set) pair:
 *   xqd = sgrproj_solve on the unit (as above);
 *   the unit filtered with those weights -- sgrproj_stripe_filter on the unit's own integral image
 *   (setup_integral_image with crop = the unit, rdo.rs:2651-2666, 2688-2702), never stored;
 *   err = rdo_loop_plane_error of that against `src` (rdo.rs:2027-2093): over the 8x8-luma blocks
 *   of the unit  cdef_dist_kernel * bias  (luma, is_chroma 0)  or  sse_wxh with |_, _| bias on
 *   (8 >> xdec) x (8 >> ydec) pixels (is_chroma 1), bias = scales[(luma y >> 3) * scale_stride +
 *   (luma x >> 3)] (NULL: the default scale), summed and multiplied by dist_scale (fi.dist_scale[pli],
 *   Q14).
 * units[i].set = 255: the "no filter option" (rdo.rs:2617-2643): err of lrf_in itself, xqd (0, 0).
 * Units start on superblock boundaries; (w, h) is the unit's VISIBLE size (rdo.rs:2651-2658): what is
 * solved and filtered.  The error covers every block of the grid the unit touches, ceil(w / bw) x
 * ceil(h / bh) blocks of bw x bh = (8 >> xdec) x (8 >> ydec) pixels, whole: where a last block reaches
 * past the visible edge, `src` is read as it is, the no-filter option reads `lrf_in` as it is, and a
 * filtered unit reads R1_PLANE_NEW_FILL (the reference's restoration working copy is never written
 * there).  Both planes must be allocated in whole blocks out to that grid, with real pixels (Frame::new
 * aligns to 8 luma pixels): a width / height that is not a multiple of bw / bh is R1_EINVAL, a unit
 * whose blocks leave a plane gets err = UINT64_MAX and xqd (0, 0).  scratch: 6 int64 per pair
 * (device).  The host adds cw.fc.count_lrf_switchable's rate to err and keeps the cheapest choice
 * (compute_rd_cost, rdo.rs:718-723). */
int r1_lrf_search_batch(r1_ctx *ctx, const R1Plane *lrf_in, const R1Plane *src,
                        const R1SgrSolveUnit *units, int n, int max_w, int max_h, int is_chroma,
                        int xdec, int ydec, const uint32_t *scales, int scale_stride,
                        uint32_t dist_scale, int64_t *scratch, int8_t *xqd_out, uint64_t *err_out,
                        void *stream);

/* ---- fused RDO candidate: the headline path.  For each candidate:
 *   pred   = put_8tap(ref @ (rx,ry), fracs, modes)              (src/mc.rs:250)
 *   sad    = get_sad(org @ (ox,oy), pred)       if sad_out     (src/dist.rs:31)
 *   satd   = get_satd(org @ (ox,oy), pred)      if satd_out    (src/dist.rs:156)
 *   resid  = diff(org, pred)                                    (src/encoder.rs:1355)
 *   coeffs = forward_transform(resid, tx_size, tx_type)  if coeffs
 * in one launch with the block staged in LDS; pred never touches HBM unless
 * pred_out is non-NULL.  tx_size must be the block's own size (w x h <= 64). */
int r1_rdo_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref,
                      int w, int h, int tx_size, const R1RdoCand *cands, int n,
                      uint32_t *sad_out, uint32_t *satd_out, void *coeffs,
                      void *pred_out, void *stream);

/* ---- full RDO candidate (SURVEY.md 8f "N4"): the fused candidate carried
 * through the quantizer, i.e. what encode_tx_block computes per transform block
 * for RDOType::TxDistEstRate (src/encoder.rs:1533-1650) with an inter
 * prediction in front (src/rdo.rs:1073 rdo_tx_size_type -> motion_compensate ->
 * encode_tx_block):
 *   pred, sad, satd, resid, coeffs     as r1_rdo_cand_batch
 *   eob      = quantize(coeffs -> qcoeffs; scan order of the candidate's tx_type)
 *                                                   (src/quantize/mod.rs:282-361)
 *   rcoeffs  = dequantize(qcoeffs)                  (src/quantize/mod.rs:363-384)
 *   tx_dist  = sum (coeffs - rcoeffs)^2, rounded and shifted by tx_scale
 *                                                   (src/encoder.rs:1615-1650)
 *   est_rate = estimate_rate(qindex, tx_size, tx_dist)       (src/rdo.rs:127-139)
 * One launch; prediction, residual, coefficients and rcoeffs never leave the
 * CU: 14 bytes per candidate go to HBM.  eob_out, tx_dist_out required;
 * sad_out, satd_out, est_rate_out optional; qcoeffs_out (optional): dense
 * coded-area blocks (min(w,32)*min(h,32) int16 for 8-bit / int32 otherwise);
 * coeffs (optional): the unquantized w*h coefficients as r1_rdo_cand_batch.
 * tx_type >= 16 (WHT) has no scan order and is rejected by the reference's
 * table bounds; here the result for such a candidate is unspecified. */
int r1_rdo_full_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, int w,
                           int h, int tx_size, const R1RdoCand *cands, int n,
                           const R1QuantParams *params, uint32_t *sad_out,
                           uint32_t *satd_out, uint16_t *eob_out, uint64_t *tx_dist_out,
                           uint64_t *est_rate_out, void *qcoeffs_out, void *coeffs,
                           void *stream);

/* ---- the default-configuration RDO evaluation of an inter transform block in
 * ONE launch: what luma_chroma_mode_rdo / rdo_tx_size_type make encode_tx_block
 * and compute_distortion do per candidate when the distortion is taken in the
 * pixel domain (tune = Psychovisual, or need_recon_pixel; src/encoder.rs:
 * 1533-1661, src/rdo.rs:254-340):
 *   pred, sad, satd, resid, coeffs, eob, qcoeffs     as r1_rdo_full_cand_batch
 *   rcoeffs = dequantize(qcoeffs)
 *   rec     = inverse_transform_add(rcoeffs, pred)    (src/transform/inverse.rs:1633)
 *   dist    = sse_wxh (R1_DIST_WSSE) / cdef_dist_wxh (R1_DIST_CDEF) of rec against
 *             the source block, with the DistortionScale grid of
 *             r1_dist_scaled_batch (same `scales` layout, xdec / ydec of the plane)
 * Prediction, residual, coefficients and reconstruction live in registers /
 * LDS; per candidate 10 bytes (eob, dist) + the optional outputs reach HBM.
 * qcoeffs_out: what the entropy coder of the host needs for the real rate
 * (RDOType::PixelDistRealRate); rec_out: dense w*h reconstructions. */
int r1_rdo_pixel_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, int w, int h,
                            int tx_size, const R1RdoCand *cands, int n,
                            const R1QuantParams *params, int dist_kind, const uint32_t *scales,
                            int scale_stride, int xdec, int ydec, uint32_t *sad_out,
                            uint32_t *satd_out, uint16_t *eob_out, uint64_t *dist_out,
                            void *qcoeffs_out, void *rec_out, void *stream);

/* The same chains for a prediction that is NOT a single-reference put_8tap:
 * `pred` holds n dense w*h predictions (r1_predict_intra_batch output for the
 * intra mode / tx-type decision of src/rdo.rs:1507-1600 and rdo_tx_size_type,
 * r1_mc_avg_batch output for compound modes); the candidates' rx / ry /
 * fractions are ignored, (ox, oy, tx_type) are used.  dist_kind 0: dist_out =
 * the transform-domain distortion of r1_rdo_full_cand_batch (rec_out must be
 * NULL); R1_DIST_WSSE / R1_DIST_CDEF: the pixel-domain leg of
 * r1_rdo_pixel_cand_batch. */
int r1_rdo_pred_cand_batch(r1_ctx *ctx, const R1Plane *org, const void *pred, int w, int h,
                           int tx_size, const R1RdoCand *cands, int n,
                           const R1QuantParams *params, int dist_kind, const uint32_t *scales,
                           int scale_stride, int xdec, int ydec, uint32_t *sad_out,
                           uint32_t *satd_out, uint16_t *eob_out, uint64_t *dist_out,
                           void *qcoeffs_out, void *rec_out, void *stream);

/* ---- the two-reference (compound) inter candidate in ONE launch (added under ABI 7): what
 * predict_inter_compound (src/predict.rs:339-382) and the SATD ranking of the inter mode pre-screen
 * (src/rdo.rs:1238-1271, 1328-1352: the eight RAV1E_INTER_COMPOUND_MODES on one reference pair) compute per
 * candidate:
 *   t0   = prep_8tap(ref0 @ (rx0, ry0), fracs0)      t1 = prep_8tap(ref1 @ (rx1, ry1), fracs1)   (src/mc.rs:360)
 *   pred = mc_avg(t0, t1)                                                                         (src/mc.rs:454)
 *   sad  = get_sad(org @ (ox, oy), pred)   if sad_out      satd = get_satd(org @ (ox, oy), pred)   if satd_out
 * The int16 intermediates never reach HBM; the prediction does only through pred_out (n dense w*h blocks in
 * the planes' pixel type -- the `pred` input of r1_rdo_pred_cand_batch / r1_rdo_txsearch_batch).  Each output is
 * optional (NULL), at least one must be given; every entry of a given output is written exactly once (no
 * zeroed buffer is needed).  (w, h): what r1_mc_prep_batch takes under this ABI -- w a power of two in 4..128,
 * h even in 2..128, w or h <= 4 selecting the 4-tap filters as get_filter does; sad_out / satd_out only for the
 * 22 BlockSizes (R1_EINVAL otherwise).  The three planes share bytes_per_px and bit_depth (8, 10, 12).
 * Positions may lie in the padding, as for R1McCand.  Chroma planes go through the same call with their own
 * (w, h) and positions, as motion_compensate does. */
typedef struct R1CompoundCand {      /* 20 bytes */
  int16_t ox, oy;                    /* block position in the org (source) plane */
  int16_t rx0, ry0, rx1, ry1;        /* full-pel positions in ref0 / ref1 (get_mv_params) */
  uint8_t col_frac0, row_frac0, col_frac1, row_frac1;   /* 0..15 */
  uint8_t mode_x, mode_y;            /* FilterMode (fi.default_filter for both references) */
  uint8_t reserved[2];
} R1CompoundCand;
int r1_rdo_compound_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref0,
                               const R1Plane *ref1, int w, int h,
                               const R1CompoundCand *cands, int n,
                               uint32_t *sad_out, uint32_t *satd_out, void *pred_out,
                               void *stream);

/* ---- the transform-type search of one prediction in ONE launch (ABI 5): rdo_tx_type_decision
 * (src/rdo.rs:1701-1817) evaluates every TxType of RAV1E_TX_TYPES (src/transform/mod.rs:28-44) that the
 * block's tx set allows (av1_tx_used[get_tx_set(..)], src/context/transform_unit.rs:37-44, 123-148) on the
 * SAME prediction -- it even re-runs motion_compensate per type (rdo.rs:1738-1742) -- through
 * write_tx_tree / write_tx_blocks -> encode_tx_block (src/encoder.rs:1404-1661) and compute_distortion /
 * compute_tx_distortion.  Here the prediction (put_8tap of `ref`, or the dense `pred` buffer of
 * r1_rdo_pred_cand_batch: exactly one of the two is non-NULL), the residual, SAD / SATD and the staged
 * source block are made ONCE per candidate; then, for every set bit t of tx_type_mask in ascending order
 * (slot j = the j-th set bit; nt = popcount(tx_type_mask)):
 *   forward_transform(t) -> quantize -> dequantize -> [inverse_transform_add(t) -> sse_wxh / cdef_dist_wxh]
 * with the residual re-formed on the CU.  The candidates' own tx_type field is ignored.
 *   dist_kind 0:                 dist_out = transform-domain distortion, est_rate_out (optional) as
 *                                r1_rdo_full_cand_batch; rec_out must be NULL
 *   R1_DIST_WSSE / R1_DIST_CDEF: the pixel-domain leg of r1_rdo_pixel_cand_batch; est_rate_out must be NULL
 * Outputs: sad_out / satd_out (optional): n words; eob_out, dist_out (, est_rate_out): n * nt entries,
 * entry [i * nt + j] = candidate i, slot j; qcoeffs_out (optional): n * nt dense coded-area blocks;
 * rec_out (optional): n * nt dense w*h reconstructions.  The rate of each slot's qcoeffs comes from
 * r1_coeff_rate_batch and the cheapest is kept by r1_rd_pick_batch (compute_rd_cost, rdo.rs:718-723), which applies
 * the reference's early exit after the first type (rdo.rs:1793-1802).  That exit is a pure saving only at the first
 * transform depth, where cur_best_rd is f64::MAX; at a later depth it DECIDES: a first type above the carried
 * cur_best_rd drops the whole depth, a later type below it included, so whoever picks must replay it.
 * Sizes up to 16x16 (up to 7 types here, 16 in AV1) run the fan-out kernel.  Sizes with a 32-point side
 * (DCT_DCT, + IDTX for inter blocks) and with a 64-point side (TX_SET_DCTONLY: tx_type_mask must be 1) run one
 * plain launch per type with the type forced -- two waves per SIMD of the fan-out kernel lose against two
 * launches at four (measured) -- same results, same slots.
 * R1_EINVAL: an empty mask, bits beyond the 16 TxTypes, a type the size has no kernel for (tx_type_mask must be a
 * subset of r1_tx_type_mask(tx_size, 1, 0, 0): the inter sets are the largest), both or neither of ref / pred. */
int r1_rdo_txsearch_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref, const void *pred, int w,
                          int h, int tx_size, const R1RdoCand *cands, int n, uint32_t tx_type_mask,
                          const R1QuantParams *params, int dist_kind, const uint32_t *scales,
                          int scale_stride, int xdec, int ydec, uint32_t *sad_out, uint32_t *satd_out,
                          uint16_t *eob_out, uint64_t *dist_out, uint64_t *est_rate_out,
                          void *qcoeffs_out, void *rec_out, void *stream);
/* ---- the intra candidate in ONE launch (added under ABI 7): what the loop over the pre-screened intra modes
 * (src/rdo.rs:1507-1600) makes encode_tx_block (src/encoder.rs:1404-1661) do per mode -- predict_intra from the
 * block's edges (1458-1503), then the transform chain -- without the prediction travelling through HBM.  For
 * candidate i the results are those of
 *   r1_predict_intra_batch(cands, edges, lens, ac)  ->  r1_rdo_txsearch_batch(ref = NULL, pred = that output, ...)
 * bit for bit; the prediction lives in registers / LDS and reaches HBM only through pred_out (optional: n dense
 * w*h blocks in the plane's pixel type, written once per candidate).
 *   cands:      n R1IntraCand as r1_predict_intra_batch takes them (avail_w / avail_h below the tx size at the
 *               right / bottom frame edge, UV_CFL_PRED with `ac` included).
 *   edge_group: >= 1 and a divisor of n.  Candidate i uses edge set, `lens` pair and `pos_xy` pair number
 *               i / edge_group (edges / edge_stride / lens: the outputs of r1_intra_edges_batch; pos_xy: the block
 *               position in `org`, as r1_intra_satd_batch takes it).  1 = the reference's own shape, one
 *               get_intra_edges(Some(mode)) per candidate; a larger group lets the modes of a block share one set
 *               built with mode = -1, as the pre-screen does.  A shared set holds every entry a mode-specific set
 *               holds, with the same values, EXCEPT the top-left entry of a block with w + h >= 24 under
 *               enable_intra_edge_filter: get_intra_edges smooths it (partition.rs:886-892) only for a mode whose
 *               angle lies strictly between 90 and 180 degrees.  There the predictions differ, and callers must
 *               use edge_group = 1 for D135 / D113 / D157 (and V / H with an angle delta that crosses into that
 *               range) -- or give those candidates sets of their own.  Every other mode and geometry may share
 *               (docs/PARITY.md, "intra candidate").
 *   ac:         candidate i uses AC block i, dense w*h int16 per candidate (UV_CFL_PRED), NULL otherwise.
 * tx_type_mask, the slot order, dist_kind (0 / R1_DIST_WSSE / R1_DIST_CDEF), which of est_rate_out / rec_out may
 * be non-NULL for which kind, the output indexing [i * nt + j] and the `scales` grid: r1_rdo_txsearch_batch's.  All
 * 19 transform sizes, bit depths 8 / 10 / 12.  Sizes up to 16x16 run the fan-out form of the kernel for any mask;
 * sizes with a 32- or 64-point side run one plain launch per type (at most two), each of which makes the prediction
 * again on the CU.  The occupancy requests of the kernels are those of the same (size, bit depth) inter
 * instantiation: the chain behind the prediction is the same code.
 * Two launches inside the call: where the fused kernel measured slower than the two launches it replaces by more
 * than the +-3-4 % between boxes (tools/bench_intra_cand.py, profiles/r12_intra_cand.jsonl, profiles/HISTORY.md) the
 * call predicts into pred_out -- or, without one, into a buffer of the context -- and runs r1_rdo_txsearch_batch's
 * kernels on it, in the caller's stream: 16x16 with dist_kind 0 (every bit depth); at 10 / 12 bits also 16x16 and
 * 32x32 with R1_DIST_WSSE / R1_DIST_CDEF and 64x64 with dist_kind 0.  Same slots, same results, same pred_out; the
 * context keeps up to four such buffers (n * (16 + w * h * bytes per pixel) bytes each) until it is destroyed.
 * Every other size, bit depth and kind runs the fused kernel: faster than the two launches at 8x8 (2-5 %), within
 * the box variance elsewhere.
 * R1_EINVAL: everything r1_rdo_txsearch_batch rejects; edge_group < 1 or not dividing n; edge_stride < 257; a NULL
 * among cands / edges / lens / pos_xy; a UV_CFL_PRED candidate without `ac` -- checked where the host can read the
 * descriptors (host or pinned memory; the Python wrapper checks NumPy descriptors before it uploads them);
 * descriptors in device memory cannot be read without a synchronising copy, and there the kernel predicts such a
 * candidate's DC and never touches `ac`. */
int r1_rdo_intra_cand_batch(r1_ctx *ctx, const R1Plane *org, int w, int h, int tx_size,
                            const R1IntraCand *cands, int n, int edge_group, const int16_t *pos_xy,
                            const void *edges, int edge_stride, const uint8_t *lens, const int16_t *ac,
                            uint32_t tx_type_mask, const R1QuantParams *params, int dist_kind,
                            const uint32_t *scales, int scale_stride, int xdec, int ydec,
                            uint32_t *sad_out, uint32_t *satd_out, uint16_t *eob_out, uint64_t *dist_out,
                            uint64_t *est_rate_out, void *qcoeffs_out, void *rec_out, void *pred_out, void *stream);
/* ---- the intra transform-split candidate in ONE launch (added under ABI 7): rdo_tx_size_type (src/rdo.rs:725-802)
 * tries an intra block's largest transform, then one split, then two, each through rdo_tx_type_decision ->
 * write_tx_blocks (src/encoder.rs:2243-2311), which walks the block's transform blocks in raster order; each is
 * predicted from a reconstruction that already holds the ones before it (need_recon_pixel, rdo.rs:1729).  This call
 * runs that loop on the device for n blocks of bw x bh pixels coded with square tx_size transforms: the block's working
 * reconstruction stays in LDS between the steps, and `rec` is never written.
 *   cands:   one R1IntraSplitCand per block.  tr_mask / bl_mask are has_top_right / has_bottom_left per transform
 *            block -- decisions on the partition tree, which stay on the host as for R1IntraEdgeCand.flags.
 *   tile:    (tile_x, tile_y, tile_w, tile_h) in plane pixels, inside `rec`; block i lies at (tile_x + x, tile_y + y)
 *            of both planes.
 * A trial is (block i, slot j), slot j = the j-th set bit of tx_type_mask, nt = popcount (r1_rdo_txsearch_batch's
 * slots); its index is i * nt + j, and ntx = (bw / tw) * (bh / th) is the transform-block grid.  Let R be a private
 * copy of `rec`.  For each transform block k in raster order over the grid, at (x_k, y_k) relative to the tile --
 * skipped when its 4x4-unit origin is at or beyond (tile_w + 3) >> 2 or (tile_h + 3) >> 2 (encoder.rs:1441, 2282) --
 * the results are, bit for bit, those of
 *   r1_intra_edges_batch(R, tile, tx_size, {x_k, y_k, mode, angle_delta,
 *                        flags = enable_intra_edge_filter | tr_mask[k] << 1 | bl_mask[k] << 2})
 *   -> r1_predict_intra_batch with the R1IntraCand predict_intra (src/predict.rs:205-249) implies: the Paeth remap
 *      and `variant` by x_k == 0 / y_k == 0, angle = mode angle + 3 * angle_delta, the block's ief, avail_w / avail_h
 *      = min(transform side, plane size - position), at least 1
 *   -> r1_rdo_txsearch_batch(pred = that, tx_type_mask = 1 << t_j, is_intra quantizer) at (x_k, y_k)
 *   -> its reconstruction (rec_out of a pixel-domain kind; the prediction itself when eob == 0) stored into R.
 * Transform block k + 1 sees the results of 0 .. k; every trial starts from the same `rec`.
 * Outputs:
 *   eob_out[trial * ntx + k]          0 for a skipped transform block
 *   qcoeffs_out (optional)            coded-area blocks at [trial * ntx + k] (int16 at 8 bits, else int32); zeros for
 *                                     a skipped transform block
 *   rec_out (optional)                one dense bw x bh block per trial: R over the block behind the last step.  What
 *                                     no step wrote is `rec` inside the tile and 0 outside it.
 *   dist_kind 0                       dist_out[trial * ntx + k] (, est_rate_out[..], optional): the raw transform-
 *                                     domain distortion and table rate per transform block (0 when skipped);
 *                                     distortion_scale differs per transform block (encoder.rs:1654), so the host
 *                                     applies it, as it does for r1_rdo_full_cand_batch.  rec_out must be NULL.
 *   R1_DIST_WSSE / R1_DIST_CDEF       dist_out[trial]: what r1_dist_scaled_batch returns for `org` against that final
 *                                     block over bw x bh with the `scales` grid (xdec = ydec = 0).  est_rate_out must
 *                                     be NULL.
 * As with r1_rdo_intra_cand_batch a block cut by the frame edge is evaluated whole -- `org` must hold every transform
 * block that is not skipped, and for a pixel-domain kind the whole block, padding included -- and the caller gets the
 * reference's visible-part distortion (clip_visible_bsize) from rec_out through r1_dist_scaled_batch.
 * Built: square transforms 4x4, 8x8, 16x16, 32x32 on blocks up to 64x64 that they divide with 2 <= ntx <= 16 (both
 * split depths of every square and 2:1 block, depth 2 of the 4:1 blocks), bit depths 8 / 10 / 12, luma modes 0 .. 12
 * as write_tx_blocks receives them (NO Paeth remap by the caller).
 * NOT built: the 2:1 transform sizes (depth 1 of the 4:1 blocks) -- they stay on the host loop over the three calls
 * above; chroma (write_tx_blocks never splits it); a routing to a multi-launch fallback (every point runs the one
 * kernel).  The real coefficient rate across the transform blocks: r1_coeff_rate_chain_batch (order 0) behind this
 * call, on qcoeffs_out / eob_out as they lie.
 * R1_EINVAL: everything r1_rdo_txsearch_batch rejects for the size, mask and kind; a tx_size that is not one of the
 * four; bw / bh that the transform does not divide, that is no block size, or ntx of 1 or above 16; a tile that is not
 * inside `rec`; planes of different pixel formats; a NULL plane, cands, params, eob_out or dist_out; est_rate_out or
 * rec_out with the wrong kind; and, where the host can read the descriptors (host or pinned memory; the Python
 * wrapper checks NumPy descriptors before it uploads them), a mode above 12 or an x / y that is negative or no
 * multiple of 4.  Descriptors in device memory are not read by the host: there a mode above 12 predicts DC and a
 * negative position skips every transform block of the trial. */
typedef struct R1IntraSplitCand {
  int16_t x, y;          /* block position relative to the tile, multiples of 4 */
  uint8_t mode;          /* luma PredictionMode 0..12 as write_tx_blocks receives it: NO Paeth remap */
  int8_t  angle_delta;
  uint8_t ief;           /* as R1IntraCand.ief: one value per BLOCK (encoder.rs:1458-1469 uses tile_partition_bo) */
  uint8_t reserved;
  uint16_t tr_mask;      /* bit k: has_top_right(..)  of transform block k (raster index in the bw/tw x bh/th grid) */
  uint16_t bl_mask;      /* bit k: has_bottom_left(..) of transform block k */
} R1IntraSplitCand;
int r1_rdo_intra_split_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *rec,
    int tile_x, int tile_y, int tile_w, int tile_h, int bw, int bh, int tx_size,
    const R1IntraSplitCand *cands, int n, int enable_intra_edge_filter, uint32_t tx_type_mask,
    const R1QuantParams *params, int dist_kind, const uint32_t *scales, int scale_stride,
    uint16_t *eob_out, uint64_t *dist_out, uint64_t *est_rate_out,
    void *qcoeffs_out, void *rec_out, void *stream);
/* The mask of that loop: bit t set = TxType t is in av1_tx_used[get_tx_set(tx_size, is_inter,
 * use_reduced_set)]; rav1e_types_only != 0 keeps only RAV1E_TX_TYPES (DCT_DCT, ADST_DCT, DCT_ADST,
 * ADST_ADST, IDTX, V_DCT, H_DCT = 0x0E0F).  0 for an invalid tx_size.  Host arithmetic, no device work. */
uint32_t r1_tx_type_mask(int tx_size, int is_inter, int use_reduced_set, int rav1e_types_only);

/* ---- the real coefficient rate of the transform-type search on the device (added under ABI 7): per TxType
 * rdo_tx_type_decision (src/rdo.rs:1744-1799) makes a fresh WriterCounter (rng 0x8000, cnt -9, no bits), takes
 * tell_frac, writes the block, takes tell_frac again and rolls the CDFs back -- so every type of a block starts from
 * the same CDF state.  With one transform block per block that rate is the cost of write_coeffs_lv_map
 * (src/context/block_unit.rs:1783-2016), a pure function of the quantized coefficients, the block's two neighbour
 * contexts and the CDF state: integer arithmetic throughout.  This call computes it for every (candidate, type) slot
 * of r1_rdo_txsearch_batch / r1_rdo_intra_cand_batch / r1_rdo_pixel_cand_batch, chained on the same stream with no
 * copy, against CDF snapshots the host hands over.
 * The dimensions are the reference's (src/context/transform_unit.rs:27, 200-219). */
#define R1_TXB_SKIP_CONTEXTS 13
#define R1_EOB_COEF_CONTEXTS 9
#define R1_SIG_COEF_CONTEXTS_EOB 4
#define R1_SIG_COEF_CONTEXTS 42
#define R1_LEVEL_CONTEXTS 21
#define R1_BR_CDF_SIZE 4
#define R1_DC_SIGN_CONTEXTS 3
#define R1_INTRA_MODES 13
/* one (txs_ctx, plane_type) slice of the reference's CDFContext, in its own shapes
 * (src/context/cdf_context.rs:23-96); the host gathers it from its entropy state.  A CDF of N symbols is N entries:
 * N - 1 probabilities and the adaptation counter. */
typedef struct R1CoeffCdfs {
  uint16_t txb_skip[R1_TXB_SKIP_CONTEXTS][2];         /* txb_skip_cdf[txs_ctx] */
  uint16_t eob_flag[2][11];                           /* eob_flag_cdf{16..1024}[plane_type][eob_multi_ctx]; the first
                                                         5 + eob_multi_size entries of a row are the CDF */
  uint16_t eob_extra[R1_EOB_COEF_CONTEXTS][2];        /* eob_extra_cdf[txs_ctx][plane_type] */
  uint16_t coeff_base_eob[R1_SIG_COEF_CONTEXTS_EOB][3];
  uint16_t coeff_base[R1_SIG_COEF_CONTEXTS][4];
  uint16_t coeff_br[R1_LEVEL_CONTEXTS][R1_BR_CDF_SIZE]; /* coeff_br_cdf[min(txs_ctx, TX_32X32)][plane_type] */
  uint16_t dc_sign[R1_DC_SIGN_CONTEXTS][2];
  uint16_t tx_type[R1_INTRA_MODES][16];               /* the table write_tx_type would use for this (tx_size, is_inter,
                                                         reduced set): row = y_mode for intra, row 0 for inter; the
                                                         first num_tx_set[set] entries of a row are the CDF */
} R1CoeffCdfs;
typedef struct R1TxbCtx { uint8_t txb_skip_ctx, dc_sign_ctx, y_mode, cdf_sel; } R1TxbCtx;   /* 4 bytes */
/*   qcoeffs / eobs: n * nt dense coded-area blocks (coeff_bytes 2 = i16 for 8-bit, 4 = i32 otherwise) and n * nt
 *                   entries, slot [i * nt + j] = candidate i with the j-th set bit of tx_type_mask (nt = its
 *                   popcount): the layout the candidate calls write.  A single-type call is a mask of one bit.
 *   ctxs[i]:        candidate i's contexts (BlockContext::get_txb_ctx, block_unit.rs:442-526; y_mode is read for an
 *                   intra luma block only but must be < 13); cdfs[ctxs[i].cdf_sel] is the snapshot it starts from,
 *                   cdf_sel < n_cdfs <= 256.  How stale a snapshot may be -- per frame, tile or superblock -- is
 *                   the host's choice.
 *   rate_out[i * nt + j] = wr.tell_frac() - tell of a fresh WriterCounter after write_coeffs_lv_map, in 1/8 bit
 *                   (OD_BITRES = 3): the txb_skip symbol; for eob > 0 also write_tx_type when plane == 0, the eob,
 *                   the levels in av1_scan_orders[tx_size][tx_type] with their contexts (tx_class, txs_ctx =
 *                   get_txsize_entropy_ctx, eob_multi_size = area_log2 - 4, the coded size of the 64-point sizes),
 *                   the signs and Golomb tails.  Every slot starts from an UNADAPTED copy of its snapshot and adapts
 *                   it symbol by symbol as update_cdf does (src/ec.rs:935-955); `cdfs` is never written.
 *   cul_level_out (optional): n * nt bytes, the value write_coeffs_lv_map hands set_coeff_context: min(63, sum |c|)
 *                   with set_dc_sign applied, 0 for eob == 0 -- what the host stores for the winner.
 * R1_EINVAL (what the host can check): a NULL required pointer, coeff_bytes not 2 / 4, an invalid tx_size, an empty
 * mask or one with bits outside r1_tx_type_mask(tx_size, is_inter, use_reduced_tx_set, 0), n_cdfs outside 1..256,
 * plane outside 0..2.  Device-resident data cannot be checked there: a slot whose eob exceeds the coded area, whose
 * txb_skip_ctx / dc_sign_ctx / y_mode is out of range or whose cdf_sel >= n_cdfs gets rate 0xFFFFFFFF and cul_level 0,
 * and nothing is read out of bounds.  Every loop of the kernel is bounded independently of the data's values.
 * Blocks that write_tx_tree / write_tx_blocks code as several transform blocks: r1_coeff_rate_chain_batch below.
 * Snapshots cut on the device from a context that carries the winners' adaptation: r1_coeff_cdf_slice_batch below.
 * OUT OF SCOPE: every non-coefficient symbol (modes, motion vectors, partition, count_lrf_switchable). */
int r1_coeff_rate_batch(r1_ctx *ctx, const void *qcoeffs, int coeff_bytes, const uint16_t *eobs, int n,
                        uint32_t tx_type_mask, int tx_size, int plane, int is_inter, int use_reduced_tx_set,
                        const R1TxbCtx *ctxs, const R1CoeffCdfs *cdfs, int n_cdfs, uint32_t *rate_out,
                        uint8_t *cul_level_out, void *stream);

/* ---- the real coefficient rate across a block's transform blocks (added under ABI 7): rdo_tx_size_type
 * (src/rdo.rs:725-802) compares transform depths by compute_rd_cost(rate, distortion) with rate = wr.tell_frac() - tell
 * around ONE write_tx_blocks (intra) or write_tx_tree (inter) call with luma_only = true (src/rdo.rs:1744-1799): nothing
 * but write_coeffs_lv_map over the block's luma transform blocks in raster order, on one WriterCounter, with the CDFs
 * adapted by every symbol of the blocks before and the neighbour contexts set_coeff_context stored for them.  This call
 * computes that rate for every (block, type) trial behind the launch that made the coefficients, with no copy.
 *   trial (i, j):   block i with the j-th set bit of tx_type_mask, as the slots of r1_coeff_rate_batch (nt = popcount).
 *   grid:           ntx = (bw / tw) * (bh / th) transform blocks in raster order, 1 <= ntx <= 16.
 *   order:          where transform block k of trial (i, j) lies in qcoeffs (dense coded-area blocks) / eobs:
 *                   0: at (i * nt + j) * ntx + k -- what r1_rdo_intra_split_batch writes;
 *                   1: at (i * ntx + k) * nt + j -- what r1_rdo_txsearch_batch writes when its candidates are the
 *                      transform blocks of the blocks, block after block.
 *   chains[i]:      the block's state in front (R1TxbChainCtx); cdfs[chains[i].cdf_sel] is the snapshot every trial of
 *                   the block starts from, unadapted.
 * Per coded transform block, in raster order, what write_coeffs_lv_map does (block_unit.rs:1783-1857): get_txb_ctx
 * (442-526, luma; txb_skip_ctx is 0 when ntx == 1) over the first frame_clipped_txw >> 2 / txh >> 2 entries; the symbols,
 * every row they touch adapted for the blocks behind (update_cdf with the row's own length, src/ec.rs:935-955);
 * set_coeff_context over the FULL tw / 4, th / 4 span with cul_level, or 0 for eob == 0.  A transform block whose origin
 * lies at or beyond mi_w / mi_h is not coded (encoder.rs:2282, 2446).
 *   rate_out[i * nt + j]:   tell_frac behind the last block minus the fresh counter's, 1/8 bit.
 *   txb_rate_out (optional) [trial * ntx + k]: tell_frac behind block k minus tell_frac in front of it; 0 for a block
 *                   that is not coded; the values of a trial sum to its rate_out.
 *   cul_level_out (optional) [trial * ntx + k].
 *   ctx_out (optional): 32 bytes per trial, `above` and `left` behind the last block: what the host stores for the
 *                   winner.
 * `cdfs` and the inputs are never written.  With ntx == 1 the numbers are r1_coeff_rate_batch's.
 * In scope: plane 0, all 19 transform sizes, bw, bh <= 64, coefficient widths 2 and 4.
 * R1_EINVAL: everything r1_coeff_rate_batch refuses (chains in place of ctxs), a transform that does not divide the
 * block, ntx outside 1..16, order outside 0..1, bw or bh that is no block size.  Device-resident data the host cannot
 * see -- an eob above the coded area in any coded transform block, y_mode >= 13, cdf_sel >= n_cdfs, mi_w > clip_w4 or
 * mi_h > clip_h4 -- gives the trial rate 0xFFFFFFFF and zero side outputs; nothing is read or written out of bounds.
 * `above` / `left` bytes hold what set_coeff_context stores (below 192); a sign field of 3 counts as no sign.
 * Every loop is bounded by ntx, the coded area, the four base-range rounds or the Golomb length.
 * The chroma half of write_tx_blocks / write_tx_tree (other R1CoeffCdfs slices, U then V behind luma on the same
 * writer): r1_coeff_rate_block_batch below.
 * The adapted CDFs are dropped here; r1_coeff_cdf_adapt_batch below keeps a block's winner's on a device-resident context.
 * OUT OF SCOPE: every non-coefficient symbol; making the serial range-coder chain itself faster. */
typedef struct R1TxbChainCtx {          /* 40 bytes */
  uint8_t above[16];   /* above_coeff_context[0][bo.x + c], c < bw / 4: the state in front of the block */
  uint8_t left[16];    /* left_coeff_context[0][bo.y_in_sb() + r], r < bh / 4 */
  uint8_t mi_w, mi_h;  /* min(255, ts.mi_width - bo.x), min(255, ts.mi_height - bo.y) */
  uint8_t clip_w4, clip_h4; /* min(255, fi.w_in_b - frame_bo.x), same for h: frame_clipped_txw >> 2 =
                          min(tw / 4, clip_w4 - x4) for the transform block at 4x4-unit origin (x4, y4) of the block
                          (encoder.rs:1561-1566) */
  uint8_t y_mode, cdf_sel, reserved[2];
} R1TxbChainCtx;
int r1_coeff_rate_chain_batch(r1_ctx *ctx, const void *qcoeffs, int coeff_bytes, const uint16_t *eobs, int n,
                              uint32_t tx_type_mask, int bw, int bh, int tx_size, int order, int is_inter,
                              int use_reduced_tx_set, const R1TxbChainCtx *chains, const R1CoeffCdfs *cdfs, int n_cdfs,
                              uint32_t *rate_out, uint32_t *txb_rate_out, uint8_t *cul_level_out, uint8_t *ctx_out,
                              void *stream);

/* ---- the real coefficient rate of a whole block: luma, U, V on one writer (added under ABI 7): the mode decision
 * (luma_chroma_mode_rdo, src/rdo.rs:855-945) makes a fresh WriterCounter per candidate, writes a handful of head symbols
 * (partition, skip, segment, modes, angle deltas, CFL alphas, tx size) and ends in ONE write_tx_blocks (intra) or
 * write_tx_tree (inter, skip = false) call with luma_only = false (src/encoder.rs:2202-2240): write_coeffs_lv_map over
 * the block's luma transform blocks, then U's, then V's, on that same writer.  This call computes the rate of that
 * coefficient part for every trial, behind the launches that made the coefficients, with no copy.
 * The hand-over: the head symbols use CDFs the coefficients never touch, and for a counting writer tell_frac behind any
 * continuation depends on the state in front through `rng` alone (total bits = a sum of per-symbol shifts plus a
 * constant).  The host writes the head on its own counter and hands over the writer's rng; then
 *     rate_out + (host tell_frac at the hand-over - tell_frac of the fresh counter)
 * is the reference's number.  rng = 0x8000 is the fresh writer.
 * Two snapshots per trial: luma and chroma rows of CDFContext are disjoint (indexed by plane_type; txb_skip is shared by
 * txs_ctx, but luma reads rows 0-6 and chroma 7-12), so cdfs[cdf_sel] is the luma slice as r1_coeff_rate_chain_batch
 * takes it and cdfs[cdf_sel_uv] the (txs_ctx(uv_tx_size), plane_type 1) slice; each is copied and adapts symbol by
 * symbol, U adapts the second and V continues on it.  `cdfs` is never written.
 *   grid:        luma ntx = (bw / tw) * (bh / th) in raster order, 1..16, as r1_coeff_rate_chain_batch.  Chroma:
 *                uv_tx_size = largest_chroma_tx_size(bsize, xdec, ydec) and the grid of src/encoder.rs:2327-2338 /
 *                2492-2505, integer divisions and the `== 0 -> 1` rule included (4x16 and 16x4 in 4:2:0 code NO chroma
 *                transform block); ntx_uv <= 4.  (xdec, ydec): (1, 1), (1, 0) or (0, 0).
 *   arrays:      transform block k of a trial's plane lies at first + k * step (dense coded-area blocks in qcoeffs_*, one
 *                entry in eobs_*): step_y 1 reads what r1_rdo_intra_split_batch left, step_y nt what
 *                r1_rdo_txsearch_batch left; several trials may name the same luma blocks.  n_txb_y / n_txb_uv: how
 *                many transform blocks the luma arrays and EACH chroma array hold.  The four chroma arrays may all be
 *                NULL when no trial has do_chroma.
 *   trials[t]:   R1BlockRateTrial, device resident.  uv_tx_type is an input: whatever the launch that made the chroma
 *                coefficients used (uv_intra_mode_to_tx_type_context or DCT_DCT for intra; tx_type.uv_inter(..), or
 *                DCT_DCT when luma had no coefficient, for inter).  do_chroma: has_chroma(..) and not Cs400.
 *   blocks[b]:   R1BlockChainCtx, device resident: R1TxbChainCtx widened to three planes.
 * Per plane, per coded transform block what r1_coeff_rate_chain_batch does; for chroma: a transform block is coded iff
 * its LUMA-unit origin lies inside mi_w / mi_h (encoder.rs:1441), get_txb_ctx takes the chroma arm (txb_skip_ctx =
 * (top != 0) + (left != 0) + 10 when the plane's block has more pixels than the transform, else + 7), write_tx_type is
 * not written, set_coeff_context covers the chroma transform's full span.
 *   rate_out[t]:        tell_frac behind the last block minus tell_frac of the start state, 1/8 bit.
 *   plane_rate_out (optional) [t * 3 + p]: the same per plane; the three sum to rate_out[t].
 *   rng_out (optional) [t]: the writer's rng behind the last block.
 *   cul_level_out (optional) [(t * 3 + p) * 16 + k]: per plane and transform block; 0 for a block that is not coded.
 *   ctx_out (optional): 96 bytes per trial, R1BlockChainCtx.ctx behind the last block.
 * A trial with do_chroma = 0 and rng = 0x8000 returns r1_coeff_rate_chain_batch's numbers.
 * R1_EINVAL (what the host can see): a NULL required pointer (chroma arrays: all four or none), coeff_bytes not 2 / 4, a
 * bad tx_size, bw / bh that is no block size up to 64x64 or that the subsampling does not admit, a transform that does
 * not divide the block, ntx outside 1..16, (xdec, ydec) outside the three pairs, a step < 1, n_blocks < 1, n_cdfs
 * outside 1..256, n_txb_* < 0.  Device-resident faults give that trial rate 0xFFFFFFFF and zero side outputs, with
 * nothing read or written out of bounds: block >= n_blocks, tx_type outside the set of (tx_size, is_inter, reduced),
 * do_chroma with a uv_tx_type the chroma size has no scan for (32-point sides: DCT_DCT and IDTX only) or, where the
 * chroma grid is not empty, with NULL chroma arrays, a `first` whose last transform block lies beyond n_txb_*, an eob
 * above the coded area in a coded transform block, y_mode >= 13, cdf_sel / cdf_sel_uv >= n_cdfs, rng < 0x8000, mi_w > clip_w4 or mi_h > clip_h4, a coded chroma
 * transform block at or beyond clip_uv_w4 / clip_uv_h4.
 * Every loop is bounded by ntx, the coded area, the four base-range rounds or the Golomb length; no spin-waits, no atomics.
 * The adapted CDFs are dropped here: r1_coeff_cdf_adapt_batch below replays the winner on a device-resident
 * R1CoeffCdfContext and leaves it adapted; r1_coeff_cdf_slice_batch cuts this call's `cdfs` out of one.
 * OUT OF SCOPE: the head symbols themselves (the host's dozen, or for intra frames r1_intra_head_rate_batch below,
 * which stores the rng this call starts from into `trials`); skip = true (no coefficient
 * is written); making the serial range-coder chain itself faster. */
typedef struct R1BlockChainCtx {        /* 108 bytes */
  uint8_t ctx[3][2][16];  /* [plane][0: above, 1: left][16]: above_coeff_context[p][(tx_bo.x >> xdec) + c] and
                             left_coeff_context[p][(tx_bo.y_in_sb() >> ydec) + r] in front of the block, tx_bo = the
                             plane's FIRST transform block: the block's offset, for chroma less the one-unit shift of a
                             4-wide / 4-high block (encoder.rs:2365-2368) */
  uint8_t mi_w, mi_h, clip_w4, clip_h4;   /* as R1TxbChainCtx */
  uint8_t clip_uv_w4, clip_uv_h4;  /* min(255, (((fi.w_in_b - frame_bo.x) << 2) >> xdec) >> 2) for the first chroma
                             transform block's frame_bo, same for h: frame_clipped_txw >> 2 of chroma transform block
                             (bx, by) = min(uv_tw / 4, clip_uv_w4 - bx * uv_tw / 4) (encoder.rs:1561-1566) */
  uint8_t y_mode, cdf_sel, cdf_sel_uv, reserved[3];
} R1BlockChainCtx;
typedef struct R1BlockRateTrial {       /* 24 bytes */
  uint32_t first_y, first_u, first_v;   /* the trial's first transform block in qcoeffs_y / _u / _v and eobs_* */
  uint32_t block;                       /* index into blocks */
  uint16_t rng;                         /* the writer's rng in front: 0x8000..0xFFFF */
  uint8_t tx_type, uv_tx_type, do_chroma, reserved[3];
} R1BlockRateTrial;
int r1_coeff_rate_block_batch(r1_ctx *ctx, const void *qcoeffs_y, const uint16_t *eobs_y, int n_txb_y, int step_y,
                              const void *qcoeffs_u, const uint16_t *eobs_u, const void *qcoeffs_v,
                              const uint16_t *eobs_v, int n_txb_uv, int step_uv, int coeff_bytes,
                              const R1BlockRateTrial *trials, int n, int bw, int bh, int tx_size, int xdec, int ydec,
                              int is_inter, int use_reduced_tx_set, const R1BlockChainCtx *blocks, int n_blocks,
                              const R1CoeffCdfs *cdfs, int n_cdfs, uint32_t *rate_out, uint32_t *plane_rate_out,
                              uint16_t *rng_out, uint8_t *cul_level_out, uint8_t *ctx_out, void *stream);

/* ---- the decision on the device (added under ABI 7): what the reference does with the rate and the distortion of
 * every trial -- compute_rd_cost (src/rdo.rs:718-723), the tail of rdo_tx_type_decision's loop (1801-1818), the carry
 * across the transform depths in rdo_tx_size_type (780-784) and `rd < best.rd_cost` in luma_chroma_mode_rdo (923-938) --
 * behind the candidate and rate launches on the same stream, with no copy and no synchronisation.  A block's decision
 * is an R1RdPick that is carried from call to call; r1_rd_commit_batch then moves the winner's results to where the
 * next step reads them.  All pointers are DEVICE pointers.
 *   state s owns rows s * group .. s * group + group - 1; trial (row r, slot j) is entry [(s * group + r) * nt + j] of
 *   rate, dist and the optional rate_add: the slot layout every candidate call and every rate call writes.
 * Trials are visited rows ascending, slots ascending, and each costs
 *   rd = fma(lambda, (double)(rate + rate_add) / 8.0, (double)dist)
 * in ONE rounding, as f64::mul_add: rate / 8 is exact and the u64 -> f64 conversion rounds to nearest even, as Rust's
 * `as f64`.  A slot whose rate is 0xFFFFFFFF (the rate calls' refusal value), or whose 64-bit sum with rate_add reaches
 * it, is invalid: it costs +infinity and sets invalid_out[s] = 1 (optional; otherwise written 0), whether or not the
 * rule below looks at the slot.
 *   R1_PICK_FIRST_MIN: a trial is kept when rd < state.best_rd, strictly: a tie keeps the earlier trial, one kept by an
 *                      earlier call included.  The mode loop (rate_add = the head's tell_frac difference that
 *                      r1_coeff_rate_block_batch tells the host to add) and the depth carry of rdo_tx_size_type.
 *   R1_PICK_TX_TYPE:   (group == 1) rdo_tx_type_decision's loop: cur_best_rd = state.best_rd on entry; when the FIRST
 *                      slot's rd > cur_best_rd nothing of this call is kept -- later slots are not considered, even one
 *                      below cur_best_rd; otherwise the call's own first minimum (strict < from f64::MAX) is taken and
 *                      kept when it is < state.best_rd (rdo.rs:780).  rdo_glue.pick_tx_type is the statement.
 * A kept trial writes all six fields with best_call = call_id; a state of which nothing is kept is not written.  The
 * three depths of a block are three calls with call_id 0, 1, 2 on the same state array, each behind its search and
 * rate launches.
 * A pick over picks (the mode loop over the states the depth calls left: rate = their best_rate, dist = their best_dist,
 * gathered) is the CALLER's to guard: a state that kept nothing holds rate 0 and distortion 0 and would cost its
 * rate_add alone.  Hand such a trial the rate 0xFFFFFFFF (best_call < 0 tells), and it costs +infinity.
 * R1_EINVAL: a NULL rate, dist or state; n_states < 0; group outside 1..4096; nt outside 1..16; group * nt > 4096; rule
 * outside 0..1; R1_PICK_TX_TYPE with group != 1; call_id outside 0..127; a lambda that is negative, infinite or NaN.
 * n_states == 0 returns 0 and touches nothing. */
typedef struct R1RdPick {      /* 24 bytes; the decision state of one block, carried from call to call */
  double   best_rd;            /* f64::MAX (DBL_MAX) = nothing kept yet */
  uint64_t best_dist;          /* the kept trial's distortion (is_zero_dist, rdo.rs:922) */
  uint32_t best_rate;          /* its rate, rate_add included, 1/8 bit */
  int16_t  best_row;           /* row inside the state's group in the winning call, -1 = none */
  int8_t   best_slot;          /* slot j of the winning call, -1 = none */
  int8_t   best_call;          /* call_id of the winning call, -1 = none */
} R1RdPick;
#define R1_PICK_FIRST_MIN 0    /* luma_chroma_mode_rdo / rdo_tx_size_type: keep on rd < best_rd */
#define R1_PICK_TX_TYPE   1    /* rdo_tx_type_decision's loop, early exit included; needs group == 1 */
int r1_rd_pick_batch(r1_ctx *ctx, const uint32_t *rate, const uint32_t *rate_add, const uint64_t *dist,
                     int n_states, int group, int nt, double lambda, int rule, int call_id,
                     R1RdPick *state, uint8_t *invalid_out, void *stream);
/* The winner's results where the next step reads them.  The call acts for every state s with
 * state[s].best_call == call_id; a state won by another call, or by none, has NOTHING of its outputs written, so the
 * commits of the three depths fill disjoint blocks of the same outputs.  Let t = (s * group + best_row) * nt + best_slot.
 * Three parts, each present whole (its inputs and outputs non-NULL) or absent (all NULL):
 *   eobs / qcoeffs -> eob_win / qcoeffs_win: transform block k < ntx of trial t lies at t * ntx + k for order 0 (the
 *       layout of r1_rdo_intra_split_batch, and of one block per trial) and, with group == 1 and order 1, at
 *       (s * ntx + k) * nt + best_slot -- the two orders of r1_coeff_rate_chain_batch.  Its eob goes to
 *       eob_win[s * 16 + k], its coded_area coefficients of coeff_bytes (2 or 4) each to element
 *       s * win_stride + k * coded_area of qcoeffs_win; win_stride >= ntx * coded_area.  Both coefficient arrays are
 *       aligned to coeff_bytes, as arrays of that type are; where both are 16-byte aligned and win_stride * coeff_bytes
 *       is a multiple of 16 the blocks move in 16-byte pieces.
 *   side -> side_win: side_bytes (1..128) bytes per trial at t * side_bytes go to side_win + s * side_bytes: ctx_out of
 *       the chain or block rate call, or cul_level.
 *   rec_trials -> rec: the dense bw x bh block of trial t in the plane's pixel type (rec_out of the candidate calls;
 *       the array 16-byte aligned) goes to `rec` at (pos_xy[2s], pos_xy[2s + 1]), clipped to [0, store_w) x
 *       [0, store_h): nothing outside that rectangle and nothing outside the plane's allocation is written.  The blocks
 *       of one call MUST NOT overlap: overlapping pixels would be stored in no defined order.
 * R1_EINVAL: a part with only some of its pointers; n_states < 0; group / nt / call_id as for the pick; ntx outside
 * 1..16; order outside 0..1, or 1 with group != 1; coeff_bytes not 2 or 4; coded_area outside 16..1024; win_stride
 * below ntx * coded_area; side_bytes outside 1..128; bw / bh that are no block size up to 64x64; a plane whose
 * bytes_per_px / bit_depth are not 1 / 8 or 2 / 10, 12; store_w above stride - xorigin or store_h above alloc_height -
 * yorigin (the visible plane plus its right and bottom padding as the allocation holds it), or negative; and two
 * alignments the kernel's loads rest on: rec_trials not 16-byte aligned (the dense blocks are read in 16-byte pieces;
 * rec_out of the candidate calls is), qcoeffs or qcoeffs_win not aligned to coeff_bytes.  n_states == 0 returns 0.
 * Device-resident faults: a best_row >= group or best_slot >= nt found in the state writes nothing for that state;
 * every loop is bounded by the arguments, never by data.  No atomics, no spin-waits. */
int r1_rd_commit_batch(r1_ctx *ctx, const R1RdPick *state, int n_states, int call_id, int group, int nt,
                       int ntx, int order, int coded_area, int coeff_bytes,
                       const uint16_t *eobs, const void *qcoeffs, const void *side, int side_bytes,
                       const void *rec_trials, int bw, int bh, const R1Plane *rec, const int16_t *pos_xy,
                       int store_w, int store_h,
                       uint16_t *eob_win, void *qcoeffs_win, int win_stride, void *side_win, void *stream);

/* ---- the adapted coefficient CDFs carried from block to block on the device (added under ABI 7): the rate calls
 * above start from R1CoeffCdfs snapshots and never write them, so a host that wants block k + 1 measured against what
 * block k's winner left would have to download the winner, adapt its own CDFContext and upload fresh slices.  These two
 * calls keep the state on the device instead: a context holds the coefficient side of the reference's CDFContext,
 * r1_coeff_cdf_slice_batch cuts the slices the rate calls take out of it, and r1_coeff_cdf_adapt_batch replays a
 * block's winner on it and leaves it adapted.  Per block, on one stream with nothing read back:
 *     slice -> rates (cdf_sel = the context's index) -> pick -> commit -> adapt (gated by the pick's state).
 * A rollback (rdo_partition_decision codes sub-block after sub-block and rolls everything back) is the caller's
 * device copy of the struct.  Head symbols use CDFs the coefficients never touch: R1HeadCdfContext, further down.
 * R1CoeffCdfContext: every field write_coeffs_lv_map and write_tx_type can touch, in the reference's shapes
 * (src/context/cdf_context.rs:23-96; [TxSize::TX_SIZES = 5][PLANE_TYPES = 2], TX_SIZE_SQR_CONTEXTS = 4), so a host
 * fills it field by field.  The padding is never read and never written. */
typedef struct R1CoeffCdfContext {      /* 7872 bytes */
  uint16_t txb_skip[5][R1_TXB_SKIP_CONTEXTS][2];
  uint16_t eob_extra[5][2][R1_EOB_COEF_CONTEXTS][2];
  uint16_t coeff_base_eob[5][2][R1_SIG_COEF_CONTEXTS_EOB][3];
  uint16_t coeff_base[5][2][R1_SIG_COEF_CONTEXTS][4];
  uint16_t coeff_br[5][2][R1_LEVEL_CONTEXTS][R1_BR_CDF_SIZE];
  uint16_t dc_sign[2][R1_DC_SIGN_CONTEXTS][2];
  uint16_t eob_flag16[2][2][5];
  uint16_t eob_flag32[2][2][6];
  uint16_t eob_flag64[2][2][7];
  uint16_t eob_flag128[2][2][8];
  uint16_t eob_flag256[2][2][9];
  uint16_t eob_flag512[2][2][10];
  uint16_t eob_flag1024[2][2][11];
  uint16_t intra_tx_1[4][R1_INTRA_MODES][7];
  uint16_t intra_tx_2[4][R1_INTRA_MODES][5];
  uint16_t inter_tx_1[4][16];
  uint16_t inter_tx_2[4][12];
  uint16_t inter_tx_3[4][2];
  uint16_t pad[6];                      /* to a multiple of 16 bytes */
} R1CoeffCdfContext;
/* slices_out[i] = the R1CoeffCdfs slice of contexts[i] that the three rate calls take for (tx_size, plane_type,
 * is_inter, use_reduced_tx_set), i < n: txs_ctx = get_txsize_entropy_ctx(tx_size); txb_skip[txs_ctx];
 * eob_flag{16 << min(area_log2 - 4, 6)}[plane_type]; eob_extra, coeff_base_eob, coeff_base[txs_ctx][plane_type];
 * coeff_br[min(txs_ctx, 3)][plane_type]; dc_sign[plane_type]; for plane_type 0 and a set of more than one type, the
 * table of get_tx_set_index at tx_size.sqr(): all 13 rows of intra_tx_1 / intra_tx_2, or row 0 from inter_tx_1 / 2 / 3.
 * Every slice entry the rule does not fill -- the tail of a row past its CDF's length, tx_type for chroma or a one-type
 * set -- is written 0.  `contexts` is never written.
 * R1_EINVAL: a NULL pointer, n < 0, an invalid tx_size, plane_type outside 0..1.  n == 0 returns 0. */
int r1_coeff_cdf_slice_batch(r1_ctx *ctx, const R1CoeffCdfContext *contexts, int n, int tx_size, int plane_type,
                             int is_inter, int use_reduced_tx_set, R1CoeffCdfs *slices_out, void *stream);
/* The winner's replay.  The coefficient, trial and block arguments are r1_coeff_rate_block_batch's, with the same
 * addressing (first + k * step), so the call reads trial arrays or r1_rd_commit_batch's winner arrays: with
 * win_stride = 16 * coded_area, transform block k of state s lies at s * 16 + k of both eob_win and qcoeffs_win
 * (first_y = s * 16, step_y = 1).  In place of cdfs / n_cdfs -- and of blocks[].cdf_sel / cdf_sel_uv, which are ignored
 * -- trial t reads and adapts contexts[t], in place: one context per trial, no two trials share one.
 *   state / call_id (optional gate): with state non-NULL, trial t acts only when state[t].best_call == call_id;
 *                otherwise NOTHING of trial t is written, neither its context nor any output -- the pattern of
 *                r1_rd_commit_batch, so the calls of the three depths fill disjoint contexts.
 * Per acting trial what r1_coeff_rate_block_batch does, on the luma slice of contexts[t] (the rule above), then the
 * chroma one; what the slice holds behind the luma plane is written back to the context, and again behind V.  A plane
 * writes only the rows it owns: luma txb_skip[txs_ctx] rows 0-6, everything indexed by plane type 0 and the tx-type
 * table; chroma txb_skip[txs_ctx(uv)] rows 7-12 and everything indexed by plane type 1.  Every other entry of the
 * context stays bit-identical.
 *   rate_out (optional) [t]: what r1_coeff_rate_block_batch returns for the trial on the slices cut from contexts[t].
 *   rng_out (optional) [t], ctx_out (optional, 96 bytes per trial): as there.
 * R1_EINVAL: what r1_coeff_rate_block_batch refuses on the host (less cdfs, n_cdfs and rate_out), a NULL contexts, a
 * call_id outside 0..127 with state given.  A trial with one of that call's device-resident faults (less the cdf_sel
 * ones) leaves contexts[t] untouched and gets rate 0xFFFFFFFF and zero side outputs.
 * Every loop is bounded as there; no atomics, no spin-waits, one wave per trial.
 * OUT OF SCOPE: head-symbol CDFs; skip = true; several winners per context in one launch. */
int r1_coeff_cdf_adapt_batch(r1_ctx *ctx, const void *qcoeffs_y, const uint16_t *eobs_y, int n_txb_y, int step_y,
                             const void *qcoeffs_u, const uint16_t *eobs_u, const void *qcoeffs_v,
                             const uint16_t *eobs_v, int n_txb_uv, int step_uv, int coeff_bytes,
                             const R1BlockRateTrial *trials, int n, int bw, int bh, int tx_size, int xdec, int ydec,
                             int is_inter, int use_reduced_tx_set, const R1BlockChainCtx *blocks, int n_blocks,
                             R1CoeffCdfContext *contexts, const R1RdPick *state, int call_id, uint32_t *rate_out,
                             uint16_t *rng_out, uint8_t *ctx_out, void *stream);

/* ---- the coefficient neighbour contexts carried from block to block on the device (added under ABI 7):
 * R1BlockChainCtx.ctx / R1TxbChainCtx.above, left are cuts from BlockContext::above_coeff_context / left_coeff_context
 * (src/context/block_unit.rs:237-238) as they stand in front of a block, and what a block leaves there --
 * set_coeff_context with the winner's cul_level -- is known on the device alone.  These calls keep the arrays on the
 * device: a context holds them for one tile (or one speculative branch of one), r1_coeff_nbr_gather_batch cuts the
 * records the rate calls take, r1_coeff_nbr_store_batch writes back what the winner left.  With the CDF context above, a
 * tile's blocks are enqueued in coding order on one stream with nothing read back:
 *     gather -> search -> slice -> rates -> pick -> commit -> winner tx type -> adapt -> store.
 * A fresh tile is the struct zeroed (BlockContext::new); a rollback (rdo_partition_decision) is the caller's device copy
 * of the struct, as for R1CoeffCdfContext -- the reference's 16-entry checkpoint window restores nothing a whole copy
 * would not.  The above_tx_context / partition contexts and the head symbols have a context pair of their own
 * (R1HeadNbrContext / R1HeadCdfContext, further down); the partition decision is r1_rd_partition_pick_batch. */
#define R1_COEFF_NBR_WIDTH 1024            /* COEFF_CONTEXT_MAX_WIDTH = MAX_TILE_WIDTH / MI_SIZE (block_unit.rs:36) */
typedef struct R1CoeffNbrContext {         /* 3120 bytes: one per tile, or per speculative branch of one */
  uint8_t above[3][R1_COEFF_NBR_WIDTH];    /* above_coeff_context[p][x >> xdec_p] */
  uint8_t left[3][16];                     /* left_coeff_context[p][y_in_sb >> ydec_p] */
} R1CoeffNbrContext;
typedef struct R1NbrBlock {                /* 20 bytes, device resident: a block's place; static geometry the host knows */
  uint32_t nbr;                            /* which context */
  uint16_t bo_x, bo_y;                     /* tile block offset, 4x4 units */
  uint16_t mi_width, mi_height;            /* the tile's (ts.mi_width / mi_height) */
  uint16_t w_in_b, h_in_b;                 /* fi.w_in_b / h_in_b less the tile's own block offset in the frame */
  uint8_t y_mode, cdf_sel, cdf_sel_uv;     /* copied into the records */
  uint8_t flags;                           /* bit 0: do_chroma (has_chroma(..) and not Cs400); bit 1: skip.  The gather
                                              reads neither */
} R1NbrBlock;
/* blocks_out[i] (optional) = the R1BlockChainCtx of the bw x bh block descs[i] on contexts[descs[i].nbr], i < n:
 * ctx[0] = above[0][bo_x ..] / left[0][bo_y % 16 ..]; ctx[1], ctx[2] from the first chroma transform block's offset --
 * ((bo_x - ax) >> xdec, ((bo_y - ay) % 16) >> ydec) with ax = xdec for a 4-wide block, ay = ydec for a 4-high one
 * (encoder.rs:2364-2369); sixteen entries each, zeros where a window runs past entry 1023 or past left[15] (and
 * throughout where a shifted chroma column would be -1).  mi_w / mi_h = min(255, mi_width - bo_x), ..; clip_w4 / clip_h4
 * = min(255, max(0, w_in_b - bo_x)), ..; clip_uv_w4 = min(255, max(0, (((w_in_b - (bo_x - ax)) << 2) >> xdec) >> 2)),
 * same for h; y_mode, cdf_sel, cdf_sel_uv copied; reserved 0.  rdo_glue.block_chain_ctx is the statement.
 * chains_out[i] (optional) = the R1TxbChainCtx of the same block (rdo_glue.txb_chain_ctx): the luma rows and clamps.
 * At least one output is given.  Many descs may name one context (the K modes of a block); `contexts` is never written.
 * A desc the device must refuse -- nbr >= n_contexts, bo_x >= 1024, y_mode >= 13, mi_width <= bo_x, mi_height <= bo_y --
 * gets an all-zero record with y_mode = 255, which every rate call answers with rate 0xFFFFFFFF.
 * R1_EINVAL: a NULL ctx, contexts or descs, both outputs NULL, n < 0, n_contexts < 1, bw / bh that are no block size up
 * to 64x64 or that the subsampling does not admit, (xdec, ydec) outside (1, 1), (1, 0), (0, 0).  n == 0 returns 0.
 * Eight lanes per desc; aligned dwords with a byte shift where contexts and outputs are 4-byte aligned, bytes otherwise. */
int r1_coeff_nbr_gather_batch(r1_ctx *ctx, const R1CoeffNbrContext *contexts, int n_contexts, const R1NbrBlock *descs,
                              int n, int bw, int bh, int xdec, int ydec, R1BlockChainCtx *blocks_out,
                              R1TxbChainCtx *chains_out, void *stream);
/* What a coded or a skipped winner leaves on contexts[descs[i].nbr].  ctx_in + 96 * i is the R1BlockChainCtx.ctx BEHIND
 * block i: ctx_out of r1_coeff_rate_block_batch / r1_coeff_cdf_adapt_batch, or r1_rd_commit_batch's side_win.
 *   state / call_id (optional gate): desc i acts when state is NULL or state[i].best_call == call_id, the gate of the
 *                commit and of the adapt call; otherwise nothing of it is written.
 * A coded block (flags bit 1 clear) stores
 *   luma:   ctx_in[0][0][c] to above[0][bo_x + c], c < bw / 4; ctx_in[0][1][r] to left[0][bo_y % 16 + r], r < bh / 4;
 *   chroma (with do_chroma), per plane: the span of the chroma transform grid -- bw_uv * (uv_tw / 4) by bh_uv *
 *           (uv_th / 4) entries, r1_coeff_rate_block_batch's grid -- from the chroma origin of the gather.  The grid of
 *           4x16 / 16x4 in 4:2:0 is empty: nothing of chroma is stored.
 * This is set_coeff_context (block_unit.rs:333-348) over the block's transform blocks: ctx_out passes through what no
 * coded transform block wrote, and a transform block coded at a tile edge writes its full span past mi_width.
 * A skipped block (bit 1 set) ignores ctx_in (NULL is allowed when every desc is skipped) and writes zeros as
 * reset_skip_context does (src/context/partition_unit.rs:434-469): the spans of bsize.subsampled_size(xdec, ydec) from
 * bo_x >> xdec / (bo_y % 16) >> ydec; chroma with do_chroma and, whatever the flag, for 4x16 / 16x4 -- `bsize >=
 * BLOCK_8X8` holds for them in the enum's order, so the reference writes three planes there.  (Under Cs400 that touches
 * chroma rows nothing reads.)
 * Every byte outside the spans stays bit-identical.  Acting descs of one call MUST name distinct contexts: two descs on
 * one context would store in no defined order; the call does not detect it.
 * tx_size: the luma transform (it must divide the block; the spans do not depend on it).
 * A desc is refused -- nothing of it is written -- on one of the gather's refusal cases, when a span leaves the arrays
 * (bo_x + bw / 4 > 1024, a chroma span past 1023, a chroma origin of -1), when bo_y % 16 + bh / 4 > 16, or when it is
 * coded and ctx_in is NULL.
 * R1_EINVAL: a NULL ctx, descs or contexts, n < 0, n_contexts < 1, the gather's size and subsampling checks, an invalid
 * tx_size or one that does not divide the block, call_id outside 0..127 with state given.  n == 0 returns 0. */
int r1_coeff_nbr_store_batch(r1_ctx *ctx, const R1NbrBlock *descs, int n, int bw, int bh, int tx_size, int xdec, int ydec,
                             const uint8_t *ctx_in, const R1RdPick *state, int call_id, R1CoeffNbrContext *contexts,
                             int n_contexts, void *stream);
/* The coefficient part of reset_left_contexts (block_unit.rs:394-401) at the start of a superblock row:
 * contexts[sel[i]].left[p][*] = 0 for p < planes, i < n; a sel[i] >= n_contexts writes nothing.
 * R1_EINVAL: a NULL pointer, n < 0, n_contexts < 1, planes outside 1..3.  n == 0 returns 0. */
int r1_coeff_nbr_reset_left_batch(r1_ctx *ctx, R1CoeffNbrContext *contexts, int n_contexts, const uint32_t *sel, int n,
                                  int planes, void *stream);
/* The winner's transform type where r1_coeff_cdf_adapt_batch reads it.  For every state s < n_states with
 * state[s].best_call == call_id, trials[s].tx_type becomes the best_slot-th set bit of tx_type_mask (the slot order of
 * every candidate call).  With is_inter, trials[s].uv_tx_type becomes write_tx_tree's (src/encoder.rs:2507-2511):
 * tx_type.uv_inter(uv_tx_size) (src/transform/mod.rs:81-97), DCT_DCT when eob_win[s * 16 + k] == 0 for all k < ntx
 * (r1_rd_commit_batch's eob_win); rdo_glue.uv_tx_type_inter is the statement.  For intra uv_tx_type belongs to the
 * chroma mode and is not touched; eob_win may be NULL.  No other field and no other state's trial is written; a
 * best_slot outside the mask's popcount writes nothing.
 * R1_EINVAL: a NULL ctx, state or trials, eob_win NULL with is_inter, n_states < 0, call_id outside 0..127, an empty
 * mask or one with bits outside r1_tx_type_mask(TX_4X4, is_inter, 0, 0) (the largest set of the prediction kind), an
 * invalid uv_tx_size, ntx outside 1..16.  n_states == 0 returns 0. */
int r1_rd_winner_tx_type_batch(r1_ctx *ctx, const R1RdPick *state, int n_states, int call_id, uint32_t tx_type_mask,
                               int is_inter, int uv_tx_size, const uint16_t *eob_win, int ntx, R1BlockRateTrial *trials,
                               void *stream);

/* ---- the partition decision on the device (added under ABI 7): the RD comparison a node of the partition quad-tree
 * makes between coding its block whole and coding it as two or four sub-blocks -- encode_partition_bottomup
 * (src/encoder.rs:2683-2843) and rdo_partition_decision with rdo_partition_none / rdo_partition_simple
 * (src/rdo.rs:1849-2024) -- behind the children's chains on the same stream, with no copy and no synchronisation.  A
 * node's decision is an R1PartPick that is carried from call to call; the two selects then move the state the winning
 * trial left to where the next node reads it.  The partition SYMBOL is a head symbol: its rate (the tell_frac
 * difference of write_partition) is handed in as part_rate exactly as rate_add is handed to the pick -- the host's, or
 * for intra frames r1_partition_rate_batch's (further down).
 * All pointers are DEVICE pointers except srcs / src_planes / dst_plane, which are host arrays of device addresses.
 * One call is ONE partition type tried at n nodes: the same node of n tiles, or any n nodes whose children are
 * finished.  Node s reads
 *   state[s]                       best_rd on entry is what the trial has to beat
 *   part_rate[s]                   u32, 1/8 bit; cost = fma(lambda, part_rate / 8, 0.0), ONE rounding as compute_rd_cost
 *                                  with a zero distortion.  part_rate == NULL is the reference's `0.0` arm (a block
 *                                  below 8x8, or the whole-block trial of a non-square block)
 *   child_idx[4 * s + k]           entry k of the node's children: an index into the array at `children` whose
 *                                  elements lie child_stride bytes apart and BEGIN with a double, the child's best_rd
 *                                  (R1RdPick and R1PartPick both do) -- or -1, or any value outside
 *                                  0 .. n_children_states - 1, for "absent": such an index loads nothing.
 *                                  PARTITION_NONE visits entry 0, HORZ and VERT entries 0 and 1, SPLIT all four
 *                                  (get_sub_partitions, src/rdo.rs:1825-1846); the others are not read
 *   must_split[s]                  optional (NULL = 0 everywhere)
 *   parent[parent_idx[s]].best_rd  the node's ref_rd_cost; parent or parent_idx NULL, or an index outside
 *                                  0 .. n_parent_states - 1, means f64::MAX
 * Every addition is the reference's, in its order, in f64, each rounded on its own; none is fused with the multiply
 * of the cost.
 *   R1_PART_BOTTOMUP, partition NONE:  rd = child0 + cost, kept UNCONDITIONALLY (encoder.rs:2708-2711); an absent
 *       child 0 keeps nothing.  early_exit = 0.
 *   R1_PART_BOTTOMUP, otherwise:       rd = cost; for each visited child in order: absent or == f64::MAX: skipped;
 *       else rd += child, and when !must_split && enable_early_exit && (rd >= best_rd || rd >= ref_rd_cost) the trial
 *       ends early: nothing kept, early_exit = 1.  Behind the loop the trial is kept when rd < best_rd, strictly.
 *   R1_PART_TOPDOWN, partition NONE:   rd = child0: no partition symbol (rdo_partition_none); kept when rd < best_rd.
 *   R1_PART_TOPDOWN, otherwise:        sum = 0.0; for each visited child in order: absent: the trial is refused
 *       (early_exit = 0); else sum += child, and when enable_early_exit && sum > best_rd (strictly; the cost is not in
 *       it) the trial is refused with early_exit = 1.  rd = cost + sum, kept when rd < best_rd.  best_rd on entry is
 *       what the caller put into the state: cached_block.rd_cost.
 * The two rules add in different orders -- ((cost + c0) + c1) + ... against cost + (((0 + c0) + c1) + ...) -- and can
 * differ in the last bit; each is kept.  A kept trial writes best_rd, best_partition = partition and best_call =
 * call_id; every visited node has early_exit written; nothing else is written, the padding included.
 * rdo_glue.partition_pick_bottomup / partition_pick_topdown are the statements.
 * R1_EINVAL: a NULL ctx, state or child_idx; children NULL with n_children_states > 0; n < 0; partition outside
 * NONE..SPLIT; rule outside 0..1; call_id outside 0..127; child_stride below 8 or no multiple of 8; a negative
 * n_children_states or n_parent_states; state, children or parent not 8-byte aligned; a lambda that is negative,
 * infinite or NaN.  n == 0 returns 0 and touches nothing.  Every loop is bounded by the arguments, never by data;
 * no atomics, no spin-waits. */
typedef struct R1PartPick {     /* 16 bytes; the decision state of one quad-tree node, carried from call to call */
  double  best_rd;              /* f64::MAX (DBL_MAX) = nothing kept */
  int8_t  best_partition;       /* R1_PARTITION_* of the kept trial, R1_PARTITION_INVALID = none */
  int8_t  best_call;            /* call_id of the kept trial, -1 = none */
  uint8_t early_exit;           /* whether the LAST trial visited ended early */
  uint8_t reserved[5];          /* never read, never written */
} R1PartPick;
#define R1_PARTITION_NONE     0   /* PartitionType's discriminants, src/partition.rs:114-126 */
#define R1_PARTITION_HORZ     1
#define R1_PARTITION_VERT     2
#define R1_PARTITION_SPLIT    3
#define R1_PARTITION_INVALID (-1) /* the state's "nothing kept" (the reference's own discriminant, 10, indexes nothing) */
#define R1_PART_BOTTOMUP 0      /* encode_partition_bottomup */
#define R1_PART_TOPDOWN  1      /* rdo_partition_decision */
int r1_rd_partition_pick_batch(r1_ctx *ctx, R1PartPick *state, int n, int partition, int call_id, int rule,
                               double lambda, int enable_early_exit, const uint32_t *part_rate,
                               const void *children, int child_stride, int n_children_states,
                               const int32_t *child_idx, const uint8_t *must_split, const R1PartPick *parent,
                               int n_parent_states, const int32_t *parent_idx, void *stream);
/* The winner's state where the next node reads it; both calls are gated by the pick and both are byte movers.
 * r1_part_select_batch: for node s < n with c = state[s].best_call in 0 .. n_src - 1 and srcs[c] non-NULL, `bytes`
 * bytes go from srcs[c] + s * src_stride to dst + s * dst_stride; every other node has NOTHING written.  Meant for the
 * snapshots of R1CoeffCdfContext and R1CoeffNbrContext the caller cloned behind each trial, and for the winner arrays
 * of r1_rd_commit_batch.  srcs[c] == dst (with equal strides) is allowed -- the trial that ran last left the live
 * state standing -- and copies nothing.  Apart from that case no source range may overlap a destination range.
 * srcs is a HOST array of n_src device addresses.  Where bytes, both strides and every address are multiples of 16
 * the copy runs in 16-byte pieces, otherwise in 4-byte pieces.
 * R1_EINVAL: a NULL ctx, state, srcs or dst; n < 0; n_src outside 1..4; bytes negative or no multiple of 4; a stride
 * that is negative or no multiple of 4; dst_stride below bytes; an address that is no multiple of 4; srcs[c] == dst
 * with unequal strides.  n == 0 or bytes == 0 returns 0 and touches nothing. */
int r1_part_select_batch(r1_ctx *ctx, const R1PartPick *state, int n, int n_src, const void *const *srcs,
                         long long src_stride, void *dst, long long dst_stride, int bytes, void *stream);
/* r1_part_select_rect_batch: the node's bw x bh rectangle at (pos_xy[2s], pos_xy[2s + 1]) goes from the winning
 * trial's plane, src_planes[state[s].best_call], into dst_plane, clipped to [0, store_w) x [0, store_h) exactly as
 * the `rec` part of r1_rd_commit_batch clips: nothing outside that rectangle and nothing outside the allocation is
 * read or written.  src_planes is a HOST array of n_src R1Plane; one whose data is NULL is "no plane" (its nodes have
 * nothing written), one whose data is dst_plane's copies nothing; every other must have the destination's geometry
 * (stride, alloc_height, xorigin, yorigin, bytes_per_px, bit_depth).  Widths from 4 pixels (the 4:2:0 chroma block of
 * an 8x8) to 64, pos_xy at multiples of 4 pixels where the widest stores are wanted; any position is correct.  The
 * rectangles of one call MUST NOT overlap, and no source plane may share memory with the destination.
 * R1_EINVAL: a NULL pointer; n < 0; n_src outside 1..4; bw / bh that are no block size up to 64x64; the plane checks
 * of r1_rd_commit_batch (1 / 8 or 2 / 10, 12 bits; store_w above stride - xorigin or store_h above alloc_height -
 * yorigin, or negative); a source plane of another geometry; a plane whose data is not aligned to its pixel.
 * n == 0 returns 0. */
int r1_part_select_rect_batch(r1_ctx *ctx, const R1PartPick *state, int n, int n_src, const R1Plane *src_planes,
                              const R1Plane *dst_plane, const int16_t *pos_xy, int bw, int bh, int store_w, int store_h,
                              void *stream);

/* ---- the intra head symbols on the device (added under ABI 7): what a mode trial of luma_chroma_mode_rdo writes in
 * front of its coefficients (src/rdo.rs:866-907) -- the partition symbol, skip, the luma mode and its angle delta, the
 * chroma mode with its CFL alphas or angle delta, the transform size -- on a fresh WriterCounter, against head CDFs that
 * adapt with every winner and neighbour contexts that hold every winner's mode and transform size.  Both are decided on
 * the device, so these calls keep them there.  With the coefficient contexts above, a tile's intra blocks are enqueued in
 * coding order on one stream with nothing read back:
 *     gather -> search -> slice -> head rate -> rates -> pick -> commit -> winner tx type -> adapt -> store -> head commit.
 * r1_intra_head_rate_batch writes rate_add, the head's tell_frac difference that r1_rd_pick_batch adds, and the writer's
 * rng behind the head straight into R1BlockRateTrial.rng, where r1_coeff_rate_block_batch starts from.
 * r1_partition_rate_batch writes the part_rate r1_rd_partition_pick_batch reads.  r1_intra_head_commit_batch replays
 * the winner.  All pointers are DEVICE pointers except tx_sizes.  rdo_glue.head_symbols / partition_symbol /
 * head_nbr_store / head_nbr_reset_left are the statements; tests/golden/head_ref.npz pins them to the reference.
 * R1HeadCdfContext: the head fields of the reference's CDFContext in its own shapes (src/context/cdf_context.rs:42-92),
 * so a host fills it field by field.  y_mode and partition_w128 are carried for the layout; nothing here reads them.
 * OUT OF SCOPE: inter frames (write_is_inter, y_mode_cdf, reference frames, motion vectors and the is_inter arms of
 * get_tx_size_context); write_segmentation; deblock deltas, palette and filter-intra symbols, which the reference never
 * enables here; skip = true trials; 128x128 superblocks (a size with a 128-point side is refused); carrying the TILE
 * writer's rng from partition symbol to partition symbol (r1_partition_rate_batch starts from the rng it is given). */
#define R1_HEAD_NBR_WIDTH 1024             /* COEFF_CONTEXT_MAX_WIDTH; above_partition_context has half of it */
typedef struct R1HeadCdfContext {          /* 2192 bytes */
  uint16_t partition_w8[4][4];
  uint16_t partition[12][10];
  uint16_t partition_w128[4][8];
  uint16_t skip[3][2];                     /* skip_cdfs */
  uint16_t kf_y[5][5][R1_INTRA_MODES];
  uint16_t y_mode[4][R1_INTRA_MODES];
  uint16_t uv_mode[R1_INTRA_MODES][13];
  uint16_t uv_mode_cfl[R1_INTRA_MODES][14];
  uint16_t angle_delta[8][7];
  uint16_t cfl_sign[8];
  uint16_t cfl_alpha[6][16];
  uint16_t tx_size_8x8[3][2];
  uint16_t tx_size[3][3][3];
  uint16_t pad[1];                         /* to a multiple of 16 bytes; never read, never written */
} R1HeadCdfContext;
/* One per tile, or per speculative branch of one, beside R1CoeffNbrContext: the arrays of BlockContext the head contexts
 * read (src/context/block_unit.rs:233-236) and, as ROW BUFFERS, what they read through blocks.above_of / left_of:
 * above_mode[x] / above_skip[x] belong to the block coded last over column x, left_mode[r] / left_skip[r] to the block
 * coded last over the rows r mod 16 -- in coding order that is the cell above_of / left_of names.  A fresh tile is the
 * struct zeroed (DC_PRED is 0); a rollback is the caller's device copy, as for the other two contexts. */
typedef struct R1HeadNbrContext {          /* 3640 bytes */
  uint8_t above_partition[R1_HEAD_NBR_WIDTH / 2], left_partition[8];
  uint8_t above_tx[R1_HEAD_NBR_WIDTH], left_tx[16];
  uint8_t above_mode[R1_HEAD_NBR_WIDTH], left_mode[16];
  uint8_t above_skip[R1_HEAD_NBR_WIDTH], left_skip[16];
} R1HeadNbrContext;
typedef struct R1HeadBlock {               /* 20 bytes: a block's static geometry, which the host knows */
  uint32_t nbr, cdf;                       /* which R1HeadNbrContext, which R1HeadCdfContext */
  uint16_t bo_x, bo_y;                     /* tile block offset, 4x4 units */
  uint16_t mi_cols, mi_rows;               /* the tile's blocks.cols() / rows() */
  uint8_t bsize;                           /* BlockSize, the reference's discriminant (src/partition.rs:130-153) */
  uint8_t has_chroma, tx_mode_select;      /* has_chroma(..) and not Cs400; fi.tx_mode_select */
  uint8_t reserved;
} R1HeadBlock;
typedef struct R1HeadTrial {               /* 16 bytes: one mode trial of a block */
  uint32_t block;                          /* index into blocks */
  uint8_t y_mode, uv_mode;                 /* PredictionMode; uv_mode 13 = UV_CFL_PRED */
  int8_t angle_y, angle_uv;                /* angle_delta.y / .uv, -3 .. 3 */
  int16_t alpha_u, alpha_v;                /* CFLParams::from_alpha(u, v), -16 .. 16 */
  uint8_t tx_size, reserved[3];            /* TxSize */
} R1HeadTrial;
/* rate_add_out[t] = tell_frac behind the head of trials[t] less tell_frac of the fresh counter, 1/8 bit; the writer's
 * rng behind the head goes to (uint16_t *)((char *)rng_out + t * rng_stride) (rng_out optional) -- &trials24[0].rng with
 * stride 24 lands it in an R1BlockRateTrial array.  In coding order: write_partition(PARTITION_NONE) for a square block
 * of 8x8 and up; write_skip(false); write_intra_mode_kf; write_angle_delta for a directional luma mode at
 * bsize >= BLOCK_8X8 IN THE ENUM'S ORDER (4x16 and 16x4 write one); with has_chroma write_intra_uv_mode (uv_mode_cfl_cdf
 * where bsize.cfl_allowed(), bsize <= BLOCK_32X32 in the enum's order), write_cfl_alphas for UV_CFL_PRED, write_angle_delta
 * for a directional chroma mode; with tx_mode_select and bsize > BLOCK_4X4 write_tx_size_intra.  Every symbol is written
 * with its CDF update (symbol_with_update!), so a second symbol on the same row -- the chroma angle delta when the chroma
 * mode equals the luma mode, the V alpha when both signs are equal -- reads what the first adapted.  has_above /
 * has_left are bo_y > 0 / bo_x > 0; above_tx / left_tx are read raw.  Contexts are never written; many trials may share a
 * block.
 *   depth_state / tx_sizes (optional, both or none): one R1RdPick per trial; the trial's transform size is
 *                tx_sizes[depth_state[t].best_call] (a HOST table of three TxSize), in place of the record's.
 *   cfl_alpha (optional): int16 pairs, (u, v) of trial t at [2t], [2t + 1] -- r1_cfl_alpha_search_batch's alpha_out with
 *                a trial's U and V candidates adjacent -- in place of the record's alphas.
 * A trial the device must refuse gets rate 0xFFFFFFFF and nothing else of it is written: block >= n_blocks, nbr / cdf out
 * of range, a bsize past the enum or with a 128-point side, mi_cols > 1024, a place outside the tile, y_mode >= 13, a
 * neighbour mode >= 13 in the context, with has_chroma a uv_mode >= 14 (13 where cfl_allowed() is false), CFL with both
 * alphas zero or one outside -16 .. 16, an angle delta that would be written outside -3 .. 3, a tx_size past the enum
 * or, where it is written, no depth 0 .. 2 of the block, PARTITION_NONE where the tile's edge cuts the block (the
 * reference asserts), best_call outside 0 .. 2 with depth_state given.
 * R1_EINVAL: a NULL ctx, nbrs, cdfs, blocks, trials or rate_add_out; n < 0; n_nbrs, n_cdfs or n_blocks < 1; exactly one
 * of depth_state / tx_sizes; a tx_sizes entry that is no TxSize; rng_out with a stride below 2 or odd, or not 2-byte
 * aligned.  n == 0 returns 0.  One lane per trial; every loop is bounded by 4; no atomics, no spin-waits. */
int r1_intra_head_rate_batch(r1_ctx *ctx, const R1HeadNbrContext *nbrs, int n_nbrs, const R1HeadCdfContext *cdfs,
                             int n_cdfs, const R1HeadBlock *blocks, int n_blocks, const R1HeadTrial *trials, int n,
                             const R1RdPick *depth_state, const uint8_t *tx_sizes, const int16_t *cfl_alpha,
                             uint32_t *rate_add_out, void *rng_out, long long rng_stride, void *stream);
/* write_partition (src/context/partition_unit.rs:267-357) alone: partitions[i] (R1_PARTITION_NONE .. SPLIT, uint8) at
 * node nodes[i] -- an R1HeadBlock whose bsize is the node's; has_chroma and tx_mode_select are not read -- from
 * rng_in[i] (NULL: 0x8000 everywhere).  part_rate_out[i] is the tell_frac difference, the array
 * r1_rd_partition_pick_batch reads; rng_out (optional) the rng behind it.  With rows and columns (bo + half the block
 * inside the tile) the symbol goes to partition_w8_cdf[ctx] for an 8x8 node, else partition_cdf[ctx - 4]; with only one
 * of them to the two-entry CDF of partition_gather_vert_alike / _horz_alike, as SPLIT or not; with neither nothing is
 * written: rate 0, rng unchanged.  Contexts are never written.
 * Refused with rate 0xFFFFFFFF: what the reference asserts against (a node below 8x8 or not square, HORZ / VERT / NONE
 * where the edge does not admit it, an 8x8 node at a one-sided edge), a type above SPLIT, an rng below 0x8000, and the
 * place and index cases of r1_intra_head_rate_batch.
 * R1_EINVAL: a NULL ctx, nbrs, cdfs, nodes, partitions or part_rate_out; n < 0; n_nbrs or n_cdfs < 1.  n == 0 returns 0. */
int r1_partition_rate_batch(r1_ctx *ctx, const R1HeadNbrContext *nbrs, int n_nbrs, const R1HeadCdfContext *cdfs,
                            int n_cdfs, const R1HeadBlock *nodes, const uint8_t *partitions, int n,
                            const uint16_t *rng_in, uint32_t *part_rate_out, uint16_t *rng_out, void *stream);
/* What the winner leaves.  State s acts when state[s].best_call == call_id, as in r1_rd_commit_batch; its trial is
 * t = (s * group + best_row) * nt + best_slot of `trials`, its desc commits[s].  In this order:
 *   the partition event (part_type >= 0): the walker's write_partition(part_type) at the node (node_x, node_y,
 *       node_bsize) adapts the node's partition row -- nothing where an edge arm or the corner writes it.  SPLIT is allowed;
 *   the winner's head symbols as the block is coded for real -- r1_intra_head_rate_batch's from write_skip on, with the
 *       same depth_state / tx_sizes / cfl_alpha; the trial's own PARTITION_NONE is no part of them, the real partition
 *       symbol being the walker's (src/encoder.rs:2688, 2781, 2862), the event above -- adapt cdfs[block.cdf] in place;
 *   on nbrs[block.nbr]: y_mode and skip = 0 over above_mode / above_skip [bo_x ..] and left_mode / left_skip
 *       [bo_y % 16 ..], the block's extent clipped to mi_cols / mi_rows as TileBlocksMut::for_each clips set_mode /
 *       set_skip; with tx_mode_select the transform's width over above_tx[bo_x .. bo_x + bw / 4] and its height over
 *       left_tx[bo_y % 16 ..] (update_tx_size_context, skip = false), clipped to the arrays;
 *   update_partition_context (subsize != R1_HEAD_NO_SUBSIZE): partition_context_lookup[subsize] over the node's spans
 *       above_partition[node_x / 2 ..] and left_partition[(node_y % 16) / 2 ..], clipped to the arrays.  The caller
 *       names it where the reference calls it: bsize >= 8x8 && (bsize == 8x8 || partition != SPLIT), behind the node's
 *       last block.
 * flags bit 0 (R1_HEAD_EVENT_ONLY): the event alone -- a SPLIT above the node the block's own event names; no trial is
 * read and a subsize is refused.
 * Acting descs of one call MUST name distinct contexts (both kinds); the call does not detect it.  Every byte outside the
 * spans and every CDF entry outside the rows touched stays bit-identical.  A desc with a device-resident fault writes
 * NOTHING: the refusal cases of the rate call (less the edge case of its PARTITION_NONE), a best_row / best_slot outside group / nt, t >= n_trials, a trial of
 * another block, a node that is not square, below 8x8 or outside the tile, a part_type the reference asserts against.
 * R1_EINVAL: a NULL ctx, nbrs, cdfs, blocks, trials, commits or state; n_states < 0; n_nbrs, n_cdfs, n_blocks or n_trials
 * < 1; call_id outside 0..127; group outside 1..4096; nt outside 1..16; depth_state / tx_sizes as above.
 * One lane per state; every loop is bounded by 16; no atomics, no spin-waits. */
#define R1_HEAD_NO_SUBSIZE 255
#define R1_HEAD_EVENT_ONLY 1
typedef struct R1HeadCommit {              /* 16 bytes */
  uint32_t block;                          /* index into blocks */
  uint16_t node_x, node_y;                 /* the walker's node: tile block offset */
  uint8_t node_bsize;                      /* and its (square) BlockSize */
  int8_t part_type;                        /* R1_PARTITION_* written in front of the block, -1 = none */
  uint8_t subsize;                         /* update_partition_context's subsize, R1_HEAD_NO_SUBSIZE = none */
  uint8_t flags, reserved[4];
} R1HeadCommit;
int r1_intra_head_commit_batch(r1_ctx *ctx, R1HeadNbrContext *nbrs, int n_nbrs, R1HeadCdfContext *cdfs, int n_cdfs,
                               const R1HeadBlock *blocks, int n_blocks, const R1HeadTrial *trials, int n_trials,
                               const R1HeadCommit *commits, const R1RdPick *state, int n_states, int call_id, int group,
                               int nt, const R1RdPick *depth_state, const uint8_t *tx_sizes, const int16_t *cfl_alpha,
                               void *stream);
/* The head part of reset_left_contexts (src/context/block_unit.rs:394-401) at the start of a superblock row:
 * left_partition and left_tx of nbrs[sel[i]] = 0, i < n; a sel[i] >= n_nbrs writes nothing.  left_mode / left_skip are
 * NOT cleared: the reference's blocks array is not.  R1_EINVAL: a NULL pointer, n < 0, n_nbrs < 1.  n == 0 returns 0. */
int r1_head_nbr_reset_left_batch(r1_ctx *ctx, R1HeadNbrContext *nbrs, int n_nbrs, const uint32_t *sel, int n,
                                 void *stream);

/* ---- the MV reference stack of an inter block on the device (mvref.hip; added under ABI 7): the tile's blocks array
 * and find_mvrefs / setup_mvref_list (src/context/block_unit.rs:795-1442, has_tr of src/partition.rs:900-955) over it.
 * The stack is built from the winning mode, references and vectors of the blocks above and left -- what the device
 * decides and the host no longer sees -- so the array lives on the device, one cell per 4x4 unit, written by
 * r1_tile_blocks_store_batch behind every coded block and read by r1_mvref_stack_batch in front of the next.
 * rdo_glue.find_mvrefs / has_tr / tile_blocks_store / tile_blocks_default / mvref_pmv are the statements;
 * tests/golden/mvref_ref.npz executes the reference.  Vectors are (row, col) in 1/8 pel, as MotionVector.
 * NOT here (the host's still): the inter head symbols and their CDFs (write_is_inter, references, write_inter_mode,
 * write_drl_mode, write_mv); fill_neighbours_ref_counts and the reference contexts; building inter_mode_set / mvs_set
 * and the R1RdoCand descriptors from the stack; intrabc, temporal and global-motion candidates (the reference has
 * none: block_unit.rs:1423-1442 are TODOs); 128x128 superblocks (has_tr assumes 64x64); a select call for the blocks
 * array across partition branches -- a speculative branch is the caller's device copy of the array, as for the
 * other three carried contexts. */
#define R1_INTRA_FRAME 0          /* RefType discriminants (src/partition.rs) */
#define R1_NONE_FRAME 8
#define R1_NEARESTMV 14           /* Block::is_inter: mode >= NEARESTMV */
#define R1_MVREF_MAX_TILES 64     /* R1TileBlocks descriptors per call (they travel in the launch's arguments) */
#define R1_MVREF_MAX_QUERIES 64   /* queries per block: one lane each */
#define R1_MVREF_REFUSED 0xFF     /* R1MvStack.count of a query the device refuses */
typedef struct R1TileBlock {      /* 16 bytes: Block (src/context/block_unit.rs:159-183) as far as the stack and the
                                   * inter head contexts read it */
  int16_t mv[2][2];               /* [list][row, col] */
  uint8_t ref_frames[2];          /* RefType discriminants */
  uint8_t mode;                   /* PredictionMode discriminant */
  uint8_t n4_w, n4_h;             /* the coded block's sides in 4x4 units: the scans step by them */
  uint8_t bsize;                  /* carried for intra_inter_context and the reference-count contexts: only stored */
  uint8_t skip;                   /* likewise */
  uint8_t reserved;
} R1TileBlock;
typedef struct R1TileBlocks {     /* HOST descriptor of one tile's (or branch's) array */
  R1TileBlock *cells;             /* DEVICE, 16-byte aligned: cell (x, y) at cells[y * stride + x] */
  int32_t stride;                 /* cells per row, >= cols */
  int32_t cols, rows;             /* the tile's blocks.cols() / rows() */
  int32_t tile_x, tile_y;         /* the tile's origin in the frame, 4x4 units: blocks.x() / y() */
  int32_t frame_cols, frame_rows; /* blocks.frame_cols() / frame_rows(): the final clamp reads the last four */
  int32_t reserved;
} R1TileBlocks;
typedef struct R1MvBlock {        /* 16 bytes: one block and where its queries lie */
  uint32_t tile;                  /* index into the descriptors */
  uint16_t bo_x, bo_y;            /* tile-relative, 4x4 units */
  uint8_t bsize;                  /* BlockSize, sides up to 64 */
  uint8_t n_queries;              /* queries[query_off .. query_off + n_queries) are this block's; 0 is allowed */
  uint16_t reserved;
  uint32_t query_off;
} R1MvBlock;
typedef struct R1MvQuery {
  uint32_t block;                 /* the R1MvBlock that lists it */
  uint8_t ref_frames[2];
  uint8_t is_compound;
  uint8_t reserved;
} R1MvQuery;
typedef struct R1CandidateMv {    /* CandidateMV, 12 bytes */
  int16_t this_mv[2], comp_mv[2];
  uint32_t weight;
} R1CandidateMv;
typedef struct R1MvStack {        /* 112 bytes */
  uint8_t count;                  /* 0 .. 9 entries, sorted by descending weight, ties in insertion order */
  uint8_t reserved;
  uint16_t mode_context;
  R1CandidateMv cand[9];          /* entries at and past count are written as zero */
} R1MvStack;
typedef struct R1MvTrial {        /* 16 bytes: what one trial would leave in the array were it the winner */
  uint32_t block;                 /* index into the R1MvBlock array */
  uint8_t mode, ref_frames[2], skip;
  int16_t mv[2][2];
} R1MvTrial;
/* Block::default() (block_unit.rs:194-211) over the whole of arrays tiles[sel[i]], i < n (rows x stride cells each, the
 * row padding included): DC_PRED, both references INTRA_FRAME, zero vectors, n4_w = n4_h = 16, BLOCK_64X64, skip 0.
 * A zeroed array is NOT a fresh tile: the scans step by a cell's n4_w / n4_h.  sel: HOST indices, or NULL for every
 * descriptor (then n == n_tiles).
 * R1_EINVAL: a NULL ctx or tiles; n_tiles outside 1..R1_MVREF_MAX_TILES; a descriptor with NULL or unaligned cells,
 * cols or rows < 1, stride < cols, cols or stride > 1024, rows > 65535, negative tile_x / tile_y, frame_cols <
 * tile_x + cols or frame_rows < tile_y + rows, frame_cols or frame_rows above 2^20; n < 0; a sel[i] outside the descriptors.  n == 0 returns 0. */
int r1_tile_blocks_reset_batch(r1_ctx *ctx, const R1TileBlocks *tiles, int n_tiles, const int32_t *sel, int n, void *stream);
/* What a coded block leaves in its tile's array: set_skip (src/encoder.rs:1900), set_block_size, set_mode,
 * set_ref_frames, set_motion_vectors (1968-1972) over the block's extent clipped as TileBlocksMut::for_each clips
 * (src/tiling/tile_blocks.rs:206-224): the width is cut to the tile where bo_x + bw >= cols, rows past the tile are
 * left out.  Every cell outside the extent stays bit-identical.
 * Gating as r1_intra_head_commit_batch: state s of n acts when state[s].best_call == call_id, on trial
 * t = (s * group + best_row) * nt + best_slot; with state == NULL every s acts on trial s (n <= n_trials).  The trial
 * names its block.  An intra winner (mode < NEARESTMV) stores its mode, {INTRA_FRAME, NONE_FRAME} and zero vectors
 * whatever the trial holds.  Acting states must name disjoint extents.  tiles: HOST; blocks, trials, state: DEVICE.
 * Nothing is written for a state whose trial or block index is out of range, whose best_row / best_slot lie outside
 * group / nt, whose block has a bsize past the enum or with a 128-point side, names no descriptor or lies outside its
 * tile, or whose mode is past NEW_NEWMV (33).
 * R1_EINVAL: the descriptor cases above; a NULL blocks or trials; n < 0, n_blocks < 1, n_trials < 1; call_id outside
 * 0..127; group outside 1..4096; nt outside 1..16; state == NULL with n > n_trials.  n == 0 returns 0. */
int r1_tile_blocks_store_batch(r1_ctx *ctx, const R1TileBlocks *tiles, int n_tiles, const R1MvBlock *blocks, int n_blocks,
                               const R1MvTrial *trials, int n_trials, const R1RdPick *state, int n, int call_id,
                               int group, int nt, void *stream);
/* find_mvrefs for every query of n_blocks blocks: stacks_out[query_off + q] for q < n_queries of each block, whole
 * structs.  sign_bias: HOST, 8 bytes: fi.ref_frame_sign_bias, entry r - 1 for reference r (RefType::to_index); entry 7
 * is not read.  A query with ref_frames[0] == INTRA_FRAME returns count 0 and context 0, as the reference.
 * One wave per block: the wave stages the block's neighbourhood (rows -1 .. -5 over its columns and one to the right,
 * columns -1 .. -5 over its rows and one below, the top-left cell; at most 171 cells) in LDS, one 16-byte cell per lane
 * and load, and lane q walks query q from there.
 * The device refuses a query -- count = R1_MVREF_REFUSED and nothing else of the struct written -- where: the block
 * names no descriptor; its bsize is past the enum or has a 128-point side; it lies outside its tile; it has more than
 * max_queries queries; the query's `block` is not the block that lists it; ref_frames[0] == NONE_FRAME; a reference
 * above NONE_FRAME; a compound query whose second reference is INTRA_FRAME or NONE_FRAME; the walk reads a cell whose
 * n4_w or n4_h is 0, not a power of two or above 16, or -- in the extra search -- one with a reference above NONE_FRAME;
 * or where the reference would panic on such a state (a scan that indexes past cols or rows, assert!(inc >= 0)).  The
 * device reads nothing outside the arrays; a query index at or past n_queries is not written at all.
 * R1_EINVAL: the descriptor cases above; a NULL blocks, queries, sign_bias or stacks_out; a stacks_out that is not
 * 4-byte aligned; n_blocks < 0; n_queries < 1;
 * max_queries outside 1..R1_MVREF_MAX_QUERIES.  n_blocks == 0 returns 0. */
int r1_mvref_stack_batch(r1_ctx *ctx, const R1TileBlocks *tiles, int n_tiles, const R1MvBlock *blocks, int n_blocks,
                         const R1MvQuery *queries, int n_queries, int max_queries, const uint8_t *sign_bias,
                         R1MvStack *stacks_out, void *stream);
/* The stack's hand-over to the block motion search (src/rdo.rs:1175-1181): for q < n, at
 * (int16_t *)((char *)pmv_out + q * stride): pmv[0] = cand[0].this_mv if count > 0 else zero, pmv[1] = cand[1].this_mv if
 * count > 1 else zero -- four int16.  With pmv_out = &cands[0].pmv and stride = sizeof(R1MeBlockCand) it fills the
 * array r1_estimate_motion_batch then runs on.  A refused stack writes nothing.
 * R1_EINVAL: a NULL ctx, stacks or pmv_out; n < 0; a pmv_out or stride that is odd; stride < 8.  n == 0 returns 0. */
int r1_mvref_pmv_batch(r1_ctx *ctx, const R1MvStack *stacks, int n, void *pmv_out, long long stride, void *stream);

/* ---- multi-GPU: the tile-boundary exchange and the reference-frame all-gather (RCCL over
 * xGMI), SURVEY.md 8(e).  One process (or host thread) per GPU, tile r on rank r.  Rendezvous:
 * rank 0 calls r1_comm_unique_id and hands the 128 bytes to the other ranks by any channel the
 * host has; every rank then calls r1_comm_create with the device of its context current.
 * All calls enqueue on `stream`; planes / buffers are device memory. */
typedef struct r1_comm r1_comm;
typedef struct R1HaloXfer {
  int32_t peer;            /* rank on the other side */
  int32_t dir;             /* 0: send this rectangle of my plane, 1: receive into it */
  int32_t x0, y0, x1, y1;  /* plane pixels, visible-area coordinates, half-open */
} R1HaloXfer;
/* RCCL is loaded on first use (dlopen), not linked: a process that never calls r1_comm_* needs no
 * RCCL at all.  Which library: $R1_RCCL_LIBRARY if set; else a librccl already loaded into the
 * process (a PyTorch process then has ONE RCCL, torch's own); else librccl.so.1 by the loader's
 * search path, then /opt/rocm/lib/librccl.so.1.  r1_comm_library() names the one in use (NULL before
 * the first r1_comm_* call or when none could be loaded; that case is R1_ECOMM). */
const char *r1_comm_library(void);
int r1_comm_unique_id(uint8_t *id128);
int r1_comm_create(r1_ctx *ctx, int rank, int world, const uint8_t *id128, r1_comm **out);
void r1_comm_destroy(r1_comm *comm);
int r1_comm_rank(const r1_comm *comm);
int r1_comm_world(const r1_comm *comm);
/* every rank contributes bytes_per_rank bytes; recv = the contributions in rank order
 * (a plane: each rank's slab of whole rows -> the whole allocation on every rank) */
int r1_comm_allgather(r1_comm *comm, const void *send, void *recv, size_t bytes_per_rank,
                      void *stream);
/* rank r owns rects4[4r .. 4r+3] = (x0, y0, x1, y1) of `plane`; afterwards every rank holds
 * every tile (pack, one all-gather of equal slots, unpack): the whole reconstructed frame as
 * the next reference */
int r1_comm_allgather_tiles(r1_comm *comm, const R1Plane *plane, const int32_t *rects4, void *stream);
/* rectangles of `plane` to / from neighbouring ranks in one grouped send / receive; the two
 * sides derive matching rectangles from the tile grid (rav1e_amd.tiles.tile_halo_plan =
 * (my tile) ^ (peer's tile + halo)), so nothing is negotiated */
int r1_comm_exchange_halos(r1_comm *comm, const R1Plane *plane, const R1HaloXfer *xfers, int n,
                           void *stream);

/* ---- the same exchange as direct peer stores (added in round 4 under ABI 4; current version: r1_abi_version()).  xGMI is a load / store fabric: once a
 * peer's plane is mapped into this process, a kernel stores this rank's rectangles straight into
 * it -- N - 1 links at once, no staging copy, nothing to unpack.  Planes have the same geometry on
 * every rank.  INVARIANT: the destination plane is in no peer's live reference set -- nobody may still
 * read it (motion search / compensation of a later frame included) when the stores start; the
 * hand-shake (r1_comm_barrier) only orders the stores of THIS step before the kernels behind it.
 * The reconstruction of a frame is a new buffer (src/encoder.rs:3322) that then sits in up to 8
 * reference slots (encoder.rs rec -> ref_frames): a host keeps a pool of (live reference slots + 1)
 * planes per rank, maps every plane of the pool ONCE at start-up (r1_comm_plane_pool_open: one blocking
 * collective for the whole pool; not a per-frame call) and stores a new reconstruction only into the plane that
 * left every rank's reference set.  bench.py / rav1e_amd.tiles.TileRing model the two-plane case (the
 * previous frame as the only reference): one reader, so rotating two is enough THERE and only there. */
typedef struct R1IpcMem {
  uint8_t handle[64];      /* hipIpcMemHandle_t of the allocation */
  uint64_t offset;         /* of the exported range inside it */
  uint64_t bytes;
} R1IpcMem;
typedef struct R1PushRect {
  int32_t peer;            /* index into peer_data */
  int32_t x0, y0, x1, y1;  /* plane pixels, visible-area coordinates, half-open */
} R1PushRect;
/* device memory of this process (any offset inside a hipMalloc allocation) as 80 bytes another
 * process maps with r1_ipc_open; the bytes travel by whatever channel the host has */
int r1_ipc_export(r1_ctx *ctx, const void *ptr, size_t bytes, R1IpcMem *out);
/* before mapping anything: 1 = the context's device can address every other GPU this process
 * sees (hipDeviceCanAccessPeer), 0 = some GPU refuses (stay on r1_comm_exchange_halos /
 * r1_comm_allgather_tiles), -1 = unknown (the process sees one GPU only) */
int r1_ipc_peer_access(r1_ctx *ctx);
int r1_ipc_open(r1_ctx *ctx, const R1IpcMem *mem, void **ptr);
int r1_ipc_close(r1_ctx *ctx, void *ptr);
/* stores rects[i] of `plane` into the same rectangle of the plane at peer_data[rects[i].peer]
 * (one launch per 16 rectangles, enqueued on `stream`; no hand-shake) */
int r1_push_rects(r1_ctx *ctx, const R1Plane *plane, void *const *peer_data, int n_peers,
                  const R1PushRect *rects, int n, void *stream);
/* with a communicator: every rank's plane mapped on every rank (peer_data: `world` entries,
 * [rank] = plane->data; the exports travel in one all-gather; blocking, once per plane) */
int r1_comm_open_peer_planes(r1_comm *comm, r1_ctx *ctx, const R1Plane *plane, void **peer_data);
int r1_comm_close_peer_planes(r1_comm *comm, r1_ctx *ctx, void **peer_data);
/* the POOL of a host (live reference slots + 1 planes, see above) in ONE blocking collective: n_planes
 * (<= 64) planes of the same geometry on every rank; peer_data: n_planes * world entries,
 * [p * world + r] = plane p of rank r ([p * world + rank] = planes[p].data).  peer_data + p * world is what
 * the r1_comm_push_* calls take for plane p.  (ABI 7) */
int r1_comm_plane_pool_open(r1_comm *comm, r1_ctx *ctx, const R1Plane *planes, int n_planes, void **peer_data);
int r1_comm_plane_pool_close(r1_comm *comm, r1_ctx *ctx, int n_planes, void **peer_data);
/* stream-ordered hand-shake (a 4-byte all-reduce): what follows on `stream` starts after every
 * rank's stream reached this call */
int r1_comm_barrier(r1_comm *comm, void *stream);
/* r1_comm_allgather_tiles / r1_comm_exchange_halos as peer stores + r1_comm_barrier (of the
 * xfers list only the dir == 0 entries are used: a rank's receives are its peers' stores) */
int r1_comm_push_tile(r1_comm *comm, r1_ctx *ctx, const R1Plane *plane, void *const *peer_data,
                      const int32_t *rects4, void *stream);
/* both legs of a frame behind ONE hand-shake: the halo stores, the tile stores, r1_comm_barrier (added in round 5 under ABI 5) */
int r1_comm_push_frame(r1_comm *comm, r1_ctx *ctx, const R1Plane *plane, void *const *peer_data,
                       const R1HaloXfer *xfers, int n, const int32_t *rects4, void *stream);
int r1_comm_push_halos(r1_comm *comm, r1_ctx *ctx, const R1Plane *plane, void *const *peer_data,
                       const R1HaloXfer *xfers, int n, void *stream);

/* ---- per-call compat shims: reference asm signatures, HOST pointers ----
 * SadFn / SatdFn (src/asm/x86/dist/mod.rs:21-43): strides in BYTES. */
uint32_t rav1e_sad_hip(const uint8_t *src, ptrdiff_t src_stride,
                       const uint8_t *dst, ptrdiff_t dst_stride, int w, int h);
uint32_t rav1e_satd_hip(const uint8_t *src, ptrdiff_t src_stride,
                        const uint8_t *dst, ptrdiff_t dst_stride, int w, int h);
uint32_t rav1e_sad_hbd_hip(const uint16_t *src, ptrdiff_t src_stride,
                           const uint16_t *dst, ptrdiff_t dst_stride, int w,
                           int h);
uint32_t rav1e_satd_hbd_hip(const uint16_t *src, ptrdiff_t src_stride,
                            const uint16_t *dst, ptrdiff_t dst_stride, int w,
                            int h, uint32_t bdmax);
/* PutFn / PutHBDFn (src/asm/x86/mc.rs:17-38); `src` must be readable 3 px
 * before and 4 px after the block in both dimensions (mc.rs:121-123).
 * mode_x/mode_y select the table entry the reference indexes with
 * get_2d_mode_idx (src/asm/x86/mc.rs:82-84). */
void rav1e_put_8tap_hip(uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src,
                        ptrdiff_t src_stride, int w, int h, int mx, int my,
                        int mode_x, int mode_y);
void rav1e_put_8tap_hbd_hip(uint16_t *dst, ptrdiff_t dst_stride,
                            const uint16_t *src, ptrdiff_t src_stride, int w,
                            int h, int mx, int my, int mode_x, int mode_y,
                            int bitdepth_max);
/* forward_transform (Rust-generic entry, src/asm/x86/transform/forward.rs:444) */
int rav1e_fwd_txfm_hip(const int16_t *input, void *output, size_t stride,
                       int tx_size, int tx_type, int bd, int coeff_bytes);

/* InvTxfmFunc / InvTxfmHBDFunc (src/asm/shared/transform/inverse.rs:15-19)
 * with the dispatch-table indices (tx_size, tx_type) explicit; dst holds the
 * prediction on entry; strides in BYTES; eob is ignored like in the Rust path. */
int rav1e_inv_txfm_add_hip(uint8_t *dst, ptrdiff_t dst_stride, const int16_t *coeff,
                           int eob, int tx_size, int tx_type);
int rav1e_inv_txfm_add_hbd_hip(uint16_t *dst, ptrdiff_t dst_stride, const int32_t *coeff,
                               int eob, int bitdepth_max, int tx_size, int tx_type);
/* CdefDirLBDFn / CdefDirHBDFn, CdefFilterFn / CdefFilterHBDFn
 * (src/asm/x86/cdef.rs:16-37,184-191); `tmp` points at the block inside the
 * reference's padded u16 tile (2 pixels of padding on every side). */
int rav1e_cdef_dir_hip(const uint8_t *img, ptrdiff_t stride, uint32_t *var);
int rav1e_cdef_dir_hbd_hip(const uint16_t *img, ptrdiff_t stride, uint32_t *var,
                           int bitdepth_max);
void rav1e_cdef_filter_hip(uint8_t *dst, ptrdiff_t dst_stride, const uint16_t *tmp,
                           ptrdiff_t tmp_stride, int pri_strength, int sec_strength,
                           int dir, int damping, int xdec, int ydec);
void rav1e_cdef_filter_hbd_hip(uint16_t *dst, ptrdiff_t dst_stride, const uint16_t *tmp,
                               ptrdiff_t tmp_stride, int pri_strength, int sec_strength,
                               int dir, int damping, int bitdepth_max, int xdec, int ydec);
/* intra prediction: the asm entry points take the pointer to the top-left
 * element of the edge buffer (src/asm/x86/predict.rs:20-36); mode / variant
 * select the table entry, ief = 0 none / 1 edge filter / 2 + smooth neighbour
 * (the flags the reference folds into `angle`, predict.rs:301-303). */
int rav1e_ipred_hip(void *dst, ptrdiff_t dst_stride, const void *topleft, int width,
                    int height, int angle, int mode, int variant, int ief, int left_len,
                    int above_len, int avail_w, int avail_h, const int16_t *ac,
                    int bit_depth);

#ifdef __cplusplus
}
#endif
#endif /* RAV1E_AMD_H */

// rdo_intra_split.hip -- the intra transform-split candidate in one launch (r1_rdo_intra_split_batch): what
// rdo_tx_size_type (src/rdo.rs:725-802) makes write_tx_blocks (src/encoder.rs:2243-2311) do for an intra block coded
// with transforms smaller than the block -- the transform blocks in raster order, each predicted from a
// reconstruction that already holds the ones before it (need_recon_pixel, rdo.rs:1729).
//
// Mapping: one wave per workgroup; lane = (trial, column of a transform block), NC = 64 / N trials per wave for an
// N x N transform (fewer when the blocks' working reconstructions would take more than 16 KB of LDS; the other
// lanes idle).  A wave holds consecutive blocks of ONE transform type (the type is wave-uniform: every 1-D kernel
// switch is a scalar branch), and its trials step through the transform blocks k in lockstep -- the geometry is the
// call's.  The working reconstruction R of each trial's block lives in LDS for the whole loop; `rec` is read for
// what lies outside the block and never written.  Per step:
//   edges     r1ip::EdgeRule over an accessor that answers from R inside the block, from `rec` outside
//   predict   r1ip::edge_filter_upsample / predict_column              (intra_pred_common.hpp)
//   forward   residual column, r1tx::fwd_1d_m24, LDS transpose, rows   (tx_common.hpp)
//   quantize  r1q::quantize_group, dequantize                          (quant_common.hpp)
//   inverse   r1itx::inv_1d with the reference's clamps, add into R    (itx_common.hpp)
// and either the transform-domain distortion with estimate_rate per step, or, behind the last step, the pixel-domain
// distortion of the whole block by the tile functions of dist_common.hpp.  The chain from the residual to the
// reconstruction is the one k_rdo_cand (rdo_cand_kernel.hpp) runs for a single transform block, phase by phase.
#include <type_traits>

#include "block_geom.hpp"
#include "common.hpp"
#include "dist_common.hpp"
#include "intra_pred_common.hpp"
#include "itx_common.hpp"
#include "quant_common.hpp"
#include "tx_common.hpp"

namespace {
using r1tx::T;

struct SplitArgs {
  R1Plane org, rec;
  int tile_x, tile_y, rect_w, rect_h, mi_w, mi_h;   // rect: the tile (inside the plane); mi: its 4x4 grid
  int bwl, bhl, ntx, nc;                            // log2 of the block, transform blocks per block, trials per wave
  const R1IntraSplitCand *cands;
  int n, enable;
  uint32_t tx_mask;
  int nt;
  r1q::QParams qp;
  const uint16_t *scan[3];
  int tx_size, q_bin, inv_shift, dist_kind;
  const uint32_t *scales;
  int scale_stride;
  int edge_off, work_off;                           // byte offsets of the edge arrays / the work tile in LDS
  uint16_t *eob;
  unsigned long long *dist, *est_rate;
  void *qcoeffs, *rec_out;
};

constexpr int kRBudget = 16 * 1024;   // LDS bytes of a wave's working reconstructions
constexpr int LSTRIDE = 65;           // dwords per row of the work tile: 64 columns of the wave's trials + 1 (banks)

template <int BD, int TL>
__global__ __launch_bounds__(64) void k_intra_split(SplitArgs a) {
  constexpr int N = 1 << TL, BPP = BD == 8 ? 1 : 2, FL = 4 * N + 1;
  typedef typename std::conditional<BD == 8, int16_t, int32_t>::type CT;
  typedef typename std::conditional<BD == 8, uint8_t, uint16_t>::type PX;
  constexpr int SH0 = r1tx::fwd_shift_ct(TL, TL, BD, 0), SH1 = r1tx::fwd_shift_ct(TL, TL, BD, 1),
                SH2 = r1tx::fwd_shift_ct(TL, TL, BD, 2);
  constexpr int LTS = (N * N > 256) + (N * N > 1024);
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x, cl = lane >> TL, c = lane & (N - 1);
  const int grp = (int)(blockIdx.x / (unsigned)a.nt), slot = (int)blockIdx.x - grp * a.nt;
  int tx_type;
  {
    uint32_t m = a.tx_mask;
    for (int j = 0; j < slot; j++) m &= m - 1;
    tx_type = (int)__builtin_ctz(m);
  }
  const int cand = grp * a.nc + cl;
  const bool valid = cl < a.nc && cand < a.n;
  R1IntraSplitCand cd = {};
  if (valid) cd = a.cands[cand];
  if (cd.mode > r1ip::PAETH_PRED) cd.mode = r1ip::DC_PRED;   // (refused where the host can read the descriptors)
  const bool sane = cd.x >= 0 && cd.y >= 0;
  const long long trial = (long long)cand * a.nt + slot;
  const int bw = 1 << a.bwl, bh = 1 << a.bhl, gwl = a.bwl - TL;
  // a lane without a trial never touches R
  PX *R = (PX *)smem + (valid ? cl : 0) * (bw * bh);
  uint16_t *eraw = (uint16_t *)(smem + a.edge_off) + cl * (5 * FL);
  const uint16_t *tl = eraw + 2 * N;
  uint16_t *ework = eraw + FL;
  int32_t *tile = (int32_t *)(smem + a.work_off);

  const uint8_t *rec0 = px_addr<BPP>(a.rec, a.tile_x, a.tile_y);
  const size_t rst = (size_t)a.rec.stride;
  auto rec_px = [&](int yy, int xx) -> int32_t { return ld_px<BPP>(rec0 + ((size_t)yy * rst + xx) * BPP); };
  // R starts as the block's part of `rec` (what the tile does not hold: 0)
  if (valid) {
    for (int i = c; i < bw * bh; i += N) {
      const int yy = cd.y + (i >> a.bwl), xx = cd.x + (i & (bw - 1));
      R[i] = (PX)((sane && xx < a.rect_w && yy < a.rect_h) ? rec_px(yy, xx) : 0);
    }
  }
  // the tile's pixel (yy, xx) as transform block k sees it
  auto cur_px = [&](int yy, int xx) -> int32_t {
    const int rx = xx - cd.x, ry = yy - cd.y;
    if ((unsigned)rx < (unsigned)bw && (unsigned)ry < (unsigned)bh) return R[(ry << a.bwl) + rx];
    return rec_px(yy, xx);
  };
  const int scan_kind = tx_type < 10 ? 0 : ((tx_type & 1) ? 2 : 1);
  const uint8_t *org0 = px_addr<BPP>(a.org, a.tile_x + cd.x + c, a.tile_y + cd.y);
  const size_t ost = (size_t)a.org.stride * BPP;

  for (int k = 0; k < a.ntx; k++) {
    const int ox = (k & ((1 << gwl) - 1)) << TL, oy = (k >> gwl) << TL;
    const int xk = cd.x + ox, yk = cd.y + oy;
    // encode_tx_block returns at once for a transform block that starts outside the tile's 4x4 grid (encoder.rs:1441)
    const bool act = valid && sane && (xk >> 2) < a.mi_w && (yk >> 2) < a.mi_h;
    const long long oslot = trial * a.ntx + k;
    __syncthreads();   // the previous step's writes to R have landed, its readers of the work tile are done
    // ---- edges (get_intra_edges) and the arguments of dispatch_predict_intra (predict_intra's remaps) ----
    R1IntraCand ic = {};
    int left_len = 0, above_len = 0;
    if (act) {
      const int flags = (a.enable & 1) | (((cd.tr_mask >> k) & 1) << 1) | (((cd.bl_mask >> k) & 1) << 2);
      const r1ip::EdgeRule er(xk, yk, cd.mode, cd.angle_delta, flags, a.rect_w, a.rect_h, N, N, BD);
      left_len = er.init_left;
      above_len = er.init_above;
      for (int i = c; i < FL; i += N) {
        const int e = 2 * r1ip::MAXTX - 2 * N + i;
        const bool init = e >= 2 * r1ip::MAXTX - left_len && e < 2 * r1ip::MAXTX + 1 + above_len;
        eraw[i] = init ? (uint16_t)er.entry(e, cur_px) : (uint16_t)0;
      }
      const int variant = (xk == 0 && yk == 0) ? 0 : (yk == 0 ? 1 : (xk == 0 ? 2 : 3));
      int mode = cd.mode;
      if (mode == r1ip::PAETH_PRED) mode = variant == 0 ? r1ip::DC_PRED : (variant == 2 ? r1ip::V_PRED : (variant == 1 ? r1ip::H_PRED : mode));
      ic.mode = (uint8_t)mode;
      ic.variant = (uint8_t)variant;
      ic.angle = (int16_t)(r1ip::mode_angle(mode) + 3 * cd.angle_delta);
      ic.ief = cd.ief;
      const int aw = a.rec.width - (a.tile_x + xk), ah = a.rec.height - (a.tile_y + yk);
      ic.avail_w = (uint8_t)(aw < N ? (aw < 1 ? 1 : aw) : N);
      ic.avail_h = (uint8_t)(ah < N ? (ah < 1 ? 1 : ah) : N);
    } else {
      for (int i = c; i < FL; i += N) eraw[i] = 0;
    }
    __syncthreads();
    const bool directional = r1ip::is_directional(ic.mode, ic.angle);
    const bool enable = directional && ic.ief != 0;
    int up_a = 0, up_l = 0;
    r1ip::edge_filter_upsample<const R1IntraCand &>(tl, 0, ework, N, N, N, c, ic, enable, left_len, above_len,
                                                     (1 << BD) - 1, up_a, up_l);
    int32_t pred[N];
    r1ip::predict_column<const R1IntraCand &>(N, N, c, ic, directional, enable, up_a, up_l, tl, 0, ework, left_len, BD,
                                               nullptr, [&](int i, int32_t pv) { pred[i] = pv; });
    // ---- residual column, column transform (k_rdo_cand, phase C) ----
    T v[N];
#pragma unroll
    for (int r = 0; r < N; r++) v[r] = 0;
    if (act) {
      const uint8_t *po = org0 + (size_t)oy * ost + (size_t)ox * BPP;
#pragma unroll
      for (int r = 0; r < N; r++) v[r] = ld_px<BPP>(po + r * ost) - pred[r];
    }
    if (r1tx::ud_flip(tx_type)) {   // wave-uniform
#pragma unroll
      for (int r = 0; r < N / 2; r++) {
        const T t0 = v[r];
        v[r] = v[N - 1 - r];
        v[N - 1 - r] = t0;
      }
    }
#pragma unroll
    for (int r = 0; r < N; r++) v[r] = r1tx::shift_fwd_ct<SH0>(v[r]);
    r1tx::fwd_1d_m24<N>(v, r1tx::vtx_1d(tx_type));
    {
      const int cc = cl * N + (r1tx::lr_flip(tx_type) ? N - 1 - c : c);
#pragma unroll
      for (int r = 0; r < N; r++) tile[r * LSTRIDE + cc] = r1tx::shift_fwd_ct<SH1>(v[r]);
    }
    __syncthreads();
    // ---- row transform (phase D): the lane that made column c now owns row c ----
    T u[N];
#pragma unroll
    for (int j = 0; j < N; j++) u[j] = tile[c * LSTRIDE + cl * N + j];
    r1tx::fwd_1d_m24<N>(u, r1tx::htx_1d(tx_type));
#pragma unroll
    for (int j = 0; j < N; j++) u[j] = (T)(CT)r1tx::shift_fwd_ct<SH2>(u[j]);   // `as T::Coeff` (forward.rs:157)
    // ---- quantizer on the coded area, in LDS (phase E) ----
    __syncthreads();
    int32_t *qt = tile + cl * (N * N);
#pragma unroll
    for (int j = 0; j < N; j++) qt[j * N + c] = u[j];
    __syncthreads();
    int eob = 0;
    unsigned long long dist = 0;
    r1q::quantize_group<CT, TL, N, true, LTS, false>(qt, cl * N, c, true, a.scan[scan_kind], a.qp, 0ull, eob, dist);
    if (valid && c == 0) {
      a.eob[oslot] = (uint16_t)(act ? eob : 0);
      if (a.dist_kind == 0) {
        a.dist[oslot] = act ? dist : 0ull;
        if (a.est_rate) a.est_rate[oslot] = act ? r1q::estimate_rate(a.q_bin, a.tx_size, dist) : 0ull;
      }
    }
    __syncthreads();
    if (a.qcoeffs && valid) {
      CT *qd = (CT *)a.qcoeffs + oslot * (N * N);
#pragma unroll
      for (int j = 0; j < N; j++) qd[j * N + c] = act ? (CT)qt[j * N + c] : (CT)0;
    }
    // ---- dequantize (mod.rs:372-383) + inverse row transform (phase F) ----
    T w_[N];
    {
      const int range = BD + 8;
      const T hi = (T)((1 << (range - 1)) - 1), lo = -hi - 1;
      constexpr int32_t off = (1 << LTS) - 1;
#pragma unroll
      for (int j = 0; j < N; j++) {
        const int32_t q = (int32_t)(CT)qt[j * N + c];
        const uint32_t quant = (j == 0 && c == 0) ? a.qp.dc_q : a.qp.ac_q;
        const uint32_t prod = (uint32_t)q * quant;
        const T raw = (T)(CT)((int32_t)(prod + (uint32_t)((q >> 31) & off)) >> LTS);
        w_[j] = r1itx::clamp3(raw, lo, hi);
      }
      r1itx::inv_1d<N, true>(w_, r1tx::htx_1d(tx_type), lo, hi);
    }
    __syncthreads();   // every coefficient has been read: the tile becomes the row buffer
#pragma unroll
    for (int j = 0; j < N; j++) tile[c * LSTRIDE + cl * N + j] = w_[j];
    __syncthreads();
    // ---- inverse column transform, reconstruction into R (phase G) ----
    {
      T rc[N];
      const int range = BD + 6 > 16 ? BD + 6 : 16;
      const T hi = (T)((1 << (range - 1)) - 1), lo = -hi - 1;
      const T pmax = (T)((1 << BD) - 1);
#pragma unroll
      for (int rr = 0; rr < N; rr++) {
        const T x = tile[rr * LSTRIDE + cl * N + c];
        rc[rr] = r1itx::clamp3((x + ((1 << a.inv_shift) >> 1)) >> a.inv_shift, lo, hi);
      }
      r1itx::inv_1d<N, true>(rc, r1tx::vtx_1d(tx_type), lo, hi);
      if (act) {
        PX *d = R + ((oy << a.bwl) + ox + c);
#pragma unroll
        for (int rr = 0; rr < N; rr++) {
          const T px = pred[rr] + ((rc[rr] + 8) >> 4);
          d[rr << a.bwl] = (PX)(px < 0 ? 0 : (px > pmax ? pmax : px));
        }
      }
    }
  }
  __syncthreads();
  // ---- behind the last step: the block's reconstruction and its pixel-domain distortion (sse_wxh / cdef_dist_wxh
  // over 8x8 tiles, a lane per tile; what r1_dist_scaled_batch computes for the block) ----
  if (a.rec_out && valid) {
    PX *d = (PX *)a.rec_out + trial * (bw * bh);
    for (int i = c; i < bw * bh; i += N) d[i] = R[i];
  }
  if (a.dist_kind != 0) {
    unsigned long long acc = 0;
    if (valid) {
      const int tw8 = (bw + 7) >> 3, nt8 = tw8 * ((bh + 7) >> 3);
      for (int t = c; t < nt8; t += N) {
        const int x0 = (t % tw8) * 8, y0 = (t / tw8) * 8;
        const int kw = bw - x0 < 8 ? bw - x0 : 8, kh = bh - y0 < 8 ? bh - y0 : 8;
        const int px = a.tile_x + cd.x + x0, py = a.tile_y + cd.y + y0;
        const uint8_t *po = px_addr<BPP>(a.org, px, py);
        const uint8_t *pr = (const uint8_t *)(R + ((y0 << a.bwl) + x0));
        if (a.dist_kind == R1_DIST_WSSE)
          acc += r1dist::tile_scaled_dist<BPP, 2>(po, ost, pr, (size_t)bw * BPP, kw, kh, px, py, a.scales,
                                                  a.scale_stride, 0, 0, BD);
        else
          acc += r1dist::tile_scaled_dist<BPP, 3>(po, ost, pr, (size_t)bw * BPP, kw, kh, px, py, a.scales,
                                                  a.scale_stride, 0, 0, BD);
      }
    }
    acc = xor_sum_u64(acc, N);
    if (valid && c == 0) a.dist[trial] = a.dist_kind == R1_DIST_WSSE ? (acc + 32) / 64 : acc;
  }
}

// where the host can read the descriptors (ordinary or pinned host memory), as r1_rdo_intra_cand_batch decides it
bool host_readable(const void *p) {
  hipPointerAttribute_t at = {};
  const hipError_t e = hipPointerGetAttributes(&at, p);
  int ndev = 0;
  const bool yes = e == hipSuccess ? at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeHost
                                   : e == hipErrorInvalidValue || hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0;
  (void)hipGetLastError();
  return yes;
}
}  // namespace

extern "C" int r1_rdo_intra_split_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *rec, int tile_x, int tile_y,
                                        int tile_w, int tile_h, int bw, int bh, int tx_size,
                                        const R1IntraSplitCand *cands, int n, int enable_intra_edge_filter,
                                        uint32_t tx_type_mask, const R1QuantParams *params, int dist_kind,
                                        const uint32_t *scales, int scale_stride, uint16_t *eob_out,
                                        uint64_t *dist_out, uint64_t *est_rate_out, void *qcoeffs_out, void *rec_out,
                                        void *stream) {
  R1_REQUIRE(ctx && org && rec && cands && params && eob_out && dist_out);
  R1_REQUIRE(r1_px_ok(*org));
  R1_REQUIRE(r1_px_fits_depth(*org));
  R1_REQUIRE(r1_depth_ok(org->bit_depth));
  R1_REQUIRE(r1_same_px(*org, *rec));
  R1_REQUIRE(r1_same_depth(*org, *rec));
  R1_REQUIRE(params->bit_depth == org->bit_depth);
  // square transforms 4x4 .. 32x32 (TxSize 0 .. 3); the 2:1 sizes and 64x64 are not built
  R1_REQUIRE(tx_size >= 0 && tx_size <= 3);
  const int tl = r1tx::kTxWLog2[tx_size], tn = 1 << tl;
  R1_REQUIRE(r1_block_size_ok(bw, bh));
  const R1LumaGrid lg = r1_luma_grid(bw, bh, tx_size);
  R1_REQUIRE(lg.divides);
  const int ntx = lg.ntx;
  R1_REQUIRE(ntx >= 2 && ntx <= 16);
  R1_REQUIRE(tile_x >= 0 && tile_y >= 0 && tile_w > 0 && tile_h > 0);
  R1_REQUIRE(tile_x + tile_w <= rec->width && tile_y + tile_h <= rec->height);
  R1_REQUIRE(dist_kind == 0 || dist_kind == R1_DIST_WSSE || dist_kind == R1_DIST_CDEF);
  R1_REQUIRE(!scales || scale_stride > 0);
  R1_REQUIRE(dist_kind != 0 || !rec_out);
  R1_REQUIRE(dist_kind == 0 || !est_rate_out);
  R1_REQUIRE(tx_type_mask != 0 && tx_type_mask <= 0xFFFFu);
  R1_REQUIRE((tx_type_mask & ~r1_tx_type_mask(tx_size, 1, 0, 0)) == 0);
  if (n <= 0) return R1_OK;
  if (host_readable(cands))
    for (int i = 0; i < n; i++) {
      R1_REQUIRE(cands[i].mode <= 12);
      R1_REQUIRE(cands[i].x >= 0 && cands[i].y >= 0 && (cands[i].x & 3) == 0 && (cands[i].y & 3) == 0);
    }
  const int bpp = org->bytes_per_px;
  int nc = 64 / tn;
  while (nc > 1 && nc * bw * bh * bpp > kRBudget) nc >>= 1;
  SplitArgs a = {};
  a.org = *org;
  a.rec = *rec;
  a.tile_x = tile_x;
  a.tile_y = tile_y;
  a.rect_w = tile_w;
  a.rect_h = tile_h;
  a.mi_w = (tile_w + 3) >> 2;
  a.mi_h = (tile_h + 3) >> 2;
  a.bwl = r1_ilog2(bw);
  a.bhl = r1_ilog2(bh);
  a.ntx = ntx;
  a.nc = nc;
  a.cands = cands;
  a.n = n;
  a.enable = enable_intra_edge_filter != 0;
  a.tx_mask = tx_type_mask;
  a.nt = __builtin_popcount(tx_type_mask);
  a.qp = r1q::make_qparams(*params, tx_size, bpp == 1 ? 2 : 4);
  for (int k = 0; k < 3; k++) a.scan[k] = ctx->scan_dev + ctx->scan_off[tx_size][k];
  a.tx_size = tx_size;
  a.q_bin = params->qindex / 32;   // RDO_QUANT_DIV
  a.inv_shift = r1itx::kInvShift[tx_size];
  a.dist_kind = dist_kind;
  a.scales = scales;
  a.scale_stride = scale_stride;
  a.eob = eob_out;
  a.dist = (unsigned long long *)dist_out;
  a.est_rate = (unsigned long long *)est_rate_out;
  a.qcoeffs = qcoeffs_out;
  a.rec_out = rec_out;
  const int r_bytes = (nc * bw * bh * bpp + 15) & ~15;
  const int e_bytes = ((64 / tn) * 5 * (4 * tn + 1) * 2 + 15) & ~15;
  a.edge_off = r_bytes;
  a.work_off = r_bytes + e_bytes;
  const size_t lds = (size_t)a.work_off + (size_t)tn * LSTRIDE * 4;
  const long long groups = ((long long)n + nc - 1) / nc;
  R1_REQUIRE(groups * a.nt < (1ll << 31));
  const unsigned grid = (unsigned)(groups * a.nt);
  hipStream_t st = (hipStream_t)stream;
  r1_by_value<12, 8, 10>(org->bit_depth, [&](auto B) {
    r1_by_value<5, 2, 3, 4>(tl, [&](auto L) {
      hipLaunchKernelGGL((k_intra_split<B.value, L.value>), dim3(grid), dim3(64), lds, st, a);
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

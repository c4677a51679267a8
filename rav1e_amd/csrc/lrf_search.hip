// lrf_search.hip -- loop restoration, the restoration leg of rdo_loop_decision (src/rdo.rs:2575-2763) but the rate:
// sgrproj_solve (src/lrf.rs:847-1096) of (unit, parameter set) pairs, the unit filtered with the solved weights and
// rdo_loop_plane_error (rdo.rs:2027-2093) of the result -- in three launches, or in one for units up to 64 x 64 -- and
// the restoration of the CDEF trials of the later passes (rdo.rs:2407-2530).  The filter is sgr_common.hpp's tile
// engine, which the frame filter (lrf.hip) runs too; here a unit is hard-cropped to itself.
#include "common.hpp"
#include "dist_common.hpp"
#include "sgr_common.hpp"
#include "sgr_trial.hpp"

namespace {
using namespace r1sgr;

// sgrproj_solve's moments (lrf.rs:1010-1054): grid.x = tiles of the largest unit, grid.y = (unit, set) pairs; five i64
// sums per pair, accumulated with atomics (integer sums: exact in any order, like the reference's f64 accumulation of
// per-line i64 sums, which never leaves the exact range).
template <int BPP>
__global__ __launch_bounds__(256) void k_sgr_moments(R1Plane cdeffed, R1Plane input, const R1SgrSolveUnit *__restrict__ units,
                                                     long long *__restrict__ acc) {
  __shared__ long long part[4][5];
  const R1SgrSolveUnit u = units[blockIdx.y];
  const int ntx = (u.w + TW - 1) / TW, nty = (u.h + 63) / 64;
  if ((int)blockIdx.x >= ntx * nty || u.set > 15) return;   // workgroup-uniform (set 255: r1_lrf_search_batch's "no filter")
  const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const SgrTile t = sgr_unit_tile<64>(u.x, u.y, u.w, u.h, u.edges, tx * TW, ty * 64);
  long long m[5] = {0, 0, 0, 0, 0};
  sgr_tile<BPP, 64, BPP == 1>(cdeffed, cdeffed, t, u.set, BPP == 1 ? 8 : cdeffed.bit_depth, &input, t.cx0, u.y + t.ty0,
                [&](int x, int y, uint32_t p, uint32_t f1, uint32_t f2, uint32_t in_px) {
    sgr_moments_add(m, p, f1, f2, in_px);
  }, [] {});
  sgr_moments_park(m, part);
  __syncthreads();
  if (threadIdx.x < 5) {
    const long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                        part[3][threadIdx.x];
    if (v) atomicAdd((unsigned long long *)acc + blockIdx.y * 5 + threadIdx.x, (unsigned long long)v);
  }
}

// the 2x2 solve in IEEE doubles, operation for operation (lrf.rs:1057-1095): m = the five moments
// (h00, h11, h01, c0, c1) of a w x h unit
__device__ __forceinline__ void sgr_solve_xqd(const long long *m, int w, int h, int set, int8_t *xqd) {
  if (set > 15) {   // no parameter set: no weights
    xqd[0] = xqd[1] = 0;
    return;
  }
  const uint32_t s2 = kSgrS[set & 15][0], s1 = kSgrS[set & 15][1];
  const double nn = __dmul_rn((double)w, (double)h);
  const double h00 = __ddiv_rn((double)m[0], nn), h11 = __ddiv_rn((double)m[1], nn);
  const double h01 = __ddiv_rn((double)m[2], nn);
  const double sc = __ddiv_rn(128.0, nn);
  const double c0 = __dmul_rn((double)m[3], sc), c1 = __dmul_rn((double)m[4], sc);
  double xq0 = 0., xq1 = 0.;
  if (s2 == 0) {
    if (h11 != 0.) xq1 = round(__ddiv_rn(c1, h11));
  } else if (s1 == 0) {
    if (h00 != 0.) xq0 = round(__ddiv_rn(c0, h00));
  } else {
    const double det = __fma_rn(h00, h11, -__dmul_rn(h01, h01));
    if (det != 0.) {
      xq0 = round(__ddiv_rn(__fma_rn(h11, c0, -__dmul_rn(h01, c1)), det));
      xq1 = round(__ddiv_rn(__fma_rn(h00, c1, -__dmul_rn(h01, c0)), det));
    }
  }
  auto sat = [](double v) -> long long {   // `as i32`
    if (v != v) return 0;
    return v > 2147483647. ? 2147483647ll : (v < -2147483648. ? -2147483648ll : (long long)v);
  };
  const long long q0 = sat(xq0), q1 = sat(xq1);
  const long long x0 = q0 < -96 ? -96 : (q0 > 31 ? 31 : q0);
  const long long t = 128 - x0 - q1;
  xqd[0] = (int8_t)x0;
  xqd[1] = (int8_t)(t < -32 ? -32 : (t > 95 ? 95 : t));
}

__global__ void k_sgr_solve(const R1SgrSolveUnit *__restrict__ units, const long long *__restrict__ acc,
                            int n, int8_t *__restrict__ xqd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R1SgrSolveUnit u = units[i];
  sgr_solve_xqd(acc + (size_t)i * 5, u.w, u.h, u.set, xqd + 2 * i);
}

// rdo_loop_plane_error's term for one block of the unit (rdo.rs:2060-2088): `test` = the filtered unit
// in LDS (row stride TS pixels), (px, py) = the block's position in the plane
template <int BPP, bool CHROMA, int TS, typename PT>
__device__ __forceinline__ unsigned long long lrf_block_err(const R1Plane &src, const PT *test, int px, int py, int bw, int bh,
                                                            int xdec, int ydec, const uint32_t *__restrict__ scales,
                                                            int scale_stride, int bd) {
  const uint8_t *po = px_addr<BPP>(src, px, py);
  const size_t so = (size_t)src.stride * BPP;
  if constexpr (!CHROMA) {
    r1dist::CdefMoments m;
    for (int r = 0; r < 8; r++)
      for (int i = 0; i < 8; i++) m.add((uint32_t)ld_px<BPP>(po + r * so + (size_t)i * BPP), test[r * TS + i]);
    // RawDistortion(cdef_dist_kernel) * bias: the tail multiplies by the block's DistortionScale
    return r1dist::cdef_tile_tail<0>(m, 64, px, py, scales, scale_stride, bd);
  } else {
    // sse_wxh with one bias for the block: get_weighted_sse over its 4x4 cells (dist.rs:234-283)
    const uint32_t sc = r1dist::dist_scale_at(scales, scale_stride, px << xdec, py << ydec);
    unsigned long long sum = 0;
    for (int cy = 0; cy < bh; cy += 4)
      for (int cx = 0; cx < bw; cx += 4) {
        uint32_t cell = 0;
        for (int r = 0; r < 4; r++)
          for (int i = 0; i < 4; i++) {
            const int32_t d = (int32_t)ld_px<BPP>(po + (cy + r) * so + (size_t)(cx + i) * BPP) -
                              (int32_t)test[(cy + r) * TS + cx + i];
            cell += (uint32_t)(d * d);
          }
        sum += r1dist::wsse_cell(cell, sc);
      }
    return (sum + 32) >> 6;
  }
}

// rdo_loop_plane_error (rdo.rs:2027-2093) of luma, the whole workgroup on it.  Round 4 gave a block to a thread: 64 of
// the 256 threads looped over 64 pixels each -- one-pixel global loads of the source at a stride of a plane
// row -- while the other waves waited at the barrier.  Now a thread owns a ROW SEGMENT of a block (the LPR lanes
// of a row read 8 * LPR contiguous source pixels), the rows of a block meet by xor-shuffles inside their wave
// (lanes LPR apart), the caller parks the five sums of every block in LDS and lets ONE pass run the fixed-point
// tails (ssim boost, 64-bit arithmetic) side by side instead of one after the other.
// Chroma keeps a block per thread: the cooperative form LOSES 5-6 % there (profiles/r05_ab_notes.md, ab4).
// This is the middle of it: the moments of segment xs of row y of the tile -- eight pixels of `src`, where the tile
// lies at (x0, y0), against the eight filtered pixels in `test` (LDS, TS pixels a row) -- where `live`, summed over
// the block's rows: every lane of a block's column returns the block's moments.
template <int BPP, int LPR, int TS, typename DT>
__device__ __forceinline__ r1dist::CdefMoments luma_block_moments(bool live, const R1Plane &src, int x0, int y0,
                                                                  int xs, int y, const DT (*test)[TS]) {
  typedef typename std::conditional<BPP == 1, uint8_t, uint16_t>::type ST;
  r1dist::CdefMoments m;
  if (live) {
    const uint8_t *po = px_addr<BPP>(src, x0 + xs * 8, y0 + y);
    // eight source pixels in one load where the segment is aligned (units start at multiples of 8 pixels in
    // every configuration the encoder ships; anything else takes the pixel-by-pixel path), eight filtered
    // pixels in one LDS read
    ST sv8[8];
    DT dv8[8];
    if (((uintptr_t)po & (8 * BPP - 1)) == 0) {
      if constexpr (BPP == 1) *(uint2 *)sv8 = *(const uint2 *)po;
      else *(uint4 *)sv8 = *(const uint4 *)po;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) sv8[i] = (ST)ld_px<BPP>(po + (size_t)i * BPP);
    }
    if constexpr (sizeof(DT) == 1) *(uint2 *)dv8 = *(const uint2 *)&test[y][xs * 8];
    else *(uint4 *)dv8 = *(const uint4 *)&test[y][xs * 8];
#pragma unroll
    for (int i = 0; i < 8; i++) m.add(sv8[i], dv8[i]);
  }
  m.xor_sum(LPR, 8 * LPR);     // the 8 rows of a block: lanes LPR apart
  return m;
}

// rdo_loop_plane_error walks the BLOCK GRID (rdo.rs:2039-2043: `loop_bo < blocks.cols() / rows()`, 2 * ceil(W / 8)
// columns), so every block a visible extent touches counts whole: the extent rounded up to blocks, in pixels (bw a
// power of two).  Past the visible edge the source and the unfiltered input are read as they are (both cut out of the
// 8-aligned allocation, rdo.rs:2277-2295) and a restored plane holds R1_PLANE_NEW_FILL (a fresh Plane::new that is only
// written inside the visible rectangle, rdo.rs:2331-2341).
__device__ __forceinline__ int grid_ext(int v, int b) { return (v + b - 1) & -b; }
// do the planes hold the blocks of the grid a unit touches?  (x, y, w, h) = its visible rectangle
__device__ __forceinline__ bool unit_in_grid(int x, int y, int w, int h, int bw, int bh, const R1Plane &a, const R1Plane &b) {
  const int x1 = x + grid_ext(w, bw), y1 = y + grid_ext(h, bh);
  return w > 0 && h > 0 && x >= 0 && y >= 0 && x1 <= a.width && y1 <= a.height && x1 <= b.width && y1 <= b.height;
}

// rdo_loop_plane_error with a block per thread (chroma everywhere -- see luma_block_moments -- and the three-launch
// plan's luma): the nbx x nby blocks of `test` (LDS; at (x0, y0) of the plane) -> the thread's sum.  Thread -> block is
// dense (a tile has at most 128 blocks, a thread at most one) or, SLOTS16, by rows of 16 block slots (a unit of up to 64
// pixels is at most 16 blocks wide: no runtime division)
template <int BPP, bool CHROMA, bool SLOTS16, int TS, typename PT>
__device__ __forceinline__ unsigned long long blocks_err(const R1Plane &src, const PT (*test)[TS], int x0, int y0, int nbx,
                                                         int nby, int bw, int bh, int xdec, int ydec,
                                                         const uint32_t *__restrict__ scales, int scale_stride, int bd) {
  auto one = [&](int bx, int by) {
    return lrf_block_err<BPP, CHROMA, TS>(src, &test[by * bh][bx * bw], x0 + bx * bw, y0 + by * bh, bw, bh, xdec, ydec,
                                          scales, scale_stride, bd);
  };
  unsigned long long mine = 0;
  if constexpr (SLOTS16) {
    for (int b = threadIdx.x; b < 16 * nby; b += 256)
      if ((b & 15) < nbx) mine += one(b & 15, b >> 4);
  } else if ((int)threadIdx.x < nbx * nby) {
    const int by = (int)threadIdx.x / nbx;
    mine = one((int)threadIdx.x - by * nbx, by);
  }
  return mine;
}

// rdo_loop_plane_error of luma with the whole workgroup on it (luma_block_moments): the 64 rows of `test` (LDS, 8 * LPR
// pixels a row, at (x0, y0) of the plane) LPR lanes a row, the five sums of every block parked in bs (LDS, 8 * LPR
// blocks), then ONE pass of the tails by the first 8 * LPR threads.  Returns the thread's block's error (0: none).
template <int BPP, int LPR, typename DT>
__device__ __forceinline__ unsigned long long luma_blocks_err(const R1Plane &src, int x0, int y0, const DT (*test)[8 * LPR], int nbx,
                                                              int nby, uint32_t (*bs)[5], const uint32_t *__restrict__ scales,
                                                              int scale_stride, int bd) {
  constexpr int ROWS = 256 / LPR;   // rows of the tile per pass of the workgroup
#pragma unroll
  for (int y0t = 0; y0t < 64; y0t += ROWS) {
    const int y = y0t + (int)threadIdx.x / LPR, xs = (int)threadIdx.x & (LPR - 1);   // tile row, 8-pixel segment of it
    const r1dist::CdefMoments m = luma_block_moments<BPP, LPR>(xs < nbx && y < nby * 8, src, x0, y0, xs, y, test);
    if ((y & 7) == 0) m.store(bs[(y >> 3) * LPR + xs]);
  }
  __syncthreads();
  const int by = (int)threadIdx.x / LPR, bx = (int)threadIdx.x & (LPR - 1);
  if (threadIdx.x >= 8 * LPR || bx >= nbx || by >= nby) return 0;
  // RawDistortion(cdef_dist_kernel) * bias: the tail multiplies by the block's DistortionScale
  return r1dist::cdef_tile_tail<0>(r1dist::CdefMoments::load(bs[threadIdx.x]), 64, x0 + bx * 8, y0 + by * 8, scales,
                                   scale_stride, bd);
}

// The restoration leg of rdo_loop_decision, per (unit, set) pair (src/rdo.rs:2575-2763): the unit filtered with the
// weights k_sgr_solve just wrote -- sgrproj_stripe_filter on the unit's OWN padded image (hard-clipped like the solve),
// never stored -- and rdo_loop_plane_error of the result against the source (rdo.rs:2027-2093): per 8x8-luma block
// cdef_dist_kernel * bias (luma) or sse_wxh with |_, _| bias on (8 >> xdec) x (8 >> ydec) pixels (chroma).  Same tiling as
// k_sgr_moments; a tile's filtered pixels go to LDS, one thread per block sums its block, the workgroup's total is added
// to the pair's plane sum.  set = 255: the "no filter option" (the unit of lrf_in as it is).
template <int BPP, bool CHROMA>
__global__ __launch_bounds__(256) void k_sgr_unit_err(R1Plane lrf_in, R1Plane src, const R1SgrSolveUnit *__restrict__ units,
                                                      const int8_t *__restrict__ xqd, int xdec, int ydec,
                                                      const uint32_t *__restrict__ scales, int scale_stride,
                                                      unsigned long long *__restrict__ acc) {
  __shared__ uint16_t F[64][TW];
  __shared__ unsigned long long part[4];
  const R1SgrSolveUnit u = units[blockIdx.y];
  const int bw = sgr_block_dim(CHROMA, xdec), bh = sgr_block_dim(CHROMA, ydec);
  if (!unit_in_grid(u.x, u.y, u.w, u.h, bw, bh, lrf_in, src)) return;   // k_lrf_err_finish reports it; workgroup-uniform
  const int ntx = (u.w + TW - 1) / TW, nty = (u.h + 63) / 64;
  if ((int)blockIdx.x >= ntx * nty) return;   // workgroup-uniform
  const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const SgrTile t = sgr_unit_tile<64>(u.x, u.y, u.w, u.h, u.edges, tx * TW, ty * 64);
  const int bd = lrf_in.bit_depth;
  // the tile out to the block grid: TW and 64 are whole blocks, so only a unit's last tiles grow
  const int gtw = grid_ext(t.tw, bw), gth = grid_ext(t.th, bh);
  if (u.set > 15) {
    sgr_stage_unfiltered<BPP>(F, lrf_in, t.cx0, u.y + t.ty0, gtw, gth);
  } else {
    sgr_fill_margin(F, t.tw, t.th, gtw, gth);   // BEFORE the filter, which writes inside t.tw x t.th only
    const int w0 = xqd[2 * blockIdx.y], w1 = xqd[2 * blockIdx.y + 1], w2 = 128 - w0 - w1;
    const int32_t pmax = (1 << bd) - 1;
    sgr_tile<BPP, 64, BPP == 1>(lrf_in, lrf_in, t, u.set, bd, nullptr, 0, 0,
                                [&](int x, int y, uint32_t p, uint32_t f1, uint32_t f2, uint32_t) {
      F[y][x] = (uint16_t)sgr_project(p, f1, f2, w0, w1, w2, pmax);
    }, [] {});
  }
  __syncthreads();
  const int nbx = gtw / bw, nby = gth / bh;   // ceil(t.tw / bw), ceil(t.th / bh)
  const unsigned long long mine = blocks_err<BPP, CHROMA, false>(src, F, t.cx0, u.y + t.ty0, nbx, nby, bw, bh, xdec, ydec,
                                                                 scales, scale_stride, bd);
  const unsigned long long v = wg_sum_u64(mine, part);
  if (threadIdx.x == 0 && v) atomicAdd(acc + blockIdx.y, v);
}

// The same leg in ONE launch for units up to 64 x 64 pixels (the 64x64 luma / 32x32 chroma units of the
// speed settings the encoder ships): a workgroup owns a (unit, set) pair, the two filter outputs of every
// pixel stay in LDS between the moments and the projection, so the box filters run once.
// PACK: both filter outputs of a pixel in one dword (f <= 16 * 1023 + rounding: up to 10 bits; at 12 bits an
// all-white unit reaches 65588)
// Occupancy (ab9, ab10): with 32-row tiles an 8-bit workgroup holds 31 KB of LDS and 96 VGPRs -- five per CU -- and a
// 16-bit one 35 KB -- four (three with the 64-row tile of round 4).  The 8-bit kernels are asked for five: with the unit's
// edge flags (t.lu / t.top) they would settle at 106 VGPRs otherwise; the request costs 12 B of scratch
template <int BPP, bool CHROMA, bool PACK>
__global__ __launch_bounds__(256, BPP == 1 ? 5 : 1) void k_lrf_search_unit(R1Plane lrf_in, R1Plane src,
                                                         const R1SgrSolveUnit *__restrict__ units, int xdec, int ydec,
                                                         const uint32_t *__restrict__ scales, int scale_stride,
                                                         uint32_t dist_scale, int8_t *__restrict__ xqd_out,
                                                         unsigned long long *__restrict__ err_out) {
  typedef typename std::conditional<BPP == 1, uint8_t, uint16_t>::type PT;
  __shared__ uint32_t F1[64][64];
  __shared__ uint32_t F2[PACK ? 1 : 64][64];         // PACK: f1 | f2 << 16 in F1
  __shared__ __attribute__((aligned(16))) PT P[64][64];   // the unit's pixels, then the filtered unit
  __shared__ long long mpart[4][5];
  __shared__ unsigned long long epart[4];
  __shared__ int8_t xq[2];
  // Consecutive workgroup ids go to the eight XCDs in turn, each with its own L2.  Callers list the parameter sets of
  // a unit next to each other (rdo_loop_decision's loop order): handing an XCD a CONTIGUOUS run of pairs keeps the nine
  // launches that read the same unit -- its pixels and the source's -- on one L2 (before: every set of a unit fetched
  // it again, 135 MB a luma launch for 17 MB of planes; the tile loads are a quarter of a wave's life)
  const int pair = xcd_run_item(blockIdx.x, gridDim.x);   // common.hpp
  const R1SgrSolveUnit u = units[pair];
  const int bd = BPP == 1 ? 8 : lrf_in.bit_depth;
  const int bw = sgr_block_dim(CHROMA, xdec), bh = sgr_block_dim(CHROMA, ydec);
  // not what max_w / max_h promised, or planes that do not hold the blocks the unit touches: no result
  if (u.w > 64 || u.h > 64 || !unit_in_grid(u.x, u.y, u.w, u.h, bw, bh, lrf_in, src)) {
    if (threadIdx.x == 0) {
      err_out[pair] = ~0ull;
      xqd_out[2 * pair] = xqd_out[2 * pair + 1] = 0;
    }
    return;
  }
  const int gw = grid_ext(u.w, bw), gh = grid_ext(u.h, bh);   // the unit out to the block grid (<= 64)
  if (u.set > 15) {
    sgr_stage_unfiltered<BPP>(P, lrf_in, u.x, u.y, gw, gh);
    if (threadIdx.x == 0) xqd_out[2 * pair] = xqd_out[2 * pair + 1] = 0;
  } else {
    long long m[5] = {0, 0, 0, 0, 0};
    // rows per tile: 32 -- the tile arrays are 9 KB smaller than with 64 and one more workgroup fits a CU at either
    // pixel width; the two extra tiles of a 64-row luma unit cost less than that buys since the tile's fixed part shrank
    // (r05_ab_notes.md ab9 / ab10)
    constexpr int TR = 32;
    const int ntx = (u.w + TW - 1) / TW;
    for (int ty = 0; ty < u.h; ty += TR)
    for (int tx = 0; tx < ntx; tx++) {
      const SgrTile t = sgr_unit_tile<TR>(u.x, u.y, u.w, u.h, u.edges, tx * TW, ty);
      // PACK (bit depth <= 10): f - u and s - u are 14-bit-and-a-sign differences of Q4 pixels (|f - u| <= 16 * 1023 +
      // rounding), their products < 2^28.1: four of them fit an int32, so the moments of a thread's four rows are
      // gathered with the full-rate 24-bit multiply-add and widened once per four rows instead of five quarter-rate
      // 64-bit multiply-adds per pixel
      int32_t a32[5] = {0, 0, 0, 0, 0};
      sgr_tile<BPP, TR, PACK>(lrf_in, lrf_in, t, u.set, bd, &src, u.x + tx * TW, u.y + ty,
                              [&](int x, int yt, uint32_t p, uint32_t f1, uint32_t f2, uint32_t src_px) {
        const int X = tx * TW + x, y = ty + yt;
        if constexpr (!PACK) { F1[y][X] = f1; F2[y][X] = f2; }
        else F1[y][X] = f1 | (f2 << 16);
        P[y][X] = (PT)p;
        if constexpr (PACK) {
          const int32_t uu = (int32_t)(p << 4);
          const int32_t sv = ((int32_t)src_px << 4) - uu, g2 = (int32_t)f2 - uu, g1 = (int32_t)f1 - uu;
          a32[0] = mad_i24(g2, g2, a32[0]); a32[1] = mad_i24(g1, g1, a32[1]); a32[2] = mad_i24(g1, g2, a32[2]);
          a32[3] = mad_i24(g2, sv, a32[3]); a32[4] = mad_i24(g1, sv, a32[4]);
        } else {
          sgr_moments_add(m, p, f1, f2, src_px);
        }
      }, [&] {
        if constexpr (PACK) {
#pragma unroll
          for (int k = 0; k < 5; k++) { m[k] += a32[k]; a32[k] = 0; }
        }
      });
      __syncthreads();   // the tile's LDS is staged again by the next one
    }
    sgr_moments_park(m, mpart);
    __syncthreads();
    if (threadIdx.x == 0) {
      long long tot[5];
      for (int k = 0; k < 5; k++) tot[k] = mpart[0][k] + mpart[1][k] + mpart[2][k] + mpart[3][k];
      sgr_solve_xqd(tot, u.w, u.h, u.set, xq);
      xqd_out[2 * pair] = xq[0];
      xqd_out[2 * pair + 1] = xq[1];
    }
    __syncthreads();
    const int w0 = xq[0], w1 = xq[1], w2 = 128 - w0 - w1;
    const int32_t pmax = (1 << bd) - 1;
    sgr_fill_margin(P, u.w, u.h, gw, gh);
    for (int e = threadIdx.x; e < 64 * u.h; e += 256) {
      const int y = e >> 6, x = e & 63;
      if (x >= u.w) continue;
      uint32_t f1, f2;
      if constexpr (!PACK) { f1 = F1[y][x]; f2 = F2[y][x]; }
      else { f1 = F1[y][x] & 0xFFFFu; f2 = F1[y][x] >> 16; }
      P[y][x] = (PT)sgr_project(P[y][x], f1, f2, w0, w1, w2, pmax);
    }
  }
  __syncthreads();
  const int nbx = gw / bw, nby = gh / bh;   // ceil(u.w / bw), ceil(u.h / bh)
  unsigned long long mine;
  if constexpr (!CHROMA) {
    // the whole workgroup on it, 8 lanes per unit row: a wave covers exactly one row of blocks per half
    uint32_t(*bs)[5] = (uint32_t(*)[5]) & F1[0][0];   // 64 x 5 sums over the filter outputs, which are dead by now
    mine = luma_blocks_err<BPP, 8>(src, u.x, u.y, P, nbx, nby, bs, scales, scale_stride, bd);
  } else {
    mine = blocks_err<BPP, CHROMA, true>(src, P, u.x, u.y, nbx, nby, bw, bh, xdec, ydec, scales, scale_stride, bd);
  }
  const unsigned long long v = wg_sum_u64(mine, epart);
  // Distortion * fi.dist_scale[pli] (rdo.rs:2092; DistortionScale::mul_u64, rdo.rs:613-615)
  if (threadIdx.x == 0) err_out[pair] = r1dist::dist_scale_mul(dist_scale, v);
}

// A later pass of rdo_loop_decision's CDEF leg (rdo.rs:2407-2530): the superblock's trial output (cdef_search.hip,
// MODE 1: the plane `trial` of cdef_index blockIdx.z) restored with the unit's CURRENT choice -- setup_integral_image
// on the superblock alone (crop = the superblock; left / above it the area's working copy `cdef_cur` where the edge
// flags say so), sgrproj_stripe_filter with the chosen (set, xqd) -- and rdo_loop_plane_error of the restored
// superblock against the source, added to the (superblock, index, plane) sum the CDEF kernels use.
constexpr int TRIAL_TR = 64;   // rows per tile
template <int BPP, bool CHROMA>
__global__ __launch_bounds__(256) void k_sgr_trial_err(R1Plane trial, size_t trial_idx_bytes, R1Plane cdef_cur, R1Plane src,
                                                       const R1TrialUnit *__restrict__ units, int pli, int xdec, int ydec,
                                                       const uint32_t *__restrict__ scales, int scale_stride,
                                                       unsigned long long *__restrict__ psum, int n_sb) {
  constexpr int TR = TRIAL_TR;
  __shared__ __attribute__((aligned(16))) uint16_t F[TR][TW];
  __shared__ unsigned long long part[4];
  const R1TrialUnit u = units[blockIdx.y];
  const int idx = blockIdx.z;
  // a unit that is not what the header promises (a superblock's visible rectangle inside the plane, a known parameter
  // set, a superblock of this frame) is skipped, never read or accumulated: workgroup-uniform
  const int bw = sgr_block_dim(CHROMA, xdec), bh = sgr_block_dim(CHROMA, ydec);
  if (u.w > 64 || u.h > 64 || u.set > 15 || u.sb < 0 || u.sb >= n_sb || !unit_in_grid(u.x, u.y, u.w, u.h, bw, bh, trial, src))
    return;
  const int ntx = (u.w + TW - 1) / TW, nty = (u.h + TR - 1) / TR;
  if ((int)blockIdx.x >= ntx * nty) return;
  const int tx = (int)blockIdx.x % ntx, ty = (int)blockIdx.x / ntx;
  trial.data = (uint8_t *)trial.data + (size_t)idx * trial_idx_bytes;
  const SgrTile t = sgr_unit_tile<TR>(u.x, u.y, u.w, u.h, u.edges, tx * TW, ty * TR);   // the unit is the superblock
  const int bd = BPP == 1 ? 8 : src.bit_depth;   // (the trial plane's descriptor carries none)
  const int w0 = u.xqd[0], w1 = u.xqd[1], w2 = 128 - w0 - w1;
  const int32_t pmax = (1 << bd) - 1;
  sgr_tile<BPP, TR, BPP == 1, true>(trial, cdef_cur, t, u.set, bd, nullptr, 0, 0,
                                    [&](int x, int y, uint32_t p, uint32_t f1, uint32_t f2, uint32_t) {
    F[y][x] = (uint16_t)sgr_project(p, f1, f2, w0, w1, w2, pmax);
  }, [] {});
  // the tile out to the block grid (TW and TR are whole blocks: only the superblock's last tiles grow): the restoration
  // working copy was never written there.  AFTER the filter: one barrier serves both
  const int gtw = grid_ext(t.tw, bw), gth = grid_ext(t.th, bh);
  sgr_fill_margin(F, t.tw, t.th, gtw, gth);
  __syncthreads();
  const int nbx = gtw / bw, nby = gth / bh;   // ceil(t.tw / bw), ceil(t.th / bh)
  unsigned long long mine;
  if constexpr (!CHROMA) {
    // the whole workgroup on it, 4 lanes per tile row; 32 threads run the tails
    static_assert(TR == 64, "luma_blocks_err walks 64 rows");
    __shared__ uint32_t bs[TR / 2][5];
    mine = luma_blocks_err<BPP, 4>(src, t.cx0, u.y + t.ty0, F, nbx, nby, bs, scales, scale_stride, bd);
  } else {
    mine = blocks_err<BPP, CHROMA, false>(src, F, t.cx0, u.y + t.ty0, nbx, nby, bw, bh, xdec, ydec, scales, scale_stride, bd);
  }
  const unsigned long long v = wg_sum_u64(mine, part);
  if (threadIdx.x == 0 && v) atomicAdd(psum + (size_t)u.sb * 24 + idx * 3 + pli, v);
}

// Distortion * fi.dist_scale[pli] (rdo.rs:2092; DistortionScale::mul_u64, rdo.rs:613-615)
// a unit whose blocks the planes do not hold has no result (as in k_lrf_search_unit)
__global__ void k_lrf_err_finish(const unsigned long long *__restrict__ acc, int n, uint32_t dist_scale,
                                 const R1SgrSolveUnit *__restrict__ units, R1Plane lrf_in, R1Plane src, int bw, int bh,
                                 int8_t *__restrict__ xqd, unsigned long long *__restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R1SgrSolveUnit u = units[i];
  if (unit_in_grid(u.x, u.y, u.w, u.h, bw, bh, lrf_in, src)) {
    err[i] = r1dist::dist_scale_mul(dist_scale, acc[i]);
  } else {
    err[i] = ~0ull;
    xqd[2 * i] = xqd[2 * i + 1] = 0;
  }
}

// grid of k_sgr_moments / k_sgr_unit_err: x = the 64-row tiles of the largest unit, y = the n (unit, set) pairs
inline dim3 unit_tile_grid(int max_w, int max_h, int n) { return dim3(((max_w + TW - 1) / TW) * ((max_h + 63) / 64), n); }

// sgrproj_solve of n pairs: `scratch` = five moments per pair, zeroed here together with what the caller keeps behind
// them (zero_words int64 in all, one memset), k_sgr_moments, k_sgr_solve -> xqd_out
inline int launch_moments_solve(const R1Plane &cdeffed, const R1Plane &input, const R1SgrSolveUnit *units, int n, int max_w,
                                int max_h, int64_t *scratch, size_t zero_words, int8_t *xqd_out, hipStream_t st) {
  R1_HIP_CHECK(hipMemsetAsync(scratch, 0, zero_words * sizeof(int64_t), st));
  r1_by_bpp(cdeffed.bytes_per_px, [&](auto B) {
    hipLaunchKernelGGL((k_sgr_moments<B.value>), unit_tile_grid(max_w, max_h, n), dim3(256), 0, st, cdeffed, input, units,
                       (long long *)scratch);
  });
  hipLaunchKernelGGL(k_sgr_solve, dim3((n + 127) / 128), dim3(128), 0, st, units, (const long long *)scratch, n, xqd_out);
  return R1_OK;
}

}  // namespace

// called by cdef_search.hip (r1_cdef_lrf_trial_batch); not part of the C ABI: declared in sgr_trial.hpp
__attribute__((visibility("hidden")))
int r1i_sgr_trial_err_launch(const R1Plane &trial, size_t trial_idx_bytes, const R1Plane &cdef_cur, const R1Plane &src,
                             const R1TrialUnit *units, int n_units, int n_idx, int pli, int xdec, int ydec,
                             const uint32_t *scales, int scale_stride, unsigned long long *psum, int n_sb, hipStream_t st) {
  R1_REQUIRE(r1_offsets_fit_u32(trial) && r1_offsets_fit_u32(cdef_cur) && r1_offsets_fit_u32(src));
  R1_REQUIRE(r1_same_px(src, trial, cdef_cur));
  const dim3 grid((64 / TW) * (64 / TRIAL_TR), n_units, n_idx);
  r1_by_bpp(src.bytes_per_px, [&](auto B) {
    r1_by_bool(pli != 0, [&](auto CH) {
      hipLaunchKernelGGL((k_sgr_trial_err<B.value, CH.value>), grid, dim3(256), 0, st, trial, trial_idx_bytes, cdef_cur,
                         src, units, pli, xdec, ydec, scales, scale_stride, psum, n_sb);
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_sgrproj_solve_batch(r1_ctx *ctx, const R1Plane *cdeffed, const R1Plane *input,
                                      const R1SgrSolveUnit *units, int n, int max_w, int max_h,
                                      int64_t *moments_scratch, int8_t *xqd_out, void *stream) {
  R1_REQUIRE(ctx && cdeffed && input);
  R1_REQUIRE(r1_offsets_fit_u32(*cdeffed) && r1_offsets_fit_u32(*input));
  R1_REQUIRE(r1_same_px(*cdeffed, *input) && r1_same_depth(*cdeffed, *input));
  R1_REQUIRE(r1_px_ok(*cdeffed));
  R1_REQUIRE(r1_px_fits_depth(*cdeffed));
  R1_REQUIRE(max_w > 0 && max_h > 0 && max_w <= 384 && max_h <= 384);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(units && moments_scratch && xqd_out);
  const int rc = launch_moments_solve(*cdeffed, *input, units, n, max_w, max_h, moments_scratch, (size_t)n * 5, xqd_out,
                                      (hipStream_t)stream);
  if (rc != R1_OK) return rc;
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// The restoration leg of rdo_loop_decision for one plane, everything but the rate (see
// k_sgr_unit_err): units as for r1_sgrproj_solve_batch, plus set = 255 for the "no filter option".
extern "C" int r1_lrf_search_batch(r1_ctx *ctx, const R1Plane *lrf_in, const R1Plane *src, const R1SgrSolveUnit *units, int n,
                                   int max_w, int max_h, int is_chroma, int xdec, int ydec, const uint32_t *scales,
                                   int scale_stride, uint32_t dist_scale, int64_t *scratch, int8_t *xqd_out,
                                   uint64_t *err_out, void *stream) {
  R1_REQUIRE(ctx && lrf_in && src);
  R1_REQUIRE(r1_offsets_fit_u32(*lrf_in) && r1_offsets_fit_u32(*src));
  R1_REQUIRE(r1_same_px(*lrf_in, *src) && r1_same_depth(*lrf_in, *src));
  R1_REQUIRE(r1_px_ok(*lrf_in));
  R1_REQUIRE(r1_px_fits_depth(*lrf_in));
  R1_REQUIRE(max_w > 0 && max_h > 0 && max_w <= 384 && max_h <= 384);
  R1_REQUIRE(r1_dec_ok(xdec, ydec) && (is_chroma || (!xdec && !ydec)));
  R1_REQUIRE(!scales || scale_stride > 0);
  // the error walks the block grid: planes allocated in whole blocks (Frame::new aligns to 8 luma pixels)
  const int bw = sgr_block_dim(is_chroma, xdec), bh = sgr_block_dim(is_chroma, ydec);
  R1_REQUIRE(lrf_in->width % bw == 0 && lrf_in->height % bh == 0 && src->width % bw == 0 && src->height % bh == 0);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(units && scratch && xqd_out && err_out);
  hipStream_t st = (hipStream_t)stream;
  if (max_w <= 64 && max_h <= 64) {
    // one launch: a workgroup per pair keeps the filter outputs in LDS between the solve and the projection
    r1_by_bpp(lrf_in->bytes_per_px, [&](auto B) {
      r1_by_bool(is_chroma != 0, [&](auto CH) {
        // one-byte pixels are always packed: there is no <1, *, false>
        r1_by_bool(lrf_in->bit_depth <= 10 || lrf_in->bytes_per_px == 1, [&](auto PK) {
          if constexpr (B.value == 2 || PK.value)
            hipLaunchKernelGGL((k_lrf_search_unit<B.value, CH.value, PK.value>), dim3(n), dim3(256), 0, st, *lrf_in, *src,
                               units, xdec, ydec, scales, scale_stride, dist_scale, xqd_out,
                               (unsigned long long *)err_out);
        });
      });
    });
    R1_HIP_CHECK(hipGetLastError());
    return R1_OK;
  }
  // larger units: moments, solve, then the box filters again for the error
  // scratch: 5 moments per pair, then the pair's plane sum, zeroed in the same memset
  const int rc = launch_moments_solve(*lrf_in, *src, units, n, max_w, max_h, scratch, (size_t)n * 6, xqd_out, st);
  if (rc != R1_OK) return rc;
  unsigned long long *acc = (unsigned long long *)scratch + (size_t)n * 5;
  r1_by_bpp(lrf_in->bytes_per_px, [&](auto B) {
    r1_by_bool(is_chroma != 0, [&](auto CH) {
      hipLaunchKernelGGL((k_sgr_unit_err<B.value, CH.value>), unit_tile_grid(max_w, max_h, n), dim3(256), 0, st, *lrf_in, *src, units,
                         (const int8_t *)xqd_out, xdec, ydec, scales, scale_stride, acc);
    });
  });
  hipLaunchKernelGGL(k_lrf_err_finish, dim3((n + 127) / 128), dim3(128), 0, st, acc, n, dist_scale, units, *lrf_in, *src,
                     bw, bh, xqd_out, (unsigned long long *)err_out);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

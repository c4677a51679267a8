// lrf.hip -- loop restoration: the self-guided (SGRPROJ) stripe filter of a whole plane (SURVEY.md 8f "N3", last stage of
// deblock -> CDEF -> LRF; reference src/lrf.rs: sgrproj_sum_finish 345-363, sgrproj_box_ab_* 176-240,
// sgrproj_box_f_r0/_r1/_r2 242-341, VertPaddedIter / HorzPaddedIter 402-524, setup_integral_image 530-627,
// sgrproj_stripe_filter 630-830, RestorationState::lrf_filter_frame 1482-1585; the encoder never selects the Wiener
// filter, src/rdo.rs:2508).
//
// The reference walks stripe by stripe and restoration unit by unit, builds an integral image of the padded stripe and
// rolls three / two rows of (a, b) intermediates down the stripe.  Every output pixel, however, only depends on the
// padded stripe within 3 pixels of it, so here:
//   * one WORKGROUP per (stripe, 32-column chunk of a restoration unit);
//   * the padded chunk ((32 + 7) x (stripe + 6) pixels: rows outside the stripe from the deblocked plane -- at most two --
//     then replicated, columns outside the unit real up to 4 / 3 pixels, replicated at the frame edge) is staged into
//     LDS once;
//   * the (a, b) pairs of both passes are computed for the whole chunk by direct 3x3 / 5x5 box sums from LDS (exact: the
//     integral image's wrapping differences are these sums) and parked in LDS packed into one dword (a <= 256: 9 bits,
//     b < 2^21);
//   * every thread then finishes 8 pixels: the weighted (a, b) stencils, the projection with xqd, clamp, store.
// u32 arithmetic wraps where the reference's release build wraps (p * s).
// All of that is the tile engine sgr_tile, in sgr_common.hpp; this file is the frame filter on it.  The restoration leg
// of rdo_loop_decision, which runs the same engine on RDO units, is lrf_search.hip.
#include "common.hpp"
#include "sgr_common.hpp"

namespace {
using namespace r1sgr;

struct LrfGeom {
  int ydec, crop_w, crop_h, stripe_n, unit_size, unit_cols, unit_rows, stripe_height, bd, chunks;   // 32-column chunks
};

template <int BPP>
__global__ __launch_bounds__(256) void k_lrf_sgr(R1Plane cdeffed, R1Plane deblocked, R1Plane out,
                                                 LrfGeom g, const R1LrfUnit *__restrict__ units) {
  const int si = blockIdx.y, chunk = blockIdx.x;
  // stripe geometry (lrf.rs:1507-1517)
  int y0, sh_;
  if (si == 0) {
    y0 = 0;
    sh_ = (64 - 8) >> g.ydec;
  } else {
    y0 = (si * 64 - 8) >> g.ydec;
    const int rest = g.crop_h - y0;
    sh_ = (64 >> g.ydec) < rest ? (64 >> g.ydec) : rest;
  }
  if (sh_ <= 0) return;
  // unit of this chunk (the last unit stretches to the crop width)
  const int cx0 = chunk * TW;
  if (cx0 >= g.crop_w) return;
  int rux = cx0 / g.unit_size;
  rux = rux < g.unit_cols - 1 ? rux : g.unit_cols - 1;
  const int x0 = rux * g.unit_size;
  const int uw = rux == g.unit_cols - 1 ? g.crop_w - x0 : g.unit_size;
  int ruy = si * g.stripe_height / g.unit_size;
  ruy = ruy < g.unit_rows - 1 ? ruy : g.unit_rows - 1;
  const R1LrfUnit u = units[ruy * g.unit_cols + rux];
  if (u.filter != 3) return;   // RESTORE_NONE: `out` already holds the CDEF output
  SgrTile t;
  t.x0 = x0; t.y0 = y0; t.uw = uw; t.uh = sh_;
  t.lu = x0 == 0 ? 0 : 4; t.top = 2;
  t.crop_w = g.crop_w; t.crop_h = g.crop_h;
  t.cx0 = cx0; t.ty0 = 0;
  t.tw = (x0 + uw - cx0) < TW ? (x0 + uw - cx0) : TW;
  t.th = sh_;
  const int w0 = u.xqd[0], w1 = u.xqd[1], w2 = 128 - w0 - w1;
  const int32_t pmax = (1 << g.bd) - 1;
  sgr_tile<BPP, 64, BPP == 1>(cdeffed, deblocked, t, u.set, BPP == 1 ? 8 : g.bd, nullptr, 0, 0,
                              [&](int x, int y, uint32_t p, uint32_t f1, uint32_t f2, uint32_t) {
    const int32_t o = sgr_project(p, f1, f2, w0, w1, w2, pmax);
    uint8_t *d = (uint8_t *)px_addr<BPP>(out, cx0 + x, y0 + y);
    if constexpr (BPP == 1) *d = (uint8_t)o;
    else *(uint16_t *)d = (uint16_t)o;
  }, [] {});
}

}  // namespace

extern "C" int r1_lrf_sgrproj_plane(r1_ctx *ctx, const R1Plane *cdeffed, const R1Plane *deblocked, const R1Plane *out,
                                    int ydec, int crop_w, int crop_h, int frame_height, int unit_size, int unit_cols,
                                    int unit_rows, int stripe_height, const R1LrfUnit *units, void *stream) {
  R1_REQUIRE(ctx && cdeffed && deblocked && out && units);
  R1_REQUIRE(r1_offsets_fit_u32(*cdeffed) && r1_offsets_fit_u32(*deblocked));   // 32-bit byte offsets in the tile loads
  R1_REQUIRE(r1_same_px(*cdeffed, *deblocked, *out));
  R1_REQUIRE(r1_px_ok(*cdeffed));
  R1_REQUIRE(r1_px_fits_depth(*cdeffed));
  R1_REQUIRE(cdeffed->data != out->data);   // the filter reads CDEF output around what it writes
  R1_REQUIRE(ydec >= 0 && ydec <= 1 && crop_w > 0 && crop_h > 0 && frame_height > 0);
  R1_REQUIRE(unit_size >= 32 && unit_size <= 256 && unit_size % 32 == 0);
  R1_REQUIRE(unit_cols > 0 && unit_rows > 0 && (stripe_height == 64 || stripe_height == 32));
  R1_REQUIRE((unit_cols - 1) * unit_size < crop_w);
  const LrfGeom g = {ydec, crop_w, crop_h, /* stripe_n */ (frame_height + 7) / 64 + 1, unit_size, unit_cols, unit_rows,
                     stripe_height, /* bd */ cdeffed->bit_depth, /* chunks */ (crop_w + TW - 1) / TW};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.chunks, g.stripe_n);
  r1_by_bpp(cdeffed->bytes_per_px, [&](auto B) {
    hipLaunchKernelGGL((k_lrf_sgr<B.value>), grid, dim3(256), 0, st, *cdeffed, *deblocked, *out, g, units);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

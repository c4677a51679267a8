// sgr_common.hpp -- what every self-guided (SGRPROJ) kernel shares: the tile engine sgr_tile (lrf.hip's header has the
// reference's line numbers and the mapping) and, behind it, the steps that the frame filter (lrf.hip) and the restoration
// leg of rdo_loop_decision (lrf_search.hip) would otherwise write out per kernel.  Device code, but for sgr_block_dim;
// the tables are file-local to each unit that includes this.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace r1sgr {

static __constant__ uint16_t kSgrS[16][2] = {{140, 3236}, {112, 2158}, {93, 1618}, {80, 1438}, {70, 1295},
                                      {58, 1177},  {47, 1079},  {37, 996},  {30, 925},  {25, 863},
                                      {0, 2589},   {0, 1618},   {0, 1177},  {0, 925},   {56, 0},
                                      {22, 0}};

constexpr int TW = 32;                 // chunk width
constexpr int SW = TW + 7;             // padded chunk width
constexpr int AW = TW + 2;             // (a, b) columns: centres -1 .. TW

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a(z) of sgrproj_sum_finish (lrf.rs:352-358): 256 for z >= 255, 1 for z = 0, else ((z << 8) + z / 2) / (z + 1)
// -- 255 quotients, tabulated at compile time instead of an integer division (~40 instructions) per (a, b) pair
struct SgrATable {
  uint16_t v[256];
  constexpr SgrATable() : v() {
    for (int z = 0; z < 256; z++) v[z] = (uint16_t)(z >= 255 ? 256 : (z == 0 ? 1 : ((z << 8) + z / 2) / (z + 1)));
  }
};
static __device__ const SgrATable kSgrA = SgrATable();

// Full-rate 24-bit multiplies, spelled out: where an operand is carried around a loop the instruction selector's
// known-bits walk loses the range and __umul24 comes out as the quarter-rate v_mul_lo_u32 (same finding as
// tx_common.hpp's m24).  Callers state the operand ranges.
__device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_mul_u32_u24_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ int32_t mad_i24(int32_t a, int32_t b, int32_t c) {
  int32_t r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Byte offset of pixel (x, y) from the start of a plane's allocation, in 32 bits with the full-rate multiplier: the
// entry points require stride, alloc_height < 2^24 and an allocation below 4 GiB (r1_offsets_fit_u32).  A load at
// `data + offset` then takes the uniform base from SGPRs and needs no 64-bit vector arithmetic (px_addr is a
// quarter-rate 64-bit multiply-add per address: 20 of them per thread and tile here).
template <int BPP>
__device__ __forceinline__ uint32_t px_off(const R1Plane &p, int x, int y) {
  return mad_u24((uint32_t)(p.yorigin + y), (uint32_t)p.stride, (uint32_t)(p.xorigin + x)) * BPP;
}
template <int BPP>
__device__ __forceinline__ uint32_t ld_px_at(const R1Plane &p, uint32_t off) {
  return ld_px<BPP>((const uint8_t *)p.data + off);
}

// sgrproj_sum_finish -> a | b << 9.  Every product but (for bit depth 12) the last has operands below 2^24 whatever
// the bit depth -- the sums are scaled to the 8-bit range first: scaled_ssq <= 25 * 2^16, scaled_sum <= 25 * 2^8,
// p = n * ssq - sum^2 <= n^2 * (255 / 2)^2 + rounding < 2^24 (the min below keeps the full-rate multiplier exact
// even if that bound were wrong: z saturates at 255 from p * s >= 255 << 20 on, and (2^24 - 1) * 22 is past it),
// (256 - a) * sum <= 255 * 25 * 4095 < 2^25 and, for bit depths up to 10 (NARROW), < 2^23
template <bool NARROW>
__device__ __forceinline__ uint32_t sum_finish(uint32_t ssq, uint32_t sum, uint32_t n,
                                               uint32_t one_over_n, uint32_t s, int bd, const uint16_t *atab) {
  const int sh = bd - 8;
  const uint32_t scaled_ssq = (ssq + ((1u << (2 * sh)) >> 1)) >> (2 * sh);
  const uint32_t scaled_sum = (sum + ((1u << sh) >> 1)) >> sh;
  const int32_t d = (int32_t)__umul24(scaled_ssq, n) - (int32_t)mul_u24(scaled_sum, scaled_sum);
  uint32_t p = (uint32_t)(d > 0 ? d : 0);
  p = p < 0xFFFFFFu ? p : 0xFFFFFFu;
  const uint32_t z = (__umul24(p, s) + (1u << 19)) >> 20;
  const uint32_t a = atab[z < 255u ? z : 255u];
  const uint32_t x = mul_u24((1u << 8) - a, sum);
  const uint32_t b = ((NARROW ? __umul24(x, one_over_n) : x * one_over_n) + (1u << 11)) >> 12;
  return a | (b << 9);
}

// One tile of one unit: columns [cx0, cx0 + tw) (absolute), rows [ty0, ty0 + th)
// relative to the unit's top (ty0 even: the radius-2 pass lives on the odd rows).
struct SgrTile {
  int x0, y0, uw, uh;      // the unit (restoration unit x stripe, or an RDO unit)
  int crop_w, crop_h;      // absolute crop of the plane / of the unit
  int cx0, ty0, tw, th;
  // What setup_integral_image sees left of / above the unit (lrf.rs: `cdeffed.x == 0`, `clamp(y, 0, crop - 1)`): it
  // asks where the unit's slice starts IN ITS PLANE.  The frame filter's plane is the frame: lu = 4 unless x0 == 0,
  // top = 2 (rows above exist down to the plane's row 0).  The restoration search's plane is rdo_loop_decision's
  // scratch copy of the AREA it is deciding (rdo.rs:2277-2296: no padding): a unit in the area's first unit column /
  // row sees nothing left of / above itself, wherever the area lies in the frame -- the caller's edge flags.
  int lu, top;             // real columns left of the unit (0 or 4) / real rows above it (0 or 2)
};
// R1SgrSolveUnit::edges -> (lu, top); a flag is void at the plane's own edge
__device__ __forceinline__ void sgr_unit_edges(SgrTile &t, int edges) {
  t.lu = (edges & R1_SGR_EDGE_LEFT) && t.x0 > 0 ? 4 : 0;
  t.top = (edges & R1_SGR_EDGE_ABOVE) && t.y0 > 0 ? 2 : 0;
}

// Stage the padded tile, compute the (a, b) pairs of both passes, then hand every pixel of the tile to
// `emit(x, y, p, f1, f2, extra)` (x, y tile-relative).
//   TROWS   the most rows a tile of this instantiation has (t.th <= TROWS): sizes the three LDS arrays -- the restoration
//           search runs 32-row tiles where that buys a workgroup per CU, the frame filter 64-row stripes
//   NARROW  the caller guarantees bit depth <= 10: sum_finish's last product fits the full-rate 24-bit multiplier
//   extra_p the pixel of this plane under every pixel of the tile (tile pixel (x, y) <-> plane pixel (ex0 + x, ey0 + y))
//           is loaded for the thread's own pixels BEFORE the tile is staged and handed to emit: the load the caller
//           needs per pixel (the source plane of the moments) is in flight behind the whole tile; null: extra = 0
//   flush() called after every four rows of a thread's column and at its end (a caller accumulating products of
//           14-bit differences in 32 bits moves them to its wide sums there)
// Round 5 (ab10): the tile went on an instruction diet -- the kernel sits at ~80 % of the VALU issue rate, so what
// counts is the count: staging walks rows with a fixed column per thread (47 -> ~15 instructions per element, no
// division in the loop), every multiply whose operands are proven below 2^24 is the full-rate v_mul_u32_u24 /
// v_mad_u32_u24 (v_mul_lo_u32 is quarter rate: 5 per (a, b) pair, 2 per pixel), and the stencil loop is unrolled
// over the thread's rows (even / odd rows of the radius-2 pass resolved at compile time, no register rotation).
//   STRICT  only the unit's own pixels come from inside_p: the columns left of it come from outside_p like the rows
//           above it (the CDEF trial of ONE superblock inside an area whose other superblocks keep their current
//           output, rdo.rs:2458-2489)
template <int BPP, int TROWS, bool NARROW, bool STRICT = false, class Emit, class Flush>
__device__ __forceinline__ void sgr_tile(const R1Plane &inside_p, const R1Plane &outside_p,
                                         const SgrTile &t, int set, int bd, const R1Plane *extra_p, int ex0, int ey0,
                                         Emit emit, Flush flush) {
  static_assert(TROWS % 2 == 0 && TROWS <= 64, "row tiles start on even rows");
  __shared__ uint16_t S[TROWS + 6][SW + 1];
  __shared__ uint32_t ab1[TROWS + 2][AW];
  __shared__ uint32_t ab2[TROWS / 2 + 1][AW];
  const int tid = threadIdx.x;
  // a(z): one table lookup per (a, b) pair; a 512-byte copy per workgroup makes it an LDS read
  __shared__ uint16_t atab_s[256];
  if (tid < 128) ((uint32_t *)atab_s)[tid] = ((const uint32_t *)kSgrA.v)[tid];   // visible after the barrier below
  const uint16_t *atab = atab_s;
  const uint32_t s2 = kSgrS[set & 15][0], s1 = kSgrS[set & 15][1];
  // ---- 0: the thread's pixels of the stencil phase (a column x over `per` rows from y0) and the caller's loads ----
  static_assert(TW == 32, "column = tid & 31");
  constexpr int PER_MAX = (((TROWS + 7) >> 3) + 1) & ~1;
  const int x = tid & (TW - 1);
  const int per = (((t.th + 7) >> 3) + 1) & ~1;
  const int y0 = (tid >> 5) * per;                       // 8 segments
  const int ny = x < t.tw ? (t.th - y0 < per ? t.th - y0 : per) : 0;   // <= 0: nothing to do in phase 3
  uint32_t extra[PER_MAX];
  if (extra_p) {
    const uint32_t o0 = px_off<BPP>(*extra_p, ex0 + x, ey0 + y0);
#pragma unroll
    for (int k = 0; k < PER_MAX; k++) extra[k] = k < ny ? ld_px_at<BPP>(*extra_p, o0 + (uint32_t)(k * extra_p->stride * BPP)) : 0u;
  } else {
#pragma unroll
    for (int k = 0; k < PER_MAX; k++) extra[k] = 0u;
  }
  // ---- 1: padded tile -> LDS (VertPaddedIter / HorzPaddedIter, lrf.rs:402-524) ----
  const int h2 = t.uh + (t.uh & 1), th2 = t.th + (t.th & 1);
  {
    constexpr int SROWS = 256 / SW;          // rows per pass: a thread keeps its column
    const int jj = tid / SW, i = tid - jj * SW;   // S[j][i] <-> unit pixel (cx0 - x0 + i - 4, ty0 + j - 4)
    if (jj < SROWS) {
      const int lu = t.lu;
      int ru = (t.crop_w - t.x0) - t.uw;
      ru = ru < 3 ? ru : 3;
      // (never left of the allocation: px_off's unsigned arithmetic would wrap a negative column to +4 GiB)
      const int xa_ = t.x0 + clampi(t.cx0 - t.x0 + i - 4, -lu, t.uw + ru - 1);
      const int xa = xa_ > -inside_p.xorigin ? xa_ : -inside_p.xorigin;
      const bool one_plane = inside_p.data == outside_p.data;   // workgroup-uniform (the search filters a unit in isolation)
      const int rows = th2 + 6;
      constexpr int NPASS = (TROWS + 6 + SROWS - 1) / SROWS;
      uint32_t v[NPASS];                     // every load of the column in flight before the first LDS store
#pragma unroll
      for (int q = 0; q < NPASS; q++) {
        const int j = jj + q * SROWS;
        const int cy = clampi(t.y0 + t.ty0 + j - 4, 0, t.crop_h - 1);   // (rows past the tile clamp to a valid address)
        const int ly_ = clampi(cy, t.y0 - t.top, t.y0 + h2 + 1);
        const int ly = ly_ > -inside_p.yorigin ? ly_ : -inside_p.yorigin;
        const bool inside = ly >= t.y0 && ly < t.y0 + h2 && (!STRICT || xa >= t.x0);
        if (one_plane) v[q] = ld_px_at<BPP>(inside_p, px_off<BPP>(inside_p, xa, ly));
        else v[q] = inside ? ld_px_at<BPP>(inside_p, px_off<BPP>(inside_p, xa, ly)) : ld_px_at<BPP>(outside_p, px_off<BPP>(outside_p, xa, ly));
      }
#pragma unroll
      for (int q = 0; q < NPASS; q++) {
        const int j = jj + q * SROWS;
        if (j < rows) S[j][i] = (uint16_t)v[q];
      }
    }
  }
  __syncthreads();
  // ---- 2: (a, b) of both passes ----
  // A thread owns a COLUMN of (a, b) centres over a segment of rows and slides the box down: per new
  // centre three (five) pixels of one new row (two new rows for the radius-2 pass, whose centres sit on
  // every other row) instead of the whole 3x3 (5x5) box -- 9 -> 3 and 25 -> 10 LDS reads per centre.
  {
    constexpr int NSEG = 256 / AW;          // row segments per column
    const int seg = tid / AW, c = tid - seg * AW;
    if (seg < NSEG && c <= t.tw + 1) {
      if (s1 > 0) {
        const int rows1 = t.th + 2, per1 = (rows1 + NSEG - 1) / NSEG;
        const int r0 = seg * per1, r1 = r0 + per1 < rows1 ? r0 + per1 : rows1;
        auto row3 = [&](int j, uint32_t &sm, uint32_t &sq) {   // S[j][c + 2 .. c + 4]
          const uint32_t v0 = S[j][c + 2], v1 = S[j][c + 3], v2 = S[j][c + 4];
          sm = v0 + v1 + v2;
          sq = __umul24(v0, v0) + __umul24(v1, v1) + __umul24(v2, v2);
        };
        if (r0 < r1) {
          uint32_t sa, qa, sb, qb, sc, qc;
          row3(r0 + 2, sa, qa);
          row3(r0 + 3, sb, qb);
          for (int r = r0; r < r1; r++) {   // centre (c - 1, r - 1): S rows r + 2 .. r + 4
            row3(r + 4, sc, qc);
            ab1[r][c] = sum_finish<NARROW>(qa + qb + qc, sa + sb + sc, 9, 455, s1, bd, atab);
            sa = sb; qa = qb; sb = sc; qb = qc;
          }
        }
      }
      if (s2 > 0) {
        const int nr = th2 / 2 + 1, per2 = (nr + NSEG - 1) / NSEG;
        const int r0 = seg * per2, r1 = r0 + per2 < nr ? r0 + per2 : nr;
        auto row5 = [&](int j, uint32_t &sm, uint32_t &sq) {   // S[j][c + 1 .. c + 5]
          sm = 0; sq = 0;
#pragma unroll
          for (int dx = 0; dx < 5; dx++) {
            const uint32_t v = S[j][c + 1 + dx];
            sm += v;
            sq += __umul24(v, v);
          }
        };
        if (r0 < r1) {
          uint32_t m1, q1, m2, q2, m3, q3, m4, q4, m5, q5;
          row5(2 * r0 + 1, m1, q1);
          row5(2 * r0 + 2, m2, q2);
          row5(2 * r0 + 3, m3, q3);
          for (int r = r0; r < r1; r++) {   // centre (c - 1, 2 r - 1): S rows 2 r + 1 .. 2 r + 5
            row5(2 * r + 4, m4, q4);
            row5(2 * r + 5, m5, q5);
            ab2[r][c] = sum_finish<NARROW>(q1 + q2 + q3 + q4 + q5, m1 + m2 + m3 + m4 + m5, 25, 164, s2, bd, atab);
            m1 = m3; q1 = q3; m2 = m4; q2 = q4; m3 = m5; q3 = q5;
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- 3: the weighted stencils ----
  // A thread owns a pixel COLUMN over a segment of rows (an even number of them: the radius-2 pass pairs
  // rows) and walks down: the 3x3 stencil of the radius-1 pass is (3 4 3) on its outer rows and (4 4 4)
  // on the middle one, so a row of (a, b) pairs is read once and its two horizontal forms kept; the
  // radius-2 pass reads one row of pairs per TWO pixel rows.  Weight sums: A <= 32 * 256, p < 2^12: 24-bit products.
  if (ny > 0) {
    auto row1 = [&](int j, uint32_t &oa, uint32_t &ob, uint32_t &ma, uint32_t &mb) {   // ab1 row j at x .. x + 2
      const uint32_t v0 = ab1[j][x], v1 = ab1[j][x + 1], v2 = ab1[j][x + 2];
      const uint32_t a0 = v0 & 511u, a1 = v1 & 511u, a2 = v2 & 511u;
      const uint32_t b0 = v0 >> 9, b1 = v1 >> 9, b2 = v2 >> 9;
      const uint32_t as = a0 + a2, bs = b0 + b2;
      oa = 3u * as + 4u * a1;
      ob = 3u * bs + 4u * b1;
      ma = 4u * (as + a1);
      mb = 4u * (bs + b1);
    };
    auto row2 = [&](int r, uint32_t &ha, uint32_t &hb) {   // ab2 row r at x .. x + 2: (5 6 5)
      const uint32_t v0 = ab2[r][x], v1 = ab2[r][x + 1], v2 = ab2[r][x + 2];
      ha = 5u * ((v0 & 511u) + (v2 & 511u)) + 6u * (v1 & 511u);
      hb = 5u * ((v0 >> 9) + (v2 >> 9)) + 6u * (v1 >> 9);
    };
    // one straight-line body per (radius-1 pass on, radius-2 pass on): the parameter set is workgroup-uniform
    auto stencil = [&](auto has1, auto has2) {
      constexpr bool H1 = decltype(has1)::value, H2 = decltype(has2)::value;
      uint32_t oa0 = 0, ob0 = 0, oa1 = 0, ob1 = 0, ma1 = 0, mb1 = 0, dump_a, dump_b;
      if constexpr (H1) {
        row1(y0, oa0, ob0, dump_a, dump_b);
        row1(y0 + 1, oa1, ob1, ma1, mb1);
      }
      uint32_t ha0 = 0, hb0 = 0;
      if constexpr (H2) row2(y0 / 2, ha0, hb0);
#pragma unroll
      for (int k = 0; k < PER_MAX; k += 2) {
        if (k < ny) {
          const int y = y0 + k;                                   // an even row and, below, the odd row after it
          const uint32_t pe = S[y + 4][x + 4];
          uint32_t f1 = pe << 4, f2 = pe << 4, ha1 = 0, hb1 = 0;   // sgrproj_box_f_r0 once per row pair: the odd row
          if constexpr (H1) {                                     // reuses the even row's value
            uint32_t oa2, ob2, ma2, mb2;
            row1(y + 2, oa2, ob2, ma2, mb2);
            f1 = mad_u24(oa0 + ma1 + oa2, pe, ob0 + mb1 + ob2 + (1u << 8)) >> 9;
            oa0 = oa1; ob0 = ob1;
            oa1 = oa2; ob1 = ob2; ma1 = ma2; mb1 = mb2;
          }
          if constexpr (H2) {
            row2(y / 2 + 1, ha1, hb1);
            f2 = mad_u24(ha0 + ha1, pe, hb0 + hb1 + (1u << 8)) >> 9;
          }
          emit(x, y, pe, f1, f2, extra[k]);
          if (k + 1 < ny) {
            const uint32_t po = S[y + 5][x + 4];
            if constexpr (H1) {
              uint32_t oa2, ob2, ma2, mb2;
              row1(y + 3, oa2, ob2, ma2, mb2);
              f1 = mad_u24(oa0 + ma1 + oa2, po, ob0 + mb1 + ob2 + (1u << 8)) >> 9;
              oa0 = oa1; ob0 = ob1;
              oa1 = oa2; ob1 = ob2; ma1 = ma2; mb1 = mb2;
            } else {
              f1 = po << 4;
            }
            if constexpr (H2) {
              f2 = mad_u24(ha1, po, hb1 + (1u << 7)) >> 8;
              ha0 = ha1; hb0 = hb1;
            }
            emit(x, y + 1, po, f1, f2, extra[k + 1]);
          }
          if ((k & 2) != 0) flush();
        }
      }
      flush();
    };
    if (s1 > 0 && s2 > 0) stencil(std::true_type(), std::true_type());
    else if (s1 > 0) stencil(std::true_type(), std::false_type());
    else if (s2 > 0) stencil(std::false_type(), std::true_type());
    else stencil(std::false_type(), std::false_type());
  }
}

// The tile -- TW columns, TR rows -- at (tx0, ty0) of a unit that is filtered in isolation: hard-clipped to itself on the
// right and below (rdo.rs:2651-2666; the CDEF trial's superblock rdo.rs:2458-2466), the caller's edge flags left and above
template <int TR>
__device__ __forceinline__ SgrTile sgr_unit_tile(int x, int y, int w, int h, int edges, int tx0, int ty0) {
  SgrTile t;
  t.x0 = x; t.y0 = y; t.uw = w; t.uh = h;
  sgr_unit_edges(t, edges);
  t.crop_w = x + w; t.crop_h = y + h;
  t.cx0 = x + tx0; t.ty0 = ty0;
  t.tw = (w - tx0) < TW ? (w - tx0) : TW;
  t.th = (h - ty0) < TR ? (h - ty0) : TR;
  return t;
}
// apply_filter (lrf.rs:796-815): pixel p and its two filter outputs projected with the weights, clamped to pmax
__device__ __forceinline__ int32_t sgr_project(uint32_t p, uint32_t f1, uint32_t f2, int w0, int w1, int w2, int32_t pmax) {
  const int32_t v = w0 * (int32_t)f2 + w1 * (int32_t)(p << 4) + w2 * (int32_t)f1;
  const int32_t s = (v + (1 << 10)) >> 11;
  return s < 0 ? 0 : (s > pmax ? pmax : s);
}
// sgrproj_solve's five moments (lrf.rs:1010-1054) of one pixel: p filtered to (f1, f2), s the source pixel under it
__device__ __forceinline__ void sgr_moments_add(long long *m, uint32_t p, uint32_t f1, uint32_t f2, uint32_t s) {
  const int32_t uu = (int32_t)(p << 4);
  const long long sv = ((int32_t)s << 4) - uu;
  const long long g2 = (int32_t)f2 - uu, g1 = (int32_t)f1 - uu;
  m[0] += g2 * g2; m[1] += g1 * g1; m[2] += g1 * g2; m[3] += g2 * sv; m[4] += g1 * sv;
}
// ... summed over each wave -> part[wave] (LDS); the caller's barrier comes next
__device__ __forceinline__ void sgr_moments_park(const long long *m, long long (*part)[5]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const long long v = (long long)xor_sum_u64((unsigned long long)m[k], WAVE);
    if (lane == 0) part[wave][k] = v;
  }
}
// The "no filter option" of a unit: the gw x gh pixels of `p` from (px, py) as they are -> F (LDS; its row length ROW is
// a constant: no runtime division)
template <int BPP, int ROW, typename T>
__device__ __forceinline__ void sgr_stage_unfiltered(T (*F)[ROW], const R1Plane &p, int px, int py, int gw, int gh) {
  for (int e = threadIdx.x; e < gh * ROW; e += 256) {
    const int y = e / ROW, x = e % ROW;
    if (x < gw) F[y][x] = (T)ld_px<BPP>(px_addr<BPP>(p, px + x, py + y));
  }
}
// The block-grid margin of a restored w x h rectangle: what of gw x gh (the rectangle out to whole blocks) lies outside
// it is never written by the filter and holds the restored plane's initial fill.  The test is workgroup-uniform.
template <int ROW, typename T>
__device__ __forceinline__ void sgr_fill_margin(T (*F)[ROW], int w, int h, int gw, int gh) {
  if (gw != w || gh != h)
    for (int e = threadIdx.x; e < gh * ROW; e += 256) {
      const int y = e / ROW, x = e % ROW;
      if (x < gw && (x >= w || y >= h)) F[y][x] = (T)R1_PLANE_NEW_FILL;
    }
}
// a side of rdo_loop_plane_error's block (rdo.rs:2039-2043: 8x8 luma pixels) in the pixels of a plane decimated by dec
__host__ __device__ __forceinline__ int sgr_block_dim(bool chroma, int dec) { return chroma ? 8 >> dec : 8; }

}  // namespace r1sgr

// cand_common.hpp -- what the fused candidate kernel (rdo_cand_kernel.hpp), the RDO-time sub-pel search
// (me_blocks.hip), the put / prep of transform-sized blocks (mc.hip, k_mc_fast; mc_mfma.hip) and the compound
// candidate (mc_compound.hip) share: the DPP Hadamard (SATD with lane = column) and its LDS-tile form for the fused
// kernel, v_sad, the packed i16 helpers, and the put_8tap / prep_8tap column filters on v_dot4 / v_dot2 with their
// packed tap tables and tap loads -- and, for the fused kernel's 64x64 and 32x32, the horizontal taps on the matrix pipe.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "dist_common.hpp"
#include "mc_common.hpp"

namespace r1cand {

// kTapI8 / kTapI16 / kTapB, static: a unit carries the tables it reads and no others
#include "mc_taps_packed.inc"

// ---- cross-lane Hadamard with DPP --------------------------------------
// DPP controls: quad_perm [1,0,3,2] = 0xB1 (lane ^ 1), [2,3,0,1] = 0x4E
// (lane ^ 2), row_half_mirror = 0x141 (lane -> 7 - lane inside each 8).
template <int CTRL>
__device__ __forceinline__ int32_t dpp(int32_t x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
}
// One butterfly stage across lanes: partner value p, the "lower" lane of a
// pair keeps x + p, the "upper" lane p - x.  sm = upper ? -1 : 0.
template <int CTRL>
__device__ __forceinline__ int32_t bfly_lanes(int32_t x, int32_t sm) {
  // +-x + partner as one v_mad_i32_i24 (|x| < 2^19 for 12-bit pixels)
  return __mul24(x, sm | 1) + dpp<CTRL>(x);
}
// |Hadamard across the TS lanes of a tile| of x, as this lane's share of the
// tile's sum: the last butterfly stage is folded into the abs because
// |a + b| + |a - b| = 2 max(|a|, |b|) -- each lane of the final pair
// contributes max(|a|, |b|).
// The 8-lane version pairs lanes with masks {1, 2, 7}: those span (Z/2)^3, so
// the three stages are a Walsh-Hadamard transform in a relabelled lane order
// -- the same multiset of coefficients as masks {1, 2, 4}, hence the same sum
// of absolute values (dist.rs:214).  "Upper" lanes are those whose coordinate
// w.r.t. the basis {1, 2, 7} is 1: y1 = b0 ^ b2, y2 = b1 ^ b2 (y3 = b2).
struct LaneSigns { int32_t s1, s2; };
template <int TS>
__device__ __forceinline__ LaneSigns lane_signs(int lane) {
  LaneSigns s;
  if constexpr (TS == 8) {
    s.s1 = -(int32_t)((lane ^ (lane >> 2)) & 1);
    s.s2 = -(int32_t)(((lane >> 1) ^ (lane >> 2)) & 1);
  } else {
    s.s1 = -(int32_t)(lane & 1);
    s.s2 = 0;
  }
  return s;
}
template <int TS>
__device__ __forceinline__ uint32_t habs_lanes(int32_t x, LaneSigns sg) {
  x = bfly_lanes<0xB1>(x, sg.s1);
  if constexpr (TS == 8) x = bfly_lanes<0x4E>(x, sg.s2);
  const int32_t ax = iabs32(x);
  const int32_t ap = TS == 8 ? dpp<0x141>(ax) : dpp<0x4E>(ax);
  return (uint32_t)(ax > ap ? ax : ap);
}

__device__ __forceinline__ uint32_t sad_u32(uint32_t a, uint32_t b, uint32_t acc) {
  uint32_t r;
  asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
  return r;
}

// ---- the same on two i16 per register (VOP3P) ------------------------------
// For pixels of up to 10 bits the 8x8 Hadamard fits i16 until its last stage:
// |residual| <= 1023, five butterfly stages reach 32 * 1023 = 32736, and the
// sixth stage is the max(|a|, |b|) fold above.  Two 8-row groups of a column
// (or the two halves of one group after its first stage) share a register, so
// every butterfly, abs and max works on two coefficients per lane per issue.
typedef short v2s_t __attribute__((ext_vector_type(2)));
typedef unsigned short v2us_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, (v2s_t)(__builtin_bit_cast(v2s_t, a) + __builtin_bit_cast(v2s_t, b)));
}
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, (v2s_t)(__builtin_bit_cast(v2s_t, a) - __builtin_bit_cast(v2s_t, b)));
}
__device__ __forceinline__ uint32_t pk_mad(uint32_t x, uint32_t s, uint32_t p) {
  uint32_t r;
  asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(s), "v"(p));
  return r;
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// both halves of (lo, hi) from the low halves of two i32
__device__ __forceinline__ uint32_t pk_pair(int32_t lo, int32_t hi) {
  return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u);
}
// The first two stages of the 8-point butterfly on packed registers, in the order of dist.rs:95-117.  The third
// (the sum and the difference of d[k] and d[k + 4], k = 0 .. 3) stays with each caller, formed where it is consumed:
// satd_tile_rows folds it into an abs, and with the eight outputs formed ahead of their uses (one function,
// uint32_t[8] out) the kernels came out in another instruction order (profiles/HISTORY.md).
__device__ __forceinline__ void pk_bfly8_s2(const uint32_t (&a)[8], uint32_t (&d)[8]) {
  uint32_t b[8];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    b[2 * k] = pk_add(a[2 * k], a[2 * k + 1]);
    b[2 * k + 1] = pk_sub(a[2 * k], a[2 * k + 1]);
  }
  d[0] = pk_add(b[0], b[2]); d[2] = pk_sub(b[0], b[2]);
  d[1] = pk_add(b[1], b[3]); d[3] = pk_sub(b[1], b[3]);
  d[4] = pk_add(b[4], b[6]); d[6] = pk_sub(b[4], b[6]);
  d[5] = pk_add(b[5], b[7]); d[7] = pk_sub(b[5], b[7]);
}
// this lane's share of sum |Hadamard across the 8 lanes| for both halves of x,
// added to acc; m1 / m2: packed +-1 of the two lane stages
__device__ __forceinline__ uint32_t habs_lanes_pk(uint32_t x, uint32_t m1, uint32_t m2, uint32_t acc) {
  x = pk_mad(x, m1, (uint32_t)dpp<0xB1>((int32_t)x));
  x = pk_mad(x, m2, (uint32_t)dpp<0x4E>((int32_t)x));
  const uint32_t ax = pk_max(x, pk_sub(0u, x));
  const uint32_t mx = pk_max(ax, (uint32_t)dpp<0x141>((int32_t)ax));
  return __builtin_amdgcn_udot2(__builtin_bit_cast(v2us_t, mx), __builtin_bit_cast(v2us_t, 0x00010001u),
                                acc, false);
}

// (lo >> sh) in the low half, (hi >> sh) in the high half.  (Tried in round 3: the second shift as
// an SDWA write into the upper word of the first one's register -- two instructions instead of
// three.  +0.5 % and NOT bit-exact in the 8-bit kernels, with or without the dst_sel wait state;
// profiles/r03_ab_notes.md.  v_perm it stays.)
__device__ __forceinline__ uint32_t ashr_pair(int32_t lo, int32_t hi, int sh) {
  return __builtin_amdgcn_perm((uint32_t)(hi >> sh), (uint32_t)(lo >> sh), 0x05040100u);
}

// First link of a dot-product chain with a constant accumulator: the VOP3P
// forms take the constant as an operand (inline 0 / 64, or an SGPR), whereas
// the compiler's choice -- the accumulate-in-place v_dot*c forms -- needs a
// v_mov to seed the accumulator first.  One instruction instead of two.
__device__ __forceinline__ int32_t dot2_seed0(uint32_t a, uint32_t b) {
  int32_t r;
  asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ int32_t dot2_seed64(uint32_t a, uint32_t b) {
  int32_t r;
  asm("v_dot2_i32_i16 %0, %1, %2, 64" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ int32_t dot2_seed(uint32_t a, uint32_t b, int32_t c_uniform) {
  int32_t r;
  asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c_uniform));
  return r;
}
__device__ __forceinline__ int32_t dot4_seed(uint32_t a, uint32_t b, int32_t c_uniform) {
  int32_t r;
  asm("v_dot4_i32_i8 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c_uniform));
  return r;
}

// ---- the taps of one candidate ----------------------------------------------
// Loaded ahead of their use (the fused kernel fetches them with the window).  8-bit pixels: the x-taps halved, as
// i8 for v_dot4 (see mc8_column_t); 16-bit pixels: i16 pairs on both axes.
template <int BPP> struct Taps;
template <> struct Taps<1> { uint32_t fx0, fx1, ty[4]; };
template <> struct Taps<2> { uint32_t tx[4], ty[4]; };
template <int BPP, int W, int H>
__device__ __forceinline__ Taps<BPP> load_taps(int cf, int rf, int mx, int my) {
  const int fxi = r1mc::filter_index(mx, W), fyi = r1mc::filter_index(my, H);
  Taps<BPP> t;
  if constexpr (BPP == 1) {
    t.fx0 = kTapI8[fxi][cf][0];
    t.fx1 = kTapI8[fxi][cf][1];
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if constexpr (BPP == 2) t.tx[j] = kTapI16[fxi][cf][j];
    t.ty[j] = kTapI16[fyi][rf][j];
  }
  return t;
}
// wave-uniform: do all (active) lanes' filters have zero outer taps?  (8-bit: the vertical one; 16-bit: both)
__device__ __forceinline__ bool taps_six(const Taps<1> &t) {
  return __all(((t.ty[0] & 0xffffu) | (t.ty[3] >> 16)) == 0);
}
__device__ __forceinline__ bool taps_six(const Taps<2> &t) {
  return __all(((t.ty[0] & 0xffffu) | (t.ty[3] >> 16) | (t.tx[0] & 0xffffu) | (t.tx[3] >> 16)) == 0);
}

// ---- the vertical 8-tap pass on packed row pairs ------------------------------
// The y-taps as i16 pairs serve the even output rows; the odd rows take the same taps moved up by one i16, five pairs
// (0, u0) (u1, u2) .. (u7, 0): R1_ODD_ROW_TAPS, for the three places that run the pass -- mc8_column_t, mc16_column_t
// and k_mc_mfma (mc_mfma.hip).  The pass itself (a rolling window of five packed row pairs, four v_dot2 for the even
// row, five or -- outer taps zero -- three for the odd one) stays written out in each of them: as one function over a
// "next pair" callable the same instructions reached the optimizer in another order, and that alone cost fused
// kernels registers, scratch and a wave per SIMD (profiles/HISTORY.md).  The tap derivation is a macro for the same
// reason: as a function over the two arrays it reordered the 16-bit kernels.
#define R1_ODD_ROW_TAPS(ty, tz)                                                                   \
  do {                                                                                            \
    tz[0] = ty[0] << 16;                                                                          \
    _Pragma("unroll") for (int j = 1; j < 4; j++) tz[j] = __builtin_amdgcn_alignbit(ty[j], ty[j - 1], 16); \
    tz[4] = ty[3] >> 16;                                                                          \
  } while (0)

// ---- 8-bit fast path of put_8tap for one column ---------------------------
// Unified 2-D evaluation.  With x-taps t (sum 128) and y-taps u (sum 128),
// ib = 4 (8-bit): mid = (sum t*p + 4) >> 3, out = clamp((sum u*mid + 1024) >> 11).
//  * col_frac == 0 (t = 128 at tap 3): mid = 16 p exactly, out =
//    (16 S + 1024) >> 11 = (S + 64) >> 7 = round_shift(S, 7)     (mc.rs:272-291)
//  * row_frac == 0 (u = 128 at tap 3): out = (128 mid + 1024) >> 11 =
//    (mid + 8) >> 4 = round_shift(round_shift(S, 3), 4)            (mc.rs:292-312)
//  * both 0: out = p                                              (mc.rs:265-271)
// so one path is bit-exact for all four cases.  The 128 tap does not fit int8,
// but every AV1 tap is even: the i8 table stores t / 2 and the shift is one less.
// PREP: prep_8tap (mc.rs:360-451) -- the i16 intermediate of the same filter,
// (sum u*mid + 64) >> 7 without clamp; the same algebra makes the one path
// exact for its four cases too (mid = 16 p when col_frac == 0, u = 128 picks
// mid when row_frac == 0).
// `six` (wave-uniform): every lane's vertical filter has zero outer taps (REGULAR, SMOOTH, bilinear:
// 6 live taps; only SHARP has 8, mc.rs:110-219).  Then the first and the last window row never meet
// a non-zero tap and the odd output rows' five tap pairs are three: 2 fewer horizontal rows per
// column and one v_dot2 less per pixel pair, the same bits.
// PACK4 (put only; the fused coefficient kernels, rdo_mc_pack4 of rdo_cand_plan.hpp): the packed intermediates are
// 4 * mid, not mid.  The horizontal accumulator 4 * mid + fraction lies in [-7106, 23494] over every row of the tap
// table with the bias below included (tests/test_mc8_pack4.py), so its low 16 bits are the value and clearing the two
// fraction bits of each half after the v_perm leaves 4 * mid there: two instructions per row pair instead of three.
// The vertical sums are then exactly four times what they were, below 2^23 in magnitude, and >> 13 returns the bits
// of >> 11.  Every other caller keeps PACK4 off and its code.
// MXNC (the fused coefficient kernels at 64x64 and 32x32, rdo_mc_matrix of rdo_cand_plan.hpp; 0 = off, every other
// caller, the code it had): the horizontal pass on the matrix pipe.  The wave holds MXNC = 1 or 2 windows, lane =
// (candidate, column); `win` is then the FIRST window of the wave, `lane` the lane and `zero` (MXNC == 2) a run of
// r1mc::mx_zero_bytes zeros.  hacc(r) becomes register r % 4 of quad r / 4: one 8-byte LDS read and one
// v_mfma_i32_16x16x32_i8 per candidate of the wave, with the window bytes as A, the candidate's half-taps as a band in
// B (r1mc::mx_band8, built once per wave) and the bias as C -- the layout, stated with its index algebra in
// mc_window.hpp, hands every lane the four accumulators of its own column, so nothing is moved between lanes and the
// pack, the rolling pairs and the vertical pass below are untouched.  With two candidates the second MFMA accumulates
// into the first one's D, and the row groups of the other candidate read `zero` through the same offsets: no VALU
// instruction per quad.  Bytes past a row's W + 7 meet zero band entries; the rows past H + 6 of the last quad are
// computed and never consumed.  The MFMAs take operands from all 64 lanes: a branch around the call must be one that
// every lane of the wave takes.
// MX4 (the fused coefficient kernels at 16x16 and 8x8 where rdo_mc_matrix4 of rdo_cand_plan.hpp ships them; off = every
// other caller, the code it had): the same pass for waves of four or eight candidates with taps of their own, on
// v_mfma_i32_4x4x4_16b_i8 -- sixteen independent 4x4x4 blocks, a block = four adjacent columns of one candidate (W is a
// multiple of 4), each with its own A and B (r1mc::mx4_*, mc_window.hpp, states the index algebra).  `win` stays the
// lane's OWN window and `c` its column, as on the v_dot4 path.  A quad of window rows is three chained MFMAs on three
// LDS dwords: A_s = the aligned dword s of row 4 q + (c & 3) at the lane's column group, B_s = t0 / t1 / t2 below (the
// half-taps shifted up by c & 3 bytes: what the v_dot4 pass multiplies by), C = the bias.  Register i of D is
// hacc(4 q + i) of the lane's own column: no band builder, no shadow, no v_readlane, nothing moves between lanes.  The
// row past H + 6 of the last quad is read (inside the allocation: r1mc::mx4_a_end) and never consumed.  As with MXNC
// the call must sit under branches the whole wave takes.
typedef int v4i_t __attribute__((ext_vector_type(4)));
template <int W, int H, int WS, bool PREP, bool PACK4 = false, int MXNC = 0, bool MX4 = false>
__device__ __forceinline__ void mc8_column_t(const uint8_t *win, int c, const Taps<1> &tp, int32_t *pred, bool six,
                                             int lane = 0, const uint8_t *zero = nullptr) {
  const uint32_t fx0 = tp.fx0, fx1 = tp.fx1;
  uint32_t ty[4], tz[5];
#pragma unroll
  for (int j = 0; j < 4; j++) ty[j] = tp.ty[j];
  R1_ODD_ROW_TAPS(ty, tz);
  // The i8 table holds h = t / 2 (all AV1 taps are even; sum h = 64).  With the
  // staged q = p - 128:  sum t*p = 2 (sum h*q + 128 * 64), so
  //   mid = (sum t*p + 4) >> 3 = (sum h*q + 8192 + 2) >> 2.
  // put only: the vertical rounding 1024 = 128 * 8 is pre-added to the
  // intermediates (every tap row sums to 128): + 8 after the shift = + 32 before.
  static_assert(!(PREP && PACK4), "the shift-free pack is stated for put_8tap only");
  constexpr int32_t bias = 8192 + 2 + (PREP ? 0 : 32);
  constexpr int WSD = WS / 4;
  const uint32_t *wrow = (const uint32_t *)win + (c >> 2);
  // The lane's 8 window bytes start at byte c & 3 of three aligned dwords.  Instead of moving the
  // PIXELS to the taps (two v_alignbyte per row), the TAPS are moved to the pixels once per lane:
  // the 8 tap bytes shifted up by c & 3 bytes into 12, zero elsewhere -- three v_dot4 per row on
  // the aligned dwords as they come from LDS.
  const uint32_t sh8 = 8u * (uint32_t)(c & 3);
  const uint64_t t64 = (((uint64_t)fx1 << 32) | fx0) << sh8;
  const uint32_t t0 = (uint32_t)t64, t1 = (uint32_t)(t64 >> 32);
  const uint32_t t2 = (uint32_t)(((uint64_t)fx1 << sh8) >> 32);
  // the window holds pixels already biased by -128 (staged with xor 0x80)
  // MXNC: the A fragments' addresses (quad q: + 4 q WS), the band(s), the bias as C, and the quad in flight
  static_assert(MXNC == 0 || ((MXNC == 1 || MXNC == 2) && W == 64 / MXNC && WS % 8 == 0), "matrix pass: 64x64, 32x32");
  const uint8_t *ap0 = win, *ap1 = win;
  long bb0 = 0, bb1 = 0;
  if constexpr (MXNC != 0) {
    const uint8_t *ad = win + r1mc::mx_a_offset(lane, MXNC, H, WS);
    const bool second = MXNC == 2 && r1mc::mx_a_cand(lane, MXNC) == 1;
    ap0 = second ? zero : ad;
    ap1 = second ? ad : zero;
    bb0 = (long)r1mc::mx_band8((uint32_t)__builtin_amdgcn_readlane((int)fx0, 0),
                               (uint32_t)__builtin_amdgcn_readlane((int)fx1, 0), lane);
    if constexpr (MXNC == 2)
      bb1 = (long)r1mc::mx_band8((uint32_t)__builtin_amdgcn_readlane((int)fx0, 32),
                                 (uint32_t)__builtin_amdgcn_readlane((int)fx1, 32), lane);
  }
  // MX4: the row of a quad whose dwords this lane supplies as A (quad q: + 4 q WSD dwords)
  static_assert(!MX4 || (MXNC == 0 && W % 4 == 0 && W <= 16 && 64 % W == 0), "4x4x4 blocks: 16x16, 8x8");
  const uint32_t *arow = wrow + (c & 3) * WSD;
  const v4i_t cbias = {bias, bias, bias, bias};
  v4i_t quad = cbias;
  int quad_at = -1;   // a constant once the calls below are unrolled
  auto hacc = [&](int r) -> int32_t {   // 4 * intermediate + rounding, before the >> 2
    if constexpr (MXNC != 0) {
      if ((r >> 2) != quad_at) {
        quad_at = r >> 2;
        quad = __builtin_amdgcn_mfma_i32_16x16x32_i8(*(const long *)(ap0 + quad_at * 4 * WS), bb0, cbias, 0, 0, 0);
        if constexpr (MXNC == 2)
          quad = __builtin_amdgcn_mfma_i32_16x16x32_i8(*(const long *)(ap1 + quad_at * 4 * WS), bb1, quad, 0, 0, 0);
      }
      return quad[r & 3];
    }
    if constexpr (MX4) {
      if ((r >> 2) != quad_at) {
        quad_at = r >> 2;
        const uint32_t *ar = arow + quad_at * 4 * WSD;
        quad = __builtin_amdgcn_mfma_i32_4x4x4i8((int)ar[0], (int)t0, cbias, 0, 0, 0);
        quad = __builtin_amdgcn_mfma_i32_4x4x4i8((int)ar[1], (int)t1, quad, 0, 0, 0);
        quad = __builtin_amdgcn_mfma_i32_4x4x4i8((int)ar[2], (int)t2, quad, 0, 0, 0);
      }
      return quad[r & 3];
    }
    const uint32_t d0 = wrow[r * WSD], d1 = wrow[r * WSD + 1], d2 = wrow[r * WSD + 2];
    int32_t acc = dot4_seed(d0, t0, bias);
    acc = __builtin_amdgcn_sdot4((int)d1, (int)t1, acc, false);
    acc = __builtin_amdgcn_sdot4((int)d2, (int)t2, acc, false);
    return acc;
  };
  auto hpair = [&](int r) -> uint32_t {   // rows r, r+1 packed as i16 x 2
    // the last pair has no second row: its upper half only ever meets a zero tap (tz[4]'s high half)
    if constexpr (PACK4) {
      if (r + 1 < H + 7) return pk_pair(hacc(r), hacc(r + 1)) & 0xfffcfffcu;
      return (uint32_t)hacc(r) & 0xfffffffcu;
    } else {
      if (r + 1 < H + 7) return ashr_pair(hacc(r), hacc(r + 1), 2);
      return (uint32_t)(hacc(r) >> 2);
    }
  };
  // rolling window of 5 packed pairs: output rows 2j and 2j+1 need the
  // intermediates 2j .. 2j+8
  auto body = [&](auto six_tag) {
    constexpr bool SIX = decltype(six_tag)::value;
    uint32_t pk[5];
    // SIX: window row 0 only meets u0 = 0 -- the pair (row 0, row 1) is (anything, row 1)
    if constexpr (PACK4) pk[0] = SIX ? ((uint32_t)hacc(1) & 0xfffcu) << 16 : hpair(0);
    else pk[0] = SIX ? (uint32_t)(hacc(1) >> 2) << 16 : hpair(0);
#pragma unroll
    for (int j = 1; j < 4; j++) pk[j] = hpair(2 * j);
#pragma unroll
    for (int j = 0; j < H / 2; j++) {
      // SIX: the last window row (H + 6) only meets u7 = 0
      if (!SIX || j + 1 < H / 2) pk[4] = hpair(2 * j + 8);
      // put: the rounding is already inside the intermediates; prep: + 64
      int32_t a0 = PREP ? dot2_seed64(pk[0], ty[0]) : dot2_seed0(pk[0], ty[0]);
#pragma unroll
      for (int k = 1; k < 4; k++)
        a0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, pk[k]),
                                    __builtin_bit_cast(v2s_t, ty[k]), a0, false);
      int32_t a1;
      if constexpr (SIX) {   // tz[0] = (0, u0) and tz[4] = (u7, 0) are zero
        a1 = PREP ? dot2_seed64(pk[1], tz[1]) : dot2_seed0(pk[1], tz[1]);
#pragma unroll
        for (int k = 2; k < 4; k++)
          a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, pk[k]),
                                      __builtin_bit_cast(v2s_t, tz[k]), a1, false);
      } else {
        a1 = PREP ? dot2_seed64(pk[0], tz[0]) : dot2_seed0(pk[0], tz[0]);
#pragma unroll
        for (int k = 1; k < 5; k++)
          a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, pk[k]),
                                      __builtin_bit_cast(v2s_t, tz[k]), a1, false);
      }
      if constexpr (PREP) {
        pred[2 * j] = a0 >> 7;
        pred[2 * j + 1] = a1 >> 7;
      } else {
        a0 >>= PACK4 ? 13 : 11;
        a1 >>= PACK4 ? 13 : 11;
        pred[2 * j] = a0 < 0 ? 0 : (a0 > 255 ? 255 : a0);
        pred[2 * j + 1] = a1 < 0 ? 0 : (a1 > 255 ? 255 : a1);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) pk[k] = pk[k + 1];
    }
  };
  if (six) body(std::true_type{});
  else body(std::false_type{});
}

// ---- 10/12-bit fast path of put_8tap for one column -------------------------
// Same unified evaluation as mc8_column_t, on u16 pixels: intermediate_bits
// ib = 4 (10-bit) or 2 (12-bit);  mid = (sum t*p + 2^(6-ib)) >> (7-ib) fits
// i16 (mc.rs:314,326), out = clamp((sum u*mid + 2^(6+ib)) >> (7+ib)).
//  * col_frac == 0 (t = 128 at tap 3): mid = p << ib exactly, out =
//    (2^ib * S + 2^(6+ib)) >> (7+ib) = round_shift(S, 7)           (mc.rs:272-291)
//  * row_frac == 0 (u = 128 at tap 3): out = (128 mid + 2^(6+ib)) >> (7+ib)
//    = round_shift(mid, ib)                                         (mc.rs:292-312)
//  * both 0: out = p                                               (mc.rs:265-271)
// The taps (128 included) and the pixels (<= 4095) fit i16, so the 8 horizontal
// taps are 4 v_dot2_i32_i16 on pixel pairs funnel-shifted to the lane's
// column, and the vertical taps 4-5 v_dot2_i32_i16 on packed intermediates.
// The rounding of the vertical pass is pre-added to the intermediates:
// 2^(6+ib) = 128 * 2^(ib-1) and every tap row sums to 128.
// PREP: (sum u*mid + 64) >> 7 - PREP_BIAS (8192), no clamp (mc.rs:355-451).
template <int W, int H, int WS, bool PREP>
__device__ __forceinline__ void mc16_column_t(const uint8_t *win, int c, const Taps<2> &tp, int bit_depth,
                                              int32_t *pred, bool six) {
  // `six` (wave-uniform): BOTH filters of every lane have zero outer taps (see mc8_column_t); the
  // fifth horizontal tap pair is then zero for odd columns as it always is for even ones
  uint32_t tx[4], ty[4], tz[5];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    tx[j] = tp.tx[j];
    ty[j] = tp.ty[j];
  }
  R1_ODD_ROW_TAPS(ty, tz);
  const int ib = r1mc::intermediate_bits(bit_depth);
  const int hsh = 7 - ib, vsh = 7 + ib;
  // H rounding, plus (put only) the V rounding 2^(ib-1) << hsh = 64 folded into mid
  const int32_t hbias = (1 << (6 - ib)) + (PREP ? 0 : 64);
  const int32_t maxv = (1 << bit_depth) - 1;
  constexpr int WSD = WS / 4;
  const uint32_t *wrow = (const uint32_t *)win + (c >> 1);
  // as in mc8_column_t the taps go to the pixels: the 8 x-taps shifted up by one i16 for odd
  // columns into five dwords -- five v_dot2 per row on aligned LDS dwords (was 4 v_alignbit + 4)
  const bool odd = c & 1;
  uint32_t u[5];
  u[0] = odd ? tx[0] << 16 : tx[0];
#pragma unroll
  for (int j = 1; j < 4; j++) u[j] = odd ? __builtin_amdgcn_alignbit(tx[j], tx[j - 1], 16) : tx[j];
  u[4] = odd ? tx[3] >> 16 : 0u;
  auto body = [&](auto six_tag) {
    constexpr bool SIX = decltype(six_tag)::value;
    auto hacc = [&](int r) -> int32_t {
      const uint32_t *p = wrow + r * WSD;
      int32_t acc = dot2_seed(p[0], u[0], hbias);
#pragma unroll
      for (int j = 1; j < (SIX ? 4 : 5); j++)
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, p[j]), __builtin_bit_cast(v2s_t, u[j]), acc, false);
      return acc;
    };
    auto hpair = [&](int r) -> uint32_t {   // rows r, r+1 packed as i16 x 2
      if (r + 1 < H + 7) return ashr_pair(hacc(r), hacc(r + 1), hsh);
      return (uint32_t)(hacc(r) >> hsh);
    };
    uint32_t pk[5];
    pk[0] = SIX ? (uint32_t)(hacc(1) >> hsh) << 16 : hpair(0);
#pragma unroll
    for (int j = 1; j < 4; j++) pk[j] = hpair(2 * j);
#pragma unroll
    for (int j = 0; j < H / 2; j++) {
      if (!SIX || j + 1 < H / 2) pk[4] = hpair(2 * j + 8);
      int32_t a0 = PREP ? dot2_seed64(pk[0], ty[0]) : dot2_seed0(pk[0], ty[0]);
#pragma unroll
      for (int k = 1; k < 4; k++)
        a0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, pk[k]), __builtin_bit_cast(v2s_t, ty[k]), a0, false);
      int32_t a1;
      if constexpr (SIX) {
        a1 = PREP ? dot2_seed64(pk[1], tz[1]) : dot2_seed0(pk[1], tz[1]);
#pragma unroll
        for (int k = 2; k < 4; k++)
          a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, pk[k]), __builtin_bit_cast(v2s_t, tz[k]), a1, false);
      } else {
        a1 = PREP ? dot2_seed64(pk[0], tz[0]) : dot2_seed0(pk[0], tz[0]);
#pragma unroll
        for (int k = 1; k < 5; k++)
          a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, pk[k]), __builtin_bit_cast(v2s_t, tz[k]), a1, false);
      }
      if constexpr (PREP) {
        pred[2 * j] = (a0 >> 7) - 8192;
        pred[2 * j + 1] = (a1 >> 7) - 8192;
      } else {
        a0 >>= vsh;
        a1 >>= vsh;
        pred[2 * j] = a0 < 0 ? 0 : (a0 > maxv ? maxv : a0);
        pred[2 * j + 1] = a1 < 0 ? 0 : (a1 > maxv ? maxv : a1);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) pk[k] = pk[k + 1];
    }
  };
  if (six) body(std::true_type{});
  else body(std::false_type{});
}

// One column of put_8tap (PREP: prep_8tap) of a W x H block at either pixel width, from a window staged with row
// stride WS (8-bit: pixels biased by -128); `six` is taps_six(tp), voted by every lane that makes the call.
// MXNC != 0 (8-bit only): the horizontal pass on the matrix pipe, see mc8_column_t for what win / lane / zero are then.
// MX4 (8-bit only): the same on sixteen 4x4x4 blocks; win and c are the lane's own, as without it.
template <int BPP, int W, int H, int WS, bool PREP, bool PACK4 = false, int MXNC = 0, bool MX4 = false>
__device__ __forceinline__ void mc_column_fast(const uint8_t *win, int c, const Taps<BPP> &tp, int bit_depth,
                                               int32_t *pred, bool six, int lane = 0, const uint8_t *zero = nullptr) {
  static_assert(!PACK4 || BPP == 1, "8 * mid of 16-bit pixels does not fit i16");
  static_assert((MXNC == 0 && !MX4) || BPP == 1, "there is no i16 matrix type");
  if constexpr (BPP == 1) mc8_column_t<W, H, WS, PREP, PACK4, MXNC, MX4>(win, c, tp, pred, six, lane, zero);
  else mc16_column_t<W, H, WS, PREP>(win, c, tp, bit_depth, pred, six);
}

// ---- SATD with the horizontal pass in registers (blocks with both sides >= 16, up to 10 bits) ----
// The lane stages of habs_lanes_pk cost 4.5 instructions per coefficient (DPP moves, +-1 multiplies) against 2 for
// the vertical half, only because the data sits lane = column.  Here the packed outputs of the vertical half go
// through LDS once and come back lane = (coefficient row, tile column) with the 8 columns of a tile in 8 registers:
// two butterfly stages and the folded last one (max(|a|, |b|) = max(max(a, b), -min(a, b))) are 36 packed
// instructions per 16 coefficients instead of 72.  Same i16 range argument: three vertical and two horizontal
// stages reach 32 * 1023 before the fold.
// The first two vertical stages of 16 rows of the lane's column: 8-row groups 2g and 2g + 1 side by side
__device__ __forceinline__ void satd_rows16_s2(const int32_t *v, uint32_t (&d)[8]) {
  uint32_t a[8];
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = pk_pair(v[k], v[8 + k]);
  pk_bfly8_s2(a, d);
}
// The vertical half, to column c of the candidate's tile: W dwords per row, row g * 8 + i = coefficient row i of
// that group pair.
template <int W, int H>
__device__ __forceinline__ void satd_tile_store(const int32_t *v, uint32_t *tcol) {
#pragma unroll
  for (int g = 0; g < H / 16; g++) {
    uint32_t d[8];
    satd_rows16_s2(v + g * 16, d);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      tcol[(g * 8 + 2 * k) * W] = pk_add(d[k], d[k + 4]);
      tcol[(g * 8 + 2 * k + 1) * W] = pk_sub(d[k], d[k + 4]);
    }
  }
}
// Horizontal half.  A tile row of W dwords is W / 8 items of 8 dwords, so item t of the candidate is dwords
// [8 t, 8 t + 8) of its tile; lane c of the candidate's P takes items c, c + P, ... (NI of them).  Returns the lane's
// share of sum |coefficient| (every final pair counts twice: |a + b| + |a - b| = 2 max(|a|, |b|)).
template <int NI, int P>
__device__ __forceinline__ uint32_t satd_tile_rows(const uint32_t *tile, int c) {
  uint32_t acc = 0;
#pragma unroll
  for (int m = 0; m < NI; m++) {
    const uint4 *p = (const uint4 *)(tile + (c + m * P) * 8);
    const uint4 lo = p[0], hi = p[1];
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t z[8];
    pk_bfly8_s2(x, z);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t mx = pk_max(pk_max(z[k], z[k + 4]), pk_sub(0u, pk_min(z[k], z[k + 4])));
      acc = __builtin_amdgcn_udot2(__builtin_bit_cast(v2us_t, mx), __builtin_bit_cast(v2us_t, 0x00020002u), acc, false);
    }
  }
  return acc;
}

// SATD contribution of one residual column (TS rows at a time).
template <int TS, int H, int BD>
__device__ __forceinline__ uint32_t satd_column(const int32_t *v, int lane) {
  const LaneSigns sg = lane_signs<TS>(lane);
  uint32_t acc = 0;
  if constexpr (TS == 8 && BD <= 10) {
    const uint32_t m1 = (uint32_t)sg.s1 | 0x00010001u, m2 = (uint32_t)sg.s2 | 0x00010001u;
    if constexpr (H == 8) {
      // first vertical stage in i32, then (sum, difference) halves side by side
      uint32_t a[4];
#pragma unroll
      for (int k = 0; k < 4; k++) a[k] = pk_pair(v[k] + v[k + 4], v[k] - v[k + 4]);
      const uint32_t a0 = pk_add(a[0], a[1]), a1 = pk_sub(a[0], a[1]);
      const uint32_t a2 = pk_add(a[2], a[3]), a3 = pk_sub(a[2], a[3]);
      acc = habs_lanes_pk(pk_add(a0, a2), m1, m2, acc);
      acc = habs_lanes_pk(pk_add(a1, a3), m1, m2, acc);
      acc = habs_lanes_pk(pk_sub(a0, a2), m1, m2, acc);
      acc = habs_lanes_pk(pk_sub(a1, a3), m1, m2, acc);
    } else {
#pragma unroll
      for (int g = 0; g < H / 16; g++) {
        uint32_t d[8];
        satd_rows16_s2(v + g * 16, d);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          acc = habs_lanes_pk(pk_add(d[k], d[k + 4]), m1, m2, acc);
          acc = habs_lanes_pk(pk_sub(d[k], d[k + 4]), m1, m2, acc);
        }
      }
    }
    return acc;
  }
#pragma unroll
  for (int g = 0; g < H / TS; g++) {
    int32_t a[TS];
#pragma unroll
    for (int k = 0; k < TS; k++) a[k] = v[g * TS + k];
    // vertical pass on the lane's own TS rows (dist.rs:126-131).  The operations of r1dist::hadamard_1d<TS>(a, 1),
    // written out: through that call the adds reach the back end with their operands commuted, and the 12-bit and
    // TS = 4 kernels come out in another instruction order (profiles/HISTORY.md)
    if constexpr (TS == 4) {
      const int32_t a0 = a[0] + a[1], a1 = a[0] - a[1];
      const int32_t a2 = a[2] + a[3], a3 = a[2] - a[3];
      a[0] = a0 + a2; a[1] = a1 + a3; a[2] = a0 - a2; a[3] = a1 - a3;
    } else {
      int32_t b[8], d[8];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        b[2 * k] = a[2 * k] + a[2 * k + 1];
        b[2 * k + 1] = a[2 * k] - a[2 * k + 1];
      }
      d[0] = b[0] + b[2]; d[2] = b[0] - b[2];
      d[1] = b[1] + b[3]; d[3] = b[1] - b[3];
      d[4] = b[4] + b[6]; d[6] = b[4] - b[6];
      d[5] = b[5] + b[7]; d[7] = b[5] - b[7];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        a[k] = d[k] + d[k + 4];
        a[k + 4] = d[k] - d[k + 4];
      }
    }
    // horizontal pass across the TS lanes of the tile (dist.rs:132-138)
#pragma unroll
    for (int k = 0; k < TS; k++) acc += habs_lanes<TS>(a[k], sg);
  }
  return acc;
}

}  // namespace r1cand

// tx_common.hpp -- forward-transform configuration tables and the 1-D
// butterfly networks as device functions.
//
// Restates (reference file:line):
//   TxSize dims                 src/transform/mod.rs:101-167
//   VTX_TAB / HTX_TAB           src/transform/mod.rs:364-402
//   valid_av1_transform         src/transform/mod.rs:405-417
//   AV1_TXFM_TYPE_LS            src/transform/forward_shared.rs:85-109
//   FWD_TXFM_SHIFT_LS           src/transform/forward_shared.rs:22-64
//   get_flip_cfg                src/transform/forward_shared.rs:155-164
//   TxOperations for i32        src/transform/forward.rs:37-65
// The 1-D networks (fwd_tx_1d.inc) are straight-line SSA emitted by
// tools/gen_tx1d.py; they operate on a per-lane register array.
#pragma once
#include "common.hpp"

namespace r1tx {

typedef int32_t T;
#define TX1D_FN __device__ __forceinline__
// i32 with wrapping semantics (Rust release build); products of i32 are taken
// mod 2^32 exactly like `self * mul` in forward.rs:43.
#define TX_ADD(a, b) ((T)((uint32_t)(a) + (uint32_t)(b)))
#define TX_SUB(a, b) ((T)((uint32_t)(a) - (uint32_t)(b)))
#define TX_MUL(a, m, s) \
  ((T)((uint32_t)(a) * (uint32_t)(m) + (uint32_t)((1 << (s)) >> 1)) >> (s))
#define TX_RSHIFT1(a) (TX_ADD((a), (T)((a) < 0)) >> 1)
#define TX_ADD_AVG(a, b) (TX_ADD(a, b) >> 1)
#define TX_SUB_AVG(a, b) (TX_SUB(a, b) >> 1)
#include "fwd_tx_1d.inc"
#undef TX_MUL

// Second instantiation for residuals that come from pixels (fused kernel):
// every multiplier input is then < 2^18.4 in magnitude for all sizes, types
// and bit depths (tools/tx_range.py, tests/test_tx_range.py), so the
// full-rate 24-bit multiply returns the same low 32 product bits as the
// wrapping i32 multiply of forward.rs:43.
namespace m24 {
template <int M>
__device__ __forceinline__ T mul24(T a) {
  T r;
  asm("v_mul_i32_i24_e32 %0, %1, %2" : "=v"(r) : "n"(M), "v"(a));
  return r;
}
// (a * M + round) as ONE full-rate v_mad_i32_i24, spelled out: left to the
// compiler (__mul24 + add) about a third of the network's multiplies came out
// as quarter-rate v_mul_lo_u32 + v_add (the 24-bit range proof is lost in the
// instruction selector's depth-limited known-bits walk).  Multiplier in an
// SGPR, rounding constant in a VGPR (VOP3 has no literals on gfx9).
template <int M, int S>
__device__ __forceinline__ T mul_rs(T a) {
  T r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(M), "v"((1 << S) >> 1));
  return r >> S;
}
#define TX_MUL(a, m, s) (mul_rs<(m), (s)>(a))
#include "fwd_tx_1d.inc"
// The column family (fwd_tx_1d_col.inc, tools/gen_tx1d.py fold()): r1_<net>_col<K0, S> takes the residuals unshifted
// and returns round_shift(r1_<net>(c << K0), S); a value is carried as (reg, k), value = reg * 2^k, so shift[0] and
// the halvings of the first levels are never executed.  The factor of every mad is the plain network's divided by
// 2^k: the 24-bit range proof above carries over (the generator asserts it per network).
// mul_rs on a value with pending scale K: floor((X 2^K M + 2^(S-1)) / 2^S) = floor((X M + 2^(S-1-K)) / 2^(S-K))
template <int M, int S, int K>
__device__ __forceinline__ T mul_rk(T a) {
  static_assert(K >= 1 && K <= S - 1, "the rounding term stays an integer");
  T r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(M), "v"(1 << (S - 1 - K)));
  return r >> (S - K);
}
// a - (b << D) as one mad by -2^D (an inline constant)
template <int D>
__device__ __forceinline__ T shl_subr(T b, T a) {
  static_assert(D >= 1 && D <= 4, "-2^D is an inline constant");
  T r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(b), "n"(-(1 << D)), "v"(a));
  return r;
}
#define TX_MULK(a, m, s, k) (mul_rk<(m), (s), (k)>(a))
#define TX_SHL(a, d) ((T)((uint32_t)(a) << (d)))
#define TX_SHL_ADD(a, d, b) ((T)(((uint32_t)(a) << (d)) + (uint32_t)(b)))
#define TX_SHL_SUBR(b, d, a) (shl_subr<(d)>((b), (a)))
#define TX_RND(a, s) (((a) + (1 << ((s) - 1))) >> (s))
#include "fwd_tx_1d_col.inc"
}  // namespace m24
// Third instantiation, both families again: the halving toward zero as (a - (a >> 24)) >> 1.  For |a| < 2^24 the
// byte a >> 24 is the sign, 0 or -1, so the value is TX_RSHIFT1's; the compiler folds the shift into the subtract's
// operand (v_sub_u32_sdwa .. sext(BYTE_3)), two instructions and one link of the dependent chain instead of three.
// Every halving operand of a column or row network of a chain fed from pixels is bounded below 2^18.01, plain and
// column family alike (tools/tx_range.py halving_bounds(), asserted by tools/gen_tx1d.py); for the square sizes
// 8x8 .. 64x64 at 8 and 10 bits, the only ones that take the form (rdo_halve2, rdo_cand_plan.hpp), both forms are also
// run against each other on the host (tests/test_tx_halve2.py).
namespace m24h {
using m24::mul_rk;
using m24::mul_rs;
using m24::shl_subr;
#undef TX_RSHIFT1
#define TX_RSHIFT1(a) (TX_SUB((a), (a) >> 24) >> 1)
#include "fwd_tx_1d.inc"
#include "fwd_tx_1d_col.inc"
#undef TX_RSHIFT1
#define TX_RSHIFT1(a) (TX_ADD((a), (T)((a) < 0)) >> 1)
}  // namespace m24h
// Fourth instantiation, both families of the networks of 8 points and more (fwd_tx_1d_hw.inc, tools/gen_tx1d.py
// hiword_family()), on m24h's halving: a multiply's product stays at scale 2^16,
//   (a M + 2^(s-1)) >> s  ==  (a (M << (16 - s)) + 2^15) >> 16,     s <= 16 the shift the multiply executes,
// exact while |a| (M << (16 - s)) + 2^15 < 2^31 and M << (16 - s) < 2^23 (still a 24-bit operand of the mad).  The value
// is stated as P >> 16: a consumer that adds or subtracts it reads the product's high word (v_add_u32_sdwa /
// v_sub_u32_sdwa, src_sel:WORD_1 sign-extended, as m24h's halving reads BYTE_3), and the shift is executed only where
// the value feeds something else.  Every function takes B, a bound of its inputs' magnitude (column family: of the
// unshifted residual), and every multiply carries QB, the largest B at which it qualifies (the generator's, from the
// node's L1 gain; tools/tx_range.py mul_bounds()): B <= QB takes the form, anything else is mul_rs / mul_rk as in m24h.
// The bounds the fused kernels pass are rdo_mul_col_bound / rdo_mul_row_bound (rdo_cand_plan.hpp), checked against
// tx_range.py and run on the host by tests/test_tx_mul_hiword.py.
namespace m24w {
using m24::mul_rk;
using m24::mul_rs;
using m24::shl_subr;
template <int M, int S, bool HW>
__device__ __forceinline__ T mul_rsw(T a) {
  if constexpr (HW) {
    static_assert(S >= 1 && S <= 16 && M > 0 && (long long)M * (1 << (16 - S)) < (1 << 23), "a 24-bit multiplier");
    T r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(M * (1 << (16 - S))), "v"(1 << 15));
    return r >> 16;
  } else {
    return mul_rs<M, S>(a);
  }
}
template <int M, int S, int K, bool HW>
__device__ __forceinline__ T mul_rkw(T a) {
  static_assert(K >= 1 && K <= S - 1, "the rounding term stays an integer");
  if constexpr (HW) return mul_rsw<M, S - K, true>(a);
  else return mul_rk<M, S, K>(a);
}
// The halving of a product: its operand is hidden from the compiler's range analysis, which otherwise knows a value of
// 16 bits and narrows the halving to four 16-bit instructions (v_lshrrev 31, v_and_sdwa, v_ashrrev_i16_sdwa,
// v_add_u16) where the shift by 16, m24h's v_sub_u32_sdwa and the shift by 1 are three.
__device__ __forceinline__ T halve_prod(T a) {
  asm("" : "+v"(a));
  return TX_SUB(a, a >> 24) >> 1;
}
#define TX_RSHIFT1W(a) (halve_prod(a))
// ... and the column family's output (x +- y + 1) >> 1 of two products, which it otherwise narrows to v_or_b32_sdwa,
// v_xor_b32_sdwa, v_ashrrev_i16 and v_sub_u16 where the add or subtract of two high words, the add of 1 and the shift
// are three
template <int S>
__device__ __forceinline__ T rnd_sum(T a) {
  asm("" : "+v"(a));
  return (a + (1 << (S - 1))) >> S;
}
#define TX_RNDW(a, s) (rnd_sum<(s)>(a))
#define TX_MULW(a, m, s, qb) (mul_rsw<(m), (s), (B <= (qb))>(a))
#define TX_MULKW(a, m, s, k, qb) (mul_rkw<(m), (s), (k), (B <= (qb))>(a))
#undef TX_RSHIFT1
#define TX_RSHIFT1(a) (TX_SUB((a), (a) >> 24) >> 1)
#include "fwd_tx_1d_hw.inc"
#undef TX_RSHIFT1
#define TX_RSHIFT1(a) (TX_ADD((a), (T)((a) < 0)) >> 1)
#undef TX_MULW
#undef TX_MULKW
#undef TX_RSHIFT1W
#undef TX_RNDW
}  // namespace m24w
#undef TX_MULK
#undef TX_SHL
#undef TX_SHL_ADD
#undef TX_SHL_SUBR
#undef TX_RND
#undef TX_MUL
#undef TX1D_FN
// m24:: or, H2, m24h:: in front of a network call
#define R1_M24(H2, ...)                  \
  do {                                   \
    if constexpr (H2) m24h::__VA_ARGS__; \
    else m24::__VA_ARGS__;               \
  } while (0)

// 1-D transform classes: 0 DCT, 1 ADST, 2 FLIPADST, 3 IDTX, 4 WHT (VTX_TAB / HTX_TAB,
// src/transform/mod.rs:364-402).  Two bits per tx_type 0..15 in one immediate (WHT = 16 apart):
// a table in memory would be a dependent global load in the middle of a kernel.
constexpr uint32_t pack_tx_tab(const uint8_t (&t)[16]) {
  uint32_t v = 0;
  for (int i = 0; i < 16; i++) v |= (uint32_t)t[i] << (2 * i);
  return v;
}
__host__ __device__ inline int vtx_1d(int tx_type) {
  constexpr uint8_t t[16] = {0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3};
  constexpr uint32_t k = pack_tx_tab(t);
  return tx_type == 16 ? 4 : (int)((k >> (2 * tx_type)) & 3u);
}
__host__ __device__ inline int htx_1d(int tx_type) {
  constexpr uint8_t t[16] = {0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2};
  constexpr uint32_t k = pack_tx_tab(t);
  return tx_type == 16 ? 4 : (int)((k >> (2 * tx_type)) & 3u);
}
// get_flip_cfg (src/transform/forward_shared.rs:155-164) as bit masks over tx_type
__host__ __device__ inline bool ud_flip(int tx_type) {
  return ((1u << 4 | 1u << 8 | 1u << 14 | 1u << 6) >> tx_type) & 1u;
}
__host__ __device__ inline bool lr_flip(int tx_type) {
  return ((1u << 5 | 1u << 7 | 1u << 15 | 1u << 6) >> tx_type) & 1u;
}

// (the 19 transform sizes, R1_TX_SIZES(X) and kTxWLog2 / kTxHLog2: entry.hpp)
// the sizes of the headline ladder: all that experiment builds of the fused candidate kernel instantiate (slice<>)
#define R1_TX_SIZES_HEADLINE(X) X(1, 3, 3) X(2, 4, 4) X(3, 5, 5) X(4, 6, 6)

inline bool valid_av1_transform(int tx_size, int tx_type) {
  if (!r1_tx_size_ok(tx_size) || tx_type < 0 || tx_type >= 17) return false;
  const int wl = kTxWLog2[tx_size], hl = kTxHLog2[tx_size];
  const int m = wl > hl ? wl : hl;
  if (tx_type == 16) return wl == 2 && hl == 2;
  if (m == 6) return tx_type == 0;
  if (m == 5) return tx_type == 0 || tx_type == 9;
  return true;
}

struct Shift3 { int8_t s[3]; };
inline Shift3 fwd_shift(int tx_size, int tx_type, int bd) {
  static const uint8_t cls[19] = {0, 1, 1, 2, 3, 1, 1, 1, 1, 2,
                                  2, 3, 3, 1, 1, 1, 1, 2, 2};
  static const int8_t tab[4][3][3] = {{{3, 0, 0}, {2, 0, 1}, {0, 0, 3}},
                                      {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
                                      {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}},
                                      {{4, -1, -2}, {2, 0, -1}, {0, 0, 1}}};
  Shift3 r;
  if (tx_type == 16) {
    r.s[0] = 0; r.s[1] = 0; r.s[2] = 2;
  } else {
    for (int i = 0; i < 3; i++) r.s[i] = tab[cls[tx_size]][(bd - 8) / 2][i];
  }
  return r;
}

// Compile-time FWD_TXFM_SHIFT_LS (forward_shared.rs:22-64) for non-WHT types:
// the triple depends only on (tx size class, bit depth), so a kernel
// instantiated per size and bit depth gets immediate shift amounts (a shift
// by 0 disappears, the rounding constant folds).
constexpr int fwd_shift_class(int wl, int hl) {
  const int mx = wl > hl ? wl : hl, mn = wl > hl ? hl : wl;
  if (mx == 2) return 0;
  if (mx == 6 && mn >= 5) return 3;
  if ((mx == 5 && mn >= 4) || (mx == 6 && mn == 4)) return 2;
  return 1;
}
constexpr int fwd_shift_ct(int wl, int hl, int bd, int stage) {
  constexpr int8_t tab[4][3][3] = {{{3, 0, 0}, {2, 0, 1}, {0, 0, 3}},
                                   {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
                                   {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}},
                                   {{4, -1, -2}, {2, 0, -1}, {0, 0, 1}}};
  return tab[fwd_shift_class(wl, hl)][(bd - 8) / 2][stage];
}
template <int SHIFT>
__device__ __forceinline__ T shift_fwd_ct(T v) {
  if constexpr (SHIFT >= 0) return (T)((uint32_t)v << SHIFT);
  else return (v + ((1 << -SHIFT) >> 1)) >> -SHIFT;
}

// av1_round_shift_array with bit = -shift (transform/mod.rs:317-331)
__device__ __forceinline__ T shift_fwd(T v, int shift) {
  // shift > 0: left shift; shift < 0: rounding right shift by -shift
  if (shift >= 0) return (T)((uint32_t)v << shift);
  const int b = -shift;
  return (v + ((1 << b) >> 1)) >> b;
}

// Same dispatch on the 24-bit-multiply instantiation.
// H2: the networks of m24h (the two-instruction halving), for the sizes that have them (N >= 8).
template <int N, bool H2 = false>
__device__ __forceinline__ void fwd_1d_m24(T *c, int k) {
  static_assert(!H2 || N >= 8, "the 4-point networks keep the plain halving");
  if (k == 3) return;
  if constexpr (N == 4) {
    if (k == 0) m24::r1_fdct4(c);
    else if (k == 4) m24::r1_fwht4(c);
    else m24::r1_fdst_vii_4(c);
  } else if constexpr (N == 8) {
    if (k == 0) R1_M24(H2, r1_fdct8(c)); else R1_M24(H2, r1_fdst8(c));
  } else if constexpr (N == 16) {
    if (k == 0) R1_M24(H2, r1_fdct16(c)); else R1_M24(H2, r1_fdst16(c));
  } else if constexpr (N == 32) {
    R1_M24(H2, r1_fdct32(c));
  } else {
    R1_M24(H2, r1_fdct64(c));
  }
}
// ... for a class the caller knows to have a kernel (anything but the identity): every arm writes all of c, so a
// switch on a wave-uniform `k` merges its arms without a copy (k_rdo_cand, TX_VOTE).  The switch is written out a
// second time: the compiler does not carry a `k != 3` assumption through to the test above, and fwd_1d_m24 expressed
// through this function changes the code of every kernel that calls it.
template <int N, bool H2 = false>
__device__ __forceinline__ void fwd_1d_m24_kernel(T *c, int k) {
  static_assert(!H2 || N >= 8, "the 4-point networks keep the plain halving");
  if constexpr (N == 4) {
    if (k == 0) m24::r1_fdct4(c);
    else if (k == 4) m24::r1_fwht4(c);
    else m24::r1_fdst_vii_4(c);
  } else if constexpr (N == 8) {
    if (k == 0) R1_M24(H2, r1_fdct8(c)); else R1_M24(H2, r1_fdst8(c));
  } else if constexpr (N == 16) {
    if (k == 0) R1_M24(H2, r1_fdct16(c)); else R1_M24(H2, r1_fdst16(c));
  } else if constexpr (N == 32) {
    R1_M24(H2, r1_fdct32(c));
  } else {
    R1_M24(H2, r1_fdct64(c));
  }
}

// The column pass of the fused kernels in one piece: c[r] = shift_fwd_ct<SH1>(fwd_1d_m24<N>(shift_fwd_ct<SH0>(c))[r]),
// bit for bit, on the column family -- the inputs are the unshifted residuals, the outputs go to the transpose tile
// as they are.  SH0 > 0 (8 and 10 bits); the WHT (4-point, k == 4) keeps the plain network between its shifts, the
// identity is one exact shift when shift[0] covers the rounding (it does at every size).  IDENT: the per-lane form
// with the identity's arm; without it the switch is fwd_1d_m24_kernel's (wave-uniform class, every arm writes all of c).
template <int SH0, int SH1>
__device__ __forceinline__ T shift_col_ident(T v) {
  if constexpr (SH0 + SH1 >= 0) return shift_fwd_ct<SH0 + SH1>(v);
  else return shift_fwd_ct<SH1>(shift_fwd_ct<SH0>(v));
}
template <int N, int SH0, int SH1, bool IDENT, bool H2>
__device__ __forceinline__ void fwd_col_m24_sw(T *c, int k) {
  static_assert(SH0 > 0 && SH1 <= 0, "shift[0] = 0 and a left shift[1] have no member in the column family");
  static_assert(!H2 || N >= 8, "the 4-point networks keep the plain halving");
  constexpr int S = -SH1;
  if constexpr (IDENT) {
    if (k == 3) {
#pragma unroll
      for (int r = 0; r < N; r++) c[r] = shift_col_ident<SH0, SH1>(c[r]);
      return;
    }
  }
  if constexpr (N == 4) {
    if (k == 0) m24::r1_fdct4_col<SH0, S>(c);
    else if (k == 4) {
#pragma unroll
      for (int r = 0; r < N; r++) c[r] = shift_fwd_ct<SH0>(c[r]);
      m24::r1_fwht4(c);
#pragma unroll
      for (int r = 0; r < N; r++) c[r] = shift_fwd_ct<SH1>(c[r]);
    } else m24::r1_fdst_vii_4_col<SH0, S>(c);
  } else if constexpr (N == 8) {
    if (k == 0) R1_M24(H2, r1_fdct8_col<SH0, S>(c)); else R1_M24(H2, r1_fdst8_col<SH0, S>(c));
  } else if constexpr (N == 16) {
    if (k == 0) R1_M24(H2, r1_fdct16_col<SH0, S>(c)); else R1_M24(H2, r1_fdst16_col<SH0, S>(c));
  } else if constexpr (N == 32) {
    R1_M24(H2, r1_fdct32_col<SH0, S>(c));
  } else {
    R1_M24(H2, r1_fdct64_col<SH0, S>(c));
  }
}
template <int N, int SH0, int SH1, bool H2 = false>
__device__ __forceinline__ void fwd_col_m24(T *c, int k) { fwd_col_m24_sw<N, SH0, SH1, true, H2>(c, k); }
template <int N, int SH0, int SH1, bool H2 = false>
__device__ __forceinline__ void fwd_col_m24_kernel(T *c, int k) { fwd_col_m24_sw<N, SH0, SH1, false, H2>(c, k); }

// The same switches on m24w (products at scale 2^16 where the bound B of the call's inputs allows; N >= 8): the
// siblings of fwd_1d_m24<N, true>, fwd_1d_m24_kernel<N, true>, fwd_col_m24<.., true> and fwd_col_m24_kernel<.., true>.
// B: |c[i]| <= B on entry -- for the column family the unshifted residual.
#define R1_M24W_SWITCH(N, SUF, ...)                                                            \
  do {                                                                                         \
    static_assert(N >= 8, "the 4-point networks have no member in m24w");                      \
    if constexpr (N == 8) {                                                                    \
      if (k == 0) m24w::r1_fdct8##SUF<__VA_ARGS__>(c); else m24w::r1_fdst8##SUF<__VA_ARGS__>(c);   \
    } else if constexpr (N == 16) {                                                            \
      if (k == 0) m24w::r1_fdct16##SUF<__VA_ARGS__>(c); else m24w::r1_fdst16##SUF<__VA_ARGS__>(c); \
    } else if constexpr (N == 32) {                                                            \
      m24w::r1_fdct32##SUF<__VA_ARGS__>(c);                                                    \
    } else {                                                                                   \
      m24w::r1_fdct64##SUF<__VA_ARGS__>(c);                                                    \
    }                                                                                          \
  } while (0)
template <int N, int B>
__device__ __forceinline__ void fwd_1d_m24w(T *c, int k) {
  if (k == 3) return;
  R1_M24W_SWITCH(N, , B);
}
template <int N, int B>
__device__ __forceinline__ void fwd_1d_m24w_kernel(T *c, int k) {
  R1_M24W_SWITCH(N, , B);
}
template <int N, int SH0, int SH1, bool IDENT, int B>
__device__ __forceinline__ void fwd_col_m24w_sw(T *c, int k) {
  static_assert(SH0 > 0 && SH1 <= 0, "shift[0] = 0 and a left shift[1] have no member in the column family");
  if constexpr (IDENT) {
    if (k == 3) {
#pragma unroll
      for (int r = 0; r < N; r++) c[r] = shift_col_ident<SH0, SH1>(c[r]);
      return;
    }
  }
  R1_M24W_SWITCH(N, _col, SH0, -SH1, B);
}
template <int N, int SH0, int SH1, int B>
__device__ __forceinline__ void fwd_col_m24w(T *c, int k) { fwd_col_m24w_sw<N, SH0, SH1, true, B>(c, k); }
template <int N, int SH0, int SH1, int B>
__device__ __forceinline__ void fwd_col_m24w_kernel(T *c, int k) { fwd_col_m24w_sw<N, SH0, SH1, false, B>(c, k); }
#undef R1_M24W_SWITCH

// One 1-D forward transform of length N on a register array, class `k`
// (0 DCT, 1/2 ADST (flip handled by the caller), 3 identity, 4 WHT).
template <int N>
__device__ __forceinline__ void fwd_1d(T *c, int k) {
  if (k == 3) return;  // fidentity is a no-op (forward_shared.rs:1775)
  if constexpr (N == 4) {
    if (k == 0) r1_fdct4(c);
    else if (k == 4) r1_fwht4(c);
    else r1_fdst_vii_4(c);
  } else if constexpr (N == 8) {
    if (k == 0) r1_fdct8(c); else r1_fdst8(c);
  } else if constexpr (N == 16) {
    if (k == 0) r1_fdct16(c); else r1_fdst16(c);
  } else if constexpr (N == 32) {
    r1_fdct32(c);
  } else {
    r1_fdct64(c);
  }
}

}  // namespace r1tx

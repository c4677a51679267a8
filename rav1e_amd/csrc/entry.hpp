// entry.hpp -- what the host half of every unit shares, stated once: the argument checks of the entry points, the
// transform sizes, and the step from a run-time value (bytes per pixel, a flag, a size) to a template argument.
// No device code and nothing of HIP: a host compiler accepts this header alone.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/rav1e_amd.h"

// ---- the check vocabulary ----
// Each is written inside R1_REQUIRE(...), so r1_last_error names the file, the line and the check that failed.
// They stay apart on purpose: an entry point makes exactly the checks it names, and siblings differ (r1_dist_batch
// never looks at bit_depth, r1_activity_scales does).

// pixels are one byte or two
inline bool r1_px_ok(int bytes_per_px) { return bytes_per_px == 1 || bytes_per_px == 2; }
inline bool r1_px_ok(const R1Plane &p) { return r1_px_ok(p.bytes_per_px); }
// one byte per pixel exactly at 8 bits
inline bool r1_px_fits_depth(int bytes_per_px, int bit_depth) { return (bytes_per_px == 1) == (bit_depth == 8); }
inline bool r1_px_fits_depth(const R1Plane &p) { return r1_px_fits_depth(p.bytes_per_px, p.bit_depth); }
inline bool r1_depth_ok(int bit_depth) { return bit_depth == 8 || bit_depth == 10 || bit_depth == 12; }
// two or more planes of one pixel format / of one bit depth
template <class... P>
inline bool r1_same_px(const R1Plane &a, const P &...rest) {
  return ((a.bytes_per_px == rest.bytes_per_px) && ...);
}
template <class... P>
inline bool r1_same_depth(const R1Plane &a, const P &...rest) {
  return ((a.bit_depth == rest.bit_depth) && ...);
}
// chroma decimation: 4:4:4, 4:2:2 and 4:2:0 have xdec, ydec in {0, 1}
inline bool r1_dec_ok(int xdec, int ydec) { return xdec >= 0 && xdec <= 1 && ydec >= 0 && ydec <= 1; }
// kernels that address a plane with 32-bit byte offsets (24-bit multiplies for the row): the allocation stays
// below 4 GiB and both of its dimensions below 2^24
inline bool r1_offsets_fit_u32(const R1Plane &p) {
  return p.stride > 0 && p.stride < (1 << 24) && p.alloc_height > 0 && p.alloc_height < (1 << 24) &&
         (unsigned long long)p.stride * (unsigned long long)p.alloc_height * (unsigned long long)p.bytes_per_px < (1ull << 32);
}
inline bool r1_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int r1_ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) l++;
  return l;
}

// ---- the 19 transform sizes, written once: X(TxSize id, log2 width, log2 height) ----
// The tables below and every tx_size -> instantiation switch (fwd_tx.hip, inv_tx.hip, mc.hip, rdo_cand_kernel.hpp)
// expand this list.
#define R1_TX_SIZES(X)                                                     \
  X(0, 2, 2) X(1, 3, 3) X(2, 4, 4) X(3, 5, 5) X(4, 6, 6) X(5, 2, 3)        \
  X(6, 3, 2) X(7, 3, 4) X(8, 4, 3) X(9, 4, 5) X(10, 5, 4) X(11, 5, 6)      \
  X(12, 6, 5) X(13, 2, 4) X(14, 4, 2) X(15, 3, 5) X(16, 5, 3) X(17, 4, 6)  \
  X(18, 6, 4)
namespace r1tx {
#define R1_TX_WL(ID, WL, HL) WL,
#define R1_TX_HL(ID, WL, HL) HL,
static const uint8_t kTxWLog2[19] = {R1_TX_SIZES(R1_TX_WL)};
static const uint8_t kTxHLog2[19] = {R1_TX_SIZES(R1_TX_HL)};
#undef R1_TX_WL
#undef R1_TX_HL
}  // namespace r1tx
inline bool r1_tx_size_ok(int tx_size) { return tx_size >= 0 && tx_size < 19; }

// ---- run-time value -> template argument ----
// One mechanism for the whole library: f is a generic lambda that takes the value as a constant,
//   r1_by_bpp(p->bytes_per_px, [&](auto B) { hipLaunchKernelGGL((k<B.value>), ...same arguments once...); });
// and the helpers nest.  A helper calls f with exactly the constants it lists, so a kernel is instantiated only
// for those; where the instantiations of a site are not a full product the site says so with `if constexpr`.
template <int V>
using r1_int = std::integral_constant<int, V>;

// f(the first of Vs that equals v), else f(Else): a ladder `if (v == A) ...<A> else if (v == B) ...<B> else ...<Else>`
template <int Else, int... Vs, class F>
inline void r1_by_value(int v, F &&f) {
  if (!((v == Vs && (f(r1_int<Vs>{}), true)) || ...)) f(r1_int<Else>{});
}
// bytes per pixel, checked by the caller (r1_px_ok): 1, else 2
// (these two hand back what f returns, for the sites whose launcher is a function with a status)
template <class F>
inline decltype(auto) r1_by_bpp(int bytes_per_px, F &&f) {
  if (bytes_per_px == 1) return f(r1_int<1>{});
  return f(r1_int<2>{});
}
template <class F>
inline decltype(auto) r1_by_bool(bool v, F &&f) {
  if (v) return f(std::true_type{});
  return f(std::false_type{});
}

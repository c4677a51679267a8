// mc_window.hpp -- the geometry of a staged reference window (mc_common.hpp), for the units that only size one, and
// of the matrix-pipe form of its horizontal filter pass (fragment addresses and the tap band: plain integer functions).
// No device code and nothing of HIP: the fused kernel's plan (rdo_cand_plan.hpp) reads it under a host compiler.
#pragma once

namespace r1mc {

// Bytes between the rows of the window of a block (or slab) w pixels wide: its w + 7 pixels, rounded up to whole
// dwords.  A constexpr function: callable from host and device code alike.
constexpr int window_stride(int w, int bpp) { return (((w + 7) * bpp + 3) >> 2) << 2; }

// ---- the horizontal 8-tap pass of an 8-bit window as a matrix product (mc8_column_t<.., MXNC>, cand_common.hpp) ----
// v_mfma_i32_16x16x32_i8, D = A B + C: lane l supplies A[M = l % 16][K = 8 (l / 16) .. + 7] and
// B[K = 8 (l / 16) .. + 7][N = l % 16], and receives D[M = 4 (l / 16) + {0 .. 3}][N = l % 16].
// A wave holds nc = 1 or 2 windows of blocks w = 64 / nc wide, one behind the other, lane = (candidate, column).
// With M = 4 g + k (g: a group of 16 lanes = 16 columns, k: a row of a quad of window rows):
//   A[4 g + k][kk] = window byte of group g's candidate at row 4 q + k, x = (g's first column) + kk
//   B[kk][j]       = h[kk - j], the eight half-taps as a band (0 <= kk - j < 8, zero elsewhere)
//   D[4 g + k][j]  = C + sum_t h[t] win[4 q + k][first column + j + t]
// so lane 16 g + j receives the accumulators of its own column for rows 4 q .. 4 q + 3.  B is one candidate's taps
// for all sixteen M rows: with two candidates a quad is two MFMAs into one D, and in each the row groups of the
// other candidate must supply zeros.
// Byte offset, from the first window, of the 8 bytes lane l supplies as A for quad 0 (quad q: + 4 q ws).
constexpr int mx_a_offset(int l, int nc, int h, int ws) {
  const int m = l & 15, g = m >> 2, k = m & 3, gpc = 4 / nc;   // gpc: lane groups per candidate
  return (g / gpc) * (h + 7) * ws + k * ws + 16 * (g % gpc) + 8 * (l >> 4);
}
// the candidate whose window lane l's A fragment comes from
constexpr int mx_a_cand(int l, int nc) { return ((l & 15) >> 2) / (4 / nc); }
// quads that cover the window's h + 7 rows (the last one may reach up to three rows past it: read, never consumed)
constexpr int mx_quads(int h) { return (h + 7 + 3) / 4; }
// one past the furthest byte any A fragment reads
constexpr int mx_a_end(int nc, int h, int ws) {
  return mx_a_offset(63, nc, h, ws) + (mx_quads(h) - 1) * 4 * ws + 8;
}
// bytes of zeros the other candidate's row groups read through the same quad offsets (nc == 2)
constexpr int mx_zero_bytes(int h, int ws) { return (((mx_quads(h) - 1) * 4 * ws + 8) + 15) & ~15; }
// The 8 bytes lane l supplies as B, from the candidate's half-taps as two little-endian dwords (kTapI8): byte b is
// h[8 (l / 16) + b - l % 16].
constexpr unsigned long long mx_band8(unsigned fx0, unsigned fx1, int l) {
  const unsigned long long t = ((unsigned long long)fx1 << 32) | fx0;
  const int d = (l & 15) - 8 * (l >> 4);
  return d >= 8 || d <= -8 ? 0ull : (d >= 0 ? t << (8 * d) : t >> (8 * -d));
}

}  // namespace r1mc

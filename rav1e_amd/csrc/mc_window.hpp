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

// ---- the same pass as sixteen small products (mc8_column_t<.., MX4>): windows narrower than 32 ----
// v_mfma_i32_4x4x4_16b_i8, D = A B + C, is sixteen independent 4x4x4 blocks; block b is lanes 4 b .. 4 b + 3.  Lane
// 4 b + i supplies A[i][K = 0 .. 3] as the four bytes of a dword, lane 4 b + j supplies B[K = 0 .. 3][j] and receives
// D[i = 0 .. 3][j] in registers 0 .. 3.  Every block has an A and a B of its own, so the candidates of a wave need not
// share their taps.  Lane = (candidate, column c) and w a multiple of 4: a block is four adjacent columns cb = c & ~3
// .. cb + 3 of ONE candidate, i = j = c & 3.  A quad q of window rows is three chained products, s = 0, 1, 2:
//   A_s[i][K] = byte cb + 4 s + K of row 4 q + i of the lane's OWN window: one aligned dword of row 4 q + (c & 3)
//   B_s[K][j] = h[4 s + K - j]: dword s of the eight half-taps shifted up by c & 3 bytes into twelve (zero elsewhere)
//   D[i][j]   = C + sum_s sum_K A_s[i][K] B_s[K][j] = C + sum_t h[t] win[4 q + i][cb + j + t]
// so the lane receives the accumulators of its own column for rows 4 q .. 4 q + 3 and nothing moves between lanes.
// the window row whose dwords the lane of column c supplies as A for quad q
constexpr int mx4_a_row(int c, int q) { return 4 * q + (c & 3); }
// byte offset, from the lane's own window, of the dword it supplies as A_s for quad q
constexpr int mx4_a_offset(int c, int q, int s, int ws) { return mx4_a_row(c, q) * ws + (c & ~3) + 4 * s; }
// one past the furthest byte any A fragment of a wave of nc windows reads, from the first window: the last lane's last
// dword of the last quad (whose rows past h + 6 are read and never consumed)
constexpr int mx4_a_end(int nc, int w, int h, int ws) {
  return (nc - 1) * (h + 7) * ws + mx4_a_offset(w - 1, mx_quads(h) - 1, 2, ws) + 4;
}
// The dword the lane of column c supplies as B_s, from the candidate's half-taps as two little-endian dwords (kTapI8):
// byte K is h[4 s + K - (c & 3)].
constexpr unsigned mx4_band(unsigned fx0, unsigned fx1, int c, int s) {
  const int sh8 = 8 * (c & 3);
  const unsigned long long t64 = (((unsigned long long)fx1 << 32) | fx0) << sh8;
  return s == 0 ? (unsigned)t64 : (s == 1 ? (unsigned)(t64 >> 32) : (unsigned)(((unsigned long long)fx1 << sh8) >> 32));
}

}  // namespace r1mc

// intra_pred_common.hpp -- the arithmetic of dispatch_predict_intra (src/predict.rs:705-784 and the kernels it
// selects, 786-1505) as device functions, called by k_intra_predict (predict.hip) and by the intra prediction source
// of the fused candidate kernel (rdo_cand_kernel.hpp, PS == 1).
// edge_filter_upsample'S ARITHMETIC STILL EXISTS A SECOND TIME in one place: k_intra_predict's 8-bit 16x16 pre-screen
// instantiation keeps an inline copy of it (INLINE_FORM in predict.hip), because with both functions from here its
// launch was 0.4 .. 0.7 % slower and the cause was not found.  A change to the edge filter here must be made there
// too; until that copy goes, test_intra_prescreen_vs_oracle (tests/test_gpu_parity.py) and tests/test_gpu_intra_partial_wave.py are
// what hold it against the oracle.
//
// Two parts.  edge_filter_upsample is COOPERATIVE: the `lanes` lanes of a candidate build the filtered /
// upsampled edges of a directional mode in LDS (ping-pong, every tap reads the unfiltered copy exactly like
// filter_edge's scratch array); it holds the barriers and every lane of the workgroup must reach it.
// predict_column is per lane: column `c` of the block, rows 0 .. H-1 through `put(row, value)`.  It does not care
// how many lanes a candidate has.
//
// Edge addressing: a candidate's raw edge is a base `e` and the index `tli` of its top-left entry (index
// 2 * MAX_TX_SIZE of the reference's IntraEdgeBuffer): e[tli - 1 - r] = the left pixel beside row r,
// e[tli + 1 + i] = above[i], and every access is written e[tli + ...].  The base is separate from the top-left entry
// because the offset field of an LDS read is unsigned: with a constant tli at or above the window's reach the left
// edge's indices are non-negative constants that fold into the instruction, where a negative index off a pointer to
// the top-left entry takes an address register of its own, one per read of an unrolled row loop.  So a caller
// whose window starts below the top-left entry passes its window's start (k_intra_predict: all 257 entries,
// tli = 2 * MAXTX); one that holds a pointer to the top-left entry passes it with tli = 0 (the fused kernel, which
// keeps only the 2 (W + H) + 1 entries around it that a W x H block can reach).
//
// The candidate record `cd` is R1IntraCand or const R1IntraCand &, and every caller has to say which (`Cand` is not
// deduced: a call without it does not compile).  The choice is visible in the code: by value the fields are unpacked
// once and compared as 32-bit integers, by reference every compare extracts its field (16-bit SDWA compares, a v_mov
// per constant).  k_intra_predict's 16x16 pre-screen launch is 1.3 % faster by value; the fused kernel's
// instantiations were tuned by reference and stay so.
#pragma once
#include "common.hpp"

namespace r1ip {

template <typename T>
struct as_stated { using type = T; };   // a parameter of this type takes no part in template argument deduction

#define R1_TABLE_QUAL static __constant__
#include "intra_tables.inc"
#undef R1_TABLE_QUAL

enum { DC_PRED = 0, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED,
       D203_PRED, D67_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED,
       UV_CFL_PRED };
constexpr int MAXTX = 64;
constexpr int EDGE_LEN = 4 * MAXTX + 1;

__device__ __forceinline__ int mode_angle(int mode) {
  constexpr int16_t a[9] = {0, 90, 180, 45, 135, 113, 157, 203, 67};
  return mode >= 0 && mode < 9 ? a[mode] : 0;
}
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// select_ief_strength / select_ief_upsample (predict.rs:1133-1201)
__device__ __forceinline__ int ief_strength(int wh, bool smooth, int delta) {
  const int d = iabs(delta);
  if (smooth) {
    if (wh <= 8) return d >= 64 ? 2 : (d >= 40 ? 1 : 0);
    if (wh <= 16) return d >= 48 ? 2 : (d >= 20 ? 1 : 0);
    if (wh <= 24) return d >= 4 ? 3 : 0;
    return 3;
  }
  if (wh <= 8) return d >= 56 ? 1 : 0;
  if (wh <= 16) return d >= 40 ? 1 : 0;
  if (wh <= 24) return d >= 32 ? 3 : (d >= 16 ? 2 : (d >= 8 ? 1 : 0));
  if (wh <= 32) return d >= 32 ? 3 : (d >= 4 ? 2 : 1);
  return 3;
}
__device__ __forceinline__ bool ief_upsample(int wh, bool smooth, int delta) {
  const int d = iabs(delta);
  if (d == 0 || d >= 40) return false;
  return smooth ? wh <= 8 : wh <= 16;
}

// filter_edge (predict.rs:1203-1233): dst[i] for 1 <= i < size from src
__device__ __forceinline__ int32_t filt5(const uint16_t *src, int i, int size, int strength) {
  constexpr uint8_t K[3][5] = {{0, 4, 8, 4, 0}, {0, 5, 6, 5, 0}, {2, 4, 4, 4, 2}};
  int32_t s = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    int k = i + j - 2;
    k = k < 0 ? 0 : (k > size - 1 ? size - 1 : k);
    s += K[strength - 1][j] * (int32_t)src[k];
  }
  return (s + 8) >> 4;
}

// a directional mode that is not the plain V / H copy
__device__ __forceinline__ bool is_directional(int mode, int angle) {
  return mode >= V_PRED && mode <= D67_PRED && !(mode == V_PRED && angle == 90) && !(mode == H_PRED && angle == 180);
}

// ---- get_intra_edges (src/partition.rs:639-898) as a rule over a pixel accessor, shared by k_intra_edges
// (predict.hip: the accessor reads the reconstructed plane) and the transform-split kernel (rdo_intra_split.hip: it
// answers from the block's working reconstruction in LDS inside the block and from the plane outside).  Every entry of
// the reference's IntraEdgeBuffer has a closed-form source -- a pixel of the tile, a replicated pixel or a frame-edge
// base value -- so the entries are produced independently.  (x, y): the transform block relative to the tile;
// rect_w / rect_h: the tile clipped to the plane; mode < 0 = None (every edge is needed); flags as R1IntraEdgeCand's.
struct EdgeRule {
  int x, y, txw, txh, tw, th, tr_avail, bl_avail, init_left, init_above;
  int32_t base;
  bool needs_left, needs_topleft, needs_top, tl_filter;

  __device__ __forceinline__ EdgeRule(int x_, int y_, int mode, int angle_delta, int flags, int rect_w, int rect_h,
                                      int txw_, int txh_, int bd)
      : x(x_), y(y_), txw(txw_), txh(txh_) {
    base = 128 << (bd - 8);
    bool needs_topright = true, needs_bottomleft = true;
    needs_left = needs_topleft = needs_top = true;
    tl_filter = false;
    if (mode >= 0) {
      if (mode == PAETH_PRED)
        mode = (x == 0 && y == 0) ? DC_PRED : (x == 0 ? V_PRED : (y == 0 ? H_PRED : PAETH_PRED));
      const bool directional = mode >= V_PRED && mode <= D67_PRED;
      const int p_angle = mode_angle(mode) + angle_delta * 3;
      const bool dc_or_cfl = mode == DC_PRED || mode == UV_CFL_PRED;
      needs_left = (!dc_or_cfl || x != 0) || (p_angle > 90 && p_angle != 180);
      needs_topleft = mode == PAETH_PRED || (directional && p_angle != 90 && p_angle != 180);
      needs_top = (!dc_or_cfl || y != 0) || (p_angle != 90 && p_angle < 180);
      needs_topright = directional && p_angle < 90;
      needs_bottomleft = directional && p_angle > 180;
      tl_filter = (flags & 1) && p_angle > 90 && p_angle < 180;
    }
    th = y + txh > rect_h ? rect_h - y : txh;     // visible rows / cols of the block
    tw = x + txw > rect_w ? rect_w - x : txw;
    tr_avail = bl_avail = 0;
    if (needs_topright && y != 0 && (flags & 2)) {
      tr_avail = rect_w - x - txw;
      tr_avail = tr_avail > txw ? txw : (tr_avail < 0 ? 0 : tr_avail);
    }
    if (needs_bottomleft && x != 0 && (flags & 4)) {
      bl_avail = rect_h - y - txh;
      bl_avail = bl_avail > txh ? txh : (bl_avail < 0 ? 0 : bl_avail);
    }
    init_left = (needs_left ? txh : 0) + (needs_bottomleft ? txw : 0);
    init_above = (needs_top ? txw : 0) + (needs_topright ? txh : 0);
  }
  // left[i], i = distance below the block's top row (index 127 - i); px(yy, xx) = the tile's pixel
  template <typename Px>
  __device__ __forceinline__ int32_t left_at(int i, Px px) const {
    if (i < txh) {
      if (x != 0) return px(y + (i < th ? i : th - 1), x - 1);
      return y != 0 ? px(y - 1, 0) : base + 1;
    }
    const int k = i - txh;                                // bottom-left part
    if (k < bl_avail) return px(y + txh + k, x - 1);
    // replicate left[2*MAX - txh - num_avail] = the entry just above
    const int j = txh + bl_avail - 1;
    if (j >= txh) return px(y + txh + bl_avail - 1, x - 1);
    if (x != 0) return px(y + (j < th ? j : th - 1), x - 1);
    return y != 0 ? px(y - 1, 0) : base + 1;
  }
  template <typename Px>
  __device__ __forceinline__ int32_t above_at(int i, Px px) const {
    if (i < txw) {
      if (y != 0) return px(y - 1, x + (i < tw ? i : tw - 1));
      return x != 0 ? px(0, x - 1) : base - 1;
    }
    const int k = i - txw;                                // top-right part
    if (k < tr_avail) return px(y - 1, x + txw + k);
    const int j = txw + tr_avail - 1;
    if (j >= txw) return px(y - 1, x + txw + tr_avail - 1);
    if (y != 0) return px(y - 1, x + (j < tw ? j : tw - 1));
    return x != 0 ? px(0, x - 1) : base - 1;
  }
  // entry k of the IntraEdgeBuffer, 2 * MAXTX - init_left <= k < 2 * MAXTX + 1 + init_above: only that range is
  // initialised, in the reference as well
  template <typename Px>
  __device__ __forceinline__ int32_t entry(int k, Px px) const {
    int32_t v = 0;
    if (k < 2 * MAXTX) {
      const int i = 2 * MAXTX - 1 - k;
      // bottom-left entries exist only behind a needed left column; the
      // reference never builds one without the other
      if (i < init_left && needs_left) v = left_at(i, px);
    } else if (k == 2 * MAXTX) {
      if (needs_topleft) {
        v = (x == 0 && y == 0) ? base
            : (y == 0 ? px(0, x - 1) : (x == 0 ? px(y - 1, 0) : px(y - 1, x - 1)));
        if (tl_filter && txw + txh >= 24)
          v = (int32_t)(((uint32_t)left_at(0, px) * 5 + (uint32_t)v * 6 + (uint32_t)above_at(0, px) * 5 + 8) >> 4);
      } else {
        v = base;
      }
    } else {
      const int i = k - 2 * MAXTX - 1;
      if (i < init_above && needs_top) v = above_at(i, px);
    }
    return v;
  }
};

// ---- edge filter / upsample in LDS (wave-uniform barriers, per-lane predicates).  `work` = the candidate's four
// arrays of FL = 2 (W + H) + 1 entries: af0 af1 lf0 lf1; the final edges are af0 / lf0.  Lane c of the candidate's
// `lanes` walks the entries c, c + lanes, ...  `enable` = this lane's candidate is directional with an edge filter.
template <typename Cand>
__device__ __forceinline__ void edge_filter_upsample(const uint16_t *e, int tli, uint16_t *work, int W, int H, int lanes,
                                                     int c, typename as_stated<Cand>::type cd, bool enable,
                                                     int left_len, int above_len, int32_t smax, int &up_a, int &up_l) {
  const int FL = 2 * (W + H) + 1;
  const int angle = cd.angle;
  const uint16_t *above = e + tli + 1;
  const int32_t top_left = e[tli];
  uint16_t *af0 = work, *af1 = work + FL, *lf0 = work + 2 * FL, *lf1 = work + 3 * FL;
  const int lb_len = left_len < W + H ? left_len : W + H;
  if (__any(enable)) {
    const bool smooth = cd.ief == 2;
    const int wh = W + H;
    if (enable) {
      const int al = above_len < FL - 1 ? above_len : FL - 1;
      const int ll = lb_len < FL - 1 ? lb_len : FL - 1;
      for (int k = c; k < FL; k += lanes) {
        af0[k] = k == 0 ? 0 : (k - 1 < al ? above[k - 1] : 0);
        // left_filtered[i] = left[left.len() - i]: i-th pixel downwards from the top
        lf0[k] = k == 0 ? 0 : (k <= ll ? e[tli - k] : 0);
      }
    }
    __syncthreads();
    int npa = 0, npl = 0, sa = 0, sl = 0;
    if (enable && angle != 90 && angle != 180) {
      if (c == 0) { af0[0] = (uint16_t)top_left; lf0[0] = (uint16_t)top_left; }
      npa = (W < cd.avail_w ? W : cd.avail_w) + (angle < 90 ? H : 0) + 1;
      npl = (H < cd.avail_h ? H : cd.avail_h) + (angle > 180 ? W : 0) + 1;
      sa = ief_strength(wh, smooth, angle - 90);
      sl = ief_strength(wh, smooth, angle - 180);
    }
    __syncthreads();
    if (enable)
      for (int k = c; k < FL; k += lanes) {
        af1[k] = (sa && k >= 1 && k < npa) ? (uint16_t)filt5(af0, k, npa, sa) : af0[k];
        lf1[k] = (sl && k >= 1 && k < npl) ? (uint16_t)filt5(lf0, k, npl, sl) : lf0[k];
      }
    __syncthreads();
    // upsample_edge (predict.rs:1235-1266): af1/lf1 (filtered) -> af0/lf0 (final)
    if (enable) {
      up_a = ief_upsample(wh, smooth, angle - 90);
      up_l = ief_upsample(wh, smooth, angle - 180);
      const int na = W + (angle < 90 ? H : 0), nl = H + (angle > 180 ? W : 0);
      auto ups = [&](const uint16_t *s, uint16_t *d, int size) {
        auto dup = [&](int i) -> int32_t {
          return i == 0 ? s[0] : (i <= size + 1 ? s[i - 1] : s[size]);
        };
        for (int k = c; k < FL; k += lanes)     // entries outside [1, 2*size] keep s
          if (k == 0 || k > 2 * size) d[k] = s[k];
        for (int i = c; i < size; i += lanes) {
          int32_t v = -dup(i) + 9 * dup(i + 1) + 9 * dup(i + 2) - dup(i + 3);
          v = (v + 8) / 16;
          v = v < 0 ? 0 : (v > smax ? smax : v);
          d[2 * i + 1] = (uint16_t)v;
          d[2 * i + 2] = (uint16_t)dup(i + 2);
        }
      };
      if (up_a) ups(af1, af0, na);
      else for (int k = c; k < FL; k += lanes) af0[k] = af1[k];
      if (up_l) ups(lf1, lf0, nl);
      else for (int k = c; k < FL; k += lanes) lf0[k] = lf1[k];
    }
    __syncthreads();
  }
}

// ---- one column of the prediction: put(row, value) for rows 0 .. H-1 of column c.  `directional` / `enable` as
// above; work / up_a / up_l as edge_filter_upsample left them.  acb: the candidate's AC block (UV_CFL_PRED), else
// unused.
template <typename Cand, typename Put>
__device__ __forceinline__ void predict_column(int W, int H, int c, typename as_stated<Cand>::type cd, bool directional,
                                               bool enable, int up_a, int up_l, const uint16_t *e, int tli,
                                               const uint16_t *work,
                                               int left_len, int bit_depth, const int16_t *acb, Put put) {
  const int FL = 2 * (W + H) + 1;
  const int mode = cd.mode, variant = cd.variant, angle = cd.angle;
  const int32_t smax = (1 << bit_depth) - 1;
  const uint16_t *above = e + tli + 1;
  const int32_t top_left = e[tli];
  // left pixel beside row r (left_slice[height-1-r])
  auto left_row = [&](int r) -> int32_t { return e[tli - 1 - r]; };
  const uint16_t *af0 = work, *lf0 = work + 2 * FL;
  const uint16_t *aedge = enable ? af0 : above;   // !enable: raw above, index 0 = above[0]
  const int lb_len = left_len < W + H ? left_len : W + H;
  // left_edge[k] of the reference (after left_filtered.reverse()) = lf0[FL-1-k];
  // raw case: left_and_left_below_slice[k] = raw[128 - lb_len + k]
  const int l = enable ? FL - 1 : lb_len - 1;
  auto ledge = [&](int k) -> int32_t {
    return enable ? (int32_t)lf0[FL - 1 - k] : (int32_t)e[tli - lb_len + k];
  };

  if (directional) {
    int dx = 0, dy = 0;
    if (angle < 90) dx = kR1DrIntraDerivative[angle];
    else if (angle > 90 && angle < 180) dx = kR1DrIntraDerivative[180 - angle];
    if (angle > 90 && angle < 180) dy = kR1DrIntraDerivative[angle - 90];
    else if (angle > 180) dy = kR1DrIntraDerivative[270 - angle];
    const int oa = (enable ? 1 : 0) << up_a, ol = (enable ? 1 : 0) << up_l;
    const int j = c;
#pragma unroll
    for (int i = 0; i < H; i++) {
      int32_t v;
      if (angle < 90) {
        const int idx = (i + 1) * dx;
        const int base = (idx >> (6 - up_a)) + (j << up_a);
        const int shift = ((idx << up_a) >> 1) & 31;
        const int mb = (H + W - 1) << up_a;
        if (base < mb)
          v = ((int32_t)aedge[base + oa] * (32 - shift) + (int32_t)aedge[base + 1 + oa] * shift + 16) >> 5;
        else
          v = aedge[mb + oa];
      } else if (angle < 180) {
        int idx = (j << 6) - (i + 1) * dx;
        int base = idx >> (6 - up_a);
        if (base >= -(1 << up_a)) {
          const int shift = ((idx << up_a) >> 1) & 31;
          const int32_t a = (!enable && base < 0) ? top_left : (int32_t)aedge[base + oa];
          const int32_t b = aedge[base + 1 + oa];
          v = (a * (32 - shift) + b * shift + 16) >> 5;
        } else {
          idx = (i << 6) - (j + 1) * dy;
          base = idx >> (6 - up_l);
          const int shift = ((idx << up_l) >> 1) & 31;
          int32_t a, b;
          if (!enable && base < 0) a = top_left;
          else if (base + ol == -2) a = ledge(0);
          else a = ledge(l - (base + ol));
          if (base + ol == -2) b = ledge(1);
          else b = ledge(l - (base + ol + 1));
          v = (a * (32 - shift) + b * shift + 16) >> 5;
        }
      } else {
        const int idx = (j + 1) * dy;
        const int base = (idx >> (6 - up_l)) + (i << up_l);
        const int shift = ((idx << up_l) >> 1) & 31;
        int ia = l - (base + ol), ib = l - (base + ol + 1);
        ia = ia < 0 ? 0 : ia;
        ib = ib < 0 ? 0 : ib;
        v = (ledge(ia) * (32 - shift) + ledge(ib) * shift + 16) >> 5;
      }
      put(i, v < 0 ? 0 : (v > smax ? smax : v));
    }
    return;
  }
  // ---- non-directional ----
  const int ls_len = left_len < H ? left_len : H;
  if (mode == V_PRED) {
    const int32_t a = above[c];
#pragma unroll
    for (int r = 0; r < H; r++) put(r, a);
  } else if (mode == H_PRED) {
#pragma unroll
    for (int r = 0; r < H; r++) put(r, left_row(r));
  } else if (mode == PAETH_PRED) {
    const int32_t rt = above[c];
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int32_t rl = left_row(r);
      const int32_t base = rt + rl - top_left;
      const int32_t pl = iabs(base - rl), pt = iabs(base - rt), ptl = iabs(base - top_left);
      put(r, (pl <= pt && pl <= ptl) ? rl : (pt <= ptl ? rt : top_left));
    }
  } else if (mode == SMOOTH_PRED || mode == SMOOTH_V_PRED || mode == SMOOTH_H_PRED) {
    const uint32_t below_pred = e[tli - ls_len], right_pred = above[W - 1];
    const uint32_t a = above[c], wc = kR1SmWeights[W + c];
#pragma unroll
    for (int r = 0; r < H; r++) {
      const uint32_t lft = (uint32_t)left_row(r), wr = kR1SmWeights[H + r];
      uint32_t p;
      if (mode == SMOOTH_PRED)
        p = (wr * a + (256 - wr) * below_pred + wc * lft + (256 - wc) * right_pred + 256) >> 9;
      else if (mode == SMOOTH_H_PRED)
        p = (wc * lft + (256 - wc) * right_pred + 128) >> 8;
      else
        p = (wr * a + (256 - wr) * below_pred + 128) >> 8;
      put(r, (int32_t)p);
    }
  } else {   // DC_PRED / UV_CFL_PRED
    uint32_t avg;
    if (variant == 0) {
      avg = 128u << (bit_depth - 8);
    } else if (variant == 1) {
      uint32_t s = 0;
      for (int i = 0; i < ls_len; i++) s += e[tli - ls_len + i];
      avg = (s + (uint32_t)(H >> 1)) / (uint32_t)H;
    } else if (variant == 2) {
      uint32_t s = 0;
      for (int i = 0; i < W; i++) s += above[i];
      avg = (s + (uint32_t)(W >> 1)) / (uint32_t)W;
    } else {
      uint32_t s = 0;
      for (int i = 0; i < H; i++) s += e[tli - ls_len + i];
      for (int i = 0; i < W; i++) s += above[i];
      avg = (s + (uint32_t)((W + H) >> 1)) / (uint32_t)(W + H);
    }
    if (mode == UV_CFL_PRED && angle != 0) {
#pragma unroll
      for (int r = 0; r < H; r++) {
        const int32_t q6 = (int32_t)(int16_t)angle * (int32_t)acb[r * W + c];
        const int32_t q0 = (iabs(q6) + 32) >> 6;
        const int32_t v = (int32_t)avg + (q6 < 0 ? -q0 : q0);
        put(r, v < 0 ? 0 : (v > smax ? smax : v));
      }
    } else {
#pragma unroll
      for (int r = 0; r < H; r++) put(r, (int32_t)avg);
    }
  }
}

}  // namespace r1ip

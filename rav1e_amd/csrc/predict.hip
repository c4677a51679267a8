// predict.hip -- batched intra prediction and intra-edge gathering
// (reference: rust::dispatch_predict_intra src/predict.rs:705-784 and the
// kernels it selects, 786-1505; get_intra_edges src/partition.rs:639-898;
// x86 dispatch src/asm/x86/predict.rs).
//
// k_intra_edges: eight lanes per candidate.  Every entry of the reference's
// IntraEdgeBuffer (left right-aligned ending at index 128, bottom->top;
// top-left at 128; above from 129) has a closed-form source -- a pixel of the
// reconstructed tile, a replicated pixel or a frame-edge base value -- so the
// 257 entries are produced independently by the lanes (no serial fill).  The rule itself
// is r1ip::EdgeRule (intra_pred_common.hpp), shared with the transform-split kernel.
// The partition-tree availability answers (has_top_right / has_bottom_left)
// are encoder state and arrive as flags.
//
// k_intra_predict: lane = (candidate, column), NC = 64 / W candidates per
// wave; the candidate's raw edge is staged in LDS.  Directional modes with the
// intra edge filter build the filtered / upsampled edges in LDS (ping-pong,
// all taps read the unfiltered copy exactly like filter_edge's scratch
// array), then every lane walks its column with the reference's index
// arithmetic.  Rows are stored as W consecutive pixels per candidate
// (coalesced).
// The predictors themselves (edge filter / upsampler, the directional walks, DC, V, H, Paeth, the smooths, CFL) are
// stated once, in intra_pred_common.hpp, and shared with the fused candidate kernel (rdo_cand_kernel.hpp, PS == 1);
// this kernel owns the staging, the grouping of candidates into waves, where a column goes and the SATD tail.
// ONE instantiation, the 8-bit 16x16 pre-screen, still carries the edge filter / upsampler inline (INLINE_FORM below):
// a change to r1ip::edge_filter_upsample must be made there too.
#include "common.hpp"
#include "dist_common.hpp"
#include "intra_pred_common.hpp"

using namespace r1ip;

namespace {

template <int BPP>
__device__ __forceinline__ int32_t ldp(const void *p, size_t i) {
  if constexpr (BPP == 1) return ((const uint8_t *)p)[i];
  else return ((const uint16_t *)p)[i];
}
template <int BPP>
__device__ __forceinline__ void stp(void *p, size_t i, int32_t v) {
  if constexpr (BPP == 1) ((uint8_t *)p)[i] = (uint8_t)v;
  else ((uint16_t *)p)[i] = (uint16_t)v;
}

// ------------------------------------------------------------------ edges
template <int BPP>
__global__ __launch_bounds__(64) void k_intra_edges(
    R1Plane rec, int tile_x, int tile_y, int rect_w, int rect_h, int txw, int txh, int lpc_log2,
    const R1IntraEdgeCand *__restrict__ cands, int n, void *__restrict__ edges,
    int edge_stride, uint8_t *__restrict__ lens) {
  // lpc = lanes per candidate (a power of two; they walk the 2*(txw+txh)+1 entries in strides of lpc)
  const int lpc = 1 << lpc_log2, cpw = 64 >> lpc_log2;
  const int cand = blockIdx.x * cpw + (threadIdx.x >> lpc_log2);
  const int l = threadIdx.x & (lpc - 1);
  if (cand >= n) return;
  const R1IntraEdgeCand cd = cands[cand];
  const EdgeRule er(cd.x, cd.y, cd.mode, cd.angle_delta, cd.flags, rect_w, rect_h, txw, txh, rec.bit_depth);
  const uint8_t *t0 = px_addr<BPP>(rec, tile_x, tile_y);
  const size_t st = (size_t)rec.stride;
  auto DST = [&](int yy, int xx) -> int32_t { return ldp<BPP>(t0, (size_t)yy * st + xx); };
  const int init_left = er.init_left, init_above = er.init_above;
  void *e = (uint8_t *)edges + (size_t)cand * edge_stride * BPP;
  // only the initialised range [128 - init_left, 129 + init_above) is written;
  // the reference leaves the rest of the buffer uninitialised as well
  for (int k = 2 * MAXTX - init_left + l; k < 2 * MAXTX + 1 + init_above; k += lpc) stp<BPP>(e, k, er.entry(k, DST));
  if (l == 0) {
    lens[2 * cand] = (uint8_t)init_left;
    lens[2 * cand + 1] = (uint8_t)init_above;
  }
}

// ---------------------------------------------------------------- predict
// SATD_OUT: the intra mode pre-screen of src/rdo.rs:1434-1506 in one launch --
// `group` consecutive candidates (the modes of one block) share one edge set
// and one source position; the prediction goes to LDS and only get_satd of it
// against the source block leaves the CU.
// WLT / HLT >= 0 (the pre-screen's square sizes): block size known at compile time -- every row loop
// unrolls, and with SATD_OUT the prediction column never leaves the lane's registers (it used to go
// through LDS and back: one ds_write + one ds_read per pixel, plus the address arithmetic of loops
// with a runtime trip count).
// waves per SIMD the register allocator is asked to make room for in the fixed-size pre-screen
// instantiations: left alone it took 79 / 113 VGPRs (16x16 / 32x32); asked, 44 / 68 without a spill
// (tools/kres.py): launches 0.136 -> 0.133 and 0.126 -> 0.103 ms.  Those figures are the inline predictors'; with the
// shared ones (intra_pred_common.hpp) the same requests give 43 / 74 at 8 bits and 56 / 74 at 10, still without a
// spill, and the 8x8 kernel, asked nothing, takes 79 and runs 6 waves (profiles/HISTORY.md has the timings).
constexpr int intra_waves_hint(bool satd, int wlt) {
  return !satd ? 1 : (wlt == 4 ? 7 : (wlt == 5 ? 5 : 1));   // 8x8: a request for 6 once measured +1.7 %, so none is made
}

// EGRP (the dense form only; the two-launch route of r1_rdo_intra_cand_batch): `group` consecutive candidates share
// one edge set, lens pair and pos_xy pair, as under SATD_OUT, but every candidate's prediction goes to dst in list
// order -- and the candidate's R1RdoCand (its block position, everything else zero: what r1_rdo_txsearch_batch reads
// beside a dense prediction) goes to `satd_out`, which is that list here, four dwords per candidate.  A compile-time
// choice: the instantiations without it are the kernels they were.
template <int BPP, bool SATD_OUT, int WLT = -1, int HLT = -1, bool EGRP = false>
__global__ __launch_bounds__(64, intra_waves_hint(SATD_OUT, WLT)) void k_intra_predict(
    int wl, int hl, const R1IntraCand *__restrict__ cands, int n,
    const void *__restrict__ edges, int edge_stride, const uint8_t *__restrict__ lens,
    const int16_t *__restrict__ ac, int bit_depth, void *__restrict__ dst, R1Plane src,
    const int16_t *__restrict__ pos_xy, int group, uint32_t *__restrict__ satd_out) {
  extern __shared__ uint16_t smem[];
  constexpr bool FIXED = WLT >= 0 && HLT >= 0;
  if constexpr (FIXED) { wl = WLT; hl = HLT; }
  const int W = 1 << wl, H = 1 << hl;
  const int NC = 64 >> wl;
  constexpr bool IN_REGS = SATD_OUT && FIXED;
  // The 8-bit 16x16 pre-screen keeps the EDGE FILTER / UPSAMPLER inline (r1ip::edge_filter_upsample's arithmetic a
  // second time), as every instantiation had it before the predictors moved to intra_pred_common.hpp.  With both
  // halves from the header its launch measured 0.4 .. 0.7 % above the inline form's run-to-run band; with either
  // half inline it is inside (profiles/HISTORY.md).  Why the pair costs what neither half does was not found.  A
  // change to the edge filter in the header must be made in that block too; test_intra_prescreen_vs_oracle (tests/test_gpu_parity.py) and
  // tests/test_gpu_intra_partial_wave.py hold this instantiation against the oracle.
  constexpr bool INLINE_FORM = BPP == 1 && SATD_OUT && WLT == 4 && HLT == 4;
  int32_t pv[IN_REGS ? (1 << (HLT < 0 ? 0 : HLT)) : 1];   // IN_REGS: the lane's prediction column
  const int FL = 2 * (W + H) + 1;
  const int lane = threadIdx.x;
  const int cl = lane >> wl, c = lane & (W - 1);
  // SATD_OUT: a wave takes ONE member of the group (one mode of the pre-screen) for NC
  // consecutive blocks, so every lane runs the same predictor; with the candidates in
  // list order a 16x16 wave held four different modes and paid for all four branches.
  // LOOPED (the fixed-size pre-screen instantiations): a wave takes ALL the members of the group, one
  // after the other, for its NC blocks -- the blocks' edges are loaded once (they were loaded once per
  // mode: 13 times) and the source columns stay in registers across the modes (8 / 16 rows).
  // 8x8 only: at 16x16 / 32x32 the loop costs registers (131 / 157 VGPRs, 3 waves per SIMD) and the
  // launch gets 15-25 % slower than one wave per (blocks, member); at 8x8 it is 24 % faster
  // (gpurun_out/r04_f: 0.243 -> 0.185 ms for 129600 blocks x 13 modes)
  constexpr bool LOOPED = IN_REGS && HLT == 3;
  constexpr bool SRC_REGS = LOOPED && HLT >= 0 && HLT <= 4;
  long long cand = (long long)blockIdx.x * NC + cl;
  bool live = cand < n;
  long long ecand = cand;             // edge set / block of this candidate
  if constexpr (LOOPED) {
    ecand = (long long)blockIdx.x * NC + cl;
    live = ecand < n / group;
    cand = ecand * group;
  } else if constexpr (SATD_OUT) {
    const unsigned bg = blockIdx.x / (unsigned)group, mi = blockIdx.x - bg * (unsigned)group;
    ecand = (long long)bg * NC + cl;
    live = ecand < n / group;
    cand = ecand * group + mi;
  } else if constexpr (EGRP) {
    ecand = (long long)((unsigned)cand / (unsigned)group);   // n < 2^31
    if (live && c == 0) {
      static_assert(sizeof(R1RdoCand) == 16, "R1RdoCand is written as four dwords");
      const uint32_t ox = (uint16_t)pos_xy[2 * ecand], oy = (uint16_t)pos_xy[2 * ecand + 1];
      *(uint4 *)(satd_out + 4 * cand) = make_uint4(ox | (oy << 16), 0u, 0u, 0u);
    }
  }
  uint16_t *raw = smem + cl * EDGE_LEN;
  uint16_t *work = smem + NC * EDGE_LEN + cl * (4 * FL);   // af0 af1 lf0 lf1
  int left_len = 0, above_len = 0;
  int32_t sv[SRC_REGS ? (1 << (HLT < 0 ? 0 : HLT)) : 1];   // SRC_REGS: the lane's source column
  if constexpr (SRC_REGS) {
#pragma unroll
    for (int r = 0; r < (1 << (HLT < 0 ? 0 : HLT)); r++) sv[r] = 0;
    if (live) {
      const uint8_t *ps = px_addr<BPP>(src, pos_xy[2 * ecand] + c, pos_xy[2 * ecand + 1]);
      const size_t ss = (size_t)src.stride * BPP;
#pragma unroll
      for (int r = 0; r < (1 << (HLT < 0 ? 0 : HLT)); r++) sv[r] = ldp<BPP>(ps + (size_t)r * ss, 0);
    }
  }
  if (live) {
    left_len = lens[2 * ecand];
    above_len = lens[2 * ecand + 1];
    const void *e = (const uint8_t *)edges + (size_t)ecand * edge_stride * BPP;
    // only [128 - left_len, 129 + above_len) is defined (and ever read)
    for (int k = 2 * MAXTX - left_len + c; k < 2 * MAXTX + 1 + above_len; k += W)
      raw[k] = (uint16_t)ldp<BPP>(e, k);
  }
  __syncthreads();
  const long long cand0 = cand;
  for (int it = 0; it < (LOOPED ? group : 1); it++) {
  if constexpr (LOOPED) {
    cand = cand0 + it;
    if (it) __syncthreads();     // the previous member's readers of the work arrays are done
  }
  R1IntraCand cd = {};
  if (live) cd = cands[cand];
  void *out = SATD_OUT ? (void *)((uint8_t *)smem + ((NC * (EDGE_LEN + 4 * FL) * 2 + 15) & ~15) +
                                  (size_t)cl * W * H * BPP)
                       : (void *)((uint8_t *)dst + (size_t)cand * W * H * BPP);
  const bool directional = live && is_directional(cd.mode, cd.angle);
  const bool enable = directional && cd.ief != 0;
  // the cooperative part holds the workgroup's barriers: dead lanes go through it too (cd by value: see the header)
  int up_a = 0, up_l = 0;
  if constexpr (INLINE_FORM) {
    const int angle = cd.angle;
    const int32_t smax = (1 << bit_depth) - 1;
    const uint16_t *above = raw + 2 * MAXTX + 1;
    const int32_t top_left = raw[2 * MAXTX];
    // ---- edge filter / upsample in LDS (wave-uniform barriers, per-lane predicates)
    uint16_t *af0 = work, *af1 = work + FL, *lf0 = work + 2 * FL, *lf1 = work + 3 * FL;
    const int lb_len = left_len < W + H ? left_len : W + H;
    if (__any(enable)) {
      const bool smooth = cd.ief == 2;
      const int wh = W + H;
      if (enable) {
        const int al = above_len < FL - 1 ? above_len : FL - 1;
        const int ll = lb_len < FL - 1 ? lb_len : FL - 1;
        for (int k = c; k < FL; k += W) {
          af0[k] = k == 0 ? 0 : (k - 1 < al ? above[k - 1] : 0);
          // left_filtered[i] = left[left.len() - i]: i-th pixel downwards from the top
          lf0[k] = k == 0 ? 0 : (k <= ll ? raw[2 * MAXTX - k] : 0);
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
        for (int k = c; k < FL; k += W) {
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
          for (int k = c; k < FL; k += W)     // entries outside [1, 2*size] keep s
            if (k == 0 || k > 2 * size) d[k] = s[k];
          for (int i = c; i < size; i += W) {
            int32_t v = -dup(i) + 9 * dup(i + 1) + 9 * dup(i + 2) - dup(i + 3);
            v = (v + 8) / 16;
            v = v < 0 ? 0 : (v > smax ? smax : v);
            d[2 * i + 1] = (uint16_t)v;
            d[2 * i + 2] = (uint16_t)dup(i + 2);
          }
        };
        if (up_a) ups(af1, af0, na);
        else for (int k = c; k < FL; k += W) af0[k] = af1[k];
        if (up_l) ups(lf1, lf0, nl);
        else for (int k = c; k < FL; k += W) lf0[k] = lf1[k];
      }
      __syncthreads();
    }
  } else {
    edge_filter_upsample<R1IntraCand>(raw, 2 * MAXTX, work, W, H, W, c, cd, enable, left_len, above_len,
                                      (1 << bit_depth) - 1, up_a, up_l);
  }
  if (!live) {
    if constexpr (LOOPED) continue;
    else return;
  }
  // one predicted pixel of this lane's column: a register (IN_REGS) or row i of `out`
  predict_column<R1IntraCand>(W, H, c, cd, directional, enable, up_a, up_l, raw, 2 * MAXTX, work, left_len, bit_depth,
                              ac ? ac + cand * (W * H) : nullptr, [&](int i, int32_t v) {
                                if constexpr (IN_REGS) pv[i] = v;
                                else stp<BPP>(out, (size_t)i * W + c, v);
                              });
  if constexpr (SATD_OUT) {
    __builtin_amdgcn_wave_barrier();
    const bool small = (W < H ? W : H) == 4;
    const int ts = small ? 4 : 8, ntx = W / ts, nt = ntx * (H / ts);
    uint32_t sum = 0;
    if (!small) {
      // get_satd with 8x8 tiles, lane = column (every lane of the candidate works): the
      // lane re-reads the column it just wrote, takes the vertical Hadamard of each 8-row
      // group on registers and the horizontal one across its 8-lane tile by DPP (the
      // fused candidate kernel's scheme, rdo_cand_kernel.hpp) -- with one lane per tile a 16x16
      // block kept 4 of its 16 lanes busy for 64 pixels each.
      const int32_t s1 = -(int32_t)((lane ^ (lane >> 2)) & 1);
      const int32_t s2 = -(int32_t)(((lane >> 1) ^ (lane >> 2)) & 1);
      const int bx = pos_xy[2 * ecand], by = pos_xy[2 * ecand + 1];
      const uint8_t *ps = px_addr<BPP>(src, bx + c, by);
      const size_t ss = (size_t)src.stride * BPP;
#pragma unroll
      for (int g = 0; g < H; g += 8) {
        int32_t a[8], b[8], d[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          int32_t pp;
          if constexpr (IN_REGS) pp = pv[g + k];
          else pp = ldp<BPP>(out, (size_t)(g + k) * W + c);
          if constexpr (SRC_REGS) a[k] = sv[g + k] - pp;
          else a[k] = ldp<BPP>(ps + (size_t)(g + k) * ss, 0) - pp;
        }
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
        for (int k = 0; k < 8; k++) {
          // masks {1, 2, 7} span (Z/2)^3: a Walsh-Hadamard transform in a relabelled lane
          // order, same multiset of coefficients; the last stage is folded into the abs,
          // |p + q| + |p - q| = 2 max(|p|, |q|)
          int32_t x = k < 4 ? d[k] + d[k + 4] : d[k - 4] - d[k];
          x = __mul24(x, s1 | 1) + __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true);
          x = __mul24(x, s2 | 1) + __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true);
          const int32_t ax = iabs(x);
          const int32_t ap = __builtin_amdgcn_update_dpp(0, ax, 0x141, 0xf, 0xf, true);
          sum += (uint32_t)(ax > ap ? ax : ap);
        }
      }
    } else if (c < nt) {
      const int tx = c % ntx, ty = c / ntx;
      const int bx = pos_xy[2 * ecand], by = pos_xy[2 * ecand + 1];
      const uint8_t *po = px_addr<BPP>(src, bx + tx * ts, by + ty * ts);
      const uint8_t *pp = (const uint8_t *)out + ((size_t)ty * ts * W + (size_t)tx * ts) * BPP;
      sum = small ? r1dist::tile_dist<BPP, 4, true>(po, (size_t)src.stride * BPP, pp, (size_t)W * BPP)
                  : r1dist::tile_dist<BPP, 8, true>(po, (size_t)src.stride * BPP, pp, (size_t)W * BPP);
    }
    for (int m = 1; m < W; m <<= 1) sum += __shfl_xor(sum, m, 64);
    const int ln = small ? 2 : 3;
    if (c == 0) satd_out[cand] = (sum + ((1u << ln) >> 1)) >> ln;
  }
  }   // members of the group (LOOPED), else one pass
}

// r1_prescreen_select_batch: one thread per (group, element).  An element's place in the
// stable sort is the number of elements that precede it: smaller key, or equal key and
// smaller index -- no sorting network, the groups have at most 64 members.
__global__ __launch_bounds__(256) void k_prescreen_select(const uint32_t *__restrict__ keys,
                                                          int n_groups, int group, int head, int k,
                                                          uint8_t *__restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long g = t / group;
  const int j = (int)(t - g * group);
  if (g >= n_groups) return;
  const uint32_t *kg = keys + g * group;
  int place = j;
  if (j >= head) {
    const uint32_t kj = kg[j];
    place = head;
    for (int i = head; i < group; i++) {
      const uint32_t ki = kg[i];
      place += (ki < kj) || (ki == kj && i < j);
    }
  }
  if (place < k) out[g * k + place] = (uint8_t)j;
}

// pred_cfl_ac (predict.rs:1020-1063): one wave per candidate
template <int BPP>
__global__ __launch_bounds__(64) void k_cfl_ac(R1Plane luma, int bw, int bh, int xdec, int ydec,
                                               const R1CflAcCand *__restrict__ cands, int n,
                                               int16_t *__restrict__ ac) {
  const int cand = blockIdx.x;
  if (cand >= n) return;
  const R1CflAcCand cd = cands[cand];
  const int mlw = (bw - cd.w_pad * 4) << xdec, mlh = (bh - cd.h_pad * 4) << ydec;
  const int mx = (mlw > 8 ? mlw : 8) - (1 << xdec), my = (mlh > 8 ? mlh : 8) - (1 << ydec);
  const uint8_t *p0 = px_addr<BPP>(luma, cd.x, cd.y);
  const size_t st = (size_t)luma.stride;
  int16_t *out = ac + (size_t)cand * bw * bh;
  int32_t sum = 0;
  for (int i = threadIdx.x; i < bw * bh; i += 64) {
    const int sy = i / bw, sx = i - sy * bw;
    const int ly = sy << ydec, lx = sx << xdec;
    const int y = ly < my ? ly : my, x = lx < mx ? lx : mx;
    int32_t s = ldp<BPP>(p0, y * st + x);
    if (xdec) s += ldp<BPP>(p0, y * st + x + 1);
    if (ydec) s += ldp<BPP>(p0, (y + 1) * st + x) + ldp<BPP>(p0, (y + 1) * st + x + 1);
    s = (int16_t)(s << (3 - xdec - ydec));
    out[i] = (int16_t)s;
    sum += s;
  }
  sum = (int32_t)group_sum<64>((uint32_t)sum);
  const int shift = 31 - __clz(bw * bh);
  const int16_t avg = (int16_t)((sum + (1 << (shift - 1))) >> shift);
  __syncthreads();
  for (int i = threadIdx.x; i < bw * bh; i += 64) out[i] = (int16_t)(out[i] - avg);
}

// rdo_cfl_alpha (src/rdo.rs:1593-1688) for one chroma plane: one wave per block.
// Lane a evaluates alpha = a - 16 (-16 .. 16): pred_cfl_inner (predict.rs:1064-1091)
// of the whole block against the source, plain SSE over the visible part
// (sse_wxh with the default scale is the plain sum); lane 0 then replays the
// reference's sequential selection (alpha 0 first, +-1 .. +-16 with the early
// exit `count < alpha`) on the 33 costs.
template <int BPP>
__global__ __launch_bounds__(64) void k_cfl_alpha(R1Plane src, int wl, int hl,
                                                  const R1CflAlphaCand *__restrict__ cands, int n,
                                                  const void *__restrict__ edges, int edge_stride,
                                                  const uint8_t *__restrict__ lens,
                                                  const int16_t *__restrict__ ac, int bit_depth,
                                                  int16_t *__restrict__ alpha_out,
                                                  unsigned long long *__restrict__ cost_out) {
  __shared__ int16_t s_ac[32 * 32];
  __shared__ uint16_t s_src[32 * 32];
  __shared__ unsigned long long s_cost[33];
  const int W = 1 << wl, H = 1 << hl, lane = threadIdx.x;
  const int cand = blockIdx.x;
  const R1CflAlphaCand cd = cands[cand];
  const int vw = cd.vis_w, vh = cd.vis_h;
  // DC_PRED average of the block's edges (predict.rs:885-933), by variant
  const void *e = (const uint8_t *)edges + (size_t)cand * edge_stride * BPP;
  const int left_len = lens[2 * cand];
  const int ls_len = left_len < H ? left_len : H;
  uint32_t avg;
  if (cd.variant == 0) {
    avg = 128u << (bit_depth - 8);
  } else {
    uint32_t sum = 0;
    if (cd.variant != 2)   // LEFT or BOTH
      for (int i = 0; i < (cd.variant == 1 ? ls_len : H); i++) sum += (uint32_t)ldp<BPP>(e, 2 * MAXTX - ls_len + i);
    if (cd.variant != 1)   // TOP or BOTH
      for (int i = 0; i < W; i++) sum += (uint32_t)ldp<BPP>(e, 2 * MAXTX + 1 + i);
    const uint32_t len = cd.variant == 1 ? (uint32_t)H : (cd.variant == 2 ? (uint32_t)W : (uint32_t)(W + H));
    avg = (sum + (len >> 1)) / len;
  }
  for (int i = lane; i < W * H; i += 64) {
    s_ac[i] = ac[(size_t)cand * W * H + i];
    const int x = i & (W - 1), y = i >> wl;
    s_src[i] = (x < vw && y < vh) ? (uint16_t)ld_px<BPP>(px_addr<BPP>(src, cd.x + x, cd.y + y)) : 0;
  }
  __syncthreads();
  if (lane < 33) {
    const int alpha = lane - 16;
    const int32_t smax = (1 << bit_depth) - 1;
    unsigned long long sse = 0;
    for (int y = 0; y < vh; y++)
      for (int x = 0; x < vw; x++) {
        const int i = (y << wl) + x;
        const int32_t q6 = alpha * (int32_t)s_ac[i];
        const int32_t q0 = ((q6 < 0 ? -q6 : q6) + 32) >> 6;
        int32_t v = (int32_t)avg + (q6 < 0 ? -q0 : q0);
        v = v < 0 ? 0 : (v > smax ? smax : v);
        const int32_t d = (int32_t)s_src[i] - v;
        sse += (unsigned long long)(uint32_t)(d * d);
      }
    s_cost[lane] = sse;
  }
  __syncthreads();
  if (lane == 0) {
    unsigned long long best = s_cost[16];
    int best_a = 0, count = 2;
    for (int a = 1; a <= 16; a++) {
      const unsigned long long cp = s_cost[16 + a], cm = s_cost[16 - a];
      if (cp < best) { best = cp; best_a = a; count += 2; }
      if (cm < best) { best = cm; best_a = -a; count += 2; }
      if (count < a) break;
    }
    alpha_out[cand] = (int16_t)best_a;
    if (cost_out) cost_out[cand] = best;
  }
}

}  // namespace

extern "C" int r1_intra_edges_batch(r1_ctx *ctx, const R1Plane *rec, int tile_x, int tile_y,
                                    int tile_w, int tile_h, int tx_size,
                                    const R1IntraEdgeCand *cands, int n, void *edges,
                                    int edge_stride, uint8_t *lens, void *stream) {
  R1_REQUIRE(ctx && rec);
  R1_REQUIRE(r1_px_ok(*rec));
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(edge_stride >= EDGE_LEN);
  R1_REQUIRE(tile_x >= 0 && tile_y >= 0 && tile_w > 0 && tile_h > 0);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands && edges && lens);
  // rect_w / rect_h: dst.rect() clipped to the plane (partition.rs:701-704)
  const int rect_w = tile_w < rec->width - tile_x ? tile_w : rec->width - tile_x;
  const int rect_h = tile_h < rec->height - tile_y ? tile_h : rec->height - tile_y;
  hipStream_t st = (hipStream_t)stream;
  const int txw = 1 << r1tx::kTxWLog2[tx_size], txh = 1 << r1tx::kTxHLog2[tx_size];
  // EIGHT lanes per block, whatever its size: what a lane does before it touches an entry (the mode / flag
  // logic, the clipping, the block's address) is the same for every lane of a block and dominates; with 8
  // lanes a wave prepares 8 blocks and walks the 17 .. 129 entries in strides of 8.  Measured against one
  // lane per entry (gpurun_out/r04_g, 4K luma): 4x4 0.097 -> 0.037 ms, 8x8 0.048 -> 0.015, 16x16 0.0165 ->
  // 0.0124, 32x32 0.0121 -> 0.0119.
  const int lpc_log2 = 3;
  const int cpw = 64 >> lpc_log2;
  const unsigned grid = (unsigned)((n + cpw - 1) / cpw);
  r1_by_bpp(rec->bytes_per_px, [&](auto B) {
    hipLaunchKernelGGL((k_intra_edges<B.value>), dim3(grid), dim3(64), 0, st, *rec, tile_x, tile_y, rect_w,
                       rect_h, txw, txh, lpc_log2, cands, n, edges, edge_stride, lens);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

namespace {
template <bool EGRP>
void predict_launch(int tx_size, const R1IntraCand *cands, int n, const void *edges, int edge_stride,
                    const uint8_t *lens, int group, const int16_t *pos_xy, R1RdoCand *rdo_cands, const int16_t *ac,
                    int bit_depth, int bytes_per_px, void *dst, hipStream_t st) {
  const int wl = r1tx::kTxWLog2[tx_size], hl = r1tx::kTxHLog2[tx_size];
  const int W = 1 << wl, H = 1 << hl;
  const int NC = 64 / W, FL = 2 * (W + H) + 1;
  const size_t lds = (size_t)NC * (EDGE_LEN + 4 * FL) * sizeof(uint16_t);
  const unsigned grid = (unsigned)((n + NC - 1) / NC);
  // square blocks 4x4 .. 32x32 with the size as a constant (unrolled row loops)
  r1_by_bpp(bytes_per_px, [&](auto B) {
    r1_by_value<-1, 2, 3, 4, 5>(wl == hl ? wl : 0, [&](auto S) {
      hipLaunchKernelGGL((k_intra_predict<B.value, false, S.value, S.value, EGRP>), dim3(grid), dim3(64), lds, st,
                         wl, hl, cands, n, edges, edge_stride, lens, ac, bit_depth, dst, R1Plane{}, pos_xy, group,
                         (uint32_t *)rdo_cands);
    });
  });
}
}  // namespace

// The first launch of r1_rdo_intra_cand_batch's two-launch route, arguments checked by the caller: candidate i
// predicts from edge set i / group into dst[i], and rdo_cands[i] takes its block position pos_xy[i / group].
int r1_predict_intra_route_launch(int tx_size, const R1IntraCand *cands, int n, const void *edges, int edge_stride,
                                  const uint8_t *lens, int group, const int16_t *pos_xy, R1RdoCand *rdo_cands,
                                  const int16_t *ac, int bit_depth, int bytes_per_px, void *dst, hipStream_t st) {
  predict_launch<true>(tx_size, cands, n, edges, edge_stride, lens, group, pos_xy, rdo_cands, ac, bit_depth,
                       bytes_per_px, dst, st);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_predict_intra_batch(r1_ctx *ctx, int tx_size, const R1IntraCand *cands, int n,
                                      const void *edges, int edge_stride, const uint8_t *lens,
                                      const int16_t *ac, int bit_depth, int bytes_per_px,
                                      void *dst, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(r1_depth_ok(bit_depth));
  R1_REQUIRE(r1_px_ok(bytes_per_px));
  R1_REQUIRE(r1_px_fits_depth(bytes_per_px, bit_depth));
  R1_REQUIRE(edge_stride >= EDGE_LEN);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands && edges && lens && dst);
  predict_launch<false>(tx_size, cands, n, edges, edge_stride, lens, 1, nullptr, nullptr, ac, bit_depth, bytes_per_px,
                        dst, (hipStream_t)stream);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_intra_satd_batch(r1_ctx *ctx, const R1Plane *src, int tx_size,
                                   const R1IntraCand *cands, int n, int group,
                                   const int16_t *pos_xy, const void *edges, int edge_stride,
                                   const uint8_t *lens, const int16_t *ac, uint32_t *satd_out,
                                   void *stream) {
  R1_REQUIRE(ctx && src);
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(r1_depth_ok(src->bit_depth));
  R1_REQUIRE(r1_px_ok(*src));
  R1_REQUIRE(r1_px_fits_depth(*src));
  R1_REQUIRE(edge_stride >= EDGE_LEN && group >= 1);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(n % group == 0);
  R1_REQUIRE(cands && edges && lens && pos_xy && satd_out);
  const int wl = r1tx::kTxWLog2[tx_size], hl = r1tx::kTxHLog2[tx_size];
  const int W = 1 << wl, H = 1 << hl;
  const int NC = 64 / W, FL = 2 * (W + H) + 1;
  const size_t lds = (((size_t)NC * (EDGE_LEN + 4 * FL) * sizeof(uint16_t) + 15) & ~(size_t)15) +
                     (size_t)NC * W * H * src->bytes_per_px;
  unsigned grid = (unsigned)((n / group + NC - 1) / NC) * (unsigned)group;   // (block group, member)
  // the pre-screen's sizes (luma transform blocks 8x8 .. 32x32) with the block size as a constant; at 8x8 a
  // wave walks the members of its blocks' groups itself
  const int sq = wl == hl ? wl : 0;
  if (sq == 3) grid /= (unsigned)group;
  hipStream_t st = (hipStream_t)stream;
  r1_by_bpp(src->bytes_per_px, [&](auto B) {
    r1_by_value<-1, 3, 4, 5>(sq, [&](auto S) {
      hipLaunchKernelGGL((k_intra_predict<B.value, true, S.value, S.value>), dim3(grid), dim3(64), lds, st, wl, hl,
                         cands, n, edges, edge_stride, lens, ac, src->bit_depth, (void *)nullptr, *src, pos_xy, group,
                         satd_out);
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_prescreen_select_batch(r1_ctx *ctx, const uint32_t *keys, int n_groups, int group,
                                         int keep_head, int k, uint8_t *idx_out, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(group >= 1 && group <= 64 && k >= 1 && k <= group && keep_head >= 0 && keep_head <= k);
  if (n_groups <= 0) return R1_OK;
  R1_REQUIRE(keys && idx_out);
  const long long total = (long long)n_groups * group;
  hipLaunchKernelGGL(k_prescreen_select, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, keys, n_groups, group, keep_head, k, idx_out);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_cfl_ac_batch(r1_ctx *ctx, const R1Plane *luma, int bw, int bh, int xdec,
                               int ydec, const R1CflAcCand *cands, int n, int16_t *ac,
                               void *stream) {
  R1_REQUIRE(ctx && luma);
  R1_REQUIRE(r1_px_ok(*luma));
  // bw x bh is the chroma block whose AC is taken, so this is not r1_block_size_ok (block_geom.hpp) and is wider on
  // purpose: any two powers of two 4 .. 64, whatever their ratio.  The formats are r1_subsampling_ok's three.
  R1_REQUIRE(r1_is_pow2(bw) && r1_is_pow2(bh) && bw >= 4 && bh >= 4 && bw <= 64 && bh <= 64);
  R1_REQUIRE(r1_dec_ok(xdec, ydec) && (ydec == 0 || xdec == 1));
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands && ac);
  hipStream_t st = (hipStream_t)stream;
  r1_by_bpp(luma->bytes_per_px, [&](auto B) {
    hipLaunchKernelGGL((k_cfl_ac<B.value>), dim3(n), dim3(64), 0, st, *luma, bw, bh, xdec, ydec, cands, n, ac);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_cfl_alpha_search_batch(r1_ctx *ctx, const R1Plane *src, int tx_size,
                                         const R1CflAlphaCand *cands, int n, const void *edges,
                                         int edge_stride, const uint8_t *lens, const int16_t *ac,
                                         int16_t *alpha_out, uint64_t *cost_out, void *stream) {
  R1_REQUIRE(ctx && src);
  R1_REQUIRE(r1_tx_size_ok(tx_size));
  R1_REQUIRE(r1_px_ok(*src));
  R1_REQUIRE(r1_px_fits_depth(*src));
  R1_REQUIRE(edge_stride >= EDGE_LEN);
  const int wl = r1tx::kTxWLog2[tx_size], hl = r1tx::kTxHLog2[tx_size];
  R1_REQUIRE(wl <= 5 && hl <= 5);   // CFL: chroma transforms up to 32x32
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands && edges && lens && ac && alpha_out);
  hipStream_t st = (hipStream_t)stream;
  r1_by_bpp(src->bytes_per_px, [&](auto B) {
    hipLaunchKernelGGL((k_cfl_alpha<B.value>), dim3(n), dim3(64), 0, st, *src, wl, hl, cands, n, edges, edge_stride,
                       lens, ac, src->bit_depth, alpha_out, (unsigned long long *)cost_out);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// me_blocks.hip -- the RDO-time block search (r1_estimate_motion_batch): independent blocks of any BlockSize up to
// 64x64 at full resolution, full-pel on the search engine of me_search.hpp, sub-pel on the fused candidate
// kernel's machinery (cand_common.hpp) or the generic put_8tap (mc_common.hpp).
#include "me_search.hpp"
#include "cand_common.hpp"

namespace {

// One sub-pel candidate of a W x H block (W, H in {8, 16}) inside a 16-lane group, on the fused
// candidate kernel's machinery (rdo_cand.hip): window staged by the group with one round trip,
// lane = column, v_dot4 / v_dot2 column filter, residual against the source block (in LDS for the
// whole search), SATD by the DPP Hadamard (or SAD).  Returns this lane's share; the caller sums the
// group.  The generic path it replaces for these sizes (scalar taps from byte reads, one lane per
// 8x8 Hadamard tile = 4 of 16 lanes busy) cost about three times the instructions.
template <int BPP, int W, int H, int BD, int NL = 16>
__device__ __forceinline__ uint32_t subpel_group_dist(uint8_t *win, const R1Plane &ref, int x, int y, int cf,
                                                      int rf, int fm, int gl, int lane, const uint8_t *src /* LDS: the W x H source block, dense */,
                                                      bool satd, int bit_depth) {
  constexpr int WS = r1mc::window_stride(W, BPP);
  r1mc::stage_window_fast<BPP, BPP == 1 ? 0x80808080u : 0u, W, H, NL>(win, WS, ref, x, y, gl);
  __builtin_amdgcn_wave_barrier();
  int32_t v[H];
#pragma unroll
  for (int r = 0; r < H; r++) v[r] = 0;
  if (gl < W) {
    int32_t pred[H];
    const r1cand::Taps<BPP> tp = r1cand::load_taps<BPP, W, H>(cf, rf, fm, fm);
    r1cand::mc_column_fast<BPP, W, H, WS, false>(win, gl, tp, bit_depth, pred, r1cand::taps_six(tp));
#pragma unroll
    for (int r = 0; r < H; r++) v[r] = ld_px<BPP>(src + (r * W + gl) * BPP) - pred[r];
  }
  __builtin_amdgcn_wave_barrier();   // the window is rewritten by the next candidate of this group
  if (satd) return r1cand::satd_column<8, H, BD>(v, lane);
  uint32_t s = 0;
#pragma unroll
  for (int r = 0; r < H; r++) s += (uint32_t)iabs32(v[r]);
  return s;
}

// ---------------------------------------------------------------------------
// estimate_motion with pmv = Some(..) (the RDO-time call, src/rdo.rs:1183-1196):
// independent blocks of any BlockSize up to 64x64, full resolution.  One
// WORKGROUP of 4 waves per block:
//   * the source block sits in LDS; in the full-pel steps wave v / slot s takes
//     candidate 4-or-less * v + s of a step (rows of a candidate on max(16, h)
//     lanes), the per-wave winners meet in LDS;
//   * in the sub-pel diamond (me.rs:1311-1383) wave v owns candidate v of the
//     four: it stages the (w+7) x (h+7) reference window in LDS, runs put_8tap
//     (mc_common.hpp) into an LDS tile and takes SATD / SAD of it against the
//     source -- the prediction never exists in HBM.
template <int BPP>
struct WgBlock {
  const uint8_t *ref0;
  long sr;
  int w, h, po_x, po_y;
  int mvx_min, mvx_max, mvy_min, mvy_max;
  MvCost mc;
  int wave, lane, RH, r, slot, ncs;
  const uint8_t *org;             // LDS, row stride w * BPP
  unsigned long long *red;        // LDS, 4 x 3 words: cost, (idx, sad), (row, col)

  __device__ __forceinline__ void eval(int row, int col, bool valid, bool check,
                                       unsigned long long &cost, uint32_t &sad) const {
    bool in = valid;
    if (check) in = in && col >= mvx_min && col <= mvx_max && row >= mvy_min && row <= mvy_max;
    uint32_t part = 0;
    if (in && r < h) {
      const uint8_t *p = ref0 + (long)(div8(row) + r) * sr + (long)div8(col) * BPP;
      const uint8_t *o = org + r * w * BPP;
      for (int g = 0; g < w / 4; g++) {
        if constexpr (BPP == 1) {
          part = __builtin_amdgcn_sad_u8(*(const uint32_t *)(o + 4 * g), ld_u32(p + 4 * g), part);
        } else {
          const U32x2 v = ld_u32x2(p + 8 * g);
          part = __builtin_amdgcn_sad_u16(*(const uint32_t *)(o + 8 * g), v.a, part);
          part = __builtin_amdgcn_sad_u16(*(const uint32_t *)(o + 8 * g + 4), v.b, part);
        }
      }
    }
    for (int s = 1; s < RH; s <<= 1) part += __shfl_xor(part, s, 64);
    cost = in ? mc.cost(row, col, part) : COST_MAX;
    sad = in ? part : 0xFFFFFFFFu;
  }

  // workgroup-wide argmin of (cost, idx): every thread returns the winner
  __device__ __forceinline__ void wg_min(unsigned long long &cost, int &idx, int &row, int &col,
                                         uint32_t &sad) const {
    if (lane == 0) {
      red[3 * wave] = cost;
      red[3 * wave + 1] = ((unsigned long long)(uint32_t)idx << 32) | sad;
      red[3 * wave + 2] = ((unsigned long long)(uint32_t)row << 32) | (uint32_t)col;
    }
    __syncthreads();
    int best = 0;
    for (int v = 1; v < 4; v++) {
      const unsigned long long c = red[3 * v], cb = red[3 * best];
      if (c < cb || (c == cb && (int)(red[3 * v + 1] >> 32) < (int)(red[3 * best + 1] >> 32))) best = v;
    }
    cost = red[3 * best];
    idx = (int)(red[3 * best + 1] >> 32);
    sad = (uint32_t)red[3 * best + 1];
    row = (int)(red[3 * best + 2] >> 32);
    col = (int)(uint32_t)red[3 * best + 2];
    __syncthreads();
  }

  // the shared search code's two-list step (Block::scan_pair): here simply one list after the other
  template <class GenA, class GenB>
  __device__ __forceinline__ void scan_pair(int na, GenA gen_a, Msr &best_a, int nb, GenB gen_b, Msr &best_b,
                                            bool check) const {
    scan(na, gen_a, check, best_a, nullptr);
    scan(nb, gen_b, check, best_b, nullptr);
  }

  template <class Gen>
  __device__ __forceinline__ void scan(int n, Gen gen, bool check, Msr &best, int *best_idx) const {
    for (int base = 0; base < n; base += 4 * ncs) {
      MeCand c{0, base + wave * ncs + slot, 0, 0, 0};
      const bool valid = c.idx < n;
      if (valid) gen(c.idx, c.row, c.col);
      eval(c.row, c.col, valid, check, c.cost, c.sad);
      c.xor_min(RH, WAVE);
      wg_min(c.cost, c.idx, c.row, c.col, c.sad);
      if (c.cost < best.cost) {
        best = Msr{c.row, c.col, c.cost, c.sad};
        if (best_idx) *best_idx = c.idx;
      }
    }
  }

  // this wave: put_8tap of the block at (sx, sy) + fractions into `pred`, then
  // get_satd / get_sad against the source (compute_mv_rd's distortion)
  __device__ __forceinline__ uint32_t predict_dist(const R1Plane &ref, uint8_t *win, uint8_t *pred,
                                                   int sx, int sy, int col_frac, int row_frac,
                                                   int mode, bool use_satd) const {
    // 8-bit 32 / 64-sized blocks: the fused candidate kernel's column filter + DPP SATD, a wave per
    // candidate (64x64 0.27 -> 0.20 ms, 32x32 0.50 -> 0.42 ms for every block of a 4K frame).  The
    // 16-bit variant of the same lost at 32x32 (0.56 -> 0.70 ms: 181 VGPRs, spills, 29 k instructions
    // of code) and stays on the generic path.
    if constexpr (BPP == 1) {
      if ((w == 32 || w == 64) && (h == 32 || h == 64)) {
        uint32_t s = 0;
#define R1_WP(W_, H_) s = subpel_group_dist<1, W_, H_, 8, 64>(win, ref, sx, sy, col_frac, row_frac, mode, lane, lane, org, use_satd, 8)
        if (w == 32 && h == 32) R1_WP(32, 32);
        else if (w == 64 && h == 64) R1_WP(64, 64);
        else if (w == 64) R1_WP(64, 32);
        else R1_WP(32, 64);
#undef R1_WP
        s = group_sum<64>(s);
        return use_satd ? (s + 4u) >> 3 : s;
      }
    }
    const int ws = r1mc::window_stride(w, BPP);
    r1mc::stage_window<BPP>(win, ws, ref, sx, sy, w, h, lane, 64);
    __builtin_amdgcn_wave_barrier();
    if (lane < w) {
      if constexpr (BPP == 1)
        r1mc::mc_column<BPP, false, 0>(win, ws, lane, w, h, col_frac, row_frac, mode, mode,
                                       ref.bit_depth,
                                       [&](int rr, int32_t v) { pred[rr * w + lane] = (uint8_t)v; });
      else
        r1mc::mc_column<BPP, false, 0>(win, ws, lane, w, h, col_frac, row_frac, mode, mode,
                                       ref.bit_depth, [&](int rr, int32_t v) {
                                         ((uint16_t *)pred)[rr * w + lane] = (uint16_t)v;
                                       });
    }
    __builtin_amdgcn_wave_barrier();
    const bool small = (w < h ? w : h) == 4;
    const int ts = small ? 4 : 8, ntx = w / ts, nt = ntx * (h / ts);
    uint32_t s = 0;
    if (lane < nt) {
      const int tx = lane % ntx, ty = lane / ntx;
      const size_t off = ((size_t)ty * ts * w + (size_t)tx * ts) * BPP, st = (size_t)w * BPP;
      if (use_satd)
        s = small ? r1dist::tile_dist<BPP, 4, true>(org + off, st, pred + off, st)
                  : r1dist::tile_dist<BPP, 8, true>(org + off, st, pred + off, st);
      else
        s = small ? r1dist::tile_dist<BPP, 4, false>(org + off, st, pred + off, st)
                  : r1dist::tile_dist<BPP, 8, false>(org + off, st, pred + off, st);
    }
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    const int ln = small ? 2 : 3;
    return use_satd ? (s + ((1u << ln) >> 1)) >> ln : s;
  }
};

template <int BPP>
__global__ __launch_bounds__(256) void k_me_blocks(R1MeJob job, R1MeParams p,
                                                   const R1MeBlockCand *__restrict__ cands,
                                                   int max_w, int max_h, int use_satd,
                                                   int filter_mode,
                                                   R1MeResult *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int16_t sh_subsets[4][kSubsetWords];
  __shared__ unsigned long long sh_red[12];
  const R1MeBlockCand cd = cands[blockIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int w = cd.w, h = cd.h;
  if (w > max_w || h > max_h || w < 4 || h < 4 || (w & (w - 1)) || (h & (h - 1))) {
    // not a block this launch was sized for: an empty MotionSearchResult
    if (threadIdx.x == 0) out[blockIdx.x] = R1MeResult{0, 0, 0xFFFFFFFFu, COST_MAX};
    return;
  }
  TileView t{job.stats, job.prev, p.stats_cols, p.stats_rows, job.tile_x / MI, job.tile_y / MI,
             job.tile_w / MI, job.tile_h / MI};
  // LDS: source block | 4 x (window | prediction)
  const int ws = r1mc::window_stride(w, BPP);
  const int org_bytes = (w * h * BPP + 15) & ~15, win_bytes = ((h + 7) * ws + 15) & ~15;
  uint8_t *org_l = smem;
  uint8_t *win = smem + org_bytes + wave * (win_bytes + org_bytes);
  uint8_t *pred = win + win_bytes;

  WgBlock<BPP> b;
  int rng[4];
  const int fbx = t.tx + cd.bx, fby = t.ty + cd.by;
  mv_range(p, fbx, fby, w, h, 0, rng);
  b.w = w; b.h = h;
  b.po_x = fbx * MI; b.po_y = fby * MI;
  b.mvx_min = rng[0]; b.mvx_max = rng[1]; b.mvy_min = rng[2]; b.mvy_max = rng[3];
  b.mc.lambda = p.lambda[0];
  b.mc.allow_hp = p.allow_hp;
  for (int k = 0; k < 2; k++) { b.mc.pmv_row[k] = cd.pmv[k][0]; b.mc.pmv_col[k] = cd.pmv[k][1]; }
  const R1Plane &org = job.org[0], &ref = job.ref[0];
  b.sr = (long)ref.stride * BPP;
  b.ref0 = px_addr<BPP>(ref, b.po_x, b.po_y);
  b.wave = wave; b.lane = lane;
  b.RH = h < 16 ? 16 : h;
  b.r = lane % b.RH; b.slot = lane / b.RH; b.ncs = 64 / b.RH;
  b.org = org_l;
  b.red = sh_red;
  {   // source block -> LDS (4-px granules)
    const int gpr = w / 4, ng = gpr * h;
    const uint8_t *o0 = px_addr<BPP>(org, b.po_x, b.po_y);
    for (int i = threadIdx.x; i < ng; i += 256) {
      const int rr = i / gpr, g = i - rr * gpr;
      const uint8_t *src = o0 + (long)rr * org.stride * BPP + g * 4 * BPP;
      if constexpr (BPP == 1) *(uint32_t *)(org_l + rr * w + 4 * g) = ld_u32(src);
      else {
        const U32x2 v = ld_u32x2(src);
        *(uint32_t *)(org_l + (rr * w + 4 * g) * 2) = v.a;
        *(uint32_t *)(org_l + (rr * w + 4 * g) * 2 + 4) = v.b;
      }
    }
  }
  __syncthreads();

  Msr best = full_pixel_me(b, t, p, cd.bx, cd.by, rng, cd.corner, false, 0, sh_subsets[wave]);

  auto in_range = [&](int row, int col) {
    return col >= b.mvx_min && col <= b.mvx_max && row >= b.mvy_min && row <= b.mvy_max;
  };
  if (use_satd) {
    // get_fullpel_mv_rd(best.mv, use_satd) (me.rs:596-613); every wave computes the same
    if (!in_range(best.row, best.col)) {
      best.cost = COST_MAX;
      best.sad = 0xFFFFFFFFu;
    } else {
      const uint32_t d = b.predict_dist(ref, win, pred, b.po_x + div8(best.col),
                                        b.po_y + div8(best.row), 0, 0, filter_mode, true);
      best.sad = d;
      best.cost = b.mc.cost(best.row, best.col, d);
    }
  }
  // subpel_diamond_search: wave v <-> DIAMOND_R1_PATTERN_SUBPEL[v]
  int radius_log2 = 2;
  const int end_log2 = p.allow_hp ? 0 : 1;
  for (;;) {
    int row = (int16_t)(best.row + (kDiamond[wave][0] << radius_log2));
    int col = (int16_t)(best.col + (kDiamond[wave][1] << radius_log2));
    unsigned long long cost = COST_MAX;
    uint32_t sad = 0xFFFFFFFFu;
    if (in_range(row, col)) {
      // get_mv_params (src/predict.rs:284-297): floor offset, 1/16 fraction
      sad = b.predict_dist(ref, win, pred, b.po_x + (col >> 3), b.po_y + (row >> 3),
                           (col << 1) & 15, (row << 1) & 15, filter_mode, use_satd != 0);
      cost = b.mc.cost(row, col, sad);
    }
    int idx = wave;
    b.wg_min(cost, idx, row, col, sad);
    if (best.cost <= cost) {
      if (radius_log2 == end_log2) break;
      radius_log2--;
    } else {
      best = Msr{row, col, cost, sad};
    }
  }
  if (threadIdx.x == 0) {
    R1MeResult r;
    r.row = (int16_t)best.row;
    r.col = (int16_t)best.col;
    r.sad = best.sad;
    r.cost = best.cost;
    out[blockIdx.x] = r;
  }
}

// Blocks up to 16x16: ONE WAVE per block (four independent blocks per
// workgroup, no workgroup barrier anywhere).  Full-pel steps run on the tile
// ME's wave-level engine (source rows in registers, 4 candidates x 16 rows);
// in the sub-pel diamond the four 16-lane groups of the wave each own one
// candidate: window staging, put_8tap (lane = column), SATD / SAD with one lane
// per Hadamard tile, all inside the group; the four costs meet by shuffles.
// The whole search is one launch.  Split in two (the full-pel search, then the sub-pel refinement, the result of the
// first travelling through `out`), it was 3-7 % SLOWER (profiles/r06_ab_notes.md, ab3).  What that showed: the
// full-pel half needs 61 / 64 VGPRs; the 168 VGPRs + 168 / 196 B of scratch (381 MB of scratch writes per 4K launch,
// profiles/r05_pmc_frame.json) are the sub-pel half's alone (eight inlined (size, bit depth) forms of the
// fused-candidate column filter + SATD), and giving it 223 VGPRs (two workgroups per CU, 0 B scratch) is SLOWER than
// three with the spills: the launch is a latency chain per block like the tile search, the scratch stores are not on it.
// (__launch_bounds__: three workgroups of 4 waves the register allocator makes room for)
template <int BPP>
__global__ __launch_bounds__(256, 3) void k_me_blocks_small(R1MeJob job, R1MeParams p,
                                                            const R1MeBlockCand *__restrict__ cands,
                                                            int n, int max_w, int max_h, int use_satd,
                                                            int filter_mode,
                                                            R1MeResult *__restrict__ out) {
  constexpr int WS_MAX = r1mc::window_stride(16, BPP);
  constexpr int GROUP_BYTES = ((23 * WS_MAX + 15) & ~15) + 16 * 16 * BPP;   // window + prediction
  __shared__ __attribute__((aligned(16))) uint8_t sh_grp[4][4][GROUP_BYTES];
  __shared__ int16_t sh_subsets[4][kSubsetWords];
  __shared__ __attribute__((aligned(16))) uint8_t sh_src[4][16 * 16 * BPP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // an XCD takes a contiguous run of the block list (common.hpp): callers list blocks in raster order, and the search
  // windows of neighbouring blocks overlap -- dealt round-robin, every XCD's L2 fetched the whole reference
  const long long bi = (long long)xcd_run_item(blockIdx.x, gridDim.x) * 4 + wave;
  if (bi >= n) return;                         // wave-uniform; no barriers below
  const R1MeBlockCand cd = cands[bi];
  const int w = cd.w, h = cd.h;
  if (w > max_w || h > max_h || w > 16 || h > 16 || w < 4 || h < 4 || (w & (w - 1)) || (h & (h - 1))) {
    if (lane == 0) out[bi] = R1MeResult{0, 0, 0xFFFFFFFFu, COST_MAX};
    return;
  }
  TileView t{job.stats, job.prev, p.stats_cols, p.stats_rows, job.tile_x / MI, job.tile_y / MI,
             job.tile_w / MI, job.tile_h / MI};
  const R1Plane &org = job.org[0], &ref = job.ref[0];
  Block<BPP, 16> b;
  int rng[4];
  const int fbx = t.tx + cd.bx, fby = t.ty + cd.by;
  mv_range(p, fbx, fby, w, h, 0, rng);
  b.w = w; b.h = h;
  b.po_x = fbx * MI; b.po_y = fby * MI;
  b.mvx_min = rng[0]; b.mvx_max = rng[1]; b.mvy_min = rng[2]; b.mvy_max = rng[3];
  b.mc.lambda = p.lambda[0];
  b.mc.allow_hp = p.allow_hp;
  for (int k = 0; k < 2; k++) { b.mc.pmv_row[k] = cd.pmv[k][0]; b.mc.pmv_col[k] = cd.pmv[k][1]; }
  Msr best;
  b.init(org, ref, lane);
  best = full_pixel_me(b, t, p, cd.bx, cd.by, rng, cd.corner, false, 0, sh_subsets[wave]);

  auto in_range = [&](int row, int col) {
    return col >= b.mvx_min && col <= b.mvx_max && row >= b.mvy_min && row <= b.mvy_max;
  };
  const bool small = (w < h ? w : h) == 4;
  const int ts = small ? 4 : 8, ntx = w / ts, nt = ntx * (h / ts), ln = small ? 2 : 3;
  const uint8_t *o0 = px_addr<BPP>(org, b.po_x, b.po_y);
  const size_t so = (size_t)org.stride * BPP;
  // distortion of the source block against `pp` (row stride sp), one lane per tile of lanes [0, nt)
  auto block_dist = [&](const uint8_t *pp, size_t sp, int gl, bool satd) -> uint32_t {
    uint32_t s = 0;
    if (gl < nt) {
      const int tx = gl % ntx, ty = gl / ntx;
      const uint8_t *a = o0 + (size_t)ty * ts * so + (size_t)tx * ts * BPP;
      const uint8_t *c = pp + (size_t)ty * ts * sp + (size_t)tx * ts * BPP;
      if (satd) s = small ? r1dist::tile_dist<BPP, 4, true>(a, so, c, sp) : r1dist::tile_dist<BPP, 8, true>(a, so, c, sp);
      else s = small ? r1dist::tile_dist<BPP, 4, false>(a, so, c, sp) : r1dist::tile_dist<BPP, 8, false>(a, so, c, sp);
    }
    return s;
  };
  if (use_satd) {
    // get_fullpel_mv_rd(best.mv, use_satd) (me.rs:596-613): the block at the integer position
    if (!in_range(best.row, best.col)) {
      best.cost = COST_MAX;
      best.sad = 0xFFFFFFFFu;
    } else {
      const uint8_t *rp = px_addr<BPP>(ref, b.po_x + div8(best.col), b.po_y + div8(best.row));
      uint32_t s = block_dist(rp, (size_t)ref.stride * BPP, lane, true);
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
      best.sad = (s + ((1u << ln) >> 1)) >> ln;
      best.cost = b.mc.cost(best.row, best.col, best.sad);
    }
  }
  // subpel_diamond_search: 16-lane group g <-> DIAMOND_R1_PATTERN_SUBPEL[g]
  const int g = lane >> 4, gl = lane & 15;
  uint8_t *win = sh_grp[wave][g];
  uint8_t *pred = win + ((23 * WS_MAX + 15) & ~15);
  const int ws = r1mc::window_stride(w, BPP);
  int radius_log2 = 2;
  const int end_log2 = p.allow_hp ? 0 : 1;
  // blocks whose sides are 8 or 16: the source block waits in LDS for the whole search
  const bool fast = (w == 8 || w == 16) && (h == 8 || h == 16);
  uint8_t *srcc = sh_src[wave];
  if (fast) {
    const int wl = w == 16 ? 4 : 3;
    for (int i = lane; i < w * h; i += 64) {
      const int r = i >> wl, c = i & (w - 1);
      if constexpr (BPP == 1) srcc[i] = (uint8_t)ld_px<1>(o0 + (size_t)r * so + c);
      else ((uint16_t *)srcc)[i] = (uint16_t)ld_px<2>(o0 + (size_t)r * so + c * 2);
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (;;) {
    int row = (int16_t)(best.row + (kDiamond[g][0] << radius_log2));
    int col = (int16_t)(best.col + (kDiamond[g][1] << radius_log2));
    const bool ok = in_range(row, col);
    uint32_t s = 0;
    if (fast) {   // wave-uniform: 8 / 16 sizes on the fused-candidate machinery
      if (ok) {
        const int x = b.po_x + (col >> 3), y = b.po_y + (row >> 3), cf = (col << 1) & 15, rf = (row << 1) & 15;
        const bool sd = use_satd != 0;
        const int bd = ref.bit_depth;
#define R1_SP(W_, H_, BD_) s = subpel_group_dist<BPP, W_, H_, BD_>(win, ref, x, y, cf, rf, filter_mode, gl, lane, srcc, sd, bd)
#define R1_SP_BD(W_, H_)                                                  \
  do {                                                                    \
    if constexpr (BPP == 1) R1_SP(W_, H_, 8);                             \
    else if (bd <= 10) R1_SP(W_, H_, 10);                                 \
    else R1_SP(W_, H_, 12);                                               \
  } while (0)
        if (w == 16 && h == 16) R1_SP_BD(16, 16);
        else if (w == 8 && h == 8) R1_SP_BD(8, 8);
        else if (w == 16) R1_SP_BD(16, 8);
        else R1_SP_BD(8, 16);
#undef R1_SP_BD
#undef R1_SP
      }
    } else {
    if (ok) {
      // get_mv_params (src/predict.rs:284-297): floor offset, 1/16 fraction
      r1mc::stage_window<BPP>(win, ws, ref, b.po_x + (col >> 3), b.po_y + (row >> 3), w, h, gl, 16);
    }
    __builtin_amdgcn_wave_barrier();
    if (ok && gl < w) {
      if constexpr (BPP == 1)
        r1mc::mc_column<BPP, false, 0>(win, ws, gl, w, h, (col << 1) & 15, (row << 1) & 15, filter_mode,
                                       filter_mode, ref.bit_depth,
                                       [&](int rr, int32_t v) { pred[rr * w + gl] = (uint8_t)v; });
      else
        r1mc::mc_column<BPP, false, 0>(win, ws, gl, w, h, (col << 1) & 15, (row << 1) & 15, filter_mode,
                                       filter_mode, ref.bit_depth, [&](int rr, int32_t v) {
                                         ((uint16_t *)pred)[rr * w + gl] = (uint16_t)v;
                                       });
    }
    __builtin_amdgcn_wave_barrier();
    if (ok) s = block_dist(pred, (size_t)w * BPP, gl, use_satd != 0);
    }
    s = group_sum<16>(s);
    uint32_t sad = use_satd ? (s + ((1u << ln) >> 1)) >> ln : s;
    unsigned long long cost = ok ? b.mc.cost(row, col, sad) : COST_MAX;
    if (!ok) sad = 0xFFFFFFFFu;
    // the same argmin as MeCand::xor_min(16, WAVE), on the loop's own variables: with the candidate in a MeCand this
    // kernel (168 VGPRs, spills) changed its spill pattern and lost 0.4 - 0.5 % (profiles/r08_reduce_ab_notes.md)
    int idx = g;
#pragma unroll
    for (int m = 16; m < WAVE; m <<= 1) {
      const unsigned long long oc = shfl_xor_u64(cost, m);
      const int oi = __shfl_xor(idx, m, WAVE), orow = __shfl_xor(row, m, WAVE), ocol = __shfl_xor(col, m, WAVE);
      const uint32_t os = (uint32_t)__shfl_xor((int)sad, m, WAVE);
      if (oc < cost || (oc == cost && oi < idx)) { cost = oc; idx = oi; row = orow; col = ocol; sad = os; }
    }
    if (best.cost <= cost) {
      if (radius_log2 == end_log2) break;
      radius_log2--;
    } else {
      best = Msr{row, col, cost, sad};
    }
  }
  if (lane == 0) {
    R1MeResult r;
    r.row = (int16_t)best.row;
    r.col = (int16_t)best.col;
    r.sad = best.sad;
    r.cost = best.cost;
    out[bi] = r;
  }
}

}  // namespace

// k_me_blocks' dynamic LDS at 64x64, 16-bit: source + 4 x (window + prediction) -- above the
// 64 KB default, so the limit is raised ONCE per context (ctx.hip) to this worst case; a
// per-launch setting would race between threads sharing a context.
static constexpr size_t kMeBlocksMaxLds = 8192 + 4 * ((((size_t)(64 + 7) * 144 + 15) & ~(size_t)15) + 8192);

int r1_me_kernel_attrs() {
  R1_HIP_CHECK(hipFuncSetAttribute((const void *)k_me_blocks<1>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMeBlocksMaxLds));
  R1_HIP_CHECK(hipFuncSetAttribute((const void *)k_me_blocks<2>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMeBlocksMaxLds));
  return R1_OK;
}

extern "C" int r1_estimate_motion_batch(r1_ctx *ctx, const R1MeJob *tile, const R1MeParams *params,
                                        const R1MeBlockCand *cands, int n, int max_w, int max_h,
                                        int use_satd, int filter_mode, R1MeResult *out,
                                        void *stream) {
  R1_REQUIRE(ctx && tile && params);
  R1_REQUIRE(r1_depth_ok(params->bit_depth));
  R1_REQUIRE(filter_mode >= 0 && filter_mode <= 3);
  R1_REQUIRE(r1_is_pow2(max_w) && r1_is_pow2(max_h) && max_w >= 4 && max_h >= 4 && max_w <= 64 &&
             max_h <= 64);
  R1_REQUIRE(tile->stats && tile->org[0].data && tile->ref[0].data);
  R1_REQUIRE(tile->tile_x % SB == 0 && tile->tile_y % SB == 0 && tile->tile_w % MI == 0 &&
             tile->tile_h % MI == 0 && tile->tile_w > 0 && tile->tile_h > 0);
  const int bpp = tile->org[0].bytes_per_px;
  R1_REQUIRE(r1_px_ok(bpp) && r1_same_px(tile->org[0], tile->ref[0]));
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands && out);
  hipStream_t st = (hipStream_t)stream;
  if (max_w <= 16 && max_h <= 16) {   // one wave per block
    const unsigned grid = (unsigned)((n + 3) / 4);
    r1_by_bpp(bpp, [&](auto B) {
      hipLaunchKernelGGL(k_me_blocks_small<B.value>, dim3(grid), dim3(256), 0, st, *tile, *params, cands, n, max_w,
                         max_h, use_satd, filter_mode, out);
    });
    R1_HIP_CHECK(hipGetLastError());
    return R1_OK;
  }
  // LDS for the largest block of the batch: source + 4 x (window + prediction)
  const int ws = r1mc::window_stride(max_w, bpp);
  const size_t blk = ((size_t)max_w * max_h * bpp + 15) & ~(size_t)15;
  const size_t lds = blk + 4 * ((((size_t)(max_h + 7) * ws + 15) & ~(size_t)15) + blk);
  R1_REQUIRE(lds <= kMeBlocksMaxLds);
  r1_by_bpp(bpp, [&](auto B) {
    hipLaunchKernelGGL(k_me_blocks<B.value>, dim3(n), dim3(256), lds, st, *tile, *params, cands, max_w, max_h, use_satd,
                       filter_mode, out);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

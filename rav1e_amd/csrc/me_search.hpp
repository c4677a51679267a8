// me_search.hpp -- the search engine of the motion estimation units: me_tile.hip (hierarchical motion estimation
// of whole tiles, k_me_diag / k_me_persist) and me_blocks.hip (the RDO-time block search, k_me_blocks*)
// (SURVEY.md 8f "N2"; reference src/me.rs: estimate_tile_motion 153-218,
// estimate_sb_motion 220-282, refine_subsampled_sb_motion 284-322,
// get_subset_predictors 386-534, estimate_motion 536-632,
// refine_subsampled_motion_estimate 634-691, full_pixel_me 693-855,
// get_best_predictor 884-911, fullpel_diamond_search 955-1000, hexagon_search
// 1055-1141, uneven_multi_hex_search 1170-1309, full_search 1464-1510,
// compute_mv_rd 1445-1462, get_mv_rate 1512-1523).
//
// What is parallel and what is not.  The reference walks the superblocks of a
// tile in raster order; a block's predictors are the (already updated) MEStats
// left of and above it plus the (not yet updated) ones right of and below it
// (me.rs:417-457), so the exact dependence graph is a wavefront: SB (x, y)
// needs (x-1, y) and (x, y-1) finished and (x+1, y), (x, y+1) untouched.
//   * one LAUNCH per anti-diagonal of superblocks; the three passes (quarter,
//     half, full resolution) run in the SAME launches, pass q two diagonals
//     behind pass q - 1 (k_me_diag: a pass needs its predecessor finished one
//     diagonal ahead, nothing more) -- the same-diagonal SBs of ALL jobs (tiles
//     x reference frames) run concurrently, grid = (diag length, jobs, passes);
//   * one WORKGROUP (4 waves) per superblock: first the refinement of the
//     previous pass' blocks (4x4 full search, me.rs:663-676), then the pass' own
//     blocks along the anti-diagonals INSIDE the superblock, one wave per block;
//   * inside a wave the candidates of one search step are evaluated together:
//     16-row blocks put 4 candidates x 16 rows on the 64 lanes, 32-row blocks
//     2 x 32; a lane holds its source row in registers, pulls the candidate's
//     reference row with unaligned dword loads (L2-resident: the search window
//     of a block is a few KB) and SADs it with v_sad_u8 / v_sad_u16; the row
//     sums meet in a segmented wave reduction; "first strictly smaller cost
//     wins" of the reference's sequential loops is an argmin with the lower
//     candidate index breaking ties.
// Every search loop of the reference is data dependent (it recentres on the
// best candidate), so a block's search is a chain of such steps; the chip is
// filled by jobs x superblocks-on-the-diagonal x blocks, not by one block.
// Device code only, in an anonymous namespace: the tables and the R1_ME_PROF counters are file-local to each unit.
#pragma once
#include "common.hpp"

namespace {
constexpr int MI = 4, SB = 64;
constexpr unsigned long long COST_MAX = ~0ull;

struct Msr {   // MotionSearchResult: wave-uniform, replicated in every lane
  int row, col;
  unsigned long long cost;
  uint32_t sad;
};
__device__ __forceinline__ Msr msr_empty() { return Msr{0, 0, COST_MAX, 0xFFFFFFFFu}; }

struct MeCand {   // one lane's candidate of a search step
  unsigned long long cost;
  int idx, row, col;
  uint32_t sad;
  // argmin over the lanes that differ in the bits from <= m < to (powers of two): the lower cost, on a tie the
  // lower candidate index (`if rd.cost < best.rd.cost { best = cand }` in candidate order); every lane of such a
  // group ends up with the winner
  __device__ __forceinline__ void xor_min(int from, int to) {
#pragma unroll
    for (int m = from; m < to; m <<= 1) {
      const unsigned long long oc = shfl_xor_u64(cost, m);
      const int oi = __shfl_xor(idx, m, WAVE), orow = __shfl_xor(row, m, WAVE), ocol = __shfl_xor(col, m, WAVE);
      const uint32_t os = (uint32_t)__shfl_xor((int)sad, m, WAVE);
      if (oc < cost || (oc == cost && oi < idx)) { cost = oc; idx = oi; row = orow; col = ocol; sad = os; }
    }
  }
};

__device__ __forceinline__ int ilog_abs(int d) {   // ILog::ilog(d.abs())
  const uint32_t a = (uint32_t)(d < 0 ? -d : d);
  return a ? 32 - __clz(a) : 0;
}
__device__ __forceinline__ int div8(int v) { return (v + ((v >> 31) & 7)) >> 3; }   // trunc

// compute_mv_rd's cost (me.rs:1456-1461) from a distortion
struct MvCost {
  uint32_t lambda;
  int allow_hp;
  int pmv_row[2], pmv_col[2];
  __device__ __forceinline__ uint32_t rate1(int row, int col, int k) const {
    const int dr = (int16_t)(row - pmv_row[k]), dc = (int16_t)(col - pmv_col[k]);
    return 2u * (uint32_t)(ilog_abs(allow_hp ? dr : dr >> 1) + ilog_abs(allow_hp ? dc : dc >> 1));
  }
  __device__ __forceinline__ unsigned long long cost(int row, int col, uint32_t dist) const {
    const uint32_t r1 = rate1(row, col, 0), r2 = rate1(row, col, 1) + 1;
    return 256ull * dist + (unsigned long long)(r1 < r2 ? r1 : r2) * lambda;
  }
};

// One block of one wave.  RH = rows per candidate slot (16 or 32): the block
// is at most RH x RH; 64 / RH candidates are evaluated per step.
// KM: candidate batches in flight per search step; 0 = by register budget (three while a batch is
// <= 4 registers, else two: k_me_diag lives on 96 registers); k_me_persist, at two waves per SIMD,
// affords three always (five: equal, eight: slower -- profiles/r02_me_persistent_experiment.md)
template <int BPP, int RH, int KM = 0>
struct Block {
  static constexpr int NCS = 64 / RH, GR = RH / 4, WPG = BPP;   // dwords per 4-px granule
  const uint8_t *ref0;   // (po.x, po.y) of the reference plane
  long sr;               // reference stride, bytes
  int w, h, po_x, po_y;
  int mvx_min, mvx_max, mvy_min, mvy_max;
  MvCost mc;
  int r, slot;               // this lane: row, candidate slot
  uint32_t o[GR * WPG];      // source row (masked)
  uint32_t m[GR * WPG];      // pixel masks of this row: 0 beyond (w, h)

  __device__ __forceinline__ void init(const R1Plane &org, const R1Plane &ref, int lane) {
    r = lane & (RH - 1);
    slot = lane / RH;
    sr = (long)ref.stride * BPP;
    ref0 = px_addr<BPP>(ref, po_x, po_y);
    const uint8_t *op = px_addr<BPP>(org, po_x, po_y) + (long)r * org.stride * BPP;
#pragma unroll
    for (int g = 0; g < GR; g++) {
      int npx = w - 4 * g;
      npx = r < h ? (npx < 0 ? 0 : (npx > 4 ? 4 : npx)) : 0;
      if constexpr (BPP == 1) {
        m[g] = npx >= 4 ? 0xFFFFFFFFu : ((1u << (8 * npx)) - 1u);
        o[g] = m[g] ? ld_u32(op + 4 * g) & m[g] : 0u;
      } else {
        m[2 * g] = npx >= 2 ? 0xFFFFFFFFu : (npx == 1 ? 0xFFFFu : 0u);
        m[2 * g + 1] = npx >= 4 ? 0xFFFFFFFFu : (npx == 3 ? 0xFFFFu : 0u);
        U32x2 v = {0u, 0u};
        if (m[2 * g]) v = ld_u32x2(op + 8 * g);
        o[2 * g] = v.a & m[2 * g];
        o[2 * g + 1] = v.b & m[2 * g + 1];
      }
    }
  }

  // compute_mv_rd of this lane's slot candidate (me.rs:1386-1462) in two halves, so that a
  // search step can have the reference rows of SEVERAL candidate batches in flight before the
  // first SAD: a block's search is a chain of dependent steps and a step is one memory round
  // trip -- batches that do not depend on each other (a predictor list, a search pattern)
  // share one.  check: the MV range test of get_fullpel_mv_rd (full_search calls
  // compute_mv_rd without it).
  __device__ __forceinline__ bool fetch(int row, int col, bool valid, bool check, uint32_t *v) const {
    bool in = valid;
    if (check) in = in && col >= mvx_min && col <= mvx_max && row >= mvy_min && row <= mvy_max;
#pragma unroll
    for (int g = 0; g < GR * WPG; g++) v[g] = 0;
    if (in) {
      const uint8_t *p = ref0 + (long)(div8(row) + r) * sr + (long)div8(col) * BPP;
#pragma unroll
      for (int g = 0; g < GR; g++) {
        if constexpr (BPP == 1) {
          if (m[g]) v[g] = ld_u32(p + 4 * g);
        } else {
          if (m[2 * g]) {
            const U32x2 t = ld_u32x2(p + 8 * g);
            v[2 * g] = t.a;
            v[2 * g + 1] = t.b;
          }
        }
      }
    }
    return in;
  }
  // every lane of the slot returns the same (cost, sad)
  __device__ __forceinline__ void finish(const uint32_t *v, bool in, int row, int col,
                                         unsigned long long &cost, uint32_t &sad) const {
    uint32_t part = 0;
#pragma unroll
    for (int g = 0; g < GR * WPG; g++) {
      if constexpr (BPP == 1) part = __builtin_amdgcn_sad_u8(o[g], v[g] & m[g], part);
      else part = __builtin_amdgcn_sad_u16(o[g], v[g] & m[g], part);
    }
    part = group_sum<RH>(part);   // DPP inside a 16-lane row: no LDS round trips
    cost = in ? mc.cost(row, col, part) : COST_MAX;
    sad = in ? part : 0xFFFFFFFFu;
  }

  // one batch of NCS candidates after its rows have arrived: the slots' costs meet, the
  // lower candidate index wins ties, `if rd.cost < best.rd.cost { best = cand }`
  __device__ __forceinline__ void settle(const uint32_t *v, bool in, int idx, int row, int col, Msr &best,
                                         int *best_idx) const {
    unsigned long long cost;
    uint32_t sad;
    finish(v, in, row, col, cost, sad);
    // Every lane of a slot holds its slot's (cost, sad, idx, row, col): the NCS costs go to SCALAR registers with
    // v_readlane (a few cycles each, no LDS crossbar round trip as a ds_bpermute shuffle is) and the tournament runs
    // on the scalar unit (instead of an xor-shuffle tournament: profiles/r06_ab_notes.md, ab5).  idx grows with the
    // slot number, so "the lower index wins ties" is a strict less-than.
    {
      int ws = 0;
      unsigned long long wc = readlane_u64(cost, 0);
#pragma unroll
      for (int sl = 1; sl < NCS; sl++) {
        const unsigned long long c = readlane_u64(cost, sl * RH);
        if (c < wc) { wc = c; ws = sl; }
      }
      const int wl = ws * RH;
      cost = wc;
      idx = __builtin_amdgcn_readlane(idx, wl);
      row = __builtin_amdgcn_readlane(row, wl);
      col = __builtin_amdgcn_readlane(col, wl);
      sad = (uint32_t)__builtin_amdgcn_readlane((int)sad, wl);
    }
    if (cost < best.cost) {
      best = Msr{row, col, cost, sad};
      if (best_idx) *best_idx = idx;
    }
  }

  // K batches with their loads issued back to back, settled in candidate order
  template <int K, class Gen>
  __device__ __forceinline__ void step(int base, int n, Gen gen, bool check, Msr &best, int *best_idx) const {
    uint32_t v[K][GR * WPG];
    int idx[K], row[K], col[K];
    bool in[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      idx[k] = base + k * NCS + slot;
      const bool valid = idx[k] < n;
      row[k] = col[k] = 0;
      if (valid) gen(idx[k], row[k], col[k]);
      in[k] = fetch(row[k], col[k], valid, check, v[k]);
    }
#pragma unroll
    for (int k = 0; k < K; k++) settle(v[k], in[k], idx[k], row[k], col[k], best, best_idx);
  }

  // two independent candidate lists (each at most one batch) evaluated in ONE round trip, each
  // into its own result: the second list is a speculation whose result the caller may drop
  template <class GenA, class GenB>
  __device__ __forceinline__ void scan_pair(int na, GenA gen_a, Msr &best_a, int nb, GenB gen_b, Msr &best_b,
                                            bool check) const {
    if (na > NCS || nb > NCS) {
      scan(na, gen_a, check, best_a, nullptr);
      scan(nb, gen_b, check, best_b, nullptr);
      return;
    }
    uint32_t va[GR * WPG], vb[GR * WPG];
    int ra = 0, ca = 0, rb = 0, cb = 0;
    if (slot < na) gen_a(slot, ra, ca);
    if (slot < nb) gen_b(slot, rb, cb);
    const bool ia = fetch(ra, ca, slot < na, check, va), ib = fetch(rb, cb, slot < nb, check, vb);
    settle(va, ia, slot, ra, ca, best_a, nullptr);
    settle(vb, ib, slot, rb, cb, best_b, nullptr);
  }

  // `for cand in cands { if rd.cost < best.rd.cost { best = cand } }` over
  // n candidates produced by gen(idx, row, col); best_idx: index of the taken one.
  // batches in flight: GR * WPG registers each.  Measured (profiles/r02_me_batch_ab.log): three for
  // 16-row slots of 8-bit pixels (4 registers a batch); two everywhere else -- a third batch of 8 or 16
  // registers spills and made the 10-bit search 18 % slower than two
  static constexpr int KMAX = KM ? KM : ((GR * WPG <= 4) ? 3 : 2);
  template <class Gen>
  __device__ __forceinline__ void scan(int n, Gen gen, bool check, Msr &best, int *best_idx) const {
    int base = 0;
    while (base < n) {
      const int left = n - base;
      if (KMAX >= 3 && left > 2 * NCS) {
        step<KMAX >= 3 ? 3 : 2>(base, n, gen, check, best, best_idx);
        base += (KMAX >= 3 ? 3 : 2) * NCS;
      } else if (KMAX >= 2 && left > NCS) {
        step<2>(base, n, gen, check, best, best_idx);
        base += 2 * NCS;
      } else {
        step<1>(base, n, gen, check, best, best_idx);
        base += NCS;
      }
    }
  }
};

#ifdef R1_ME_PROF
// [0] predictor gather, [1] the candidate scan, [2] the diamond, [3] diamond iterations, [4] searches (non-extensive)
__device__ unsigned long long g_me_fine[8];
#endif
__constant__ int8_t kDiamond[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};   // (row, col)
__constant__ int8_t kHexagon[6][2] = {{-2, 0}, {-1, 2}, {1, 2}, {2, 0}, {1, -2}, {-1, -2}};
__constant__ int8_t kSquare[8][2] = {{1, -1}, {1, 0}, {1, 1}, {0, -1}, {0, 1}, {-1, -1}, {-1, 0}, {-1, 1}};
// UMH_PATTERN as written in the reference (entry 13 repeats entry 7), me.rs:1153-1156
__constant__ int8_t kUmh[16][2] = {{4, -2}, {4, -1}, {4, 0}, {4, 1}, {4, 2}, {2, 3}, {0, 4}, {-2, 3},
                                   {-4, 2}, {-4, 1}, {-4, 0}, {-4, -1}, {-4, -2}, {-2, 3}, {0, -4}, {2, -3}};

template <class B>
__device__ __forceinline__ void fullpel_diamond_search(const B &b, Msr &cur) {
  // me.rs:955-1000: radius 2 until no candidate improves, then radius 1 until none does.  While at
  // radius 2 the four radius-1 candidates of the same centre are fetched in the same round trip:
  // they are what the next step evaluates whenever radius 2 brings no improvement (the common
  // case at the end of every search); otherwise the speculation is dropped.  Same evaluations,
  // same comparisons, same order -- one memory latency less per search.
  int radius_log2 = 1;
  for (;;) {
#ifdef R1_ME_PROF
    if (threadIdx.x == 0) atomicAdd(&g_me_fine[3], 1ull);
#endif
    Msr best = msr_empty();
    const int cr = cur.row, cc = cur.col;
    if (radius_log2 == 1) {
      Msr next = msr_empty();
      b.scan_pair(4, [&](int i, int &row, int &col) {
        row = (int16_t)(cr + (kDiamond[i][0] << 4));
        col = (int16_t)(cc + (kDiamond[i][1] << 4));
      }, best, 4, [&](int i, int &row, int &col) {
        row = (int16_t)(cr + (kDiamond[i][0] << 3));
        col = (int16_t)(cc + (kDiamond[i][1] << 3));
      }, next, true);
      if (cur.cost <= best.cost) {
        radius_log2 = 0;
        if (cur.cost <= next.cost) break;   // the radius-1 step of this centre
        cur = next;
      } else {
        cur = best;
      }
      continue;
    }
    b.scan(4, [&](int i, int &row, int &col) {
      row = (int16_t)(cr + (kDiamond[i][0] << 3));
      col = (int16_t)(cc + (kDiamond[i][1] << 3));
    }, true, best, nullptr);
    if (cur.cost <= best.cost) break;
    cur = best;
  }
}

template <class B>
__device__ __forceinline__ void hexagon_search(const B &b, Msr &cur) {
  int best_idx = 0;
  Msr best = msr_empty();
  {
    const int cr = cur.row, cc = cur.col;
    b.scan(6, [&](int i, int &row, int &col) {
      row = (int16_t)(cr + kHexagon[i][0] * 8);
      col = (int16_t)(cc + kHexagon[i][1] * 8);
    }, true, best, &best_idx);
  }
  while (best.cost < cur.cost) {
    cur = best;
    best = msr_empty();
    const int center = best_idx, cr = cur.row, cc = cur.col;
    int k = 0;
    // the three directions next to the one just taken; k is the visiting order
    b.scan(3, [&](int j, int &row, int &col) {
      const int i = (center + 5 + j) % 6;
      row = (int16_t)(cr + kHexagon[i][0] * 8);
      col = (int16_t)(cc + kHexagon[i][1] * 8);
    }, true, best, &k);
    best_idx = (center + 5 + k) % 6;
  }
  best = msr_empty();
  {
    const int cr = cur.row, cc = cur.col;
    b.scan(8, [&](int i, int &row, int &col) {
      row = (int16_t)(cr + kSquare[i][0] * 8);
      col = (int16_t)(cc + kSquare[i][1] * 8);
    }, true, best, nullptr);
  }
  if (best.cost < cur.cost) cur = best;
}

template <class B>
__device__ __forceinline__ void uneven_multi_hex_search(const B &b, Msr &cur, int me_range) {
  {
    const int cr = cur.row, cc = cur.col;
    const int nh = (me_range + 1) / 2;   // i = 1, 3, .. <= me_range
    b.scan(2 * nh, [&](int k, int &row, int &col) {
      const int i = 2 * (k >> 1) + 1;
      row = (int16_t)(cr + ((k & 1) ? 8 : -8) * i);   // the reference's "horizontal" line steps the row
      col = cc;
    }, true, cur, nullptr);
    const int nv = ((me_range >> 1) + 1) / 2;
    b.scan(2 * nv, [&](int k, int &row, int &col) {
      const int i = 2 * (k >> 1) + 1;
      row = cr;
      col = (int16_t)(cc + ((k & 1) ? 8 : -8) * i);
    }, true, cur, nullptr);
  }
  {   // 5x5: offsets in 1/8 pel as the reference has them (me.rs:1241-1247)
    const int cr = cur.row, cc = cur.col;
    b.scan(24, [&](int k, int &row, int &col) {
      const int j = k >= 12 ? k + 1 : k;   // skip the centre
      row = (int16_t)(cr + j / 5 - 2);
      col = (int16_t)(cc + j % 5 - 2);
    }, true, cur, nullptr);
  }
  {
    const int cr = cur.row, cc = cur.col;
    b.scan(16 * (me_range >> 2), [&](int k, int &row, int &col) {
      const int i = (k >> 4) + 1, p = k & 15;
      row = (int16_t)(cr + kUmh[p][0] * 8 * i);
      col = (int16_t)(cc + kUmh[p][1] * 8 * i);
    }, true, cur, nullptr);
  }
  hexagon_search(b, cur);
}

// full_search (me.rs:1464-1510): rows outer, every `step`-th window
template <class B>
__device__ __forceinline__ Msr full_search(const B &b, int x_lo, int x_hi, int y_lo, int y_hi, int step) {
  Msr best = msr_empty();
  if (x_hi < x_lo || y_hi < y_lo) return best;
  const int nx = (x_hi - x_lo) / step + 1, ny = (y_hi - y_lo) / step + 1;
  b.scan(nx * ny, [&](int k, int &row, int &col) {
    row = (int16_t)(8 * (int16_t)(y_lo + (k / nx) * step - b.po_y));
    col = (int16_t)(8 * (int16_t)(x_lo + (k % nx) * step - b.po_x));
  }, false, best, nullptr);
  return best;
}

struct TileView {
  R1MeStats *stats;
  const R1MeStats *prev;
  int cols_f, rows_f;          // FrameMEStats dims
  int tx, ty, tcols, trows;    // tile origin / size, 4x4 units
  const R1MeStats *rstats = nullptr;   // k_me_persist: the refined statistics (see there)
  __device__ __forceinline__ R1MeStats *at(int y, int x) const {
    return stats + (size_t)(ty + y) * cols_f + tx + x;
  }
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int iclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// MotionEstimationSubsets (me.rs:364-384) of one wave, in LDS (the lists are
// indexed by lane-dependent candidate numbers): (row, col) pairs.
struct Subsets {
  uint32_t min_sad;
  int has_median, nb, nc;
  int16_t *median, *b, *c, *all;   // 1, <= 5, <= 5, <= 11 pairs
};
constexpr int kSubsetWords = 2 * (1 + 5 + 5 + 11);

// one MEStats entry: written by another wave of THIS workgroup a barrier ago
// (same CU, same L1: workgroup scope is enough -- an agent-scope fence per
// diagonal would write back / invalidate the XCD's L2 and made the 64-job
// launches 3.6x slower) or by another workgroup in an earlier launch (kernel
// boundaries make that visible)
template <bool AGENT = false>
__device__ __forceinline__ unsigned long long load_entry(const R1MeStats *s) {
  if constexpr (AGENT)   // k_me_persist: written by a wave anywhere on the device, in this launch
    return __hip_atomic_load((const unsigned long long *)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    return __hip_atomic_load((const unsigned long long *)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool AGENT = false>
__device__ __forceinline__ void load_stats(const R1MeStats *s, int &row, int &col, uint32_t &nsad) {
  const unsigned long long v = load_entry<AGENT>(s);
  row = (int16_t)(v & 0xFFFF);
  col = (int16_t)((v >> 16) & 0xFFFF);
  nsad = (uint32_t)(v >> 32);
}

// process_cand (me.rs:407-414) on a loaded entry
__device__ __forceinline__ void process_cand(unsigned long long v, const int *rng, uint32_t &min_sad,
                                             int16_t *out) {
  const int srow = (int16_t)(v & 0xFFFF), scol = (int16_t)((v >> 16) & 0xFFFF);
  const uint32_t ns = (uint32_t)(v >> 32);
  min_sad = ns < min_sad ? ns : min_sad;
  out[0] = (int16_t)iclamp(div8(srow) * 8, rng[2], rng[3]);
  out[1] = (int16_t)iclamp(div8(scol) * 8, rng[0], rng[1]);
}

// get_subset_predictors (me.rs:386-534).  The up to ten MEStats entries it samples (left, top,
// right, bottom, centre of this frame; the same five of the previous frame) are fetched by ten
// LANES in one load instruction and handed round by shuffles: one memory round trip instead of
// ten dependent ones (a block's search is a latency chain).  Entries of this frame were written
// by another wave of THIS workgroup a barrier ago (same CU, same L1: workgroup scope is enough
// -- an agent-scope fence per diagonal would write back / invalidate the XCD's L2 and made the
// 64-job launches 3.6x slower) or by another workgroup in an earlier launch (kernel boundaries
// make that visible).
template <bool AGENT = false>
__device__ __forceinline__ void get_subset_predictors(const TileView &t, int bx, int by, int pix_w, int pix_h,
                                      const int *rng, int corner, int ssdec, Subsets &s) {
  uint32_t min_sad = 0xFFFFFFFFu;
  s.nb = s.nc = s.has_median = 0;
  const int lane = threadIdx.x & 63;
  const int w = ((pix_w << ssdec) + MI - 1) >> 2, h = ((pix_h << ssdec) + MI - 1) >> 2;
  const int half_w = imin(w >> 1, t.tcols - 1 - bx), half_h = imin(h >> 1, t.trows - 1 - by);
  const int fx = t.tx + bx, fy = t.ty + by;
  const int hw = imin(w >> 1, t.cols_f - 1 - fx), hh = imin(h >> 1, t.rows_f - 1 - fy);
  const bool hp = t.prev != nullptr;
  bool ok[10];
  ok[0] = bx > 0;
  ok[1] = by > 0;
  ok[2] = corner && (corner & 2) && bx + w < t.tcols;
  ok[3] = corner && (corner & 4) && by + h < t.trows;
  ok[4] = corner != 0;
  ok[5] = hp && fx > 0;
  ok[6] = hp && fy > 0;
  ok[7] = hp && fx + w < t.cols_f;
  ok[8] = hp && fy + h < t.rows_f;
  ok[9] = hp;
  // (y, x) of entry `lane` in frame coordinates
  const int ey[10] = {t.ty + by + half_h, t.ty + by - 1, t.ty + by + half_h, t.ty + by + h, t.ty + by + half_h,
                      fy + hh, fy - 1, fy + hh, fy + h, fy + hh};
  const int ex[10] = {t.tx + bx - 1, t.tx + bx + half_w, t.tx + bx + w, t.tx + bx + half_w, t.tx + bx + half_w,
                      fx - 1, fx + hw, fx + w, fx + hw, fx + hw};
  int my_y = 0, my_x = 0;
  bool my_ok = false;
#pragma unroll
  for (int k = 0; k < 10; k++)
    if (lane == k) { my_y = ey[k]; my_x = ex[k]; my_ok = ok[k]; }
  unsigned long long mine = 0;
  if (my_ok) {
    const R1MeStats *base = lane < 5 ? (const R1MeStats *)t.stats : t.prev;
    if constexpr (AGENT) {
      // k_me_persist: the centre, and the right / bottom samples inside this block's own superblock,
      // are the REFINED vectors of the previous pass (second buffer); everything else the live array
      const bool same_sb = ((my_x - t.tx) >> 4) == (bx >> 4) && ((my_y - t.ty) >> 4) == (by >> 4);
      if (lane == 4 || ((lane == 2 || lane == 3) && same_sb)) base = t.rstats;
    }
    mine = load_entry<AGENT && true>(base + (size_t)my_y * t.cols_f + my_x);
  }
  auto entry = [&](int k) -> unsigned long long { return shfl_u64(mine, k); };
  if (ok[0]) process_cand(entry(0), rng, min_sad, s.b + 2 * s.nb++);
  if (ok[1]) process_cand(entry(1), rng, min_sad, s.b + 2 * s.nb++);
  if (ok[2]) process_cand(entry(2), rng, min_sad, s.b + 2 * s.nb++);
  if (ok[3]) process_cand(entry(3), rng, min_sad, s.b + 2 * s.nb++);
  if (corner) {
    s.has_median = 1;
    process_cand(entry(4), rng, min_sad, s.median);
  } else if (s.nb == 3) {
    // unreachable at INIT (at most left + top), kept for the rule's sake: median of three
    s.has_median = 1;
    for (int k = 0; k < 2; k++) {
      const int a = s.b[k], bb = s.b[2 + k], c = s.b[4 + k];
      s.median[k] = (int16_t)imax(imin(a, bb), imin(imax(a, bb), c));
    }
  }
  s.b[2 * s.nb] = 0;
  s.b[2 * s.nb + 1] = 0;
  s.nb++;
  if (hp) {
#pragma unroll
    for (int k = 5; k < 10; k++)
      if (ok[k]) process_cand(entry(k), rng, min_sad, s.c + 2 * s.nc++);
  }
  s.min_sad = (uint32_t)(((unsigned long long)min_sad * (unsigned long long)(pix_w * pix_h)) >> 14);
  // dec_mv (me.rs:519-532) and all_mvs (me.rs:371-383)
  int n = 0;
  if (s.has_median) {
    s.median[0] >>= ssdec;
    s.median[1] >>= ssdec;
    s.all[0] = s.median[0];
    s.all[1] = s.median[1];
    n = 1;
  }
  for (int i = 0; i < 2 * s.nb; i++) s.all[2 * n + i] = (s.b[i] >>= ssdec);
  n += s.nb;
  for (int i = 0; i < 2 * s.nc; i++) s.all[2 * n + i] = (s.c[i] >>= ssdec);
}

// Inlined, the running best by value.  As an out-of-line function (round 4) every call received the Block BY
// REFERENCE: the 112-byte block state (source rows, masks, MV range, cost model) was written to scratch memory per
// block and read back through flat loads by each of the up to four calls of a step, and the running best (20 bytes)
// was stored and reloaded around every call -- all on the dependent chain of the persistent kernel.
template <class B>
__device__ __forceinline__ Msr try_cands(const B &b, const int16_t *list, int n, const Msr best) {
  Msr r = msr_empty();
#ifdef R1_ME_PROF
  const unsigned long long f0 = wall_clock64();
#endif
  b.scan(n, [&](int i, int &row, int &col) { row = list[2 * i]; col = list[2 * i + 1]; }, true, r,
         nullptr);
#ifdef R1_ME_PROF
  const unsigned long long f1 = wall_clock64();
#endif
  fullpel_diamond_search(b, r);
#ifdef R1_ME_PROF
  if (threadIdx.x == 0) {
    atomicAdd(&g_me_fine[1], f1 - f0);
    atomicAdd(&g_me_fine[2], wall_clock64() - f1);
    atomicAdd(&g_me_fine[4], 1ull);
  }
#endif
  return r.cost < best.cost ? r : best;
}

template <class B, bool AGENT = false>
__device__ __forceinline__ Msr full_pixel_me(const B &b, const TileView &t, const R1MeParams &p, int bx, int by,
                             const int *rng, int corner, bool extensive, int ssdec,
                             int16_t *lds) {
  Subsets s;
  s.median = lds;
  s.b = lds + 2;
  s.c = lds + 12;
  s.all = lds + 22;
#ifdef R1_ME_PROF
  const unsigned long long g0 = wall_clock64();
#endif
  get_subset_predictors<AGENT>(t, bx, by, b.w, b.h, rng, corner, ssdec, s);
#ifdef R1_ME_PROF
  if (threadIdx.x == 0) atomicAdd(&g_me_fine[0], wall_clock64() - g0);
#endif
  Msr best = msr_empty();
  if (!extensive) {
    return try_cands(b, s.all, s.has_median + s.nb + s.nc, best);
  }
  // (min_sad as f32 * 1.2) as u32 + ((w * h) << (bit_depth - 8)), me.rs:773-774
  const uint32_t thresh = (uint32_t)__fmul_rn((float)s.min_sad, 1.2f) +
                          ((uint32_t)(b.w * b.h) << (p.bit_depth - 8));
  if (s.has_median) {
    best = try_cands(b, s.median, 1, best);
    if (best.sad < thresh) return best;
  }
  best = try_cands(b, s.b, s.nb, best);
  if (best.sad < thresh) return best;
  best = try_cands(b, s.c, s.nc, best);
  if (best.sad < thresh) return best;
  uneven_multi_hex_search(b, best, 24);
  if (!p.allow_full_search || best.sad < thresh) return best;
  const int range_x = (192 * p.me_range_scale) >> ssdec, range_y = (64 * p.me_range_scale) >> ssdec;
  const Msr r = full_search(b, b.po_x + imax(-range_x, div8(b.mvx_min)),
                            b.po_x + imin(range_x, div8(b.mvx_max)),
                            b.po_y + imax(-range_y, div8(b.mvy_min)),
                            b.po_y + imin(range_y, div8(b.mvy_max)), 4 >> ssdec);
  return r.cost < best.cost ? r : best;
}

// get_mv_range (me.rs:339-362) >> ssdec (me.rs:563-564)
__device__ __forceinline__ void mv_range(const R1MeParams &p, int fbx, int fby, int blk_w, int blk_h,
                                         int ssdec, int *r) {
  const int border_w = 128 + blk_w * 8, border_h = 128 + blk_h * 8;
  r[0] = imax(-fbx * (8 * MI) - border_w, -(1 << 14) + 1) >> ssdec;
  r[1] = imin(((p.w_in_b - fbx) - blk_w / MI) * (8 * MI) + border_w, (1 << 14) - 1) >> ssdec;
  r[2] = imax(-fby * (8 * MI) - border_h, -(1 << 14) + 1) >> ssdec;
  r[3] = imin(((p.h_in_b - fby) - blk_h / MI) * (8 * MI) + border_h, (1 << 14) - 1) >> ssdec;
}

template <class B>
__device__ __forceinline__ void setup_block(B &b, const R1Plane &org, const R1Plane &ref, const R1MeParams &p,
                                            const TileView &t, int bx, int by, int w, int h,
                                            int ssdec, int lane, int *rng) {
  const int fbx = t.tx + bx, fby = t.ty + by;
  mv_range(p, fbx, fby, w << ssdec, h << ssdec, ssdec, rng);
  b.w = w;
  b.h = h;
  b.po_x = (fbx * MI) >> ssdec;
  b.po_y = (fby * MI) >> ssdec;
  b.mvx_min = rng[0]; b.mvx_max = rng[1]; b.mvy_min = rng[2]; b.mvy_max = rng[3];
  // (a select, not p.lambda[ssdec]: a run-time index into the by-value parameter block sends the whole block to
  // scratch memory -- 112 bytes re-read on every step of the persistent kernel's dependent chain)
  b.mc.lambda = ssdec == 0 ? p.lambda[0] : (ssdec == 1 ? p.lambda[1] : p.lambda[2]);
  b.mc.allow_hp = p.allow_hp;
  // estimate_motion with pmv = None / refine_subsampled_motion_estimate: pmv = [0, 0]
  b.mc.pmv_row[0] = b.mc.pmv_row[1] = b.mc.pmv_col[0] = b.mc.pmv_col[1] = 0;
  b.init(org, ref, lane);
}

template <class B>
__device__ __forceinline__ void setup_block(B &b, const R1MeJob &job, const R1MeParams &p,
                                            const TileView &t, int bx, int by, int w, int h,
                                            int ssdec, int lane, int *rng) {
  setup_block(b, job.org[ssdec], job.ref[ssdec], p, t, bx, by, w, h, ssdec, lane, rng);
}

// save_me_stats (me.rs:324-337) with the normalisation of me.rs:268-270
template <bool AGENT = false, bool WIDE = false>
__device__ __forceinline__ void store_result(const TileView &t, int size_in_b, int bx, int by,
                                             const Msr &r, int w, int h, int ssdec, int lane) {
  // shifts where the block area / the entry count per row are powers of two (ab5)
  // (wave-uniform branches: a 64-bit division and two 32-bit ones by run-time values are ~200 dependent instructions
  // between a search's last compare and the progress word its neighbours wait for)
  const uint32_t wh = (uint32_t)(w * h);
  const uint32_t nsad = (wh & (wh - 1)) == 0
                            ? (uint32_t)((((unsigned long long)r.sad) << 14) >> (31 - __clz(wh)))
                            : (uint32_t)((((unsigned long long)r.sad) << 14) / (unsigned long long)wh);
  const int nx = imin(bx + size_in_b, t.tcols) - bx, ny = imin(by + size_in_b, t.trows) - by;
  const bool nx_p2 = (nx & (nx - 1)) == 0;
  const int nx_l2 = 31 - __clz((unsigned)nx);
  R1MeStats v;
  v.row = (int16_t)(r.row << ssdec);
  v.col = (int16_t)(r.col << ssdec);
  v.normalized_sad = nsad;
  if constexpr (AGENT) {
    const unsigned long long bits = ((unsigned long long)v.normalized_sad << 32) |
                                    ((unsigned long long)(uint16_t)v.col << 16) | (uint16_t)v.row;
    // plain stores: the line stays in THIS XCD's L2, where the job's other waves (all on this
    // XCD, see k_me_persist) read it with L1-bypassing loads
    // (WIDE: the job's waves sit on any XCD -- agent-scope stores, written through)
    for (int i = lane; i < nx * ny; i += 64) {
      const int iy = nx_p2 ? i >> nx_l2 : i / nx, ix = nx_p2 ? i & (nx - 1) : i % nx;
      unsigned long long *d = (unsigned long long *)t.at(by + iy, bx + ix);
      if constexpr (WIDE) __hip_atomic_store(d, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *d = bits;
    }
  } else {
    for (int i = lane; i < nx * ny; i += 64) {
      const int iy = nx_p2 ? i >> nx_l2 : i / nx, ix = nx_p2 ? i & (nx - 1) : i % nx;
      *t.at(by + iy, bx + ix) = v;
    }
  }
}
}  // namespace

// rd_pick.hip -- the decision behind the candidate and rate launches, on the device.
// r1_rd_pick_batch: compute_rd_cost (src/rdo.rs:718-723) of every trial of a block and the comparison the reference
// makes with it -- the tail of rdo_tx_type_decision's loop (1801-1818, early exit included), the carry across the
// transform depths of rdo_tx_size_type (780-784) and `rd < best.rd_cost` of luma_chroma_mode_rdo (923-938) -- on a
// 24-byte state per block that is carried from call to call.
// r1_rd_commit_batch: the winner's eobs, coefficients, side bytes and reconstruction gathered to where the next step
// reads them; the reconstruction goes into the plane, which is where the next block's edges come from.
// Both enqueue on the caller's stream; nothing is read back.  Pinned by tests/golden/rd_pick_ref.npz.
#include "block_geom.hpp"
#include "common.hpp"

#include <math.h>

static_assert(sizeof(R1RdPick) == 24, "R1RdPick is 24 bytes");

// ---- the pick ----
struct PickArgs {
  const uint32_t *rate, *rate_add;
  const uint64_t *dist;
  R1RdPick *state;
  uint8_t *invalid;
  double lambda;
  int n_states, trials, nt, rule, call_id, lanes, lanes_log2;
};

// The (cost, trial index) pair with the smaller cost, the smaller index on a tie: the trial a serial walk with
// `rd < best` meets first among the cheapest.
__device__ __forceinline__ void first_min(double &rd, int &idx, double o_rd, int o_idx) {
  if (o_rd < rd || (o_rd == rd && o_idx < idx)) rd = o_rd, idx = o_idx;
}

// Mapping: 2^k lanes per state, 2^k = the state's trial count rounded up to a power of two, 64 at most (args.lanes).
// The kernel is nothing but its loads -- 12 to 16 bytes per trial, 24 written per state -- so what decides is that
// they coalesce for the shapes that occur: a transform-type pick has 1 to 16 trials per state and thousands of
// states, and with one lane per trial the lanes of a wave read one contiguous run of `rate` and `dist` (state s + 1's
// trials follow state s's); a lane per state would stride them by nt words.  A whole wave per state would idle 57 of
// 64 lanes there.  Large groups (up to 4096 trials) get the whole wave, each lane walking trials lane, lane + 64, ...
// The serial rule `rd < best_rd, trials ascending` is kept for any count by carrying the trial's index through the
// reduction: a lane keeps the first of its own minima (its indices ascend), and the butterfly over the group's lanes
// prefers the smaller index between equal costs.  Partners of __shfl_xor with a mask below `lanes` stay inside the
// group; lanes past the last state load nothing and write nothing but take part in the shuffles, so the result does
// not depend on n_states filling the wave or the workgroup.
__global__ __launch_bounds__(256) void k_rd_pick(const PickArgs a) {
  const unsigned long long tid = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const int s = (int)(tid >> a.lanes_log2), sub = (int)threadIdx.x & (a.lanes - 1);   // 256 is a multiple of `lanes`
  const bool live = s < a.n_states;
  const size_t base = (size_t)(live ? s : 0) * (size_t)a.trials;
  double rd = INFINITY, rd0 = INFINITY;
  uint64_t dist_kept = 0;
  uint32_t rate_kept = 0;
  int idx = 0x7fffffff, invalid = 0;
  if (live) {
    for (int i = sub; i < a.trials; i += a.lanes) {
      const unsigned long long r = (unsigned long long)a.rate[base + i] + (a.rate_add ? a.rate_add[base + i] : 0u);
      const uint64_t d = a.dist[base + i];
      const bool bad = r >= 0xFFFFFFFFull;
      invalid |= bad;
      // fi.lambda.mul_add(rate / 8, distortion): rate / 8 is exact, u64 -> f64 rounds to nearest even, one rounding
      const double c = bad ? (double)INFINITY : __builtin_fma(a.lambda, (double)(uint32_t)r * 0.125, (double)d);
      if (i == 0) rd0 = c;
      if (c < rd) rd = c, idx = i, dist_kept = d, rate_kept = (uint32_t)r;
    }
  }
  const double mine = rd;
  const int mine_idx = idx;
  for (int m = 1; m < a.lanes; m <<= 1) {
    const double o_rd = __shfl_xor(rd, m, WAVE);
    const int o_idx = __shfl_xor(idx, m, WAVE);
    invalid |= __shfl_xor(invalid, m, WAVE);
    first_min(rd, idx, o_rd, o_idx);
  }
  // the group's first lane holds trial 0
  rd0 = __shfl(rd0, (int)(threadIdx.x & 63u) & ~(a.lanes - 1), WAVE);
  if (!live) return;
  R1RdPick *st = a.state + s;
  const double best = st->best_rd;
  if (sub == 0 && a.invalid) a.invalid[s] = (uint8_t)invalid;
  // rdo.rs:1801: the loop over the types ends behind the first one when that is already above what is kept
  if (a.rule == R1_PICK_TX_TYPE && rd0 > best) return;
  // the lane that holds the winner has its rate and distortion: it writes the state (one lane: indices are unique)
  if (rd < best && idx == mine_idx && rd == mine) {
    R1RdPick w;
    w.best_rd = rd;
    w.best_dist = dist_kept;
    w.best_rate = rate_kept;
    w.best_row = (int16_t)(idx / a.nt);
    w.best_slot = (int8_t)(idx % a.nt);
    w.best_call = (int8_t)a.call_id;
    *st = w;
  }
}

extern "C" int r1_rd_pick_batch(r1_ctx *ctx, const uint32_t *rate, const uint32_t *rate_add, const uint64_t *dist,
                                int n_states, int group, int nt, double lambda, int rule, int call_id, R1RdPick *state,
                                uint8_t *invalid_out, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(rate && dist && state);
  R1_REQUIRE(n_states >= 0);
  R1_REQUIRE(group >= 1 && group <= 4096);
  R1_REQUIRE(nt >= 1 && nt <= 16);
  R1_REQUIRE(group * nt <= 4096);
  R1_REQUIRE(rule == R1_PICK_FIRST_MIN || rule == R1_PICK_TX_TYPE);
  R1_REQUIRE(rule != R1_PICK_TX_TYPE || group == 1);
  R1_REQUIRE(call_id >= 0 && call_id <= 127);
  R1_REQUIRE(lambda >= 0.0 && !isinf(lambda));   // NaN fails the first
  if (n_states == 0) return R1_OK;
  PickArgs a = {rate, rate_add, dist, state, invalid_out, lambda, n_states, group * nt, nt, rule, call_id, 1, 0};
  while (a.lanes < a.trials && a.lanes < WAVE) a.lanes <<= 1, a.lanes_log2++;
  const long long threads = (long long)n_states * a.lanes;
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_rd_pick, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// ---- the commit ----
struct CommitArgs {
  const R1RdPick *state;
  const uint16_t *eobs;
  const uint8_t *qc, *side, *rec_trials;
  const int16_t *pos_xy;
  uint16_t *eob_win;
  uint8_t *qc_win, *side_win;
  R1Plane rec;
  size_t win_stride_bytes;                // one state's row of qcoeffs_win (win_stride has no upper bound)
  int n_states, call_id, group, nt, ntx, order, side_bytes, bw, bh, store_w, store_h;
  unsigned txb_bytes;                     // one transform block's coefficients: at most 4096
};

// n bytes (n <= 16, a multiple of the pixel size) from the low end of (lo, hi) to dst, in the widest stores the
// address admits: the steps up to 16-byte alignment, then down again.  A step is taken only when the bytes are there,
// so nothing beyond dst + n is written; the shifts are by constants and the value stays in registers.
__device__ __forceinline__ void shr128(uint64_t &lo, uint64_t &hi, int bits) {   // 0 < bits < 64
  lo = (lo >> bits) | (hi << (64 - bits));
  hi >>= bits;
}
template <int BPP>
__device__ __forceinline__ void store_run(uint8_t *dst, uint64_t lo, uint64_t hi, int n) {
  if (n == 16 && ((uintptr_t)dst & 15) == 0) {
    *(uint4 *)dst = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    return;
  }
  if (BPP == 1 && n >= 1 && ((uintptr_t)dst & 1)) *dst = (uint8_t)lo, shr128(lo, hi, 8), dst += 1, n -= 1;
  if (n >= 2 && ((uintptr_t)dst & 2)) *(uint16_t *)dst = (uint16_t)lo, shr128(lo, hi, 16), dst += 2, n -= 2;
  if (n >= 4 && ((uintptr_t)dst & 4)) *(uint32_t *)dst = (uint32_t)lo, shr128(lo, hi, 32), dst += 4, n -= 4;
  if (n >= 8 && ((uintptr_t)dst & 8)) *(uint64_t *)dst = lo, lo = hi, hi = 0, dst += 8, n -= 8;
  if (n >= 8) *(uint64_t *)dst = lo, lo = hi, hi = 0, dst += 8, n -= 8;
  if (n >= 4) *(uint32_t *)dst = (uint32_t)lo, shr128(lo, hi, 32), dst += 4, n -= 4;
  if (n >= 2) *(uint16_t *)dst = (uint16_t)lo, shr128(lo, hi, 16), dst += 2, n -= 2;
  if (BPP == 1 && n >= 1) *dst = (uint8_t)lo;
}

// `bytes` from src to dst, both aligned to V, by the wave: lane l moves pieces l, l + 64, ...
template <class V>
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, unsigned bytes, int lane) {
  for (unsigned o = (unsigned)lane * sizeof(V); o < bytes; o += WAVE * sizeof(V)) *(V *)(dst + o) = *(const V *)(src + o);
}

// One wave per state, four states per workgroup.  A state the call did not win -- or whose row / slot in device
// memory lies outside the call's group x nt -- leaves through a wave-uniform branch before any other load, so the
// commits of several calls over one state array cost the losers 24 bytes each.  The winner's wave then moves three
// things, every loop bounded by an argument:
//   coefficients  ntx runs of txb_bytes, as 16-byte pieces (VEC: every address involved is a multiple of 16, which
//                 the host checks) or in the coefficient's own width
//   side          up to 128 bytes, bytewise (`side_bytes` has no alignment)
//   rec           the dense bw x bh block in 16-byte loads (the blocks are multiples of 16 bytes and the host checks
//                 the base), lane l taking pieces l, l + 64, ...; a piece is cut into runs that lie in one row (a row of
//                 the narrow blocks is 4 or 8 bytes), each run clipped to [0, store_w) x [0, store_h) and stored by
//                 store_run.  R1Plane promises element alignment only, so the width of a store follows the address.
// No atomics, no LDS, no scratch: the blocks of one call must not overlap (two waves would store to the same pixels in
// no defined order).
template <int BPP, bool VEC, class CT>
__global__ __launch_bounds__(256) void k_rd_commit(const CommitArgs a) {
  const int s = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  if (s >= a.n_states) return;
  const R1RdPick st = a.state[s];
  const int call = __builtin_amdgcn_readfirstlane((int)st.best_call);
  const int row = __builtin_amdgcn_readfirstlane((int)st.best_row);
  const int slot = __builtin_amdgcn_readfirstlane((int)st.best_slot);
  if (call != a.call_id || row < 0 || row >= a.group || slot < 0 || slot >= a.nt) return;
  const size_t t = ((size_t)s * (size_t)a.group + (size_t)row) * (size_t)a.nt + (size_t)slot;

  if (a.eobs) {
    // transform block k of the trial: order 0 behind the trial's others, order 1 (group == 1) behind block s's types
    const size_t first = a.order == 0 ? t * (size_t)a.ntx : (size_t)s * (size_t)a.ntx * (size_t)a.nt + (size_t)slot;
    const size_t step = a.order == 0 ? 1 : (size_t)a.nt;
    if (lane < a.ntx) a.eob_win[(size_t)s * 16 + lane] = a.eobs[first + (size_t)lane * step];
    uint8_t *dst = a.qc_win + (size_t)s * a.win_stride_bytes;
    for (int k = 0; k < a.ntx; k++) {
      const uint8_t *src = a.qc + (first + (size_t)k * step) * a.txb_bytes;
      if constexpr (VEC) wave_copy<uint4>(dst + (size_t)k * a.txb_bytes, src, a.txb_bytes, lane);
      else wave_copy<CT>(dst + (size_t)k * a.txb_bytes, src, a.txb_bytes, lane);
    }
  }

  if (a.side)
    for (int o = lane; o < a.side_bytes; o += WAVE)
      a.side_win[(size_t)s * (size_t)a.side_bytes + o] = a.side[t * (size_t)a.side_bytes + o];

  if (a.rec_trials) {
    const int px = a.pos_xy[2 * (size_t)s], py = a.pos_xy[2 * (size_t)s + 1];
    const int pieces = a.bw * a.bh * BPP / 16;                  // 1 .. 512
    const int run_px = a.bw < 16 / BPP ? a.bw : 16 / BPP;       // pixels of a piece that lie in one row
    const int runs = 16 / BPP / run_px;                         // 1, 2 or 4
    const uint8_t *src = a.rec_trials + t * (size_t)(a.bw * a.bh * BPP);
    for (int c = lane; c < pieces; c += WAVE) {
      const uint4 v = *(const uint4 *)(src + (size_t)c * 16);
      const uint64_t vlo = v.x | ((uint64_t)v.y << 32), vhi = v.z | ((uint64_t)v.w << 32);
      for (int r = 0; r < runs; r++) {
        const int p = c * (16 / BPP) + r * run_px;
        const int x = px + p % a.bw, y = py + p / a.bw;
        // the run's pixels [x0, x1) of [x, x + run_px) that lie in the store rectangle
        const int x0 = x < 0 ? 0 : x, x1 = x + run_px < a.store_w ? x + run_px : a.store_w;
        if (y < 0 || y >= a.store_h || x0 >= x1) continue;
        uint64_t lo = vlo, hi = vhi;
        const int skip = (r * run_px + (x0 - x)) * BPP * 8;     // bits in front of the first pixel stored: 0 .. 120
        if (skip >= 64) lo = hi >> (skip - 64), hi = 0;
        else if (skip > 0) shr128(lo, hi, skip);
        uint8_t *dst = (uint8_t *)a.rec.data +
                       ((size_t)(a.rec.yorigin + y) * (size_t)a.rec.stride + (size_t)(a.rec.xorigin + x0)) * BPP;
        store_run<BPP>(dst, lo, hi, (x1 - x0) * BPP);
      }
    }
  }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int r1_rd_commit_batch(r1_ctx *ctx, const R1RdPick *state, int n_states, int call_id, int group, int nt,
                                  int ntx, int order, int coded_area, int coeff_bytes, const uint16_t *eobs,
                                  const void *qcoeffs, const void *side, int side_bytes, const void *rec_trials, int bw,
                                  int bh, const R1Plane *rec, const int16_t *pos_xy, int store_w, int store_h,
                                  uint16_t *eob_win, void *qcoeffs_win, int win_stride, void *side_win, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(state);
  R1_REQUIRE(n_states >= 0);
  R1_REQUIRE(call_id >= 0 && call_id <= 127);
  R1_REQUIRE(group >= 1 && group <= 4096);
  R1_REQUIRE(nt >= 1 && nt <= 16);
  R1_REQUIRE(group * nt <= 4096);
  // each part is there whole or not at all
  const int n_tx = (eobs != nullptr) + (qcoeffs != nullptr) + (eob_win != nullptr) + (qcoeffs_win != nullptr);
  R1_REQUIRE(n_tx == 0 || n_tx == 4);
  R1_REQUIRE((side != nullptr) == (side_win != nullptr));
  const int n_rec = (rec_trials != nullptr) + (rec != nullptr) + (pos_xy != nullptr);
  R1_REQUIRE(n_rec == 0 || n_rec == 3);
  CommitArgs a = {};
  if (n_tx) {
    R1_REQUIRE(ntx >= 1 && ntx <= 16);
    R1_REQUIRE(order == 0 || order == 1);
    R1_REQUIRE(order == 0 || group == 1);
    R1_REQUIRE(coeff_bytes == 2 || coeff_bytes == 4);
    R1_REQUIRE(coded_area >= 16 && coded_area <= 1024);
    R1_REQUIRE(win_stride >= ntx * coded_area);
    a.txb_bytes = (unsigned)(coded_area * coeff_bytes);
    a.win_stride_bytes = (size_t)win_stride * (size_t)coeff_bytes;
    // the arrays are arrays of coefficients: the piecewise copy moves whole elements
    R1_REQUIRE(((uintptr_t)qcoeffs | (uintptr_t)qcoeffs_win) % (uintptr_t)coeff_bytes == 0);
  }
  if (side) R1_REQUIRE(side_bytes >= 1 && side_bytes <= 128);
  int bpp = 1;
  if (n_rec) {
    R1_REQUIRE(r1_block_size_ok(bw, bh));
    R1_REQUIRE(r1_px_ok(*rec) && r1_depth_ok(rec->bit_depth) && r1_px_fits_depth(*rec));
    R1_REQUIRE(rec->data && rec->stride > 0 && rec->alloc_height > 0 && rec->xorigin >= 0 && rec->yorigin >= 0);
    // the store rectangle: the visible plane and its padding to the right and below, as far as the allocation goes
    R1_REQUIRE(store_w >= 0 && store_w <= rec->stride - rec->xorigin);
    R1_REQUIRE(store_h >= 0 && store_h <= rec->alloc_height - rec->yorigin);
    R1_REQUIRE(aligned16(rec_trials));                   // the dense blocks are read in 16-byte pieces
    bpp = rec->bytes_per_px;
    a.rec = *rec;
  }
  if (n_states == 0 || n_tx + (side != nullptr) + n_rec == 0) return R1_OK;
  a.state = state, a.eobs = eobs, a.qc = (const uint8_t *)qcoeffs, a.side = (const uint8_t *)side;
  a.rec_trials = (const uint8_t *)rec_trials, a.pos_xy = pos_xy;
  a.eob_win = eob_win, a.qc_win = (uint8_t *)qcoeffs_win, a.side_win = (uint8_t *)side_win;
  a.n_states = n_states, a.call_id = call_id, a.group = group, a.nt = nt, a.ntx = ntx, a.order = order;
  a.side_bytes = side_bytes, a.bw = bw, a.bh = bh, a.store_w = store_w, a.store_h = store_h;
  const bool vec = n_tx && aligned16(qcoeffs) && aligned16(qcoeffs_win) && a.txb_bytes % 16 == 0 && a.win_stride_bytes % 16 == 0;
  const dim3 grid((unsigned)(((long long)n_states + 3) / 4));
  R1DeviceGuard guard(ctx);
  r1_by_bpp(bpp, [&](auto B) {
    r1_by_bool(vec, [&](auto V) {
      r1_by_value<4, 2>(n_tx ? coeff_bytes : 4, [&](auto CB) {
        using CT = std::conditional_t<CB.value == 2, uint16_t, uint32_t>;
        // the piecewise form needs one instantiation per coefficient width, the 16-byte form one in all
        if constexpr (V.value && CB.value == 2) hipLaunchKernelGGL((k_rd_commit<B.value, true, uint32_t>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((k_rd_commit<B.value, V.value, CT>), grid, dim3(256), 0, (hipStream_t)stream, a);
      });
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// mc_compound.hip -- the two-reference (compound) inter candidate in one launch:
//   t0 = prep_8tap(ref0), t1 = prep_8tap(ref1), pred = mc_avg(t0, t1), SAD / SATD of pred against the source
// (reference: predict_inter_compound src/predict.rs:339-382; prep_8tap / mc_avg src/mc.rs:360-479; get_sad /
// get_satd src/dist.rs:31-221; the compound leg of the inter mode pre-screen src/rdo.rs:1238-1271, 1328-1352).
// The int16 intermediates live in registers (fast path) or LDS (general path) and never reach HBM; the
// prediction reaches HBM only through pred_out.  Every sum is an integer sum, so the results do not depend on the
// order the lanes add in, and every output word has exactly one writer: no atomics, no zeroed buffers.
//
// Two mappings, chosen by block size alone.  Why each was chosen rests on the LDS bytes and registers a wave needs,
// counted from the layouts below; NOTHING here was measured when this was written (tools/bench_compound.py is the
// tool that does).
//
//  * k_compound_fast -- blocks whose size is a transform size (W, H <= 64, powers of two), k_mc_fast's mapping:
//    compile-time W x H, P = max(W, H) lanes per candidate, 64 / P candidates per wave, one wave per workgroup.
//    Both (H + 7) x (W + 7) windows of a candidate sit side by side in LDS, staged with ONE global round trip
//    (all loads of both windows go out before the first LDS write).  Lane = column: the two prep columns
//    (mc_column_fast of cand_common.hpp, PREP) are 2 * H registers, averaged in place; the residual column goes through
//    satd_column's DPP Hadamard and group_sum.
//    LDS bytes per wave = 2 * (H + 7) * row stride * candidates per wave: 64x64 at 16 bits is 2 * 71 * 144 =
//    20448 B -> 8 workgroups in a CU's 160 KiB = 2 waves per SIMD; 64x64 at 8 bits 10224 B -> 4 per SIMD; 32x32
//    and below need at most 12480 B (8 per SIMD by LDS).  The 64-row instantiations hold 2 * 64 column registers
//    plus the filter state -- the compiler reports 165 VGPRs, 3 waves per SIMD by the register table -- so only the
//    16-bit 64x64 launch is held lower by its LDS image than by its registers (2 against 3).
//    Workgroups take the candidate list in XCD-contiguous eighths (grid = multiple of 8): the candidates of one
//    block are neighbours in the list and share the source block and most of both windows.
//
//  * k_compound -- everything else (128-wide / -high blocks, heights that are not a power of two), k_mc's slab
//    scheme at run-time sizes: a slab is P = min(w, 64) columns by hc = h (h <= 64) or h / 2 rows, a wave owns
//    64 / P candidates and walks the slabs of its candidates one after the other, so a block's SAD / SATD
//    partials over its slabs are summed in the lanes that produced them, inside the workgroup.  Per slab both
//    windows are staged, the first prep column is parked as int16 in an LDS tile (hc x P, each lane reads back
//    only what it wrote), the second column's emit averages, stores, and leaves the residual in the same tile for
//    the Hadamard.  LDS per wave = (64 / P) * (2 * (hc + 7) * row stride + hc * P * 2): 28640 B for a 128x128
//    16-bit block -> 5 waves per CU, at most 62720 B (4-wide, 16 bits, 64 rows).  This path trades occupancy
//    for having no per-size code; the sizes the encoder sends most are on the fast path.
#include "cand_common.hpp"
#include "tx_common.hpp"

namespace {

static_assert(sizeof(R1CompoundCand) == 20, "R1CompoundCand is 20 bytes");

__device__ __forceinline__ R1CompoundCand load_cand(const R1CompoundCand *p) {
  // a 16-byte and a 4-byte load (left to the compiler the 2-byte aligned struct comes in ten pieces)
  struct { U32x4 a; U32x1 b; } raw = {ld_u32x4((const uint8_t *)p), {ld_u32((const uint8_t *)p + 16)}};
  R1CompoundCand cd;
  __builtin_memcpy(&cd, &raw, sizeof(cd));
  return cd;
}

// get_satd's final normalisation (dist.rs:214-220): the sum of |coefficients| over ln2 = log2(Hadamard size)
__device__ __forceinline__ uint32_t satd_norm(uint32_t s, int ln) { return (s + ((1u << ln) >> 1)) >> ln; }

template <int BD, int WL, int HL>
__global__ __launch_bounds__(64) void k_compound_fast(R1Plane org, R1Plane ref0, R1Plane ref1,
                                                      const R1CompoundCand *__restrict__ cands, int n,
                                                      uint32_t *__restrict__ sad_out,
                                                      uint32_t *__restrict__ satd_out,
                                                      void *__restrict__ pred_out) {
  constexpr int BPP = BD == 8 ? 1 : 2;
  constexpr int W = 1 << WL, H = 1 << HL;
  constexpr int P = W > H ? W : H, NC = 64 / P;
  constexpr int TS = (W < H ? W : H) == 4 ? 4 : 8;   // the reference's Hadamard size rule (dist.rs:166)
  constexpr int WS = r1mc::window_stride(W, BPP);
  constexpr int WIN = (H + 7) * WS;
  constexpr uint32_t XORM = BPP == 1 ? 0x80808080u : 0u;   // mc8_column_t wants pixels biased to i8
  __shared__ __attribute__((aligned(16))) uint8_t smem[NC * 2 * WIN];
  const unsigned wg = xcd_contiguous_wg();
  if ((long long)wg * NC >= (long long)n) return;   // the whole wave: no lane of it has a candidate
  const int lane = threadIdx.x;
  const int cl = lane / P, c = lane % P;
  const long long cand = (long long)wg * NC + cl;
  const bool live = cand < n;
  R1CompoundCand cd = {};
  if (live) cd = load_cand(cands + cand);
  uint8_t *win0 = smem + cl * 2 * WIN, *win1 = win0 + WIN;
  if (live) {
    r1mc::WindowStage<BPP, XORM, W, H, P> st0, st1;
    st0.load(ref0, cd.rx0, cd.ry0, c);
    st1.load(ref1, cd.rx1, cd.ry1, c);
    st0.store(win0, WS);
    st1.store(win1, WS);
  }
  __syncthreads();
  // No lane leaves before the reductions: the DPP / shuffle steps below want the whole wave.  Lanes without a
  // column (c >= W of a tall block, candidates past the list end) carry a zero residual.
  const bool col_live = live && c < W;
  const bool dist = sad_out || satd_out;   // wave-uniform: kernel arguments
  int32_t v[H];
#pragma unroll
  for (int r = 0; r < H; r++) v[r] = 0;
  if (col_live) {
    int32_t t0[H], t1[H];
    const r1cand::Taps<BPP> tp0 = r1cand::load_taps<BPP, W, H>(cd.col_frac0, cd.row_frac0, cd.mode_x, cd.mode_y);
    r1cand::mc_column_fast<BPP, W, H, WS, true>(win0, c, tp0, BD, t0, r1cand::taps_six(tp0));
    const r1cand::Taps<BPP> tp1 = r1cand::load_taps<BPP, W, H>(cd.col_frac1, cd.row_frac1, cd.mode_x, cd.mode_y);
    r1cand::mc_column_fast<BPP, W, H, WS, true>(win1, c, tp1, BD, t1, r1cand::taps_six(tp1));
#pragma unroll
    for (int r = 0; r < H; r++) t0[r] = r1mc::avg_px(t0[r], t1[r], BD);
    if (pred_out) {
      if constexpr (BPP == 1) {
        uint8_t *pp = (uint8_t *)pred_out + (size_t)cand * W * H + c;
#pragma unroll
        for (int r = 0; r < H; r++) pp[(size_t)r * W] = (uint8_t)t0[r];
      } else {
        uint16_t *pp = (uint16_t *)pred_out + (size_t)cand * W * H + c;
#pragma unroll
        for (int r = 0; r < H; r++) pp[(size_t)r * W] = (uint16_t)t0[r];
      }
    }
    if (dist) {
      const uint8_t *po = px_addr<BPP>(org, cd.ox + c, cd.oy);
      const size_t so = (size_t)org.stride * BPP;
#pragma unroll
      for (int r = 0; r < H; r++) v[r] = ld_px<BPP>(po + r * so) - t0[r];
    }
  }
  if (sad_out) {
    uint32_t sad = 0;
#pragma unroll
    for (int r = 0; r < H; r++) sad += (uint32_t)iabs32(v[r]);
    const uint32_t s = group_sum<P>(sad);
    if (live && c == 0) sad_out[cand] = s;
  }
  if (satd_out) {
    const uint32_t s = group_sum<P>(r1cand::satd_column<TS, H, BD>(v, lane));
    if (live && c == 0) satd_out[cand] = satd_norm(s, TS == 4 ? 2 : 3);
  }
}

template <int BPP>
__global__ __launch_bounds__(64) void k_compound(R1Plane org, R1Plane ref0, R1Plane ref1, int w, int h,
                                                 const R1CompoundCand *__restrict__ cands, int n,
                                                 uint32_t *__restrict__ sad_out,
                                                 uint32_t *__restrict__ satd_out,
                                                 void *__restrict__ pred_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int P = w < 64 ? w : 64;        // columns per slab
  const int spc = w / P;                // column slabs per candidate: 1 or 2
  const int hc = h <= 64 ? h : h >> 1;  // rows per slab; h > 64 splits in two halves (both > 4 rows: same filters)
  const int nrc = h / hc;               // 1 or 2
  const int ws = r1mc::window_stride(P, BPP);
  const int winb = (hc + 7) * ws;
  const int per = 2 * winb + hc * P * 2;   // LDS bytes of one candidate's slab: two windows + the int16 tile
  const int lane = threadIdx.x;
  const int sl = lane / P, c = lane - sl * P;
  const long long cand = (long long)blockIdx.x * (64 / P) + sl;
  const bool live = cand < n;
  uint8_t *win0 = smem + (size_t)sl * per, *win1 = win0 + winb;
  int16_t *tile = (int16_t *)(win1 + winb) + c;   // this lane's column: row r at tile[r * P]
  R1CompoundCand cd = {};
  if (live) cd = load_cand(cands + cand);
  const int bd = org.bit_depth;
  const bool dist = sad_out || satd_out;          // wave-uniform: kernel arguments
  const int ts = (w < h ? w : h) == 4 ? 4 : 8;    // Hadamard size (dist.rs:166); read when satd_out only
  const size_t so = (size_t)org.stride * BPP;
  uint32_t sad = 0, satd = 0;
  for (int s = 0; s < spc * nrc; s++) {           // the same trip count for every lane
    const int sy = s / spc;
    const int x0 = (s - sy * spc) * P, y0 = sy * hc;
    if (s) __syncthreads();                       // the previous slab's windows are dead
    if (live) {
      r1mc::stage_window<BPP>(win0, ws, ref0, cd.rx0 + x0, cd.ry0 + y0, P, hc, c, P);
      r1mc::stage_window<BPP>(win1, ws, ref1, cd.rx1 + x0, cd.ry1 + y0, P, hc, c, P);
    }
    __syncthreads();
    if (live) {
      r1mc::mc_column<BPP, true, 0>(win0, ws, c, w, hc, cd.col_frac0, cd.row_frac0, cd.mode_x, cd.mode_y, bd,
                                    [&](int r, int32_t t) { tile[r * P] = (int16_t)t; });
      const uint8_t *po = px_addr<BPP>(org, cd.ox + x0 + c, cd.oy + y0);
      const size_t pbase = ((size_t)cand * h + y0) * w + x0 + c;
      r1mc::mc_column<BPP, true, 0>(win1, ws, c, w, hc, cd.col_frac1, cd.row_frac1, cd.mode_x, cd.mode_y, bd,
                                    [&](int r, int32_t t) {
        const int32_t p = r1mc::avg_px((int32_t)tile[r * P], t, bd);
        if (pred_out) {
          if constexpr (BPP == 1) ((uint8_t *)pred_out)[pbase + (size_t)r * w] = (uint8_t)p;
          else ((uint16_t *)pred_out)[pbase + (size_t)r * w] = (uint16_t)p;
        }
        if (dist) {
          const int32_t d = ld_px<BPP>(po + r * so) - p;
          sad += (uint32_t)iabs32(d);
          tile[r * P] = (int16_t)d;   // |d| < 2^12: the residual column, for the Hadamard below
        }
      });
    }
    if (satd_out) {
      // every lane takes part (DPP across the lanes of a tile); a lane without a candidate adds zeros
      for (int g = 0; g < hc / ts; g++) {
        int32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = live && k < ts ? (int32_t)tile[(g * ts + k) * P] : 0;
        satd += ts == 4 ? r1cand::satd_column<4, 4, 12>(v, lane) : r1cand::satd_column<8, 8, 12>(v, lane);
      }
    }
  }
  for (int m = 1; m < P; m <<= 1) {   // the P lanes of a candidate are consecutive
    sad += __shfl_xor(sad, m, WAVE);
    satd += __shfl_xor(satd, m, WAVE);
  }
  if (live && c == 0) {
    if (sad_out) sad_out[cand] = sad;
    if (satd_out) satd_out[cand] = satd_norm(satd, ts == 4 ? 2 : 3);
  }
}

template <int BD, int WL, int HL>
int launch_fast(const R1Plane &org, const R1Plane &ref0, const R1Plane &ref1, const R1CompoundCand *cands, int n,
                uint32_t *sad_out, uint32_t *satd_out, void *pred_out, hipStream_t st) {
  constexpr int W = 1 << WL, H = 1 << HL, P = W > H ? W : H, NC = 64 / P;
  const unsigned grid = xcd_grid((unsigned)((n + NC - 1) / NC));
  hipLaunchKernelGGL((k_compound_fast<BD, WL, HL>), dim3(grid), dim3(64), 0, st, org, ref0, ref1, cands, n,
                     sad_out, satd_out, pred_out);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// the 22 BlockSizes (src/partition.rs:130-153): powers of two 4 .. 128, aspect ratio up to 4, 128 only beside 64 / 128
bool is_block_size(int w, int h) {
  if (!r1_is_pow2(w) || !r1_is_pow2(h) || w < 4 || h < 4 || w > 128 || h > 128) return false;
  const int lo = w < h ? w : h, hi = w < h ? h : w;
  return hi <= 4 * lo && (hi < 128 || lo >= 64);
}

}  // namespace

extern "C" int r1_rdo_compound_cand_batch(r1_ctx *ctx, const R1Plane *org, const R1Plane *ref0,
                                          const R1Plane *ref1, int w, int h, const R1CompoundCand *cands, int n,
                                          uint32_t *sad_out, uint32_t *satd_out, void *pred_out, void *stream) {
  R1_REQUIRE(ctx && org && ref0 && ref1);
  const int bd = org->bit_depth, bpp = org->bytes_per_px;
  R1_REQUIRE(r1_depth_ok(bd));
  R1_REQUIRE(r1_px_ok(*org) && r1_px_fits_depth(*org));
  R1_REQUIRE(r1_same_depth(*org, *ref0, *ref1));
  R1_REQUIRE(r1_same_px(*org, *ref0, *ref1));
  R1_REQUIRE(r1_is_pow2(w) && w >= 4 && w <= 128);
  R1_REQUIRE(h >= 2 && h <= 128 && (h & 1) == 0);
  R1_REQUIRE(sad_out || satd_out || pred_out);
  if (sad_out || satd_out) R1_REQUIRE(is_block_size(w, h));
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands);
  hipStream_t st = (hipStream_t)stream;
  // transform sizes: the compile-time mapping
  int ts = -1;
  for (int t = 0; t < 19; t++)
    if ((1 << r1tx::kTxWLog2[t]) == w && (1 << r1tx::kTxHLog2[t]) == h) ts = t;
#define R1_CF_CASE(ID, WL, HL)                                                                                    \
  case ID:                                                                                                        \
    return bd == 8    ? launch_fast<8, WL, HL>(*org, *ref0, *ref1, cands, n, sad_out, satd_out, pred_out, st)     \
           : bd == 10 ? launch_fast<10, WL, HL>(*org, *ref0, *ref1, cands, n, sad_out, satd_out, pred_out, st)    \
                      : launch_fast<12, WL, HL>(*org, *ref0, *ref1, cands, n, sad_out, satd_out, pred_out, st);
  switch (ts) { R1_TX_SIZES(R1_CF_CASE) }
#undef R1_CF_CASE
  // the slab kernel for the rest
  const int P = w < 64 ? w : 64, NS = 64 / P, hc = h <= 64 ? h : h >> 1;
  const int ws = r1mc::window_stride(P, bpp);
  const size_t lds = (size_t)NS * (2 * (size_t)(hc + 7) * ws + (size_t)hc * P * 2);   // <= 62720
  const unsigned grid = (unsigned)((n + NS - 1) / NS);
  r1_by_bpp(bpp, [&](auto B) {
    hipLaunchKernelGGL((k_compound<B.value>), dim3(grid), dim3(64), lds, st, *org, *ref0, *ref1, w, h, cands, n,
                       sad_out, satd_out, pred_out);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

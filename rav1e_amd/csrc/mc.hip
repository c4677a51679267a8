// mc.hip -- batched motion compensation: put_8tap / prep_8tap / mc_avg
// (reference: src/mc.rs:250-479; dispatch tables src/asm/x86/mc.rs:17-78).
//
// Mapping: a block is cut into slabs of P = min(w, 64) columns; one wave
// (workgroup of 64) owns 64 / P slabs.  The wave first stages each slab's
// (h+7) x (P+7) reference window into LDS with unaligned dword loads, then
// lane = (slab, column) runs the separable filter down its column with an
// 8-deep register window (one new LDS row per output row for the vertical
// taps).  Output blocks are dense (stride = w), so a row's P lanes store P
// consecutive samples.
#include "cand_common.hpp"
#include "tx_common.hpp"

namespace {

template <int BPP, bool PREP>
__global__ __launch_bounds__(64) void k_mc(R1Plane ref, int w, int h,
                                           const R1McCand *__restrict__ cands,
                                           int n, void *__restrict__ dst_) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int P = w < 64 ? w : 64;
  const int spc = w / P;      // slabs per candidate
  const int NS = 64 / P;      // slabs per wave
  const int ws = r1mc::window_stride(P, BPP);
  const int lane = threadIdx.x;
  const int sl = lane / P, c = lane - sl * P;
  const long long slab = (long long)blockIdx.x * NS + sl;
  const long long cand = slab / spc;
  const int x0 = (int)(slab - cand * spc) * P;
  const bool live = cand < n;
  uint8_t *win = smem + (size_t)sl * (h + 7) * ws;
  R1McCand cd = {};
  if (live) {
    cd = cands[cand];
    r1mc::stage_window<BPP>(win, ws, ref, cd.rx + x0, cd.ry, P, h, c, P);
  }
  __syncthreads();
  if (!live) return;
  const size_t base = (size_t)cand * w * h + x0 + c;
  if constexpr (PREP) {
    int16_t *dst = (int16_t *)dst_ + base;
    r1mc::mc_column<BPP, true, 0>(win, ws, c, w, h, cd.col_frac, cd.row_frac,
                               cd.mode_x, cd.mode_y, ref.bit_depth,
                               [&](int r, int32_t v) { dst[(size_t)r * w] = (int16_t)v; });
  } else if constexpr (BPP == 1) {
    uint8_t *dst = (uint8_t *)dst_ + base;
    r1mc::mc_column<BPP, false, 0>(win, ws, c, w, h, cd.col_frac, cd.row_frac,
                                cd.mode_x, cd.mode_y, ref.bit_depth,
                                [&](int r, int32_t v) { dst[(size_t)r * w] = (uint8_t)v; });
  } else {
    uint16_t *dst = (uint16_t *)dst_ + base;
    r1mc::mc_column<BPP, false, 0>(win, ws, c, w, h, cd.col_frac, cd.row_frac,
                                cd.mode_x, cd.mode_y, ref.bit_depth,
                                [&](int r, int32_t v) { dst[(size_t)r * w] = (uint16_t)v; });
  }
}

template <int BPP>
__global__ __launch_bounds__(256) void k_avg(const int16_t *__restrict__ t1,
                                             const int16_t *__restrict__ t2,
                                             long long total, int bit_depth,
                                             void *__restrict__ dst_) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long long)gridDim.x * 256) {
    const int32_t v = r1mc::avg_px((int32_t)t1[i], (int32_t)t2[i], bit_depth);
    if constexpr (BPP == 1) ((uint8_t *)dst_)[i] = (uint8_t)v;
    else ((uint16_t *)dst_)[i] = (uint16_t)v;
  }
}

// put_8tap / prep_8tap alone on the same machinery (blocks whose size is a
// transform size): window staged with one round trip, dot4 / dot2 columns.
template <int BPP, int WL, int HL, bool PREP>
__global__ __launch_bounds__(64) void k_mc_fast(R1Plane ref, const R1McCand *__restrict__ cands,
                                                int n, void *__restrict__ dst) {
  constexpr int W = 1 << WL, H = 1 << HL;
  constexpr int P = W > H ? W : H, NC = 64 / P;
  constexpr int WS = r1mc::window_stride(W, BPP);
  __shared__ __attribute__((aligned(16))) uint8_t smem[NC * (H + 7) * WS];
  const int lane = threadIdx.x;
  const int cl = lane / P, c = lane % P;
  const unsigned wg = xcd_contiguous_wg();
  const long long cand = (long long)wg * NC + cl;
  const bool live = cand < n;
  R1McCand cd = {};
  if (live) cd = cands[cand];
  uint8_t *win = smem + cl * (H + 7) * WS;
  if (live)
    r1mc::stage_window_fast<BPP, BPP == 1 ? 0x80808080u : 0u, W, H, P>(win, WS, ref, cd.rx, cd.ry, c);
  __syncthreads();
  if (!(live && c < W)) return;
  int32_t pred[H];
  const r1cand::Taps<BPP> tp = r1cand::load_taps<BPP, W, H>(cd.col_frac, cd.row_frac, cd.mode_x, cd.mode_y);
  r1cand::mc_column_fast<BPP, W, H, WS, PREP>(win, c, tp, ref.bit_depth, pred, r1cand::taps_six(tp));
  // the predictions stream out (non-temporal: they would only push the reference rows out of the L2)
  if constexpr (PREP || BPP == 2) {
    uint16_t *pp = (uint16_t *)dst + (size_t)cand * W * H + c;
#pragma unroll
    for (int r = 0; r < H; r++) __builtin_nontemporal_store((uint16_t)pred[r], &pp[(size_t)r * W]);
  } else {
    uint8_t *pp = (uint8_t *)dst + (size_t)cand * W * H + c;
#pragma unroll
    for (int r = 0; r < H; r++) __builtin_nontemporal_store((uint8_t)pred[r], &pp[(size_t)r * W]);
  }
}

template <int BPP, int WL, int HL>
int launch_mc_fast(bool prep, const R1Plane &ref, const R1McCand *cands, int n, void *dst,
                   hipStream_t st) {
  constexpr int W = 1 << WL, H = 1 << HL, P = W > H ? W : H, NC = 64 / P;
  const unsigned grid = xcd_grid((unsigned)((n + NC - 1) / NC));
  r1_by_bool(prep, [&](auto PREP) {
    hipLaunchKernelGGL((k_mc_fast<BPP, WL, HL, PREP.value>), dim3(grid), dim3(64), 0, st, ref, cands, n, dst);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// The put / prep of block sizes that are transform sizes; returns 1 when (w, h) is not one of them.
int r1_mc_fast_launch(bool prep, const R1Plane *ref, int w, int h, const R1McCand *cands, int n,
                      void *dst, hipStream_t st) {
  int ts = -1;
  for (int t = 0; t < 19; t++)
    if ((1 << r1tx::kTxWLog2[t]) == w && (1 << r1tx::kTxHLog2[t]) == h) ts = t;
  if (ts < 0) return 1;
#define R1_MF_CASE(ID, WL, HL)                                                                             \
  case ID:                                                                                                 \
    return r1_by_bpp(ref->bytes_per_px, [&](auto B) {                                                      \
      return launch_mc_fast<B.value, WL, HL>(prep, *ref, cands, n, dst, st);                               \
    });
  switch (ts) { R1_TX_SIZES(R1_MF_CASE) }
#undef R1_MF_CASE
  return 1;
}

int mc_launch(bool prep, const R1Plane *ref, int w, int h, const R1McCand *cands,
              int n, void *dst, hipStream_t st) {
  R1_REQUIRE(ref && r1_px_ok(*ref));
  R1_REQUIRE(r1_is_pow2(w) && w >= 2 && w <= 128);
  R1_REQUIRE(h >= 2 && h <= 128 && (h & 1) == 0);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(cands && dst);
  // block sizes that are transform sizes take the dot4 / dot2 path of the
  // fused kernel (k_mc_fast above); the slab kernel below covers the rest
  // (w = 2, 128-wide / -high blocks, odd aspect ratios)
  {
    const int rc = r1_mc_fast_launch(prep, ref, w, h, cands, n, dst, st);
    if (rc <= 0) return rc;
  }
  const int bpp = ref->bytes_per_px;
  const int P = w < 64 ? w : 64, NS = 64 / P, spc = w / P;
  const int ws = r1mc::window_stride(P, bpp);
  const size_t lds = (size_t)NS * (h + 7) * ws;
  const long long slabs = (long long)n * spc;
  const unsigned grid = (unsigned)((slabs + NS - 1) / NS);
  r1_by_bpp(bpp, [&](auto B) {
    r1_by_bool(prep, [&](auto PREP) {
      hipLaunchKernelGGL((k_mc<B.value, PREP.value>), dim3(grid), dim3(64), lds, st, *ref, w, h, cands, n, dst);
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

}  // namespace

extern "C" int r1_mc_put_batch(r1_ctx *ctx, const R1Plane *ref, int w, int h,
                               const R1McCand *cands, int n, void *dst,
                               void *stream) {
  R1_REQUIRE(ctx);
  return mc_launch(false, ref, w, h, cands, n, dst, (hipStream_t)stream);
}

extern "C" int r1_mc_prep_batch(r1_ctx *ctx, const R1Plane *ref, int w, int h,
                                const R1McCand *cands, int n, int16_t *tmp,
                                void *stream) {
  R1_REQUIRE(ctx);
  return mc_launch(true, ref, w, h, cands, n, tmp, (hipStream_t)stream);
}

extern "C" int r1_mc_avg_batch(r1_ctx *ctx, const int16_t *tmp1,
                               const int16_t *tmp2, int w, int h, int n,
                               int bit_depth, int bytes_per_px, void *dst,
                               void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(r1_px_ok(bytes_per_px));
  R1_REQUIRE(r1_depth_ok(bit_depth));
  R1_REQUIRE(w > 0 && h > 0);
  if (n <= 0) return R1_OK;
  R1_REQUIRE(tmp1 && tmp2 && dst);
  const long long total = (long long)n * w * h;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  r1_by_bpp(bytes_per_px, [&](auto B) {
    hipLaunchKernelGGL((k_avg<B.value>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tmp1, tmp2,
                       total, bit_depth, dst);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// rdo_cand_kernel.hpp -- the fused RDO candidate kernel: for every candidate
//   pred  = put_8tap(ref)            (src/mc.rs:250-353)
//   sad   = get_sad(org, pred)       (src/dist.rs:31-52)
//   satd  = get_satd(org, pred)      (src/dist.rs:156-221)
//   resid = org - pred               (diff, src/encoder.rs:1355-1381)
//   coeff = forward_transform(resid) (src/transform/forward.rs:71-161)
// in ONE launch; the prediction and the residual never leave the CU.
// This is the reference's per-candidate call chain
// (predict_inter_single src/predict.rs:304-331 -> compute_mv_rd
// src/me.rs:1445-1454 / rdo.rs:1328-1352 -> encode_tx_block
// src/encoder.rs:1533-1552) restructured as a batch.
//
// Mapping (wave = 64, one wave per workgroup): a wave owns NC = 64 / max(W,H)
// candidates.
//  A  every lane pulls its source column into registers (H loads in flight)
//     while the wave stages each candidate's (H+7)x(W+7) reference window in
//     LDS (batched unaligned dword loads).
//  B  lane = (candidate, column) filters its column.  8-bit pixels: three
//     aligned LDS dwords per window row, v_alignbyte to the lane's byte
//     phase, pixels biased by -128 so that the horizontal 8 taps are two
//     v_dot4_i32_i8; the i16 intermediates are packed in pairs and the
//     vertical 8 taps are 4 (even rows) or 5 (odd rows) v_dot2_i32_i16.
//     All four (col_frac==0?, row_frac==0?) cases of mc.rs:264-352 go through
//     this one code path: a 128-valued tap at phase 0 reproduces the copy and
//     1-D paths bit for bit (see the derivation at mc8_column_t, cand_common.hpp).
//     8-bit 64x64 and 32x32 coefficient kernels (MC_MATRIX, rdo_cand_plan.hpp): the
//     horizontal taps are one v_mfma_i32_16x16x32_i8 per candidate and quad of
//     window rows instead -- window bytes as A, the taps as a band in B, every
//     lane receives the accumulators of its own column.  8-bit 16x16 and 8x8
//     coefficient kernels (MC_MATRIX4), four and eight candidates per wave: three
//     chained v_mfma_i32_4x4x4_16b_i8 per quad -- sixteen independent blocks of four
//     adjacent columns of one candidate, three dwords of the lane's own window as A,
//     its candidate's shifted taps as B, the same accumulators out.
//     The residual COLUMN stays in registers.  SAD is a lane sum.  SATD: the
//     vertical Hadamard on 8 registers, the horizontal one across the 8
//     neighbouring lanes with DPP (quad_perm / row_half_mirror) -- no LDS; blocks
//     with both sides >= 16 (up to 10 bits) turn the packed intermediates through
//     an LDS tile over the dead window instead and finish in registers (SATD_T).
//  C  column transform on the same registers (24-bit multiplies, exact here),
//     transpose through LDS (odd stride, aliasing the dead window).
//  D  lane = (candidate, row): row transform, stores in the reference's
//     transposed 32x32-chunk coefficient order.
// With the intra prediction source (PS = 1) phases A / B read
//   pred  = predict_intra(edges)     (src/predict.rs:205-249, 705-1505; encode_tx_block, src/encoder.rs:1458-1503)
// instead: the candidate's edge set goes to LDS in place of the window, the P lanes of a candidate filter /
// upsample it together, lane = (candidate, column) walks its column into the same registers (intra_pred_common.hpp).
#pragma once
#include <cstdlib>
#include <type_traits>

#include "cand_common.hpp"
#include "dist_common.hpp"
#include "intra_pred_common.hpp"
#include "itx_common.hpp"
#include "mc_common.hpp"
#include "quant_common.hpp"
#include "rdo_cand_args.hpp"
#include "tx_common.hpp"

#ifdef R1_PHASE_PROF
// experiment build only (make prof): wall-clock cycles a wave spends in each phase of the
// headline kernel, summed over all waves; read back by r1_debug_phase_prof_b<BD>() (rdo_cand_slice.hip).
// every 64th workgroup writes its own row: no atomics, so the probes do not queue up
static __device__ unsigned long long g_phase[4096][8];   // one per profiled slice
#define R1_PROF(i)                                                          \
  do {                                                                      \
    const unsigned long long t_ = __builtin_readcyclecounter();             \
    if (QM == 0 && threadIdx.x == 0 && (blockIdx.x & 63) == 0 && (blockIdx.x >> 6) < 4096) \
      g_phase[blockIdx.x >> 6][i] = t_ - tprev_;                            \
    tprev_ = t_;                                                            \
  } while (0)
#define R1_PROF_INIT unsigned long long tprev_ = __builtin_readcyclecounter()
#else
#define R1_PROF(i) do {} while (0)
#define R1_PROF_INIT do {} while (0)
#endif

// (Round 3 tried a software pipeline over two candidate groups per wave -- next group's loads in
// flight under this group's arithmetic.  Measured, profiles/r03_ab_notes.md ab3: -2.3 % on the 8-bit
// 8x8 launch, a LOSS everywhere else (the launches are VALU-issue bound; the registers of the loads
// in flight cost more occupancy than the hidden round trip is worth), and the machine scheduler did
// not terminate on the QM = 2 instantiations of that loop.  Not kept.)
//
// Translation units.  k_rdo_cand has 19 sizes x 3 bit depths x 3 QM variants = 171 instantiations, plus the
// type search's (MT) 9 sizes x 3 bit depths x 2 QM variants = 54; compiled in one piece they take many minutes
// of one core.  So this header is compiled fifteen times, in parallel, by rdo_cand_slice.hip: one (bit depth,
// slice) pair each (-DR1_RDO_TU_BD=8|10|12 -DR1_RDO_TU_QM=0..4, slices 3 / 4 = MT of QM 1 / 2), the kernel and one
// r1_rdo_slice_b*_q* launcher per object.  The sixteenth unit, rdo_cand.hip (argument checks, dispatch over the
// slices, the C entry points), shares rdo_cand_args.hpp with them and does not see this header.
// The intra prediction source (PS = 1, r1_rdo_intra_cand_batch) adds 105 instantiations -- the fan-out form of the nine
// sizes up to 16x16, the plain form of QM 1 / 2 for the ten sizes with a 32- or 64-point side, three bit depths, less
// the points that take two launches -- in twelve more objects of the same unit (-DR1_RDO_TU_INTRA, slices 1..4:
// r1_rdo_islice_b*_q*).  Which instantiations exist, and the compile-time plan of each (geometry, LDS layout, waves
// asked for), is stated once in rdo_cand_plan.hpp.
// Experiment builds swap slice objects of the shipped library (tools/build_variant.sh, make prof).
namespace {
using r1tx::T;
using r1cand::sad_u32;

// QM: 0 = coefficients to HBM (headline), 1 = + quantizer, tx-domain distortion,
// rate (N4), 2 = + quantizer, inverse transform, pixel-domain distortion.
// PS: where the prediction comes from, a compile-time choice -- 0 = put_8tap of the reference window, or the
// dense qa.pred_in buffer (a run-time branch of those instantiations); 1 = intra prediction from the candidate's
// edge set (r1_rdo_intra_cand_batch), made inside the chain by the predictors of intra_pred_common.hpp.  The
// PS = 0 instantiations do not see the intra code: their kernels are the ones they were before PS existed.
template <int BD, int WL, int HL, typename CT, int QM, bool MT = false, int PS = 0>
__global__ __launch_bounds__(64, rdo_waves_hint(BD, WL, HL, QM, MT)) void k_rdo_cand(
    R1Plane org, R1Plane ref, const R1RdoCand *__restrict__ cands, int n,
    uint32_t *__restrict__ sad_out, uint32_t *__restrict__ satd_out,
    CT *__restrict__ coeffs, void *__restrict__ pred_out, RdoQuantArgs qa,
    typename std::conditional<PS == 1, RdoIntraArgs, RdoNoIntraArgs>::type ia) {
  // the instantiation's geometry, choices and LDS layout: rdo_cand_plan.hpp, under the names the body uses
  using PL = RdoCandPlan<BD, WL, HL, QM, MT, PS>;
  constexpr int BPP = PL::BPP, W = PL::W, H = PL::H, P = PL::P, NC = PL::NC, TS = PL::TS, WS = PL::WS, FL = PL::FL, HU = PL::HU;
  constexpr bool INTRA = PL::INTRA, SPLIT_T = PL::SPLIT_T, SRC_LDS = PL::SRC_LDS, SRC_LATE = PL::SRC_LATE,
                 SRC_KEEP = PL::SRC_KEEP, SATD_T = PL::SATD_T, COLSHARE = PL::COLSHARE;
  typedef typename PL::TB TB;
  constexpr int LSTRIDE = PL::LSTRIDE, ISTRIDE = PL::ISTRIDE, QT_STRIDE = PL::QT_STRIDE, SRC_ROW = PL::SRC_ROW,
                SRC_CSTRIDE = PL::SRC_CSTRIDE, SATD_STRIDE = PL::SATD_STRIDE, LDS_WORK = PL::LDS_WORK,
                SRC_OFF = PL::SRC_OFF, TKEEP_OFF = PL::TKEEP_OFF, LDS_BYTES = PL::LDS_BYTES;
  static_assert(!INTRA || LDS_BYTES <= RdoCandPlan<BD, WL, HL, QM, MT, 0>::LDS_BYTES,
                "an intra instantiation's LDS must not exceed its inter twin's");
  // forward-transform shifts of this (size, bit depth): immediates
  constexpr int SH0 = r1tx::fwd_shift_ct(WL, HL, BD, 0), SH1 = r1tx::fwd_shift_ct(WL, HL, BD, 1),
                SH2 = r1tx::fwd_shift_ct(WL, HL, BD, 2);
  // COL_FOLD (rdo_cand_plan.hpp): phase C runs the column family, whose outputs already carry shift[1] -- the tile
  // stores then shift by SH1C = 0
  constexpr bool COL_FOLD = PL::COL_FOLD;
  static_assert(!COL_FOLD || SH0 > 0, "the column family starts from a pending shift[0]");
  constexpr int SH1C = COL_FOLD ? 0 : SH1;
  // HALVE2 / MC_PACK4 (rdo_cand_plan.hpp): the networks of m24h in both passes; the shift-free pack of the 8-bit filter
  constexpr bool HALVE2 = PL::HALVE2, MC_PACK4 = PL::MC_PACK4;
  // MUL_HW (rdo_mul_hiword, rdo_cand_plan.hpp): the networks of m24w in both passes, products at scale 2^16 where the
  // pass's input bound allows (CB: columns, RB: rows)
  constexpr bool MUL_HW = PL::MUL_HW;
  constexpr int CB = rdo_mul_col_bound(BD, SH0, COL_FOLD), RB = rdo_mul_row_bound(BD, WL, HL);
  // MC_MATRIX (rdo_cand_plan.hpp): the 8-bit filter's horizontal pass on the matrix pipe, MX_NC candidates per wave
  constexpr int MX_NC = PL::MX_NC;
  static_assert(MX_NC == 0 || (BPP == 1 && QM == 0 && !INTRA && P == W && NC * W == 64),
                "a coefficient kernel of 8-bit pixels, lane = (candidate, column) with no idle lane");
  // MC_MATRIX4 (rdo_cand_plan.hpp): the same pass on sixteen 4x4x4 blocks, four or eight candidates per wave
  constexpr bool MC_MATRIX4 = PL::MC_MATRIX4;
  static_assert(!MC_MATRIX4 || (BPP == 1 && QM == 0 && !INTRA && P == W && NC * W == 64),
                "a coefficient kernel of 8-bit pixels, lane = (candidate, column) with no idle lane");
  __shared__ __attribute__((aligned(16))) uint8_t smem[LDS_BYTES];
  T *buf = (T *)smem;
  TB *tbuf = (TB *)smem;
  TB *tkeep = COLSHARE ? (TB *)(smem + TKEEP_OFF) : tbuf;

  R1_PROF_INIT;
  const unsigned wg = xcd_contiguous_wg();   // workgroup -> candidate group, XCD-aware (common.hpp)
  if ((long long)wg * NC >= (long long)n) return;
  const int lane = threadIdx.x;
  const int cl = lane / P, c = lane % P;
  // n < 2^31 candidates: the liveness test and the lane-local parts of every address are 32-bit;
  // what is 64-bit is the workgroup's base (wg * per-workgroup bytes), which the scalar
  // unit computes
  const int cand_i = (int)wg * NC + cl;
  const long long cand = cand_i;
  // Only STORES look at whether this lane's candidate exists (live_st).  The dead slots of the
  // launch's last wave load and compute the launch's last candidate once more: no masked regions,
  // no zero-initialised registers for the lanes that would have sat out (35 v_mov of the 8x8
  // kernel's 766 VALU instructions), every wave runs the same straight line.
  // Measured (profiles/r03_ab_notes.md, ab4): -3 % at 8x8, -1 % at 16x16 / 32x32, +2 % on the 10-bit
  // step; the 8-bit 64x64 instantiation alone loses (121 -> 143 VGPRs, 4 -> 3 waves per SIMD) and
  // keeps its masked regions.
  constexpr bool UNMASK = !(BD == 8 && WL == 6 && HL == 6);
  const bool live_st = cand_i < n;
  static_assert(!MC_MATRIX4 || UNMASK, "the 4x4x4 MFMAs take operands from all 64 lanes: dead slots repeat a candidate");
  const bool live = UNMASK || live_st;
  const int cl_ld = live_st ? cl : n - 1 - (int)wg * NC;     // >= 0: the wave's first candidate exists
  const long long cand_ld = live_st ? cand : (long long)n - 1;
  R1RdoCand cd = {};
  R1IntraCand ic = {};
  int eset = 0;   // INTRA: the candidate's edge set / lens pair / position pair
  if constexpr (INTRA) {
    if (live) {
      ic = ia.cands[cand_ld];
      eset = (int)cand_ld / ia.edge_group;
      cd.ox = ia.pos_xy[2 * eset];
      cd.oy = ia.pos_xy[2 * eset + 1];
    }
  } else {
    if (live) cd = (cands + (size_t)wg * NC)[cl_ld];
  }
#ifdef R1_PHASE_PROF
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  R1_PROF(5);   // A0: descriptor round trip
#endif
  constexpr bool QUANT = QM != 0;
  // QM == 2 keeps the prediction column (packed pixels) for the reconstruction
  constexpr int PPK = QM == 2 ? (H * BPP + 3) / 4 : 1;
  uint32_t ppk[PPK];
#pragma unroll
  for (int k = 0; k < PPK; k++) ppk[k] = 0;

  // ---- A: source block (registers, or LDS in wide chunks), reference window into LDS ----
  T v[H];
#pragma unroll
  for (int r = 0; r < H; r++) v[r] = 0;
  const bool col_live = live && c < W;
  const uint8_t *src_l = smem + SRC_OFF + cl * SRC_CSTRIDE + c * BPP;
  // A.1: every global load the wave needs goes out before it waits for any of them -- source
  // block, reference window, tap tables depend on the descriptor only (one round trip behind it,
  // not three)
  constexpr int CHS = SRC_ROW >= 16 ? 16 : SRC_ROW;      // source bytes per lane per pass
  constexpr int CPR = SRC_ROW / CHS;                      // chunks per source row
  constexpr int RPP = P / CPR;                            // rows per pass (P lanes per candidate)
  constexpr int SPASS = SRC_LDS ? (H + RPP - 1) / RPP : 1;
  const int srow = c / CPR, sch = c - srow * CPR;
  U32x4 q[SPASS];
  if constexpr (SRC_LDS) {
    // planes are far below 4 GB: a 32-bit byte offset from the allocation's start
    const uint8_t *po = (const uint8_t *)org.data +
                        (((uint32_t)(org.yorigin + cd.oy) * (uint32_t)org.stride + (uint32_t)(org.xorigin + cd.ox)) * BPP +
                         (uint32_t)(sch * CHS));
    const uint32_t so = (uint32_t)org.stride * BPP;
#pragma unroll
    for (int u = 0; u < SPASS; u++) {
      const int rr = srow + u * RPP;
      q[u] = U32x4{0, 0, 0, 0};
      if (live && rr < H) {
        if constexpr (CHS == 16) q[u] = ld_u32x4(po + rr * so);
        else if constexpr (CHS == 8) { const U32x2 t = ld_u32x2(po + rr * so); q[u].a = t.a; q[u].b = t.b; }
        else q[u].a = ld_u32(po + rr * so);
      }
    }
  } else if (col_live) {
    const uint8_t *po = px_addr<BPP>(org, cd.ox + c, cd.oy);
    const size_t so = (size_t)org.stride * BPP;
#pragma unroll
    for (int r = 0; r < H; r++) v[r] = ld_px<BPP>(po + r * so);
  }
  uint8_t *win = smem + cl * (H + 7) * WS;
  const bool from_ref = !INTRA && live && !qa.pred_in;   // !pred_in is wave-uniform: kernel argument
  r1mc::WindowStage<BPP, BPP == 1 ? 0x80808080u : 0u, W, H, P> wst;
  if (from_ref) wst.load(ref, cd.rx, cd.ry, c);
  r1cand::Taps<BPP> tp = {};
  if (from_ref) tp = r1cand::load_taps<BPP, W, H>(cd.col_frac, cd.row_frac, cd.mode_x, cd.mode_y);
  // every filter of the wave with zero outer taps (anything but SHARP): the short column filter
  const bool six = r1cand::taps_six(tp);
  // MC_MATRIX, two candidates: the zeros that the other candidate's row groups supply (under the loads' round trip)
  if constexpr (PL::MX_ZERO_BYTES != 0) {
#pragma unroll
    for (int k = 0; k < (PL::MX_ZERO_BYTES / 16 + 63) / 64; k++)
      if (lane + 64 * k < PL::MX_ZERO_BYTES / 16)
        *(uint4 *)(smem + PL::MX_ZERO_OFF + 16 * (lane + 64 * k)) = make_uint4(0u, 0u, 0u, 0u);
  }
  // A.2: into LDS
  auto stage_source = [&]() {
    if (live) {
      uint8_t *sd = smem + SRC_OFF + cl * SRC_CSTRIDE + sch * CHS;
#pragma unroll
      for (int u = 0; u < SPASS; u++) {
        const int rr = srow + u * RPP;
        if (rr < H) {
          if constexpr (CHS == 16) *(uint4 *)(sd + rr * SRC_ROW) = make_uint4(q[u].a, q[u].b, q[u].c, q[u].d);
          else if constexpr (CHS == 8) *(uint2 *)(sd + rr * SRC_ROW) = make_uint2(q[u].a, q[u].b);
          else *(uint32_t *)(sd + rr * SRC_ROW) = q[u].a;
        }
      }
    }
  };
  if constexpr (SRC_LDS && !SRC_LATE && !INTRA) stage_source();
  if (from_ref) wst.store(win, WS);
  // INTRA: the raw edge, the 2 (W + H) + 1 entries around the top-left one that a W x H block can reach (what lies
  // outside [128 - lens[0], 129 + lens[1]) is undefined in the caller's buffer and never used, as in k_intra_predict),
  // by the P lanes of the candidate
  uint16_t *eraw = (uint16_t *)smem + cl * (5 * FL);
  int left_len = 0, above_len = 0;
  if constexpr (INTRA) {
    if (live) {
      left_len = ia.lens[2 * eset];
      above_len = ia.lens[2 * eset + 1];
      const uint8_t *e = (const uint8_t *)ia.edges + ((size_t)eset * ia.edge_stride + (2 * r1ip::MAXTX - (W + H))) * BPP;
      for (int k = c; k < FL; k += P) eraw[k] = (uint16_t)ld_px<BPP>(e + k * BPP);
    }
  }
#ifdef R1_PHASE_PROF
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  R1_PROF(6);   // A1: source column + window round trip (+ LDS writes issued)
#endif
  __syncthreads();
  R1_PROF(0);   // A: descriptor, source column, window staged

  // ---- B: prediction column, residual, SAD / SATD ----
  uint32_t sad_acc = 0;
  if constexpr (INTRA) {
    // the cooperative part (edge filter / upsample: every lane of the wave, P per candidate), then lane =
    // (candidate, column) walks its column into registers
    const bool directional = live && r1ip::is_directional(ic.mode, ic.angle);
    const bool enable = directional && ic.ief != 0;
    const uint16_t *tl = eraw + (W + H);
    uint16_t *work = eraw + FL;
    int up_a = 0, up_l = 0;
    r1ip::edge_filter_upsample<const R1IntraCand &>(tl, 0, work, W, H, P, c, ic, enable, left_len, above_len,
                                                     (1 << BD) - 1, up_a, up_l);
    int32_t pred[H];
    if (col_live) {
      // (a CFL candidate without an AC buffer -- the entry point refuses the ones it can see -- predicts its DC)
      if (ic.mode == r1ip::UV_CFL_PRED && !ia.ac) ic.angle = 0;
      const int16_t *acb = ic.mode == r1ip::UV_CFL_PRED && ia.ac ? ia.ac + (size_t)cand_ld * (W * H) : nullptr;
      r1ip::predict_column<const R1IntraCand &>(W, H, c, ic, directional, enable, up_a, up_l, tl, 0, work, left_len, BD,
                                                 acb, [&](int i, int32_t pv) { pred[i] = pv; });
      if (pred_out && live_st) {
        if constexpr (BPP == 1) {
          uint8_t *pp = (uint8_t *)pred_out + (size_t)cand * W * H + c;
#pragma unroll
          for (int r = 0; r < H; r++) pp[(size_t)r * W] = (uint8_t)pred[r];
        } else {
          uint16_t *pp = (uint16_t *)pred_out + (size_t)cand * W * H + c;
#pragma unroll
          for (int r = 0; r < H; r++) pp[(size_t)r * W] = (uint16_t)pred[r];
        }
      }
      if constexpr (QM == 2) {
#pragma unroll
        for (int r = 0; r < H; r++) {
          if constexpr (BPP == 1) ppk[r >> 2] |= (uint32_t)pred[r] << (8 * (r & 3));
          else ppk[r >> 1] |= (uint32_t)pred[r] << (16 * (r & 1));
        }
      }
    }
    if constexpr (SRC_LDS) {
      __syncthreads();   // every lane has made its column: the edge arrays are dead
      stage_source();
      __syncthreads();
    }
    if (col_live) {
      if constexpr (SRC_LDS) {
#pragma unroll
        for (int r = 0; r < H; r++) {
          const uint32_t sp = BPP == 1 ? (uint32_t)src_l[r * SRC_ROW] : (uint32_t) * (const uint16_t *)(src_l + r * SRC_ROW);
          sad_acc = sad_u32(sp, (uint32_t)pred[r], sad_acc);
          v[r] = (T)sp - pred[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < H; r++) v[r] -= pred[r];
      }
    }
  } else
  if constexpr (BPP == 1) {
    if (col_live) {
      int32_t pred[H];
      if (qa.pred_in) {
        const uint8_t *pi = (const uint8_t *)qa.pred_in + (size_t)cand_ld * W * H + c;
#pragma unroll
        for (int r = 0; r < H; r++) pred[r] = pi[(size_t)r * W];
      } else {
        // MC_MATRIX: the MFMAs take their operands from every lane.  All 64 lanes are here then -- lane = (candidate,
        // column) with no idle lane, a wave that runs has its first candidate, and the second slot of the last 32x32
        // wave repeats the launch's last one (UNMASK) -- under the wave-uniform branch on the kernel argument above.
        if constexpr (MX_NC != 0)
          r1cand::mc_column_fast<BPP, W, H, WS, false, MC_PACK4, MX_NC>(smem, c, tp, BD, pred, six, lane,
                                                                         smem + PL::MX_ZERO_OFF);
        // MC_MATRIX4: likewise all 64 lanes (UNMASK: the dead slots of the last wave repeat the launch's last
        // candidate); every lane on its own window and column, with its own candidate's taps
        else if constexpr (MC_MATRIX4)
          r1cand::mc_column_fast<BPP, W, H, WS, false, MC_PACK4, 0, true>(win, c, tp, BD, pred, six);
        else
        r1cand::mc_column_fast<BPP, W, H, WS, false, MC_PACK4>(win, c, tp, BD, pred, six);
      }
      if (pred_out && live_st) {
        uint8_t *pp = (uint8_t *)pred_out + (size_t)cand * W * H + c;
#pragma unroll
        for (int r = 0; r < H; r++) pp[(size_t)r * W] = (uint8_t)pred[r];
      }
      if constexpr (QM == 2) {
#pragma unroll
        for (int r = 0; r < H; r++) ppk[r >> 2] |= (uint32_t)pred[r] << (8 * (r & 3));
      }
      if constexpr (SRC_LDS) {
#pragma unroll
        for (int r = 0; r < H; r++) {
          const uint32_t sp = src_l[r * SRC_ROW];
          sad_acc = sad_u32(sp, (uint32_t)pred[r], sad_acc);   // |source - prediction| summed in one op
          v[r] = (T)sp - pred[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < H; r++) v[r] -= pred[r];
      }
    }
  } else {
    int32_t pred[H];
    if (col_live) {
      if (qa.pred_in) {
        const uint16_t *pi = (const uint16_t *)qa.pred_in + (size_t)cand_ld * W * H + c;
#pragma unroll
        for (int r = 0; r < H; r++) pred[r] = pi[(size_t)r * W];
      } else {
        r1cand::mc_column_fast<BPP, W, H, WS, false>(win, c, tp, BD, pred, six);
      }
      if (pred_out && live_st) {
        uint16_t *pp = (uint16_t *)pred_out + (size_t)cand * W * H + c;
#pragma unroll
        for (int r = 0; r < H; r++) pp[(size_t)r * W] = (uint16_t)pred[r];
      }
      if constexpr (QM == 2) {
#pragma unroll
        for (int r = 0; r < H; r++) ppk[r >> 1] |= (uint32_t)pred[r] << (16 * (r & 1));
      }
    }
    if constexpr (SRC_LATE) {
      __syncthreads();   // every lane has filtered its column: the window is dead
      stage_source();
      __syncthreads();
    }
    if (col_live) {
      if constexpr (SRC_LDS) {
#pragma unroll
        for (int r = 0; r < H; r++) {
          const uint32_t sp = *(const uint16_t *)(src_l + r * SRC_ROW);
          sad_acc = sad_u32(sp, (uint32_t)pred[r], sad_acc);
          v[r] = (T)sp - pred[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < H; r++) v[r] -= pred[r];
      }
    }
  }
  R1_PROF(1);   // B1: motion compensation + residual
  if (sad_out) {
    uint32_t sad = sad_acc;
    if constexpr (!SRC_LDS) {
#pragma unroll
      for (int r = 0; r < H; r++) sad += (uint32_t)iabs32(v[r]);
    }
    const uint32_t s = group_sum<P>(sad);
    // (non-temporal here too was tried: no difference, gpurun_out/r04_ab4 -- 8 bytes per candidate)
    if (live_st && c == 0) (sad_out + (size_t)wg * NC)[cl] = s;
  }
  if (satd_out) {
    uint32_t part;
    if constexpr (SATD_T) {
      uint32_t *tile = (uint32_t *)smem + cl * SATD_STRIDE;
      __syncthreads();   // every lane has read its window and source column
      if (c < W) r1cand::satd_tile_store<W, H>(v, tile + c);
      __syncthreads();
      part = r1cand::satd_tile_rows<(W < H ? W : H) / 16, P>(tile, c);   // the reads end before phase C's first barrier
    } else {
      part = r1cand::satd_column<TS, H, BD>(v, lane);
    }
    const uint32_t s = group_sum<P>(part);
    constexpr int LN = TS == 4 ? 2 : 3;
    if (live_st && c == 0) (satd_out + (size_t)wg * NC)[cl] = (s + ((1u << LN) >> 1)) >> LN;
  }
  R1_PROF(2);   // B2: SAD + SATD
  if (!QUANT && !coeffs) return;   // wave-uniform: kernel argument

  // ---- MT: the transform-type fan-out (rdo_tx_type_decision, src/rdo.rs:1701-1817).  The reference runs
  // motion_compensate + write_tx_tree + compute_distortion once per type of RAV1E_TX_TYPES
  // (src/transform/mod.rs:28-44) that the block's tx set allows, on the SAME prediction; here phases A / B ran
  // once and C .. H loop over the set bits of the launch's mask (a kernel argument: wave-uniform, every
  // 1-D kernel switch below is a scalar branch).  What an iteration needs again is the residual column: where
  // the source block stays in LDS (SRC_KEEP) it is re-formed from there and the packed prediction the
  // reconstruction keeps anyway -- no register is live across the loop for it; elsewhere a register copy.
  constexpr bool MT_RECOMP = MT && SRC_KEEP;
  T vkeep[MT && !MT_RECOMP ? H : 1];
  if constexpr (MT && !MT_RECOMP) {
#pragma unroll
    for (int r = 0; r < H; r++) vkeep[r] = v[r];
  }
  // TAIL_DEFER (type search of an 8x8 block under cdef_dist: one 8x8 kernel per candidate, eight lanes per
  // candidate, at most seven types): see the end of the kernel
  constexpr bool TAIL_DEFER = MT && QM == 2 && W == 8 && H == 8;
  // (a mask of more than eight types -- the full AV1 inter set has sixteen -- keeps its tails inside the loop)
  const bool tail_defer = TAIL_DEFER && qa.dist_kind == R1_DIST_CDEF && qa.nt <= 8;   // wave-uniform
  r1dist::CdefMoments tail_keep;
  // The loop: groups of types that share the column pass (same vertical 1-D kernel and the same flips; without
  // COLSHARE every type is a group of its own), and inside a group the types in ascending order.  The result slot of
  // a type is its rank in the launch's mask, whatever order the groups come in.
  uint32_t rem = MT ? qa.tx_mask : 1u;
  bool fresh = true;   // v still holds the residual as phase B left it
  do {
  int t0 = 0;
  uint32_t gmask = 1u;
  if constexpr (MT) {
    t0 = (int)__builtin_ctz(rem);
    gmask = 1u << t0;
    if constexpr (COLSHARE) {
      auto colkey = [](int t) { return r1tx::vtx_1d(t) | ((int)r1tx::ud_flip(t) << 4) | ((int)r1tx::lr_flip(t) << 5); };
      const int k0 = colkey(t0);
      for (uint32_t m = rem & (rem - 1); m != 0; m &= m - 1) {   // scalar: the mask is a kernel argument
        const int t = (int)__builtin_ctz(m);
        if (colkey(t) == k0) gmask |= 1u << t;
      }
    }
    rem &= ~gmask;
    if (!fresh) {   // wave-uniform
      if constexpr (MT_RECOMP) {
        if (col_live) {
#pragma unroll
          for (int r = 0; r < H; r++) {
            const T sp = BPP == 1 ? (T)src_l[r * SRC_ROW] : (T) * (const uint16_t *)(src_l + r * SRC_ROW);
            const T pr = BPP == 1 ? (T)((ppk[r >> 2] >> (8 * (r & 3))) & 0xFF)
                                  : (T)((ppk[r >> 1] >> (16 * (r & 1))) & 0xFFFF);
            v[r] = sp - pr;
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < H; r++) v[r] = vkeep[r];
      }
    }
    fresh = false;
  }
  // ---- C: column transform on the residual registers ----
  __syncthreads();  // every lane is done reading the window (MT: the previous type's last phase); LDS becomes buf
  const int tx_col = MT ? t0 : (QM != 0 && qa.tx_mask != 0 ? (int)__builtin_ctz(qa.tx_mask) : (int)cd.tx_type);
  // TX_VOTE (rdo_tx_vote, rdo_cand_plan.hpp): the type comes from the descriptors, a per-lane value -- the 1-D kernel
  // switches of phases C and D are lane-divergent branches then, paid by every wave in class decodes, exec
  // bookkeeping and the copies that merge the arms with the identity's pass-through.  A mode-decision pass evaluates
  // ONE type over many predictions, so the wave votes once: when all its candidates agree (every lane holds a
  // descriptor: the dead slots of the last wave repeat a live candidate and agree by construction) the type goes
  // through readfirstlane and the switch between the kernels is a scalar branch.  A wave of mixed types keeps the
  // per-lane switch, and so does a wave of one type whose class in this pass is the identity (col_uni / row_uni): with
  // no pass-through arm every arm of the scalar switch writes all its outputs and nothing is copied to merge them.
  // Only the switch forks: the flip, the shifts and the tile stores around it are one code for both, or the values
  // the fork's second arm reads stay live across its first (the scalar branch sits inside structurized control flow)
  // and the 16x16 kernel loses a wave per SIMD (profiles/r16_txuniform_notes.md).
  constexpr bool TX_VOTE = rdo_tx_vote(WL, HL, QM, MT, PS);
  static_assert(!TX_VOTE || UNMASK, "the vote reads every lane's descriptor");
  int tx_s = 0;
  bool tx_uni = false, col_uni = false, row_uni = false;
  if constexpr (TX_VOTE) {
    tx_s = __builtin_amdgcn_readfirstlane(tx_col);
    tx_uni = __all(tx_col == tx_s);
    col_uni = tx_uni && r1tx::vtx_1d(tx_s) != 3;
    row_uni = tx_uni && r1tx::htx_1d(tx_s) != 3;
  }
  bool any_ud;
  if (TX_VOTE && tx_uni) any_ud = r1tx::ud_flip(tx_s);   // scalar
  else any_ud = __any(live && r1tx::ud_flip(tx_col));
  if (col_live) {
    if (any_ud) {   // wave-uniform: skipped when no candidate of the wave flips
      const bool ud = r1tx::ud_flip(tx_col);
#pragma unroll
      for (int r = 0; r < H / 2; r++) {
        const T t0 = v[r], t1 = v[H - 1 - r];
        v[r] = ud ? t1 : t0;
        v[H - 1 - r] = ud ? t0 : t1;
      }
    }
    if constexpr (COL_FOLD) {   // shift[0], the network and shift[1] as one: the column family on the unshifted residuals
      if constexpr (MUL_HW) {
        if (TX_VOTE && col_uni) r1tx::fwd_col_m24w_kernel<H, SH0, SH1, CB>(v, r1tx::vtx_1d(tx_s));
        else r1tx::fwd_col_m24w<H, SH0, SH1, CB>(v, r1tx::vtx_1d(tx_col));
      } else {
        if (TX_VOTE && col_uni) r1tx::fwd_col_m24_kernel<H, SH0, SH1, HALVE2>(v, r1tx::vtx_1d(tx_s));
        else r1tx::fwd_col_m24<H, SH0, SH1, HALVE2>(v, r1tx::vtx_1d(tx_col));
      }
    } else {
#pragma unroll
      for (int r = 0; r < H; r++) v[r] = r1tx::shift_fwd_ct<SH0>(v[r]);
      if constexpr (MUL_HW) {
        if (TX_VOTE && col_uni) r1tx::fwd_1d_m24w_kernel<H, CB>(v, r1tx::vtx_1d(tx_s));
        else r1tx::fwd_1d_m24w<H, CB>(v, r1tx::vtx_1d(tx_col));
      } else {
        if (TX_VOTE && col_uni) r1tx::fwd_1d_m24_kernel<H, HALVE2>(v, r1tx::vtx_1d(tx_s));
        else r1tx::fwd_1d_m24<H, HALVE2>(v, r1tx::vtx_1d(tx_col));
      }
    }
    if constexpr (!SPLIT_T) {
      const int cc = cl * W + (r1tx::lr_flip(tx_col) ? W - 1 - c : c);
#pragma unroll
      for (int r = 0; r < HU; r++)
        tkeep[r * LSTRIDE + cc] = (TB)r1tx::shift_fwd_ct<SH1C>(v[r]);
    }
  }
  if constexpr (!SPLIT_T) __syncthreads();
  R1_PROF(3);   // C: column transform, transpose written
  do {   // the types of the group: rows from the shared tile, then everything that depends on the type
  const int tx_type = MT ? (int)__builtin_ctz(gmask) : tx_col;
  const int slot = MT ? (int)__builtin_popcount(qa.tx_mask & ((1u << tx_type) - 1u)) : 0;
  // result slot of (candidate, type)
  const long long oslot = MT ? cand * (long long)qa.nt + slot
                             : (QM != 0 && qa.nt != 0 ? cand * (long long)qa.nt + qa.slot : cand);
  // ---- D: row transform, transposed store ----
  // P lanes per candidate again: the lane that filtered column c of candidate cl now owns row c
  // of the same candidate -- its descriptor is still in registers
  const int cl2 = cl, r = c;
  const bool live2 = live;
  const bool row_live = live2 && r < HU;
  const int tt = tx_type;
  constexpr int OS = H < 32 ? H : 32, WC = W < 32 ? W : 32;
  T u[W];
  if constexpr (SPLIT_T) {
    // rows 0..31 travel first and are picked up by lanes 0..31, then rows 32..63 through
    // the same bytes for lanes 32..63 (one candidate per wave here: cl = cl2 = 0)
    const int cc = r1tx::lr_flip(tx_type) ? W - 1 - c : c;
#pragma unroll
    for (int half = 0; half < HU / 32; half++) {
      if (col_live) {
#pragma unroll
        for (int rr = 0; rr < 32; rr++)
          tbuf[rr * LSTRIDE + cc] = (TB)r1tx::shift_fwd_ct<SH1C>(v[half * 32 + rr]);
      }
      __syncthreads();
      if (row_live && (r >> 5) == half) {
#pragma unroll
        for (int k = 0; k < W; k++) u[k] = tbuf[(r & 31) * LSTRIDE + k];
      }
      __syncthreads();
    }
  }
  if (row_live) {
    if constexpr (!SPLIT_T) {
#pragma unroll
      for (int k = 0; k < W; k++) u[k] = tkeep[r * LSTRIDE + cl2 * W + k];
    }
    // the switch on the scalar or per lane, as in phase C (the left-right flip is the tile store's column)
    if constexpr (MUL_HW) {
      if (TX_VOTE && row_uni) r1tx::fwd_1d_m24w_kernel<W, RB>(u, r1tx::htx_1d(tx_s));
      else r1tx::fwd_1d_m24w<W, RB>(u, r1tx::htx_1d(tt));
    } else {
      if (TX_VOTE && row_uni) r1tx::fwd_1d_m24_kernel<W, HALVE2>(u, r1tx::htx_1d(tx_s));
      else r1tx::fwd_1d_m24<W, HALVE2>(u, r1tx::htx_1d(tt));
    }
#pragma unroll
    for (int k = 0; k < W; k++) {
      u[k] = r1tx::shift_fwd_ct<SH2>(u[k]);
      // `as T::Coeff` (forward.rs:157): the stores below truncate by themselves; only the
      // quantizer variants go on computing with the value
      if constexpr (QUANT) u[k] = (T)(CT)u[k];
    }
  }
  if constexpr (MT) {
    // the type search keeps its coefficients on the CU
  } else
  if constexpr (P > 16) {
    // large blocks: direct element stores (measured: the LDS detour costs more than the
    // 16-byte stores save at 32x32 and 64x64, profiles/r02_wide_store_ab.log)
    if (coeffs && row_live && live_st) {
      CT *dst = coeffs + (size_t)wg * (NC * W * H) + (cl2 * (W * H) + (r >= 32 ? OS * WC : 0) + (r & 31));
#pragma unroll
      for (int cg = 0; cg < W; cg += 32)
#pragma unroll
        for (int k = 0; k < WC; k++) __builtin_nontemporal_store((CT)u[k + cg], &dst[H * cg + k * OS]);
    }
  } else
  if (coeffs) {   // wave-uniform: kernel argument
    // The reference's transposed coefficient order (forward.rs:135-159) puts the rows r of a
    // column k next to each other: with lane = row a direct store is one 2- or 4-byte element
    // per lane per instruction -- W (64x64: 128) scattered store instructions per wave, and
    // this kernel runs at the texture-address unit's ~16 cycles per vector-memory instruction
    // (DESIGN.md 5.1).  So the block is assembled in LDS in its final order (the transpose
    // tile is dead: every lane holds its row) and leaves as 16-byte stores, W*sizeof(CT)/16
    // per wave.  64x64 32-bit coefficients (16 KB) go in two halves (k < 32, k >= 32), which
    // are contiguous halves of the output.
    constexpr int ESZ = (int)sizeof(CT);
    constexpr int NP = NC * W * H * ESZ > LDS_WORK ? 2 : 1;
    static_assert(NP == 1 || W == 64, "only the 64-wide blocks are split");
    static_assert(NC * W * H * ESZ / NP <= LDS_WORK, "a pass fits the LDS of the kernel");
    constexpr int EPP = W * H / NP;                 // elements of one candidate per pass
    constexpr int CBY = EPP * ESZ;                  // bytes of one candidate per pass
    constexpr int CH = CBY / P >= 16 ? 16 : CBY / P;   // bytes a lane moves per step
    constexpr int NCH = CBY / P / CH;
    static_assert(CH * NCH * P == CBY && (CH == 16 || CH == 8 || CH == 4), "whole chunks");
    // candidates one row of P elements apart: with the bare stride (a multiple of 32 dwords for
    // 8x8 / 16x16) the NC candidates of a lane group hit the same banks with their element
    // writes (4-way at 8x8: SQ_LDS_BANK_CONFLICT 4.1 M -> 20.7 M per launch when this path came in)
    constexpr int TPAD = NC > 1 ? ((P * ESZ + 15) & ~15) / ESZ : 0;
    static_assert(NC * (EPP + TPAD) * ESZ <= LDS_WORK, "the padded tiles fit the LDS of the kernel");
    static_assert(((EPP + TPAD) * ESZ) % 16 == 0, "16-byte reads stay aligned");
    CT *tile = (CT *)smem + cl2 * (EPP + TPAD);
    uint8_t *gdst = (uint8_t *)(coeffs + (size_t)wg * (NC * W * H)) + cl2 * (W * H * ESZ);
#pragma unroll
    for (int p = 0; p < NP; p++) {
      __syncthreads();   // rows are in registers (pass 0) / the previous half has been copied out
      if (row_live) {
        constexpr int KP = W / NP;
#pragma unroll
        for (int k = p * KP; k < (p + 1) * KP; k++) {
          const int e = (r >= 32 ? OS * WC : 0) + (r & 31) + H * (k & ~31) + (k & 31) * OS - p * EPP;
          tile[e] = (CT)u[k];
        }
      }
      __syncthreads();
      if (live_st) {
        const uint8_t *src = (const uint8_t *)tile + r * CH;
        uint8_t *dst = gdst + p * CBY + r * CH;
#pragma unroll
        for (int j = 0; j < NCH; j++) {
          // The coefficients are not read again by this launch, and a step writes 0.26 GB (8-bit) / 0.53 GB
          // (10-bit) of them per ladder size: written through the L2 as ordinary stores they evict the window
          // rows the K candidates of a block share.  Non-temporal stores (same-box A/B, gpurun_out/r04_ab3):
          // 8-bit 8x8 launch 0.226 -> 0.206 ms, 10-bit 8x8 0.308 -> 0.232, 10-bit 16x16 0.252 -> 0.221; step
          // +3.3 % / +11 %.
          if constexpr (CH == 16) {
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(*(const u32x4_t *)(src + j * P * CH), (u32x4_t *)(dst + j * P * CH));
          } else if constexpr (CH == 8) {
            typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
            __builtin_nontemporal_store(*(const u32x2_t *)(src + j * P * CH), (u32x2_t *)(dst + j * P * CH));
          } else {
            __builtin_nontemporal_store(*(const uint32_t *)(src + j * P * CH), (uint32_t *)(dst + j * P * CH));
          }
        }
      }
    }
  }
  R1_PROF(4);   // D: row transform + stores issued
  if constexpr (QUANT) {
    // ---- E: quantizer on the coded area, in LDS (aliases the transpose tile:
    // every row lane has its row in registers by now) ----
    constexpr int CODED = OS * WC;
    constexpr int PL = WL > HL ? WL : HL;          // log2(P)
    constexpr int NPLQ = CODED / P;
    static_assert(CODED % P == 0 && NPLQ >= 1, "P lanes share the coded area");
    __syncthreads();
    int32_t *tile = (int32_t *)smem + cl2 * QT_STRIDE;
    unsigned long long tail = 0;
    if (row_live) {
#pragma unroll
      for (int k = 0; k < W; k++) {
        if (r < 32 && k < 32) {
          tile[k * OS + r] = u[k];
        } else {   // beyond the coded area: rcoeff = 0 (encoder.rs:1628-1634)
          tail += (unsigned long long)(long long)(int32_t)((uint32_t)u[k] * (uint32_t)u[k]);
        }
      }
    }
    __syncthreads();
    const int kind = tt < 10 ? 0 : ((tt & 1) ? 2 : 1);
    int eob = 0;
    unsigned long long dist = 0;
    // log_tx_scale follows from the block size (quantize/mod.rs:get_log_tx_scale): a constant here
    constexpr int LTS = (W * H > 256) + (W * H > 1024);
#ifndef R1_QUANT_MID
#define R1_QUANT_MID 0   // the 24-bit quantizer for i32 coefficients: exact (tests/test_tx_range.py, GPU-tested at the range
                         // limits) and no faster -- 10-bit pixel chain 283-285 k -> 282 k Mpx/s, the 32x32 launch +5 % slower
                         // (profiles/r06_ab_notes.md, ab4).  Off: the round-5 arithmetic stays the product path.
#endif
    // i32 coefficients here come from a pixel residual: |c << lts| <= 2^21 (quant_common.hpp, QParams::ac_m22)
    constexpr bool QMID = R1_QUANT_MID && sizeof(CT) == 4;
    r1q::quantize_group<CT, PL, NPLQ, QM == 1, LTS, QMID>(tile, cl2 * P, r, live2, qa.scan[kind], qa.qp, tail,
                                                          eob, dist);
    if (live_st && r == 0) {
      qa.eob[oslot] = (uint16_t)eob;
      if constexpr (QM == 1) {
        qa.tx_dist[oslot] = dist;
        if (qa.est_rate) qa.est_rate[oslot] = r1q::estimate_rate(qa.q_bin, qa.tx_size, dist);
      }
    }
    if (qa.qcoeffs) {
      __syncthreads();
      if (live_st) {
        CT *qd = (CT *)qa.qcoeffs + oslot * CODED;
#pragma unroll
        for (int k = 0; k < NPLQ; k++) qd[k * P + r] = (CT)tile[k * P + r];
      }
    }
    if constexpr (QM == 2) {
      // ---- F: dequantize (mod.rs:372-383) + inverse row transform
      // (inverse_transform_add, src/transform/inverse.rs:1633-1705; k_inv_tx) ----
      constexpr int HC = OS;
      constexpr bool RECT1 = (WL > HL ? WL - HL : HL - WL) == 1;
      __syncthreads();
      const bool irow_live = live2 && r < HC;
      T w_[W];
      {
        const int range = BD + 8;
        const T hi = (T)((1 << (range - 1)) - 1), lo = -hi - 1;
        constexpr int32_t off = (1 << LTS) - 1;
        if (irow_live) {
#pragma unroll
          for (int k = 0; k < WC; k++) {
            const int32_t q = (int32_t)(CT)tile[k * OS + r];
            const uint32_t quant = (k == 0 && r == 0) ? qa.qp.dc_q : qa.qp.ac_q;
            const uint32_t prod = QMID ? (uint32_t)r1q::mul24_wrap(q, (int32_t)quant) : (uint32_t)q * quant;
            const T raw = (T)(CT)((int32_t)(prod + (uint32_t)((q >> 31) & off)) >> LTS);
            const T val = RECT1 ? ((T)((uint32_t)raw * 2896u + 2048u) >> 12) : raw;
            w_[k] = r1itx::clamp3(val, lo, hi);
          }
#pragma unroll
          for (int k = WC; k < W; k++) w_[k] = 0;
          r1itx::inv_1d<W, true>(w_, r1tx::htx_1d(tt), lo, hi);
        }
      }
      __syncthreads();   // every coefficient has been read: the tile becomes the row buffer
      if (irow_live) {
#pragma unroll
        for (int k = 0; k < W; k++) buf[r * ISTRIDE + cl2 * W + k] = w_[k];
      }
      __syncthreads();
      // ---- G: inverse column transform, reconstruction (lane = column again) ----
      T rc[H];
      if (col_live) {
        const int range = BD + 6 > 16 ? BD + 6 : 16;
        const T hi = (T)((1 << (range - 1)) - 1), lo = -hi - 1;
        const T pmax = (T)((1 << BD) - 1);
#pragma unroll
        for (int rr = 0; rr < HC; rr++) {
          const T x = buf[rr * ISTRIDE + cl * W + c];
          rc[rr] = r1itx::clamp3((x + ((1 << qa.inv_shift) >> 1)) >> qa.inv_shift, lo, hi);
        }
#pragma unroll
        for (int rr = HC; rr < H; rr++) rc[rr] = 0;
        r1itx::inv_1d<H, true>(rc, r1tx::vtx_1d(tx_type), lo, hi);
#pragma unroll
        for (int rr = 0; rr < H; rr++) {
          const T pr = BPP == 1 ? (T)((ppk[rr >> 2] >> (8 * (rr & 3))) & 0xFF)
                                : (T)((ppk[rr >> 1] >> (16 * (rr & 1))) & 0xFFFF);
          const T px = pr + ((rc[rr] + 8) >> 4);
          rc[rr] = px < 0 ? 0 : (px > pmax ? pmax : px);
        }
      }
      if (col_live && live_st && qa.rec) {
        if constexpr (BPP == 1) {
          uint8_t *d = (uint8_t *)qa.rec + (size_t)oslot * W * H + c;
#pragma unroll
          for (int rr = 0; rr < H; rr++) d[(size_t)rr * W] = (uint8_t)rc[rr];
        } else {
          uint16_t *d = (uint16_t *)qa.rec + (size_t)oslot * W * H + c;
#pragma unroll
          for (int rr = 0; rr < H; rr++) d[(size_t)rr * W] = (uint16_t)rc[rr];
        }
      }
      unsigned long long acc = 0;
      constexpr bool COL_DIST = H <= 16;
      if constexpr (COL_DIST) {
        // ---- H (blocks up to 32 rows): sse_wxh / cdef_dist_wxh with lane = column.  The
        // reconstruction column is still in registers, the source column is read
        // again; a tile's 8 (4) lanes meet by xor-shuffles, its first lane runs the
        // fixed-point tail (dist_common.hpp).  With one lane per 8x8 tile (the H = 64
        // path below) an 8x8 candidate keeps 8 of the 64 lanes busy for 64 pixels each.
        constexpr int KW = W < 8 ? W : 8, KH = H < 8 ? H : 8;
        const uint8_t *po = px_addr<BPP>(org, cd.ox + (col_live ? c : 0), cd.oy);
        const size_t so = (size_t)org.stride * BPP;
        if (qa.dist_kind == R1_DIST_CDEF) {
          // the five sums of every tile row first, ONE fixed-point tail afterwards: after the xor-shuffles
          // all KW lanes of a tile hold its sums, so lane j of the group takes tile row j (16-row blocks have
          // two) -- the tail (ssim boost in 64-bit arithmetic) used to run once per tile row with one lane
          // of the group alive
          constexpr int NR = H / KH;
          static_assert(NR <= KW, "a tile group has a lane for every tile row");
          uint32_t S[NR][5];   // the tile rows' moments, parked
#pragma unroll
          for (int t = 0; t < NR; t++) {
            const int y0 = t * KH;
            r1dist::CdefMoments m;   // a local: the sums sit in registers before the t loop is unrolled
            if (col_live) {
#pragma unroll
              for (int rr = 0; rr < KH; rr++) {
                uint32_t sv;
                if constexpr (SRC_KEEP) sv = BPP == 1 ? (uint32_t)src_l[(y0 + rr) * SRC_ROW]
                                                      : (uint32_t) * (const uint16_t *)(src_l + (y0 + rr) * SRC_ROW);
                else sv = (uint32_t)ld_px<BPP>(po + (y0 + rr) * so);
                m.add(sv, (uint32_t)rc[y0 + rr]);
              }
            }
            m.xor_sum(1, KW);
            m.store(S[t]);
          }
          // the lane select runs on the parked dwords, sum by sum: on an array of CdefMoments, field by field, the
          // 8-bit 8x8 type-search kernel spilled two dwords more and lost 0.24 % (profiles/r08_reduce_ab_notes.md)
          const int j = c & (KW - 1);
          uint32_t P5a[5];
#pragma unroll
          for (int q5 = 0; q5 < 5; q5++) {
            P5a[q5] = S[0][q5];
#pragma unroll
            for (int t = 1; t < NR; t++) P5a[q5] = j == t ? S[t][q5] : P5a[q5];
          }
          const r1dist::CdefMoments P5 = r1dist::CdefMoments::load(P5a);
          if (TAIL_DEFER && tail_defer) {
            // type search, 8x8: lane `slot` of the candidate's eight keeps this type's five sums; the tails run
            // once, behind the loop
            if (j == slot) tail_keep = P5;
          } else if (col_live && j < NR)
            acc += r1dist::cdef_tile_tail<BD>(P5, KW * KH, cd.ox + c - j, cd.oy + j * KH, qa.scales, qa.scale_stride,
                                              BD);
        } else {
#pragma unroll
          for (int y0 = 0; y0 < H; y0 += 4) {
            uint32_t cell = 0;
            if (col_live) {
#pragma unroll
              for (int rr = 0; rr < 4; rr++) {
                int32_t sv;
                if constexpr (SRC_KEEP) sv = BPP == 1 ? (int32_t)src_l[(y0 + rr) * SRC_ROW]
                                                      : (int32_t) * (const uint16_t *)(src_l + (y0 + rr) * SRC_ROW);
                else sv = ld_px<BPP>(po + (y0 + rr) * so);
                const int32_t d = sv - (int32_t)rc[y0 + rr];
                cell += (uint32_t)(d * d);
              }
            }
            cell += __shfl_xor(cell, 1, 64);
            cell += __shfl_xor(cell, 2, 64);
            if (col_live && (c & 3) == 0) {
              const int lx = (cd.ox + c) << qa.xdec, ly = (cd.oy + y0) << qa.ydec;
              acc += r1dist::wsse_cell(cell, r1dist::dist_scale_at(qa.scales, qa.scale_stride, lx, ly));
            }
          }
        }
      } else {
      __syncthreads();   // the row buffer has been read: LDS becomes the reconstruction
      uint8_t *rec_l = smem + cl * (W * H * BPP);
      if (col_live) {
#pragma unroll
        for (int rr = 0; rr < H; rr++) {
          if constexpr (BPP == 1) rec_l[rr * W + c] = (uint8_t)rc[rr];
          else ((uint16_t *)rec_l)[rr * W + c] = (uint16_t)rc[rr];
        }
      }
      __syncthreads();
      // ---- H (64-row blocks): one lane per 8x8 tile (dist_common.hpp) ----
      constexpr int TW8 = (W + 7) / 8, NT8 = TW8 * ((H + 7) / 8);
      static_assert(NT8 <= P, "a candidate's lanes cover its 8x8 tiles");
      if (live && c < NT8) {
        const int x0 = (c % TW8) * 8, y0 = (c / TW8) * 8;
        const int kw = W - x0 < 8 ? W - x0 : 8, kh = H - y0 < 8 ? H - y0 : 8;
        const uint8_t *po = px_addr<BPP>(org, cd.ox + x0, cd.oy + y0);
        const uint8_t *pr = rec_l + (y0 * W + x0) * BPP;
        if (qa.dist_kind == R1_DIST_WSSE)
          acc = r1dist::tile_scaled_dist<BPP, 2>(po, (size_t)org.stride * BPP, pr, (size_t)W * BPP, kw, kh,
                                                 cd.ox + x0, cd.oy + y0, qa.scales, qa.scale_stride,
                                                 qa.xdec, qa.ydec, BD);
        else
          acc = r1dist::tile_scaled_dist<BPP, 3>(po, (size_t)org.stride * BPP, pr, (size_t)W * BPP, kw, kh,
                                                 cd.ox + x0, cd.oy + y0, qa.scales, qa.scale_stride,
                                                 qa.xdec, qa.ydec, BD);
      }
      }
      if (!(TAIL_DEFER && tail_defer)) {   // wave-uniform
        acc = xor_sum_u64(acc, P);
        if (live_st && c == 0) qa.pix_dist[oslot] = qa.dist_kind == R1_DIST_WSSE ? (acc + 32) / 64 : acc;
      }
    }
  }
  if constexpr (!MT) break;
  gmask &= gmask - 1;
  } while (gmask != 0);
  if constexpr (!MT) break;
  } while (rem != 0);
  if constexpr (TAIL_DEFER) {
    // the fixed-point tails of cdef_dist_kernel (ssim boost, 64-bit arithmetic, ~120 instructions): inside the loop
    // they ran once per type with ONE lane of a candidate's eight alive; here lane j runs the tail of type j --
    // one pass for all (up to seven) types of the candidate
    if (tail_defer && col_live && c < qa.nt) {
      const unsigned long long d = r1dist::cdef_tile_tail<BD>(tail_keep, 64, cd.ox, cd.oy, qa.scales, qa.scale_stride, BD);
      if (live_st) qa.pix_dist[cand * (long long)qa.nt + c] = d;
    }
  }
}

template <int BD, int WL, int HL, int QM, bool MT, int PS = 0>
int launch(const R1Plane &org, const R1Plane &ref, const R1RdoCand *cands, int n,
           uint32_t *sad, uint32_t *satd, void *coeffs, void *pred, const RdoQuantArgs *qa,
           hipStream_t st, const RdoIntraArgs *ia = nullptr) {
  constexpr int NC = RdoCandPlan<BD, WL, HL, QM, MT, PS>::NC;
  typedef typename std::conditional<BD == 8, int16_t, int32_t>::type CT;
  const unsigned grid = xcd_grid((unsigned)((n + NC - 1) / NC));
  if constexpr (PS == 1)
    hipLaunchKernelGGL((k_rdo_cand<BD, WL, HL, CT, QM, MT, 1>), dim3(grid), dim3(64), 0, st,
                       org, ref, cands, n, sad, satd, (CT *)coeffs, pred, *qa, *ia);
  else
    hipLaunchKernelGGL((k_rdo_cand<BD, WL, HL, CT, QM, MT>), dim3(grid), dim3(64), 0, st,
                       org, ref, cands, n, sad, satd, (CT *)coeffs, pred, qa ? *qa : RdoQuantArgs{}, RdoNoIntraArgs{});
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// one (bit depth, QM) slice: tx_size -> instantiation
template <int BD, int QM, bool MT, int PS = 0>
int slice(int tx_size, const R1Plane &org, const R1Plane &ref, const R1RdoCand *cands, int n,
          uint32_t *sad, uint32_t *satd, void *coeffs, void *pred, const RdoQuantArgs *qa,
          hipStream_t st, const RdoIntraArgs *ia = nullptr) {
  // the transform sizes this slice instantiates: rdo_cand_instantiated (rdo_cand_plan.hpp)
#define R1_RC_CASE(ID, WL, HL)                                                                   \
  case ID:                                                                                       \
    if constexpr (rdo_cand_instantiated(BD, WL, HL, QM, MT, PS))                                  \
      return launch<BD, WL, HL, QM, MT, PS>(org, ref, cands, n, sad, satd, coeffs, pred, qa, st, ia); \
    else                                                                                         \
      break;
  switch (tx_size) {
#ifdef R1_HEADLINE_ONLY   // experiment builds (tools/build_variant.sh): the headline instantiations only
    R1_TX_SIZES_HEADLINE(R1_RC_CASE)
#else
    R1_TX_SIZES(R1_RC_CASE)
#endif
  }
#undef R1_RC_CASE
  return R1_EINVAL;
}

}  // namespace

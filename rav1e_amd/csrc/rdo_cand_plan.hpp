// rdo_cand_plan.hpp -- the compile-time plan of the fused candidate kernel (k_rdo_cand, rdo_cand_kernel.hpp), stated
// once: which (bit depth, size, QM, MT, PS) have an instantiation, which route an intra call takes, the waves per SIMD
// each instantiation asks for, and RdoCandPlan -- the geometry, the choices and the LDS layout of one instantiation.
// No device code and nothing of HIP: the kernel, its launcher, the host unit (rdo_cand.hip) and a host-only test
// (tests/test_rdo_plan.py, against the LDS sizes of the built library) all read this one header.
#pragma once
#include <cstdint>
#include <type_traits>

#include "mc_window.hpp"

// QM: 0 = coefficients to HBM (headline), 1 = + quantizer, tx-domain distortion,
// rate (N4), 2 = + quantizer, inverse transform, pixel-domain distortion.
// Waves per SIMD the register allocator is asked to make room for (0 = no request).  Only
// where the kernel sits a few registers above an allocation step (512 / n, in eights) and
// the step costs no spill worth mentioning -- measured, see DESIGN.md 5.1 "occupancy".
constexpr int rdo_waves_hint(int bd, int wl, int hl, int qm, bool mt = false) {
  // the type-search instantiations (see the MT loop of k_rdo_cand): their own steps
  if (mt) {
    // what the straight-line kernels are asked for leaves the loop with 50-350 B of scratch per lane, and at
    // thousands of waves in flight that is traffic to the Infinity Cache: same-box A/B (r05_ab_notes.md, ab1)
    // 16x16 fan-out 0.754 -> 0.610 ms (8-bit), 0.855 -> 0.602 (10-bit), 10-bit 8x8 0.655 -> 0.553 at the steps below
    if (wl <= 3 && hl <= 3) return qm == 2 ? (bd == 8 ? 7 : 6) : 1;
    return qm == 2 ? 4 : 1;
  }
  // (10-bit 64x64 sits at 165 VGPRs, 3 waves; asked for 4: 152 B of spills, launch 0.281 -> 0.365 ms)
  if (wl == 5 && hl == 5 && qm == 0 && bd != 8) return 6;   // 89 -> 80 VGPRs, no spill: 5 -> 6 waves, launch -1.7 % (ab7)
  // the pixel-domain chain sat a few registers above an allocation step at three sizes; asked for the
  // step, the allocator gets there without a spill worth mentioning (same-box, r04_ab_notes.md ab8:
  // 8-bit 290.3 -> 295.0 k, 10-bit 274.2 -> 283.5 k)
  if (wl == 3 && hl == 3 && qm == 2) return 8;   // 73 / 74 VGPRs -> 58 / 62: 6 -> 8 waves, launch -2.2 / -3.7 % (10-bit at 7: 72 VGPRs, -1.6 %; ab13)
  if (wl == 4 && hl == 4 && qm == 2) return bd == 8 ? 6 : 5;   // 105 / 107 -> 80 + 44 B scratch / 94: 4 -> 6 / 5 waves, -6 / -5.1 % (10-bit at 6: 68 B of scratch, +1 %; ab13)
  if (wl == 5 && hl == 5 && qm == 2) return 4;              // 8-bit 132 -> 128; 10-bit 131 -> 128 (8 B of scratch): 3 -> 4 waves, -5.4 %
  if (wl == 5 && hl == 5 && qm == 1) return 5;              // 8-bit 97 -> 96; 10-bit 120 -> 96 (20 B of scratch): 4 -> 5 waves, launch -4 % (ab10)
  if (wl == 6 && hl == 6 && qm == 2) return bd == 8 ? 4 : 3;   // 8-bit: 168 -> 128 + 64 B of scratch, launch -2.9 %; 10-bit at 4: +14 % (ab12) -> 3: 181 -> 168
  return 1;
}

// ---- which instantiations exist, which route a call takes ----
// A transform size is (wl, hl) = log2 of its sides: the 19 sizes of AV1 have sides 4 .. 64 at a ratio up to 4.
constexpr bool rdo_tx_size_exists(int wl, int hl) {
  return wl >= 2 && wl <= 6 && hl >= 2 && hl <= 6 && wl - hl <= 2 && hl - wl <= 2;
}
// The sizes whose transform-type search is ONE launch of the fan-out (MT) kernel: both sides up to 16, the nine
// TxSize ids 0-2, 5-8, 13, 14 (as a mask over the ids: 0x61E7).  A 64-point side has TX_SET_DCTONLY (get_tx_set,
// src/context/transform_unit.rs:123-131) and a 32-point side DCT_DCT (+ IDTX for inter blocks): one or two types,
// which the plain kernel evaluates at twice the occupancy, one launch per type (same-box A/B,
// profiles/r05_ab_notes.md: the 32x32 fan-out kernel held 2 waves per SIMD and LOST 13-22 % against two launches)
constexpr bool rdo_type_fanout(int wl, int hl) { return wl <= 4 && hl <= 4; }
// Where the launch with the prediction made on the CU lost to r1_predict_intra_batch -> r1_rdo_txsearch_batch(pred)
// by more than the +-3-4 % between boxes (profiles/r12_intra_cand.jsonl, 4K luma, 4 modes per block): those points
// take the two launches inside r1_rdo_intra_cand_batch and have no intra instantiation.  Measured at 8 and 10
// bits; 12 bits is the 10-bit code at another constant and follows it, R1_DIST_WSSE shares the chain up to the
// distortion with R1_DIST_CDEF and follows it.  qm: 1 = dist_kind 0, 2 = a pixel-domain kind.
//   16x16, dist_kind 0                 +11.5 % (8-bit), +10.9 % (10-bit)
//   16x16, pixel kinds, 16-bit pixels  +3.6 % (two runs)
//   64x64, dist_kind 0, 16-bit pixels  +13 %
//   32x32, pixel kinds, 16-bit pixels  +4.3 %
constexpr bool r1_intra_two_launch(int wl, int hl, int bd, int qm) {
  return wl == hl && ((wl == 4 && (qm == 1 || bd != 8)) || (wl == 6 && qm == 1 && bd != 8) ||
                      (wl == 5 && qm == 2 && bd != 8));
}
// The route of an r1_rdo_intra_cand_batch call: the fan-out kernel with the prediction made on the CU (it serves any
// mask, a single type included), one plain launch per type with the prediction made again in each, or the two
// launches above.
enum RdoIntraRoute { RDO_INTRA_FANOUT, RDO_INTRA_PER_TYPE, RDO_INTRA_TWO_LAUNCH };
constexpr RdoIntraRoute rdo_intra_route(int wl, int hl, int bd, int qm) {
  return r1_intra_two_launch(wl, hl, bd, qm) ? RDO_INTRA_TWO_LAUNCH
                                             : (rdo_type_fanout(wl, hl) ? RDO_INTRA_FANOUT : RDO_INTRA_PER_TYPE);
}
// Whether k_rdo_cand<bd, wl, hl, ., qm, mt, ps> is instantiated (slice<> of rdo_cand_kernel.hpp): the plain kernels
// (PS = 0, MT off) at every size and QM, 19 x 3 bit depths x 3 = 171; the type search's (MT) where it fans out,
// 9 x 3 x 2 QM = 54; the intra prediction source (PS = 1) in the form its route names -- fan-out for those nine sizes,
// plain for the other ten, none where the call takes the two launches -- 105.
constexpr bool rdo_cand_instantiated(int bd, int wl, int hl, int qm, bool mt, int ps) {
  if (!(bd == 8 || bd == 10 || bd == 12) || !rdo_tx_size_exists(wl, hl) || qm < 0 || qm > 2 || ps < 0 || ps > 1)
    return false;
  if (ps == 1)
    return qm != 0 && rdo_intra_route(wl, hl, bd, qm) == (mt ? RDO_INTRA_FANOUT : RDO_INTRA_PER_TYPE);
  return !mt || (qm != 0 && rdo_type_fanout(wl, hl));
}

// Whether an instantiation votes on its wave's transform types before phase C and takes the switch between the 1-D
// kernels as a scalar branch when they agree (TX_VOTE, rdo_cand_kernel.hpp).  Only where the type is a per-lane
// value from the descriptors: the coefficient kernels (QM 0).  The quantizer chains take the type from a kernel
// argument whenever the caller gives a mask, the type search (MT) and the intra prediction source always do; a
// 64-point side admits only DCT_DCT.  Those instantiations keep their code.  So do the sizes with a 32-point side,
// which has one kernel and the identity, nothing to switch between: with the vote the 8-bit 32x32 launch was not
// faster (+0.2 %, inside the spread), the 16-bit 32x32 kernel, held at 80 VGPRs by rdo_waves_hint, spilled 20 B per
// lane, and 8x32 / 32x8 / 16x32 / 32x16 lost one to three waves per SIMD (profiles/r16_txuniform_notes.md).
constexpr bool rdo_tx_vote(int wl, int hl, int qm, bool mt, int ps) {
  return qm == 0 && !mt && ps == 0 && wl <= 4 && hl <= 4;
}

// Whether an instantiation's column pass (phase C) runs the column family of the 1-D networks (fwd_col_m24,
// tx_common.hpp: unshifted residuals in, shift[1] already applied on the way out) instead of shift[0], the plain
// network and shift[1].  At 12 bits shift[0] is 0 and there is nothing pending.  Elsewhere the family is taken only
// where its launch was measured faster, every folded pass against every plain pass of a same-box A/B, in two
// sessions (profiles/r19_colfold_notes.md): the coefficient kernels at 8x8 / 16x16 / 32x32 (8 bits -1.6 / -2.0 /
// -1.0 %) and 16x16 / 32x32 (10 bits -1.1 / -1.6 %), and the 8-bit transform-domain chain at 8x8 / 16x16 (-1.4 %
// each).  Measured and not faster, so on the plain column with the code they had: 64x64 at both depths (8 bits: 95
// VALU instructions fewer per wave, 2.3 %, and the launch within +-0.4 % -- what identical kernels differ by between
// two builds), 10-bit 8x8, the 8-bit QM 1 chain at 32x32 / 64x64 (+0.3 / +1.3 %), the 8-bit pixel-domain chain at
// every size (+0.7 % at 64x64).  Not measured, so on the plain column too: the rectangular sizes, 4x4, the type
// search (MT), the intra prediction source and the 10-bit quantizer chains; of those, 20 would also have lost a
// waves-per-SIMD step or gained scratch (tools/kres.py).
constexpr bool rdo_col_fold(int bd, int wl, int hl, int qm, bool mt, int ps) {
  if (mt || ps != 0 || wl != hl) return false;
  if (bd == 8) return qm == 0 ? (wl >= 3 && wl <= 5) : (qm == 1 && (wl == 3 || wl == 4));
  return bd == 10 && qm == 0 && (wl == 4 || wl == 5);
}

// Whether an instantiation's forward networks, both passes, halve toward zero in two instructions (m24h, tx_common.hpp:
// exact while the operand is below 2^24, and every halving operand of a chain fed from pixels is below 2^18.01), and
// whether its 8-bit motion compensation packs the horizontal accumulators without shifting them (mc8_column_t<..,
// PACK4>, cand_common.hpp).  Both are exact; like COL_FOLD each is on only where its launch was measured faster than
// the parent's on one box, in four sessions of alternated passes (profiles/r20_halve_pack_notes.md).  Candidates were
// the coefficient kernels (QM 0) of the square sizes 8x8 .. 64x64: the halving at 8 and 10 bits, the pack at 8 bits.
//   halving, 8 bits    64x64 / 32x32 / 16x16 / 8x8 launches -3.1 / -3.7 / -2.4 / -1.3 %
//   halving, 10 bits   64x64 / 16x16 -1.8 / -1.9 %.  32x32 measured -3.7 % but the kernel, held at 80 VGPRs by
//                      rdo_waves_hint, gains 8 B of scratch per lane: off (tools/kres.py).  8x8: inside the spread, off.
//   pack, on the halving   32x32 / 16x16 / 8x8 a further -0.3 .. -0.9 %; 64x64 nothing in any session: off there.
// Nothing else was measured, so the quantizer chains, the type search, the intra prediction source, the rectangles, 4x4
// and 12 bits keep the code they had.
constexpr bool rdo_plain_square(int wl, int hl, int qm, bool mt, int ps) {
  return qm == 0 && !mt && ps == 0 && wl == hl && wl >= 3 && wl <= 6;
}
constexpr bool rdo_halve2(int bd, int wl, int hl, int qm, bool mt, int ps) {
  if (!rdo_plain_square(wl, hl, qm, mt, ps)) return false;
  return bd == 8 || (bd == 10 && (wl == 4 || wl == 6));
}
constexpr bool rdo_mc_pack4(int bd, int wl, int hl, int qm, bool mt, int ps) {
  return bd == 8 && rdo_plain_square(wl, hl, qm, mt, ps) && wl <= 5;
}
// Whether an instantiation's forward networks, both passes, keep their multiplies' products at scale 2^16 where the
// factor's bound allows (m24w, tx_common.hpp: exact while |a| (M << (16 - s)) + 2^15 < 2^31), so that an add or a
// subtract reads the product's high word and the rounding shift is not executed.  rdo_mul_hiword_built: the
// instantiations the form is stated, bounded and tested for -- the 8-bit coefficient kernels of the square sizes, the
// family of HALVE2, whose halving the form keeps.  rdo_mul_hiword: those of them that ship.
// rdo_mul_col_bound / rdo_mul_row_bound: the bound B of the inputs' magnitude each pass hands to the networks --
// columns: the unshifted residual where the column family runs (COL_FOLD), residual << shift[0] elsewhere; rows: the
// column outputs after shift[1], the largest over the transform types the size admits (tools/tx_range.py
// chain_input_bounds(): 8x8 5774, 16x16 8164, 32x32 5776, 64x64 16334; tests/test_tx_mul_hiword.py holds the header
// to them).  At those bounds every multiply of the column networks takes the form but 24 of fdct64's 191; of the
// row networks' all of fdct8 / fdst8, 27 of 31 (fdct16), 42 of 48 (fdst16), 70 of 81 (fdct32), 87 of 191 (fdct64).
// Measured like HALVE2 / MC_MATRIX, the parent's library against this one on one box per session, three sessions of four
// to five alternated passes (profiles/r24_mul_hiword_notes.md): 64x64 launch -4.9 / -4.5 / -4.7 %, 32x32 -6.7 / -6.4 /
// -6.6 %, 16x16 -5.5 / -5.3 / -5.4 %, 8x8 -1.6 / -1.2 / -1.4 %, every pass below every parent pass: all four ship.
// SQ_INSTS_VALU per wave 3839 -> 3614, 1706 -> 1560, 769 -> 713, 445 -> 418; registers 118 -> 115 at 64x64 and as before
// elsewhere, LDS and waves per SIMD as before, no scratch (tools/kres.py).
constexpr bool rdo_mul_hiword_built(int bd, int wl, int hl, int qm, bool mt, int ps) {
  return bd == 8 && rdo_plain_square(wl, hl, qm, mt, ps);
}
constexpr bool rdo_mul_hiword(int bd, int wl, int hl, int qm, bool mt, int ps) {
  return rdo_mul_hiword_built(bd, wl, hl, qm, mt, ps);
}
constexpr int rdo_mul_col_bound(int bd, int sh0, bool col_fold) { return ((1 << bd) - 1) << (col_fold ? 0 : sh0); }
constexpr int rdo_mul_row_bound(int bd, int wl, int hl) {
  return bd == 8 && wl == hl ? (wl == 3 ? 5774 : wl == 4 ? 8164 : wl == 5 ? 5776 : wl == 6 ? 16334 : 0) : 0;
}
// Whether an instantiation's 8-bit motion compensation runs its horizontal 8-tap pass on the matrix pipe
// (mc8_column_t<.., MXNC>, cand_common.hpp; the fragment geometry is r1mc::mx_*, mc_window.hpp): a quad of window
// rows is one 8-byte LDS read and one v_mfma_i32_16x16x32_i8 per candidate of the wave instead of twelve v_dot4 on
// twelve LDS dwords, every lane receives the accumulators of its own column, and the pack and the vertical pass stay
// as they are.  Candidates are the family of HALVE2 / MC_PACK4.  Built for 64x64 (one candidate per wave) and 32x32
// (two: two chained MFMAs, the other candidate's row groups read a zeroed shadow behind the source block); 16x16 and
// 8x8 (four and eight tap sets per wave) have no layout in this form -- theirs is rdo_mc_matrix4, below -- and everything
// else keeps the v_dot4 pass.
// Measured like COL_FOLD / HALVE2, the parent's library against this one on one box, three sessions of alternated passes
// (profiles/r22_mc_matrix_notes.md): 64x64 launch -8.2 %, 32x32 -4.2 %, every pass below every parent pass;
// SQ_INSTS_VALU per wave 4069 -> 3839 and 1772 -> 1706, a third of the LDS instructions gone; registers, LDS and waves
// per SIMD as before (tools/kres.py).
constexpr bool rdo_mc_matrix(int bd, int wl, int hl, int qm, bool mt, int ps) {
  return bd == 8 && rdo_plain_square(wl, hl, qm, mt, ps) && wl >= 5;
}
// The same pass for the waves of four and eight candidates, on v_mfma_i32_4x4x4_16b_i8 (mc8_column_t<.., MX4>,
// cand_common.hpp; geometry r1mc::mx4_*, mc_window.hpp): sixteen independent 4x4x4 blocks, each four adjacent columns of
// one candidate with that candidate's taps, so a quad of window rows is three chained MFMAs on three LDS dwords of the
// lane's own window instead of twelve v_dot4 on twelve, with no shadow and no band builder.  rdo_mc_matrix4_layout: the
// sizes the layout is stated and checked for (the 8-bit QM 0 plain squares 16x16 and 8x8); rdo_mc_matrix4: those of them
// that ship, each only where its launch was measured faster than the parent's.  Both are on.  Measured like MC_MATRIX,
// the parent's library against this one on one box per session, three sessions of four to five alternated passes
// (profiles/r23_mc_matrix4_notes.md): 16x16 launch -6.7 / -6.1 / -6.5 %, 8x8 -4.4 / -3.8 / -3.8 %, every pass below every
// parent pass; SQ_INSTS_VALU per wave (MFMAs included) 810 -> 769 and 468 -> 445, 18 / 12 MFMAs per wave, SQ_INSTS_LDS
// -25 / -29 %; 50 -> 53 and 40 -> 42 VGPRs, LDS as before, no scratch, 8 waves per SIMD as before (tools/kres.py).
constexpr bool rdo_mc_matrix4_layout(int bd, int wl, int hl, int qm, bool mt, int ps) {
  return bd == 8 && rdo_plain_square(wl, hl, qm, mt, ps) && (wl == 4 || wl == 3);
}
constexpr bool rdo_mc_matrix4(int bd, int wl, int hl, int qm, bool mt, int ps) {
  return rdo_mc_matrix4_layout(bd, wl, hl, qm, mt, ps) && (wl == 4 || wl == 3);
}

// ---- one instantiation: geometry, choices, LDS layout ----
// PS: where the prediction comes from -- 0 = put_8tap of the reference window (or the dense qa.pred_in buffer),
// 1 = intra prediction from the candidate's edge set.  One wave per workgroup; a wave owns NC candidates.
template <int BD, int WL, int HL, int QM, bool MT, int PS>
struct RdoCandPlan {
  static constexpr int BPP = BD == 8 ? 1 : 2;
  static constexpr bool INTRA = PS == 1;
  static constexpr int W = 1 << WL, H = 1 << HL;
  static constexpr int P = W > H ? W : H, NC = 64 / P;
  static constexpr int TS = (W < H ? W : H) == 4 ? 4 : 8;
  static constexpr bool COL_FOLD = rdo_col_fold(BD, WL, HL, QM, MT, PS);
  static constexpr bool HALVE2 = rdo_halve2(BD, WL, HL, QM, MT, PS);
  static constexpr bool MC_PACK4 = rdo_mc_pack4(BD, WL, HL, QM, MT, PS);
  static constexpr bool MUL_HW = rdo_mul_hiword(BD, WL, HL, QM, MT, PS);
  static_assert(!MUL_HW || (HALVE2 && rdo_mul_row_bound(BD, WL, HL) > 0), "m24w keeps m24h's halving; a stated row bound");
  static constexpr int WS = r1mc::window_stride(W, BPP);
  // INTRA: no reference window.  The candidate's edge arrays (raw edge + the four filter / upsample arrays, FL
  // entries each) take its place and may lie over the WHOLE allocation: the source block waits in registers until
  // the prediction is made (see SRC_LATE) and nothing else of the chain is alive yet.
  static constexpr int WIN_BYTES = INTRA ? 0 : NC * (H + 7) * WS;
  static constexpr int FL = 2 * (W + H) + 1;               // entries of one edge array
  static constexpr int EDGE_BYTES = INTRA ? ((NC * 5 * FL * 2 + 15) & ~15) : 0;
  // The transpose tile holds the column pass's outputs after shift[1]: bounded by 16353 at 8-bit
  // (every size and type) and by 23214 at 10-bit with sides up to 32 (tools/tx_range.py: pixel range,
  // shift[0], the L1 gain of the column network, shift[1]), so int16 holds them exactly.  Used for
  // 10-bit 32x32 only, together with SRC_LATE below: tile 8320 -> 4224 B, window + source 10336 ->
  // 6240 B, 4 -> 5 waves per SIMD, launch 0.252 -> 0.237 ms (profiles/r04_ab_notes.md).  At 8-bit
  // 32x32 the same change (5 -> 6 waves) made the launch 1.5 % SLOWER -- that kernel is not short of
  // waves -- and is off.  Row stride 66 int16 = 33 dwords: a candidate's row lanes read 32 banks.
  // The type search's shared tile (COLSHARE, below) is int16 at every bit depth: with both sides <= 16 the column
  // pass's output after shift[1] is bounded by 8193 / 16433 / 16445 at 8 / 10 / 12 bits (tests/test_tx_range.py).
  static constexpr bool TB16 = (BD == 10 && WL == 5 && HL == 5) || (MT && W <= 16 && H <= 16);
  typedef typename std::conditional<TB16, int16_t, int32_t>::type TB;   // the tile's element
  static constexpr int LSTRIDE = NC * W + (TB16 ? 2 : 1);
  static constexpr int ISTRIDE = NC * W + 1;       // the inverse transform's row buffer (QM == 2): int32
  // 64x64: the transpose goes through LDS in two halves of 32 rows (8.3 KB instead of
  // 16.6 KB per wave).  At 16.6 KB the CU held 9 waves where the registers allow 12, and
  // this kernel lives on occupancy: a wave issues one instruction per ~10 cycles whatever
  // the size, so the SIMD's throughput is proportional to the waves it holds.
  static constexpr bool SPLIT_T = W == 64 && H == 64;
  static constexpr int TXB_ROWS = SPLIT_T ? 32 : H;
  static constexpr int TXB_BYTES = TXB_ROWS * LSTRIDE * (int)sizeof(TB);
  static constexpr int IRB_BYTES = QM == 2 ? (H < 32 ? H : 32) * ISTRIDE * 4 : 0;
  // The quantizer's coded-area tile, one per candidate, P dwords of padding between candidates: at the bare
  // stride (64 / 128 / 256 dwords for 8x8 .. 16x16) the NC candidates of a lane group wrote, gathered and read
  // back the same banks (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.36 / 0.26 of the pixel chain's 8x8 / 16x16
  // launches, profiles/r04_v5_pmc_pixel_summary.json); the forward kernel's TPAD, carried over
  // (two candidates per wave sit in different 32-lane groups and never meet in a bank: no padding there --
  // with it the 10-bit 32x32 launch was 2.8 % slower, r05_ab_notes.md ab2)
  static constexpr int QT_PAD = NC > 2 ? P : 0;
  static constexpr int QT_STRIDE = (W < 32 ? W : 32) * (H < 32 ? H : 32) + QT_PAD;
  static constexpr int QT_BYTES = QM != 0 ? NC * QT_STRIDE * 4 : 0;
  // QM == 2 (pixel-domain leg): only the coded area (32 x 32 of a 64-point side) is quantized, and there is no
  // `tail` energy to sum (encoder.rs:1617-1640 computes it only when rdo_type.needs_tx_dist()), so vertical
  // frequencies >= 32 are never read: the column pass does not store them -- the compiler then prunes the
  // fdct64 network down to the outputs that are (its upper-half outputs are dead) -- and the row pass runs
  // on rows 0 .. 31 only; horizontal frequencies >= 32 die the same way inside the row lanes
  static constexpr int HU = (QM == 2 && H > 32) ? 32 : H;   // vertical frequencies that are used
  static constexpr int REC_BYTES = QM == 2 ? NC * W * H * BPP : 0;
  // The source block is staged in LDS next to the window (16-byte row chunks: H*W*BPP/1024
  // load instructions per wave instead of H one-pixel-per-lane loads) and read back column by
  // column AFTER the motion compensation: the H source registers are not live across the
  // filter any more.  Not for 64-wide 16-bit blocks: + 8 KB of LDS would cost a wave per SIMD.
  static constexpr bool SRC_LDS = BPP == 1 || P <= 32;
  // SRC_LATE: the source chunks wait in registers (SPASS x 4 VGPRs) while the window is filtered and
  // go to LDS afterwards, OVER the dead window -- window + source side by side (10336 B at 10-bit
  // 32x32) held the CU at 15 waves (4 per SIMD after rounding); with the source over the window the
  // footprint is the window's 6240 B and the ~93 VGPRs allow 5.
  // 16-bit 16x16, headline only (the pixel chain keeps its source block in LDS for the distortion,
  // SRC_KEEP below): 6592 -> 4416 B, 6 -> 8 waves, launch 0.2255 -> 0.217 ms (r04_ab_notes.md, ab7)
  static constexpr bool SRC_LATE0 = SRC_LDS && BD != 8 && (P == 32 || (P == 16 && QM == 0));
  static constexpr int SRC_ROW = W * BPP;
  static constexpr int WIN_PAD = (WIN_BYTES + 15) & ~15;
  // A candidate's source block starts max(16, row bytes) past a multiple of its own size: with the bare
  // stride (16 / 32 / 64 / 128 dwords) the column reads of the NC candidates of a lane group hit the SAME
  // banks with different addresses -- 2-way at 8-bit 8x8 and at 16x16, 4-way at 10-bit 8x8: this, not the
  // window staging, was the SQ_LDS_BANK_CONFLICT of those launches (0.18 / 0.30 of the LDS cycles)
  static constexpr int SRC_CSTRIDE = H * SRC_ROW + (NC > 1 ? (SRC_ROW > 16 ? SRC_ROW : 16) : 0);
  static constexpr int SRC_BYTES = SRC_LDS ? NC * SRC_CSTRIDE : 0;
  // SRC_KEEP (pixel-domain chain, blocks up to 16 rows): the staged source block sits BEHIND the work area
  // that the later phases alias (transpose tile, quantizer tile, row buffer), so the distortion at the end of
  // the chain reads its source column from LDS again instead of issuing H more global loads per lane
  static constexpr bool SRC_KEEP = QM == 2 && H <= 16 && SRC_LDS && !SRC_LATE0;
  // INTRA: the source always goes to LDS after the prediction (to its SRC_KEEP place behind the work area, or over
  // the dead edge arrays)
  static constexpr bool SRC_LATE = INTRA ? SRC_LDS && !SRC_KEEP : SRC_LATE0;
  static constexpr int WS_BYTES =
      SRC_KEEP ? WIN_PAD : (SRC_LATE ? (WIN_PAD > SRC_BYTES ? WIN_PAD : SRC_BYTES) : WIN_PAD + SRC_BYTES);
  static constexpr int LDS_A0 = WS_BYTES > TXB_BYTES ? WS_BYTES : TXB_BYTES;
  static constexpr int LDS_A = LDS_A0 > IRB_BYTES ? LDS_A0 : IRB_BYTES;
  // SATD_T: the horizontal half of the SATD in registers, through a tile in LDS (cand_common.hpp, satd_tile_store /
  // satd_tile_rows): H / 2 rows of W packed dwords per candidate, P dwords between candidates (the bare strides are
  // multiples of the bank count, as with QT_PAD).  The tile lies at the start of the work area, over the window and
  // the source block -- dead once the residual and the SAD are formed; a kept source block (SRC_KEEP) sits behind
  // LDS_WORK and is not touched -- and is taken only where it fits what phases A, C and F need anyway: no
  // instantiation's LDS grows, an instantiation it does not fit stays on the lane stages (satd_column).  So does the
  // 64x64 pixel-domain chain: it is held at an allocation step below its need (rdo_waves_hint) and its spills grew
  // with the tile path (8-bit 68 -> 76 B, 10-bit 100 -> 116 B of scratch per lane).
  static constexpr int SATD_STRIDE = W * H / 2 + (NC > 1 ? P : 0);
  static constexpr int SATD_BYTES = NC * SATD_STRIDE * 4;
  static constexpr bool SATD_T = TS == 8 && BD <= 10 && (W < H ? W : H) >= 16 && SATD_BYTES <= LDS_A &&
                                 !(QM == 2 && WL == 6 && HL == 6);
  static_assert(SATD_STRIDE % 4 == 0, "16-byte reads stay aligned");
  static constexpr int LDS_B = QT_BYTES > REC_BYTES ? QT_BYTES : REC_BYTES;
  static constexpr int LDS_WORK = ((LDS_A > LDS_B ? LDS_A : LDS_B) + 15) & ~15;
  static constexpr int SRC_OFF = SRC_KEEP ? LDS_WORK : (SRC_LATE ? 0 : WIN_PAD);
  // MT, COLSHARE: the transposed output of the column pass in a tile of its own behind everything else -- the later
  // phases of a type alias the work area, and the types that share a column kernel (the seven RAV1E types use three:
  // DCT x3, ADST x2, identity x2) all read their rows from this one tile (see the type loop)
  static constexpr bool COLSHARE = MT && !SPLIT_T;
  static constexpr int TKEEP_OFF = (LDS_WORK + (SRC_KEEP ? SRC_BYTES : 0) + 15) & ~15;
  static constexpr int LDS_CHAIN =
      COLSHARE ? TKEEP_OFF + H * LSTRIDE * (int)sizeof(TB) : LDS_WORK + (SRC_KEEP ? SRC_BYTES : 0);
  static constexpr int LDS_BYTES = LDS_CHAIN > EDGE_BYTES ? LDS_CHAIN : EDGE_BYTES;
  // MC_MATRIX (rdo_mc_matrix): the horizontal pass on the matrix pipe.  MX_NC = candidates per wave there, 0 where it
  // is off.  With two candidates the zeroed shadow (MX_ZERO_BYTES at MX_ZERO_OFF) lies behind the staged source block,
  // inside what the transpose tile needs anyway; phase A clears it and nothing writes there until every lane has
  // filtered its column.  No instantiation's LDS grows: what the fragments read lies inside LDS_BYTES.
  static constexpr bool MC_MATRIX = rdo_mc_matrix(BD, WL, HL, QM, MT, PS);
  static constexpr int MX_NC = MC_MATRIX ? NC : 0;
  static constexpr int MX_ZERO_BYTES = MC_MATRIX && NC > 1 ? r1mc::mx_zero_bytes(H, WS) : 0;
  static constexpr int MX_ZERO_OFF = (WIN_PAD + SRC_BYTES + 15) & ~15;
  static_assert(!MC_MATRIX || (NC <= 2 && WS % 8 == 0 && !SRC_LATE && !SRC_KEEP && SRC_OFF == WIN_PAD),
                "the matrix pass reads aligned 8-byte fragments of one or two windows; the shadow follows the source");
  static_assert(!MC_MATRIX || r1mc::mx_a_end(NC > 2 ? 2 : NC, H, WS) <= LDS_BYTES,
                "the furthest byte an A fragment reads lies inside the allocation");
  static_assert(!MC_MATRIX || MX_ZERO_OFF + MX_ZERO_BYTES <= LDS_BYTES, "the zeroed shadow lies inside the allocation");
  // MC_MATRIX4 (rdo_mc_matrix4): the pass on sixteen 4x4x4 blocks, every lane on its own window.  MX4_A_END = one past
  // the furthest byte a fragment reads (the row past H + 6 of the last candidate's last quad: in the staged source
  // block), stated for every size the layout covers whether it ships or not.  Nothing is added to any allocation.
  static constexpr bool MC_MATRIX4 = rdo_mc_matrix4(BD, WL, HL, QM, MT, PS);
  static constexpr int MX4_A_END = rdo_mc_matrix4_layout(BD, WL, HL, QM, MT, PS) ? r1mc::mx4_a_end(NC, W, H, WS) : 0;
  static_assert(!MC_MATRIX4 || !MC_MATRIX, "one matrix form per instantiation");
  static_assert(MX4_A_END == 0 || (NC * W == 64 && W % 4 == 0 && WS % 4 == 0 && WS >= W + 8 && !SRC_LATE),
                "lane = (candidate, column) with no idle lane; a block is four columns of one candidate; its three "
                "dwords stay inside the row");
  static_assert(MX4_A_END <= LDS_BYTES, "the furthest byte an A fragment reads lies inside the allocation");
};

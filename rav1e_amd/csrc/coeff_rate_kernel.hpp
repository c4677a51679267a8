// coeff_rate_kernel.hpp -- the device half of the coefficient-rate unit (its entry points: coeff_rate.hip): the three
// rate kernels on one per-transform-block body (txb_rate), one update_cdf, one snapshot load and one plane walk; the
// whole-block body (block_trial) once more on a device-resident R1CoeffCdfContext that it leaves adapted
// (k_coeff_cdf_adapt), and the copy that cuts a snapshot out of such a context (k_coeff_cdf_slice).
//
// One wave per slot, four slots per workgroup.  Inside a slot, per transform block (txb_rate, stated once):
//  A  (parallel over the coded area) txb_init_levels: min(|c|, 127), transposed, stride H + TX_PAD_HOR, in LDS.
//  then, per chunk of 256 scan positions, from eob - 1 down (the order encode_coeffs codes them in):
//  1  (parallel, four positions per lane) get_nz_map_ctx / the eob context, get_br_ctx and the symbol count of
//     each position -> a 16-bit token and, by a wave prefix sum, the index of its first symbol in the chunk.
//  2  (parallel over CDF rows) the only rows a slot hits more than once are coeff_base (42) and coeff_br (21):
//     lane l < 42 keeps coeff_base[l], lane 42 + r keeps coeff_br[r] in registers, walks the chunk's tokens and,
//     for those of its row, emits (fl, fh, nms) from its adapting copy (update_cdf, src/ec.rs:935-955) at the
//     symbol's index.  txb_skip, tx_type, eob_flag, eob_extra, coeff_base_eob and dc_sign are hit once per
//     transform block: a single-block slot reads them from the snapshot as they stand, the chain from its LDS copy,
//     which it updates behind every use.
//  3  (serial) the chain over (fl, fh, nms) through rng and bits (lr_compute + leading_zeros), run by every lane
//     on the same values: a dozen instructions per symbol, no divergence.
//  then encode_coeff_signs, in chunks from scan position 0 up: the values gathered in parallel, the sign bits,
//  the DC sign symbol and the Golomb tails chained serially (they depend on rng only).
// Every loop bound is eob <= area, the four base-range rounds or the Golomb length <= 32; no spin-waits, no
// atomics, no dependence between workgroups.  `cdfs` is never written; k_coeff_cdf_adapt writes its trial's own context,
// which no other wave touches.
//
// Restated from the reference (pinned by tests/golden/coeff_rate_ref.npz through every fixture case):
//  tx_type_to_class, eob_to_pos_small / eob_to_pos_large, k_eob_group_start, k_eob_offset_bits, nz_map_ctx_offset_1d
//  as the closed forms below; av1_nz_map_ctx_offset by the rule of transform_unit.rs:866-876.
#pragma once
#include "common.hpp"

namespace {
constexpr int kChunk = 256;               // scan positions per chunk: four per lane
constexpr int kSymMax = kChunk * 5;       // a base symbol and at most four base-range rounds per position
constexpr int kLevelBytes = 36 * 36 + 16; // (W + TX_PAD_HOR) columns of stride H + TX_PAD_HOR, W, H <= 32
constexpr int kBaseRows = R1_SIG_COEF_CONTEXTS, kBrRows = R1_LEVEL_CONTEXTS;
static_assert(kBaseRows + kBrRows <= 63, "one lane per adapting CDF row, lane 63 for coeff_base_eob");
static_assert(R1_BR_CDF_SIZE == 4, "coeff_base and coeff_br rows are four-entry CDFs in four registers");
static_assert(sizeof(R1TxbCtx) == 4 && sizeof(R1CoeffCdfs) == 1088, "ABI layout");

struct RateArgs {
  const void *qc;
  const uint16_t *eobs;
  const R1TxbCtx *ctxs;
  const R1CoeffCdfs *cdfs;
  const uint16_t *scan[3];   // av1_scan_orders[tx_size] by kind (quantize.hip)
  uint32_t *rate;
  uint8_t *cul;
  int n_slots, nt, n_cdfs, plane;
  int w_coded, hl, area;     // coded width, log2 of the coded height, coded area
  int shape;                 // nominal w < h: 1, w > h: 2, square: 0 (av1_nz_map_ctx_offset)
  int eob_flag_n;            // 5 + eob_multi_size: the length of the eob_flag CDF
  int tx_n;                  // num_tx_set of the block's set when write_tx_type codes a symbol, else 0
  int is_inter;
  uint8_t type[16], tx_sym[16];   // per slot j: TxType, av1_tx_ind[set][type]
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// WriterBase<WriterCounter>: store = lr_compute + leading_zeros.  fl, fh arrive as their top 10 bits (>> EC_PROB_SHIFT),
// all lr_compute reads of them; fl = 32768 (the first symbol) is 512.
struct Counter {
  uint32_t rng = 0x8000, bits = 0;
  __device__ __forceinline__ void store(uint32_t flq, uint32_t fhq, uint32_t nms) {
    const uint32_t r8 = rng >> 8;
    const uint32_t u = flq >= 512 ? rng : ((r8 * flq) >> 1) + 4 * nms;
    const uint32_t v = ((r8 * fhq) >> 1) + 4 * (nms - 1);
    const uint32_t r = (u - v) & 0xffffu;
    const uint32_t d = (uint32_t)__clz((int)r) - 16;    // r == 0 (not a CDF): 16, nothing is indexed by it
    bits += d;
    rng = (r << d) & 0xffffu;
  }
  // symbol(s, cdf) on a row of the snapshot; n = the CDF's length (its last entry is the counter)
  __device__ __forceinline__ void symbol(const uint16_t *cdf, int n, int s) {
    store(s > 0 ? (uint32_t)cdf[s - 1] >> 6 : 512u, (uint32_t)cdf[s] >> 6, (uint32_t)(n - s));
  }
  __device__ __forceinline__ void bit(uint32_t b) {     // bool(b, 16384)
    if (b) store(256, 0, 1);
    else store(512, 256, 2);
  }
  __device__ __forceinline__ uint32_t tell_frac() const {   // frac_compute(tell(), rng); tell = bits + cnt + 10
    uint32_t r = rng, l = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      r = (r * r) >> 15;
      const uint32_t b = r >> 16;
      l = (l << 1) | b;
      r >>= b;
    }
    return ((bits + 1) << 3) - l;
  }
};

__device__ __forceinline__ uint32_t pack_sym(uint32_t fl, uint32_t fh, uint32_t nms) {
  return (fl >> 6) | ((fh >> 6) << 10) | (nms << 20);
}
__device__ __forceinline__ uint32_t min3(uint32_t v) { return v < 3 ? v : 3; }

// The adapting rows, one per lane: coeff_base[lane] / coeff_br[lane - 42], four entries each (the last is the counter)
struct LaneRow {
  uint32_t c0, c1, c2, cnt;
  __device__ __forceinline__ void load(const R1CoeffCdfs *cdf, int lane) {
    const uint16_t *r = lane < kBaseRows ? cdf->coeff_base[lane] : cdf->coeff_br[lane < 63 ? lane - kBaseRows : 0];
    c0 = r[0], c1 = r[1], c2 = r[2], cnt = r[3];
  }
  // the row back into a copy the lanes were loaded from (lane 63 keeps none)
  __device__ __forceinline__ void store(R1CoeffCdfs *cdf, int lane) const {
    if (lane >= 63) return;
    uint16_t *r = lane < kBaseRows ? cdf->coeff_base[lane] : cdf->coeff_br[lane - kBaseRows];
    r[0] = (uint16_t)c0, r[1] = (uint16_t)c1, r[2] = (uint16_t)c2, r[3] = (uint16_t)cnt;
  }
};

// the LDS of one wave
struct WaveLds {
  uint8_t *lv;
  uint16_t *tok, *off;
  uint32_t *sym;
};

// update_cdf (src/ec.rs:935-955) in its three steps, for a row of n entries whose last is the counter: the rows in LDS
// (once_symbol), the lanes' four registers (row_symbol) and the three-entry coeff_base_eob rows all adapt by these.
__device__ __forceinline__ uint32_t cdf_rate(uint32_t count, int n) {
  const uint32_t rate = 3 + (n > 3 ? 2 : 1) + (count >> 4);   // 3 + (nsymbs >> 1).min(2)
  return rate < 15 ? rate : 15;                               // (a counter >= 64 is not a CDF; keeps the shift defined)
}
// entry i of the row behind symbol s; at_or_above: i >= s
__device__ __forceinline__ uint32_t cdf_step(uint32_t p, bool at_or_above, uint32_t rate) {
  return at_or_above ? p - (p >> rate) : p + ((32768u - p) >> rate);
}
__device__ __forceinline__ uint32_t cdf_count(uint32_t count) { return count + 1 - (count >> 5); }

// A symbol on one of the rows a transform block hits once.  kChain: `row` lies in the trial's LDS copy and adapts for
// the transform blocks behind this one -- update_cdf with the row's own length n, entry i by lane i, the counter by
// lane n - 1, between two wave barriers: every lane has read the row before it changes, and the next read sees it
// changed.  Called from wave-uniform control flow only.
template <bool kChain, typename Row>
__device__ __forceinline__ void once_symbol(Counter &w, Row *row, int n, int s, int lane) {
  w.symbol(row, n, s);
  if constexpr (kChain) {
    const uint32_t cnt = row[n - 1];
    const uint32_t mine = row[lane < n ? lane : 0];
    wave_sync();
    if (lane < n - 1) row[lane] = (uint16_t)cdf_step(mine, lane >= s, cdf_rate(cnt, n));
    else if (lane == n - 1) row[lane] = (uint16_t)cdf_count(cnt);
    wave_sync();
  }
}

// write_coeffs_lv_map (block_unit.rs:1783-1857) between get_txb_ctx and set_coeff_context, for one transform block on
// the wave's counter: phases A, 1, 2, 3, the signs and the Golomb tails.  `cdf`: the snapshot (k_coeff_rate) or the
// trial's adapting LDS copy (kChain); `row`: the lane's adapting row -- loaded here per block from the snapshot, or
// loaded once per trial by the caller and carried (kChain).  -> false for eob == 0 (only the txb_skip symbol was
// written); else true and `sum` = the sum of |c| over the coded positions on every lane.
template <typename CT, bool kChain, typename Cdfs>
__device__ __forceinline__ bool txb_rate(const RateArgs &a, Counter &w, Cdfs *cdf, LaneRow &row, const CT *qc,
                                         const int eob, const int skip_ctx, const int sign_ctx, const int y_mode,
                                         const int j, const int lane, const WaveLds lds, uint32_t &sum) {
  const int area = a.area;
  once_symbol<kChain>(w, cdf->txb_skip[skip_ctx], 2, eob == 0, lane);
  if (eob == 0) return false;
  const int tx_type = a.type[j];
  const int cls = tx_type < 10 ? 0 : ((tx_type & 1) ? 1 : 2);   // tx_type_to_class: 2D, HORIZ (H_*), VERT (V_*)
  const uint16_t *scan = a.scan[tx_type < 10 ? 0 : ((tx_type & 1) ? 2 : 1)];
  const int hl = a.hl, H = 1 << hl, stride = H + 4;
  uint8_t *lv = lds.lv;

  // A: txb_init_levels (transform_unit.rs:780-792) into zeroed padding
  for (int e = lane; e < kLevelBytes / 4; e += 64) ((uint32_t *)lv)[e] = 0;
  wave_sync();
  for (int e = lane; e < area; e += 64) {
    const int32_t c = (int32_t)qc[e];
    const uint32_t m = (uint32_t)(c < 0 ? -c : c);
    lv[(e >> hl) * stride + (e & (H - 1))] = (uint8_t)(m < 127 ? m : 127);
  }
  wave_sync();

  // write_tx_type (luma only), encode_eob
  if (a.plane == 0 && a.tx_n > 1) once_symbol<kChain>(w, cdf->tx_type[a.is_inter ? 0 : y_mode], a.tx_n, a.tx_sym[j], lane);
  {
    // get_eob_pos_token: eob_to_pos_small / eob_to_pos_large, k_eob_group_start, k_eob_offset_bits
    const int eob_pt = eob < 3 ? eob : (32 - __clz(eob - 1)) + 1;
    const int extra = eob - (eob_pt < 3 ? eob_pt : (1 << (eob_pt - 2)) + 1);
    const int nbits = eob_pt < 3 ? 0 : eob_pt - 2;
    once_symbol<kChain>(w, cdf->eob_flag[cls != 0], a.eob_flag_n, eob_pt - 1, lane);
    if (nbits > 0) {
      once_symbol<kChain>(w, cdf->eob_extra[eob_pt - 3], 2, (extra >> (nbits - 1)) & 1, lane);
      for (int i = nbits - 2; i >= 0; i--) w.bit((extra >> i) & 1);
    }
  }

  if constexpr (!kChain) row.load(cdf, lane);
  uint32_t &c0 = row.c0, &c1 = row.c1, &c2 = row.c2, &cnt = row.cnt;
  // symbol(s) + update_cdf(s) on the lane's row -> the packed (fl, fh, nms)
  auto row_symbol = [&](uint32_t s) -> uint32_t {
    const uint32_t fl = s == 0 ? 32768u : (s == 1 ? c0 : (s == 2 ? c1 : c2));
    const uint32_t fh = s == 0 ? c0 : (s == 1 ? c1 : (s == 2 ? c2 : cnt));
    const uint32_t rate = cdf_rate(cnt, 4);
    cnt = cdf_count(cnt);
    c0 = cdf_step(c0, 0 >= s, rate);
    c1 = cdf_step(c1, 1 >= s, rate);
    c2 = cdf_step(c2, 2 >= s, rate);
    return pack_sym(fl, fh, 4 - s);
  };

  // encode_coeffs: scan positions eob - 1 .. 0
  for (int hi = eob; hi > 0; hi -= kChunk) {
    const int np = hi < kChunk ? hi : kChunk;
    // 1: tokens = ctx | br_ctx << 6 | min(level, 15) << 11 | (position eob - 1) << 15, and symbol counts
    uint32_t tok[4], ns[4], tot = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int idx = lane * 4 + q;
      tok[q] = 0, ns[q] = 0;
      if (idx < np) {
        const int c = hi - 1 - idx;
        const int pos = scan[c];
        const int col = pos >> hl, row = pos & (H - 1);
        const uint8_t *p = lv + col * stride + row;
        const uint32_t level = p[0];
        uint32_t ctx;
        if (c == eob - 1) {
          ctx = c == 0 ? 0 : (c <= (area >> 3) ? 1 : (c <= (area >> 2) ? 2 : 3));   // get_nz_map_ctx, is_eob
        } else {
          uint32_t mag = min3(p[1]) + min3(p[stride]);                               // get_nz_mag
          if (cls == 0) mag += min3(p[stride + 1]) + min3(p[2]) + min3(p[2 * stride]);
          else if (cls == 2) mag += min3(p[2]) + min3(p[3]) + min3(p[4]);
          else mag += min3(p[2 * stride]) + min3(p[3 * stride]) + min3(p[4 * stride]);
          if (cls == 0 && pos == 0) {
            ctx = 0;
          } else {
            ctx = (mag + 1) >> 1;
            ctx = ctx < 4 ? ctx : 4;
            if (cls == 0) {   // av1_nz_map_ctx_offset[tx_size][min(row, 4)][min(col, 4)] by its rule
              if (a.shape == 1 && row < 2) ctx += 11;
              else if (a.shape == 2 && col < 2) ctx += 16;
              else ctx += row + col < 2 ? 1 : (row + col < 4 ? 6 : 21);
            } else {          // nz_map_ctx_offset_1d[col or row]
              const int k = cls == 1 ? col : row;
              ctx += 26 + (k == 0 ? 0 : (k == 1 ? 5 : 10));
            }
          }
        }
        uint32_t br = 0, rounds = 0;
        if (level > 2) {                                                             // get_br_ctx
          uint32_t mag = (uint32_t)p[1] + p[stride];
          bool near;
          if (cls == 0) mag += p[stride + 1], near = row < 2 && col < 2;
          else if (cls == 1) mag += p[2 * stride], near = col == 0;
          else mag += p[2], near = row == 0;
          mag = (mag + 1) >> 1;
          mag = mag < 6 ? mag : 6;
          br = pos == 0 ? mag : (near ? mag + 7 : mag + 14);
          rounds = (level - 3) / 3 + 1;
          rounds = rounds < 4 ? rounds : 4;
        }
        tok[q] = ctx | (br << 6) | ((level < 15 ? level : 15) << 11) | ((uint32_t)(c == eob - 1) << 15);
        ns[q] = 1 + rounds;
      }
      tot += ns[q];
    }
    uint32_t incl = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += t;
    }
    const int total = __builtin_amdgcn_readlane((int)incl, 63);
    uint32_t off = incl - tot;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int idx = lane * 4 + q;
      if (idx < np) {
        lds.tok[idx] = (uint16_t)tok[q];
        lds.off[idx] = (uint16_t)off;
      }
      off += ns[q];
    }
    wave_sync();
    // 2: every row's lane emits its symbols in coding order
    for (int idx = 0; idx < np; idx++) {
      const uint32_t t = lds.tok[idx], o = lds.off[idx];
      const uint32_t ctx = t & 63, br = (t >> 6) & 31, level = (t >> 11) & 15;
      if (t >> 15) {
        if (lane == 63) {   // coeff_base_eob: one symbol per transform block, from the snapshot or the LDS copy
          auto *r = cdf->coeff_base_eob[ctx];
          const uint32_t s = (level < 3 ? (level > 1 ? level : 1) : 3) - 1;          // min(level, 3) - 1; level >= 1
          lds.sym[o] = pack_sym(s > 0 ? r[s - 1] : 32768u, r[s], 3 - s);
          if constexpr (kChain) {   // update_cdf on a three-entry row; lane 63 alone reads and writes these rows
            const uint32_t n = r[2], rate = cdf_rate(n, 3);
            const uint32_t p0 = r[0], p1 = r[1];
            r[0] = (uint16_t)cdf_step(p0, 0 >= s, rate);
            r[1] = (uint16_t)cdf_step(p1, 1 >= s, rate);
            r[2] = (uint16_t)cdf_count(n);
          }
        }
      } else if ((uint32_t)lane == ctx) {
        lds.sym[o] = row_symbol(min3(level));
      }
      if (level > 2 && (uint32_t)lane == kBaseRows + br) {
        for (uint32_t base = level - 3, k = 0; k < 4; k++) {                        // level 15 stands for >= 15
          const uint32_t s = min3(base - 3 * k);
          lds.sym[o + 1 + k] = row_symbol(s);
          if (s < 3) break;
        }
      }
    }
    wave_sync();
    // 3: the chain
    for (int k = 0; k < total; k++) {
      const uint32_t x = lds.sym[k];
      w.store(x & 1023, (x >> 10) & 1023, x >> 20);
    }
    wave_sync();   // the next chunk rewrites the three buffers
  }

  // encode_coeff_signs: scan positions 0 .. eob - 1; cul_level = sum of |c| over them
  sum = 0;
  for (int lo = 0; lo < eob; lo += kChunk) {
    const int np = eob - lo < kChunk ? eob - lo : kChunk;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int idx = q * 64 + lane;
      if (idx < np) {
        const int32_t v = (int32_t)qc[scan[lo + idx]];
        const uint32_t m = (uint32_t)(v < 0 ? -v : v);
        sum += m;
        lds.sym[idx] = (m << 1) | (uint32_t)(v < 0);
      }
    }
    wave_sync();
    for (int idx = 0; idx < np; idx++) {
      const uint32_t x = lds.sym[idx], m = x >> 1;
      if (m == 0) continue;
      if (lo + idx == 0) once_symbol<kChain>(w, cdf->dc_sign[sign_ctx], 2, x & 1, lane);
      else w.bit(x & 1);
      if (m > 14) {   // write_golomb(level - COEFF_BASE_RANGE - NUM_BASE_LEVELS - 1)
        const uint32_t g = m - 14;
        const int len = 32 - __clz((int)g);
        for (int i = 0; i < len - 1; i++) w.bit(0);
        for (int i = len - 1; i >= 0; i--) w.bit((g >> i) & 1);
      }
    }
    wave_sync();
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m, WAVE);
  return true;
}

// the value write_coeffs_lv_map hands set_coeff_context; dc = coeffs[0]: every scan order starts at coefficient 0
__device__ __forceinline__ uint32_t cul_level(uint32_t sum, int32_t dc) {
  uint32_t cul = sum < 63 ? sum : 63;  // COEFF_CONTEXT_MASK, then set_dc_sign (block_unit.rs:325-331)
  if (dc < 0) cul |= 1u << 6;
  else if (dc > 0) cul += 2u << 6;
  return cul;
}

// the four waves' buffers and this wave's part of them
#define R1_RATE_LDS(wave)                                                  \
  __shared__ __attribute__((aligned(16))) uint8_t s_lv[4][kLevelBytes];    \
  __shared__ uint16_t s_tok[4][kChunk];                                    \
  __shared__ uint16_t s_off[4][kChunk];                                    \
  __shared__ uint32_t s_sym[4][kSymMax];                                   \
  const WaveLds lds{s_lv[wave], s_tok[wave], s_off[wave], s_sym[wave]}

template <typename CT>
__global__ __launch_bounds__(256) void k_coeff_rate(const RateArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  R1_RATE_LDS(wave);
  const int slot = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
  if (slot >= a.n_slots) return;
  const int ci = slot / a.nt, j = slot - ci * a.nt;
  const R1TxbCtx cx = a.ctxs[ci];
  const int eob = __builtin_amdgcn_readfirstlane((int)a.eobs[slot]);
  const int skip_ctx = __builtin_amdgcn_readfirstlane((int)cx.txb_skip_ctx);
  const int sign_ctx = __builtin_amdgcn_readfirstlane((int)cx.dc_sign_ctx);
  const int y_mode = __builtin_amdgcn_readfirstlane((int)cx.y_mode);
  const int sel = __builtin_amdgcn_readfirstlane((int)cx.cdf_sel);
  if (eob > a.area || skip_ctx >= R1_TXB_SKIP_CONTEXTS || sign_ctx >= R1_DC_SIGN_CONTEXTS || y_mode >= R1_INTRA_MODES ||
      sel >= a.n_cdfs) {
    if (lane == 0) {
      a.rate[slot] = 0xFFFFFFFFu;
      if (a.cul) a.cul[slot] = 0;
    }
    return;
  }
  const R1CoeffCdfs *cdf = a.cdfs + sel;
  const CT *qc = (const CT *)a.qc + (size_t)slot * (size_t)a.area;
  Counter w;
  const uint32_t tell = w.tell_frac();
  LaneRow row;
  uint32_t sum, cul = 0;
  if (txb_rate<CT, false>(a, w, cdf, row, qc, eob, skip_ctx, sign_ctx, y_mode, j, lane, lds, sum))
    cul = cul_level(sum, (int32_t)qc[0]);
  if (lane == 0) {
    a.rate[slot] = w.tell_frac() - tell;
    if (a.cul) a.cul[slot] = (uint8_t)cul;
  }
}

// ---- what the chain and the whole block share: a plane's grid of transform blocks, the snapshot load, the walk
struct TxbGrid {
  int ntx, gw;                 // transform blocks per trial and per row (chroma: encoder.rs:2327-2338, 2492-2505;
                               // ntx 0..4, gw >= 1)
  int tw4, th4;                // the transform in the plane's 4x4 units
  int xdec, ydec, adj_x, adj_y;   // luma-unit origin of block (bx, by) = ((bx * tw4) << xdec) - adj_x: the subsampling and
                               // the one-unit shift of a 4-wide / 4-high block (encoder.rs:2365-2368); luma: all 0
};

// whether the loop codes transform block k of the grid (encoder.rs:1441, 2282, 2446: the LUMA-unit origin against the
// tile grid), and its origin in the plane's 4x4 units
__device__ __forceinline__ bool txb_coded(const TxbGrid &g, int k, int mi_w, int mi_h, int &x4, int &y4) {
  const int by = k / g.gw, bx = k - by * g.gw;
  x4 = bx * g.tw4, y4 = by * g.th4;
  return (x4 << g.xdec) - g.adj_x < mi_w && (y4 << g.ydec) - g.adj_y < mi_h;
}

// A snapshot (1088 bytes, in dwords) into the wave's adapting LDS copy -- the rows a block hits once -- and the lanes'
// coeff_base / coeff_br rows; both stay across chunks and transform blocks.  The barrier covers the caller's LDS writes.
__device__ __forceinline__ void load_snapshot(R1CoeffCdfs *cdf, LaneRow &row, const R1CoeffCdfs *snap, int lane) {
  for (int e = lane; e < (int)(sizeof(R1CoeffCdfs) / 4); e += 64) ((uint32_t *)cdf)[e] = ((const uint32_t *)snap)[e];
  row.load(snap, lane);
  wave_sync();
}

// One plane's transform blocks in raster order on the carried counter, CDF copy, lane rows and the plane's 32 context
// bytes `nb` (above[16], left[16], in LDS): per block the skip test, get_txb_ctx, txb_rate, cul_level and
// set_coeff_context, all wave-uniform.  at(k): where block k lies in qcoeffs / eobs; out(k, cul, rate): the kernel's
// outputs for block k, zeros for a block the loop does not code.  cw4, ch4: the plane's frame clips (a coded block's
// span is 1 or more by the callers' tests).  The loop is bounded by ntx <= 16.
template <typename CT, typename At, typename Out>
__device__ __forceinline__ void plane_walk(const RateArgs &a, const TxbGrid &g, const void *qcoeffs, const uint16_t *eobs,
                                           const bool chroma, const int uv_skip_off, const int mi_w, const int mi_h,
                                           const int cw4, const int ch4, uint8_t *nb, const int y_mode, const int j,
                                           const int lane, Counter &w, R1CoeffCdfs *cdf, LaneRow &row, const WaveLds lds,
                                           At at, Out out) {
  const int ntx = g.ntx, tw4 = g.tw4, th4 = g.th4;
  for (int k = 0; k < ntx; k++) {
    int x4, y4;
    if (!txb_coded(g, k, mi_w, mi_h, x4, y4)) {
      out(k, 0u, 0u);
      continue;
    }
    const size_t idx = at(k);
    const int eob = __builtin_amdgcn_readfirstlane((int)eobs[idx]);
    const CT *qc = (const CT *)qcoeffs + idx * (size_t)a.area;
    // get_txb_ctx (block_unit.rs:442-526) over the frame-clipped span (encoder.rs:1561-1566).  A sign field of 3 is
    // nothing set_dc_sign stores: it counts as 0.
    const int sw = tw4 < cw4 - x4 ? tw4 : cw4 - x4, sh = th4 < ch4 - y4 ? th4 : ch4 - y4;
    int dc_sign = 0;
    uint32_t top = 0, left = 0;
    for (int i = 0; i < sw; i++) {
      const uint32_t v = nb[x4 + i];
      top |= v;
      dc_sign += (v >> 6) == 1 ? -1 : ((v >> 6) == 2 ? 1 : 0);
    }
    for (int i = 0; i < sh; i++) {
      const uint32_t v = nb[16 + y4 + i];
      left |= v;
      dc_sign += (v >> 6) == 1 ? -1 : ((v >> 6) == 2 ? 1 : 0);
    }
    const int sign_ctx = dc_sign == 0 ? 0 : (dc_sign < 0 ? 1 : 2);
    int skip_ctx = 0;
    if (chroma) {          // the chroma arm: the whole bytes, sign bits included
      skip_ctx = (int)(top != 0) + (int)(left != 0) + uv_skip_off;
    } else if (ntx > 1) {  // plane_bsize != tx_size.block_size(): skip_contexts[min][max]
      top &= 63, left &= 63;
      const uint32_t mx = (top | left) < 4 ? (top | left) : 4, lo = top < left ? top : left, mn = lo < 4 ? lo : 4;
      skip_ctx = mx == 0 ? 1 : (mn == 0 ? 2 + (mx > 3) : (mx <= 3 ? 4 : (mn <= 3 ? 5 : 6)));
    }
    const uint32_t t0 = w.tell_frac();
    uint32_t sum, cul = 0;
    if (txb_rate<CT, true>(a, w, cdf, row, qc, eob, skip_ctx, sign_ctx, y_mode, j, lane, lds, sum))
      cul = cul_level(sum, (int32_t)qc[0]);
    // set_coeff_context over the full span (block_unit.rs:333-347); the reads above are behind the barriers of txb_rate
    if (lane < 16 ? (lane >= x4 && lane < x4 + tw4) : (lane < 32 && lane - 16 >= y4 && lane - 16 < y4 + th4))
      nb[lane] = (uint8_t)cul;
    wave_sync();
    out(k, cul, w.tell_frac() - t0);
  }
}

// ---- the chain: a block's luma transform blocks in raster order on one counter (r1_coeff_rate_chain_batch)
struct ChainArgs {
  RateArgs r;                  // r.ctxs is unused; r.cul holds ntx bytes per trial; r.n_slots = trials
  const R1TxbChainCtx *chains;
  uint32_t *txb_rate;          // optional
  uint8_t *ctx_out;            // optional
  TxbGrid g;                   // the luma grid: xdec = ydec = adj_x = adj_y = 0
  int order;
};
static_assert(sizeof(R1TxbChainCtx) == 40, "ABI layout");

// One wave per trial, four trials per workgroup, as k_coeff_rate.  The trial's R1CoeffCdfs is copied to LDS once and
// adapts there; the 32 context bytes live in LDS, where plane_walk reads and sets them.
template <typename CT>
__global__ __launch_bounds__(256) void k_coeff_rate_chain(const ChainArgs c) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  R1_RATE_LDS(wave);
  __shared__ __attribute__((aligned(16))) R1CoeffCdfs s_cdf[4];
  __shared__ uint8_t s_nb[4][32];      // above[16], left[16]
  const RateArgs &a = c.r;
  const int trial = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
  if (trial >= a.n_slots) return;
  const int ci = trial / a.nt, j = trial - ci * a.nt;
  const TxbGrid g{c.g.ntx, c.g.gw, c.g.tw4, c.g.th4, 0, 0, 0, 0};   // luma: the zeros as constants, so that they fold away
  const int ntx = g.ntx;
  const uint8_t *chb = (const uint8_t *)(c.chains + ci);
  const int mi_w = __builtin_amdgcn_readfirstlane((int)chb[32]), mi_h = __builtin_amdgcn_readfirstlane((int)chb[33]);
  const int clip_w4 = __builtin_amdgcn_readfirstlane((int)chb[34]), clip_h4 = __builtin_amdgcn_readfirstlane((int)chb[35]);
  const int y_mode = __builtin_amdgcn_readfirstlane((int)chb[36]), sel = __builtin_amdgcn_readfirstlane((int)chb[37]);
  // where transform block k of this trial lies in qcoeffs / eobs
  auto at = [&](int k) -> size_t { return c.order == 0 ? (size_t)trial * ntx + k : ((size_t)ci * ntx + k) * a.nt + j; };
  // device-resident data the host cannot see: lane k looks at transform block k; mi_w <= clip_w4 keeps the span of a
  // coded block at 1 or more
  bool bad = y_mode >= R1_INTRA_MODES || sel >= a.n_cdfs || mi_w > clip_w4 || mi_h > clip_h4;
  int x4, y4;
  if (lane < ntx && txb_coded(g, lane, mi_w, mi_h, x4, y4) && (int)a.eobs[at(lane)] > a.area) bad = true;
  if (__ballot(bad) != 0) {
    if (lane == 0) a.rate[trial] = 0xFFFFFFFFu;
    if (lane < ntx) {
      if (c.txb_rate) c.txb_rate[(size_t)trial * ntx + lane] = 0;
      if (a.cul) a.cul[(size_t)trial * ntx + lane] = 0;
    }
    if (c.ctx_out && lane < 32) c.ctx_out[(size_t)trial * 32 + lane] = 0;
    return;
  }
  R1CoeffCdfs *cdf = &s_cdf[wave];
  uint8_t *nb = s_nb[wave];
  if (lane < 32) nb[lane] = chb[lane];
  LaneRow row;
  load_snapshot(cdf, row, a.cdfs + sel, lane);
  Counter w;
  const uint32_t tell0 = w.tell_frac();
  plane_walk<CT>(a, g, a.qc, a.eobs, false, 0, mi_w, mi_h, clip_w4, clip_h4, nb, y_mode, j, lane, w, cdf, row, lds, at,
                 [&](int k, uint32_t cul, uint32_t rate) {
                   if (lane == 0 && c.txb_rate) c.txb_rate[(size_t)trial * ntx + k] = rate;
                   if (lane == 0 && a.cul) a.cul[(size_t)trial * ntx + k] = (uint8_t)cul;
                 });
  if (lane == 0) a.rate[trial] = w.tell_frac() - tell0;
  if (c.ctx_out && lane < 32) c.ctx_out[(size_t)trial * 32 + lane] = nb[lane];
}

// ---- the whole block: luma, then U, then V on one counter that starts at a handed-over rng (r1_coeff_rate_block_batch)
struct PlaneArgs {             // one plane's arrays and its grid
  const void *qc;
  const uint16_t *eobs;
  int n_txb, step;             // transform blocks in the arrays; block k of a trial lies at first + k * step
  TxbGrid g;
};
struct BlockArgs {
  RateArgs r[2];               // by plane type; .cul = 48 bytes per trial, type[] = identity, r[0].n_slots = trials;
                               // .qc, .eobs, .ctxs, .nt are unused
  PlaneArgs pl[3];
  const R1BlockRateTrial *trials;
  const R1BlockChainCtx *blocks;
  uint32_t *plane_rate;        // optional
  uint16_t *rng_out;           // optional
  uint8_t *ctx_out;            // optional
  uint32_t mask[2];            // the types the luma set / the chroma size's scans admit
  int n_blocks;
  int uv_skip_off;             // 10 when the plane's block has more pixels than the chroma transform, else 7
};
static_assert(sizeof(R1BlockChainCtx) == 108 && sizeof(R1BlockRateTrial) == 24, "ABI layout");

// ---- where a trial's CDFs come from and where they go: the two places in which r1_coeff_rate_block_batch and
// r1_coeff_cdf_adapt_batch differ, as the `Io` parameter of one body (block_trial)
// Snapshots the host hands over, picked by the block's cdf_sel / cdf_sel_uv; what has adapted is dropped.
struct FromSnapshots {
  static constexpr bool kRateOptional = false;
  __device__ __forceinline__ bool acts(int) const { return true; }
  __device__ __forceinline__ bool bad_sel(const BlockArgs &c, int sel) const { return sel >= c.r[0].n_cdfs; }
  __device__ __forceinline__ void load(const RateArgs &a, R1CoeffCdfs *cdf, LaneRow &row, int, int, int sel, int lane) const {
    load_snapshot(cdf, row, a.cdfs + sel, lane);
  }
  __device__ __forceinline__ void store(R1CoeffCdfs *, const LaneRow &, int, int, int) const {}
};

// One field of an R1CoeffCdfs slice inside an R1CoeffCdfContext, in uint16_t units: `rows` rows of `n` entries from
// `src` on, row after row.  The slice's own row has sizeof(field[0]) / 2 entries, `n` or more; what lies beyond `n` and
// beyond `rows` is no part of the context and reads 0.  The plane that adapts the slice owns rows own_lo .. own_hi - 1.
struct CdfSeg {
  uint16_t src, n, rows, own_lo, own_hi;
};
struct CdfMap {
  CdfSeg seg[8];   // in R1CoeffCdfs field order
};
static_assert(sizeof(R1CoeffCdfContext) == 7872 && sizeof(R1CoeffCdfContext) % 16 == 0, "ABI layout");

// f(field index, the field's first entry, row length and entry count in the slice, all compile-time once inlined)
#define R1_SLICE_FIELD(i, name)                                                                        \
  f(i, (int)(offsetof(R1CoeffCdfs, name) / 2), (int)(sizeof(((R1CoeffCdfs *)nullptr)->name[0]) / 2), \
    (int)(sizeof(((R1CoeffCdfs *)nullptr)->name) / 2))
template <typename F>
__device__ __forceinline__ void slice_fields(F f) {
  R1_SLICE_FIELD(0, txb_skip);
  R1_SLICE_FIELD(1, eob_flag);
  R1_SLICE_FIELD(2, eob_extra);
  R1_SLICE_FIELD(3, coeff_base_eob);
  R1_SLICE_FIELD(4, coeff_base);
  R1_SLICE_FIELD(5, coeff_br);
  R1_SLICE_FIELD(6, dc_sign);
  R1_SLICE_FIELD(7, tx_type);
}
#undef R1_SLICE_FIELD

// The slice of context `ctx` that `map` describes into `slice` (LDS or global), every entry of it written; by one wave.
// The loops are bounded by the slice's size.
__device__ __forceinline__ void cdf_gather(const CdfMap &map, const uint16_t *ctx, uint16_t *slice, int lane) {
  slice_fields([&](int i, int dst, int stride, int len) __attribute__((always_inline)) {
    const int src = map.seg[i].src, n = map.seg[i].n, rows = map.seg[i].rows;
    for (int e = lane; e < len; e += 64) {
      const int r = e / stride, col = e - r * stride;
      slice[dst + e] = r < rows && col < n ? ctx[src + r * n + col] : (uint16_t)0;
    }
  });
}
// ... and back: the rows the plane owns, nothing else of the context
__device__ __forceinline__ void cdf_scatter(const CdfMap &map, uint16_t *ctx, const uint16_t *slice, int lane) {
  slice_fields([&](int i, int dst, int stride, int len) __attribute__((always_inline)) {
    const int src = map.seg[i].src, n = map.seg[i].n, lo = map.seg[i].own_lo, hi = map.seg[i].own_hi;
    for (int e = lane; e < len; e += 64) {
      const int r = e / stride, col = e - r * stride;
      if (r >= lo && r < hi && col < n) ctx[src + r * n + col] = slice[dst + e];
    }
  });
}

// A device-resident context per trial, read and adapted in place; an optional gate on the pick's state.
struct InContext {
  static constexpr bool kRateOptional = true;
  R1CoeffCdfContext *contexts;
  const R1RdPick *state;     // optional
  int call_id;
  CdfMap map[2];             // by plane type
  __device__ __forceinline__ bool acts(int trial) const {
    return state == nullptr || __builtin_amdgcn_readfirstlane((int)state[trial].best_call) == call_id;
  }
  __device__ __forceinline__ bool bad_sel(const BlockArgs &, int) const { return false; }
  // the plane type's slice into the wave's LDS copy and the lanes' rows; the first barrier covers the caller's LDS
  // writes and the copy, as load_snapshot's
  __device__ __forceinline__ void load(const RateArgs &, R1CoeffCdfs *cdf, LaneRow &row, int pt, int trial, int, int lane) const {
    cdf_gather(map[pt], (const uint16_t *)(contexts + trial), (uint16_t *)cdf, lane);
    wave_sync();
    row.load(cdf, lane);
    wave_sync();
  }
  // what stands in the lanes' rows and in LDS, back to the context; the copy may be overwritten behind the last barrier
  __device__ __forceinline__ void store(R1CoeffCdfs *cdf, const LaneRow &row, int pt, int trial, int lane) const {
    row.store(cdf, lane);
    wave_sync();
    cdf_scatter(map[pt], (uint16_t *)(contexts + trial), (const uint16_t *)cdf, lane);
    wave_sync();
  }
};
struct AdaptArgs {
  BlockArgs b;               // b.r[].cdfs / n_cdfs are unused; b.r[0].rate is optional
  InContext io;
};

// One wave per trial, four trials per workgroup, as k_coeff_rate_chain and on the same walk.  The wave's LDS CDF copy
// and the lanes' coeff_base / coeff_br rows hold the luma slice for the luma plane and are overwritten with the
// chroma slice in front of U; V continues on what U left.  io.store stands behind the luma plane and behind V.
// The 96 context bytes live in LDS (s_nb), 32 per plane.
// A plane's record is read from the arguments by the plane index and handed on by reference: selects on the index
// would keep all three planes' values live in SGPRs.  The loop is bounded by three planes.
template <typename CT, typename Io>
__device__ __forceinline__ void block_trial(const BlockArgs &c, const Io &io, const int trial, const int wave,
                                            const int lane, const WaveLds lds, R1CoeffCdfs *s_cdf, uint8_t (*s_nb)[96]) {
  if (!io.acts(trial)) return;
  const R1BlockRateTrial *tr = c.trials + trial;
  const uint32_t *first = &tr->first_y;      // first_y, first_u, first_v
  const uint32_t bi = (uint32_t)__builtin_amdgcn_readfirstlane((int)tr->block);
  const uint32_t rng0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)tr->rng);
  const int np = __builtin_amdgcn_readfirstlane((int)tr->do_chroma) != 0 ? 3 : 1;
  const uint8_t *chb = (const uint8_t *)(c.blocks + (bi < (uint32_t)c.n_blocks ? bi : 0));   // n_blocks >= 1
  const int mi_w = __builtin_amdgcn_readfirstlane((int)chb[96]), mi_h = __builtin_amdgcn_readfirstlane((int)chb[97]);
  const int y_mode = __builtin_amdgcn_readfirstlane((int)chb[102]), sel = __builtin_amdgcn_readfirstlane((int)chb[103]);
  const int sel_uv = __builtin_amdgcn_readfirstlane((int)chb[104]);
  {
    // device-resident data the host cannot see: lane k looks at transform block k of every plane
    bool bad = bi >= (uint32_t)c.n_blocks || rng0 < 0x8000u || y_mode >= R1_INTRA_MODES || io.bad_sel(c, sel) ||
               mi_w > (int)chb[98] || mi_h > (int)chb[99] || (np == 3 && io.bad_sel(c, sel_uv));
    for (int p = 0; p < np; p++) {
      const PlaneArgs &pl = c.pl[p];
      const int tt = p ? tr->uv_tx_type : tr->tx_type;
      if (tt >= 16 || !((c.mask[p != 0] >> (tt & 15)) & 1)) bad = true;
      if (pl.g.ntx == 0 || bad) continue;
      if (pl.qc == nullptr) {     // chroma arrays the call left out
        bad = true;
        continue;
      }
      const uint32_t f = first[p];
      if ((uint64_t)f + (uint64_t)(pl.g.ntx - 1) * (uint32_t)pl.step >= (uint64_t)pl.n_txb) {
        bad = true;
        continue;
      }
      int x4, y4;      // the read is inside n_txb by the test above
      if (lane < pl.g.ntx && txb_coded(pl.g, lane, mi_w, mi_h, x4, y4)) {
        if ((int)pl.eobs[(size_t)f + (size_t)lane * pl.step] > c.r[p != 0].area) bad = true;
        if (p && ((int)chb[100] - x4 < 1 || (int)chb[101] - y4 < 1)) bad = true;
      }
    }
    if (__ballot(bad) != 0) {
      if (lane == 0) {
        if (!Io::kRateOptional || c.r[0].rate) c.r[0].rate[trial] = 0xFFFFFFFFu;
        if (c.rng_out) c.rng_out[trial] = 0;
      }
      if (c.plane_rate && lane < 3) c.plane_rate[(size_t)trial * 3 + lane] = 0;
      if (c.r[0].cul && lane < 48) c.r[0].cul[(size_t)trial * 48 + lane] = 0;
      if (c.ctx_out)
        for (int e = lane; e < 96; e += 64) c.ctx_out[(size_t)trial * 96 + e] = 0;
      return;
    }
  }
  R1CoeffCdfs *cdf = &s_cdf[wave];
  for (int e = lane; e < 96; e += 64) s_nb[wave][e] = chb[e];
  LaneRow row;
  Counter w;
  w.rng = rng0;
  const uint32_t tell0 = w.tell_frac();
  uint32_t tell_p = tell0;
  for (int p = 0; p < np; p++) {
    const RateArgs &a = c.r[p != 0];
    const PlaneArgs &pl = c.pl[p];
    // the plane type's slice; in front of U every lane is behind its last read of the luma copy (the barriers of
    // txb_rate and of io.store)
    if (p < 2) io.load(a, cdf, row, p, trial, p ? sel_uv : sel, lane);
    const int cw4 = __builtin_amdgcn_readfirstlane((int)chb[p ? 100 : 98]), ch4 = __builtin_amdgcn_readfirstlane((int)chb[p ? 101 : 99]);
    const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)first[p]);
    const int j = __builtin_amdgcn_readfirstlane((int)(p ? tr->uv_tx_type : tr->tx_type));
    uint8_t *cul_out = a.cul ? a.cul + (size_t)trial * 48 + p * 16 : nullptr;
    plane_walk<CT>(
        a, pl.g, pl.qc, pl.eobs, p != 0, c.uv_skip_off, mi_w, mi_h, cw4, ch4, s_nb[wave] + p * 32, y_mode, j, lane, w, cdf,
        row, lds, [&](int k) -> size_t { return (size_t)f + (size_t)k * pl.step; },
        [&](int k, uint32_t cul, uint32_t) {
          if (lane == 0 && cul_out) cul_out[k] = (uint8_t)cul;
        });
    if (p != 1) io.store(cdf, row, p != 0, trial, lane);
    if (cul_out && lane >= pl.g.ntx && lane < 16) cul_out[lane] = 0;    // the entries no transform block stands for
    const uint32_t t = w.tell_frac();
    if (lane == 0 && c.plane_rate) c.plane_rate[(size_t)trial * 3 + p] = t - tell_p;
    tell_p = t;
  }
  if (lane == 0) {
    if (!Io::kRateOptional || c.r[0].rate) c.r[0].rate[trial] = tell_p - tell0;
    if (c.rng_out) c.rng_out[trial] = (uint16_t)w.rng;
  }
  if (np == 1) {
    if (c.plane_rate && lane >= 1 && lane < 3) c.plane_rate[(size_t)trial * 3 + lane] = 0;
    if (c.r[0].cul && lane >= 16 && lane < 48) c.r[0].cul[(size_t)trial * 48 + lane] = 0;
  }
  if (c.ctx_out)
    for (int e = lane; e < 96; e += 64) c.ctx_out[(size_t)trial * 96 + e] = s_nb[wave][e];
}

// the wave's adapting CDF copy and the trial's 96 context bytes ([plane]: above[16], left[16])
#define R1_BLOCK_LDS                                                      \
  __shared__ __attribute__((aligned(16))) R1CoeffCdfs s_cdf[4];           \
  __shared__ uint8_t s_nb[4][96]

template <typename CT>
__global__ __launch_bounds__(256) void k_coeff_rate_block(const BlockArgs c) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  R1_RATE_LDS(wave);
  R1_BLOCK_LDS;
  const int trial = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
  if (trial >= c.r[0].n_slots) return;
  block_trial<CT>(c, FromSnapshots{}, trial, wave, lane, lds, s_cdf, s_nb);
}

// r1_coeff_cdf_adapt_batch: the same trial on contexts[trial], which it leaves adapted
template <typename CT>
__global__ __launch_bounds__(256) void k_coeff_cdf_adapt(const AdaptArgs c) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  R1_RATE_LDS(wave);
  R1_BLOCK_LDS;
  const int trial = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
  if (trial >= c.b.r[0].n_slots) return;
  block_trial<CT>(c.b, c.io, trial, wave, lane, lds, s_cdf, s_nb);
}
#undef R1_BLOCK_LDS

// r1_coeff_cdf_slice_batch: one wave per context, four per workgroup; one small copy
struct SliceArgs {
  const R1CoeffCdfContext *contexts;
  R1CoeffCdfs *out;
  int n;
  CdfMap map;
};
__global__ __launch_bounds__(256) void k_coeff_cdf_slice(const SliceArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (i >= a.n) return;
  cdf_gather(a.map, (const uint16_t *)(a.contexts + i), (uint16_t *)(a.out + i), lane);
}
#undef R1_RATE_LDS
}  // namespace


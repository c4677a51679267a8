// scales.hip -- the temporal-RDO scale maps and the segmentation inputs on device (SURVEY.md 8f "N1" -> "N4").
//
// Once per coded frame the reference turns the lookahead's maps (intra costs, block importances) and the activity
// scales into the DistortionScale grid every distortion reads, and fits the segment quantizers to it:
//   distortion_scale_for per importance block           src/api/internal.rs:1211-1230, src/rdo.rs:506-553
//   compute_spatiotemporal_scores / _temporal_scores    src/encoder.rs:744-777 (DistortionScale::inv_mean, rdo.rs:585)
//   k-means of blog16(score), k = 3 .. 8                src/segmentation.rs:77-94, src/util/kmeans.rs
//   the choice of k, deltas and thresholds (HOST)       src/segmentation.rs:96-160, src/encoder.rs:566-580
//   spatiotemporal_scale + segment_idx_from_distortion  src/rdo.rs:464-504, src/segmentation.rs:192-196
//
// r1_frame_scales: three launches.  (1) one lane per block: d, score = d * a; the workgroup's sum of
// blog32_q11(score) goes to the frame total with ONE 64-bit integer atomic (the sum is an integer: any order is
// exact).  (2) one lane: inv_mean through bexp64, blog64 -- once, as the reference states them.  (3) one lane per
// block: both maps times inv_mean.  The one float is pow(frac, 1/3) in f64.
//
// r1_scale_kmeans: no sort.  The keys are i16 in [-28672, 28672] (scores are in [1, 2^28 - 1]), so a histogram with
// inclusive prefix counts C and prefix sums S holds everything the reference reads off its sorted array:
// after `scan`, high[i] = #{d <= t_i} = C[t_i], low[i + 1] = #{d < t_i} = C[t_i - 1], and the cluster sums are
// differences of S; the initial low[i] = i (n - 1) / (K - 1) is an order statistic of C.  (1) histogram: each
// workgroup counts into an LDS window of 16384 bins around key 0 (scores within 2^+-4 of the frame's mean, which
// inv_mean has just put at 1.0) and merges its non-empty bins with integer atomics; the rare key outside goes to
// HBM directly.  (2) one workgroup scans the bins and then runs the six k-means, one wave each, lane j = cluster j.
#include "common.hpp"
#include "quant_tables.inc"
#include "scale_common.hpp"

using namespace r1scale;

namespace {

constexpr int KEY_MIN = -(DS_SHIFT << 11);      // blog16(1)
constexpr int KEY_BINS = (28 << 11) + 1;        // blog16(2^28 - 1) = 28672: the quartic's fraction reaches 0
constexpr int WIN_BINS = 16384, WIN_LO = -KEY_MIN - WIN_BINS / 2;   // the LDS window, in bin indices
constexpr int HIST_PER_WG = 2048;               // keys per workgroup of the histogram launch
constexpr int SCAN_THREADS = 512;
constexpr int SCAN_PER_THREAD = (KEY_BINS + SCAN_THREADS - 1) / SCAN_THREADS;

// distortion_scale_for (rdo.rs:506-553): two f64 operations and the platform's pow
__device__ __forceinline__ uint32_t distortion_scale_for(float importance, uint32_t intra_cost) {
  if (intra_cost == 0) return 1u << DS_SHIFT;
  const double intra = (double)intra_cost;
  const double frac = (intra + (double)importance) / intra;
  return ds_from_f64(pow(frac, 1.0 / 3.0));
}

__global__ __launch_bounds__(256) void k_scores(const uint32_t *__restrict__ intra_costs,
                                                const float *__restrict__ importances,
                                                const uint32_t *__restrict__ activity, int n,
                                                uint32_t *__restrict__ dist_out, uint32_t *__restrict__ score_out,
                                                R1ScaleStats *__restrict__ stats) {
  __shared__ unsigned long long part[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  long long lg = 0;
  if (i < n) {
    const uint32_t d = distortion_scale_for(importances[i], intra_costs[i]);
    const uint32_t s = activity ? ds_mul(d, activity[i]) : d;
    dist_out[i] = d;
    score_out[i] = s;
    lg = blog32_q11(s);
  }
  const unsigned long long tot = wg_sum_u64((unsigned long long)lg, part);
  if (threadIdx.x == 0) atomicAdd((unsigned long long *)&stats->log_sum_q11, tot);
}

// DistortionScale::inv_mean's tail and compute_*_scores' return value, on one lane
__global__ void k_inv_mean(R1ScaleStats *stats, int n) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t log_inv_mean_q11 = (int64_t)(DS_SHIFT << 11) - stats->log_sum_q11 / n;
  int64_t v = bexp64((log_inv_mean_q11 + (DS_SHIFT << 11)) * ((int64_t)1 << (57 - 11)));
  v = v < 1 ? 1 : v > (int64_t)DS_MAX ? (int64_t)DS_MAX : v;
  stats->inv_mean = (uint32_t)v;
  stats->reserved = 0;
  stats->log_isqrt_mean_scale = (blog64(v) - q57(DS_SHIFT)) >> 1;
}

__global__ __launch_bounds__(256) void k_normalise(const R1ScaleStats *__restrict__ stats, int n,
                                                   uint32_t *__restrict__ dist, uint32_t *__restrict__ score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t im = stats->inv_mean;
  dist[i] = ds_mul(dist[i], im);
  score[i] = ds_mul(score[i], im);
}

// ---- k-means of blog16(score) ----
__global__ __launch_bounds__(256) void k_key_hist(const uint32_t *__restrict__ scores, int n,
                                                  uint32_t *__restrict__ hist) {
  __shared__ uint32_t win[WIN_BINS];
  for (int b = threadIdx.x; b < WIN_BINS; b += 256) win[b] = 0;
  __syncthreads();
  const int base = blockIdx.x * HIST_PER_WG;
  for (int k = threadIdx.x; k < HIST_PER_WG; k += 256) {
    const int i = base + k;
    if (i < n) {
      // a score outside [1, 2^28 - 1] is not a DistortionScale: its key is clamped to the table
      int bin = blog32_q11(scores[i]) - (DS_SHIFT << 11) - KEY_MIN;
      bin = bin < 0 ? 0 : bin >= KEY_BINS ? KEY_BINS - 1 : bin;
      const int wb = bin - WIN_LO;
      if (wb >= 0 && wb < WIN_BINS) atomicAdd(&win[wb], 1u);
      else atomicAdd(&hist[bin], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < WIN_BINS; b += 256) {
    const uint32_t c = win[b];
    if (c) atomicAdd(&hist[WIN_LO + b], c);
  }
}

// #{d <= t} and their sum, read off the prefix tables (t: a key, any value)
__device__ __forceinline__ void upto(const uint32_t *cnt, const long long *tot, int t, long long &c, long long &s) {
  int b = t - KEY_MIN;
  if (b >= KEY_BINS) b = KEY_BINS - 1;
  if (b < 0) { c = 0; s = 0; }
  else { c = cnt[b]; s = tot[b]; }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_kmeans(const uint32_t *__restrict__ hist, int n,
                                                              uint32_t *cnt, long long *tot,
                                                              int16_t *__restrict__ centroids) {
  __shared__ uint32_t pc[SCAN_THREADS];
  __shared__ long long ps[SCAN_THREADS];
  const int t = threadIdx.x;
  // inclusive prefix counts / sums: thread t owns SCAN_PER_THREAD consecutive bins
  const int b0 = t * SCAN_PER_THREAD, b1 = min(b0 + SCAN_PER_THREAD, KEY_BINS);
  uint32_t c = 0;
  long long s = 0;
  for (int b = b0; b < b1; b++) {
    const uint32_t h = hist[b];
    c += h;
    s += (long long)h * (b + KEY_MIN);
  }
  pc[t] = c;
  ps[t] = s;
  __syncthreads();
  for (int m = 1; m < SCAN_THREADS; m <<= 1) {          // Hillis-Steele inclusive scan
    const uint32_t ac = t >= m ? pc[t - m] : 0;
    const long long as = t >= m ? ps[t - m] : 0;
    __syncthreads();
    pc[t] += ac;
    ps[t] += as;
    __syncthreads();
  }
  c = pc[t] - c;
  s = ps[t] - s;
  for (int b = b0; b < b1; b++) {
    const uint32_t h = hist[b];
    c += h;
    s += (long long)h * (b + KEY_MIN);
    cnt[b] = c;
    tot[b] = s;
  }
  __syncthreads();   // the tables are this workgroup's own stores: visible to all of it from here on

  // wave w: kmeans::<K = 8 - w>; lane j < K is cluster j (src/util/kmeans.rs:11-66)
  const int wave = t >> 6, lane = t & 63;
  if (wave >= 6) return;
  const int K = 8 - wave;
  const int j = lane < K ? lane : K - 1;                 // idle lanes shadow the last cluster
  const long long total = tot[KEY_BINS - 1];
  int mean;
  {
    // data[low] of the sorted array, low = j (n - 1) / (K - 1): the first bin whose prefix count exceeds low
    const uint32_t low = (uint32_t)(((long long)j * (n - 1)) / (K - 1));
    int lo = 0, hi = KEY_BINS - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cnt[mid] > low) hi = mid;
      else lo = mid + 1;
    }
    mean = lo + KEY_MIN;
  }
  const int limit = 2 * (32 - __builtin_clz((unsigned)n));
  for (int round = 0; round < limit; round++) {
    // threshold between clusters j and j + 1 is (c1 + c2 + 1) >> 1; a key equal to it counts in both
    const int up = __shfl(mean, j + 1 < K ? j + 1 : j, WAVE), down = __shfl(mean, j > 0 ? j - 1 : 0, WAVE);
    long long lc = 0, ls = 0, hc = n, hs = total;
    if (j > 0) upto(cnt, tot, ((mean + down + 1) >> 1) - 1, lc, ls);
    if (j < K - 1) upto(cnt, tot, (up + mean + 1) >> 1, hc, hs);
    const long long count = hc - lc;
    int next = mean;
    if (count != 0) next = (int)((hs - ls + (count >> 1)) / count);   // i64 division, toward zero
    const bool changed = __any(next != mean);
    mean = next;
    if (!changed) break;
  }
  if (lane < 8) centroids[wave * 8 + lane] = lane < K ? (int16_t)mean : (int16_t)0;
}

// ---- per coded block ----
__constant__ const uint8_t kBlockImpW[22] = {1, 1, 1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8, 16, 16, 1, 2, 1, 4, 2, 8};
__constant__ const uint8_t kBlockImpH[22] = {1, 1, 1, 1, 2, 1, 2, 4, 2, 4, 8, 4, 8, 16, 8, 16, 2, 1, 4, 1, 8, 2};

struct SegThresholds { uint32_t t[7]; };

__global__ __launch_bounds__(256) void k_block_scales(const uint32_t *__restrict__ dist,
                                                      const uint32_t *__restrict__ activity, int w, int h,
                                                      const R1ScaleBlock *__restrict__ blocks, int n,
                                                      SegThresholds thr, int have_thr, int min_segment,
                                                      uint32_t *__restrict__ scale_out,
                                                      uint8_t *__restrict__ sidx_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const R1ScaleBlock b = blocks[i];   // checked on the host: a BlockSize, origin inside the map
  const int x0 = b.bo_x >> 1, y0 = b.bo_y >> 1;
  const int x1 = min(x0 + (int)kBlockImpW[b.bsize], w), y1 = min(y0 + (int)kBlockImpH[b.bsize], h);
  const unsigned long long den = (unsigned long long)((x1 - x0) * (y1 - y0)) << DS_SHIFT;
  unsigned long long sum = 0;
  for (int y = y0; y < y1; y++)
    for (int x = x0; x < x1; x++) {
      const size_t at = (size_t)y * w + x;
      sum += (unsigned long long)dist[at] * (activity ? activity[at] : (1u << DS_SHIFT));
    }
  const uint32_t scale = (uint32_t)((sum + (den >> 1)) / den);
  if (scale_out) scale_out[i] = scale;
  if (sidx_out) {
    // partition_point of `s < t` over all seven thresholds, the zero ones included: they never increase
    // (update_threshold), so the point is the length of the leading run
    int sidx = 0;
    if (have_thr)
      while (sidx < 7 && scale < thr.t[sidx]) sidx++;
    sidx_out[i] = (uint8_t)(sidx > min_segment ? sidx : min_segment);
  }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct KmScratch { size_t hist, cnt, tot, total; };
KmScratch km_layout() {
  KmScratch s;
  s.hist = 0;
  s.cnt = s.hist + up256((size_t)KEY_BINS * 4);
  s.tot = s.cnt + up256((size_t)KEY_BINS * 4);
  s.total = s.tot + up256((size_t)KEY_BINS * 8);
  return s;
}

// ---- host: ac_q / select_ac_qi (src/quantize/mod.rs:44-97) ----
int bd_index(int bit_depth) { return bit_depth == 8 ? 0 : bit_depth == 10 ? 1 : 2; }
uint64_t ac_q(int qindex, int delta_q, int bit_depth) {
  const int q = qindex + delta_q;
  return kR1AcQLookup[bd_index(bit_depth)][q < 0 ? 0 : q > 255 ? 255 : q];
}
int select_ac_qi(int64_t quantizer, int bit_depth) {
  const uint16_t *t = kR1AcQLookup[bd_index(bit_depth)];
  if (quantizer < t[0]) return 0;
  if (quantizer >= t[255]) return 255;
  int lo = 0, hi = 256;             // the table is strictly increasing: first entry >= quantizer
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < quantizer) lo = mid + 1;
    else hi = mid;
  }
  if (t[lo] == quantizer) return lo;
  // the closest quantizer in the log domain
  const int32_t qthresh = (int32_t)t[lo - 1] * (int32_t)t[lo], q2 = (int32_t)quantizer * (int32_t)quantizer;
  return q2 < qthresh ? lo - 1 : lo;
}

}  // namespace

extern "C" long long r1_frame_scales_scratch_bytes(int n) {
  if (n <= 0 || n > (1 << 28)) return -1;
  return 256;   // nothing beyond the outputs is needed today; the argument stays for a layout that does
}

extern "C" int r1_frame_scales(r1_ctx *ctx, const uint32_t *intra_costs, const float *block_importances,
                               const uint32_t *activity_scales, int n, uint32_t *distortion_scales_out,
                               uint32_t *spatiotemporal_out, R1ScaleStats *stats_out, void *scratch,
                               long long scratch_bytes, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(n > 0 && n <= (1 << 28));
  R1_REQUIRE(intra_costs && block_importances && distortion_scales_out && spatiotemporal_out && stats_out);
  R1_REQUIRE(distortion_scales_out != spatiotemporal_out);
  R1_REQUIRE(scratch && scratch_bytes >= r1_frame_scales_scratch_bytes(n));
  R1DeviceGuard guard(ctx);
  hipStream_t st = (hipStream_t)stream;
  R1_HIP_CHECK(hipMemsetAsync(stats_out, 0, sizeof(R1ScaleStats), st));
  const unsigned g = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_scores, dim3(g), dim3(256), 0, st, intra_costs, block_importances, activity_scales, n,
                     distortion_scales_out, spatiotemporal_out, stats_out);
  hipLaunchKernelGGL(k_inv_mean, dim3(1), dim3(64), 0, st, stats_out, n);
  hipLaunchKernelGGL(k_normalise, dim3(g), dim3(256), 0, st, stats_out, n, distortion_scales_out,
                     spatiotemporal_out);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" long long r1_scale_kmeans_scratch_bytes(int n) {
  if (n <= 0 || n > (1 << 28)) return -1;
  return (long long)km_layout().total;
}

extern "C" int r1_scale_kmeans(r1_ctx *ctx, const uint32_t *spatiotemporal, int n, int16_t *centroids_out,
                               void *scratch, long long scratch_bytes, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(n > 0 && n <= (1 << 28));
  R1_REQUIRE(spatiotemporal && centroids_out && scratch);
  const KmScratch s = km_layout();
  R1_REQUIRE(scratch_bytes >= (long long)s.total);
  R1_REQUIRE(((uintptr_t)scratch & 255) == 0);
  R1DeviceGuard guard(ctx);
  hipStream_t st = (hipStream_t)stream;
  uint8_t *b = (uint8_t *)scratch;
  uint32_t *hist = (uint32_t *)(b + s.hist), *cnt = (uint32_t *)(b + s.cnt);
  long long *tot = (long long *)(b + s.tot);
  R1_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)KEY_BINS * 4, st));
  hipLaunchKernelGGL(k_key_hist, dim3((unsigned)((n + HIST_PER_WG - 1) / HIST_PER_WG)), dim3(256), 0, st,
                     spatiotemporal, n, hist);
  hipLaunchKernelGGL(k_scan_kmeans, dim3(1), dim3(SCAN_THREADS), 0, st, hist, n, cnt, tot, centroids_out);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_segmentation_from_centroids(const int16_t *centroids, int base_q_idx, int bit_depth,
                                              R1SegmentationData *out) {
  R1_REQUIRE(centroids && out);
  R1_REQUIRE(base_q_idx >= 0 && base_q_idx <= 255);
  R1_REQUIRE(r1_depth_ok(bit_depth));
  // variance in spacing between successive centroids, per k; the LAST k of minimal variance (rposition)
  uint64_t variance[6];
  for (int r = 0; r < 6; r++) {
    const int16_t *c = centroids + r * 8;
    const int nd = 8 - r - 1;
    int64_t delta[7], sum = 0;
    for (int i = 0; i < nd; i++) {
      delta[i] = (int64_t)c[i] - (int64_t)c[i + 1];
      sum += delta[i];
    }
    const int64_t mean = sum / nd;
    uint64_t v = 0;
    for (int i = 0; i < nd; i++) v += (uint64_t)((delta[i] - mean) * (delta[i] - mean));
    variance[r] = v;
  }
  int position = 0;
  for (int r = 1; r < 6; r++)
    if (variance[r] <= variance[position]) position = r;
  const int k = 8 - position;
  const int16_t *c = centroids + position * 8;
  // compute_delta: scale Q'^2 = Q^2 in the log domain, centroids in reverse
  const int64_t log2_base_ac_q_q57 = blog64((int64_t)ac_q(base_q_idx, 0, bit_depth));
  const int offset_lower_limit = 1 - base_q_idx;
  *out = R1SegmentationData{};
  for (int i = 0; i < k; i++) {
    const int64_t q = bexp64(log2_base_ac_q_q57 - (int64_t)c[k - 1 - i] * ((int64_t)1 << (57 - 11 - 1)));
    const int qi = select_ac_qi(q, bit_depth);
    const int delta = (qi > 1 ? qi : 1) - base_q_idx;
    out->seg_delta[i] = (int16_t)(delta > offset_lower_limit ? delta : offset_lower_limit);
  }
  out->min_segment = 0;
  out->max_segment = (uint8_t)(k - 1);
  out->k = (uint8_t)k;
  out->position = (uint8_t)position;
  // update_threshold: `data as i8` truncates, as the reference's cast does
  const uint64_t base_ac_q = ac_q(base_q_idx, 0, bit_depth);
  uint64_t real_ac_q[8];
  for (int i = 0; i < k; i++) real_ac_q[i] = ac_q(base_q_idx, (int8_t)out->seg_delta[i], bit_depth);
  for (int i = 0; i + 1 < k; i++) out->threshold[i] = ds_new(base_ac_q * base_ac_q, real_ac_q[i + 1] * real_ac_q[i]);
  return R1_OK;
}

extern "C" int r1_spatiotemporal_scale_batch(r1_ctx *ctx, const uint32_t *distortion_scales,
                                             const uint32_t *activity_scales, int w_in_imp_b, int h_in_imp_b,
                                             const R1ScaleBlock *blocks, int n, const uint32_t *thresholds,
                                             int min_segment, uint32_t *scale_out, uint8_t *sidx_out,
                                             void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(n > 0);
  R1_REQUIRE(w_in_imp_b > 0 && h_in_imp_b > 0 && (long long)w_in_imp_b * h_in_imp_b <= (1 << 28));
  R1_REQUIRE(distortion_scales && blocks && (scale_out || sidx_out));
  R1_REQUIRE(min_segment >= 0 && min_segment <= 7);
  for (int i = 0; i < n; i++) {
    const R1ScaleBlock &b = blocks[i];
    R1_REQUIRE(b.bsize >= 0 && b.bsize < 22);
    R1_REQUIRE(b.bo_x >= 0 && b.bo_y >= 0 && (b.bo_x >> 1) < w_in_imp_b && (b.bo_y >> 1) < h_in_imp_b);
  }
  SegThresholds thr = {};
  if (thresholds)
    for (int i = 0; i < 7; i++) thr.t[i] = thresholds[i];
  R1DeviceGuard guard(ctx);
  hipStream_t st = (hipStream_t)stream;
  // the list travels in stream order: allocated, filled, read and freed on `stream`, nothing outlives the call
  const size_t bytes = (size_t)n * sizeof(R1ScaleBlock);
  R1ScaleBlock *dev = nullptr;
  R1_HIP_CHECK(hipMallocAsync((void **)&dev, bytes, st));
  hipError_t e = hipMemcpyAsync(dev, blocks, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_block_scales, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, distortion_scales,
                       activity_scales, w_in_imp_b, h_in_imp_b, dev, n, thr, thresholds ? 1 : 0, min_segment,
                       scale_out, sidx_out);
    e = hipGetLastError();
  }
  const hipError_t f = hipFreeAsync(dev, st);
  R1_HIP_CHECK(e);
  R1_HIP_CHECK(f);
  return R1_OK;
}

// part_pick.hip -- the partition decision behind the children's chains, on the device.
// r1_rd_partition_pick_batch: one partition type tried at n quad-tree nodes -- the comparison encode_partition_bottomup
// (src/encoder.rs:2683-2843) or rdo_partition_decision (src/rdo.rs:1849-2024) makes with the children's costs -- on a
// 16-byte state per node that is carried from call to call.
// r1_part_select_batch / r1_part_select_rect_batch: the state the winning trial left (the snapshots of the carried
// contexts, the winner arrays of the commit, the reconstruction) moved to where the next node reads it.
// All three enqueue on the caller's stream; nothing is read back.  Pinned by tests/golden/part_pick_ref.npz.
// The pick is a launch-bound kernel of a few loads per node (16 bytes of state, four indices, up to four costs, a
// rate, a parent cost): one lane per node, and no claim beyond that.  The selects are byte movers.
#include "block_geom.hpp"
#include "common.hpp"

#include <float.h>
#include <math.h>

static_assert(sizeof(R1PartPick) == 16, "R1PartPick is 16 bytes");
static_assert(offsetof(R1PartPick, best_rd) == 0 && offsetof(R1RdPick, best_rd) == 0, "a child's cost is read from either");

// ---- the pick ----
struct PartPickArgs {
  R1PartPick *state;
  const uint32_t *part_rate;
  const uint8_t *children;
  const int32_t *child_idx;
  const uint8_t *must_split;
  const R1PartPick *parent;
  const int32_t *parent_idx;
  double lambda;
  size_t child_stride;
  int n, n_children_states, n_parent_states, partition, rule, call_id, early_exit, visited;
};

// One lane per node.  The additions are the reference's, in its order, each rounded on its own: the unit is compiled
// with contraction allowed, so the function states that none may happen here -- neither `cost + child` nor a later
// sum may take the multiply of the cost into it.  The cost itself is one rounding (fma with a zero addend), as in
// k_rd_pick.  Every loop runs over the four entries of a node.
__global__ __launch_bounds__(256) void k_part_pick(const PartPickArgs a) {
#pragma clang fp contract(off)
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= a.n) return;
  R1PartPick *st = a.state + s;
  const double best = st->best_rd;
  double ref = DBL_MAX;
  if (a.parent && a.parent_idx) {
    const int p = a.parent_idx[s];
    if (p >= 0 && p < a.n_parent_states) ref = a.parent[p].best_rd;
  }
  const bool must = a.must_split && a.must_split[s] != 0;
  const double cost = a.part_rate ? __builtin_fma(a.lambda, (double)a.part_rate[s] * 0.125, 0.0) : 0.0;
  double c[4];
  bool present[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = k < a.visited ? a.child_idx[(size_t)s * 4 + k] : -1;
    present[k] = i >= 0 && i < a.n_children_states;
    c[k] = present[k] ? *(const double *)(a.children + (size_t)i * a.child_stride) : DBL_MAX;
  }
  double rd = 0.0;
  bool keep = false, early = false;
  if (a.rule == R1_PART_BOTTOMUP) {
    if (a.partition == R1_PARTITION_NONE) {
      // encoder.rs:2708-2711: best_rd = mode_decision.rd_cost + cost, whatever stood there
      rd = c[0] + cost;
      keep = present[0];
    } else {
      rd = cost;
#pragma unroll
      for (int k = 0; k < 4; k++) {                                     // present[k] is false from `visited` on
        if (early || !present[k] || c[k] == DBL_MAX) continue;          // encoder.rs:2802, 2820
        rd = rd + c[k];
        if (!must && a.early_exit && (rd >= best || rd >= ref)) early = true;   // encoder.rs:2822-2828
      }
      keep = !early && rd < best;                                       // encoder.rs:2835
    }
  } else {
    if (a.partition == R1_PARTITION_NONE) {
      rd = c[0];                                                        // rdo.rs:1856-1861: no partition symbol
      keep = present[0] && rd < best;
    } else {
      double sum = 0.0;
      bool refused = false;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (refused || k >= a.visited) continue;
        if (!present[k]) { refused = true; continue; }                  // rdo.rs:1933-1936
        sum = sum + c[k];
        if (a.early_exit && sum > best) refused = early = true;         // rdo.rs:1912
      }
      rd = cost + sum;                                                  // rdo.rs:1939
      keep = !refused && rd < best;                                     // rdo.rs:2006
    }
  }
  if (keep) {
    st->best_rd = rd;
    st->best_partition = (int8_t)a.partition;
    st->best_call = (int8_t)a.call_id;
  }
  st->early_exit = (uint8_t)early;
}

extern "C" int r1_rd_partition_pick_batch(r1_ctx *ctx, R1PartPick *state, int n, int partition, int call_id, int rule,
                                          double lambda, int enable_early_exit, const uint32_t *part_rate,
                                          const void *children, int child_stride, int n_children_states,
                                          const int32_t *child_idx, const uint8_t *must_split, const R1PartPick *parent,
                                          int n_parent_states, const int32_t *parent_idx, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(state && child_idx);
  R1_REQUIRE(n >= 0);
  R1_REQUIRE(partition >= R1_PARTITION_NONE && partition <= R1_PARTITION_SPLIT);
  R1_REQUIRE(rule == R1_PART_BOTTOMUP || rule == R1_PART_TOPDOWN);
  R1_REQUIRE(call_id >= 0 && call_id <= 127);
  R1_REQUIRE(child_stride >= 8 && child_stride % 8 == 0);
  R1_REQUIRE(n_children_states >= 0 && n_parent_states >= 0);
  R1_REQUIRE(children || n_children_states == 0);
  R1_REQUIRE((uintptr_t)children % 8 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)parent % 8 == 0);
  R1_REQUIRE(lambda >= 0.0 && !isinf(lambda));   // NaN fails the first
  if (n == 0) return R1_OK;
  PartPickArgs a = {state, part_rate, (const uint8_t *)children, child_idx, must_split, parent, parent_idx, lambda,
                    (size_t)child_stride, n, n_children_states, n_parent_states, partition, rule, call_id,
                    enable_early_exit != 0,
                    partition == R1_PARTITION_NONE ? 1 : partition == R1_PARTITION_SPLIT ? 4 : 2};
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_part_pick, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// ---- the selects ----
struct SelectArgs {
  const R1PartPick *state;
  const uint8_t *srcs[4];
  uint8_t *dst;
  size_t src_stride, dst_stride;
  unsigned bytes;
  int n, n_src;
};

// One wave per node, four nodes per workgroup.  A node whose best_call names no source of this call -- none kept, a
// call beyond n_src, a NULL source, or the source that IS the destination -- leaves through a wave-uniform branch
// after its 16-byte state; the others move `bytes` bytes in pieces of V, lane l taking pieces l, l + 64, ...
template <class V>
__global__ __launch_bounds__(256) void k_part_select(const SelectArgs a) {
  const int s = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  if (s >= a.n) return;
  const int call = __builtin_amdgcn_readfirstlane((int)a.state[s].best_call);
  if (call < 0 || call >= a.n_src) return;
  const uint8_t *base = call == 0 ? a.srcs[0] : call == 1 ? a.srcs[1] : call == 2 ? a.srcs[2] : a.srcs[3];
  if (!base || base == a.dst) return;
  const uint8_t *src = base + (size_t)s * a.src_stride;
  uint8_t *dst = a.dst + (size_t)s * a.dst_stride;
  for (unsigned o = (unsigned)lane * sizeof(V); o < a.bytes; o += WAVE * sizeof(V)) *(V *)(dst + o) = *(const V *)(src + o);
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int r1_part_select_batch(r1_ctx *ctx, const R1PartPick *state, int n, int n_src, const void *const *srcs,
                                    long long src_stride, void *dst, long long dst_stride, int bytes, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(state && srcs && dst);
  R1_REQUIRE(n >= 0);
  R1_REQUIRE(n_src >= 1 && n_src <= 4);
  R1_REQUIRE(bytes >= 0 && bytes % 4 == 0);
  R1_REQUIRE(src_stride >= 0 && dst_stride >= 0 && src_stride % 4 == 0 && dst_stride % 4 == 0);
  R1_REQUIRE(dst_stride >= bytes);               // the nodes' destinations are disjoint
  R1_REQUIRE((uintptr_t)dst % 4 == 0);
  SelectArgs a = {};
  bool vec = aligned16(dst) && bytes % 16 == 0 && src_stride % 16 == 0 && dst_stride % 16 == 0;
  for (int k = 0; k < n_src; k++) {
    R1_REQUIRE((uintptr_t)srcs[k] % 4 == 0);
    R1_REQUIRE(srcs[k] != dst || src_stride == dst_stride);
    a.srcs[k] = (const uint8_t *)srcs[k];
    vec = vec && aligned16(srcs[k]);
  }
  if (n == 0 || bytes == 0) return R1_OK;
  a.state = state, a.dst = (uint8_t *)dst, a.src_stride = (size_t)src_stride, a.dst_stride = (size_t)dst_stride;
  a.bytes = (unsigned)bytes, a.n = n, a.n_src = n_src;
  const dim3 grid((unsigned)(((long long)n + 3) / 4));
  R1DeviceGuard guard(ctx);
  r1_by_bool(vec, [&](auto V) {
    using T = std::conditional_t<V.value, uint4, uint32_t>;
    hipLaunchKernelGGL((k_part_select<T>), grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

struct SelectRectArgs {
  const R1PartPick *state;
  const uint8_t *srcs[4];
  const int16_t *pos_xy;
  R1Plane rec;
  int n, n_src, bw, bh, store_w, store_h, max_chunks;
};

// n bytes from src to dst, both inside one 16-byte-aligned window and src == dst modulo 16: the steps up to the
// alignment the address reaches, then down again -- the widest loads and stores the addresses admit.  A step is taken
// only when the bytes are there, so nothing beyond dst + n is written and nothing beyond src + n read.
template <int BPP, class T>
__device__ __forceinline__ void copy_step(uint8_t *&dst, const uint8_t *&src, int &n) {
  *(T *)dst = *(const T *)src, dst += sizeof(T), src += sizeof(T), n -= (int)sizeof(T);
}
template <int BPP>
__device__ __forceinline__ void copy_run(uint8_t *dst, const uint8_t *src, int n) {
  if (n == 16) {                                 // the whole window
    *(uint4 *)dst = *(const uint4 *)src;
    return;
  }
  if (BPP == 1 && n >= 1 && ((uintptr_t)dst & 1)) copy_step<BPP, uint8_t>(dst, src, n);
  if (n >= 2 && ((uintptr_t)dst & 2)) copy_step<BPP, uint16_t>(dst, src, n);
  if (n >= 4 && ((uintptr_t)dst & 4)) copy_step<BPP, uint32_t>(dst, src, n);
  if (n >= 8 && ((uintptr_t)dst & 8)) copy_step<BPP, uint64_t>(dst, src, n);
  if (n >= 8) copy_step<BPP, uint64_t>(dst, src, n);
  if (n >= 4) copy_step<BPP, uint32_t>(dst, src, n);
  if (n >= 2) copy_step<BPP, uint16_t>(dst, src, n);
  if (BPP == 1 && n >= 1) copy_step<BPP, uint8_t>(dst, src, n);
}

// One wave per node, four nodes per workgroup; the gate is k_part_select's.  The node's rectangle, clipped to
// [0, store_w) x [0, store_h) as k_rd_commit clips, is cut into the 16-byte-aligned windows of the DESTINATION's
// rows: at most max_chunks = ceil(bw * BPP / 16) + 1 per row (a run that starts inside a window ends inside one more), lane l
// taking pieces l, l + 64, ... of bh * max_chunks.  CONG: every source is congruent to the destination modulo 16 (the
// host checks; planes of one geometry out of one allocator are), and a window moves by copy_run; otherwise it moves
// pixel by pixel.  No atomics, no LDS, no scratch: the rectangles of one call must not overlap.
template <int BPP, bool CONG>
__global__ __launch_bounds__(256) void k_part_select_rect(const SelectRectArgs a) {
  const int s = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  if (s >= a.n) return;
  const int call = __builtin_amdgcn_readfirstlane((int)a.state[s].best_call);
  if (call < 0 || call >= a.n_src) return;
  const uint8_t *sbase = call == 0 ? a.srcs[0] : call == 1 ? a.srcs[1] : call == 2 ? a.srcs[2] : a.srcs[3];
  uint8_t *dbase = (uint8_t *)a.rec.data;
  if (!sbase || sbase == dbase) return;
  const int px = a.pos_xy[2 * (size_t)s], py = a.pos_xy[2 * (size_t)s + 1];
  const int x0 = px < 0 ? 0 : px, x1 = px + a.bw < a.store_w ? px + a.bw : a.store_w;
  if (x0 >= x1) return;
  const int pieces = a.bh * a.max_chunks;
  for (int p = lane; p < pieces; p += WAVE) {
    const int y = py + p / a.max_chunks, j = p % a.max_chunks;
    if (y < 0 || y >= a.store_h) continue;
    const size_t row = ((size_t)(a.rec.yorigin + y) * (size_t)a.rec.stride + (size_t)a.rec.xorigin) * BPP;
    const uintptr_t b0 = (uintptr_t)dbase + row + (size_t)x0 * BPP, b1 = (uintptr_t)dbase + row + (size_t)x1 * BPP;
    const uintptr_t w0 = (b0 & ~(uintptr_t)15) + (uintptr_t)j * 16;     // window j of the row's run [b0, b1)
    const uintptr_t lo = w0 > b0 ? w0 : b0, hi = w0 + 16 < b1 ? w0 + 16 : b1;
    if (lo >= hi) continue;
    uint8_t *dst = (uint8_t *)lo;
    const uint8_t *src = sbase + (lo - (uintptr_t)dbase);
    if constexpr (CONG) copy_run<BPP>(dst, src, (int)(hi - lo));
    else {
      using PT = std::conditional_t<BPP == 1, uint8_t, uint16_t>;
      for (int o = 0; o < 16 / BPP; o++)
        if (o * BPP < (int)(hi - lo)) ((PT *)dst)[o] = ((const PT *)src)[o];
    }
  }
}

extern "C" int r1_part_select_rect_batch(r1_ctx *ctx, const R1PartPick *state, int n, int n_src,
                                         const R1Plane *src_planes, const R1Plane *dst_plane, const int16_t *pos_xy,
                                         int bw, int bh, int store_w, int store_h, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(state && src_planes && dst_plane && pos_xy);
  R1_REQUIRE(n >= 0);
  R1_REQUIRE(n_src >= 1 && n_src <= 4);
  R1_REQUIRE(r1_block_size_ok(bw, bh));
  const R1Plane &rec = *dst_plane;
  R1_REQUIRE(r1_px_ok(rec) && r1_depth_ok(rec.bit_depth) && r1_px_fits_depth(rec));
  R1_REQUIRE(rec.data && rec.stride > 0 && rec.alloc_height > 0 && rec.xorigin >= 0 && rec.yorigin >= 0);
  // the store rectangle: the visible plane and its padding to the right and below, as far as the allocation goes
  R1_REQUIRE(store_w >= 0 && store_w <= rec.stride - rec.xorigin);
  R1_REQUIRE(store_h >= 0 && store_h <= rec.alloc_height - rec.yorigin);
  R1_REQUIRE((uintptr_t)rec.data % (uintptr_t)rec.bytes_per_px == 0);
  SelectRectArgs a = {};
  bool cong = true;
  for (int k = 0; k < n_src; k++) {
    const R1Plane &sp = src_planes[k];
    if (!sp.data) continue;                      // a trial that was never coded has no plane
    // the source is read at the destination's addresses: it has the destination's geometry
    R1_REQUIRE(sp.stride == rec.stride && sp.alloc_height == rec.alloc_height && sp.xorigin == rec.xorigin &&
               sp.yorigin == rec.yorigin && sp.bytes_per_px == rec.bytes_per_px && sp.bit_depth == rec.bit_depth);
    R1_REQUIRE((uintptr_t)sp.data % (uintptr_t)rec.bytes_per_px == 0);
    a.srcs[k] = (const uint8_t *)sp.data;
    cong = cong && (((uintptr_t)sp.data ^ (uintptr_t)rec.data) & 15) == 0;
  }
  if (n == 0) return R1_OK;
  a.state = state, a.pos_xy = pos_xy, a.rec = rec, a.n = n, a.n_src = n_src, a.bw = bw, a.bh = bh;
  a.store_w = store_w, a.store_h = store_h, a.max_chunks = (bw * rec.bytes_per_px + 15) / 16 + 1;
  const dim3 grid((unsigned)(((long long)n + 3) / 4));
  R1DeviceGuard guard(ctx);
  r1_by_bpp(rec.bytes_per_px, [&](auto B) {
    r1_by_bool(cong, [&](auto G) {
      hipLaunchKernelGGL((k_part_select_rect<B.value, G.value>), grid, dim3(256), 0, (hipStream_t)stream, a);
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// me_tile.hip -- hierarchical motion estimation of whole tiles (r1_estimate_tile_motion_batch, r1_me_status) on the
// search engine of me_search.hpp, which also says what is parallel and what is not: k_me_diag (one launch per
// superblock diagonal), k_me_persist (one launch, hand-overs through progress counters) and their host state (the
// ring slot, the per-geometry row cache, the captured diagonal graph).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "me_search.hpp"

namespace {
// refine_subsampled_motion_estimate (me.rs:634-691): the previous pass' vector of the block at this resolution, then
// every position of [mv - 1, mv + 2]^2 inside the range.  The caller has waited for the entry to be final.
template <bool AGENT, class B>
__device__ __forceinline__ Msr refine_search(const B &b, const TileView &t, int bx, int by, int ssdec) {
  int mvr, mvc;
  uint32_t ns;
  load_stats<AGENT>(t.at(by, bx), mvr, mvc, ns);
  mvr >>= ssdec;
  mvc >>= ssdec;
  return full_search(b, b.po_x + imax(div8(mvc) - 1, div8(b.mvx_min)), b.po_x + imin(div8(mvc) + 2, div8(b.mvx_max)),
                     b.po_y + imax(div8(mvr) - 1, div8(b.mvy_min)), b.po_y + imin(div8(mvr) + 2, div8(b.mvy_max)), 1);
}

// One pass (log2b = 4, 3, 2 <-> ssdec 2, 1, 0) over the superblocks of one
// anti-diagonal of every job.  The three passes run SKEWED in the same launch:
// a superblock of pass q + 1 on diagonal d reads, besides its own area, the
// left / top neighbours (diagonal d - 1, already pass q + 1) and the right /
// bottom neighbours (diagonal d + 1, still pass q: get_subset_predictors samples
// edge midpoints only, me.rs:420-452, never a diagonal neighbour), so it may
// run as soon as pass q has finished diagonal d + 1 -- two launches behind.
// Pass q on diagonal d + 2 meanwhile touches diagonals d + 1 .. d + 3 only.
constexpr int kPassSkew = 2;
#ifdef R1_ME_PROF
// experiment build only: per pass, [0] workgroups, [1] sum of workgroup lifetimes, [2] longest
// workgroup, [3] sum of the refinement phase (100 MHz wall-clock ticks)
__device__ unsigned long long g_me_prof[3][4];
// k_me_persist, search rows: per pass [0] block searches, [1] set-up + wait for the neighbours, [2] the search
// (predictors, candidates, diamond), [3] result stores + publish (100 MHz ticks, summed over the waves)
__device__ unsigned long long g_me_step[3][4];
#endif
template <int BPP>
__global__ __launch_bounds__(256, 5) void k_me_diag(const R1MeJob *__restrict__ jobs,
                                                    const R1MeParams *__restrict__ pp,
                                                    R1MeStats *const *__restrict__ rbufs, int step) {
  const R1MeParams p = *pp;   // uniform: lives in SGPRs; in device memory so that the launch
                              // arguments (and with them the captured graph) do not depend on it
  // blockIdx.z = role.  0..2: the SEARCH of pass z on diagonal step - kPassSkew * z (pass q works
  // kPassSkew diagonals behind pass q - 1, see the host loop).  3, 4: the REFINEMENT
  // (refine_subsampled_sb_motion) for pass z - 2, ONE DIAGONAL AHEAD of that pass' search.  A
  // superblock's refinement depends on nothing but its own statistics of the previous pass, which
  // are final one launch before its search; done inside the search workgroup it was 12 of its
  // 53 us (the chain that bounds every launch), done here it runs beside the searches of the
  // diagonal before.  Its results must stay invisible to those searches -- their right / bottom
  // predictors in this superblock are the UNREFINED vectors -- so they go to a second buffer
  // (rbufs[job], same geometry as the statistics) that the superblock's own search copies in first.
  const int role = (int)blockIdx.z;
  const bool refine_role = role >= 3;
  const int pass = refine_role ? role - 2 : role;
  const int log2b = 4 - pass, diag = step - kPassSkew * pass + (refine_role ? 1 : 0);
  const R1MeJob &job = jobs[blockIdx.y];
  const int sbw = (job.tile_w + SB - 1) / SB, sbh = (job.tile_h + SB - 1) / SB;
  if (diag < 0) return;
  const int sby = (int)blockIdx.x + imax(0, diag - (sbw - 1)), sbx = diag - sby;
  if (sby >= sbh || sbx < 0 || sbx >= sbw) return;   // workgroup-uniform
  __shared__ int16_t sh_subsets[4][kSubsetWords];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#ifdef R1_ME_PROF
  const unsigned long long prof_t0 = wall_clock64();
  unsigned long long prof_t1 = prof_t0;
#endif
  const bool init = log2b == 4;
  const int ssdec = log2b - 2;
  TileView t{job.stats, job.prev, p.stats_cols, p.stats_rows, job.tile_x / MI, job.tile_y / MI,
             job.tile_w / MI, job.tile_h / MI};
  R1MeStats *const rbuf = rbufs[blockIdx.y];
  const int sb_w = imin(SB, job.tile_w - sbx * SB), sb_h = imin(SB, job.tile_h - sby * SB);

  if (refine_role) {
    // refine_subsampled_sb_motion: the previous pass' blocks at this resolution, into rbuf
    TileView tr = t;
    tr.stats = rbuf;
    const int sz = MI << (log2b + 1);
    const int nbx = (sb_w + sz - 1) / sz, nby = (sb_h + sz - 1) / sz;
    if (wave < nbx * nby) {
      const int x = (wave % nbx) * sz, y = (wave / nbx) * sz;
      const int bx = sbx * 16 + x / MI, by = sby * 16 + y / MI;
      const int w = imin(sz, sb_w - x + (1 << ssdec) - 1) >> ssdec;
      const int h = imin(sz, sb_h - y + (1 << ssdec) - 1) >> ssdec;
      Block<BPP, 32> b;
      int rng[4];
      setup_block(b, job, p, t, bx, by, w, h, ssdec, lane, rng);
      const Msr r = refine_search<false>(b, t, bx, by, ssdec);
      store_result(tr, 1 << (log2b + 1), bx, by, r, w, h, ssdec, lane);
    }
    return;
  }

  if (!init) {
    // the refinement of this superblock (previous launch, role 3 / 4) becomes visible now
    const int bx0 = sbx * 16, by0 = sby * 16;
    const int nx = imin(16, t.tcols - bx0), ny = imin(16, t.trows - by0);
    for (int i = threadIdx.x; i < nx * ny; i += 256) {
      const int y = i / nx, xx = i - y * nx;
      const size_t o = (size_t)(t.ty + by0 + y) * t.cols_f + t.tx + bx0 + xx;
      const unsigned long long v = *(const unsigned long long *)(rbuf + o);
      __hip_atomic_store((unsigned long long *)(t.stats + o), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();   // workgroup-scope release / acquire of the stats just written
#ifdef R1_ME_PROF
    prof_t1 = wall_clock64();
#endif
  }

  // estimate_sb_motion: raster order inside the superblock = anti-diagonals
  const int sz = MI << log2b;
  const int nbx = (sb_w + sz - 1) / sz, nby = (sb_h + sz - 1) / sz;
  for (int d = 0; d < nbx + nby - 1; d++) {
    const int j0 = imax(0, d - (nbx - 1));
    const int jy = j0 + wave, jx = d - jy;
    if (jy < nby && jx >= 0 && jx < nbx) {
      const int x = jx * sz, y = jy * sz;
      const int corner = init ? 0 : (1 | ((x & sz) ? 2 : 0) | ((y & sz) ? 4 : 0));
      const int bx = sbx * 16 + x / MI, by = sby * 16 + y / MI;
      const int w = imin(sz, sb_w - x + (1 << ssdec) - 1) >> ssdec;
      const int h = imin(sz, sb_h - y + (1 << ssdec) - 1) >> ssdec;
      Block<BPP, 16> b;
      int rng[4];
      setup_block(b, job, p, t, bx, by, w, h, ssdec, lane, rng);
      const Msr r = full_pixel_me(b, t, p, bx, by, rng, corner, init, ssdec, sh_subsets[wave]);
      store_result(t, 1 << log2b, bx, by, r, w, h, ssdec, lane);
    }
    __syncthreads();   // workgroup-scope release / acquire of the stats just written
  }
#ifdef R1_ME_PROF
  if (threadIdx.x == 0) {
    const unsigned long long t2 = wall_clock64();
    atomicAdd(&g_me_prof[pass][0], 1ull);
    atomicAdd(&g_me_prof[pass][1], t2 - prof_t0);
    atomicMax(&g_me_prof[pass][2], t2 - prof_t0);
    atomicAdd(&g_me_prof[pass][3], prof_t1 - prof_t0);
  }
#endif
}

// ---------------------------------------------------------------------------
// k_me_persist: the same three passes as ONE launch whose waves hand results over through
// progress counters in memory instead of kernel boundaries (R1MeParams::launch_mode 2 / 3).  A wave WALKS A
// ROW: the blocks of one block row of one pass (or the refinements of one row of the previous
// pass' blocks) from left to right.  The left neighbour is then the wave's own previous block;
// the only same-pass hand-over is the row above, which runs one block ahead -- in the steady
// state its result is already there when it is asked for, so the chain is rows + columns block
// steps (127 for a 960 x 1088 tile at 16 x 16) instead of 7 x 31 superblock-diagonal steps.
// Rows are taken from an atomic counter in an order in which everything a row waits for comes
// earlier (key = bottom edge of the row in 16-pixel cells + a per-pass offset): a wave only waits
// for rows that are already running, so there is no deadlock whatever the residency.
//   a search block (pass q) waits for: the row above having passed it; q > 0: the refinement of
//   its own parent block and of the parents of its right / bottom sample positions when those lie
//   in its own superblock (read refined), their pass q - 1 SEARCH when they lie in the next
//   superblock (read unrefined, from the live array).  A refinement waits for the pass q - 1
//   search of its block.
// Visibility.  PIN (launch_mode 2): every wave of a job sits on the XCD job % 8 (a wave asks
// HW_REG_XCC_ID where it is and takes rows from that XCD's list), so results are plain stores --
// they stay in that XCD's L2 -- read back with L1-bypassing (agent-scope) loads, and the progress
// word is a workgroup-scope store behind s_waitcnt(0).  !PIN (launch_mode 3, fewer jobs than XCDs):
// one list, any wave takes any row; results and progress words are agent-scope stores, written
// through.  Why not an __ATOMIC_RELEASE store / fence: at agent scope gfx950 spells it `buffer_wbl2 sc1`
// + s_waitcnt -- a write-back of the XCD's whole L2 per hand-over (round 2 saw that as a "hang": the
// waits ran out of patience behind it).  Measured in round 4 with every shared entry an agent-scope
// atomic, fence(release) before the progress word and fence(acquire) behind each wait
// (profiles/r04_me_fence_ab.md): bit-exact, no hang, and 1.3x (1 job) .. 4.1x (64 jobs) SLOWER.  The
// product keeps the ISA-level argument: the statistics are acknowledged by the memory system
// (s_waitcnt vmcnt(0)) before the progress word is issued -- written through (sc1) where the
// readers may sit on another XCD, left in the L2 that all readers share where they are pinned -- and
// every read of shared data is an L1-bypassing atomic load issued after the wait returned.  The C++
// model has no scope between "workgroup" and "agent" to say "this XCD", so the pinned mode stays a
// data race on paper; launch_mode 1 (kernel boundaries) is the formally clean path and the automatic
// fallback (r1_me_status / Context.estimate_frame_motion).
// Residency: TWO waves per SIMD (host: grid 2048) -- a searching wave is a dependent instruction
// chain that wants a VALU slot every ~8 cycles; a third and fourth wave on the SIMD stretch every
// step of a chain without slack -- so the kernel is not held to k_me_diag's 96
// registers and keeps three candidate batches in flight at every pixel size.
// Refined vectors live in the second buffer and are never copied: the samples pick their buffer.
struct MeRow { uint16_t job; uint8_t kind, pad; uint16_t gy, nb; };   // kind 0..2 search, 3 / 4 refine for pass 1 / 2
struct MePersistArgs {
  const R1MeJob *jobs;
  const R1MeParams *params;
  R1MeStats *const *rbufs;
  const MeRow *rows;            // sorted per XCD: rows of the jobs with job % 8 == xcd (PIN; else one list), in key order
  int n_rows;
  int xoff[9];                  // rows of XCD x: [xoff[x], xoff[x + 1])
  unsigned int *counter;        // [8]: next row of each XCD
  unsigned int *prog;           // per row: epoch << 16 | blocks done
  const unsigned int *foff;     // [job][5]: offset of the job's progress array of each kind
  unsigned int epoch;           // 1 .. 65535
  unsigned int *err;            // set when a wait ran out of patience
  int spin;                     // polls before a wait gives up
};

__device__ __forceinline__ bool me_wait(const unsigned int *f, unsigned int epoch, unsigned int need, int spin) {
  for (int it = 0; it < spin; it++) {
    const unsigned int v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((v >> 16) == epoch && (v & 0xFFFFu) >= need) return true;
    if (it > 64) __builtin_amdgcn_s_sleep(8);
    else if (it > 4) __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

// up to four progress counters polled by four lanes in ONE load per round (a wait is a memory
// round trip even when the counter is already there): a lane with mf != nullptr polls *mf for mn
__device__ __forceinline__ bool me_wait_lanes(const unsigned int *mf, unsigned int mn, unsigned int epoch, int spin) {
  for (int it = 0; it < spin; it++) {
    bool done = true;
    if (mf) {
      const unsigned int v = __hip_atomic_load(mf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      done = (v >> 16) == epoch && (v & 0xFFFFu) >= mn;
    }
    if (__all(done)) return true;
    if (it > 64) __builtin_amdgcn_s_sleep(8);
    else if (it > 4) __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

// PIN: every job on one XCD (launch_mode 2); !PIN: one row list for the whole device, results and
// progress words written through at agent scope (launch_mode 3: fewer jobs than XCDs)
template <int BPP, bool PIN>
__global__ __launch_bounds__(64, 2) void k_me_persist(MePersistArgs a) {
  __shared__ int16_t sh_subsets[kSubsetWords];
  __shared__ unsigned int sh_item;
  const R1MeParams p = *a.params;
  const int lane = threadIdx.x;
  // every wave of a job sits on ONE XCD (the job's rows are handed out only to waves that find
  // themselves there), so a hand-over never leaves that XCD's L2
  const int xcd = PIN ? (__builtin_amdgcn_s_getreg(6164) & 7) : 0;   // hwreg(HW_REG_XCC_ID, 0, 4)
  // this XCD's slice of the row list, by selects: a.xoff[xcd] -- a run-time index into the kernel's by-value
  // argument block -- made the compiler keep a copy of the whole block in scratch memory
  int x_lo = a.xoff[0], x_hi = a.xoff[1];
#pragma unroll
  for (int k = 1; k < 8; k++)
    if (xcd == k) { x_lo = a.xoff[k]; x_hi = a.xoff[k + 1]; }
  for (;;) {
    if (lane == 0) sh_item = atomicAdd(a.counter + xcd, 1u);
    __syncthreads();
    const unsigned int ii = __builtin_amdgcn_readfirstlane(sh_item) + (unsigned int)x_lo;
    __syncthreads();
    if (ii >= (unsigned int)x_hi) return;
    const MeRow row = a.rows[ii];
    // the row's view of its job BY VALUE (scalar registers): nothing of it is re-read per block
    // behind the stores and atomics of the loop
    const R1MeJob &gjob = a.jobs[row.job];
    struct { R1MeStats *stats; const R1MeStats *prev; int tile_x, tile_y, tile_w, tile_h; } job =
        {gjob.stats, gjob.prev, gjob.tile_x, gjob.tile_y, gjob.tile_w, gjob.tile_h};
    const unsigned int *fo = a.foff + 5 * row.job;
    const bool refine = row.kind >= 3;
    const int pass = refine ? row.kind - 2 : row.kind;         // the pass the row belongs to
    const int log2b = 4 - pass, ssdec = log2b - 2;
    const bool init = log2b == 4;
    const R1Plane org = gjob.org[ssdec], ref = gjob.ref[ssdec];
    TileView t{job.stats, job.prev, p.stats_cols, p.stats_rows, job.tile_x / MI, job.tile_y / MI,
               job.tile_w / MI, job.tile_h / MI};
    t.rstats = a.rbufs[row.job];
    unsigned int *mine = a.prog + fo[row.kind] + row.gy;
    bool ok = true;
    for (int gx = 0; gx < row.nb; gx++) {
      if (refine) {
        // refine_subsampled_motion_estimate of block (gx, gy) of pass `pass - 1`
        const int sz = MI << (log2b + 1);
        const int x = gx * sz, y = row.gy * sz;                // tile px
        const int sbx = x / SB, sby = y / SB;
        const int sb_w = imin(SB, job.tile_w - sbx * SB), sb_h = imin(SB, job.tile_h - sby * SB);
        const int xin = x - sbx * SB, yin = y - sby * SB;
        const int bx = x / MI, by = y / MI;
        const int w = imin(sz, sb_w - xin + (1 << ssdec) - 1) >> ssdec;
        const int h = imin(sz, sb_h - yin + (1 << ssdec) - 1) >> ssdec;
        Block<BPP, 32, 3> b;
        int rng[4];
        setup_block(b, org, ref, p, t, bx, by, w, h, ssdec, lane, rng);
        if (lane == 0) ok = me_wait(a.prog + fo[pass - 1] + row.gy, a.epoch, gx + 1, a.spin) && ok;
        ok = __shfl((int)ok, 0, 64) != 0;
        const Msr r = refine_search<true>(b, t, bx, by, ssdec);
        TileView tr = t;
        tr.stats = (R1MeStats *)t.rstats;
        store_result<true, !PIN>(tr, 1 << (log2b + 1), bx, by, r, w, h, ssdec, lane);
      } else {
        const int sz = MI << log2b;
        const int x = gx * sz, y = row.gy * sz;
        const int sbx = x / SB, sby = y / SB;
        const int sb_w = imin(SB, job.tile_w - sbx * SB), sb_h = imin(SB, job.tile_h - sby * SB);
        const int xin = x - sbx * SB, yin = y - sby * SB;
        const int bx = x / MI, by = y / MI;
        const int w = imin(sz, sb_w - xin + (1 << ssdec) - 1) >> ssdec;
        const int h = imin(sz, sb_h - yin + (1 << ssdec) - 1) >> ssdec;
        // everything that does not depend on the neighbours first: source rows, masks, MV range
#ifdef R1_ME_PROF
        const unsigned long long st0 = wall_clock64();
#endif
        Block<BPP, 16, 3> b;
        int rng[4];
        setup_block(b, org, ref, p, t, bx, by, w, h, ssdec, lane, rng);
        {
          // up to four progress words, lane k polling the k-th: each lane's own (pointer, count) pair is set
          // directly -- lists indexed by a run-time count lived in scratch memory, a store and a load round trip
          // on every step of the chain
          const unsigned int *mf = nullptr;
          unsigned int mn = 0;
          if (row.gy > 0 && lane == 0) { mf = a.prog + fo[pass] + row.gy - 1; mn = gx + 1; }
          if (!init) {
            const int psz = sz * 2;                            // the parents' size, px
            if (lane == 1) { mf = a.prog + fo[2 + pass] + y / psz; mn = x / psz + 1; }   // own parent refined
            // get_subset_predictors' right / bottom sample positions (me.rs:420-452), tile px
            const int wu = ((w << ssdec) + MI - 1) >> 2, hu = ((h << ssdec) + MI - 1) >> 2;   // 4x4 units
            const int half_w = imin(wu >> 1, t.tcols - 1 - bx), half_h = imin(hu >> 1, t.trows - 1 - by);
            if (bx + wu < t.tcols && lane == 2) {
              const int px = (bx + wu) * MI, py = (by + half_h) * MI;
              const bool same = px / SB == sbx && py / SB == sby;
              mf = a.prog + fo[same ? 2 + pass : pass - 1] + py / psz; mn = px / psz + 1;
            }
            if (by + hu < t.trows && lane == 3) {
              const int px = (bx + half_w) * MI, py = (by + hu) * MI;
              const bool same = px / SB == sbx && py / SB == sby;
              mf = a.prog + fo[same ? 2 + pass : pass - 1] + py / psz; mn = px / psz + 1;
            }
          }
          if (row.gy > 0 || !init) ok = me_wait_lanes(mf, mn, a.epoch, a.spin) && ok;
        }
        const int corner = init ? 0 : (1 | ((xin & sz) ? 2 : 0) | ((yin & sz) ? 4 : 0));
#ifdef R1_ME_PROF
        const unsigned long long st1 = wall_clock64();
#endif
        const Msr r = full_pixel_me<Block<BPP, 16, 3>, true>(b, t, p, bx, by, rng, corner, init, ssdec, sh_subsets);
#ifdef R1_ME_PROF
        const unsigned long long st2 = wall_clock64();
#endif
        store_result<true, !PIN>(t, 1 << log2b, bx, by, r, w, h, ssdec, lane);
#ifdef R1_ME_PROF
        __builtin_amdgcn_s_waitcnt(0);
        if (lane == 0) {
          const unsigned long long st3 = wall_clock64();
          atomicAdd(&g_me_step[pass][0], 1ull);
          atomicAdd(&g_me_step[pass][1], st1 - st0);
          atomicAdd(&g_me_step[pass][2], st2 - st1);
          atomicAdd(&g_me_step[pass][3], st3 - st2);
        }
#endif
      }
      // publish: the statistics first (agent-scope stores, acknowledged), then the progress
      asm volatile("" ::: "memory");   // no result store may sink below the wait, no progress store rise above it
      __builtin_amdgcn_s_waitcnt(0);
      asm volatile("" ::: "memory");
      if (lane == 0) {
        const unsigned int word = (a.epoch << 16) | (unsigned int)(gx + 1);
        if constexpr (PIN) __hip_atomic_store(mine, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_store(mine, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // the error word is host-mapped pinned memory (one per ring slot): the host reads it where the
    // slot's event is waited for, without a copy (r1_me_status / the slot's reuse)
    if (lane == 0 && !ok) __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

#ifdef R1_ME_PROF
// experiment build only (tools/me_prof.py finds the three by name): copies a counter array out and optionally clears it
template <class Sym>
static int me_debug_read(const Sym &sym, unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sym), sizeof(Sym)) != hipSuccess) return -1;
  if (reset) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(sym)) != hipSuccess) return -1;
    if (hipMemset(p, 0, sizeof(Sym)) != hipSuccess) return -1;
  }
  return 0;
}
// g_me_fine lives in me_search.hpp, one copy per including unit: this is the tile unit's, the probes as they fire
// under k_me_diag / k_me_persist -- all that me_prof.py exercises (the block unit's copy is not read back)
extern "C" int r1_debug_me_fine(unsigned long long *out, int reset) { return me_debug_read(g_me_fine, out, reset); }   /* out[8] */
extern "C" int r1_debug_me_step(unsigned long long *out, int reset) { return me_debug_read(g_me_step, out, reset); }   /* out[3][4] */
extern "C" int r1_debug_me_prof(unsigned long long *out, int reset) { return me_debug_read(g_me_prof, out, reset); }   /* out[3][4] */
#endif

// ---- k_me_persist, host side: the item list of a call's geometry (cached per ring slot), the
// flag arrays, one launch ----
namespace {
struct MePersistCache {
  std::vector<int> geo;            // signature: per job tile_w, tile_h
  void *rows = nullptr;            // device: MeRow[n_rows]
  void *foff = nullptr;            // device: uint32[n_jobs][5]
  void *prog = nullptr;            // device: uint32 per row (epoch << 16 | blocks done)
  void *ctl = nullptr;             // device: counter
  unsigned int *err_host = nullptr;   // pinned, host-mapped: set by a wave whose dependency wait ran out
  unsigned int *err_dev = nullptr;    // the same word as the device sees it
  unsigned long long call_id = 0;     // r1_estimate_tile_motion_batch call this slot last served
  int n_rows = 0;
  int xoff[9] = {0};
  unsigned int epoch = 0;
  bool launched = false;
};

// ordering key of a row, in half units of 16-pixel cells: its bottom edge plus a per-pass offset
// chosen so that every row a row waits for has a smaller key
inline int me_row_key(int kind, int gy) {
  static const int c2[3] = {0, 18, 32};
  const int q = kind >= 3 ? kind - 3 : kind, s = 4 >> q;
  return 2 * (gy * s + s - 1) + c2[q] + (kind >= 3 ? 1 : 0);
}

// k_me_persist hands a job's rows out to the waves of ONE XCD (job % 8), which is only right on
// a device whose launches spread over all eight: probed once per context.
__global__ void k_me_xcd_probe(unsigned int *mask) {
  if (threadIdx.x == 0) atomicOr(mask, 1u << (__builtin_amdgcn_s_getreg(6164) & 15));
}

int me_probe_xcds(r1_ctx *ctx, hipStream_t st) {
  unsigned int *d = nullptr, h = 0;
  R1_HIP_CHECK(hipMalloc(&d, sizeof(h)));
  hipError_t e = hipMemsetAsync(d, 0, sizeof(h), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_me_xcd_probe, dim3(1024), dim3(64), 0, st, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d);
  R1_HIP_CHECK(e);
  // The pinned hand-over (plain result stores that stay in the job's XCD L2, readers bypassing L1)
  // leans on gfx942 / gfx950 cache behaviour, not on the HIP memory model: explicit allow-list on
  // top of the probe.  Anything else takes the unpinned launch (agent-scope write-through).
  hipDeviceProp_t prop;
  R1_HIP_CHECK(hipGetDeviceProperties(&prop, ctx->device));
  const bool arch_ok = !strncmp(prop.gcnArchName, "gfx950", 6) || !strncmp(prop.gcnArchName, "gfx942", 6);
  ctx->me_xcds = (h == 0xFFu && arch_ok) ? 8 : 0;   // anything but exactly XCD 0..7: no pinned launches
  return R1_OK;
}

// What a call's ring slot hands to its launches: one upload of `bytes` from the slot's pinned staging brings the job
// descriptors, the parameters and the per-job refinement buffer pointers to these device addresses
struct MeStaged { int slot; size_t bytes; const R1MeJob *djobs; const R1MeParams *dparams; R1MeStats *const *drbufs; };

// the error word of a slot whose launch has completed: recorded against the call it served
void me_collect_slot(r1_ctx *ctx, MePersistCache &c) {
  if (!c.launched || !c.err_host) return;
  c.launched = false;
  if (*(volatile unsigned int *)c.err_host) {
    ctx->me_failed++;
    if (!ctx->me_first_failed) ctx->me_first_failed = c.call_id;
  }
}

int me_launch_persistent(r1_ctx *ctx, const MeStaged &sc, const R1MeJob *jobs, int n_jobs, int bpp, hipStream_t st,
                         bool pin) {
  const int slot = sc.slot;
  if (!ctx->me_persist[slot]) ctx->me_persist[slot] = new MePersistCache();
  MePersistCache &c = *(MePersistCache *)ctx->me_persist[slot];
  // A dependency wait of the previous call on this slot that ran out of patience (the slot's event
  // has been waited for by the caller of this function): THAT call's statistics are not to be
  // trusted.  It is recorded against that call (r1_me_status reports its id); this call goes ahead.
  me_collect_slot(ctx, c);
  if (!c.err_host) {
    R1_HIP_CHECK(hipHostMalloc((void **)&c.err_host, 64, hipHostMallocMapped));
    *c.err_host = 0;
    hipError_t e = hipHostGetDevicePointer((void **)&c.err_dev, c.err_host, 0);
    if (e != hipSuccess) { (void)hipHostFree(c.err_host); c.err_host = nullptr; R1_HIP_CHECK(e); }
  }
  std::vector<int> geo;
  geo.push_back(pin ? 1 : 0);
  for (int j = 0; j < n_jobs; j++) { geo.push_back(jobs[j].tile_w); geo.push_back(jobs[j].tile_h); }
  if (geo != c.geo || c.epoch >= 65535) {
    // nothing of the old geometry survives a failed rebuild: forget it before freeing
    c.geo.clear();
    c.n_rows = 0;
    for (void **pp : {&c.rows, &c.foff, &c.prog, &c.ctl})
      if (*pp) { (void)hipFree(*pp); *pp = nullptr; }
    std::vector<MeRow> rows;
    std::vector<unsigned int> foff((size_t)n_jobs * 5);
    unsigned int nprog = 0;
    for (int j = 0; j < n_jobs; j++) {
      for (int kind = 0; kind < 5; kind++) {
        const int q = kind >= 3 ? kind - 3 : kind;
        const int nbx = (jobs[j].tile_w + (SB >> q) - 1) / (SB >> q), nby = (jobs[j].tile_h + (SB >> q) - 1) / (SB >> q);
        foff[(size_t)j * 5 + kind] = nprog;
        nprog += (unsigned int)nby;
        for (int gy = 0; gy < nby; gy++)
          rows.push_back(MeRow{(uint16_t)j, (uint8_t)kind, 0, (uint16_t)gy, (uint16_t)nbx});
      }
    }
    const int xmask = pin ? 7 : 0;
    std::stable_sort(rows.begin(), rows.end(), [xmask](const MeRow &a, const MeRow &b) {
      const int xa = a.job & xmask, xb = b.job & xmask;
      if (xa != xb) return xa < xb;
      return me_row_key(a.kind, a.gy) < me_row_key(b.kind, b.gy);
    });
    for (int x = 0; x <= 8; x++) c.xoff[x] = 0;
    for (const MeRow &r : rows) c.xoff[(r.job & xmask) + 1]++;
    for (int x = 0; x < 8; x++) c.xoff[x + 1] += c.xoff[x];
    R1_HIP_CHECK(hipMalloc(&c.rows, rows.size() * sizeof(MeRow)));
    R1_HIP_CHECK(hipMalloc(&c.foff, foff.size() * sizeof(unsigned int)));
    R1_HIP_CHECK(hipMalloc(&c.prog, (size_t)nprog * sizeof(unsigned int)));
    R1_HIP_CHECK(hipMalloc(&c.ctl, 8 * sizeof(unsigned int)));
    R1_HIP_CHECK(hipMemcpy(c.rows, rows.data(), rows.size() * sizeof(MeRow), hipMemcpyHostToDevice));
    R1_HIP_CHECK(hipMemcpy(c.foff, foff.data(), foff.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
    R1_HIP_CHECK(hipMemset(c.prog, 0, (size_t)nprog * sizeof(unsigned int)));
    c.n_rows = (int)rows.size();
    c.epoch = 0;
    c.geo = geo;
  }
  c.epoch++;
  R1_HIP_CHECK(hipMemcpyAsync(ctx->me_jobs[slot], ctx->me_jobs_host[slot], sc.bytes, hipMemcpyHostToDevice, st));
  R1_HIP_CHECK(hipMemsetAsync(c.ctl, 0, 8 * sizeof(unsigned int), st));
  *c.err_host = 0;   // the slot's previous launch has completed (event) and been collected
  MePersistArgs a;
  a.jobs = sc.djobs; a.params = sc.dparams; a.rbufs = sc.drbufs;
  a.rows = (const MeRow *)c.rows; a.n_rows = c.n_rows;
  a.counter = (unsigned int *)c.ctl; a.err = c.err_dev;
  for (int x = 0; x <= 8; x++) a.xoff[x] = c.xoff[x];
  a.prog = (unsigned int *)c.prog; a.foff = (const unsigned int *)c.foff;
  a.epoch = c.epoch;
  a.spin = 1 << 18;
  // TWO waves per SIMD (256 CUs x 4 SIMDs x 2), not as many as fit: a searching wave wants a VALU
  // instruction every ~8 cycles at 2.6-4.4 issue cycles each, so a third and fourth wave on a SIMD
  // stretch every block step of a chain that has no slack (measured, 24 jobs: grid 4096 1.73 ms,
  // 3072 1.60, 2048 1.50, 1536 1.54; 10-bit 2.08 / 1.96 / 1.89 / 2.03, 1024: 2.11).  Rows beyond the grid are taken by
  // the waves that finish theirs, in key order.
  const int grid = c.n_rows < 2048 ? c.n_rows : 2048;
  if (getenv("R1_ME_PERSISTENT_DEBUG")) fprintf(stderr, "k_me_persist: %d rows, grid %d, epoch %u\n", c.n_rows, grid, a.epoch);
  r1_by_bpp(bpp, [&](auto B) {
    r1_by_bool(pin, [&](auto PIN) {
      hipLaunchKernelGGL((k_me_persist<B.value, PIN.value>), dim3(grid), dim3(64), 0, st, a);
    });
  });
  R1_HIP_CHECK(hipGetLastError());
  R1_HIP_CHECK(hipEventRecord(ctx->me_done[slot], st));
  c.launched = true;
  c.call_id = ctx->me_calls;
  if (getenv("R1_ME_PERSISTENT_CHECK")) {   // debugging aid: synchronous check of this very call
    R1_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned int e = *(volatile unsigned int *)c.err_host;
    if (getenv("R1_ME_PERSISTENT_DEBUG")) fprintf(stderr, "k_me_persist: rows %d, err %u\n", c.n_rows, e);
    c.launched = false;
    if (e) { r1_set_error("k_me_persist: a dependency wait timed out"); return R1_EHIP; }
  }
  return R1_OK;
}

// The checks of a call's jobs; hands back the pixel size and the largest tile in superblocks.
int me_check_jobs(const R1MeJob *jobs, int n_jobs, const R1MeParams *params, int &bpp, int &max_sbw, int &max_sbh) {
  R1_REQUIRE(jobs);
  R1_REQUIRE(n_jobs <= 256);   // tiles x reference frames of one frame
  R1_REQUIRE(r1_depth_ok(params->bit_depth));
  R1_REQUIRE(params->stats_cols > 0 && params->stats_rows > 0);
  bpp = jobs[0].org[0].bytes_per_px;
  R1_REQUIRE(r1_px_ok(bpp));
  max_sbw = max_sbh = 0;
  for (int j = 0; j < n_jobs; j++) {
    const R1MeJob &b = jobs[j];
    R1_REQUIRE(b.stats);
    R1_REQUIRE(b.tile_x >= 0 && b.tile_y >= 0 && b.tile_w > 0 && b.tile_h > 0);
    R1_REQUIRE(b.tile_x % SB == 0 && b.tile_y % SB == 0 && b.tile_w % MI == 0 && b.tile_h % MI == 0);
    R1_REQUIRE((b.tile_x + b.tile_w) / MI <= params->stats_cols &&
               (b.tile_y + b.tile_h) / MI <= params->stats_rows);
    for (int l = 0; l < 3; l++)
      R1_REQUIRE(b.org[l].data && b.ref[l].data && r1_same_px(jobs[0].org[0], b.org[l], b.ref[l]));
    const int sbw = (b.tile_w + SB - 1) / SB, sbh = (b.tile_h + SB - 1) / SB;
    max_sbw = sbw > max_sbw ? sbw : max_sbw;
    max_sbh = sbh > max_sbh ? sbh : max_sbh;
  }
  return R1_OK;
}

// Takes the ring's next slot for a call and stages the call into it (the caller holds ctx->me_mu): job descriptors
// + parameters: caller's memory -> pinned staging (the launch uploads it), and the refinement buffers.
int me_stage_call(r1_ctx *ctx, const R1MeJob *jobs, int n_jobs, const R1MeParams *params, MeStaged &sc) {
  const size_t jobs_bytes = ((size_t)n_jobs * sizeof(R1MeJob) + 15) & ~(size_t)15;
  const size_t params_bytes = (sizeof(R1MeParams) + 15) & ~(size_t)15;
  const size_t bytes = jobs_bytes + params_bytes + (size_t)n_jobs * sizeof(R1MeStats *);
  const int slot = ctx->me_next;
  if (ctx->me_done[slot]) R1_HIP_CHECK(hipEventSynchronize(ctx->me_done[slot]));
  else R1_HIP_CHECK(hipEventCreateWithFlags(&ctx->me_done[slot], hipEventDisableTiming));
  // Fail-safe for callers that never poll r1_me_status: a persistent launch that has FINISHED with a
  // timed-out dependency wait (stale predictors, non-reference statistics) makes every following call
  // refuse with R1_ETIMEDOUT until r1_me_status has reported -- and thereby consumed -- the flag.
  // Nothing is enqueued and the ring does not advance.
  for (int s = 0; s < r1_ctx::kMeSlots; s++) {
    MePersistCache *pc = (MePersistCache *)ctx->me_persist[s];
    if (!pc || !pc->launched || !ctx->me_done[s]) continue;
    if (s != slot && hipEventQuery(ctx->me_done[s]) != hipSuccess) continue;
    me_collect_slot(ctx, *pc);
  }
  if (ctx->me_failed) {
    r1_set_error("r1_estimate_tile_motion_batch: %d earlier call(s) (first: call %llu) ran with a timed-out "
                 "dependency wait and have not been acknowledged; call r1_me_status and re-issue them with "
                 "launch_mode 1", ctx->me_failed, ctx->me_first_failed);
    return R1_ETIMEDOUT;
  }
  ctx->me_calls++;
  ctx->me_next = (slot + 1) % r1_ctx::kMeSlots;
  if (ctx->me_jobs_bytes[slot] < bytes) {
    if (ctx->me_graph[slot]) (void)hipGraphExecDestroy(ctx->me_graph[slot]);   // it holds the old pointers
    ctx->me_graph[slot] = nullptr;
    if (ctx->me_jobs[slot]) (void)hipFree(ctx->me_jobs[slot]);
    if (ctx->me_jobs_host[slot]) (void)hipHostFree(ctx->me_jobs_host[slot]);
    ctx->me_jobs[slot] = ctx->me_jobs_host[slot] = nullptr;
    ctx->me_jobs_bytes[slot] = 0;
    R1_HIP_CHECK(hipMalloc(&ctx->me_jobs[slot], bytes));
    R1_HIP_CHECK(hipHostMalloc(&ctx->me_jobs_host[slot], bytes, hipHostMallocDefault));
    ctx->me_jobs_bytes[slot] = bytes;
  }
  // the refinement buffers: one MEStats frame per DISTINCT statistics array of the call (the tiles
  // of a frame share theirs), same geometry, so a job's entries sit at the same offsets
  const size_t frame_bytes = (size_t)params->stats_cols * params->stats_rows * sizeof(R1MeStats);
  int uniq_of[256], n_uniq = 0;
  for (int j = 0; j < n_jobs; j++) {
    int u = -1;
    for (int k = 0; k < j && u < 0; k++)
      if (jobs[k].stats == jobs[j].stats) u = uniq_of[k];
    uniq_of[j] = u >= 0 ? u : n_uniq++;
  }
  if (ctx->me_refine_bytes[slot] < frame_bytes * n_uniq) {
    if (ctx->me_graph[slot]) (void)hipGraphExecDestroy(ctx->me_graph[slot]);
    ctx->me_graph[slot] = nullptr;
    if (ctx->me_refine[slot]) (void)hipFree(ctx->me_refine[slot]);
    ctx->me_refine[slot] = nullptr;
    ctx->me_refine_bytes[slot] = 0;
    R1_HIP_CHECK(hipMalloc(&ctx->me_refine[slot], frame_bytes * n_uniq));
    ctx->me_refine_bytes[slot] = frame_bytes * n_uniq;
  }
  memcpy(ctx->me_jobs_host[slot], jobs, (size_t)n_jobs * sizeof(R1MeJob));
  memcpy((uint8_t *)ctx->me_jobs_host[slot] + jobs_bytes, params, sizeof(R1MeParams));
  {
    R1MeStats **rp = (R1MeStats **)((uint8_t *)ctx->me_jobs_host[slot] + jobs_bytes + params_bytes);
    for (int j = 0; j < n_jobs; j++)
      rp[j] = (R1MeStats *)((uint8_t *)ctx->me_refine[slot] + frame_bytes * uniq_of[j]);
  }
  const uint8_t *dev = (const uint8_t *)ctx->me_jobs[slot];
  sc = MeStaged{slot, bytes, (const R1MeJob *)dev, (const R1MeParams *)(dev + jobs_bytes),
                (R1MeStats *const *)(dev + jobs_bytes + params_bytes)};
  return R1_OK;
}

// One launch per superblock diagonal (k_me_diag), as a hipGraph built once per geometry and replayed.
int me_launch_diagonals(r1_ctx *ctx, const MeStaged &sc, int n_jobs, int bpp, int max_sbw, int max_sbh,
                        hipStream_t st) {
  const int slot = sc.slot;
  const int ndiag = max_sbw + max_sbh - 1;
  const int dlen = max_sbw < max_sbh ? max_sbw : max_sbh;
  // software pipeline over the passes: launch `step` runs diagonal step - 2 q of pass q
  // (grid z = pass); ndiag + 4 launches instead of 3 * ndiag
  const int nsteps = ndiag + 2 * kPassSkew;
  const void *fn = bpp == 1 ? (const void *)k_me_diag<1> : (const void *)k_me_diag<2>;
  // The sequence (upload, then one launch per diagonal step, each depending on the one before)
  // is a function of (pixel size, jobs, diagonal length, steps) and of the slot's buffers only --
  // the job contents and the parameters travel through the upload.  It is built once as an
  // explicit hipGraph and replayed with a single hipGraphLaunch per call.
  const long long sig[5] = {bpp, n_jobs, dlen, nsteps, (long long)(size_t)ctx->me_refine[slot]};
  if (!ctx->me_graph[slot] || memcmp(sig, ctx->me_graph_sig[slot], sizeof(sig)) != 0) {
    if (ctx->me_graph[slot]) (void)hipGraphExecDestroy(ctx->me_graph[slot]);
    ctx->me_graph[slot] = nullptr;
    hipGraph_t g;
    R1_HIP_CHECK(hipGraphCreate(&g, 0));
    hipGraphNode_t prev;
    hipError_t e = hipGraphAddMemcpyNode1D(&prev, g, nullptr, 0, ctx->me_jobs[slot], ctx->me_jobs_host[slot],
                                           sc.bytes, hipMemcpyHostToDevice);
    for (int step = 0; step < nsteps && e == hipSuccess; step++) {
      int step_arg = step;
      void *args[4] = {(void *)&sc.djobs, (void *)&sc.dparams, (void *)&sc.drbufs, (void *)&step_arg};
      hipKernelNodeParams kp;
      memset(&kp, 0, sizeof(kp));
      kp.func = (void *)fn;
      kp.gridDim = dim3(dlen, n_jobs, 5);   // roles: three searches, two refinements (k_me_diag)
      kp.blockDim = dim3(256);
      kp.sharedMemBytes = 0;
      kp.kernelParams = args;   // copied at node creation
      hipGraphNode_t node;
      e = hipGraphAddKernelNode(&node, g, &prev, 1, &kp);
      prev = node;
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&ctx->me_graph[slot], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) {
      ctx->me_graph[slot] = nullptr;
      R1_HIP_CHECK(e);
    }
    memcpy(ctx->me_graph_sig[slot], sig, sizeof(sig));
  }
  R1_HIP_CHECK(hipGraphLaunch(ctx->me_graph[slot], st));
  R1_HIP_CHECK(hipEventRecord(ctx->me_done[slot], st));
  return R1_OK;
}
}  // namespace

// Results of the persistent tile-ME launches (launch_mode 2 / 3) are valid once this has said so:
// a wave whose dependency wait runs out of patience (a bounded spin, so that a placement the
// protocol did not foresee cannot hang the GPU) goes on with stale predictors and flags the call.
// wait != 0: first waits for every launch enqueued so far.  Returns R1_OK when no call since the
// last r1_me_status has been flagged; R1_ETIMEDOUT otherwise, with *first_failed_call = the 1-based
// index (per context) of the first flagged r1_estimate_tile_motion_batch call -- the caller
// re-issues that call with launch_mode = 1 (the launch-boundary version has no waits).  Flags are
// consumed by the report.  *calls (optional) = calls made on this context so far.
extern "C" int r1_me_status(r1_ctx *ctx, int wait, unsigned long long *first_failed_call,
                            unsigned long long *calls) {
  R1_REQUIRE(ctx);
  std::lock_guard<std::mutex> ring_lock(ctx->me_mu);
  R1DeviceGuard dev_guard(ctx);
  for (int s = 0; s < r1_ctx::kMeSlots; s++) {
    MePersistCache *c = (MePersistCache *)ctx->me_persist[s];
    if (!c || !c->launched || !ctx->me_done[s]) continue;
    if (wait) R1_HIP_CHECK(hipEventSynchronize(ctx->me_done[s]));
    else if (hipEventQuery(ctx->me_done[s]) != hipSuccess) continue;
    me_collect_slot(ctx, *c);
  }
  if (calls) *calls = ctx->me_calls;
  if (first_failed_call) *first_failed_call = ctx->me_first_failed;
  const bool bad = ctx->me_failed != 0;
  if (bad) r1_set_error("k_me_persist: %d call(s) flagged a timed-out dependency wait, first: call %llu; "
                        "re-issue with launch_mode 1", ctx->me_failed, ctx->me_first_failed);
  ctx->me_failed = 0;
  ctx->me_first_failed = 0;
  return bad ? R1_ETIMEDOUT : R1_OK;
}

void r1_me_persist_free(void *cache) {
  MePersistCache *c = (MePersistCache *)cache;
  if (!c) return;
  for (void *p : {c->rows, c->foff, c->prog, c->ctl})
    if (p) (void)hipFree(p);
  if (c->err_host) (void)hipHostFree(c->err_host);
  delete c;
}

extern "C" int r1_estimate_tile_motion_batch(r1_ctx *ctx, const R1MeJob *jobs, int n_jobs,
                                             const R1MeParams *params, void *stream) {
  R1_REQUIRE(ctx && params);
  if (n_jobs <= 0) return R1_OK;
  int bpp, max_sbw, max_sbh;
  if (const int rc = me_check_jobs(jobs, n_jobs, params, bpp, max_sbw, max_sbh)) return rc;
  hipStream_t st = (hipStream_t)stream;
  // one ring slot per call.  The ring is the one piece of mutable state a context has: concurrent callers (rav1e's
  // per-tile rayon workers share a context) take turns for the enqueue.
  std::lock_guard<std::mutex> ring_lock(ctx->me_mu);
  R1DeviceGuard dev_guard(ctx);
  MeStaged sc;
  if (const int rc = me_stage_call(ctx, jobs, n_jobs, params, sc)) return rc;
  // one persistent launch (k_me_persist) or one launch per superblock diagonal (k_me_diag): the
  // pinned persistent path (2) puts every job on one XCD, so it wants a job per XCD; below that the
  // unpinned one (3: any wave takes any row, results written through at agent scope).  Measured,
  // 8-bit 4K, ms, diagonal launches / pinned / unpinned: 1 job 4.12 / 9.9 / 2.91, 4 jobs 4.80 / 4.7 /
  // 3.96, 8 jobs 1.74 / 1.14 / 1.31, 16 jobs 2.93 / 2.08 / 2.29, 64 jobs 2.03 / 1.69 / 1.77
  int mode = params->launch_mode ? params->launch_mode : (n_jobs >= 8 ? 2 : 3);
  R1_REQUIRE(mode >= 1 && mode <= 3);
  if (mode == 2) {
    if (ctx->me_xcds < 0) { const int rc = me_probe_xcds(ctx, st); if (rc != R1_OK) return rc; }
    if (ctx->me_xcds != 8) {
      if (params->launch_mode == 2) {
        r1_set_error("r1_estimate_tile_motion_batch: launch_mode 2 needs a device whose launches spread over 8 XCDs");
        return R1_EINVAL;
      }
      mode = 3;
    }
  }
  if (mode >= 2) return me_launch_persistent(ctx, sc, jobs, n_jobs, bpp, st, mode == 2);
  return me_launch_diagonals(ctx, sc, n_jobs, bpp, max_sbw, max_sbh, st);
}

// head_rate.hip -- the entry points of the head-symbol unit (its kernels: head_rate_kernel.hpp): the intra head symbols
// of an intra frame on the device.
// r1_intra_head_rate_batch: the head's tell_frac difference per mode trial -- rate_add of r1_rd_pick_batch -- and the
// writer's rng behind it, stored where r1_coeff_rate_block_batch starts from.
// r1_partition_rate_batch: write_partition alone, the part_rate of r1_rd_partition_pick_batch.
// r1_intra_head_commit_batch: the winner's symbols on its R1HeadCdfContext, and what the coded block leaves on its
// R1HeadNbrContext.  r1_head_nbr_reset_left_batch: the head part of reset_left_contexts.
// All enqueue on the caller's stream; nothing is read back.  Pinned by tests/golden/head_ref.npz.
#include "head_rate_kernel.hpp"

static unsigned head_grid(long long n, int lanes) { return (unsigned)((n * lanes + 255) / 256); }

// depth_state and tx_sizes come together; the table holds three TxSize
static int head_tx_sizes(const R1RdPick *depth_state, const uint8_t *tx_sizes, uint32_t &out) {
  R1_REQUIRE((depth_state != nullptr) == (tx_sizes != nullptr));
  out = 0;
  if (tx_sizes)
    for (int k = 0; k < 3; k++) {
      R1_REQUIRE(r1_tx_size_ok(tx_sizes[k]));
      out |= (uint32_t)tx_sizes[k] << (8 * k);
    }
  return R1_OK;
}

extern "C" int r1_intra_head_rate_batch(r1_ctx *ctx, const R1HeadNbrContext *nbrs, int n_nbrs, const R1HeadCdfContext *cdfs,
                                        int n_cdfs, const R1HeadBlock *blocks, int n_blocks, const R1HeadTrial *trials,
                                        int n, const R1RdPick *depth_state, const uint8_t *tx_sizes,
                                        const int16_t *cfl_alpha, uint32_t *rate_add_out, void *rng_out,
                                        long long rng_stride, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(nbrs && cdfs && blocks && trials && rate_add_out);
  R1_REQUIRE(n >= 0 && n_nbrs >= 1 && n_cdfs >= 1 && n_blocks >= 1);
  R1_REQUIRE(!rng_out || (rng_stride >= 2 && rng_stride % 2 == 0 && ((uintptr_t)rng_out & 1) == 0));
  HeadRateArgs a = {};
  const int rc = head_tx_sizes(depth_state, tx_sizes, a.tx_sizes);
  if (rc != R1_OK) return rc;
  if (n == 0) return R1_OK;
  a.nbrs = nbrs, a.cdfs = cdfs, a.blocks = blocks, a.trials = trials, a.depth_state = depth_state, a.cfl_alpha = cfl_alpha;
  a.rate_add = rate_add_out, a.rng_out = (uint8_t *)rng_out, a.rng_stride = rng_stride;
  a.n = n, a.n_nbrs = n_nbrs, a.n_cdfs = n_cdfs, a.n_blocks = n_blocks;
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_intra_head_rate, dim3(head_grid(n, 1)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_partition_rate_batch(r1_ctx *ctx, const R1HeadNbrContext *nbrs, int n_nbrs, const R1HeadCdfContext *cdfs,
                                       int n_cdfs, const R1HeadBlock *nodes, const uint8_t *partitions, int n,
                                       const uint16_t *rng_in, uint32_t *part_rate_out, uint16_t *rng_out, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(nbrs && cdfs && nodes && partitions && part_rate_out);
  R1_REQUIRE(n >= 0 && n_nbrs >= 1 && n_cdfs >= 1);
  if (n == 0) return R1_OK;
  const PartRateArgs a = {nbrs, cdfs, nodes, partitions, rng_in, part_rate_out, rng_out, n, n_nbrs, n_cdfs};
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_partition_rate, dim3(head_grid(n, 1)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_intra_head_commit_batch(r1_ctx *ctx, R1HeadNbrContext *nbrs, int n_nbrs, R1HeadCdfContext *cdfs,
                                          int n_cdfs, const R1HeadBlock *blocks, int n_blocks, const R1HeadTrial *trials,
                                          int n_trials, const R1HeadCommit *commits, const R1RdPick *state, int n_states,
                                          int call_id, int group, int nt, const R1RdPick *depth_state,
                                          const uint8_t *tx_sizes, const int16_t *cfl_alpha, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(nbrs && cdfs && blocks && trials && commits && state);
  R1_REQUIRE(n_states >= 0 && n_nbrs >= 1 && n_cdfs >= 1 && n_blocks >= 1 && n_trials >= 1);
  R1_REQUIRE(call_id >= 0 && call_id <= 127);
  R1_REQUIRE(group >= 1 && group <= 4096 && nt >= 1 && nt <= 16);
  HeadCommitArgs a = {};
  const int rc = head_tx_sizes(depth_state, tx_sizes, a.tx_sizes);
  if (rc != R1_OK) return rc;
  if (n_states == 0) return R1_OK;
  a.nbrs = nbrs, a.cdfs = cdfs, a.blocks = blocks, a.trials = trials, a.commits = commits, a.state = state;
  a.depth_state = depth_state, a.cfl_alpha = cfl_alpha;
  a.n_states = n_states, a.n_nbrs = n_nbrs, a.n_cdfs = n_cdfs, a.n_blocks = n_blocks, a.n_trials = n_trials;
  a.call_id = call_id, a.group = group, a.nt = nt;
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_intra_head_commit, dim3(head_grid(n_states, 1)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_head_nbr_reset_left_batch(r1_ctx *ctx, R1HeadNbrContext *nbrs, int n_nbrs, const uint32_t *sel, int n,
                                            void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(nbrs && sel);
  R1_REQUIRE(n >= 0 && n_nbrs >= 1);
  if (n == 0) return R1_OK;
  const HeadResetArgs a = {nbrs, sel, n, n_nbrs};
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_head_nbr_reset_left, dim3(head_grid(n, 32)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

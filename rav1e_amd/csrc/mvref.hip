// mvref.hip -- the entry points of the MV-stack unit (its kernels: mvref_kernel.hpp): the tile's blocks array on the
// device and the MV reference stack of an inter block over it.
// r1_tile_blocks_reset_batch: Block::default() over whole arrays.  r1_tile_blocks_store_batch: what a coded block leaves
// (set_skip, set_block_size, set_mode, set_ref_frames, set_motion_vectors), gated like r1_intra_head_commit_batch.
// r1_mvref_stack_batch: find_mvrefs / setup_mvref_list for every query of a batch of blocks, one wave per block.
// r1_mvref_pmv_batch: the stack's first two vectors to where r1_estimate_motion_batch reads pmv.
// All enqueue on the caller's stream; nothing is read back.  The descriptors travel in the launch's arguments.
// Pinned by tests/golden/mvref_ref.npz.
#include "mvref_kernel.hpp"

// the descriptors of a call, checked and copied into the launch's arguments
static int mv_tiles(const R1TileBlocks *tiles, int n_tiles, MvTiles &out) {
  R1_REQUIRE(tiles);
  R1_REQUIRE(n_tiles >= 1 && n_tiles <= R1_MVREF_MAX_TILES);
  for (int i = 0; i < n_tiles; i++) {
    const R1TileBlocks &t = tiles[i];
    R1_REQUIRE(t.cells && ((uintptr_t)t.cells & 15) == 0);
    R1_REQUIRE(t.cols >= 1 && t.rows >= 1 && t.stride >= t.cols);
    R1_REQUIRE(t.cols <= 1024 && t.stride <= 1024 && t.rows <= 65535);
    R1_REQUIRE(t.tile_x >= 0 && t.tile_y >= 0);
    R1_REQUIRE(t.frame_cols <= (1 << 20) && t.frame_rows <= (1 << 20));
    R1_REQUIRE(t.frame_cols - t.tile_x >= t.cols && t.frame_rows - t.tile_y >= t.rows);
    out.t[i] = t;
  }
  return R1_OK;
}

extern "C" int r1_tile_blocks_reset_batch(r1_ctx *ctx, const R1TileBlocks *tiles, int n_tiles, const int32_t *sel, int n,
                                          void *stream) {
  R1_REQUIRE(ctx);
  TileResetArgs a = {};
  const int rc = mv_tiles(tiles, n_tiles, a.tiles);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(n >= 0 && n <= R1_MVREF_MAX_TILES);
  R1_REQUIRE(sel || n == n_tiles);
  long long most = 0;
  for (int i = 0; i < n; i++) {
    const int k = sel ? sel[i] : i;
    R1_REQUIRE(k >= 0 && k < n_tiles);
    a.sel[i] = (uint8_t)k;
    const long long cells = (long long)tiles[k].rows * tiles[k].stride;
    most = cells > most ? cells : most;
  }
  if (n == 0) return R1_OK;
  const long long want = (most + 255) / 256;
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_tile_blocks_reset, dim3((unsigned)(want < 1024 ? want : 1024), (unsigned)n), dim3(256), 0,
                     (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_tile_blocks_store_batch(r1_ctx *ctx, const R1TileBlocks *tiles, int n_tiles, const R1MvBlock *blocks,
                                          int n_blocks, const R1MvTrial *trials, int n_trials, const R1RdPick *state, int n,
                                          int call_id, int group, int nt, void *stream) {
  R1_REQUIRE(ctx);
  TileStoreArgs a = {};
  const int rc = mv_tiles(tiles, n_tiles, a.tiles);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(blocks && trials);
  R1_REQUIRE(n >= 0 && n_blocks >= 1 && n_trials >= 1);
  R1_REQUIRE(call_id >= 0 && call_id <= 127);
  R1_REQUIRE(group >= 1 && group <= 4096 && nt >= 1 && nt <= 16);
  R1_REQUIRE(state || n <= n_trials);
  if (n == 0) return R1_OK;
  a.blocks = blocks, a.trials = trials, a.state = state;
  a.n = n, a.n_tiles = n_tiles, a.n_blocks = n_blocks, a.n_trials = n_trials, a.call_id = call_id, a.group = group, a.nt = nt;
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_tile_blocks_store, dim3((unsigned)n), dim3(kMvLanes), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_mvref_stack_batch(r1_ctx *ctx, const R1TileBlocks *tiles, int n_tiles, const R1MvBlock *blocks, int n_blocks,
                                    const R1MvQuery *queries, int n_queries, int max_queries, const uint8_t *sign_bias,
                                    R1MvStack *stacks_out, void *stream) {
  R1_REQUIRE(ctx);
  MvStackArgs a = {};
  const int rc = mv_tiles(tiles, n_tiles, a.tiles);
  if (rc != R1_OK) return rc;
  R1_REQUIRE(blocks && queries && sign_bias && stacks_out);
  R1_REQUIRE(((uintptr_t)stacks_out & 3) == 0);
  R1_REQUIRE(n_blocks >= 0 && n_queries >= 1);
  R1_REQUIRE(max_queries >= 1 && max_queries <= R1_MVREF_MAX_QUERIES);
  if (n_blocks == 0) return R1_OK;
  a.blocks = blocks, a.queries = queries, a.out = stacks_out;
  a.n_blocks = n_blocks, a.n_queries = n_queries, a.n_tiles = n_tiles, a.max_queries = max_queries;
  for (int k = 0; k < 8; k++) a.sign_bias[k] = sign_bias[k] ? 1 : 0;
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_mvref_stack, dim3((unsigned)n_blocks), dim3(kMvLanes), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

extern "C" int r1_mvref_pmv_batch(r1_ctx *ctx, const R1MvStack *stacks, int n, void *pmv_out, long long stride, void *stream) {
  R1_REQUIRE(ctx);
  R1_REQUIRE(stacks && pmv_out);
  R1_REQUIRE(n >= 0);
  R1_REQUIRE(stride >= 8 && stride % 2 == 0 && ((uintptr_t)pmv_out & 1) == 0);
  if (n == 0) return R1_OK;
  const MvPmvArgs a = {stacks, (uint8_t *)pmv_out, stride, n};
  R1DeviceGuard guard(ctx);
  hipLaunchKernelGGL(k_mvref_pmv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  R1_HIP_CHECK(hipGetLastError());
  return R1_OK;
}

// Prints what rav1e_amd/csrc/block_geom.hpp says, as the host compiler sees it; tests/test_block_geom.py holds every
// line against the host statements the fixtures pin to the reference.
//   B bw bh xdec ydec size_ok sub_ok admits [every R1BlockGeom field in its order, where the three hold]
//   L bw bh tx_size ntx gw tw4 th4 divides          every block size x the 19 transform sizes
//   T tx_size is_inter reduced set mask num_tx_set uv_rule txs_ctx sqr sqr_up ind[0..15]
#include <cstdio>

#include "block_geom.hpp"

int main() {
  const int sides[8] = {2, 4, 8, 12, 16, 32, 64, 128};
  for (int bw : sides)
    for (int bh : sides)
      for (int xdec = 0; xdec < 2; xdec++)
        for (int ydec = 0; ydec < 2; ydec++) {
          const bool size = r1_block_size_ok(bw, bh), sub = r1_subsampling_ok(xdec, ydec),
                     admits = r1_subsampling_admits(xdec, ydec, bw, bh);
          std::printf("B %d %d %d %d %d %d %d", bw, bh, xdec, ydec, (int)size, (int)sub, (int)admits);
          if (!(size && sub && admits)) {
            std::printf("\n");
            continue;
          }
          const R1BlockGeom g = r1_block_geom(bw, bh, xdec, ydec);
          std::printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", g.bw4, g.bh4, g.sub_w4, g.sub_h4, g.uv_tx_size,
                      g.uw, g.uh, g.bw_uv, g.bh_uv, g.uv_w4, g.uv_h4, g.adj_x, g.adj_y, g.uv_skip_off, g.skip_all_planes);
        }
  for (int bw : sides)
    for (int bh : sides)
      for (int ts = 0; ts < 19 && r1_block_size_ok(bw, bh); ts++) {
        const R1LumaGrid l = r1_luma_grid(bw, bh, ts);
        std::printf("L %d %d %d %d %d %d %d %d\n", bw, bh, ts, l.ntx, l.gw, l.tw4, l.th4, (int)l.divides);
      }
  for (int ts = 0; ts < 19; ts++)
    for (int inter = 0; inter < 2; inter++)
      for (int reduced = 0; reduced < 2; reduced++) {
        const int set = r1_tx_set(ts, inter, reduced);
        std::printf("T %d %d %d %d %u %d %d %d %d %d", ts, inter, reduced, set, (unsigned)r1tx::kTxUsed[set],
                    (int)r1tx::kNumTxSet[set], r1_uv_inter_rule(ts), r1_txs_ctx(ts), r1_txsize_sqr_log2(ts),
                    r1_txsize_sqr_up_log2(ts));
        for (int t = 0; t < 16; t++) std::printf(" %d", (int)r1tx::kTxInd[set][t]);
        std::printf("\n");
      }
  return 0;
}

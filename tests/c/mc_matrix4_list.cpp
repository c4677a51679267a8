// Prints, as the host compiler sees them, the pieces of the 4x4x4-block form of the matrix-pipe horizontal filter pass
// that tests/test_mc_matrix4_layout.py checks against a NumPy restatement of v_mfma_i32_4x4x4_16b_i8: the fragment
// geometry and the tap dwords (r1mc::mx4_*, rav1e_amd/csrc/mc_window.hpp), the packed half-tap table the kernels load
// (kTapI8, mc_taps_packed.inc) and what the plan (rdo_cand_plan.hpp) chooses.
//   P bd wl MC_MATRIX4 MX_NC NC WS WIN_BYTES SRC_OFF SRC_BYTES MX4_A_END LDS_BYTES   per square coefficient kernel
//   Q w nc ws quads a_end                                                           per layout (w = h = 16, 8)
//   A w c quad s row offset                                                         per layout, column, quad and dword
//   T set frac fx0 fx1                                                              per row of the tap table
//   B set frac j t0 t1 t2                                                           per row and byte phase j = c & 3
#include <cstdint>
#include <cstdio>

#include "rdo_cand_plan.hpp"

#define __constant__
#include "mc_taps_packed.inc"

template <int BD, int WL>
void plan() {
  using PL = RdoCandPlan<BD, WL, WL, 0, false, 0>;
  std::printf("P %d %d %d %d %d %d %d %d %d %d %d\n", BD, WL, (int)PL::MC_MATRIX4, PL::MX_NC, PL::NC, PL::WS, PL::WIN_BYTES,
              PL::SRC_OFF, PL::SRC_BYTES, PL::MX4_A_END, PL::LDS_BYTES);
}

static void layout(int w) {
  const int h = w, nc = 64 / w, ws = r1mc::window_stride(w, 1), quads = r1mc::mx_quads(h);
  std::printf("Q %d %d %d %d %d\n", w, nc, ws, quads, r1mc::mx4_a_end(nc, w, h, ws));
  for (int c = 0; c < w; c++)
    for (int q = 0; q < quads; q++)
      for (int s = 0; s < 3; s++)
        std::printf("A %d %d %d %d %d %d\n", w, c, q, s, r1mc::mx4_a_row(c, q), r1mc::mx4_a_offset(c, q, s, ws));
}

int main() {
  plan<8, 3>(), plan<8, 4>(), plan<8, 5>(), plan<8, 6>();
  plan<10, 3>(), plan<10, 4>(), plan<10, 5>(), plan<10, 6>();
  plan<12, 3>(), plan<12, 4>(), plan<12, 5>(), plan<12, 6>();
  layout(16), layout(8);
  (void)kTapI16, (void)kTapB;
  for (int f = 0; f < 6; f++)
    for (int q = 0; q < 16; q++) {
      std::printf("T %d %d %u %u\n", f, q, kTapI8[f][q][0], kTapI8[f][q][1]);
      for (int j = 0; j < 4; j++)
        std::printf("B %d %d %d %u %u %u\n", f, q, j, r1mc::mx4_band(kTapI8[f][q][0], kTapI8[f][q][1], j, 0),
                    r1mc::mx4_band(kTapI8[f][q][0], kTapI8[f][q][1], j, 1), r1mc::mx4_band(kTapI8[f][q][0], kTapI8[f][q][1], j, 2));
    }
  return 0;
}

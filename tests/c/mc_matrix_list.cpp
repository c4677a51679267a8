// Prints, as the host compiler sees them, the pieces of the matrix-pipe horizontal filter pass that
// tests/test_mc_matrix_layout.py checks against a NumPy restatement of the MFMA's index algebra: the fragment geometry
// and the band builder (r1mc::mx_*, rav1e_amd/csrc/mc_window.hpp), the packed half-tap table the kernels load
// (kTapI8, mc_taps_packed.inc) and where the plan (rdo_cand_plan.hpp) turns the pass on.
//   P bd wl MX_NC WS WIN_BYTES SRC_OFF SRC_BYTES MX_ZERO_OFF MX_ZERO_BYTES LDS_BYTES   per square coefficient kernel
//   Q nc h ws quads a_end zero_bytes                                                    per layout
//   G nc lane a_offset a_cand                                                           per layout and lane
//   T set frac fx0 fx1                                                                  per row of the tap table
//   B set frac lane band                                                                per row and lane
#include <cstdint>
#include <cstdio>

#include "rdo_cand_plan.hpp"

#define __constant__
#include "mc_taps_packed.inc"

template <int BD, int WL>
void plan() {
  using PL = RdoCandPlan<BD, WL, WL, 0, false, 0>;
  std::printf("P %d %d %d %d %d %d %d %d %d %d\n", BD, WL, PL::MX_NC, PL::WS, PL::WIN_BYTES, PL::SRC_OFF, PL::SRC_BYTES,
              PL::MX_ZERO_OFF, PL::MX_ZERO_BYTES, PL::LDS_BYTES);
}

static void layout(int nc) {
  const int h = 64 / nc, ws = r1mc::window_stride(h, 1);
  std::printf("Q %d %d %d %d %d %d\n", nc, h, ws, r1mc::mx_quads(h), r1mc::mx_a_end(nc, h, ws), r1mc::mx_zero_bytes(h, ws));
  for (int l = 0; l < 64; l++) std::printf("G %d %d %d %d\n", nc, l, r1mc::mx_a_offset(l, nc, h, ws), r1mc::mx_a_cand(l, nc));
}

int main() {
  plan<8, 3>(), plan<8, 4>(), plan<8, 5>(), plan<8, 6>();
  plan<10, 3>(), plan<10, 4>(), plan<10, 5>(), plan<10, 6>();
  plan<12, 3>(), plan<12, 4>(), plan<12, 5>(), plan<12, 6>();
  layout(1), layout(2);
  (void)kTapI16, (void)kTapB;
  for (int f = 0; f < 6; f++)
    for (int q = 0; q < 16; q++) {
      std::printf("T %d %d %u %u\n", f, q, kTapI8[f][q][0], kTapI8[f][q][1]);
      for (int l = 0; l < 64; l++)
        std::printf("B %d %d %d %llu\n", f, q, l, r1mc::mx_band8(kTapI8[f][q][0], kTapI8[f][q][1], l));
    }
  return 0;
}

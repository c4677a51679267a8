// Prints the route an r1_rdo_intra_cand_batch call takes (rdo_intra_route, rav1e_amd/csrc/rdo_cand_plan.hpp) as the
// host compiler sees it: one line "BD WL HL QM ROUTE" per bit depth, transform size and QM 1 / 2 (dist_kind 0 / a
// pixel-domain kind); ROUTE 0 = fan-out, 1 = one launch per type, 2 = the two launches.  tests/test_gpu_depth12.py
// asks it which sizes have a fused and a two-launch point at 12 bits.
#include <cstdio>

#include "rdo_cand_plan.hpp"

int main() {
  for (int bd = 8; bd <= 12; bd += 2)
    for (int wl = 2; wl <= 6; wl++)
      for (int hl = 2; hl <= 6; hl++)
        for (int qm = 1; qm <= 2; qm++)
          if (rdo_tx_size_exists(wl, hl)) std::printf("%d %d %d %d %d\n", bd, wl, hl, qm, (int)rdo_intra_route(wl, hl, bd, qm));
  return 0;
}

// Prints, for every (bit depth, size, QM, MT, PS) the high-word multiply form (m24w, tx_common.hpp) is built or enabled
// for, the plan's choices and the input bounds its two passes hand to the networks (rdo_cand_plan.hpp).  Host compiler
// alone; read by tests/test_tx_mul_hiword.py.
//   bd wl hl qm mt ps built on halve2 col_fold col_bound(shift[0] = 4) row_bound
#include <cstdio>

#include "rdo_cand_plan.hpp"

int main() {
  for (int bd = 8; bd <= 12; bd += 2)
    for (int wl = 2; wl <= 6; wl++)
      for (int hl = 2; hl <= 6; hl++)
        for (int qm = 0; qm < 3; qm++)
          for (int mt = 0; mt < 2; mt++)
            for (int ps = 0; ps < 2; ps++) {
              const bool built = rdo_mul_hiword_built(bd, wl, hl, qm, mt, ps), on = rdo_mul_hiword(bd, wl, hl, qm, mt, ps);
              if (!built && !on) continue;
              const bool cf = rdo_col_fold(bd, wl, hl, qm, mt, ps);
              std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", bd, wl, hl, qm, mt, ps, (int)built, (int)on,
                          (int)rdo_halve2(bd, wl, hl, qm, mt, ps), (int)cf, rdo_mul_col_bound(bd, 4, cf),
                          rdo_mul_row_bound(bd, wl, hl));
            }
}

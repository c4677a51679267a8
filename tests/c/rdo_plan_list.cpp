// Prints the fused candidate kernel's plan (rav1e_amd/csrc/rdo_cand_plan.hpp) as the host compiler sees it: one line
// "BD WL HL QM MT PS LDS_BYTES" per instantiation that rdo_cand_instantiated names, over the 19 transform sizes x
// {8, 10, 12} bits x QM 0..2 x MT x PS.  tests/test_rdo_plan.py holds the list against the built library.
#include <cstdio>

#include "rdo_cand_plan.hpp"

template <int BD, int WL, int HL, int QM, bool MT, int PS>
void one() {
  if constexpr (rdo_cand_instantiated(BD, WL, HL, QM, MT, PS))
    std::printf("%d %d %d %d %d %d %d\n", BD, WL, HL, QM, (int)MT, PS, RdoCandPlan<BD, WL, HL, QM, MT, PS>::LDS_BYTES);
}
template <int BD, int WL, int HL, int QM>
void forms() {
  one<BD, WL, HL, QM, false, 0>();
  one<BD, WL, HL, QM, true, 0>();
  one<BD, WL, HL, QM, false, 1>();
  one<BD, WL, HL, QM, true, 1>();
}
template <int WL, int HL>
void size() {
  static_assert(rdo_tx_size_exists(WL, HL), "one of the 19");
  forms<8, WL, HL, 0>(), forms<8, WL, HL, 1>(), forms<8, WL, HL, 2>();
  forms<10, WL, HL, 0>(), forms<10, WL, HL, 1>(), forms<10, WL, HL, 2>();
  forms<12, WL, HL, 0>(), forms<12, WL, HL, 1>(), forms<12, WL, HL, 2>();
}

int main() {
  // the TxSize ids 0 .. 18 as (log2 width, log2 height)
  size<2, 2>(), size<3, 3>(), size<4, 4>(), size<5, 5>(), size<6, 6>(), size<2, 3>(), size<3, 2>(), size<3, 4>();
  size<4, 3>(), size<4, 5>(), size<5, 4>(), size<5, 6>(), size<6, 5>(), size<2, 4>(), size<4, 2>(), size<3, 5>();
  size<5, 3>(), size<4, 6>(), size<6, 4>();
  return 0;
}

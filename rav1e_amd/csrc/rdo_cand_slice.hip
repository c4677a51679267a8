// rdo_cand_slice.hip -- one (bit depth, slice) of the fused candidate kernel (rdo_cand_kernel.hpp), chosen by
// -DR1_RDO_TU_BD=8|10|12 -DR1_RDO_TU_QM=0..4: its k_rdo_cand instantiations and the r1_rdo_slice_b<BD>_q<QM>
// function that rdo_dispatch (rdo_cand.hip) calls.  Compiled fifteen times (Makefile: rdo_cand_b<BD>_q<QM>.o).
// With -DR1_RDO_TU_INTRA (slices 1..4, twelve more objects: rdo_cand_i_b<BD>_q<QM>.o): the same slice with the intra
// prediction source (PS = 1) and the r1_rdo_islice_b<BD>_q<QM> function that r1_rdo_intra_cand_batch calls.
#include "rdo_cand_kernel.hpp"

#define R1_CAT2(A, B) A##B
#define R1_CAT4(A, B, C, D) A##B##C##D
#define R1_SLICE_NAME(B, Q) R1_CAT4(r1_rdo_slice_b, B, _q, Q)
// slice numbers 0..2 = QM; 3 / 4 = the type-search (MT) instantiations of QM 1 / 2
#ifdef R1_RDO_TU_INTRA
#define R1_ISLICE_NAME(B, Q) R1_CAT4(r1_rdo_islice_b, B, _q, Q)
int R1_ISLICE_NAME(R1_RDO_TU_BD, R1_RDO_TU_QM)(R1_INTRA_SLICE_ARGS) {
  return slice<R1_RDO_TU_BD, (R1_RDO_TU_QM >= 3 ? R1_RDO_TU_QM - 2 : R1_RDO_TU_QM), (R1_RDO_TU_QM >= 3), 1>(
      tx_size, org, R1Plane{}, nullptr, n, sad, satd, nullptr, pred, qa, st, ia);
}
#else
int R1_SLICE_NAME(R1_RDO_TU_BD, R1_RDO_TU_QM)(R1_SLICE_ARGS) {
  return slice<R1_RDO_TU_BD, (R1_RDO_TU_QM >= 3 ? R1_RDO_TU_QM - 2 : R1_RDO_TU_QM), (R1_RDO_TU_QM >= 3)>(
      tx_size, org, ref, cands, n, sad, satd, coeffs, pred, qa, st);
}
#endif

#ifdef R1_PHASE_PROF
// make prof: r1_debug_phase_prof_b<BD> reads (and clears) the phase timers of this slice's kernels
#define R1_PROF_NAME(B) R1_CAT2(r1_debug_phase_prof_b, B)
extern "C" int R1_PROF_NAME(R1_RDO_TU_BD)(unsigned long long *out, int reset) {   /* out[4096][8] */
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), 4096 * 64) != hipSuccess) return -1;
  if (reset) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_phase)) != hipSuccess) return -1;
    if (hipMemset(p, 0, 4096 * 64) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// sgr_trial.hpp -- the one call between the two halves of rdo_loop_decision's later CDEF passes (rdo.rs:2407-2530):
// cdef_search.hip (r1_cdef_lrf_trial_batch) writes a superblock's trial output per strength index, lrf_search.hip
// restores it with the unit's current choice and adds rdo_loop_plane_error to the sums the CDEF kernels use.
// Host declaration only: the tile engine stays out of the CDEF units.
#pragma once
#include "common.hpp"

// the restoration trial of one plane (k_sgr_trial_err, lrf_search.hip); not part of the C ABI
__attribute__((visibility("hidden")))
int r1i_sgr_trial_err_launch(const R1Plane &trial, size_t trial_idx_bytes, const R1Plane &cdef_cur, const R1Plane &src,
                             const R1TrialUnit *units, int n_units, int n_idx, int pli, int xdec, int ydec,
                             const uint32_t *scales, int scale_stride, unsigned long long *psum, int n_sb, hipStream_t st);

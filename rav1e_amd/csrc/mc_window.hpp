// mc_window.hpp -- the geometry of a staged reference window (mc_common.hpp), for the units that only size one.
// No device code and nothing of HIP: the fused kernel's plan (rdo_cand_plan.hpp) reads it under a host compiler.
#pragma once

namespace r1mc {

// Bytes between the rows of the window of a block (or slab) w pixels wide: its w + 7 pixels, rounded up to whole
// dwords.  A constexpr function: callable from host and device code alike.
constexpr int window_stride(int w, int bpp) { return (((w + 7) * bpp + 3) >> 2) << 2; }

}  // namespace r1mc

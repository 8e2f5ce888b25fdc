// ge_dims.hpp -- the dimension bounds and LDS record shape the kernels (ge_pair.hpp) and
// the host schedules (ge_fa_sched.hpp) share.  Host only, no includes beyond <cstddef>.
#pragma once

#include <cstddef>

namespace ge {

// Dimensions.  Every kernel takes D at compile time, 1..kMaxDim (the oracle's
// bound).  D <= kNarrowMaxDim has every schedule: the one-workgroup kernel, the
// persistent coarsest-level kernel, the symmetric sweeps, FAST mode and all the
// lane / row-slot variants.  Above it only the "wide" schedule is compiled: the
// ordered-pair kernels, the fused step and the one-workgroup kernel's general form
// in one variant each (REPEL_ONE = false and LINEAR = false, which give the same
// bits as their specialisations) and two or three group sizes, because
// per-lane state grows as xi[D] + acc[D] + e[D] and the build as the number of
// instantiations.  GE_WIDE_MIN_DIM (default kNarrowMaxDim + 1) sends
// smaller dimensions through the wide schedule too: same results, for comparisons
// (wide_dim, ge_pair.hpp).
constexpr int kMaxDim = 16;
constexpr int kNarrowMaxDim = 4;

// Doubles per LDS member record {x_0..x_{D-1}, deg+1}: 4 up to D = 3 and 8 up to
// D = 7 (the widths D <= 4 has always had), then D + 1 rounded up to even, so that
// records stay 16-byte aligned for ds_read_b128.
constexpr int rec_width(int D) { return D + 1 <= 4 ? 4 : D + 1 <= 8 ? 8 : (D + 2) & ~1; }

// LDS a workgroup may use on gfx950 (160 KiB), less 1 KiB kept for the kernels'
// small static arrays.
constexpr size_t kLdsBlock = 160 * 1024 - 1024;

}  // namespace ge

// ge_group.hpp -- the ordered sum of a row's terms over the G lanes that share the row,
// for the kernels that keep a level in one workgroup (fa_small_strict, ge_fa.hip) or one
// graph per wave or workgroup (ge_fa_batch.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "ge_internal.hpp"
#include "ge_pair.hpp"
#include "ge_rows.hpp"  // wave_lds_sync

namespace ge {

// The G lanes of a group hold U terms each (term u of lane g is partner
// g + G*u of the chunk); the group's first lane adds the first cnt in order.
// SKIP: the leader stops reading at the first batch of 8 slots past cnt (none of them is
// added): the same adds, for callers whose chunks are mostly short (ge_fa_batch.hip: a
// graph of n rows has chunks of n < G partners, and rows of a few entries).
template <int D, int G, int U, bool SKIP = false>
__device__ __forceinline__ void group_add(const double (&t)[U][D], int tid, int g, int cnt,
                                          bool leader, double* __restrict__ tb,
                                          double (&acc)[D]) {
  if (G == 1) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < cnt)
#pragma unroll
        for (int k = 0; k < D; ++k) acc[k] = acc[k] + t[u][k];
    return;
  }
  const int base = tid - g;  // the group's first lane
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < D; ++k) tb[(base * U + g + G * u) * D + k] = t[u][k];
  wave_lds_sync();
  if (leader) {
    constexpr int B = (G * U < 8) ? G * U : 8;  // terms read ahead of the ordered adds
#pragma unroll
    for (int l0 = 0; l0 < G * U; l0 += B) {
      if (SKIP && l0 >= cnt) break;
      double v[B][D];
#pragma unroll
      for (int l = 0; l < B; ++l)
#pragma unroll
        for (int k = 0; k < D; ++k) v[l][k] = tb[(base * U + l0 + l) * D + k];
#pragma unroll
      for (int l = 0; l < B; ++l)
        if (l0 + l < cnt)
#pragma unroll
          for (int k = 0; k < D; ++k) acc[k] = acc[k] + v[l][k];
    }
  }
  wave_lds_sync();
}

}  // namespace ge

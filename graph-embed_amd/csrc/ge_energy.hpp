// ge_energy.hpp -- the pair term of the layout energy's all-pairs pass (ge_energy.hip)
// and the entry points ge_fa.hip and ge_dist.hip call (include/ge.h, "layout energy").
#pragma once

#include "ge_internal.hpp"
#include "ge_pair.hpp"

namespace ge {

// Shape of the all-pairs pass: fa_repulse_fast's (ge_fa.hip).  256 lanes x 4 row slots,
// partner tiles of 256, the j range in jb = max(1, min(16, ceil(n / 256))) chunks: a
// function of n alone, so a row's bits do not depend on the plan's row range.
constexpr int kEnergyThreads = 256;
constexpr int kEnergyRows = 4;
constexpr int kEnergyTileJ = 256;
constexpr int kEnergyJBlocks = 16;
constexpr int kEnergyWideW = kMaxDim + 1;  // doubles per LDS record of the run-time-d form
constexpr int kEnergyLaneRow = 64;         // CSR rows up to this many entries: one lane
constexpr int kEnergyBlockRows = 1024;     // rows per block of the totals' reduction

inline int energy_jblocks(int n) {
  return std::max(1, std::min(kEnergyJBlocks, (n + kEnergyTileJ - 1) / kEnergyTileJ));
}

#ifdef __HIPCC__
// Partner j's share of row i's two all-pairs sums: P += m_j / max(d, eps) and L += d,
// d = |x_i - x_j|.  s and y = 1 / sqrt(s) as fast_rep_pair forms them (fma chain,
// v_rsq_f64 and two Newton steps); d = s y before the clamp; yh = min(y, 1 / eps).
//   s == 0 (the self pair, coincident points): rsq = inf and the Newton steps give NaN;
//     d is forced to 0 and fmin takes 1 / eps, the reference's clamp.
//   the self pair: `self` (the caller compares the two indices: coincident points must
//     keep their m_j / eps, so s == 0 cannot stand for it) selects yh = +0, and with the
//     forced d = +0 both sums receive fma(m_j, +0, P) and L + 0: exactly nothing.  m_j is
//     finite there or the row's output is NaN anyway (below).
//   a vertex with a coordinate that is not finite: the caller turns all its coordinates
//     into NaN and, as a partner, its mass too.  fmin drops the NaN y, but m_j = NaN
//     carries it into P, and d = s y = NaN into L; as a row, the caller writes NaN.
// One fma and one add per pair, each written out: with -ffp-contract=off nothing else
// can fuse, so a row's chain over ascending j has the same bits in both kernels.
template <int D>
__device__ __forceinline__ void energy_pair(const double (&xi)[D], const double (&xj)[D],
                                            double mj, bool self, double& P, double& L) {
  constexpr double inv_eps = 1.0 / kFaEps;
  double e[D];
#pragma unroll
  for (int k = 0; k < D; ++k) e[k] = xi[k] - xj[k];
  double s = e[0] * e[0];
#pragma unroll
  for (int k = 1; k < D; ++k) s = fma(e[k], e[k], s);
  double y = __builtin_amdgcn_rsq(s);
  const double hs = 0.5 * s;
  y = y * fma(-hs * y, y, 1.5);
  y = y * fma(-hs * y, y, 1.5);
  const double d = s == 0.0 ? 0.0 : s * y;
  double yh = fmin(y, inv_eps);
  yh = self ? 0.0 : yh;
  P = fma(mj, yh, P);
  L = L + d;
}
#endif

// Scratch of a plan's energy calls, made by the first one (never by plan creation).
struct EnergyScratch {
  DevBuf<double> part, rows, blocks, totals;
};

// Rows [rb, re) of the five columns (GE_ENERGY_*) into d_rows (device, (re - rb) * 5;
// nullptr: the scratch's own buffer) on stream s.  Does not synchronise.
double* energy_rows(hipStream_t s, EnergyScratch& sc, int n, int dim, int rb, int re,
                    const int* ip, const int* ix, const double* dx, const double* dp1,
                    const ge_fa_params& p, const double* d_x, double* d_rows);
// The column sums of `rows` rows of d_rows into totals (host, 5) in the documented order;
// synchronises s.
void energy_totals(hipStream_t s, EnergyScratch& sc, int rows, const double* d_rows,
                   double* totals);

}  // namespace ge

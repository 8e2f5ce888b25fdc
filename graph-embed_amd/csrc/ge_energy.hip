// ge_energy.hip -- the layout energy of include/ge.h ("layout energy"): per row the
// five columns GE_ENERGY_REP, _ATT, _GRAV, _PAIRDIST, _EDGELEN, and their totals.
//
//   energy_pairs<D> / energy_pairs_wide   the two all-pairs sums P_i = sum_{j != i} m_j /
//       max(d_ij, eps) and L_i = sum_{j != i} d_ij (energy_pair, ge_energy.hpp), one
//       partial per row and j-chunk into the part buffer;
//   energy_rows_kernel   adds a row's partials in chunk order, walks the row's CSR
//       entries for the attraction energy and the edge lengths, adds gravity and writes
//       the five columns;
//   energy_block_sums / energy_sum_blocks   the totals.
//
// Every sum has one fixed order that depends on n (the chunks), on the row's length (the
// CSR sums) or on the number of rows reduced (the totals) and on nothing else, so the
// bits are the same for every mode, every row range and every rank of a sharded call.
#include <algorithm>
#include <cmath>

#include "ge_energy.hpp"

namespace ge {
namespace {

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < __builtin_inf(); }

// fa_repulse_fast's shape (ge_fa.hip): lane t, slot r holds row base + t + 256 r; the
// block walks j-chunk blockIdx.y in tiles of 256 records {x_0 .. x_{D-1}, m} and writes
// part[(chunk * rows + row) * 2 + {0, 1}] = {P, L}.
template <int D, int R>
__global__ void __launch_bounds__(kEnergyThreads)
energy_pairs(int n, int rb, int re, const double* __restrict__ X,
             const double* __restrict__ dp1, int jblocks, double* __restrict__ part) {
  constexpr int W = D + 1;
  __shared__ double tile[kEnergyTileJ * W];
  const int tid = threadIdx.x;
  const int rows_here = re - rb;
  const int base = rb + blockIdx.x * (kEnergyThreads * R);
  const int jb = blockIdx.y;
  const int jchunk = (n + jblocks - 1) / jblocks;
  const int jbeg = jb * jchunk;
  const int jend = min(n, jbeg + jchunk);

  double xi[R][D], P[R], L[R];
  int row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = base + tid + r * kEnergyThreads;
    const bool ok = i < re;
    row[r] = ok ? i : -1;  // a slot without a row has no self pair
    bool fin = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[r][k] = ok ? X[(size_t)i * D + k] : 0.0;
      fin = fin && finite_d(xi[r][k]);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) xi[r][k] = fin ? xi[r][k] : __builtin_nan("");
    P[r] = 0.0;
    L[r] = 0.0;
  }
  for (int j0 = jbeg; j0 < jend; j0 += kEnergyTileJ) {
    const int cnt = min(kEnergyTileJ, jend - j0);
    __syncthreads();
    if (tid < cnt) {
      const int j = j0 + tid;  // < jend <= n
      double xj[D];
      bool fin = true;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        xj[k] = X[(size_t)j * D + k];
        fin = fin && finite_d(xj[k]);
      }
#pragma unroll
      for (int k = 0; k < D; ++k) tile[tid * W + k] = fin ? xj[k] : __builtin_nan("");
      tile[tid * W + D] = fin ? dp1[j] : __builtin_nan("");
    }
    __syncthreads();
    // Only a tile that overlaps the block's own rows can hold a self pair; every other
    // tile (all but ~5 of a chunk's at large n) runs without the index compare.  `self`
    // only selects, so the two loops give a pair the same bits.
    if (j0 < base + kEnergyThreads * R && j0 + cnt > base) {
      for (int jj = 0; jj < cnt; ++jj) {
        double xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = tile[jj * W + k];
        const double mj = tile[jj * W + D];
        const int j = j0 + jj;
#pragma unroll
        for (int r = 0; r < R; ++r) energy_pair<D>(xi[r], xj, mj, j == row[r], P[r], L[r]);
      }
    } else {
      for (int jj = 0; jj < cnt; ++jj) {
        double xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = tile[jj * W + k];
        const double mj = tile[jj * W + D];
#pragma unroll
        for (int r = 0; r < R; ++r) energy_pair<D>(xi[r], xj, mj, false, P[r], L[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (row[r] >= 0) {
      const size_t o = ((size_t)jb * rows_here + (row[r] - rb)) * 2;
      part[o] = P[r];
      part[o + 1] = L[r];
    }
  }
}

// Dimensions 5 .. 16 at run time: one row per lane, records of 17 doubles {x_0 .. x_15, m}
// with the coordinates past d stored as +0 on both sides, so that the chain's extra
// fma(0, 0, s) return s unchanged and the bits are those of a chain of length d.
__global__ void __launch_bounds__(kEnergyThreads)
energy_pairs_wide(int n, int d, int rb, int re, const double* __restrict__ X,
                  const double* __restrict__ dp1, int jblocks, double* __restrict__ part) {
  constexpr int W = kEnergyWideW, DM = kMaxDim;
  __shared__ double tile[kEnergyTileJ * W];
  const int tid = threadIdx.x;
  const int rows_here = re - rb;
  const int i = rb + blockIdx.x * kEnergyThreads + tid;
  const int jb = blockIdx.y;
  const int jchunk = (n + jblocks - 1) / jblocks;
  const int jbeg = jb * jchunk;
  const int jend = min(n, jbeg + jchunk);
  const bool ok = i < re;
  const int row = ok ? i : -1;

  double xi[DM], P = 0.0, L = 0.0;
  {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      xi[k] = ok && k < d ? X[(size_t)i * d + k] : 0.0;
      fin = fin && finite_d(xi[k]);
    }
#pragma unroll
    for (int k = 0; k < DM; ++k) xi[k] = fin ? xi[k] : __builtin_nan("");
  }
  for (int j0 = jbeg; j0 < jend; j0 += kEnergyTileJ) {
    const int cnt = min(kEnergyTileJ, jend - j0);
    __syncthreads();
    if (tid < cnt) {
      const int j = j0 + tid;  // < jend <= n
      bool fin = true;
      for (int k = 0; k < d; ++k) fin = fin && finite_d(X[(size_t)j * d + k]);
      for (int k = 0; k < DM; ++k)
        tile[tid * W + k] = k < d ? (fin ? X[(size_t)j * d + k] : __builtin_nan("")) : 0.0;
      tile[tid * W + DM] = fin ? dp1[j] : __builtin_nan("");
    }
    __syncthreads();
    for (int jj = 0; jj < cnt; ++jj) {
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = tile[jj * W + k];
      energy_pair<DM>(xi, xj, tile[jj * W + DM], j0 + jj == row, P, L);
    }
  }
  if (ok) {
    const size_t o = ((size_t)jb * rows_here + (i - rb)) * 2;
    part[o] = P;
    part[o + 1] = L;
  }
}

struct RowConst {
  double half_repel, half_attract, gravity, delta;
  int use_weights, linlog, nohubs;
};

// One CSR entry of row i: its distance d (unclamped; NaN when the neighbour has a
// coordinate that is not finite) and its attraction term a' psi(max(d, eps)).
__device__ __forceinline__ void energy_edge(int d, const double* __restrict__ X, int i, int j,
                                            double a, const RowConst& c, double& term,
                                            double& len) {
  double s = 0.0;
  bool fin = true;
  for (int k = 0; k < d; ++k) {
    const double xj = X[(size_t)j * d + k];
    fin = fin && finite_d(xj);
    const double e = xj - X[(size_t)i * d + k];
    s = fma(e, e, s);
  }
  len = fin ? sqrt(s) : __builtin_nan("");
  const double dh = clamp_eps(len);  // NaN stays NaN
  double psi;
  if (c.linlog) {
    // log1p, not log(1 + dh): rounding 1 + dh alone is an absolute 2^-53, 2e-6 of
    // psi(eps) = 5e-11
    const double q = 1.0 + dh;
    psi = q * log1p(dh) - dh;
  } else {
    psi = (0.5 * dh) * dh;
  }
  if (!c.use_weights || c.delta == 0.0) {
    term = psi;
  } else if (c.delta == 1.0) {
    term = a * psi;
  } else {
    const double sgn = a < 0 ? -1.0 : 1.0;
    term = (sgn * pow(fabs(a), c.delta)) * psi;
  }
}

// Thread q is row rb + q.  Rows of up to 64 entries: this lane, stored order.  Longer
// rows: afterwards the wave takes its lanes' long rows one by one; lane l adds the
// entries l, l + 64, ... in order, and the 64 lane sums are added in lane order from +0.
__global__ void __launch_bounds__(256)
energy_rows_kernel(int n, int d, int rb, int re, int jblocks, const int* __restrict__ ip,
                   const int* __restrict__ ix, const double* __restrict__ dx,
                   const double* __restrict__ dp1, const double* __restrict__ X, RowConst c,
                   const double* __restrict__ part, double* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int rows_here = re - rb;
  const bool ok = q < rows_here;
  const int i = rb + q;
  const int e0 = ok ? ip[i] : 0, e1 = ok ? ip[i + 1] : 0;
  const bool lng = e1 - e0 > kEnergyLaneRow;
  double att = 0.0, len = 0.0;
  if (ok && !lng) {
    for (int e = e0; e < e1; ++e) {
      double t, l;
      energy_edge(d, X, i, ix[e], c.use_weights ? dx[e] : 1.0, c, t, l);
      att = att + t;
      len = len + l;
    }
  }
  unsigned long long todo = __ballot(lng);
  const int lane = threadIdx.x & 63;
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int wi = __shfl(i, src), w0 = __shfl(e0, src), w1 = __shfl(e1, src);
    double ta = 0.0, tl = 0.0;
    for (int e = w0 + lane; e < w1; e += 64) {
      double t, l;
      energy_edge(d, X, wi, ix[e], c.use_weights ? dx[e] : 1.0, c, t, l);
      ta = ta + t;
      tl = tl + l;
    }
    double sa = 0.0, sl = 0.0;
    for (int k = 0; k < 64; ++k) {
      sa = sa + __shfl(ta, k);
      sl = sl + __shfl(tl, k);
    }
    if (lane == src) {
      att = sa;
      len = sl;
    }
  }
  if (!ok) return;
  double P = 0.0, L = 0.0;
  for (int b = 0; b < jblocks; ++b) {
    const size_t o = ((size_t)b * rows_here + q) * 2;
    P = P + part[o];
    L = L + part[o + 1];
  }
  const double m = dp1[i];
  // |x_i|, scaled by nothing: below ~1e-154 the squares underflow and it reads as 0
  double s = 0.0;
  bool fin = true;
  for (int k = 0; k < d; ++k) {
    const double v = X[(size_t)i * d + k];
    fin = fin && finite_d(v);
    s = fma(v, v, s);
  }
  double o[GE_ENERGY_COLS];
  o[GE_ENERGY_REP] = (c.half_repel * m) * P;
  o[GE_ENERGY_ATT] = c.nohubs ? (c.half_attract * att) / m : c.half_attract * att;
  o[GE_ENERGY_GRAV] = (c.gravity * m) * sqrt(s);
  o[GE_ENERGY_PAIRDIST] = L;
  o[GE_ENERGY_EDGELEN] = len;
#pragma unroll
  for (int k = 0; k < GE_ENERGY_COLS; ++k)
    out[(size_t)q * GE_ENERGY_COLS + k] = fin ? o[k] : __builtin_nan("");
}

// Totals, per column.  Block b takes the rows [1024 b, 1024 b + 1024) (+0 past the
// last): thread t adds its four consecutive rows as (v0 + v1) + (v2 + v3), then the 256
// thread sums fold in halves, a[t] = a[t] + a[t + h] for h = 128, 64, ..., 1.
// energy_sum_blocks adds the block sums in block order from +0.
__global__ void __launch_bounds__(256)
energy_block_sums(int rows, const double* __restrict__ vals, double* __restrict__ blocks) {
  __shared__ double a[256];
  const int t = threadIdx.x;
  const long long first = (long long)blockIdx.x * kEnergyBlockRows + 4 * t;
  for (int c = 0; c < GE_ENERGY_COLS; ++c) {
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = first + k < rows ? vals[(size_t)(first + k) * GE_ENERGY_COLS + c] : 0.0;
    __syncthreads();
    a[t] = (v[0] + v[1]) + (v[2] + v[3]);
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (t < h) a[t] = a[t] + a[t + h];
      __syncthreads();
    }
    if (t == 0) blocks[(size_t)blockIdx.x * GE_ENERGY_COLS + c] = a[0];
  }
}

__global__ void energy_sum_blocks(int nblocks, const double* __restrict__ blocks,
                                  double* __restrict__ totals) {
  const int c = threadIdx.x;
  if (c >= GE_ENERGY_COLS) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s = s + blocks[(size_t)b * GE_ENERGY_COLS + c];
  totals[c] = s;
}

}  // namespace

double* energy_rows(hipStream_t s, EnergyScratch& sc, int n, int dim, int rb, int re,
                    const int* ip, const int* ix, const double* dx, const double* dp1,
                    const ge_fa_params& p, const double* d_x, double* d_rows) {
  const int rows = re - rb;
  if (rows <= 0) return d_rows;
  const int jb = energy_jblocks(n);
  if (sc.part.n < (size_t)rows * 2 * jb) sc.part.alloc((size_t)rows * 2 * jb);
  if (!d_rows) {
    if (sc.rows.n < (size_t)rows * GE_ENERGY_COLS) sc.rows.alloc((size_t)rows * GE_ENERGY_COLS);
    d_rows = sc.rows.p;
  }
  if (dim <= kNarrowMaxDim) {
    dispatch_dim_narrow(dim, [&](auto Dc) {
      constexpr int D = decltype(Dc)::value;
      const int per = kEnergyThreads * kEnergyRows;
      hipLaunchKernelGGL((energy_pairs<D, kEnergyRows>), dim3((rows + per - 1) / per, jb),
                         dim3(kEnergyThreads), 0, s, n, rb, re, d_x, dp1, jb, sc.part.p);
    });
  } else {
    hipLaunchKernelGGL(energy_pairs_wide, dim3((rows + kEnergyThreads - 1) / kEnergyThreads, jb),
                       dim3(kEnergyThreads), 0, s, n, dim, rb, re, d_x, dp1, jb, sc.part.p);
  }
  GE_HIP(hipGetLastError());
  RowConst c;
  c.half_repel = 0.5 * p.repel;
  c.half_attract = 0.5 * p.attract;
  c.gravity = p.gravity;
  c.delta = p.delta;
  c.use_weights = p.use_weights;
  c.linlog = p.linlog;
  c.nohubs = p.nohubs;
  hipLaunchKernelGGL(energy_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, n, dim, rb, re,
                     jb, ip, ix, dx, dp1, d_x, c, sc.part.p, d_rows);
  GE_HIP(hipGetLastError());
  return d_rows;
}

void energy_totals(hipStream_t s, EnergyScratch& sc, int rows, const double* d_rows,
                   double* totals) {
  for (int k = 0; k < GE_ENERGY_COLS; ++k) totals[k] = 0.0;
  if (rows <= 0) {
    GE_HIP(hipStreamSynchronize(s));
    return;
  }
  const int nblocks = (rows + kEnergyBlockRows - 1) / kEnergyBlockRows;
  if (sc.blocks.n < (size_t)nblocks * GE_ENERGY_COLS) sc.blocks.alloc((size_t)nblocks * GE_ENERGY_COLS);
  if (!sc.totals.p) sc.totals.alloc(GE_ENERGY_COLS);
  hipLaunchKernelGGL(energy_block_sums, dim3(nblocks), dim3(256), 0, s, rows, d_rows, sc.blocks.p);
  hipLaunchKernelGGL(energy_sum_blocks, dim3(1), dim3(64), 0, s, nblocks, sc.blocks.p, sc.totals.p);
  GE_HIP(hipGetLastError());
  sc.totals.download(totals, GE_ENERGY_COLS, s);
  GE_HIP(hipStreamSynchronize(s));
}

}  // namespace ge

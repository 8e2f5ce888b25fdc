// ge_faml.hip -- multilevel ForceAtlas (one level) on gfx950.
//
// Reference: partition::forceAtlasMultilevel, include/forceatlas.hpp:314-574,
// called once per level with iterations = 100 (src/embed.cpp:793).
//
// Aggregates never exchange data during the iterations (the external pull reads
// only the frozen coarse coordinates coords_A, :454, :462), so each aggregate is
// an independent N-body problem.  Layout: a member's state is indexed by its
// P_T storage position c (aggregate a owns positions pt_ip[a]..pt_ip[a+1]);
// pos_of[fine id] = c.
//
// Aggregates are bucketed by size s:
//   s <= 64          packs of aggregates with <= 64 members total, 64-thread block
//   64 < s <= 256    packs with <= 256 members, 256-thread block
//   256 < s <= cap   one aggregate per 256-thread block; cap = large_cap(dim): 4096
//                    members at dim <= 3, 2048 at dim 4..7, ..., 874 at dim 16
//   (all three: coordinates resident in LDS, all iterations in ONE launch)
//   s > cap          "streamed": per iteration a force kernel (j tiles through
//                    LDS) and an update kernel, coordinates in HBM.
// Dimensions 5..16 run the wide schedule (ge_pair.hpp): the same resident kernels,
// and the streamed aggregates on faml_big_repulse<D, 1, 1> (no symmetric sweeps).
//
// STRICT op order, as ge_fa.hip: per member the j loop runs over the aggregate's
// members in P_T order (:394-410), then the CSR row in stored order with the
// reference's internal/external test `v_A[j] == a && j != i` (i the LOCAL index,
// :417), gravity with mag clamped to eps (:411-414), swing clamped (:484-486).
// The centring mean (:540-553) is a serial sum in member order (one thread per
// aggregate); the max norm (:555-561) is order-free.
// Random init replays the reference's single-thread mt19937 draw order: the
// host generates draw c*dim+k for position c (include/forceatlas.hpp:356-360).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <numeric>
#include <queue>
#include <string>
#include <vector>

#include "ge_faml_sched.hpp"
#include "ge_far.hpp"
#include "ge_internal.hpp"
#include "ge_pair.hpp"
#include "ge_rows.hpp"
#include "ge_sym.hpp"

namespace ge {
namespace {

constexpr double kEps = kFaEps;
using MlConst = FaConst;

template <int D>
struct W {
  static constexpr int v = rec_width(D);
};

// Largest aggregate kept resident in LDS: 128 KiB of member records (rec_width(D)
// doubles each), or what the block's LDS leaves after faml_resident's other arrays
// (the 257 + 256 pack offsets and the 256 x (D + 1) doubles of centres) where that
// is less: 4096 members at D <= 3, 2048 at D = 4..7, 1638 at D = 8, 874 at D = 16.
constexpr size_t resident_fixed_bytes(int dim) {
  return sizeof(int) * (2 * 256 + 1) + sizeof(double) * 256 * (dim + 1) + 16;
}
constexpr int large_cap(int dim) {
  const size_t left = kLdsBlock - resident_fixed_bytes(dim);
  return (int)((left < 128 * 1024 ? left : 128 * 1024) / (sizeof(double) * rec_width(dim)));
}
static_assert(large_cap(3) == 4096 && large_cap(4) == 2048, "the D <= 4 caps are unchanged");

// Internal degree + 1 of member at position c in aggregate a (:362-383).
__device__ __forceinline__ double internal_dp1(int v, int a, const int* __restrict__ ip,
                                               const int* __restrict__ ix,
                                               const double* __restrict__ dx,
                                               const int* __restrict__ vA, int use_weights) {
  double s = 0.0;
  for (int e = ip[v]; e < ip[v + 1]; ++e)
    if (vA[ix[e]] == a) s += use_weights ? dx[e] : 1.0;
  return s + 1;
}

// ((t / dis) * 100.0) / mag for the external pull of one CSR entry (:452-465).
template <int D, bool SHARED>
__device__ __forceinline__ void pull_edge(const double* __restrict__ ca,
                                          const double* __restrict__ cb, double mag,
                                          const Recip& rmag, double (&acc)[D]) {
  double t[D];
#pragma unroll
  for (int k = 0; k < D; ++k) t[k] = cb[k] - ca[k];
  double q = t[0] * t[0];
#pragma unroll
  for (int k = 1; k < D; ++k) q = q + t[k] * t[k];
  const double dis = clamp_eps(sqrt(q));
  if (SHARED) {
    const Recip rc = recip_of(dis);
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = acc[k] + div_by(div_by(t[k], dis, rc) * 100.0, mag, rmag);
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = acc[k] + (t[k] / dis) * 100.0 / mag;
  }
}

// Force on one member (:391-474).  xs(l) returns the coordinates of local member
// l of the same aggregate; xi/dip1 the member's own.
template <int D, class XS, class DS>
__device__ __forceinline__ void member_force(int li, int s, int a, int v, const double (&xi)[D],
                                             double dip1, XS xs, DS ds, int pt_base,
                                             const int* __restrict__ ip, const int* __restrict__ ix,
                                             const double* __restrict__ dx,
                                             const int* __restrict__ vA,
                                             const int* __restrict__ pos_of,
                                             const double* __restrict__ cA, const MlConst& c,
                                             double (&F)[D]) {
  double acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = 0.0;
  const bool row_ok = all_coord_ok<D>(xi);
  const bool rep_ok = row_ok && weight_ok(dip1) && weight_ok(c.repel);
  for (int j = 0; j < s; ++j) {  // :394-410
    const double* xj = xs(j);
    if (rep_ok && vertex_ok<D>(xj, ds(j)))
      rep_pair<D, true, false>(xi, xj, dip1, ds(j), c.repel, acc);
    else
      rep_pair_fb<D, false>(xi, xj, dip1, ds(j), c.repel, j == li, acc);
  }
  double m2 = xi[0] * xi[0];
#pragma unroll
  for (int k = 1; k < D; ++k) m2 = m2 + xi[k] * xi[k];
  double mag = sqrt(m2);
  if (mag < kEps) mag = kEps;
  const Recip rmag = recip_of(mag);
  const double* ca = cA + (size_t)a * D;
  const bool ca_ok = all_coord_ok<D>(ca);
  for (int e = ip[v]; e < ip[v + 1]; ++e) {  // :415-467
    const int j = ix[e];
    const int b = vA[j];
    if (b == a && j != li) {  // sic: global j against local i (:417)
      const double* xj = xs(pos_of[j] - pt_base);
      const double w = c.use_weights ? dx[e] : 1.0;
      if (row_ok && all_coord_ok<D>(xj))
        attr_edge<D, true>(xi, xj, w, dip1, c, acc);
      else
        attr_edge<D, false>(xi, xj, w, dip1, c, acc);
    } else {
      const double* cb = cA + (size_t)b * D;
      if (row_ok && ca_ok && all_coord_ok<D>(cb))
        pull_edge<D, true>(ca, cb, mag, rmag, acc);
      else
        pull_edge<D, false>(ca, cb, mag, rmag, acc);
    }
  }
  double unit[D];
  neg_over<D>(xi, mag, unit);
#pragma unroll
  for (int k = 0; k < D; ++k) F[k] = acc[k] + unit[k] * c.gravity * dip1;  // :469-474
}

// Swing (clamped) + speed + update of one member (:477-530).
template <int D>
__device__ __forceinline__ void member_update(double (&x)[D], const double (&F)[D],
                                              const double (&Fp)[D], const MlConst& c) {
  double s = 0.0, f2 = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double t = F[k] - Fp[k];
    s = (k == 0) ? t * t : s + t * t;
    f2 = (k == 0) ? F[k] * F[k] : f2 + F[k] * F[k];
  }
  double swing = sqrt(s);
  if (swing < kEps) swing = kEps;
  const double totalF = sqrt(f2);
  double speed = c.ks_gS / (1 + c.gS * sqrt(swing));
  const double cap = c.ksmax / totalF;
  if (speed > cap) speed = cap;
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = F[k] * speed + x[k];
}

// ---------------------------------------------------------------------------
// Resident kernel: one block = one pack of aggregates (order[pack_beg[p]..
// pack_beg[p+1])), members in LDS, all iterations in-kernel.

template <int D, int T, int CAP>
__global__ void __launch_bounds__(T)
faml_resident(const int* __restrict__ order, const int* __restrict__ pack_beg,
              const int* __restrict__ pt_ip, const int* __restrict__ pt_ix,
              const int* __restrict__ pos_of, const int* __restrict__ vA,
              const int* __restrict__ ip, const int* __restrict__ ix,
              const double* __restrict__ dx, const double* __restrict__ cA,
              const double* __restrict__ rA, const double* __restrict__ init,
              double* __restrict__ Fscr, double* __restrict__ Fprev,
              double* __restrict__ Xout, int iterations, MlConst c) {
  constexpr int WV = W<D>::v;
  constexpr int MAXAGG = (CAP < T) ? CAP : T;  // aggregates per pack <= T
  __shared__ __attribute__((aligned(16))) double rec[CAP * WV];
  __shared__ int seg[MAXAGG + 1];
  __shared__ int agg_of_seg[MAXAGG];
  __shared__ double ball[MAXAGG * (D + 1)];

  const int tid = threadIdx.x;
  const int p0 = pack_beg[blockIdx.x], p1 = pack_beg[blockIdx.x + 1];
  const int naggs = p1 - p0;
  if (tid == 0) {
    int off = 0;
    for (int q = 0; q < naggs; ++q) {
      const int a = order[p0 + q];
      seg[q] = off;
      agg_of_seg[q] = a;
      off += pt_ip[a + 1] - pt_ip[a];
    }
    seg[naggs] = off;
  }
  __syncthreads();
  const int S = seg[naggs];

  // member q -> (segment, aggregate, local index, position)
  auto locate = [&](int q, int& g, int& a, int& li, int& pc) {
    int lo = 0, hi = naggs - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (seg[mid] <= q) lo = mid; else hi = mid - 1;
    }
    g = lo;
    a = agg_of_seg[lo];
    li = q - seg[lo];
    pc = pt_ip[a] + li;
  };

  for (int q = tid; q < S; q += T) {
    int g, a, li, pc;
    locate(q, g, a, li, pc);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      rec[q * WV + k] = init[(size_t)pc * D + k];
      Fprev[(size_t)pc * D + k] = 0.0;
    }
    rec[q * WV + D] = internal_dp1(pt_ix[pc], a, ip, ix, dx, vA, c.use_weights);
  }

  for (int it = 0; it < iterations; ++it) {
    __syncthreads();
    for (int q = tid; q < S; q += T) {
      int g, a, li, pc;
      locate(q, g, a, li, pc);
      const int s0 = seg[g];
      const int s = seg[g + 1] - s0;
      double xi[D], F[D];
#pragma unroll
      for (int k = 0; k < D; ++k) xi[k] = rec[q * WV + k];
      const double dip1 = rec[q * WV + D];
      member_force<D>(li, s, a, pt_ix[pc], xi, dip1,
                      [&](int l) { return &rec[(s0 + l) * WV]; },
                      [&](int l) { return rec[(s0 + l) * WV + D]; }, pt_ip[a], ip, ix, dx, vA,
                      pos_of, cA, c, F);
#pragma unroll
      for (int k = 0; k < D; ++k) Fscr[(size_t)pc * D + k] = F[k];
    }
    __syncthreads();
    for (int q = tid; q < S; q += T) {
      int g, a, li, pc;
      locate(q, g, a, li, pc);
      double x[D], F[D], Fp[D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        x[k] = rec[q * WV + k];
        F[k] = Fscr[(size_t)pc * D + k];
        Fp[k] = Fprev[(size_t)pc * D + k];
      }
      member_update<D>(x, F, Fp, c);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        rec[q * WV + k] = x[k];
        Fprev[(size_t)pc * D + k] = F[k];
      }
    }
  }
  __syncthreads();
  // centre + max norm per aggregate (:539-564): serial mean in member order
  for (int g = tid; g < naggs; g += T) {
    const int s0 = seg[g], s = seg[g + 1] - seg[g];
    double avg[D];
#pragma unroll
    for (int k = 0; k < D; ++k) avg[k] = 0.0;
    for (int l = 0; l < s; ++l)
#pragma unroll
      for (int k = 0; k < D; ++k) avg[k] = avg[k] + rec[(s0 + l) * WV + k];
#pragma unroll
    for (int k = 0; k < D; ++k) avg[k] = avg[k] / s;
    double big = 0.0;
    for (int l = 0; l < s; ++l) {
      double m2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double t = rec[(s0 + l) * WV + k] - avg[k];
        m2 = (k == 0) ? t * t : m2 + t * t;
      }
      const double len = sqrt(m2);
      if (len > big) big = len;
    }
    if (big < kEps) big = kEps;
#pragma unroll
    for (int k = 0; k < D; ++k) ball[g * (D + 1) + k] = avg[k];
    ball[g * (D + 1) + D] = big;
  }
  __syncthreads();
  for (int q = tid; q < S; q += T) {
    int g, a, li, pc;
    locate(q, g, a, li, pc);
    const double big = ball[g * (D + 1) + D];
    const int v = pt_ix[pc];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double x = rec[q * WV + k] - ball[g * (D + 1) + k];
      Xout[(size_t)v * D + k] = cA[(size_t)a * D + k] + rA[a] * (x / big);
    }
  }
}

// ---------------------------------------------------------------------------
// Streamed path for aggregates too large to stay resident.  Per iteration:
//   faml_big_repulse  the in-aggregate all-pairs sum, one WAVE per work item
//                     (aggregate a, rows r0 .. r0 + 64R); items are taken from
//                     an atomic queue in descending-work order (list scheduling
//                     over aggregates of very different sizes);
//   FamlRows          (classed_rows_kernel, ge_rows.hpp) the CSR row's terms
//                     added to the repulsion sum in stored order, then gravity
//                     and the swing/speed update.
// `rows` lists the P_T positions of all streamed members.

constexpr int kHT = 256;   // threads per block of the streamed kernels
constexpr int kBigW = 64;  // records per wave tile

template <int D>
__global__ void __launch_bounds__(kHT)
faml_huge_init(int nrows, const int* __restrict__ rows, const double* __restrict__ init,
               double* __restrict__ Xp, double* __restrict__ Fprev) {
  const int q = blockIdx.x * kHT + threadIdx.x;
  if (q >= nrows) return;
  const int c = rows[q];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    Xp[(size_t)c * D + k] = init[(size_t)c * D + k];
    Fprev[(size_t)c * D + k] = 0.0;
  }
}

// internal deg + 1 of the streamed members (:362-383): a property of the graph
// and P_T, computed once per plan (a hub row's serial sum takes tens of ms).
__global__ void __launch_bounds__(kHT)
faml_huge_dp(int nrows, const int* __restrict__ rows, const int* __restrict__ pt_ix,
             const int* __restrict__ vA, const int* __restrict__ ip, const int* __restrict__ ix,
             const double* __restrict__ dx, double* __restrict__ DP, int use_weights) {
  const int q = blockIdx.x * kHT + threadIdx.x;
  if (q >= nrows) return;
  const int c = rows[q];
  const int v = pt_ix[c];
  DP[c] = internal_dp1(v, vA[v], ip, ix, dx, vA, use_weights);
}

// R row slots per lane, U consecutive partners evaluated together (their terms
// are then added in j order).
template <int D, int R, int U, bool REPEL_ONE>
__global__ void __launch_bounds__(kHT)
faml_big_repulse(int nitems, const int2* __restrict__ items, int* __restrict__ queue,
                 const int* __restrict__ pt_ip, const double* __restrict__ Xp,
                 const double* __restrict__ DP, double repel, double* __restrict__ Fscr) {
  constexpr int WV = W<D>::v;
  __shared__ __attribute__((aligned(16))) double tiles[kHT / 64][kBigW * WV];
  const int lane = threadIdx.x & 63;
  double* tile = tiles[threadIdx.x >> 6];
  const bool repel_ok = REPEL_ONE || weight_ok(repel);
  for (;;) {
    int q = 0;
    if (lane == 0) q = atomicAdd(queue, 1);
    q = __builtin_amdgcn_readfirstlane(q);
    if (q >= nitems) break;  // every wave leaves once the queue is drained
    const int2 item = items[q];
    const int base = pt_ip[item.x];
    const int s = pt_ip[item.x + 1] - base;
    const int r0 = item.y;
    const int nr = min(R, (s - r0 + 63) >> 6);  // wave-uniform
    double xi[R][D], di[R], acc[R][D];
    bool rows_ok = repel_ok;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int li = r0 + lane + 64 * r;
      const bool ok = r < nr && li < s;
      const size_t c = (size_t)base + (ok ? li : 0);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        xi[r][k] = ok ? Xp[c * D + k] : 0.0;
        acc[r][k] = 0.0;
      }
      di[r] = ok ? DP[c] : 1.0;
      rows_ok = rows_ok && vertex_ok<D>(xi[r], di[r]);
    }
    for (int j0 = 0; j0 < s; j0 += kBigW) {
      const int cnt = min(kBigW, s - j0);
      bool ok = rows_ok;
      wave_lds_sync();  // the previous tile has been read by every lane
      if (lane < cnt) {
        const size_t c = (size_t)base + j0 + lane;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double v = Xp[c * D + k];
          tile[lane * WV + k] = v;
          ok = ok && coord_ok(v);
        }
        const double w = DP[c];
        tile[lane * WV + D] = w;
        ok = ok && weight_ok(w);
      }
      wave_lds_sync();
      if (__all(ok)) {
        int jj = 0;
        if (nr == R) {
          // every row slot of the wave is used: no per-slot branches, so the
          // partner record is read once for all R rows and the independent
          // chains (R rows x U partners) interleave
          if constexpr (U == 1) {
            for (; jj < cnt; ++jj) {
              const double* xj = &tile[jj * WV];
              const double dj = tile[jj * WV + D];
#pragma unroll
              for (int r = 0; r < R; ++r) rep_pair<D, true, REPEL_ONE>(xi[r], xj, di[r], dj, repel, acc[r]);
            }
          } else {
            for (; jj + U <= cnt; jj += U) {
              double t[U][R][D];
#pragma unroll
              for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r)
                  rep_term<D, true, REPEL_ONE>(xi[r], &tile[(jj + u) * WV], di[r],
                                               tile[(jj + u) * WV + D], repel, t[u][r]);
#pragma unroll
              for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                  for (int k = 0; k < D; ++k) acc[r][k] = acc[r][k] + t[u][r][k];
            }
          }
        } else if (U > 1) {
          for (; jj + U <= cnt; jj += U) {
            double t[U][R][D];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
              for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int k = 0; k < D; ++k) t[u][r][k] = 0.0;
                if (r < nr)
                  rep_pair<D, true, REPEL_ONE>(xi[r], &tile[(jj + u) * WV], di[r],
                                               tile[(jj + u) * WV + D], repel, t[u][r]);
              }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
              for (int r = 0; r < R; ++r)
#pragma unroll
                for (int k = 0; k < D; ++k) acc[r][k] = acc[r][k] + t[u][r][k];
          }
        }
        for (; jj < cnt; ++jj) {
          const double* xj = &tile[jj * WV];
          const double dj = tile[jj * WV + D];
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (r < nr) rep_pair<D, true, REPEL_ONE>(xi[r], xj, di[r], dj, repel, acc[r]);
        }
      } else {
        for (int jj = 0; jj < cnt; ++jj) {
          const double* xj = &tile[jj * WV];
          const double dj = tile[jj * WV + D];
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (r < nr)
              rep_pair_fb<D, REPEL_ONE>(xi[r], xj, di[r], dj, repel,
                                        j0 + jj == r0 + lane + 64 * r, acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int li = r0 + lane + 64 * r;
      if (r < nr && li < s) {
#pragma unroll
        for (int k = 0; k < D; ++k) Fscr[((size_t)base + li) * D + k] = acc[r][k];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// FAST mode (GE_MODE_FAST, D <= 4): the streamed aggregates' repulsion in closed
// form (fast_rep_pair, ge_pair.hpp), every ordered pair, no ordering between waves.
// Work items are (aggregate, rows [r0, r1)) with r1 - r0 <= 64 R, taken from the
// queue by wave; a lane owns up to R rows (r0 + lane + 64 r) in registers and runs
// over ALL members of the aggregate in P_T order, 64-record tiles through the
// wave's LDS slice (the next tile's record is loaded into registers while the
// current one is evaluated).  A row's sum is one lane's fma chain over j = 0 .. s - 1,
// so its bits do not depend on the item list: a whole plan, a subset plan and a shard
// plan's local tiles of a split aggregate give the same sums.
//
// R = 4 (kFastR): the partner record (D + 1 doubles, one broadcast ds_read per two)
// is read once for four rows, and four independent chains per lane cover the
// quarter-rate v_rsq_f64 and the Newton steps' dependent FMAs without a second wave.
// Per lane 4 x (xi[D] + acc[D] + dir), the record and its prefetched successor, and
// e / s / y / w of the pairs in flight: 86 / 124 / 122 VGPRs at D = 1 / 2 / 3, inside
// the 128 of four waves per SIMD, and 168 at D = 4 (three waves; held to 128 it spills
// 34 registers), no scratch anywhere.  The plan launches as many blocks per CU as
// fit, at most four.  Inner loop at D = 3: 21 VALU + one v_rsq_f64 per ordered pair,
// two ds_read_b128 per partner for its four rows (FAST mode).
// The last item of a row range may use fewer than R row slots (nr, wave-uniform): its
// partner loop is instantiated per nr, so no slot past r1 is evaluated.

constexpr int kFastR = 4;

template <int D, int R, int NR>
__device__ __forceinline__ void fast_rows(const double* __restrict__ tile, int cnt,
                                          const double (&xi)[R][D], const double (&di)[R],
                                          double (&acc)[R][D]) {
  constexpr int WV = W<D>::v;
  for (int jj = 0; jj < cnt; ++jj) {
    double xj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xj[k] = tile[jj * WV + k];
    const double dj = tile[jj * WV + D];
#pragma unroll
    for (int r = 0; r < NR; ++r) fast_rep_pair<D>(xi[r], xj, di[r], dj, acc[r]);
  }
}

template <int D, int R>
__global__ void __launch_bounds__(kHT, D <= 3 ? 4 : 3)
faml_fast_repulse(int nitems, const int4* __restrict__ items, int* __restrict__ queue,
                  const int* __restrict__ pt_ip, const double* __restrict__ Xp,
                  const double* __restrict__ DP, double repel, double* __restrict__ Fscr) {
  static_assert(R >= 1 && R <= 4, "the partner loop is instantiated for 1..4 row slots");
  constexpr int WV = W<D>::v;
  __shared__ __attribute__((aligned(16))) double tiles[kHT / 64][kBigW * WV];
  const int lane = threadIdx.x & 63;
  double* tile = tiles[threadIdx.x >> 6];
  for (;;) {
    int q = 0;
    if (lane == 0) q = atomicAdd(queue, 1);
    q = __builtin_amdgcn_readfirstlane(q);
    if (q >= nitems) break;  // the queue drain is the kernel's only loop over items
    const int4 item = items[q];
    const int base = pt_ip[item.x];
    const int s = pt_ip[item.x + 1] - base;
    const int r0 = item.y;
    const int r1 = min(item.z, s);
    const int nr = min(R, (r1 - r0 + 63) >> 6);  // wave-uniform
    double xi[R][D], di[R], acc[R][D];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int li = r0 + lane + 64 * r;
      const bool ok = li < r1;
      const size_t c = (size_t)base + (ok ? li : r0);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        xi[r][k] = ok ? Xp[c * D + k] : 0.0;
        acc[r][k] = 0.0;
      }
      di[r] = ok ? DP[c] * repel : 0.0;
    }
    double nx[D + 1];  // this lane's record of the next tile
    {
      const size_t c = (size_t)base + min(lane, s - 1);
#pragma unroll
      for (int k = 0; k < D; ++k) nx[k] = Xp[c * D + k];
      nx[D] = DP[c];
    }
    for (int j0 = 0; j0 < s; j0 += kBigW) {
      const int cnt = min(kBigW, s - j0);
      wave_lds_sync();  // the previous tile has been read by every lane
#pragma unroll
      for (int k = 0; k <= D; ++k) tile[lane * WV + k] = nx[k];
      wave_lds_sync();
      if (j0 + kBigW < s) {  // lanes past the end re-read the last member (in bounds, unused)
        const size_t c = (size_t)base + min(j0 + kBigW + lane, s - 1);
#pragma unroll
        for (int k = 0; k < D; ++k) nx[k] = Xp[c * D + k];
        nx[D] = DP[c];
      }
      switch (nr) {
        case 1: fast_rows<D, R, 1>(tile, cnt, xi, di, acc); break;
        case 2: fast_rows<D, R, (R >= 2 ? 2 : R)>(tile, cnt, xi, di, acc); break;
        case 3: fast_rows<D, R, (R >= 3 ? 3 : R)>(tile, cnt, xi, di, acc); break;
        default: fast_rows<D, R, R>(tile, cnt, xi, di, acc); break;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int li = r0 + lane + 64 * r;
      if (li < r1) {
#pragma unroll
        for (int k = 0; k < D; ++k) Fscr[((size_t)base + li) * D + k] = acc[r][k];
      }
    }
  }
}

// Per streamed member, after faml_big_repulse: the CSR row (:415-467) added to
// the repulsion sum in stored order (degree-classed, ge_rows.hpp), gravity
// (:469-474) and the swing/speed update (:477-530).
// ecode[e] for a streamed member's CSR entry e: the neighbour's P_T position
// when the entry is internal (v_A[j] == a && j != local i, :417), else
// -(v_A[j] + 1).  Static per level, so the per-iteration edge pass does one
// gather per entry instead of three dependent ones.
__global__ void edge_code_kernel(int nrows, const int* __restrict__ rows,
                                 const int* __restrict__ pt_ip, const int* __restrict__ pt_ix,
                                 const int* __restrict__ pos_of, const int* __restrict__ vA,
                                 const int* __restrict__ ip, const int* __restrict__ ix,
                                 int* __restrict__ ecode) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nrows) return;
  const int c = rows[q];
  const int v = pt_ix[c];
  const int a = vA[v];
  const int li = c - pt_ip[a];
  for (int e = ip[v]; e < ip[v + 1]; ++e) {
    const int j = ix[e];
    const int b = vA[j];
    ecode[e] = (b == a && j != li) ? pos_of[j] : -(b + 1);
  }
}

template <int D>
struct FamlRows {
  const int *pt_ip, *pt_ix, *ecode, *ip, *vA;
  const double *dx, *cA, *Xc, *DP, *Fscr;
  double *Xn, *Fprev;
  MlConst c;
  struct State {
    int cpos, a, li, e0, e1;
    double xi[D], acc[D], fprev[D], dip1, mag;
    Recip rmag;
    bool row_ok, ca_ok;
  };
  __device__ __forceinline__ void load(int cpos, State& s) const {
    const int v = pt_ix[cpos];
    s.cpos = cpos;
    s.a = vA[v];
    s.li = cpos - pt_ip[s.a];
    s.e0 = ip[v];
    s.e1 = ip[v + 1];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      s.xi[k] = Xc[(size_t)cpos * D + k];
      s.acc[k] = Fscr[(size_t)cpos * D + k];
      s.fprev[k] = Fprev[(size_t)cpos * D + k];  // loaded early: off the row's critical path
    }
    s.dip1 = DP[cpos];
    s.row_ok = all_coord_ok<D>(s.xi);
    double m2 = s.xi[0] * s.xi[0];
#pragma unroll
    for (int k = 1; k < D; ++k) m2 = m2 + s.xi[k] * s.xi[k];
    s.mag = sqrt(m2);
    if (s.mag < kEps) s.mag = kEps;
    s.rmag = recip_of(s.mag);
    s.ca_ok = all_coord_ok<D>(cA + (size_t)s.a * D);
  }
  __device__ __forceinline__ void term(const State& s, int e, double (&t)[D]) const {
    const int code = ecode[e];
    // the neighbour's (or its aggregate's) coordinates into registers before
    // the branch, so a thread's gathers issue together
    const double* src = code >= 0 ? Xc + (size_t)code * D : cA + (size_t)(-code - 1) * D;
    double xv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xv[k] = src[k];
    if (code >= 0) {  // internal entry (edge_code_kernel)
      const double* xj = xv;
      const double wt = c.use_weights ? dx[e] : 1.0;
      if (s.row_ok && all_coord_ok<D>(xj))
        attr_edge<D, true>(s.xi, xj, wt, s.dip1, c, t);
      else
        attr_edge<D, false>(s.xi, xj, wt, s.dip1, c, t);
    } else {
      const double* ca = cA + (size_t)s.a * D;
      const double* cb = xv;
      if (s.row_ok && s.ca_ok && all_coord_ok<D>(cb))
        pull_edge<D, true>(ca, cb, s.mag, s.rmag, t);
      else
        pull_edge<D, false>(ca, cb, s.mag, s.rmag, t);
    }
  }
  __device__ __forceinline__ void finish(State& s, bool writer) const {
    double unit[D], F[D], Fp[D], x[D];
    neg_over<D>(s.xi, s.mag, unit);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      F[k] = s.acc[k] + unit[k] * c.gravity * s.dip1;
      Fp[k] = s.fprev[k];
      x[k] = s.xi[k];
    }
    member_update<D>(x, F, Fp, c);
    if (writer) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        Xn[(size_t)s.cpos * D + k] = x[k];
        Fprev[(size_t)s.cpos * D + k] = F[k];
      }
    }
  }
};

// One block per huge aggregate: serial mean by lane 0, max by reduction.
template <int D>
__global__ void __launch_bounds__(kHT)
faml_huge_finish(const int* __restrict__ huge, const int* __restrict__ pt_ip,
                 const int* __restrict__ pt_ix, const double* __restrict__ Xp,
                 const double* __restrict__ cA, const double* __restrict__ rA,
                 double* __restrict__ Xout) {
  __shared__ double avg[D];
  __shared__ double red[kHT];
  const int a = huge[blockIdx.x];
  const int base = pt_ip[a], s = pt_ip[a + 1] - base;
  if (threadIdx.x == 0) {
    double t[D];
#pragma unroll
    for (int k = 0; k < D; ++k) t[k] = 0.0;
    for (int l = 0; l < s; ++l)
#pragma unroll
      for (int k = 0; k < D; ++k) t[k] = t[k] + Xp[(size_t)(base + l) * D + k];
#pragma unroll
    for (int k = 0; k < D; ++k) avg[k] = t[k] / s;
  }
  __syncthreads();
  double big = 0.0;
  for (int l = threadIdx.x; l < s; l += kHT) {
    double m2 = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double t = Xp[(size_t)(base + l) * D + k] - avg[k];
      m2 = (k == 0) ? t * t : m2 + t * t;
    }
    const double len = sqrt(m2);
    if (len > big) big = len;
  }
  red[threadIdx.x] = big;
  __syncthreads();
  for (int w = kHT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w && red[threadIdx.x + w] > red[threadIdx.x])
      red[threadIdx.x] = red[threadIdx.x + w];
    __syncthreads();
  }
  double mx = red[0];
  if (mx < kEps) mx = kEps;
  for (int l = threadIdx.x; l < s; l += kHT) {
    const int v = pt_ix[base + l];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double x = Xp[(size_t)(base + l) * D + k] - avg[k];
      Xout[(size_t)v * D + k] = cA[(size_t)a * D + k] + rA[a] * (x / mx);
    }
  }
}

__global__ void pos_of_kernel(int N, const int* __restrict__ pt_ix, int* __restrict__ pos_of) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < N) pos_of[pt_ix[c]] = c;
}

// The schedule (ge_faml_sched.hpp) restates what the kernels fix and lays its tables
// out as the kernels read them.
static_assert(kSchedFastR == kFastR && kSchedSymWaves == kSymT / 64 &&
                  kSchedSweep == kUnitSweep && kSchedRows == kUnitRows,
              "the schedule's constants are the kernels'");
static_assert(sizeof(SchedInt2) == sizeof(int2) && alignof(SchedInt2) <= alignof(int2) &&
                  sizeof(SchedInt4) == sizeof(int4) && alignof(SchedInt4) <= alignof(int4) &&
                  offsetof(SchedInt4, w) == offsetof(int4, w),
              "schedule items and units are uploaded as int2 / int4");

template <int D>  // the variants of D <= kNarrowMaxDim (below)
void launch_big_repulse_narrow(int code, int blocks, hipStream_t st, int nitems,
                               const int2* items, int* queue, const int* pt_ip, const double* X,
                               const double* DP, double repel, double* F);

template <int D>
void launch_big_repulse(int code, int blocks, hipStream_t st, int nitems, const int2* items,
                        int* queue, const int* pt_ip, const double* X, const double* DP,
                        double repel, double* F, bool wide) {
  if (wide || D > kNarrowMaxDim) {  // the wide schedule's one variant (faml_plan_build)
    if (code != big_code(1, 1)) throw Error(GE_ERR_STATE, "unknown streamed repulsion variant");
    hipLaunchKernelGGL((faml_big_repulse<D, 1, 1, false>), dim3(blocks), dim3(kHT), 0, st, nitems,
                       items, queue, pt_ip, X, DP, repel, F);
    return;
  }
  if constexpr (D <= kNarrowMaxDim) launch_big_repulse_narrow<D>(code, blocks, st, nitems, items,
                                                                 queue, pt_ip, X, DP, repel, F);
}

template <int D>
void launch_big_repulse_narrow(int code, int blocks, hipStream_t st, int nitems,
                               const int2* items, int* queue, const int* pt_ip, const double* X,
                               const double* DP, double repel, double* F) {
  switch (code) {
#define GE_BIG_LAUNCH(RR, UU)                                                                 \
  case big_code(RR, UU):                                                                      \
    if (repel == 1.0)                                                                         \
      hipLaunchKernelGGL((faml_big_repulse<D, RR, UU, true>), dim3(blocks), dim3(kHT), 0, st, \
                         nitems, items, queue, pt_ip, X, DP, repel, F);                       \
    else                                                                                      \
      hipLaunchKernelGGL((faml_big_repulse<D, RR, UU, false>), dim3(blocks), dim3(kHT), 0,    \
                         st, nitems, items, queue, pt_ip, X, DP, repel, F);                   \
    break;
    GE_BIG_VARIANTS(GE_BIG_LAUNCH)
#undef GE_BIG_LAUNCH
    default:
      throw Error(GE_ERR_STATE, "unknown streamed repulsion variant");
  }
}

// resident blocks per CU of faml_big_repulse<dim, R, U>
int rep_occupancy(int dim, int code) {
  int nb = 1;
  dispatch_dim(dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    const void* k = (const void*)faml_big_repulse<D, 1, 1, false>;
    if constexpr (D <= kNarrowMaxDim) {
      switch (code) {
#define GE_BIG_KERNEL(RR, UU) \
  case big_code(RR, UU): k = (const void*)faml_big_repulse<D, RR, UU, false>; break;
        GE_BIG_VARIANTS(GE_BIG_KERNEL)
#undef GE_BIG_KERNEL
        default: break;
      }
    }
    GE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, kHT, 0));
  });
  return std::max(nb, 1);
}

}  // namespace

}  // namespace ge

// ---------------------------------------------------------------------------
// plan: bucketing, pack tables and scratch built once per (graph, P_T) level

struct ge_faml_plan {
  ge_ctx* ctx = nullptr;
  int n = 0, m = 0, dim = 0, iterations = 0;
  const int *ip = nullptr, *ix = nullptr, *pt_ip = nullptr, *pt_ix = nullptr, *vA = nullptr;
  const double* dx = nullptr;
  ge::FaConst c{};
  int ns = 0, nm = 0, nl = 0, nhuge = 0;
  int res_cap = 0, census[4] = {0, 0, 0, 0};  // aggregates: small, mid, large-resident, streamed
  size_t off_m = 0, off_l = 0;
  ge::DevBuf<int> pos, order, beg, rows, erows, queue, huge, ecode;
  ge::RowClasses ecls;
  ge::RowStreams rstreams;
  ge::DevBuf<int2> items;
  int nrows = 0, nitems = 0, R = 1, code = 0, rep_blocks = 0;
  // FAST mode (faml_fast_repulse): set when the caller asked for GE_MODE_FAST, the plan
  // has streamed rows and the dimension is not on the wide schedule; then no sweep
  // units, hand-over buffers or progress counters exist
  int mode = GE_MODE_STRICT;  // as requested (ge_fa_params.mode)
  bool fast = false;
  ge::DevBuf<int4> fitems;  // (aggregate, first row, end row, 0), descending work
  int nfitems = 0, fast_blocks = 0;
  // FARFIELD mode (ge_far.hip, the segmented engine): the streamed whole aggregates of
  // at least far_min_ml members, larger first; the other streamed rows are FAST items
  ge::FarSegEngine* far = nullptr;
  int far_reason = GE_FAR_NOT_REQUESTED, far_min_ml = 0;
  double theta = 0.5;
  std::vector<int> faraggs;
  // symmetric repulsion (ge_sym.hpp): sweep units and per-tile progress counters
  bool sym = false;
  bool wide = false;  // the wide schedule (ge_pair.hpp): dim > 4, or GE_WIDE_MIN_DIM
  ge::DevBuf<int4> units;
  ge::DevBuf<int> prog;
  ge::DevBuf<double> hand;  // column sums handed between sweeps, component-major [dim][n]
  ge::DevBuf<int> sym_err;  // set by a hand-over wait that timed out
  long long sym_limit = 0;  // that wait's bound in ticks of the device wall clock
  int nunits = 0, ntiles = 0, sym_blocks = 0;
  int rows_mode = 0, swept = 0;  // streamed aggregates by schedule (ge_sym.hpp)
  std::vector<ge::SchedInt4> h_units;  // host copy of `units` (timeline dumps)
  ge::DevBuf<long long> stamps;       // GE_SYM_STAMPS: per-unit timeline of the last launch
  std::string stamp_path;
  double streamed_pairs = 0.0;
  ge::DevBuf<double> Fscr, Fprev, Xa, Xb, DP;
  // the size classes are independent: streamed path, large, mid and small
  // packs each run on their own stream and join the context stream at the end
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t fork = nullptr, join[3] = {nullptr, nullptr, nullptr};
  bool profiling = false;
  ge::EventPool ev{64};    // 4 per timed run: start, resident end, streamed start/end
  ge::EventPool rev{256};  // 2 per profiled repulsion launch
  ge::EventPool aev{256};  // 2 per profiled member-row pass (FamlRows)
  long long streamed_entries = 0;  // CSR entries of the streamed members' rows
  // aggregates split by row tiles across the ranks of `comm`: this
  // rank computes its rows' forces and updates, and the split aggregates' rows are
  // exchanged after every iteration (exchange_rows, stream-ordered)
  ge_comm* comm = nullptr;
  ge::DevBuf<int> irows;  // positions initialised / given deg+1: rows + the other ranks' split rows
  int nirows = 0;
  ge::DevBuf<int> xrows, xcounts, xfirst;
  ge::DevBuf<double> xbuf;
  std::vector<int> h_xcounts, h_xfirst;
  int xwidth = 0;
};

namespace ge {

// blocks per CU of faml_sym_repulse<dim> (1 where the sweeps are not compiled)
static int sym_occupancy(int dim) {
  int occ = 1;
  if (dim > kNarrowMaxDim) return occ;
  dispatch_dim_narrow(dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    GE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &occ, (const void*)faml_sym_repulse<D, false>, kSymT, 0));
  });
  return occ;
}

// The scheduler's inputs: the caller's lists and device figures, with what the
// dimension and the environment settle.
static FamlSchedIn faml_sched_in(const int* h_pt_ip, const std::vector<int>& aggs,
                                 const std::vector<int>& split, int rank, int nranks, int dim,
                                 int mode, int cus, int sym_occ) {
  FamlSchedIn in;
  in.pt_ip = h_pt_ip;
  in.aggs = &aggs;
  in.split = &split;
  in.rank = rank;
  in.nranks = nranks;
  in.dim = dim;
  in.mode = mode;
  in.large_cap = large_cap(dim);
  in.wide = wide_dim(dim);
  in.cus = cus;
  in.sym_occ = sym_occ;
  in.knobs = faml_knobs_from_env();
  return in;
}

// aggs: the aggregates this plan runs (strictly increasing ids).
// split: aggregates whose row tiles are dealt over the ranks of pl->comm (the
// same list on every rank; tiles [T r / N, T (r + 1) / N) to rank r).
// The schedule is faml_schedule's (ge_faml_sched.hpp); this is its device part.
static void faml_plan_build(ge_faml_plan* pl, const int* h_pt_ip, const std::vector<int>& aggs,
                            const std::vector<int>& split = std::vector<int>()) {
  hipStream_t st = pl->ctx->stream;
  const int dim = pl->dim, n = pl->n;
  const int cus = device_cus();
  const int nranks = pl->comm ? pl->comm->nranks : 1;
  FamlSchedIn sin = faml_sched_in(h_pt_ip, aggs, split, pl->comm ? pl->comm->rank : 0, nranks,
                                  dim, pl->mode, cus, sym_occupancy(dim));
  FamlSched s = faml_schedule(sin);
  pl->far_min_ml = sin.knobs.far_min_ml;
  bool dp_done = false;
  if (pl->mode == GE_MODE_FARFIELD) {
    // every internal deg + 1 of the streamed rows must be a mass: checked once, here
    pl->far_reason = sin.wide || dim > kNarrowMaxDim ? GE_FAR_DIM
                     : s.faraggs.empty()            ? GE_FAR_SMALL
                                                    : GE_FAR_ACTIVE;
    if (pl->far_reason == GE_FAR_ACTIVE) {
      pl->irows.alloc(s.irows.size());
      pl->irows.upload(s.irows.data(), s.irows.size(), st);
      pl->DP.alloc(n);
      hipLaunchKernelGGL(faml_huge_dp, dim3(((int)s.irows.size() + kHT - 1) / kHT), dim3(kHT), 0,
                         st, (int)s.irows.size(), pl->irows.p, pl->pt_ix, pl->vA, pl->ip, pl->ix,
                         pl->dx, pl->DP.p, pl->c.use_weights);
      GE_HIP(hipGetLastError());
      dp_done = true;
      if (!far_masses_ok_rows(st, (int)s.irows.size(), pl->irows.p, pl->DP.p)) {
        pl->far_reason = GE_FAR_MASS;  // the whole plan runs FAST
        sin.mode = GE_MODE_FAST;
        s = faml_schedule(sin);
      }
    }
  }
  pl->faraggs = s.faraggs;
  pl->res_cap = s.res_cap;
  std::copy(s.census, s.census + 4, pl->census);
  pl->off_m = s.off_m;
  pl->off_l = s.off_l;
  pl->ns = s.ns;
  pl->nm = s.nm;
  pl->nl = s.nl;
  pl->nrows = (int)s.rows.size();
  pl->nirows = (int)s.irows.size();
  pl->nitems = (int)s.items.size();
  pl->nhuge = (int)s.huge.size();
  pl->R = s.R;
  pl->code = s.code;
  pl->wide = s.wide;
  pl->fast = s.fast;
  pl->nfitems = (int)s.fitems.size();
  pl->sym = s.sym;
  pl->nunits = (int)s.units.size();
  pl->ntiles = s.ntiles;
  pl->sym_blocks = s.sym_blocks;
  pl->rows_mode = s.rows_mode;
  pl->swept = s.swept;
  pl->streamed_pairs = s.streamed_pairs;
  if (!s.rows.empty()) {  // degree classes of the streamed members' CSR rows
    std::vector<int> h_ip(n + 1), h_ptix(n), erows;
    GE_HIP(hipMemcpyAsync(h_ip.data(), pl->ip, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, st));
    GE_HIP(hipMemcpyAsync(h_ptix.data(), pl->pt_ix, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    GE_HIP(hipStreamSynchronize(st));
    std::vector<int> deg(s.rows.size());
    for (size_t q = 0; q < s.rows.size(); ++q) {
      const int v = h_ptix[s.rows[q]];
      deg[q] = h_ip[v + 1] - h_ip[v];
      pl->streamed_entries += deg[q];
    }
    // the in-aggregate repulsion is not far above the external pulls (measured
    // at C3: every heavy row left the binade), so heavy rows store their terms
    std::vector<int> hdeg;
    classify_rows(s.rows, deg, erows, pl->ecls, kSegStore, &hdeg);
    pl->ecode.alloc(std::max(h_ip[n], 1));
    pl->erows.alloc(erows.size());
    pl->erows.upload(erows.data(), erows.size(), st);
    pl->ecls.bind(pl->erows.p);
    pl->rstreams.attach(pl->ecls, dim, st, hdeg);
  }
  if (s.sym && !s.huge.empty()) {  // sweep units, hand-over buffers and progress counters
    pl->units.alloc(s.units.size());
    pl->units.upload(reinterpret_cast<const int4*>(s.units.data()), s.units.size(), st);
    if (const char* e = std::getenv("GE_SYM_STAMPS")) {  // diagnostics: timeline of each launch
      pl->stamp_path = e;
      pl->h_units = s.units;
      pl->stamps.alloc(s.units.size() * kStampWords);
    }
    pl->prog.alloc(std::max(s.ntiles, 1));
    if (s.ntiles > 0) pl->hand.alloc((size_t)n * dim);
    pl->sym_err.alloc(1);
    GE_HIP(hipMemsetAsync(pl->sym_err.p, 0, sizeof(int), st));
    int dev = 0, khz = 0;
    GE_HIP(hipGetDevice(&dev));
    GE_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    // one hand-over normally waits at most a few tile-times (tens of microseconds)
    pl->sym_limit = (long long)std::max(khz, 1000) * 5000;  // ~5 s
  }
  // 4 waves per SIMD: more items per wave for the queue to balance (C3 level
  // 0: 961 ms per call against 1091 ms at the full 8 waves per SIMD)
  pl->rep_blocks = cus * std::min(4, rep_occupancy(dim, pl->code));
  if (pl->fast) {  // four waves per SIMD, the occupancy faml_fast_repulse is built for
    int focc = 1;
    dispatch_dim_narrow(dim, [&](auto Dc) {
      constexpr int D = decltype(Dc)::value;
      GE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &focc, (const void*)faml_fast_repulse<D, kFastR>, kHT, 0));
    });
    pl->fast_blocks = cus * std::min(4, std::max(focc, 1));
    pl->fitems.alloc(s.fitems.size());
    pl->fitems.upload(reinterpret_cast<const int4*>(s.fitems.data()), s.fitems.size(), st);
  }
  pl->pos.alloc(std::max(n, 1));
  pl->order.alloc(std::max<size_t>(s.order.size(), 1));
  pl->beg.alloc(std::max<size_t>(s.beg.size(), 1));
  pl->rows.alloc(std::max<size_t>(s.rows.size(), 1));
  pl->items.alloc(std::max<size_t>(s.items.size(), 1));
  pl->queue.alloc(std::max(pl->iterations, 1));
  pl->huge.alloc(std::max<size_t>(s.huge.size(), 1));
  if (!dp_done) {
    pl->irows.alloc(std::max<size_t>(s.irows.size(), 1));
    pl->irows.upload(s.irows.data(), s.irows.size(), st);
  }
  pl->order.upload(s.order.data(), s.order.size(), st);
  pl->beg.upload(s.beg.data(), s.beg.size(), st);
  pl->rows.upload(s.rows.data(), s.rows.size(), st);
  pl->items.upload(reinterpret_cast<const int2*>(s.items.data()), s.items.size(), st);
  pl->huge.upload(s.huge.data(), s.huge.size(), st);
  if (!split.empty() && nranks > 1) {  // the per-iteration exchange of the split rows
    pl->h_xcounts = s.xcounts;
    pl->h_xfirst.assign(nranks + 1, 0);
    for (int r = 0; r < nranks; ++r) pl->h_xfirst[r + 1] = pl->h_xfirst[r] + s.xcounts[r];
    pl->xwidth = std::max(1, *std::max_element(s.xcounts.begin(), s.xcounts.end()));
    pl->xrows.alloc(std::max<size_t>(s.xr.size(), 1));
    pl->xrows.upload(s.xr.data(), s.xr.size(), st);
    pl->xcounts.alloc(nranks);
    pl->xcounts.upload(s.xcounts.data(), nranks, st);
    pl->xfirst.alloc(nranks + 1);
    pl->xfirst.upload(pl->h_xfirst.data(), nranks + 1, st);
    pl->xbuf.alloc((size_t)pl->xwidth * dim * nranks);
  }
  pl->Fscr.alloc((size_t)std::max(n, 1) * dim);
  pl->Fprev.alloc((size_t)std::max(n, 1) * dim);
  if (pl->nirows > 0) {
    pl->Xa.alloc((size_t)n * dim);
    pl->Xb.alloc((size_t)n * dim);
    if (!dp_done) pl->DP.alloc(n);
  }
  if (!pl->faraggs.empty()) {  // items of 64 rows unless GE_FAR_R=4 (256), as on the single level
    std::vector<int> base, size;
    for (int a : pl->faraggs) {
      base.push_back(h_pt_ip[a]);
      size.push_back(h_pt_ip[a + 1] - h_pt_ip[a]);
    }
    int item_rows = kFarLeaf;
    if (const char* e = std::getenv("GE_FAR_R")) item_rows = std::atoi(e) == 4 ? 4 * kFarLeaf : kFarLeaf;
    pl->far = far_seg_create(st, dim, pl->theta, item_rows, cus, base, size);
  }
  hipLaunchKernelGGL(pos_of_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, pl->pt_ix,
                     pl->pos.p);
  if (pl->nrows > 0) {
    hipLaunchKernelGGL(edge_code_kernel, dim3((pl->nrows + 255) / 256), dim3(256), 0, st,
                       pl->nrows, pl->rows.p, pl->pt_ip, pl->pt_ix, pl->pos.p, pl->vA, pl->ip,
                       pl->ix, pl->ecode.p);
  }
  if (pl->nirows > 0 && !dp_done)
    hipLaunchKernelGGL(faml_huge_dp, dim3((pl->nirows + kHT - 1) / kHT), dim3(kHT), 0, st,
                       pl->nirows, pl->irows.p, pl->pt_ix, pl->vA, pl->ip, pl->ix, pl->dx, pl->DP.p,
                       pl->c.use_weights);
  GE_HIP(hipGetLastError());
  for (int k = 0; k < 3; ++k) {
    GE_HIP(hipStreamCreateWithFlags(&pl->side[k], hipStreamNonBlocking));
    GE_HIP(hipEventCreateWithFlags(&pl->join[k], hipEventDisableTiming));
  }
  GE_HIP(hipEventCreateWithFlags(&pl->fork, hipEventDisableTiming));
  GE_HIP(hipStreamSynchronize(st));
}

// One repulsion pass over the plan's streamed rows on stream ss: reads the
// coordinates `cur` (P_T storage order) and DP, writes each row's sum to F at its
// P_T position.  queue: a zeroed counter of its own for this launch.
template <int D>
static void faml_launch_repulse(ge_faml_plan* pl, hipStream_t ss, int* queue, const double* cur,
                                double* F) {
  const FaConst& c = pl->c;
  if (pl->fast || pl->far) {
    // the far aggregates' pass first (the largest aggregates), then the FAST items of
    // the streamed rows that are left; the two write disjoint rows of F
    if (pl->far) far_seg_repulse(pl->far, ss, cur, pl->DP.p, c.repel, F);
    if constexpr (D <= kNarrowMaxDim)  // neither is ever set on the wide schedule
      if (pl->fast)
        hipLaunchKernelGGL((faml_fast_repulse<D, kFastR>), dim3(pl->fast_blocks), dim3(kHT), 0, ss,
                           pl->nfitems, pl->fitems.p, queue, pl->pt_ip, cur, pl->DP.p, c.repel, F);
  } else if (pl->sym) {
    if (pl->ntiles) GE_HIP(hipMemsetAsync(pl->prog.p, 0, sizeof(int) * pl->ntiles, ss));
    double* H = pl->hand.p;  // hand-overs component-major (ge_sym.hpp sym_handover)
    const size_t hs = (size_t)pl->n;
    int* err = pl->sym_err.p;
    const long long lim = pl->sym_limit;
    if (!pl->stamp_path.empty()) {
      if constexpr (D <= kNarrowMaxDim)  // sym is never set on the wide schedule
        hipLaunchKernelGGL((faml_sym_repulse<D, false, true>), dim3(pl->sym_blocks), dim3(kSymT),
                           0, ss, pl->nunits, pl->units.p, queue, pl->pt_ip, cur, pl->DP.p,
                           c.repel, F, H, hs, pl->prog.p, err, lim, pl->stamps.p);
    } else {
      sym_repulse_launch(D, pl->sym_blocks, ss, pl->nunits, pl->units.p, queue, pl->pt_ip, cur,
                         pl->DP.p, c.repel, F, H, hs, pl->prog.p, err, lim);
    }
  } else {
    launch_big_repulse<D>(pl->code, pl->rep_blocks, ss, pl->nitems, pl->items.p, queue, pl->pt_ip,
                          cur, pl->DP.p, c.repel, F, pl->wide);
  }
}

// A hand-over wait of the symmetric sweeps that timed out fails the call.
static void faml_check_sym(ge_faml_plan* pl, hipStream_t st) {
  if (!pl->sym || pl->nunits <= 0) return;
  int err = 0;
  GE_HIP(hipMemcpyAsync(&err, pl->sym_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
  GE_HIP(hipStreamSynchronize(st));
  if (err) {
    GE_HIP(hipMemsetAsync(pl->sym_err.p, 0, sizeof(int), st));
    throw Error(GE_ERR_STATE, "forceAtlasMultilevel: a symmetric sweep's hand-over wait timed out");
  }
}

// ge_faml_plan_repulse: one pass on the caller's coordinates, on the context stream.
// It uses the first queue counter, which every run zeroes again before its launches.
static void faml_plan_repulse(ge_faml_plan* pl, const double* x, double* frep) {
  hipStream_t st = pl->ctx->stream;
  if (pl->nrows <= 0) return;
  GE_HIP(hipMemsetAsync(pl->queue.p, 0, sizeof(int), st));
  dispatch_dim(pl->dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    faml_launch_repulse<D>(pl, st, pl->queue.p, x, frep);
  });
  GE_HIP(hipGetLastError());
  faml_check_sym(pl, st);
  GE_HIP(hipStreamSynchronize(st));
}

static void faml_plan_run(ge_faml_plan* pl, const double* cA, const double* rA, const double* init,
                          double* X) {
  hipStream_t st = pl->ctx->stream;
  hipEvent_t* ev = pl->profiling ? pl->ev.take(4) : nullptr;
  const int iters = pl->iterations;
  const FaConst& c = pl->c;
  dispatch_dim(pl->dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    GE_HIP(hipEventRecord(pl->fork, st));
    for (int k = 0; k < 3; ++k) GE_HIP(hipStreamWaitEvent(pl->side[k], pl->fork, 0));
    if (ev) GE_HIP(hipEventRecord(ev[0], st));
    // resident classes: large on side[1], mid on side[2], small on the context stream
    auto launch_resident = [&] {
      if (pl->nl > 0)
        hipLaunchKernelGGL((faml_resident<D, 256, large_cap(D)>), dim3(pl->nl), dim3(256), 0,
                           pl->side[1], pl->order.p, pl->beg.p + pl->off_l, pl->pt_ip, pl->pt_ix,
                           pl->pos.p, pl->vA, pl->ip, pl->ix, pl->dx, cA, rA, init, pl->Fscr.p,
                           pl->Fprev.p, X, iters, c);
      if (pl->nm > 0)
        hipLaunchKernelGGL((faml_resident<D, 256, 256>), dim3(pl->nm), dim3(256), 0, pl->side[2],
                           pl->order.p, pl->beg.p + pl->off_m, pl->pt_ip, pl->pt_ix, pl->pos.p,
                           pl->vA, pl->ip, pl->ix, pl->dx, cA, rA, init, pl->Fscr.p, pl->Fprev.p,
                           X, iters, c);
      if (pl->ns > 0)
        hipLaunchKernelGGL((faml_resident<D, 64, 64>), dim3(pl->ns), dim3(64), 0, st, pl->order.p,
                           pl->beg.p, pl->pt_ip, pl->pt_ix, pl->pos.p, pl->vA, pl->ip, pl->ix,
                           pl->dx, cA, rA, init, pl->Fscr.p, pl->Fprev.p, X, iters, c);
    };
    // streamed path (side[0])
    hipStream_t ss = pl->side[0];
    if (ev) GE_HIP(hipEventRecord(ev[2], ss));
    if (pl->nirows > 0) {
      const int nr = pl->nirows;
      hipLaunchKernelGGL((faml_huge_init<D>), dim3((nr + kHT - 1) / kHT), dim3(kHT), 0, ss,
                         nr, pl->irows.p, init, pl->Xa.p, pl->Fprev.p);
      GE_HIP(hipMemsetAsync(pl->queue.p, 0, sizeof(int) * iters, ss));
      double* cur = pl->Xa.p;
      double* nxt = pl->Xb.p;
      for (int it = 0; it < iters; ++it) {
        hipEvent_t* re = pl->profiling ? pl->rev.take(2) : nullptr;
        if (re) GE_HIP(hipEventRecord(re[0], ss));
        const FamlRows<D> fr{pl->pt_ip, pl->pt_ix, pl->ecode.p, pl->ip, pl->vA, pl->dx,
                             cA, cur, pl->DP.p, pl->Fscr.p, nxt, pl->Fprev.p, c};
        faml_launch_repulse<D>(pl, ss, pl->queue.p + it, cur, pl->Fscr.p);
        if (re) GE_HIP(hipEventRecord(re[1], ss));
        hipEvent_t* ae = pl->profiling ? pl->aev.take(2) : nullptr;
        if (ae) GE_HIP(hipEventRecord(ae[0], ss));
        if (pl->nrows > 0) launch_rows<D>(pl->ecls, fr, ss, pl->rstreams);
        if (ae) GE_HIP(hipEventRecord(ae[1], ss));
        if (pl->xwidth > 0)  // every rank's rows of the split aggregates, for the next step
          exchange_rows(pl->comm, ss, D, pl->xrows.p, pl->xcounts.p, pl->xfirst.p,
                        pl->h_xcounts.data(), pl->h_xfirst.data(), pl->xwidth, pl->xbuf.p, nxt);
        std::swap(cur, nxt);
      }
      hipLaunchKernelGGL((faml_huge_finish<D>), dim3(pl->nhuge), dim3(kHT), 0, ss, pl->huge.p,
                         pl->pt_ip, pl->pt_ix, cur, cA, rA, X);
    }
    if (ev) GE_HIP(hipEventRecord(ev[3], ss));
    // the resident classes beside the streamed path: queued after it, they cost the
    // repulsion launch ~0.3 ms; run after it, ~1.4 ms per step; queued before it,
    // nothing changes (profiles/r04/ab_launch_order.log)
    launch_resident();
    for (int k = 0; k < 3; ++k) GE_HIP(hipEventRecord(pl->join[k], pl->side[k]));
    for (int k = 1; k < 3; ++k) GE_HIP(hipStreamWaitEvent(st, pl->join[k], 0));
    if (ev) GE_HIP(hipEventRecord(ev[1], st));  // resident classes done
    GE_HIP(hipStreamWaitEvent(st, pl->join[0], 0));
  });
  GE_HIP(hipGetLastError());
  faml_check_sym(pl, st);
  if (!pl->stamp_path.empty() && pl->nunits > 0) {  // the last launch's timeline
    std::vector<long long> h((size_t)pl->nunits * kStampWords);
    GE_HIP(hipStreamSynchronize(st));
    GE_HIP(hipMemcpy(h.data(), pl->stamps.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(pl->stamp_path.c_str(), "wb")) {
      const int hdr[4] = {pl->nunits, kStampWords, pl->sym_blocks, kSymT};
      std::fwrite(hdr, sizeof(int), 4, f);
      std::fwrite(pl->h_units.data(), sizeof(SchedInt4), pl->h_units.size(), f);
      std::fwrite(h.data(), sizeof(long long), h.size(), f);
      std::fclose(f);
    }
  }
}

void sym_repulse_launch(int dim, int blocks, hipStream_t s, int nunits, const int4* units,
                        int* queue, const int* seg, const double* X, const double* DP,
                        double repel, double* F, double* H, size_t hs, int* prog, int* err,
                        long long limit) {
  dispatch_dim_narrow(dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    if (repel == 1.0)
      hipLaunchKernelGGL((faml_sym_repulse<D, true>), dim3(blocks), dim3(kSymT), 0, s, nunits,
                         units, queue, seg, X, DP, repel, F, H, hs, prog, err, limit, nullptr);
    else
      hipLaunchKernelGGL((faml_sym_repulse<D, false>), dim3(blocks), dim3(kSymT), 0, s, nunits,
                         units, queue, seg, X, DP, repel, F, H, hs, prog, err, limit, nullptr);
  });
  GE_HIP(hipGetLastError());
}

// Blocks per CU of a single-level symmetric launch (one aggregate of n / 64 row
// tiles: one convoy of sweeps, each behind the one before).  Two of the four that
// fit: C2 1539.8 ms per iteration against 1631.9 at three and 1806.8 at four
// (profiles/r04/c2_sym_blocks.log) -- fewer sweeps in flight wait less on each other.
int sym_blocks_per_cu(int dim) { return std::min(std::max(sym_occupancy(dim), 1), 2); }

static void faml_plan_free(ge_faml_plan* pl) {
  if (!pl) return;
  for (int k = 0; k < 3; ++k) {
    if (pl->side[k]) {
      (void)hipStreamSynchronize(pl->side[k]);
      (void)hipStreamDestroy(pl->side[k]);
    }
    if (pl->join[k]) (void)hipEventDestroy(pl->join[k]);
  }
  if (pl->fork) (void)hipEventDestroy(pl->fork);
  if (pl->far) far_seg_destroy(pl->far);
  delete pl;
}

// The caller's graph, P_T and parameters of a new plan.
static void fill_plan(ge_faml_plan* pl, ge_ctx* ctx, ge_comm* comm, int n, const int* d_ip,
                      const int* d_ix, const double* d_dx, int m, const int* d_pt_ip,
                      const int* d_pt_ix, const int* d_vA, int dim, int iterations,
                      const ge_fa_params& p) {
  pl->ctx = ctx;
  pl->comm = comm;
  pl->n = n;
  pl->m = m;
  pl->dim = dim;
  pl->iterations = iterations;
  pl->ip = d_ip;
  pl->ix = d_ix;
  pl->dx = d_dx;
  pl->pt_ip = d_pt_ip;
  pl->pt_ix = d_pt_ix;
  pl->vA = d_vA;
  pl->c = make_fa_const(p);
  check_far_params(p);
  pl->mode = p.mode;
  pl->theta = p.theta;
}

void faml_run_device(ge_ctx* ctx, int n, const int* d_ip, const int* d_ix, const double* d_dx,
                     int m, const int* h_pt_ip, const int* d_pt_ip, const int* d_pt_ix,
                     const int* d_vA, const double* d_cA, const double* d_rA,
                     const double* d_init, double* d_x, int dim, int iterations,
                     const ge_fa_params& p) {
  GE_REQUIRE(h_pt_ip[m] == n, "P_T must have one entry per fine vertex");
  auto* pl = new ge_faml_plan();
  try {
    fill_plan(pl, ctx, nullptr, n, d_ip, d_ix, d_dx, m, d_pt_ip, d_pt_ix, d_vA, dim, iterations, p);
    std::vector<int> all(m);
    std::iota(all.begin(), all.end(), 0);
    faml_plan_build(pl, h_pt_ip, all);
    faml_plan_run(pl, d_cA, d_rA, d_init, d_x);
    GE_HIP(hipStreamSynchronize(ctx->stream));
  } catch (...) {
    faml_plan_free(pl);
    throw;
  }
  faml_plan_free(pl);
}

}  // namespace ge

extern "C" {

static int faml_plan_create_impl(ge_ctx* ctx, int n, const int* d_ip, const int* d_ix,
                                 const double* d_dx, int m, const int* h_pt_ip,
                                 const int* d_pt_ip, const int* d_pt_ix, const int* d_vA,
                                 int dim, const ge_fa_params* p, int iterations,
                                 const std::vector<int>& aggs, ge_faml_plan** out,
                                 ge_comm* comm = nullptr,
                                 const std::vector<int>& split = std::vector<int>()) {
  return ge::guarded([&] {
    ge::DeviceGuard g(ctx);
    auto* pl = new ge_faml_plan();
    try {
      ge::fill_plan(pl, ctx, comm, n, d_ip, d_ix, d_dx, m, d_pt_ip, d_pt_ix, d_vA, dim,
                    iterations, *p);
      ge::faml_plan_build(pl, h_pt_ip, aggs, split);
    } catch (...) {
      ge::faml_plan_free(pl);
      throw;
    }
    *out = pl;
  });
}

static void faml_plan_check(ge_ctx* ctx, int n, int m, const int* h_pt_ip, int dim,
                            const ge_fa_params* p, void* out) {
  GE_REQUIRE(ctx && p && out && h_pt_ip, "null argument");
  GE_REQUIRE(dim >= 1 && dim <= ge::kMaxDim, "dimension must be 1..16");
  GE_REQUIRE(n > 0 && m > 0 && h_pt_ip[0] == 0 && h_pt_ip[m] == n,
             "P_T must have one entry per fine vertex");
}

// ids[0..cnt): strictly increasing aggregate ids below m, copied to `out`.
static void check_ids(const int* ids, int cnt, int m, const char* msg, std::vector<int>& out) {
  for (int q = 0; q < cnt; ++q)
    GE_REQUIRE(ids[q] >= 0 && ids[q] < m && (q == 0 || ids[q] > ids[q - 1]), msg);
  out.assign(ids, ids + cnt);
}

int ge_faml_plan_create(ge_ctx* ctx, int n, const int* d_ip, const int* d_ix, const double* d_dx,
                        int m, const int* h_pt_ip, const int* d_pt_ip, const int* d_pt_ix,
                        const int* d_vA, int dim, const ge_fa_params* p, int iterations,
                        int agg_begin, int agg_end, ge_faml_plan** out) {
  std::vector<int> aggs;
  const int rc = ge::guarded([&] {
    faml_plan_check(ctx, n, m, h_pt_ip, dim, p, out);
    GE_REQUIRE(0 <= agg_begin && agg_begin <= agg_end && agg_end <= m, "bad aggregate range");
    aggs.resize(agg_end - agg_begin);
    std::iota(aggs.begin(), aggs.end(), agg_begin);
  });
  if (rc != GE_OK) return rc;
  return faml_plan_create_impl(ctx, n, d_ip, d_ix, d_dx, m, h_pt_ip, d_pt_ip, d_pt_ix, d_vA, dim,
                               p, iterations, aggs, out);
}

int ge_faml_plan_create_subset(ge_ctx* ctx, int n, const int* d_ip, const int* d_ix,
                               const double* d_dx, int m, const int* h_pt_ip,
                               const int* d_pt_ip, const int* d_pt_ix, const int* d_vA, int dim,
                               const ge_fa_params* p, int iterations, const int* h_aggs,
                               int n_aggs, ge_faml_plan** out) {
  std::vector<int> aggs;
  const int rc = ge::guarded([&] {
    faml_plan_check(ctx, n, m, h_pt_ip, dim, p, out);
    GE_REQUIRE(n_aggs >= 0 && (h_aggs || n_aggs == 0), "bad aggregate list");
    check_ids(h_aggs, n_aggs, m, "aggregate ids must be strictly increasing and < m", aggs);
  });
  if (rc != GE_OK) return rc;
  return faml_plan_create_impl(ctx, n, d_ip, d_ix, d_dx, m, h_pt_ip, d_pt_ip, d_pt_ix, d_vA, dim,
                               p, iterations, aggs, out);
}

int ge_faml_plan_create_shard(ge_ctx* ctx, ge_comm* comm, int n, const int* d_ip,
                              const int* d_ix, const double* d_dx, int m, const int* h_pt_ip,
                              const int* d_pt_ip, const int* d_pt_ix, const int* d_vA, int dim,
                              const ge_fa_params* p, int iterations, const int* h_aggs,
                              int n_aggs, const int* h_split, int n_split, ge_faml_plan** out) {
  std::vector<int> aggs, split;
  const int rc = ge::guarded([&] {
    faml_plan_check(ctx, n, m, h_pt_ip, dim, p, out);
    GE_REQUIRE(comm && comm->ctx == ctx, "the communicator must belong to the plan's context");
    GE_REQUIRE(n_aggs >= 0 && (h_aggs || n_aggs == 0) && n_split >= 0 && (h_split || n_split == 0),
               "bad aggregate lists");
    check_ids(h_aggs, n_aggs, m, "aggregate ids must be strictly increasing and < m", aggs);
    check_ids(h_split, n_split, m, "split aggregate ids must be strictly increasing and < m",
              split);
    std::vector<char> seen(m, 0);
    for (int a : aggs) seen[a] = 1;
    for (int a : split) GE_REQUIRE(!seen[a], "an aggregate is both whole and split");
  });
  if (rc != GE_OK) return rc;
  return faml_plan_create_impl(ctx, n, d_ip, d_ix, d_dx, m, h_pt_ip, d_pt_ip, d_pt_ix, d_vA, dim,
                               p, iterations, aggs, out, comm, split);
}

int ge_faml_plan_run(ge_faml_plan* pl, const double* d_cA, const double* d_rA,
                     const double* d_init, double* d_coords) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && d_cA && d_rA && d_init && d_coords, "null argument");
    ge::DeviceGuard g(pl->ctx);
    ge::faml_plan_run(pl, d_cA, d_rA, d_init, d_coords);
  });
}

int ge_faml_plan_repulse(ge_faml_plan* pl, const double* d_x, double* d_frep) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && d_x && d_frep, "null argument");
    ge::DeviceGuard g(pl->ctx);
    ge::faml_plan_repulse(pl, d_x, d_frep);
  });
}

int ge_faml_plan_mode(ge_faml_plan* pl, int* mode, int* fast_items) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && mode && fast_items, "null argument");
    *mode = pl->far ? GE_MODE_FARFIELD : pl->fast ? GE_MODE_FAST : GE_MODE_STRICT;
    *fast_items = pl->nfitems;
  });
}

int ge_faml_plan_far_info(ge_faml_plan* pl, int* active, int* reason, double* theta,
                          int* far_min_ml, int* item_rows, int* key_bits, int* aggregates,
                          long long* rows, int* bad_boxes, long long* accepted,
                          long long* exact_leaves, long long* pair_terms, double* prep_ms,
                          double* item_ms) {
  return ge::guarded([&] {
    GE_REQUIRE(pl, "null plan");
    ge::DeviceGuard g(pl->ctx);
    if (active) *active = pl->far ? 1 : 0;
    if (reason) *reason = pl->far_reason;
    if (far_min_ml) *far_min_ml = pl->far_min_ml;
    if (pl->far) {
      // the run's passes are on the streamed path's stream, which the context stream
      // joins at the end of a run; the hook runs on the context stream
      GE_HIP(hipStreamSynchronize(pl->side[0]));
      ge::far_seg_info(pl->far, pl->ctx->stream, theta, item_rows, key_bits, aggregates, rows,
                       bad_boxes, accepted, exact_leaves, pair_terms, prep_ms, item_ms);
      return;
    }
    if (theta) *theta = pl->theta;
    if (item_rows) *item_rows = 0;
    if (key_bits) *key_bits = 0;
    if (aggregates) *aggregates = 0;
    if (rows) *rows = 0;
    if (bad_boxes) *bad_boxes = 0;
    if (accepted)
      for (int l = 0; l < GE_FAR_MAX_LEVELS; ++l) accepted[l] = 0;
    if (exact_leaves) *exact_leaves = 0;
    if (pair_terms) *pair_terms = 0;
    if (prep_ms) *prep_ms = 0.0;
    if (item_ms) *item_ms = 0.0;
  });
}

int ge_faml_plan_far_aggregates(ge_faml_plan* pl, int* aggs) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && aggs, "null argument");
    std::copy(pl->faraggs.begin(), pl->faraggs.end(), aggs);
  });
}

// the far aggregate's index in the engine, or GE_ERR_ARG
static int far_segment_of(ge_faml_plan* pl, int agg) {
  GE_REQUIRE(pl, "null plan");
  const auto it = std::find(pl->faraggs.begin(), pl->faraggs.end(), agg);
  GE_REQUIRE(pl->far && it != pl->faraggs.end(), "not a far-field aggregate of this plan");
  return (int)(it - pl->faraggs.begin());
}

int ge_faml_plan_far_shape(ge_faml_plan* pl, int agg, int* members, int* levels,
                           int* level_cells, int* items) {
  return ge::guarded([&] {
    ge::far_seg_shape(pl->far, far_segment_of(pl, agg), members, levels, level_cells, items);
  });
}

int ge_faml_plan_far_layout(ge_faml_plan* pl, int agg, int* perm, unsigned long long* keys,
                            double* box, double* cells, double* items) {
  return ge::guarded([&] {
    const int f = far_segment_of(pl, agg);
    ge::DeviceGuard g(pl->ctx);
    GE_HIP(hipStreamSynchronize(pl->side[0]));
    ge::far_seg_layout(pl->far, pl->ctx->stream, f, perm, keys, box, cells, items);
  });
}

int ge_faml_plan_set_profiling(ge_faml_plan* pl, int enable) {
  return ge::guarded([&] {
    GE_REQUIRE(pl, "null plan");
    pl->profiling = enable != 0;
    pl->ev.reset();
    pl->rev.reset();
    pl->aev.reset();
  });
}

int ge_faml_plan_kernel_ms(ge_faml_plan* pl, double* resident_ms, double* streamed_ms,
                           int* runs) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && resident_ms && streamed_ms && runs, "null argument");
    ge::DeviceGuard g(pl->ctx);
    GE_HIP(hipStreamSynchronize(pl->ctx->stream));
    *resident_ms = pl->ev.mean_ms(4, 0, 1, runs);
    *streamed_ms = pl->ev.mean_ms(4, 2, 3);
  });
}

int ge_faml_plan_repulse_ms(ge_faml_plan* pl, double* ms, int* launches, double* pairs) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && ms && launches && pairs, "null argument");
    *pairs = pl->streamed_pairs;
    ge::DeviceGuard g(pl->ctx);
    GE_HIP(hipStreamSynchronize(pl->ctx->stream));
    *ms = pl->rev.mean_ms(2, 0, 1, launches);
  });
}

int ge_faml_plan_rows_ms(ge_faml_plan* pl, double* ms, int* passes, long long* rows,
                         long long* entries) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && ms && passes && rows && entries, "null argument");
    *rows = pl->nrows;
    *entries = pl->streamed_entries;
    ge::DeviceGuard g(pl->ctx);
    GE_HIP(hipStreamSynchronize(pl->ctx->stream));
    *ms = pl->aev.mean_ms(2, 0, 1, passes);
  });
}

int ge_faml_plan_schedule(ge_faml_plan* pl, int* sweeps, int* banded, int* row_blocks,
                          int* units) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && sweeps && banded && row_blocks && units, "null argument");
    *sweeps = pl->swept;
    *banded = 0;  // bands were removed in round 5 (the ABI keeps the field)
    *row_blocks = pl->rows_mode;
    *units = pl->nunits;
  });
}

int ge_faml_plan_classes(ge_faml_plan* pl, int* res_cap, int* aggregates, int* blocks,
                          int* rows) {
  return ge::guarded([&] {
    GE_REQUIRE(pl && res_cap && aggregates && blocks && rows, "null argument");
    *res_cap = pl->res_cap;
    for (int k = 0; k < 4; ++k) aggregates[k] = pl->census[k];
    blocks[0] = pl->ns;
    blocks[1] = pl->nm;
    blocks[2] = pl->nl;
    const ge::RowClasses& rc = pl->ecls;
    const int r[6] = {rc.ntiles, rc.nheavy, rc.nseg, rc.seg_mode, rc.nearly, rc.nseg_early};
    for (int k = 0; k < 6; ++k) rows[k] = r[k];
  });
}

int ge_faml_plan_destroy(ge_faml_plan* pl) {
  return ge::guarded([&] { ge::faml_plan_free(pl); });
}

struct ge_faml_sched {
  ge::FamlSched s;
  std::vector<int> scalars;
};

int ge_faml_sched_create(int m, const int* h_pt_ip, const int* h_aggs, int n_aggs,
                         const int* h_split, int n_split, int rank, int nranks, int dim, int mode,
                         int cus, int sym_occ, ge_faml_sched** out) {
  return ge::guarded([&] {
    GE_REQUIRE(out && h_pt_ip && m >= 0, "null argument");
    GE_REQUIRE(dim >= 1 && dim <= ge::kMaxDim, "dimension must be 1..16");
    GE_REQUIRE(n_aggs >= 0 && (h_aggs || n_aggs == 0) && n_split >= 0 && (h_split || n_split == 0),
               "bad aggregate lists");
    GE_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks && cus >= 1, "bad rank / size");
    std::vector<int> aggs, split;
    check_ids(h_aggs, n_aggs, m, "aggregate ids must be strictly increasing and < m", aggs);
    check_ids(h_split, n_split, m, "split aggregate ids must be strictly increasing and < m",
              split);
    auto* h = new ge_faml_sched();
    std::unique_ptr<ge_faml_sched> hold(h);
    h->s = ge::faml_schedule(ge::faml_sched_in(h_pt_ip, aggs, split, rank, nranks, dim,
                                               mode, cus, sym_occ));
    const ge::FamlSched& s = h->s;
    h->scalars = {s.res_cap, s.census[0], s.census[1], s.census[2], s.census[3],
                  (int)s.off_m, (int)s.off_l, s.ns, s.nm, s.nl,
                  s.R, s.U, s.code, (int)s.fast, (int)s.sym,
                  (int)s.wide, s.ntiles, s.swept, s.rows_mode, s.sym_blocks};
    *out = hold.release();
  });
}

int ge_faml_sched_table(const ge_faml_sched* h, int k, const int** data, long long* len) {
  return ge::guarded([&] {
    GE_REQUIRE(h && data && len, "null argument");
    const ge::FamlSched& s = h->s;
    auto put = [&](const void* p, size_t ints) {
      *data = (const int*)p;
      *len = (long long)ints;
    };
    switch (k) {
      case GE_FAML_SCHED_ORDER: put(s.order.data(), s.order.size()); break;
      case GE_FAML_SCHED_BEG: put(s.beg.data(), s.beg.size()); break;
      case GE_FAML_SCHED_ROWS: put(s.rows.data(), s.rows.size()); break;
      case GE_FAML_SCHED_IROWS: put(s.irows.data(), s.irows.size()); break;
      case GE_FAML_SCHED_HUGE: put(s.huge.data(), s.huge.size()); break;
      case GE_FAML_SCHED_XROWS: put(s.xr.data(), s.xr.size()); break;
      case GE_FAML_SCHED_XCOUNTS: put(s.xcounts.data(), s.xcounts.size()); break;
      case GE_FAML_SCHED_ITEMS: put(s.items.data(), 2 * s.items.size()); break;
      case GE_FAML_SCHED_FITEMS: put(s.fitems.data(), 4 * s.fitems.size()); break;
      case GE_FAML_SCHED_UNITS: put(s.units.data(), 4 * s.units.size()); break;
      case GE_FAML_SCHED_SCALARS: put(h->scalars.data(), h->scalars.size()); break;
      case GE_FAML_SCHED_FARAGGS: put(s.faraggs.data(), s.faraggs.size()); break;
      default: throw ge::Error(GE_ERR_ARG, "unknown schedule table");
    }
  });
}

int ge_faml_sched_pairs(const ge_faml_sched* h, double* streamed_pairs) {
  return ge::guarded([&] {
    GE_REQUIRE(h && streamed_pairs, "null argument");
    *streamed_pairs = h->s.streamed_pairs;
  });
}

int ge_faml_sched_destroy(ge_faml_sched* h) {
  return ge::guarded([&] { delete h; });
}

}  // extern "C"


// ge_minimize_dev.hip -- one level of anyToMultilevel(embedViaMinimization)
// (src/embed.cpp:23-83 over :341-559) as one batched device call.
//
// A single embedViaMinimization call is a chain of ordered sums and stays on the
// host (ge_minimize.cpp).  A level is m independent calls, each vertex of which
// runs 2d independent line searches, every term of whose sums is independent; only
// the adds are ordered.  Two kernels by aggregate size r:
//   packed (r <= GE_MIN_PACK_MAX): one lane per (aggregate, direction); the lane
//     runs its whole line search serially, so its sums are in the reference's order
//     by construction.  The 2d lanes of an aggregate sit in one group of a wave,
//     exchange (J, t) by shuffle after each vertex and lane 0 of the group applies
//     the update to the aggregate's coordinates in LDS.  Aggregates are sorted by r
//     so that the groups of a wave share trip counts.
//   wave per direction (r up to what the LDS holds): one block per aggregate, its
//     coordinates in LDS, one wave per direction (the waves loop when the block has
//     fewer than 2d).  The lanes evaluate a 64-term chunk in parallel; the chunk is
//     then added onto the running sum lane by lane (v_readlane chain), never as a
//     tree.  One barrier per vertex: the waves publish (t, J) into a parity slot,
//     meet, and every wave applies the same update.
//   Aggregates whose coordinates exceed the LDS run on the host code inside the
//   same call, overlapped with the kernels.
// Every term keeps the operand grouping of ge_minimize.cpp: line_search; `/` and
// sqrt() are the correctly rounded ones (-ffp-contract=off -fno-fast-math).

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ge_internal.hpp"

namespace ge {

namespace {

constexpr double kMinEps = 10e-12;          // src/embed.cpp:345 (sic: 1e-11)
constexpr double kEdgeWeight = 1000000.0;   // :415
constexpr int kPackCap = 64;                // the largest packed threshold
constexpr int kPackDefault = 16;            // the sweep on config 1
constexpr int kResDoubles = 32;             // (t, J) of 2 parities x 8 directions

struct LineRes {
  double t, J;
};

// +e_k for direction 2k, -e_k for 2k + 1 (:363-379)
__device__ inline double dir_component(int s, int k) {
  return (s >> 1) == k ? ((s & 1) ? -1.0 : 1.0) : 0.0;
}

// ---------------------------------------------------------------------------
// the terms, shared by both kernels (ge_minimize.cpp: line_search)

template <int DIM>
__device__ inline double djump_pair(const double* xr, const double* xi, const double* u, double t) {
  double term1 = 0.0, term2 = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double v = xi[k] - xr[k];
    const double z = u[k] * t + v;
    term1 = term1 + z * z;
    term2 = term2 + z * u[k];
  }
  if (term1 < kMinEps) term1 = kMinEps;
  return -((1.0 / sqrt(term1 * term1 * term1)) * term2);
}

template <int DIM>
__device__ inline double djump_edge(const double* xr, const double* xi, const double* xs,
                                    double t) {
  double term = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double a = (1 - t) * xi[k] + t * xs[k] - xr[k];
    term += kEdgeWeight * 2.0 * a * (xs[k] - xi[k]);
  }
  return term;
}

template <int DIM>
__device__ inline double energy_pair(const double* xr, const double* xi, const double* u,
                                     double t) {
  double term1 = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double v = xi[k] - xr[k];
    const double z = u[k] * t + v;
    term1 = term1 + z * z;
  }
  if (term1 < kMinEps) term1 = kMinEps;
  return 1.0 / sqrt(term1);
}

template <int DIM>
__device__ inline double energy_edge(const double* xr, const double* xi, const double* xs,
                                     double t) {
  double term = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double a = (1 - t) * xi[k] + t * xs[k] - xr[k];
    term += a * a;
  }
  return kEdgeWeight * term;
}

// Centring and scaling over vertices 1..n-1 (:528-557, sic), then anyToMultilevel's
// normalisation by the largest norm and the placement in the ball (:67-79).  One lane.
template <int DIM>
__device__ void finalize(double* X, int n, const int* v, const double* ca, double ra,
                         double* out) {
  if (n > 1) {
    double avg[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) avg[k] = 0.0;
    for (int i = 1; i < n; ++i)
#pragma unroll
      for (int k = 0; k < DIM; ++k) avg[k] = avg[k] + X[i * DIM + k];
#pragma unroll
    for (int k = 0; k < DIM; ++k) avg[k] = avg[k] / (n - 1);
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int k = 0; k < DIM; ++k) X[i * DIM + k] -= avg[k];
    double max_length = 0.0;
    for (int i = 1; i < n; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) acc = acc + X[i * DIM + k] * X[i * DIM + k];
      const double len = sqrt(acc);
      if (max_length < len) max_length = len;
    }
    for (int i = 0; i < n * DIM; ++i) X[i] = X[i] / max_length;
  }
  double mx = 0.0;
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) acc += X[i * DIM + k] * X[i * DIM + k];
    const double mg = sqrt(acc);
    if (mg > mx) mx = mg;
  }
  for (int i = 0; i < n; ++i)
#pragma unroll
    for (int k = 0; k < DIM; ++k)
      out[(size_t)v[i] * DIM + k] = ca[k] + ra * (X[i * DIM + k] / mx);
}

// ---------------------------------------------------------------------------
// packed: one lane per (aggregate, direction)

template <int DIM>
__device__ LineRes line_search_lane(const double* X, int i, int n, const int* nb, int cnt,
                                    int s) {
  double xi[DIM], xs[DIM], u[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    xi[k] = X[i * DIM + k];
    xs[k] = dir_component(s, k);
    u[k] = xs[k] - xi[k];
  }
  double t = 0.5;
  double jump = 0.25;
  do {
    double dJ = 0.0;
    for (int r = 0; r < n; ++r) {
      if (i == r) continue;
      dJ += djump_pair<DIM>(X + r * DIM, xi, u, t);
    }
    for (int q = 0; q < cnt; ++q) dJ += djump_edge<DIM>(X + nb[q] * DIM, xi, xs, t);
    if (dJ < 0.0) t = t + jump;
    else t = t - jump;
    jump = jump / 2.0;
  } while (jump > 1.e-4);
  double Jl = 0.0;
  for (int r = 0; r < n; ++r) {
    if (i == r) continue;
    Jl = Jl + energy_pair<DIM>(X + r * DIM, xi, u, t);
  }
  for (int q = 0; q < cnt; ++q) Jl += energy_edge<DIM>(X + nb[q] * DIM, xi, xs, t);
  return {t, Jl};
}

template <int DIM>
struct Pack {
  static constexpr int G = DIM == 1 ? 2 : DIM == 2 ? 4 : 8;  // lanes of one aggregate
  static constexpr int NG = 64 / G;                          // aggregates of one wave
};

// aggs[0..naggs): the packed aggregates by descending r; block b takes NG of them.
// LDS: NG x stride x DIM coordinates.
template <int DIM>
__global__ __launch_bounds__(64) void min_packed(int naggs, const int* __restrict__ aggs,
                                                 const int* __restrict__ pt_ip,
                                                 const int* __restrict__ pt_ix,
                                                 const int* __restrict__ rowoff,
                                                 const int* __restrict__ cnt,
                                                 const int* __restrict__ nb,
                                                 const double* __restrict__ cA,
                                                 const double* __restrict__ rA, int iterations,
                                                 int stride, double* __restrict__ out) {
  constexpr int G = Pack<DIM>::G, NG = Pack<DIM>::NG;
  extern __shared__ double smem[];
  const int lane = threadIdx.x;
  const int grp = lane / G, s = lane % G;
  const int q = blockIdx.x * NG + grp;
  const bool valid = q < naggs;
  const int a = valid ? aggs[q] : 0;
  const int base = valid ? pt_ip[a] : 0;
  const int r = valid ? pt_ip[a + 1] - base : 0;
  const int a0 = aggs[blockIdx.x * NG];  // the block's largest
  const int rmax = pt_ip[a0 + 1] - pt_ip[a0];
  double* X = smem + (size_t)grp * stride * DIM;
  if (s == 0)
    for (int j = 0; j < r * DIM; ++j) X[j] = 0.0;
  __syncthreads();
  for (int iter = 0; iter < iterations; ++iter) {
    for (int i = 0; i < rmax; ++i) {
      const int c = i < r ? cnt[base + i] : 0;  // :389-394: no neighbour but itself, skipped
      LineRes lr = {0.0, std::numeric_limits<double>::infinity()};
      if (c > 0 && s < 2 * DIM) lr = line_search_lane<DIM>(X, i, r, nb + rowoff[base + i], c, s);
      double min_J = std::numeric_limits<double>::infinity();
      double min_t = 0.0;
      int min_s = -1;
#pragma unroll
      for (int s2 = 0; s2 < 2 * DIM; ++s2) {  // :524-528, in direction order
        const double J2 = __shfl(lr.J, grp * G + s2);
        const double t2 = __shfl(lr.t, grp * G + s2);
        if (J2 < min_J) {
          min_J = J2;
          min_t = t2;
          min_s = s2;
        }
      }
      if (c > 0 && s == 0 && min_s >= 0) {
#pragma unroll
        for (int k = 0; k < DIM; ++k)
          X[i * DIM + k] = X[i * DIM + k] * (1 - min_t) + dir_component(min_s, k) * min_t;
      }
      __syncthreads();
    }
  }
  if (valid && s == 0) finalize<DIM>(X, r, pt_ix + base, cA + (size_t)a * DIM, rA[a], out);
}

// ---------------------------------------------------------------------------
// wave per direction

__device__ inline double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

// sum + term[0] + term[1] + ... + term[count-1], the adds in lane order
__device__ inline double ordered_add(double sum, double term, int count) {
  if (count == 64) {
#pragma unroll
    for (int l = 0; l < 64; ++l) sum = sum + lane_value(term, l);
  } else {
    for (int l = 0; l < count; ++l) sum = sum + lane_value(term, l);
  }
  return sum;
}

// The line search of vertex i towards direction s by one wave.  The n - 1 other
// members are numbered 0..n-2 in ascending order with i left out, so a chunk never
// holds a skipped term.
template <int DIM>
__device__ LineRes line_search_wave(const double* X, const double* xi, int i, int n,
                                    const int* nb, int cnt, int s, int lane) {
  double xs[DIM], u[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    xs[k] = dir_component(s, k);
    u[k] = xs[k] - xi[k];
  }
  const int others = n - 1;
  double t = 0.5;
  double jump = 0.25;
  do {
    double dJ = 0.0;
    for (int b = 0; b < others; b += 64) {
      const int q = b + lane;
      double term = 0.0;
      if (q < others) term = djump_pair<DIM>(X + (q + (q >= i)) * DIM, xi, u, t);
      dJ = ordered_add(dJ, term, min(64, others - b));
    }
    for (int b = 0; b < cnt; b += 64) {
      const int q = b + lane;
      double term = 0.0;
      if (q < cnt) term = djump_edge<DIM>(X + nb[q] * DIM, xi, xs, t);
      dJ = ordered_add(dJ, term, min(64, cnt - b));
    }
    if (dJ < 0.0) t = t + jump;
    else t = t - jump;
    jump = jump / 2.0;
  } while (jump > 1.e-4);
  double Jl = 0.0;
  for (int b = 0; b < others; b += 64) {
    const int q = b + lane;
    double term = 0.0;
    if (q < others) term = energy_pair<DIM>(X + (q + (q >= i)) * DIM, xi, u, t);
    Jl = ordered_add(Jl, term, min(64, others - b));
  }
  for (int b = 0; b < cnt; b += 64) {
    const int q = b + lane;
    double term = 0.0;
    if (q < cnt) term = energy_edge<DIM>(X + nb[q] * DIM, xi, xs, t);
    Jl = ordered_add(Jl, term, min(64, cnt - b));
  }
  return {t, Jl};
}

// aggs[0..gridDim.x): the aggregates of this class by descending r, one per block.
// LDS: kResDoubles for the (t, J) slots, then r x DIM coordinates.
template <int DIM>
__global__ void min_wave(const int* __restrict__ aggs, const int* __restrict__ pt_ip,
                         const int* __restrict__ pt_ix, const int* __restrict__ rowoff,
                         const int* __restrict__ cnt, const int* __restrict__ nb,
                         const double* __restrict__ cA, const double* __restrict__ rA,
                         int iterations, double* __restrict__ out) {
  extern __shared__ double smem[];
  double* res = smem;
  double* X = smem + kResDoubles;
  const int a = aggs[blockIdx.x];
  const int base = pt_ip[a];
  const int r = pt_ip[a + 1] - base;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = blockDim.x >> 6;
  for (int j = tid; j < r * DIM; j += blockDim.x) X[j] = 0.0;
  __syncthreads();
  int par = 0;
  for (int iter = 0; iter < iterations; ++iter) {
    for (int i = 0; i < r; ++i) {
      const int c = cnt[base + i];
      if (c == 0) continue;  // uniform over the block
      // X[i] is read before the barrier: a wave that is ahead rewrites it after it
      double xi[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) xi[k] = X[i * DIM + k];
      const int* nbi = nb + rowoff[base + i];
      for (int s = w; s < 2 * DIM; s += W) {
        const LineRes lr = line_search_wave<DIM>(X, xi, i, r, nbi, c, s, lane);
        if (lane == 0) {
          res[(par * 2 * DIM + s) * 2] = lr.t;
          res[(par * 2 * DIM + s) * 2 + 1] = lr.J;
        }
      }
      __syncthreads();
      double min_J = std::numeric_limits<double>::infinity();
      double min_t = 0.0;
      int min_s = -1;
      for (int s = 0; s < 2 * DIM; ++s) {  // :524-528, in direction order
        const double t2 = res[(par * 2 * DIM + s) * 2];
        const double J2 = res[(par * 2 * DIM + s) * 2 + 1];
        if (J2 < min_J) {
          min_J = J2;
          min_t = t2;
          min_s = s;
        }
      }
      // every wave stores the same value, so each may go on without a second barrier:
      // its own store is ordered before its next reads, another wave's changes nothing.
      // The slot of this parity is written again only two vertices on, past the next
      // barrier, which no wave reaches before all have read it.
      if (min_s >= 0) {
#pragma unroll
        for (int k = 0; k < DIM; ++k)
          if (lane == k) X[i * DIM + k] = xi[k] * (1 - min_t) + dir_component(min_s, k) * min_t;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      par ^= 1;
    }
  }
  __syncthreads();
  if (tid == 0) finalize<DIM>(X, r, pt_ix + base, cA + (size_t)a * DIM, rA[a], out);
}

// Per P_T slot (member g of aggregate a): the local indices of g's internal
// neighbours -- entries j of g's row with vertex_A[j] == a and j != g -- in stored
// order, written over the row's own span of nb; their count; the span's start.
__global__ void min_prep(int n, const int* __restrict__ ip, const int* __restrict__ ix,
                         const int* __restrict__ pt_ix, const int* __restrict__ vA,
                         const int* __restrict__ local_of, int* __restrict__ rowoff,
                         int* __restrict__ cnt, int* __restrict__ nb) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n) return;
  const int g = pt_ix[slot];
  const int a = vA[g];
  const int off = ip[g];
  int c = 0;
  for (int kk = off; kk < ip[g + 1]; ++kk) {
    const int j = ix[kk];
    if (vA[j] == a && j != g) nb[off + c++] = local_of[j];
  }
  rowoff[slot] = off;
  cnt[slot] = c;
}

int env_int(const char* name, int fallback) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : fallback;
}

template <int DIM>
void launch_level(hipStream_t main, hipStream_t side, int npk, const int* d_pk, int nwv,
                  const int* d_wv, int pack_max, int waves, size_t wave_lds, const int* pt_ip,
                  const int* pt_ix, const int* rowoff, const int* cnt, const int* nb,
                  const double* cA, const double* rA, int iterations, double* out) {
  if (nwv > 0) {  // the giants first
    GE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&min_wave<DIM>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)wave_lds));
    hipLaunchKernelGGL(min_wave<DIM>, dim3(nwv), dim3(64 * waves), wave_lds, main, d_wv, pt_ip,
                       pt_ix, rowoff, cnt, nb, cA, rA, iterations, out);
    GE_HIP(hipGetLastError());
  }
  if (npk > 0) {
    constexpr int NG = Pack<DIM>::NG;
    const size_t lds = (size_t)NG * pack_max * DIM * sizeof(double);
    hipLaunchKernelGGL(min_packed<DIM>, dim3((npk + NG - 1) / NG), dim3(64), lds, side, npk,
                       d_pk, pt_ip, pt_ix, rowoff, cnt, nb, cA, rA, iterations, pack_max, out);
    GE_HIP(hipGetLastError());
  }
}

struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t ready = nullptr, done = nullptr;
  SideStream() {
    GE_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    GE_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    GE_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
  }
  ~SideStream() {
    if (ready) (void)hipEventDestroy(ready);
    if (done) (void)hipEventDestroy(done);
    if (s) (void)hipStreamDestroy(s);
  }
};

void minimize_ml_device(ge_ctx* ctx, int n, const int* I, const int* J, int m, const int* PI,
                        const int* PJ, const int* vA, const int* local_of, const double* cA,
                        const double* rA, int dim, int iterations, double* coords,
                        int* classes) {
  DeviceGuard guard(ctx);
  int lds_cap = 0;
  GE_HIP(hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  lds_cap = std::min(lds_cap, env_int("GE_MIN_LDS_BYTES", lds_cap));
  const int pack_max = std::clamp(env_int("GE_MIN_PACK_MAX", kPackDefault), 0, kPackCap);
  // dim 1..3: a wave per direction; dim 4: 4 waves, two directions each
  const int waves = std::clamp(env_int("GE_MIN_WAVES", dim <= 3 ? 2 * dim : 4), 1, 2 * dim);

  std::vector<int> pk, wv, host;
  size_t wave_lds = 0;
  for (int a = 0; a < m; ++a) {
    const int r = PI[a + 1] - PI[a];
    const size_t need = ((size_t)kResDoubles + (size_t)r * dim) * sizeof(double);
    if (r <= pack_max) {
      pk.push_back(a);
    } else if (need <= (size_t)lds_cap) {
      wv.push_back(a);
      wave_lds = std::max(wave_lds, need);
    } else {
      host.push_back(a);
    }
  }
  // descending cost r^2 (ties: lower id): a giant starts first, and the groups of a
  // packed wave share trip counts
  auto by_size = [&](int a, int b) { return PI[a + 1] - PI[a] > PI[b + 1] - PI[b]; };
  std::stable_sort(pk.begin(), pk.end(), by_size);
  std::stable_sort(wv.begin(), wv.end(), by_size);
  if (classes) {
    classes[0] = (int)pk.size();
    classes[1] = (int)wv.size();
    classes[2] = (int)host.size();
    classes[3] = 1;
  }

  hipStream_t st = ctx->stream;
  const int nnz = I[n];
  DevBuf<int> d_ip(n + 1), d_ix(std::max(nnz, 1)), d_pip(m + 1), d_pix(n), d_vA(n), d_loc(n),
      d_rowoff(n), d_cnt(n), d_nb(std::max(nnz, 1)), d_pk(std::max<size_t>(pk.size(), 1)),
      d_wv(std::max<size_t>(wv.size(), 1));
  DevBuf<double> d_cA((size_t)m * dim), d_rA(m), d_out((size_t)n * dim);
  d_ip.upload(I, n + 1, st);
  d_ix.upload(J, nnz, st);
  d_pip.upload(PI, m + 1, st);
  d_pix.upload(PJ, n, st);
  d_vA.upload(vA, n, st);
  d_loc.upload(local_of, n, st);
  d_pk.upload(pk.data(), pk.size(), st);
  d_wv.upload(wv.data(), wv.size(), st);
  d_cA.upload(cA, (size_t)m * dim, st);
  d_rA.upload(rA, m, st);
  GE_HIP(hipMemsetAsync(d_out.p, 0, (size_t)n * dim * sizeof(double), st));
  hipLaunchKernelGGL(min_prep, dim3((n + 255) / 256), dim3(256), 0, st, n, d_ip.p, d_ix.p,
                     d_pix.p, d_vA.p, d_loc.p, d_rowoff.p, d_cnt.p, d_nb.p);
  GE_HIP(hipGetLastError());
  // the packed kernel on a stream of its own, so that it runs beside the wave kernel
  SideStream side;
  GE_HIP(hipEventRecord(side.ready, st));
  GE_HIP(hipStreamWaitEvent(side.s, side.ready, 0));
  const int npk = (int)pk.size(), nwv = (int)wv.size();
  auto go = [&](auto tag) {
    launch_level<decltype(tag)::value>(st, side.s, npk, d_pk.p, nwv, d_wv.p, pack_max, waves,
                                       wave_lds, d_pip.p, d_pix.p, d_rowoff.p, d_cnt.p, d_nb.p,
                                       d_cA.p, d_rA.p, iterations, d_out.p);
  };
  try {
    switch (dim) {
      case 1: go(std::integral_constant<int, 1>{}); break;
      case 2: go(std::integral_constant<int, 2>{}); break;
      case 3: go(std::integral_constant<int, 3>{}); break;
      default: go(std::integral_constant<int, 4>{}); break;
    }
    GE_HIP(hipEventRecord(side.done, side.s));
    GE_HIP(hipStreamWaitEvent(st, side.done, 0));
  } catch (...) {
    (void)hipStreamSynchronize(side.s);  // nothing of this call may outlive its buffers
    (void)hipStreamSynchronize(st);
    throw;
  }
  // the aggregates beyond the LDS, on the host while the kernels run
  std::vector<double> hx;
  if (!host.empty()) {
    hx.assign((size_t)n * dim, 0.0);
    try {
      minimize_ml_host(I, J, PI, PJ, vA, local_of, cA, rA, dim, iterations, hx.data(),
                       host.data(), (int)host.size());
    } catch (...) {
      (void)hipStreamSynchronize(st);
      throw;
    }
  }
  d_out.download(coords, (size_t)n * dim, st);
  const hipError_t e = hipStreamSynchronize(st);
  (void)hipStreamSynchronize(side.s);
  GE_HIP(e);
  for (int a : host)
    for (int c = PI[a]; c < PI[a + 1]; ++c)
      for (int k = 0; k < dim; ++k)
        coords[(size_t)PJ[c] * dim + k] = hx[(size_t)PJ[c] * dim + k];
}

}  // namespace

}  // namespace ge

extern "C" int ge_embed_via_minimization_ml(ge_ctx* ctx, int n, const int* indptr,
                                            const int* indices, int m, const int* pt_indptr,
                                            const int* pt_indices, const int* vertex_A,
                                            const double* coords_A, const double* r_A, int dim,
                                            int iterations, double* coords, int* classes) {
  return ge::guarded([&] {
    GE_REQUIRE(n >= 0 && m >= 0 && dim >= 1 && iterations >= 0, "bad arguments");
    if (classes) classes[0] = classes[1] = classes[2] = classes[3] = 0;
    GE_REQUIRE(pt_indptr && pt_indptr[0] == 0, "null or bad P_T indptr");
    for (int a = 0; a < m; ++a)
      GE_REQUIRE(pt_indptr[a + 1] >= pt_indptr[a], "P_T indptr decreases");
    GE_REQUIRE(pt_indptr[m] == n, "P_T must have one entry per fine vertex");
    if (n == 0) return;
    GE_REQUIRE(indptr && indices && pt_indices && vertex_A && coords_A && r_A && coords,
               "null argument");
    GE_REQUIRE(indptr[0] == 0, "bad indptr");
    bool ascending = true;  // the device path reads rows in stored order (see below)
    for (int i = 0; i < n; ++i) {
      GE_REQUIRE(indptr[i + 1] >= indptr[i], "indptr decreases");
      for (int kk = indptr[i]; kk < indptr[i + 1]; ++kk) {
        GE_REQUIRE((unsigned)indices[kk] < (unsigned)n, "column index out of range");
        if (kk > indptr[i] && indices[kk] <= indices[kk - 1]) ascending = false;
      }
    }
    // P_T is a partition of the fine vertices and vertex_A is its inverse
    std::vector<int> local_of(n, -1);
    for (int a = 0; a < m; ++a)
      for (int c = pt_indptr[a]; c < pt_indptr[a + 1]; ++c) {
        const int g = pt_indices[c];
        GE_REQUIRE((unsigned)g < (unsigned)n && local_of[g] < 0,
                   "P_T must list every fine vertex once");
        GE_REQUIRE(vertex_A[g] == a, "vertex_A does not match P_T");
        local_of[g] = c - pt_indptr[a];
        if (c > pt_indptr[a] && g <= pt_indices[c - 1]) ascending = false;
      }
    // The reference sorts each sub-matrix row by local index and merges duplicates
    // (CooMatrix::ToSparse).  With strictly ascending rows of A and of P_T that is the
    // stored order, which the kernels read; any other input takes the host path.
    const char* force = std::getenv("GE_MINIMIZE_HOST");
    const bool host = !ctx || (force && *force && *force != '0') || !ascending || dim > 4;
    if (host) {
      ge::minimize_ml_host(indptr, indices, pt_indptr, pt_indices, vertex_A, local_of.data(),
                           coords_A, r_A, dim, iterations, coords, nullptr, m);
      if (classes) classes[2] = m;
      return;
    }
    ge::minimize_ml_device(ctx, n, indptr, indices, m, pt_indptr, pt_indices, vertex_A,
                           local_of.data(), coords_A, r_A, dim, iterations, coords, classes);
  });
}

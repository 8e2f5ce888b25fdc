// ge_fa_batch.hip -- many independent small graphs' single-level ForceAtlas in one call
// (ge_force_atlas_batch, include/ge.h).
//
// The graphs arrive as one block-diagonal CSR: graph g owns rows and columns
// [off[g], off[g+1]).  Every graph's iteration is fa_small_strict's general form
// (ge_fa.hip): the level's records {x, deg + 1} resident in LDS, a row's terms evaluated
// by the G lanes that share the row and added in order by the group's first lane
// (group_add, which here stops reading a chunk's slots past its last term), the
// in-domain bodies when every row of the graph lies in the exact-division domain and
// the `/` bodies otherwise.  A row's sum is therefore the
// reference's serial sum, whatever G is, and a graph reads nothing of another graph: each
// keeps the bits of ge_force_atlas on it alone.  The host schedule (fa_batch_schedule,
// ge_fa_sched.hpp) puts a graph in one of three classes:
//   wave    fa_batch_wave: one wave per graph, kBatchWaves graphs per workgroup.  A wave
//           has its own LDS slice (records, then the term buffer), synchronises with
//           wave_lds_sync() only and takes the domain test as a wave vote: no
//           __syncthreads, no wave waits on another.
//   block   fa_batch_block: one workgroup per graph.
//   serial  fa_run_device, one graph after another, after the two launches are enqueued.
// Both kernels are plain launches: no cooperative launch, no grid barrier, no atomics.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ge_fa_sched.hpp"
#include "ge_group.hpp"
#include "ge_internal.hpp"
#include "ge_pair.hpp"

namespace ge {
namespace {

// How the lanes that hold one graph synchronise and vote.
struct WaveScope {
  static __device__ __forceinline__ void sync() { wave_lds_sync(); }
  static __device__ __forceinline__ bool all(bool p) {
    return __builtin_amdgcn_ballot_w64(!p) == 0;
  }
};
struct BlockScope {
  static __device__ __forceinline__ void sync() { __syncthreads(); }
  static __device__ __forceinline__ bool all(bool p) { return __syncthreads_and(p); }
};

// LDS doubles of one wave of fa_batch_wave: kBatchWaveMax records, then the term buffer
// of 64 lanes x D.  Bytes per wave: 3.5 K at D = 3, 6 K at D = 4, 17 K at D = 16.
constexpr int batch_wave_slice(int D) { return kBatchWaveMax * rec_width(D) + 64 * D; }
// Threads of fa_batch_block: fa_small_strict's general kernel's per dimension.  (A
// narrow dimension on the wide schedule, GE_WIDE_MIN_DIM, gets its lanes per row for
// kSmallWideT threads and runs them in this larger block.)
constexpr int batch_block_threads(int D) { return D <= kNarrowMaxDim ? kSmallGenT : kSmallWideT; }

// All iterations of one graph of n rows by `tid` of the scope's lanes (n G of them at
// least).  ip, dp1, X: the graph's first row; ix, dx: the concatenated entries, columns
// less r0; sx: n records; tb: the term buffer (one slot of D doubles per lane).
// fa_small_strict<D, G, T, false, false> with the previous forces starting at zero.
template <int D, int G, class S>
__device__ __forceinline__ void batch_graph(int n, int tid, int lanes, int r0,
                                            const int* __restrict__ ip,
                                            const int* __restrict__ ix,
                                            const double* __restrict__ dx,
                                            const double* __restrict__ dp1,
                                            double* __restrict__ X, double* sx, double* tb,
                                            int iterations, const FaConst& c) {
  constexpr int W = rec_width(D);
  const int g = tid % G;
  const int i = tid / G;
  const bool active = i < n;
  const bool leader = active && g == 0;
  for (int q = tid; q < n; q += lanes) {
#pragma unroll
    for (int k = 0; k < D; ++k) sx[q * W + k] = X[(size_t)q * D + k];
    sx[q * W + D] = dp1[q];
  }
  const int e0 = active ? ip[i] : 0;
  const int e1 = active ? ip[i + 1] : 0;
  double fprev[D], F[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    fprev[k] = 0.0;
    F[k] = 0.0;
  }
  for (int it = 0; it < iterations; ++it) {
    S::sync();
    double xi[D], acc[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[k] = active ? sx[i * W + k] : 0.0;
      acc[k] = 0.0;
    }
    const double dip1 = active ? sx[i * W + D] : 1.0;
    const bool row_ok = all_coord_ok<D>(xi);
    const bool rep_ok = row_ok && weight_ok(dip1) && weight_ok(c.repel);
    // every row of this graph in the shared-reciprocal domain: the branch-free bodies
    const bool dom = S::all(!active || rep_ok);
    if (dom) {
      for (int j0 = 0; j0 < n; j0 += G) {  // :151-167, j ascending
        double t[1][D];
        const int j = j0 + g;
        const int jj = min(j, n - 1);
        rep_term<D, true, false>(xi, &sx[jj * W], dip1, sx[jj * W + D], c.repel, t[0]);
        if (j >= n)
#pragma unroll
          for (int k = 0; k < D; ++k) t[0][k] = 0.0;
        group_add<D, G, 1, true>(t, tid, g, min(G, n - j0), leader, tb, acc);
      }
      for (int b = e0; b < e1; b += G) {  // :169-203, CSR order
        double t[1][D];
        const int e = b + g;
        const int ee = min(e, e1 - 1);
#pragma unroll
        for (int k = 0; k < D; ++k) t[0][k] = 0.0;
        attr_edge<D, true, false>(xi, &sx[(ix[ee] - r0) * W], c.use_weights ? dx[ee] : 1.0, dip1,
                                  c, t[0]);
        if (e >= e1)
#pragma unroll
          for (int k = 0; k < D; ++k) t[0][k] = 0.0;
        group_add<D, G, 1, true>(t, tid, g, min(G, e1 - b), leader, tb, acc);
      }
    } else {
      for (int j0 = 0; j0 < n; j0 += G) {  // :151-167, j ascending
        double t[1][D];
        const int j = j0 + g;
#pragma unroll
        for (int k = 0; k < D; ++k) t[0][k] = 0.0;
        if (active && j < n) {
          const double* xj = &sx[j * W];
          if (rep_ok && vertex_ok<D>(xj, sx[j * W + D]))
            rep_pair<D, true, false>(xi, xj, dip1, sx[j * W + D], c.repel, t[0]);
          else
            rep_pair_fb<D, false>(xi, xj, dip1, sx[j * W + D], c.repel, j == i, t[0]);
        }
        group_add<D, G, 1, true>(t, tid, g, min(G, n - j0), leader, tb, acc);
      }
      for (int b = e0; b < e1; b += G) {  // :169-203, CSR order
        double t[1][D];
        const int e = b + g;
#pragma unroll
        for (int k = 0; k < D; ++k) t[0][k] = 0.0;
        if (e < e1) {
          const double* xj = &sx[(ix[e] - r0) * W];
          const double a = c.use_weights ? dx[e] : 1.0;
          if (row_ok && all_coord_ok<D>(xj))
            attr_edge<D, true>(xi, xj, a, dip1, c, t[0]);
          else
            attr_edge<D, false>(xi, xj, a, dip1, c, t[0]);
        }
        group_add<D, G, 1, true>(t, tid, g, min(G, e1 - b), leader, tb, acc);
      }
    }
    if (leader) {  // gravity :205-211 (mag not clamped)
      double m2 = xi[0] * xi[0];
#pragma unroll
      for (int k = 1; k < D; ++k) m2 = m2 + xi[k] * xi[k];
      const double mag = sqrt(m2);
      double unit[D];
      neg_over<D>(xi, mag, unit);
#pragma unroll
      for (int k = 0; k < D; ++k) F[k] = acc[k] + unit[k] * c.gravity * dip1;
    }
    S::sync();
    if (leader) {  // swing + update :214-269
      double s2 = 0.0, f2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double t = fprev[k] - F[k];
        s2 = (k == 0) ? t * t : s2 + t * t;
        f2 = (k == 0) ? F[k] * F[k] : f2 + F[k] * F[k];
      }
      const double swing = sqrt(s2);
      const double totalF = sqrt(f2);
      double speed = c.ks_gS / (1 + c.gS * sqrt(swing));
      const double cap = c.ksmax / totalF;
      if (speed > cap) speed = cap;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        sx[i * W + k] = F[k] * speed + sx[i * W + k];
        fprev[k] = F[k];
      }
    }
  }
  S::sync();
  for (int q = tid; q < n; q += lanes)
#pragma unroll
    for (int k = 0; k < D; ++k) X[(size_t)q * D + k] = sx[q * W + k];
}

// items: {graph, lanes per row} in launch order.  Wave w of a workgroup takes item
// blockIdx.x kBatchWaves + w and picks its lanes-per-row body by a wave-uniform switch.
template <int D>
__global__ void __launch_bounds__(64 * kBatchWaves)
fa_batch_wave(int nitems, const int2* __restrict__ items, const int* __restrict__ off,
              const int* __restrict__ ip, const int* __restrict__ ix,
              const double* __restrict__ dx, const double* __restrict__ dp1,
              double* __restrict__ X, int iterations, FaConst c) {
  constexpr int kSlice = batch_wave_slice(D);
  __shared__ __attribute__((aligned(16))) double lds[kBatchWaves * kSlice];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = threadIdx.x % 64;
  const int item = blockIdx.x * kBatchWaves + wave;
  if (item >= nitems) return;  // the whole wave
  const int gi = __builtin_amdgcn_readfirstlane(items[item].x);
  const int G = __builtin_amdgcn_readfirstlane(items[item].y);
  const int r0 = __builtin_amdgcn_readfirstlane(off[gi]);
  const int n = __builtin_amdgcn_readfirstlane(off[gi + 1]) - r0;
  if (n < 1 || n > kBatchWaveMax || n * G > 64) return;  // not this class (the host checks)
  double* sx = lds + wave * kSlice;
  double* tb = sx + kBatchWaveMax * rec_width(D);
#define GE_BATCH_WAVE_CASE(GG)                                                              \
  case GG:                                                                                  \
    batch_graph<D, GG, WaveScope>(n, lane, 64, r0, ip + r0, ix, dx, dp1 + r0,               \
                                  X + (size_t)r0 * D, sx, tb, iterations, c);               \
    break;
  switch (G) {
    GE_BATCH_WAVE_CASE(1) GE_BATCH_WAVE_CASE(2) GE_BATCH_WAVE_CASE(4) GE_BATCH_WAVE_CASE(8)
    GE_BATCH_WAVE_CASE(16) GE_BATCH_WAVE_CASE(32) GE_BATCH_WAVE_CASE(64)
    default: break;
  }
#undef GE_BATCH_WAVE_CASE
}

// Workgroup b takes item b: fa_small_strict's general form with the graph taken from
// blockIdx.x.
template <int D>
__global__ void __launch_bounds__(batch_block_threads(D))
fa_batch_block(const int2* __restrict__ items, const int* __restrict__ off,
               const int* __restrict__ ip, const int* __restrict__ ix,
               const double* __restrict__ dx, const double* __restrict__ dp1,
               double* __restrict__ X, int iterations, FaConst c) {
  constexpr int T = batch_block_threads(D);
  __shared__ __attribute__((aligned(16))) double sx[small_cap(D) * rec_width(D)];
  __shared__ __attribute__((aligned(16))) double tb[T * D];
  const int gi = items[blockIdx.x].x;
  const int G = items[blockIdx.x].y;
  const int r0 = off[gi];
  const int n = off[gi + 1] - r0;
  if (n < 1 || n > small_cap(D) || n * G > T) return;  // not this class (the host checks)
#define GE_BATCH_BLOCK_CASE(GG)                                                             \
  case GG:                                                                                  \
    batch_graph<D, GG, BlockScope>(n, threadIdx.x, T, r0, ip + r0, ix, dx, dp1 + r0,        \
                                   X + (size_t)r0 * D, sx, tb, iterations, c);              \
    break;
  switch (G) {
    GE_BATCH_BLOCK_CASE(1) GE_BATCH_BLOCK_CASE(2) GE_BATCH_BLOCK_CASE(4)
    default: break;
  }
#undef GE_BATCH_BLOCK_CASE
  static_assert(kBatchBlockLanes == 4, "the cases above");
}

}  // namespace

void fa_batch_device(ge_ctx* ctx, int count, const int* off, const int* ip, const int* ix,
                     const double* dx, int dim, double* X, int iterations,
                     const ge_fa_params& p) {
  FaBatchIn in;
  in.dim = dim;
  in.mode = p.mode;
  in.wide = wide_dim(dim);
  in.knobs = fa_knobs_from_env();
  std::vector<int> sizes(count), entries(count), cls(count), lanes(count);
  for (int g = 0; g < count; ++g) {
    sizes[g] = off[g + 1] - off[g];
    entries[g] = ip[off[g + 1]] - ip[off[g]];
  }
  int totals[GE_FA_BATCH_TOTALS];
  fa_batch_schedule(in, count, sizes.data(), cls.data(), lanes.data(), totals);
  std::copy(totals, totals + GE_FA_BATCH_TOTALS, ctx->fa_batch);
  const int N = count ? off[count] : 0;
  if (N == 0 || iterations <= 0) return;
  const int nw = totals[0], nb = totals[1];
  // the launch order of the two classes, {graph, lanes per row} each
  std::vector<int> order(nw + nb);
  fa_batch_order(count, sizes.data(), entries.data(), cls.data(), GE_FA_BATCH_WAVE, order.data());
  fa_batch_order(count, sizes.data(), entries.data(), cls.data(), GE_FA_BATCH_BLOCK,
                 order.data() + nw);
  // one upload: the offsets, then the items from an even index (int2)
  const size_t items_at = ((size_t)count + 2) / 2 * 2;
  std::vector<int> ints(items_at + 2 * (size_t)(nw + nb), 0);
  std::copy(off, off + count + 1, ints.begin());
  const int block_threads = dim <= kNarrowMaxDim ? kSmallGenT : kSmallWideT;
  for (int k = 0; k < nw + nb; ++k) {
    const int g = order[k];
    const int width = k < nw ? 64 : block_threads;
    if ((long long)sizes[g] * lanes[g] > width)
      throw Error(GE_ERR_STATE, "forceAtlas batch: a graph's lanes do not fit its class");
    ints[items_at + 2 * (size_t)k] = g;
    ints[items_at + 2 * (size_t)k + 1] = lanes[g];
  }
  hipStream_t s = ctx->stream;
  DevCsr A(N, ip, ix, dx, s);
  DevBuf<double> dbl((size_t)N * dim + N);  // the coordinates, then deg + 1
  DevBuf<int> dints(ints.size());
  double* const dX = dbl.p;
  double* const dp1 = dbl.p + (size_t)N * dim;
  const int* const doff = dints.p;
  const int2* const ditems = reinterpret_cast<const int2*>(dints.p + items_at);
  dbl.upload(X, (size_t)N * dim, s);
  dints.upload(ints.data(), ints.size(), s);
  launch_degp1(s, N, A.ip.p, A.dx.p, p.use_weights, dp1);
  const FaConst c = make_fa_const(p);
  dispatch_dim(dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    static_assert(batch_block_threads(D) >= kSmallWideT, "a block holds the wide schedule's lanes");
    if (nw)
      hipLaunchKernelGGL((fa_batch_wave<D>), dim3(totals[3]), dim3(64 * kBatchWaves), 0, s, nw,
                         ditems, doff, A.ip.p, A.ix.p, A.dx.p, dp1, dX, iterations, c);
    if (nb)
      hipLaunchKernelGGL((fa_batch_block<D>), dim3(nb), dim3(batch_block_threads(D)), 0, s,
                         ditems + nw, doff, A.ip.p, A.ix.p, A.dx.p, dp1, dX, iterations, c);
  });
  GE_HIP(hipGetLastError());
  // the serial class: ge_force_atlas's own device path on a rebased copy of the graph
  for (int g = 0; g < count; ++g) {
    if (cls[g] != GE_FA_BATCH_SERIAL || sizes[g] == 0) continue;
    const int r0 = off[g], n = sizes[g], e0 = ip[r0];
    std::vector<int> lip(n + 1), lix(entries[g]);
    for (int i = 0; i <= n; ++i) lip[i] = ip[r0 + i] - e0;
    for (int e = 0; e < entries[g]; ++e) lix[e] = ix[e0 + e] - r0;
    DevCsr Ag(n, lip.data(), lix.data(), dx + e0, s);
    fa_run_device(ctx, n, Ag.nnz, Ag.ip.p, Ag.ix.p, Ag.dx.p, dim, dX + (size_t)r0 * dim,
                  iterations, p);  // synchronises
  }
  dbl.download(X, (size_t)N * dim, s);
  GE_HIP(hipStreamSynchronize(s));
}

}  // namespace ge

extern "C" {

int ge_fa_batch_sched_query(int count, const int* sizes, const int* entries, int dim,
                            const ge_fa_params* p, int* cls, int* lanes, int* totals) {
  return ge::guarded([&] {
    GE_REQUIRE(p && count >= 0 && (count == 0 || sizes), "null argument or negative count");
    GE_REQUIRE(dim >= 1 && dim <= ge::kMaxDim, "dimension must be 1..16");
    (void)entries;  // they order a class's launch; the class itself is decided by the rows
    ge::FaBatchIn in;
    in.dim = dim;
    in.mode = p->mode;
    in.wide = ge::wide_dim(dim);
    in.knobs = ge::fa_knobs_from_env();
    std::vector<int> c(count), l(count);
    int t[GE_FA_BATCH_TOTALS];
    ge::fa_batch_schedule(in, count, sizes, c.data(), l.data(), t);
    if (cls) std::copy(c.begin(), c.end(), cls);
    if (lanes) std::copy(l.begin(), l.end(), lanes);
    if (totals) std::copy(t, t + GE_FA_BATCH_TOTALS, totals);
  });
}

int ge_fa_batch_info(const ge_ctx* ctx, int* totals) {
  return ge::guarded([&] {
    GE_REQUIRE(ctx && totals, "null argument");
    std::copy(ctx->fa_batch, ctx->fa_batch + GE_FA_BATCH_TOTALS, totals);
  });
}

}  // extern "C"

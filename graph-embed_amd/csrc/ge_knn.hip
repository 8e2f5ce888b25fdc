// ge_knn.hip -- the exact k nearest neighbours of include/ge.h ("layout neighbours") on
// the device.
//
//   knn_scan<W, U>   one query row per lane; the partners of j split blockIdx.y stream
//       through LDS tiles in ascending j; the lane keeps its sorted list of k entries
//       {s, j} in LDS and the list's last s as the threshold tau in a register;
//   knn_merge        with more than one j split: every entry of every partial list finds
//       its rank under the full (s, j) order by binary searches in the other lists and,
//       if that is below k, writes itself there.
//
// The list starts as k entries {+inf, -1} and tau as +inf, so that the one test s < tau
// is the whole candidate rule: it fails for a NaN or infinite s, and a list that never
// fills keeps the -1 / +inf the definition asks for past the last candidate.
#include <cstdlib>

#include "ge_knn.hpp"
#include "ge_pair.hpp"

namespace ge {

struct KnnScratch {
  DevBuf<double> part_s;  // the partial lists of a split call: (split, query row, k)
  DevBuf<int> part_j;
  DevBuf<unsigned long long> ins;  // the call's insertions
  unsigned long long* h_ins = nullptr;  // pinned; the copy a call enqueues behind its kernels
};

void knn_release(KnnScratch* s) {
  if (!s) return;
  if (s->h_ins) (void)hipHostFree(s->h_ins);
  delete s;
}

long long knn_device_insertions(const KnnScratch* s) {
  return s && s->h_ins ? (long long)*(volatile unsigned long long*)s->h_ins : 0;
}

namespace {

// The squared distance of include/ge.h: e_k = x_i[k] - x_j[k], s = e_0 e_0, then
// s = fma(e_k, e_k, s).  The form of energy_pair (ge_energy.hpp), restated here.  Each
// operation is written out and the build has -ffp-contract=off, so nothing else fuses.
template <int W>
__device__ __forceinline__ double knn_dist2(const double (&xi)[W], const double* __restrict__ xj) {
  double e[W];
#pragma unroll
  for (int c = 0; c < W; ++c) e[c] = xi[c] - xj[c];
  double s = e[0] * e[0];
#pragma unroll
  for (int c = 1; c < W; ++c) s = fma(e[c], e[c], s);
  return s;
}

// W: doubles per record (d for d <= 4; kMaxDim for the run-time-d form, the coordinates
// past d stored as +0 on both sides).  U: partners per step of the scan.  blockDim.x = R
// query rows.  Dynamic LDS: tile[kKnnTileJ * W] doubles, ls[k * R] doubles, lj[k * R]
// ints; entry t of lane l at t * R + l, so a lane touches its own column only and the
// lists need no barrier.
// out_j / out_s: (split * n_rows + query row) * k + t; out_s may be null when there is
// one split and the caller wants no distances.
template <int W, int U>
__global__ void __launch_bounds__(kKnnMaxRows)
knn_scan(int n, int d, const double* __restrict__ X, int k, int n_rows,
         const int* __restrict__ rows, int jsplit, int* __restrict__ out_j,
         double* __restrict__ out_s, unsigned long long* __restrict__ ins) {
  static_assert(kKnnTileJ % U == 0, "a tile holds whole steps");
  extern __shared__ __attribute__((aligned(16))) double knn_lds[];
  const int R = blockDim.x;
  const int tid = threadIdx.x;
  double* tile = knn_lds;
  double* ls = tile + kKnnTileJ * W;
  int* lj = reinterpret_cast<int*>(ls + (size_t)k * R);

  const int q = blockIdx.x * R + tid;
  const int jb = blockIdx.y;
  const int jchunk = (n + jsplit - 1) / jsplit;
  const long long jlo = (long long)jb * jchunk;
  const int jbeg = (int)(jlo < n ? jlo : n);
  const int jend = (int)(jlo + jchunk < n ? jlo + jchunk : n);

  int row = -1;
  if (q < n_rows) {
    row = rows ? rows[q] : q;
    if (row < 0 || row >= n) row = -1;  // reads nothing, gets no neighbours
  }
  double xi[W];
#pragma unroll
  for (int c = 0; c < W; ++c)
    xi[c] = row < 0 ? __builtin_nan("") : (c < d ? X[(size_t)row * d + c] : 0.0);
  for (int t = 0; t < k; ++t) {
    ls[t * R + tid] = __builtin_inf();
    lj[t * R + tid] = -1;
  }
  double tau = __builtin_inf();
  unsigned inserted = 0;

  for (int j0 = jbeg; j0 < jend; j0 += kKnnTileJ) {
    const int cnt = min(kKnnTileJ, jend - j0);
    const int cntu = (cnt + U - 1) / U * U;  // <= kKnnTileJ; the records past cnt are NaN
    __syncthreads();
    for (int e = tid; e < cntu * W; e += R) {
      const int p = e / W, c = e - p * W;
      double v = __builtin_nan("");
      if (p < cnt) v = c < d ? X[(size_t)(j0 + p) * d + c] : 0.0;  // j0 + p < jend <= n
      tile[e] = v;
    }
    __syncthreads();
    for (int jj = 0; jj < cntu; jj += U) {
      double s[U];
      bool any = false;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u] = knn_dist2<W>(xi, tile + (jj + u) * W);
        any = any || s[u] < tau;
      }
      if (any) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + jj + u;
          // Strict less: a later j that ties with tau loses to the entries held.  The
          // self pair (s = 0 unless the row is not finite) is dropped by its index.
          if (s[u] < tau && j != row) {
            int p = k - 1;  // the last entry falls off
            while (p > 0 && ls[(p - 1) * R + tid] > s[u]) {
              ls[p * R + tid] = ls[(p - 1) * R + tid];
              lj[p * R + tid] = lj[(p - 1) * R + tid];
              --p;
            }
            ls[p * R + tid] = s[u];  // behind every equal s: they have lower j
            lj[p * R + tid] = j;
            tau = ls[(k - 1) * R + tid];
            ++inserted;
          }
        }
      }
    }
  }
  if (q < n_rows) {
    const size_t o = ((size_t)jb * n_rows + q) * k;
    for (int t = 0; t < k; ++t) {
      out_j[o + t] = lj[t * R + tid];
      if (out_s) out_s[o + t] = ls[t * R + tid];
    }
  }
  // one atomic per wave
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) inserted += __shfl_xor(inserted, off);
  if ((tid & 63) == 0 && inserted) atomicAdd(ins, (unsigned long long)inserted);
}

// How many of the k ascending values a[0 .. k) are < v (strict) or <= v.
__device__ __forceinline__ int knn_count_below(const double* __restrict__ a, int k, double v,
                                               bool strict) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool below = strict ? a[mid] < v : a[mid] <= v;
    if (below) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Thread (q, b, t): entry t of split b's partial list of query row q.  A real entry
// (j >= 0, s finite) stands behind the t entries before it in its own list, behind every
// entry with s' <= s of a lower split (lower j) and every entry with s' < s of a higher
// one.  The padding {+inf, -1} stands behind all real entries, in (b, t) order.  The
// ranks are a permutation of 0 .. jsplit k - 1, so each of the k outputs is written once.
__global__ void __launch_bounds__(256)
knn_merge(int n_rows, int k, int jsplit, const double* __restrict__ ps,
          const int* __restrict__ pj, int* __restrict__ idx, double* __restrict__ dist2) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per_row = (size_t)jsplit * k;
  if (gid >= per_row * n_rows) return;
  const int q = (int)(gid / per_row);
  const int b = (int)((gid - (size_t)q * per_row) / k);
  const int t = (int)(gid - (size_t)q * per_row - (size_t)b * k);
  const size_t own = ((size_t)b * n_rows + q) * k;
  const double s = ps[own + t];
  const int j = pj[own + t];
  int rank;
  if (j >= 0) {
    rank = t;
    for (int o = 0; o < jsplit; ++o)
      if (o != b) rank += knn_count_below(ps + ((size_t)o * n_rows + q) * k, k, s, o > b);
  } else {
    rank = t;  // the real entries of the own list, and its padding before t
    for (int o = 0; o < jsplit; ++o) {
      if (o == b) continue;
      const int real = knn_count_below(ps + ((size_t)o * n_rows + q) * k, k, __builtin_inf(), true);
      rank += o < b ? k : real;
    }
  }
  if (rank < k) {
    idx[(size_t)q * k + rank] = j;
    if (dist2) dist2[(size_t)q * k + rank] = s;
  }
}

template <int W, int U>
void launch_scan(hipStream_t s, int blocks, int jsplit, int R, size_t lds, int n, int d,
                 const double* X, int k, int n_rows, const int* rows, int* out_j, double* out_s,
                 unsigned long long* ins) {
  if (lds > 65536)  // above the default dynamic-LDS limit
    GE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_scan<W, U>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((knn_scan<W, U>), dim3(blocks, jsplit), dim3(R), lds, s, n, d, X, k, n_rows,
                     rows, jsplit, out_j, out_s, ins);
}

}  // namespace

void knn_device(ge_ctx* ctx, int n, int dim, const double* d_x, int k, int n_rows,
                const int* d_rows, int* d_idx, double* d_dist2) {
  hipStream_t s = ctx->stream;
  if (!ctx->knn_scratch) {
    auto* sc = new KnnScratch();
    ctx->knn_scratch = sc;
    GE_HIP(hipHostMalloc((void**)&sc->h_ins, sizeof(unsigned long long), hipHostMallocDefault));
    *sc->h_ins = 0;
    sc->ins.alloc(1);
  }
  KnnScratch& sc = *ctx->knn_scratch;
  const int R = knn_rows_per_wg(k, dim);
  int jsplit = knn_jsplit(n, n_rows, R);
  if (const char* e = std::getenv("GE_KNN_JSPLIT"))  // tests: changes no result
    jsplit = std::max(1, std::min(kKnnMaxSplit, std::atoi(e)));
  ctx->knn.path = GE_KNN_PATH_DEVICE;
  ctx->knn.form = dim <= kNarrowMaxDim ? GE_KNN_FORM_NARROW : GE_KNN_FORM_WIDE;
  ctx->knn.rows_per_wg = R;
  ctx->knn.jsplit = jsplit;
  ctx->knn.host_insertions = 0;
  GE_HIP(hipMemsetAsync(sc.ins.p, 0, sizeof(unsigned long long), s));
  if (n_rows > 0) {
    int* out_j = d_idx;
    double* out_s = d_dist2;
    if (jsplit > 1) {
      const size_t need = (size_t)jsplit * n_rows * k;
      if (sc.part_s.n < need) {
        sc.part_s.alloc(need);
        sc.part_j.alloc(need);
      }
      out_j = sc.part_j.p;
      out_s = sc.part_s.p;
    }
    const int blocks = (n_rows + R - 1) / R;
    const size_t lds = knn_lds_bytes(R, k, dim);
    if (dim <= kNarrowMaxDim) {
      dispatch_dim_narrow(dim, [&](auto Dc) {
        launch_scan<decltype(Dc)::value, 4>(s, blocks, jsplit, R, lds, n, dim, d_x, k, n_rows,
                                            d_rows, out_j, out_s, sc.ins.p);
      });
    } else {
      launch_scan<kMaxDim, 2>(s, blocks, jsplit, R, lds, n, dim, d_x, k, n_rows, d_rows, out_j,
                              out_s, sc.ins.p);
    }
    GE_HIP(hipGetLastError());
    if (jsplit > 1) {
      const size_t total = (size_t)jsplit * n_rows * k;
      hipLaunchKernelGGL(knn_merge, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n_rows,
                         k, jsplit, sc.part_s.p, sc.part_j.p, d_idx, d_dist2);
      GE_HIP(hipGetLastError());
    }
  }
  GE_HIP(hipMemcpyAsync(sc.h_ins, sc.ins.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}

}  // namespace ge

extern "C" int ge_layout_knn_device(ge_ctx* ctx, int n, int dim, const double* d_x, int k,
                                    int n_rows, const int* d_rows, int* d_idx, double* d_dist2) {
  return ge::guarded([&] {
    GE_REQUIRE(ctx, "ge_layout_knn_device needs a context");
    GE_REQUIRE(dim >= 1 && dim <= ge::kMaxDim, "dimension must be 1..16");
    GE_REQUIRE(k >= 1 && k <= GE_KNN_MAX_K, "k must be 1..64");
    GE_REQUIRE(n >= 1, "n must be at least 1");
    GE_REQUIRE(n_rows >= 0 && (d_rows || n_rows == n),
               "n_rows must be >= 0, and n when no row list is given");
    GE_REQUIRE(d_x && (d_idx || n_rows == 0), "null coordinates or idx");
    ge::DeviceGuard g(ctx);
    ge::knn_device(ctx, n, dim, d_x, k, n_rows, d_rows, d_idx, d_dist2);
  });
}

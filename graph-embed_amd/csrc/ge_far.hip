// ge_far.hip -- GE_MODE_FARFIELD: a Barnes-Hut style far field for the single
// level's all-pairs repulsion (include/forceatlas.hpp:151-167), D = 1..4, fp64, and
// (the segmented engine, second half of the file) for the streamed aggregates of a
// multilevel level (include/forceatlas.hpp:394-410).
//
// One pass, all on the plan's stream, nothing allocated:
//   far_box_part / far_box_final  min and max of the coordinates per axis; a box that
//                                 is not finite ends the pass (the caller runs FAST)
//   far_keys                      Morton key, floor(63 / D) bits per axis, one scale
//   rocprim::radix_sort_pairs     stable: equal keys keep vertex order
//   far_gather                    sorted records {x_0 .. x_{D-1}, deg + 1}
//   far_cells                     per level, one wave per cell: M, c, a from the
//                                 cell's member records; the items' balls likewise
//   far_repulse_kernel<D, R>      the item kernel
// The hierarchy is flat: level l has ceil(n / (64 G^l)) cells, cell q of level l + 1
// holds cells [G q, G q + G) of level l, levels are added until the top has at most G
// cells.  A cell is {c_0 .. c_{D-1}, M, a}.
//
// far_repulse_kernel: a wave takes an item (64 R consecutive sorted rows; lane, slot r -> row
// r0 + lane + 64 r) from the queue and walks the hierarchy depth first from the top
// level's cell 0 without a stack (the parent of cell q is q / G, its first child G q).
// Every decision is wave-uniform, made from the item's ball {c_I, a_I}:
//   accept C  iff  a_C <= theta (Dist - a_I)  and  Dist - a_I - a_C >= kFaEps,
//   Dist = sqrt(sum_k (c_I,k - c_C,k)^2), plain ascending sum, IEEE sqrt
// accepted: one fast_rep_pair(x_i, c_C, dir_i, M_C) per row slot; rejected above the
// leaves: descend; a rejected leaf: its 64 records through the wave's LDS slice and
// fast_rep_pair per record (the self pair is a zero term).  A row's sum is one lane's
// fma chain in walk order, so results do not depend on the grid or on timing.  No
// kernel waits on another workgroup.  -ffp-contract=off: every fma is written out.
//
// gfx950 ISA of far_repulse_kernel (-O3): no scratch at any <D, R>; VGPRs at D = 1 / 2 /
// 3 / 4: 32 / 40 / 48 / 56 for R = 1 and 86 / 118 / 114 / 142 for R = 4.  Inner loop of a
// rejected leaf at D = 3, R = 1, per partner: 22 fp64 VALU (10 v_mul, 7 v_fma / v_fmac,
// 3 v_add, v_min, v_rsq_f64) and two ds_read_b128; the cell records come in through
// scalar loads.  Known limit (FARFIELD mode): the launch ends with its most
// expensive item, and an item whose ball is large accepts nothing.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <rocprim/device/device_radix_sort.hpp>
#include <vector>

#include "ge_far.hpp"
#include "ge_pair.hpp"
#include "ge_rows.hpp"

namespace ge {

using u64 = unsigned long long;

struct FarEngine {
  int n = 0, dim = 0, cus = 0, R = 1;
  double theta = 0.5;
  int nlev = 0, cnt[kFarMaxLevels] = {}, off[kFarMaxLevels] = {};
  long long pts[kFarMaxLevels] = {};
  int ncells = 0, nitems = 0, key_bits = 0;
  DevBuf<double> part, box, rec, cells, items;
  DevBuf<u64> keys_in, keys, counters;
  DevBuf<int> ids, perm, lev, flag, queue;
  DevBuf<unsigned char> sort_tmp;
  size_t sort_bytes = 0;
  int* flag_h = nullptr;  // pinned
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ran = false, fell_back = false;
  ~FarEngine() {
    if (flag_h) (void)hipHostFree(flag_h);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

constexpr int kBoxBlocks = 256;
constexpr int kFarT = 256;  // threads per block of every kernel here

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < __builtin_inf(); }

// Partial min / max of block b's strided share: part[b] = {lo[D], hi[D], bad}.
template <int D>
__global__ void __launch_bounds__(kFarT)
far_box_part(int n, const double* __restrict__ X, double* __restrict__ part) {
  __shared__ double sh[kFarT / 64][2 * D + 1];
  double lo[D], hi[D];
  int bad = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = __builtin_inf();
    hi[k] = -__builtin_inf();
  }
  for (size_t i = (size_t)blockIdx.x * kFarT + threadIdx.x; i < (size_t)n;
       i += (size_t)gridDim.x * kFarT) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double v = X[i * D + k];
      bad |= !finite_d(v);
      lo[k] = fmin(lo[k], v);
      hi[k] = fmax(hi[k], v);
    }
  }
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], o));
    }
    bad |= __shfl_xor(bad, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      sh[w][k] = lo[k];
      sh[w][D + k] = hi[k];
    }
    sh[w][2 * D] = bad ? 1.0 : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + (size_t)blockIdx.x * (2 * D + 1);
    for (int k = 0; k < D; ++k) {
      double a = sh[0][k], b = sh[0][D + k];
      for (int v = 1; v < kFarT / 64; ++v) {
        a = fmin(a, sh[v][k]);
        b = fmax(b, sh[v][D + k]);
      }
      o[k] = a;
      o[D + k] = b;
    }
    double f = 0.0;
    for (int v = 0; v < kFarT / 64; ++v) f = fmax(f, sh[v][2 * D]);
    o[2 * D] = f;
  }
}

// One wave: box = {lo[D], scale}, scale = 2^bits / (largest extent) (0 when every point
// coincides or the quotient is not finite); flag = 1 when every coordinate is finite.
template <int D>
__global__ void __launch_bounds__(64)
far_box_final(int nparts, const double* __restrict__ part, double* __restrict__ box,
              int* __restrict__ flag) {
  const int lane = threadIdx.x;
  double lo[D], hi[D], bad = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = __builtin_inf();
    hi[k] = -__builtin_inf();
  }
  for (int b = lane; b < nparts; b += 64) {
    const double* p = part + (size_t)b * (2 * D + 1);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      lo[k] = fmin(lo[k], p[k]);
      hi[k] = fmax(hi[k], p[D + k]);
    }
    bad = fmax(bad, p[2 * D]);
  }
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], o));
    }
    bad = fmax(bad, __shfl_xor(bad, o));
  }
  if (lane == 0) {
    double ext = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) ext = fmax(ext, hi[k] - lo[k]);
    constexpr int bits = 63 / D;
    double scale = ext > 0.0 ? ldexp(1.0, bits) / ext : 0.0;
    if (!finite_d(scale)) scale = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) box[k] = lo[k];
    box[D] = scale;
    flag[0] = bad == 0.0 ? 1 : 0;
  }
}

// key: bit (b D + k) is bit b of q_k = min(2^bits - 1, (u64) floor((x_k - lo_k) scale)).
template <int D>
__global__ void __launch_bounds__(kFarT)
far_keys(int n, const double* __restrict__ X, const double* __restrict__ box,
         u64* __restrict__ keys, int* __restrict__ ids) {
  const int i = blockIdx.x * kFarT + threadIdx.x;
  if (i >= n) return;
  constexpr int bits = 63 / D;
  constexpr u64 qmax = (1ull << bits) - 1;
  const double scale = box[D];
  u64 key = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double t = (X[(size_t)i * D + k] - box[k]) * scale;
    const double f = floor(t);
    u64 q = f >= 0x1p63 ? qmax : (u64)f;  // t >= 0: lo is the minimum
    q = q < qmax ? q : qmax;
    if constexpr (D == 1) {
      key = q;
    } else {
      for (int b = 0; b < bits; ++b) key |= ((q >> b) & 1ull) << (b * D + k);
    }
  }
  keys[i] = key;
  ids[i] = i;
}

template <int D>
__global__ void __launch_bounds__(kFarT)
far_gather(int n, const double* __restrict__ X, const double* __restrict__ dp1,
           const int* __restrict__ perm, double* __restrict__ rec) {
  const int p = blockIdx.x * kFarT + threadIdx.x;
  if (p >= n) return;
  const int v = perm[p];
#pragma unroll
  for (int k = 0; k < D; ++k) rec[(size_t)p * (D + 1) + k] = X[(size_t)v * D + k];
  rec[(size_t)p * (D + 1) + D] = dp1[v];
}

// One wave per cell: M = sum m_j, c = (sum m_j x_j) / M, a = (1 + 2^-40) sqrt(max_j
// sum_k (x_jk - c_k)^2) over the records [begin, end).  Fixed order: a lane adds its
// records (begin + lane, + 64, ...) ascending, then the xor butterfly 32, 16, .. 1, whose
// sums are the same bits on every lane.  The factor covers the roundings of the squared
// distance and of the root (a few 2^-53), so a is never below the exact max |x_j - c|.
template <int D>
__device__ __forceinline__ void cell_summary(const double* __restrict__ rec, long long begin,
                                             long long end, int lane, double* __restrict__ o) {
  double M = 0.0, sx[D];
#pragma unroll
  for (int k = 0; k < D; ++k) sx[k] = 0.0;
  for (long long j = begin + lane; j < end; j += 64) {
    const double m = rec[(size_t)j * (D + 1) + D];
    M = M + m;
#pragma unroll
    for (int k = 0; k < D; ++k) sx[k] = fma(m, rec[(size_t)j * (D + 1) + k], sx[k]);
  }
  for (int o2 = 32; o2; o2 >>= 1) {
    M = M + __shfl_xor(M, o2);
#pragma unroll
    for (int k = 0; k < D; ++k) sx[k] = sx[k] + __shfl_xor(sx[k], o2);
  }
  double c[D];
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = sx[k] / M;
  double s2 = 0.0;
  for (long long j = begin + lane; j < end; j += 64) {
    double e = rec[(size_t)j * (D + 1)] - c[0];
    double s = e * e;
#pragma unroll
    for (int k = 1; k < D; ++k) {
      e = rec[(size_t)j * (D + 1) + k] - c[k];
      s = s + e * e;
    }
    s2 = fmax(s2, s);
  }
  for (int o2 = 32; o2; o2 >>= 1) s2 = fmax(s2, __shfl_xor(s2, o2));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) o[k] = c[k];
    o[D] = M;
    o[D + 1] = sqrt(s2) * (1.0 + 0x1p-40);
  }
}

// Cell `cell` of `csz` consecutive records of the n.
template <int D>
__global__ void __launch_bounds__(kFarT)
far_cells(int n, long long csz, int ncell, const double* __restrict__ rec,
          double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * (kFarT / 64) + (threadIdx.x >> 6);
  if (cell >= ncell) return;  // wave-uniform
  const long long begin = (long long)cell * csz;
  const long long end = begin + csz < (long long)n ? begin + csz : (long long)n;
  cell_summary<D>(rec, begin, end, lane, out + (size_t)cell * (D + 2));
}

__global__ void far_mass_check(int n, const double* __restrict__ dp1, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !(dp1[i] > 0.0 && finite_d(dp1[i]))) atomicOr(bad, 1);
}

// The item kernel (header comment).  lev = {levels, cells per level [8], first cell of
// each level in `cells` [8]}.  counters: cells accepted per level [8], leaves evaluated
// pair by pair, pair terms (rows x partners, an accepted cell being one partner, less
// each row's self pair); lanes 0..9 of the wave add an item's share at its end.
template <int D, int R>
__global__ void __launch_bounds__(kFarT)
far_repulse_kernel(int n, int nitems, const int* __restrict__ lev,
                   const double* __restrict__ cells, const double* __restrict__ items,
                   const double* __restrict__ rec, const int* __restrict__ perm, double theta,
                   double repel, int* __restrict__ queue, u64* __restrict__ counters,
                   double* __restrict__ Frep) {
  constexpr int WV = rec_width(D);
  constexpr int CW = D + 2;
  constexpr int G = kFarGroup;
  __shared__ __attribute__((aligned(16))) double tiles[kFarT / 64][kFarLeaf * WV];
  __shared__ u64 wcnt[kFarT / 64][kFarMaxLevels + 2];
  const int lane = threadIdx.x & 63;
  double* tile = tiles[threadIdx.x >> 6];
  u64* cnt = wcnt[threadIdx.x >> 6];
  const int top = lev[0] - 1;
  const int ntop = lev[1 + top];
  if (lane < kFarMaxLevels + 2) cnt[lane] = 0;
  for (;;) {
    int q = 0;
    if (lane == 0) q = atomicAdd(queue, 1);
    q = __builtin_amdgcn_readfirstlane(q);
    if (q >= nitems) break;
    const int r0 = q * (kFarLeaf * R);  // nitems * 64 R < n + 64 R: no overflow (far_create)
    const int r1 = min(n, r0 + kFarLeaf * R);
    double xi[R][D], di[R], acc[R][D];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int p = r0 + lane + kFarLeaf * r;
      const bool ok = p < r1;
      const size_t c = (size_t)(ok ? p : r0);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        xi[r][k] = ok ? rec[c * (D + 1) + k] : 0.0;
        acc[r][k] = 0.0;
      }
      di[r] = ok ? rec[c * (D + 1) + D] * repel : 0.0;
    }
    double cI[D];
#pragma unroll
    for (int k = 0; k < D; ++k) cI[k] = items[(size_t)q * CW + k];
    const double aI = items[(size_t)q * CW + D + 1];
    wave_lds_sync();  // cnt zeroed / the last item's counters read
    int l = top, idx = 0;
    u64 partners = 0;
    for (;;) {
      const double* cc = cells + ((size_t)lev[1 + kFarMaxLevels + l] + (size_t)idx) * CW;
      double cC[D];
#pragma unroll
      for (int k = 0; k < D; ++k) cC[k] = cc[k];
      const double MC = cc[D], aC = cc[D + 1];
      double e = cI[0] - cC[0];
      double s = e * e;
#pragma unroll
      for (int k = 1; k < D; ++k) {
        e = cI[k] - cC[k];
        s = s + e * e;
      }
      const double t = sqrt(s) - aI;
      const bool take = __builtin_amdgcn_readfirstlane((int)(aC <= theta * t && t - aC >= kFaEps));
      if (take) {
#pragma unroll
        for (int r = 0; r < R; ++r) fast_rep_pair<D>(xi[r], cC, di[r], MC, acc[r]);
        if (lane == 0) cnt[l] += 1;
        partners += 1;
      } else if (l == 0) {
        const int j0 = idx * kFarLeaf;
        const int m = min(kFarLeaf, n - j0);
        wave_lds_sync();  // the previous leaf has been read by every lane
        {
          const size_t c = (size_t)min(j0 + lane, n - 1);
#pragma unroll
          for (int k = 0; k <= D; ++k) tile[lane * WV + k] = rec[c * (D + 1) + k];
        }
        wave_lds_sync();
        for (int jj = 0; jj < m; ++jj) {
          double xj[D];
#pragma unroll
          for (int k = 0; k < D; ++k) xj[k] = tile[jj * WV + k];
          const double dj = tile[jj * WV + D];
#pragma unroll
          for (int r = 0; r < R; ++r) fast_rep_pair<D>(xi[r], xj, di[r], dj, acc[r]);
        }
        if (lane == 0) cnt[kFarMaxLevels] += 1;
        partners += (u64)m;
      } else {
        l -= 1;
        idx *= G;
        continue;
      }
      // the next cell in walk order: the right sibling, else the parent's
      bool done = false;
      for (;;) {
        ++idx;
        if (l == top) {
          done = idx >= ntop;
          break;
        }
        if (idx % G == 0 || idx >= lev[1 + l]) {
          idx = (idx - 1) / G;
          ++l;
          continue;
        }
        break;
      }
      if (done) break;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int p = r0 + lane + kFarLeaf * r;
      if (p < r1) {
        const size_t v = (size_t)perm[p];
#pragma unroll
        for (int k = 0; k < D; ++k) Frep[v * D + k] = acc[r][k];
      }
    }
    if (lane == 0) cnt[kFarMaxLevels + 1] = (partners - 1) * (u64)(r1 - r0);  // less the self pair
    wave_lds_sync();
    if (lane < kFarMaxLevels + 2) {
      const u64 v = cnt[lane];
      if (v) atomicAdd(&counters[lane], v);
      cnt[lane] = 0;
    }
  }
}

template <class F>
void far_dim(int dim, F&& f) {
  switch (dim) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: throw Error(GE_ERR_STATE, "the far field is built for dimensions 1..4");
  }
}

inline int blocks_for(long long threads) { return (int)((threads + kFarT - 1) / kFarT); }

}  // namespace

FarEngine* far_create(hipStream_t s, int n, int dim, double theta, int item_rows, int cus) {
  GE_REQUIRE(n > 0 && dim >= 1 && dim <= 4, "far field: bad n or dim");
  GE_REQUIRE(item_rows == kFarLeaf || item_rows == 4 * kFarLeaf, "far field: items of 64 or 256 rows");
  GE_REQUIRE(n <= 0x7fffffff - 4 * kFarLeaf, "far field: n too large");
  std::unique_ptr<FarEngine> e(new FarEngine());
  e->n = n;
  e->dim = dim;
  e->cus = cus;
  e->theta = theta;
  e->R = item_rows / kFarLeaf;
  e->key_bits = (63 / dim) * dim;
  long long pts = kFarLeaf;
  int cnt = (n + kFarLeaf - 1) / kFarLeaf, off = 0;
  for (int l = 0; l < kFarMaxLevels; ++l) {
    e->cnt[l] = cnt;
    e->off[l] = off;
    e->pts[l] = pts;
    e->nlev = l + 1;
    off += cnt;
    if (cnt <= kFarGroup) break;
    cnt = (cnt + kFarGroup - 1) / kFarGroup;
    pts *= kFarGroup;
  }
  e->ncells = off;
  e->nitems = (n + item_rows - 1) / item_rows;
  e->part.alloc((size_t)kBoxBlocks * (2 * dim + 1));
  e->box.alloc(dim + 1);
  e->rec.alloc((size_t)n * (dim + 1));
  e->cells.alloc((size_t)e->ncells * (dim + 2));
  e->items.alloc((size_t)e->nitems * (dim + 2));
  e->keys_in.alloc(n);
  e->keys.alloc(n);
  e->ids.alloc(n);
  e->perm.alloc(n);
  e->counters.alloc(kFarMaxLevels + 2);
  e->flag.alloc(1);
  e->queue.alloc(1);
  std::vector<int> h_lev(1 + 2 * kFarMaxLevels, 0);
  h_lev[0] = e->nlev;
  for (int l = 0; l < e->nlev; ++l) {
    h_lev[1 + l] = e->cnt[l];
    h_lev[1 + kFarMaxLevels + l] = e->off[l];
  }
  e->lev.alloc(h_lev.size());
  e->lev.upload(h_lev.data(), h_lev.size(), s);
  GE_HIP(rocprim::radix_sort_pairs(nullptr, e->sort_bytes, e->keys_in.p, e->keys.p, e->ids.p,
                                   e->perm.p, (size_t)n, 0, e->key_bits, s));
  e->sort_tmp.alloc(std::max<size_t>(e->sort_bytes, 1));
  GE_HIP(hipHostMalloc((void**)&e->flag_h, sizeof(int), hipHostMallocDefault));
  *e->flag_h = 0;
  for (hipEvent_t& ev : e->ev) GE_HIP(hipEventCreate(&ev));
  GE_HIP(hipMemsetAsync(e->counters.p, 0, sizeof(u64) * e->counters.n, s));
  GE_HIP(hipStreamSynchronize(s));  // h_lev is read by the upload
  return e.release();
}

void far_destroy(FarEngine* e) { delete e; }

bool far_masses_ok(hipStream_t s, int n, const double* dp1) {
  DevBuf<int> bad(1);
  int h = 0;
  GE_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(far_mass_check, dim3(blocks_for(n)), dim3(kFarT), 0, s, n, dp1, bad.p);
  GE_HIP(hipGetLastError());
  GE_HIP(hipMemcpyAsync(&h, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  GE_HIP(hipStreamSynchronize(s));
  return h == 0;
}

bool far_repulse(FarEngine* e, hipStream_t s, const double* X, const double* dp1, double repel,
                 double* Frep) {
  const int n = e->n;
  bool ran = false;
  far_dim(e->dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    GE_HIP(hipEventRecord(e->ev[0], s));
    const int nparts = std::min(kBoxBlocks, blocks_for(n));
    hipLaunchKernelGGL((far_box_part<D>), dim3(nparts), dim3(kFarT), 0, s, n, X, e->part.p);
    hipLaunchKernelGGL((far_box_final<D>), dim3(1), dim3(64), 0, s, nparts, e->part.p, e->box.p,
                       e->flag.p);
    GE_HIP(hipGetLastError());
    GE_HIP(hipMemcpyAsync(e->flag_h, e->flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GE_HIP(hipStreamSynchronize(s));
    e->ran = true;
    e->fell_back = *e->flag_h == 0;
    if (e->fell_back) return;
    hipLaunchKernelGGL((far_keys<D>), dim3(blocks_for(n)), dim3(kFarT), 0, s, n, X, e->box.p,
                       e->keys_in.p, e->ids.p);
    GE_HIP(hipGetLastError());
    GE_HIP(rocprim::radix_sort_pairs(e->sort_tmp.p, e->sort_bytes, e->keys_in.p, e->keys.p,
                                     e->ids.p, e->perm.p, (size_t)n, 0, e->key_bits, s));
    hipLaunchKernelGGL((far_gather<D>), dim3(blocks_for(n)), dim3(kFarT), 0, s, n, X, dp1,
                       e->perm.p, e->rec.p);
    for (int l = 0; l < e->nlev; ++l)
      hipLaunchKernelGGL((far_cells<D>), dim3(blocks_for((long long)e->cnt[l] * 64)), dim3(kFarT),
                         0, s, n, e->pts[l], e->cnt[l], e->rec.p,
                         e->cells.p + (size_t)e->off[l] * (D + 2));
    hipLaunchKernelGGL((far_cells<D>), dim3(blocks_for((long long)e->nitems * 64)), dim3(kFarT), 0,
                       s, n, (long long)kFarLeaf * e->R, e->nitems, e->rec.p, e->items.p);
    GE_HIP(hipGetLastError());
    GE_HIP(hipMemsetAsync(e->queue.p, 0, sizeof(int), s));
    GE_HIP(hipMemsetAsync(e->counters.p, 0, sizeof(u64) * e->counters.n, s));
    GE_HIP(hipEventRecord(e->ev[1], s));
    const int waves = kFarT / 64;
    const int blocks = std::max(1, std::min(e->cus * 4, (e->nitems + waves - 1) / waves));
    auto go = [&](auto Rc) {
      constexpr int RC = decltype(Rc)::value;
      hipLaunchKernelGGL((far_repulse_kernel<D, RC>), dim3(blocks), dim3(kFarT), 0, s, n,
                         e->nitems, e->lev.p, e->cells.p, e->items.p, e->rec.p, e->perm.p,
                         e->theta, repel, e->queue.p, e->counters.p, Frep);
    };
    if (e->R == 4) go(std::integral_constant<int, 4>());
    else go(std::integral_constant<int, 1>());
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(e->ev[2], s));
    ran = true;
  });
  return ran;
}

void far_info(FarEngine* e, hipStream_t s, double* theta, int* item_rows, int* levels,
              int* level_cells, long long* level_points, int* fallback, long long* accepted,
              long long* exact_leaves, long long* pair_terms, double* prep_ms, double* item_ms) {
  GE_HIP(hipStreamSynchronize(s));
  if (theta) *theta = e->theta;
  if (item_rows) *item_rows = kFarLeaf * e->R;
  if (levels) *levels = e->nlev;
  for (int l = 0; l < kFarMaxLevels; ++l) {
    if (level_cells) level_cells[l] = l < e->nlev ? e->cnt[l] : 0;
    if (level_points) level_points[l] = l < e->nlev ? e->pts[l] : 0;
  }
  const bool counted = e->ran && !e->fell_back;
  u64 h[kFarMaxLevels + 2] = {};
  if (counted) {
    GE_HIP(hipMemcpyAsync(h, e->counters.p, sizeof(h), hipMemcpyDeviceToHost, s));
    GE_HIP(hipStreamSynchronize(s));
  }
  if (fallback) *fallback = e->ran && e->fell_back ? 1 : 0;
  if (accepted)
    for (int l = 0; l < kFarMaxLevels; ++l) accepted[l] = (long long)h[l];
  if (exact_leaves) *exact_leaves = (long long)h[kFarMaxLevels];
  if (pair_terms) *pair_terms = (long long)h[kFarMaxLevels + 1];
  float a = 0.f, b = 0.f;
  if (counted) {
    GE_HIP(hipEventElapsedTime(&a, e->ev[0], e->ev[1]));
    GE_HIP(hipEventElapsedTime(&b, e->ev[1], e->ev[2]));
  }
  if (prep_ms) *prep_ms = a;
  if (item_ms) *item_ms = b;
}

void far_layout(FarEngine* e, hipStream_t s, int* perm, unsigned long long* keys, double* box,
                double* cells, double* items) {
  if (!e->ran || e->fell_back)
    throw Error(GE_ERR_STATE, "far field: no pass has run (or the last one fell back to FAST)");
  GE_HIP(hipStreamSynchronize(s));
  if (perm) e->perm.download(perm, e->n, s);
  if (keys) e->keys.download(keys, e->n, s);
  if (box) e->box.download(box, e->dim + 1, s);
  if (cells) e->cells.download(cells, (size_t)e->ncells * (e->dim + 2), s);
  if (items) e->items.download(items, (size_t)e->nitems * (e->dim + 2), s);
  GE_HIP(hipStreamSynchronize(s));
}

// ---------------------------------------------------------------------------
// The segmented engine (ge_far.hpp): the same scheme per streamed aggregate of a
// multilevel level, every pass on the caller's stream with no host synchronisation.
//   far_seg_box      one block per segment: its own box and scale, and a flag that is 0
//                    when a coordinate is not finite
//   far_seg_keys     key = segment rank above the Morton bits (all zero under a 0 flag)
//   rocprim::radix_sort_pairs   one stable sort of all segments: a segment's members
//                    stay in its range, equal keys keep P_T order
//   far_seg_gather   sorted records {x, DP} and each sorted row's P_T position
//   far_seg_cells    one wave per cell or item ball, from a table of record ranges
//   far_seg_repulse_kernel<D, R>   far_repulse_kernel's walk inside one segment
// The rows are kept in the segments' order (larger first), and so are the items, so
// the queue hands out the largest aggregates' items first.  Items of 64 rows: on levels
// of equal aggregates of 2^12 .. 2^16 members they took 0.92 .. 0.67 of the step that
// 256-row items took (profiles/r19/crossover.jsonl; GE_FAR_R=4 selects 256).
//
// gfx950 ISA of far_seg_repulse_kernel (-O3): no scratch at any <D, R>; VGPRs at D = 1 /
// 2 / 3 / 4: 32 / 40 / 48 / 56 for R = 1 and 86 / 118 / 114 / 142 for R = 4 (the walk reads the
// segment through scalar loads: 12 more SGPRs than far_repulse_kernel).  The inner
// loop of a rejected leaf is far_repulse_kernel's: at D = 3, R = 1, per partner 22 fp64
// VALU (10 v_mul, 7 v_fma / v_fmac, 3 v_add, v_min, v_rsq_f64) and two ds_read_b128.

struct FarSeg {  // one segment, as the kernels read it
  int fb, s, base, nlev;     // first sorted row, members, first P_T position, levels
  int cnt[kFarMaxLevels];    // cells per level, leaves first
  int off[kFarMaxLevels];    // first cell of each level in `sums`
};

struct FarSegEngine {
  int nseg = 0, dim = 0, cus = 0, R = 1, bits = 0, sort_bits = 0;
  long long N = 0;  // rows of all segments
  double theta = 0.5;
  int ncells = 0, nitems = 0;
  std::vector<FarSeg> h_seg;
  std::vector<int> item0;  // first item of each segment (+ the total)
  DevBuf<FarSeg> seg;
  DevBuf<int> seg_of, flag, ids, permc, pos, queue;
  DevBuf<int2> ranges;  // record range of every cell, then of every item
  DevBuf<int4> itemd;   // (segment, first sorted row, end row, 0)
  DevBuf<double> box, rec, sums;  // sums: the cells, then the items' balls
  DevBuf<u64> keys_in, keys, counters;
  DevBuf<unsigned char> sort_tmp;
  size_t sort_bytes = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ran = false;
  ~FarSegEngine() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

template <int D>
__global__ void __launch_bounds__(kFarT)
far_seg_box(const FarSeg* __restrict__ segs, int bits, const double* __restrict__ X,
            double* __restrict__ box, int* __restrict__ flag) {
  __shared__ double sh[kFarT / 64][2 * D + 1];
  const int base = segs[blockIdx.x].base, s = segs[blockIdx.x].s;
  double lo[D], hi[D];
  int bad = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = __builtin_inf();
    hi[k] = -__builtin_inf();
  }
  for (int i = threadIdx.x; i < s; i += kFarT) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double v = X[((size_t)base + i) * D + k];
      bad |= !finite_d(v);
      lo[k] = fmin(lo[k], v);
      hi[k] = fmax(hi[k], v);
    }
  }
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], o));
    }
    bad |= __shfl_xor(bad, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      sh[w][k] = lo[k];
      sh[w][D + k] = hi[k];
    }
    sh[w][2 * D] = bad ? 1.0 : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = box + (size_t)blockIdx.x * (D + 1);
    double ext = 0.0, f = 0.0;
    for (int k = 0; k < D; ++k) {
      double a = sh[0][k], b = sh[0][D + k];
      for (int v = 1; v < kFarT / 64; ++v) {
        a = fmin(a, sh[v][k]);
        b = fmax(b, sh[v][D + k]);
      }
      o[k] = a;
      ext = fmax(ext, b - a);
    }
    for (int v = 0; v < kFarT / 64; ++v) f = fmax(f, sh[v][2 * D]);
    double scale = ext > 0.0 ? ldexp(1.0, bits) / ext : 0.0;
    if (!finite_d(scale)) scale = 0.0;
    o[D] = scale;
    flag[blockIdx.x] = f == 0.0 ? 1 : 0;
  }
}

// key: the segment's rank above D * bits Morton bits (far_keys' interleaving).
template <int D>
__global__ void __launch_bounds__(kFarT)
far_seg_keys(long long N, int bits, const FarSeg* __restrict__ segs,
             const int* __restrict__ seg_of, const int* __restrict__ flag,
             const double* __restrict__ X, const double* __restrict__ box,
             u64* __restrict__ keys, int* __restrict__ ids) {
  const long long i = (long long)blockIdx.x * kFarT + threadIdx.x;
  if (i >= N) return;
  const int f = seg_of[i];
  const size_t c = (size_t)segs[f].base + (size_t)(i - segs[f].fb);
  const u64 qmax = (1ull << bits) - 1;
  const double* bx = box + (size_t)f * (D + 1);
  const double scale = bx[D];
  u64 key = 0;
  if (flag[f]) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double t = (X[c * D + k] - bx[k]) * scale;
      const double fl = floor(t);
      u64 q = fl >= 0x1p63 ? qmax : (u64)fl;  // t >= 0: lo is the minimum
      q = q < qmax ? q : qmax;
      if constexpr (D == 1) {
        key = q;
      } else {
        for (int b = 0; b < bits; ++b) key |= ((q >> b) & 1ull) << (b * D + k);
      }
    }
  }
  keys[i] = ((u64)f << (bits * D)) | key;
  ids[i] = (int)i;
}

template <int D>
__global__ void __launch_bounds__(kFarT)
far_seg_gather(long long N, const FarSeg* __restrict__ segs, const int* __restrict__ seg_of,
               const int* __restrict__ permc, const double* __restrict__ X,
               const double* __restrict__ DP, double* __restrict__ rec, int* __restrict__ pos) {
  const long long p = (long long)blockIdx.x * kFarT + threadIdx.x;
  if (p >= N) return;
  const int f = seg_of[p];  // the sort keeps every segment in its range
  const int c = segs[f].base + (permc[p] - segs[f].fb);
#pragma unroll
  for (int k = 0; k < D; ++k) rec[(size_t)p * (D + 1) + k] = X[(size_t)c * D + k];
  rec[(size_t)p * (D + 1) + D] = DP[c];
  pos[p] = c;
}

template <int D>
__global__ void __launch_bounds__(kFarT)
far_seg_cells(int nranges, const int2* __restrict__ ranges, const double* __restrict__ rec,
              double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (kFarT / 64) + (threadIdx.x >> 6);
  if (q >= nranges) return;  // wave-uniform
  cell_summary<D>(rec, ranges[q].x, ranges[q].y, lane, out + (size_t)q * (D + 2));
}

__global__ void far_mass_check_rows(int nrows, const int* __restrict__ rows,
                                    const double* __restrict__ dp, int* __restrict__ bad) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nrows && !(dp[rows[q]] > 0.0 && finite_d(dp[rows[q]]))) atomicOr(bad, 1);
}

// far_repulse_kernel's walk inside the item's segment: cells and leaves are indexed
// within the segment, a 0 flag rejects every cell, and a row's sum goes to its P_T
// position.  counters as far_repulse_kernel's.
template <int D, int R>
__global__ void __launch_bounds__(kFarT)
far_seg_repulse_kernel(int nitems, const int4* __restrict__ itemd, const FarSeg* __restrict__ segs,
                       const int* __restrict__ flag, const double* __restrict__ cells,
                       const double* __restrict__ items, const double* __restrict__ rec,
                       const int* __restrict__ pos, double theta, double repel,
                       int* __restrict__ queue, u64* __restrict__ counters,
                       double* __restrict__ Frep) {
  constexpr int WV = rec_width(D);
  constexpr int CW = D + 2;
  constexpr int G = kFarGroup;
  __shared__ __attribute__((aligned(16))) double tiles[kFarT / 64][kFarLeaf * WV];
  __shared__ u64 wcnt[kFarT / 64][kFarMaxLevels + 2];
  const int lane = threadIdx.x & 63;
  double* tile = tiles[threadIdx.x >> 6];
  u64* cnt = wcnt[threadIdx.x >> 6];
  if (lane < kFarMaxLevels + 2) cnt[lane] = 0;
  for (;;) {
    int q = 0;
    if (lane == 0) q = atomicAdd(queue, 1);
    q = __builtin_amdgcn_readfirstlane(q);
    if (q >= nitems) break;
    const int4 it = itemd[q];
    const FarSeg* __restrict__ sg = segs + it.x;
    const int fb = sg->fb, s = sg->s;
    const int top = sg->nlev - 1;
    const int ntop = sg->cnt[top];
    const bool box_ok = flag[it.x] != 0;
    const int r0 = it.y, r1 = it.z;  // sorted rows of all segments: fb <= r0 < r1 <= fb + s
    double xi[R][D], di[R], acc[R][D];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int p = r0 + lane + kFarLeaf * r;
      const bool ok = p < r1;
      const size_t c = (size_t)(ok ? p : r0);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        xi[r][k] = ok ? rec[c * (D + 1) + k] : 0.0;
        acc[r][k] = 0.0;
      }
      di[r] = ok ? rec[c * (D + 1) + D] * repel : 0.0;
    }
    double cI[D];
#pragma unroll
    for (int k = 0; k < D; ++k) cI[k] = items[(size_t)q * CW + k];
    const double aI = items[(size_t)q * CW + D + 1];
    wave_lds_sync();  // cnt zeroed / the last item's counters read
    int l = top, idx = 0;
    u64 partners = 0;
    for (;;) {
      const double* cc = cells + ((size_t)sg->off[l] + (size_t)idx) * CW;
      double cC[D];
#pragma unroll
      for (int k = 0; k < D; ++k) cC[k] = cc[k];
      const double MC = cc[D], aC = cc[D + 1];
      double e = cI[0] - cC[0];
      double sq = e * e;
#pragma unroll
      for (int k = 1; k < D; ++k) {
        e = cI[k] - cC[k];
        sq = sq + e * e;
      }
      const double t = sqrt(sq) - aI;
      const bool take = __builtin_amdgcn_readfirstlane(
          (int)(box_ok && aC <= theta * t && t - aC >= kFaEps));
      if (take) {
#pragma unroll
        for (int r = 0; r < R; ++r) fast_rep_pair<D>(xi[r], cC, di[r], MC, acc[r]);
        if (lane == 0) cnt[l] += 1;
        partners += 1;
      } else if (l == 0) {
        const int j0 = idx * kFarLeaf;  // within the segment
        const int m = min(kFarLeaf, s - j0);
        wave_lds_sync();  // the previous leaf has been read by every lane
        {
          const size_t c = (size_t)fb + (size_t)min(j0 + lane, s - 1);
#pragma unroll
          for (int k = 0; k <= D; ++k) tile[lane * WV + k] = rec[c * (D + 1) + k];
        }
        wave_lds_sync();
        for (int jj = 0; jj < m; ++jj) {
          double xj[D];
#pragma unroll
          for (int k = 0; k < D; ++k) xj[k] = tile[jj * WV + k];
          const double dj = tile[jj * WV + D];
#pragma unroll
          for (int r = 0; r < R; ++r) fast_rep_pair<D>(xi[r], xj, di[r], dj, acc[r]);
        }
        if (lane == 0) cnt[kFarMaxLevels] += 1;
        partners += (u64)m;
      } else {
        l -= 1;
        idx *= G;
        continue;
      }
      // the next cell in walk order: the right sibling, else the parent's
      bool done = false;
      for (;;) {
        ++idx;
        if (l == top) {
          done = idx >= ntop;
          break;
        }
        if (idx % G == 0 || idx >= sg->cnt[l]) {
          idx = (idx - 1) / G;
          ++l;
          continue;
        }
        break;
      }
      if (done) break;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int p = r0 + lane + kFarLeaf * r;
      if (p < r1) {
        const size_t v = (size_t)pos[p];
#pragma unroll
        for (int k = 0; k < D; ++k) Frep[v * D + k] = acc[r][k];
      }
    }
    if (lane == 0) cnt[kFarMaxLevels + 1] = (partners - 1) * (u64)(r1 - r0);  // less the self pair
    wave_lds_sync();
    if (lane < kFarMaxLevels + 2) {
      const u64 v = cnt[lane];
      if (v) atomicAdd(&counters[lane], v);
      cnt[lane] = 0;
    }
  }
}

}  // namespace

FarSegEngine* far_seg_create(hipStream_t s, int dim, double theta, int item_rows, int cus,
                             const std::vector<int>& base, const std::vector<int>& size) {
  GE_REQUIRE(dim >= 1 && dim <= 4 && !base.empty() && base.size() == size.size(),
             "far field: bad segments or dim");
  GE_REQUIRE(item_rows == kFarLeaf || item_rows == 4 * kFarLeaf, "far field: items of 64 or 256 rows");
  GE_REQUIRE(base.size() < ((size_t)1 << kFarSegRankBits), "far field: too many segments");
  std::unique_ptr<FarSegEngine> e(new FarSegEngine());
  e->nseg = (int)base.size();
  e->dim = dim;
  e->cus = cus;
  e->theta = theta;
  e->R = item_rows / kFarLeaf;
  e->bits = far_seg_key_bits(dim);
  int rank_bits = 1;
  while (((size_t)1 << rank_bits) < base.size()) ++rank_bits;
  e->sort_bits = e->bits * dim + rank_bits;
  std::vector<int> h_seg_of;
  std::vector<int2> h_ranges, h_item_ranges;
  std::vector<int4> h_itemd;
  long long N = 0;
  for (int f = 0; f < e->nseg; ++f) {
    GE_REQUIRE(size[f] > 0 && base[f] >= 0, "far field: empty segment");
    N += size[f];
  }
  GE_REQUIRE(N <= 0x7fffffff - 4 * kFarLeaf, "far field: too many rows");
  e->N = N;
  h_seg_of.reserve((size_t)N);
  int fb = 0;
  for (int f = 0; f < e->nseg; ++f) {
    FarSeg g{};
    g.fb = fb;
    g.s = size[f];
    g.base = base[f];
    long long pts = kFarLeaf;
    int cnt = (g.s + kFarLeaf - 1) / kFarLeaf;
    for (int l = 0; l < kFarMaxLevels; ++l) {
      g.cnt[l] = cnt;
      g.off[l] = (int)h_ranges.size();
      g.nlev = l + 1;
      for (int q = 0; q < cnt; ++q) {
        const long long a = (long long)q * pts, b = std::min<long long>(g.s, a + pts);
        h_ranges.push_back(make_int2(fb + (int)a, fb + (int)b));
      }
      if (cnt <= kFarGroup) break;
      cnt = (cnt + kFarGroup - 1) / kFarGroup;
      pts *= kFarGroup;
    }
    e->item0.push_back((int)h_itemd.size());
    for (int r0 = 0; r0 < g.s; r0 += item_rows) {
      const int r1 = std::min(g.s, r0 + item_rows);
      h_itemd.push_back(make_int4(f, fb + r0, fb + r1, 0));
      h_item_ranges.push_back(make_int2(fb + r0, fb + r1));
    }
    h_seg_of.insert(h_seg_of.end(), (size_t)g.s, f);
    e->h_seg.push_back(g);
    fb += g.s;
  }
  e->item0.push_back((int)h_itemd.size());
  e->ncells = (int)h_ranges.size();
  e->nitems = (int)h_itemd.size();
  h_ranges.insert(h_ranges.end(), h_item_ranges.begin(), h_item_ranges.end());
  e->seg.alloc(e->nseg);
  e->seg.upload(e->h_seg.data(), e->h_seg.size(), s);
  e->seg_of.alloc((size_t)N);
  e->seg_of.upload(h_seg_of.data(), h_seg_of.size(), s);
  e->ranges.alloc(h_ranges.size());
  e->ranges.upload(h_ranges.data(), h_ranges.size(), s);
  e->itemd.alloc(h_itemd.size());
  e->itemd.upload(h_itemd.data(), h_itemd.size(), s);
  e->flag.alloc(e->nseg);
  e->box.alloc((size_t)e->nseg * (dim + 1));
  e->rec.alloc((size_t)N * (dim + 1));
  e->sums.alloc(h_ranges.size() * (dim + 2));
  e->keys_in.alloc((size_t)N);
  e->keys.alloc((size_t)N);
  e->ids.alloc((size_t)N);
  e->permc.alloc((size_t)N);
  e->pos.alloc((size_t)N);
  e->counters.alloc(kFarMaxLevels + 2);
  e->queue.alloc(1);
  GE_HIP(rocprim::radix_sort_pairs(nullptr, e->sort_bytes, e->keys_in.p, e->keys.p, e->ids.p,
                                   e->permc.p, (size_t)N, 0, e->sort_bits, s));
  e->sort_tmp.alloc(std::max<size_t>(e->sort_bytes, 1));
  for (hipEvent_t& ev : e->ev) GE_HIP(hipEventCreate(&ev));
  GE_HIP(hipMemsetAsync(e->counters.p, 0, sizeof(u64) * e->counters.n, s));
  GE_HIP(hipStreamSynchronize(s));  // the host tables are read by the uploads
  return e.release();
}

void far_seg_destroy(FarSegEngine* e) { delete e; }

bool far_seg_ran(const FarSegEngine* e) { return e->ran; }

bool far_masses_ok_rows(hipStream_t s, int nrows, const int* rows, const double* dp) {
  DevBuf<int> bad(1);
  int h = 0;
  GE_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), s));
  if (nrows > 0)
    hipLaunchKernelGGL(far_mass_check_rows, dim3(blocks_for(nrows)), dim3(kFarT), 0, s, nrows,
                       rows, dp, bad.p);
  GE_HIP(hipGetLastError());
  GE_HIP(hipMemcpyAsync(&h, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  GE_HIP(hipStreamSynchronize(s));
  return h == 0;
}

void far_seg_repulse(FarSegEngine* e, hipStream_t s, const double* X, const double* DP,
                     double repel, double* Frep) {
  const long long N = e->N;
  far_dim(e->dim, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    GE_HIP(hipEventRecord(e->ev[0], s));
    hipLaunchKernelGGL((far_seg_box<D>), dim3(e->nseg), dim3(kFarT), 0, s, e->seg.p, e->bits, X,
                       e->box.p, e->flag.p);
    hipLaunchKernelGGL((far_seg_keys<D>), dim3(blocks_for(N)), dim3(kFarT), 0, s, N, e->bits,
                       e->seg.p, e->seg_of.p, e->flag.p, X, e->box.p, e->keys_in.p, e->ids.p);
    GE_HIP(hipGetLastError());
    GE_HIP(rocprim::radix_sort_pairs(e->sort_tmp.p, e->sort_bytes, e->keys_in.p, e->keys.p,
                                     e->ids.p, e->permc.p, (size_t)N, 0, e->sort_bits, s));
    hipLaunchKernelGGL((far_seg_gather<D>), dim3(blocks_for(N)), dim3(kFarT), 0, s, N, e->seg.p,
                       e->seg_of.p, e->permc.p, X, DP, e->rec.p, e->pos.p);
    const int nranges = e->ncells + e->nitems;
    hipLaunchKernelGGL((far_seg_cells<D>), dim3(blocks_for((long long)nranges * 64)), dim3(kFarT),
                       0, s, nranges, e->ranges.p, e->rec.p, e->sums.p);
    GE_HIP(hipGetLastError());
    GE_HIP(hipMemsetAsync(e->queue.p, 0, sizeof(int), s));
    GE_HIP(hipMemsetAsync(e->counters.p, 0, sizeof(u64) * e->counters.n, s));
    GE_HIP(hipEventRecord(e->ev[1], s));
    const int waves = kFarT / 64;
    const int blocks = std::max(1, std::min(e->cus * 4, (e->nitems + waves - 1) / waves));
    const double* cells = e->sums.p;
    const double* items = e->sums.p + (size_t)e->ncells * (D + 2);
    auto go = [&](auto Rc) {
      constexpr int RC = decltype(Rc)::value;
      hipLaunchKernelGGL((far_seg_repulse_kernel<D, RC>), dim3(blocks), dim3(kFarT), 0, s,
                         e->nitems, e->itemd.p, e->seg.p, e->flag.p, cells, items, e->rec.p,
                         e->pos.p, e->theta, repel, e->queue.p, e->counters.p, Frep);
    };
    if (e->R == 4) go(std::integral_constant<int, 4>());
    else go(std::integral_constant<int, 1>());
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(e->ev[2], s));
    e->ran = true;
  });
}

void far_seg_info(FarSegEngine* e, hipStream_t s, double* theta, int* item_rows, int* key_bits,
                  int* segments, long long* rows, int* bad_boxes, long long* accepted,
                  long long* exact_leaves, long long* pair_terms, double* prep_ms,
                  double* item_ms) {
  GE_HIP(hipStreamSynchronize(s));
  if (theta) *theta = e->theta;
  if (item_rows) *item_rows = kFarLeaf * e->R;
  if (key_bits) *key_bits = e->bits;
  if (segments) *segments = e->nseg;
  if (rows) *rows = e->N;
  u64 h[kFarMaxLevels + 2] = {};
  int bad = 0;
  float a = 0.f, b = 0.f;
  if (e->ran) {
    std::vector<int> hf(e->nseg);
    GE_HIP(hipMemcpyAsync(h, e->counters.p, sizeof(h), hipMemcpyDeviceToHost, s));
    e->flag.download(hf.data(), hf.size(), s);
    GE_HIP(hipStreamSynchronize(s));
    for (int f : hf) bad += f == 0;
    GE_HIP(hipEventElapsedTime(&a, e->ev[0], e->ev[1]));
    GE_HIP(hipEventElapsedTime(&b, e->ev[1], e->ev[2]));
  }
  if (bad_boxes) *bad_boxes = bad;
  if (accepted)
    for (int l = 0; l < kFarMaxLevels; ++l) accepted[l] = (long long)h[l];
  if (exact_leaves) *exact_leaves = (long long)h[kFarMaxLevels];
  if (pair_terms) *pair_terms = (long long)h[kFarMaxLevels + 1];
  if (prep_ms) *prep_ms = a;
  if (item_ms) *item_ms = b;
}

void far_seg_shape(const FarSegEngine* e, int f, int* members, int* levels, int* level_cells,
                   int* items) {
  GE_REQUIRE(f >= 0 && f < e->nseg, "far field: no such segment");
  const FarSeg& g = e->h_seg[f];
  if (members) *members = g.s;
  if (levels) *levels = g.nlev;
  if (level_cells)
    for (int l = 0; l < kFarMaxLevels; ++l) level_cells[l] = l < g.nlev ? g.cnt[l] : 0;
  if (items) *items = e->item0[f + 1] - e->item0[f];
}

void far_seg_layout(FarSegEngine* e, hipStream_t s, int f, int* perm, unsigned long long* keys,
                    double* box, double* cells, double* items) {
  GE_REQUIRE(f >= 0 && f < e->nseg, "far field: no such segment");
  if (!e->ran) throw Error(GE_ERR_STATE, "far field: no pass has run");
  const FarSeg& g = e->h_seg[f];
  const int d = e->dim;
  GE_HIP(hipStreamSynchronize(s));
  if (perm) GE_HIP(hipMemcpyAsync(perm, e->pos.p + g.fb, sizeof(int) * g.s, hipMemcpyDeviceToHost, s));
  if (keys) GE_HIP(hipMemcpyAsync(keys, e->keys.p + g.fb, sizeof(u64) * g.s, hipMemcpyDeviceToHost, s));
  if (box)
    GE_HIP(hipMemcpyAsync(box, e->box.p + (size_t)f * (d + 1), sizeof(double) * (d + 1),
                          hipMemcpyDeviceToHost, s));
  if (cells) {  // a segment's levels are consecutive in `sums`
    int nc = 0;
    for (int l = 0; l < g.nlev; ++l) nc += g.cnt[l];
    GE_HIP(hipMemcpyAsync(cells, e->sums.p + (size_t)g.off[0] * (d + 2),
                          sizeof(double) * nc * (d + 2), hipMemcpyDeviceToHost, s));
  }
  if (items)
    GE_HIP(hipMemcpyAsync(items, e->sums.p + ((size_t)e->ncells + e->item0[f]) * (d + 2),
                          sizeof(double) * (e->item0[f + 1] - e->item0[f]) * (d + 2),
                          hipMemcpyDeviceToHost, s));
  GE_HIP(hipStreamSynchronize(s));
  if (perm)
    for (int p = 0; p < g.s; ++p) perm[p] -= g.base;  // position within the aggregate
  if (keys)  // the Morton part: the rank above it is the segment's
    for (int p = 0; p < g.s; ++p) keys[p] &= (1ull << (e->bits * d)) - 1;
}

}  // namespace ge

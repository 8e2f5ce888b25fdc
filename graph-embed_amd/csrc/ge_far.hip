// ge_far.hip -- GE_MODE_FARFIELD: a Barnes-Hut style far field for the single
// level's all-pairs repulsion (include/forceatlas.hpp:151-167), D = 1..4, fp64.
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

// One wave per cell of `csz` consecutive records: M = sum m_j, c = (sum m_j x_j) / M,
// a = (1 + 2^-40) sqrt(max_j sum_k (x_jk - c_k)^2).  Fixed order: a lane adds its records
// (lane, lane + 64, ...) ascending, then the xor butterfly 32, 16, .. 1, whose sums are
// the same bits on every lane.  The factor covers the roundings of the squared distance
// and of the root (a few 2^-53), so a is never below the exact max |x_j - c|.
template <int D>
__global__ void __launch_bounds__(kFarT)
far_cells(int n, long long csz, int ncell, const double* __restrict__ rec,
          double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * (kFarT / 64) + (threadIdx.x >> 6);
  if (cell >= ncell) return;  // wave-uniform
  const long long begin = (long long)cell * csz;
  const long long end = begin + csz < (long long)n ? begin + csz : (long long)n;
  double M = 0.0, sx[D];
#pragma unroll
  for (int k = 0; k < D; ++k) sx[k] = 0.0;
  for (long long j = begin + lane; j < end; j += 64) {
    const double m = rec[(size_t)j * (D + 1) + D];
    M = M + m;
#pragma unroll
    for (int k = 0; k < D; ++k) sx[k] = fma(m, rec[(size_t)j * (D + 1) + k], sx[k]);
  }
  for (int o = 32; o; o >>= 1) {
    M = M + __shfl_xor(M, o);
#pragma unroll
    for (int k = 0; k < D; ++k) sx[k] = sx[k] + __shfl_xor(sx[k], o);
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
  for (int o = 32; o; o >>= 1) s2 = fmax(s2, __shfl_xor(s2, o));
  if (lane == 0) {
    double* o = out + (size_t)cell * (D + 2);
#pragma unroll
    for (int k = 0; k < D; ++k) o[k] = c[k];
    o[D] = M;
    o[D + 1] = sqrt(s2) * (1.0 + 0x1p-40);
  }
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

}  // namespace ge

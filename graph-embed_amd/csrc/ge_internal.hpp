// ge_internal.hpp -- shared internals of libge.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "ge.h"

namespace ge {

// Error plumbing: internal code throws ge::Error; every extern "C" entry point
// catches it, records the message for ge_last_error() and returns the code.
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string& msg);

#define GE_HIP(call)                                                                  \
  do {                                                                                \
    hipError_t _e = (call);                                                           \
    if (_e != hipSuccess)                                                             \
      throw ::ge::Error(GE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e) + \
                                        " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

#define GE_REQUIRE(cond, msg)                                 \
  do {                                                        \
    if (!(cond)) throw ::ge::Error(GE_ERR_ARG, (msg));        \
  } while (0)

// GE_MODE_FARFIELD's parameter (include/ge.h); read in no other mode.
inline void check_far_params(const ge_fa_params& p) {
  if (p.mode != GE_MODE_FARFIELD) return;
  GE_REQUIRE(p.theta >= 0.0 && p.theta < 1.0,  // false for NaN
             "GE_MODE_FARFIELD: theta must be finite and in 0 <= theta < 1");
}
// The entry points without a far field (the multilevel level, embed, the sharded
// forms) run GE_MODE_FARFIELD as GE_MODE_FAST.
inline ge_fa_params far_as_fast(ge_fa_params p) {
  check_far_params(p);
  if (p.mode == GE_MODE_FARFIELD) p.mode = GE_MODE_FAST;
  return p;
}

template <class F>
int guarded(F&& f) {
  try {
    f();
    return GE_OK;
  } catch (const Error& e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::bad_alloc&) {
    set_last_error("host allocation failed");
    return GE_ERR_NOMEM;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return GE_ERR_STATE;
  }
}

// RAII device buffer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  explicit DevBuf(size_t count) { alloc(count); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) GE_HIP(hipMalloc(&p, count * sizeof(T)));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void upload(const T* h, size_t count, hipStream_t s) {
    if (count) GE_HIP(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void download(T* h, size_t count, hipStream_t s) const {
    if (count) GE_HIP(hipMemcpyAsync(h, p, count * sizeof(T), hipMemcpyDeviceToHost, s));
  }
};

// Profiling events: taken in groups (one per timed step, launch or pass), created a
// chunk at a time, reused from the start after reset().
struct EventPool {
  std::vector<hipEvent_t> ev;
  size_t next = 0, chunk;
  explicit EventPool(size_t chunk_) : chunk(chunk_) {}
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  // k consecutive events, valid until the next take()
  hipEvent_t* take(size_t k) {
    if (next + k > ev.size())
      for (size_t q = 0; q < chunk; ++q) {
        hipEvent_t e;
        GE_HIP(hipEventCreate(&e));
        ev.push_back(e);
      }
    next += k;
    return &ev[next - k];
  }
  void reset() { next = 0; }
  // Mean ms from event a to event b of the groups of `stride` taken since reset()
  // (all recorded and complete); groups: how many.
  double mean_ms(size_t stride, size_t a, size_t b, int* groups = nullptr) const {
    double t = 0.0;
    int cnt = 0;
    for (size_t k = 0; k + stride <= next; k += stride) {
      float x = 0.f;
      GE_HIP(hipEventElapsedTime(&x, ev[k + a], ev[k + b]));
      t += x;
      ++cnt;
    }
    if (groups) *groups = cnt;
    return cnt ? t / cnt : 0.0;
  }
};

inline int device_cus() {
  int dev = 0, cus = 0;
  GE_HIP(hipGetDevice(&dev));
  GE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return cus > 0 ? cus : 256;
}

// Device copy of a host CSR.
struct DevCsr {
  DevBuf<int> ip, ix;
  DevBuf<double> dx;
  int n = 0, nnz = 0;
  DevCsr(int rows, const int* hip_, const int* hix, const double* hdx, hipStream_t s)
      : ip(rows + 1), ix(hip_[rows] > 0 ? hip_[rows] : 1), dx(hip_[rows] > 0 ? hip_[rows] : 1),
        n(rows), nnz(hip_[rows]) {
    ip.upload(hip_, rows + 1, s);
    ix.upload(hix, nnz, s);
    dx.upload(hdx, nnz, s);
  }
};

// The scratch of a context's nearest-neighbour calls (ge_knn.hip), made by the first one.
struct KnnScratch;
void knn_release(KnnScratch* s);

}  // namespace ge

struct ge_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  // What the last call of each set-up step took (ge_ptap_info, ge_graph_info,
  // ge_radius_info): host values the calls have anyway, kept for the tests' census.
  struct {
    int bn = 0, bb = 0, ba = 0, split = GE_PTAP_SORT_NONE;
    long long entries = 0, runs = 0;
  } ptap;
  struct {
    long long chunk = 0;  // items per library sort or scan call (GE_GRAPH_CHUNK)
    int sort_segments = 0, scans = 0, scan_calls = 0;
  } graph;
  struct {
    int rounds = 0, max_pops = 0;
  } radius;
  int fa_batch[GE_FA_BATCH_TOTALS] = {0, 0, 0, 0};  // ge_fa_batch_info
  struct {  // ge_knn_info; the device path's insertions are read from the scratch
    int path = GE_KNN_PATH_NONE, form = GE_KNN_FORM_NARROW, rows_per_wg = 0, jsplit = 0;
    long long host_insertions = 0;
  } knn;
  ge::KnnScratch* knn_scratch = nullptr;
};

// A communicator (ge_dist.hip): RCCL, or a caller transport staged through host
// memory.  `nccl` is an ncclComm_t kept opaque here.
struct ge_comm {
  ge_ctx* ctx = nullptr;
  int nranks = 1, rank = 0;
  void* nccl = nullptr;
  ge_transport tp{};
};

namespace ge {
// Multi-GPU helpers (ge_dist.hip) used inside per-level plans.
void allgather_stream(ge_comm* c, hipStream_t s, const void* d_send, void* d_recv, size_t bytes);
void exchange_rows(ge_comm* c, hipStream_t s, int dim, const int* d_rows, const int* d_counts,
                   const int* d_first, const int* h_counts, const int* h_first, int width,
                   double* d_buf, double* d_x);
}  // namespace ge

// Host CSR (returned to callers through ge_csr*).
struct ge_csr {
  int rows = 0, cols = 0;
  std::vector<int> indptr, indices;
  std::vector<double> data;
};

struct ge_hier {
  std::vector<int> rows, cols;
  std::vector<std::vector<int>> indptr, indices;
  // which path built it (GE_PARTITION_PATH_*), its rounds, the lists rebuilt by
  // the device's wave / block / global kernels, and what the round loop ended
  // with: the alive vertices' adjacency and alpha by `used` slot
  int path = GE_PARTITION_PATH_HOST, rounds = 0;
  long long rebuilt[3] = {0, 0, 0};
  ge_partition_census census{};  // all zeros unless GE_PARTITION_CENSUS=1 (device paths)
  ge_csr final_adj;
  std::vector<double> final_alpha;
};

namespace ge {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(const ge_ctx* c) {
    GE_HIP(hipGetDevice(&prev));
    if (prev != c->device) GE_HIP(hipSetDevice(c->device));
  }
  ~DeviceGuard() {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0) (void)hipSetDevice(prev);
  }
};

// libstdc++ uniform_real_distribution<double>(-1,1) over mt19937(seed); written
// out explicitly (see ge_rng.cpp) and tested equal to std:: in tests.
void uniform_stream(unsigned seed, size_t count, double* out);
// Host CSR validation (indptr, index range); throws GE_ERR_ARG.
void check_csr(int n, const int* ip, const int* ix, const double* dx);

// Device entry points implemented in the .hip files, called by host drivers.
// One launch of the symmetric all-pairs repulsion (ge_sym.hpp, faml_sym_repulse)
// over `nunits` units {aggregate, row tile, progress offset, kind}; queue and
// prog zeroed by the caller.  Defined in ge_faml.hip, shared with single-level
// forceAtlas (ge_fa.hip).  sym_blocks_per_cu: the resident blocks it is sized for.
void sym_repulse_launch(int dim, int blocks, hipStream_t s, int nunits, const int4* units,
                        int* queue, const int* seg, const double* X, const double* DP,
                        double repel, double* F, double* H, size_t hs, int* prog, int* err,
                        long long limit);
int sym_blocks_per_cu(int dim);

void fa_run_device(ge_ctx* ctx, int n, int nnz, const int* d_ip, const int* d_ix,
                   const double* d_dx, int dim, double* d_x, int iterations,
                   const ge_fa_params& p);
// deg + 1 of n rows (degp1_kernel, ge_fa.hip) on stream s.
void launch_degp1(hipStream_t s, int n, const int* d_ip, const double* d_dx, int use_weights,
                  double* d_dp1);
// The device part of ge_force_atlas_batch on validated host arrays (ge_fa_batch.hip): the
// iterations of every graph of the block-diagonal CSR on X (N*dim, in/out) -- the wave
// and block launches, then the serial graphs through fa_run_device -- and the class
// totals into ctx->fa_batch.  The initial draw and normalize are the caller's.
void fa_batch_device(ge_ctx* ctx, int count, const int* off, const int* ip, const int* ix,
                     const double* dx, int dim, double* X, int iterations,
                     const ge_fa_params& p);
// The layout energy on a plan (ge_fa.hip over ge_energy.hip): the five columns of the
// plan's rows into d_rows (device; nullptr: the plan's own buffer, returned) on its
// stream, and the column sums of `rows` rows of d_rows into totals (host, 5;
// synchronises).  Both touch only the plan's energy scratch.
double* plan_energy_rows(ge_fa_plan* pl, const double* d_x, double* d_rows);
void plan_energy_totals(ge_fa_plan* pl, int rows, const double* d_rows, double* totals);
void faml_run_device(ge_ctx* ctx, int n, const int* d_ip, const int* d_ix, const double* d_dx,
                     int m, const int* h_pt_ip, const int* d_pt_ip, const int* d_pt_ix,
                     const int* d_vA, const double* d_cA, const double* d_rA,
                     const double* d_init, double* d_x, int dim, int iterations,
                     const ge_fa_params& p);
// single: the one-level overloads (src/partitioner.cpp:970-1544): no snapshots,
// one P_T over all n columns, and the loop also stops once M <= num_parts
// (num_parts <= 0: no target); cf is unused.
ge_hier* partition_incremental(int n, const int* I, const int* J, const double* Dv, double cf,
                               bool printing, bool positive, double stall, int matching,
                               bool single = false, int num_parts = 0);
// Device path (ge_partition_dev.hip); nullptr when the input needs the host path
// (a weight that is not finite or is -0.0, asymmetric A, rows not strictly ascending).
ge_hier* partition_device(ge_ctx* ctx, int n, const int* I, const int* J, const double* Dv,
                          double cf, bool printing, bool positive, double stall, int matching,
                          bool single = false, int num_parts = 0);
// Coarse rows [a0, a1) of P_T A P_T^T (a0 = 0, a1 = m: the whole matrix) into a
// host CSR of a1 - a0 rows and m columns.  h_pt_ip: P_T's indptr on the host.
void ptap_device(ge_ctx* ctx, int n, const int* d_ip, const int* d_ix, const double* d_dx,
                 int nnz, int m, const int* h_pt_ip, const int* d_pt_ip, const int* d_pt_ix,
                 int a0, int a1, ge_csr* out);

// Host-array drivers (ge_host.cpp) and their sharded forms (ge_dist.hip).
void fa_host(ge_ctx* ctx, int n, const int* ip, const int* ix, const double* dx, int dim,
             double* X, bool init_random, int iterations, const ge_fa_params& p);
void faml_host(ge_ctx* ctx, int n, const int* ip, const int* ix, const double* dx, int m,
               const int* pip, const int* pix, const int* vA, const double* cA,
               const double* rA, double* X, int dim, int iterations, const ge_fa_params& p);
void normalize_host(double* X, int n, int dim);
// radius step (src/embed.cpp:615-777): host replay of the serial event loop
// (ge_host.cpp) and the device rounds (ge_radius.hip; false: a zero distance,
// the caller must use the host version)
void radius_step_host(int m, double* cA, double* rA, int dim, bool base, int mc, const int* PIc,
                      const int* PJc, const double* cAc, const double* rAc, const int* AcI,
                      const int* AcJ);
bool radius_step_device(ge_ctx* ctx, int m, double* cA, double* rA, int dim, bool base, int mc,
                        const int* PIc, const int* PJc, const double* cAc, const double* rAc,
                        const int* AcI, const int* AcJ);
void fa_host_dist(ge_comm* comm, int n, const int* ip, const int* ix, const double* dx, int dim,
                  double* X, bool init_random, int iterations, const ge_fa_params& p);
void faml_host_dist(ge_comm* comm, int n, const int* ip, const int* ix, const double* dx, int m,
                    const int* pip, const int* pix, const int* vA, const double* cA,
                    const double* rA, double* X, int dim, int iterations,
                    const ge_fa_params& p);
// embedViaMinimization (ge_minimize.cpp) and one level of anyToMultilevel over it
// for the aggregates aggs[0..naggs) (nullptr: all), on the host; local_of[g] is
// g's position in its aggregate's member list.
void embed_via_minimization(int n, const int* I, const int* J, int dim, double* X,
                            bool init_random, unsigned seed, int iterations);
void minimize_ml_host(const int* I, const int* J, const int* PI, const int* PJ, const int* vA,
                      const int* local_of, const double* cA, const double* rA, int dim,
                      int iterations, double* coords, const int* aggs, int naggs);
// the embed orchestration (src/embed.cpp:561-796); comm == nullptr: one GPU
void embed_impl(ge_ctx* ctx, ge_comm* comm, int levels, const int* a_n, const int* a_off,
                const int* a_nz_off, const int* a_ip, const int* a_ix, const double* a_dx,
                const int* p_rows, const int* p_off, const int* p_nz_off, const int* p_ip,
                const int* p_ix, int dim, int base_iterations, int ml_iterations,
                int print_progress, const ge_fa_params& p, double* coords_out);

}  // namespace ge

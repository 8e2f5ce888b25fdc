// ge_knn.cpp -- the host side of include/ge.h's "layout neighbours": the host path of the
// exact k nearest neighbours (the plain double loop; the same bits as ge_knn.hip, this
// file being built with contraction off like the rest of the host code), the
// neighbourhood precision on top of either path, and the host-pointer entry points.
#include <cmath>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "ge_knn.hpp"

namespace ge {

// Query row q scans j = 0 .. n-1 as one chain: s < tau against the list's last s, tau
// starting at +inf, which is the whole candidate rule (ge_knn.hip).  Returns the
// insertions summed over the rows.
long long knn_host(int n, int dim, const double* x, int k, int n_rows, const int* rows, int* idx,
                   double* dist2) {
  const double inf = std::numeric_limits<double>::infinity();
  long long inserted = 0;
#pragma omp parallel for reduction(+ : inserted) schedule(dynamic, 16)
  for (int q = 0; q < n_rows; ++q) {
    const int i = rows ? rows[q] : q;
    double ls[GE_KNN_MAX_K];
    int lj[GE_KNN_MAX_K];
    for (int t = 0; t < k; ++t) {
      ls[t] = inf;
      lj[t] = -1;
    }
    const double* xi = x + (size_t)i * dim;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double* xj = x + (size_t)j * dim;
      const double e0 = xi[0] - xj[0];
      double s = e0 * e0;
      for (int c = 1; c < dim; ++c) {
        const double e = xi[c] - xj[c];
        s = std::fma(e, e, s);
      }
      if (!(s < ls[k - 1])) continue;
      int p = k - 1;
      while (p > 0 && ls[p - 1] > s) {
        ls[p] = ls[p - 1];
        lj[p] = lj[p - 1];
        --p;
      }
      ls[p] = s;
      lj[p] = j;
      ++inserted;
    }
    for (int t = 0; t < k; ++t) {
      idx[(size_t)q * k + t] = lj[t];
      if (dist2) dist2[(size_t)q * k + t] = ls[t];
    }
  }
  return inserted;
}

namespace {

void check_knn_args(int n, int dim, const double* coords, int k, const char* kname, int n_rows,
                    const int* rows) {
  GE_REQUIRE(dim >= 1 && dim <= kMaxDim, "dimension must be 1..16");
  GE_REQUIRE(k >= 1 && k <= GE_KNN_MAX_K, std::string(kname) + " must be 1..64");
  GE_REQUIRE(n >= 1, "n must be at least 1");
  GE_REQUIRE(n_rows >= 0, "n_rows must be >= 0");
  GE_REQUIRE(rows || n_rows == n, "n_rows must be n when no row list is given");
  GE_REQUIRE(coords, "null coordinates");
  for (int q = 0; rows && q < n_rows; ++q)
    GE_REQUIRE(rows[q] >= 0 && rows[q] < n,
               "row id " + std::to_string(rows[q]) + " at position " + std::to_string(q) +
                   " is outside 0.." + std::to_string(n - 1));
}

bool force_host() {
  const char* e = std::getenv("GE_KNN_HOST");
  return e && *e && *e != '0';
}

// ge_layout_knn on checked arguments.
void knn_any(ge_ctx* ctx, int n, int dim, const double* coords, int k, int n_rows, const int* rows,
             int* idx, double* dist2) {
  if (!ctx || force_host()) {
    const long long ins = knn_host(n, dim, coords, k, n_rows, rows, idx, dist2);
    if (ctx) {
      ctx->knn.path = GE_KNN_PATH_HOST;
      ctx->knn.form = dim <= kNarrowMaxDim ? GE_KNN_FORM_NARROW : GE_KNN_FORM_WIDE;
      ctx->knn.rows_per_wg = 0;
      ctx->knn.jsplit = 1;
      ctx->knn.host_insertions = ins;
    }
    return;
  }
  DeviceGuard g(ctx);
  hipStream_t s = ctx->stream;
  const size_t out = (size_t)n_rows * k;
  DevBuf<double> x((size_t)n * dim), d2(dist2 ? out : 0);
  DevBuf<int> r(rows ? n_rows : 0), ix(out);
  x.upload(coords, (size_t)n * dim, s);
  if (rows) r.upload(rows, n_rows, s);
  knn_device(ctx, n, dim, x.p, k, n_rows, rows ? r.p : nullptr, ix.p, dist2 ? d2.p : nullptr);
  ix.download(idx, out, s);
  if (dist2) d2.download(dist2, out, s);
  GE_HIP(hipStreamSynchronize(s));
}

}  // namespace
}  // namespace ge

extern "C" {

int ge_layout_knn(ge_ctx* ctx, int n, int dim, const double* coords, int k, int n_rows,
                  const int* rows, int* idx, double* dist2) {
  return ge::guarded([&] {
    ge::check_knn_args(n, dim, coords, k, "k", n_rows, rows);
    GE_REQUIRE(idx || n_rows == 0, "null idx");
    ge::knn_any(ctx, n, dim, coords, k, n_rows, rows, idx, dist2);
  });
}

int ge_layout_neighbourhood(ge_ctx* ctx, int n, const int* ip, const int* ix, int dim,
                            const double* coords, int kmax, int n_rows, const int* rows,
                            int* per_row, long long* totals) {
  return ge::guarded([&] {
    ge::check_knn_args(n, dim, coords, kmax, "kmax", n_rows, rows);
    GE_REQUIRE(ip && totals, "null indptr or totals");
    GE_REQUIRE(ip[0] == 0, "bad indptr: it must start at 0");
    for (int i = 0; i < n; ++i) {
      GE_REQUIRE(ip[i + 1] >= ip[i], "bad indptr: it decreases at row " + std::to_string(i));
      GE_REQUIRE(ip[i + 1] == ip[i] || ix, "null indices");
      for (int e = ip[i]; e < ip[i + 1]; ++e) {
        GE_REQUIRE(ix[e] >= 0 && ix[e] < n,
                   "row " + std::to_string(i) + " has a column outside 0.." + std::to_string(n - 1));
        GE_REQUIRE(e == ip[i] || ix[e - 1] <= ix[e],
                   "row " + std::to_string(i) + " is not ascending");
      }
    }
    std::vector<int> nb((size_t)n_rows * kmax);
    ge::knn_any(ctx, n, dim, coords, kmax, n_rows, rows, nb.data(), nullptr);
    long long t_rows = 0, t_k = 0, t_hits = 0;
#pragma omp parallel for reduction(+ : t_rows, t_k, t_hits) schedule(static)
    for (int q = 0; q < n_rows; ++q) {
      const int i = rows ? rows[q] : q;
      const int *b = ix + ip[i], *e = ix + ip[i + 1];
      int g = 0;  // distinct columns other than i: the row is ascending
      for (const int* c = b; c < e; ++c) g += *c != i && (c == b || c[-1] != *c);
      const int ki = g < kmax ? g : kmax;
      int hits = 0;
      for (int t = 0; t < ki; ++t) {
        const int j = nb[(size_t)q * kmax + t];
        if (j < 0) break;  // fewer candidates than k_i
        hits += std::binary_search(b, e, j);
      }
      if (per_row) {
        per_row[2 * (size_t)q] = ki;
        per_row[2 * (size_t)q + 1] = hits;
      }
      t_rows += ki > 0;
      t_k += ki;
      t_hits += hits;
    }
    totals[GE_NBHD_ROWS] = t_rows;
    totals[GE_NBHD_K] = t_k;
    totals[GE_NBHD_HITS] = t_hits;
  });
}

int ge_knn_info(const ge_ctx* ctx, int* path, int* form, int* rows_per_wg, int* jsplit,
                long long* insertions) {
  return ge::guarded([&] {
    GE_REQUIRE(ctx, "null context");
    if (path) *path = ctx->knn.path;
    if (form) *form = ctx->knn.form;
    if (rows_per_wg) *rows_per_wg = ctx->knn.rows_per_wg;
    if (jsplit) *jsplit = ctx->knn.jsplit;
    if (insertions)
      *insertions = ctx->knn.path == GE_KNN_PATH_DEVICE
                        ? ge::knn_device_insertions(ctx->knn_scratch)
                        : ctx->knn.host_insertions;
  });
}

}  // extern "C"

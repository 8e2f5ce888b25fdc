// ge_minimize.cpp -- partition::embedViaMinimization (src/embed.cpp:341-559),
// the reference's alternative single-level embedder: Gauss-Seidel sweeps over
// the vertices; for each vertex with a neighbour other than itself, a bisection
// line search (12 halvings of the step, from t = 1/2) towards each of the 2d
// unit directions on the energy sum_r 1/|x_i - x_r| + w sum_(i,r) |x_i - x_r|^2,
// w = 1e6, then a move to the direction of least energy.
//
// Host C++.  Inside one call the work per vertex is a chain of serial n-term
// sums whose order fixes the bits (the line search branches on their signs), so a
// single call stays on the host; the 2d directions of a vertex are independent and
// run on OpenMP threads.  A level of anyToMultilevel(embedViaMinimization) is a
// different matter: its aggregates are independent, and ge_minimize_dev.hip runs
// them as one batched device call.  minimize_ml_host below is that level's host
// twin (ctx == NULL, GE_MINIMIZE_HOST=1, inputs the device path does not take, and
// the aggregates beyond the device's LDS capacity).
// Every sum keeps the reference's order and operand grouping (-ffp-contract=off).

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "ge_internal.hpp"

namespace ge {

namespace {

constexpr double kMinEps = 10e-12;  // src/embed.cpp:345 (sic: 1e-11)
constexpr double kEdgeWeight = 1000000.0;  // :415

struct LineResult {
  double t, J;
};

// Line search from x_i towards direction s (:417-494) and the energy at its end.
LineResult line_search(int i, int n, int dim, const int* I, const int* J, const double* X,
                       const double* xs) {
  const double* xi = X + (size_t)i * dim;
  double t = 0.5;
  double jump = 0.25;
  do {
    double dJ = 0.0;
    for (int r = 0; r < n; ++r) {
      if (i == r) continue;
      const double* xr = X + (size_t)r * dim;
      double term1 = 0.0, term2 = 0.0;
      for (int k = 0; k < dim; ++k) {
        const double u = xs[k] - xi[k];
        const double v = xi[k] - xr[k];
        const double z = u * t + v;
        term1 = term1 + z * z;
        term2 = term2 + z * u;
      }
      if (term1 < kMinEps) term1 = kMinEps;
      dJ += -((1.0 / std::sqrt(term1 * term1 * term1)) * term2);
    }
    for (int kk = I[i]; kk < I[i + 1]; ++kk) {
      const int r = J[kk];
      if (i == r) continue;
      const double* xr = X + (size_t)r * dim;
      double term = 0.0;
      for (int k = 0; k < dim; ++k) {
        const double a = (1 - t) * xi[k] + t * xs[k] - xr[k];
        term += kEdgeWeight * 2.0 * a * (xs[k] - xi[k]);
      }
      dJ += term;
    }
    if (dJ < 0.0) t = t + jump;
    else t = t - jump;
    jump = jump / 2.0;
  } while (jump > 1.e-4);
  double Jl = 0.0;  // :496-523
  for (int r = 0; r < n; ++r) {
    if (i == r) continue;
    const double* xr = X + (size_t)r * dim;
    double term1 = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double u = xs[k] - xi[k];
      const double v = xi[k] - xr[k];
      const double z = u * t + v;
      term1 = term1 + z * z;
    }
    if (term1 < kMinEps) term1 = kMinEps;
    Jl = Jl + 1.0 / std::sqrt(term1);
  }
  for (int kk = I[i]; kk < I[i + 1]; ++kk) {
    const int r = J[kk];
    if (i == r) continue;
    const double* xr = X + (size_t)r * dim;
    double term = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double a = (1 - t) * xi[k] + t * xs[k] - xr[k];
      term += a * a;
    }
    Jl += kEdgeWeight * term;
  }
  return {t, Jl};
}

}  // namespace

void embed_via_minimization(int n, const int* I, const int* J, int dim, double* X,
                            bool init_random, unsigned seed, int iterations) {
  if (init_random) uniform_stream(seed, (size_t)n * dim, X);  // :353-361, i-major
  // directions (:363-379): +e_k, -e_k for k = 0..d-1 (the d = 2, 3 lists are this order)
  const int ndir = 2 * dim;
  std::vector<double> dirs((size_t)ndir * dim, 0.0);
  for (int k = 0; k < dim; ++k) {
    dirs[(size_t)(2 * k) * dim + k] = 1;
    dirs[(size_t)(2 * k + 1) * dim + k] = -1;
  }
  std::vector<LineResult> res(ndir);
  for (int iter = 0; iter < iterations; ++iter) {
    for (int i = 0; i < n; ++i) {
      int count = 0;  // :389-394
      for (int kk = I[i]; kk < I[i + 1]; ++kk)
        if (J[kk] != i) count++;
      if (count == 0) continue;
#pragma omp parallel for schedule(static, 1) if (n > 64)
      for (int s = 0; s < ndir; ++s)
        res[s] = line_search(i, n, dim, I, J, X, dirs.data() + (size_t)s * dim);
      double min_J = std::numeric_limits<double>::infinity();
      double min_t = 0.0f;
      double min_s = -1;
      for (int s = 0; s < ndir; ++s) {  // :524-528, in direction order
        if (res[s].J < min_J) {
          min_J = res[s].J;
          min_t = res[s].t;
          min_s = s;
        }
      }
      if (min_s >= 0) {  // :554-558
        const double* ds = dirs.data() + (size_t)min_s * dim;
        for (int k = 0; k < dim; ++k)
          X[(size_t)i * dim + k] = X[(size_t)i * dim + k] * (1 - min_t) + ds[k] * min_t;
      }
    }
  }
  if (n > 1) {  // :562-583: centre on the mean of vertices 1..n-1, scale by their max norm
    std::vector<double> avg(dim, 0.0);
    for (int i = 1; i < n; ++i)
      for (int k = 0; k < dim; ++k) avg[k] = avg[k] + X[(size_t)i * dim + k];
    for (int k = 0; k < dim; ++k) avg[k] = avg[k] / (n - 1);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < dim; ++k) X[(size_t)i * dim + k] -= avg[k];
    double max_length = 0.0;
    for (int i = 1; i < n; ++i) {
      double acc = 0.0;  // magnitude (include/forceatlas.hpp:80-87)
      for (int k = 0; k < dim; ++k) acc = acc + X[(size_t)i * dim + k] * X[(size_t)i * dim + k];
      const double len = std::sqrt(acc);
      if (max_length < len) max_length = len;
    }
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < dim; ++k) X[(size_t)i * dim + k] = X[(size_t)i * dim + k] / max_length;
  }
}

// anyToMultilevel(embedViaMinimization) (src/embed.cpp:23-83) for the aggregates
// aggs[0..naggs) (aggs == nullptr: all m).  Per aggregate a: the members' internal
// edges as an r x r pattern (columns sorted, duplicates merged, as the reference's
// CooMatrix::ToSparse leaves them), `iterations` sweeps from a zero start, the
// result normalised by its largest norm and placed in a's ball.  local_of[g]: g's
// position in its aggregate's member list.
void minimize_ml_host(const int* I, const int* J, const int* PI, const int* PJ, const int* vA,
                      const int* local_of, const double* cA, const double* rA, int dim,
                      int iterations, double* coords, const int* aggs, int naggs) {
  auto one = [&](int a) {
    const int* v = PJ + PI[a];
    const int r = PI[a + 1] - PI[a];
    std::vector<int> ci(r + 1, 0), cj, cols;
    for (int i = 0; i < r; ++i) {
      cols.clear();
      for (int kk = I[v[i]]; kk < I[v[i] + 1]; ++kk)
        if (vA[J[kk]] == a) cols.push_back(local_of[J[kk]]);
      std::sort(cols.begin(), cols.end());
      cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
      cj.insert(cj.end(), cols.begin(), cols.end());
      ci[i + 1] = (int)cj.size();
    }
    std::vector<double> X((size_t)r * dim, 0.0);
    embed_via_minimization(r, ci.data(), cj.data(), dim, X.data(), false, 0, iterations);
    double mx = 0.0;
    for (int i = 0; i < r; ++i) {
      double acc = 0.0;  // magnitude (include/forceatlas.hpp:80-87)
      for (int k = 0; k < dim; ++k) acc += X[(size_t)i * dim + k] * X[(size_t)i * dim + k];
      const double mg = std::sqrt(acc);
      if (mg > mx) mx = mg;
    }
    for (int i = 0; i < r; ++i)
      for (int k = 0; k < dim; ++k)
        coords[(size_t)v[i] * dim + k] =
            cA[(size_t)a * dim + k] + rA[a] * (X[(size_t)i * dim + k] / mx);
  };
  // aggregates are independent: the small ones (whose calls are serial inside) run
  // on OpenMP threads, the others one after another with their directions on threads
  std::vector<int> small, large;
  for (int q = 0; q < naggs; ++q) {
    const int a = aggs ? aggs[q] : q;
    (PI[a + 1] - PI[a] > 64 ? large : small).push_back(a);
  }
  for (int a : large) one(a);
#pragma omp parallel for schedule(dynamic, 1)
  for (size_t q = 0; q < small.size(); ++q) one(small[q]);
}

}  // namespace ge

extern "C" int ge_embed_via_minimization(int n, const int* indptr, const int* indices, int dim,
                                         double* coords, int init_random, unsigned seed,
                                         int iterations) {
  return ge::guarded([&] {
    GE_REQUIRE(n >= 0 && dim >= 1 && iterations >= 0, "bad arguments");
    GE_REQUIRE(n == 0 || (indptr && indices && coords && indptr[0] == 0), "null argument");
    ge::embed_via_minimization(n, indptr, indices, dim, coords, init_random != 0, seed,
                               iterations);
  });
}

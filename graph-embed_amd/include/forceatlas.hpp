// Drop-in for include/forceatlas.hpp (LLNL/graph-embed).  Same names, parameter
// order and defaults; the iterations run on the MI355X through libge.so.
//   forceAtlas(A, dim, coords, ...)        include/forceatlas.hpp:89-305
//   forceAtlas(A, dim = 2)                 :307-312 (100000 iterations)
//   forceAtlasMultilevel(A, P, v_A, ...)   :314-574
// Differences: the random init uses mt19937(seed) (partition::setSeed / $GE_SEED)
// instead of std::random_device, and forceAtlasMultilevel draws in the
// reference's single-thread order (the reference races on its generator across
// OpenMP threads, :340-358).  The functions are inline (the reference defines
// them non-inline in this header).  partition::setMode(GE_MODE_FAST | GE_MODE_FARFIELD)
// / $GE_MODE=fast | farfield (the latter with partition::setTheta / $GE_THETA) selects
// a tolerance mode of include/ge.h; the default is the reference's bits.
#ifndef FORCEATLAS_HPP
#define FORCEATLAS_HPP

#include <array>
#include <cassert>
#include <cmath>
#include <vector>

#include "ge_dropin.hpp"
#include "matrixutils.hpp"

namespace partition {

inline double abs(double val) { return (val < 0) ? -val : val; }

inline double distance(const std::vector<double>& v1, const std::vector<double>& v2) {
  assert(v1.size() == v2.size());
  double acc = 0.0;
  for (size_t k = 0; k < v1.size(); ++k) {
    const double t = v2[k] - v1[k];
    acc += t * t;
  }
  return std::sqrt(acc);
}

inline double magnitude(const std::vector<double>& v) {
  double acc = 0.0;
  for (double x : v) acc += x * x;
  return std::sqrt(acc);
}

inline void forceAtlas(const SparseMatrix& A, const int dim,
                       std::vector<std::vector<double>>& coords, const int iterations = 100000,
                       const double ks = 0.1, const double ksmax = 1.0, const double repel = 1.0,
                       const double attract = 1.0, const double gravity = 1.0,
                       const bool useWeights = true, const bool linlog = false,
                       const bool nohubs = false, const double delta = 1.0,
                       const double tolerate = 1.0, const bool normalize = false) {
  ge_fa_params p;
  ge_fa_params_default(&p);
  p.ks = ks;
  p.ksmax = ksmax;
  p.repel = repel;
  p.attract = attract;
  p.gravity = gravity;
  p.use_weights = useWeights;
  p.linlog = linlog;
  p.nohubs = nohubs;
  p.delta = delta;
  p.tolerate = tolerate;
  p.normalize = normalize;
  p.seed = detail::seed_ref();
  p.mode = detail::mode_ref();
  p.theta = detail::theta_ref();
  const int n = A.Rows();
  const bool init = coords.empty();
  std::vector<double> X = detail::flatten(coords, n, dim);
  detail::check(ge_force_atlas(detail::context(), n, A.GetIndptr().data(),
                               A.GetIndices().data(), A.GetData().data(), dim, X.data(),
                               init ? 1 : 0, iterations, &p));
  detail::unflatten(X, n, dim, coords);
}

inline std::vector<std::vector<double>> forceAtlas(const SparseMatrix& A, const int dim = 2) {
  std::vector<std::vector<double>> coords(0);
  forceAtlas(A, dim, coords);
  return coords;
}

// An addition: the reference has no such function.  forceAtlas on every graph of `As` in
// one device call (ge_force_atlas_batch): coords[g] ends with the bits of
// forceAtlas(As[g], dim, coords[g], ...) alone.  An empty coords draws every graph's
// start from mt19937(seed), as forceAtlas does for an empty coords; otherwise it holds
// one n_g x dim start per graph.
inline void forceAtlasBatch(const std::vector<SparseMatrix>& As, const int dim,
                            std::vector<std::vector<std::vector<double>>>& coords,
                            const int iterations = 100000, const double ks = 0.1,
                            const double ksmax = 1.0, const double repel = 1.0,
                            const double attract = 1.0, const double gravity = 1.0,
                            const bool useWeights = true, const bool linlog = false,
                            const bool nohubs = false, const double delta = 1.0,
                            const double tolerate = 1.0, const bool normalize = false) {
  ge_fa_params p;
  ge_fa_params_default(&p);
  p.ks = ks;
  p.ksmax = ksmax;
  p.repel = repel;
  p.attract = attract;
  p.gravity = gravity;
  p.use_weights = useWeights;
  p.linlog = linlog;
  p.nohubs = nohubs;
  p.delta = delta;
  p.tolerate = tolerate;
  p.normalize = normalize;
  p.seed = detail::seed_ref();
  p.mode = detail::mode_ref();
  p.theta = detail::theta_ref();
  const int count = (int)As.size();
  const bool init = coords.empty();
  if (!init && (int)coords.size() != count)
    throw std::invalid_argument("forceAtlasBatch: one coordinate set per graph");
  std::vector<int> off(count + 1, 0), ip(1, 0), ix;
  std::vector<double> dx, X;
  for (int g = 0; g < count; ++g) {
    const SparseMatrix& A = As[g];
    const int n = A.Rows(), e0 = (int)ix.size();
    for (int i = 0; i < n; ++i) ip.push_back(e0 + A.GetIndptr()[i + 1]);
    for (int j : A.GetIndices()) ix.push_back(off[g] + j);
    dx.insert(dx.end(), A.GetData().begin(), A.GetData().end());
    off[g + 1] = off[g] + n;
    const std::vector<double> x =
        init ? std::vector<double>((size_t)n * dim) : detail::flatten(coords[g], n, dim);
    X.insert(X.end(), x.begin(), x.end());
  }
  if (ix.empty()) {  // the ABI wants arrays
    ix.push_back(0);
    dx.push_back(0.0);
  }
  if (X.empty()) X.push_back(0.0);
  detail::check(ge_force_atlas_batch(detail::context(), count, off.data(), ip.data(), ix.data(),
                                     dx.data(), dim, X.data(), init ? 1 : 0, nullptr, iterations,
                                     &p));
  coords.resize(count);
  for (int g = 0; g < count; ++g) {
    const std::vector<double> x(X.begin() + (size_t)off[g] * dim,
                                X.begin() + (size_t)off[g + 1] * dim);
    detail::unflatten(x, off[g + 1] - off[g], dim, coords[g]);
  }
}

inline void forceAtlasMultilevel(const SparseMatrix& A, const SparseMatrix& P,
                                 const std::vector<int>& v_A,
                                 const std::vector<std::vector<double>>& coords_A,
                                 const std::vector<double>& r_A,
                                 std::vector<std::vector<double>>& coords, int dim = 2,
                                 int iterations = 10, double ks = 0.1, double ksmax = 1.0,
                                 bool useWeights = true, bool linlog = false, bool nohubs = false,
                                 double repel = 1.0, double attract = 1.0, double gravity = 1.0,
                                 double delta = 1.0, double tolerate = 1.0) {
  ge_fa_params p;
  ge_fa_params_default(&p);
  p.ks = ks;
  p.ksmax = ksmax;
  p.use_weights = useWeights;
  p.linlog = linlog;
  p.nohubs = nohubs;
  p.repel = repel;
  p.attract = attract;
  p.gravity = gravity;
  p.delta = delta;
  p.tolerate = tolerate;
  p.seed = detail::seed_ref();
  p.mode = detail::mode_ref();
  p.theta = detail::theta_ref();
  const int n = A.Rows();
  const int m = P.Rows();
  std::vector<double> cA = detail::flatten(coords_A, m, dim);
  std::vector<double> X((size_t)n * dim, 0.0);
  detail::check(ge_force_atlas_ml(detail::context(), n, A.GetIndptr().data(),
                                  A.GetIndices().data(), A.GetData().data(), m,
                                  P.GetIndptr().data(), P.GetIndices().data(), v_A.data(),
                                  cA.data(), r_A.data(), X.data(), dim, iterations, &p));
  detail::unflatten(X, n, dim, coords);
}

// An addition: the reference has no such function.  The layout energy of include/ge.h
// ("layout energy") of the coordinates on graph A: the totals {REP, ATT, GRAV, PAIRDIST,
// EDGELEN} (GE_ENERGY_*), E = [0] + [1] + [2]; -dE/dx is forceAtlas's force for a
// symmetric A with nohubs = false.  Parameters and defaults are forceAtlas's.
inline std::array<double, GE_ENERGY_COLS> layoutEnergy(
    const SparseMatrix& A, const std::vector<std::vector<double>>& coords, const double repel = 1.0,
    const double attract = 1.0, const double gravity = 1.0, const bool useWeights = true,
    const bool linlog = false, const bool nohubs = false, const double delta = 1.0) {
  ge_fa_params p;
  ge_fa_params_default(&p);
  p.repel = repel;
  p.attract = attract;
  p.gravity = gravity;
  p.use_weights = useWeights;
  p.linlog = linlog;
  p.nohubs = nohubs;
  p.delta = delta;
  const int n = A.Rows();
  const int dim = coords.empty() ? 0 : (int)coords[0].size();
  std::vector<double> X = detail::flatten(coords, n, dim);
  std::array<double, GE_ENERGY_COLS> totals{};
  detail::check(ge_layout_energy(detail::context(), n, A.GetIndptr().data(),
                                 A.GetIndices().data(), A.GetData().data(), dim, X.data(), &p,
                                 nullptr, totals.data()));
  return totals;
}

// An addition: the reference has no such function.  The exact k nearest neighbours of
// every vertex in the layout ("layout neighbours" in include/ge.h), row i in ascending
// order of (squared distance, index); -1 past the last candidate.  1 <= k <= GE_KNN_MAX_K.
inline std::vector<std::vector<int>> layoutNeighbours(
    const std::vector<std::vector<double>>& coords, const int k) {
  const int n = (int)coords.size();
  const int dim = coords.empty() ? 0 : (int)coords[0].size();
  std::vector<double> X = detail::flatten(coords, n, dim);
  std::vector<int> idx((size_t)n * (k > 0 ? k : 0));
  detail::check(ge_layout_knn(detail::context(), n, dim, X.data(), k, n, nullptr, idx.data(),
                              nullptr));
  std::vector<std::vector<int>> out(n);
  for (int i = 0; i < n; ++i)  // check() has thrown unless 1 <= k
    out[i].assign(idx.begin() + (size_t)i * k, idx.begin() + (size_t)(i + 1) * k);
  return out;
}

// An addition.  The neighbourhood precision of the layout on graph A (ascending rows):
// the totals {rows with a neighbour, sum k_i, sum hits_i} (GE_NBHD_*) over all vertices,
// k_i = min(distinct neighbours of i, kmax); the pooled score is [2] / [1].
inline std::array<long long, GE_NBHD_TOTALS> neighbourhoodPrecision(
    const SparseMatrix& A, const std::vector<std::vector<double>>& coords, const int kmax = 16) {
  const int n = A.Rows();
  const int dim = coords.empty() ? 0 : (int)coords[0].size();
  std::vector<double> X = detail::flatten(coords, n, dim);
  std::array<long long, GE_NBHD_TOTALS> totals{};
  detail::check(ge_layout_neighbourhood(detail::context(), n, A.GetIndptr().data(),
                                        A.GetIndices().data(), dim, X.data(), kmax, n, nullptr,
                                        nullptr, totals.data()));
  return totals;
}

}  // namespace partition

#endif  // FORCEATLAS_HPP

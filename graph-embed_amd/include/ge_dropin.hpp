// ge_dropin.hpp -- glue between the reference's C++ API (namespace partition)
// and libge.so's C ABI (include/ge.h).  Header-only: the drop-in headers touch a
// SparseMatrix only through GetIndptr/GetIndices/GetData/Rows/Cols and the
// (I, J, D, rows, cols) constructor, so they build against the real linalgcpp
// or against the subset in graph-embed_amd/compat.
#ifndef GE_DROPIN_HPP
#define GE_DROPIN_HPP

#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "ge.h"

namespace partition {
namespace detail {

// Non-zero status -> exception.  The reference has no error reporting beyond
// assert; an uncaught exception terminates like a failed assert does.
inline void check(int rc) {
  if (rc != 0) throw std::runtime_error(std::string("graph-embed_amd: ") + ge_last_error());
}

// One context (device + stream) per host thread, device from $GE_DEVICE.
struct CtxHolder {
  ge_ctx* c = nullptr;
  ~CtxHolder() {
    if (c) ge_ctx_destroy(c);
  }
};

inline ge_ctx* context() {
  thread_local CtxHolder h;
  if (!h.c) {
    const char* d = std::getenv("GE_DEVICE");
    check(ge_ctx_create(d ? std::atoi(d) : 0, &h.c));
  }
  return h.c;
}

// The reference seeds every generator from std::random_device; the drop-in
// uses one fixed seed per thread ($GE_SEED, default 12345; partition::setSeed).
inline unsigned& seed_ref() {
  thread_local unsigned s = [] {
    const char* e = std::getenv("GE_SEED");
    return e ? (unsigned)std::strtoul(e, nullptr, 10) : 12345u;
  }();
  return s;
}

// The reference has one arithmetic; the drop-in runs GE_MODE_STRICT unless this
// thread asks for GE_MODE_FAST or GE_MODE_FARFIELD ($GE_MODE = strict | fast |
// farfield, default strict; partition::setMode).  Anything else in $GE_MODE is an
// error, not a silent default.
inline int& mode_ref() {
  thread_local int m = [] {
    const char* e = std::getenv("GE_MODE");
    if (!e || !*e || std::string(e) == "strict") return GE_MODE_STRICT;
    if (std::string(e) == "fast") return GE_MODE_FAST;
    if (std::string(e) == "farfield") return GE_MODE_FARFIELD;
    throw std::runtime_error("graph-embed_amd: GE_MODE must be strict, fast or farfield");
  }();
  return m;
}

// GE_MODE_FARFIELD's opening parameter ($GE_THETA, default the library's 0.5;
// partition::setTheta): finite, 0 <= theta < 1, anything else is an error.
inline double checked_theta(double t) {
  if (!(t >= 0.0 && t < 1.0))
    throw std::invalid_argument("graph-embed_amd: theta must be finite and in 0 <= theta < 1");
  return t;
}
inline double& theta_ref() {
  thread_local double t = [] {
    const char* e = std::getenv("GE_THETA");
    if (!e || !*e) {
      ge_fa_params p;
      ge_fa_params_default(&p);
      return p.theta;
    }
    char* end = nullptr;
    const double v = std::strtod(e, &end);
    if (end == e || *end) throw std::invalid_argument("graph-embed_amd: GE_THETA is not a number");
    return checked_theta(v);
  }();
  return t;
}

inline std::vector<double> flatten(const std::vector<std::vector<double>>& c, int n, int dim) {
  std::vector<double> out((size_t)n * dim, 0.0);
  for (int i = 0; i < n && i < (int)c.size(); ++i)
    for (int k = 0; k < dim && k < (int)c[i].size(); ++k) out[(size_t)i * dim + k] = c[i][k];
  return out;
}

inline void unflatten(const std::vector<double>& x, int n, int dim,
                      std::vector<std::vector<double>>& c) {
  c.assign(n, std::vector<double>(dim));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) c[i][k] = x[(size_t)i * dim + k];
}

template <class M>
inline std::vector<int> vertex_of(const M& P_T) {  // P_T.Transpose().GetIndices()
  std::vector<int> v(P_T.Cols(), 0);
  const auto& I = P_T.GetIndptr();
  const auto& J = P_T.GetIndices();
  for (int a = 0; a < P_T.Rows(); ++a)
    for (int c = I[a]; c < I[a + 1]; ++c) v[J[c]] = a;
  return v;
}

template <class M>
inline M from_ge_csr(ge_csr* c) {
  int rows = 0, cols = 0;
  long long nnz = 0;
  check(ge_csr_shape(c, &rows, &cols, &nnz));
  std::vector<int> I(rows + 1), J((size_t)nnz);
  std::vector<double> D((size_t)nnz);
  check(ge_csr_copy(c, I.data(), J.data(), D.data()));
  ge_csr_free(c);
  return M(I, J, D, rows, cols);
}

}  // namespace detail

// Extension: fix the seed that replaces std::random_device in this thread.
inline void setSeed(unsigned seed) { detail::seed_ref() = seed; }

// Extension: GE_MODE_STRICT (the default, the reference's bits), GE_MODE_FAST or
// GE_MODE_FARFIELD (include/ge.h) for forceAtlas, forceAtlasMultilevel, embed and
// embedMultilevel called from this thread.
inline void setMode(int mode) {
  if (mode != GE_MODE_STRICT && mode != GE_MODE_FAST && mode != GE_MODE_FARFIELD)
    throw std::invalid_argument(
        "graph-embed_amd: setMode takes GE_MODE_STRICT, GE_MODE_FAST or GE_MODE_FARFIELD");
  detail::mode_ref() = mode;
}

// Extension: GE_MODE_FARFIELD's opening parameter for calls from this thread.
inline void setTheta(double theta) { detail::theta_ref() = detail::checked_theta(theta); }

}  // namespace partition

#endif  // GE_DROPIN_HPP

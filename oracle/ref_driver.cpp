/*
 * ref_driver.cpp -- command-line front end of oracle/_ref/ge_ref, the binary
 * that oracle/Makefile links from the reference's own translation units
 * (LLNL/graph-embed src/partitioner.cpp, src/embed.cpp, src/matrixutils.cpp)
 * and this file, against graph-embed_amd/compat/ for linalgcpp.
 *
 * TEST INFRASTRUCTURE ONLY (tests/ref_lib.py runs it).  Everything computed
 * here is computed by the reference's code; this file only moves arrays between
 * binary files and the reference's C++ types.
 *
 *   ge_ref <subcommand> key=value ...
 *
 * Every key of a subcommand is required (no defaults are restated here).
 * Common keys: threads (omp_set_num_threads), seed (what every
 * std::random_device of the reference returns, see ref_shim.hpp), out.
 *
 * File formats (little-endian, as tests/test_dropin.py:write_csr):
 *   CSR     int32 rows, nnz; int32 indptr[rows+1]; int32 indices[nnz]; f64 data[nnz]
 *           A matrices are square; a P_T has one entry per column, so cols = nnz.
 *   coords  f64[n*dim], vertex-major;  ints  int32[];  reals  f64[]
 *   hier    int32 L; L+1 CSRs As[0..L]; L CSRs P_Ts[0..L-1]
 *
 *   fa          A start(- = seeded) dim iterations ks ksmax repel attract gravity
 *               use_weights linlog nohubs delta tolerate normalize   -> coords
 *   ml          A PT vA cA rA dim iterations ks ksmax use_weights linlog nohubs
 *               repel attract gravity delta tolerate                 -> coords
 *   partition   A mode(cf|parts|single) value positive_merging stall matching
 *               merge_leaves                         -> int32 count; count CSRs
 *   modularity  A PT                                                 -> f64
 *   interp      sets(CSR whose rows are the sets) cols               -> CSR
 *   embed       hier dim                                             -> coords
 *   minimize    A start(- = seeded, the empty-coords branch; default = the
 *               two-argument overload, which ignores iterations) dim iterations
 *                                                                    -> coords
 *   minimize_ml hier dim                                             -> coords
 *   laplacian   A                 -> CSRs identity, toLaplacian, fromLaplacian(L)
 */
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "embed.hpp"
#include "matrixutils.hpp"
#include "partitioner.hpp"

unsigned ge_ref_seed = 0;

/* include/forceatlas.hpp defines its functions non-inline and src/embed.cpp
 * already includes it, so the two entry points are declared here instead. */
namespace partition {
void forceAtlas(const SparseMatrix& A, int dim, std::vector<std::vector<double>>& coords,
                int iterations, double ks, double ksmax, double repel, double attract,
                double gravity, bool useWeights, bool linlog, bool nohubs, double delta,
                double tolerate, bool normalize);
void forceAtlasMultilevel(const SparseMatrix& A, const SparseMatrix& P,
                          const std::vector<int>& v_A,
                          const std::vector<std::vector<double>>& coords_A,
                          const std::vector<double>& r_A,
                          std::vector<std::vector<double>>& coords, int dim, int iterations,
                          double ks, double ksmax, bool useWeights, bool linlog, bool nohubs,
                          double repel, double attract, double gravity, double delta,
                          double tolerate);
}  // namespace partition

namespace {

using Coords = std::vector<std::vector<double>>;

struct Args {
  std::map<std::string, std::string> kv;
  const std::string& str(const std::string& k) const {
    auto it = kv.find(k);
    if (it == kv.end()) throw std::runtime_error("missing argument " + k + "=");
    return it->second;
  }
  int i(const std::string& k) const { return std::atoi(str(k).c_str()); }
  bool b(const std::string& k) const { return i(k) != 0; }
  /* strtod reads what Python's repr() writes back to the same double */
  double d(const std::string& k) const { return std::strtod(str(k).c_str(), nullptr); }
};

FILE* open_file(const std::string& path, const char* mode) {
  FILE* f = std::fopen(path.c_str(), mode);
  if (!f) throw std::runtime_error("cannot open " + path);
  return f;
}

template <typename T>
void read_exact(FILE* f, T* p, size_t count) {
  if (count && std::fread(p, sizeof(T), count, f) != count)
    throw std::runtime_error("short read");
}

template <typename T>
std::vector<T> read_all(const std::string& path) {
  FILE* f = open_file(path, "rb");
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(bytes / sizeof(T));
  read_exact(f, v.data(), v.size());
  std::fclose(f);
  return v;
}

SparseMatrix read_csr(FILE* f, bool square) {
  int hdr[2];
  read_exact(f, hdr, 2);
  std::vector<int> ip(hdr[0] + 1), ix(hdr[1]);
  std::vector<double> dx(hdr[1]);
  read_exact(f, ip.data(), ip.size());
  read_exact(f, ix.data(), ix.size());
  read_exact(f, dx.data(), dx.size());
  return SparseMatrix(ip, ix, dx, hdr[0], square ? hdr[0] : hdr[1]);
}

SparseMatrix read_csr(const std::string& path, bool square) {
  FILE* f = open_file(path, "rb");
  SparseMatrix M = read_csr(f, square);
  std::fclose(f);
  return M;
}

void write_csr(FILE* f, const SparseMatrix& M) {
  const int hdr[2] = {M.Rows(), (int)M.GetIndices().size()};
  std::fwrite(hdr, sizeof(int), 2, f);
  std::fwrite(M.GetIndptr().data(), sizeof(int), M.GetIndptr().size(), f);
  std::fwrite(M.GetIndices().data(), sizeof(int), M.GetIndices().size(), f);
  std::fwrite(M.GetData().data(), sizeof(double), M.GetData().size(), f);
}

Coords read_coords(const std::string& path, int dim) {
  const std::vector<double> flat = read_all<double>(path);
  Coords c(flat.size() / dim, std::vector<double>(dim));
  for (size_t i = 0; i < c.size(); ++i)
    for (int k = 0; k < dim; ++k) c[i][k] = flat[i * dim + k];
  return c;
}

void write_coords(const std::string& path, const Coords& c, int dim) {
  FILE* f = open_file(path, "wb");
  for (const auto& row : c) {
    if ((int)row.size() != dim) throw std::runtime_error("coordinate row of wrong length");
    std::fwrite(row.data(), sizeof(double), dim, f);
  }
  std::fclose(f);
}

void read_hier(const std::string& path, std::vector<SparseMatrix>& As,
               std::vector<SparseMatrix>& PTs) {
  FILE* f = open_file(path, "rb");
  int levels = 0;
  read_exact(f, &levels, 1);
  for (int l = 0; l <= levels; ++l) As.push_back(read_csr(f, true));
  for (int l = 0; l < levels; ++l) PTs.push_back(read_csr(f, false));
  std::fclose(f);
}

int run(const std::string& cmd, const Args& a) {
  omp_set_num_threads(a.i("threads"));
  ge_ref_seed = (unsigned)std::strtoul(a.str("seed").c_str(), nullptr, 10);
  const std::string& out = a.str("out");

  if (cmd == "fa") {
    const SparseMatrix A = read_csr(a.str("A"), true);
    const int dim = a.i("dim");
    Coords X;
    if (a.str("start") != "-") X = read_coords(a.str("start"), dim);
    partition::forceAtlas(A, dim, X, a.i("iterations"), a.d("ks"), a.d("ksmax"), a.d("repel"),
                          a.d("attract"), a.d("gravity"), a.b("use_weights"), a.b("linlog"),
                          a.b("nohubs"), a.d("delta"), a.d("tolerate"), a.b("normalize"));
    write_coords(out, X, dim);
  } else if (cmd == "ml") {
    const SparseMatrix A = read_csr(a.str("A"), true);
    const SparseMatrix PT = read_csr(a.str("PT"), false);
    const int dim = a.i("dim");
    const std::vector<int> vA = read_all<int>(a.str("vA"));
    const Coords cA = read_coords(a.str("cA"), dim);
    const std::vector<double> rA = read_all<double>(a.str("rA"));
    Coords X(A.Rows(), std::vector<double>(dim, 0.0));
    partition::forceAtlasMultilevel(A, PT, vA, cA, rA, X, dim, a.i("iterations"), a.d("ks"),
                                    a.d("ksmax"), a.b("use_weights"), a.b("linlog"),
                                    a.b("nohubs"), a.d("repel"), a.d("attract"), a.d("gravity"),
                                    a.d("delta"), a.d("tolerate"));
    write_coords(out, X, dim);
  } else if (cmd == "partition") {
    const SparseMatrix A = read_csr(a.str("A"), true);
    const std::string& mode = a.str("mode");
    const bool pm = a.b("positive_merging"), leaves = a.b("merge_leaves");
    const double stall = a.d("stall");
    const int matching = a.i("matching");
    std::vector<SparseMatrix> h;
    if (mode == "cf")
      h = partition::partition(A, a.d("value"), false, pm, stall, matching, leaves);
    else if (mode == "parts")
      h.push_back(partition::partition(A, a.i("value"), false, pm, stall, matching, leaves));
    else if (mode == "single")
      h.push_back(partition::partition(A, false, pm, stall, matching, leaves));
    else
      throw std::runtime_error("mode is cf, parts or single");
    FILE* f = open_file(out, "wb");
    const int count = (int)h.size();
    std::fwrite(&count, sizeof(int), 1, f);
    for (const auto& PT : h) write_csr(f, PT);
    std::fclose(f);
  } else if (cmd == "modularity") {
    const double q = partition::modularity(read_csr(a.str("A"), true), read_csr(a.str("PT"), false));
    FILE* f = open_file(out, "wb");
    std::fwrite(&q, sizeof(double), 1, f);
    std::fclose(f);
  } else if (cmd == "interp") {
    const SparseMatrix S = read_csr(a.str("sets"), false);
    std::vector<std::vector<int>> sets(S.Rows());
    for (int r = 0; r < S.Rows(); ++r)
      sets[r].assign(S.GetIndices().begin() + S.GetIndptr()[r],
                     S.GetIndices().begin() + S.GetIndptr()[r + 1]);
    FILE* f = open_file(out, "wb");
    write_csr(f, partition::interpolationMatrix(a.i("cols"), sets));
    std::fclose(f);
  } else if (cmd == "embed" || cmd == "minimize_ml") {
    std::vector<SparseMatrix> As, PTs;
    read_hier(a.str("hier"), As, PTs);
    const int dim = a.i("dim");
    Coords X;
    if (cmd == "embed") {
      X = partition::embed(As, PTs, dim);
    } else {
      using Embedder = Coords (*)(const SparseMatrix&, const int);
      X = partition::embedVia(
          As, PTs, dim,
          partition::anyToMultilevel(static_cast<Embedder>(partition::embedViaMinimization)));
    }
    write_coords(out, X, dim);
  } else if (cmd == "minimize") {
    const SparseMatrix A = read_csr(a.str("A"), true);
    const int dim = a.i("dim");
    Coords X;
    if (a.str("start") == "default") {
      X = partition::embedViaMinimization(A, dim);
    } else {
      if (a.str("start") != "-") X = read_coords(a.str("start"), dim);
      partition::embedViaMinimization(A, dim, X, a.i("iterations"));
    }
    write_coords(out, X, dim);
  } else if (cmd == "laplacian") {
    const SparseMatrix A = read_csr(a.str("A"), true);
    const SparseMatrix L = partition::toLaplacian(A);
    FILE* f = open_file(out, "wb");
    write_csr(f, partition::identity(A.Rows()));
    write_csr(f, L);
    write_csr(f, partition::fromLaplacian(L));
    std::fclose(f);
  } else {
    throw std::runtime_error("unknown subcommand " + cmd);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: ge_ref <subcommand> key=value ...\n");
    return 2;
  }
  Args a;
  for (int i = 2; i < argc; ++i) {
    const std::string s = argv[i];
    const size_t eq = s.find('=');
    if (eq == std::string::npos) {
      std::fprintf(stderr, "ge_ref: argument without '=': %s\n", argv[i]);
      return 2;
    }
    a.kv[s.substr(0, eq)] = s.substr(eq + 1);
  }
  try {
    return run(argv[1], a);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ge_ref %s: %s\n", argv[1], e.what());
    return 1;
  }
}

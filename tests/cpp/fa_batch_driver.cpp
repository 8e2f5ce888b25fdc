// embedVia(As, hierarchy, d, forceAtlasToMultilevel(ITER)) and embedVia(As, hierarchy, d,
// anyToMultilevel(<forceAtlas with ITER iterations>)) through the drop-in headers, both in
// one process: the batched level and the per-aggregate composition it replaces.  Also
// forceAtlasBatch on the two coarsest matrices against forceAtlas on each (exit status 3
// when they differ).  The hierarchy is partition(A, cf) with P^T A P per level, as
// examples/embed.cpp:93-102 builds it.
//   fa_batch_driver <in.bin> <out_batched.bin> <out_composed.bin> <dim> <seed> <cf> <ITER>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "embed.hpp"
#include "partitioner.hpp"

using Coords = std::vector<std::vector<double>>;

static void write(const char* path, const Coords& c, int dim) {
  std::ofstream out(path, std::ios::binary);
  for (const auto& row : c) out.write((const char*)row.data(), sizeof(double) * dim);
}

static bool same_bits(const Coords& a, const Coords& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].size() != b[i].size() ||
        std::memcmp(a[i].data(), b[i].data(), sizeof(double) * a[i].size()) != 0)
      return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int n = 0, nnz = 0;
  in.read((char*)&n, sizeof(int));
  in.read((char*)&nnz, sizeof(int));
  std::vector<int> I(n + 1), J(nnz);
  std::vector<double> D(nnz);
  in.read((char*)I.data(), sizeof(int) * (n + 1));
  in.read((char*)J.data(), sizeof(int) * nnz);
  in.read((char*)D.data(), sizeof(double) * nnz);
  SparseMatrix A(I, J, D, n, n);
  const int dim = std::atoi(argv[4]);
  partition::setSeed((unsigned)std::strtoul(argv[5], nullptr, 10));
  const double cf = std::atof(argv[6]);
  const int iterations = std::atoi(argv[7]);

  std::vector<SparseMatrix> hierarchy = partition::partition(A, cf);
  std::vector<SparseMatrix> As = {A};
  for (size_t level = 0; level < hierarchy.size(); level++)
    As.push_back(partition::galerkin(hierarchy[level], As[level]));

  write(argv[2], partition::embedVia(As, hierarchy, dim, partition::forceAtlasToMultilevel(iterations)),
        dim);
  const partition::MultilevelEmbedder composed =
      partition::anyToMultilevel([iterations](const SparseMatrix& S, const int d) {
        Coords c;
        partition::forceAtlas(S, d, c, iterations);
        return c;
      });
  write(argv[3], partition::embedVia(As, hierarchy, dim, composed), dim);

  const std::vector<SparseMatrix> two(As.end() - (As.size() > 1 ? 2 : 1), As.end());
  std::vector<Coords> batch;
  partition::forceAtlasBatch(two, dim, batch, 50);
  for (size_t g = 0; g < two.size(); ++g) {
    Coords alone;
    partition::forceAtlas(two[g], dim, alone, 50);
    if (!same_bits(batch[g], alone)) return 3;
  }
  return 0;
}

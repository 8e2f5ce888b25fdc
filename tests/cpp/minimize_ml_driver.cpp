// embedVia(As, hierarchy, d, minimizationToMultilevel(ITER)) through the drop-in
// headers: the reference's alternative multilevel embedder (src/embed.cpp:23-338)
// with the finest level's minimiser as one batched libge call.  The hierarchy is
// partition(A, cf) with P^T A P per level, as examples/embed.cpp:93-102 builds it.
//   minimize_ml_driver <in.bin> <out.bin> <dim> <seed> <cf> [ITER]
#include <cstdlib>
#include <fstream>
#include <vector>

#include "embed.hpp"
#include "partitioner.hpp"

int main(int argc, char** argv) {
  if (argc < 6) return 2;
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
  const int dim = std::atoi(argv[3]);
  partition::setSeed((unsigned)std::strtoul(argv[4], nullptr, 10));
  const double cf = std::atof(argv[5]);

  std::vector<SparseMatrix> hierarchy = partition::partition(A, cf);
  std::vector<SparseMatrix> As = {A};
  for (size_t level = 0; level < hierarchy.size(); level++)
    As.push_back(partition::galerkin(hierarchy[level], As[level]));
  const partition::MultilevelEmbedder embedder =
      argc > 6 ? partition::minimizationToMultilevel(std::atoi(argv[6]))
               : partition::minimizationToMultilevel();
  const std::vector<std::vector<double>> coords = partition::embedVia(As, hierarchy, dim, embedder);
  std::ofstream out(argv[2], std::ios::binary);
  for (const auto& row : coords) out.write((const char*)row.data(), sizeof(double) * dim);
  return 0;
}

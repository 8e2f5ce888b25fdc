// Dimensions above 4 through the drop-in headers only, as a caller of the reference
// would write them: partition::forceAtlas(A, 6) on one graph, and on another
// partition(B, 0.2), P^T A P per level and partition::embed(As, Ps, 8).
//   dims_driver <fa_in.bin> <fa_out.bin> <embed_in.bin> <embed_out.bin> <seed>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "embed.hpp"
#include "forceatlas.hpp"
#include "partitioner.hpp"

static SparseMatrix read_csr(const char* path) {
  std::ifstream in(path, std::ios::binary);
  int n = 0, nnz = 0;
  in.read((char*)&n, sizeof(int));
  in.read((char*)&nnz, sizeof(int));
  std::vector<int> I(n + 1), J(nnz);
  std::vector<double> D(nnz);
  in.read((char*)I.data(), sizeof(int) * (n + 1));
  in.read((char*)J.data(), sizeof(int) * nnz);
  in.read((char*)D.data(), sizeof(double) * nnz);
  return SparseMatrix(I, J, D, n, n);
}

static void write_coords(const char* path, const std::vector<std::vector<double>>& coords,
                         size_t dim) {
  std::ofstream out(path, std::ios::binary);
  for (const auto& row : coords) {
    if (row.size() != dim) std::exit(4);
    out.write((const char*)row.data(), sizeof(double) * dim);
  }
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  partition::setSeed((unsigned)std::strtoul(argv[5], nullptr, 10));

  SparseMatrix A = read_csr(argv[1]);
  write_coords(argv[2], partition::forceAtlas(A, 6), 6);

  SparseMatrix B = read_csr(argv[3]);
  std::vector<SparseMatrix> Ps = partition::partition(B, 0.2);
  std::vector<SparseMatrix> As = {B};
  for (size_t level = 0; level < Ps.size(); level++)
    As.push_back(partition::galerkin(Ps[level], As[level]));
  write_coords(argv[4], partition::embed(As, Ps, 8), 8);
  return 0;
}

// partition::layoutNeighbours and partition::neighbourhoodPrecision through the drop-in
// header only.
//   knn_driver <graph.bin> <coords.bin> <dim> <k> <kmax> <idx_out.bin> <totals_out.bin>
// idx_out: n * k ints, row-major; totals_out: 3 long longs (GE_NBHD_*).
#include <cstdlib>
#include <fstream>
#include <vector>

#include "forceatlas.hpp"

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

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  SparseMatrix A = read_csr(argv[1]);
  const int dim = std::atoi(argv[3]), k = std::atoi(argv[4]), kmax = std::atoi(argv[5]);
  std::vector<std::vector<double>> coords(A.Rows(), std::vector<double>(dim));
  std::ifstream in(argv[2], std::ios::binary);
  for (auto& row : coords) in.read((char*)row.data(), sizeof(double) * dim);
  if (!in) return 3;
  const auto nb = partition::layoutNeighbours(coords, k);
  std::ofstream idx(argv[6], std::ios::binary);
  for (const auto& row : nb) idx.write((const char*)row.data(), sizeof(int) * row.size());
  const auto t = partition::neighbourhoodPrecision(A, coords, kmax);
  std::ofstream tot(argv[7], std::ios::binary);
  tot.write((const char*)t.data(), sizeof(long long) * t.size());
  return 0;
}

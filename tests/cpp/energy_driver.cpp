// partition::layoutEnergy through the drop-in header only: the five totals of a layout,
// with forceAtlas's defaults and with every option set.
//   energy_driver <graph.bin> <coords.bin> <dim> <totals_out.bin>
// totals_out: 5 doubles of the defaults, then 5 of (repel 3.5, attract 0.75, gravity 2,
// useWeights, linlog, nohubs, delta 0.5).
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
  if (argc < 5) return 2;
  SparseMatrix A = read_csr(argv[1]);
  const int dim = std::atoi(argv[3]);
  std::vector<std::vector<double>> coords(A.Rows(), std::vector<double>(dim));
  std::ifstream in(argv[2], std::ios::binary);
  for (auto& row : coords) in.read((char*)row.data(), sizeof(double) * dim);
  if (!in) return 3;
  std::ofstream out(argv[4], std::ios::binary);
  const auto a = partition::layoutEnergy(A, coords);
  out.write((const char*)a.data(), sizeof(double) * a.size());
  const auto b = partition::layoutEnergy(A, coords, 3.5, 0.75, 2.0, true, true, true, 0.5);
  out.write((const char*)b.data(), sizeof(double) * b.size());
  return 0;
}

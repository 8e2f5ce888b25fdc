// forceAtlas through the drop-in header on one graph and start read from files, in
// GE_MODE_FARFIELD chosen by partition::setMode / setTheta ("set") or left to $GE_MODE
// and $GE_THETA ("env"): tests/test_gpu_farfield.py compares the coordinates with the
// Python binding's bit for bit.  A rejected theta ends with status 5.
//   farfield_driver <a.bin> <x0.bin> <out.bin> <dim> <iterations> <how> <theta>
// a.bin: n, nnz (int), indptr / indices (int), data (double); x0.bin: n * dim doubles.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <string>
#include <vector>

#include "forceatlas.hpp"

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int n = 0, nnz = 0;
  in.read((char*)&n, sizeof(int));
  in.read((char*)&nnz, sizeof(int));
  const int dim = std::atoi(argv[4]);
  std::vector<int> I(n + 1), J(nnz);
  std::vector<double> D(nnz), X0((size_t)n * dim);
  in.read((char*)I.data(), sizeof(int) * (n + 1));
  in.read((char*)J.data(), sizeof(int) * nnz);
  in.read((char*)D.data(), sizeof(double) * nnz);
  std::ifstream xin(argv[2], std::ios::binary);
  xin.read((char*)X0.data(), sizeof(double) * X0.size());
  if (!in || !xin) return 3;
  SparseMatrix A(I, J, D, n, n);
  std::vector<std::vector<double>> coords(n, std::vector<double>(dim));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) coords[i][k] = X0[(size_t)i * dim + k];
  try {
    const std::string how = argv[6];
    if (how == "set") {
      partition::setMode(GE_MODE_FARFIELD);
      partition::setTheta(std::atof(argv[7]));
    } else if (how != "env") {
      return 2;
    }
    partition::forceAtlas(A, dim, coords, std::atoi(argv[5]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  std::ofstream out(argv[3], std::ios::binary);
  for (const auto& row : coords) out.write((const char*)row.data(), sizeof(double) * dim);
  return out ? 0 : 4;
}

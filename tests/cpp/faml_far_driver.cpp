// forceAtlasMultilevel through the drop-in header on one level read from a file, with
// GE_MODE_FARFIELD chosen by partition::setMode / setTheta ("set") or left to $GE_MODE
// and $GE_THETA ("env"): tests/test_gpu_faml_far.py compares the coordinates with the
// Python binding's bit for bit.
//   faml_far_driver <in.bin> <out.bin> <dim> <seed> <iterations> <repel> <how> <theta>
// in.bin: n, nnz, m (int), A's indptr / indices (int) / data (double), P_T's indptr /
// indices (int), coords_A (m * dim doubles), r_A (m doubles).
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <string>
#include <vector>

#include "forceatlas.hpp"

int main(int argc, char** argv) {
  if (argc != 9) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int n = 0, nnz = 0, m = 0;
  in.read((char*)&n, sizeof(int));
  in.read((char*)&nnz, sizeof(int));
  in.read((char*)&m, sizeof(int));
  const int dim = std::atoi(argv[3]);
  std::vector<int> I(n + 1), J(nnz), PI(m + 1), PJ(n);
  std::vector<double> D(nnz), cA((size_t)m * dim), rA(m);
  in.read((char*)I.data(), sizeof(int) * (n + 1));
  in.read((char*)J.data(), sizeof(int) * nnz);
  in.read((char*)D.data(), sizeof(double) * nnz);
  in.read((char*)PI.data(), sizeof(int) * (m + 1));
  in.read((char*)PJ.data(), sizeof(int) * n);
  in.read((char*)cA.data(), sizeof(double) * cA.size());
  in.read((char*)rA.data(), sizeof(double) * m);
  if (!in) return 3;
  SparseMatrix A(I, J, D, n, n);
  SparseMatrix P(PI, PJ, std::vector<double>(n, 1.0), m, n);
  std::vector<int> v_A(n);
  for (int a = 0; a < m; ++a)
    for (int c = PI[a]; c < PI[a + 1]; ++c) v_A[PJ[c]] = a;
  std::vector<std::vector<double>> coords_A(m, std::vector<double>(dim));
  for (int a = 0; a < m; ++a)
    for (int k = 0; k < dim; ++k) coords_A[a][k] = cA[(size_t)a * dim + k];
  std::vector<std::vector<double>> coords;
  try {
    partition::setSeed((unsigned)std::strtoul(argv[4], nullptr, 10));
    const std::string how = argv[7];
    if (how == "set") {
      partition::setMode(GE_MODE_FARFIELD);
      partition::setTheta(std::atof(argv[8]));
    } else if (how != "env") {
      return 2;
    }
    partition::forceAtlasMultilevel(A, P, v_A, coords_A, rA, coords, dim, std::atoi(argv[5]), 0.1,
                                    1.0, true, false, false, std::atof(argv[6]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  std::ofstream out(argv[2], std::ios::binary);
  for (const auto& row : coords) out.write((const char*)row.data(), sizeof(double) * dim);
  return out ? 0 : 4;
}

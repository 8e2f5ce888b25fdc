// The one-level overloads of the drop-in partitioner.hpp, selected the way a
// caller of the reference selects them:
//   partition_overloads <in.bin> <out.bin> single
//       -> partition::partition(A)
//   partition_overloads <in.bin> <out.bin> bool <positive> <stall> <matching>
//       -> partition::partition(A, false, positive, stall, matching)
//   partition_overloads <in.bin> <out.bin> parts <numParts> <positive> <stall> <matching>
//       -> partition::partition(A, numParts, false, positive, stall, matching)
// The P_T goes to <out.bin> as rows, cols, indptr, indices.
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "partitioner.hpp"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
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
  const std::string mode = argv[3];
  SparseMatrix P;
  if (mode == "single" && argc == 4) {
    P = partition::partition(A);
  } else if (mode == "bool" && argc == 7) {
    P = partition::partition(A, false, std::atoi(argv[4]) != 0, std::atof(argv[5]),
                             std::atoi(argv[6]));
  } else if (mode == "parts" && argc == 8) {
    const int numParts = std::atoi(argv[4]);
    P = partition::partition(A, numParts, false, std::atoi(argv[5]) != 0, std::atof(argv[6]),
                             std::atoi(argv[7]));
  } else {
    return 2;
  }
  std::ofstream out(argv[2], std::ios::binary);
  const int rows = P.Rows(), cols = P.Cols();
  out.write((const char*)&rows, sizeof(int));
  out.write((const char*)&cols, sizeof(int));
  out.write((const char*)P.GetIndptr().data(), sizeof(int) * (rows + 1));
  out.write((const char*)P.GetIndices().data(), sizeof(int) * cols);
  return 0;
}

// The device library's log1p and pow on the operand ranges of the layout energy's linlog
// and delta paths (tests/energy_cases.py takes its LOG1P_ULP and POW_ULP from this).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off scripts/micro/ocml_ulp.hip \
//         -o scripts/micro/ocml_ulp
//   scripts/micro/ocml_ulp out.bin && python scripts/ocml_ulp.py out.bin
// out.bin: N x {x, log1p(x)}, x log-uniform in [1e-5, 4], then N x {a, pow(a, 0.5)}, a
// uniform in [0.125, 2]; N = 2^20.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#define CHECK(call)                                                     \
  do {                                                                  \
    hipError_t e_ = (call);                                             \
    if (e_ != hipSuccess) {                                             \
      std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));   \
      return 1;                                                         \
    }                                                                   \
  } while (0)

__global__ void eval(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n) return;
  out[i] = i < n ? log1p(in[i]) : pow(in[i], 0.5);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int n = 1 << 20;
  std::vector<double> in(2 * n), out(2 * n);
  for (int k = 0; k < n; ++k) {
    in[k] = 1e-5 * std::exp(std::log(4e5) * k / (n - 1));
    in[n + k] = 0.125 + 1.875 * k / (n - 1);
  }
  double *d_in = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_in, sizeof(double) * 2 * n));
  CHECK(hipMalloc(&d_out, sizeof(double) * 2 * n));
  CHECK(hipMemcpy(d_in, in.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(eval, dim3((2 * n + 255) / 256), dim3(256), 0, 0, n, d_in, d_out);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(out.data(), d_out, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 3;
  for (int k = 0; k < 2 * n; ++k) {
    std::fwrite(&in[k], sizeof(double), 1, f);
    std::fwrite(&out[k], sizeof(double), 1, f);
  }
  std::fclose(f);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return 0;
}

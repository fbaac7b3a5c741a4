// Stand-alone check of csrc/perm_line.hpp, perm_tensor_line_coefficients (host-only): perm_tensor_line_check DIM FIXED_LO FIXED_HI h_0 .. h_{n-1} then DIM blocks of n
// layer values (x first) prints the 2 (DIM + 1) coefficient arrays, one line each.  Built by tests/test_permeability_tensor_cpu.py with -fsanitize=address,undefined and
// run directly.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "perm_line.hpp"

int main(int argc, char **argv) {
  const int dim = argc > 1 ? std::atoi(argv[1]) : 0;
  if ((dim != 2 && dim != 3) || argc < 4 + (dim + 1) || (argc - 4) % (dim + 1)) { std::fprintf(stderr, "usage: perm_tensor_line_check DIM LO HI h... kx... ky... [kz...]\n"); return 2; }
  const int n = (argc - 4) / (dim + 1);
  std::vector<double> h(n), layer[3];
  for (int i = 0; i < n; ++i) h[i] = std::strtod(argv[4 + i], nullptr);
  for (int d = 0; d < dim; ++d) { layer[d].resize(n); for (int i = 0; i < n; ++i) layer[d][i] = std::strtod(argv[4 + (d + 1) * n + i], nullptr); }
  const std::vector<double> c = poro::perm_tensor_line_coefficients(dim, h, layer, std::atoi(argv[2]) != 0, std::atoi(argv[3]) != 0);
  for (int r = 0; r < 2 * (dim + 1); ++r) { for (int i = 0; i <= n; ++i) std::printf("%.17g ", c[(size_t)r * (n + 1) + i]); std::printf("\n"); }
  return 0;
}

// Stand-alone check of csrc/perm_line.hpp (host-only): perm_line_check NW FIXED_LO FIXED_HI h_0 .. h_{n-1}, then NW blocks of n weight-line layer values and one block of
// n Laplace layer values, prints the 2 (NW + 2) coefficient arrays, one line each.  One k / mu per cell: NW = 1 and its layer values twice; the diagonal tensor: NW =
// dim - 1 and its components, x first.  Built by tests/test_permeability_cpu.py and tests/test_permeability_tensor_cpu.py with -fsanitize=address,undefined and run directly.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "perm_line.hpp"

int main(int argc, char **argv) {
  const int nw = argc > 1 ? std::atoi(argv[1]) : 0;
  if ((nw != 1 && nw != 2) || argc < 4 + (nw + 2) || (argc - 4) % (nw + 2)) { std::fprintf(stderr, "usage: perm_line_check NW LO HI h... w0... [w1...] k...\n"); return 2; }
  const int n = (argc - 4) / (nw + 2);
  std::vector<double> h(n), layer[3];
  for (int i = 0; i < n; ++i) h[i] = std::strtod(argv[4 + i], nullptr);
  for (int d = 0; d <= nw; ++d) { layer[d].resize(n); for (int i = 0; i < n; ++i) layer[d][i] = std::strtod(argv[4 + (d + 1) * n + i], nullptr); }
  const std::vector<double> c = poro::perm_line_coefficients(h, layer, nw, layer[nw], std::atoi(argv[2]) != 0, std::atoi(argv[3]) != 0);
  for (int r = 0; r < 2 * (nw + 2); ++r) { for (int i = 0; i <= n; ++i) std::printf("%.17g ", c[(size_t)r * (n + 1) + i]); std::printf("\n"); }
  return 0;
}

// Stand-alone check of csrc/perm_line.hpp (host-only): perm_line_check FIXED_LO FIXED_HI h_0 .. h_{n-1} k_0 .. k_{n-1} prints the six coefficient arrays, one line each.
// Built by tests/test_permeability_cpu.py with -fsanitize=address,undefined and run directly.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "perm_line.hpp"

int main(int argc, char **argv) {
  if (argc < 5 || (argc - 3) % 2) { std::fprintf(stderr, "usage: perm_line_check LO HI h... k...\n"); return 2; }
  const int n = (argc - 3) / 2;
  std::vector<double> h(n), k(n);
  for (int i = 0; i < n; ++i) { h[i] = std::strtod(argv[3 + i], nullptr); k[i] = std::strtod(argv[3 + n + i], nullptr); }
  const std::vector<double> c = poro::perm_line_coefficients(h, k, std::atoi(argv[1]) != 0, std::atoi(argv[2]) != 0);
  for (int r = 0; r < 6; ++r) { for (int i = 0; i <= n; ++i) std::printf("%.17g ", c[(size_t)r * (n + 1) + i]); std::printf("\n"); }
  return 0;
}

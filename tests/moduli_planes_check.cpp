// Stand-alone check of csrc/moduli_planes.hpp (host-only):
//   moduli_planes_check K lam_0 .. lam_{n-1} G_0 .. G_{n-1}
// prints the per-plane weight table of the structured operator for layered moduli, one line of four values (lambda_lo, G_lo, lambda_hi, G_hi) per node plane, K n + 1
// lines.  The refusals (a degree other than 1 or 2, no layer) are exercised first.  Built by tests/test_moduli_structured_cpu.py with -fsanitize=address,undefined and
// run directly.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>
#include "moduli_planes.hpp"

template <class F> static bool refuses(F &&f) { try { f(); } catch (const std::runtime_error &) { return true; } return false; }

int main(int argc, char **argv) {
  if (argc < 4 || (argc - 2) % 2) { std::fprintf(stderr, "usage: moduli_planes_check K lam... G...\n"); return 2; }
  const int k = std::atoi(argv[1]), n = (argc - 2) / 2;
  std::vector<double> lam(n), G(n);
  for (int i = 0; i < n; ++i) { lam[i] = std::strtod(argv[2 + i], nullptr); G[i] = std::strtod(argv[2 + n + i], nullptr); }
  if (!refuses([&] { poro::moduli_plane_table(3, lam, G); }) || !refuses([&] { poro::moduli_plane_table(k, {}, {}); }) ||
      !refuses([&] { poro::moduli_plane_table(k, lam, std::vector<double>(G.begin(), G.end() - 1)); })) return 3;
  const std::vector<double> t = poro::moduli_plane_table(k, lam, G);
  if (t.size() != (size_t)(k * n + 1) * poro::kModuliPlaneStride) return 4;
  for (size_t p = 0; p < t.size() / 4; ++p) std::printf("%.17g %.17g %.17g %.17g\n", t[4 * p], t[4 * p + 1], t[4 * p + 2], t[4 * p + 3]);
  return 0;
}

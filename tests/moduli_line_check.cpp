// Stand-alone check of csrc/moduli_line.hpp (host-only):
//   moduli_line_check DIM K COMP FIXED_LO FIXED_HI L0 L1 h_0 .. h_{n-1} lam_0 .. lam_{n-1} G_0 .. G_{n-1} b_0 .. b_{nl-1}        (nl = K n + 1; L0 / L1 may be "inf")
// prints the 3 (K + 1) band arrays of the component's coefficient block, the K + 1 arrays of the factorisation of the column (L0, L1) and the solution of T x = b, one
// line each.  Before that it compares the bands for weight 1 with the dense matrices of fe1d (fdm_tables.hpp).  Built by tests/test_moduli_cpu.py with
// -fsanitize=address,undefined and run directly.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fdm_tables.hpp"
#include "moduli_line.hpp"

int main(int argc, char **argv) {
  if (argc < 8) { std::fprintf(stderr, "usage: moduli_line_check DIM K COMP LO HI L0 L1 h... lam... G... b...\n"); return 2; }
  const int dim = std::atoi(argv[1]), k = std::atoi(argv[2]), comp = std::atoi(argv[3]);
  const bool lo = std::atoi(argv[4]) != 0, hi = std::atoi(argv[5]) != 0;
  const double l0 = std::strtod(argv[6], nullptr), l1 = std::strtod(argv[7], nullptr);
  const int rest = argc - 8;
  if ((k != 1 && k != 2) || (rest - 1) % (3 + k)) { std::fprintf(stderr, "moduli_line_check: argument count\n"); return 2; }
  const int n = (rest - 1) / (3 + k), nl = k * n + 1;
  std::vector<double> h(n), lam(n), G(n), b(nl);
  for (int i = 0; i < n; ++i) { h[i] = std::strtod(argv[8 + i], nullptr); lam[i] = std::strtod(argv[8 + n + i], nullptr); G[i] = std::strtod(argv[8 + 2 * n + i], nullptr); }
  for (int i = 0; i < nl; ++i) b[i] = std::strtod(argv[8 + 3 * n + i], nullptr);
  // weight 1, free ends: the bands of fe1d's dense matrices
  {
    std::vector<double> M, K; poro::fe1d(k, h, M, K);
    const std::vector<double> one(n, 1.0), bm = poro::moduli_bands(k, h, one, false, false, false), bk = poro::moduli_bands(k, h, one, true, false, false);
    for (int band = 0; band <= k; ++band) for (int i = 0; i < nl; ++i) {
      const double wm = i + band < nl ? M[(size_t)i * nl + i + band] : 0.0, wk = i + band < nl ? K[(size_t)i * nl + i + band] : 0.0;
      if (std::fabs(bm[(size_t)band * nl + i] - wm) > 1e-15 * std::fabs(wm) || std::fabs(bk[(size_t)band * nl + i] - wk) > 1e-15 * std::fabs(wk)) return 3;
    }
    for (int i = 0; i < nl; ++i) for (int j = i + k + 1; j < nl; ++j) if (M[(size_t)i * nl + j] != 0 || K[(size_t)i * nl + j] != 0) return 4;      // nothing outside the bands
  }
  const std::vector<double> coef = poro::moduli_line_coefficients(dim, k, comp, h, lam, G, lo, hi);
  for (int r = 0; r < 3 * (k + 1); ++r) { for (int i = 0; i < nl; ++i) std::printf("%.17g ", coef[(size_t)r * nl + i]); std::printf("\n"); }
  std::vector<double> fac((size_t)(k + 1) * nl);
  poro::moduli_line_factor_host(coef.data(), k, (size_t)nl, l0, l1, fac.data());
  for (int r = 0; r <= k; ++r) { for (int i = 0; i < nl; ++i) std::printf("%.17g ", fac[(size_t)r * nl + i]); std::printf("\n"); }
  poro::moduli_line_solve_host(fac.data(), k, (size_t)nl, !(std::isfinite(l0) && std::isfinite(l1)), lo, hi, b.data());
  for (int i = 0; i < nl; ++i) std::printf("%.17g ", b[i]);
  std::printf("\n");
  return 0;
}

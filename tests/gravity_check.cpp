// Stand-alone check of csrc/gravity_weights.hpp (host-only), the closed forms of the gravity kernels of uniform boxes:
//   gravity_check HX HY HZ
// For cells of sides (HX, HY[, HZ]) in 2D and 3D and degrees 1 and 2: the 1D weights int phi_s sum to h and agree with Gauss quadrature of the Lagrange basis; the
// gradient integrals int_c d_d phi_v sum to 0 over the vertices of a cell for every direction and agree with Gauss quadrature of the Q1 basis.  Prints every value it
// checked; exit code 0 when all hold to 1e-14 of the cell's scale (a few dozen roundings of 1.1e-16 in the quadrature sums).  Built by tests/test_gravity_cpu.py with -fsanitize=address,undefined and run directly.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "gravity_weights.hpp"

static const double kGaussX[3] = {0.5 - 0.5 * 0.7745966692414834, 0.5, 0.5 + 0.5 * 0.7745966692414834};      // three points on [0, 1]: exact to degree 5
static const double kGaussW[3] = {5.0 / 18, 8.0 / 18, 5.0 / 18};

// equidistant Lagrange basis of degree k on [0, 1]: value and derivative of shape function s at t
static double lagrange(int k, int s, double t, double *deriv) {
  double v = 1, d = 0;
  for (int m = 0; m <= k; ++m) {
    if (m == s) continue;
    const double f = (t - (double)m / k) / ((double)s / k - (double)m / k);
    d = d * f + v / ((double)s / k - (double)m / k);
    v *= f;
  }
  if (deriv) *deriv = d;
  return v;
}

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: gravity_check HX HY HZ\n"); return 2; }
  const double h[3] = {std::strtod(argv[1], nullptr), std::strtod(argv[2], nullptr), std::strtod(argv[3], nullptr)};
  int bad = 0;
  for (int k = 1; k <= 2; ++k)
    for (int d = 0; d < 3; ++d) {
      double sum = 0;
      for (int s = 0; s <= k; ++s) {
        const double w = poro::gravity_weight_1d(k, s, h[d]);
        double q = 0;
        for (int p = 0; p < 3; ++p) q += kGaussW[p] * lagrange(k, s, kGaussX[p], nullptr) * h[d];
        std::printf("weight k=%d s=%d h=%.17g: %.17g (Gauss %.17g)\n", k, s, h[d], w, q);
        if (!(std::fabs(w - q) <= 1e-14 * h[d])) ++bad;
        sum += w;
      }
      if (!(std::fabs(sum - h[d]) <= 1e-14 * h[d])) { std::printf("weights of k=%d do not sum to h=%.17g: %.17g\n", k, h[d], sum); ++bad; }
      if (poro::gravity_weight_1d(k, k + 1, h[d]) != 0.0 || poro::gravity_weight_1d(3, 0, h[d]) != 0.0) ++bad;      // outside the table: 0
    }
  for (int dim = 2; dim <= 3; ++dim) {
    double vol = 1; for (int e = 0; e < dim; ++e) vol *= h[e];
    for (int d = 0; d < dim; ++d) {
      double sum = 0;
      for (int v = 0; v < (1 << dim); ++v) {
        const double a = poro::gravity_gradient_integral(dim, h, v, d);
        // Gauss quadrature of d_d phi_v over the cell: the product of the 1D integrals of the Q1 factors (derivative along d, value along the others)
        double q = 1;
        for (int e = 0; e < dim; ++e) {
          double one = 0;
          for (int p = 0; p < 3; ++p) { double dv = 0; const double val = lagrange(1, (v >> e) & 1, kGaussX[p], &dv); one += kGaussW[p] * (e == d ? dv : val * h[e]); }
          q *= one;
        }
        std::printf("gradient dim=%d v=%d d=%d: %.17g (Gauss %.17g)\n", dim, v, d, a, q);
        if (!(std::fabs(a - q) <= 1e-14 * vol / h[d])) ++bad;
        sum += a;
      }
      if (!(std::fabs(sum) <= 1e-14 * vol / h[d])) /* (equal magnitudes, but a running sum of three of them is rounded) */ { std::printf("gradient integrals of dim=%d d=%d sum to %.17g\n", dim, d, sum); ++bad; }
    }
  }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

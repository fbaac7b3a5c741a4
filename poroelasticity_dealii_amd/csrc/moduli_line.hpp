// Host-only: the 1D mathematics of the line solve that PORO_PREC_FDM runs along the slowest direction of the DISPLACEMENT system when per-cell moduli are set
// (kernels_fdmu_line.hip).  With lambda(z), G(z) layered along that direction the diagonal block of component c is still a Kronecker sum,
//   A_cc = Kx (x) My (x) Mz^{w(c,0)} + Mx (x) Ky (x) Mz^{w(c,1)} + Mx (x) My (x) Kz^{w(c,2)},   w(c,d) = lambda + 2G (d == c) | G,
// with the FE_Q(k) mass / stiffness matrices of the line assembled with the layer weights.  After the x / y transforms one SPD banded system per mode (p, q) is left,
//   T = lam0_c[p] Mz^{w(c,0)} + lam1_c[q] Mz^{w(c,1)} + Kz^{w(c,2)}       (2D: T = lam0_c[p] My^{w(c,0)} + Ky^{w(c,1)}),
// of bandwidth k: tridiagonal for Q1, pentadiagonal for Q2.  Here: the band arrays, and the banded L D L^T factorisation and sweeps exactly as the kernels run them (the
// stand-alone check tests/moduli_line_check.cpp runs these under the sanitizers).  No HIP, no project header.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace poro {

// element matrices of FE_Q(k) on a cell of length h, weight 1 - the constants of fe1d (fdm_tables.hpp)
inline double moduli_me(int k, int a, int b, double h) {
  static const double M2[3][3] = {{4, 2, -1}, {2, 16, 2}, {-1, 2, 4}}, M1[2][2] = {{2, 1}, {1, 2}};
  return k == 2 ? h / 30.0 * M2[a][b] : h / 6.0 * M1[a][b];
}
inline double moduli_ke(int k, int a, int b, double h) {
  static const double K2[3][3] = {{7, -8, 1}, {-8, 16, -8}, {1, -8, 7}}, K1[2][2] = {{1, -1}, {-1, 1}};
  return k == 2 ? K2[a][b] / (3.0 * h) : K1[a][b] / h;
}

// band b (0 .. k) of the weighted mass (stiffness = true: stiffness) matrix: out[b * nl + i] = B(i, i + b), nl = k n_cells + 1, zero where i + b >= nl.
// fixed_lo / fixed_hi: the end node leaves the system - its couplings are zero; its diagonal is 1 in the stiffness matrix and 0 in the mass matrix (an identity row of T)
inline std::vector<double> moduli_bands(int k, const std::vector<double> &hcell, const std::vector<double> &w, bool stiffness, bool fixed_lo, bool fixed_hi) {
  const size_t n = hcell.size(), nl = (size_t)k * n + 1;
  std::vector<double> B((size_t)(k + 1) * nl, 0.0);
  for (size_t e = 0; e < n; ++e)
    for (int a = 0; a <= k; ++a) for (int b = a; b <= k; ++b)
      B[(size_t)(b - a) * nl + k * e + a] += w[e] * (stiffness ? moduli_ke(k, a, b, hcell[e]) : moduli_me(k, a, b, hcell[e]));
  auto drop = [&](size_t node) {
    for (int b = 1; b <= k; ++b) { B[(size_t)b * nl + node] = 0; if (node >= (size_t)b) B[(size_t)b * nl + node - b] = 0; }
    B[node] = stiffness ? 1.0 : 0.0;
  };
  if (fixed_lo) drop(0);
  if (fixed_hi) drop(nl - 1);
  return B;
}

// the coefficient block of one component: [matrix m = 0, 1, 2][band b = 0 .. k][nl] - m = 0, 1: the mass matrices that go with the eigenvalues of the first and the second
// leading direction (the second is zero in 2D), m = 2: the stiffness matrix of the line direction.  layer_lam / layer_G: one value per cell layer of the line
inline std::vector<double> moduli_line_coefficients(int dim, int k, int comp, const std::vector<double> &hcell, const std::vector<double> &layer_lam, const std::vector<double> &layer_G,
                                                    bool fixed_lo, bool fixed_hi) {
  const size_t n = hcell.size(), nl = (size_t)k * n + 1, per = (size_t)(k + 1) * nl;
  const int last = dim - 1;
  std::vector<double> l2g(n), G(layer_G.begin(), layer_G.begin() + n);
  for (size_t e = 0; e < n; ++e) l2g[e] = layer_lam[e] + 2 * layer_G[e];
  std::vector<double> out(3 * per, 0.0);
  for (int d = 0; d < last; ++d) {
    const std::vector<double> B = moduli_bands(k, hcell, d == comp ? l2g : G, false, fixed_lo, fixed_hi);
    for (size_t i = 0; i < per; ++i) out[(size_t)d * per + i] = B[i];
  }
  const std::vector<double> B = moduli_bands(k, hcell, last == comp ? l2g : G, true, fixed_lo, fixed_hi);
  for (size_t i = 0; i < per; ++i) out[2 * per + i] = B[i];
  return out;
}

// T = l0 B0 + l1 B1 + B2 of one column from a component's coefficient block: band b at node i
inline double moduli_line_entry(const double *coef, int k, size_t nl, double l0, double l1, int b, size_t i) {
  const size_t per = (size_t)(k + 1) * nl, at = (size_t)b * nl + i;
  return l0 * coef[at] + l1 * coef[per + at] + coef[2 * per + at];
}

// banded L D L^T without pivoting of one column, as k_fdmu_line_factor: fac = [inv | m1 | m2] (k = 1: [inv | m1]), nl entries each: reciprocal pivots 1 / d_i and the
// multipliers m1[i] = L(i + 1, i), m2[i] = L(i + 2, i).  A column whose x or y mode was removed (eigenvalue not finite) gets zeros: no product with the placeholder is formed
inline void moduli_line_factor_host(const double *coef, int k, size_t nl, double l0, double l1, double *fac) {
  double *inv = fac, *m1 = fac + nl, *m2 = k == 2 ? fac + 2 * nl : nullptr;
  if (!(std::isfinite(l0) && std::isfinite(l1))) { for (size_t i = 0; i < (size_t)(k + 1) * nl; ++i) fac[i] = 0; return; }
  double d1 = 0, d2 = 0, p1 = 0, p2 = 0, pp2 = 0;      // d_{i-1}, d_{i-2}, m1[i-1], m2[i-1], m2[i-2]
  for (size_t i = 0; i < nl; ++i) {
    const double d = moduli_line_entry(coef, k, nl, l0, l1, 0, i) - p1 * p1 * d1 - pp2 * pp2 * d2, r = 1.0 / d;
    const double a = (moduli_line_entry(coef, k, nl, l0, l1, 1, i) - p2 * p1 * d1) * r;
    const double b = k == 2 ? moduli_line_entry(coef, k, nl, l0, l1, 2, i) * r : 0.0;
    inv[i] = r; m1[i] = a; if (m2) m2[i] = b;
    d2 = d1; d1 = d; pp2 = p2; p2 = b; p1 = a;
  }
}
// the sweeps of k_fdmu_line_solve on one column, in place: forward substitution, scaling with the reciprocal pivots, back substitution - no division
inline void moduli_line_solve_host(const double *fac, int k, size_t nl, bool removed, bool fixed_lo, bool fixed_hi, double *v) {
  const double *inv = fac, *m1 = fac + nl, *m2 = k == 2 ? fac + 2 * nl : nullptr;
  if (removed) { for (size_t i = 0; i < nl; ++i) v[i] = 0; return; }
  double y1 = 0, y2 = 0, p1 = 0, p2 = 0, pp2 = 0;
  for (size_t i = 0; i < nl; ++i) {
    const double b = ((i == 0 && fixed_lo) || (i == nl - 1 && fixed_hi)) ? 0.0 : v[i];
    const double y = b - p1 * y1 - pp2 * y2;
    v[i] = y * inv[i];
    y2 = y1; y1 = y; pp2 = p2; p2 = m2 ? m2[i] : 0.0; p1 = m1[i];
  }
  double x1 = 0, x2 = 0;
  for (size_t i = nl; i-- > 0;) {
    const double x = v[i] - m1[i] * x1 - (m2 ? m2[i] : 0.0) * x2;
    v[i] = x; x2 = x1; x1 = x;
  }
}

}  // namespace poro

// Host-only: the closed forms behind the two gravity vectors of a uniform box (kernels_gravity.hip).
//   body force   b_i = sum_c rho_c int_c g . phi_i: on a box cell int_c phi_i is the product over the directions of the 1D weights int phi_s of the node's position s
//                in the cell: h / 2, h / 2 for Q1; h / 6, 4 h / 6, h / 6 for Q2 (Simpson's weights: the Lagrange basis on equidistant nodes)
//   Darcy flux   f_i = -sum_c rho_f int_c (kappa_c g) . grad(phi_i), Q1: int_c d_d phi_i = +- prod_{e != d} h_e / 2, + where the node sits on the high side of the cell
//                in direction d, - on the low side
// Everything is constexpr and free of HIP and of project headers: the kernels evaluate the same functions the stand-alone check tests/gravity_check.cpp runs under the
// sanitizers.
#pragma once

namespace poro {

// int over a cell of length h of the 1D Lagrange shape function at local node s (0 .. k) of degree k = 1 | 2; 0 for anything else
constexpr double gravity_weight_1d(int k, int s, double h) {
  if (k == 1) return (s == 0 || s == 1) ? h / 2 : 0.0;
  if (k == 2) return (s == 0 || s == 2) ? h / 6 : s == 1 ? 4 * h / 6 : 0.0;
  return 0.0;
}
// sign of int d phi / dx of the 1D Q1 shape function at local vertex v (0: low end, 1: high end); the integral itself is +-1
constexpr double gravity_sign_1d(int v) { return v ? 1.0 : -1.0; }
// int_c d_d phi_i over a box cell of sides h[0 .. dim): local vertex number v = v0 + 2 v1 (+ 4 v2)
constexpr double gravity_gradient_integral(int dim, const double *h, int v, int d) {
  double a = gravity_sign_1d((v >> d) & 1);
  for (int e = 0; e < dim; ++e) if (e != d) a *= h[e] / 2;
  return a;
}

}  // namespace poro

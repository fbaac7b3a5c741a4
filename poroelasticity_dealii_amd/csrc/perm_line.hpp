// Host-only: the 1D coefficient arrays of the line solve that PORO_PREC_FDM runs along the slowest direction when a per-cell k / mu or its diagonal tensor is set
// (kernels_fdm.hip: k_q1_line_solve).  No HIP, no project header: compiles into the device library and into stand-alone checks alike.  (What is common to every
// per-cell field, the classification by layers among it: cell_field.hpp.)
#pragma once
#include <cstddef>
#include <vector>

namespace poro {

// In the eigenbasis of the leading directions the line system of mode (p, q) is  a Mz + lam_x[p] Mz^kx + lam_y[q] Mz^ky + Kz^kz  (2D: a My + lam_x[p] My^kx + Ky^ky):
// every weight line is a mass line weighted with its layer values, the Laplace line is weighted with the line direction's.  One k / mu per cell: one weight line, its
// layer values (kx = ky multiplies lam_x + lam_y), which are the Laplace weights as well; the diagonal tensor: dim - 1 weight lines and its last component.
// [md mo | w_0d w_0o | ... | kd ko]: 2 (n_weight_lines + 2) arrays of nl = hcell.size() + 1 entries, diagonal and off-diagonal (entry k couples nodes k and k + 1; entry
// nl - 1 is 0) of the 1D Q1 matrices on the line with cell sizes hcell.
// fixed_lo / fixed_hi: the end node is prescribed - its row and column leave the system: identity row (md = w_d = 0, kd = 1), no coupling; the kernel zeroes its right-hand side.
inline std::vector<double> perm_line_coefficients(const std::vector<double> &hcell, const std::vector<double> *weight_layers, int n_weight_lines, const std::vector<double> &laplace_layer,
                                                  bool fixed_lo, bool fixed_hi) {
  const size_t n = hcell.size(), nl = n + 1; const int na = 2 * (n_weight_lines + 2);
  std::vector<double> c((size_t)na * nl, 0.0);
  double *md = c.data(), *mo = md + nl, *kd = md + (size_t)(na - 2) * nl, *ko = kd + nl;
  for (size_t e = 0; e < n; ++e) {
    const double h = hcell[e], k = laplace_layer[e];
    md[e] += h / 3; md[e + 1] += h / 3; mo[e] += h / 6;
    for (int d = 0; d < n_weight_lines; ++d) {
      double *wd = md + (size_t)(2 + 2 * d) * nl, *wo = wd + nl; const double w = weight_layers[d][e];
      wd[e] += w * h / 3; wd[e + 1] += w * h / 3; wo[e] += w * h / 6;
    }
    kd[e] += k / h; kd[e + 1] += k / h; ko[e] -= k / h;
  }
  for (int side = 0; side < 2; ++side) {
    if (!(side ? fixed_hi : fixed_lo)) continue;
    const size_t at = side ? n : 0;
    for (int arr = 0; arr < na; arr += 2) {
      double *dg = md + (size_t)arr * nl, *of = dg + nl;
      dg[at] = arr == na - 2 ? 1.0 : 0.0;
      if (!side) of[0] = 0; else if (n) of[n - 1] = 0;
    }
  }
  return c;
}

}  // namespace poro

// Host-only: the 1D coefficient arrays of the line solve that PORO_PREC_FDM runs along the slowest direction when a per-cell k / mu is set (kernels_fdm.hip:
// k_q1_line_solve).  No HIP, no project header: compiles into the device library and into stand-alone checks alike.  (What is common to every per-cell field,
// the classification by layers among it: cell_field.hpp.)
#pragma once
#include <cstddef>
#include <vector>

namespace poro {

// [md | mo | wd | wo | kd | ko], nl = hcell.size() + 1 entries each: diagonal and off-diagonal (entry k couples nodes k and k + 1; entry nl - 1 is 0) of the 1D Q1
// matrices Mz (mass), Mz^kappa (mass weighted with the layer values) and Kz^kappa (weighted Laplace) on the line with cell sizes hcell.
// fixed_lo / fixed_hi: the end node is prescribed - its row and column leave the system: identity row (md = wd = 0, kd = 1), no coupling; the kernel zeroes its right-hand side.
inline std::vector<double> perm_line_coefficients(const std::vector<double> &hcell, const std::vector<double> &layer, bool fixed_lo, bool fixed_hi) {
  const size_t n = hcell.size(), nl = n + 1;
  std::vector<double> c(6 * nl, 0.0);
  double *md = c.data(), *mo = md + nl, *wd = mo + nl, *wo = wd + nl, *kd = wo + nl, *ko = kd + nl;
  for (size_t e = 0; e < n; ++e) {
    const double h = hcell[e], k = layer[e];
    md[e] += h / 3; md[e + 1] += h / 3; mo[e] += h / 6;
    wd[e] += k * h / 3; wd[e + 1] += k * h / 3; wo[e] += k * h / 6;
    kd[e] += k / h; kd[e + 1] += k / h; ko[e] -= k / h;
  }
  if (fixed_lo) { md[0] = wd[0] = 0; kd[0] = 1; mo[0] = wo[0] = ko[0] = 0; }
  if (fixed_hi) { md[n] = wd[n] = 0; kd[n] = 1; if (n) mo[n - 1] = wo[n - 1] = ko[n - 1] = 0; }
  return c;
}

// The same for a layered diagonal tensor diag(kx, ky[, kz]) (poro_ctx_set_cell_permeability_tensor; k_q1_line_solve_tensor).  In the eigenbasis of the leading
// directions the line system of mode (p, q) is  a Mz + lam_x[p] Mz^kx + lam_y[q] Mz^ky + Kz^kz  (2D: a My + lam_x[p] My^kx + Ky^ky): every leading direction brings
// its own weighted mass line, the line direction's component weights the Laplace line.
// [md | mo | w0d | w0o | (w1d | w1o) | kd | ko]: 2 (dim + 1) arrays of nl = hcell.size() + 1 entries; layer[d]: the layer values of component d, d < dim.
inline std::vector<double> perm_tensor_line_coefficients(int dim, const std::vector<double> &hcell, const std::vector<double> *layer, bool fixed_lo, bool fixed_hi) {
  const size_t n = hcell.size(), nl = n + 1; const int na = 2 * (dim + 1);
  std::vector<double> c((size_t)na * nl, 0.0);
  double *md = c.data(), *mo = md + nl, *kd = md + (size_t)(na - 2) * nl, *ko = kd + nl;
  for (size_t e = 0; e < n; ++e) {
    const double h = hcell[e], k = layer[dim - 1][e];
    md[e] += h / 3; md[e + 1] += h / 3; mo[e] += h / 6;
    for (int d = 0; d + 1 < dim; ++d) {
      double *wd = md + (size_t)(2 + 2 * d) * nl, *wo = wd + nl; const double w = layer[d][e];
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

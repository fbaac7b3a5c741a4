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

}  // namespace poro

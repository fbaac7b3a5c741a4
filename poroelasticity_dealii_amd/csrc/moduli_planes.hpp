// Host-only: the per-plane weight table of the structured box operator for layered per-cell moduli (kernels_kron_lm.hip).  lambda and G are constant within every
// cell layer of the slowest direction; along that direction the 1D matrices of the Kronecker form carry the weight, Mz^w = sum_l w_l M_l (K, C alike), so a row of a
// weighted band is the sum of the two one-sided halves of the unweighted row, each times the weight of the layer on its side.  Per node plane the table holds those two
// weight pairs.  No HIP, no project header (the stand-alone check tests/moduli_planes_check.cpp runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <stdexcept>
#include <vector>

namespace poro {

constexpr int kModuliPlaneStride = 4;   // doubles per node plane: lambda_lo, G_lo, lambda_hi, G_hi

// k = 1 | 2: degree of the displacement space; layer_lam / layer_G: one value per cell layer, n of them.  Node plane p of the k n + 1 planes:
//   vertex plane (p % k == 0) between the layers lo = p / k - 1 and hi = p / k: (lambda, G) of lo, then of hi; zeros where the box ends (no layer on that side)
//   mid plane (k == 2, p odd) inside layer p / 2: that layer's pair on both sides
inline std::vector<double> moduli_plane_table(int k, const std::vector<double> &layer_lam, const std::vector<double> &layer_G) {
  if (k != 1 && k != 2) throw std::runtime_error("moduli_plane_table: degree 1 or 2");
  if (layer_lam.empty() || layer_lam.size() != layer_G.size()) throw std::runtime_error("moduli_plane_table: one lambda and one G per cell layer, at least one layer");
  const size_t n = layer_lam.size(), np = (size_t)k * n + 1;
  std::vector<double> t(np * kModuliPlaneStride, 0.0);
  for (size_t p = 0; p < np; ++p) {
    double *e = t.data() + p * kModuliPlaneStride;
    if (p % (size_t)k) { const size_t l = p / (size_t)k; e[0] = e[2] = layer_lam[l]; e[1] = e[3] = layer_G[l]; continue; }
    const size_t hi = p / (size_t)k;
    if (hi > 0) { e[0] = layer_lam[hi - 1]; e[1] = layer_G[hi - 1]; }
    if (hi < n) { e[2] = layer_lam[hi]; e[3] = layer_G[hi]; }
  }
  return t;
}

}  // namespace poro

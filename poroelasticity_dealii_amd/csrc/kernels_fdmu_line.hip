// Line solve of the block fast diagonalisation of the DISPLACEMENT system with per-cell moduli layered along the slowest direction (poro_ctx_set_cell_moduli; the
// mathematics and the host twin of both kernels: moduli_line.hpp).  Between the forward and the backward x / y transforms of fdmu_apply (stages 0 and 1) the planar
// intermediate array [component][z][y][x] holds, per component c and mode column (p, q), the right-hand side of one SPD banded system along z,
//   T = lam0_c[p] Mz^{w(c,0)} + lam1_c[q] Mz^{w(c,1)} + Kz^{w(c,2)},    bandwidth KU (tridiagonal for Q1, pentadiagonal for Q2).
// T does not depend on dt: k_fdmu_line_factor runs once per field and stores the reciprocal pivots and the multipliers of the banded L D L^T factorisation (no pivoting),
// (KU + 1) doubles per dof; k_fdmu_line_solve is then a forward sweep, a scaling and a backward sweep without a division.
// One lane per column, one component per blockIdx.y: the 1D coefficient arrays are wave-uniform, consecutive lanes touch consecutive addresses of a plane.
// End conditions: a Dirichlet end face of the line direction is an identity row of T (host arrays) with a zero right-hand side (here); a column whose x or y mode was
// removed (eigenvalue not finite in LineTables) is stored as exact zeros and never meets the placeholder in a product.
#include "common.hpp"

namespace poro {
namespace {

constexpr int kLineBlock = 256;

__device__ __forceinline__ bool mode_removed(double l0, double l1) { return !(fabs(l0) < 1e300 && fabs(l1) < 1e300); }   // (false for NaN as well)

// the eigenvalues of the column: lam0 by x position; lam1 by y position in 3D, absent (0) in 2D
__device__ __forceinline__ void column_modes(const FdmuLineArgs &a, int c, int64_t col, double &l0, double &l1) {
  const int64_t q = col / a.n0; const int p = (int)(col - q * a.n0);
  l0 = a.lam0[c][p]; l1 = a.lam1[c] ? a.lam1[c][q] : 0.0;
}

template <int KU> __global__ void __launch_bounds__(kLineBlock)
k_fdmu_line_factor(FdmuLineArgs a, double *__restrict__ fac) {
  const int64_t col = (int64_t)blockIdx.x * kLineBlock + threadIdx.x;
  if (col >= a.ncol) return;
  const int c = blockIdx.y, nl = a.nl;
  const int64_t plane = a.ncol, arr = (int64_t)nl * plane;
  double *inv = fac + (int64_t)c * (KU + 1) * arr + col, *m1 = inv + arr, *m2 = KU == 2 ? inv + 2 * arr : inv;   // (m2: KU == 2 only)
  double l0, l1; column_modes(a, c, col, l0, l1);
  if (mode_removed(l0, l1)) {
    for (int i = 0; i < nl; ++i) { inv[(int64_t)i * plane] = 0.0; m1[(int64_t)i * plane] = 0.0; if (KU == 2) m2[(int64_t)i * plane] = 0.0; }
    return;
  }
  const int per = (KU + 1) * nl;
  const double *B0 = a.coef + (int64_t)c * 3 * per, *B1 = B0 + per, *B2 = B1 + per;       // [band][node] of the three 1D matrices, wave-uniform
  double d1 = 0, d2 = 0, p1 = 0, p2 = 0, pp2 = 0;       // d_{i-1}, d_{i-2}, m1[i-1], m2[i-1], m2[i-2]
  for (int i = 0; i < nl; ++i) {
    const double t0 = fma(l0, B0[i], fma(l1, B1[i], B2[i])), t1 = fma(l0, B0[nl + i], fma(l1, B1[nl + i], B2[nl + i]));
    const double d = t0 - p1 * p1 * d1 - pp2 * pp2 * d2, r = 1.0 / d;
    const double m = (t1 - p2 * p1 * d1) * r;
    double b = 0.0;
    if (KU == 2) b = fma(l0, B0[2 * nl + i], fma(l1, B1[2 * nl + i], B2[2 * nl + i])) * r;
    inv[(int64_t)i * plane] = r; m1[(int64_t)i * plane] = m; if (KU == 2) m2[(int64_t)i * plane] = b;
    d2 = d1; d1 = d; pp2 = p2; p2 = b; p1 = m;
  }
}

// in place on v = [component][nl][ncol]
template <int KU> __global__ void __launch_bounds__(kLineBlock)
k_fdmu_line_solve(FdmuLineArgs a, const double *__restrict__ fac, double *__restrict__ v) {
  const int64_t col = (int64_t)blockIdx.x * kLineBlock + threadIdx.x;
  if (col >= a.ncol) return;
  const int c = blockIdx.y, nl = a.nl;
  const int64_t plane = a.ncol, arr = (int64_t)nl * plane;
  const double *inv = fac + (int64_t)c * (KU + 1) * arr + col, *m1 = inv + arr, *m2 = KU == 2 ? inv + 2 * arr : inv;
  double *x = v + (int64_t)c * arr + col;
  double l0, l1; column_modes(a, c, col, l0, l1);
  if (mode_removed(l0, l1)) { for (int i = 0; i < nl; ++i) x[(int64_t)i * plane] = 0.0; return; }
  const bool fixed_lo = a.fixed[c][0] != 0, fixed_hi = a.fixed[c][1] != 0;
  double y1 = 0, y2 = 0, p1 = 0, p2 = 0, pp2 = 0;
  for (int i = 0; i < nl; ++i) {
    const int64_t at = (int64_t)i * plane;
    const double b = ((i == 0 && fixed_lo) || (i == nl - 1 && fixed_hi)) ? 0.0 : x[at];
    const double y = b - p1 * y1 - pp2 * y2;
    x[at] = y * inv[at];
    y2 = y1; y1 = y; pp2 = p2; p2 = KU == 2 ? m2[at] : 0.0; p1 = m1[at];
  }
  double x1 = 0, x2 = 0;
  for (int i = nl - 1; i >= 0; --i) {
    const int64_t at = (int64_t)i * plane;
    double t = x[at] - m1[at] * x1;
    if (KU == 2) t -= m2[at] * x2;
    x[at] = t; x2 = x1; x1 = t;
  }
}

}  // namespace

void fdmu_line_factor(hipStream_t s, int ku, int ncomp, const FdmuLineArgs &a, double *fac) {
  if (ku != 1 && ku != 2) throw Error("fdmu_line_factor: degree 1 or 2");
  if (!a.ncol || !a.nl) return;
  const dim3 grid((unsigned)((a.ncol + kLineBlock - 1) / kLineBlock), (unsigned)ncomp);
  if (ku == 2) hipLaunchKernelGGL(k_fdmu_line_factor<2>, grid, dim3(kLineBlock), 0, s, a, fac);
  else hipLaunchKernelGGL(k_fdmu_line_factor<1>, grid, dim3(kLineBlock), 0, s, a, fac);
}
void fdmu_line_solve(hipStream_t s, int ku, int ncomp, const FdmuLineArgs &a, const double *fac, double *v) {
  if (ku != 1 && ku != 2) throw Error("fdmu_line_solve: degree 1 or 2");
  if (!a.ncol || !a.nl) return;
  const dim3 grid((unsigned)((a.ncol + kLineBlock - 1) / kLineBlock), (unsigned)ncomp);
  if (ku == 2) hipLaunchKernelGGL(k_fdmu_line_solve<2>, grid, dim3(kLineBlock), 0, s, a, fac, v);
  else hipLaunchKernelGGL(k_fdmu_line_solve<1>, grid, dim3(kLineBlock), 0, s, a, fac, v);
}

}  // namespace poro

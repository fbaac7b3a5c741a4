// Stand-alone check of csrc/stress_measures.hpp (principal values, invariants and the Mohr-Coulomb function of kernels_stress.hip: k_stress_measures).  For a list of
// symmetric 3 x 3 states - a triple root, double roots, a double root perturbed by 1e-9 relative, pure shear, plane-strain states whose out-of-plane stress is the
// largest, the middle and the smallest principal value, and dense states rotated out of the axes - it prints one line per state with the packed tensor
// (xx, xy, xz, yy, yz, zz) and the six measures at 17 digits; tests/test_stress_cpu.py compares them with NumPy.  Its own checks: descending order, the trace and the
// Frobenius norm reproduced by the eigenvalues, f = 0 without a criterion.  Built with -fsanitize=address,undefined and run directly; the exit code names the state.
#include <cmath>
#include <cstdio>
#include "stress_measures.hpp"

using namespace poro;

// R diag(d) R^T for the rotation R = Rz(a) Ry(b) Rx(c), packed
static void rotated(const double d[3], double a, double b, double c, double (&s)[6]) {
  const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b), cc = std::cos(c), sc = std::sin(c);
  const double R[3][3] = {{ca * cb, ca * sb * sc - sa * cc, ca * sb * cc + sa * sc}, {sa * cb, sa * sb * sc + ca * cc, sa * sb * cc - ca * sc}, {-sb, cb * sc, cb * cc}};
  double T[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { T[i][j] = 0; for (int k = 0; k < 3; ++k) T[i][j] += R[i][k] * d[k] * R[j][k]; }
  s[0] = T[0][0]; s[1] = 0.5 * (T[0][1] + T[1][0]); s[2] = 0.5 * (T[0][2] + T[2][0]); s[3] = T[1][1]; s[4] = 0.5 * (T[1][2] + T[2][1]); s[5] = T[2][2];
}

static int report(int id, const char *name, const double (&s)[6]) {
  const double sin_phi = std::sin(0.5), c_cos_phi = 2.0e6 * std::cos(0.5);
  double m[kStressMeasures], m0[kStressMeasures];
  stress_measures(s, true, sin_phi, c_cos_phi, m);
  stress_measures(s, false, sin_phi, c_cos_phi, m0);
  double scale = 0;
  for (int i = 0; i < 6; ++i) scale = std::fmax(scale, std::fabs(s[i]));
  if (!(m[0] >= m[1] && m[1] >= m[2])) return id;
  const double tr = s[0] + s[3] + s[5], fro = s[0] * s[0] + s[3] * s[3] + s[5] * s[5] + 2 * (s[1] * s[1] + s[2] * s[2] + s[4] * s[4]);
  if (std::fabs((m[0] + m[1] + m[2]) - tr) > 1e-14 * 3 * scale) return 32 + id;
  if (std::fabs((m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) - fro) > 1e-14 * 9 * scale * scale) return 64 + id;
  if (m0[5] != 0.0 || m0[0] != m[0] || m0[4] != m[4]) return 96 + id;
  std::printf("%s: s %.17g %.17g %.17g %.17g %.17g %.17g -> %.17g %.17g %.17g %.17g %.17g %.17g\n", name, s[0], s[1], s[2], s[3], s[4], s[5], m[0], m[1], m[2], m[3], m[4], m[5]);
  return 0;
}

int main() {
  const double a = 3.7e6;
  int rc, id = 0;
  { const double s[6] = {a, 0, 0, a, 0, a}; if ((rc = report(++id, "triple", s))) return rc; }
  { const double s[6] = {0, 0, 0, 0, 0, a}; if ((rc = report(++id, "double_axis", s))) return rc; }
  { const double s[6] = {0, a, 0, 0, 0, 0}; if ((rc = report(++id, "pure_shear", s))) return rc; }
  { const double s[6] = {0, 0, 0, 0, 0, 0}; if ((rc = report(++id, "zero", s))) return rc; }
  { const double d[3] = {a, a, a}; double s[6]; rotated(d, 0.7, -0.4, 1.1, s); if ((rc = report(++id, "triple_rotated", s))) return rc; }
  { const double d[3] = {-a, -a, 2 * a}; double s[6]; rotated(d, 0.7, -0.4, 1.1, s); if ((rc = report(++id, "double_rotated", s))) return rc; }
  { const double d[3] = {a, a * (1 + 1e-9), -0.3 * a}; double s[6]; rotated(d, -1.3, 0.9, 0.2, s); if ((rc = report(++id, "double_perturbed", s))) return rc; }
  { const double d[3] = {a * (1 - 1e-9), a, a * (1 + 1e-9)}; double s[6]; rotated(d, 0.3, 0.5, -0.8, s); if ((rc = report(++id, "triple_perturbed", s))) return rc; }
  { const double d[3] = {2.5 * a, -1.5 * a, 0.25 * a}; double s[6]; rotated(d, 2.1, -0.6, 0.4, s); if ((rc = report(++id, "dense", s))) return rc; }
  // plane strain: in-plane block (xx, xy, yy) and zz = nu (xx + yy)
  { const double s[6] = {-a, 0.2 * a, 0, -2 * a, 0, 0.3 * -3 * a}; if ((rc = report(++id, "plane_zz_largest", s))) return rc; }
  { const double s[6] = {2 * a, 0.5 * a, 0, -a, 0, 0.3 * a}; if ((rc = report(++id, "plane_zz_middle", s))) return rc; }
  { const double s[6] = {2 * a, 0.2 * a, 0, 3 * a, 0, 0.3 * 5 * a}; if ((rc = report(++id, "plane_zz_smallest", s))) return rc; }
  { const double s[6] = {1e-300, 1e-310, 0, 1e-300, 0, -1e-300}; if ((rc = report(++id, "tiny", s))) return rc; }
  std::printf("stress_measures_check ok\n");
  return 0;
}

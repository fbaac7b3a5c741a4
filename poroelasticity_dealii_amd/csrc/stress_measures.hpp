// Host + device: principal values, invariants and the Mohr-Coulomb function of a symmetric 3 x 3 stress (kernels_stress.hip: k_stress_measures; definitions:
// include/poroel_hip.h, poro_disp_cell_measures).  Free of HIP types and of project headers: the kernel evaluates the same functions the stand-alone check
// tests/stress_measures_check.cpp runs under the sanitizers.
//   packed order of a symmetric 3 x 3 tensor: xx, xy, xz, yy, yz, zz (the order of PORO_VEC_STRAIN0 + e in 3D)
//   eigenvalues: kStressJacobiSweeps cyclic Jacobi sweeps (pairs (0,1), (0,2), (1,2), Rutishauser's update through t = tan of the rotation angle).  Every rotation is an
//   exact similarity up to rounding, so repeated and nearly repeated eigenvalues come out to a few ulps of max|s| - the acos closed form loses half the digits of the two
//   close ones there.  A 3 x 3 matrix converges quadratically after the second sweep; the count is fixed so that every lane of a wave does the same work, and a pair
//   whose off-diagonal entry is already exactly zero is left alone.  Everything lives in named scalars: no array is indexed at run time.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PORO_STRESS_HD __host__ __device__
#else
#define PORO_STRESS_HD
#endif

namespace poro {

constexpr int kStressJacobiSweeps = 8;
constexpr int kStressMeasures = 6;      // columns per cell: s1, s2, s3, mean, von Mises, Mohr-Coulomb f

// one Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix; r is the third index: app, aqq, apq and the two entries arp, arq that couple the plane to r
PORO_STRESS_HD inline void stress_jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  // the smaller root of t^2 + 2 theta t - 1 = 0; |theta| = inf (apq negligible against the gap) gives t = 0
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
  const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  app -= t * apq; aqq += t * apq; apq = 0.0;
  const double p = arp, q = arq;
  arp = p - s * (q + tau * p);
  arq = q + s * (p - tau * q);
}

// eigenvalues of the packed symmetric tensor s, descending: ev[0] >= ev[1] >= ev[2]
PORO_STRESS_HD inline void stress_principal(const double (&s)[6], double (&ev)[3]) {
  double a00 = s[0], a01 = s[1], a02 = s[2], a11 = s[3], a12 = s[4], a22 = s[5];
  for (int sweep = 0; sweep < kStressJacobiSweeps; ++sweep) {
    stress_jacobi_rotate(a00, a11, a01, a02, a12);
    stress_jacobi_rotate(a00, a22, a02, a01, a12);
    stress_jacobi_rotate(a11, a22, a12, a01, a02);
  }
  double e0 = a00, e1 = a11, e2 = a22, t;
  if (e0 < e1) { t = e0; e0 = e1; e1 = t; }
  if (e1 < e2) { t = e1; e1 = e2; e2 = t; }
  if (e0 < e1) { t = e0; e0 = e1; e1 = t; }
  ev[0] = e0; ev[1] = e1; ev[2] = e2;
}

// mean stress tr / 3 and von Mises stress sqrt(3 J2), J2 from the differences of the normal stresses (no cancellation against the mean)
PORO_STRESS_HD inline double stress_mean(const double (&s)[6]) { return (s[0] + s[3] + s[5]) / 3.0; }
PORO_STRESS_HD inline double stress_von_mises(const double (&s)[6]) {
  const double d0 = s[0] - s[3], d1 = s[3] - s[5], d2 = s[5] - s[0];
  const double j2 = (d0 * d0 + d1 * d1 + d2 * d2) / 6.0 + (s[1] * s[1] + s[2] * s[2] + s[4] * s[4]);
  return std::sqrt(3.0 * j2);
}
// Mohr-Coulomb function, tension positive: f = (s1 - s3) / 2 + (s1 + s3) / 2 sin(phi) - c cos(phi); f >= 0: the envelope is reached
PORO_STRESS_HD inline double stress_mohr_coulomb(double s1, double s3, double sin_phi, double c_cos_phi) { return 0.5 * (s1 - s3) + 0.5 * (s1 + s3) * sin_phi - c_cos_phi; }

// the six columns of one cell; with_mc false: f = 0
PORO_STRESS_HD inline void stress_measures(const double (&s)[6], bool with_mc, double sin_phi, double c_cos_phi, double (&out)[kStressMeasures]) {
  double ev[3];
  stress_principal(s, ev);
  out[0] = ev[0]; out[1] = ev[1]; out[2] = ev[2];
  out[3] = stress_mean(s);
  out[4] = stress_von_mises(s);
  out[5] = with_mc ? stress_mohr_coulomb(ev[0], ev[2], sin_phi, c_cos_phi) : 0.0;
}

}  // namespace poro

// Stand-alone check of csrc/darcy_faces.hpp (the face quadrature of the boundary discharge, kernels_darcy.hip): for a unit cell and a sheared (affine) cell, in 2D
// and 3D, every local face f = 2 d + side must give an OUTWARD n dS at every face point - along the vector from the cell's centre to the face's centre - and its
// weights times |n dS| must sum to the face measure (unit cell: 1; sheared cell: the length of the image edge / the area of the image parallelogram); the face points
// lie on the face, inside it, and the points of a face are distinct.  n dS is built as the header says: sign * T_t0 x T_t1 (3D), sign * rot * (T_y, -T_x) (2D), from
// the tangents of the face's own map.  Prints one line per face, then "darcy_faces_check ok".  Built by tests/test_darcy_cpu.py with -fsanitize=address,undefined
// and run directly; the exit code names the check that failed.
#include <cmath>
#include <cstdio>
#include "darcy_faces.hpp"

using namespace poro;

// affine cell x = A xi + b (A = identity: the unit cell)
struct Cell { int dim; double A[3][3]; double b[3]; };

static void image(const Cell &c, const double *xi, double *x) {
  for (int r = 0; r < c.dim; ++r) { x[r] = c.b[r]; for (int k = 0; k < c.dim; ++k) x[r] += c.A[r][k] * xi[k]; }
}

static int check_cell(const Cell &c, const char *name) {
  const int dim = c.dim;
  double centre_ref[3] = {0.5, 0.5, 0.5}, centre[3];
  image(c, centre_ref, centre);
  for (int f = 0; f < 2 * dim; ++f) {
    const int d = f >> 1, side = f & 1, nq = darcy_face_points(dim);
    const int t0 = darcy_face_tangent(dim, d, 0), t1 = dim == 3 ? darcy_face_tangent(dim, d, 1) : -1;
    if (t0 == d || t0 < 0 || t0 >= dim || (dim == 3 && (t1 == d || t1 == t0 || t1 < 0 || t1 >= dim))) return 10 + f;
    // the face measure of the affine image: |T_t0| in 2D, |T_t0 x T_t1| in 3D
    double T0[3] = {0, 0, 0}, T1[3] = {0, 0, 0};
    for (int r = 0; r < dim; ++r) { T0[r] = c.A[r][t0]; if (dim == 3) T1[r] = c.A[r][t1]; }
    double N[3] = {0, 0, 0};
    if (dim == 2) { N[0] = darcy_face_rot2d(d) * T0[1]; N[1] = -darcy_face_rot2d(d) * T0[0]; }
    else { N[0] = T0[1] * T1[2] - T0[2] * T1[1]; N[1] = T0[2] * T1[0] - T0[0] * T1[2]; N[2] = T0[0] * T1[1] - T0[1] * T1[0]; }
    for (int r = 0; r < 3; ++r) N[r] *= darcy_face_sign(f);
    const double measure = std::sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    double face_ref[3] = {0.5, 0.5, 0.5}, face_centre[3];
    face_ref[d] = side;
    image(c, face_ref, face_centre);
    double sum = 0, wsum = 0, points[4][3];
    for (int q = 0; q < nq; ++q) {
      for (int k = 0; k < dim; ++k) {
        const double v = darcy_face_point(dim, f, q, k);
        points[q][k] = v;
        if (k == d ? v != (double)side : !(v > 0.0 && v < 1.0)) return 30 + f;         // on the face, strictly inside it
      }
      for (int p = 0; p < q; ++p) { bool same = true; for (int k = 0; k < dim; ++k) same = same && points[p][k] == points[q][k]; if (same) return 50 + f; }
      // (an affine cell: the tangents, hence n dS, are the same at every point)
      double out = 0;
      for (int r = 0; r < dim; ++r) out += N[r] * (face_centre[r] - centre[r]);
      if (!(out > 0)) return 70 + f;                                                   // outward
      sum += darcy_face_weight(dim) * measure; wsum += darcy_face_weight(dim);
    }
    if (std::fabs(wsum - 1.0) > 1e-15) return 90 + f;
    if (std::fabs(sum - measure) > 1e-14 * measure) return 110 + f;
    std::printf("%s face %d: sign %+.0f tangents %d %d measure %.17g\n", name, f, darcy_face_sign(f), t0, t1, sum);
  }
  // the Gauss points: symmetric about 1/2 and exact for x^2 and x^3 on [0, 1]
  const double a = darcy_gauss(0), b = darcy_gauss(1);
  if (std::fabs(a + b - 1.0) > 1e-15 || std::fabs(0.5 * (a * a + b * b) - 1.0 / 3) > 1e-15 || std::fabs(0.5 * (a * a * a + b * b * b) - 0.25) > 1e-15) return 5;
  return 0;
}

int main() {
  const Cell unit2{2, {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, {0, 0, 0}}, unit3{3, {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, {0, 0, 0}};
  const Cell shear2{2, {{1.0, 0.35, 0}, {-0.2, 0.9, 0}, {0, 0, 1}}, {0.3, -1.1, 0}};
  const Cell shear3{3, {{1.0, 0.3, 0.2}, {0.1, 1.1, -0.25}, {-0.15, 0.2, 0.9}}, {0.3, -1.1, 2.0}};
  int rc;
  if ((rc = check_cell(unit2, "unit2"))) return rc;
  if ((rc = check_cell(unit3, "unit3"))) return rc;
  if ((rc = check_cell(shear2, "shear2"))) return 128 + rc / 2;
  if ((rc = check_cell(shear3, "shear3"))) return 192 + rc / 4;
  std::printf("darcy_faces_check ok\n");
  return 0;
}

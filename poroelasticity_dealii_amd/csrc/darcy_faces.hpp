// Host-only: the face quadrature behind the boundary discharge Q_b = int_F q . n dS (kernels_darcy.hip; definition: include/poroel_hip.h, poro_pres_boundary_discharge).
//   local face f = 2 d + side of a cell (d the normal direction, side 0 low | 1 high), tensorised Gauss(2) on the face, x fastest: point q = q0 + 2 q1 has the reference
//   coordinates  xi[d] = side,  xi[t0] = gauss(q0),  xi[t1] = gauss(q1)  with (t0, t1) = darcy_face_tangent(dim, d, 0 | 1) (2D: t0 alone), every weight 1 / 2^(dim-1);
//   n dS = darcy_face_sign(f) * T_t0 x T_t1 with T_t = d x / d xi_t on the face (MappingQ1) - the column d of det(J) J^-T, the convention of the Neumann term and of the
//   Kelly indicator; 2D: n dS = darcy_face_sign(f) * darcy_face_rot2d(d) * (T_y, -T_x), T = T_t0.  For a cell of positive orientation the result points outward.
// Everything is constexpr and free of HIP and of project headers: the kernels evaluate the same functions the stand-alone check tests/darcy_faces_check.cpp runs under the
// sanitizers.
#pragma once

namespace poro {

constexpr double kDarcyGauss[2] = {0.5 - 0.28867513459481288225, 0.5 + 0.28867513459481288225};   // Gauss(2) on [0, 1]; both weights 1/2

constexpr double darcy_gauss(int i) { return i ? kDarcyGauss[1] : kDarcyGauss[0]; }
constexpr int darcy_face_points(int dim) { return 1 << (dim - 1); }
constexpr double darcy_face_weight(int dim) { return 1.0 / (double)(1 << (dim - 1)); }
// outward factor of column d of det(J) J^-T on local face f = 2 d + side
constexpr double darcy_face_sign(int f) { return (f & 1) ? 1.0 : -1.0; }
// k-th tangential direction of a face with normal direction d, in the cyclic order that makes T_t0 x T_t1 the column d of det(J) J^-T: 3D (1, 2), (2, 0), (0, 1); 2D the other direction
constexpr int darcy_face_tangent(int dim, int d, int k) { return dim == 2 ? 1 - d : (d + 1 + k) % 3; }
constexpr double darcy_face_rot2d(int d) { return d == 0 ? 1.0 : -1.0; }
// reference coordinate k of face point q of local face f.  The points are enumerated over the tangential directions in ASCENDING direction order, x fastest (the order of
// the Kelly kernel), which the cyclic pair above permutes for d = 1 only; the rule is symmetric, the sum is the same
constexpr double darcy_face_point(int dim, int f, int q, int k) {
  const int d = f >> 1;
  if (k == d) return (double)(f & 1);
  const int first = d == 0 ? 1 : 0;                  // the lower tangential direction
  return k == first ? darcy_gauss(q & 1) : darcy_gauss((q >> 1) & 1);
}

}  // namespace poro

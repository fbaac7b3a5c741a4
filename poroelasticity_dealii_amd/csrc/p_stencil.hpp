// One row of y = (a M + kappa K) x for the Q1 pressure space on a uniform box .
// M = Mx (x) My (x) Mz, K = Kx (x) My (x) Mz + Mx (x) Ky (x) Mz + Mx (x) My (x) Kz with the tridiagonal 1D Q1 matrices
// M1 = h/6 (1,4,1), K1 = 1/h (-1,2,-1) (boundary rows: h/6 (2,1), 1/h (1,-1)) -- what MatrixCreator::create_mass_matrix /
// create_laplace_matrix (PoroElasticPressureSolver.h:96-101) produce on such a mesh.
//
// The row is split into its loads and its sum.  The vector lives in L2, so a row costs what its chain of dependent round trips costs: with one exec-mask
// branch per neighbour (`if (w != 0) acc = fma(w, x[..], acc)`) the compiler waits for every load before it enters the next branch - 27 round trips in a
// row (k_p_stencil<3>: 13 us, k_p_residual_stencil<3>: 32 us at 73^3 nodes).  Here every neighbour index is clamped into the box, all loads are unconditional and
// issued before the first use, and the weight test is a select: a missing neighbour has weight zero and leaves the sum untouched whatever the clamped load
// returned, and the FMAs keep their order, so the result is the same bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace poro {

template <int DIM> struct PStencilTaps { static constexpr int N = DIM == 2 ? 9 : 27; double v[N]; };

// the 3^DIM neighbour values of `node`, index = di + 3 dj (+ 9 dk); neighbours outside the box: the value of the nearest node inside (never used, see above)
template <int DIM> __device__ __forceinline__ void p_stencil_load(int n0, int n1, int n2, int64_t node, const double *__restrict__ x, PStencilTaps<DIM> &T) {
  const int idx[3] = {(int)(node % n0), (int)((node / n0) % n1), (int)(node / ((int64_t)n0 * n1))};
  const int nd[3] = {n0, n1, n2};
  int at[3][3];                // [direction][offset -1,0,+1]: the clamped coordinate
#pragma unroll
  for (int d = 0; d < DIM; ++d) { at[d][0] = max(idx[d] - 1, 0); at[d][1] = idx[d]; at[d][2] = min(idx[d] + 1, nd[d] - 1); }
  if constexpr (DIM == 2) {
#pragma unroll
    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
      for (int di = 0; di < 3; ++di) T.v[3 * dj + di] = x[(int64_t)at[1][dj] * n0 + at[0][di]];
  } else {
#pragma unroll
    for (int dk = 0; dk < 3; ++dk)
#pragma unroll
      for (int dj = 0; dj < 3; ++dj)
#pragma unroll
        for (int di = 0; di < 3; ++di) T.v[9 * dk + 3 * dj + di] = x[((int64_t)at[2][dk] * n1 + at[1][dj]) * n0 + at[0][di]];
  }
}

template <int DIM> __device__ __forceinline__ double p_stencil_sum(int n0, int n1, int n2, double h0, double h1, double h2, double a, double kappa, int64_t node,
                                                                   const PStencilTaps<DIM> &T) {
  const int idx[3] = {(int)(node % n0), (int)((node / n0) % n1), (int)(node / ((int64_t)n0 * n1))};
  const int nd[3] = {n0, n1, n2};
  const double h[3] = {h0, h1, h2};
  double M1[3][3], K1[3][3];   // [direction][offset -1,0,+1]; zero where the neighbour does not exist
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const double L = idx[d] > 0 ? 1.0 : 0.0, R = idx[d] < nd[d] - 1 ? 1.0 : 0.0;
    M1[d][0] = L * h[d] / 6; M1[d][2] = R * h[d] / 6; M1[d][1] = (L + R) * h[d] / 3;
    K1[d][0] = -L / h[d]; K1[d][2] = -R / h[d]; K1[d][1] = (L + R) / h[d];
  }
  double acc = 0;
  if constexpr (DIM == 2) {
#pragma unroll
    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
      for (int di = 0; di < 3; ++di) {
        const double wM = M1[0][di] * M1[1][dj], wK = K1[0][di] * M1[1][dj] + M1[0][di] * K1[1][dj];
        const double w = a * wM + kappa * wK;
        acc = w != 0.0 ? fma(w, T.v[3 * dj + di], acc) : acc;
      }
  } else {
#pragma unroll
    for (int dk = 0; dk < 3; ++dk)
#pragma unroll
      for (int dj = 0; dj < 3; ++dj) {
        const double mm = M1[1][dj] * M1[2][dk], km = K1[1][dj] * M1[2][dk] + M1[1][dj] * K1[2][dk];
#pragma unroll
        for (int di = 0; di < 3; ++di) {
          const double w = a * (M1[0][di] * mm) + kappa * (K1[0][di] * mm + M1[0][di] * km);
          acc = w != 0.0 ? fma(w, T.v[9 * dk + 3 * dj + di], acc) : acc;
        }
      }
  }
  return acc;
}

// ---- per-cell coefficient: y = (a M + K_kappa) x, K_kappa = sum_c K_c(kappa_c) ---------------------------------------------------------------------------------
// The row of a node is the constant mass stencil above plus, over the <= 2^DIM cells around it, the row of the weighted Q1 element Laplace matrix of a box cell,
// K_e = kx k (x) m (x) m + ky m (x) k (x) m + kz m (x) m (x) k with the 1D element matrices m = h/6 [[2, 1], [1, 2]], k = 1/h [[1, -1], [-1, 1]].  NK weights per cell:
// 1 (one k / mu: kx = ky = kz, summed before the weight multiplies) or DIM (its diagonal tensor, component d weights the derivatives along direction d).  kap holds one
// plane of cells per component, each in lattice cell order (x fastest), so that consecutive lanes read consecutive addresses of every plane.  Same discipline as
// above: the cell index is clamped into the box and loaded unconditionally, a cell outside the box gets weight 0 by a select, and cells, components and taps are
// summed in one fixed order - the result is the same bit for bit from call to call.
template <int DIM, int NK> struct PStencilCells { static constexpr int N = 1 << DIM; double w[NK][N]; };

// one component's weights of the 2^DIM cells around `node`, index = c0 + 2 c1 (+ 4 c2) with c_d = 0 for the cell on the low side of the node in direction d
template <int DIM> __device__ __forceinline__ void p_stencil_load_plane(int n0, int n1, int n2, int64_t node, const double *__restrict__ kap, double (&w)[1 << DIM]) {
  const int idx[3] = {(int)(node % n0), (int)((node / n0) % n1), (int)(node / ((int64_t)n0 * n1))};
  const int nc[3] = {n0 - 1, n1 - 1, n2 - 1};      // cells per direction (>= 1 in every direction of the box)
  int at[3][2]; bool in[3][2];
#pragma unroll
  for (int d = 0; d < DIM; ++d)
#pragma unroll
    for (int c = 0; c < 2; ++c) { const int ci = idx[d] - 1 + c; in[d][c] = ci >= 0 && ci < nc[d]; at[d][c] = min(max(ci, 0), nc[d] - 1); }
  if constexpr (DIM == 2) {
#pragma unroll
    for (int c1 = 0; c1 < 2; ++c1)
#pragma unroll
      for (int c0 = 0; c0 < 2; ++c0) { const double v = kap[(int64_t)at[1][c1] * nc[0] + at[0][c0]]; w[2 * c1 + c0] = (in[0][c0] && in[1][c1]) ? v : 0.0; }
  } else {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int c1 = 0; c1 < 2; ++c1)
#pragma unroll
        for (int c0 = 0; c0 < 2; ++c0) {
          const double v = kap[((int64_t)at[2][c2] * nc[1] + at[1][c1]) * nc[0] + at[0][c0]];
          w[4 * c2 + 2 * c1 + c0] = (in[0][c0] && in[1][c1] && in[2][c2]) ? v : 0.0;
        }
  }
}
// all NK components.  (One component: without the plane arithmetic in the source - the compiler does not fold it away without a trace: the 2D kernels take one more SGPR with it)
template <int DIM, int NK> __device__ __forceinline__ void p_stencil_load_cells(int n0, int n1, int n2, int64_t node, const double *__restrict__ kap, PStencilCells<DIM, NK> &C) {
  if constexpr (NK == 1) p_stencil_load_plane<DIM>(n0, n1, n2, node, kap, C.w[0]);
  else {
    const int64_t plane = (int64_t)(n0 - 1) * (n1 - 1) * (DIM == 3 ? n2 - 1 : 1);
#pragma unroll
    for (int k = 0; k < NK; ++k) p_stencil_load_plane<DIM>(n0, n1, n2, node, kap + k * plane, C.w[k]);
  }
}

// MASS: the a M part is summed with the taps (the Jacobian); without it the function gives K_kappa x alone
template <int DIM, int NK, bool MASS> __device__ __forceinline__ double p_stencil_sum_cells(int n0, int n1, int n2, double h0, double h1, double h2, double a, int64_t node,
                                                                                            const PStencilTaps<DIM> &T, const PStencilCells<DIM, NK> &C) {
  static_assert(NK == 1 || NK == DIM, "one weight per cell, or one per direction");
  const int idx[3] = {(int)(node % n0), (int)((node / n0) % n1), (int)(node / ((int64_t)n0 * n1))};
  const int nd[3] = {n0, n1, n2};
  const double h[3] = {h0, h1, h2};
  double M1[3][3];             // the assembled 1D mass rows, as in p_stencil_sum
  double em[3][2][3], ek[3][2][3];   // [direction][cell side][offset -1,0,+1]: the node's row of the 1D ELEMENT matrices of that cell; zero where the cell does not hold the neighbour
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const double L = idx[d] > 0 ? 1.0 : 0.0, R = idx[d] < nd[d] - 1 ? 1.0 : 0.0;
    M1[d][0] = L * h[d] / 6; M1[d][2] = R * h[d] / 6; M1[d][1] = (L + R) * h[d] / 3;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        const int own = 1 - c, other = own + o - 1;           // local vertex numbers of the node and of its neighbour in that cell
        const bool held = other == 0 || other == 1;
        em[d][c][o] = held ? (other == own ? h[d] / 3 : h[d] / 6) : 0.0;
        ek[d][c][o] = held ? (other == own ? 1.0 / h[d] : -1.0 / h[d]) : 0.0;
      }
  }
  // The weight expressions of NK = 1 and NK = DIM stay apart as they are: the compiler contracts into fma across an expression, so that a regrouped one rounds differently
  double acc = 0;
  if constexpr (DIM == 2) {
#pragma unroll
    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
      for (int di = 0; di < 3; ++di) {
        double wK = 0;
#pragma unroll
        for (int c1 = 0; c1 < 2; ++c1)
#pragma unroll
          for (int c0 = 0; c0 < 2; ++c0) {
            const bool held = (di == 1 || di == 2 * c0) && (dj == 1 || dj == 2 * c1);        // (known at compile time after unrolling)
            if (held) {
              const int cell = 2 * c1 + c0;
              if constexpr (NK == 1) wK = fma(C.w[0][cell], ek[0][c0][di] * em[1][c1][dj] + em[0][c0][di] * ek[1][c1][dj], wK);
              else {
                wK = fma(C.w[0][cell], ek[0][c0][di] * em[1][c1][dj], wK);
                wK = fma(C.w[1][cell], em[0][c0][di] * ek[1][c1][dj], wK);
              }
            }
          }
        const double w = MASS ? a * (M1[0][di] * M1[1][dj]) + wK : wK;
        acc = w != 0.0 ? fma(w, T.v[3 * dj + di], acc) : acc;
      }
  } else {
#pragma unroll
    for (int dk = 0; dk < 3; ++dk)
#pragma unroll
      for (int dj = 0; dj < 3; ++dj)
#pragma unroll
        for (int di = 0; di < 3; ++di) {
          double wK = 0;
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int c1 = 0; c1 < 2; ++c1)
#pragma unroll
              for (int c0 = 0; c0 < 2; ++c0) {
                const bool held = (di == 1 || di == 2 * c0) && (dj == 1 || dj == 2 * c1) && (dk == 1 || dk == 2 * c2);
                if (held) {
                  const int cell = 4 * c2 + 2 * c1 + c0;
                  if constexpr (NK == 1)
                    wK = fma(C.w[0][cell],
                             ek[0][c0][di] * (em[1][c1][dj] * em[2][c2][dk]) + em[0][c0][di] * (ek[1][c1][dj] * em[2][c2][dk] + em[1][c1][dj] * ek[2][c2][dk]), wK);
                  else {
                    wK = fma(C.w[0][cell], ek[0][c0][di] * (em[1][c1][dj] * em[2][c2][dk]), wK);
                    wK = fma(C.w[1][cell], em[0][c0][di] * (ek[1][c1][dj] * em[2][c2][dk]), wK);
                    wK = fma(C.w[2][cell], em[0][c0][di] * (em[1][c1][dj] * ek[2][c2][dk]), wK);
                  }
                }
              }
          const double w = MASS ? a * (M1[0][di] * (M1[1][dj] * M1[2][dk])) + wK : wK;
          acc = w != 0.0 ? fma(w, T.v[9 * dk + 3 * dj + di], acc) : acc;
        }
  }
  return acc;
}

template <int DIM> __device__ __forceinline__ double p_stencil_row(int n0, int n1, int n2, double h0, double h1, double h2, double a, double kappa, int64_t node,
                                                                   const double *__restrict__ x) {
  PStencilTaps<DIM> T;
  p_stencil_load<DIM>(n0, n1, n2, node, x, T);
  return p_stencil_sum<DIM>(n0, n1, n2, h0, h1, h2, a, kappa, node, T);
}

}  // namespace poro

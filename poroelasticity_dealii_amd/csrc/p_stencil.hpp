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

template <int DIM> __device__ __forceinline__ double p_stencil_row(int n0, int n1, int n2, double h0, double h1, double h2, double a, double kappa, int64_t node,
                                                                   const double *__restrict__ x) {
  PStencilTaps<DIM> T;
  p_stencil_load<DIM>(n0, n1, n2, node, x, T);
  return p_stencil_sum<DIM>(n0, n1, n2, h0, h1, h2, a, kappa, node, T);
}

}  // namespace poro

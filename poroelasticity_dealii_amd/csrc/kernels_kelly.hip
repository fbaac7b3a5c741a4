// Mesh adaptation on the device (refine_mesh, PoroelasticityFSS.h:447-498): the Kelly error indicator of a pressure-space vector (KellyErrorEstimator<dim>::estimate,
// :452-458) and the row kernel that carries the three pressure-space vectors to the next mesh (SolutionTransfer<dim>::interpolate, :474-497).
//
// The indicator (definition: include/poroel_hip.h, poro_pres_estimate_error) runs in two passes without atomics, so that it is bitwise reproducible:
//   k_kelly_faces  one lane per interior (sub)face: J_F = int_F [n . (grad p|_A - grad p|_B)]^2 dS with the tensorised Gauss(2) rule on the face of side A;
//   k_kelly_cells  one lane per cell: eta = sqrt(sum over the cell's faces of (diameter / 24) J_F), in the fixed order of the cell's face list.
// Every array a lane holds (vertex coordinates, nodal values, Jacobians) is indexed by compile-time constants only: the face number and the position of side B's
// points are run-time VALUES that enter through the reference coordinates at which the Q1 basis is evaluated, never through an index.  No LDS, no cross-lane traffic.
#include "common.hpp"

namespace poro {
namespace {
constexpr int kKellyBlock = 256;
constexpr double kGauss0 = 0.5 - 0.28867513459481288225, kGauss1 = 0.5 + 0.28867513459481288225;   // Gauss(2) on [0, 1]; both weights 1/2

template <int DIM> struct KellyCell { double X[1 << DIM][DIM]; double p[1 << DIM]; };

template <int DIM> __device__ inline void kelly_load(KellyCell<DIM> &K, const double *__restrict__ cell_X, const int32_t *__restrict__ cell_dofs_p, const double *__restrict__ p, int32_t cell) {
  constexpr int NV = 1 << DIM;
  const double *x = cell_X + (int64_t)cell * NV * DIM; const int32_t *d = cell_dofs_p + (int64_t)cell * NV;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int k = 0; k < DIM; ++k) K.X[v][k] = x[v * DIM + k];
    K.p[v] = p[d[v]];
  }
}

// at the reference point xi of the cell: g = J^-T grad_xi p_h (the physical gradient of the Q1 function) and cof = det(J) J^-T (MappingQ1: J[r][b] = d x_r / d xi_b)
template <int DIM> __device__ inline void kelly_grad(const KellyCell<DIM> &K, const double (&xi)[DIM], double (&g)[DIM], double (&cof)[DIM][DIM]) {
  constexpr int NV = 1 << DIM;
  double J[DIM][DIM], gh[DIM];
#pragma unroll
  for (int r = 0; r < DIM; ++r) { gh[r] = 0;
#pragma unroll
    for (int b = 0; b < DIM; ++b) J[r][b] = 0; }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double f[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) f[k] = ((v >> k) & 1) ? xi[k] : 1.0 - xi[k];
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      double dn = ((v >> b) & 1) ? 1.0 : -1.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) if (k != b) dn *= f[k];
      gh[b] = fma(K.p[v], dn, gh[b]);
#pragma unroll
      for (int r = 0; r < DIM; ++r) J[r][b] = fma(K.X[v][r], dn, J[r][b]);
    }
  }
  double det;
  if constexpr (DIM == 2) {
    cof[0][0] = J[1][1]; cof[0][1] = -J[1][0]; cof[1][0] = -J[0][1]; cof[1][1] = J[0][0];
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  } else {
    cof[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1]; cof[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2]; cof[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    cof[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2]; cof[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0]; cof[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    cof[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1]; cof[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2]; cof[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    det = J[0][0] * cof[0][0] + J[0][1] * cof[0][1] + J[0][2] * cof[0][2];
  }
  const double inv = 1.0 / det;
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    double s = 0;
#pragma unroll
    for (int b = 0; b < DIM; ++b) s = fma(cof[r][b], gh[b], s);
    g[r] = s * inv;
  }
}

// code: bits 0-2 local face of side A; bits 3 + 2 (3 j + k): twice the k-th reference coordinate IN CELL B of vertex j of A's face (0, 1 or 2: a vertex of B, or on a
// hanging face the midpoint of an edge / the centre of B's face); bits 27-29 local face of side B (not needed here)
template <int DIM> __global__ void __launch_bounds__(kKellyBlock)
k_kelly_faces(int64_t n_faces, const int32_t *__restrict__ cell_a, const int32_t *__restrict__ cell_b, const int32_t *__restrict__ code, const double *__restrict__ cell_X,
              const int32_t *__restrict__ cell_dofs_p, const double *__restrict__ p, double *__restrict__ jump) {
  const int64_t i = (int64_t)blockIdx.x * kKellyBlock + threadIdx.x;
  if (i >= n_faces) return;
  constexpr int NFV = 1 << (DIM - 1), NQ = NFV;
  const int32_t cd = code[i];
  const int fa = cd & 7, da = fa >> 1; const double side = (double)(fa & 1);
  const int t1 = da == 0 ? 1 : 0;                      // first tangential direction of the face (the second is the remaining one)
  double ref_b[NFV][DIM];
#pragma unroll
  for (int j = 0; j < NFV; ++j)
#pragma unroll
    for (int k = 0; k < DIM; ++k) ref_b[j][k] = 0.5 * (double)((cd >> (3 + 2 * (3 * j + k))) & 3);
  KellyCell<DIM> A, B;
  kelly_load<DIM>(A, cell_X, cell_dofs_p, p, cell_a[i]);
  kelly_load<DIM>(B, cell_X, cell_dofs_p, p, cell_b[i]);
  double pick[DIM];
#pragma unroll
  for (int b = 0; b < DIM; ++b) pick[b] = b == da ? 1.0 : 0.0;
  double acc = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double s = (q & 1) ? kGauss1 : kGauss0, t = (q >> 1) ? kGauss1 : kGauss0;
    double xa[DIM], xb[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      xa[k] = k == da ? side : (k == t1 ? s : t);
      double v = 0;
#pragma unroll
      for (int j = 0; j < NFV; ++j) { const double nj = ((j & 1) ? s : 1.0 - s) * (DIM == 3 ? ((j >> 1) ? t : 1.0 - t) : 1.0); v = fma(nj, ref_b[j][k], v); }
      xb[k] = v;
    }
    double ga[DIM], gb[DIM], ca[DIM][DIM], cb[DIM][DIM];
    kelly_grad<DIM>(A, xa, ga, ca);
    kelly_grad<DIM>(B, xb, gb, cb);
    // n dS = det(J) J^-T e_da on the face of side A (the convention of the Neumann term, kernels_asm.hip); its sign drops out of the square
    double jn = 0, nn = 0;
#pragma unroll
    for (int r = 0; r < DIM; ++r) {
      double nr = 0;                                     // column da of the cofactor matrix, picked by exact 0 / 1 factors (an index would be a run-time one)
#pragma unroll
      for (int b = 0; b < DIM; ++b) nr = fma(ca[r][b], pick[b], nr);
      jn = fma(nr, ga[r] - gb[r], jn); nn = fma(nr, nr, nn);
    }
    acc += (1.0 / NQ) * jn * jn / sqrt(nn);             // w_q (n . jump)^2 dS with n = N / |N|, dS = |N|
  }
  jump[i] = acc;
}

template <int DIM> __device__ inline double kelly_diameter(const double *__restrict__ x) {   // the longest vertex diagonal (v <-> NV - 1 - v)
  constexpr int NV = 1 << DIM;
  double best = 0;
#pragma unroll
  for (int v = 0; v < NV / 2; ++v) {
    double d2 = 0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) { const double d = x[(NV - 1 - v) * DIM + k] - x[v * DIM + k]; d2 = fma(d, d, d2); }
    best = fmax(best, d2);
  }
  return sqrt(best);
}

// entries of cell c: ent_ptr[c] .. ent_ptr[c + 1]; entry e = face ent_face[e] with the factor diameter(ent_hcell[e]) / 24 (the cell itself, or the coarse cell of a hanging face)
template <int DIM> __global__ void __launch_bounds__(kKellyBlock)
k_kelly_cells(int64_t n_cells, const int64_t *__restrict__ ent_ptr, const int32_t *__restrict__ ent_face, const int32_t *__restrict__ ent_hcell, const double *__restrict__ cell_X,
              const double *__restrict__ jump, double *__restrict__ eta) {
  const int64_t c = (int64_t)blockIdx.x * kKellyBlock + threadIdx.x;
  if (c >= n_cells) return;
  constexpr int NV = 1 << DIM;
  const double own = kelly_diameter<DIM>(cell_X + c * NV * DIM);
  double sum = 0;
  for (int64_t e = ent_ptr[c]; e < ent_ptr[c + 1]; ++e) {
    const int32_t hc = ent_hcell[e];
    const double h = hc == c ? own : kelly_diameter<DIM>(cell_X + (int64_t)hc * NV * DIM);
    sum = fma(h * (1.0 / 24.0), jump[ent_face[e]], sum);
  }
  eta[c] = sqrt(sum);
}

// out_e[row] = sum_k w[k] in_e[col[k]] for e = 0, 1, 2: one lane per row, the sum in the row's entry order
struct Transfer3 { const double *in[3]; double *out[3]; };
__global__ void __launch_bounds__(kKellyBlock)
k_transfer_rows3(int64_t n_rows, const int64_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ w, Transfer3 V) {
  const int64_t row = (int64_t)blockIdx.x * kKellyBlock + threadIdx.x;
  if (row >= n_rows) return;
  double a0 = 0, a1 = 0, a2 = 0;
  for (int64_t k = ptr[row]; k < ptr[row + 1]; ++k) {
    const double wk = w[k]; const int32_t j = col[k];
    a0 = fma(wk, V.in[0][j], a0); a1 = fma(wk, V.in[1][j], a1); a2 = fma(wk, V.in[2][j], a2);
  }
  V.out[0][row] = a0; V.out[1][row] = a1; V.out[2][row] = a2;
}
}  // namespace

void kelly_faces(hipStream_t s, int dim, int64_t n_faces, const int32_t *cell_a, const int32_t *cell_b, const int32_t *code, const double *cell_X, const int32_t *cell_dofs_p,
                 const double *p, double *jump) {
  if (!n_faces) return;
  const unsigned grid = (unsigned)((n_faces + kKellyBlock - 1) / kKellyBlock);
  if (dim == 2) hipLaunchKernelGGL(k_kelly_faces<2>, grid, kKellyBlock, 0, s, n_faces, cell_a, cell_b, code, cell_X, cell_dofs_p, p, jump);
  else hipLaunchKernelGGL(k_kelly_faces<3>, grid, kKellyBlock, 0, s, n_faces, cell_a, cell_b, code, cell_X, cell_dofs_p, p, jump);
}
void kelly_cells(hipStream_t s, int dim, int64_t n_cells, const int64_t *ent_ptr, const int32_t *ent_face, const int32_t *ent_hcell, const double *cell_X, const double *jump, double *eta) {
  if (!n_cells) return;
  const unsigned grid = (unsigned)((n_cells + kKellyBlock - 1) / kKellyBlock);
  if (dim == 2) hipLaunchKernelGGL(k_kelly_cells<2>, grid, kKellyBlock, 0, s, n_cells, ent_ptr, ent_face, ent_hcell, cell_X, jump, eta);
  else hipLaunchKernelGGL(k_kelly_cells<3>, grid, kKellyBlock, 0, s, n_cells, ent_ptr, ent_face, ent_hcell, cell_X, jump, eta);
}
void transfer_rows3(hipStream_t s, int64_t n_rows, const int64_t *ptr, const int32_t *col, const double *w, const double *const in[3], double *const out[3]) {
  if (!n_rows) return;
  Transfer3 V; for (int e = 0; e < 3; ++e) { V.in[e] = in[e]; V.out[e] = out[e]; }
  hipLaunchKernelGGL(k_transfer_rows3, (unsigned)((n_rows + kKellyBlock - 1) / kKellyBlock), kKellyBlock, 0, s, n_rows, ptr, col, w, V);
}

}  // namespace poro

// Flow post-processing on the device (definitions: include/poroel_hip.h, "Darcy velocity, boundary discharge and fluid mass balance"):
//   k_darcy_cells       one lane per cell: q_c = -kappa_c (grad p_h(x_c) - rho_f g) at the image of the reference centre;
//   k_darcy_bfaces      one lane per boundary face: Q_b = int_F q . n dS, tensorised Gauss(2) on the face (darcy_faces.hpp), q from the face's own cell;
//   k_darcy_label_sums  one workgroup per requested label: the sum of the Q_b of its faces, fixed face-to-lane assignment, block_sum in fixed order;
//   k_flow_balance      one pass over the pressure dofs: the six sums of the discrete balance as per-block partials (device_reduce.hpp), finished in fixed order.
// NK selects what kappa_c is: 0 the material's scalar, 1 one value per cell, DIM the per-cell diagonal tensor (componentwise product).
// As in kernels_kelly.hip every array a lane holds is indexed by compile-time constants only: the local face is a run-time VALUE that enters through the reference
// coordinates of the face points and through exact 0 / 1 factors.  Plain vector stores, no atomics, no LDS beyond block_sum's four words, no scratch.
// (The cell load and the J^-T gradient are a second copy of kelly_load / kelly_grad: sharing them through a header would have to leave the Kelly kernels' code as it is.)
#include "common.hpp"
#include "darcy_faces.hpp"
#include "device_reduce.hpp"

namespace poro {
namespace {
constexpr int kDarcyBlock = 256;

template <int DIM> struct DarcyCell { double X[1 << DIM][DIM]; double p[1 << DIM]; };

template <int DIM> __device__ inline void darcy_load(DarcyCell<DIM> &K, const double *__restrict__ cell_X, const int32_t *__restrict__ cell_dofs_p, const double *__restrict__ p, int64_t cell) {
  constexpr int NV = 1 << DIM;
  const double *x = cell_X + cell * NV * DIM; const int32_t *d = cell_dofs_p + cell * NV;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int k = 0; k < DIM; ++k) K.X[v][k] = x[v * DIM + k];
    K.p[v] = p[d[v]];
  }
}

// at the reference point xi of the cell: g = J^-T grad_xi p_h (the physical gradient of the Q1 function) and cof = det(J) J^-T (MappingQ1: J[r][b] = d x_r / d xi_b)
template <int DIM> __device__ inline void darcy_grad(const DarcyCell<DIM> &K, const double (&xi)[DIM], double (&g)[DIM], double (&cof)[DIM][DIM]) {
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

// kappa_c of cell `cell` as a diagonal: the scalar, the per-cell value, or the per-cell tensor
template <int DIM, int NK> __device__ inline void darcy_kappa(double (&kap)[DIM], double kappa, const double *__restrict__ perm_cell, int64_t cell) {
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    if constexpr (NK == 0) kap[r] = kappa;
    else if constexpr (NK == 1) kap[r] = perm_cell[cell];
    else kap[r] = perm_cell[cell * DIM + r];
  }
}

template <int DIM, int NK> __global__ void __launch_bounds__(kDarcyBlock)
k_darcy_cells(int64_t n_cells, const double *__restrict__ cell_X, const int32_t *__restrict__ cell_dofs_p, const double *__restrict__ p, double kappa,
              const double *__restrict__ perm_cell, DarcyGravity rg, double *__restrict__ q) {
  const int64_t c = (int64_t)blockIdx.x * kDarcyBlock + threadIdx.x;
  if (c >= n_cells) return;
  DarcyCell<DIM> K;
  darcy_load<DIM>(K, cell_X, cell_dofs_p, p, c);
  double xi[DIM], g[DIM], cof[DIM][DIM], kap[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) xi[k] = 0.5;
  darcy_grad<DIM>(K, xi, g, cof);
  darcy_kappa<DIM, NK>(kap, kappa, perm_cell, c);
#pragma unroll
  for (int r = 0; r < DIM; ++r) q[c * DIM + r] = -kap[r] * (g[r] - rg.v[r]);
}

template <int DIM, int NK> __global__ void __launch_bounds__(kDarcyBlock)
k_darcy_bfaces(int64_t n_bfaces, const int32_t *__restrict__ bface_cell, const int32_t *__restrict__ bface_local, const double *__restrict__ cell_X,
               const int32_t *__restrict__ cell_dofs_p, const double *__restrict__ p, double kappa, const double *__restrict__ perm_cell, DarcyGravity rg,
               double *__restrict__ Q) {
  const int64_t b = (int64_t)blockIdx.x * kDarcyBlock + threadIdx.x;
  if (b >= n_bfaces) return;
  constexpr int NQ = 1 << (DIM - 1);
  const int64_t c = bface_cell[b]; const int f = bface_local[b], d = f >> 1;
  DarcyCell<DIM> K;
  darcy_load<DIM>(K, cell_X, cell_dofs_p, p, c);
  double kap[DIM], pick[DIM];
  darcy_kappa<DIM, NK>(kap, kappa, perm_cell, c);
  const double sign = darcy_face_sign(f);
#pragma unroll
  for (int k = 0; k < DIM; ++k) pick[k] = k == d ? sign : 0.0;      // column d of the cofactor matrix with the outward sign, picked by exact factors
  double acc = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double xi[DIM], g[DIM], cof[DIM][DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) xi[k] = darcy_face_point(DIM, f, q, k);
    darcy_grad<DIM>(K, xi, g, cof);
    double qn = 0;
#pragma unroll
    for (int r = 0; r < DIM; ++r) {
      double nr = 0;                                                  // (n dS)_r
#pragma unroll
      for (int k = 0; k < DIM; ++k) nr = fma(cof[r][k], pick[k], nr);
      qn = fma(-kap[r] * (g[r] - rg.v[r]), nr, qn);
    }
    acc = fma(darcy_face_weight(DIM), qn, acc);
  }
  Q[b] = acc;
}

// workgroup l: out[l] = sum of Q[b] over the faces with bface_id[b] == labels[l]; lane t takes the faces t, t + 256, ... in ascending order
__global__ void __launch_bounds__(kDarcyBlock)
k_darcy_label_sums(int64_t n_bfaces, const int32_t *__restrict__ bface_id, const double *__restrict__ Q, const int32_t *__restrict__ labels, double *__restrict__ out) {
  __shared__ double sh[4];
  const int32_t label = labels[blockIdx.x];
  double v = 0;
  // (both loads unconditional and the loop unrolled: the loads of four faces are in flight together; a face of another label adds an exact 0.0, in the same order)
#pragma unroll 4
  for (int64_t b = threadIdx.x; b < n_bfaces; b += kDarcyBlock) { const double qb = Q[b]; v += bface_id[b] == label ? qb : 0.0; }
  v = block_sum(v, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// the six sums of the balance (FlowBalanceArgs): block partials into slabs 0 .. 5 of `partials`
__global__ void __launch_bounds__(kBlock)
k_flow_balance(FlowBalanceArgs A, double *__restrict__ partials) {
  __shared__ double sh[4];
  double s_strain = 0, s_pres = 0, s_src = 0, s_out = 0, s_free = 0, s_sq = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * kBlock) {
    const double m = A.m[i];
    s_strain = fma(m, A.c_strain * (A.ev[i] - A.ev0[i]), s_strain);
    s_pres = fma(m, A.c_pres * (A.p[i] - A.p_old[i]), s_pres);
    s_src += A.src[i];
    const double r = A.Rt[i];
    if (A.pdir_mask && A.pdir_mask[i]) s_out += r;
    else { s_free += r; s_sq = fma(r, r, s_sq); }
  }
  s_strain = block_sum(s_strain, sh); store_partial(partials, s_strain);
  s_pres = block_sum(s_pres, sh); store_partial(partials + kMaxPartials, s_pres);
  s_src = block_sum(s_src, sh); store_partial(partials + 2 * kMaxPartials, s_src);
  s_out = block_sum(s_out, sh); store_partial(partials + 3 * kMaxPartials, s_out);
  s_free = block_sum(s_free, sh); store_partial(partials + 4 * kMaxPartials, s_free);
  s_sq = block_sum(s_sq, sh); store_partial(partials + 5 * kMaxPartials, s_sq);
}

__global__ void __launch_bounds__(kDarcyBlock)
k_darcy_gather(int64_t n, const int32_t *__restrict__ idx, const double *__restrict__ src, double *__restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * kDarcyBlock + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

template <int DIM, int NK> void launch_cells(hipStream_t s, const DarcyArgs &a, double *q) {
  hipLaunchKernelGGL((k_darcy_cells<DIM, NK>), (unsigned)((a.n_cells + kDarcyBlock - 1) / kDarcyBlock), kDarcyBlock, 0, s, a.n_cells, a.cell_X, a.cell_dofs_p, a.p, a.kappa, a.perm_cell, a.rg, q);
}
template <int DIM, int NK> void launch_bfaces(hipStream_t s, const DarcyArgs &a, int64_t n_bfaces, const int32_t *bface_cell, const int32_t *bface_local, double *Q) {
  hipLaunchKernelGGL((k_darcy_bfaces<DIM, NK>), (unsigned)((n_bfaces + kDarcyBlock - 1) / kDarcyBlock), kDarcyBlock, 0, s, n_bfaces, bface_cell, bface_local, a.cell_X, a.cell_dofs_p, a.p,
                     a.kappa, a.perm_cell, a.rg, Q);
}
int darcy_form(const DarcyArgs &a) {
  if (a.dim != 2 && a.dim != 3) throw Error("darcy: dimension must be 2 or 3");
  if (a.ncomp != 0 && a.ncomp != 1 && a.ncomp != a.dim) throw Error("darcy: the permeability has neither 0, 1 nor dim components");
  if (a.ncomp && !a.perm_cell) throw Error("darcy: the per-cell permeability is missing on the device");
  return a.ncomp == 0 ? 0 : a.ncomp == 1 ? 1 : 2;
}
}  // namespace

void darcy_cells(hipStream_t s, const DarcyArgs &a, double *q) {
  const int form = darcy_form(a);
  if (!a.n_cells) return;
  if (a.dim == 2) { if (form == 0) launch_cells<2, 0>(s, a, q); else if (form == 1) launch_cells<2, 1>(s, a, q); else launch_cells<2, 2>(s, a, q); }
  else { if (form == 0) launch_cells<3, 0>(s, a, q); else if (form == 1) launch_cells<3, 1>(s, a, q); else launch_cells<3, 3>(s, a, q); }
}
void darcy_bfaces(hipStream_t s, const DarcyArgs &a, int64_t n_bfaces, const int32_t *bface_cell, const int32_t *bface_local, double *Q) {
  const int form = darcy_form(a);
  if (!n_bfaces) return;
  if (a.dim == 2) { if (form == 0) launch_bfaces<2, 0>(s, a, n_bfaces, bface_cell, bface_local, Q); else if (form == 1) launch_bfaces<2, 1>(s, a, n_bfaces, bface_cell, bface_local, Q); else launch_bfaces<2, 2>(s, a, n_bfaces, bface_cell, bface_local, Q); }
  else { if (form == 0) launch_bfaces<3, 0>(s, a, n_bfaces, bface_cell, bface_local, Q); else if (form == 1) launch_bfaces<3, 1>(s, a, n_bfaces, bface_cell, bface_local, Q); else launch_bfaces<3, 3>(s, a, n_bfaces, bface_cell, bface_local, Q); }
}
void darcy_label_sums(hipStream_t s, int64_t n_bfaces, const int32_t *bface_id, const double *Q, const int32_t *labels, int32_t n_labels, double *out) {
  if (n_labels > 0) hipLaunchKernelGGL(k_darcy_label_sums, (unsigned)n_labels, kDarcyBlock, 0, s, n_bfaces, bface_id, Q, labels, out);
}
void flow_balance_partials(hipStream_t s, const FlowBalanceArgs &A, double *partials) {
  hipLaunchKernelGGL(k_flow_balance, reduce_grid(A.n), kBlock, 0, s, A, partials);
}
void darcy_gather(hipStream_t s, int64_t n, const int32_t *idx, const double *src, double *dst) {
  if (n) hipLaunchKernelGGL(k_darcy_gather, (unsigned)((n + kDarcyBlock - 1) / kDarcyBlock), kDarcyBlock, 0, s, n, idx, src, dst);
}

}  // namespace poro

// Mechanical post-processing on the device (definitions: include/poroel_hip.h, "Cell stresses, failure measures and support reactions"):
//   k_stress_cells<DIM, KU, NM>  one lane per cell: eps_c = sym grad u_h(x_c), sigma'_c = lambda_c tr(eps_c) I + 2 G_c eps_c, sigma_c = sigma'_c - alpha p_h(x_c) I at
//                                the image of the reference centre (the point of k_darcy_cells); NM = 0 the material's scalars, 1 the cell's own (lambda, G);
//   k_stress_measures<DIM>       one lane per cell, grid-stride: principal values, mean, von Mises and the Mohr-Coulomb function of the 3 x 3 effective stress
//                                (stress_measures.hpp), and the block partials of the summary (max f with the lowest cell that attains it, number of cells with f >= 0);
//   k_stress_summary_finish      one block: the partials in block order - a tie keeps the lower cell;
//   k_force_balance<DIM>         one pass over the displacement dofs: the 5 dim + 1 sums of the force balance as per-block partials (device_reduce.hpp);
//   k_force_deficit<DIM>         one block over the constraint rows: the part of the hanging rows' residual whose (prescribed) masters the closed list dropped;
//   k_force_residual, k_dof_components: r = A_full u - b, and the component of every dof from cell_dofs_u.
// The tensor structure at the centre: the 1D FE_Q(k) values and derivatives at 1/2 are constants.  Q1: values (1/2, 1/2), derivatives (-1, 1) - every vertex enters with
// the weight +- 2^-(dim-1).  Q2: values (0, 1, 0), derivatives (-1, 0, 1) - d u / d xi_b is the difference of the two nodes at the centres of the faces xi_b = 1 and
// xi_b = 0, so a cell reads 2 dim nodes (18 doubles in 3D), not its (k+1)^dim.  Every array a lane holds is indexed by compile-time constants; plain vector stores, no
// atomics, no LDS beyond the reductions' few words, no scratch.
#include "common.hpp"
#include "device_reduce.hpp"
#include "stress_measures.hpp"

namespace poro {
namespace {
constexpr int kStressBlock = 256;

// at the reference centre of the cell: cof = det(J) J^-T and det(J) (MappingQ1: J[r][b] = d x_r / d xi_b = 2^-(dim-1) sum_v +-X[v][r])
template <int DIM> __device__ inline double centre_cofactors(const double *__restrict__ x /* [2^DIM][DIM] of the cell */, double (&cof)[DIM][DIM]) {
  constexpr int NV = 1 << DIM;
  constexpr double w = 1.0 / (double)(1 << (DIM - 1));
  double J[DIM][DIM];
#pragma unroll
  for (int r = 0; r < DIM; ++r)
#pragma unroll
    for (int b = 0; b < DIM; ++b) J[r][b] = 0;
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int r = 0; r < DIM; ++r) {
      const double xv = x[v * DIM + r];
#pragma unroll
      for (int b = 0; b < DIM; ++b) J[r][b] += ((v >> b) & 1) ? xv : -xv;
    }
#pragma unroll
  for (int r = 0; r < DIM; ++r)
#pragma unroll
    for (int b = 0; b < DIM; ++b) J[r][b] *= w;
  if constexpr (DIM == 2) {
    cof[0][0] = J[1][1]; cof[0][1] = -J[1][0]; cof[1][0] = -J[0][1]; cof[1][1] = J[0][0];
    return J[0][0] * J[1][1] - J[0][1] * J[1][0];
  } else {
    cof[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1]; cof[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2]; cof[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    cof[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2]; cof[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0]; cof[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    cof[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1]; cof[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2]; cof[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    return J[0][0] * cof[0][0] + J[0][1] * cof[0][1] + J[0][2] * cof[0][2];
  }
}

// gh[c][b] = d u_c / d xi_b at the reference centre from the cell's own dofs (local index s * DIM + c, s lexicographic, x fastest)
template <int DIM, int KU> __device__ inline void centre_ref_gradient(const int32_t *__restrict__ dofs, const double *__restrict__ u, double (&gh)[DIM][DIM]) {
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int b = 0; b < DIM; ++b) gh[c][b] = 0;
  if constexpr (KU == 1) {
    constexpr int NV = 1 << DIM;
    constexpr double w = 1.0 / (double)(1 << (DIM - 1));
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const double uv = u[dofs[v * DIM + c]];
#pragma unroll
        for (int b = 0; b < DIM; ++b) gh[c][b] += ((v >> b) & 1) ? uv : -uv;
      }
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
      for (int b = 0; b < DIM; ++b) gh[c][b] *= w;
  } else {
    static_assert(KU == 2, "FE_Q(1) or FE_Q(2)");
    constexpr int centre = DIM == 2 ? 4 : 13;                     // (1, 1[, 1]) of the 3^DIM lattice
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      const int stride = b == 0 ? 1 : b == 1 ? 3 : 9;
      const int hi = centre + stride, lo = centre - stride;         // the centres of the faces xi_b = 1 and xi_b = 0
#pragma unroll
      for (int c = 0; c < DIM; ++c) gh[c][b] = u[dofs[hi * DIM + c]] - u[dofs[lo * DIM + c]];
    }
  }
}

template <int DIM, int KU, int NM> __global__ void __launch_bounds__(kStressBlock)
k_stress_cells(StressArgs a, double *__restrict__ strain, double *__restrict__ eff, double *__restrict__ tot) {
  constexpr int NV = 1 << DIM, NS = DIM * (DIM + 1) / 2, DPC = DIM * (KU == 1 ? (1 << DIM) : (DIM == 2 ? 9 : 27));
  const int64_t cell = (int64_t)blockIdx.x * kStressBlock + threadIdx.x;
  if (cell >= a.n_cells) return;
  double cof[DIM][DIM], gh[DIM][DIM], g[DIM][DIM];
  const double inv = 1.0 / centre_cofactors<DIM>(a.cell_X + cell * NV * DIM, cof);
  centre_ref_gradient<DIM, KU>(a.cell_dofs_u + cell * DPC, a.u, gh);
  // g[c][d] = d u_c / d x_d = sum_b gh[c][b] (J^-1)[b][d], (J^-1)[b][d] = cof[d][b] / det
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      double s = 0;
#pragma unroll
      for (int b = 0; b < DIM; ++b) s = fma(gh[c][b], cof[d][b], s);
      g[c][d] = s * inv;
    }
  double lam, G;
  if constexpr (NM == 0) { lam = a.lam; G = a.G; } else { lam = a.cell_mod[2 * cell]; G = a.cell_mod[2 * cell + 1]; }
  double tr = 0;
#pragma unroll
  for (int c = 0; c < DIM; ++c) tr += g[c][c];
  double ap = 0;                                                  // alpha p_h(x_c): the mean of the cell's vertex values
  if (a.p) {
    double s = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v) s += a.p[a.cell_dofs_p[cell * NV + v]];
    ap = a.alpha * (s * (1.0 / (double)NV));
  }
  double e[NS], se[NS], st[NS];
  int k = 0;
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int d = c; d < DIM; ++d) {
      e[k] = c == d ? g[c][c] : 0.5 * (g[c][d] + g[d][c]);
      se[k] = c == d ? fma(lam, tr, 2.0 * G * e[k]) : 2.0 * G * e[k];
      st[k] = c == d ? se[k] - ap : se[k];
      ++k;
    }
#pragma unroll
  for (int i = 0; i < NS; ++i) { strain[cell * NS + i] = e[i]; eff[cell * NS + i] = se[i]; tot[cell * NS + i] = st[i]; }
}

// (f, cell) pairs: the larger f wins, a tie goes to the lower cell
__device__ inline void take_better(double &f, double &idx, double f2, double idx2) {
  if (f2 > f || (f2 == f && idx2 < idx)) { f = f2; idx = idx2; }
}
__device__ inline void block_argmax(double &f, double &idx, double *sh /*[8]*/) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const double f2 = __shfl_xor(f, off, 64), i2 = __shfl_xor(idx, off, 64); take_better(f, idx, f2, i2); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[w] = f; sh[4 + w] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) { f = sh[0]; idx = sh[4]; take_better(f, idx, sh[1], sh[5]); take_better(f, idx, sh[2], sh[6]); take_better(f, idx, sh[3], sh[7]); }
  __syncthreads();
}

// measures[n_cells][6]; with_mc: block b leaves partials[b] = max f, partials[kMaxPartials + b] = its lowest cell (an integer below 2^53, exact in a double),
// partials[2 kMaxPartials + b] = the number of cells with f >= 0
template <int DIM> __global__ void __launch_bounds__(kBlock)
k_stress_measures(int64_t n_cells, const double *__restrict__ strain, const double *__restrict__ eff, double lam0, const double *__restrict__ cell_mod, int with_mc, double sin_phi,
                  double c_cos_phi, double *__restrict__ measures, double *__restrict__ partials) {
  constexpr int NS = DIM * (DIM + 1) / 2;
  __shared__ double sh[8];
  double best = -INFINITY, best_cell = 9.1e15, count = 0;         // (above every cell index: an empty lane never wins a tie)
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * kBlock) {
    double s[6], m[kStressMeasures];
    if constexpr (DIM == 3) {
#pragma unroll
      for (int i = 0; i < 6; ++i) s[i] = eff[c * NS + i];
    } else {
      // plane strain: the in-plane block and sigma'_zz = lambda_c tr(eps_c)
      const double lam = cell_mod ? cell_mod[2 * c] : lam0;
      s[0] = eff[c * NS]; s[1] = eff[c * NS + 1]; s[2] = 0; s[3] = eff[c * NS + 2]; s[4] = 0; s[5] = lam * (strain[c * NS] + strain[c * NS + 2]);
    }
    stress_measures(s, with_mc != 0, sin_phi, c_cos_phi, m);
#pragma unroll
    for (int i = 0; i < kStressMeasures; ++i) measures[c * kStressMeasures + i] = m[i];
    if (with_mc) { take_better(best, best_cell, m[5], (double)c); count += m[5] >= 0.0 ? 1.0 : 0.0; }
  }
  if (!with_mc) return;                                            // (uniform over the grid)
  block_argmax(best, best_cell, sh);
  count = block_sum(count, sh);
  if (threadIdx.x == 0) { partials[blockIdx.x] = best; partials[kMaxPartials + blockIdx.x] = best_cell; partials[2 * kMaxPartials + blockIdx.x] = count; }
}

// out[0] = max f, out[1] = the lowest cell that attains it, out[2] = the number of failing cells, from the nb block partials in block order
__global__ void __launch_bounds__(kBlock)
k_stress_summary_finish(int nb, const double *__restrict__ partials, double *__restrict__ out) {
  __shared__ double sh[8];
  double best = -INFINITY, best_cell = 9.1e15, count = 0;
  for (int b = threadIdx.x; b < nb; b += kBlock) { take_better(best, best_cell, partials[b], partials[kMaxPartials + b]); count += partials[2 * kMaxPartials + b]; }
  block_argmax(best, best_cell, sh);
  count = block_sum(count, sh);
  if (threadIdx.x == 0) { out[0] = best; out[1] = best_cell; out[2] = count; }
}

// comp[dof] = the component of the dof, from every cell's list (local index s * dim + comp; a dof several cells share gets the same byte from each)
__global__ void __launch_bounds__(kStressBlock)
k_dof_components(int64_t n_entries, int dim, const int32_t *__restrict__ cell_dofs_u, uint8_t *__restrict__ comp) {
  const int64_t i = (int64_t)blockIdx.x * kStressBlock + threadIdx.x;
  if (i < n_entries) comp[cell_dofs_u[i]] = (uint8_t)(i % dim);   // (dpc_u is a multiple of dim: the position in the whole list has the remainder of the local index)
}

// r = A_full u - (b_cpl + b_neu + b_body); body may be null
__global__ void __launch_bounds__(kBlock)
k_force_residual(int64_t n, const double *__restrict__ Au, const double *__restrict__ cpl, const double *__restrict__ neu, const double *__restrict__ body, double *__restrict__ r) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    double b = cpl[i] + neu[i];
    if (body) b += body[i];
    r[i] = Au[i] - b;
  }
}

// slabs of `partials`, kMaxPartials block partials each: 5 k + 0 reaction (Rt on the Dirichlet rows of component k), 5 k + 1 free rows, 5 k + 2 traction, 5 k + 3 body,
// 5 k + 4 coupling; 5 DIM: Rt^2 over the non-Dirichlet rows.  A dof of another component adds an exact 0.0, in the same order
template <int DIM> __global__ void __launch_bounds__(kBlock)
k_force_balance(ForceBalanceArgs A, double *__restrict__ partials) {
  __shared__ double sh[4];
  double acc[DIM][5], sq = 0;
#pragma unroll
  for (int k = 0; k < DIM; ++k)
#pragma unroll
    for (int t = 0; t < 5; ++t) acc[k][t] = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * kBlock) {
    const int comp = A.comp[i];
    const bool fixed = A.dir_mask && A.dir_mask[i];
    const double r = A.Rt[i], neu = A.neu[i], body = A.body ? A.body[i] : 0.0, cpl = A.cpl[i];
    if (!fixed) sq = fma(r, r, sq);
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const bool mine = comp == k;
      acc[k][0] += mine && fixed ? r : 0.0;
      acc[k][1] += mine && !fixed ? r : 0.0;
      acc[k][2] += mine ? neu : 0.0;
      acc[k][3] += mine ? body : 0.0;
      acc[k][4] += mine ? cpl : 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < DIM; ++k)
#pragma unroll
    for (int t = 0; t < 5; ++t) { const double v = block_sum(acc[k][t], sh); store_partial(partials + (5 * k + t) * kMaxPartials, v); }
  sq = block_sum(sq, sh); store_partial(partials + 5 * DIM * kMaxPartials, sq);
}

// out[k] = sum over the constrained rows h of component k of (1 - sum_m w_hm) r_h, one block in fixed order: the share of a hanging row that went to prescribed masters,
// which the closed list no longer names (a hanging node on a supported face).  Weights that sum to one (every other row, every tie) add an exact 0.0
template <int DIM> __global__ void __launch_bounds__(kBlock)
k_force_deficit(int64_t n_cons, const int32_t *__restrict__ dof, const int64_t *__restrict__ ptr, const double *__restrict__ weight, const double *__restrict__ r,
                const uint8_t *__restrict__ comp, double *__restrict__ out) {
  __shared__ double sh[4];
  double acc[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) acc[k] = 0;
  for (int64_t i = threadIdx.x; i < n_cons; i += kBlock) {
    double w = 0;
    for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) w += weight[k];
    const int32_t h = dof[i];
    const double v = (1.0 - w) * r[h];
    const int ch = comp[h];
#pragma unroll
    for (int k = 0; k < DIM; ++k) acc[k] += ch == k ? v : 0.0;
  }
#pragma unroll
  for (int k = 0; k < DIM; ++k) { const double v = block_sum(acc[k], sh); if (threadIdx.x == 0) out[k] = v; }
}

template <int DIM, int KU> void launch_stress_cells(hipStream_t s, const StressArgs &a, double *strain, double *eff, double *tot) {
  const unsigned grid = (unsigned)((a.n_cells + kStressBlock - 1) / kStressBlock);
  if (a.cell_mod) hipLaunchKernelGGL((k_stress_cells<DIM, KU, 1>), grid, kStressBlock, 0, s, a, strain, eff, tot);
  else hipLaunchKernelGGL((k_stress_cells<DIM, KU, 0>), grid, kStressBlock, 0, s, a, strain, eff, tot);
}
}  // namespace

void stress_cells(hipStream_t s, const StressArgs &a, double *strain, double *eff, double *tot) {
  if ((a.dim != 2 && a.dim != 3) || (a.k_u != 1 && a.k_u != 2)) throw Error("cell stress: dimension 2 or 3 and displacement degree 1 or 2");
  if (!a.cell_X || !a.cell_dofs_u || !a.u || (a.p && !a.cell_dofs_p)) throw Error("cell stress: a mesh array is missing on the device");
  if (!a.n_cells) return;
  if (a.dim == 2) { if (a.k_u == 1) launch_stress_cells<2, 1>(s, a, strain, eff, tot); else launch_stress_cells<2, 2>(s, a, strain, eff, tot); }
  else { if (a.k_u == 1) launch_stress_cells<3, 1>(s, a, strain, eff, tot); else launch_stress_cells<3, 2>(s, a, strain, eff, tot); }
}

void stress_measures_cells(hipStream_t s, int dim, int64_t n_cells, const double *strain, const double *eff, double lam0, const double *cell_mod, bool with_mc, double sin_phi,
                           double c_cos_phi, double *measures, double *partials, double *summary) {
  if (!n_cells) return;
  const int nb = reduce_grid(n_cells);
  if (dim == 2) hipLaunchKernelGGL(k_stress_measures<2>, nb, kBlock, 0, s, n_cells, strain, eff, lam0, cell_mod, with_mc ? 1 : 0, sin_phi, c_cos_phi, measures, partials);
  else hipLaunchKernelGGL(k_stress_measures<3>, nb, kBlock, 0, s, n_cells, strain, eff, lam0, cell_mod, with_mc ? 1 : 0, sin_phi, c_cos_phi, measures, partials);
  if (with_mc) hipLaunchKernelGGL(k_stress_summary_finish, 1, kBlock, 0, s, nb, partials, summary);
}

void dof_components(hipStream_t s, int64_t n_entries, int dim, const int32_t *cell_dofs_u, uint8_t *comp) {
  if (n_entries) hipLaunchKernelGGL(k_dof_components, (unsigned)((n_entries + kStressBlock - 1) / kStressBlock), kStressBlock, 0, s, n_entries, dim, cell_dofs_u, comp);
}
void force_residual(hipStream_t s, int64_t n, const double *Au, const double *cpl, const double *neu, const double *body, double *r) {
  if (n) hipLaunchKernelGGL(k_force_residual, grid_for(n), kBlock, 0, s, n, Au, cpl, neu, body, r);
}
void force_deficit(hipStream_t s, int dim, const ConsDev &C, const double *r, const uint8_t *comp, double *out) {
  if (dim == 2) hipLaunchKernelGGL(k_force_deficit<2>, 1, kBlock, 0, s, C.n, C.dof.p, C.ptr.p, C.weight.p, r, comp, out);
  else hipLaunchKernelGGL(k_force_deficit<3>, 1, kBlock, 0, s, C.n, C.dof.p, C.ptr.p, C.weight.p, r, comp, out);
}
void force_balance_partials(hipStream_t s, int dim, const ForceBalanceArgs &A, double *partials) {
  if (dim == 2) hipLaunchKernelGGL(k_force_balance<2>, reduce_grid(A.n), kBlock, 0, s, A, partials);
  else hipLaunchKernelGGL(k_force_balance<3>, reduce_grid(A.n), kBlock, 0, s, A, partials);
}

}  // namespace poro

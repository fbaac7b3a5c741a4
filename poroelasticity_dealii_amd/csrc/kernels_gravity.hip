// Gravity (gfx950): the two right-hand-side vectors a gravity vector g adds, built once at set-up (poro_ctx_set_gravity, ctx_fields.hip) and folded into the constant
// vectors the step kernels already read - no per-step kernel knows about them.
//   body force   body_u[i] = sum_c rho_c int_c g . phi_i                        (rho_c: bulk density per cell, or one scalar)
//   Darcy flux   flux_p[i] = -sum_c rho_f int_c (kappa_c g) . grad(phi_i)       (q = -kappa (grad p - rho_f g); kappa_c: the scalar, a per-cell k / mu or its diagonal tensor)
// Uniform boxes: one thread per node sums its <= 2^dim cells in a fixed order from the closed forms of gravity_weights.hpp - one launch, no colours, no index arrays.
// Every other mesh: one wave per cell with the quadrature of k_asm_u_rhs / k_asm_p, colour by colour.  Plain vector stores, no atomics: the same bits from call to call.
#include "common.hpp"
#include "gravity_weights.hpp"

namespace poro {
namespace {

constexpr int kTB = 256, kMaxNq = 27, kMaxNv = 8;
struct Vec3 { double v[3]; };

// ---- uniform boxes ----------------------------------------------------------------------------------------------------------------------
// one direction of a displacement node: the (at most two) cells that hold it and int phi over each; a slot without a cell has weight 0 and a clamped cell index
struct NodeCells { int cell[2]; double w[2]; };
template <int K> __device__ __forceinline__ NodeCells node_cells(int i, int n, double h) {
  const int e = i / K, s = i - e * K;
  NodeCells r;
  if (s != 0) { r.cell[0] = e; r.w[0] = gravity_weight_1d(K, s, h); r.cell[1] = e; r.w[1] = 0.0; }      // inside cell e (K = 2: its mid node)
  else {                                                                                                // vertex e: last node of cell e - 1, first node of cell e
    r.cell[0] = max(e - 1, 0); r.w[0] = e >= 1 ? gravity_weight_1d(K, K, h) : 0.0;
    r.cell[1] = min(e, n - 1); r.w[1] = e <= n - 1 ? gravity_weight_1d(K, 0, h) : 0.0;
  }
  return r;
}
// rho: one value per cell in lattice order (x fastest), or null: rho0 everywhere.  out[node * DIM + d] = g_d sum_c rho_c int_c phi_node
template <int DIM, int K> __global__ void __launch_bounds__(kTB)
k_box_body_u(BoxDev box, const double *__restrict__ rho, double rho0, Vec3 g, double *__restrict__ out) {
  const int nu0 = K * box.n[0] + 1, nu1 = K * box.n[1] + 1, nu2 = DIM == 3 ? K * box.n[2] + 1 : 1;
  const int64_t node = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (node >= (int64_t)nu0 * nu1 * nu2) return;
  const int i0 = (int)(node % nu0), i1 = (int)((node / nu0) % nu1), i2 = (int)(node / ((int64_t)nu0 * nu1));
  const NodeCells c0 = node_cells<K>(i0, box.n[0], box.h[0]), c1 = node_cells<K>(i1, box.n[1], box.h[1]);
  NodeCells c2; c2.cell[0] = c2.cell[1] = 0; c2.w[0] = 1.0; c2.w[1] = 0.0;
  if constexpr (DIM == 3) c2 = node_cells<K>(i2, box.n[2], box.h[2]);
  double acc = 0;
#pragma unroll
  for (int s2 = 0; s2 < (DIM == 3 ? 2 : 1); ++s2)
#pragma unroll
    for (int s1 = 0; s1 < 2; ++s1)
#pragma unroll
      for (int s0 = 0; s0 < 2; ++s0) {
        const double w = c0.w[s0] * (c1.w[s1] * c2.w[s2]);
        const double r = rho ? rho[((int64_t)c2.cell[s2] * box.n[1] + c1.cell[s1]) * box.n[0] + c0.cell[s0]] : rho0;      // (clamped index: loaded whatever the weight)
        acc = w != 0.0 ? fma(r, w, acc) : acc;
      }
#pragma unroll
  for (int d = 0; d < DIM; ++d) out[node * DIM + d] = g.v[d] * acc;
}

// kap: NK planes of per-cell weights in lattice order (poro_ctx::perm.lattice), or null (NK = 1): kap0 in every cell.  n0, n1, n2: pressure nodes per direction
template <int DIM, int NK> __global__ void __launch_bounds__(kTB)
k_box_gravity_p(int n0, int n1, int n2, double h0, double h1, double h2, const double *__restrict__ kap, double kap0, double rho_f, Vec3 g, double *__restrict__ out) {
  static_assert(NK == 1 || NK == DIM, "one weight per cell, or one per direction");
  const int64_t node = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (node >= (int64_t)n0 * n1 * n2) return;
  const int idx[3] = {(int)(node % n0), (int)((node / n0) % n1), (int)(node / ((int64_t)n0 * n1))};
  const int nc[3] = {n0 - 1, n1 - 1, DIM == 3 ? n2 - 1 : 1};
  const double h[3] = {h0, h1, h2};
  const int64_t plane = (int64_t)nc[0] * nc[1] * nc[2];
  int at[3][2]; bool in[3][2];      // [direction][0: the cell on the low side of the node, 1: on the high side]
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (d < DIM) { const int ci = idx[d] - 1 + c; in[d][c] = ci >= 0 && ci < nc[d]; at[d][c] = min(max(ci, 0), nc[d] - 1); }
      else { in[d][c] = c == 0; at[d][c] = 0; }
    }
  double acc = 0;
#pragma unroll
  for (int c2 = 0; c2 < (DIM == 3 ? 2 : 1); ++c2)
#pragma unroll
    for (int c1 = 0; c1 < 2; ++c1)
#pragma unroll
      for (int c0 = 0; c0 < 2; ++c0) {
        const bool held = in[0][c0] && in[1][c1] && in[2][c2];
        const int64_t cell = ((int64_t)at[2][c2] * nc[1] + at[1][c1]) * nc[0] + at[0][c0];
        const int v = (1 - c0) + 2 * (1 - c1) + (DIM == 3 ? 4 * (1 - c2) : 0);      // the node's local vertex number in that cell
        double s = 0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          const double k = kap ? kap[cell + (NK == 1 ? 0 : d * plane)] : kap0;
          s = fma(k * g.v[d], gravity_gradient_integral(DIM, h, v, d), s);
        }
        acc = held ? acc + s : acc;
      }
  out[node] = -rho_f * acc;
}

// ---- general meshes ---------------------------------------------------------------------------------------------------------------------
// MappingQ1: J_ab = sum_v X_v[a] dN_v / dxi_b; returns det J and writes adj = det J * J^-1 ([b][c] = det J d xi_b / d x_c): no division
template <int DIM> __device__ inline double jacobian_adjugate(const double *X /*[nv][DIM]*/, const double *dN /*[nv][DIM]*/, double *adj /*[DIM*DIM]*/) {
  constexpr int NV = 1 << DIM;
  double J[DIM][DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      double s = 0;
#pragma unroll
      for (int v = 0; v < NV; ++v) s += X[v * DIM + a] * dN[v * DIM + b];
      J[a][b] = s;
    }
  if constexpr (DIM == 2) {
    adj[0] = J[1][1]; adj[1] = -J[0][1]; adj[2] = -J[1][0]; adj[3] = J[0][0];
    return J[0][0] * J[1][1] - J[0][1] * J[1][0];
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    adj[0] = c00; adj[1] = J[0][2] * J[2][1] - J[0][1] * J[2][2]; adj[2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
    adj[3] = c01; adj[4] = J[0][0] * J[2][2] - J[0][2] * J[2][0]; adj[5] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
    adj[6] = c02; adj[7] = J[0][1] * J[2][0] - J[0][0] * J[2][1]; adj[8] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    return J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
  }
}

// out[dof(s, d)] += rho_c g_d sum_q phi_s(x_q) JxW_q over the cells of one colour (one wave per cell; the quadrature of k_asm_u_rhs)
template <int DIM> __global__ void __launch_bounds__(64)
k_asm_u_body(AsmArgs a, const int32_t *__restrict__ cells, const double *__restrict__ cell_rho, double rho0, Vec3 g, double *__restrict__ out) {
  __shared__ double sJxW[kMaxNq];
  __shared__ double sX[kMaxNv * DIM];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t cell = cells[blockIdx.x];
  const int nq = a.fe.nq_u, ns = a.ns_u, dpc = a.dpc_u, nv = a.nv;
  for (int i = tid; i < nv * DIM; i += nt) sX[i] = a.cell_X[cell * nv * DIM + i];
  __syncthreads();
  for (int q = tid; q < nq; q += nt) {
    double adj[DIM * DIM];
    sJxW[q] = jacobian_adjugate<DIM>(sX, a.fe.dq1_qu + (size_t)q * nv * DIM, adj) * a.fe.w_qu[q];
  }
  __syncthreads();
  const double rho = cell_rho ? cell_rho[cell] : rho0;
  for (int i = tid; i < dpc; i += nt) {
    const int s = i / DIM, c = i % DIM;
    double acc = 0;
    for (int q = 0; q < nq; ++q) acc += a.fe.u_qu[(size_t)q * ns + s] * sJxW[q];
    out[a.cell_dofs_u[cell * dpc + i]] += (rho * g.v[c]) * acc;
  }
}

// out[dof_i] += -rho_f sum_q (kappa_c g) . grad(phi_i)(x_q) JxW_q over the cells of one colour (one wave per cell; the quadrature of k_asm_p).  grad(phi) JxW =
// adj^T grad_ref(phi) w_q: the determinant cancels.  cell_w: [n_cells] (TENSOR: [n_cells][DIM]) or null: kap0
template <int DIM, bool TENSOR> __global__ void __launch_bounds__(64)
k_asm_p_gravity(AsmArgs a, const int32_t *__restrict__ cells, const double *__restrict__ cell_w, double kap0, double rho_f, Vec3 g, double *__restrict__ out) {
  constexpr int NV = 1 << DIM;
  __shared__ double sAdj[NV * DIM * DIM];
  __shared__ double sX[NV * DIM];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t cell = cells[blockIdx.x];
  const int nq = a.fe.nq_p;      // = NV (QGauss(2))
  for (int i = tid; i < NV * DIM; i += nt) sX[i] = a.cell_X[cell * NV * DIM + i];
  __syncthreads();
  for (int q = tid; q < nq && q < NV; q += nt) (void)jacobian_adjugate<DIM>(sX, a.fe.dq1_qp + (size_t)q * NV * DIM, sAdj + q * DIM * DIM);
  __syncthreads();
  double kg[DIM];                // kappa_c g, component by component
#pragma unroll
  for (int c = 0; c < DIM; ++c) kg[c] = (cell_w ? (TENSOR ? cell_w[cell * DIM + c] : cell_w[cell]) : kap0) * g.v[c];
  for (int i = tid; i < NV; i += nt) {
    double acc = 0;
    for (int q = 0; q < nq && q < NV; ++q) {
      const double *gr = a.fe.dq1_qp + ((size_t)q * NV + i) * DIM, *adj = sAdj + q * DIM * DIM;
      double dot = 0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        double gc = 0;
#pragma unroll
        for (int b = 0; b < DIM; ++b) gc += adj[b * DIM + c] * gr[b];
        dot += kg[c] * gc;
      }
      acc += dot * a.fe.w_qp[q];
    }
    out[a.cell_dofs_p[cell * NV + i]] += -rho_f * acc;
  }
}

Vec3 vec3(const double *g, int dim) { Vec3 v{{0, 0, 0}}; for (int d = 0; d < dim; ++d) v.v[d] = g[d]; return v; }

}  // namespace

void box_body_u(hipStream_t s, int dim, int k_u, const BoxDev &box, const double *rho_lattice, double rho0, const double *g, double *out) {
  if (k_u != 1 && k_u != 2) throw Error("box_body_u: degree 1 or 2");
  const int64_t nodes = (int64_t)(k_u * box.n[0] + 1) * (k_u * box.n[1] + 1) * (dim == 3 ? k_u * box.n[2] + 1 : 1);
  const unsigned grid = (unsigned)((nodes + kTB - 1) / kTB); const Vec3 gv = vec3(g, dim);
  if (dim == 2) { if (k_u == 1) hipLaunchKernelGGL((k_box_body_u<2, 1>), grid, kTB, 0, s, box, rho_lattice, rho0, gv, out); else hipLaunchKernelGGL((k_box_body_u<2, 2>), grid, kTB, 0, s, box, rho_lattice, rho0, gv, out); }
  else if (k_u == 1) hipLaunchKernelGGL((k_box_body_u<3, 1>), grid, kTB, 0, s, box, rho_lattice, rho0, gv, out);
  else hipLaunchKernelGGL((k_box_body_u<3, 2>), grid, kTB, 0, s, box, rho_lattice, rho0, gv, out);
}
void box_gravity_p(hipStream_t s, int dim, const BoxDev &box, const double *kap_lattice, int ncomp, double kap0, double rho_f, const double *g, double *out) {
  if (ncomp != 1 && ncomp != dim) throw Error("box_gravity_p: " + std::to_string(ncomp) + " components per cell in " + std::to_string(dim) + "D");
  const int n0 = box.n[0] + 1, n1 = box.n[1] + 1, n2 = dim == 3 ? box.n[2] + 1 : 1;
  const unsigned grid = (unsigned)(((int64_t)n0 * n1 * n2 + kTB - 1) / kTB); const Vec3 gv = vec3(g, dim);
  const double h2 = dim == 3 ? box.h[2] : 1.0;
  if (dim == 2) { if (ncomp == 1) hipLaunchKernelGGL((k_box_gravity_p<2, 1>), grid, kTB, 0, s, n0, n1, n2, box.h[0], box.h[1], h2, kap_lattice, kap0, rho_f, gv, out); else hipLaunchKernelGGL((k_box_gravity_p<2, 2>), grid, kTB, 0, s, n0, n1, n2, box.h[0], box.h[1], h2, kap_lattice, kap0, rho_f, gv, out); }
  else if (ncomp == 1) hipLaunchKernelGGL((k_box_gravity_p<3, 1>), grid, kTB, 0, s, n0, n1, n2, box.h[0], box.h[1], h2, kap_lattice, kap0, rho_f, gv, out);
  else hipLaunchKernelGGL((k_box_gravity_p<3, 3>), grid, kTB, 0, s, n0, n1, n2, box.h[0], box.h[1], h2, kap_lattice, kap0, rho_f, gv, out);
}
void asm_u_body(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n, const double *cell_rho, double rho0, const double *g, double *out) {
  if (!n) return;
  if (a.fe.nq_u > kMaxNq || a.nv > kMaxNv) throw Error("asm_u_body: quadrature or cell larger than the kernel's tables");
  const Vec3 gv = vec3(g, a.dim);
  if (a.dim == 2) hipLaunchKernelGGL(k_asm_u_body<2>, (unsigned)n, 64, 0, s, a, cells, cell_rho, rho0, gv, out);
  else hipLaunchKernelGGL(k_asm_u_body<3>, (unsigned)n, 64, 0, s, a, cells, cell_rho, rho0, gv, out);
}
void asm_p_gravity(hipStream_t s, const AsmArgs &a, const int32_t *cells, int64_t n, const double *cell_w, int ncomp, double kap0, double rho_f, const double *g, double *out) {
  if (!n) return;
  const Vec3 gv = vec3(g, a.dim);
  if (cell_w && ncomp != 1) { if (a.dim == 2) hipLaunchKernelGGL((k_asm_p_gravity<2, true>), (unsigned)n, 64, 0, s, a, cells, cell_w, kap0, rho_f, gv, out); else hipLaunchKernelGGL((k_asm_p_gravity<3, true>), (unsigned)n, 64, 0, s, a, cells, cell_w, kap0, rho_f, gv, out); }
  else if (a.dim == 2) hipLaunchKernelGGL((k_asm_p_gravity<2, false>), (unsigned)n, 64, 0, s, a, cells, cell_w, kap0, rho_f, gv, out);
  else hipLaunchKernelGGL((k_asm_p_gravity<3, false>), (unsigned)n, 64, 0, s, a, cells, cell_w, kap0, rho_f, gv, out);
}

}  // namespace poro

// Device side of the hybrid operator form on refined boxes (poro_ctx_set_operator_form, PORO_OPFORM_HYBRID; gfx950, wave64):
//
//   A x = S (A_box x_box - sum_{refined box cells c} K_c x_box) + sum_{fine cells f} K_f x,   x_box = S^T x,
//
// S = the injection box node -> mesh node (every box node is a mesh node and never a hanging one).  The fine cells go through the general cell kernels
// (kernels_mfg.hip) and the box product through the structured kernel (kernels_kron.hip); this file holds what lies between them:
//   hyb_gather    x_box[b] = x[inj[b]], node-wise
//   hyb_combine   y[inj[b]] += y_box[b] - sum_{refined cells c containing b} (Ke x_box|_c)_{row of b in c}
// Both are owner-computes (one lane owns a box node, the injection is one-to-one; one thread owns an entry of the slab below), so there are no atomics and two
// applications agree bit for bit.
//
// hyb_combine is three launches.
//   k_hyb_add     box nodes that touch no refined cell take the plain add y[inj[b]] += y_box[b] (streaming).
//   k_hyb_cells   v_r = Ke x_box|_c for every refined box cell c (Dirichlet columns zeroed), into a slab V[r][dofs per cell] of the plan.  A thread owns one row of Ke
//                 for 8 cells at once: it walks the row through the TRANSPOSED copy of Ke (coalesced over the rows; Ke is read once per 8 cells, from L2) while the 8
//                 x vectors sit in LDS and are read as broadcasts (15.5 KB per workgroup for 3D Q2; small elements put several 8-cell groups into a workgroup).
//   k_hyb_nodes   the box nodes of the refined cells, from a list built at enable, sorted by their position class in the cell (vertex / mid node per direction for
//                 Q2; Q1 has one class) and padded to whole waves per class, so that the adjacent cells and the node's row inside each are the same loop for a whole
//                 wave: y[inj[b]] += y_box[b] - (the slab entries of b's rows in the refined cells around it, summed in a fixed order).
// A first form without the slab - every listed node gathering its rows of Ke x_c itself, Ke rows through the scalar data path as in k_mf_apply - took 100 us
// at 512 and at 4096 refined cells alike (a few hundred waves, each a serial chain of ~2000 loads); the slab form has one thread per (cell, row).
#include "common.hpp"

namespace poro {
namespace {

template <int DIM> __global__ void __launch_bounds__(256)
k_hyb_gather(int64_t n_nodes, const int64_t *__restrict__ inj, const double *__restrict__ x, double *__restrict__ x_box) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_nodes) return;
  const int64_t m = inj[b];
#pragma unroll
  for (int a = 0; a < DIM; ++a) x_box[b * DIM + a] = x[m * DIM + a];
}

template <int DIM> __global__ void __launch_bounds__(256)
k_hyb_add(int64_t n_nodes, const int64_t *__restrict__ inj, const uint8_t *__restrict__ touched, const double *__restrict__ y_box, double *__restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_nodes || touched[b]) return;
  const int64_t m = inj[b];
#pragma unroll
  for (int a = 0; a < DIM; ++a) y[m * DIM + a] += y_box[b * DIM + a];
}

struct HybGeom { int nn[3]; int nc[3]; };

// V[r][i] = sum_j Ke[i][j] x_box[dof j of refined cell r], KeT[j][i] = Ke[i][j].  Thread = (group of 8 cells, row i); GROUPS groups per workgroup
template <int DIM, int K> __global__ void __launch_bounds__(256)
k_hyb_cells(HybGeom g, int64_t n_removed, const int32_t *__restrict__ removed_cells, const double *__restrict__ KeT, const uint8_t *__restrict__ nodemask, int constrained,
            const double *__restrict__ x_box, double *__restrict__ V) {
  constexpr int N1 = K + 1, NS = DIM == 2 ? N1 * N1 : N1 * N1 * N1, DPC = NS * DIM, GROUPS = 256 / DPC, CPG = 8, CPW = GROUPS * CPG;
  __shared__ double xs[GROUPS * DPC * CPG];                          // [group][j][cell of the group]
  const int64_t r0 = (int64_t)blockIdx.x * CPW;
  for (int idx = threadIdx.x; idx < CPW * NS; idx += 256) {
    const int q = idx / NS, j = idx % NS;                            // cell of the workgroup, local node
    const int64_t r = r0 + q;
    double v[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = 0.0;
    if (r < n_removed) {
      const int64_t c = removed_cells[r];
      const int c0 = (int)(c % g.nc[0]), c1 = (int)((c / g.nc[0]) % g.nc[1]), c2 = DIM == 3 ? (int)(c / ((int64_t)g.nc[0] * g.nc[1])) : 0;
      const int j0 = j % N1, j1 = (j / N1) % N1, j2 = DIM == 3 ? j / (N1 * N1) : 0;
      const int64_t nd = ((int64_t)(c2 * K + j2) * g.nn[1] + (c1 * K + j1)) * g.nn[0] + (c0 * K + j0);
      const unsigned m = constrained ? nodemask[nd] : 0u;
#pragma unroll
      for (int a = 0; a < DIM; ++a) v[a] = (m >> a) & 1u ? 0.0 : x_box[nd * DIM + a];
    }
    const int grp = q / CPG, qq = q % CPG;
#pragma unroll
    for (int a = 0; a < DIM; ++a) xs[(grp * DPC + j * DIM + a) * CPG + qq] = v[a];
  }
  __syncthreads();
  const int grp = threadIdx.x / DPC, i = threadIdx.x % DPC;
  if (grp >= GROUPS) return;
  double acc[CPG];
#pragma unroll
  for (int q = 0; q < CPG; ++q) acc[q] = 0.0;
  const double *xg = xs + grp * DPC * CPG;
  for (int j = 0; j < DPC; ++j) {
    const double k = KeT[j * DPC + i];
#pragma unroll
    for (int q = 0; q < CPG; ++q) acc[q] = fma(k, xg[j * CPG + q], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < CPG; ++q) {
    const int64_t r = r0 + grp * CPG + q;
    if (r < n_removed) V[r * DPC + i] = acc[q];
  }
}

// one wave per chunk of 64 listed nodes; chunk_cls[chunk] = position class (bit d set: the nodes are mid nodes in direction d); slot[box cell] = its row of V or -1
template <int DIM, int K> __global__ void __launch_bounds__(256)
k_hyb_nodes(HybGeom g, int64_t n_chunks, const int32_t *__restrict__ chunk_cls, const int64_t *__restrict__ nodes, const int32_t *__restrict__ slot,
            const int64_t *__restrict__ inj, const double *__restrict__ V, const double *__restrict__ y_box, double *__restrict__ y) {
  constexpr int N1 = K + 1, NS = DIM == 2 ? N1 * N1 : N1 * N1 * N1, DPC = NS * DIM;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (chunk >= n_chunks) return;
  const int cls = __builtin_amdgcn_readfirstlane(chunk_cls[chunk]);
  const int64_t b = nodes[chunk * 64 + (threadIdx.x & 63)];          // -1: padding of the class to whole waves
  if (b < 0) return;
  const int node[3] = {(int)(b % g.nn[0]), (int)((b / g.nn[0]) % g.nn[1]), DIM == 3 ? (int)(b / ((int64_t)g.nn[0] * g.nn[1])) : 0};
  int vertex[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) vertex[d] = K == 2 ? !((cls >> d) & 1) : 1;
  double acc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) acc[a] = 0.0;
  const int nopt0 = vertex[0] ? 2 : 1, nopt1 = vertex[1] ? 2 : 1, nopt2 = DIM == 3 ? (vertex[2] ? 2 : 1) : 1;
  for (int o2 = 0; o2 < nopt2; ++o2)
    for (int o1 = 0; o1 < nopt1; ++o1)
      for (int o0 = 0; o0 < nopt0; ++o0) {
        const int o[3] = {o0, o1, o2};
        int cell[3] = {0, 0, 0}, loc[3] = {0, 0, 0}; bool exists = true;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          if (vertex[d]) { cell[d] = node[d] / K - 1 + o[d]; loc[d] = o[d] ? 0 : K; }
          else { cell[d] = (node[d] - 1) / 2; loc[d] = 1; }
          exists = exists && cell[d] >= 0 && cell[d] < g.nc[d];
        }
        if (!exists) continue;
        const int32_t r = slot[((int64_t)cell[2] * g.nc[1] + cell[1]) * g.nc[0] + cell[0]];
        if (r < 0) continue;
        const int li = loc[0] + N1 * (loc[1] + (DIM == 3 ? N1 * loc[2] : 0));   // wave-uniform local scalar node
#pragma unroll
        for (int a = 0; a < DIM; ++a) acc[a] += V[(int64_t)r * DPC + li * DIM + a];
      }
  const int64_t mnode = inj[b];
#pragma unroll
  for (int a = 0; a < DIM; ++a) y[mnode * DIM + a] += y_box[b * DIM + a] - acc[a];
}

template <int DIM, int K> void launch_removed(hipStream_t s, const HybGeom &g, const HybCombine &h, const double *Ke_t, const uint8_t *nodemask, bool constrained, double *y) {
  constexpr int N1 = K + 1, DPC = (DIM == 2 ? N1 * N1 : N1 * N1 * N1) * DIM, CPW = (256 / DPC) * 8;
  hipLaunchKernelGGL((k_hyb_cells<DIM, K>), (unsigned)((h.n_removed + CPW - 1) / CPW), 256, 0, s, g, h.n_removed, h.removed_cells, Ke_t, nodemask, constrained ? 1 : 0, h.x_box, h.V);
  hipLaunchKernelGGL((k_hyb_nodes<DIM, K>), (unsigned)((h.n_chunks + 3) / 4), 256, 0, s, g, h.n_chunks, h.chunk_cls, h.nodes, h.slot, h.inj, h.V, h.y_box, y);
}

}  // namespace

void hyb_gather(hipStream_t s, int dim, int64_t n_box_nodes, const int64_t *inj, const double *x, double *x_box) {
  if (!n_box_nodes) return;
  const unsigned grid = (unsigned)((n_box_nodes + 255) / 256);
  if (dim == 2) hipLaunchKernelGGL(k_hyb_gather<2>, grid, 256, 0, s, n_box_nodes, inj, x, x_box);
  else hipLaunchKernelGGL(k_hyb_gather<3>, grid, 256, 0, s, n_box_nodes, inj, x, x_box);
}

void hyb_combine(hipStream_t s, const MfArgs &box, const double *Ke_t, bool constrained, const HybCombine &h, double *y) {
  if (!h.n_box_nodes) return;
  const unsigned grid = (unsigned)((h.n_box_nodes + 255) / 256);
  if (box.dim == 2) hipLaunchKernelGGL(k_hyb_add<2>, grid, 256, 0, s, h.n_box_nodes, h.inj, h.touched, h.y_box, y);
  else hipLaunchKernelGGL(k_hyb_add<3>, grid, 256, 0, s, h.n_box_nodes, h.inj, h.touched, h.y_box, y);
  if (!h.n_removed) return;
  HybGeom g{};
  for (int d = 0; d < 3; ++d) { g.nc[d] = d < box.dim ? box.box.n[d] : 1; g.nn[d] = d < box.dim ? box.k_u * box.box.n[d] + 1 : 1; }
  if (box.dim == 2 && box.k_u == 1) launch_removed<2, 1>(s, g, h, Ke_t, box.nodemask, constrained, y);
  else if (box.dim == 2 && box.k_u == 2) launch_removed<2, 2>(s, g, h, Ke_t, box.nodemask, constrained, y);
  else if (box.dim == 3 && box.k_u == 1) launch_removed<3, 1>(s, g, h, Ke_t, box.nodemask, constrained, y);
  else if (box.dim == 3 && box.k_u == 2) launch_removed<3, 2>(s, g, h, Ke_t, box.nodemask, constrained, y);
  else throw Error("hyb_combine: unsupported dim / degree");
}

}  // namespace poro

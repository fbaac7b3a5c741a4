// Fast-diagonalisation preconditioners on the host side: set-up and application for the Q1 systems and for the displacement blocks, incl. the slab-distributed forms (all-to-all of column groups).
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <optional>
#include <thread>
#include <unordered_map>
#include "common.hpp"
#include "ctx_internal.hpp"
#include "perm_line.hpp"
#include "moduli_line.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace poro {
namespace ctx_detail {
// ---- fast diagonalisation of the Q1 box operators (kernels_fdm.hip) -------------------------------------------------------------
bool fdm_p_supported(poro_ctx *c) {
  if (!c->lines.on) return false;
  if (!c->box.enabled && c->comm.multi()) return false;     // tensor-product grids: one rank
  if (c->comm.multi() && !(c->comm.nccl_comm || (c->comm.ar && c->comm.sr))) return false;
  return true;
}
// the second table set: the pressure Jacobian with whole prescribed faces (one rank)
bool fdm_pj_supported(poro_ctx *c) { return c->n_pdir && c->pdir_faces_ok && !c->comm.multi() && fdm_p_supported(c); }
// The 1D tables of one direction, with or without its end nodes.  Deleting the rows and columns of a face from a M + kappa K deletes the end node of that direction's 1D
// matrices; line_tables (fdm_tables.hpp) gives their eigenpairs in full-length storage (zero rows of S at removed nodes, zero columns and lam = inf behind the free
// modes), so the transform kernels run unchanged and return exactly 0 there.
static void upload_dir(FdmDir &D, const LineTables &T, FdmOct *fused = nullptr, int dir = 0) {
  const int n = T.n; const std::vector<double> &S = T.S;
  if (fused) fdmo_scalar_upload_dir(*fused, dir, T);
  std::vector<double> St((size_t)n * n), lam = T.lam;
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) St[(size_t)j * n + i] = S[(size_t)i * n + j];
  // six-launch form: its kernel divides by a + sum k_d lam_d.  A removed mode's coefficient is exactly 0 (zero row of S^T), so any finite positive eigenvalue in its
  // place gives the 0 that lam = inf gives, without inf * 0 where a coefficient k_d is 0
  for (double &l : lam) if (!(l < 1e300)) l = 1e300;
  D.n = n; D.S.upload(S); D.St.upload(St); D.lam.upload(lam);
}
// every rank learns all slab thicknesses through the existing all-reduce.  nodes_per_cell: 1 for the Q1 space, k_u for the displacement space; ncol_total: the nodes of one
// plane.  Returns the global number of cell layers
int slab_layout(poro_ctx *c, SlabLayout &L, int nodes_per_cell, int64_t ncol_total) {
  const int N = std::max(1, c->comm.part.n_ranks), r = c->comm.part.rank, last = c->dim - 1;
  L.n_ranks = N; L.rank = r;
  std::vector<double> lay(N, 0.0); lay[r] = c->box.n[last];
  DevBuf<double> tmp; tmp.upload(lay);
  for (int base = 0; base < N; base += kScalarSlots) {
    const int m = std::min(kScalarSlots, N - base);
    PORO_HIP(hipMemcpyAsync(c->red.p, tmp.p + base, m * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    allreduce_sum(c, c->red.p, m);
    PORO_HIP(hipMemcpyAsync(lay.data() + base, c->red.p, m * sizeof(double), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
  }
  L.layers.resize(N); L.off.resize(N); int acc = 0;
  for (int q = 0; q < N; ++q) { L.layers[q] = (int)std::lround(lay[q]); L.off[q] = nodes_per_cell * acc; acc += L.layers[q]; }
  L.ng = nodes_per_cell * acc + 1;
  L.ncol_total = ncol_total;
  L.C = (L.ncol_total + N - 1) / N;
  L.max_own = 0; L.max_nl = 0;
  for (int q = 0; q < N; ++q) { L.max_own = std::max(L.max_own, nodes_per_cell * L.layers[q] + (q == N - 1 ? 1 : 0)); L.max_nl = std::max(L.max_nl, nodes_per_cell * L.layers[q] + 1); }
  return acc;
}
// the slab-partitioned part of the free table set: the global line of the last direction, the exchange buffers and windows, the slab form of the fused kernels
static void build_fdm_dist(poro_ctx *c, const int np3[3]) {
  FdmDist &F = c->fdm_dist; FdmOct &fused = c->q1_free.fused; const int last = c->dim - 1;
  int64_t ncol_total = 1; for (int d = 0; d < last; ++d) ncol_total *= c->box.n[d] + 1;
  const int acc = slab_layout(c, F, 1, ncol_total), N = F.n_ranks, r = F.rank;
  // slab form of the same three-launch kernels (kernels_fdmo.hip): 3D, local planes and the global line of at most 80 vertices
  { int g3[3] = {np3[0], np3[1], acc + 1};
    const bool fused_slab = c->dim == 3 && fdmo_scalar_usable(3, np3) && fdmo_scalar_usable(3, g3) && !std::getenv("PORO_FDM_P_UNFUSED");
    if (fused_slab) {
      fdmo_scalar_init_slab(fused, np3, r, F.layers, c->stream);
      for (int d = 0; d < 2; ++d) fdmo_scalar_upload_dir(fused, d, q1_eig(c->box.n[d], c->box.h[d]));
      fdmo_scalar_upload_dir(fused, 2, q1_eig(acc, c->box.h[last]));
      fused.built = true;
    } }
  upload_dir(F.last, q1_eig(acc, c->box.h[last]));
  const size_t blk = (size_t)std::max(F.max_own, F.max_nl) * F.C;
  F.sendbuf.alloc(blk * N); F.recvbuf.alloc(blk * N); F.tz1.alloc((size_t)F.ng * F.C); F.tz2.alloc((size_t)F.ng * F.C);
  F.sendbuf.zero(c->stream); F.recvbuf.zero(c->stream); F.tz1.zero(c->stream); F.tz2.zero(c->stream);
  // the four window copies of an application, one entry per peer: local grid -> send blocks (own planes), gathered blocks -> whole lines, whole lines -> send blocks
  // (every rank's planes incl. the shared ones), scattered blocks -> local grid
  std::vector<FdmWindow> W((size_t)4 * N);
  auto ncols_of = [&](int q) { return std::max<int64_t>(0, std::min<int64_t>(F.C, F.ncol_total - (int64_t)q * F.C)); };
  const int own_r = F.layers[r] + (r == N - 1 ? 1 : 0), nl_r = c->box.n[last] + 1;
  for (int q = 0; q < N; ++q) {
    W[q] = FdmWindow{own_r, ncols_of(q), (int64_t)q * F.C, 0};
    W[N + q] = FdmWindow{F.layers[q] + (q == N - 1 ? 1 : 0), F.C, 0, F.off[q]};
    W[2 * N + q] = FdmWindow{F.layers[q] + 1, F.C, 0, F.off[q]};
    W[3 * N + q] = FdmWindow{nl_r, ncols_of(q), (int64_t)q * F.C, 0};
  }
  F.windows.upload(W);
  F.built = true;
}
// One builder for both table sets.  Q1Set::free_ends: every end free (the projection mass matrix, the pressure Jacobian without prescribed rows), on slab partitions with
// the distributed part.  Q1Set::fixed_ends: the ends of c->pdir_face removed; built lazily by the first solve that needs it, never without prescribed pressures
void build_fdm_q1(poro_ctx *c, Q1Set which) {
  const bool fixed = which == Q1Set::fixed_ends;
  FdmQ1 &T = q1_set(c, which);
  if (T.nodal.built) return;
  if (fixed) {
    if (!fdm_pj_supported(c)) throw Error("PORO_PREC_FDM with prescribed pressures needs a uniform box or tensor-product grid on one rank whose prescribed set is a union of whole faces");
    if (c->timing) c->timers["fdm_pj_build"].enqueued += 1;          // (a count, no time: contexts without prescribed pressures never get here)
  } else if (!fdm_p_supported(c)) throw Error("PORO_PREC_FDM needs a uniform box (poro_desc.box.enabled) and, when partitioned, an initialised communicator");
  T.nodal.dim = c->dim;
  const bool multi = !fixed && c->comm.multi();                      // (the fixed-ends set: one rank, see fdm_pj_supported)
  // one rank, 3D, lines of at most 80 nodes: the three-launch form through the block-FDM transform kernel (kernels_fdmo.hip) instead of six single-direction launches
  int np3[3] = {c->lines.n[0] + 1, c->lines.n[1] + 1, c->dim == 3 ? c->lines.n[2] + 1 : 1};
  const bool fused = !multi && fdmo_scalar_usable(c->dim, np3) && !std::getenv("PORO_FDM_P_UNFUSED");
  if (fused) {
    fdmo_scalar_init(T.fused, np3, c->stream);
    const char *strips = std::getenv("PORO_FDMO_SCALAR_STRIPS");     // (=0: every pass in the block-per-workgroup form; another number: that factor in place of kFdmoStripFill)
    T.fused.strip_limit = (strips ? std::max(0.0, std::atof(strips)) : kFdmoStripFill) * c->n_cus;
  }
  for (int d = 0; d < c->dim; ++d) {                                 // (partitioned: the local slab; the last direction is replaced by fdm_dist.last)
    const std::vector<double> &hcell = c->lines.hcell[d]; const bool lo = fixed && c->pdir_face[d][0], hi = fixed && c->pdir_face[d][1];
    upload_dir(T.nodal.dir[d], c->lines.uniform && !lo && !hi ? q1_eig((int)hcell.size(), hcell[0]) : line_tables(1, hcell, lo, hi), fused ? &T.fused : nullptr, d);   // (closed form on a uniform line with free ends)
  }
  if (!multi) T.fused.built = fused;
  if (c->fdm_t1.n < (size_t)c->n_p) { c->fdm_t1.alloc(c->n_p); c->fdm_t2.alloc(c->n_p); }
  if (multi) build_fdm_dist(c, np3);
  T.nodal.built = true;
}
// every rank sends block q of `send` (blk doubles) to rank q and receives block q of `recv` from it
void alltoall_blocks(poro_ctx *c, double *send, double *recv, int64_t blk, bool self_in_place) {
  Comm &cm = c->comm; const int N = cm.part.n_ranks, r = cm.part.rank;
  Timed tm(c, "alltoall");
  if (!self_in_place) PORO_HIP(hipMemcpyAsync(recv + (size_t)r * blk, send + (size_t)r * blk, blk * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (N <= 1) return;
  if (cm.nccl_comm) {
    ncclComm_t comm = (ncclComm_t)cm.nccl_comm;
    PORO_NCCL(g_rccl.GroupStart());
    for (int q = 0; q < N; ++q) if (q != r) {
      PORO_NCCL(g_rccl.Send(send + (size_t)q * blk, blk, ncclFloat64, q, comm, c->stream));
      PORO_NCCL(g_rccl.Recv(recv + (size_t)q * blk, blk, ncclFloat64, q, comm, c->stream));
    }
    PORO_NCCL(g_rccl.GroupEnd());
  } else if (cm.sr) {
    FdmDist &F = c->fdm_dist; if ((int64_t)F.hsend.size() < blk) { F.hsend.resize(blk); F.hrecv.resize(blk); }
    for (int step = 0; step < N; ++step) {                       // pairwise schedule: at step s rank r meets (s - r) mod N, which meets r
      const int q = ((step - r) % N + N) % N;
      if (q == r) continue;
      PORO_HIP(hipMemcpyAsync(F.hsend.data(), send + (size_t)q * blk, blk * sizeof(double), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
      cm.sr(F.hsend.data(), F.hrecv.data(), blk, q, cm.user);
      PORO_HIP(hipMemcpyAsync(recv + (size_t)q * blk, F.hrecv.data(), blk * sizeof(double), hipMemcpyHostToDevice, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
    }
  } else throw Error("partitioned context without a communicator");
}
// z = (a M + sum_d k_d K_d)^-1 g for the Q1 space of the (global) box, from the table set `which`
// Q1Set::fixed_ends (whole prescribed faces removed, one rank): z = J_ff^-1 g_f on the free rows, exactly 0 on the prescribed ones whatever g holds there
void count_strip_launches(poro_ctx *c, int n) { if (n) c->timers["fdm_q1_strip_launches"].enqueued += n; }      // (a count, no time: launches of the scalar passes in the strip form)
void fdm_precondition_p(poro_ctx *c, double a, const double k[3], const double *g, double *z, Q1Set which) {
  Timed tm(c, "precondition_p_fdm");
  hipStream_t s = c->stream;
  const bool fixed = which == Q1Set::fixed_ends, isotropic = k[0] == k[1] && k[1] == k[2];
  FdmQ1 &T = q1_set(c, which);
  if (fixed || !c->comm.multi()) {
    std::optional<Timed> tf; if (fixed) tf.emplace(c, "precondition_p_fdm_fixed_ends");
    if (T.fused.built && isotropic) count_strip_launches(c, fdmo_scalar_apply(s, T.fused, a, k[0], g, z));
    else fdm_apply(s, T.nodal, a, k, g, z, c->fdm_t1.p, c->fdm_t2.p);
    return;
  }
  if (T.fused.built && T.fused.slab.on && isotropic) {
    // the slab form of the fused kernels: x / y sweeps on the local planes straight into the exchange buffer, whole z lines per column share, scatter, y / x sweeps
    FdmOct &O = T.fused; auto &S = O.slab; double *send = S.buf.p, *recv = S.buf.p + S.recv_off;
    fdmo_scalar_slab_pass(s, O, 1, a, k[0], g, S.buf.p);
    alltoall_blocks(c, send, recv, (int64_t)S.max_own * S.scols, true);
    fdmo_scalar_slab_pass(s, O, 2, a, k[0], S.buf.p, S.tz.p);
    fdmo_slab_scatter_pack(s, O, nullptr);
    alltoall_blocks(c, send, recv, (int64_t)S.max_nl * S.scols, true);
    fdmo_scalar_slab_pass(s, O, 3, a, k[0], S.buf.p, z);
    return;
  }
  FdmDist &F = c->fdm_dist; const FdmScalar &L = T.nodal;
  const int dim = c->dim, N = F.n_ranks, r = F.rank, last = dim - 1;
  const int n0 = L.dir[0].n, nl = c->box.n[last] + 1;             // local planes incl. the shared ones
  const int64_t SIp = F.ncol_total;
  double *t1 = c->fdm_t1.p, *t2 = c->fdm_t2.p;
  // leading directions: local (the shared planes are transformed by both owners)
  const double *cur = g;
  if (dim == 3) { fdm_transform(s, L.dir[0].St.p, n0, 1, (int64_t)L.dir[1].n * nl, g, t1, nullptr); fdm_transform(s, L.dir[1].St.p, L.dir[1].n, n0, nl, t1, t2, nullptr); cur = t2; }
  else { fdm_transform(s, L.dir[0].St.p, n0, 1, nl, g, t1, nullptr); cur = t1; }
  // gather whole lines of the last direction for this rank's column group
  const int64_t blk1 = (int64_t)F.max_own * F.C;
  fdm_window_batch(s, const_cast<double *>(cur), F.sendbuf.p, F.recvbuf.p, r, true, F.windows.p, N, F.max_own, F.C, SIp, blk1);
  alltoall_blocks(c, F.sendbuf.p, F.recvbuf.p, blk1, true);
  fdm_window_batch(s, F.tz1.p, F.recvbuf.p, nullptr, r, false, F.windows.p + N, N, F.max_own, F.C, F.C, blk1);       // (the owned planes of all ranks cover every global plane: tz1 is overwritten in full)
  FdmScale sc{}; sc.a = a; sc.ncol = F.C; sc.col0 = (int64_t)r * F.C; sc.col_total = F.ncol_total;
  for (int d = 0; d < 3; ++d) { sc.lam[d] = d < dim ? (d == last ? F.last.lam.p : L.dir[d].lam.p) : nullptr; sc.k[d] = d < dim ? k[d] : 0.0; sc.n[d] = d < dim ? (d == last ? F.ng : L.dir[d].n) : 1; }
  fdm_transform(s, F.last.St.p, F.ng, F.C, 1, F.tz1.p, F.tz2.p, &sc);
  fdm_transform(s, F.last.S.p, F.ng, F.C, 1, F.tz2.p, F.tz1.p, nullptr);
  // scatter back: every rank gets all of its planes (shared ones included) of every column group
  const int64_t blk2 = (int64_t)F.max_nl * F.C;
  fdm_window_batch(s, F.tz1.p, F.sendbuf.p, F.recvbuf.p, r, true, F.windows.p + 2 * N, N, F.max_nl, F.C, F.C, blk2);
  alltoall_blocks(c, F.sendbuf.p, F.recvbuf.p, blk2, true);
  double *back = dim == 3 ? t2 : t1;
  fdm_window_batch(s, back, F.recvbuf.p, nullptr, r, false, F.windows.p + 3 * N, N, F.max_nl, F.C, SIp, blk2);
  if (dim == 3) { fdm_transform(s, L.dir[1].S.p, L.dir[1].n, n0, nl, t2, t1, nullptr); fdm_transform(s, L.dir[0].S.p, n0, 1, (int64_t)L.dir[1].n * nl, t1, z, nullptr); }
  else fdm_transform(s, L.dir[0].S.p, n0, 1, nl, t1, z, nullptr);
}

// A per-cell k / mu is set (c->perm): z = (a M + K_layer)^-1 g with K_layer built from c->perm.layer, the layer values (kind 1: the exact inverse of the Jacobian) or the
// layer means (kind 2: a preconditioner).  x / y transforms with the table set `which` (coefficient 1: kappa sits in the 1D matrices of the slowest direction), the line
// solve, and back.  The 1D arrays are uploaded at the first use after the field changed, the reciprocal pivots computed on the device whenever a changed
void fdm_precondition_p_layered(poro_ctx *c, double a, const double *g, double *z, Q1Set which) {
  Timed tm(c, "precondition_p_fdm_layered");
  const bool fixed = which == Q1Set::fixed_ends; const int last = c->dim - 1, nl = c->lines.n[last] + 1;
  poro_ctx::Perm &P = c->perm;
  if (!P.kind || c->comm.multi()) throw Error("fdm_precondition_p_layered: needs a per-cell permeability on a single-rank context");
  FdmQ1 &T = q1_set(c, which);
  const int nw = P.ncomp == 1 ? 1 : last;      // weighted mass lines: one k / mu weights the one line of lam_x + lam_y, a diagonal tensor one line per leading direction
  poro_ctx::Perm::Line &L = P.line[fixed ? 1 : 0];
  if (!L.built) {
    L.lo = fixed && c->pdir_face[last][0]; L.hi = fixed && c->pdir_face[last][1];
    L.coef.upload(perm_line_coefficients(c->lines.hcell[last], P.layer, nw, P.layer[P.ncomp - 1], L.lo, L.hi));
    if (L.inv.n != (size_t)c->n_p) L.inv.alloc(c->n_p);
    L.a = -1; L.built = true;
  }
  if (L.a != a) { q1_line_factor(c->stream, c->dim, nw, T.nodal, nl, a, L.coef.p, L.inv.p); L.a = a; }
  // 5 launches in 3D, 3 in 2D
  hipStream_t s = c->stream; const FdmScalar &F = T.nodal; const int n0 = F.dir[0].n, n1 = F.dir[1].n; double *t1 = c->fdm_t1.p, *t2 = c->fdm_t2.p;
  auto lines = [&](const double *in, double *out) { Timed tl(c, "q1_line_solve"); q1_line_solve(s, c->dim, nw, F, nl, a, L.lo, L.hi, L.coef.p, L.inv.p, in, out); };
  if (c->dim == 2) {
    fdm_transform(s, F.dir[0].St.p, n0, 1, nl, g, t1, nullptr);
    lines(t1, t2);
    fdm_transform(s, F.dir[0].S.p, n0, 1, nl, t2, z, nullptr);
  } else {
    fdm_transform(s, F.dir[0].St.p, n0, 1, (int64_t)n1 * nl, g, t1, nullptr);
    fdm_transform(s, F.dir[1].St.p, n1, n0, nl, t1, t2, nullptr);
    lines(t2, t1);
    fdm_transform(s, F.dir[1].S.p, n1, n0, nl, t1, t2, nullptr);
    fdm_transform(s, F.dir[0].S.p, n0, 1, (int64_t)n1 * nl, t2, z, nullptr);
  }
}

// ---- block fast diagonalisation of the displacement system (kernels_fdmu.hip) ---------------------------------------------------------
// Usable when the box is node-interleaved and, per component, the Dirichlet dofs are exactly a union of whole faces (then the 1D matrices
// of that component just lose their end nodes) with at least one face each (otherwise the block is singular).
void analyse_fdm_u(poro_ctx *c) {
  if (c->fdm_u_state != 0) return;
  c->fdm_u_state = -1;
  const bool multi = c->comm.multi();
  if (multi && !(c->comm.nccl_comm || (c->comm.ar && c->comm.sr))) { c->fdm_u_state = 0; c->fdm_u_why = "partitioned context without a communicator yet"; return; }
  const int dim = c->dim, last = dim - 1; const int64_t nn[3] = {c->lines.nn[0], c->lines.nn[1], dim == 3 ? c->lines.nn[2] : 1};
  std::string why;
  FdmU &F = c->fdm_u;
  if (!c->lines.on || !c->interleaved_u || (multi && !c->box.enabled)) why = "needs a uniform box (or, on one rank, a tensor-product grid) with node-interleaved displacement dofs";
  else {
    for (int d = 0; d < dim; ++d) if (nn[d] > 4096) why = "more than 4096 nodes per grid line";
  }
  if (why.empty()) {
    const std::vector<uint8_t> &nm = c->h_node_mask;
    // a face of the partitioned direction is a physical boundary only at the first / last rank
    int physical[3][2] = {{1, 1}, {1, 1}, {1, 1}};
    if (multi) { physical[last][0] = !c->comm.part.has_lower; physical[last][1] = !c->comm.part.has_upper; }
    for (int comp = 0; comp < dim && why.empty(); ++comp)
      if (!whole_faces(nn, dim, nm.data(), comp, physical, F.fix[comp])) why = "Dirichlet dofs are not a union of whole faces per component";
  }
  // ranks agree on the verdict and on the face flags (the end faces of the partitioned direction live on the first / last rank only)
  if (multi) {
    double h[kScalarSlots] = {0}; int m = 0;
    for (int comp = 0; comp < 3; ++comp) for (int d = 0; d < 3; ++d) for (int side = 0; side < 2; ++side) h[m++] = (comp < dim && d < dim) ? F.fix[comp][d][side] : 0;
    h[m++] = why.empty() ? 0.0 : 1.0;
    PORO_HIP(hipMemcpyAsync(c->red.p, h, m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    allreduce_sum(c, c->red.p, m);
    PORO_HIP(hipMemcpyAsync(h, c->red.p, m * sizeof(double), hipMemcpyDeviceToHost, c->stream)); PORO_HIP(hipStreamSynchronize(c->stream));
    m = 0;
    for (int comp = 0; comp < 3; ++comp) for (int d = 0; d < 3; ++d) for (int side = 0; side < 2; ++side) { if (comp < dim && d < dim) F.fix[comp][d][side] = h[m] > 0.5 ? 1 : 0; ++m; }
    if (h[m] > 0.5 && why.empty()) why = "another rank's Dirichlet dofs are not face-separable";
  }
  // lines of more than 320 points only have the even / odd (blocked) transform kernels: every component needs the same condition at both ends of such a direction.
  // Checked here, after the ranks have agreed on the face flags, so that poro_supports_preconditioner() is authoritative and no rank throws alone at solve time
  if (why.empty()) for (int d = 0; d < dim; ++d) {
    const int64_t line = (multi && d == last) ? 0 : nn[d];        // (the partitioned direction's GLOBAL line length is only known in build_fdm_u; its limit of 4096 is checked there on every rank alike)
    if (line > 320 && !(dim == 2 && !multi)) for (int comp = 0; comp < dim; ++comp) if (F.fix[comp][d][0] != F.fix[comp][d][1]) why = "a grid line of more than 320 points needs the same Dirichlet condition at both of its ends (even / odd transforms)";   // (2D on one rank: the planar form takes lines of any length with any end conditions)
  }
  if (why.empty()) for (int comp = 0; comp < dim; ++comp) {
    bool any = false;
    for (int d = 0; d < dim; ++d) any = any || F.fix[comp][d][0] || F.fix[comp][d][1];
    if (!any) why = "a displacement component without a constrained face (singular block)";
  }
  c->fdm_u_why = why;
  c->fdm_u_state = why.empty() ? 1 : -1;
}
// everything build_fdm_u made, released: the next use builds it again (poro_ctx_set_fdm_form).  The buffers are not copyable, so the two structures are constructed afresh
void release_fdm_u(poro_ctx *c) {
  if (!c->fdm_u.built) return;
  PORO_HIP(hipStreamSynchronize(c->stream));
  c->fdm_oct.~FdmOct(); new (&c->fdm_oct) FdmOct();
  c->fdm_u.~FdmU(); new (&c->fdm_u) FdmU();
  c->fdm_u_state = 0; c->fdm_u_why.clear();
}
void build_fdm_u(poro_ctx *c) {
  FdmU &F = c->fdm_u;
  if (F.built) return;
  analyse_fdm_u(c);
  if (c->fdm_u_state != 1) throw Error("PORO_PREC_FDM (displacement): " + c->fdm_u_why);
  const int dim = c->dim, last = dim - 1, ku = c->k_u;
  const bool multi = c->comm.multi();
  // per-cell moduli (one rank): the nodal tables of the leading directions alone - no octant, planar, per-direction or fp32 form, whatever the settings ask for - and the
  // banded line solve of the last direction (kernels_fdmu_line.hip) with the layer values (kind 1: the exact block inverse) or the layer means (kind 2)
  const bool line = c->mod.kind != 0;
  if (line && multi) throw Error("PORO_PREC_FDM (displacement): per-cell moduli on a partitioned context");
  F.dim = dim; F.single = !multi && !line && std::getenv("PORO_FDMU_SINGLE") != nullptr;   // fp32 transforms (experimental switch, one rank)
  for (int d = 0; d < 3; ++d) F.nn[d] = d < dim ? c->lines.nn[d] : 1;
  const double l2g = c->mat.lame_lambda + 2 * c->mat.shear_G, G = c->mat.shear_G;
  for (int comp = 0; comp < dim; ++comp) for (int d = 0; d < dim; ++d) F.coef[comp][d] = d == comp ? l2g : G;
  int n_cells_last = c->lines.n[last];
  if (multi) {
    int64_t ncol_total = 1; for (int d = 0; d < last; ++d) ncol_total *= F.nn[d];
    F.dist = true; n_cells_last = slab_layout(c, F, ku, ncol_total);
    if (F.ng > 4096) throw Error("PORO_PREC_FDM (displacement): more than 4096 nodes per global grid line");
    const int N = F.n_ranks;
    const size_t blk = (size_t)dim * std::max(F.max_own, F.max_nl) * F.C;
    F.sendbuf.alloc(blk * N); F.recvbuf.alloc(blk * N); F.tz1.alloc((size_t)dim * F.ng * F.C); F.tz2.alloc((size_t)dim * F.ng * F.C);
    F.sendbuf.zero(c->stream); F.recvbuf.zero(c->stream); F.tz1.zero(c->stream); F.tz2.zero(c->stream);
  }
  // eigenpairs per (direction, end conditions); components with the same end conditions share the host work.  same_ends[d]: every component has the same condition at
  // both ends of direction d; parity[d]: every component's eigenvectors came out even or odd there (they do on a uniform line with the same ends, not on a graded one)
  LineTables tables[3][4]; ClassSplitTables classes[3][4]; bool same_ends[3], parity[3], parity_cd[3][3] = {};
  const auto key_of = [&](int comp, int d) { return F.fix[comp][d][0] * 2 + F.fix[comp][d][1]; };
  for (int d = 0; d < dim; ++d) {
    if (line && d == last) { same_ends[d] = parity[d] = false; continue; }      // (no eigenpairs along the line direction)
    const bool global_dir = multi && d == last;
    const std::vector<double> hcell = global_dir ? std::vector<double>((size_t)n_cells_last, c->box.h[d]) : c->lines.hcell[d];
    same_ends[d] = parity[d] = true;
    for (int comp = 0; comp < dim; ++comp) {
      LineTables &T = tables[d][key_of(comp, d)];
      if (!T.n) T = line_tables(ku, hcell, F.fix[comp][d][0], F.fix[comp][d][1]);
      same_ends[d] = same_ends[d] && F.fix[comp][d][0] == F.fix[comp][d][1]; parity[d] = parity[d] && T.parity; parity_cd[comp][d] = T.parity;
    }
  }
  // octant form (kernels_fdmo.hip): one rank, 3D, every direction mirror-symmetric for every component, half lines of at most 128 entries
  // slab partitions: the quadrant form (x, y split locally; the z butterfly next to the all-to-all) under the same conditions on the GLOBAL line
  bool oct_ok = !F.single && !line && !std::getenv("PORO_FDMU_NO_OCT");
  // per-direction form (opt-in, poro_ctx_set_fdm_form; one rank, 3D): the same passes where only some directions are mirror-symmetric - one decision function (fdm_tables.hpp).
  // A box whose directions are all split is the octant form and takes its code path below; one with a line beyond the kernel's reach keeps the nodal kernels
  bool per_dir = false; FdmFormDecision form;
  bool planar = false;     // 2D, one rank: the quadrant form with a single plane, transforms as batched GEMMs (lines of any length; without the parity split where the end conditions differ)
  { int nn3[3] = {F.nn[0], F.nn[1], F.nn[2]}, sym3[3] = {F.nn[0], F.nn[1], multi ? F.ng : F.nn[2]};
    planar = dim == 2 && !multi && fdmo_planar_usable(dim, nn3);
    oct_ok = oct_ok && (planar || fdmo_usable(dim, sym3));
    bool symmetric = true, all_parity = true;
    for (int d = 0; d < dim; ++d) { symmetric = symmetric && same_ends[d]; all_parity = all_parity && parity[d]; }
    // the planar form also runs without the parity split; its split form and the 3D forms need the same ends everywhere and eigenvectors that are all even or odd
    oct_ok = oct_ok && ((planar && !symmetric) || (symmetric && all_parity));
    if (c->fdm_form == PORO_FDM_FORM_PER_DIRECTION && !c->fdm_form_fixed && dim == 3 && !multi && !F.single && !line && !std::getenv("PORO_FDMU_NO_OCT")) {
      form = fdm_form_decide(F.fix, parity_cd, nn3);
      per_dir = form.usable && !form.all_split;
    }
    if (per_dir) { fdmo_init_per_direction(c->fdm_oct, nn3, F.coef, form, c->stream); oct_ok = true; }
    else if (oct_ok && planar) fdmo_init_planar(c->fdm_oct, nn3, F.coef, c->stream, symmetric);
    else if (oct_ok && !multi) {
      fdmo_init(c->fdm_oct, nn3, F.coef, c->stream);
      // class-split passes: Q2 lines on which the vertex / midpoint classes decouple frequency by frequency - all nine (component, direction) lines must pass the numerical
      // check of class_split_tables; PORO_FDMO_CLASS_SPLIT=0 (read here, once per build) keeps the dense passes
      const char *hook = std::getenv("PORO_FDMO_CLASS_SPLIT");
      bool all = !(hook && std::atoi(hook) == 0);
      for (int d = 0; d < dim && all; ++d) for (int comp = 0; comp < dim && all; ++comp) {
        ClassSplitTables &CS = classes[d][key_of(comp, d)];
        if (!CS.n) CS = class_split_tables(ku, c->lines.hcell[d], F.fix[comp][d][0] != 0, F.fix[comp][d][1] != 0, tables[d][key_of(comp, d)]);
        all = all && CS.ok;
      }
      c->fdm_oct.class_split = all;
    }
    if (oct_ok && multi) { std::vector<int> node_layers(F.n_ranks); for (int q = 0; q < F.n_ranks; ++q) node_layers[q] = ku * F.layers[q];
                           fdmo_init_slab(c->fdm_oct, nn3, F.coef, F.rank, node_layers, c->comm.part.has_upper != 0, c->stream); } }
  // A direction takes the even / odd form of the nodal kernels (half the MFMA work) when it has the same ends and the parity for every component - all components
  // of a pass share one kernel
  for (int d = 0; d < dim; ++d) for (int comp = 0; comp < dim; ++comp) {
    if (line && d == last) continue;
    const bool global_dir = multi && d == last;
    const LineTables &T = tables[d][key_of(comp, d)];
    FdmuDir &D = global_dir ? F.last_global[comp] : F.dir[comp][d];
    if (!(planar && oct_ok && T.n > 320 && !same_ends[d])) fdmu_upload_dir(D, T, global_dir ? false : F.single, same_ends[d] && parity[d]);   // (the nodal kernels have no full-length form beyond 320 points; the planar form does not need them)
    if (oct_ok) { if (planar) fdmo_upload_dir_planar(c->fdm_oct, comp, d, T); else fdmo_upload_dir(c->fdm_oct, comp, d, T); }
    if (oct_ok && c->fdm_oct.class_split) fdmo_upload_dir_classes(c->fdm_oct, comp, d, classes[d][key_of(comp, d)]);
  }
  c->fdmu_t1.alloc(c->n_u); c->fdmu_t2.alloc(c->n_u); c->fdmu_t1.zero(c->stream); c->fdmu_t2.zero(c->stream);   // (only finite values ever live in the scratch arrays)
  if (!c->wz_u.p) { c->wz_u.alloc(c->n_u); c->wz_u.zero(c->stream); }
  if (oct_ok && !planar) fdmo_finalize(c->fdm_oct);
  c->fdm_oct.built = oct_ok;
  if (line) {
    std::vector<double> coef;
    for (int comp = 0; comp < dim; ++comp) {
      const std::vector<double> cc = moduli_line_coefficients(dim, ku, comp, c->lines.hcell[last], c->mod.layer[0], c->mod.layer[1], F.fix[comp][last][0] != 0, F.fix[comp][last][1] != 0);
      coef.insert(coef.end(), cc.begin(), cc.end());
    }
    F.line_coef.upload(coef);
    F.line_fac.alloc((size_t)(ku + 1) * c->n_u);                                    // reciprocal pivots and multipliers: (k_u + 1) n_u doubles, at most 3 n_u
    F.line = true;
    fdmu_line_factor(c->stream, ku, dim, fdmu_line_args(c), F.line_fac.p);            // T does not depend on dt: once per field
  }
  F.built = true;
}
FdmuLineArgs fdmu_line_args(poro_ctx *c) {
  const FdmU &F = c->fdm_u; const int dim = F.dim, last = dim - 1;
  FdmuLineArgs a{};
  a.nl = F.nn[last]; a.n0 = F.nn[0]; a.ncol = c->n_u / dim / a.nl; a.coef = F.line_coef.p;
  for (int comp = 0; comp < dim; ++comp) {
    a.lam0[comp] = F.dir[comp][0].lam.p; a.lam1[comp] = dim == 3 ? F.dir[comp][1].lam.p : nullptr;
    a.fixed[comp][0] = F.fix[comp][last][0]; a.fixed[comp][1] = F.fix[comp][last][1];
  }
  return a;
}
// slab form of the octant kernels: g, z in quadrant layout.  x / y sweeps on the local planes, whole z lines per column share between two all-to-alls
static void fdm_precondition_u_slab(poro_ctx *c, const double *g, double *z, const PcgScalars *gate) {
  hipStream_t s = c->stream; FdmOct &O = c->fdm_oct; auto &S = O.slab;
  double *send = S.buf.p, *recv = S.buf.p + S.recv_off;
  fdmo_slab_pass(s, O, 1, g, S.buf.p, gate);                                          // x, y forward on the local planes; the owned planes go straight into the exchange buffer
  alltoall_blocks(c, send, recv, (int64_t)S.max_own * S.scols, true);
  if (S.zboth) { Timed tp(c, "fdm_u_slab_z_stage"); fdmo_slab_pass(s, O, 2, S.buf.p, S.buf.p, gate); }   // whole z lines of this rank's column share, both parity parts per workgroup: gathered planes in, scattered planes out
  else {
    fdmo_slab_pass(s, O, 2, S.buf.p, S.tz.p, gate);                                   // (tile counts without that variant: one parity part per workgroup, then v_k = a + b, v_k' = a - b in a kernel of its own)
    Timed tp(c, "fdm_u_slab_z_stage"); fdmo_slab_scatter_pack(s, O, gate);
  }
  alltoall_blocks(c, send, recv, (int64_t)S.max_nl * S.scols, true);
  fdmo_slab_pass(s, O, 3, S.buf.p, z, gate);                                          // y, x backward, reading the received planes in place
}
// g, z in the layout of the form that is built (c->fdm_oct.built): quadrants on slabs, the planar form in 2D, octants on one rank - the one place that switches between them.
// The octant form runs as three transform dispatches.  A sampled call times them one by one (per-kernel roofline of the bench): the sampling runs on
// fdm_u_pass1, passes 2 and 3 are counted alongside and fdmo_apply takes one event pair per pass
// gz_part != null (octant form; the others ignore it): pass 2 also leaves the partial sums of g . z there (returns true: no separate dot kernel)
// scratch == null (octant form): the passes work on z itself (fp64 transforms only)
bool fdm_precondition_u_form(poro_ctx *c, const double *g, double *z, const PcgScalars *gate, int precision, double *scratch, double *gz_part, const PcgStopTest &stop) {
  Timed tm(c, "precondition_u_fdm");
  const FdmOct &O = c->fdm_oct;
  if (O.slab.on) { if (stop.gg_part) throw Error("fdm_precondition_u_form: the slab form runs no stopping test"); fdm_precondition_u_slab(c, g, z, gate); return false; }
  if (O.planar) { fdmo_apply_planar(c->stream, O, g, z, gate, stop); return false; }
  const char *names[3] = {"fdm_u_pass1", "fdm_u_pass2", "fdm_u_pass3"};
  if (fdmo_class_split_runs(O, precision)) c->timers["fdm_u_class_split"].enqueued++;      // (a count, no time: applications that took the class-split passes)
  if (!begin_sampled_dispatch(c, names[0])) {
    fdmo_apply(c->stream, O, g, z, scratch, gate, nullptr, gz_part, precision, stop);
    return gz_part != nullptr;
  }
  c->timers[names[1]].enqueued++;
  c->timers[names[2]].enqueued++;
  hipEvent_t ev[6];
  for (auto &e : ev) e = event_get(c);
  fdmo_apply(c->stream, O, g, z, scratch, gate, ev, gz_part, precision, stop);
  for (int k = 0; k < 3; ++k) {
    Timer &t = c->timers[names[k]];
    t.pending.emplace_back(ev[2 * k], ev[2 * k + 1]);
    t.launches++;
  }
  return gz_part != nullptr;
}
// nodal g -> whichever form of the block FDM is built -> nodal z
void fdm_precondition_u_nodal(poro_ctx *c, const double *g, double *z, int precision) {
  FdmOct &O = c->fdm_oct;
  if (!O.built) { fdm_precondition_u(c, g, z); return; }
  fdmo_from_nodal(c->stream, O, g, O.g.p); fdm_precondition_u_form(c, O.g.p, O.z.p, nullptr, precision, O.t.p); fdmo_to_nodal(c->stream, O, O.z.p, z);
}
// ---- additive two-level preconditioner on refinements of a uniform box (poro_desc.coarse) ----------------------------------------------------
// P holds every local row (prolongation / combination); its transpose (restriction) only the owned rows [0, n_owned), so that the pieces of a general partition
// sum every global row exactly once (one rank: n_owned = n_fine)
// row_bound > 0 (general partitions): the lanes of P follow from the longest possible row instead of the piece's mean row length.  The lane count fixes the order in
// which a row is summed, and the copies of a shared dof must come out bitwise equal on every rank that holds it
static void upload_interp(poro_ctx::Interp &T, int64_t n_fine, int64_t n_owned, int64_t n_coarse, const int64_t *ptr, const int32_t *node, const double *weight, const char *what,
                          int row_bound = 0) {
  T.n_fine = n_fine; T.n_coarse = n_coarse;
  validate_rows(ptr, node, weight, n_fine, n_coarse, std::string("poro_desc.coarse: ") + what);   // before ptr[n_fine] is used or a row is walked
  const int64_t nnz = ptr[n_fine], nnz_t = ptr[n_owned];
  const auto lanes_for = [](int64_t nnz, int64_t rows) { return nnz >= 6 * rows ? 8 : nnz >= 3 * rows ? 4 : 1; };   // mean row length -> lanes per row
  T.lanes = row_bound > 0 ? lanes_for(row_bound, 1) : lanes_for(nnz, n_fine); T.lanes_t = lanes_for(nnz_t, n_coarse);
  std::vector<int64_t> tp((size_t)n_coarse + 1, 0);
  for (int64_t k = 0; k < nnz_t; ++k) tp[node[k] + 1]++;
  { int64_t longest = 0; for (int64_t j = 0; j < n_coarse; ++j) longest = std::max(longest, tp[j + 1]);      // restriction: a few very long rows (refined block) beside single-entry ones
    if (longest >= 48) T.lanes_t = std::max(T.lanes_t, 16); }                     // (measured on the refined 32^3 box and the Gmsh grid: 16 lanes 3 % ahead of 8, 32 lanes behind both)
  for (int64_t j = 0; j < n_coarse; ++j) tp[j + 1] += tp[j];
  std::vector<int32_t> tc((size_t)nnz_t); std::vector<double> tw((size_t)nnz_t); std::vector<int64_t> pos(tp.begin(), tp.end() - 1);
  for (int64_t i = 0; i < n_fine; ++i) {
    if (i < n_owned) for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) { const int64_t at = pos[node[k]]++; tc[at] = (int32_t)i; tw[at] = weight[k]; }
  }
  T.p_ptr.upload(ptr, (size_t)n_fine + 1); T.p_col.upload(node, (size_t)nnz); T.p_w.upload(weight, (size_t)nnz);
  T.pt_ptr.upload(tp); T.pt_col.upload(tc); T.pt_w.upload(tw);
}
void setup_two_level(poro_ctx *c, const poro_desc *d) {
  auto &T = c->two_level; const int dim = c->dim;
  const bool general = c->comm.general;      // (rows of P interpolate the box's FE functions of one cell: at most (k + 1)^dim entries)
  upload_interp(T, c->n_u / dim, general ? c->comm.ifc_u.n_owned / dim : c->n_u / dim, T.box->n_u / dim, d->coarse.ptr, d->coarse.node, d->coarse.weight, "displacement",
                general ? ipow(c->k_u + 1, dim) : 0);
  if (d->coarse.ptr_p) {
    if (!d->coarse.node_p || !d->coarse.weight_p) throw Error("poro_desc.coarse: node_p / weight_p missing");
    upload_interp(T.pressure, c->n_p, general ? c->comm.ifc_p.n_owned : c->n_p, T.box->n_p, d->coarse.ptr_p, d->coarse.node_p, d->coarse.weight_p, "pressure", general ? 1 << dim : 0);
    // prescribed pressures: a fine dof that IS a coarse dof (one entry of weight 1) with a prescribed coarse value must be prescribed here as well, or the coarse
    // space would lack the function the fine space has there
    T.pdir_nested = false;
    const poro_desc *H = d->coarse.box_problem;
    if (c->n_pdir && H->n_dirichlet_p > 0 && H->dirichlet_dof_p) {
      std::vector<uint8_t> fine(c->n_p, 0), coarse(T.box->n_p, 0);
      for (int64_t i = 0; i < d->n_dirichlet_p; ++i) fine[d->dirichlet_dof_p[i]] = 1;
      for (int64_t i = 0; i < H->n_dirichlet_p; ++i) coarse[H->dirichlet_dof_p[i]] = 1;      // (range-checked when the box's context was created)
      bool ok = true;
      for (int64_t i = 0; i < c->n_p && ok; ++i) {
        const int64_t k = d->coarse.ptr_p[i];
        if (d->coarse.ptr_p[i + 1] - k == 1 && std::fabs(d->coarse.weight_p[k] - 1.0) <= 1e-12 && coarse[d->coarse.node_p[k]] && !fine[i]) ok = false;
      }
      T.pdir_nested = ok;
    }
  }
}
bool two_level_supported(poro_ctx *c) {
  if (!c->two_level.box) return false;
  analyse_fdm_u(c->two_level.box);
  return c->two_level.box->fdm_u_state == 1;
}
bool two_level_supported_p(poro_ctx *c) { return c->two_level.box && c->two_level.pressure.n_fine == c->n_p && fdm_p_supported(c->two_level.box); }
// the pressure Jacobian with prescribed rows: the coarse solve is (J_H)_ff^-1, the box's second table set, so the box must carry a prescribed set of whole faces itself,
// and the fine mesh must prescribe every dof that sits on a prescribed coarse dof (setup_two_level: pdir_nested)
bool two_level_supported_pj(poro_ctx *c) {
  return c->n_pdir && two_level_supported_p(c) && c->two_level.pdir_nested && c->two_level.box->n_pdir && fdm_pj_supported(c->two_level.box);
}
// the scalar analogue for the pressure Jacobian a M + kappa K and the projection mass matrix (a = 1, kappa = 0): Jacobi on this mesh + the box's exact fast diagonalisation
// inert: the rows of z left 0 (hanging rows; for the Jacobian also the prescribed ones).  coarse_set = Q1Set::fixed_ends: z = omega D^-1 g + P (J_H)_ff^-1 P^T g, the coarse box's
// table set without its prescribed faces' end nodes - whatever P^T g holds on those coarse rows, the coarse correction is exactly 0 there
void two_level_precondition_p(poro_ctx *c, double a, double kappa, const double *dinv, const double *g, double *z, double omega, const uint8_t *inert, Q1Set coarse_set) {
  Timed tm(c, "precondition_p_two_level");
  auto &T = c->two_level.pressure; poro_ctx *H = c->two_level.box; hipStream_t s = c->stream;
  build_fdm_q1(H, coarse_set);
  if (!H->wz_p.p) H->wz_p.alloc(H->n_p);
  double *rc = H->wg_p.p, *zc = H->wz_p.p;
  la_nodal_interp(s, T.pt_ptr.p, T.pt_col.p, T.pt_w.p, T.n_coarse, 1, g, rc, T.lanes_t);
  if (c->comm.multi()) allreduce_sum_vec(c, rc, T.n_coarse, "two_level_coarse_allreduce");      // partitioned: every rank restricted its owned rows; all hold P^T g after the sum
  const double kk[3] = {kappa, kappa, kappa};
  fdm_precondition_p(H, a, kk, rc, zc, coarse_set);
  la_two_level_combine(s, T.p_ptr.p, T.p_col.p, T.p_w.p, T.n_fine, 1, zc, g, dinv, inert, omega, z, T.lanes);
}
void two_level_precondition_u(poro_ctx *c, const double *g, double *z, double omega) {
  Timed tm(c, "precondition_u_two_level");
  auto &T = c->two_level; poro_ctx *H = T.box; hipStream_t s = c->stream; const int dim = c->dim;
  build_fdm_u(H);
  double *rc = H->wg_u.p, *zc = H->wz_u.p;                                  // the box context's work vectors (it never solves anything itself)
  la_nodal_interp(s, T.pt_ptr.p, T.pt_col.p, T.pt_w.p, T.n_coarse, dim, g, rc, T.lanes_t);              // r_H = P^T g
  // partitioned (general pieces): the owned rows' partial restriction, summed over the ranks.  The coarse solve then runs replicated on identical data and the
  // combination below covers every local row, so the copies of a shared dof stay bitwise equal.  One all-reduce per application on every rank alike
  if (c->comm.multi()) allreduce_sum_vec(c, rc, T.n_coarse * dim, "two_level_coarse_allreduce");
  fdm_precondition_u_nodal(H, rc, zc, PORO_FDM_FP64);                         // z_H = blockdiag(A_H)^-1 r_H (zero on the box's Dirichlet faces)
  la_two_level_combine(s, T.p_ptr.p, T.p_col.p, T.p_w.p, T.n_fine, dim, zc, g, c->dinv_u.p, c->cons_u.inert.p, omega, z, T.lanes);
}

void fdm_precondition_u(poro_ctx *c, const double *g, double *z) {
  Timed tm(c, "precondition_u_fdm");
  hipStream_t s = c->stream; FdmU &F = c->fdm_u;
  if (F.line) {      // per-cell moduli: x (y) forward, one banded solve per mode column and component along the last direction, (y) x backward
    fdmu_apply(s, F, g, z, c->fdmu_t1.p, c->fdmu_t2.p, 0);
    { Timed tl(c, "fdm_u_line_solve"); fdmu_line_solve(s, c->k_u, F.dim, fdmu_line_args(c), F.line_fac.p, F.dim == 3 ? c->fdmu_t2.p : c->fdmu_t1.p); }
    fdmu_apply(s, F, g, z, c->fdmu_t1.p, c->fdmu_t2.p, 1);
    return;
  }
  if (!F.dist) { fdmu_apply(s, F, g, z, c->fdmu_t1.p, c->fdmu_t2.p, 2); return; }
  // leading directions locally (the shared planes are transformed by both owners), then whole lines of the partitioned direction for this
  // rank's column group: gather by an all-to-all, fused forward / scale / backward pass with the GLOBAL 1D eigenvectors, scatter back
  const int dim = F.dim, N = F.n_ranks, r = F.rank, last = dim - 1, ku = c->k_u;
  const int nl = F.nn[last];
  fdmu_apply(s, F, g, z, c->fdmu_t1.p, c->fdmu_t2.p, 0);
  double *cur = dim == 3 ? c->fdmu_t2.p : c->fdmu_t1.p;
  auto ncols_of = [&](int q) { return std::max<int64_t>(0, std::min<int64_t>(F.C, F.ncol_total - (int64_t)q * F.C)); };
  auto own_of = [&](int q) { return ku * F.layers[q] + (q == N - 1 ? 1 : 0); };
  const int64_t blk1 = (int64_t)dim * F.max_own * F.C;
  for (int q = 0; q < N; ++q) fdmu_window(s, F.sendbuf.p + (size_t)q * blk1, cur, true, dim, own_of(r), F.max_own, F.C, ncols_of(q), F.ncol_total, nl, (int64_t)q * F.C, 0);
  alltoall_blocks(c, F.sendbuf.p, F.recvbuf.p, blk1);
  PORO_HIP(hipMemsetAsync(F.tz1.p, 0, (size_t)dim * F.ng * F.C * sizeof(double), s));
  for (int q = 0; q < N; ++q) fdmu_window(s, F.tz1.p, F.recvbuf.p + (size_t)q * blk1, false, dim, own_of(q), F.max_own, F.C, F.C, F.C, F.ng, 0, F.off[q]);
  fdmu_lines(s, F, F.last_global, F.C, (int64_t)r * F.C, ncols_of(r), F.tz1.p, F.tz2.p);
  const int64_t blk2 = (int64_t)dim * F.max_nl * F.C;
  for (int q = 0; q < N; ++q) fdmu_window(s, F.sendbuf.p + (size_t)q * blk2, F.tz2.p, true, dim, ku * F.layers[q] + 1, F.max_nl, F.C, F.C, F.C, F.ng, 0, F.off[q]);
  alltoall_blocks(c, F.sendbuf.p, F.recvbuf.p, blk2);
  for (int q = 0; q < N; ++q) fdmu_window(s, cur, F.recvbuf.p + (size_t)q * blk2, false, dim, nl, F.max_nl, F.C, ncols_of(q), F.ncol_total, nl, (int64_t)q * F.C, 0);
  fdmu_apply(s, F, g, z, c->fdmu_t1.p, c->fdmu_t2.p, 1);
}

// ---- what a context supports: the one verdict behind poro_supports_preconditioner and the three solve entry points ------------------------------------------------
// null where the preconditioner `prec` is usable on system `which_system` (0 displacement, 1 pressure Jacobian, 2 projection mass matrix), else the reason.  The
// per-feature predicates stay where their features are; the refusals inside the builders and solves remain as checks for internal callers.
// solving: asked by a solve entry point.  The one difference: a value that has no implementation on the system runs there as PORO_PREC_NONE does - CG without a
// preconditioner, the Krylov driver applies the diagonal for PORO_PREC_JACOBI alone (see the two marked lines)
const char *prec_refusal(poro_ctx *c, int which_system, int prec, bool solving) {
  static thread_local std::string why;
  if (prec == PORO_PREC_NONE || prec == PORO_PREC_JACOBI) return nullptr;
  const bool multi = c->comm.multi(), sweeps = prec == PORO_PREC_SSOR || prec == PORO_PREC_ILU0;
  const char *one_rank = prec == PORO_PREC_SSOR ? "PORO_PREC_SSOR is a single-rank fidelity mode (the sweeps are order dependent)"
                                                : "PORO_PREC_ILU0 is implemented for one rank (the factorisation is sequential in the row order)";
  if (which_system == 0) {
    // per-cell moduli (poro_ctx_set_cell_moduli): the coarse box of the two-level form and the tables of the block fast diagonalisation are constant-coefficient
    if (c->mod.kind && prec == PORO_PREC_TWO_LEVEL)
      return "PORO_PREC_TWO_LEVEL (displacement): not available while per-cell moduli are set - the coarse box is a constant-coefficient context (PORO_PREC_JACOBI / CHEBYSHEV / NONE everywhere, ILU0 / SSOR on the assembled operator, PORO_PREC_FDM on boxes and tensor-product grids)";
    if (prec == PORO_PREC_TWO_LEVEL)
      return two_level_supported(c) ? nullptr : "PORO_PREC_TWO_LEVEL needs poro_desc.coarse (a refinement of a uniform box whose Dirichlet conditions cover whole faces)";
    // condensed operators exist at operator level only: Jacobi, the polynomial built on it, the two-level form above
    if (c->cons_u.n && prec != PORO_PREC_CHEBYSHEV) return "meshes with constraint lists: PORO_PREC_JACOBI / CHEBYSHEV / TWO_LEVEL / NONE only (the operator is condensed on the fly)";
    if (prec == PORO_PREC_CHEBYSHEV) return nullptr;
    if (sweeps) return c->operator_mode != PORO_OP_CSR ? (prec == PORO_PREC_SSOR ? "PORO_PREC_SSOR needs the assembled CSR operator" : "PORO_PREC_ILU0 needs the assembled CSR operator") : multi ? one_rank : nullptr;
    if (prec == PORO_PREC_FDM) {
      analyse_fdm_u(c);                                      // (state 0, a partitioned context without a communicator yet: unsupported, and asked again next time)
      if (c->fdm_u_state == 1) return nullptr;
      why = "PORO_PREC_FDM (displacement): " + c->fdm_u_why;
      return why.c_str();
    }
    return solving ? nullptr : "unknown preconditioner";      // asymmetry kept: disp_solve runs an unknown value as PORO_PREC_NONE
  }
  if (which_system != 1 && which_system != 2) return "unknown system (0 displacement, 1 pressure, 2 projection)";
  // a per-cell k / mu (poro_ctx_set_cell_permeability): the coarse box of the two-level form is a constant-coefficient context
  if (which_system == 1 && c->perm.kind && prec == PORO_PREC_TWO_LEVEL)
    return "PORO_PREC_TWO_LEVEL (pressure): not available while a per-cell permeability is set - the coarse box is a constant-coefficient context (PORO_PREC_JACOBI / NONE / ILU0 / SSOR everywhere, PORO_PREC_FDM on boxes and tensor-product grids)";
  if (which_system == 1 && (c->cons_p.n || c->n_pdir)) {
    // hanging rows: the two-level form.  Prescribed rows: two-level where the coarse box carries the condition as whole faces (two_level_supported_pj), the
    // fixed-ends table set where they cover whole faces of a box / tensor grid on one rank (fdm_pj_supported: never with hanging rows)
    const bool ok = prec == PORO_PREC_TWO_LEVEL ? (!c->n_pdir || two_level_supported_pj(c)) : prec == PORO_PREC_FDM && fdm_pj_supported(c);
    if (!ok) return "meshes with hanging-node constraints or prescribed pressures: PORO_PREC_JACOBI / NONE (hanging nodes: also TWO_LEVEL; with prescribed pressures where the coarse box carries them as whole faces) only; prescribed pressures that cover whole faces of a uniform box or tensor-product grid on one rank: also PORO_PREC_FDM";
  }
  // (the projection's mass matrix has no prescribed rows)
  if (which_system == 2 && c->cons_p.n && prec != PORO_PREC_TWO_LEVEL) return "meshes with hanging-node constraints: PORO_PREC_JACOBI / TWO_LEVEL / NONE only";
  if (prec == PORO_PREC_TWO_LEVEL)
    return two_level_supported_p(c) ? nullptr : "PORO_PREC_TWO_LEVEL (pressure / projection): needs poro_desc.coarse with the pressure interpolation (ptr_p / node_p / weight_p)";
  if (sweeps) return multi ? one_rank : nullptr;
  if (prec == PORO_PREC_FDM) return fdm_p_supported(c) ? nullptr : "PORO_PREC_FDM needs a uniform box (poro_desc.box.enabled) and, when partitioned, an initialised communicator";
  return solving ? nullptr : "PORO_PREC_CHEBYSHEV (and unknown values) have no form on the Q1 systems";   // asymmetry kept: the Q1 solves run these as PORO_PREC_NONE; an error is a later issue
}

}  // namespace ctx_detail
}  // namespace poro

// Flow post-processing entry points: the Darcy velocity per cell, the discharge through boundary faces and its sums per label, and the terms of the discrete fluid
// mass balance (definitions: include/poroel_hip.h).  The kernels are in kernels_darcy.hip.  Pure additions: the calls read the context's state and write scratch of
// their own (poro_ctx::flux); no PORO_VEC_* vector changes.
#include <cmath>
#include "common.hpp"
#include "ctx_internal.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace {
// what the context holds now: the permeability form and rho_f g under the residual's own condition
DarcyArgs darcy_args(poro_ctx *c, const double *p) {
  DarcyArgs a{};
  a.dim = c->dim; a.ncomp = c->perm.kind ? c->perm.ncomp : 0; a.n_cells = c->n_cells; a.cell_X = c->cell_X.p; a.cell_dofs_p = c->cell_dofs_p.p; a.p = p;
  a.kappa = c->mat.k_over_mu; a.perm_cell = c->perm.kind ? c->perm.cell.p : nullptr;
  for (int k = 0; k < 3; ++k) a.rg.v[k] = c->grav.flux_on() && k < c->dim ? c->grav.rho_f * c->grav.g[k] : 0.0;
  if (!a.cell_X || !a.cell_dofs_p) throw Error("darcy: a mesh array is missing on the device");
  return a;
}
void build_flux(poro_ctx *c) {
  poro_ctx::Flux &F = c->flux;
  if (F.built) return;
  F.q.alloc((size_t)c->n_cells * c->dim); F.Qf.alloc((size_t)c->n_bfaces);
  F.m.alloc((size_t)c->n_p); F.t.alloc((size_t)c->n_p); F.rt.alloc((size_t)c->n_p); F.sums.alloc(6);
  if (c->n_pdir) { F.pdir_dof.upload(c->h_pdir_dof); F.out.alloc((size_t)c->n_pdir); }
  // m = M 1, the row sums of the context's own pressure mass matrix (the uncondensed one the residual applies)
  la_fill(c->stream, F.t.p, 1.0, c->n_p);
  la_csr_spmv(c->stream, c->Ap, c->Mp.p, F.t.p, F.m.p);
  F.built = true;
}
}  // namespace

extern "C" {

int poro_pres_darcy_velocity(poro_ctx *c, int which_vec, double *q_host) {
  return guarded([&] {
    require_single_rank(c, "poro_pres_darcy_velocity");
    if (!q_host) throw Error("null argument");
    const double *p = space_vector(c, which_vec, false, "poro_pres_darcy_velocity");
    PORO_HIP(hipSetDevice(c->device));
    build_flux(c);
    { Timed tm(c, "darcy"); darcy_cells(c->stream, darcy_args(c, p), c->flux.q.p); }
    PORO_HIP(hipMemcpyAsync(q_host, c->flux.q.p, (size_t)c->n_cells * c->dim * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PORO_HIP(hipStreamSynchronize(c->stream));
    return 0;
  });
}

int poro_pres_boundary_discharge(poro_ctx *c, int which_vec, double *Q_face_host, const int32_t *labels, int32_t n_labels, double *Q_label_host) {
  return guarded([&] {
    require_single_rank(c, "poro_pres_boundary_discharge");
    if (n_labels < 0 || (n_labels && (!labels || !Q_label_host))) throw Error("poro_pres_boundary_discharge: labels without a list or without a place for their sums");
    const double *p = space_vector(c, which_vec, false, "poro_pres_boundary_discharge");
    PORO_HIP(hipSetDevice(c->device));
    build_flux(c);
    poro_ctx::Flux &F = c->flux;
    if (n_labels) {
      if (F.labels.n < (size_t)n_labels) { PORO_HIP(hipStreamSynchronize(c->stream)); F.labels.alloc((size_t)n_labels); F.Ql.alloc((size_t)n_labels); }
      PORO_HIP(hipMemcpyAsync(F.labels.p, labels, (size_t)n_labels * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    { Timed tm(c, "darcy");
      { Timed t1(c, "darcy_bfaces"); darcy_bfaces(c->stream, darcy_args(c, p), c->n_bfaces, c->bface_cell.p, c->bface_local.p, F.Qf.p); }      // (the kernels alone, inside the call's family)
      { Timed t2(c, "darcy_label_sums"); darcy_label_sums(c->stream, c->n_bfaces, c->bface_id.p, F.Qf.p, F.labels.p, n_labels, F.Ql.p); } }
    if (Q_face_host && c->n_bfaces) PORO_HIP(hipMemcpyAsync(Q_face_host, F.Qf.p, (size_t)c->n_bfaces * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_labels) PORO_HIP(hipMemcpyAsync(Q_label_host, F.Ql.p, (size_t)n_labels * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PORO_HIP(hipStreamSynchronize(c->stream));
    return 0;
  });
}

int poro_pres_flow_balance(poro_ctx *c, double dt, poro_flow_balance_terms *out, double *outflow_dof_host) {
  return guarded([&] {
    require_single_rank(c, "poro_pres_flow_balance");
    if (!out) throw Error("null argument");
    if (!(dt > 0) || !std::isfinite(dt)) throw Error("poro_pres_flow_balance: time_step must be finite and > 0");
    PORO_HIP(hipSetDevice(c->device));
    build_flux(c);
    poro_ctx::Flux &F = c->flux;
    hipStream_t s = c->stream;
    const double *p = vec(c, PORO_VEC_P), *p_old = vec(c, PORO_VEC_P_OLD), *ev = vec(c, PORO_VEC_EPSV), *ev0 = vec(c, PORO_VEC_EPSV0);
    const PressureCoeffs k = pressure_coeffs(c, dt);
    {
      Timed tm(c, "flow_balance");
      // Rt = C^T(-r): the rows of poro_pres_assemble_residual and its la_cons_reduce, into scratch
      pressure_residual_rows(c, k, F.t.p, F.rt.p);
      la_cons_reduce(s, c->cons_p, F.rt.p);
      FlowBalanceArgs A{c->n_p, p, p_old, ev, ev0, F.m.p, k.src, F.rt.p, c->n_pdir ? c->pdir_mask.p : nullptr, k.c_strain, k.c_pres};
      { Timed t1(c, "flow_balance_sums"); flow_balance_partials(s, A, c->partials.p); la_reduce_finish(s, c->partials.p, 6, F.sums.p, 0); }   // (the one pass and its finish alone)
      if (outflow_dof_host && c->n_pdir) darcy_gather(s, c->n_pdir, F.pdir_dof.p, F.rt.p, F.out.p);
    }
    double h[6];
    PORO_HIP(hipMemcpyAsync(h, F.sums.p, sizeof(h), hipMemcpyDeviceToHost, s));
    if (outflow_dof_host && c->n_pdir) PORO_HIP(hipMemcpyAsync(outflow_dof_host, F.out.p, (size_t)c->n_pdir * sizeof(double), hipMemcpyDeviceToHost, s));
    PORO_HIP(hipStreamSynchronize(s));
    out->storage_rate_strain = h[0]; out->storage_rate_pressure = h[1]; out->source_sum = h[2];
    out->outflow_prescribed = h[3]; out->free_row_sum = h[4]; out->residual_l2 = std::sqrt(h[5]);
    return 0;
  });
}

}  // extern "C"

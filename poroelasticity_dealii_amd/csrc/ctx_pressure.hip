// The scalar Q1 systems (a M + kappa K) x = b on the pattern Ap - the pressure Jacobian and the projection mass matrix - and the extern "C" entry points of the pressure and
// projection stages (include/poroel_hip.h).  One place each for the coefficients of the pressure equation, its residual rows and the application of a Q1 operator.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include "common.hpp"
#include "ctx_internal.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace {
struct Q1System {
  double a, kappa;                    // (1 / (M_b dt), k / mu) or (1, 0)
  const double *val;                  // CSR values
  const double *dinv;                 // reciprocal diagonal, zero on the inert dofs
  DevBuf<double> *ilu;                // ILU(0) factor and whether it belongs to the present values
  bool *ilu_valid;
  double *x;
  const double *b;
  int *hint;                          // iteration counts of the last two solves
  const uint8_t *inert;               // the inert mask of the two-level and Jacobi paths; null selects the kernel form without a mask
  const uint8_t *inert_fdm = nullptr; // FDM: none, except with prescribed pressures on whole faces (the free-row system: residual norm and g . z see free rows only)
  Q1Set set = Q1Set::free_ends;       // FDM: the table set; fixed_ends = without the prescribed faces' end nodes
  Q1Set coarse_set = Q1Set::free_ends; // two-level: the coarse box's table set; fixed_ends = (J_H)_ff^-1 (the pressure Jacobian with prescribed rows)
  const double *kap = nullptr;        // a per-cell k / mu is set and the operator is the box stencil: the field in lattice cell order (kappa is then 1: val holds a M + K_kappa)
  int kap_ncomp = 0;                  // the planes of kap: c->perm.ncomp, 1 or dim (the diagonal tensor of poro_ctx_set_cell_permeability_tensor)
  int perm_kind = 0;                  // c->perm.kind for the pressure Jacobian (FDM: the line-solve form; direct only for kind 1), 0 for the projection
  bool distribute_inhom = true;       // constraints.distribute with the inhomogeneities; an UPDATE of a vector that already carries them (dp beside prescribed pressures) is distributed without
};

// the projection's mass matrix has no prescribed rows: where the pressure space has both lists its inert rows are the hanging ones alone
const uint8_t *proj_inert(poro_ctx *c) { return c->cons_p.hanging.p ? c->cons_p.hanging.p : c->cons_p.inert.p; }

// uniform box, matrix-free: both matrices are constant-coefficient stencils
bool q1_stencil(poro_ctx *c) { return c->operator_mode == PORO_OP_MATRIX_FREE && c->box.enabled; }

// A/B hook, read once per process: no direct pressure solve, and with it no batched Newton loop
bool pres_iterative_forced() { static const bool forced = std::getenv("PORO_PRES_ITERATIVE") != nullptr; return forced; }

// packed index of entry `tensor_index` (row-major, dim x dim) of a symmetric tensor (TensorIndexer.h:24-31)
int sym_entry(int dim, int tensor_index) {
  static const int m2[4] = {0, 1, 1, 2}, m3[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
  return dim == 2 ? m2[tensor_index] : m3[tensor_index];
}

// y = (a M + kappa K) x, uncondensed and rank-partial: the constant stencil, the stencil that reads the per-cell field, or the CSR values.  Only the first takes a gate
void q1_apply(poro_ctx *c, const Q1System &q, const double *x, double *y, const PcgScalars *gate = nullptr) {
  if (gate && (!q1_stencil(c) || q.kap)) throw Error("q1_apply: only the constant-coefficient stencil can be gated");
  if (!q1_stencil(c)) la_csr_spmv(c->stream, c->Ap, q.val, x, y);
  else if (q.kap) p_stencil_apply_var(c->stream, c->dim, c->box, q.a, q.kap, q.kap_ncomp, x, y);
  else p_stencil_apply(c->stream, c->dim, c->box, q.a, q.kappa, x, y, gate);
}

// the pressure Jacobian of c->jac_dt as form_jacobian left it; x, b and the prescribed-pressure adjustments are the caller's
Q1System jacobian_system(poro_ctx *c) {
  const PressureCoeffs k = pressure_coeffs(c, c->jac_dt);
  Q1System J;
  J.a = k.c_pres; J.kappa = k.kappa; J.perm_kind = c->perm.kind;
  if (c->perm.kind && q1_stencil(c)) { J.kap = c->perm.lattice.p; J.kap_ncomp = c->perm.ncomp; }
  J.val = c->Jp.p; J.dinv = c->dinv_J.p; J.hint = c->pcg_hint_p;
  J.ilu = &c->ilu_J; J.ilu_valid = &c->ilu_J_valid;
  J.inert = (c->cons_p.n || c->n_pdir) ? c->cons_p.inert.p : nullptr;     // hanging and prescribed rows alike (the union where both lists are present)
  return J;
}
// projection_matrix = mass_matrix (StrainProjector.h:104)
Q1System mass_system(poro_ctx *c) {
  Q1System M;
  M.a = 1.0; M.kappa = 0.0;
  M.val = c->Mp.p; M.dinv = c->dinv_M.p; M.hint = c->pcg_hint_proj;
  M.ilu = &c->ilu_M; M.ilu_valid = &c->ilu_M_valid;
  M.inert = c->cons_p.n ? proj_inert(c) : nullptr;
  return M;
}

// Direct solve of n <= 3 systems that share the operator q where the fast diagonalisation is the exact inverse (uniform box, slab partitions included: the
// distributed form is the same inverse): x_e = (a M + kappa K)^-1 b_e, then the residuals are checked against the reference's stopping rule with one poll
// for all norms.  info[e].iterations = 0 marks a directly solved system; returns whether every system met the rule (if not, x_e is a good start for CG).
// y: scratch of n vectors.  batched: all right-hand sides in one set of launches (c->q1_free.fused)
// q.set = Q1Set::fixed_ends + q.inert_fdm (prescribed pressures on whole faces): x_e = J_ff^-1 b_e on the free rows and exactly 0 on the masked ones; the check leaves the masked
// rows out, where (J x)_i is the coupling to the free neighbours and not part of the system
bool solve_q1_direct(poro_ctx *c, const Q1System &q, int n, const double *const *b, double *const *x, double *y_scratch, bool batched, const poro_solver_opts *opts, poro_solve_info *info) {
  // q.kap != null (a layered per-cell k / mu, one rank): the line-solve form is the exact inverse, the check runs through the variable-coefficient stencil
  hipStream_t s = c->stream;
  const double *y[3];
  for (int e = 0; e < n; ++e) y[e] = y_scratch + (size_t)e * c->n_p;
  const auto t0 = std::chrono::steady_clock::now();
  if (batched) {
    Timed tm(c, "precondition_p_fdm");
    count_strip_launches(c, fdmo_scalar_apply_many(s, c->q1_free.fused, q.a, q.kappa, n, b, x));
  } else {
    const double kk[3] = {q.kappa, q.kappa, q.kappa};
    for (int e = 0; e < n; ++e) { if (q.kap) fdm_precondition_p_layered(c, q.a, b[e], x[e], q.set); else fdm_precondition_p(c, q.a, kk, b[e], x[e], q.set); }
  }
  for (int e = 0; e < n; ++e) {
    { Timed tm(c, "apply_p_stencil"); q1_apply(c, q, x[e], const_cast<double *>(y[e])); }
    exchange_add(c, const_cast<double *>(y[e]), c->n_p, c->comm.part.plane_p);
  }
  la_residual_norms_many(s, n, y, b, owned(c, c->n_p, c->comm.part.plane_p), c->partials.p, q.inert_fdm);
  post_sums_and_wait(c, c->partials.p, 2 * n, 0, 2 * n);      // (sums: la_reduce_finish adds in the order of pcg_scalars_sum)
  bool all = true;
  for (int e = 0; e < n; ++e) {
    const double res = std::sqrt(c->mailbox->vals[2 * e]), bn = std::sqrt(c->mailbox->vals[2 * e + 1]);
    const bool ok = res <= std::max(opts->abs_tol, opts->rel_tol * bn);
    all = all && ok;
    if (!info) continue;
    info[e] = poro_solve_info{};
    info[e].iterations = 0;
    info[e].converged = ok ? 1 : 0;
    info[e].initial_residual = bn;
    info[e].final_residual = res;
    info[e].operator_applications = 1;
    info[e].seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n;
  }
  return all;
}

// ILU(0) / SSOR / fast-diagonalisation / two-level / Jacobi PCG on one system.  direct_first (FDM only): try the direct solve, whose result is the
// start of the iteration where its check fails
int solve_q1(poro_ctx *c, const Q1System &q, const poro_solver_opts *opts, poro_solve_info *info, bool direct_first = false) {
  const int prec = opts->preconditioner;
  const int64_t n = c->n_p, plane = c->comm.part.plane_p;
  KrylovSystem sys;
  sys.n = n; sys.plane = plane;
  sys.x = q.x; sys.b = q.b;
  sys.diag.full = q.dinv;
  sys.inert = q.inert;
  sys.g = c->wg_p.p; sys.d = c->wd_p.p; sys.h = c->wh_p.p;
  sys.cg1_set = 1;
  sys.hint = q.hint;
  if (prec == PORO_PREC_ILU0 || prec == PORO_PREC_SSOR) return pcg_csr_sweeps(c, c->Ap, q.val, *q.ilu, *q.ilu_valid, sys, opts, info);
  const char *const family = q1_stencil(c) ? "apply_p_stencil" : "apply_p_csr";
  // the condensed matrix C^T (a M + kappa K) C (:168, StrainProjector.h:104-105)
  sys.apply = [&](const double *x, double *y, double *) {
    la_cons_expand(c->stream, c->cons_p, const_cast<double *>(x), false);
    { Timed tm(c, family); q1_apply(c, q, x, y); }
    la_cons_reduce(c->stream, c->cons_p, y);
    exchange_add(c, y, n, plane);
    return false;
  };
  if (prec == PORO_PREC_FDM || prec == PORO_PREC_TWO_LEVEL) {
    if (!c->wz_p.p) c->wz_p.alloc(n);
    sys.prec.z = c->wz_p.p;
  }
  if (prec == PORO_PREC_FDM) {
    build_fdm_q1(c, q.set);
    if (direct_first) {
      poro_solve_info direct;
      if (solve_q1_direct(c, q, 1, &q.b, &q.x, sys.h, false, opts, &direct)) {
        if (info) *info = direct;
        return 0;
      }
    }
    const double kk[3] = {q.kappa, q.kappa, q.kappa};
    sys.inert = q.inert_fdm;
    sys.prec.fn = [&](const double *g, double *z, const PrecCall &) {
      if (q.perm_kind) fdm_precondition_p_layered(c, q.a, g, z, q.set);       // layer values (exact) or layer means
      else fdm_precondition_p(c, q.a, kk, g, z, q.set);
      return GzLeft::nowhere;
    };
    return pcg(c, sys, opts, info);
  }
  const double om = opts->omega > 0 ? opts->omega : 1.0;
  if (prec == PORO_PREC_TWO_LEVEL)
    sys.prec.fn = [&](const double *g, double *z, const PrecCall &) {
      two_level_precondition_p(c, q.a, q.kappa, q.dinv, g, z, om, q.inert, q.coarse_set);
      return GzLeft::nowhere;
    };
  const int rc = pcg(c, sys, opts, info);
  la_cons_expand(c->stream, c->cons_p, q.x, q.distribute_inhom);                // constraints.distribute (:180, StrainProjector.h:216)
  return rc;
}

}  // namespace

// the numbers of the pressure equation at time step dt, from what the context holds now
PressureCoeffs poro::ctx_detail::pressure_coeffs(poro_ctx *c, double dt) {
  PressureCoeffs k;
  k.c_strain = c->mat.biot_alpha / dt;
  k.c_pres = 1. / c->mat.biot_M / dt;
  k.kappa = c->perm.kind ? 1.0 : c->mat.k_over_mu;      // a per-cell k / mu: Kp holds K_kappa (coefficient 1), the box stencil reads the field
  k.strain_update = c->mat.biot_alpha / c->mat.bulk_K;
  k.src = c->grav.flux_on() ? c->grav.src_p.p : c->src_local.p;      // the well source alone, or (gravity with a fluid density) well + Darcy gravity flux, summed at set-up
  return k;
}

// rows = the uncondensed residual of PORO_VEC_P / P_OLD / EPSV / EPSV0 (tmp: its storage term, scratch of n_p).  What follows - condensation, exchange, masking, norm - differs
// by caller and stays there.  Only the constant-coefficient stencil takes a gate; no entry point reaches the refusal, since newton_loop_supported excludes the other two forms
void poro::ctx_detail::pressure_residual_rows(poro_ctx *c, const PressureCoeffs &k, double *tmp, double *rows, const PcgScalars *gate) {
  hipStream_t s = c->stream; const double *p = vec(c, PORO_VEC_P);
  const bool stencil = q1_stencil(c);
  if (gate && (!stencil || c->perm.kind)) throw Error("pressure_residual_rows: only the constant-coefficient stencil can be gated");
  la_pressure_tmp(s, tmp, vec(c, PORO_VEC_EPSV), vec(c, PORO_VEC_EPSV0), p, vec(c, PORO_VEC_P_OLD), k.c_strain, k.c_pres, c->n_p, gate);
  if (!stencil) la_csr_residual(s, c->Ap, c->Mp.p, c->Kp.p, k.kappa, tmp, p, k.src, rows);
  else if (c->perm.kind) p_residual_stencil_var(s, c->dim, c->box, c->perm.lattice.p, c->perm.ncomp, tmp, p, k.src, rows);
  else p_residual_stencil(s, c->dim, c->box, k.kappa, tmp, p, k.src, rows, gate);
}

extern "C" {

int poro_pres_apply_jacobian(poro_ctx *c, const double *x_host, double *y_host) {
  return guarded([&] {
    if (!c || !x_host || !y_host) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device)); hipStream_t s = c->stream;
    if (c->jac_dt < 0) throw Error("pres_apply_jacobian before pres_assemble_jacobian");
    DevBuf<double> x, y; x.upload(x_host, c->n_p); y.alloc(c->n_p);
    q1_apply(c, jacobian_system(c), x.p, y.p);
    exchange_add(c, y.p, c->n_p, c->comm.part.plane_p);
    PORO_HIP(hipMemcpyAsync(y_host, y.p, c->n_p * sizeof(double), hipMemcpyDeviceToHost, s)); PORO_HIP(hipStreamSynchronize(s)); return 0;
  });
}

int poro_pres_assemble_residual(poro_ctx *c, double dt, double *l2) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream; double *R = vec(c, PORO_VEC_RESIDUAL_P);
    { Timed tm(c, "pressure_residual"); pressure_residual_rows(c, pressure_coeffs(c, dt), c->tmp_p.p, R); }
    la_cons_reduce(s, c->cons_p, R);                                              // constraints.condense(residual) (:153); partial rows first, interface sums after
    exchange_add(c, R, c->n_p, c->comm.part.plane_p);
    if (c->n_pdir) la_mask_zero(s, R, c->pdir_mask.p, c->n_p);                    // prescribed-pressure rows are not part of the Newton system
    la_dot_partials(s, R, R, owned(c, c->n_p, c->comm.part.plane_p), c->partials.p);
    post_sums_and_wait(c, c->partials.p, 1, 0, 1);
    if (l2) *l2 = std::sqrt(c->mailbox->vals[0]);
    return 0;
  });
}

int poro_pres_apply_boundary_values(poro_ctx *c) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (c->n_pdir) la_set_constrained(c->stream, vec(c, PORO_VEC_P), c->pdir_mask.p, c->pdir_val.p, c->n_p);
    if (c->n_pdir && c->cons_p.n) {
      // hanging nodes beside the prescribed set: p[h] = sum w p[m] + b, so that a row with a prescribed master is conforming from the start (only updates are
      // distributed afterwards, homogeneously).  A dof in both lists reproduces its value up to rounding; the second pass makes it the listed value exactly
      la_cons_expand(c->stream, c->cons_p, vec(c, PORO_VEC_P), true);
      la_set_constrained(c->stream, vec(c, PORO_VEC_P), c->pdir_mask.p, c->pdir_val.p, c->n_p);
    }
    return 0;
  });
}

// J = M/(M_b dt) + (k/mu) K depends on dt only (the reference recomputes it every pressure iteration): same dt, same matrix
static int form_jacobian(poro_ctx *c, double dt) {
  if (c->jac_dt == dt) return 0;
  Timed tm(c, "pressure_jacobian");
  const PressureCoeffs k = pressure_coeffs(c, dt);
  la_jacobian(c->stream, c->Jp.p, c->Mp.p, c->Kp.p, k.c_pres, k.kappa, c->Ap.nnz);   // (per-cell k / mu: Kp holds K_kappa)
  la_csr_diag(c->stream, c->Ap, c->Jp.p, c->diag_J.p);
  exchange_add(c, c->diag_J.p, c->n_p, c->comm.part.plane_p);
  if (!c->dinv_J.p) c->dinv_J.alloc(c->n_p);
  la_reciprocal(c->stream, c->dinv_J.p, c->diag_J.p, c->n_p);
  if (c->cons_p.n || c->n_pdir) la_mask_zero(c->stream, c->dinv_J.p, c->cons_p.inert.p, c->n_p);
  c->ilu_J_valid = false;
  c->jac_dt = dt;
  return 0;
}
int poro_pres_assemble_jacobian(poro_ctx *c, double dt) {
  return guarded([&] { PORO_HIP(hipSetDevice(c->device)); return form_jacobian(c, dt); });
}

int poro_pres_solve(poro_ctx *c, const poro_solver_opts *opts, poro_solve_info *info) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (c->jac_dt < 0) throw Error("pres_solve before pres_assemble_jacobian");
    const int prec = opts->preconditioner;
    if (const char *why = prec_refusal(c, 1, prec, true)) throw Error(why);
    const bool fdm_fixed_ends = prec == PORO_PREC_FDM && c->n_pdir;                 // prescribed pressures on whole faces of a box / tensor grid, one rank (the verdict has checked fdm_pj_supported)
    const bool two_level_pdir = prec == PORO_PREC_TWO_LEVEL && c->n_pdir;           // the coarse box carries the prescribed set as whole faces (two_level_supported_pj)
    Q1System J = jacobian_system(c);
    J.x = vec(c, PORO_VEC_DP);
    J.b = vec(c, PORO_VEC_RESIDUAL_P);
    if (two_level_pdir) J.coarse_set = Q1Set::fixed_ends;
    if (c->n_pdir && (c->cons_p.n || two_level_pdir)) {
      J.distribute_inhom = false;
      la_mask_zero(c->stream, vec(c, PORO_VEC_RESIDUAL_P), c->pdir_mask.p, c->n_p);   // as on the fixed-ends path below: the prescribed rows are not part of the system, and the update is 0 there,
      la_mask_zero(c->stream, vec(c, PORO_VEC_DP), c->pdir_mask.p, c->n_p);           // so that a hanging row beside them (expanded homogeneously) gets its free masters' share alone
    }
    if (fdm_fixed_ends) {
      J.set = Q1Set::fixed_ends;
      J.inert_fdm = c->pdir_mask.p;
      la_mask_zero(c->stream, vec(c, PORO_VEC_RESIDUAL_P), c->pdir_mask.p, c->n_p);   // R_f: poro_pres_assemble_residual leaves zeros there already; a caller's own right-hand side may not
      la_mask_zero(c->stream, vec(c, PORO_VEC_DP), c->pdir_mask.p, c->n_p);           // the update is 0 there: CG never touches an inert row of its start vector, the direct solve writes 0 itself
    }
    // one rank or slabs, uniform box (2D or 3D): the fast diagonalisation is the exact inverse of J, so the update is computed directly and its residual checked
    // against the reference's stopping rule (:175); a failed check goes on to CG with that update as start
    const bool direct_first = prec == PORO_PREC_FDM && !pres_iterative_forced() && opts->stop_rule == PORO_STOP_RHS && q1_stencil(c) && c->perm.kind != 2;   // (a general field: the layer means precondition CG, never a direct solve)
    return solve_q1(c, J, opts, info, direct_first);
  });
}

int poro_pres_update_volumetric_strain(poro_ctx *c) {
  return guarded([&] { PORO_HIP(hipSetDevice(c->device)); if (c->mod.kind) la_strain_update_nodal(c->stream, vec(c, PORO_VEC_EPSV), vec(c, PORO_VEC_DP), c->mat.biot_alpha, c->mod.node.p, c->n_p);   // per-cell moduli: K = lambda + 2 G / 3 from the nodal means
                         else la_axpy(c->stream, vec(c, PORO_VEC_EPSV), c->mat.biot_alpha / c->mat.bulk_K, vec(c, PORO_VEC_DP), c->n_p);
                         return 0; });
}

// ---- the pressure Newton loop as gated batches (include/poroel_hip.h: poro_pres_newton_loop; newton_record.hpp) ---------------------------------------------------
static bool newton_loop_supported(poro_ctx *c, const poro_solver_opts *opts) {
  if (!c || !opts || c->pres_host_loop || pres_iterative_forced()) return false;
  // the constant-coefficient box stencil on one rank without constraint lists: nothing stands between the residual kernel and its norm, or between the stencil and its check
  if (!q1_stencil(c) || c->perm.kind || c->cons_p.n || c->n_pdir || c->comm.multi() || c->mod.kind || c->dim != 3) return false;
  if (opts->preconditioner != PORO_PREC_FDM || opts->stop_rule != PORO_STOP_RHS || prec_refusal(c, 1, PORO_PREC_FDM, true)) return false;
  build_fdm_q1(c, Q1Set::free_ends);
  return c->q1_free.fused.built && !c->q1_free.fused.slab.on;
}
int poro_supports_pres_newton_loop(poro_ctx *c, const poro_solver_opts *opts) {
  int yes = 0;
  const int rc = guarded([&] { PORO_HIP(hipSetDevice(c->device)); yes = newton_loop_supported(c, opts) ? 1 : 0; return 0; });
  return rc == 0 ? yes : 0;
}
int poro_pres_newton_loop(poro_ctx *c, double dt, double pressure_tol, int32_t max_iterations, const poro_solver_opts *opts, int32_t hint_slot, poro_newton_record *out) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (!out || !out->l2 || !out->res || !out->bn) throw Error("pres_newton_loop: no record");
    if (max_iterations < 1) throw Error("pres_newton_loop: max_iterations < 1");
    if (!newton_loop_supported(c, opts)) throw Error("pres_newton_loop: not supported on this context with these options (poro_supports_pres_newton_loop tells)");
    hipStream_t s = c->stream;
    form_jacobian(c, dt);      // (only where dt changed; before the batch, which cannot stop for it)
    const PressureCoeffs pk = pressure_coeffs(c, dt); const Q1System J = jacobian_system(c); const double strain = pk.strain_update;
    double *const p = vec(c, PORO_VEC_P), *const dp = vec(c, PORO_VEC_DP), *const R = vec(c, PORO_VEC_RESIDUAL_P), *const ev = vec(c, PORO_VEC_EPSV), *const y = c->wh_p.p;
    PcgScalars *const gate = c->newton_gate.p; double *const rec = c->newton_rec.p;
    const int predicted = hint_slot >= 0 && hint_slot < 8 ? c->newton_hint[hint_slot] : 0;
    NewtonState S; int batches = 0;
    while (!S.finished) {
      const NewtonBatch B = newton_plan_batch(S, max_iterations, predicted);
      if (B.slots < 1) throw Error("pres_newton_loop: empty batch");
      la_newton_reset(s, gate, rec);
      for (int j = 0; j < B.slots; ++j) {
        const bool solve_here = j + 1 < B.slots || B.last_solve, solved_before = j > 0;     // (a slot behind another one follows that one's solve part)
        if (j > 0 || B.first_residual) {
          if (!solved_before) la_axpy_gated(s, ev, strain, dp, c->n_p, gate);               // update_volumetric_strain (:360); behind a solve part: done with its p += dp
          { Timed tm(c, "pressure_residual"); pressure_residual_rows(c, pk, c->tmp_p.p, R, gate); }     // assemble_residual (:361-363), the rows of poro_pres_assemble_residual
          la_dot_partials(s, R, R, c->n_p, c->partials.p, gate);
          la_newton_residual_test(s, c->partials.p, pressure_tol, j, gate, rec);            // l2 < pressure_tol (:366)
        }
        if (solve_here) {
          {
            Timed tm(c, "precondition_p_fdm");                                              // solve (:378): dp = J^-1 R ...
            count_strip_launches(c, fdmo_scalar_apply(s, c->q1_free.fused, J.a, J.kappa, R, dp, gate));
          }
          { Timed tm(c, "apply_p_stencil"); q1_apply(c, J, dp, y, gate); }                  // ... checked against the reference's stopping rule (solve_q1_direct)
          const double *ys[1] = {y}, *bs[1] = {R};
          la_residual_norms_many(s, 1, ys, bs, c->n_p, c->partials.p, nullptr, gate);
          la_newton_check_test(s, c->partials.p, opts->abs_tol, opts->rel_tol, j, gate, rec);
          if (j + 1 < B.slots) la_newton_update(s, p, ev, strain, dp, c->n_p, gate);        // p += dp (:379) and the next iteration's update_volumetric_strain (:360)
          else la_axpy_gated(s, p, 1.0, dp, c->n_p, gate);                                  // p += dp (:379)
        }
      }
      // (the sums of a batch go to its record alone: c->red, where k_reduce_post leaves a copy of what it publishes, has no reader behind these calls)
      la_norm_partials(s, p, c->n_p, c->partials.p, c->partials.p + kMaxPartials);          // |p|_inf (:387-389), whatever the gate says
      newton_post_and_wait(c, c->partials.p + kMaxPartials);
      double r[kNewtonRecord];
      for (int k = 0; k < kNewtonRecord; ++k) r[k] = c->mailbox->vals[k];
      if (!newton_absorb(S, B, r, max_iterations)) throw Error("pres_newton_loop: the record of a batch contradicts what was enqueued");
      ++batches;
    }
    if (hint_slot >= 0 && hint_slot < 8) c->newton_hint[hint_slot] = S.entered;
    if (hint_slot == 0) c->timers["pressure_newton_batched"].enqueued++;      // (a count, no time: the time steps whose loop ran as batches - slot 0 is a step's first call)
    out->iterations = S.entered; out->solves = S.solves; out->outcome = S.code; out->batches = batches; out->pinf = S.pinf;
    for (size_t i = 0; i < S.l2.size(); ++i) out->l2[i] = S.l2[i];
    for (size_t i = 0; i < S.res.size(); ++i) { out->res[i] = S.res[i]; out->bn[i] = S.bn[i]; }
    return 0;
  });
}

int poro_proj_assemble_matrix(poro_ctx *c) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    la_csr_diag(c->stream, c->Ap, c->Mp.p, c->diag_M.p);                       // projection_matrix = mass_matrix (StrainProjector.h:104)
    exchange_add(c, c->diag_M.p, c->n_p, c->comm.part.plane_p);
    if (!c->dinv_M.p) c->dinv_M.alloc(c->n_p);
    la_reciprocal(c->stream, c->dinv_M.p, c->diag_M.p, c->n_p);
    if (c->cons_p.n) la_mask_zero(c->stream, c->dinv_M.p, proj_inert(c), c->n_p);
    c->projection_matrix_ready = true; return 0;
  });
}

int poro_proj_assemble_rhs(poro_ctx *c, const int32_t *tensor_components, int32_t n_comp) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    const int dim = c->dim; if (n_comp < 0 || n_comp > 6) throw Error("n_comp out of range");
    double *rhs[6];
    for (int k = 0; k < n_comp; ++k) {
      if (tensor_components[k] < 0 || tensor_components[k] >= dim * dim) throw Error("tensor component out of range");
      rhs[k] = vec(c, PORO_VEC_PROJ_RHS0 + sym_entry(dim, tensor_components[k])); if (!c->box_asm) la_fill(c->stream, rhs[k], 0.0, c->n_p);   // :146-147
    }
    {
      Timed tm(c, "projection_rhs");
      if (c->box_asm) box_proj_rhs(c->stream, c->dim, c->box_cpl, vec(c, PORO_VEC_U), n_comp, tensor_components, rhs);
      else {
        const AsmArgs a = asm_args(c);
        for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_proj_rhs(c->stream, a, cells, n_cells, vec(c, PORO_VEC_U), n_comp, tensor_components, rhs); });
      }
    }
    for (int k = 0; k < n_comp; ++k) { la_cons_reduce(c->stream, c->cons_p, rhs[k]); exchange_add(c, rhs[k], c->n_p, c->comm.part.plane_p); }   // StrainProjector.h:191-194 (partial rows folded, then the interface sums)
    return 0;
  });
}

int poro_proj_solve(poro_ctx *c, int32_t entry, const poro_solver_opts *opts, poro_solve_info *info) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (!c->projection_matrix_ready) throw Error("proj_solve before proj_assemble_matrix");
    if (entry < 0 || entry >= c->dim * (c->dim + 1) / 2) throw Error("rhs_entry out of range");
    const int prec = opts->preconditioner;
    if (const char *why = prec_refusal(c, 2, prec, true)) throw Error(why);
    Q1System M = mass_system(c);
    M.x = vec(c, PORO_VEC_STRAIN0 + entry);
    M.b = vec(c, PORO_VEC_PROJ_RHS0 + entry);
    return solve_q1(c, M, opts, info);
  });
}

// Several projection systems at once (the three normal strains of a time step, PoroelasticityFSS.h:153-164).  Where the fast diagonalisation is the EXACT inverse of the
// projection mass matrix (uniform box or tensor grid, no constraint lists) the systems are solved directly (solve_q1_direct; stopping rule of the reference's CG:
// SolverControl, StrainProjector.h:209).  Otherwise - or if a check fails - every entry goes through poro_proj_solve.  info[e].iterations = 0 marks a directly solved entry.
int poro_proj_solve_many(poro_ctx *c, const int32_t *entries, int32_t n_entries, const poro_solver_opts *opts, poro_solve_info *info) {
  if (!c || !entries || !opts || n_entries < 0) { g_err = "null argument"; return -1; }
  int done_direct = 0;
  const int rc0 = guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    if (!c->projection_matrix_ready) throw Error("proj_solve before proj_assemble_matrix");
    for (int e = 0; e < n_entries; ++e) if (entries[e] < 0 || entries[e] >= c->dim * (c->dim + 1) / 2) throw Error("rhs_entry out of range");
    static const bool iterative = std::getenv("PORO_PROJ_ITERATIVE") != nullptr;
    if (n_entries < 1) return 0;
    if (const char *why = prec_refusal(c, 2, opts->preconditioner, true)) throw Error(why);      // (FDM past this line: no constraint list, fdm_p_supported)
    if (iterative || opts->preconditioner != PORO_PREC_FDM || opts->stop_rule != PORO_STOP_RHS || !q1_stencil(c) || n_entries > 3) return 0;
    build_fdm_q1(c, Q1Set::free_ends);
    const bool batched = !c->comm.multi() && c->q1_free.fused.built && !c->q1_free.fused.slab.on;      // one rank, 3D, lines of <= 128 vertices: all right-hand sides in one set of launches
    if (c->proj_y.n < (size_t)3 * c->n_p) c->proj_y.alloc((size_t)3 * c->n_p);
    const double *b[3];
    double *x[3];
    for (int e = 0; e < n_entries; ++e) {
      b[e] = vec(c, PORO_VEC_PROJ_RHS0 + entries[e]);
      x[e] = vec(c, PORO_VEC_STRAIN0 + entries[e]);
    }
    done_direct = solve_q1_direct(c, mass_system(c), n_entries, b, x, c->proj_y.p, batched, opts, info) ? 1 : 0;     // (a failed check leaves x_e = M^-1 b_e as the warm start of the iterative solve below)
    return 0;
  });
  if (rc0 != 0) return rc0;
  if (done_direct) return 0;
  int worst = 0;
  for (int e = 0; e < n_entries; ++e) { const int rc = poro_proj_solve(c, entries[e], opts, info ? info + e : nullptr); if (rc < 0) return rc; worst = std::max(worst, rc); }
  return worst;
}

int poro_get_volumetric_strain(poro_ctx *c) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    const int dim = c->dim; const double *sp[3];
    for (int a = 0; a < dim; ++a) sp[a] = vec(c, PORO_VEC_STRAIN0 + sym_entry(dim, a * dim + a));
    la_sum_strains(c->stream, vec(c, PORO_VEC_EPSV), sp, dim, c->n_p); return 0;
  });
}

int poro_get_effective_stresses(poro_ctx *c) {
  return guarded([&] {
    PORO_HIP(hipSetDevice(c->device));
    const int ne = c->dim * (c->dim + 1) / 2; const double *e[6]; double *g[6];
    for (int k = 0; k < ne; ++k) { e[k] = vec(c, PORO_VEC_STRAIN0 + k); g[k] = vec(c, PORO_VEC_STRESS0 + k); }
    if (c->mod.kind) la_effective_stress_nodal(c->stream, e, g, c->dim, c->mod.node.p, c->n_p);      // per-cell moduli: the nodal means
    else la_effective_stress(c->stream, e, g, c->dim, c->mat.lame_lambda, c->mat.shear_G, c->n_p);
    PORO_HIP(hipStreamSynchronize(c->stream)); return 0;
  });
}

}  // extern "C"

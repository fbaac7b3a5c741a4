// Mechanical post-processing entry points: strain, effective and total stress per cell, principal stresses / invariants / the Mohr-Coulomb function with a device-side
// summary, and the force balance of the displacement system with the support reactions (definitions: include/poroel_hip.h).  The kernels are in kernels_stress.hip.
// Pure additions: the calls read the context's state and write scratch of their own (poro_ctx::stress); no PORO_VEC_* vector changes.
#include <cmath>
#include "common.hpp"
#include "ctx_internal.hpp"
#include "stress_measures.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace {
constexpr double kHalfPi = 1.57079632679489661923;

int n_sym(const poro_ctx *c) { return c->dim * (c->dim + 1) / 2; }

void build_cells(poro_ctx *c) {
  poro_ctx::Stress &S = c->stress;
  if (S.cells_built) return;
  const size_t n = (size_t)c->n_cells * n_sym(c);
  S.strain.alloc(n); S.eff.alloc(n); S.tot.alloc(n); S.measures.alloc((size_t)c->n_cells * kStressMeasures); S.summary.alloc(3); S.partials.alloc((size_t)16 * kMaxPartials);
  S.cells_built = true;
}
// what the context holds now: the moduli (the scalars or the cells' own pairs) and Biot's coefficient; p null: no pressure
void run_stress_cells(poro_ctx *c, const double *u, const double *p) {
  StressArgs a{};
  a.dim = c->dim; a.k_u = c->k_u; a.n_cells = c->n_cells; a.cell_X = c->cell_X.p; a.cell_dofs_u = c->cell_dofs_u.p; a.cell_dofs_p = c->cell_dofs_p.p; a.u = u; a.p = p;
  a.lam = c->mat.lame_lambda; a.G = c->mat.shear_G; a.alpha = c->mat.biot_alpha; a.cell_mod = c->mod.kind ? c->mod.cell.p : nullptr;
  if (c->mod.kind && !a.cell_mod) throw Error("cell stress: the per-cell moduli are missing on the device");
  stress_cells(c->stream, a, c->stress.strain.p, c->stress.eff.p, c->stress.tot.p);
}

void build_balance(poro_ctx *c) {
  poro_ctx::Stress &S = c->stress;
  if (S.balance_built) return;
  hipStream_t s = c->stream;
  build_cells(c);                                                  // (the partial slabs)
  S.au.alloc((size_t)c->n_u); S.cpl.alloc((size_t)c->n_u); S.neu.alloc((size_t)c->n_u); S.sums.alloc(19);
  if (c->h_dir_dof.size()) S.out.alloc(c->h_dir_dof.size());
  if (c->box_asm) { S.zero_u.alloc((size_t)c->n_u); S.zero_u.zero(s); S.zero_mask.alloc((size_t)c->n_u); S.zero_mask.zero(s); }
  S.comp.alloc((size_t)c->n_u); S.comp.zero(s);
  dof_components(s, c->n_cells * (int64_t)c->dpc_u, c->dim, c->cell_dofs_u.p, S.comp.p);
  S.balance_built = true;
}
// y = A_full x: the unconstrained operator of the lifting, in the branch the context's matrix build takes
void apply_A_full(poro_ctx *c, const double *x, double *y) {
  hipStream_t s = c->stream; const AsmArgs a = asm_args(c);
  if (box_fast_u(c) && (c->operator_mode == PORO_OP_MATRIX_FREE || c->box_asm)) {
    if (!c->matrix_built || !c->Ke.p) {                           // the element matrix the matrix build would make (the same kernel, the same bits)
      if (!c->Ke.p) c->Ke.alloc((size_t)c->dpc_u * c->dpc_u);
      asm_u_element_matrix(s, a, 0, c->Ke.p);
    }
    mf_operator(c, x, y, false);
  } else count_mfg_launches(c, mfg_apply(s, a, c->color_cells.p, c->color_off, c->n_u, x, y, false, 0));
}
}  // namespace

extern "C" {

int poro_disp_cell_stress(poro_ctx *c, int which_u, int which_p, double *strain_host, double *stress_eff_host, double *stress_tot_host) {
  return guarded([&] {
    require_single_rank(c, "poro_disp_cell_stress");
    const double *u = space_vector(c, which_u, true, "poro_disp_cell_stress");
    const double *p = which_p == -1 ? nullptr : space_vector(c, which_p, false, "poro_disp_cell_stress");
    PORO_HIP(hipSetDevice(c->device));
    build_cells(c);
    { Timed tm(c, "cell_stress"); run_stress_cells(c, u, p); }
    const size_t bytes = (size_t)c->n_cells * n_sym(c) * sizeof(double);
    if (bytes) {
      if (strain_host) PORO_HIP(hipMemcpyAsync(strain_host, c->stress.strain.p, bytes, hipMemcpyDeviceToHost, c->stream));
      if (stress_eff_host) PORO_HIP(hipMemcpyAsync(stress_eff_host, c->stress.eff.p, bytes, hipMemcpyDeviceToHost, c->stream));
      if (stress_tot_host) PORO_HIP(hipMemcpyAsync(stress_tot_host, c->stress.tot.p, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    PORO_HIP(hipStreamSynchronize(c->stream));
    return 0;
  });
}

int poro_disp_cell_measures(poro_ctx *c, int which_u, int which_p, const poro_mohr_coulomb *mc, double *measures_host, poro_failure_summary *summary) {
  return guarded([&] {
    require_single_rank(c, "poro_disp_cell_measures");
    const double *u = space_vector(c, which_u, true, "poro_disp_cell_measures");
    if (which_p != -1) space_vector(c, which_p, false, "poro_disp_cell_measures");       // checked, then ignored: the measures are of the effective stress
    if (mc && !(mc->cohesion >= 0 && std::isfinite(mc->cohesion))) throw Error("poro_disp_cell_measures: the cohesion must be finite and >= 0");
    if (mc && !(mc->friction_angle >= 0 && mc->friction_angle < kHalfPi)) throw Error("poro_disp_cell_measures: the friction angle must lie in [0, pi/2) (radians)");
    PORO_HIP(hipSetDevice(c->device));
    build_cells(c);
    poro_ctx::Stress &S = c->stress;
    const bool with_mc = mc && c->n_cells;
    {
      Timed tm(c, "cell_measures");
      run_stress_cells(c, u, nullptr);
      stress_measures_cells(c->stream, c->dim, c->n_cells, S.strain.p, S.eff.p, c->mat.lame_lambda, c->mod.kind ? c->mod.cell.p : nullptr, with_mc,
                            mc ? std::sin(mc->friction_angle) : 0.0, mc ? mc->cohesion * std::cos(mc->friction_angle) : 0.0, S.measures.p, S.partials.p, S.summary.p);
    }
    double h[3] = {0, 0, 0};
    if (measures_host && c->n_cells) PORO_HIP(hipMemcpyAsync(measures_host, S.measures.p, (size_t)c->n_cells * kStressMeasures * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (with_mc) PORO_HIP(hipMemcpyAsync(h, S.summary.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PORO_HIP(hipStreamSynchronize(c->stream));
    if (summary) { summary->max_f = h[0]; summary->argmax_cell = (int64_t)h[1]; summary->n_failing = (int64_t)h[2]; }
    return 0;
  });
}

int poro_disp_force_balance(poro_ctx *c, poro_force_balance_terms *out, double *reaction_dof_host) {
  return guarded([&] {
    require_single_rank(c, "poro_disp_force_balance");
    if (!out) throw Error("null argument");
    PORO_HIP(hipSetDevice(c->device));
    build_balance(c);
    poro_ctx::Stress &S = c->stress;
    hipStream_t s = c->stream; const AsmArgs a = asm_args(c);
    const int dim = c->dim, n_sets = 5 * dim + 1;
    const int64_t n_dir = (int64_t)c->h_dir_dof.size();
    const double *u = vec(c, PORO_VEC_U), *p = vec(c, PORO_VEC_P);
    const double *body = c->grav.on ? c->grav.body_u.p : nullptr;
    {
      Timed tm(c, "force_balance");
      // the three parts of b on all rows: the right-hand side's own builders with a zero mask, zero lifting and no loads; the tractions alone from zero
      if (c->box_asm) box_rhs_u(s, dim, c->box_cpl, c->mat.biot_alpha, p, S.zero_u.p, S.zero_u.p, S.zero_mask.p, S.cpl.p);
      else {
        la_fill(s, S.cpl.p, 0.0, c->n_u);
        for_each_colour(c, [&](const int32_t *cells, int64_t n_cells) { asm_u_rhs(s, a, cells, n_cells, p, S.cpl.p); });
      }
      la_fill(s, S.neu.p, 0.0, c->n_u);
      asm_u_neumann(s, a, c->bface_order.p, c->bface_group_off, c->bface_cell.p, c->bface_local.p, c->bface_id.p, c->n_neumann, c->neu_label.p, c->neu_comp.p, c->neu_val.p, S.neu.p);
      apply_A_full(c, u, S.au.p);
      force_residual(s, c->n_u, S.au.p, S.cpl.p, S.neu.p, body, S.au.p);                  // r, in place
      la_fill(s, S.sums.p + 16, 0.0, 3);
      if (c->cons_u.n) force_deficit(s, dim, c->cons_u, S.au.p, S.comp.p, S.sums.p + 16);  // what the closed list no longer carries to prescribed masters
      la_cons_reduce(s, c->cons_u, S.au.p);                                              // Rt = C^T r
      ForceBalanceArgs A{c->n_u, S.comp.p, c->dir_mask.p, S.au.p, S.neu.p, body, S.cpl.p};
      force_balance_partials(s, dim, A, S.partials.p);
      la_reduce_finish(s, S.partials.p, n_sets, S.sums.p, 0);
      if (reaction_dof_host && n_dir) darcy_gather(s, n_dir, c->dir_dofs.p, S.au.p, S.out.p);
    }
    double h[19] = {};
    PORO_HIP(hipMemcpyAsync(h, S.sums.p, sizeof(h), hipMemcpyDeviceToHost, s));
    if (reaction_dof_host && n_dir) PORO_HIP(hipMemcpyAsync(reaction_dof_host, S.out.p, (size_t)n_dir * sizeof(double), hipMemcpyDeviceToHost, s));
    PORO_HIP(hipStreamSynchronize(s));
    *out = poro_force_balance_terms{};
    for (int k = 0; k < dim; ++k) {
      out->reaction_sum[k] = h[5 * k] + h[16 + k]; out->free_row_sum[k] = h[5 * k + 1]; out->traction_sum[k] = h[5 * k + 2]; out->body_sum[k] = h[5 * k + 3]; out->coupling_sum[k] = h[5 * k + 4];
    }
    out->residual_l2 = std::sqrt(h[5 * dim]);
    return 0;
  });
}

}  // extern "C"

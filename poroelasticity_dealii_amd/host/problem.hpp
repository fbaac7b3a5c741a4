// Host-side mirror of the reference's operator interface for the hot path: the same class and member
// names, argument meaning and error behaviour as lib/include/PoroElasticDisplacementSolver.h,
// PoroElasticPressureSolver.h, StrainProjector.h and the FSS loop of PoroelasticityFSS.h:294-415,
// forwarding to the C-ABI of include/poroel_hip.h.  deal.II Vector<double> members become handles to
// device-resident vectors; nothing here computes on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include <fstream>
#include <cstdio>
#include "../../include/poroel_hip.h"
#include "mesh.hpp"
#include "run_controls.hpp"

namespace poro_host {

// analogue of dealii::SolverControl::NoConvergence (thrown by cg.solve, e.g. PoroElasticDisplacementSolver.h:305)
struct NoConvergence : std::runtime_error {
  int last_step; double last_residual;
  NoConvergence(const std::string &who, int it, double r)
      : std::runtime_error(who + ": iterative method did not converge in " + std::to_string(it) + " steps, residual " + std::to_string(r)),
        last_step(it), last_residual(r) {}
};

inline void check(int rc, const char *what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + poro_last_error());
}

// stand-in for dealii::Vector<double> members that now live in HBM
struct DeviceVector {
  poro_ctx *ctx = nullptr; int id = -1;
  DeviceVector &operator=(double v) { check(poro_vec_fill(ctx, id, v), "vec_fill"); return *this; }
  DeviceVector &operator=(const DeviceVector &o) { if (o.id != id || o.ctx != ctx) check(poro_vec_copy(ctx, id, o.id), "vec_copy"); return *this; }
  DeviceVector &operator+=(const DeviceVector &o) { check(poro_vec_axpy(ctx, id, 1.0, o.id), "vec_axpy"); return *this; }
  double l2_norm() const { double a, b; check(poro_vec_norm(ctx, id, &a, &b), "vec_norm"); return a; }
  double linfty_norm() const { double a, b; check(poro_vec_norm(ctx, id, &a, &b), "vec_norm"); return b; }
  void get(std::vector<double> &h, int64_t n) const { h.resize(n); check(poro_vec_get(ctx, id, h.data(), n), "vec_get"); }
};

}  // namespace poro_host

namespace solvers {
using poro_host::DeviceVector;

template <int dim> class PoroElasticDisplacementSolver {
 public:
  DeviceVector solution;                                   // PoroElasticDisplacementSolver.h:47
  poro_solver_opts control{1e-12, 0.0, 1000, PORO_PREC_JACOBI, 1.2, PORO_STOP_RHS, 0};   // :298-299, omega :303 (Jacobi is the fast default; PORO_PREC_SSOR = the reference's)
  poro_solve_info  last{};
  explicit PoroElasticDisplacementSolver(poro_ctx *c) : ctx(c) { solution.ctx = c; solution.id = PORO_VEC_U; }
  void rebind(poro_ctx *c) { ctx = c; solution.ctx = c; rebuild_system_matrix = true; }   // a new mesh (refine_mesh): the solver follows the problem to its new context
  void setup_dofs() { rebuild_system_matrix = true; }      // :106-153 (pattern / constraints are built by poro_ctx_create)
  // :155-291 — pressure_solution must be the pressure solver's `solution`
  void assemble_system(DeviceVector &pressure_solution) {
    if (pressure_solution.id != PORO_VEC_P) throw std::invalid_argument("assemble_system expects pressure_solver.solution");
    poro_host::check(poro_disp_assemble_system(ctx, rebuild_system_matrix ? 1 : 0), "disp_assemble_system");
    rebuild_system_matrix = false;                         // :290
  }
  void solve() {                                           // :294-307
    const int rc = poro_disp_solve(ctx, &control, &last);
    poro_host::check(rc, "disp_solve");
    if (rc > 0) throw poro_host::NoConvergence("PoroElasticDisplacementSolver::solve", last.iterations, last.final_residual);
  }
 private:
  poro_ctx *ctx; bool rebuild_system_matrix = true;        // :55
};

template <int dim> class PoroElasticPressureSolver {
 public:
  DeviceVector solution, solution_update, old_solution, residual;   // PoroElasticPressureSolver.h:38-40
  poro_solver_opts control{0.0, 1e-8, 1000, PORO_PREC_JACOBI, 1.0, PORO_STOP_RHS, 0};       // :175, omega :178
  poro_solve_info  last{};
  explicit PoroElasticPressureSolver(poro_ctx *c) : ctx(c) {
    solution.ctx = solution_update.ctx = old_solution.ctx = residual.ctx = c;
    solution.id = PORO_VEC_P; solution_update.id = PORO_VEC_DP; old_solution.id = PORO_VEC_P_OLD; residual.id = PORO_VEC_RESIDUAL_P;
  }
  void rebind(poro_ctx *c) { ctx = c; solution.ctx = solution_update.ctx = old_solution.ctx = residual.ctx = c; }
  void setup_dofs() {}                                     // :68-111 (mass / Laplace matrices are built by poro_ctx_create)
  void assemble_jacobian(double time_step) { poro_host::check(poro_pres_assemble_jacobian(ctx, time_step), "pres_assemble_jacobian"); }   // :158-169
  // :113-155 — the strains must be the problem's volumetric_strain / initial_volumetric_strain
  void assemble_residual(double time_step, DeviceVector &volumetric_strain, DeviceVector &initial_volumetric_strain) {
    if (volumetric_strain.id != PORO_VEC_EPSV || initial_volumetric_strain.id != PORO_VEC_EPSV0) throw std::invalid_argument("assemble_residual expects the problem's strain vectors");
    poro_host::check(poro_pres_assemble_residual(ctx, time_step, &residual_l2), "pres_assemble_residual");
  }
  void update_volumetric_strain(DeviceVector &volumetric_strain) {   // :187-194
    if (volumetric_strain.id != PORO_VEC_EPSV) throw std::invalid_argument("update_volumetric_strain expects the problem's volumetric_strain");
    poro_host::check(poro_pres_update_volumetric_strain(ctx), "pres_update_volumetric_strain");
  }
  void solve() {                                           // :172-185
    const int rc = poro_pres_solve(ctx, &control, &last);
    poro_host::check(rc, "pres_solve");
    if (rc > 0) throw poro_host::NoConvergence("PoroElasticPressureSolver::solve", last.iterations, last.final_residual);
  }
  // The whole Newton loop of one fixed-stress iteration (:358-380) as gated batches, where the context supports it (poro_pres_newton_loop): the host waits once.
  // The record holds what the per-call loop would have produced; `last` is the info of the last solve whose check held
  bool newton_loop_supported() { return poro_supports_pres_newton_loop(ctx, &control) != 0; }
  const poro_newton_record &newton_loop(double time_step, double pressure_tol, int max_iterations, int hint_slot) {
    rec_l2.assign(max_iterations, 0.0); rec_res.assign(max_iterations, 0.0); rec_bn.assign(max_iterations, 0.0);
    record = poro_newton_record{}; record.l2 = rec_l2.data(); record.res = rec_res.data(); record.bn = rec_bn.data();
    poro_host::check(poro_pres_newton_loop(ctx, time_step, pressure_tol, max_iterations, &control, hint_slot, &record), "pres_newton_loop");
    if (record.solves > 0) {
      last = poro_solve_info{}; last.iterations = 0; last.converged = 1; last.initial_residual = rec_bn[record.solves - 1]; last.final_residual = rec_res[record.solves - 1]; last.operator_applications = 1;
    }
    return record;
  }
  double residual_l2 = 0;   // residual.l2_norm() of the last assemble_residual, computed on device in the same pass
 private:
  poro_newton_record record{}; std::vector<double> rec_l2, rec_res, rec_bn;
  poro_ctx *ctx;
};
}  // namespace solvers

namespace projection {
template <int dim> class StrainProjector {
 public:
  poro_solver_opts control{0.0, 1e-8, 1000, PORO_PREC_JACOBI, 1.0, PORO_STOP_RHS, 0};       // StrainProjector.h:209, omega :212
  poro_solve_info  last{};
  StrainProjector() {}
  void set_solvers(poro_ctx *c) { ctx = c; }               // :73-79
  void setup_dofs() {}                                     // :82-98
  void assemble_projection_matrix() { poro_host::check(poro_proj_assemble_matrix(ctx), "proj_assemble_matrix"); }   // :101-106
  void assemble_projection_rhs(std::vector<int> tensor_components) {   // :109-198
    std::vector<int32_t> tc(tensor_components.begin(), tensor_components.end());
    poro_host::check(poro_proj_assemble_rhs(ctx, tc.data(), (int32_t)tc.size()), "proj_assemble_rhs");
  }
  void solve_projection_systems(const std::vector<int32_t> &rhs_entries, std::vector<poro_solve_info> &infos) {
    infos.assign(rhs_entries.size(), poro_solve_info{});
    const int rc = poro_proj_solve_many(ctx, rhs_entries.data(), (int32_t)rhs_entries.size(), &control, infos.data());
    poro_host::check(rc, "proj_solve_many");
    if (!infos.empty()) last = infos.back();
    if (rc > 0) throw poro_host::NoConvergence("StrainProjector::solve_projection_systems", last.iterations, last.final_residual);
  }
  void solve_projection_system(int rhs_entry) {            // :201-232
    const int rc = poro_proj_solve(ctx, rhs_entry, &control, &last);
    poro_host::check(rc, "proj_solve");
    if (rc > 0) throw poro_host::NoConvergence("StrainProjector::solve_projection_system", last.iterations, last.final_residual);
  }
 private:
  poro_ctx *ctx = nullptr;
};
}  // namespace projection

namespace indexing {
// TensorIndexer.h:6-52
template <int dim> class TensorIndexer {
 public:
  int entryIndex(int tensor_index) const {
    static const int m2[4] = {0, 1, 1, 2}, m3[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    return dim == 2 ? m2[tensor_index] : m3[tensor_index];
  }
};
}  // namespace indexing

namespace poro_host {

// PoroElasticProblem<dim> (PoroelasticityFSS.h:42-90): owns the context and reproduces run()'s call sequence
// (:294-415) with mesh creation left to the caller.  Mesh adaptation (:333-340, refine_mesh :447-498) is there for the mesh class the host provider
// can rebuild - boxes with ONE level of refinement (mask- or block-refined, the analogue of `Max refinement level = 1`), one rank: estimate on the device,
// mark and rebuild on the host, new context, transfer on the device.  Off unless RunControls::refine_every is set or refine_mesh is called.
template <int dim> class PoroElasticProblem {
  poro_ctx *ctx;   // declared first: the solver members below are constructed from it
 public:
  PoroElasticProblem(ProblemData &P, int device, int operator_mode) : ctx(make_ctx(P, device, operator_mode)), pressure_solver(ctx), displacement_solver(ctx), pd(&P), device_(device), operator_mode_(operator_mode) {
    volumetric_strain.ctx = initial_volumetric_strain.ctx = ctx;
    volumetric_strain.id = PORO_VEC_EPSV; initial_volumetric_strain.id = PORO_VEC_EPSV0;
    if (dim == 2) { strain_tensor_volumetric_components = {0, 3}; strain_tensor_shear_components = {1}; }
    else { strain_tensor_volumetric_components = {0, 4, 8}; strain_tensor_shear_components = {1, 2, 5}; }   // :104-111
  }
  ~PoroElasticProblem() { if (ctx) poro_ctx_destroy(ctx); }
  poro_ctx *context() { return ctx; }
  poro_ctx *release() { poro_ctx *c = ctx; ctx = nullptr; return c; }
  const ProblemData *problem() const { return pd; }                    // the mesh the context currently belongs to (the caller's, or the last one refine_mesh built)
  ProblemData *release_problem() { return adapted.release(); }        // the mesh refine_mesh built last, handed to the caller (null: never refined)

  // refine_mesh (:447-498) on one-level refined boxes, followed by the two calls of :338-339.  Sequence: estimate (KellyErrorEstimator on the device) -> mark
  // (fixed fraction + level limits, mesh.hpp) -> the new ProblemData from the mask -> a new context in the same operator mode, scatter mode, FDM precision and operator form ->
  // setup_dofs -> transfer of p, eps_v, eps_v0 on the device -> swap, the old context is destroyed.  The preconditioner choice of initialize() is made again on the
  // new context (rc.preconditioner < 0 lands on the two-level form once hanging nodes exist; with a per-cell k / mu the pressure system takes Jacobi there: the library
  // refuses the two-level form of the pressure system while a field is set).  Work counters carry over; the displacement warm start is lost (every
  // reinit of the reference leaves zero vectors).  Returns the cell counts before and after.
  std::pair<int64_t, int64_t> refine_mesh(const RunControls &rc) {
    const ProblemData &O = *pd;
    if (!O.refined_box) throw std::runtime_error("refine_mesh: the problem is not a mask- or block-refined box (the host provider adapts boxes with one level of refinement)");
    if (O.part.n_ranks > 1) throw std::runtime_error("refine_mesh: implemented for one rank");
    std::vector<double> eta((size_t)O.d.n_cells);
    check(poro_pres_estimate_error(ctx, PORO_VEC_P, eta.data()), "pres_estimate_error");     // :452-458
    std::vector<uint8_t> mask;
    mark_fixed_fraction(O, eta.data(), rc.refine_fraction, rc.coarsen_fraction, mask);       // :460-472
    std::unique_ptr<ProblemData> N(new ProblemData());
    N->bc = O.bc; N->mat = O.mat;
    build_refined_box_problem_mask(*N, O.mesh.dim, O.box_n, O.box_size, O.box_k_u, mask);    // :481-483
    N->inherit_cell_moduli(O);                                                               // lambda, G (poro_ctx_set_cell_moduli); make_ctx below hands the fields to the new context
    N->permeability.inherit(*N, O, O.permeability, "inherit_cell_permeability");             // a child takes its parent's k / mu, or its parent's diag(kx, ky, kz) / mu component by component
    N->inherit_cell_density(O);                                                              // the bulk density likewise, with g and the two scalar densities (poro_ctx_set_gravity)
    std::vector<int64_t> ptr; std::vector<int32_t> node; std::vector<double> weight;
    transfer_rows_p(O, *N, ptr, node, weight);
    int32_t scatter = PORO_SCATTER_COLOURED, fdm_req = PORO_FDM_FP64;
    check(poro_ctx_get_scatter_mode(ctx, &scatter), "ctx_get_scatter_mode");
    if (rc.fdm_fp32) fdm_req = PORO_FDM_FP32;
    struct Guard { poro_ctx *c; ~Guard() { if (c) poro_ctx_destroy(c); } } fresh{make_ctx(*N, device_, operator_mode_)};
    if (scatter != PORO_SCATTER_COLOURED || rc.atomic_scatter) check(poro_ctx_set_scatter_mode(fresh.c, rc.atomic_scatter ? PORO_SCATTER_ATOMIC : scatter), "ctx_set_scatter_mode");
    if (fdm_req != PORO_FDM_FP64) check(poro_ctx_set_fdm_precision(fresh.c, fdm_req), "ctx_set_fdm_precision");
    if (rc.fdm_per_direction) check(poro_ctx_set_fdm_form(fresh.c, PORO_FDM_FORM_PER_DIRECTION), "ctx_set_fdm_form");      // (next to the FDM precision: the new context takes the requested form of the block FDM)
    if (rc.moduli_structured) check(poro_ctx_set_moduli_operator(fresh.c, PORO_MODULI_OP_STRUCTURED), "ctx_set_moduli_operator");      // (recorded; a refined mesh has no box tag and keeps the cell loop)
    int32_t form = PORO_OPFORM_GENERAL;
    check(poro_ctx_get_operator_form(ctx, &form, nullptr, nullptr), "ctx_get_operator_form");
    if (form != PORO_OPFORM_GENERAL || rc.hybrid_operator) check(poro_ctx_set_operator_form(fresh.c, rc.hybrid_operator ? PORO_OPFORM_HYBRID : form), "ctx_set_operator_form");
    poro_ctx *old = ctx;
    const std::pair<int64_t, int64_t> counts(O.d.n_cells, N->d.n_cells);
    rebind(fresh.c);
    try {
      setup_dofs();                                                                          // :485
      check(poro_state_transfer_p(old, ctx, ptr.data(), node.data(), weight.data()), "state_transfer_p");   // :488-497
      check(poro_pres_apply_boundary_values(ctx), "pres_apply_boundary_values");
    } catch (...) { rebind(old); throw; }
    fresh.c = nullptr;
    poro_ctx_destroy(old);
    adapted = std::move(N); pd = adapted.get();                                              // (the previous adapted mesh, if any, goes with its context)
    choose_preconditioners(rc);
    first_assembly = true; jacobian_dt = -1;
    assemble_displacement();                                                                 // :338
    strain_projector.assemble_projection_matrix();                                           // :339
    return counts;
  }

  void setup_dofs() {                                      // :131-151
    pressure_solver.setup_dofs(); displacement_solver.setup_dofs();
    strain_projector.set_solvers(ctx); strain_projector.setup_dofs();
    // every reinit() of the reference's setup_dofs leaves a zero vector (PoroElasticDisplacementSolver.h:150-151,
    // PoroElasticPressureSolver.h:103-108, StrainProjector.h:93-96, PoroelasticityFSS.h:145-146)
    const int n_sym = dim * (dim + 1) / 2;
    for (int id : {PORO_VEC_U, PORO_VEC_RHS_U, PORO_VEC_P, PORO_VEC_P_OLD, PORO_VEC_DP, PORO_VEC_RESIDUAL_P, PORO_VEC_EPSV, PORO_VEC_EPSV0})
      check(poro_vec_fill(ctx, id, 0.0), "vec_fill");
    for (int e = 0; e < n_sym; ++e) { check(poro_vec_fill(ctx, PORO_VEC_STRAIN0 + e, 0.0), "vec_fill"); check(poro_vec_fill(ctx, PORO_VEC_PROJ_RHS0 + e, 0.0), "vec_fill"); }
  }
  void get_normal_strain_components() {                    // :153-164
    strain_projector.assemble_projection_rhs(strain_tensor_volumetric_components);
    // the loop of :157-163 over the volumetric components in one library call (solved together where the library can, entry by entry otherwise)
    std::vector<int32_t> entries; for (const auto &comp : strain_tensor_volumetric_components) entries.push_back(tensor_indexer.entryIndex(comp));
    std::vector<poro_solve_info> infos(entries.size());
    strain_projector.solve_projection_systems(entries, infos);
    for (const auto &li : infos) { work.cg_proj += li.iterations; work.apply_p += li.operator_applications; }
  }
  void get_volumetric_strain() { check(poro_get_volumetric_strain(ctx), "get_volumetric_strain"); }   // :179-186
  // :167-176.  The reference never assembles the shear right-hand sides (assemble_projection_rhs is only called with the volumetric
  // components, :157), so these solves see rhs = 0 and return eps_ij = 0; `corrected` assembles them first.
  void get_shear_strain_components(bool corrected = false) {
    if (corrected) strain_projector.assemble_projection_rhs(strain_tensor_shear_components);
    for (const auto &comp : strain_tensor_shear_components) strain_projector.solve_projection_system(tensor_indexer.entryIndex(comp));
  }
  void get_effective_stresses() { check(poro_get_effective_stresses(ctx), "get_effective_stresses"); }   // :189-224
  // :227-291: legacy-VTK file of u, p, strains and stresses, one patch per cell with its 2^dim vertices (build_patches(min degree) = 1
  // subdivision), fields in the reference's order.  2D quirk: the reference writes stresses[0] under the name "sigma_yy" (:257-258).
  void output_results(unsigned int step, const std::string &dir, bool corrected = false, bool darcy = false, bool stress = false) {
    const ProblemData &P = *pd; const int nv = 1 << dim, k = P.d.degree_u, n1 = k + 1, ns = P.d.fe.ns_u;
    const int64_t nc = P.d.n_cells, npts = nc * nv;
    std::vector<double> u, p; displacement_solver.solution.get(u, P.d.n_dofs_u); pressure_solver.solution.get(p, P.d.n_dofs_p);
    const int n_sym = dim * (dim + 1) / 2;
    std::vector<std::vector<double>> eps(n_sym), sig(n_sym);
    for (int e = 0; e < n_sym; ++e) { eps[e].resize(P.d.n_dofs_p); sig[e].resize(P.d.n_dofs_p);
      check(poro_vec_get(ctx, PORO_VEC_STRAIN0 + e, eps[e].data(), P.d.n_dofs_p), "vec_get"); check(poro_vec_get(ctx, PORO_VEC_STRESS0 + e, sig[e].data(), P.d.n_dofs_p), "vec_get"); }
    char name[64]; std::snprintf(name, sizeof name, "/solution-%04u", step);
    std::string file = dir + name + (P.part.n_ranks > 1 ? ".r" + std::to_string(P.part.rank) : std::string()) + ".vtk";
    std::ofstream out(file);
    if (!out) throw std::runtime_error("cannot write " + file);
    out.precision(12);
    out << "# vtk DataFile Version 3.0\n#This file was generated by poroelasticity_dealii_amd (layout of deal.II DataOut::write_vtk)\nASCII\nDATASET UNSTRUCTURED_GRID\n\n";
    out << "POINTS " << npts << " double\n";
    for (int64_t c = 0; c < nc; ++c) for (int v = 0; v < nv; ++v) {
      const double *x = &P.mesh.vertices[(size_t)P.mesh.cells[c * nv + v] * dim];
      out << x[0] << ' ' << x[1] << ' ' << (dim == 3 ? x[2] : 0.0) << '\n';
    }
    static const int vtk2[4] = {0, 1, 3, 2}, vtk3[8] = {0, 1, 3, 2, 4, 5, 7, 6};   // lexicographic -> VTK quad / hexahedron order
    out << "\nCELLS " << nc << ' ' << nc * (nv + 1) << '\n';
    for (int64_t c = 0; c < nc; ++c) { out << nv; for (int v = 0; v < nv; ++v) out << '\t' << c * nv + (dim == 2 ? vtk2[v] : vtk3[v]); out << '\n'; }
    out << "\nCELL_TYPES " << nc << '\n';
    for (int64_t c = 0; c < nc; ++c) out << (dim == 2 ? 9 : 12) << (c + 1 < nc ? ' ' : '\n');
    out << "POINT_DATA " << npts << '\n' << "VECTORS u double\n";
    for (int64_t c = 0; c < nc; ++c) for (int v = 0; v < nv; ++v) {
      const int a = (v & 1) * k, b = ((v >> 1) & 1) * k, cc = (v >> 2) * k, sidx = a + n1 * (b + n1 * cc);
      double w[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) w[d] = u[P.dofs.cell_u[((size_t)c * ns + sidx) * dim + d]];
      out << w[0] << ' ' << w[1] << ' ' << w[2] << '\n';
    }
    auto scalar = [&](const char *nm, const std::vector<double> &f) {
      out << "SCALARS " << nm << " double 1\nLOOKUP_TABLE default\n";
      for (int64_t c = 0; c < nc; ++c) { for (int v = 0; v < nv; ++v) out << f[P.dofs.cell_p[c * nv + v]] << ' '; }
      out << '\n';
    };
    scalar("p", p); scalar("eps_xx", eps[0]); scalar("sigma_xx", sig[0]);
    if (dim == 2) {
      scalar("eps_xy", eps[1]); scalar("eps_yy", eps[2]); scalar("sigma_xy", sig[1]); scalar("sigma_yy", corrected ? sig[2] : sig[0]);
    } else {
      scalar("eps_xy", eps[1]); scalar("eps_xz", eps[2]); scalar("eps_yy", eps[3]); scalar("eps_yz", eps[4]); scalar("eps_zz", eps[5]);
      scalar("sigma_xy", sig[1]); scalar("sigma_xz", sig[2]); scalar("sigma_yy", sig[3]); scalar("sigma_yz", sig[4]); scalar("sigma_zz", sig[5]);
    }
    if (darcy) {                                           // (extension, only on request: the file is otherwise what it was) one Darcy velocity per cell
      const std::vector<double> q = darcy_velocity();
      out << "CELL_DATA " << nc << "\nVECTORS darcy_velocity double\n";
      for (int64_t c = 0; c < nc; ++c) out << q[c * dim] << ' ' << q[c * dim + 1] << ' ' << (dim == 3 ? q[c * dim + 2] : 0.0) << '\n';
    }
    if (stress) {                                          // (extension, only on request, after whatever `darcy` appends) the cell stresses and two failure measures
      const CellStress S = cell_stress();
      const CellMeasures M = cell_measures();
      if (!darcy) out << "CELL_DATA " << nc << '\n';
      static const int at2[3][3] = {{0, 1, -1}, {1, 2, -1}, {-1, -1, -1}}, at3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};   // packed index of entry (a, b)
      auto tensors = [&](const char *nm, const std::vector<double> &t) {
        out << "TENSORS " << nm << " double\n";
        for (int64_t c = 0; c < nc; ++c) { for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) { const int e = dim == 2 ? at2[a][b] : at3[a][b]; out << (e < 0 ? 0.0 : t[(size_t)c * n_sym + e]) << (b < 2 ? ' ' : '\n'); } } out << '\n'; }
      };
      tensors("effective_stress", S.effective); tensors("total_stress", S.total);
      auto cells = [&](const char *nm, int col) {
        out << "SCALARS " << nm << " double 1\nLOOKUP_TABLE default\n";
        for (int64_t c = 0; c < nc; ++c) out << M.values[(size_t)c * 6 + col] << ' ';
        out << '\n';
      };
      cells("mohr_coulomb", 5); cells("von_mises", 4);
    }
  }
  // the tail of the time loop body (:409-411)
  void postprocess(const RunControls &rc) {
    get_shear_strain_components(rc.corrected_postprocessing);
    get_effective_stresses();
    if (!rc.output_dir.empty()) output_results((unsigned)time_step_number, rc.output_dir, rc.corrected_postprocessing, flow_controls.darcy_output, stress_controls.stress_output);
  }

  // ---- flow post-processing (extension; definitions: include/poroel_hip.h) ----
  // The two switches, set by the command line (poro_run --flow-balance, --darcy-output) and by the Runner's methods.  They live here and not in RunControls, whose
  // member list is pinned together with poro_host_run_options (tests/run_options_check.cpp).  flow_balance: after every time step the terms of the discrete fluid
  // balance go into flow_history and, times dt, into flow_totals.  darcy_output: output_results appends CELL_DATA / VECTORS darcy_velocity.  Both off: nothing changes
  struct FlowControls { bool flow_balance = false, darcy_output = false; } flow_controls;
  // q_c = -kappa_c (grad p_h(x_c) - rho_f g) of the present pressure, [n_cells][dim]
  std::vector<double> darcy_velocity() {
    std::vector<double> q((size_t)pd->d.n_cells * dim);
    check(poro_pres_darcy_velocity(ctx, PORO_VEC_P, q.data()), "pres_darcy_velocity");
    return q;
  }
  // The terms of the discrete fluid balance of the present state, and per prescribed label (in the order of bc.pressure_labels, every label once) the conservative
  // outflow - the sum of C^T(-r) over the dofs the label prescribed, ProblemData::dirichlet_label_p - and the face-integrated discharge
  struct FlowBalance {
    poro_flow_balance_terms terms{};
    std::vector<int32_t> labels; std::vector<double> outflow_by_label, discharge_by_label;
    // what the identity leaves: storage + source + outflow = -free_row_sum up to rounding, and |free_row_sum| <= sqrt(n) residual_l2
    double imbalance() const { return terms.storage_rate_strain + terms.storage_rate_pressure + terms.source_sum + terms.outflow_prescribed; }
  };
  FlowBalance flow_balance(const RunControls &rc) {
    const ProblemData &P = *pd;
    FlowBalance B;
    for (int32_t l : P.bc.pressure_labels) if (std::find(B.labels.begin(), B.labels.end(), l) == B.labels.end()) B.labels.push_back(l);
    std::vector<double> per_dof((size_t)P.d.n_dirichlet_p);
    check(poro_pres_flow_balance(ctx, rc.time_step, &B.terms, per_dof.empty() ? nullptr : per_dof.data()), "pres_flow_balance");
    B.outflow_by_label.assign(B.labels.size(), 0.0); B.discharge_by_label.assign(B.labels.size(), 0.0);
    if (P.dirichlet_label_p.size() == per_dof.size())
      for (size_t i = 0; i < per_dof.size(); ++i)
        for (size_t k = 0; k < B.labels.size(); ++k) if (B.labels[k] == P.dirichlet_label_p[i]) B.outflow_by_label[k] += per_dof[i];
    if (!B.labels.empty()) check(poro_pres_boundary_discharge(ctx, PORO_VEC_P, nullptr, B.labels.data(), (int32_t)B.labels.size(), B.discharge_by_label.data()), "pres_boundary_discharge");
    return B;
  }
  // time integrals of the terms over the steps taken while flow_controls.flow_balance was set (dt * each term, per step): cumulative storage change, injected volume
  // (source), drained volume in total and per label.  Reset by initialize, carried across refine_mesh like the work counters
  struct FlowTotals {
    int steps = 0; double storage_strain = 0, storage_pressure = 0, source = 0, outflow = 0, free_rows = 0, bound = 0 /* sum of dt sqrt(n) residual_l2 */;
    std::vector<int32_t> labels; std::vector<double> outflow_by_label, discharge_by_label;
  } flow_totals;
  std::vector<FlowBalance> flow_history;                   // one entry per such step (the driver's log)

  // ---- mechanical post-processing (extension; definitions: include/poroel_hip.h) ----
  // The switches, set by the command line (poro_run --stress-output, --mohr-coulomb, --force-balance) and by the Runner's methods; here and not in RunControls for the
  // reason given at FlowControls.  stress_output: output_results appends the cell stresses and two failure measures.  mohr_coulomb: the criterion of cell_measures
  // (off: f = 0).  force_balance / failure_log: after every time step the force balance / the failure summary goes into force_history / failure_history.  All off:
  // nothing changes
  struct StressControls { bool stress_output = false, force_balance = false, failure_log = false, mohr_coulomb = false; double cohesion = 0, friction_angle = 0; } stress_controls;
  struct CellStress { std::vector<double> strain, effective, total; };       // [n_cells][n_sym] each
  CellStress cell_stress() {
    const size_t n = (size_t)pd->d.n_cells * (dim * (dim + 1) / 2);
    CellStress S; S.strain.resize(n); S.effective.resize(n); S.total.resize(n);
    check(poro_disp_cell_stress(ctx, PORO_VEC_U, PORO_VEC_P, S.strain.data(), S.effective.data(), S.total.data()), "disp_cell_stress");
    return S;
  }
  struct CellMeasures { std::vector<double> values; poro_failure_summary summary{}; };   // [n_cells][6]
  CellMeasures cell_measures() {
    CellMeasures M; M.values.resize((size_t)pd->d.n_cells * 6);
    const poro_mohr_coulomb mc{stress_controls.cohesion, stress_controls.friction_angle};
    check(poro_disp_cell_measures(ctx, PORO_VEC_U, -1, stress_controls.mohr_coulomb ? &mc : nullptr, M.values.data(), &M.summary), "disp_cell_measures");
    return M;
  }
  // The force balance of the present state and, per displacement condition (label, component) in the order of the conditions, every pair once, the reaction: the sum of
  // C^T r over the dofs the condition prescribed (ProblemData::dirichlet_label_u)
  struct ForceBalance {
    poro_force_balance_terms terms{};
    std::vector<int32_t> labels, components; std::vector<double> reaction_by_label;
    // what the identity leaves per component: reaction + traction + body + coupling = -free_row_sum up to rounding, and |free_row_sum| <= sqrt(n) residual_l2
    double imbalance(int k) const { return terms.reaction_sum[k] + terms.traction_sum[k] + terms.body_sum[k] + terms.coupling_sum[k]; }
  };
  ForceBalance force_balance() {
    const ProblemData &P = *pd;
    ForceBalance B;
    for (size_t i = 0; i < P.bc.dirichlet_labels.size(); ++i) {
      bool seen = false;
      for (size_t k = 0; k < B.labels.size(); ++k) seen = seen || (B.labels[k] == P.bc.dirichlet_labels[i] && B.components[k] == P.bc.dirichlet_components[i]);
      if (!seen) { B.labels.push_back(P.bc.dirichlet_labels[i]); B.components.push_back(P.bc.dirichlet_components[i]); }
    }
    std::vector<double> per_dof((size_t)P.d.n_dirichlet);
    check(poro_disp_force_balance(ctx, &B.terms, per_dof.empty() ? nullptr : per_dof.data()), "disp_force_balance");
    B.reaction_by_label.assign(B.labels.size(), 0.0);
    if (P.dirichlet_label_u.size() == 2 * per_dof.size())
      for (size_t i = 0; i < per_dof.size(); ++i)
        for (size_t k = 0; k < B.labels.size(); ++k) if (B.labels[k] == P.dirichlet_label_u[2 * i] && B.components[k] == P.dirichlet_label_u[2 * i + 1]) B.reaction_by_label[k] += per_dof[i];
    return B;
  }
  std::vector<ForceBalance> force_history;                 // one entry per step taken while stress_controls.force_balance was set; reset by initialize
  std::vector<poro_failure_summary> failure_history;       // likewise for stress_controls.failure_log

  // work counters of the metric "DoF-updates in assemble + SpMV" (SURVEY 8d): operator applications and assembly passes
  struct Work { int64_t apply_u = 0, apply_p = 0, asm_rhs_u = 0, asm_matrix_u = 0, residual_p = 0, jacobian_p = 0, proj_rhs = 0;
                int64_t cg_u = 0, cg_p = 0, cg_proj = 0; double seconds_solve_u = 0; } work;

  // the solver controls and the preconditioner choice from rc and from what the CURRENT context supports (initialize, and again after every refine_mesh)
  void choose_preconditioners(const RunControls &rc) {
    displacement_solver.control.abs_tol = rc.abs_tol_u; displacement_solver.control.rel_tol = rc.rel_tol_u; displacement_solver.control.stop_rule = rc.stop_rule_u;
    displacement_solver.control.max_iter = pressure_solver.control.max_iter = strain_projector.control.max_iter = rc.max_iter;
    // rc.preconditioner < 0: the strongest displacement preconditioner this mesh supports
    displacement_solver.control.preconditioner = rc.preconditioner >= 0 ? rc.preconditioner
        : poro_supports_preconditioner(context(), 0, PORO_PREC_FDM) ? PORO_PREC_FDM : poro_supports_preconditioner(context(), 0, PORO_PREC_TWO_LEVEL) ? PORO_PREC_TWO_LEVEL : PORO_PREC_CHEBYSHEV;
    if (displacement_solver.control.preconditioner == PORO_PREC_CHEBYSHEV) { displacement_solver.control.omega = rc.chebyshev_ratio; displacement_solver.control.poly_degree = rc.chebyshev_degree; }
    // the pressure Jacobian and the projection's mass matrix are asked separately: prescribed pressures take rows out of the former only, so the projection keeps the
    // fast diagonalisation (and its batched direct solve) whatever the prescribed set looks like
    const auto q1_choice = [&](int which_system) {
      return rc.preconditioner == PORO_PREC_SSOR ? (int)PORO_PREC_SSOR : rc.preconditioner_p >= 0 ? rc.preconditioner_p
          : poro_supports_preconditioner(context(), which_system, PORO_PREC_FDM) ? (int)PORO_PREC_FDM : (int)PORO_PREC_JACOBI;
    };
    pressure_solver.control.preconditioner = q1_choice(1);
    strain_projector.control.preconditioner = q1_choice(2);
    // the pressure Jacobian's stiffness part makes Jacobi-CG grow with 1/h: the two-level form where the mesh carries a coarse space.  (The projection's mass matrix
    // is well conditioned under Jacobi on any mesh: 12-15 iterations, fewer than the additive two-level form needs; below ~4k pressure dofs a CG iteration is
    // launch-bound and the two-level form's extra launches cost more than the iterations it saves - profiles/r03_refined_box_step.json.)
    // (the GLOBAL pressure dof count on the pieces of a partition: every rank makes the choice a single rank would make)
    const int64_t n_dofs_p = pd->n_dofs_p_global > 0 ? pd->n_dofs_p_global : pd->d.n_dofs_p;
    if (rc.preconditioner != PORO_PREC_SSOR && rc.preconditioner_p < 0 && pressure_solver.control.preconditioner == PORO_PREC_JACOBI && n_dofs_p >= 4096 && poro_supports_preconditioner(context(), 1, PORO_PREC_TWO_LEVEL))
      pressure_solver.control.preconditioner = PORO_PREC_TWO_LEVEL;
    pressure_newton_batched = pressure_solver.newton_loop_supported();      // fixed per context and preconditioner: asked once, here
  }
  // trace rows: [step, fss_iteration, pressure_iterations, inner pressure error, |p|_inf, error after displacement, u CG its, p CG its]
  void initialize(const RunControls &rc) {
    if (rc.atomic_scatter) check(poro_ctx_set_scatter_mode(context(), PORO_SCATTER_ATOMIC), "ctx_set_scatter_mode");
    if (rc.fdm_fp32) check(poro_ctx_set_fdm_precision(context(), PORO_FDM_FP32), "ctx_set_fdm_precision");
    if (rc.fdm_per_direction) check(poro_ctx_set_fdm_form(context(), PORO_FDM_FORM_PER_DIRECTION), "ctx_set_fdm_form");
    if (rc.moduli_structured) check(poro_ctx_set_moduli_operator(context(), PORO_MODULI_OP_STRUCTURED), "ctx_set_moduli_operator");
    if (rc.hybrid_operator) check(poro_ctx_set_operator_form(context(), PORO_OPFORM_HYBRID), "ctx_set_operator_form");
    choose_preconditioners(rc);
    setup_dofs();                                          // :308
    pressure_solver.solution = rc.p_init;                  // :311
    if (pd->hydrostatic_init && pd->has_gravity()) {       // (extension: gravity) p_init at the top, hydrostatic below
      if (pd->part.n_ranks > 1) throw std::runtime_error("initialize: hydrostatic_init is implemented for one rank");
      const std::vector<double> ph = pd->hydrostatic_pressure(rc.p_init);
      check(poro_vec_set(ctx, PORO_VEC_P, ph.data(), (int64_t)ph.size()), "vec_set");
    }
    check(poro_pres_apply_boundary_values(ctx), "pres_apply_boundary_values");   // (extension: prescribed pressures; no-op for the reference's problems)
    assemble_displacement();                               // :312
    solve_displacement();                                  // :313
    strain_projector.assemble_projection_matrix();         // :314
    normal_strains();                                      // :315
    get_volumetric_strain();                               // :316
    initial_volumetric_strain = volumetric_strain;         // :317
    time_step_number = 0;
    flow_totals = FlowTotals(); flow_history.clear(); force_history.clear(); failure_history.clear();
  }
  // one pass of the time loop body (:328-407); returns the number of trace rows written (= FSS iterations)
  int time_step(const RunControls &rc, double *trace, int max_rows) {
    int rows = 0;
    time_step_number++;                                    // :329
    if (rc.refine_every > 0 && time_step_number % rc.refine_every == 0) {                  // :333-340
      const std::pair<int64_t, int64_t> cells = refine_mesh(rc);
      if (on_adapt) on_adapt(time_step_number, cells.first, cells.second);
    }
    pressure_solver.old_solution = pressure_solver.solution;   // :342
    if (rc.incremental_strain && time_step_number > 1) initial_volumetric_strain = volumetric_strain;
    double pressure_error = rc.pressure_tol * 2; int fss_iteration = 0;   // :345-346
    while (fss_iteration < rc.max_fss_iterations && pressure_error > rc.fss_tol) {   // :347-348
      fss_iteration++;
      int pressure_iteration = 0, pcg = 0; double inner = 0;
      pressure_solver.solution_update = 0.0;               // :356
      // :358-380 and :387-389 in one call where the context can run the loop as gated batches: same numbers, one wait.  A failed check of a direct solve hands the
      // loop back at that iteration's solve (resume_at_solve), and the rest of it runs per call
      bool resume_at_solve = false, have_pinf = false; double pinf = 0;
      const bool batched = rc.max_pressure_iterations >= 1 && pressure_newton_batched;
      if (batched) {
        const poro_newton_record &N = pressure_solver.newton_loop(rc.time_step, rc.pressure_tol, rc.max_pressure_iterations, fss_iteration - 1);
        pressure_iteration = N.iterations; work.residual_p += N.iterations;      // :359-363
        pressure_error = inner = N.l2[N.iterations - 1];                         // :364
        work.apply_p += N.solves;                                                // :378 (direct solves: no CG iterations, one operator application each)
        if (N.solves > 0 && rc.time_step != jacobian_dt) { work.jacobian_p++; jacobian_dt = rc.time_step; }   // :377
        if (N.outcome == PORO_NEWTON_FALLBACK) resume_at_solve = true;
        else { pinf = N.pinf; have_pinf = true; }                                // :387-389
      }
      while (resume_at_solve || (!have_pinf && pressure_iteration < rc.max_pressure_iterations)) {   // :358 (have_pinf: the batches ran the loop to its end)
        if (!resume_at_solve) {
          pressure_iteration++;
          pressure_solver.update_volumetric_strain(volumetric_strain);   // :360
          pressure_solver.assemble_residual(rc.time_step, volumetric_strain, initial_volumetric_strain); work.residual_p++;   // :361-363
          pressure_error = pressure_solver.residual_l2;      // :364
          inner = pressure_error;
          if (pressure_error < rc.pressure_tol) break;       // :366-371
        }
        resume_at_solve = false;
        pressure_solver.assemble_jacobian(rc.time_step);                       // :377
        if (rc.time_step != jacobian_dt) { work.jacobian_p++; jacobian_dt = rc.time_step; }   // the library re-forms J only when dt changed
        pressure_solver.solve();                           // :378
        pcg += pressure_solver.last.iterations; work.cg_p += pressure_solver.last.iterations; work.apply_p += pressure_solver.last.operator_applications;
        pressure_solver.solution += pressure_solver.solution_update;   // :379
      }
      if (!have_pinf) pinf = pressure_solver.solution.linfty_norm();   // :387-389
      assemble_displacement();                             // :395
      solve_displacement();                                // :396
      normal_strains();                                    // :398  (get_volumetric_strain() stays commented out, :399)
      if (rc.coupled_fss) get_volumetric_strain();
      pressure_solver.assemble_residual(rc.time_step, volumetric_strain, initial_volumetric_strain); work.residual_p++;   // :402-404
      pressure_error = pressure_solver.residual_l2;        // :405
      if (rows < max_rows) { double *r = trace + 8 * rows++; r[0] = time_step_number; r[1] = fss_iteration; r[2] = pressure_iteration - 1; r[3] = inner; r[4] = pinf; r[5] = pressure_error; r[6] = displacement_solver.last.iterations; r[7] = pcg; }
    }
    if (flow_controls.flow_balance) account_flow(rc);
    if (stress_controls.force_balance) force_history.push_back(force_balance());
    if (stress_controls.failure_log) failure_history.push_back(cell_measures().summary);
    return rows;
  }
  // device-side snapshot / rollback of the whole solver state (retry or repeat a time step)
  void save_state() { check(poro_state_save(ctx), "state_save"); saved_step_number = time_step_number; }
  void restore_state() { check(poro_state_restore(ctx), "state_restore"); time_step_number = saved_step_number; }
  int run(const RunControls &rc, double *trace, int max_rows) {
    int rows = 0;
    if (rc.refine_every > 0 && !pd->refined_box) throw std::runtime_error("run: refine_every needs a mask- or block-refined box (the mesh class the host provider can adapt)");
    initialize(rc);
    if (rows < max_rows) { double *r = trace + 8 * rows++; for (int i = 0; i < 8; ++i) r[i] = 0; r[6] = displacement_solver.last.iterations; }
    for (int s = 1; s <= rc.n_steps; ++s) { rows += time_step(rc, trace + 8 * rows, max_rows - rows); if (!rc.output_dir.empty()) postprocess(rc); }   // :327, :409-411
    return rows;
  }

  std::function<void(int step, int64_t cells_before, int64_t cells_after)> on_adapt;   // called after every refine_mesh of time_step (the driver's log); unset: nothing
  solvers::PoroElasticPressureSolver<dim>     pressure_solver;     // :77
  solvers::PoroElasticDisplacementSolver<dim> displacement_solver; // :78
  projection::StrainProjector<dim>            strain_projector;    // :79
  indexing::TensorIndexer<dim>                tensor_indexer;      // :81
  DeviceVector volumetric_strain, initial_volumetric_strain;       // :83
  std::vector<int> strain_tensor_volumetric_components, strain_tensor_shear_components;   // :86-87

 private:
  void assemble_displacement() { const bool rebuild = first_assembly; displacement_solver.assemble_system(pressure_solver.solution); first_assembly = false; work.asm_rhs_u++; if (rebuild) work.asm_matrix_u++; }
  void solve_displacement() {
    displacement_solver.solve();
    work.cg_u += displacement_solver.last.iterations; work.apply_u += displacement_solver.last.operator_applications; work.seconds_solve_u += displacement_solver.last.seconds;
  }
  void normal_strains() {
    get_normal_strain_components(); work.proj_rhs++;
  }
  // the balance of the step just taken (the state the step's last residual saw) into flow_history and, times dt, into flow_totals
  void account_flow(const RunControls &rc) {
    const FlowBalance B = flow_balance(rc);
    FlowTotals &T = flow_totals; const double dt = rc.time_step;
    if (T.labels != B.labels) { T.labels = B.labels; T.outflow_by_label.assign(B.labels.size(), 0.0); T.discharge_by_label.assign(B.labels.size(), 0.0); }
    T.steps++; T.storage_strain += dt * B.terms.storage_rate_strain; T.storage_pressure += dt * B.terms.storage_rate_pressure; T.source += dt * B.terms.source_sum;
    T.outflow += dt * B.terms.outflow_prescribed; T.free_rows += dt * B.terms.free_row_sum; T.bound += dt * std::sqrt((double)pd->d.n_dofs_p) * B.terms.residual_l2;
    for (size_t k = 0; k < B.labels.size(); ++k) { T.outflow_by_label[k] += dt * B.outflow_by_label[k]; T.discharge_by_label[k] += dt * B.discharge_by_label[k]; }
    flow_history.push_back(B);
  }
  // the problem and its solver members move to another context (refine_mesh); the caller looks after the context left behind
  void rebind(poro_ctx *c) {
    ctx = c; pressure_solver.rebind(c); displacement_solver.rebind(c); strain_projector.set_solvers(c);
    volumetric_strain.ctx = initial_volumetric_strain.ctx = c;
  }
  bool pressure_newton_batched = false;   // the context runs the pressure Newton loop as gated batches (choose_preconditioners)
  bool first_assembly = true; int time_step_number = 0, saved_step_number = 0; double jacobian_dt = -1;
  const ProblemData *pd; int device_, operator_mode_;
  std::unique_ptr<ProblemData> adapted;   // the mesh the last refine_mesh built (the first mesh belongs to the caller)
  static poro_ctx *make_ctx(ProblemData &P, int device, int operator_mode) {
    poro_ctx *c = nullptr;
    check(poro_ctx_create(&P.d, device, operator_mode, &c), "poro_ctx_create");
    // the per-cell fields of the problem go to the context before anything is assembled from it
    const ProblemData::PerCellField &k = P.permeability, &m = P.moduli, &rho = P.density; const int64_t n = P.mesh.n_cells();
    const std::vector<double> tensor = k.ncomp() > 1 ? k.interleaved() : std::vector<double>();      // [cell][dim], x first
    const char *failed = k.ncomp() == 1 && poro_ctx_set_cell_permeability(c, k.comp[0].data(), n) != 0 ? "ctx_set_cell_permeability: "
                         : k.ncomp() > 1 && poro_ctx_set_cell_permeability_tensor(c, tensor.data(), n) != 0 ? "ctx_set_cell_permeability_tensor: "
                         : !m.empty() && poro_ctx_set_cell_moduli(c, m.comp[0].data(), m.comp[1].data(), n) != 0 ? "ctx_set_cell_moduli: "
                         : !rho.empty() && poro_ctx_set_cell_density(c, rho.comp[0].data(), n) != 0 ? "ctx_set_cell_density: "
                         : P.has_gravity() && poro_ctx_set_gravity(c, P.gravity, P.bulk_density, P.fluid_density) != 0 ? "ctx_set_gravity: " : nullptr;      // (after the permeability: the gravity flux is built once)
    if (failed) { const std::string why = poro_last_error(); poro_ctx_destroy(c); throw std::runtime_error(failed + why); }
    return c;
  }
};

}  // namespace poro_host

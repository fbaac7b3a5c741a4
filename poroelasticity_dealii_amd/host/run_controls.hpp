// Host-only: the options of a run.  RunControls is what the C++ driver (problem.hpp, runner.cpp) reads; poro_host_run_options is the same set as a plain-C struct, the
// form in which the options cross the C boundary of host_capi.cpp (mirrored field by field by RunOptions in __init__.py; tests/run_options_check.cpp prints its layout).
// to_run_controls is the one place that maps the second onto the first.  No project header but the PORO_* constants: compiles into stand-alone checks.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include "../../include/poroel_hip.h"

extern "C" {
// one member per option; the switches are 0 / 1
typedef struct poro_host_run_options {
  double p_init, time_step; int32_t n_steps;
  double fss_tol, pressure_tol; int32_t max_fss_iterations, max_pressure_iterations;
  double abs_tol_u, rel_tol_u; int32_t max_iter, preconditioner;
  int32_t stop_rule_u, preconditioner_p /* -1: automatic */;
  int32_t coupled_fss, incremental_strain, atomic_scatter, fdm_fp32, hybrid_operator, fdm_per_direction, moduli_structured;
  int32_t chebyshev_degree; double chebyshev_ratio;
  int32_t refine_every; double refine_fraction, coarsen_fraction;
} poro_host_run_options;
}

namespace poro_host {

struct RunControls {
  double p_init = 10e6, time_step = 60; int n_steps = 1;
  double fss_tol = 1e-8, pressure_tol = 1e-8; int max_fss_iterations = 50, max_pressure_iterations = 50;
  double abs_tol_u = 1e-12, rel_tol_u = 0.0; int max_iter = 1000;   // PoroElasticDisplacementSolver.h:298-299
  int stop_rule_u = PORO_STOP_RHS;                                  // PORO_STOP_REDUCTION: rel_tol_u is taken against the residual of the warm start (every step of a transient solves)
  int preconditioner = PORO_PREC_JACOBI;                            // displacement solve; PORO_PREC_SSOR = the reference's PreconditionSSOR (CSR operator, one rank) for all three systems
  bool coupled_fss = false;                                         // true = restore the get_volumetric_strain() call the reference commented out (:399): eps_v follows the new
                                                                    // displacement inside the fixed-stress loop, which then really iterates (SURVEY 8f-4 "corrected physics", first half)
  bool incremental_strain = false;                                  // true = storage term against the previous step, alpha (eps_v - eps_v^n) / dt, instead of the initial state eps_v0 (:317, :361-363)
  bool corrected_postprocessing = false;                            // false = the reference's output (shear RHS never assembled, 2D "sigma_yy" shows sigma_xx); true = both fixed
  std::string output_dir;                                           // "" = no files; the reference always writes ./solution/solution-NNNN.vtk (:285-290)
  int chebyshev_degree = 0; double chebyshev_ratio = 0.0;           // PORO_PREC_CHEBYSHEV: 0 = the library's defaults
  int preconditioner_p = -1;                                        // pressure / projection solves; -1 = fast diagonalisation where the context supports it, else the two-level form, else Jacobi
  bool fdm_fp32 = false;                                            // PORO_FDM_FP32: fp32 transforms in the displacement system's block FDM where it runs in the single-rank 3D octant form (elsewhere no effect).  Never chosen automatically
  bool fdm_per_direction = false;                                   // PORO_FDM_FORM_PER_DIRECTION: the block FDM's contiguous passes on single-rank 3D boxes whose directions are not all mirror-symmetric (elsewhere no effect).  Never chosen automatically
  bool moduli_structured = false;                                   // PORO_MODULI_OP_STRUCTURED: the structured operator on single-rank uniform 3D boxes with moduli layered along z, matrix-free (elsewhere no effect).  Never chosen automatically
  bool atomic_scatter = false;                                      // general meshes, matrix-free: PORO_SCATTER_ATOMIC (one launch per operator application; not bitwise reproducible).  Never chosen automatically
  bool hybrid_operator = false;                                     // refined boxes, matrix-free: PORO_OPFORM_HYBRID (structured kernel on the coarse box + general kernels on the fine cells); a no-op on box-tagged meshes, an error on meshes that cannot take it.  Never chosen automatically
  int refine_every = 0;                                             // refine_mesh when time_step_number % refine_every == 0 (the reference hard-wires 5, PoroelasticityFSS.h:333); 0 = never
  double refine_fraction = 0.6, coarsen_fraction = 0.4;             // refine_and_coarsen_fixed_fraction (:460-462)
};

// the options a default-constructed RunControls stands for
inline poro_host_run_options default_run_options() {
  const RunControls d;
  return {d.p_init, d.time_step, d.n_steps, d.fss_tol, d.pressure_tol, d.max_fss_iterations, d.max_pressure_iterations, d.abs_tol_u, d.rel_tol_u, d.max_iter, d.preconditioner,
          d.stop_rule_u, d.preconditioner_p, d.coupled_fss, d.incremental_strain, d.atomic_scatter, d.fdm_fp32, d.hybrid_operator, d.fdm_per_direction, d.moduli_structured,
          d.chebyshev_degree, d.chebyshev_ratio, d.refine_every, d.refine_fraction, d.coarsen_fraction};
}

// every value as given (no clipping, no rounding); output_dir and corrected_postprocessing do not cross the boundary and keep their defaults
inline RunControls to_run_controls(const poro_host_run_options &o) {
  if (o.refine_every < 0) throw std::runtime_error("run_adaptive: refine_every must be >= 0");
  RunControls rc;
  rc.p_init = o.p_init; rc.time_step = o.time_step; rc.n_steps = o.n_steps;
  rc.fss_tol = o.fss_tol; rc.pressure_tol = o.pressure_tol; rc.max_fss_iterations = o.max_fss_iterations; rc.max_pressure_iterations = o.max_pressure_iterations;
  rc.abs_tol_u = o.abs_tol_u; rc.rel_tol_u = o.rel_tol_u; rc.max_iter = o.max_iter; rc.preconditioner = o.preconditioner;
  rc.stop_rule_u = o.stop_rule_u; rc.preconditioner_p = o.preconditioner_p;
  rc.coupled_fss = o.coupled_fss != 0; rc.incremental_strain = o.incremental_strain != 0; rc.atomic_scatter = o.atomic_scatter != 0; rc.fdm_fp32 = o.fdm_fp32 != 0;
  rc.hybrid_operator = o.hybrid_operator != 0; rc.fdm_per_direction = o.fdm_per_direction != 0; rc.moduli_structured = o.moduli_structured != 0;
  rc.chebyshev_degree = o.chebyshev_degree; rc.chebyshev_ratio = o.chebyshev_ratio;
  rc.refine_every = o.refine_every; rc.refine_fraction = o.refine_fraction; rc.coarsen_fraction = o.coarsen_fraction;
  return rc;
}

}  // namespace poro_host

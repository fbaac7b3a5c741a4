"""ctypes front end of the MI355X-native fixed-stress Biot hot path.

Thin plumbing only: the product is the C-ABI library ``lib/libporoel_hip.so`` (hand-written HIP kernels,
``include/poroel_hip.h``) and the C++ host layer ``lib/libporoel_host.so`` (mesh / DoF / FE-table provider,
parameter-file front end, ``PoroElasticProblem<dim>::run()`` mirror).  There is no CPU fallback: creating a
context without a HIP device fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

# ids of include/poroel_hip.h
PREC_NONE, PREC_JACOBI, PREC_SSOR, PREC_FDM, PREC_ILU0, PREC_CHEBYSHEV, PREC_TWO_LEVEL = 0, 1, 2, 3, 4, 5, 6
STOP_RHS, STOP_REDUCTION = 0, 1
OP_CSR, OP_MATRIX_FREE = 0, 1
SCATTER_COLOURED, SCATTER_ATOMIC = 0, 1
OPFORM_GENERAL, OPFORM_HYBRID = 0, 1
FDM_FP64, FDM_FP32 = 0, 1
FDM_FORM_DEFAULT, FDM_FORM_PER_DIRECTION = 0, 1
MODULI_OP_CELLS, MODULI_OP_STRUCTURED = 0, 1
FDM_RUNS_NODAL, FDM_RUNS_OCTANT, FDM_RUNS_PER_DIRECTION, FDM_RUNS_SLAB, FDM_RUNS_PLANAR = 0, 1, 2, 3, 4
MAT_A_U, MAT_MASS_P, MAT_LAPLACE_P, MAT_JACOBIAN_P = 0, 1, 2, 3
VEC_U, VEC_RHS_U, VEC_P, VEC_P_OLD, VEC_DP, VEC_RESIDUAL_P, VEC_EPSV, VEC_EPSV0, VEC_SOURCE_P = range(9)
VEC_STRAIN0, VEC_PROJ_RHS0, VEC_DIAG_U, VEC_STRESS0 = 16, 32, 48, 64

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


class FeTables(C.Structure):
    _fields_ = [("nq_u", C.c_int32), ("nq_p", C.c_int32), ("nq_f", C.c_int32), ("ns_u", C.c_int32), ("ns_p", C.c_int32)] + [
        (n, _dp) for n in ("w_qu", "w_qp", "w_qf", "u_qu", "du_qu", "du_qp", "q1_qu", "dq1_qu", "q1_qp", "dq1_qp", "u_qf", "dq1_qf")]


class Material(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lame_lambda", "shear_G", "biot_alpha", "bulk_K", "biot_M", "k_over_mu", "r_well", "flow_rate")]


class Structured(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("n", C.c_int32 * 3), ("origin", C.c_double * 3), ("h", C.c_double * 3)]


class Partition(C.Structure):
    _fields_ = [("rank", C.c_int32), ("n_ranks", C.c_int32), ("has_lower", C.c_int32), ("has_upper", C.c_int32), ("plane_u", C.c_int64), ("plane_p", C.c_int64),
                ("n_neighbours", C.c_int32), ("neighbour_rank", _ip), ("shared_ptr_u", _lp), ("shared_dof_u", _ip), ("shared_ptr_p", _lp), ("shared_dof_p", _ip),
                ("n_owned_u", C.c_int64), ("n_owned_p", C.c_int64)]


class Constraints(C.Structure):
    _fields_ = [("n", C.c_int64), ("dof", _ip), ("ptr", C.POINTER(C.c_int64)), ("master", _ip), ("weight", _dp), ("inhomogeneity", _dp)]


class TensorGrid(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("n", C.c_int32 * 3), ("grid", _dp * 3)]


class CoarseSpace(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("box_problem", C.c_void_p), ("ptr", C.POINTER(C.c_int64)), ("node", _ip), ("weight", _dp),
                ("ptr_p", C.POINTER(C.c_int64)), ("node_p", _ip), ("weight_p", _dp)]


class Desc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("dim", C.c_int32), ("degree_u", C.c_int32), ("degree_p", C.c_int32),
                ("n_cells", C.c_int64), ("n_vertices", C.c_int64), ("n_dofs_u", C.c_int64), ("n_dofs_p", C.c_int64),
                ("vertex_coords", _dp), ("cell_vertices", _ip), ("cell_dofs_u", _ip), ("cell_dofs_p", _ip),
                ("fe", FeTables),
                ("n_bfaces", C.c_int64), ("bface_cell", _ip), ("bface_local", _ip), ("bface_id", _ip),
                ("n_dirichlet", C.c_int64), ("dirichlet_dof", _ip), ("dirichlet_value", _dp),
                ("n_neumann", C.c_int32), ("neumann_label", _ip), ("neumann_component", _ip), ("neumann_value", _dp),
                ("mat", Material), ("box", Structured), ("part", Partition), ("cons_u", Constraints), ("cons_p", Constraints),
                ("n_dirichlet_p", C.c_int64), ("dirichlet_dof_p", _ip), ("dirichlet_value_p", _dp), ("tensor", TensorGrid), ("coarse", CoarseSpace)]


class SolverOpts(C.Structure):
    _fields_ = [("abs_tol", C.c_double), ("rel_tol", C.c_double), ("max_iter", C.c_int32), ("preconditioner", C.c_int32), ("omega", C.c_double),
                ("stop_rule", C.c_int32), ("poly_degree", C.c_int32)]


class NewtonRecord(C.Structure):      # poro_newton_record
    _fields_ = [("iterations", C.c_int32), ("solves", C.c_int32), ("outcome", C.c_int32), ("batches", C.c_int32), ("pinf", C.c_double),
                ("l2", C.POINTER(C.c_double)), ("res", C.POINTER(C.c_double)), ("bn", C.POINTER(C.c_double))]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("initial_residual", C.c_double), ("final_residual", C.c_double),
                ("seconds", C.c_double), ("operator_applications", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FlowBalanceTerms(C.Structure):
    """poro_flow_balance_terms (include/poroel_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("storage_rate_strain", "storage_rate_pressure", "source_sum", "outflow_prescribed", "free_row_sum", "residual_l2")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MohrCoulomb(C.Structure):
    """poro_mohr_coulomb (include/poroel_hip.h): cohesion and friction angle in radians"""
    _fields_ = [("cohesion", C.c_double), ("friction_angle", C.c_double)]


class FailureSummary(C.Structure):
    """poro_failure_summary (include/poroel_hip.h)"""
    _fields_ = [("max_f", C.c_double), ("argmax_cell", C.c_int64), ("n_failing", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ForceBalanceTerms(C.Structure):
    """poro_force_balance_terms (include/poroel_hip.h)"""
    _fields_ = [(n, C.c_double * 3) for n in ("reaction_sum", "free_row_sum", "traction_sum", "body_sum", "coupling_sum")] + [("residual_l2", C.c_double)]


class RunOptions(C.Structure):
    """poro_host_run_options (host/run_controls.hpp), member by member; tests/test_run_options_cpu.py holds the two layouts against each other"""
    _fields_ = [("p_init", C.c_double), ("time_step", C.c_double), ("n_steps", C.c_int32), ("fss_tol", C.c_double), ("pressure_tol", C.c_double),
                ("max_fss_iterations", C.c_int32), ("max_pressure_iterations", C.c_int32), ("abs_tol_u", C.c_double), ("rel_tol_u", C.c_double), ("max_iter", C.c_int32),
                ("preconditioner", C.c_int32), ("stop_rule_u", C.c_int32), ("preconditioner_p", C.c_int32)] + [
        (n, C.c_int32) for n in ("coupled_fss", "incremental_strain", "atomic_scatter", "fdm_fp32", "hybrid_operator", "fdm_per_direction", "moduli_structured")] + [
        ("chebyshev_degree", C.c_int32), ("chebyshev_ratio", C.c_double), ("refine_every", C.c_int32), ("refine_fraction", C.c_double), ("coarsen_fraction", C.c_double)]


class InputFlat(C.Structure):
    _fields_ = [("dim", C.c_int32), ("domain_size", C.c_double * 3), ("initial_refinement_level", C.c_int32), ("max_refinement_level", C.c_int32)] + [
        (n, C.c_double) for n in ("youngs_modulus", "poisson_ratio", "biot_coef", "perm", "poro", "visc", "bulk_density", "f_comp", "r_well", "flow_rate",
                                  "p_init", "time_step", "t_max", "fss_tol", "pressure_tol")] + [
        ("max_fss_iterations", C.c_int32), ("max_pressure_iterations", C.c_int32),
        ("n_dirichlet", C.c_int32), ("dirichlet_labels", C.c_int32 * 16), ("dirichlet_components", C.c_int32 * 16), ("dirichlet_values", C.c_double * 16),
        ("n_neumann", C.c_int32), ("neumann_labels", C.c_int32 * 16), ("neumann_components", C.c_int32 * 16), ("neumann_values", C.c_double * 16)] + [
        (n, C.c_double) for n in ("lame_constant", "shear_modulus", "bulk_modulus", "grain_bulk_modulus", "n_modulus", "m_modulus")] + [("material", Material)]


ALLREDUCE_FN = C.CFUNCTYPE(None, _dp, C.c_int32, C.c_void_p)
SENDRECV_FN = C.CFUNCTYPE(None, _dp, _dp, C.c_int64, C.c_int32, C.c_void_p)

# every symbol include/poroel_hip.h declares (checked by the CPU test-suite against the built library)
HIP_SYMBOLS = [
    "poro_last_error", "poro_abi_version", "poro_ctx_create", "poro_ctx_destroy", "poro_ctx_synchronize", "poro_ctx_set_scatter_mode", "poro_ctx_get_scatter_mode", "poro_ctx_set_operator_form", "poro_ctx_get_operator_form", "poro_ctx_set_fdm_precision", "poro_ctx_get_fdm_precision", "poro_comm_unique_id", "poro_ctx_comm_init_rccl",
    "poro_ctx_comm_init_callbacks", "poro_vec_set", "poro_vec_get", "poro_vec_fill", "poro_vec_copy", "poro_vec_axpy", "poro_vec_norm",
    "poro_state_save", "poro_state_restore", "poro_disp_assemble_system", "poro_disp_solve", "poro_supports_preconditioner", "poro_pres_assemble_residual", "poro_pres_apply_boundary_values", "poro_pres_assemble_jacobian", "poro_pres_solve",
    "poro_pres_update_volumetric_strain", "poro_supports_pres_newton_loop", "poro_pres_newton_loop", "poro_proj_assemble_matrix", "poro_proj_assemble_rhs", "poro_proj_solve", "poro_proj_solve_many", "poro_get_volumetric_strain", "poro_get_effective_stresses",
    "poro_pres_estimate_error", "poro_state_transfer_p",
    "poro_export_csr_size", "poro_export_csr", "poro_apply_operator", "poro_apply_preconditioner_u", "poro_bench_operator", "poro_timers_reset", "poro_timers_enable", "poro_timers_get",
    "poro_ctx_set_fdm_form", "poro_ctx_get_fdm_form",
    "poro_ctx_set_cell_permeability", "poro_ctx_get_cell_permeability", "poro_pres_apply_jacobian",
    "poro_ctx_set_cell_permeability_tensor", "poro_ctx_get_cell_permeability_tensor",
    "poro_ctx_set_cell_moduli", "poro_ctx_get_cell_moduli",
    "poro_ctx_set_moduli_operator", "poro_ctx_get_moduli_operator",
    "poro_ctx_set_gravity", "poro_ctx_get_gravity", "poro_ctx_set_cell_density", "poro_ctx_get_cell_density", "poro_get_gravity_vectors",
    "poro_pres_darcy_velocity", "poro_pres_boundary_discharge", "poro_pres_flow_balance",
    "poro_disp_cell_stress", "poro_disp_cell_measures", "poro_disp_force_balance"]

_hip = None
_host = None


def _need(path):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no fallback path")
    return path


def load_hip():
    """The C-ABI library (HIP kernels).  Loads without a GPU; compute calls need one."""
    global _hip
    if _hip is None:
        L = C.CDLL(_need(os.path.join(LIB_DIR, "libporoel_hip.so")), mode=C.RTLD_GLOBAL)
        L.poro_last_error.restype = C.c_char_p
        L.poro_ctx_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.poro_ctx_destroy.argtypes = [C.c_void_p]
        L.poro_ctx_destroy.restype = None
        L.poro_ctx_synchronize.argtypes = [C.c_void_p]
        L.poro_ctx_set_scatter_mode.argtypes = [C.c_void_p, C.c_int32]
        L.poro_ctx_get_scatter_mode.argtypes = [C.c_void_p, _ip]
        L.poro_ctx_set_operator_form.argtypes = [C.c_void_p, C.c_int32]
        L.poro_ctx_get_operator_form.argtypes = [C.c_void_p, _ip, _lp, _lp]
        L.poro_ctx_set_fdm_precision.argtypes = [C.c_void_p, C.c_int32]
        L.poro_ctx_get_fdm_precision.argtypes = [C.c_void_p, _ip, _ip]
        L.poro_ctx_set_fdm_form.argtypes = [C.c_void_p, C.c_int32]
        L.poro_ctx_get_fdm_form.argtypes = [C.c_void_p, _ip, _ip, _ip]
        L.poro_ctx_set_moduli_operator.argtypes = [C.c_void_p, C.c_int32]
        L.poro_ctx_get_moduli_operator.argtypes = [C.c_void_p, _ip, _ip]
        L.poro_comm_unique_id.argtypes = [C.c_void_p]
        L.poro_ctx_comm_init_rccl.argtypes = [C.c_void_p, C.c_void_p]
        L.poro_ctx_comm_init_callbacks.argtypes = [C.c_void_p, ALLREDUCE_FN, SENDRECV_FN, C.c_void_p]
        L.poro_vec_set.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64]
        L.poro_vec_get.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64]
        L.poro_vec_fill.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.poro_vec_copy.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.poro_vec_axpy.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int]
        L.poro_vec_norm.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.poro_disp_assemble_system.argtypes = [C.c_void_p, C.c_int]
        L.poro_state_save.argtypes = [C.c_void_p]
        L.poro_state_restore.argtypes = [C.c_void_p]
        L.poro_disp_solve.argtypes = [C.c_void_p, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]
        L.poro_supports_preconditioner.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.poro_pres_assemble_residual.argtypes = [C.c_void_p, C.c_double, _dp]
        L.poro_pres_assemble_jacobian.argtypes = [C.c_void_p, C.c_double]
        L.poro_pres_apply_boundary_values.argtypes = [C.c_void_p]
        L.poro_pres_solve.argtypes = [C.c_void_p, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]
        L.poro_pres_update_volumetric_strain.argtypes = [C.c_void_p]
        L.poro_supports_pres_newton_loop.argtypes = [C.c_void_p, C.c_void_p]
        L.poro_pres_newton_loop.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.poro_proj_assemble_matrix.argtypes = [C.c_void_p]
        L.poro_proj_assemble_rhs.argtypes = [C.c_void_p, _ip, C.c_int32]
        L.poro_proj_solve.argtypes = [C.c_void_p, C.c_int32, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]
        L.poro_proj_solve_many.argtypes = [C.c_void_p, _ip, C.c_int32, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]
        L.poro_get_volumetric_strain.argtypes = [C.c_void_p]
        L.poro_get_effective_stresses.argtypes = [C.c_void_p]
        L.poro_pres_estimate_error.argtypes = [C.c_void_p, C.c_int, _dp]
        L.poro_state_transfer_p.argtypes = [C.c_void_p, C.c_void_p, _lp, _ip, _dp]
        L.poro_export_csr_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.poro_export_csr.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), _ip, _dp]
        L.poro_apply_operator.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.poro_bench_operator.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
        L.poro_apply_preconditioner_u.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, C.c_int32, _dp]
        L.poro_timers_reset.argtypes = [C.c_void_p]
        L.poro_timers_enable.argtypes = [C.c_void_p, C.c_int]
        L.poro_timers_get.argtypes = [C.c_void_p, C.c_char_p, _dp, C.POINTER(C.c_int64)]
        L.poro_ctx_set_cell_permeability.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.poro_ctx_get_cell_permeability.argtypes = [C.c_void_p, _dp, C.c_int64, _ip]
        L.poro_ctx_set_cell_permeability_tensor.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.poro_ctx_get_cell_permeability_tensor.argtypes = [C.c_void_p, _dp, C.c_int64, _ip]
        L.poro_pres_apply_jacobian.argtypes = [C.c_void_p, _dp, _dp]
        L.poro_ctx_set_cell_moduli.argtypes = [C.c_void_p, _dp, _dp, C.c_int64]
        L.poro_ctx_get_cell_moduli.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, _ip]
        L.poro_ctx_set_gravity.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double]
        L.poro_ctx_get_gravity.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
        L.poro_ctx_set_cell_density.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.poro_ctx_get_cell_density.argtypes = [C.c_void_p, _dp, C.c_int64, _ip]
        L.poro_get_gravity_vectors.argtypes = [C.c_void_p, _dp, _dp]
        L.poro_pres_darcy_velocity.argtypes = [C.c_void_p, C.c_int, _dp]
        L.poro_pres_boundary_discharge.argtypes = [C.c_void_p, C.c_int, _dp, _ip, C.c_int32, _dp]
        L.poro_pres_flow_balance.argtypes = [C.c_void_p, C.c_double, C.POINTER(FlowBalanceTerms), _dp]
        L.poro_disp_cell_stress.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
        L.poro_disp_cell_measures.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MohrCoulomb), _dp, C.POINTER(FailureSummary)]
        L.poro_disp_force_balance.argtypes = [C.c_void_p, C.POINTER(ForceBalanceTerms), _dp]
        _hip = L
    return _hip


def load_host():
    """The C++ host layer (mesh / DoFs / FE tables / parameter file / run() driver)."""
    global _host
    if _host is None:
        load_hip()
        L = C.CDLL(_need(os.path.join(LIB_DIR, "libporoel_host.so")))
        L.poro_host_last_error.restype = C.c_char_p
        bc = [C.c_int, _ip, _ip, _dp, C.c_int, _ip, _ip, _dp, C.POINTER(Material)]
        L.poro_host_build_graded_box.restype = C.c_void_p
        L.poro_host_build_graded_box.argtypes = [C.c_int, _ip, _dp, C.c_int, _dp] + bc
        L.poro_host_build_box.restype = C.c_void_p
        L.poro_host_build_box.argtypes = [C.c_int, _ip, _dp, C.c_int, C.c_int, C.c_int] + bc
        L.poro_host_build_refined_box.restype = C.c_void_p
        L.poro_host_build_refined_box.argtypes = [C.c_int, _ip, _dp, C.c_int, _ip, _ip] + bc
        L.poro_host_build_refined_box_mask.restype = C.c_void_p
        L.poro_host_build_refined_box_mask.argtypes = [C.c_int, _ip, _dp, C.c_int, _ip] + bc
        L.poro_host_refine_mask.restype = C.c_int64
        L.poro_host_refine_mask.argtypes = [C.c_void_p, _ip]
        L.poro_host_cell_parents.restype = C.c_int64
        L.poro_host_cell_parents.argtypes = [C.c_void_p, _ip, _ip]
        L.poro_host_mark_fixed_fraction.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, _ip]
        L.poro_host_transfer_rows_p.restype = C.c_int64
        L.poro_host_transfer_rows_p.argtypes = [C.c_void_p, C.c_void_p, _lp, _ip, _dp]
        L.poro_host_run_adaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RunOptions), _dp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.poro_host_runner_adapt.argtypes = [C.c_void_p, C.c_double, C.c_double, _lp]
        L.poro_host_runner_problem.restype = C.c_void_p
        L.poro_host_runner_problem.argtypes = [C.c_void_p]
        L.poro_host_kelly_tables.restype = C.c_int64
        L.poro_host_kelly_tables.argtypes = [C.c_void_p, _lp, _ip, _ip, _ip, _lp, _ip, _ip]
        L.poro_host_build_gmsh.restype = C.c_void_p
        L.poro_host_build_gmsh.argtypes = [C.c_char_p, C.c_int] + bc
        L.poro_host_build_gmsh_refined.restype = C.c_void_p
        L.poro_host_build_gmsh_refined.argtypes = [C.c_char_p, C.c_int, C.c_int] + bc
        L.poro_host_set_pressure_bc.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.poro_host_tie_boundary.argtypes = [C.c_void_p, C.c_int, _ip, _ip]
        L.poro_host_set_cell_permeability.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.poro_host_set_permeability_layers.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.poro_host_inherit_cell_permeability.argtypes = [C.c_void_p, C.c_void_p]
        L.poro_host_get_cell_permeability.restype = C.c_int64
        L.poro_host_get_cell_permeability.argtypes = [C.c_void_p, _dp]
        L.poro_host_set_cell_permeability_tensor.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.poro_host_set_permeability_tensor_layers.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        L.poro_host_inherit_cell_permeability_tensor.argtypes = [C.c_void_p, C.c_void_p]
        L.poro_host_get_cell_permeability_tensor.restype = C.c_int64
        L.poro_host_get_cell_permeability_tensor.argtypes = [C.c_void_p, _dp]
        L.poro_host_set_cell_moduli.argtypes = [C.c_void_p, _dp, _dp, C.c_int64]
        L.poro_host_set_moduli_layers.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        L.poro_host_inherit_cell_moduli.argtypes = [C.c_void_p, C.c_void_p]
        L.poro_host_get_cell_moduli.restype = C.c_int64
        L.poro_host_get_cell_moduli.argtypes = [C.c_void_p, _dp, _dp]
        L.poro_host_set_gravity.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, C.c_int]
        L.poro_host_get_gravity.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
        L.poro_host_set_cell_density.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.poro_host_set_density_layers.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.poro_host_inherit_cell_density.argtypes = [C.c_void_p, C.c_void_p]
        L.poro_host_get_cell_density.restype = C.c_int64
        L.poro_host_get_cell_density.argtypes = [C.c_void_p, _dp]
        L.poro_host_partition.restype = C.c_void_p
        L.poro_host_partition.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.poro_host_partition_ex.restype = C.c_void_p
        L.poro_host_partition_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.poro_host_local_to_global.restype = C.c_int64
        L.poro_host_local_to_global.argtypes = [C.c_void_p, C.c_int, _ip]
        L.poro_host_desc.restype = C.POINTER(Desc)
        L.poro_host_desc.argtypes = [C.c_void_p]
        L.poro_host_free.argtypes = [C.c_void_p]
        L.poro_host_free.restype = None
        L.poro_host_read_input.argtypes = [C.c_char_p, C.POINTER(InputFlat)]
        L.poro_host_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RunOptions), _dp, C.c_int, C.POINTER(C.c_void_p)]
        L.poro_host_runner_create.restype = C.c_void_p
        L.poro_host_runner_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RunOptions)]
        L.poro_host_runner_ctx.restype = C.c_void_p
        L.poro_host_runner_ctx.argtypes = [C.c_void_p]
        L.poro_host_runner_initialize.argtypes = [C.c_void_p]
        L.poro_host_runner_step.argtypes = [C.c_void_p, _dp, C.c_int, C.POINTER(C.c_int64)]
        L.poro_host_runner_restore_and_step.argtypes = [C.c_void_p, _dp, C.c_int, C.POINTER(C.c_int64)]
        L.poro_host_runner_work.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.poro_host_runner_work.restype = None
        L.poro_host_runner_postprocess.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.poro_host_runner_state.argtypes = [C.c_void_p, C.c_int]
        L.poro_host_runner_postprocess_darcy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        L.poro_host_runner_track_flow.argtypes = [C.c_void_p, C.c_int]
        L.poro_host_runner_postprocess_fields.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        L.poro_host_runner_mohr_coulomb.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
        L.poro_host_runner_track_force.argtypes = [C.c_void_p, C.c_int]
        L.poro_host_runner_force_history.argtypes = [C.c_void_p, C.c_int, _dp]
        L.poro_host_runner_flow_balance.argtypes = [C.c_void_p, _dp, _ip, _dp, _dp, C.c_int, _dp, _dp, _dp]
        L.poro_host_pressure_bc_labels.restype = C.c_int64
        L.poro_host_pressure_bc_labels.argtypes = [C.c_void_p, _ip]
        L.poro_host_displacement_bc_labels.restype = C.c_int64
        L.poro_host_displacement_bc_labels.argtypes = [C.c_void_p, _ip]
        L.poro_host_runner_preconditioners.argtypes = [C.c_void_p, _ip]
        L.poro_host_runner_preconditioners.restype = None
        L.poro_host_runner_pressure_solver_tolerances.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.poro_host_runner_free.argtypes = [C.c_void_p]
        L.poro_host_runner_free.restype = None
        _host = L
    return _host


def _arr_i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def _arr_d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _field_args(*arrays):
    """the arguments of a per-cell field setter behind its handle: (the flattened arrays, which the caller keeps alive over the call; [pointer, ..., length]).  All None
    (back to the scalars): null pointers and length 0"""
    if all(a is None for a in arrays):
        return (), [None] * len(arrays) + [0]
    flat = [_arr_d(np.asarray(a).reshape(-1)) for a in arrays]
    if len({a.size for a, _ in flat}) != 1:
        raise ValueError("set_cell_moduli: lame_lambda and shear_G differ in length")
    return flat, [p for _, p in flat] + [flat[0][0].size]


def _layer_args(layers):
    """the arguments of a layer setter behind its handle: layers [(top, value, ...), ...] -> (the columns to keep alive, [n_layers, pointer to the tops, pointer per value])"""
    cols = [_arr_d(c) for c in zip(*layers)]
    return cols, [len(layers)] + [p for _, p in cols]


def _tensor_args(values, dim):
    """the arguments of a tensor setter behind its handle: values of shape (n_cells, dim), x first -> (the array to keep alive, [pointer, n_cells]); None: back to the scalar"""
    if values is None:
        return None, [None, 0]
    a, p = _arr_d(np.asarray(values, dtype=np.float64).reshape(-1))
    if a.size % dim:
        raise ValueError(f"set_cell_permeability_tensor: values of shape (n_cells, {dim}) are needed")
    return a, [p, a.size // dim]


def read_input(path=None):
    """InputDataPoroel::read_input_file (InputDataPoroel.h:77-86); path=None gives the declared defaults."""
    out = InputFlat()
    if load_host().poro_host_read_input(path.encode() if path else None, C.byref(out)) != 0:
        raise RuntimeError(load_host().poro_host_last_error().decode())
    return out


class Problem:
    """Mesh + DoFs + FE tables + constraints = everything poro_desc points at (owned by the C++ host layer)."""

    def __init__(self, handle, owned=True):
        if not handle:
            raise RuntimeError(load_host().poro_host_last_error().decode())
        self.handle = C.c_void_p(handle)
        self.owned = owned                      # False: the C++ side (a Runner that adapted its mesh) frees it
        self.desc_ptr = load_host().poro_host_desc(self.handle)
        self.desc = self.desc_ptr.contents

    @staticmethod
    def _bc(dirichlet, neumann):
        dl, dc, dv = (list(x) for x in zip(*dirichlet)) if dirichlet else ([], [], [])
        nl, nc, nv = (list(x) for x in zip(*neumann)) if neumann else ([], [], [])
        keep = [_arr_i(dl), _arr_i(dc), _arr_d(dv), _arr_i(nl), _arr_i(nc), _arr_d(nv)]
        return keep, [len(dl), keep[0][1], keep[1][1], keep[2][1], len(nl), keep[3][1], keep[4][1], keep[5][1]]

    @classmethod
    def box(cls, dim, n, size, degree_u, material, dirichlet, neumann=(), rank=0, n_ranks=1):
        """hyper_rectangle(colorize) box of n[d] cells (PoroelasticityFSS.h:418-435); dirichlet / neumann = [(label, component, value)]."""
        keep, args = cls._bc(dirichlet, neumann)
        n3, pn = _arr_i(list(n) + [1] * (3 - len(n)))
        s3, ps = _arr_d(list(size) + [1.0] * (3 - len(size)))
        return cls(load_host().poro_host_build_box(dim, pn, ps, degree_u, rank, n_ranks, *args, C.byref(material)))

    @classmethod
    def graded_box(cls, dim, n, size, degree_u, material, dirichlet, grading, neumann=()):
        """the colorized box with exponentially graded vertex spacing (grading[d] = 0: uniform in that direction): rectilinear cells of different sizes, NO box tag -
        the general (unstructured) kernels run on it"""
        keep, args = cls._bc(dirichlet, neumann)
        n3, pn = _arr_i(list(n) + [1] * (3 - len(n)))
        s3, ps = _arr_d(list(size) + [1.0] * (3 - len(size)))
        g3, pg = _arr_d(list(grading) + [0.0] * (3 - len(grading)))
        return cls(load_host().poro_host_build_graded_box(dim, pn, ps, degree_u, pg, *args, C.byref(material)))

    @classmethod
    def refined_box(cls, dim, n, size, degree_u, material, dirichlet, refine_lo, refine_hi, neumann=()):
        """box of n[d] coarse cells whose cells with index in [refine_lo, refine_hi) are split once (2^dim children): a mesh with hanging nodes,
        as one refine_mesh() pass of the reference produces (PoroelasticityFSS.h:447-498); the constraint lists come with the descriptor"""
        keep, args = cls._bc(dirichlet, neumann)
        n3, pn = _arr_i(list(n) + [1] * (3 - len(n)))
        s3, ps = _arr_d(list(size) + [1.0] * (3 - len(size)))
        lo, plo = _arr_i(list(refine_lo) + [0] * (3 - len(refine_lo)))
        hi, phi = _arr_i(list(refine_hi) + [1] * (3 - len(refine_hi)))
        return cls(load_host().poro_host_build_refined_box(dim, pn, ps, degree_u, plo, phi, *args, C.byref(material)))

    @classmethod
    def refined_box_mask(cls, dim, n, size, degree_u, material, dirichlet, mask, neumann=()):
        """the same mesh class from a mask: mask[c] != 0 splits coarse cell c (lexicographic, x fastest; any array with prod(n) entries).  The block form is this
        with the block's mask.  An all-zero mask gives the uniform box as a GENERAL mesh with the coarse space of PREC_TWO_LEVEL and no box tag - the starting
        point of an adaptive run; `box` is the way to the structured kernels"""
        keep, args = cls._bc(dirichlet, neumann)
        n3, pn = _arr_i(list(n) + [1] * (3 - len(n)))
        s3, ps = _arr_d(list(size) + [1.0] * (3 - len(size)))
        m, pm = _arr_i(np.asarray(mask).reshape(-1) != 0)
        if m.size != int(np.prod(n3)):
            raise ValueError("refined_box_mask: the mask needs one entry per coarse cell")
        return cls(load_host().poro_host_build_refined_box_mask(dim, pn, ps, degree_u, pm, *args, C.byref(material)))

    def refine_mask(self):
        """the refinement mask of a refined box (one int32 per coarse cell)"""
        H = load_host()
        n = H.poro_host_refine_mask(self.handle, None)
        if n < 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        m = np.zeros(n, dtype=np.int32)
        H.poro_host_refine_mask(self.handle, m.ctypes.data_as(_ip))
        return m

    def cell_parents(self):
        """(coarse cell, child number) of every cell of a refined box; child = cx + 2 cy + 4 cz, -1 for an unrefined coarse cell"""
        H = load_host()
        n = H.poro_host_cell_parents(self.handle, None, None)
        if n < 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        a, b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        H.poro_host_cell_parents(self.handle, a.ctypes.data_as(_ip), b.ctypes.data_as(_ip))
        return a, b

    def mark_fixed_fraction(self, eta, refine_fraction=0.6, coarsen_fraction=0.4):
        """refine_and_coarsen_fixed_fraction on the criteria eta[n_cells] + the level limits of refine_mesh (PoroelasticityFSS.h:460-472): the mask of the next mesh"""
        H = load_host()
        e, pe = _arr_d(eta)
        if e.size != self.desc.n_cells:
            raise ValueError("mark_fixed_fraction: one eta per cell")
        m = np.zeros(len(self.refine_mask()), dtype=np.int32)
        if H.poro_host_mark_fixed_fraction(self.handle, pe, refine_fraction, coarsen_fraction, m.ctypes.data_as(_ip)) != 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        return m

    def kelly_tables(self):
        """the face tables Context.pres_estimate_error builds for this mesh (the same host code, without a GPU): dict of cell_a, cell_b, code [n_faces], ent_ptr [n_cells + 1],
        ent_face, ent_hcell [n_entries]; layout in csrc/kelly_tables.hpp and csrc/kernels_kelly.hip"""
        H = load_host()
        ne = C.c_int64()
        nf = H.poro_host_kelly_tables(self.handle, C.byref(ne), None, None, None, None, None, None)
        if nf < 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        T = dict(cell_a=np.zeros(nf, np.int32), cell_b=np.zeros(nf, np.int32), code=np.zeros(nf, np.int32), ent_ptr=np.zeros(self.desc.n_cells + 1, np.int64),
                 ent_face=np.zeros(ne.value, np.int32), ent_hcell=np.zeros(ne.value, np.int32))
        H.poro_host_kelly_tables(self.handle, None, *(T[k].ctypes.data_as(_lp if k == "ent_ptr" else _ip) for k in ("cell_a", "cell_b", "code", "ent_ptr", "ent_face", "ent_hcell")))
        return T

    def transfer_rows_p(self, new):
        """(ptr, node, weight): row i evaluates this (old) problem's pressure FE function at vertex i of `new` (both refined boxes over the same coarse box)"""
        H = load_host()
        ptr = np.zeros(new.desc.n_dofs_p + 1, dtype=np.int64)
        nnz = H.poro_host_transfer_rows_p(self.handle, new.handle, ptr.ctypes.data_as(_lp), None, None)
        if nnz < 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        node, w = np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
        H.poro_host_transfer_rows_p(self.handle, new.handle, ptr.ctypes.data_as(_lp), node.ctypes.data_as(_ip), w.ctypes.data_as(_dp))
        return ptr, node, w

    @classmethod
    def gmsh(cls, path, degree_u, material, dirichlet, neumann=(), refine=0):
        """Gmsh 2.2 quadrilateral mesh (read_mesh, PoroelasticityFSS.h:438-445), optionally after `refine` uniform refinements.  Where the mesh fills a rectangle whose sides
        carry the colorized boundary ids the descriptor also gets an auxiliary uniform box as coarse space (poro_desc.coarse -> PREC_TWO_LEVEL)"""
        keep, args = cls._bc(dirichlet, neumann)
        if refine:
            return cls(load_host().poro_host_build_gmsh_refined(path.encode(), degree_u, int(refine), *args, C.byref(material)))
        return cls(load_host().poro_host_build_gmsh(path.encode(), degree_u, *args, C.byref(material)))

    def partition(self, rank, n_ranks, coarse=False):
        """piece `rank` of a general partition of this (global) problem: contiguous ranges of the cells in Morton order + interface lists
        (poro_partition.n_neighbours > 0); .local_to_global_u / _p map the piece's dofs back.  coarse=True: the piece also carries the
        coarse space of PREC_TWO_LEVEL (poro_desc.coarse: its own copy of the whole box problem + the global interpolation rows of its nodes)"""
        H = load_host()
        h = H.poro_host_partition_ex(self.handle, rank, n_ranks, 1 if coarse else 0)
        if not h:
            raise RuntimeError(H.poro_host_last_error().decode())
        P = type(self)(h)
        for name, space in (("local_to_global_u", 0), ("local_to_global_p", 1)):
            a = np.zeros(H.poro_host_local_to_global(h, space, None), dtype=np.int32)
            H.poro_host_local_to_global(h, space, a.ctypes.data_as(_ip))
            setattr(P, name, a)
        return P

    def tie_boundary(self, conditions):
        """extension: rigid frictionless plates [(boundary label, component)] - that displacement component takes one (unknown) value on the whole boundary;
        ordinary entries x[dof] = x[master] of the displacement constraint list (poro_desc.cons_u)"""
        lab, pl = _arr_i([c[0] for c in conditions]); comp, pc = _arr_i([c[1] for c in conditions])
        self._host("tie_boundary", len(conditions), pl, pc)
        self.desc = self.desc_ptr.contents
        return self

    def set_pressure_bc(self, conditions):
        """extension (the reference has no pressure boundary conditions): prescribed pressure [(boundary label, value)], e.g. a drained face p = 0.  One rank.  Also on
        meshes with hanging nodes (refined boxes, adapted meshes): every vertex of the labelled faces is listed, a hanging one among them with the value its (listed)
        masters give.  The coarse problem of PREC_TWO_LEVEL (refined boxes: same labels; Gmsh grids with an auxiliary box: the labels translated to the box's sides)
        gets the same condition, also when it was built before this call"""
        lab, pl = _arr_i([c[0] for c in conditions]); val, pv = _arr_d([c[1] for c in conditions])
        self._host("set_pressure_bc", len(conditions), pl, pv)
        self.desc = self.desc_ptr.contents
        return self

    def pressure_bc_labels(self):
        """per entry of desc.dirichlet_dof_p the boundary label that prescribed it; on an edge shared by two labelled faces the first condition of set_pressure_bc wins"""
        H = load_host()
        out = np.zeros(H.poro_host_pressure_bc_labels(self.handle, None), dtype=np.int32)
        H.poro_host_pressure_bc_labels(self.handle, out.ctypes.data_as(_ip))
        return out

    def displacement_bc_labels(self):
        """[n_dirichlet, 2]: per entry of desc.dirichlet_dof the (boundary label, component) of the displacement condition that prescribed it; where two conditions
        meet in a dof the first one of the list wins, as for the values.  Empty where the Dirichlet list was given by the caller (pieces of a partition)"""
        H = load_host()
        out = np.zeros((H.poro_host_displacement_bc_labels(self.handle, None), 2), dtype=np.int32)
        if out.size:
            H.poro_host_displacement_bc_labels(self.handle, out.ctypes.data_as(_ip))
        return out

    def _host(self, name, *args):
        """poro_host_<name>(handle, *args); raises what the host layer reports"""
        H = load_host()
        if getattr(H, "poro_host_" + name)(self.handle, *args) != 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        return self

    def _carried(self, name, n_arrays):
        """the n_arrays arrays of the per-cell field poro_host_get_<name> reads, or None where the problem carries none"""
        get = getattr(load_host(), "poro_host_get_" + name)
        n = get(self.handle, *[None] * n_arrays)
        if not n:
            return None
        out = [np.empty(n) for _ in range(n_arrays)]
        get(self.handle, *[o.ctypes.data_as(_dp) for o in out])
        return out

    def set_cell_permeability(self, values):
        """extension: per-cell k / mu of the pressure system, one value per cell of this mesh (None: back to the scalar of the material).  Kept with the problem: Context,
        run_problem and Runner hand it to the contexts they create, and an adaptive run carries it to every new mesh (a child takes its parent's value)"""
        keep, args = _field_args(values)
        return self._host("set_cell_permeability", *args)

    def set_permeability_layers(self, layers):
        """the same by layers [(top, value), ...] along the slowest direction (z in 3D, y in 2D), tops ascending: a cell takes the value of the first layer whose top is >=
        the coordinate of its centre"""
        keep, args = _layer_args(layers)
        return self._host("set_permeability_layers", *args)

    def inherit_cell_permeability(self, old):
        """what an adaptive run does with the field: this refined box takes the field of `old`, a refined box over the same coarse box, coarse cell by coarse cell"""
        return self._host("inherit_cell_permeability", old.handle)

    def cell_permeability(self):
        """the per-cell k / mu this problem carries, or None"""
        f = self._carried("cell_permeability", 1)
        return f and f[0]

    def set_cell_permeability_tensor(self, values):
        """extension: the per-cell diagonal tensor diag(kx, ky[, kz]) / mu of the pressure system, shape (n_cells, dim), x first (None: none).  Kept with the problem and
        handed over like the scalar field, which it replaces (a problem carries one of the two); an adaptive run carries it to every new mesh, component by component"""
        keep, args = _tensor_args(values, self.desc.dim)
        return self._host("set_cell_permeability_tensor", *args)

    def set_permeability_tensor_layers(self, layers):
        """the same by layers [(top, kx, ky[, kz]), ...] along the slowest direction, tops ascending, chosen by cell centres as set_permeability_layers does"""
        dim = self.desc.dim
        if any(len(l) != dim + 1 for l in layers):
            raise ValueError(f"set_permeability_tensor_layers: every layer is (top, {', '.join(['kx', 'ky', 'kz'][:dim])})")
        keep, args = _layer_args(layers)
        return self._host("set_permeability_tensor_layers", *args, *[None] * (3 - dim))

    def inherit_cell_permeability_tensor(self, old):
        """what an adaptive run does with the tensor: a child takes its parent's components exactly, a coarsened parent the per-component mean"""
        return self._host("inherit_cell_permeability_tensor", old.handle)

    def cell_permeability_tensor(self):
        """the per-cell tensor this problem carries, shape (n_cells, dim), or None"""
        f = self._carried("cell_permeability_tensor", 1)
        return f and f[0].reshape(-1, self.desc.dim)

    def set_cell_moduli(self, lame_lambda, shear_G):
        """extension: per-cell Lame lambda and shear modulus G of the displacement system, one pair per cell of this mesh (both None: back to the scalars of the material).
        Kept with the problem like the permeability: Context, run_problem and Runner hand it to the contexts they create, an adaptive run carries it to every new mesh"""
        keep, args = _field_args(lame_lambda, shear_G)
        return self._host("set_cell_moduli", *args)

    def set_moduli_layers(self, layers):
        """the same by layers [(top, young, poisson), ...] along the slowest direction (z in 3D, y in 2D), tops ascending: a cell takes the first layer whose top is >= the
        coordinate of its centre; lambda = E nu / ((1 + nu) (1 - 2 nu)), G = E / (2 (1 + nu)) as for the parameter file's values"""
        keep, args = _layer_args(layers)
        return self._host("set_moduli_layers", *args)

    def inherit_cell_moduli(self, old):
        """what an adaptive run does with the field: this refined box takes the moduli of `old`, a refined box over the same coarse box, coarse cell by coarse cell"""
        return self._host("inherit_cell_moduli", old.handle)

    def cell_moduli(self):
        """(lame_lambda, shear_G) this problem carries, or None"""
        f = self._carried("cell_moduli", 2)
        return f and tuple(f)

    def set_gravity(self, g, fluid_density=0.0, bulk_density=None, hydrostatic_init=False):
        """extension: gravity.  g: the vector, one component per dimension (None or zeros: off); fluid_density: rho_f of the Darcy gravity flux q = -kappa (grad p - rho_f g)
        (0: no flux term); bulk_density: the scalar rho_b of the body force rho_b g (None: keep the problem's, 2700 at first - the default of "Properties/Bulk density");
        hydrostatic_init: a run starts from p_init + rho_f g . (x - x_top), x_top the vertex furthest against g.  Kept with the problem like the per-cell fields: Context,
        run_problem and Runner hand it to the contexts they create, an adaptive run to every new mesh"""
        gp = None
        if g is not None:
            ga, gp = _arr_d(g)
            if ga.size != self.desc.dim:
                raise ValueError(f"set_gravity: g needs {self.desc.dim} components")
        return self._host("set_gravity", gp, float(fluid_density), -1.0 if bulk_density is None else float(bulk_density), int(bool(hydrostatic_init)))

    def gravity(self):
        """(g[dim], fluid_density, bulk_density, hydrostatic_init) this problem carries; g is None while gravity is off"""
        g, rf, rb, hy = (C.c_double * 3)(), C.c_double(), C.c_double(), C.c_int32()
        on = load_host().poro_host_get_gravity(self.handle, g, C.byref(rf), C.byref(rb), C.byref(hy))
        return (np.array(g[:self.desc.dim]) if on else None), rf.value, rb.value, bool(hy.value)

    def set_cell_density(self, values):
        """extension: per-cell bulk density of the body force, one value per cell of this mesh (None: back to the scalar).  Kept and carried like the other per-cell fields"""
        keep, args = _field_args(values)
        return self._host("set_cell_density", *args)

    def set_density_layers(self, layers):
        """the same by layers [(top, rho), ...] along the slowest direction, tops ascending, chosen by cell centres as set_permeability_layers does"""
        keep, args = _layer_args(layers)
        return self._host("set_density_layers", *args)

    def inherit_cell_density(self, old):
        """what an adaptive run does with the density: a child takes its parent's value, a coarsened parent the mean of its children; g and the scalar densities go along"""
        return self._host("inherit_cell_density", old.handle)

    def cell_density(self):
        """the per-cell bulk density this problem carries, or None"""
        f = self._carried("cell_density", 1)
        return f and f[0]

    def close(self):
        if self.handle:
            if self.owned:
                load_host().poro_host_free(self.handle)
            self.handle = None

    def array(self, name, shape, dtype=np.float64):
        ptr = getattr(self.desc, name)
        return np.ctypeslib.as_array(ptr, shape=shape).copy() if int(np.prod(shape)) else np.zeros(shape, dtype)


class Context:
    """Handle to the device-resident solver state behind the C-ABI."""

    def __init__(self, problem, device=0, operator_mode=OP_CSR, ptr=None):
        self.L = load_hip()
        self.problem = problem
        self.n_u, self.n_p, self.dim = problem.desc.n_dofs_u, problem.desc.n_dofs_p, problem.desc.dim
        if ptr is None:
            p = C.c_void_p()
            self._chk(self.L.poro_ctx_create(problem.desc_ptr, device, operator_mode, C.byref(p)))
            ptr = p
            # the per-cell fields the problem carries (Problem.set_cell_permeability / set_permeability_layers, set_cell_moduli / set_moduli_layers)
            for name, hand_over in (("cell_permeability", self.set_cell_permeability), ("cell_permeability_tensor", self.set_cell_permeability_tensor), ("cell_moduli", self.set_cell_moduli),
                                    ("cell_density", self.set_cell_density), ("gravity", lambda g, rho_f, rho_b, _hyd: g is not None and self.set_gravity(g, rho_b, rho_f))):
                carried = getattr(problem, name, None)                 # (a Problem; descriptor holders of other kinds carry no field)
                field = carried() if carried else None
                if field is not None:
                    self.ptr = ptr
                    try:
                        hand_over(*(field if isinstance(field, tuple) else (field,)))
                    except RuntimeError:
                        self.close()
                        raise
        self.ptr = ptr
        self._cb = None

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.poro_last_error().decode())
        return rc

    def close(self):
        if self.ptr:
            self.L.poro_ctx_destroy(self.ptr)
            self.ptr = None

    def synchronize(self):
        """wait for everything the context has enqueued (device-only entry points are stream-ordered)"""
        self._chk(self.L.poro_ctx_synchronize(self.ptr))

    def set_scatter_mode(self, mode):
        """SCATTER_COLOURED (default: one launch per colour class, bitwise reproducible) or SCATTER_ATOMIC (one launch, fp64 atomic adds, last bits differ from run
        to run) for the matrix-free operator on general meshes; a no-op on box-tagged contexts"""
        self._chk(self.L.poro_ctx_set_scatter_mode(self.ptr, int(mode)))

    def get_scatter_mode(self):
        m = C.c_int32()
        self._chk(self.L.poro_ctx_get_scatter_mode(self.ptr, C.byref(m)))
        return m.value

    def set_operator_form(self, form):
        """OPFORM_GENERAL (default: the general cell kernels over every cell) or OPFORM_HYBRID for the matrix-free operator on refined boxes: the coarse box's structured
        kernel over the whole box, minus the element products of the refined box cells, plus the general kernels over the fine cells only.  The first enable derives the
        plan on the host and checks one product (outside timed regions); raises where the mesh cannot take the form, which then stays as it was.  A no-op on
        box-tagged contexts"""
        self._chk(self.L.poro_ctx_set_operator_form(self.ptr, int(form)))

    def get_operator_form(self):
        """(form, cells the general kernels run over per application, refined box cells whose element products are subtracted)"""
        f, g, r = C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self.L.poro_ctx_get_operator_form(self.ptr, C.byref(f), C.byref(g), C.byref(r)))
        return f.value, g.value, r.value

    def set_fdm_precision(self, precision):
        """FDM_FP64 (default) or FDM_FP32: fp32 transforms in the displacement system's block FDM where it runs in the single-rank 3D octant form (the CG around it
        stays fp64); no effect on any other form"""
        self._chk(self.L.poro_ctx_set_fdm_precision(self.ptr, int(precision)))

    def get_fdm_precision(self):
        """(requested, effective); with FDM_FP32 requested this builds the block FDM where the context can use it, so that `effective` is final"""
        r, e = C.c_int32(), C.c_int32()
        self._chk(self.L.poro_ctx_get_fdm_precision(self.ptr, C.byref(r), C.byref(e)))
        return r.value, e.value

    def set_fdm_form(self, form):
        """FDM_FORM_DEFAULT (the octant form where every direction is mirror-symmetric, else the nodal kernels) or FDM_FORM_PER_DIRECTION: the octant form's three
        contiguous passes on single-rank 3D boxes where only some directions are (one-sided faces, graded lines).  Any time between solves; a block FDM built in the
        other form is rebuilt at its next use.  Partitioned and 2D contexts record the request and run what they ran; raises on an unknown value"""
        self._chk(self.L.poro_ctx_set_fdm_form(self.ptr, int(form)))

    def get_fdm_form(self):
        """(requested, effective FDM_RUNS_*, (split_x, split_y, split_z)); builds the block FDM where the context can use it, so that the answer is final"""
        r, e, m = C.c_int32(), C.c_int32(), (C.c_int32 * 3)()
        self._chk(self.L.poro_ctx_get_fdm_form(self.ptr, C.byref(r), C.byref(e), m))
        return r.value, e.value, tuple(int(v) for v in m)

    def set_moduli_operator(self, form):
        """MODULI_OP_CELLS (the general cell loop on a box with per-cell moduli, the default) or MODULI_OP_STRUCTURED: one structured launch per operator application
        where the field is constant within every cell layer of z.  Any time; stays through field changes.  Effective on single-rank uniform 3D boxes of degree 1 or 2 in
        matrix-free mode with a kind-1 field; everywhere else the request is recorded and the context runs what it ran.  Raises on an unknown value"""
        self._chk(self.L.poro_ctx_set_moduli_operator(self.ptr, int(form)))

    def get_moduli_operator(self):
        """(requested, effective): MODULI_OP_*; effective = what an operator application runs now"""
        r, e = C.c_int32(), C.c_int32()
        self._chk(self.L.poro_ctx_get_moduli_operator(self.ptr, C.byref(r), C.byref(e)))
        return r.value, e.value

    def _get_field(self, get, n_arrays):
        """(array or None, ..., kind) of the per-cell field the getter `get` of the library reads"""
        kind = C.c_int32()
        self._chk(get(self.ptr, *[None] * n_arrays, 0, C.byref(kind)))
        if not kind.value:
            return (None,) * n_arrays + (0,)
        out = [np.empty(self.problem.desc.n_cells) for _ in range(n_arrays)]
        self._chk(get(self.ptr, *[o.ctypes.data_as(_dp) for o in out], out[0].size, C.byref(kind)))
        return (*out, kind.value)

    def set_cell_permeability(self, values):
        """per-cell k / mu of the pressure system, one value per cell in the descriptor's cell order (None: back to the scalar of the material).  One rank; re-assembles
        the Laplace matrix and invalidates the cached Jacobian: call pres_assemble_jacobian again.  Raises on a wrong length and on values that are not finite and > 0"""
        keep, args = _field_args(values)
        self._chk(self.L.poro_ctx_set_cell_permeability(self.ptr, *args))

    def get_cell_permeability(self):
        """(values or None, kind): kind 0 no field, 1 layered along the slowest direction of a box / tensor-product grid (PREC_FDM is exact), 2 general"""
        return self._get_field(self.L.poro_ctx_get_cell_permeability, 1)

    def set_cell_permeability_tensor(self, values):
        """per-cell diagonal tensor diag(kx, ky[, kz]) / mu of the pressure system, shape (n_cells, dim), x first, cells in the descriptor's order (None: back to the scalar
        of the material).  Replaces a scalar field (a context holds one of the two).  One rank; invalidates like set_cell_permeability: call pres_assemble_jacobian
        again.  Raises on a wrong length and on a component that is not finite and > 0"""
        keep, args = _tensor_args(values, self.dim)
        self._chk(self.L.poro_ctx_set_cell_permeability_tensor(self.ptr, *args))

    def get_cell_permeability_tensor(self):
        """(values of shape (n_cells, dim) or None, kind): kind 0 no tensor, 1 every component layered along the slowest direction of a box / tensor-product grid
        (PREC_FDM is exact), 2 general"""
        kind = C.c_int32()
        self._chk(self.L.poro_ctx_get_cell_permeability_tensor(self.ptr, None, 0, C.byref(kind)))
        if not kind.value:
            return None, 0
        out = np.empty((self.problem.desc.n_cells, self.dim))
        self._chk(self.L.poro_ctx_get_cell_permeability_tensor(self.ptr, out.ctypes.data_as(_dp), out.shape[0], C.byref(kind)))
        return out, kind.value

    def set_cell_moduli(self, lame_lambda, shear_G):
        """per-cell Lame lambda and shear modulus G of the displacement system, one pair per cell in the descriptor's cell order (both None: back to the scalars of the
        material; one None is refused).  One rank.  Drops the assembled displacement system: call disp_assemble next.  Raises on a wrong length and on values that are
        not finite with G > 0 and 3 lambda + 2 G > 0"""
        if (lame_lambda is None) != (shear_G is None):
            a, pa = _arr_d(np.asarray(shear_G if lame_lambda is None else lame_lambda).reshape(-1))      # (the library words the refusal)
            self._chk(self.L.poro_ctx_set_cell_moduli(self.ptr, None if lame_lambda is None else pa, None if shear_G is None else pa, a.size))
            return
        keep, args = _field_args(lame_lambda, shear_G)
        self._chk(self.L.poro_ctx_set_cell_moduli(self.ptr, *args))

    def get_cell_moduli(self):
        """(lame_lambda or None, shear_G or None, kind): kind 0 no field, 1 layered along the slowest direction of a box / tensor-product grid, 2 general"""
        return self._get_field(self.L.poro_ctx_get_cell_moduli, 2)

    def set_gravity(self, g, bulk_density, fluid_density=0.0):
        """gravity vector g (one component per dimension; None or zeros: off), the scalar bulk density rho_b of the body force and the fluid density rho_f of the Darcy
        gravity flux (0: none).  Right-hand sides only: b_i += sum_c rho_b int_c g . phi_i, and R = -((M t + kappa K p) + (src + f_g)) with
        f_g[i] = -sum_c rho_f int_c (kappa_c g) . grad(phi_i).  Any time; the next disp_assemble_system rebuilds the load vector alone, whatever its `rebuild` says"""
        gp = None
        if g is not None:
            ga, gp = _arr_d(g)
            if ga.size != self.dim:
                raise ValueError(f"set_gravity: g needs {self.dim} components")
        self._chk(self.L.poro_ctx_set_gravity(self.ptr, gp, float(bulk_density), float(fluid_density)))

    def get_gravity(self):
        """(g[dim], bulk_density, fluid_density, on)"""
        g, rb, rf, on = np.zeros(self.dim), C.c_double(), C.c_double(), C.c_int32()
        self._chk(self.L.poro_ctx_get_gravity(self.ptr, g.ctypes.data_as(_dp), C.byref(rb), C.byref(rf), C.byref(on)))
        return g, rb.value, rf.value, bool(on.value)

    def set_cell_density(self, values):
        """per-cell bulk density in place of the scalar of set_gravity, one value per cell in the descriptor's cell order (None: back to the scalar).  One rank.  Raises on a
        wrong length and on a value that is not finite and > 0 (the message names the cell); the context then stays as it was"""
        keep, args = _field_args(values)
        self._chk(self.L.poro_ctx_set_cell_density(self.ptr, *args))

    def get_cell_density(self):
        """(values or None, kind): kind 0 no field, 1 layered along the slowest direction of a box / tensor-product grid, 2 general"""
        return self._get_field(self.L.poro_ctx_get_cell_density, 1)

    def gravity_vectors(self):
        """(body_u[n_u], flux_p[n_p]): the two gravity vectors alone, without tractions and well source (zeros while gravity is off / the fluid density is 0)"""
        b, f = np.empty(self.n_u), np.empty(self.n_p)
        self._chk(self.L.poro_get_gravity_vectors(self.ptr, b.ctypes.data_as(_dp), f.ctypes.data_as(_dp)))
        return b, f

    def pres_apply_jacobian(self, x):
        """y = J x with the operator the Krylov solver of pres_solve applies (the stencil on matrix-free boxes, CSR elsewhere); after pres_assemble_jacobian"""
        a, p = _arr_d(x)
        if a.size != self.n_p:
            raise ValueError("pres_apply_jacobian: one value per pressure dof")
        y = np.empty_like(a)
        self._chk(self.L.poro_pres_apply_jacobian(self.ptr, p, y.ctypes.data_as(_dp)))
        return y

    def _len(self, which):
        return self.n_u if which in (VEC_U, VEC_RHS_U, VEC_DIAG_U) else self.n_p

    def set(self, which, arr):
        a, p = _arr_d(arr)
        self._chk(self.L.poro_vec_set(self.ptr, which, p, a.size))

    def get(self, which):
        out = np.empty(self._len(which))
        self._chk(self.L.poro_vec_get(self.ptr, which, out.ctypes.data_as(_dp), out.size))
        return out

    def fill(self, which, v):
        self._chk(self.L.poro_vec_fill(self.ptr, which, v))

    def copy(self, dst, src):
        self._chk(self.L.poro_vec_copy(self.ptr, dst, src))

    def axpy(self, y, a, x):
        self._chk(self.L.poro_vec_axpy(self.ptr, y, a, x))

    def norm(self, which):
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.poro_vec_norm(self.ptr, which, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pres_estimate_error(self, which=VEC_P):
        """Kelly error indicator of a pressure-space vector, one value per cell (definition: include/poroel_hip.h)"""
        eta = np.empty(self.problem.desc.n_cells)
        self._chk(self.L.poro_pres_estimate_error(self.ptr, int(which), eta.ctypes.data_as(_dp)))
        return eta

    def darcy_velocity(self, which=VEC_P):
        """q_c = -kappa_c (grad p_h(x_c) - rho_f g) at the cell centres, [n_cells][dim] (definition: include/poroel_hip.h)"""
        q = np.empty((self.problem.desc.n_cells, self.dim))
        self._chk(self.L.poro_pres_darcy_velocity(self.ptr, int(which), q.ctypes.data_as(_dp)))
        return q

    def boundary_discharge(self, labels=None, which=VEC_P):
        """(Q_face[n_bfaces], Q_label[len(labels)]): int_F q . n dS per boundary face, outward positive, and its deterministic sums over the faces of each label"""
        Q = np.empty(self.problem.desc.n_bfaces)
        lab, pl = _arr_i([] if labels is None else labels)
        Ql = np.empty(lab.size)
        self._chk(self.L.poro_pres_boundary_discharge(self.ptr, int(which), Q.ctypes.data_as(_dp), pl if lab.size else None, int(lab.size), Ql.ctypes.data_as(_dp) if lab.size else None))
        return Q, Ql

    def flow_balance(self, dt):
        """(terms, outflow_dof): the terms of the discrete fluid balance as a dict and C^T(-r) on the prescribed-pressure dofs in the order of dirichlet_dof_p"""
        t = FlowBalanceTerms()
        out = np.empty(self.problem.desc.n_dirichlet_p)
        self._chk(self.L.poro_pres_flow_balance(self.ptr, float(dt), C.byref(t), out.ctypes.data_as(_dp) if out.size else None))
        return t.as_dict(), out

    def cell_stress(self, which_u=VEC_U, which_p=VEC_P):
        """(strain, effective, total), [n_cells][n_sym] each: eps_c = sym grad u_h(x_c), sigma'_c = lambda_c tr(eps_c) I + 2 G_c eps_c with the cell's OWN moduli,
        sigma_c = sigma'_c - alpha p_h(x_c) I at the cell centres; which_p=None (or -1): no pressure, total = effective (definition: include/poroel_hip.h)"""
        nc, ns = self.problem.desc.n_cells, self.dim * (self.dim + 1) // 2
        e, se, st = (np.empty((nc, ns)) for _ in range(3))
        self._chk(self.L.poro_disp_cell_stress(self.ptr, int(which_u), -1 if which_p is None else int(which_p), e.ctypes.data_as(_dp), se.ctypes.data_as(_dp), st.ctypes.data_as(_dp)))
        return e, se, st

    def cell_measures(self, which_u=VEC_U, which_p=VEC_P, cohesion=None, friction_angle=None):
        """(measures [n_cells][6], summary): per cell s1 >= s2 >= s3, mean, von Mises and the Mohr-Coulomb function f of the 3 x 3 EFFECTIVE stress (2D: plane strain);
        summary = {max_f, argmax_cell, n_failing} from the device.  cohesion and friction_angle (radians) both None: f = 0 and a summary of zeros.  which_p is checked
        and ignored (include/poroel_hip.h)"""
        if (cohesion is None) != (friction_angle is None):
            raise ValueError("cell_measures: give both cohesion and friction_angle, or neither")
        m = np.empty((self.problem.desc.n_cells, 6))
        mc = None if cohesion is None else MohrCoulomb(float(cohesion), float(friction_angle))
        summ = FailureSummary()
        self._chk(self.L.poro_disp_cell_measures(self.ptr, int(which_u), -1 if which_p is None else int(which_p), None if mc is None else C.byref(mc), m.ctypes.data_as(_dp), C.byref(summ)))
        return m, summ.as_dict()

    def force_balance(self):
        """The force balance of the displacement system at the present PORO_VEC_U / PORO_VEC_P (include/poroel_hip.h, poro_disp_force_balance): per component the arrays
        reaction_sum, free_row_sum, traction_sum, body_sum, coupling_sum [dim] and residual_l2; reaction_dof = C^T r on the Dirichlet dofs in the order of
        desc.dirichlet_dof; reaction_by_label[(label, component)] = its sums over the dofs each displacement condition prescribed (Problem.displacement_bc_labels;
        empty where the problem has no such record)"""
        t = ForceBalanceTerms()
        nd = self.problem.desc.n_dirichlet
        per_dof = np.empty(nd)
        self._chk(self.L.poro_disp_force_balance(self.ptr, C.byref(t), per_dof.ctypes.data_as(_dp) if nd else None))
        res = {n: np.array(getattr(t, n)[:self.dim]) for n in ("reaction_sum", "free_row_sum", "traction_sum", "body_sum", "coupling_sum")}
        res["residual_l2"] = t.residual_l2
        res["reaction_dof"] = per_dof
        by = {}
        if getattr(self, "_bc_pairs", None) is None:             # (the record belongs to the problem the context was made from: read once)
            owner = self.problem if hasattr(self.problem, "displacement_bc_labels") else getattr(self.problem, "source", None)      # (a descriptor copy keeps its source's dofs)
            labels = owner.displacement_bc_labels() if hasattr(owner, "displacement_bc_labels") else np.zeros((0, 2), dtype=np.int32)
            self._bc_pairs = np.unique(labels, axis=0, return_inverse=True) if len(labels) else (labels, np.zeros(0, dtype=np.int64))
        pairs, inverse = self._bc_pairs
        if len(inverse) == nd and nd:
            sums = np.bincount(np.asarray(inverse).ravel(), weights=per_dof, minlength=len(pairs))      # in the order of the dof list
            by = {(int(l), int(c)): float(v) for (l, c), v in zip(pairs.tolist(), sums.tolist())}
        res["reaction_by_label"] = by
        return res

    def transfer_p_from(self, other, rows):
        """VEC_P, VEC_EPSV, VEC_EPSV0 of `other` (the context of the previous mesh) -> this context through rows = (ptr, node, weight), e.g. other.problem.transfer_rows_p(self.problem)"""
        ptr = np.ascontiguousarray(rows[0], dtype=np.int64)
        node, pn = _arr_i(rows[1]); w, pw = _arr_d(rows[2])
        if ptr.size != self.n_p + 1:
            raise ValueError("transfer_p_from: ptr needs n_dofs_p + 1 entries")
        self._chk(self.L.poro_state_transfer_p(other.ptr, self.ptr, ptr.ctypes.data_as(_lp), pn, pw))

    def state_save(self):
        self._chk(self.L.poro_state_save(self.ptr))

    def state_restore(self):
        self._chk(self.L.poro_state_restore(self.ptr))

    def disp_assemble_system(self, rebuild=True):
        self._chk(self.L.poro_disp_assemble_system(self.ptr, int(rebuild)))

    @staticmethod
    def _opts(abs_tol, rel_tol, max_iter, prec, omega=1.0, stop_rule=STOP_RHS, poly_degree=0):
        return SolverOpts(abs_tol, rel_tol, max_iter, prec, omega, stop_rule, poly_degree)

    def supports_preconditioner(self, which_system, prec):
        """which_system: 0 displacement, 1 pressure / projection, 2 projection alone (prescribed pressures restrict 1, not 2)."""
        return bool(self.L.poro_supports_preconditioner(self.ptr, which_system, prec))

    def disp_solve(self, abs_tol=1e-12, rel_tol=0.0, max_iter=1000, prec=PREC_JACOBI, omega=1.2, reduction=False, poly_degree=0):
        """omega: SSOR relaxation, or (PREC_CHEBYSHEV) the interval ratio lambda_max / a (<= 0: default); poly_degree: Chebyshev degree (0: default)"""
        info = SolveInfo()
        if prec == PREC_CHEBYSHEV and omega == 1.2:
            omega = 0.0
        rc = self._chk(self.L.poro_disp_solve(self.ptr, C.byref(self._opts(abs_tol, rel_tol, max_iter, prec, omega, STOP_REDUCTION if reduction else STOP_RHS, poly_degree)), C.byref(info)))
        return rc, info

    def pres_assemble_residual(self, dt):
        l2 = C.c_double()
        self._chk(self.L.poro_pres_assemble_residual(self.ptr, dt, C.byref(l2)))
        return l2.value

    def pres_assemble_jacobian(self, dt):
        self._chk(self.L.poro_pres_assemble_jacobian(self.ptr, dt))

    def pres_apply_boundary_values(self):
        """VEC_P = listed value on the prescribed dofs; with hanging pressure nodes as well the constraints are then distributed, p[h] = sum w p[master] + b, so that
        the pressure is conforming beside a prescribed master (no-op without prescribed pressures)"""
        self._chk(self.L.poro_pres_apply_boundary_values(self.ptr))

    def pres_solve(self, abs_tol=0.0, rel_tol=1e-8, max_iter=1000, prec=PREC_JACOBI, omega=1.0):
        info = SolveInfo()
        rc = self._chk(self.L.poro_pres_solve(self.ptr, C.byref(self._opts(abs_tol, rel_tol, max_iter, prec, omega)), C.byref(info)))
        return rc, info

    def pres_update_volumetric_strain(self):
        self._chk(self.L.poro_pres_update_volumetric_strain(self.ptr))

    def supports_pres_newton_loop(self, abs_tol=0.0, rel_tol=1e-8, max_iter=1000, prec=PREC_FDM):
        return bool(self.L.poro_supports_pres_newton_loop(self.ptr, C.byref(self._opts(abs_tol, rel_tol, max_iter, prec, 1.0))))

    def pres_newton_loop(self, dt, pressure_tol, max_iterations, abs_tol=0.0, rel_tol=1e-8, max_iter=1000, prec=PREC_FDM, hint_slot=-1):
        """poro_pres_newton_loop (include/poroel_hip.h): the pressure Newton loop of one fixed-stress iteration as gated batches.  Returns a dict: iterations, solves,
        outcome (0 cap, 1 converged, 2 fallback), batches, pinf, l2[iterations], res / bn of every check that ran"""
        l2, res, bn = (np.zeros(max_iterations) for _ in range(3))
        rec = NewtonRecord(l2=l2.ctypes.data_as(_dp), res=res.ctypes.data_as(_dp), bn=bn.ctypes.data_as(_dp))
        self._chk(self.L.poro_pres_newton_loop(self.ptr, dt, pressure_tol, max_iterations, C.byref(self._opts(abs_tol, rel_tol, max_iter, prec, 1.0)), hint_slot, C.byref(rec)))
        checks = rec.solves + (1 if rec.outcome == 2 else 0)
        return dict(iterations=rec.iterations, solves=rec.solves, outcome=rec.outcome, batches=rec.batches, pinf=rec.pinf, l2=l2[:rec.iterations].copy(), res=res[:checks].copy(), bn=bn[:checks].copy())

    def proj_assemble_matrix(self):
        self._chk(self.L.poro_proj_assemble_matrix(self.ptr))

    def proj_assemble_rhs(self, comps):
        a, p = _arr_i(comps)
        self._chk(self.L.poro_proj_assemble_rhs(self.ptr, p, a.size))

    def proj_solve(self, entry, abs_tol=0.0, rel_tol=1e-8, max_iter=1000, prec=PREC_JACOBI, omega=1.0):
        info = SolveInfo()
        rc = self._chk(self.L.poro_proj_solve(self.ptr, entry, C.byref(self._opts(abs_tol, rel_tol, max_iter, prec, omega)), C.byref(info)))
        return rc, info

    def proj_solve_many(self, entries, abs_tol=0.0, rel_tol=1e-8, max_iter=1000, prec=PREC_JACOBI, omega=1.0):
        """several projection systems in one call (solved directly and together where PREC_FDM is the exact inverse: info.iterations == 0)"""
        ent, pe = _arr_i(list(entries)); infos = (SolveInfo * len(entries))()
        rc = self._chk(self.L.poro_proj_solve_many(self.ptr, pe, len(entries), C.byref(self._opts(abs_tol, rel_tol, max_iter, prec, omega)), infos))
        return rc, list(infos)

    def get_volumetric_strain(self):
        self._chk(self.L.poro_get_volumetric_strain(self.ptr))

    def get_effective_stresses(self):
        self._chk(self.L.poro_get_effective_stresses(self.ptr))

    def export_csr(self, which):
        n, nnz = C.c_int64(), C.c_int64()
        self._chk(self.L.poro_export_csr_size(self.ptr, which, C.byref(n), C.byref(nnz)))
        rp, col, val = np.empty(n.value + 1, np.int64), np.empty(nnz.value, np.int32), np.empty(nnz.value)
        self._chk(self.L.poro_export_csr(self.ptr, which, rp.ctypes.data_as(C.POINTER(C.c_int64)), col.ctypes.data_as(_ip), val.ctypes.data_as(_dp)))
        return rp, col, val

    def apply(self, which, x):
        a, p = _arr_d(x)
        y = np.empty_like(a)
        self._chk(self.L.poro_apply_operator(self.ptr, which, p, y.ctypes.data_as(_dp)))
        return y

    def apply_preconditioner_u(self, prec, g, reps=0):
        """z = P^-1 g with the displacement preconditioner; returns z (and the mean device seconds per application when reps > 0)"""
        a, p = _arr_d(g)
        z = np.empty_like(a)
        t = C.c_double(0.0)
        self._chk(self.L.poro_apply_preconditioner_u(self.ptr, prec, p, z.ctypes.data_as(_dp), reps, C.byref(t)))
        return (z, t.value) if reps > 0 else z

    def bench_operator(self, operator_mode, reps):
        t = C.c_double()
        self._chk(self.L.poro_bench_operator(self.ptr, MAT_A_U, operator_mode, reps, C.byref(t)))
        return t.value

    def timers_reset(self):
        self._chk(self.L.poro_timers_reset(self.ptr))

    def timers_enable(self, on):
        self._chk(self.L.poro_timers_enable(self.ptr, int(on)))

    def timer(self, name):
        s, n = C.c_double(), C.c_int64()
        self._chk(self.L.poro_timers_get(self.ptr, name.encode(), C.byref(s), C.byref(n)))
        return s.value, n.value

    def comm_callbacks(self, allreduce, sendrecv):
        """host-staged communicator (tests); allreduce(np_view) sums in place, sendrecv(send_view, recv_view, peer)."""
        def _ar(buf, n, _u):
            allreduce(np.ctypeslib.as_array(buf, shape=(n,)))

        def _sr(send, recv, n, peer, _u):
            sendrecv(np.ctypeslib.as_array(send, shape=(n,)), np.ctypeslib.as_array(recv, shape=(n,)), peer)
        self._cb = (ALLREDUCE_FN(_ar), SENDRECV_FN(_sr))
        self._chk(self.L.poro_ctx_comm_init_callbacks(self.ptr, self._cb[0], self._cb[1], None))

    def comm_rccl(self, unique_id_bytes):
        buf = C.create_string_buffer(bytes(unique_id_bytes), 128)
        self._chk(self.L.poro_ctx_comm_init_rccl(self.ptr, buf))


def rccl_unique_id():
    buf = C.create_string_buffer(128)
    L = load_hip()
    if L.poro_comm_unique_id(buf) != 0:
        raise RuntimeError(L.poro_last_error().decode())
    return buf.raw


def _hand_gravity(problem, gravity, fluid_density, density, hydrostatic_init):
    """the gravity arguments of run_problem / Runner -> Problem.set_gravity / set_cell_density on `problem`, which keeps them; nothing given: nothing touched"""
    if gravity is None and fluid_density is None and density is None and not hydrostatic_init:
        return
    g0, rho_f0, _, _ = problem.gravity()
    scalar = density is not None and np.ndim(density) == 0
    problem.set_gravity(g0 if gravity is None else gravity, rho_f0 if fluid_density is None else fluid_density, float(density) if scalar else None, hydrostatic_init)
    if density is not None and not scalar:
        problem.set_cell_density(density)


def _run_options(kw):
    """the RunOptions of a run from the keyword arguments of run_problem / Runner (their locals()); every value goes through as given"""
    return RunOptions(
        p_init=kw["p_init"], time_step=kw["dt"], n_steps=kw.get("n_steps", 1), fss_tol=kw["fss_tol"], pressure_tol=kw["pressure_tol"], max_fss_iterations=kw["max_fss"],
        max_pressure_iterations=kw["max_pres"], abs_tol_u=kw["abs_u"], rel_tol_u=kw["rel_u"], max_iter=kw["max_it"], preconditioner=kw["prec"],
        stop_rule_u=STOP_REDUCTION if kw["reduction"] else STOP_RHS,
        preconditioner_p=PREC_TWO_LEVEL if kw["two_level_p"] else PREC_JACOBI if kw["jacobi_p"] else -1,      # -1: the strongest form the mesh supports
        chebyshev_degree=int(kw["cheb_degree"]), chebyshev_ratio=kw["cheb_ratio"],
        refine_every=int(kw.get("refine_every") or 0), refine_fraction=kw.get("refine_fraction", 0.6), coarsen_fraction=kw.get("coarsen_fraction", 0.4),
        **{n: bool(kw[n]) for n in ("coupled_fss", "incremental_strain", "atomic_scatter", "fdm_fp32", "hybrid_operator", "fdm_per_direction", "moduli_structured")})


def run_problem(problem, n_steps, p_init, dt, device=0, operator_mode=OP_CSR, fss_tol=1e-8, pressure_tol=1e-8, max_fss=50, max_pres=50,
                abs_u=1e-12, rel_u=0.0, max_it=1000, prec=PREC_JACOBI, coupled_fss=False, incremental_strain=False, reduction=False, cheb_degree=0, cheb_ratio=0, jacobi_p=False, two_level_p=False,
                atomic_scatter=False, fdm_fp32=False, hybrid_operator=False, fdm_per_direction=False, refine_every=None, refine_fraction=0.6, coarsen_fraction=0.4, permeability=None, permeability_tensor=None,
                moduli_structured=False, gravity=None, fluid_density=None, density=None, hydrostatic_init=False):
    """PoroElasticProblem<dim>::run() (PoroelasticityFSS.h:294-415) through the C++ host driver; returns (trace, Context).
    refine_every = N (not None) goes through the adaptive entry: refine_mesh every N-th step (:333-340; 0 = never) on a mask- or block-refined box; the returned
    Context then belongs to the mesh the run ended on (Context.problem, a new Problem the caller closes when the mesh was refined at least once).
    hybrid_operator=True: OPFORM_HYBRID on refined boxes (carried over to every adapted mesh; a no-op on box-tagged meshes, an error where the mesh cannot take it).
    fdm_per_direction=True: FDM_FORM_PER_DIRECTION for the block FDM of the displacement system (Context.set_fdm_form; carried over to every adapted mesh).
    moduli_structured=True: MODULI_OP_STRUCTURED for the displacement operator (Context.set_moduli_operator; requested on every adapted mesh, where it has no effect:
    a refined mesh has no box tag).
    permeability: per-cell k / mu (Problem.set_cell_permeability on `problem`, which keeps it), carried over to every adapted mesh.
    permeability_tensor: per-cell diag(kx, ky[, kz]) / mu, shape (n_cells, dim) (Problem.set_cell_permeability_tensor), likewise.
    gravity: the vector g (Problem.set_gravity on `problem`, which keeps it); fluid_density: rho_f of the Darcy gravity flux; density: the bulk density, one scalar or one
    value per cell (Problem.set_cell_density); hydrostatic_init: start from p_init + rho_f g . (x - x_top) instead of the uniform p_init.  Carried to every adapted mesh."""
    H = load_host()
    opts = _run_options(locals())
    _hand_gravity(problem, gravity, fluid_density, density, hydrostatic_init)
    if permeability is not None:
        problem.set_cell_permeability(permeability)
    if permeability_tensor is not None:
        problem.set_cell_permeability_tensor(permeability_tensor)
    max_rows = 1 + n_steps * max_fss
    trace = np.zeros((max_rows, 8))
    ctx = C.c_void_p()
    if refine_every is not None:
        last = C.c_void_p()
        rows = H.poro_host_run_adaptive(problem.handle, device, operator_mode, C.byref(opts), trace.ctypes.data_as(_dp), max_rows, C.byref(ctx), C.byref(last))
        if rows < 0:
            raise RuntimeError(H.poro_host_last_error().decode())
        return trace[:rows], Context(Problem(last.value) if last.value else problem, ptr=ctx)
    rows = H.poro_host_run(problem.handle, device, operator_mode, C.byref(opts), trace.ctypes.data_as(_dp), max_rows, C.byref(ctx))
    if rows < 0:
        raise RuntimeError(H.poro_host_last_error().decode())
    return trace[:rows], Context(problem, ptr=ctx)


WORK_FIELDS = ("apply_u", "apply_p", "asm_rhs_u", "asm_matrix_u", "residual_p", "jacobian_p", "proj_rhs", "cg_u", "cg_p", "cg_proj", "usec_solve_u")


class Runner:
    """Steppable PoroElasticProblem<dim> (C++ host driver): initialize() = PoroelasticityFSS.h:308-317, step() = one pass of :328-407."""

    def __init__(self, problem, device=0, operator_mode=OP_MATRIX_FREE, p_init=10e6, dt=60.0, fss_tol=1e-8, pressure_tol=1e-8, max_fss=50, max_pres=50,
                 abs_u=1e-12, rel_u=0.0, max_it=1000, prec=PREC_JACOBI, coupled_fss=False, incremental_strain=False, reduction=False, cheb_degree=0, cheb_ratio=0, jacobi_p=False, two_level_p=False,
                 atomic_scatter=False, fdm_fp32=False, hybrid_operator=False, fdm_per_direction=False, permeability=None, permeability_tensor=None, moduli_structured=False,
                 gravity=None, fluid_density=None, density=None, hydrostatic_init=False):
        self.H = load_host()
        opts = _run_options(locals())
        _hand_gravity(problem, gravity, fluid_density, density, hydrostatic_init)      # Problem.set_gravity / set_cell_density on `problem`, which keeps them; adapt() carries them to every new mesh
        if permeability_tensor is not None:      # per-cell diag(kx, ky[, kz]) / mu, shape (n_cells, dim): Problem.set_cell_permeability_tensor, kept and carried like the scalar field
            problem.set_cell_permeability_tensor(permeability_tensor)
        if permeability is not None:             # per-cell k / mu: Problem.set_cell_permeability on `problem`, which keeps it; adapt() carries it to every new mesh
            problem.set_cell_permeability(permeability)
        self.max_fss = max_fss
        h = self.H.poro_host_runner_create(problem.handle, device, operator_mode, C.byref(opts))
        if not h:
            raise RuntimeError(self.H.poro_host_last_error().decode())
        self.h = C.c_void_p(h)
        self.problem = problem
        self.ctx = Context(problem, ptr=C.c_void_p(self.H.poro_host_runner_ctx(self.h)))

    def initialize(self):
        if self.H.poro_host_runner_initialize(self.h) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def step(self, restore=False):
        """one time step; restore=True: roll the device state back to the snapshot first (same call)"""
        trace = np.zeros((self.max_fss, 8))
        work = (C.c_int64 * 11)()
        rows = (self.H.poro_host_runner_restore_and_step if restore else self.H.poro_host_runner_step)(self.h, trace.ctypes.data_as(_dp), self.max_fss, work)
        if rows < 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())
        return trace[:rows], dict(zip(WORK_FIELDS, list(work)))

    def adapt(self, refine_fraction=0.6, coarsen_fraction=0.4):
        """refine_mesh (PoroelasticityFSS.h:447-498) + the re-assembly of :338-339 between two steps: estimate, mark, new mesh, new context, transfer.  Returns the
        cell counts (before, after); .problem / .ctx then refer to the new mesh, which the runner owns and frees (the problem handed to the constructor stays the caller's).
        Prescribed pressures (Problem.set_pressure_bc) are carried to every new mesh and re-imposed on the transferred pressure, which is conforming afterwards;
        the preconditioners are chosen again for the new context"""
        cells = (C.c_int64 * 2)()
        if self.H.poro_host_runner_adapt(self.h, refine_fraction, coarsen_fraction, cells) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())
        self.ctx.ptr = None                      # destroyed by the runner
        self.problem = Problem(self.H.poro_host_runner_problem(self.h), owned=False)
        self.ctx = Context(self.problem, ptr=C.c_void_p(self.H.poro_host_runner_ctx(self.h)))
        return cells[0], cells[1]

    def save_state(self):
        """device-side snapshot of every solver vector (and the step counter)"""
        if self.H.poro_host_runner_state(self.h, 0) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def restore_state(self):
        if self.H.poro_host_runner_state(self.h, 1) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def postprocess(self, output_dir=None, corrected=False, darcy=False, stress=False, cohesion=None, friction_angle=None):
        """PoroelasticityFSS.h:409-411: shear strains, effective stresses (PORO_VEC_STRESS0+e) and, with a directory, solution-NNNN.vtk; darcy=True appends the Darcy
        velocity per cell (CELL_DATA / VECTORS darcy_velocity) to the file; stress=True appends behind it the cell stresses and two failure measures (TENSORS
        effective_stress, TENSORS total_stress, SCALARS mohr_coulomb - with cohesion and friction_angle in radians, 0 without - and SCALARS von_mises)"""
        d = output_dir.encode() if output_dir else None
        if stress:
            if (cohesion is None) != (friction_angle is None):
                raise ValueError("postprocess: give both cohesion and friction_angle, or neither")
            rc = self.H.poro_host_runner_mohr_coulomb(self.h, int(cohesion is not None), float(cohesion or 0.0), float(friction_angle or 0.0))
            if rc == 0:
                rc = self.H.poro_host_runner_postprocess_fields(self.h, d, int(corrected), int(darcy), 1)
        else:
            rc = self.H.poro_host_runner_postprocess_darcy(self.h, d, int(corrected), 1) if darcy else self.H.poro_host_runner_postprocess(self.h, d, int(corrected))
        if rc < 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def cell_stress(self):
        """(strain, effective, total) per cell of the present state (Context.cell_stress)"""
        return self.ctx.cell_stress()

    def cell_measures(self, cohesion=None, friction_angle=None):
        """(measures [n_cells][6], summary) of the present effective stress (Context.cell_measures)"""
        return self.ctx.cell_measures(cohesion=cohesion, friction_angle=friction_angle)

    def track_force_balance(self, on=True):
        """while on, every step() appends its force balance to the records force_balance() returns under `history`; initialize() clears them"""
        if self.H.poro_host_runner_track_force(self.h, int(bool(on))) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def force_balance(self):
        """The force balance of the present state (Context.force_balance: the terms per component, reaction_dof, reaction_by_label[(label, component)]) and `history`:
        one dict of the terms per step taken since track_force_balance()"""
        res = self.ctx.force_balance()
        n = self.H.poro_host_runner_force_history(self.h, 0, None)
        if n < 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())
        dim, hist = self.ctx.dim, []
        for s in range(n):
            t = np.zeros(16)
            if self.H.poro_host_runner_force_history(self.h, s, t.ctypes.data_as(_dp)) < 0:
                raise RuntimeError(self.H.poro_host_last_error().decode())
            rec = {name: t[3 * i:3 * i + dim].copy() for i, name in enumerate(("reaction_sum", "free_row_sum", "traction_sum", "body_sum", "coupling_sum"))}
            rec["residual_l2"] = float(t[15])
            hist.append(rec)
        res["history"] = hist
        return res

    def darcy_velocity(self):
        """q_c = -kappa_c (grad p_h(x_c) - rho_f g) of the present pressure, [n_cells][dim] (Context.darcy_velocity)"""
        return self.ctx.darcy_velocity()

    def track_flow_balance(self, on=True):
        """while on, every step() adds dt * the terms of its fluid balance to the cumulative volumes flow_balance() reports; initialize() resets them, adapt() keeps them"""
        if self.H.poro_host_runner_track_flow(self.h, int(bool(on))) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def flow_balance(self):
        """The discrete fluid balance of the present state (include/poroel_hip.h, poro_pres_flow_balance): the six terms; `labels` = the prescribed-pressure labels;
        outflow_by_label = the conservative discharge C^T(-r) summed over the dofs each label prescribed; discharge_by_label = the face integrals of q . n;
        `cumulative` = the time integrals over the steps taken since track_flow_balance(): steps, storage_strain, storage_pressure, source (injected volume, negative
        for an injecting well), outflow, free_rows, bound (sum of dt sqrt(n_dofs_p) residual_l2), outflow_by_label, discharge_by_label"""
        cap = 64
        terms = np.zeros(6); totals = np.zeros(8)
        labels = np.zeros(cap, dtype=np.int32); out, dis, tout, tdis = (np.zeros(cap) for _ in range(4))
        n = self.H.poro_host_runner_flow_balance(self.h, terms.ctypes.data_as(_dp), labels.ctypes.data_as(_ip), out.ctypes.data_as(_dp), dis.ctypes.data_as(_dp), cap,
                                                 totals.ctypes.data_as(_dp), tout.ctypes.data_as(_dp), tdis.ctypes.data_as(_dp))
        if n < 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())
        res = dict(zip([f[0] for f in FlowBalanceTerms._fields_], terms.tolist()))
        lab = [int(l) for l in labels[:n]]
        res.update(labels=lab, outflow_by_label=dict(zip(lab, out[:n].tolist())), discharge_by_label=dict(zip(lab, dis[:n].tolist())))
        nt = int(totals[7])
        res["cumulative"] = dict(steps=int(totals[0]), storage_strain=totals[1], storage_pressure=totals[2], source=totals[3], outflow=totals[4], free_rows=totals[5], bound=totals[6],
                                 outflow_by_label=dict(zip(lab[:nt], tout[:nt].tolist())), discharge_by_label=dict(zip(lab[:nt], tdis[:nt].tolist())))
        return res

    def preconditioners(self):
        """(displacement, pressure, projection): the PREC_* the driver chose for the current context (made in initialize(), and again after every adapt())"""
        out = (C.c_int32 * 3)()
        self.H.poro_host_runner_preconditioners(self.h, out)
        return tuple(out)

    def set_pressure_solver_tolerances(self, abs_tol=0.0, rel_tol=1e-8):
        """the stopping rule of the pressure solve, ||g|| <= max(abs_tol, rel_tol ||R||) (the reference's: 0, 1e-8); kept over initialize() and adapt()"""
        if self.H.poro_host_runner_pressure_solver_tolerances(self.h, abs_tol, rel_tol) != 0:
            raise RuntimeError(self.H.poro_host_last_error().decode())

    def work(self):
        """cumulative work counters since creation"""
        work = (C.c_int64 * 11)()
        self.H.poro_host_runner_work(self.h, work)
        return dict(zip(WORK_FIELDS, list(work)))

    def close(self):
        if self.h:
            self.ctx.ptr = None          # owned by the runner
            self.H.poro_host_runner_free(self.h)
            self.h = None

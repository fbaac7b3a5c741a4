"""Prescribed pressures on the fast-diagonalisation path (uniform boxes and tensor-product grids, one rank).

Where the prescribed set is a union of whole faces, deleting those rows and columns from a M + kappa K leaves a Kronecker sum of 1D matrices without their end nodes, which
has its own exact fast diagonalisation (the second table set, ctx_prec.hip: build_fdm_q1).  Checked here: the exact inverse against a sparse direct solve of the deleted
system, the direct path (no CG iteration) on matrix-free boxes, CG + FDM on tensor grids and CSR contexts, the projection's untouched direct solve, the support queries,
Terzaghi's column end to end, the CLI, and that contexts without prescribed pressures compute what they computed before (stored results of the previous code).

Bounds: rel2 <= 1e-9 against the reference solution and final <= 1e-12 x initial residual are those of test_parity_gpu.py::test_fast_diagonalisation_preconditioner for the
unconstrained case; the run-to-run bounds 1e-8 on p and u are those of test_terzaghi.py::test_device_follows_the_oracle_with_prescribed_pressures; 0.02 against the
analytic series is test_terzaghi.py::test_device_consolidation_matches_terzaghi's."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import GOLDEN, INPUT_DATA, csr_to_scipy, material

pytestmark = pytest.mark.gpu
DT = 60.0
EXE = os.path.join(os.path.dirname(GOLDEN), os.pardir, "poroelasticity_dealii_amd", "lib", "poro_run")
STORED = os.path.join(GOLDEN, "pressure_bc_fdm")


def rel2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def rollers(dim):
    return [(2 * d, d, 0.0) for d in range(dim)]


def box(n, pbc, size=None):
    dim = len(n)
    P = pk.Problem.box(dim, list(n), size or [float(m) for m in n], 1, material(), rollers(dim))     # cells of edge 1: a M and kappa K of comparable size
    return P.set_pressure_bc(pbc) if pbc else P


def graded(n, pbc):
    P = pk.Problem.graded_box(3, list(n), [float(m) for m in n], 1, material(), rollers(3), [0.6, 0.0, 0.9])
    return P.set_pressure_bc(pbc) if pbc else P


def prescribed(P):
    n = P.desc.n_dirichlet_p
    return P.array("dirichlet_dof_p", (n,), np.int32), P.array("dirichlet_value_p", (n,))


def rhs_for(n_p):
    return np.random.default_rng(1234 + n_p).standard_normal(n_p)          # non-zero on the prescribed rows as well


_reference = {}


def reference(key, P):
    """(a M + kappa K) with the prescribed rows and columns deleted, solved by a sparse direct method; M and K from a CSR context of the same problem.  Computed once per case"""
    if key not in _reference:
        import scipy.sparse.linalg as spla
        C = pk.Context(P, 0, pk.OP_CSR)
        try:
            M = csr_to_scipy(*C.export_csr(pk.MAT_MASS_P)); K = csr_to_scipy(*C.export_csr(pk.MAT_LAPLACE_P))
        finally:
            C.close()
        m = material()
        J = (M / (m.biot_M * DT) + m.k_over_mu * K).tocsc()
        dofs, _ = prescribed(P)
        free = np.setdiff1d(np.arange(P.desc.n_dofs_p), dofs)
        b = rhs_for(P.desc.n_dofs_p)
        x = np.zeros(P.desc.n_dofs_p)
        x[free] = spla.spsolve(J[free][:, free], b[free])
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def fdm_solve(G, b, **kw):
    G.set(pk.VEC_RESIDUAL_P, b)
    G.fill(pk.VEC_DP, 0.0)
    G.pres_assemble_jacobian(DT)
    rc, info = G.pres_solve(rel_tol=1e-8, prec=pk.PREC_FDM, **kw)
    return rc, info, G.get(pk.VEC_DP)


# (id, builder, cells, prescribed faces, direct solve expected on the matrix-free context)
CASES = {
    "box-2x3x5-top": (box, (2, 3, 5), [(5, 0.0)]),                      # one-sided; every line has a different length
    "box-4x4x17-both-z": (box, (4, 4, 17), [(4, 0.0), (5, 0.0)]),       # 18 nodes, 16 free: the 16-row MFMA tile boundary of the fused kernel
    "box-17x3x3-low-x": (box, (17, 3, 3), [(0, 0.0)]),                  # 17 free
    "box-2x2x82-top": (box, (2, 2, 82), [(5, 0.0)]),                    # 83 nodes > the fused kernel's 80: the six-launch form
    "box-5x7-2d": (box, (5, 7), [(1, 0.0), (2, 0.0), (3, 0.0)]),        # the 2D form: one side of x, both sides of y
    "graded-3x4x6-top": (graded, (3, 4, 6), [(5, 0.0)]),                # non-uniform 1D matrices; CG with FDM instead of the direct path
    "box-2x3x5-two-values": (box, (2, 3, 5), [(4, 2e5), (5, 0.0)]),     # different values per face
}


@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_exact_inverse_of_the_free_block(case):
    build, n, pbc = CASES[case]
    P = build(n, pbc)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(1, pk.PREC_FDM)
        assert not G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)
        dofs, vals = prescribed(P)
        assert len(dofs) > 0
        b = rhs_for(G.n_p)
        assert np.all(b[dofs] != 0.0)
        x0 = reference(case, P)
        G.timers_reset()
        rc, info, x = fdm_solve(G, b)
        print(f"{case}: iterations {info.iterations} residual {info.final_residual:.3e} / {info.initial_residual:.3e} rel2 {rel2(x, x0):.3e}")
        assert rc == 0 and info.converged == 1
        assert np.all(x[dofs] == 0.0)                                       # exactly: p keeps the values poro_pres_apply_boundary_values wrote
        assert info.final_residual <= 1e-12 * info.initial_residual
        assert rel2(x, x0) <= 1e-9
        assert G.timer("fdm_pj_build")[1] == 1 and G.timer("precondition_p_fdm_fixed_ends")[1] >= 1
        if build is box:
            assert info.iterations == 0                                     # the direct path: no CG iteration
        else:
            assert 1 <= info.iterations <= 2
        if case == "box-2x3x5-two-values":
            # one full Newton step: the values written by apply_boundary_values survive it
            p = 1e5 * (1 + 0.1 * np.sin(0.37 * np.arange(G.n_p)))
            G.set(pk.VEC_P, p); G.pres_apply_boundary_values(); G.copy(pk.VEC_P_OLD, pk.VEC_P)
            G.set(pk.VEC_P, 1.01 * p); G.pres_apply_boundary_values()
            G.pres_assemble_residual(DT); G.pres_assemble_jacobian(DT)
            G.fill(pk.VEC_DP, 0.0)
            rc, info = G.pres_solve(rel_tol=1e-8, prec=pk.PREC_FDM)
            assert rc == 0 and info.iterations == 0 and info.converged == 1
            G.axpy(pk.VEC_P, 1.0, pk.VEC_DP)
            pn = G.get(pk.VEC_P)
            assert set(vals) == {0.0, 2e5} and np.array_equal(pn[dofs], vals)
            assert G.pres_assemble_residual(DT) <= 1e-12 * info.initial_residual          # the step solved the (linear) free-row system
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("kind", ["graded-matrix-free", "graded-csr", "box-csr"])
def test_cg_with_fdm_needs_no_more_iterations_than_without_prescribed_pressures(kind):
    """tensor grids and CSR contexts have no direct path: CG preconditioned by the exact inverse of the free block"""
    build, n = (graded, (3, 4, 6)) if kind.startswith("graded") else (box, (2, 3, 5))
    mode = pk.OP_MATRIX_FREE if kind.endswith("matrix-free") else pk.OP_CSR
    its = {}
    for name, pbc in (("free", None), ("drained", [(5, 0.0)])):
        P = build(n, pbc)
        G = pk.Context(P, 0, mode)
        try:
            assert G.supports_preconditioner(1, pk.PREC_FDM)
            b = rhs_for(G.n_p)
            rc, info, x = fdm_solve(G, b)
            assert rc == 0 and info.converged == 1 and info.iterations >= 1
            its[name] = info.iterations
            if pbc:
                dofs, _ = prescribed(P)
                assert np.all(x[dofs] == 0.0)
                assert info.final_residual <= 1e-12 * info.initial_residual
                assert rel2(x, reference("cg-" + kind.split("-")[0], P)) <= 1e-9
        finally:
            G.close(); P.close()
    print(kind, its)
    assert its["drained"] <= its["free"] + 1, its


def test_projection_keeps_its_direct_solve():
    """the projection's mass matrix has no prescribed rows: same tables, same batched direct solve, same strains as without the pressure condition"""
    strains = {}
    for name, pbc in (("free", None), ("drained", [(4, 0.0), (5, 0.0)])):
        P = box((4, 4, 17), pbc)
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        try:
            assert G.supports_preconditioner(2, pk.PREC_FDM)
            G.set(pk.VEC_U, 1e-5 * np.sin(0.05 * np.arange(G.n_u)))
            G.proj_assemble_matrix(); G.proj_assemble_rhs([0, 4, 8])
            G.timers_reset()
            rc, infos = G.proj_solve_many([0, 3, 5], rel_tol=1e-8, prec=pk.PREC_FDM)
            assert rc == 0 and [i.iterations for i in infos] == [0, 0, 0] and all(i.converged for i in infos)
            assert G.timer("fdm_pj_build")[1] == 0                          # the mass matrix never uses the second table set
            strains[name] = [G.get(pk.VEC_STRAIN0 + e) for e in (0, 3, 5)]
        finally:
            G.close(); P.close()
    for a, b in zip(strains["drained"], strains["free"]):
        assert rel2(a, b) <= 1e-9


def test_support_queries_and_refusals():
    P = box((2, 3, 5), [(5, 0.0)])
    try:
        for mode in (pk.OP_MATRIX_FREE, pk.OP_CSR):
            G = pk.Context(P, 0, mode)
            assert G.supports_preconditioner(1, pk.PREC_FDM) and G.supports_preconditioner(1, pk.PREC_JACOBI) and G.supports_preconditioner(2, pk.PREC_FDM)
            assert not G.supports_preconditioner(1, pk.PREC_TWO_LEVEL) and not G.supports_preconditioner(1, pk.PREC_ILU0)
            G.close()
        # one node of the face left out of the list: not a union of whole faces any more
        n_full = P.desc.n_dirichlet_p
        P.desc.n_dirichlet_p = n_full - 1
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        try:
            assert not G.supports_preconditioner(1, pk.PREC_FDM)
            assert G.supports_preconditioner(2, pk.PREC_FDM)                # the projection is not affected
            G.set(pk.VEC_RESIDUAL_P, rhs_for(G.n_p)); G.pres_assemble_jacobian(DT)
            with pytest.raises(RuntimeError, match="meshes with hanging-node constraints or prescribed pressures"):
                G.pres_solve(prec=pk.PREC_FDM)
            rc, info = G.pres_solve(rel_tol=1e-10, prec=pk.PREC_JACOBI)       # today's path still solves it
            assert rc == 0 and info.iterations > 0
        finally:
            G.close()
            P.desc.n_dirichlet_p = n_full
    finally:
        P.close()
    P = graded((3, 4, 6), [(5, 0.0)])
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(1, pk.PREC_FDM) and not G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)
        G.set(pk.VEC_RESIDUAL_P, rhs_for(G.n_p)); G.pres_assemble_jacobian(DT)
        with pytest.raises(RuntimeError, match="meshes with hanging-node constraints or prescribed pressures"):
            G.pres_solve(prec=pk.PREC_TWO_LEVEL)
    finally:
        G.close(); P.close()


# ---- Terzaghi's column (tests/test_terzaghi.py) with the automatic pressure choice against jacobi_p -------------------------------------------------
H, SIGMA0 = 10.0, 1.0e6
KW = dict(fss_tol=1e-11, pressure_tol=1e-11, max_fss=200, max_it=50000)


def column(dim, ny, deg, nx=2):
    n = [nx] * (dim - 1) + [ny]
    last = dim - 1
    bc = [(2 * d, d, 0.0) for d in range(dim - 1)] + [(2 * d + 1, d, 0.0) for d in range(dim - 1)] + [(2 * last, last, 0.0)]
    m = material(flow_rate=0.0)
    P = pk.Problem.box(dim, n, [10.0] * (dim - 1) + [H], deg, m, bc, [(2 * last + 1, last, -SIGMA0)])
    P.set_pressure_bc([(2 * last + 1, 0.0)])
    return P, m


def analytic(m, depth, t):
    Kv = m.lame_lambda + 2 * m.shear_G
    s = m.biot_alpha ** 2 / Kv + 1.0 / m.biot_M
    p0 = (m.biot_alpha * SIGMA0 / Kv) / s; cv = m.k_over_mu / s
    out = np.zeros_like(depth)
    for k in range(400):
        a = (2 * k + 1) * np.pi / (2 * H)
        out += 4 * p0 / np.pi / (2 * k + 1) * np.sin(a * depth) * np.exp(-a * a * cv * t)
    return out, p0, cv


def profile(P, p, dim):
    X = np.ctypeslib.as_array(P.desc.vertex_coords, shape=(P.desc.n_vertices, dim))
    line = np.all(np.abs(X[:, :dim - 1] - X[0, :dim - 1]) < 1e-12, axis=1)
    return H / 2 - X[line, dim - 1], p[line]


@pytest.mark.parametrize("dim,ny,deg", [(2, 20, 2), (3, 8, 1)], ids=str)
def test_terzaghi_with_the_automatic_pressure_choice(dim, ny, deg):
    """The drained column with FDM chosen for the pressure system (direct solves) and with Jacobi-CG forced: the same fixed-stress history, the same fields.
    Measured error against the series at t = 600 s, dt = 30 s: 2D ny = 20 Q2 and 3D ny = 8 Q1 both below the existing test's 0.02 (figures in the PR's summary)."""
    P, m = column(dim, ny, deg)
    _, p0, _ = analytic(m, np.zeros(1), 0.0)
    steps, dt = 20, 30.0
    out = {}
    try:
        for name, jp in (("auto", False), ("jacobi", True)):
            tr, G = pk.run_problem(P, steps, p0, dt, operator_mode=pk.OP_MATRIX_FREE, prec=pk.PREC_CHEBYSHEV, jacobi_p=jp, coupled_fss=True, incremental_strain=True, **KW)
            out[name] = (tr, G.get(pk.VEC_P), G.get(pk.VEC_U))
            assert G.supports_preconditioner(1, pk.PREC_FDM)
            G.close()
        (ta, pa, ua), (tj, pj, uj) = out["auto"], out["jacobi"]
        depth, pn = profile(P, pa, dim)
        e = np.abs(pn - analytic(m, depth, steps * dt)[0]).max() / p0
        print(f"terzaghi {dim}d ny={ny} Q{deg}: error {e:.3e}, rows {len(ta)}, pressure CG iterations auto {int(ta[1:, 7].sum())} jacobi {int(tj[1:, 7].sum())}, "
              f"|dp| {np.abs(pa - pj).max() / np.abs(pj).max():.2e} |du| {np.linalg.norm(ua - uj) / np.linalg.norm(uj):.2e}")
        assert len(ta) == len(tj) and np.array_equal(ta[:, :3], tj[:, :3])           # fixed-stress and pressure iteration counts per step
        assert np.abs(pa - pj).max() <= 1e-8 * np.abs(pj).max()
        assert np.linalg.norm(ua - uj) <= 1e-8 * np.linalg.norm(uj)
        assert e < 0.02
        assert ta[1:, 7].sum() == 0 and tj[1:, 7].sum() > 0                         # every pressure solve of the automatic path was direct
    finally:
        P.close()


def test_cli_runs_a_drained_box():
    base = [EXE, INPUT_DATA, "--matrix-free", "--fastest", "--steps", "1"]
    r = subprocess.run(base + ["--pressure-bc", "3=0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"prescribed pressures: 17 dofs; pressure preconditioner: FDM, projection preconditioner: FDM", r.stdout), r.stdout[-500:]
    q = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and "prescribed" not in q.stdout and "preconditioner" not in q.stdout
    assert re.findall(r"pressure converged; iterations: (\d+)", q.stdout) and q.stdout.startswith("starting time loop\ntime max ")


# ---- nothing else moved -----------------------------------------------------------------------------------------------------------------------------
STORED_CASES = {"3d-matrix-free": ((4, 3, 5), pk.OP_MATRIX_FREE), "2d-matrix-free": ((5, 7), pk.OP_MATRIX_FREE), "3d-csr": ((4, 3, 5), pk.OP_CSR)}


def stored_case_solve(name):
    """pres_solve(PREC_FDM) on a box WITHOUT prescribed pressures (direct on matrix-free contexts, CG on CSR); tools of the stored results below"""
    n, mode = STORED_CASES[name]
    P = box(n, None)
    G = pk.Context(P, 0, mode)
    try:
        G.timers_reset()
        rc, info, x = fdm_solve(G, rhs_for(G.n_p))
        return rc, info.iterations, x, G.timer("fdm_pj_build")[1], G.timer("precondition_p_fdm_fixed_ends")[1]
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("name", list(STORED_CASES), ids=str)
def test_boxes_without_prescribed_pressures_compute_what_they_did(name):
    """bitwise equal to the results recorded from the code before the second table set existed (tests/golden/pressure_bc_fdm/*.npy), which is never built here"""
    rc, its, x, builds, fixed_applies = stored_case_solve(name)
    want = np.load(os.path.join(STORED, name + ".npy"))
    assert rc == 0 and builds == 0 and fixed_applies == 0
    assert its == int(want[0])
    assert np.array_equal(x, want[1:])

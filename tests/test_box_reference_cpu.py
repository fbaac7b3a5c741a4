"""The Kronecker-product reference of tests/box_reference.py against the CPU oracle (no GPU): every operator, the right-hand sides, the exact block
inverse and the restated CG recurrence, on small uniform, anisotropic, thin and graded boxes, Q1 and Q2, 2D and 3D, with face-wise and mixed Dirichlet
lists.  Once these hold, the reference stands in for the oracle at the benchmark sizes the oracle cannot reach (tests/test_box_reference_gpu.py)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import poroelasticity_dealii_amd as pk
import oracle_py
from box_reference import BoxReference, reference_pcg
from common import BC_2D, BC_3D, REF, box_problem, csr_to_scipy, material

MIXED_3D = [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (3, 1, -1e-5), (4, 2, 0.0), (2, 0, 2e-6), (5, 1, 0.0)]     # as tests/test_fdm_u_gpu.py
MIXED_2D = [(0, 0, 0.0), (2, 1, 0.0), (3, 0, 1e-6)]

# (dim, cells, degree, Dirichlet list, grading or None)
CASES = [(3, (4, 4, 4), 2, BC_3D, None), (3, (4, 3, 5), 1, BC_3D, None), (3, (9, 2, 3), 2, BC_3D, None), (3, (3, 4, 2), 2, MIXED_3D, None),
         (3, (5, 3, 4), 1, MIXED_3D, None), (2, (6, 5), 2, BC_2D, None), (2, (7, 4), 1, MIXED_2D, None), (2, (9, 2), 2, BC_2D, None),
         (3, (4, 3, 5), 2, BC_3D, (1.0, 0.5, -0.7)), (3, (5, 4, 3), 1, MIXED_3D, (0.8, 0.0, 1.2)), (2, (6, 4), 2, BC_2D, (1.5, -0.6))]
IDS = [f"{d}d-{'x'.join(map(str, n))}-q{k}-bc{len(bc)}" + ("-graded" if gr else "") for d, n, k, bc, gr in CASES]


def make(dim, n, deg, bc, grading):
    if grading is None:
        return box_problem(dim, n, deg, bc=bc)
    return pk.Problem.graded_box(dim, list(n), [10.0] * dim, deg, material(), bc, list(grading))


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(params=CASES, ids=IDS)
def case(request):
    P = make(*request.param)
    O = oracle_py.Oracle(P, hoisted=True)
    R = BoxReference(P)
    yield P, O, R
    O.close(); P.close()


def test_displacement_operator_diagonal_and_rhs(case):
    P, O, R = case
    p = REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(R.n_p)))
    O.set(pk.VEC_P, p); O.disp_assemble_system(True)
    A = csr_to_scipy(*O.export_csr(pk.MAT_A_U))
    rng = np.random.default_rng(3)
    for x in (rng.standard_normal(R.n_u), np.sin(0.37 * np.arange(R.n_u))):
        y0 = O.apply(pk.MAT_A_U, x)
        assert rel(R.apply_A(x), y0) <= 1e-13
        assert rel(R.apply_A(x), A @ x) <= 1e-13
    assert rel(R.diag_A(), A.diagonal()) <= 1e-13
    b0 = O.get(pk.VEC_RHS_U)
    assert rel(R.rhs_u(p), b0) <= 1e-13
    assert np.all(b0[R.mask] == 0.0)


def test_pressure_and_projection_operators(case):
    P, O, R = case
    dt = REF["dt"]
    O.pres_assemble_jacobian(dt)
    x = np.cos(0.23 * np.arange(R.n_p)) + 0.1
    for which, f in ((pk.MAT_MASS_P, R.mass_p), (pk.MAT_LAPLACE_P, R.laplace_p), (pk.MAT_JACOBIAN_P, lambda v: R.jacobian_p(v, dt))):
        assert rel(f(x), O.apply(which, x)) <= 1e-13, which
        assert rel(f(x), csr_to_scipy(*O.export_csr(which)) @ x) <= 1e-13, which
    # projection right-hand sides of a non-polynomial displacement, every tensor entry (packed entry e <-> full index a*dim+b)
    u = np.sin(0.37 * np.arange(R.n_u)) * 1e-5
    O.set(pk.VEC_U, u)
    dim = R.dim
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    O.proj_assemble_rhs([a * dim + b for a, b in pairs])
    for a, b in pairs:
        e = a * dim + b - a * (a + 1) // 2          # packed symmetric entry (TensorIndexer: 2D 0,1,2 = xx,xy,yy; 3D 0..5 = xx,xy,xz,yy,yz,zz)
        assert rel(R.proj_rhs(u, a, b), O.get(pk.VEC_PROJ_RHS0 + e)) <= 1e-13, (a, b)


def test_exact_inverses_equal_sparse_direct_solves(case):
    P, O, R = case
    dt = REF["dt"]
    O.fill(pk.VEC_P, 0.0); O.disp_assemble_system(True); O.pres_assemble_jacobian(dt)
    A = csr_to_scipy(*O.export_csr(pk.MAT_A_U))
    rng = np.random.default_rng(11)
    g = rng.standard_normal(R.n_u) * 1e3; g[R.mask] = 0.0
    z0 = np.zeros_like(g)
    for c in range(R.dim):
        idx = np.arange(c, R.n_u, R.dim); idx = idx[~R.mask[idx]]
        z0[idx] = spla.splu(A[idx][:, idx].tocsc()).solve(g[idx])
    assert rel(R.block_inverse_u(g), z0) <= 1e-11
    r = rng.standard_normal(R.n_p)
    for which, f in ((pk.MAT_JACOBIAN_P, lambda v: R.jacobian_p_inverse(v, dt)), (pk.MAT_MASS_P, R.mass_p_inverse)):
        J = csr_to_scipy(*O.export_csr(which)).tocsc()
        assert rel(f(r), spla.splu(J).solve(r)) <= 1e-11, which


@pytest.mark.parametrize("reduction", [False, True], ids=["stop_rhs", "stop_reduction"])
def test_reference_pcg_reproduces_the_oracle_solve(case, reduction):
    """the restated recurrence with the oracle's own CSR and its Jacobi preconditioner: the oracle's iteration count, residuals and iterate.  Jacobi-CG
    needs 40 - 80 iterations here, and the different summation order of the dot products (BLAS against the oracle's loop) moves the recursive residual by
    ~3e-12 ||g_0|| over such a run (measured, 4x3x5 Q1 box): at a 1e-10 reduction that is a few % of ||g_final|| and flips the count near the threshold.
    The check therefore stops at a 1e-6 reduction.  The drift grows with the condition number: the 2D boxes with the mixed list (one face holds u_y)
    measured 5.7e-11 ||g_0|| (7x4 Q1), hence the residual bound 1e-9 ||g_0||; count and iterate are exact."""
    P, O, R = case
    p = REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(R.n_p)))
    O.set(pk.VEC_P, p); O.disp_assemble_system(True)
    A = csr_to_scipy(*O.export_csr(pk.MAT_A_U))
    b = O.get(pk.VEC_RHS_U)
    dinv = 1.0 / A.diagonal()
    rc, info = O.disp_solve(abs_tol=1e-14, rel_tol=1e-6, max_iter=5000, prec=oracle_py.PREC_JACOBI, reduction=reduction)
    x, its, hist, tol = reference_pcg(lambda v: A @ v, lambda v: dinv * v, b, np.zeros(R.n_u), 1e-14, 1e-6, 5000, int(reduction), inert=R.mask)
    assert rc == 0 and its == info.iterations, (its, info.iterations)
    assert abs(hist[0] - info.initial_residual) <= 1e-12 * info.initial_residual
    assert abs(hist[-1] - info.final_residual) <= 1e-9 * info.initial_residual, (hist[-1], info.final_residual, info.initial_residual)
    x[R.dir_dof] = R.dir_val                     # constraints.distribute
    u0 = O.get(pk.VEC_U)
    assert np.abs(x - u0).max() <= 1e-9 * np.abs(u0).max()
    # the reference operator with the exact block inverse converges to the oracle's tight solution
    O.fill(pk.VEC_U, 0.0)
    assert O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=5000, reduction=reduction)[0] == 0
    u1 = O.get(pk.VEC_U)
    xr, itr, _, _ = reference_pcg(R.apply_A, R.block_inverse_u, R.rhs_u(p), np.zeros(R.n_u), 1e-14, 1e-12, 500, int(reduction), inert=R.mask)
    xr[R.dir_dof] = R.dir_val
    assert np.abs(xr - u1).max() <= 1e-9 * np.abs(u1).max() and itr < 60, itr

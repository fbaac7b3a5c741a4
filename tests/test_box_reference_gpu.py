"""The box kernels against the Kronecker-product reference (tests/box_reference.py, itself checked against the oracle by test_box_reference_cpu.py) at the
benchmark sizes the oracle cannot reach: the operator, its diagonal and right-hand sides, the block fast diagonalisation against the exact block inverse
(octant, nodal and planar forms, tile and padding boundaries), the pressure / projection direct solves, and the fused PCG recurrence step by step
(iteration count, residuals, iterate).  The kernel variants behind environment switches run the same checks in child processes (the switches are read
once per process).

Tolerances, relative to the max of the reference: the operator and the diagonal 1e-12; the right-hand sides 1e-11 (the lifting -A g is a difference of
terms 1e3 x larger than the result near the loaded faces: 1e3 * eps * ~10 summands ~ 2e-12); the exact inverses 1e-10 (fp64 MFMA transforms of up to 257
points per line in three directions: 3 x 257 x eps ~ 2e-13 per transform, times the eigenvector conditioning)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":          # a child process of test_variant_switches: the repository root and the oracle on the path, as tests/conftest.py puts them
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]

import poroelasticity_dealii_amd as pk
from box_reference import BoxReference, reference_pcg
from common import BC_2D, BC_3D, REF, box_problem, material

pytestmark = pytest.mark.gpu

FULL = [(3, 72, 2), (3, 99, 1), (2, 336, 2)]     # BASELINE configs 4, 3, 2
BENCH_TOL = dict(abs_tol=1e-12, rel_tol=1e-8, reduction=True)      # bench.py defaults: --rel-tol 1e-8, --stop reduction, abs 1e-12
DT = REF["dt"]


def context(P):
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    if os.environ.get("PORO_FORCE_PARTITIONED_PATH"):            # the partitioned code path on one rank: RCCL as the communicator
        G.comm_rccl(pk.rccl_unique_id())
    return G


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def pressure(n_p):
    return REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(n_p)))


def spikes(R, c):
    """unit entries of component c at nodes 0, 1 and 2 layers in from every edge and corner of the box (their images under A do not overlap)"""
    x = np.zeros(R.shape_u)
    for idx in np.ndindex(*([3] * R.dim)):
        pos = []
        for a, i in enumerate(idx):
            n1 = R.shape_u[a]
            pos.append([0, n1 // 2, n1 - 1][i])
        off = sum(idx) % 3                                 # 0, 1 or 2 nodes in from the boundary, towards the middle
        pos = [p + off if p == 0 else p - off if p == R.shape_u[a] - 1 else p for a, p in enumerate(pos)]
        x[tuple(pos)] = 1.0
    f = [np.zeros(R.shape_u) for _ in range(R.dim)]
    f[c] = x
    return R.pack(f)


# ---- (a) operators at full size --------------------------------------------------------------------------------------------------------------------
def check_operator(dim, n, deg):
    P = box_problem(dim, n, deg)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        R = BoxReference(P)
        p = pressure(G.n_p)
        G.set(pk.VEC_P, p); G.disp_assemble_system(True)
        x = np.random.default_rng(5).standard_normal(G.n_u)
        assert (e := rel(G.apply(pk.MAT_A_U, x), R.apply_A(x))) <= 1e-12, ("random x", e)
        for c in range(dim):
            s = spikes(R, c)
            assert (e := rel(G.apply(pk.MAT_A_U, s), R.apply_A(s))) <= 1e-12, ("spikes", c, e)
        assert (e := rel(G.get(pk.VEC_DIAG_U), R.diag_A())) <= 1e-12, ("diag", e)
        b = R.rhs_u(p)
        assert (e := rel(G.get(pk.VEC_RHS_U), b)) <= 1e-11, ("rhs_u", e)
        # projection right-hand sides of a non-polynomial displacement, all tensor entries
        u = 1e-5 * np.sin(0.37 * np.arange(G.n_u))
        G.set(pk.VEC_U, u)
        pairs = [(a, bb) for a in range(dim) for bb in range(a, dim)]
        G.proj_assemble_matrix(); G.proj_assemble_rhs([a * dim + bb for a, bb in pairs])
        for a, bb in pairs:
            e_ = a * dim + bb - a * (a + 1) // 2
            assert (e := rel(G.get(pk.VEC_PROJ_RHS0 + e_), R.proj_rhs(u, a, bb))) <= 1e-11, ("proj rhs", a, bb, e)
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("dim,n,deg", FULL, ids=str)
def test_operator_diagonal_and_rhs_at_full_size(dim, n, deg):
    check_operator(dim, n, deg)


# ---- (b) block fast diagonalisation = exact block inverse -------------------------------------------------------------------------------------------
# Q2 3D: the headline; half lines h = n + 1 at 16-point tile boundaries (16/17, 32/33, 48/64/65, 80/81, 112/113); odd and even x half lines (hxp padding);
# h = 128 (largest octant case) and one cell above it (the octant form refuses it: nodal fallback).  Q1: config 3 and h = 128.  2D: config 2.
FDM_CASES = [(3, (72, 72, 72), 2), (3, (15, 16, 17), 2), (3, (31, 32, 33), 2), (3, (47, 63, 64), 2), (3, (79, 80, 3), 2), (3, (111, 112, 6), 2),
             (3, (16, 31, 5), 2), (3, (127, 3, 2), 2), (3, (128, 3, 2), 2), (3, (99, 99, 99), 1), (3, (254, 3, 4), 1), (2, (336, 336), 2)]
GRADED = (3, (20, 17, 12), 2, (1.0, 0.5, -0.7))


def check_block_fdm(dim, n, deg, grading=None, tol=1e-10):
    P = box_problem(dim, n, deg) if grading is None else pk.Problem.graded_box(dim, list(n), [10.0] * dim, deg, material(), BC_3D if dim == 3 else BC_2D, list(grading))
    G = context(P)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        R = BoxReference(P)
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        rng = np.random.default_rng(7)
        worst = 0.0
        for _ in range(2):                                  # twice: the second call reuses the built transforms
            g = rng.standard_normal(G.n_u) * 1e3; g[R.mask] = 0.0
            z = G.apply_preconditioner_u(pk.PREC_FDM, g)
            z0 = R.block_inverse_u(g)
            assert np.abs(z[R.mask]).max() == 0.0
            worst = max(worst, rel(z, z0))
        assert worst <= tol, (n, deg, worst)
        return worst
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("dim,n,deg", FDM_CASES, ids=str)
def test_block_fdm_equals_the_exact_block_inverse(dim, n, deg):
    check_block_fdm(dim, n, deg)


def test_block_fdm_on_a_graded_box_equals_the_exact_block_inverse():
    """tensor-product grid (no box tag): the 1D matrices come from the graded grids"""
    dim, n, deg, grading = GRADED
    check_block_fdm(dim, n, deg, grading)


# ---- (c) pressure and projection direct solves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(3, 72), (3, 99), (2, 336), (3, (9, 5, 2))], ids=str)   # the last: Q1 lines of 10 / 6 / 3 nodes = 3 / 2 / 1 MFMA k-steps in one tile, a direction mix-up truncates a contraction
def test_pressure_and_projection_fdm_solves_are_the_exact_inverses(dim, n):
    P = box_problem(dim, n, 1)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        R = BoxReference(P)
        assert G.supports_preconditioner(1, pk.PREC_FDM)
        i = np.arange(G.n_p)
        G.set(pk.VEC_P, pressure(G.n_p)); G.set(pk.VEC_P_OLD, REF["p_init"] * (1 + 0.1 * np.cos(0.21 * i)))
        G.set(pk.VEC_EPSV, 1e-6 * np.sin(0.13 * i)); G.fill(pk.VEC_EPSV0, 0.0)
        G.pres_assemble_residual(DT); G.pres_assemble_jacobian(DT)
        G.fill(pk.VEC_DP, 0.0)
        rc, info = G.pres_solve(prec=pk.PREC_FDM)
        assert rc == 0
        r = G.get(pk.VEC_RESIDUAL_P)
        assert (e := rel(G.get(pk.VEC_DP), R.jacobian_p_inverse(r, DT))) <= 1e-10, ("pressure", e)
        u = 1e-5 * np.sin(0.37 * np.arange(G.n_u)) + 1e-6 * np.cos(0.05 * np.arange(G.n_u))
        G.set(pk.VEC_U, u)
        ent = list(range(dim * (dim + 1) // 2))
        full = [a * dim + b for a in range(dim) for b in range(a, dim)]
        G.proj_assemble_matrix(); G.proj_assemble_rhs(full)
        rc, infos = G.proj_solve_many(ent, prec=pk.PREC_FDM)
        assert rc == 0
        for e_ in ent:
            assert (e := rel(G.get(pk.VEC_STRAIN0 + e_), R.mass_p_inverse(G.get(pk.VEC_PROJ_RHS0 + e_)))) <= 1e-10, ("projection", e_, e)
    finally:
        G.close(); P.close()


# ---- (d) the PCG recurrence -------------------------------------------------------------------------------------------------------------------------
def assert_same_count(its, its_ref, hist, tol, what):
    """identical iteration counts; +-1 only where the reference's residual at the deciding iteration lies within 1e-6 (relative) of the tolerance"""
    if its == its_ref:
        return
    k = min(its, its_ref)
    near = abs(its - its_ref) == 1 and k < len(hist) and abs(hist[k] - tol) <= 1e-6 * tol
    assert near, f"{what}: device {its} iterations, reference {its_ref} (reference residual at iteration {k}: {hist[min(k, len(hist) - 1)]:.6e}, tolerance {tol:.6e})"
    print(f"{what}: device {its}, reference {its_ref}: allowed, the residual at iteration {k} is within 1e-6 of the tolerance")


def check_pcg(dim, n, deg):
    P = box_problem(dim, n, deg)
    G = context(P)
    try:
        R = BoxReference(P)
        p = pressure(G.n_p)
        G.set(pk.VEC_P, p); G.disp_assemble_system(True)
        b = G.get(pk.VEC_RHS_U)                     # the device's own right-hand side (the reference's is checked in (a))
        x = np.zeros(G.n_u)
        G.fill(pk.VEC_U, 0.0)
        counts = []
        for start in ("zero", "warm", "zero again"):
            if start == "zero again":
                G.fill(pk.VEC_U, 0.0); x = np.zeros(G.n_u)
            rc, info = G.disp_solve(abs_tol=BENCH_TOL["abs_tol"], rel_tol=BENCH_TOL["rel_tol"], max_iter=200, prec=pk.PREC_FDM, reduction=BENCH_TOL["reduction"])
            xr, its, hist, tol = reference_pcg(R.apply_A, R.block_inverse_u, b, x, BENCH_TOL["abs_tol"], BENCH_TOL["rel_tol"], 200, 1, inert=R.mask)
            xr[R.dir_dof] = R.dir_val
            what = f"{n} Q{deg} from {start}"
            assert rc == 0, what
            assert_same_count(info.iterations, its, hist, tol, what)
            # from zero g_0 = -b; from the warm start g_0 = A u - b is a 1e-8 remainder of terms of size ||b||, so the two operators' rounding (eps ||b||) is the floor
            floor = 1e-12 * hist[0] if start != "warm" else 1e-12 * hist[0] + 1e-14 * np.linalg.norm(b)
            assert abs(info.initial_residual - hist[0]) <= floor, (what, info.initial_residual, hist[0])
            assert abs(info.final_residual - hist[-1]) <= 1e-6 * hist[-1], (what, info.final_residual, hist[-1])
            u = G.get(pk.VEC_U)
            assert (e := rel(u, xr)) <= 1e-9, (what, e)
            counts.append(info.iterations)
            x = u.copy()
        return counts
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("n", [24, 72], ids=str)
def test_pcg_recurrence_equals_the_reference_pcg(n):
    print("iterations (zero, warm, zero):", check_pcg(3, n, 2))


# ---- (e) variants behind environment switches, one child process each --------------------------------------------------------------------------------
def run_child(env_over, checks, timeout=900):
    env = dict(os.environ, **env_over)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), checks], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "child ok" in r.stdout, (env_over, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    print(env_over, f"{time.time() - t0:.1f} s:", r.stdout.strip())
    return r.stdout


FDM_PAIR = "fdm"              # (b) on the nodal-path shapes
# the three nodal-kernel switches only act where the octant form is off (PORO_FDMU_NO_OCT): lines of 95 - 129 (Q2) and 100 (Q1) points take the register /
# parity-split forms by default, the switches the LDS form, the unsplit lines and the unswapped x pass
NO_OCT = {"PORO_FDMU_NO_OCT": "1"}
VARIANTS = [(dict(NO_OCT, PORO_FDMU_LDS_FORM="1"), FDM_PAIR), (NO_OCT, FDM_PAIR), (dict(NO_OCT, PORO_FDMU_NO_SPLIT="1"), FDM_PAIR),
            (dict(NO_OCT, PORO_FDMU_NO_SWAP="1"), FDM_PAIR), ({"PORO_KRON_COLMAJOR": "1"}, "op"), ({"PORO_KRON_MIN_CHUNK": "4"}, "op"), ({"PORO_KRON_MIN_CHUNK": "1"}, "op"),
            ({"PORO_FORCE_PARTITIONED_PATH": "1"}, "pcg"), ({"PORO_FORCE_PARTITIONED_PATH": "1", "PORO_TWO_REDUCTION_CG": "1"}, "pcg"),
            ({"PORO_FDMO_UPDATE_G_SINGLE": "1"}, "pcg")]


@pytest.mark.parametrize("env,checks", VARIANTS, ids=lambda v: ",".join(f"{k}={w}" for k, w in v.items()) if isinstance(v, dict) else v)
def test_variant_switches(env, checks):
    run_child(env, checks)


def test_single_precision_block_fdm_bound():
    """PORO_FDMU_SINGLE: the nodal transforms in fp32 (v_mfma_f32_16x16x4_f32), the rest of the preconditioner in fp64.  Bound asserted: 1e-5
    relative to max|z|; measured on the MI355X: 7.3e-7 at 47 x 63 x 64 Q2, 8.4e-7 at 99^3 Q1 (sums over up to 129 points per line in three
    directions at fp32 eps 6e-8, times the eigenvector conditioning).  The constrained dofs stay exactly zero."""
    run_child({"PORO_FDMU_SINGLE": "1"}, "fdm_single")


def _child(checks):
    if checks in ("fdm", "fdm_single"):
        tol = 1e-5 if checks == "fdm_single" else 1e-10
        for dim, n, deg in ((3, (47, 63, 64), 2), (3, (99, 99, 99), 1)):
            print(f"block fdm {n} Q{deg}: {check_block_fdm(dim, n, deg, tol=tol):.3e}")
    elif checks == "op":
        check_operator(3, 72, 2)
        print("operator 72^3 Q2 ok")
    elif checks == "pcg":
        for dim, n, deg in ((3, 24, 2), (3, 72, 2)):                    # (d) at 24^3 and at the 72^3 headline
            print(f"pcg {n}: iterations {check_pcg(dim, n, deg)}")
        for dim, n, deg in ((3, (31, 32, 33), 2),):
            print(f"block fdm {n} Q{deg}: {check_block_fdm(dim, n, deg):.3e}")
    else:
        raise SystemExit(f"unknown check {checks}")
    print("child ok")


if __name__ == "__main__":
    _child(sys.argv[1])

"""The general-mesh kernels on skewed, non-affine and locally refined cells, against the oracle and against the fp64 reference of
tests/general_reference.py (itself pinned by test_general_reference_cpu.py).  Every mesh of the other tests has axis-aligned cells, where the MappingQ1
Jacobian is diagonal and a transposed J^-1, a wrong cofactor or a wrong face normal goes unseen.

(a) tail shapes: maps shear / multilinear / jitter / one_vertex, 2D / 3D, Q1 / Q2, at box sizes whose colour classes end in a workgroup holding 1 and
    (cells per workgroup - 1) cells; the operator with a random vector and with unit spikes in the last, partial workgroup of every colour, the
    diagonal, the right-hand side with Neumann faces; matrix-free and CSR.
(b) the kernel variants behind PORO_MFG_NO_SUMFAC (k_mfg mode 0) and PORO_MFG_NO_AFFINE, in child processes (the switches are read once per process).
(c) the profiled sizes of this path against the reference.  (d) time steps and (e) solvers against the oracle on distorted meshes.
(f) set-up: the affine detector and the refusal of inverted cells.  (g) FE tables other than the ones the sum-factorised kernels hard-code.

Tolerances relative to the max of the reference: 1e-12 (operator, diagonal, right-hand sides), 1e-13 (assembled pressure matrices)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":          # a child process of run_child: the repository root and the oracle on the path, as tests/conftest.py puts them
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]

import poroelasticity_dealii_amd as pk
import oracle_py
from common import BC_2D, BC_3D, REF, csr_to_scipy, host_material, material
from general_reference import (MAPS, GeneralReference, cells_per_workgroup, colour_classes, distorted_msh, jitter, mapped, mirror, multilinear,
                               q1_at, rule_1d, tensor_shapes)

pytestmark = pytest.mark.gpu

DT = REF["dt"]
# per (dim, degree): box sizes whose colour classes end in a partial workgroup of 1 and of (cells per workgroup - 1) cells (greedy colouring: 2^dim
# parity classes; no single box has both remainders)
TAIL_SIZES = {(3, 2): [(3, 5, 5), (3, 5, 9)], (3, 1): [(9, 9, 17), (5, 5, 13)], (2, 2): [(7, 21), (13, 17)], (2, 1): [(9, 25), (29, 33)]}
NEUMANN = {2: [(1, 1, 3e6), (3, 0, -2e6)], 3: [(1, 1, 3e6), (1, 2, -1e6), (5, 0, -2e6)]}     # components the Dirichlet list leaves free on those faces


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def pressure(n_p):
    return REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(n_p)))


def graded(dim, n, deg, neumann=()):
    return pk.Problem.graded_box(dim, list(n), [10.0] * dim, deg, material(), BC_2D if dim == 2 else BC_3D, [0.3, -0.2, 0.15][:dim], neumann)


def tail_spikes(M, R, deg):
    """unit entries at free dofs of the cells of the last, partial workgroup of every colour"""
    cpw = cells_per_workgroup(M.desc.dim, deg)
    x = np.zeros(R.n_u)
    for k, cells in enumerate(colour_classes(M.desc)):
        tail = cells[len(cells) - len(cells) % cpw:] if len(cells) % cpw else cells[-cpw:]
        for j, c in enumerate((tail[0], tail[-1])):
            dofs = [d for d in R.cdu[c] if not R.mask[d]]
            if dofs:
                x[dofs[(k + 3 * j) % len(dofs)]] = 1.0
    return x


def check_tail(name, dim, deg, n, modes=(pk.OP_MATRIX_FREE, pk.OP_CSR), with_rhs=None):
    """operator (random x, tail spikes), diagonal and right-hand side of one mapped box against the oracle and the reference"""
    with_rhs = name in ("shear", "jitter") if with_rhs is None else with_rhs
    P = graded(dim, n, deg, NEUMANN[dim] if with_rhs else ())
    M = mapped(P, MAPS[name](P))
    O = oracle_py.Oracle(M, hoisted=True)
    R = GeneralReference(M)
    ctxs = [pk.Context(M, 0, m) for m in modes]
    try:
        cpw = cells_per_workgroup(dim, deg)
        rems = [len(c) % cpw for c in colour_classes(M.desc)]
        p = pressure(M.desc.n_dofs_p)
        for S in [O] + ctxs:
            S.set(pk.VEC_P, p); S.disp_assemble_system(True)
        x = np.random.default_rng(5).standard_normal(R.n_u)
        s = tail_spikes(M, R, deg)
        yx, ys, dg = R.apply_A(x), R.apply_A(s), R.diag_A()
        assert rel(O.apply(pk.MAT_A_U, x), yx) <= 1e-12
        b0 = O.get(pk.VEC_RHS_U)
        for mode, G in zip(modes, ctxs):
            what = (name, dim, deg, n, "matrix-free" if mode == pk.OP_MATRIX_FREE else "csr")
            assert (e := rel(G.apply(pk.MAT_A_U, x), yx)) <= 1e-12, (what, "random", e)
            assert (e := rel(G.apply(pk.MAT_A_U, s), ys)) <= 1e-12, (what, "tail spikes", e)
            assert (e := rel(G.get(pk.VEC_DIAG_U), dg)) <= 1e-12, (what, "diag", e)
            assert (e := rel(G.get(pk.VEC_RHS_U), b0)) <= 1e-12, (what, "rhs", e)
        return rems
    finally:
        for G in ctxs:
            G.close()
        O.close(); M.close()


TAIL_CASES = [(m, dim, deg, n) for m in MAPS for (dim, deg), sizes in TAIL_SIZES.items() for n in sizes]


@pytest.mark.parametrize("name,dim,deg,n", TAIL_CASES, ids=[f"{m}-{d}d-q{k}-{'x'.join(map(str, n))}" for m, d, k, n in TAIL_CASES])
def test_tail_shapes_against_oracle_and_reference(name, dim, deg, n):
    rems = check_tail(name, dim, deg, n)
    cpw = cells_per_workgroup(dim, deg)
    assert (1 in rems) or (cpw - 1 in rems), rems


def test_tail_sizes_cover_both_remainders():
    for (dim, deg), sizes in TAIL_SIZES.items():
        cpw = cells_per_workgroup(dim, deg)
        rems = set()
        for n in sizes:
            P = graded(dim, n, deg)
            rems |= {len(c) % cpw for c in colour_classes(P.desc)}
            P.close()
        assert {1, cpw - 1} <= rems, (dim, deg, rems)


# ---- (b) variants behind environment switches ------------------------------------------------------------------------------------------------------
def run_child(env_over, checks, timeout=600):
    env = dict(os.environ, **env_over)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), checks], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "child ok" in r.stdout, (env_over, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    print(env_over, f"{time.time() - t0:.1f} s:", r.stdout.strip())


def test_table_driven_kernel_mode_0():
    """PORO_MFG_NO_SUMFAC: k_mfg<2|3> applies the operator (mode 0) instead of the sum-factorised kernels"""
    run_child({"PORO_MFG_NO_SUMFAC": "1"}, "no_sumfac")


def test_non_affine_kernel_on_mapped_boxes():
    """PORO_MFG_NO_AFFINE: k_mfg3_sf<N, false> (Jacobian from the eight vertices at every point) on the shear and multilinear maps"""
    run_child({"PORO_MFG_NO_AFFINE": "1"}, "no_affine")


def _child(checks):
    if checks == "no_sumfac":
        for name in MAPS:
            for (dim, deg), sizes in TAIL_SIZES.items():
                check_tail(name, dim, deg, sizes[1], modes=(pk.OP_MATRIX_FREE,), with_rhs=False)
    elif checks == "no_affine":
        for name in ("shear", "multilinear"):
            for deg in (1, 2):
                for n in TAIL_SIZES[(3, deg)]:
                    check_tail(name, 3, deg, n, modes=(pk.OP_MATRIX_FREE,), with_rhs=False)
    else:
        raise SystemExit(f"unknown check {checks}")
    print("child ok")


# ---- (c) full size against the reference -------------------------------------------------------------------------------------------------------
def check_full(M, diag=True):
    G = pk.Context(M, 0, pk.OP_MATRIX_FREE)
    try:
        t0 = time.time()
        R = GeneralReference(M)
        G.set(pk.VEC_P, pressure(M.desc.n_dofs_p)); G.disp_assemble_system(True)
        x = np.random.default_rng(9).standard_normal(R.n_u)
        assert (e := rel(G.apply(pk.MAT_A_U, x), R.apply_A(x))) <= 1e-12, ("operator", e)
        t1 = time.time()
        if diag:
            assert (e := rel(G.get(pk.VEC_DIAG_U), R.diag_A())) <= 1e-12, ("diag", e)
        print(f"{R.n_u} dofs: reference operator {t1 - t0:.1f} s, diagonal {time.time() - t1:.1f} s ({R.threads} threads)")
    finally:
        G.close()


@pytest.mark.parametrize("name", ["multilinear", "shear"])
def test_72_cubed_q2_mapped(name):
    """the tools/mfg_bench.py shape (72^3 Q2 graded box, 9.1 M dofs) under the multilinear map (k_mfg3_sf<3, false>) and the shear map (<3, true>)"""
    P = pk.Problem.graded_box(3, [72] * 3, [10.0] * 3, 2, material(), BC_3D, [0.0] * 3)
    M = mapped(P, MAPS[name](P))
    try:
        check_full(M, diag=name == "multilinear")
    finally:
        M.close()


def test_distorted_gmsh_refined_5_times(tmp_path):
    P = pk.Problem.gmsh(distorted_msh(tmp_path), 2, material(), BC_2D, refine=5)
    try:
        check_full(P)
    finally:
        P.close()


def test_refined_box_32_multilinear():
    P = pk.Problem.refined_box(3, [32] * 3, [10.0] * 3, 2, material(), BC_3D, [8] * 3, [24] * 3)
    M = mapped(P, multilinear(P))
    try:
        check_full(M)
    finally:
        M.close()


# ---- (d) time steps against the oracle ---------------------------------------------------------------------------------------------------------
def check_pressure_and_projection(O, G, dim):
    for S in (O, G):
        S.pres_assemble_jacobian(DT)
    for which in (pk.MAT_MASS_P, pk.MAT_LAPLACE_P, pk.MAT_JACOBIAN_P):
        Ao, Ag = csr_to_scipy(*O.export_csr(which)), csr_to_scipy(*G.export_csr(which))
        assert abs(Ao - Ag).max() <= 1e-13 * abs(Ao).max(), which
    pairs = [a * dim + b for a in range(dim) for b in range(a, dim)]
    for S in (O, G):
        S.proj_assemble_rhs(pairs)
    for e in range(len(pairs)):
        assert rel(G.get(pk.VEC_PROJ_RHS0 + e), O.get(pk.VEC_PROJ_RHS0 + e)) <= 1e-12, e


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("mode", [pk.OP_MATRIX_FREE, pk.OP_CSR], ids=["matrix_free", "csr"])
def test_time_step_on_the_distorted_gmsh_grid(tmp_path, deg, mode):
    """BASELINE config 1 (input.data) on the distorted grid: the trace (iteration counts) and the fields of the oracle"""
    P = pk.Problem.gmsh(distorted_msh(tmp_path), deg, host_material(), BC_2D)
    O = oracle_py.Oracle(P, hoisted=True)
    G = None
    try:
        t0, _ = O.run(1, REF["p_init"], DT, max_it=5000)
        t1, G = pk.run_problem(P, 1, REF["p_init"], DT, operator_mode=mode, max_it=5000)
        assert np.array_equal(t1[:, :3], t0[:, :3]), (t1, t0)
        assert np.linalg.norm(G.get(pk.VEC_U) - O.get(pk.VEC_U)) <= 1e-8 * np.linalg.norm(O.get(pk.VEC_U))
        assert np.abs(G.get(pk.VEC_P) - O.get(pk.VEC_P)).max() <= 1e-10 * np.abs(O.get(pk.VEC_P)).max()
        # volumetric strain after the step = eps_v0 (projected once at the start) + (alpha / K)(p - p_init) (the fixed-stress updates; the
        # reference does not re-project after the displacement solve): the update part holds to rounding on both sides
        m = P.desc.mat
        for S in (G, O):
            assert rel(S.get(pk.VEC_EPSV) - S.get(pk.VEC_EPSV0), m.biot_alpha / m.bulk_K * (S.get(pk.VEC_P) - REF["p_init"])) <= 1e-10
        # eps_v0 comes out of CG solves of M_p x = r stopped at ||res|| <= 1e-8 ||r|| (Jacobi on the device, SSOR in the oracle), with r from
        # displacements that agree to 1e-8: the two differ by at most 3 cond(M_p) 1e-8 ||x|| (measured 5.8e-8 - 7.3e-8 in max norm; cond = 31)
        Mp = csr_to_scipy(*O.export_csr(pk.MAT_MASS_P))
        lam = np.linalg.eigvalsh(Mp.toarray())
        e0, g0 = O.get(pk.VEC_EPSV0), G.get(pk.VEC_EPSV0)
        assert np.linalg.norm(g0 - e0) <= 3 * lam[-1] / lam[0] * 1e-8 * np.linalg.norm(e0), (np.linalg.norm(g0 - e0) / np.linalg.norm(e0), lam[-1] / lam[0])
        check_pressure_and_projection(O, G, 2)
    finally:
        if G is not None:
            G.close()
        O.close(); P.close()


def test_step_phases_on_a_multilinear_graded_box():
    """3D: displacement solve, pressure matrices and projection right-hand sides of a mapped graded box (no host problem: the phases one by one)"""
    P = graded(3, (6, 5, 4), 2)
    M = mapped(P, multilinear(P))
    O = oracle_py.Oracle(M, hoisted=True)
    G = pk.Context(M, 0, pk.OP_MATRIX_FREE)
    try:
        p = pressure(M.desc.n_dofs_p)
        for S in (O, G):
            S.set(pk.VEC_P, p); S.disp_assemble_system(True)
        assert rel(G.get(pk.VEC_RHS_U), O.get(pk.VEC_RHS_U)) <= 1e-12
        assert O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=20000)[0] == 0
        rc, _ = G.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=20000)
        assert rc == 0 and np.linalg.norm(G.get(pk.VEC_U) - O.get(pk.VEC_U)) <= 1e-9 * np.linalg.norm(O.get(pk.VEC_U))
        G.set(pk.VEC_U, O.get(pk.VEC_U))
        check_pressure_and_projection(O, G, 3)
    finally:
        G.close(); O.close(); M.close()


# ---- (e) solvers on constrained and distorted meshes -------------------------------------------------------------------------------------------
def check_solvers(M, label):
    O = oracle_py.Oracle(M, hoisted=True)
    G = pk.Context(M, 0, pk.OP_MATRIX_FREE)
    try:
        p = pressure(M.desc.n_dofs_p)
        for S in (O, G):
            S.set(pk.VEC_P, p); S.disp_assemble_system(True)
        assert O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=50000)[0] == 0
        u0 = O.get(pk.VEC_U)
        counts = {}
        for name, prec in (("jacobi", pk.PREC_JACOBI), ("chebyshev", pk.PREC_CHEBYSHEV), ("two_level", pk.PREC_TWO_LEVEL)):
            assert G.supports_preconditioner(0, prec), name
            G.fill(pk.VEC_U, 0.0)
            rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=50000, prec=prec)
            assert rc == 0 and np.linalg.norm(G.get(pk.VEC_U) - u0) <= 1e-9 * np.linalg.norm(u0), name
            counts[name] = info.iterations
        print(label, "CG iterations:", counts)
        assert counts["two_level"] <= counts["jacobi"], counts
    finally:
        G.close(); O.close()


def test_solvers_on_a_multilinear_refined_box():
    P = pk.Problem.refined_box(3, [4] * 3, [10.0] * 3, 2, material(), BC_3D, [1] * 3, [3] * 3)
    M = mapped(P, multilinear(P))
    try:
        check_solvers(M, "refined box, multilinear map")
    finally:
        M.close()


@pytest.mark.parametrize("refine", [0, 1, 2])
def test_solvers_on_the_jittered_gmsh_grid(tmp_path, refine):
    """the jitter map alone: the grid still fills the rectangle, so it keeps its auxiliary box (the coarse space of PREC_TWO_LEVEL)"""
    P = pk.Problem.gmsh(distorted_msh(tmp_path, jitter(None, X0=np.array([[-5.0, -5.0], [5.0, 5.0]]), h=1.0)), 2, material(), BC_2D, refine=refine)
    try:
        assert P.desc.coarse.enabled
        check_solvers(P, f"jittered Gmsh grid, refine {refine}")
    finally:
        P.close()


# ---- (f) set-up ---------------------------------------------------------------------------------------------------------------------------------
def test_mirrored_mesh_is_refused():
    for dim in (2, 3):
        P = graded(dim, (3, 4, 2)[:dim], 2)
        M = mapped(P, mirror(P), check=False)
        try:
            with pytest.raises(RuntimeError, match="det J"):
                pk.Context(M, 0, pk.OP_MATRIX_FREE)
            with pytest.raises(RuntimeError, match="det J"):
                pk.Context(M, 0, pk.OP_CSR)
        finally:
            M.close()


def test_one_moved_vertex_leaves_the_affine_path():
    """shear + one vertex moved: the detector must send the whole mesh to the trilinear kernel (the affine one would use the wrong Jacobian there)"""
    for deg in (1, 2):
        check_tail("one_vertex", 3, deg, TAIL_SIZES[(3, deg)][0], modes=(pk.OP_MATRIX_FREE,), with_rhs=False)


# ---- (g) FE tables the sum-factorised kernels do not hard-code ---------------------------------------------------------------------------------
class LobattoTables:
    """the mapped problem with u-quadrature tables from the (k+1)-point Gauss-Lobatto rule (same nq_u)"""

    def __init__(self, M):
        self.M = M
        d = M.desc
        dim, k = d.dim, d.degree_u
        t1, w1 = rule_1d(k + 1, "lobatto")
        qi = np.array(list(np.ndindex(*([k + 1] * dim))))[:, ::-1]
        val, grad = tensor_shapes(dim, k, t1)
        qv, qg = q1_at(dim, t1[qi])
        self.keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (np.prod(w1[qi], axis=1), val, grad, qv, qg)]
        self.desc = pk.Desc.from_buffer_copy(d)
        for name, a in zip(("w_qu", "u_qu", "du_qu", "q1_qu", "dq1_qu"), self.keep):
            setattr(self.desc.fe, name, a.ctypes.data_as(C.POINTER(C.c_double)))
        self.desc_ptr = C.pointer(self.desc)


@pytest.mark.parametrize("dim,deg", [(2, 1), (2, 2), (3, 1), (3, 2)], ids=str)
def test_gauss_lobatto_tables_reach_the_matrix_free_operator(dim, deg):
    P = graded(dim, TAIL_SIZES[(dim, deg)][1], deg)
    M = mapped(P, multilinear(P))
    L = LobattoTables(M)
    F, A = pk.Context(L, 0, pk.OP_MATRIX_FREE), pk.Context(L, 0, pk.OP_CSR)
    try:
        R = GeneralReference(M, rule="lobatto")
        for S in (F, A):
            S.set(pk.VEC_P, pressure(M.desc.n_dofs_p)); S.disp_assemble_system(True)
        x = np.random.default_rng(2).standard_normal(R.n_u)
        y = R.apply_A(x)
        assert (e := rel(F.apply(pk.MAT_A_U, x), y)) <= 1e-12, ("matrix-free", e)
        assert (e := rel(A.apply(pk.MAT_A_U, x), y)) <= 1e-12, ("csr", e)
        assert (e := rel(F.get(pk.VEC_DIAG_U), R.diag_A())) <= 1e-12, ("diag", e)
        assert rel(F.get(pk.VEC_RHS_U), A.get(pk.VEC_RHS_U)) <= 1e-12
    finally:
        F.close(); A.close(); M.close()


if __name__ == "__main__":
    _child(sys.argv[1])

"""The hybrid operator form of the matrix-free displacement operator on refined boxes (poro_ctx_set_operator_form, PORO_OPFORM_HYBRID): the coarse box's structured
kernel over the whole box, minus the element products of the refined box cells, plus the general cell kernels over the fine cells only.

(1) the operator against the fp64 reference of tests/general_reference.py and against the same context's general coloured product, on the shapes and masks of
    tests/hybrid_reference.py (2D / 3D, Q1 / Q2; no cell, every cell, a block, a Dirichlet corner cell, a random 30 % refined): a random vector and unit spikes; the
    getter's counts, the cell-kernel launch counts, bitwise repeatability in the coloured mode, the atomic scatter mode.
(2) plumbing: default, round trip, set-up vectors bitwise independent of the form, unknown forms, box-tagged contexts, refusals with their messages.
(3) Jacobi-, Chebyshev- and two-level-preconditioned solves in both forms against the oracle.
(4) a 3-step adaptive run through the driver in both forms.

Operator tolerance: 1e-12 relative to the max of the reference, the bound tests/test_general_mesh_gpu.py applies to the coloured kernels and tests/test_mfg_atomic_gpu.py
to the atomic mode: the hybrid adds one subtraction of same-size terms, a few ulps of sum |contributions|.  Solves: iteration counts within +-1, u within 1e-9
relative of the oracle's (the bounds of tests/test_mfg_atomic_gpu.py / tests/test_constraints_gpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":          # the child process of the partitioned-path refusal: the repository root and the oracle on the path, as tests/conftest.py puts them
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]

import poroelasticity_dealii_amd as pk
import oracle_py
from common import BC_2D, BC_3D, DOMAIN_MSH, REF, box_problem, material
from general_reference import GeneralReference, colour_classes, mapped, multilinear
from hybrid_reference import MASKS, SHAPES, HybridPlan, make_mask, refined_problem, shape_id, spike_dofs

gpu = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def rel2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def pressure(n_p):
    return REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(n_p)))


def assembled(P):
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    G.set(pk.VEC_P, pressure(P.desc.n_dofs_p)); G.disp_assemble_system(True)
    return G


def cell_launches(G, x):
    G.timers_reset()
    y = G.apply(pk.MAT_A_U, x)
    n = G.timer("mfg_cell_kernels")[1]
    box_launches = G.timer("apply_u_hybrid_box")[1]
    G.timers_enable(0)
    return n, box_launches, y


# ---- (1) the operator ----------------------------------------------------------------------------------------------------------------------------------
CASES = [(dim, deg, n, m) for dim, deg, n in SHAPES for m in MASKS]


@gpu
@pytest.mark.parametrize("dim,deg,n,name", CASES, ids=[f"{shape_id(d, k, n)}-{m}" for d, k, n, m in CASES])
def test_hybrid_operator_against_reference_and_general_form(dim, deg, n, name):
    mask = make_mask(name, n)
    P = refined_problem(dim, deg, n, mask)
    G = None
    try:
        R = GeneralReference(P)
        plan = HybridPlan(P)
        G = assembled(P)
        n_ref = int(mask.sum())
        assert G.get_operator_form() == (pk.OPFORM_GENERAL, P.desc.n_cells, 0)
        vectors = {"random": np.random.default_rng(5).standard_normal(R.n_u)}
        for label, dof in spike_dofs(P, plan, R).items():
            e = np.zeros(R.n_u); e[dof] = 1.0
            vectors[label] = e
        general = {label: G.apply(pk.MAT_A_U, x) for label, x in vectors.items()}
        G.set_operator_form(pk.OPFORM_HYBRID)
        assert G.get_operator_form() == (pk.OPFORM_HYBRID, n_ref << dim, n_ref)          # the getter's counts are the mask's
        what = (shape_id(dim, deg, n), name)
        for label, x in vectors.items():
            yr = R.apply_A(x)
            y = G.apply(pk.MAT_A_U, x)
            er, eg = rel(y, yr), float(np.abs(y - general[label]).max() / np.abs(yr).max())
            print(what, label, f"vs reference {er:.2e}, vs general form {eg:.2e}")
            assert er <= 1e-12, (what, label, "reference", er)
            assert eg <= 1e-12, (what, label, "general form", eg)
            assert np.array_equal(G.apply(pk.MAT_A_U, x), y), (what, label, "two coloured hybrid applications differ")
        # launches of the cell kernels per application: one per colour class that holds a fine cell; none at all without refined cells
        fine = np.zeros(P.desc.n_cells, bool); fine[plan.fine] = True
        n_classes = sum(1 for cl in colour_classes(P.desc) if fine[cl].any())
        x = vectors["random"]
        n_launch, n_box, _ = cell_launches(G, x)
        assert n_launch == n_classes and n_box == 1, (what, n_launch, n_classes, n_box)
        if name == "none":
            assert n_launch == 0 and G.get_operator_form()[1] == 0
        # the atomic scatter mode composes with the form: one launch over the fine cells
        G.set_scatter_mode(pk.SCATTER_ATOMIC)
        n_launch, _, ya = cell_launches(G, x)
        assert n_launch == (1 if n_ref else 0), (what, n_launch)
        assert (e := rel(ya, R.apply_A(x))) <= 1e-12, (what, "atomic", e)
    finally:
        if G is not None:
            G.close()
        P.close()


# ---- (2) plumbing --------------------------------------------------------------------------------------------------------------------------------------
def block_problem(dim, deg=2, n=4):
    return pk.Problem.refined_box(dim, [n] * dim, [10.0] * dim, deg, material(), BC_2D if dim == 2 else BC_3D, [1] * dim, [n - 1] * dim)


@gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_default_round_trip_and_unknown_forms(dim):
    P = block_problem(dim)
    G = assembled(P)
    try:
        assert G.get_operator_form()[0] == pk.OPFORM_GENERAL                             # the default
        x = np.random.default_rng(1).standard_normal(G.n_u)
        y0 = G.apply(pk.MAT_A_U, x)
        for bad in (2, -1, 17):
            with pytest.raises(RuntimeError, match="unknown form"):
                G.set_operator_form(bad)
            assert G.get_operator_form()[0] == pk.OPFORM_GENERAL
        G.set_operator_form(pk.OPFORM_HYBRID)
        assert G.get_operator_form()[0] == pk.OPFORM_HYBRID
        y1 = G.apply(pk.MAT_A_U, x)
        assert rel(y1, y0) <= 1e-12
        G.set_operator_form(pk.OPFORM_GENERAL)
        assert G.get_operator_form() == (pk.OPFORM_GENERAL, P.desc.n_cells, 0)
        assert np.array_equal(G.apply(pk.MAT_A_U, x), y0)                                # back in the general form: bitwise the results from before
        G.set_operator_form(pk.OPFORM_HYBRID)
        assert np.array_equal(G.apply(pk.MAT_A_U, x), y1)                                # and the hybrid form again, from the plan that was built once
    finally:
        G.close(); P.close()


@gpu
@pytest.mark.parametrize("inhomogeneous", [False, True], ids=["homogeneous", "inhomogeneous"])
def test_setup_vectors_do_not_depend_on_the_form(inhomogeneous):
    """VEC_DIAG_U and VEC_RHS_U are set-up quantities: the general coloured kernels over all cells in either form, also where the condensed right-hand side takes an
    operator product (constraints with inhomogeneities)"""
    P = block_problem(3)
    c = P.desc.cons_u
    assert c.n > 0
    if inhomogeneous:
        for i in range(c.n):
            c.inhomogeneity[i] = 0.01 * np.sin(1.0 + i)
    G = assembled(P)
    try:
        d0, b0 = G.get(pk.VEC_DIAG_U), G.get(pk.VEC_RHS_U)
        G.set_operator_form(pk.OPFORM_HYBRID)
        n_colours = sum(1 for cl in colour_classes(P.desc) if len(cl))
        G.timers_reset(); G.disp_assemble_system(False)
        n = G.timer("mfg_cell_kernels")[1]
        G.timers_enable(0)
        assert n == (n_colours if inhomogeneous else 0), n                               # the product with x_inh: all cells, coloured
        assert np.array_equal(G.get(pk.VEC_RHS_U), b0)
        G.disp_assemble_system(True)
        assert np.array_equal(G.get(pk.VEC_DIAG_U), d0) and np.array_equal(G.get(pk.VEC_RHS_U), b0)
        assert G.get_operator_form()[0] == pk.OPFORM_HYBRID
    finally:
        G.close(); P.close()


@gpu
def test_box_tagged_context_is_unchanged():
    P = box_problem(3, 4, 2)
    G = assembled(P)
    try:
        x = np.random.default_rng(4).standard_normal(G.n_u)
        y0 = G.apply(pk.MAT_A_U, x)
        G.set_operator_form(pk.OPFORM_HYBRID)                                            # succeeds, changes nothing: the structured kernels run on every cell already
        assert G.get_operator_form() == (pk.OPFORM_GENERAL, 0, 0)
        assert np.array_equal(G.apply(pk.MAT_A_U, x), y0)
        with pytest.raises(RuntimeError, match="unknown form"):
            G.set_operator_form(5)
    finally:
        G.close(); P.close()


def refused(P, match):
    G = assembled(P)
    try:
        x = np.random.default_rng(2).standard_normal(G.n_u)
        y0 = G.apply(pk.MAT_A_U, x)
        with pytest.raises(RuntimeError, match=match):
            G.set_operator_form(pk.OPFORM_HYBRID)
        assert G.get_operator_form() == (pk.OPFORM_GENERAL, P.desc.n_cells, 0)
        assert np.array_equal(G.apply(pk.MAT_A_U, x), y0)
    finally:
        G.close()


@gpu
def test_a_mapped_refined_box_is_refused():
    P = block_problem(3)
    M = mapped(P, multilinear(P))
    try:
        assert M.desc.coarse.enabled
        refused(M, "vertices of mesh cell")
    finally:
        M.close()


@gpu
def test_the_gmsh_mesh_with_its_auxiliary_box_is_refused():
    P = pk.Problem.gmsh(DOMAIN_MSH, 2, material(), BC_2D)
    try:
        assert P.desc.coarse.enabled
        refused(P, "no injected image")
    finally:
        P.close()


@gpu
def test_a_context_without_a_coarse_space_is_refused():
    P = pk.Problem.graded_box(3, [4, 3, 3], [10.0] * 3, 2, material(), BC_3D, [0.3, -0.2, 0.15])
    try:
        assert not P.desc.coarse.enabled
        refused(P, "no coarse space")
    finally:
        P.close()


@gpu
def test_an_assembled_csr_context_is_refused():
    P = block_problem(2)
    G = pk.Context(P, 0, pk.OP_CSR)
    try:
        with pytest.raises(RuntimeError, match="PORO_OP_MATRIX_FREE"):
            G.set_operator_form(pk.OPFORM_HYBRID)
        assert G.get_operator_form()[0] == pk.OPFORM_GENERAL
    finally:
        G.close(); P.close()


@gpu
def test_the_partitioned_path_is_refused():
    """PORO_FORCE_PARTITIONED_PATH=1 is read at context creation: a child process"""
    env = dict(os.environ, PORO_FORCE_PARTITIONED_PATH="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "partitioned"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _child(check):
    if check != "partitioned":
        raise SystemExit(f"unknown check {check}")
    P = block_problem(2)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        G.set_operator_form(pk.OPFORM_HYBRID)
    except RuntimeError as e:
        assert "partitioned" in str(e), str(e)
        assert G.get_operator_form()[0] == pk.OPFORM_GENERAL
        print("child ok")
    finally:
        G.close(); P.close()


# ---- (3) solves ----------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_solves_in_both_forms_against_the_oracle(dim):
    """the (4, 4, 4) Q2 box with its block [1, 3)^3 refined and the 2D twin: hanging nodes condensed, so the Krylov operator, the Chebyshev recurrence, the two-level
    form's fine-level products and C^T A C all go through the form"""
    P = block_problem(dim)
    O = oracle_py.Oracle(P, hoisted=True)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert P.desc.cons_u.n > 0
        p = pressure(P.desc.n_dofs_p)
        for S in (O, G):
            S.set(pk.VEC_P, p); S.disp_assemble_system(True)
        assert O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=50000)[0] == 0
        u0 = O.get(pk.VEC_U)
        for name, prec in (("jacobi", pk.PREC_JACOBI), ("chebyshev", pk.PREC_CHEBYSHEV), ("two_level", pk.PREC_TWO_LEVEL)):
            assert G.supports_preconditioner(0, prec), name
            its = {}
            for form in (pk.OPFORM_GENERAL, pk.OPFORM_HYBRID):
                G.set_operator_form(form)
                G.fill(pk.VEC_U, 0.0)
                rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=50000, prec=prec)
                assert rc == 0 and info.converged, (name, form)
                its[form] = info.iterations
                e = rel2(G.get(pk.VEC_U), u0)
                print(dim, name, "form", form, "CG iterations", info.iterations, "|u - u_oracle| / |u_oracle|", e)
                assert e <= 1e-9, (name, form, e)
            assert abs(its[pk.OPFORM_HYBRID] - its[pk.OPFORM_GENERAL]) <= 1, (name, its)
    finally:
        G.close(); O.close(); P.close()


# ---- (4) the adaptive driver -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_three_step_adaptive_run_in_both_forms():
    """run_problem(refine_every=1) from the all-zero mask at 4^3 Q2: the same refinement masks and FSS / pressure iteration counts, CG counts within 1, p and u
    within 1e-9.  The same run step by step (Runner, adapt before every step): the context of every adapted mesh reports the hybrid form with the mask's counts"""
    n = (4, 4, 4)
    P = refined_problem(3, 2, n, make_mask("none", n))
    res = {}
    try:
        for hybrid in (False, True):
            trace, G = pk.run_problem(P, 3, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, prec=-1, refine_every=1, hybrid_operator=hybrid)
            problem = G.problem
            try:
                mask = problem.refine_mask()
                form, general_cells, removed = G.get_operator_form()
                assert form == (pk.OPFORM_HYBRID if hybrid else pk.OPFORM_GENERAL)
                assert (general_cells, removed) == ((8 * int(mask.sum()), int(mask.sum())) if hybrid else (problem.desc.n_cells, 0))
                res[hybrid] = (trace, mask, G.get(pk.VEC_P), G.get(pk.VEC_U))
            finally:
                G.close()
                if problem is not P:
                    problem.close()
        (t0, m0, p0, u0), (t1, m1, p1, u1) = res[False], res[True]
        assert np.array_equal(m0, m1) and m0.any()                                       # the run did refine, and to the same mesh
        assert t0.shape == t1.shape and np.array_equal(t0[:, :3], t1[:, :3])             # step, FSS iteration, pressure iterations
        assert np.abs(t0[:, 6] - t1[:, 6]).max() <= 1 and np.abs(t0[:, 7] - t1[:, 7]).max() <= 1      # u and p CG iterations
        assert rel2(p1, p0) <= 1e-9 and rel2(u1, u0) <= 1e-9
        R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=REF["p_init"], dt=REF["dt"], prec=-1, hybrid_operator=True)
        try:
            R.initialize()
            assert R.ctx.get_operator_form() == (pk.OPFORM_HYBRID, 0, 0)                # the all-zero mask: no cell for the general kernels
            rows = []
            for _ in range(3):
                R.adapt()
                k = int(R.problem.refine_mask().sum())
                assert R.ctx.get_operator_form() == (pk.OPFORM_HYBRID, 8 * k, k)
                rows.append(R.step()[0])
            assert np.array_equal(R.problem.refine_mask(), m1) and np.array_equal(np.vstack(rows), t1[1:])
        finally:
            R.close()
    finally:
        P.close()


if __name__ == "__main__":
    _child(sys.argv[1])

"""Per-direction form of the displacement system's block FDM (poro_ctx_set_fdm_form / PORO_FDM_FORM_PER_DIRECTION, Context.set_fdm_form, run_problem / Runner
(fdm_per_direction=True), PORO_FDMO_FORM): single-rank 3D boxes where only some directions are mirror-symmetric (one-sided Dirichlet faces, graded lines) run the octant
form's three contiguous passes with 2^(split directions) parity parts per component.

Bounds.  z = P^-1 g against the block inverse of the ORACLE's assembled matrix (sparse direct solve per component): 1e-10 of max |z0|, the project's bound for every fp64
form (tests/test_fdm_u_gpu.py), exact zeros on the Dirichlet dofs.  Inside PCG: u within 1e-9 of the oracle's SSOR-CG solution (both to 1e-12 |b|), the iteration count
within +-1 of the same context's nodal-form solve (the same mathematics in fp64; +-1 is the project's allowance between forms).  With PORO_FDMO_SEPARATE_GZ=1 (a child
process): the same iteration count and u to 1e-14 relative (measured 3e-17 and 3e-20 on the two shapes; the figure is printed).  Whole steps: the bounds of test_run_with_block_fdm_matches_the_oracle_trace."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":          # a child process: the repository root and the oracle on the path, as tests/conftest.py puts them
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]

import poroelasticity_dealii_amd as pk
from common import BC_3D, REF, box_problem, csr_to_scipy, material
from fdm_form_cases import BOXES, COLUMN, FORM_CASES, GRADED, X_ONE_SIDED, Y_ONE_SIDED

pytestmark = pytest.mark.gpu

DEFAULT, PER_DIRECTION = pk.FDM_FORM_DEFAULT, pk.FDM_FORM_PER_DIRECTION
FAMILY = "fdm_u_per_direction_form"


def problem(cells, deg, bc, grading=None):
    return box_problem(3, cells, deg, bc=bc) if grading is None else pk.Problem.graded_box(3, list(cells), [10.0] * 3, deg, material(), bc, list(grading))


# ---- 1. which form runs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES, ids=str)
@pytest.mark.parametrize("name", list(FORM_CASES), ids=str)
def test_every_boundary_list_runs_the_form_with_its_mask(name, box):
    mask, bc = FORM_CASES[name]
    P = problem(box[0], box[1], bc)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.get_fdm_form() == (DEFAULT, pk.FDM_RUNS_NODAL, (0, 0, 0))          # the default stays "octant form or nodal kernels"
        G.set_fdm_form(PER_DIRECTION)
        assert G.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PER_DIRECTION, mask)
        G.set_fdm_form(DEFAULT)
        assert G.get_fdm_form() == (DEFAULT, pk.FDM_RUNS_NODAL, (0, 0, 0))
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("box", BOXES, ids=str)
def test_a_symmetric_box_runs_the_octant_form_whatever_is_requested(box):
    P = problem(box[0], box[1], BC_3D)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.get_fdm_form() == (DEFAULT, pk.FDM_RUNS_OCTANT, (1, 1, 1))
        G.set_fdm_form(PER_DIRECTION)
        assert G.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_OCTANT, (1, 1, 1))
        G.set_fdm_precision(pk.FDM_FP32)
        assert G.get_fdm_precision() == (pk.FDM_FP32, pk.FDM_FP32)                 # the octant form keeps its fp32 mode
    finally:
        G.close(); P.close()


def test_a_graded_box_splits_its_uniform_direction_only():
    cells, deg, grading, mask = GRADED
    P = problem(cells, deg, BC_3D, grading)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.get_fdm_form() == (DEFAULT, pk.FDM_RUNS_NODAL, (0, 0, 0))
        G.set_fdm_form(PER_DIRECTION)
        assert G.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PER_DIRECTION, mask)
        G.set_fdm_precision(pk.FDM_FP32)
        assert G.get_fdm_precision() == (pk.FDM_FP32, pk.FDM_FP64)                 # fp32 fragments for this form are out of scope: the transforms stay fp64
    finally:
        G.close(); P.close()


def test_two_dimensional_contexts_ignore_the_request():
    from common import BC_2D
    P = box_problem(2, (5, 7), 2, bc=[(2, 1, 0.0), (1, 0, -1e-5)])
    Q = box_problem(2, (5, 7), 2, bc=BC_2D)
    G, H = pk.Context(P, 0, pk.OP_MATRIX_FREE), pk.Context(Q, 0, pk.OP_MATRIX_FREE)
    try:
        for C_, split in ((G, (0, 0, 0)), (H, (1, 1, 0))):
            C_.set_fdm_form(PER_DIRECTION)
            assert C_.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PLANAR, split)
    finally:
        G.close(); H.close(); P.close(); Q.close()


# ---- 2. equals the block inverse ---------------------------------------------------------------------------------------------------------------------
# (cells, degree, Dirichlet list, grading, effective form).  The tile-edge cases: n = nodes of the whole line
INVERSE_CASES = {f"{name}-{box[0]}-q{box[1]}": (box[0], box[1], bc, None, pk.FDM_RUNS_PER_DIRECTION) for box in BOXES for name, (_, bc) in FORM_CASES.items()}
INVERSE_CASES.update({
    "graded": (GRADED[0], GRADED[1], BC_3D, GRADED[2], pk.FDM_RUNS_PER_DIRECTION),
    "z17 one tile + 1": ((2, 3, 8), 2, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "z33 odd chunk count": ((3, 2, 16), 2, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "z73 five tiles, four waves": ((2, 2, 36), 2, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "z89 six tiles, > 64 KB LDS": ((2, 2, 44), 2, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "z127": ((2, 2, 63), 2, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "z128 q1, the cap": ((2, 2, 127), 1, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "x73 whole": ((36, 2, 3), 2, X_ONE_SIDED, None, pk.FDM_RUNS_PER_DIRECTION),
    "y73 whole": ((2, 36, 3), 2, Y_ONE_SIDED, None, pk.FDM_RUNS_PER_DIRECTION),
    "x half 41 (pitch 42), z73 whole: two tile counts": ((40, 3, 36), 2, COLUMN, None, pk.FDM_RUNS_PER_DIRECTION),
    "z129: beyond the cap, nodal kernels": ((2, 2, 64), 2, COLUMN, None, pk.FDM_RUNS_NODAL),
})


def block_inverse(A, mask, g):
    """blockdiag(A_cc)^-1 g on the free dofs of every component, zero on the Dirichlet dofs"""
    import scipy.sparse.linalg as spla
    z = np.zeros_like(g)
    for c in range(3):
        idx = np.arange(c, A.shape[0], 3)
        idx = idx[~mask[idx]]
        z[idx] = spla.splu(A[idx][:, idx].tocsc()).solve(g[idx])
    return z


@pytest.mark.parametrize("name", list(INVERSE_CASES), ids=str)
def test_the_form_equals_the_block_inverse(name):
    import oracle_py
    cells, deg, bc, grading, runs = INVERSE_CASES[name]
    P = problem(cells, deg, bc, grading)
    O = oracle_py.Oracle(P, hoisted=True)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        G.set_fdm_form(PER_DIRECTION)
        assert G.get_fdm_form()[1] == runs
        O.fill(pk.VEC_P, 0.0); O.disp_assemble_system(True)
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        A = csr_to_scipy(*O.export_csr(pk.MAT_A_U))
        nd = P.desc.n_dirichlet
        mask = np.zeros(G.n_u, bool); mask[np.ctypeslib.as_array(P.desc.dirichlet_dof, shape=(nd,))] = True
        rng = np.random.default_rng(7)
        g = rng.standard_normal(G.n_u) * 1e3; g[mask] = 0.0
        z = G.apply_preconditioner_u(pk.PREC_FDM, g)
        z0 = block_inverse(A, mask, g)
        err = float(np.abs(z - z0).max() / np.abs(z0).max())
        print(name, f"max |z - z0| / max |z0| = {err:.3e}")
        assert np.abs(z[mask]).max() == 0.0
        assert err <= 1e-10, err
        # symmetric positive definite as CG needs it
        g2 = rng.standard_normal(G.n_u); g2[mask] = 0.0
        z2 = G.apply_preconditioner_u(pk.PREC_FDM, g2)
        assert abs(g2 @ z - g @ z2) <= 1e-10 * abs(g2 @ z) + 1e-300 and g @ z > 0
    finally:
        G.close(); O.close(); P.close()


# ---- 3. inside PCG -----------------------------------------------------------------------------------------------------------------------------------
PCG_SHAPES = {"q2": ((6, 6, 6), 2), "q1": ((7, 5, 9), 1)}


def pcg_setup(shape, form):
    cells, deg = PCG_SHAPES[shape]
    P = problem(cells, deg, COLUMN)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    G.set_fdm_form(form)
    p = REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(G.n_p)))
    G.set(pk.VEC_P, p); G.disp_assemble_system(True)
    return P, G, p


def pcg_solve(G):
    G.fill(pk.VEC_U, 0.0)
    rc, info = G.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=200, prec=pk.PREC_FDM)
    return rc, info.iterations, G.get(pk.VEC_U).copy()


@pytest.mark.parametrize("shape", list(PCG_SHAPES), ids=str)
def test_pcg_with_the_form_solves_like_the_oracle_and_like_the_nodal_kernels(shape, tmp_path):
    import oracle_py
    P, G, p = pcg_setup(shape, PER_DIRECTION)
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        assert G.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PER_DIRECTION, (1, 1, 0))
        O.set(pk.VEC_P, p); O.disp_assemble_system(True)
        rc0, _ = O.disp_solve(abs_tol=1e-14, rel_tol=1e-12, max_iter=5000)
        counts = {f: G.timer(f)[1] for f in (FAMILY, "fdm_u_shared_buffers", "fdm_u_final_prec_skipped")}
        rc1, it1, u1 = pcg_solve(G)
        assert rc0 == 0 and rc1 == 0
        u0 = O.get(pk.VEC_U)
        err = float(np.linalg.norm(u1 - u0) / np.linalg.norm(u0))
        print(shape, f"per-direction form: {it1} iterations, |u - u_oracle| / |u_oracle| = {err:.3e}")
        assert err <= 1e-9, err
        for f, before in counts.items():            # the form keeps the octant form's place in the solve: shared h | z array, stopping test in pass 1
            assert G.timer(f)[1] == before + 1, (f, before, G.timer(f)[1])
        # the same context with the nodal kernels: the same mathematics in fp64
        G.set_fdm_form(DEFAULT)
        assert G.get_fdm_form()[1] == pk.FDM_RUNS_NODAL
        rc2, it2, u2 = pcg_solve(G)
        print(shape, f"nodal kernels: {it2} iterations")
        assert rc2 == 0 and abs(it1 - it2) <= 1, (it1, it2)
        assert G.timer(FAMILY)[1] == counts[FAMILY] + 1                                      # the nodal solve does not count
        assert np.linalg.norm(u2 - u0) <= 1e-9 * np.linalg.norm(u0)
        # g . z by the separate dot kernel instead of pass 2's partial sums (the switch is read per solve; a child process keeps this one's environment clean)
        out = tmp_path / "u.npy"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "separate_gz", shape, str(out)], env=dict(os.environ, PORO_FDMO_SEPARATE_GZ="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
        it3 = int(r.stdout.split("iterations=")[1].split()[0]); u3 = np.load(out)
        dev = float(np.linalg.norm(u1 - u3) / np.linalg.norm(u3))
        print(shape, f"separate g.z: {it3} iterations, |u_pass - u_separate| / |u_separate| = {dev:.3e}")
        assert it3 == it1, (it1, it3)
        assert dev <= 1e-14, dev
    finally:
        G.close(); O.close(); P.close()


# ---- 4. whole steps ----------------------------------------------------------------------------------------------------------------------------------
def test_time_steps_with_the_form_match_the_oracle_trace():
    import oracle_py
    P = problem((4, 4, 6), 2, COLUMN)
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        t0, _ = O.run(3, REF["p_init"], REF["dt"], max_it=5000)
        t1, G = pk.run_problem(P, 3, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, max_it=500, prec=pk.PREC_FDM, fdm_per_direction=True)
        try:
            assert G.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PER_DIRECTION, (1, 1, 0))
            assert G.timer(FAMILY)[1] >= 3                                 # (at least one displacement solve per step, every one in the form)
            assert np.array_equal(t1[:, :3], t0[:, :3])
            eu = float(np.linalg.norm(G.get(pk.VEC_U) - O.get(pk.VEC_U)) / np.linalg.norm(O.get(pk.VEC_U)))
            ep = float(np.abs(G.get(pk.VEC_P) - O.get(pk.VEC_P)).max() / np.abs(O.get(pk.VEC_P)).max())
            print(f"3 steps: |du| / |u| = {eu:.3e}, |dp|_inf / |p|_inf = {ep:.3e}, CG iterations {t1[1:, 6]}")
            assert eu <= 1e-8 and ep <= 1e-10, (eu, ep)
        finally:
            G.close()
    finally:
        O.close(); P.close()


def test_runner_takes_the_flag():
    P = problem((3, 3, 4), 2, COLUMN)
    R = pk.Runner(P, prec=pk.PREC_FDM, fdm_per_direction=True)
    try:
        R.initialize()                                                      # (the controls reach the context here)
        assert R.ctx.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PER_DIRECTION, (1, 1, 0))
        R.step()
        assert R.ctx.timer(FAMILY)[1] >= 1
    finally:
        R.close(); P.close()


def test_an_adaptive_run_keeps_the_flag_on_the_adapted_context():
    """refine_every = 2 over 3 steps: the context the run ends on was created by refine_mesh; it carries the request (its meshes are not boxes: the nodal kernels of the
    two-level form's coarse box run there, which ignores the request)"""
    n = (4, 4, 4)
    P = pk.Problem.refined_box_mask(3, list(n), [10.0] * 3, 1, material(), COLUMN, np.zeros(int(np.prod(n)), dtype=np.int32))
    try:
        t, G = pk.run_problem(P, 3, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, max_it=5000, prec=-1, fdm_per_direction=True, refine_every=2)
        try:
            assert G.problem is not P                                      # the mesh was adapted: a new context
            assert G.get_fdm_form()[0] == PER_DIRECTION
        finally:
            Q = G.problem; G.close()
            if Q is not P:
                Q.close()
    finally:
        P.close()


# ---- 5. setter semantics -----------------------------------------------------------------------------------------------------------------------------
def test_switching_the_form_between_solves_gives_the_bits_of_a_fresh_context():
    fresh = {}
    for form in (DEFAULT, PER_DIRECTION):
        P, G, _ = pcg_setup("q2", form)
        try:
            fresh[form] = pcg_solve(G)
        finally:
            G.close(); P.close()
    P, G, _ = pcg_setup("q2", PER_DIRECTION)
    try:
        for form in (PER_DIRECTION, DEFAULT, PER_DIRECTION, DEFAULT, DEFAULT, PER_DIRECTION):
            G.set_fdm_form(form)
            rc, it, u = pcg_solve(G)
            assert G.get_fdm_form()[:2] == (form, pk.FDM_RUNS_PER_DIRECTION if form == PER_DIRECTION else pk.FDM_RUNS_NODAL)
            assert rc == 0 and it == fresh[form][1] and np.array_equal(u, fresh[form][2]), (form, it, fresh[form][1])
        with pytest.raises(RuntimeError, match="poro_ctx_set_fdm_form: unknown form 7"):
            G.set_fdm_form(7)
        assert G.get_fdm_form()[0] == PER_DIRECTION                          # a refused value changes nothing
    finally:
        G.close(); P.close()


def test_the_environment_sets_the_initial_request():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "env"], env=dict(os.environ, PORO_FDMO_FORM="per-direction"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-3000:] + r.stderr[-3000:])


def _child(argv):
    if argv[0] == "separate_gz":
        assert os.environ.get("PORO_FDMO_SEPARATE_GZ")
        P, G, _ = pcg_setup(argv[1], PER_DIRECTION)
        rc, it, u = pcg_solve(G)
        assert rc == 0 and G.get_fdm_form()[1] == pk.FDM_RUNS_PER_DIRECTION
        np.save(argv[2], u)
        print(f"iterations={it}")
        G.close(); P.close()
    elif argv[0] == "env":
        P = problem((3, 4, 5), 2, COLUMN)
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        assert G.get_fdm_form() == (PER_DIRECTION, pk.FDM_RUNS_PER_DIRECTION, (1, 1, 0))       # requested without any call
        G.close(); P.close()
    else:
        raise SystemExit(f"unknown check {argv[0]}")
    print("child ok")


if __name__ == "__main__":
    _child(sys.argv[1:])

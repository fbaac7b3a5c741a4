"""Structured box operator for layered per-cell moduli (Context.set_moduli_operator(MODULI_OP_STRUCTURED), csrc/kernels_kron_lm.hip): the operator against the per-cell
NumPy reference and against the cell loop of the same context, bitwise repeatability, the constant field against the scalar structured kernel, clearing the field,
the cases where the request has no effect, CG solves (block FDM, Jacobi with the fused x . y, the unfused Chebyshev recurrence), a transient run and the driver.

Fields come from layer_decades through per_cell: lambda and G over three decades, a new pair in every cell layer of z, so every vertex plane is an interface.

Bounds: 1e-12 of max|y| for the operator (the project's bound for every operator path), 1e-13 of max|y| for the constant field against the scalar kernel, +-1 for CG
iteration counts, 1e-9 for solutions against a sparse direct solve (CG stops at 1e-12 ||rhs||), 1e-10 of the maxima for u and p of the transient run."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import poroelasticity_dealii_amd as pk
from common import BC_2D, BC_3D, material
from moduli_reference import FDM_CASES, MIXED3, ModuliReference, cell_centres, fdm_problem, layer_decades, per_cell

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, CELLS = pk.MODULI_OP_STRUCTURED, pk.MODULI_OP_CELLS


def synth(n, ph=0.0):
    return np.sin(0.37 * np.arange(n) + ph)


def err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def box3(n, deg, bc=BC_3D):
    return pk.Problem.box(3, list(n), [float(v) for v in n], deg, material(), bc)


def layered(P):
    """(lambda, G) per cell: a new pair in every cell layer of the slowest direction"""
    ll, lG = layer_decades(material(), len(np.unique(np.round(cell_centres(P)[:, -1], 9))))
    return per_cell(P, ll), per_cell(P, lG)


def general(P):
    """the same, modulated cell by cell: kind 2"""
    lam, G = layered(P)
    c = cell_centres(P)
    c3 = np.concatenate([c, np.zeros((len(c), 3 - c.shape[1]))], axis=1)
    return lam * (1 + 0.5 * np.sin(1.7 * c3[:, 0] + 2.3 * c3[:, 1] + 0.9 * c3[:, 2])), G * (1 + 0.4 * np.cos(0.8 * c3[:, 0] - 1.9 * c3[:, 1] + 1.3 * c3[:, 2]))


def ready(C, lam=None, G=None, form=None):
    """field, request, assembled system with p = 0"""
    if form is not None:
        C.set_moduli_operator(form)
    if lam is not None:
        C.set_cell_moduli(lam, G)
    C.fill(pk.VEC_P, 0.0)
    C.disp_assemble_system(True)
    return C


# ---- 1. the operator --------------------------------------------------------------------------------------------------------------------------------------------
# Q2: one cell; an odd plane count; several rows; 63 x 15 x 17 nodes = one 64-lane and one 32-lane tile column, two tile rows, several z-chunks with interfaces on the
# chunk boundaries.  Q1: 64 x 16 x 10 nodes, the same coverage for the 62 x 14 / 30 x 30 tiles
SHAPES = [(2, (1, 1, 1)), (2, (2, 1, 3)), (2, (5, 4, 3)), (2, (31, 7, 8)), (1, (3, 2, 1)), (1, (5, 4, 3)), (1, (63, 15, 9))]


@pytest.mark.parametrize("bc", [BC_3D, MIXED3], ids=["bc3d", "mixed3"])
@pytest.mark.parametrize("deg,n", SHAPES, ids=[f"q{d}-{'x'.join(map(str, n))}" for d, n in SHAPES])
def test_operator_against_the_reference_and_the_cell_loop(deg, n, bc):
    P = box3(n, deg, bc)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        lam, G = layered(P)
        R = ModuliReference(P, lam, G)
        x = synth(R.n_u)
        y0 = R.apply_A(x)
        ready(C, lam, G, ST)
        assert C.get_cell_moduli()[2] == 1 and C.get_moduli_operator() == (ST, ST)
        y = C.apply(pk.MAT_A_U, x)
        assert np.array_equal(C.apply(pk.MAT_A_U, x), y)                  # bitwise repeatable
        C.set_moduli_operator(CELLS)
        assert C.get_moduli_operator() == (CELLS, CELLS)
        yc = C.apply(pk.MAT_A_U, x)
        e0, e1 = err(y, y0), err(y, yc)
        print(f"Q{deg} {n}: structured vs reference {e0:.2e}, vs cell loop {e1:.2e} (cell loop vs reference {err(yc, y0):.2e})")
        assert np.all(np.isfinite(y)) and e0 <= 1e-12 and e1 <= 1e-12
    finally:
        C.close(); P.close()


# ---- 2. bitwise repeatability of applications and of a solve with the fused x . y ------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,n", [(2, (31, 7, 8)), (1, (63, 15, 9))], ids=["q2", "q1"])
def test_bitwise_repeatability(deg, n):
    P = box3(n, deg, MIXED3)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        lam, G = layered(P)
        C.set_moduli_operator(ST); C.set_cell_moduli(lam, G)
        C.set(pk.VEC_P, 1e7 * (1 + 0.2 * synth(C.n_p))); C.disp_assemble_system(True)
        assert C.get_moduli_operator()[1] == ST
        x = synth(C.n_u, 0.3)
        assert np.array_equal(C.apply(pk.MAT_A_U, x), C.apply(pk.MAT_A_U, x))
        runs = []
        for _ in range(2):
            C.fill(pk.VEC_U, 0.0)
            rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-6, max_iter=40, prec=pk.PREC_JACOBI)      # 40 iterations of the fused operator, converged or not
            runs.append((C.get(pk.VEC_U), info.iterations, info.final_residual))
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    finally:
        C.close(); P.close()


# ---- 3. a constant field is the scalar structured kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,n", [(2, (5, 4, 3)), (1, (5, 4, 3)), (2, (31, 7, 8))], ids=["q2", "q1", "q2-tiles"])
def test_constant_field_is_the_scalar_kernel(deg, n):
    P = box3(n, deg)
    m = P.desc.mat
    nc = P.desc.n_cells
    A, B = pk.Context(P, 0, pk.OP_MATRIX_FREE), pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        x = synth(A.n_u)
        ready(A)
        ready(B, np.full(nc, m.lame_lambda), np.full(nc, m.shear_G), ST)
        assert B.get_moduli_operator() == (ST, ST)
        e = err(B.apply(pk.MAT_A_U, x), A.apply(pk.MAT_A_U, x))
        print(f"Q{deg} {n}: constant field, structured layered kernel vs scalar kernel {e:.2e}")
        assert e <= 1e-13
    finally:
        A.close(); B.close(); P.close()


# ---- 4. clearing the field with the request still set ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [2, 1])
def test_clearing_the_field_restores_the_scalar_path_bitwise(deg):
    P = box3((5, 4, 3), deg)
    A, B = pk.Context(P, 0, pk.OP_MATRIX_FREE), pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        x = synth(A.n_u)
        p = 1e7 * (1 + 0.2 * synth(A.n_p))

        def run(C):
            C.set(pk.VEC_P, p); C.disp_assemble_system(True); C.fill(pk.VEC_U, 0.0)
            y = C.apply(pk.MAT_A_U, x)
            rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=50000, prec=pk.PREC_JACOBI)
            assert rc == 0
            return y, C.get(pk.VEC_DIAG_U), C.get(pk.VEC_RHS_U), C.get(pk.VEC_U), info.iterations
        base = run(A)
        lam, G = layered(P)
        B.set_moduli_operator(ST); B.set_cell_moduli(lam, G)
        assert B.get_moduli_operator() == (ST, ST)
        run(B)
        B.set_cell_moduli(None, None)
        assert B.get_moduli_operator() == (ST, CELLS) and B.get_cell_moduli() == (None, None, 0)
        back = run(B)
        for a, b in zip(back[:4], base[:4]):
            assert np.array_equal(a, b)
        assert back[4] == base[4]
        B.set_cell_moduli(lam, G)                                             # the request stayed: effective again with the next layered field
        assert B.get_moduli_operator() == (ST, ST)
    finally:
        A.close(); B.close(); P.close()


# ---- 5. where the form cannot apply -------------------------------------------------------------------------------------------------------------------------------
def refined_mask_problem(deg):
    mask = np.zeros((3, 4, 3), dtype=np.int32); mask[1, 1:3, 1] = 1; mask[0, 0, 0] = 1      # [z][y][x]
    return pk.Problem.refined_box_mask(3, [3, 4, 3], [3.0, 4.0, 3.0], deg, material(), BC_3D, mask)


INEFFECTIVE = {
    "kind2-q2": (lambda: box3((5, 4, 3), 2), general, pk.OP_MATRIX_FREE),
    "box2-q2": (lambda: pk.Problem.box(2, [7, 5], [7.0, 5.0], 2, material(), BC_2D), layered, pk.OP_MATRIX_FREE),
    "box2-q1": (lambda: pk.Problem.box(2, [6, 5], [6.0, 5.0], 1, material(), BC_2D), layered, pk.OP_MATRIX_FREE),
    "graded3-q2": (lambda: pk.Problem.graded_box(3, [4, 3, 5], [10.0] * 3, 2, material(), BC_3D, [1.0, 0.5, -0.7]), layered, pk.OP_MATRIX_FREE),
    "refined3-q2": (lambda: refined_mask_problem(2), layered, pk.OP_MATRIX_FREE),
    "csr-q2": (lambda: box3((5, 4, 3), 2), layered, pk.OP_CSR),
}


@pytest.mark.parametrize("name", list(INEFFECTIVE), ids=str)
def test_request_without_effect_changes_nothing(name):
    make, fld, mode = INEFFECTIVE[name]
    P = make()
    A, B = pk.Context(P, 0, mode), pk.Context(P, 0, mode)
    try:
        lam, G = fld(P)
        x = synth(A.n_u)
        p = 1e7 * (1 + 0.2 * synth(A.n_p))

        def run(C):
            C.set(pk.VEC_P, p); C.disp_assemble_system(True); C.fill(pk.VEC_U, 0.0)
            y = C.apply(pk.MAT_A_U, x)
            rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-10, max_iter=50000, prec=pk.PREC_JACOBI)
            assert rc == 0
            return y, C.get(pk.VEC_DIAG_U), C.get(pk.VEC_RHS_U), C.get(pk.VEC_U), info.iterations
        A.set_cell_moduli(lam, G)
        B.set_moduli_operator(ST); B.set_cell_moduli(lam, G)
        assert A.get_moduli_operator() == (CELLS, CELLS) and B.get_moduli_operator() == (ST, CELLS)
        a, b = run(A), run(B)
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(u, v)
        assert a[4] == b[4]
    finally:
        A.close(); B.close(); P.close()


def test_environment_variable_and_unknown_form(monkeypatch):
    P = box3((2, 1, 3), 2)
    monkeypatch.setenv("PORO_MODULI_OPERATOR", "structured")
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    monkeypatch.delenv("PORO_MODULI_OPERATOR")
    D = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert C.get_moduli_operator() == (ST, CELLS) and D.get_moduli_operator() == (CELLS, CELLS)      # no field yet
        lam, G = layered(P)
        C.set_cell_moduli(lam, G)
        assert C.get_moduli_operator() == (ST, ST)
        with pytest.raises(RuntimeError, match="unknown form"):
            C.set_moduli_operator(2)
        assert C.get_moduli_operator() == (ST, ST)
        C.set_scatter_mode(pk.SCATTER_ATOMIC)                                 # stored and reported, not used while the form is effective
        assert C.get_scatter_mode() == pk.SCATTER_ATOMIC
    finally:
        C.close(); D.close(); P.close()


# ---- 6. solves ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [pk.PREC_FDM, pk.PREC_JACOBI, pk.PREC_CHEBYSHEV], ids=["fdm", "jacobi", "chebyshev"])      # Jacobi: the fused x . y; Chebyshev: the unfused recurrence
@pytest.mark.parametrize("name", ["q2-5x4x6-mixed", "q1-5x4x6-mixed"])
def test_cg_solves(name, prec):
    m = material()
    P, bc = fdm_problem(name, m)
    ll, lG = layer_decades(m, FDM_CASES[name][1][-1])
    lam, G = per_cell(P, ll), per_cell(P, lG)
    got = {}
    try:
        for form in (ST, CELLS):
            C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
            try:
                C.set_moduli_operator(form); C.set_cell_moduli(lam, G)
                C.set(pk.VEC_P, 1e7 * (1 + 0.2 * synth(C.n_p))); C.disp_assemble_system(True)
                assert C.get_moduli_operator()[1] == form
                rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=50000, prec=prec)
                assert rc == 0
                got[form] = (C.get(pk.VEC_U), info.iterations, C.get(pk.VEC_RHS_U))
            finally:
                C.close()
        R = ModuliReference(P, lam, G)
        free = np.flatnonzero(~R.mask)
        want = spl.spsolve(R.assemble()[free][:, free].tocsc(), got[ST][2][free])
        e = np.linalg.norm(got[ST][0][free] - want) / np.linalg.norm(want)
        print(f"{name} prec {prec}: {got[ST][1]} iterations structured, {got[CELLS][1]} cell loop; solution vs spsolve {e:.2e}")
        assert np.array_equal(got[ST][2], got[CELLS][2])                      # the right-hand side is a set-up quantity: the cell loop in both
        assert abs(got[ST][1] - got[CELLS][1]) <= 1 and e <= 1e-9
    finally:
        P.close()


# ---- 7. transient run -----------------------------------------------------------------------------------------------------------------------------------------------
def test_transient_run_matches_the_cell_loop():
    """three steps of a layered 4 x 4 x 6 Q2 column (held at the bottom, loaded at its drained top, a stiff caprock of two cell layers)"""
    height, sigma0 = 6.0, 1e5
    bc = [(2 * d, d, 0.0) for d in range(2)] + [(2 * d + 1, d, 0.0) for d in range(2)] + [(4, c, 0.0) for c in range(3)]
    runs = {}
    for structured in (True, False):
        P = pk.Problem.box(3, [4, 4, 6], [4.0, 4.0, height], 2, material(flow_rate=0.0), bc, [(5, 2, -sigma0)])
        P.set_pressure_bc([(5, 0.0)])
        cap = height / 2 - 2 * height / 6
        P.set_moduli_layers([(cap, 1.4e10, 0.3), (height / 2, 1.4e12, 0.25)])
        try:
            trace, G = pk.run_problem(P, 3, 1e5, 60.0, device=0, operator_mode=pk.OP_MATRIX_FREE, fss_tol=1e-11, pressure_tol=1e-11, max_fss=200, max_it=50000, prec=-1,
                                      coupled_fss=True, moduli_structured=structured)
            try:
                assert G.get_cell_moduli()[2] == 1 and G.get_moduli_operator() == ((ST, ST) if structured else (CELLS, CELLS))
                runs[structured] = (trace[:, :3].copy(), G.get(pk.VEC_U), G.get(pk.VEC_P))
            finally:
                G.close()
        finally:
            P.close()
    (t1, u1, p1), (t0, u0, p0) = runs[True], runs[False]
    eu, ep = np.abs(u1 - u0).max() / np.abs(u0).max(), np.abs(p1 - p0).max() / np.abs(p0).max()
    print(f"{len(t1)} trace rows; u {eu:.2e} p {ep:.2e}")
    assert np.array_equal(t1, t0)                                             # fixed-stress and pressure iteration counts of every step
    assert eu <= 1e-10 and ep <= 1e-10


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------------------------------------------
def test_driver_prints_the_effective_form(tmp_path):
    exe = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
    data2 = os.path.join(ROOT, "tests", "golden", "input.data")               # 2D: [-5, 5]^2
    text = open(data2).read()
    for old, new in (("= 2\n", "= 3\n"), ("= 10, 10\n", "= 4, 4, 4\n"), ("level = 4\n", "level = 2\n"), ("labels     = 0, 1, 2, 3\n", "labels     = 0, 1, 2, 3, 4\n"),
                     ("components = 0, 0, 1, 1\n", "components = 0, 0, 1, 1, 2\n"), ("values     = 0, -1e-5, 0, -1e-5\n", "values     = 0, -1e-5, 0, -1e-5, 0\n")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    data3 = str(tmp_path / "input3d.data")                                    # 3D: 4^3 cells on [-2, 2]^3, held at the bottom in z
    open(data3, "w").write(text)
    r = subprocess.run([exe, data3, "--matrix-free", "--fastest", "--steps", "1", "--moduli-layers", "0=1.4e10:0.3,2=1.4e12:0.25", "--moduli-structured"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "moduli layers: 2, field kind 1; displacement preconditioner: FDM; moduli operator: structured" in r.stdout
    r = subprocess.run([exe, data2, "--matrix-free", "--fastest", "--steps", "1", "--moduli-layers", "0=1.4e10:0.3,5=1.4e12:0.25", "--moduli-structured"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "moduli layers: 2, field kind 1; displacement preconditioner: FDM; moduli operator: cell loop" in r.stdout      # a 2D box: the request has no effect

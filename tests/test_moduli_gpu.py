"""Per-cell Lame lambda and shear modulus G of the displacement system (Context.set_cell_moduli): operator, diagonal, assembled matrix and lifting on every path
against the per-cell NumPy reference (tests/moduli_reference.py), the constant field against the scalar path, a layered column with a known answer, the nodal
constants of the stresses and of the fixed-stress update, the refusals, PREC_FDM with a field (the exact block inverse on layered fields, the layer-mean preconditioner
otherwise, CG iteration counts against a NumPy PCG with the same preconditioner), and time steps, adaptation and the driver end to end.

Fields: lambda and G take values over three decades, layer by layer along the slowest direction (kind 1 on boxes and tensor-product grids) and, for kind 2,
modulated cell by cell.

Bounds: 1e-12 of max|y| for operator and diagonal (the project's bound for the general kernels), 1e-13 of max|A| for CSR values, 1e-13 of max|y| for the constant
field against the scalar path, 1e-9 where two CG solves stop at 1e-12 ||rhs|| and for the analytic column, 1e-10 of max|z| for the block inverse (the project's bound
for it), +-1 for iteration counts against the NumPy PCG."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, BC_3D, DOMAIN_MSH, csr_to_scipy, material
from moduli_reference import ModuliReference, cell_centres

pytestmark = pytest.mark.gpu


def decade(k):
    return 10.0 ** (-3 * ((7 * int(k)) % 5) / 4)          # 1, 10^-0.75, ... 10^-3 in a scrambled order


def field(P, kind, bands=5):
    """(lambda, G) per cell: bands of the slowest coordinate (cells of one cell layer share a band), lambda and G with different band orders; kind 2: times a cell-wise factor"""
    m = P.desc.mat
    c = cell_centres(P)
    z = c[:, -1]
    band = np.minimum((bands * (z - z.min()) / max(z.max() - z.min(), 1e-300) * (1 - 1e-12)).astype(int), bands - 1) if z.max() > z.min() else np.zeros(len(z), int)
    lam = m.lame_lambda * np.array([decade(b) for b in band])
    G = m.shear_G * np.array([decade(b + 2) for b in band])
    if kind == 2:
        c3 = np.concatenate([c, np.zeros((len(c), 3 - c.shape[1]))], axis=1)
        lam = lam * (1 + 0.5 * np.sin(1.7 * c3[:, 0] + 2.3 * c3[:, 1] + 0.9 * c3[:, 2]))
        G = G * (1 + 0.4 * np.cos(0.8 * c3[:, 0] - 1.9 * c3[:, 1] + 1.3 * c3[:, 2]))
    return lam, G


def refined_mask_problem(deg):
    mask = np.zeros((3, 4, 3), dtype=np.int32); mask[1, 1:3, 1] = 1; mask[0, 0, 0] = 1      # [z][y][x]
    return pk.Problem.refined_box_mask(3, [3, 4, 3], [3.0, 4.0, 3.0], deg, material(), BC_3D, mask)


PROBLEMS = {
    "box3-q2-5x4x3": lambda: pk.Problem.box(3, [5, 4, 3], [5.0, 4.0, 3.0], 2, material(), BC_3D),      # 60 cells: a partial workgroup of 8
    "box3-q2-2x1x3": lambda: pk.Problem.box(3, [2, 1, 3], [2.0, 1.0, 3.0], 2, material(), BC_3D),
    "box3-q2-1x1x1": lambda: pk.Problem.box(3, [1, 1, 1], [1.0, 1.0, 1.0], 2, material(), BC_3D),
    "box3-q1-5x4x3": lambda: pk.Problem.box(3, [5, 4, 3], [5.0, 4.0, 3.0], 1, material(), BC_3D),
    "box2-q2-7x5": lambda: pk.Problem.box(2, [7, 5], [7.0, 5.0], 2, material(), BC_2D),
    "box2-q1-6x5": lambda: pk.Problem.box(2, [6, 5], [6.0, 5.0], 1, material(), BC_2D),
    "graded3-q2": lambda: pk.Problem.graded_box(3, [4, 3, 5], [10.0] * 3, 2, material(), BC_3D, [1.0, 0.5, -0.7]),
    "graded2-q1": lambda: pk.Problem.graded_box(2, [5, 6], [10.0] * 2, 1, material(), BC_2D, [0.8, -1.1]),
    "gmsh-q2": lambda: pk.Problem.gmsh(DOMAIN_MSH, 2, material(), BC_2D),
    "gmsh-q1": lambda: pk.Problem.gmsh(DOMAIN_MSH, 1, material(), BC_2D),
    "refined3-q2": lambda: refined_mask_problem(2),
    "refined3-q1": lambda: refined_mask_problem(1),
}
LINES = ("box", "graded")       # mesh classes with lines.on: layered fields are kind 1 there


def expected_kind(P, name, lam, G):
    """1: a mesh with grid lines and both arrays exactly constant within every cell layer of the slowest direction (a box of one cell per layer is layered)"""
    if not name.startswith(LINES):
        return 2
    z = np.round(cell_centres(P)[:, -1], 9)
    return 1 if all(len(np.unique(lam[z == v])) == 1 and len(np.unique(G[z == v])) == 1 for v in np.unique(z)) else 2


def synth(n, ph=0.0):
    return np.sin(0.37 * np.arange(n) + ph)


def err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ---- 1. operator, diagonal, matrix, lifting ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", list(PROBLEMS), ids=str)
def test_operator_diagonal_matrix(name, kind):
    P = PROBLEMS[name]()
    lam, G = field(P, kind)
    R = ModuliReference(P, lam, G)
    x = synth(R.n_u)
    y0, d0 = R.apply_A(x), R.diag_A()
    free = ~R.mask
    g = np.zeros(R.n_u); g[R.dir_dof] = R.dir_val
    lift0 = -R.apply_full(g)
    hanging = P.desc.cons_u.n > 0
    rhs = {}
    try:
        for label, mode, scatter in (("mf-coloured", pk.OP_MATRIX_FREE, pk.SCATTER_COLOURED), ("mf-atomic", pk.OP_MATRIX_FREE, pk.SCATTER_ATOMIC), ("csr", pk.OP_CSR, None)):
            C = pk.Context(P, 0, mode)
            try:
                C.set_cell_moduli(lam, G)
                if scatter is not None:
                    C.set_scatter_mode(scatter)
                    assert C.get_scatter_mode() == scatter          # (honoured on a box with a field as well)
                glam, gG, gkind = C.get_cell_moduli()
                assert np.array_equal(glam, lam) and np.array_equal(gG, G)
                assert gkind == expected_kind(P, name, lam, G), (name, gkind)
                C.fill(pk.VEC_P, 0.0)
                C.disp_assemble_system(False)                        # the setter dropped the system: rebuilt whatever the flag says
                ey, ed = err(C.apply(pk.MAT_A_U, x), y0), err(C.get(pk.VEC_DIAG_U), d0)
                print(f"{name} kind {kind} {label}: operator {ey:.2e} diagonal {ed:.2e}")
                assert ey <= 1e-12 and ed <= 1e-12
                rhs[label] = C.get(pk.VEC_RHS_U)
                if not hanging:                                       # p = 0, no traction: the right-hand side of a free row is the lifting -(A_full g)
                    el = np.abs(rhs[label] - lift0)[free].max() / max(np.abs(lift0).max(), 1e-300)
                    print(f"   lifting {el:.2e}")
                    assert el <= 1e-12
                if mode == pk.OP_CSR:
                    A, A0 = csr_to_scipy(*C.export_csr(pk.MAT_A_U)), R.assemble()
                    ea = abs(A - A0).max() / abs(A0).max()
                    print(f"   MAT_A_U {ea:.2e}")
                    assert ea <= 1e-13
            finally:
                C.close()
        if hanging:      # condensed right-hand side with non-zero Dirichlet values: the cell-loop lifting against the assembly kernel's
            scale = np.abs(rhs["csr"]).max()
            assert np.abs(rhs["mf-coloured"] - rhs["csr"]).max() <= 1e-12 * scale and np.abs(rhs["mf-atomic"] - rhs["csr"]).max() <= 1e-12 * scale
    finally:
        P.close()


@pytest.mark.parametrize("name", ["refined3-q2", "refined3-q1", "box3-q2-2x1x3", "gmsh-q2"])
def test_solutions_of_the_paths_agree(name):
    """Jacobi-CG to 1e-12 ||rhs|| on the matrix-free and the assembled operator, and the reference's residual: with p = 0 and no traction the unconstrained product
    A_full u vanishes on every row that is neither constrained nor the master of a hanging dof"""
    P = PROBLEMS[name]()
    lam, G = field(P, 2)
    R = ModuliReference(P, lam, G)
    sol = {}
    try:
        for label, mode in (("mf", pk.OP_MATRIX_FREE), ("csr", pk.OP_CSR)):
            C = pk.Context(P, 0, mode)
            try:
                C.set_cell_moduli(lam, G); C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
                rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=50000, prec=pk.PREC_JACOBI)
                assert rc == 0
                sol[label] = C.get(pk.VEC_U)
            finally:
                C.close()
        e = np.linalg.norm(sol["mf"] - sol["csr"]) / np.linalg.norm(sol["csr"])
        r = R.apply_full(sol["mf"])
        inner = ~R.mask
        c = P.desc.cons_u
        if c.n:
            from test_constraints_cpu import cons_arrays
            dof, ptr, master, _, _ = cons_arrays(c)
            inner[dof] = False; inner[master] = False
        er = np.abs(r[inner]).max() / np.abs(r).max()
        print(f"{name}: mf vs csr {e:.2e}, interior residual of the reference / largest reaction {er:.2e}")
        assert e <= 1e-9 and er <= 1e-9
    finally:
        P.close()


# ---- 2. constant field against the scalar path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pk.OP_MATRIX_FREE, pk.OP_CSR], ids=["mf", "csr"])
@pytest.mark.parametrize("name", ["box3-q2-5x4x3", "box2-q1-6x5", "graded3-q2", "gmsh-q2"])
def test_constant_field_is_the_scalar_path_and_clearing_restores_it(name, mode):
    P = PROBLEMS[name]()
    m = P.desc.mat
    n = P.desc.n_cells
    A, B = pk.Context(P, 0, mode), pk.Context(P, 0, mode)
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
        B.set_cell_moduli(np.full(n, m.lame_lambda), np.full(n, m.shear_G))
        assert B.get_cell_moduli()[2] == (1 if name.startswith(LINES) else 2)
        got = run(B)
        ey, ed, eu = err(got[0], base[0]), err(got[1], base[1]), np.linalg.norm(got[3] - base[3]) / np.linalg.norm(base[3])
        print(f"{name}: constant field vs scalar: operator {ey:.2e} diagonal {ed:.2e} solution {eu:.2e}")
        assert ey <= 1e-13 and ed <= 1e-13 and eu <= 1e-9
        B.set_cell_moduli(None, None)
        assert B.get_cell_moduli() == (None, None, 0)
        with pytest.raises(RuntimeError, match="disp_assemble_system"):
            B.disp_solve()
        back = run(B)
        for a, b in zip(back[:4], base[:4]):
            assert np.array_equal(a, b)
        assert back[4] == base[4]
    finally:
        A.close(); B.close(); P.close()


# ---- 3. a layered column with a known answer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pk.OP_MATRIX_FREE, pk.OP_CSR], ids=["mf", "csr"])
@pytest.mark.parametrize("dim,deg", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_layered_column(dim, deg, mode):
    """lateral rollers, fixed bottom, uniform vertical traction t on top, p = 0, layers aligned with cell faces: u_vertical is piecewise linear with slope
    t / (lambda_l + 2 G_l) in layer l, the other components vanish - exact in the FE space, independent of every reference"""
    n = [3, 4] if dim == 2 else [2, 3, 4]
    t = -2.5e6
    last = dim - 1
    bc = [(2 * d, d, 0.0) for d in range(dim)] + [(2 * d + 1, d, 0.0) for d in range(last)]
    P = pk.Problem.box(dim, n, [float(v) for v in n], deg, material(), bc, [(2 * last + 1, last, t)])
    m = P.desc.mat
    layer_lam = m.lame_lambda * np.array([1.0, 1e-3, 0.2, 3e-2])
    layer_G = m.shear_G * np.array([1e-2, 1.0, 1e-3, 0.5])
    c = cell_centres(P)
    layer = np.floor(c[:, last] - (c[:, last].min() - 0.5) + 1e-9).astype(int)
    C = pk.Context(P, 0, mode)
    try:
        C.set_cell_moduli(layer_lam[layer], layer_G[layer])
        assert C.get_cell_moduli()[2] == 1
        C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
        rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=50000, prec=pk.PREC_JACOBI)
        assert rc == 0
        u = C.get(pk.VEC_U).reshape(-1, dim)
        R = ModuliReference(P, layer_lam[layer], layer_G[layer])
        X, comp = R.node_coords()
        z = X[::dim, last] - X[:, last].min()
        slope = t / (layer_lam + 2 * layer_G)
        knots = np.concatenate([[0.0], np.cumsum(slope)])                   # cells of edge 1
        exact = np.interp(z, np.arange(len(knots)), knots)
        e = max(np.abs(u[:, last] - exact).max(), np.abs(np.delete(u, last, axis=1)).max()) / np.abs(exact).max()
        print(f"column {dim}D Q{deg}: {info.iterations} iterations, error {e:.2e} of max|u|")
        assert e <= 1e-9
    finally:
        C.close(); P.close()


# ---- 4. stresses and the fixed-stress update ------------------------------------------------------------------------------------------------------------------
def nodal_means(P, lam, G):
    d = P.desc
    cd = P.array("cell_dofs_p", (d.n_cells, 1 << d.dim), np.int32)
    cnt = np.bincount(cd.ravel(), minlength=d.n_dofs_p)
    return (np.bincount(cd.ravel(), weights=np.repeat(lam, cd.shape[1]), minlength=d.n_dofs_p) / cnt,
            np.bincount(cd.ravel(), weights=np.repeat(G, cd.shape[1]), minlength=d.n_dofs_p) / cnt)


@pytest.mark.parametrize("name", ["box3-q2-2x1x3", "box2-q1-6x5", "refined3-q1"])
def test_stresses_and_strain_update_use_nodal_means(name):
    P = PROBLEMS[name]()
    m = P.desc.mat
    dim, n = P.desc.dim, P.desc.n_cells
    ne = dim * (dim + 1) // 2
    diag = (0, 2) if dim == 2 else (0, 3, 5)
    A, B = pk.Context(P, 0, pk.OP_MATRIX_FREE), pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        eps = [1e-4 * synth(A.n_p, 0.7 * k) for k in range(ne)]
        dp, ev0 = 1e6 * synth(A.n_p, 2.0), 1e-4 * synth(A.n_p, 3.0)

        def run(C):
            for k in range(ne):
                C.set(pk.VEC_STRAIN0 + k, eps[k])
            C.set(pk.VEC_DP, dp); C.set(pk.VEC_EPSV, ev0)
            C.get_effective_stresses(); C.pres_update_volumetric_strain()
            return [C.get(pk.VEC_STRESS0 + k) for k in range(ne)], C.get(pk.VEC_EPSV)
        s0, e0 = run(A)
        # one material: the scalar path (its bulk modulus is lambda + 2 G / 3 up to rounding)
        B.set_cell_moduli(np.full(n, m.lame_lambda), np.full(n, m.shear_G))
        s1, e1 = run(B)
        for k in range(ne):
            assert err(s1[k], s0[k]) <= 1e-14
        assert np.abs((e1 - ev0) - (e0 - ev0)).max() <= 1e-13 * np.abs(e0 - ev0).max()
        # two layers: the definition, from the strains the device holds
        z = cell_centres(P)[:, -1]
        upper = z > 0.5 * (z.min() + z.max())
        lam, G = np.where(upper, 50.0, 1.0) * m.lame_lambda, np.where(upper, 0.02, 1.0) * m.shear_G
        B.set_cell_moduli(lam, G)
        s2, e2 = run(B)
        nl, nG = nodal_means(P, lam, G)
        assert len(np.unique(nl)) >= 3                                       # both layers and the interface mean
        tr = sum(eps[k] for k in diag)
        for k in range(ne):
            want = 2 * nG * eps[k] + (nl * tr if k in diag else 0.0)
            assert err(s2[k], want) <= 1e-14
        want = m.biot_alpha / (nl + 2 * nG / 3) * dp
        assert np.abs((e2 - ev0) - want).max() <= 1e-13 * np.abs(want).max()
    finally:
        A.close(); B.close(); P.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    P = PROBLEMS["box3-q1-5x4x3"]()
    m = P.desc.mat
    n = P.desc.n_cells
    lam, G = np.full(n, m.lame_lambda), np.full(n, m.shear_G)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        cases = [((np.r_[lam, 1.0], np.r_[G, 1.0]), "n_cells"), ((lam, None), "come together"), ((None, G), "come together"),
                 ((np.r_[lam[:-1], np.nan], G), f"cell {n - 1} are not finite"), ((lam, np.r_[G[:-1], np.inf]), f"cell {n - 1} are not finite"),
                 ((lam, np.r_[0.0, G[1:]]), "shear_G of cell 0 is not > 0"), ((np.r_[lam[:3], -G[3], lam[4:]], G), r"3 lambda \+ 2 G of cell 3")]
        for (a, b), word in cases:
            with pytest.raises(RuntimeError, match=word):
                C.set_cell_moduli(a, b)
            assert C.get_cell_moduli() == (None, None, 0)
        assert C.supports_preconditioner(0, pk.PREC_FDM)
    finally:
        C.close(); P.close()
    # partitioned contexts: the test hook of the partitioned code path, and a 2-slab descriptor
    monkeypatch.setenv("PORO_FORCE_PARTITIONED_PATH", "1")
    P = PROBLEMS["box3-q1-5x4x3"](); C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    monkeypatch.delenv("PORO_FORCE_PARTITIONED_PATH")
    try:
        with pytest.raises(RuntimeError, match="one rank"):
            C.set_cell_moduli(lam, G)
    finally:
        C.close(); P.close()
    P = pk.Problem.box(3, [3, 2, 4], [3.0, 2.0, 4.0], 1, material(), BC_3D, (), 0, 2); C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        with pytest.raises(RuntimeError, match="one rank"):
            C.set_cell_moduli(np.ones(P.desc.n_cells), np.ones(P.desc.n_cells))
    finally:
        C.close(); P.close()


def test_two_level_and_hybrid_are_refused_with_a_field():
    P = pk.Problem.refined_box(3, [4, 4, 4], [4.0] * 3, 2, material(), BC_3D, [1, 1, 1], [3, 3, 3])
    lam, G = field(P, 2)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert C.supports_preconditioner(0, pk.PREC_TWO_LEVEL)
        C.set_cell_moduli(lam, G); C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
        assert not C.supports_preconditioner(0, pk.PREC_TWO_LEVEL)
        with pytest.raises(RuntimeError, match="constant-coefficient"):
            C.disp_solve(prec=pk.PREC_TWO_LEVEL)
        with pytest.raises(RuntimeError, match="PORO_OPFORM_HYBRID"):
            C.set_operator_form(pk.OPFORM_HYBRID)
        assert C.get_operator_form()[0] == pk.OPFORM_GENERAL
        assert C.supports_preconditioner(0, pk.PREC_CHEBYSHEV) and C.supports_preconditioner(0, pk.PREC_JACOBI)
        rc, _ = C.disp_solve(abs_tol=0.0, rel_tol=1e-10, max_iter=50000, prec=pk.PREC_CHEBYSHEV)
        assert rc == 0
        # the other order: a context already in the hybrid form refuses the field
        C.set_cell_moduli(None, None)
        C.set_operator_form(pk.OPFORM_HYBRID)
        with pytest.raises(RuntimeError, match="PORO_OPFORM_HYBRID"):
            C.set_cell_moduli(lam, G)
        assert C.get_cell_moduli() == (None, None, 0) and C.get_operator_form()[0] == pk.OPFORM_HYBRID
    finally:
        C.close(); P.close()


# ---- 6. PREC_FDM with a field: the exact block inverse (kind 1), the layer-mean preconditioner (kind 2) -----------------------------------------------------------
import scipy.sparse.linalg as spl                                            # noqa: E402
from moduli_reference import FDM_CASES, fdm_problem, layer_decades, layer_means, per_cell     # noqa: E402


def block_solver(R):
    """g -> blockdiag(A_cc)^-1 g on the free dofs, 0 on the Dirichlet dofs"""
    free = np.flatnonzero(~R.mask)
    lu = spl.splu(R.block_diagonal()[free][:, free].tocsc())

    def solve(g):
        z = np.zeros(R.n_u); z[free] = lu.solve(np.asarray(g)[free])
        return z
    return solve


def numpy_pcg(A, b, prec, tol, max_iter=2000):
    """SolverCG's recurrence with a preconditioner; stops at ||r|| <= tol; returns (x, iterations)"""
    x = np.zeros_like(b); r = b.copy(); z = prec(r); d = z.copy(); rz = r @ z
    for it in range(1, max_iter + 1):
        h = A @ d
        alpha = rz / (d @ h)
        x += alpha * d; r -= alpha * h
        if np.linalg.norm(r) <= tol:
            return x, it
        z = prec(r); rz_new = r @ z
        d = z + (rz_new / rz) * d; rz = rz_new
    return x, max_iter


def layered(name, scale=1.0):
    m = material()
    P, bc = fdm_problem(name, m)
    ll, lG = layer_decades(m, FDM_CASES[name][1][-1], scale)
    return P, per_cell(P, ll), per_cell(P, lG)


@pytest.mark.parametrize("name", list(FDM_CASES), ids=str)
def test_fdm_is_the_exact_block_inverse_on_layered_fields(name):
    P, lam, G = layered(name)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        C.set_cell_moduli(lam, G)
        assert C.get_cell_moduli()[2] == 1 and C.supports_preconditioner(0, pk.PREC_FDM)
        C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
        R = ModuliReference(P, lam, G)
        g = synth(R.n_u, 0.4)
        want = block_solver(R)(g)
        z = C.apply_preconditioner_u(pk.PREC_FDM, g)
        e = np.abs(z - want).max() / np.abs(want).max()
        print(f"{name}: block inverse {e:.2e} of max|z|")
        assert np.all(np.isfinite(z)) and np.all(z[R.mask] == 0.0) and e <= 1e-10
    finally:
        C.close(); P.close()


def test_fdm_scaled_field_with_removed_modes_stays_finite():
    """the field times 1e12, u_x fixed on both x faces (two removed x modes per line): nothing non-finite, the same relative accuracy"""
    P, lam, G = layered("q2-5x4x6-mixed", 1e12)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        C.set_cell_moduli(lam, G); C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
        R = ModuliReference(P, lam, G)
        g = synth(R.n_u, 1.1)
        want = block_solver(R)(g)
        z = C.apply_preconditioner_u(pk.PREC_FDM, g)
        assert np.all(np.isfinite(z)) and np.all(z[R.mask] == 0.0)
        assert np.abs(z - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        C.close(); P.close()


@pytest.mark.parametrize("how", ["fp32", "per-direction", "env"])
def test_fdm_settings_of_the_other_forms_are_ignored(how, monkeypatch):
    if how == "env":
        monkeypatch.setenv("PORO_FDMO_PRECISION", "fp32"); monkeypatch.setenv("PORO_FDMO_FORM", "per-direction")
    P, lam, G = layered("q2-5x4x6-mixed")
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        if how == "fp32":
            C.set_fdm_precision(pk.FDM_FP32)
        if how == "per-direction":
            C.set_fdm_form(pk.FDM_FORM_PER_DIRECTION)
        C.set_cell_moduli(lam, G); C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
        assert C.get_fdm_precision()[1] == pk.FDM_FP64 and C.get_fdm_form()[1] == pk.FDM_RUNS_NODAL
        R = ModuliReference(P, lam, G)
        g = synth(R.n_u, 0.4)
        want = block_solver(R)(g)
        assert np.abs(C.apply_preconditioner_u(pk.PREC_FDM, g) - want).max() <= 1e-10 * np.abs(want).max()
        # without the field the tables of the scalars are rebuilt (in whatever form the settings select): the block inverse of the constant material
        C.set_cell_moduli(None, None); C.disp_assemble_system(True)
        m = P.desc.mat
        want = block_solver(ModuliReference(P, np.full(P.desc.n_cells, m.lame_lambda), np.full(P.desc.n_cells, m.shear_G)))(g)
        z = C.apply_preconditioner_u(pk.PREC_FDM, g)
        assert np.abs(z - want).max() <= (1e-10 if C.get_fdm_precision()[1] == pk.FDM_FP64 else 1e-4) * np.abs(want).max()
    finally:
        C.close(); P.close()


@pytest.mark.parametrize("mode", [pk.OP_MATRIX_FREE, pk.OP_CSR], ids=["mf", "csr"])
@pytest.mark.parametrize("name", ["q2-5x4x6-mixed", "q1-5x4x6-mixed", "2d-q2-5x4-mixed", "q2-graded-4x3x5-bottom"])
def test_cg_with_a_layered_field(name, mode):
    P, lam, G = layered(name)
    C = pk.Context(P, 0, mode)
    try:
        C.set_cell_moduli(lam, G)
        C.set(pk.VEC_P, 1e7 * (1 + 0.2 * synth(C.n_p))); C.disp_assemble_system(True)
        rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=500, prec=pk.PREC_FDM)
        assert rc == 0
        R = ModuliReference(P, lam, G)
        free = np.flatnonzero(~R.mask)
        A = R.assemble()[free][:, free].tocsr()
        b = C.get(pk.VEC_RHS_U)
        u = C.get(pk.VEC_U)
        want = spl.spsolve(A.tocsc(), b[free])
        prec = block_solver(R)
        full = lambda v: np.bincount(free, weights=v, minlength=R.n_u)       # noqa: E731
        _, it = numpy_pcg(A, b[free], lambda r: prec(full(r))[free], 1e-12 * np.linalg.norm(b[free]))
        e = np.linalg.norm(u[free] - want) / np.linalg.norm(want)
        print(f"{name}: FDM-CG {info.iterations} iterations (numpy PCG with the exact block inverse: {it}), solution {e:.2e}")
        assert e <= 1e-9 and abs(info.iterations - it) <= 1
    finally:
        C.close(); P.close()


@pytest.mark.parametrize("name", ["q2-5x4x6-mixed", "2d-q1-6x5-both"])
def test_cg_with_a_general_field_uses_the_layer_means(name):
    m = material()
    P, bc = fdm_problem(name, m)
    ll, lG = layer_decades(m, FDM_CASES[name][1][-1])
    c3 = np.concatenate([cell_centres(P), np.zeros((P.desc.n_cells, 3 - P.desc.dim))], axis=1)
    lam = per_cell(P, ll) * (1 + 0.5 * np.sin(1.7 * c3[:, 0] + 2.3 * c3[:, 1] + 0.9 * c3[:, 2]))      # layers over three decades, modulated cell by cell
    G = per_cell(P, lG) * (1 + 0.4 * np.cos(0.8 * c3[:, 0] - 1.9 * c3[:, 1] + 1.3 * c3[:, 2]))
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        C.set_cell_moduli(lam, G)
        assert C.get_cell_moduli()[2] == 2 and C.supports_preconditioner(0, pk.PREC_FDM)
        C.set(pk.VEC_P, 1e7 * (1 + 0.2 * synth(C.n_p))); C.disp_assemble_system(True)
        rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=2000, prec=pk.PREC_FDM)
        u = C.get(pk.VEC_U)
        C.fill(pk.VEC_U, 0.0)
        rcj, infoj = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=20000, prec=pk.PREC_JACOBI)
        assert rc == 0 and rcj == 0
        R = ModuliReference(P, lam, G)
        Rm = ModuliReference(P, per_cell(P, layer_means(P, lam)), per_cell(P, layer_means(P, G)))
        free = np.flatnonzero(~R.mask)
        A = R.assemble()[free][:, free].tocsr()
        b = C.get(pk.VEC_RHS_U)
        prec = block_solver(Rm)
        full = lambda v: np.bincount(free, weights=v, minlength=R.n_u)       # noqa: E731
        _, it = numpy_pcg(A, b[free], lambda r: prec(full(r))[free], 1e-12 * np.linalg.norm(b[free]))
        x = spl.spsolve(A.tocsc(), b[free])
        e = np.linalg.norm(u[free] - x) / np.linalg.norm(x)
        print(f"{name}: layer-mean FDM-CG {info.iterations} iterations (numpy: {it}), Jacobi {infoj.iterations}; solutions {e:.2e}")
        assert abs(info.iterations - it) <= 1 and info.iterations < infoj.iterations and e <= 1e-9
    finally:
        C.close(); P.close()


def test_supports_preconditioner_is_the_verdict_with_a_field():
    for name, fdm in (("box3-q2-2x1x3", True), ("graded3-q2", True), ("gmsh-q1", False), ("refined3-q1", False)):
        P = PROBLEMS[name]()
        lam, G = field(P, 2)
        C = pk.Context(P, 0, pk.OP_CSR)
        try:
            C.set_cell_moduli(lam, G); C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
            assert C.supports_preconditioner(0, pk.PREC_FDM) == fdm, name
            assert not C.supports_preconditioner(0, pk.PREC_TWO_LEVEL)
            if not P.desc.cons_u.n:
                assert C.supports_preconditioner(0, pk.PREC_ILU0) and C.supports_preconditioner(0, pk.PREC_SSOR)
            if name == "box3-q2-2x1x3":                                     # the sweeps follow the assembled matrix by themselves: one small solve each
                for prec in (pk.PREC_ILU0, pk.PREC_SSOR):
                    C.fill(pk.VEC_U, 0.0)
                    rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-10, max_iter=2000, prec=prec)
                    assert rc == 0
            if not fdm:
                with pytest.raises(RuntimeError, match="PORO_PREC_"):
                    C.disp_solve(prec=pk.PREC_FDM)
        finally:
            C.close(); P.close()


# ---- 7. end to end: time steps, adaptation, the driver ------------------------------------------------------------------------------------------------------------
import os                                                                    # noqa: E402
import re                                                                    # noqa: E402
import subprocess                                                            # noqa: E402

HEIGHT, SIGMA0 = 6.0, 1e5
KW = dict(fss_tol=1e-11, pressure_tol=1e-11, max_fss=200, max_it=50000)      # absolute residual norms, as test_terzaghi.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def layered_column(dim, n, deg, mask=None):
    """a column held at the bottom and loaded at its drained top; the two top cell layers are a caprock: 100 times stiffer, 1e-3 times the reservoir's k / mu"""
    last = dim - 1
    bc = [(2 * d, d, 0.0) for d in range(last)] + [(2 * d + 1, d, 0.0) for d in range(last)] + [(2 * last, c, 0.0) for c in range(dim)]
    m = material(flow_rate=0.0)
    size = [float(v) for v in n[:-1]] + [HEIGHT]
    if mask is None:
        P = pk.Problem.box(dim, list(n), size, deg, m, bc, [(2 * last + 1, last, -SIGMA0)])
    else:
        P = pk.Problem.refined_box_mask(dim, list(n), size, deg, m, bc, mask, [(2 * last + 1, last, -SIGMA0)])
    P.set_pressure_bc([(2 * last + 1, 0.0)])
    cap = HEIGHT / 2 - 2 * HEIGHT / n[-1]
    P.set_permeability_layers([(cap, m.k_over_mu), (HEIGHT / 2, 1e-3 * m.k_over_mu)])
    P.set_moduli_layers([(cap, 1.4e10, 0.3), (HEIGHT / 2, 1.4e12, 0.25)])
    return P, m


def test_time_steps_with_moduli_and_permeability_layers():
    runs = {}
    for name, mode in (("mf", pk.OP_MATRIX_FREE), ("csr", pk.OP_CSR)):
        P, m = layered_column(3, (3, 3, 6), 2)
        lam, G = P.cell_moduli()
        assert len(np.unique(lam)) == 2 and lam[0] == pytest.approx(m.lame_lambda, rel=1e-14) and G[0] == pytest.approx(m.shear_G, rel=1e-14)
        R = pk.Runner(P, 0, mode, p_init=1e5, dt=60.0, coupled_fss=True, prec=-1, **KW)
        try:
            R.initialize()
            assert R.ctx.get_cell_moduli()[2] == 1 and R.ctx.get_cell_permeability()[1] == 1
            counts = [len(R.step()[0]) for _ in range(3)]
            runs[name] = (counts, R.ctx.get(pk.VEC_P), R.ctx.get(pk.VEC_U), R.preconditioners())
        finally:
            R.close(); P.close()
    (c1, p1, u1, pr1), (c2, p2, u2, pr2) = runs["mf"], runs["csr"]
    ep, eu = abs(p1 - p2).max() / abs(p2).max(), abs(u1 - u2).max() / abs(u2).max()
    print(f"fixed-stress iterations {c1} / {c2}; p {ep:.2e} u {eu:.2e}; preconditioners {pr1} / {pr2}")
    assert pr1[0] == pk.PREC_FDM and pr2[0] == pk.PREC_FDM
    assert c1 == c2 and max(c1) < KW["max_fss"]
    assert ep <= 1e-9 and eu <= 1e-9


def test_adaptation_carries_the_moduli():
    P, m = layered_column(2, (4, 6), 1, mask=np.zeros(24, dtype=np.int32))
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=1e5, dt=60.0, coupled_fss=True, prec=-1, **KW)
    try:
        R.initialize()
        old_lam, old_G, _ = R.ctx.get_cell_moduli()
        assert np.array_equal(old_lam, P.cell_moduli()[0]) and np.array_equal(old_G, P.cell_moduli()[1])
        R.step()
        before, after = R.adapt()
        assert after > before
        coarse, child = R.problem.cell_parents()
        lam, G, kind = R.ctx.get_cell_moduli()
        assert np.array_equal(lam, old_lam[coarse]) and np.array_equal(G, old_G[coarse]) and (child >= 0).any()      # a child takes its parent's pair, exactly
        assert np.array_equal(R.problem.cell_moduli()[0], lam) and kind == 2              # (no lattice on a mesh with hanging nodes)
        assert R.preconditioners()[0] == pk.PREC_CHEBYSHEV                               # (two-level and FDM are not available there with a field)
        rows = R.step()[0]
        print(f"cells {before} -> {after}; step after the adaptation: {len(rows)} fixed-stress iterations, error {rows[-1, 5]:.2e}")
        assert len(rows) < KW["max_fss"] and rows[-1, 5] <= KW["fss_tol"]
    finally:
        R.close(); P.close()


def test_driver_moduli_layers():
    exe = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
    data = os.path.join(ROOT, "tests", "golden", "input.data")
    layers = "0=1.4e10:0.3,5=1.4e12:0.25"                                      # the default box is [-5, 5]^3: the upper half 100 times stiffer
    r = subprocess.run([exe, data, "--matrix-free", "--fastest", "--steps", "1", "--moduli-layers", layers], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "moduli layers: 2, field kind 1; displacement preconditioner: FDM" in r.stdout
    r = subprocess.run([exe, data, "--degree", "1", "--matrix-free", "--fastest", "--steps", "2", "--refine-every", "1", "--moduli-layers", layers], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"adapted before step \d+: moduli layers: 2, field kind 2; displacement preconditioner: Chebyshev", r.stdout)
    r = subprocess.run([exe, data, "--moduli-layers", "0=1.4e10"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "TOP=YOUNG:POISSON" in r.stderr

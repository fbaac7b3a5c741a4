"""Per-cell k / mu of the pressure system (Context.set_cell_permeability): assembled matrices, the variable-coefficient stencils of matrix-free boxes, the line-solve
form of PREC_FDM (exact on layered boxes, layer means otherwise), a two-layer column with a known answer, and the refusals.

The reference is written here in numpy / scipy and shares nothing with csrc/ or oracle/: Q1 element mass and Laplace matrices under MappingQ1 with the tensorised
Gauss(2) rule, assembled cell by cell with kappa_c.

Material of these tests: biot_M = 1, k_over_mu = 1, dt = 1 on cells of edge 1, so that J = M + K_kappa with the field's values (1e-3 .. 1.5) taken literally.

Bounds: 1e-13 of the largest entry for CSR values, 1e-12 of max|y| for vectors, 1e-10 of max|dp| for the direct inverse, 1e-6 of the maximum where two iterative
solves stop at 1e-8 ||rhs|| - the project's bounds for these situations (test_parity_gpu.py, test_pressure_bc_fdm_gpu.py)."""
import itertools

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import DOMAIN_MSH, csr_to_scipy, material

pytestmark = pytest.mark.gpu
DT = 1.0


def mat1(**over):
    m = material()
    m.biot_M, m.k_over_mu, m.flow_rate = 1.0, 1.0, 0.0
    for k, v in over.items():
        setattr(m, k, v)
    return m


def rollers(dim):
    return [(2 * d, d, 0.0) for d in range(dim)]


def box(n, pbc=None, size=None, m=None):
    P = pk.Problem.box(len(n), list(n), size or [float(v) for v in n], 1, m or mat1(), rollers(len(n)))
    return P.set_pressure_bc(pbc) if pbc else P


def layer_value(k):
    return 10.0 ** (-3 + 3 * ((7 * int(k)) % 5) / 4)


def box_field(n, layered_only=False):
    """kappa_c = L[k] (1 + 0.5 sin(1.7 i + 2.3 j + 0.9 k)) in lattice cell order (x fastest); k = the index along the slowest direction (j in 2D)"""
    dim = len(n)
    out = np.empty(int(np.prod(n)))
    for c, idx in enumerate(itertools.product(*[range(m) for m in n[::-1]])):
        ijk = list(idx[::-1]) + [0] * (3 - dim)
        layer = ijk[dim - 1]
        out[c] = layer_value(layer) * (1.0 if layered_only else 1 + 0.5 * np.sin(1.7 * ijk[0] + 2.3 * ijk[1] + 0.9 * ijk[2]))
    return out


def mesh_of(P):
    d = P.desc
    nv = 1 << d.dim
    return d.dim, P.array("vertex_coords", (d.n_vertices, d.dim)), P.array("cell_vertices", (d.n_cells, nv), np.int32), P.array("cell_dofs_p", (d.n_cells, nv), np.int32)


def centre_field(P):
    """the same formula with the cell centre's coordinates in place of (i, j, k)"""
    dim, X, cv, _ = mesh_of(P)
    c = X[cv].mean(axis=1)
    c3 = np.concatenate([c, np.zeros((len(c), 3 - dim))], axis=1)
    L = np.array([layer_value(np.floor(v)) for v in c[:, dim - 1]])
    return L * (1 + 0.5 * np.sin(1.7 * c3[:, 0] + 2.3 * c3[:, 1] + 0.9 * c3[:, 2]))


def assemble(P, kappa):
    """(M, K_kappa) as scipy CSR: per-cell Q1 matrices, MappingQ1, Gauss(2)"""
    import scipy.sparse as sp
    dim, X, cv, cd = mesh_of(P)
    nv = 1 << dim
    g = 0.5 + np.array([-1.0, 1.0]) / (2 * np.sqrt(3.0))
    pts = np.array(list(itertools.product(g, repeat=dim)))[:, ::-1]
    bits = np.array([[(v >> e) & 1 for e in range(dim)] for v in range(nv)])
    N = np.empty((len(pts), nv)); dN = np.empty((len(pts), nv, dim))
    for q, xi in enumerate(pts):
        f = np.where(bits == 1, xi, 1 - xi); df = np.where(bits == 1, 1.0, -1.0)
        N[q] = f.prod(axis=1)
        for e in range(dim):
            t = f.copy(); t[:, e] = df[:, e]
            dN[q, :, e] = t.prod(axis=1)
    w = 0.5 ** dim
    rows, cols, mv, kv = [], [], [], []
    for c in range(len(cv)):
        x = X[cv[c]]
        Me = np.zeros((nv, nv)); Ke = np.zeros((nv, nv))
        for q in range(len(pts)):
            J = x.T @ dN[q]
            G = dN[q] @ np.linalg.inv(J)
            jxw = np.linalg.det(J) * w
            Me += np.outer(N[q], N[q]) * jxw
            Ke += (G @ G.T) * jxw
        rows.append(np.repeat(cd[c], nv)); cols.append(np.tile(cd[c], nv)); mv.append(Me.ravel()); kv.append(kappa[c] * Ke.ravel())
    n = P.desc.n_dofs_p
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sp.csr_matrix((np.concatenate(mv), (rows, cols)), shape=(n, n)), sp.csr_matrix((np.concatenate(kv), (rows, cols)), shape=(n, n))


def jacobian(P, kappa, a=1.0):
    M, K = assemble(P, kappa)
    return (a * M + K).tocsr()


def maxdiff(A, B):
    return abs(A - B).max() if A.nnz or B.nnz else 0.0


BOXES = [(7, 5), (1, 1), (5, 4, 6), (2, 1, 3), (1, 1, 1)]


def general_meshes():
    yield "gmsh", pk.Problem.gmsh(DOMAIN_MSH, 1, mat1(), rollers(2))
    mask = np.zeros((3, 4, 3), dtype=np.int32); mask[1, 1:3, 1] = 1; mask[0, 0, 0] = 1      # [z][y][x]
    yield "refined", pk.Problem.refined_box_mask(3, [3, 4, 3], [3.0, 4.0, 3.0], 1, mat1(), rollers(3), mask)


# ---- 1. matrices --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES, ids=str)
@pytest.mark.parametrize("mode", [pk.OP_CSR, pk.OP_MATRIX_FREE], ids=["csr", "mf"])
def test_exported_matrices_on_boxes(n, mode):
    P = box(n); G = pk.Context(P, 0, mode)
    try:
        kap = box_field(n)
        G.set_cell_permeability(kap)
        G.pres_assemble_jacobian(DT)
        M, K = assemble(P, kap)
        Kd = csr_to_scipy(*G.export_csr(pk.MAT_LAPLACE_P)); Jd = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
        eK, eJ = maxdiff(Kd, K) / abs(K).max(), maxdiff(Jd, M + K) / abs(M + K).max()
        print(f"{n}: K {eK:.2e} J {eJ:.2e}")
        assert eK <= 1e-13 and eJ <= 1e-13
        got, kind = G.get_cell_permeability()
        layers = kap.reshape(n[-1], -1)
        assert kind == (1 if np.all(layers == layers[:, :1]) else 2) and np.array_equal(got, kap)       # (a box of one cell per layer is layered)
    finally:
        G.close(); P.close()


def test_exported_matrices_on_general_meshes():
    for name, P in general_meshes():
        G = pk.Context(P, 0, pk.OP_CSR)
        try:
            kap = centre_field(P)
            assert kap.min() > 0 and kap.max() > 1.5 * kap.min()
            G.set_cell_permeability(kap)
            G.pres_assemble_jacobian(DT)
            M, K = assemble(P, kap)
            Kd = csr_to_scipy(*G.export_csr(pk.MAT_LAPLACE_P)); Jd = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
            eK, eJ = maxdiff(Kd, K) / abs(K).max(), maxdiff(Jd, M + K) / abs(M + K).max()
            print(f"{name}: cells {P.desc.n_cells} K {eK:.2e} J {eJ:.2e}")
            assert eK <= 1e-13 and eJ <= 1e-13
            assert G.get_cell_permeability()[1] == 2
        finally:
            G.close(); P.close()


# ---- 2. operator and residual on matrix-free boxes -----------------------------------------------------------------------------------------------------------
def set_state(G, rng):
    st = {v: rng.standard_normal(G.n_p) for v in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0)}
    for v, a in st.items():
        G.set(v, a)
    return st


@pytest.mark.parametrize("n", BOXES, ids=str)
def test_operator_and_residual_on_matrix_free_boxes(n):
    m = mat1(); P = box(n, m=m)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE); H = pk.Context(P, 0, pk.OP_CSR)
    try:
        kap = box_field(n); rng = np.random.default_rng(7 + len(n) + n[0])
        M, K = assemble(P, kap)
        x = rng.standard_normal(G.n_p)
        res, ys = [], []
        for ctx in (G, H):
            ctx.set_cell_permeability(kap)
            ctx.pres_assemble_jacobian(DT)
            st = set_state(ctx, np.random.default_rng(99))
            ys.append(ctx.pres_apply_jacobian(x))
            ctx.pres_assemble_residual(DT)
            res.append(ctx.get(pk.VEC_RESIDUAL_P))
        t = m.biot_alpha / DT * (st[pk.VEC_EPSV] - st[pk.VEC_EPSV0]) + 1.0 / m.biot_M / DT * (st[pk.VEC_P] - st[pk.VEC_P_OLD])
        y0 = (M + K) @ x; r0 = -(M @ t + K @ st[pk.VEC_P])
        ey, er = abs(ys[0] - y0).max() / abs(y0).max(), abs(res[0] - r0).max() / abs(r0).max()
        cy, cr = abs(ys[0] - ys[1]).max() / abs(y0).max(), abs(res[0] - res[1]).max() / abs(r0).max()
        print(f"{n}: operator {ey:.2e} residual {er:.2e}; matrix-free against CSR {cy:.2e} {cr:.2e}")
        assert ey <= 1e-12 and er <= 1e-12 and cy <= 1e-12 and cr <= 1e-12
        assert np.array_equal(G.pres_apply_jacobian(x), ys[0])                     # bitwise from call to call
        G.pres_assemble_residual(DT)
        assert np.array_equal(G.get(pk.VEC_RESIDUAL_P), res[0])
    finally:
        G.close(); H.close(); P.close()


# ---- 3. constant field ---------------------------------------------------------------------------------------------------------------------------------------
def test_constant_field_reproduces_the_scalar_path():
    n = (5, 4, 6); P = box(n)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE); F = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        rng = np.random.default_rng(3)
        for ctx in (G, F):
            set_state(ctx, np.random.default_rng(5))
            ctx.pres_assemble_jacobian(DT); ctx.pres_assemble_residual(DT)
        J0 = csr_to_scipy(*F.export_csr(pk.MAT_JACOBIAN_P)); R0 = F.get(pk.VEC_RESIDUAL_P)
        G.set_cell_permeability(np.full(P.desc.n_cells, mat1().k_over_mu))
        assert G.get_cell_permeability()[1] == 1
        G.pres_assemble_jacobian(DT)
        J1 = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
        assert maxdiff(J1, J0) <= 1e-13 * abs(J0).max()
        b = rng.standard_normal(G.n_p)
        G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
        rc, info = G.pres_solve(rel_tol=1e-12, prec=pk.PREC_FDM)
        assert rc == 0 and info.iterations == 0 and info.converged == 1
        import scipy.sparse.linalg as spla
        x0 = spla.spsolve(J0.tocsc(), b)
        assert abs(G.get(pk.VEC_DP) - x0).max() <= 1e-10 * abs(x0).max()
        G.set_cell_permeability(None)
        assert G.get_cell_permeability() == (None, 0)
        G.pres_assemble_jacobian(DT); G.pres_assemble_residual(DT)
        J2 = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
        assert np.array_equal(J2.data, J0.data) and np.array_equal(G.get(pk.VEC_RESIDUAL_P), R0)      # bitwise those of a fresh context
    finally:
        G.close(); F.close(); P.close()


# ---- 4. layered direct solve ---------------------------------------------------------------------------------------------------------------------------------
def solve(G, b, prec, rel_tol):
    G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
    rc, info = G.pres_solve(rel_tol=rel_tol, prec=prec)
    return rc, info, G.get(pk.VEC_DP)


@pytest.mark.parametrize("n", [(5, 4, 6), (9, 8, 7), (2, 1, 3), (1, 1, 1), (7, 5), (1, 1)], ids=str)
def test_layered_direct_solve(n):
    import scipy.sparse.linalg as spla
    P = box(n); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n, layered_only=True)
        G.set_cell_permeability(kap)
        assert G.get_cell_permeability()[1] == 1 and G.supports_preconditioner(1, pk.PREC_FDM)
        G.pres_assemble_jacobian(DT)
        b = np.random.default_rng(11 + G.n_p).standard_normal(G.n_p)
        rc, info, x = solve(G, b, pk.PREC_FDM, 1e-12)
        x0 = spla.spsolve(jacobian(P, kap).tocsc(), b)
        err = abs(x - x0).max() / abs(x0).max()
        print(f"{n}: iterations {info.iterations} residual {info.final_residual:.2e} / {info.initial_residual:.2e} error {err:.2e}")
        assert rc == 0 and info.iterations == 0 and info.converged == 1
        assert err <= 1e-10
    finally:
        G.close(); P.close()


def test_layered_field_preconditions_cg_on_csr_and_graded_contexts():
    import scipy.sparse.linalg as spla
    n = (5, 4, 6)
    cases = [("csr box", box(n), pk.OP_CSR),
             ("graded", pk.Problem.graded_box(3, list(n), [float(v) for v in n], 1, mat1(), rollers(3), [0.6, 0.0, 0.9]), pk.OP_MATRIX_FREE)]
    for name, P, mode in cases:
        G = pk.Context(P, 0, mode)
        try:
            kap = box_field(n, layered_only=True)
            G.set_cell_permeability(kap)
            assert G.get_cell_permeability()[1] == 1
            G.pres_assemble_jacobian(DT)
            b = np.random.default_rng(21).standard_normal(G.n_p)
            rc, info, x = solve(G, b, pk.PREC_FDM, 1e-12)
            x0 = spla.spsolve(jacobian(P, kap).tocsc(), b)
            err = abs(x - x0).max() / abs(x0).max()
            print(f"{name}: iterations {info.iterations} error {err:.2e}")
            assert rc == 0 and info.converged == 1 and 1 <= info.iterations <= 2
            assert err <= 1e-10
        finally:
            G.close(); P.close()


def test_layered_direct_solve_with_prescribed_faces():
    import scipy.sparse.linalg as spla
    n = (5, 4, 6)
    P = box(n, pbc=[(5, 0.0), (0, 0.0)]); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n, layered_only=True)
        nd = P.desc.n_dirichlet_p; dofs = P.array("dirichlet_dof_p", (nd,), np.int32)
        free = np.setdiff1d(np.arange(G.n_p), dofs)
        b = np.random.default_rng(31).standard_normal(G.n_p)
        for scale in (1.0, 1e12):
            G.set_cell_permeability(scale * kap)
            assert G.supports_preconditioner(1, pk.PREC_FDM)
            G.pres_assemble_jacobian(DT)
            rc, info, x = solve(G, b, pk.PREC_FDM, 1e-12)
            assert np.all(np.isfinite(x)) and np.all(x[dofs] == 0.0)                # the removed modes return exactly 0, nothing of the size kappa h 1e300 is formed
            J = jacobian(P, scale * kap).tocsc()
            x0 = spla.spsolve(J[free][:, free], b[free])
            err = abs(x[free] - x0).max() / abs(x0).max()
            print(f"scale {scale:g}: iterations {info.iterations} converged {info.converged} error {err:.2e}")
            if scale == 1.0:
                assert rc == 0 and info.iterations == 0 and info.converged == 1 and err <= 1e-10
    finally:
        G.close(); P.close()


# ---- 5. general field with the layer-mean preconditioner -----------------------------------------------------------------------------------------------------
def numpy_pcg(J, prec, b, rel_tol):
    x = np.zeros_like(b); g = b.copy(); z = prec(g); d = z.copy(); gz = g @ z
    for it in range(1, 1000):
        h = J @ d; al = gz / (d @ h)
        x += al * d; g -= al * h
        if np.linalg.norm(g) <= rel_tol * np.linalg.norm(b):
            return it, x
        z = prec(g); gz_new = g @ z; d = z + (gz_new / gz) * d; gz = gz_new
    return 1000, x


@pytest.mark.parametrize("n", [(5, 4, 6), (9, 8, 7)], ids=str)
def test_general_field_with_the_layer_mean_preconditioner(n):
    import scipy.sparse.linalg as spla
    P = box(n); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n)
        G.set_cell_permeability(kap)
        assert G.get_cell_permeability()[1] == 2 and G.supports_preconditioner(1, pk.PREC_FDM)
        G.pres_assemble_jacobian(DT)
        b = np.random.default_rng(41).standard_normal(G.n_p)
        J = jacobian(P, kap)
        means = kap.reshape(n[2], -1).mean(axis=1)
        Jm = spla.factorized(jacobian(P, np.repeat(means, n[0] * n[1])).tocsc())
        it_np, _ = numpy_pcg(J, Jm, b, 1e-8)
        rc, info, x = solve(G, b, pk.PREC_FDM, 1e-8)
        rcj, infoj, _ = solve(G, b, pk.PREC_JACOBI, 1e-8)
        x0 = spla.spsolve(J.tocsc(), b)
        err = abs(x - x0).max() / abs(x0).max()
        print(f"{n}: FDM (layer means) {info.iterations} iterations, numpy {it_np}, Jacobi {infoj.iterations}; error {err:.2e}")
        assert rc == 0 and info.converged == 1 and info.iterations > 0
        assert err <= 1e-6
        assert info.iterations <= it_np + 2
        assert rcj == 0 and info.iterations < infoj.iterations
    finally:
        G.close(); P.close()


# ---- 6. known answer: two-layer column -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec", [(pk.OP_MATRIX_FREE, pk.PREC_FDM), (pk.OP_CSR, pk.PREC_JACOBI)], ids=["mf-fdm", "csr-jacobi"])
def test_two_layer_column(mode, prec):
    n, h = (2, 2, 6), 0.5
    P = box(n, pbc=[(4, 0.0), (5, 1.0)], size=[1.0, 1.0, 3.0]); G = pk.Context(P, 0, mode)
    try:
        layers = np.array([1.0, 1.0, 1.0, 100.0, 100.0, 100.0])
        G.set_cell_permeability(np.repeat(layers, 4))
        dt = 1e21                                                                     # a h^2 / kappa_min = 2.5e-22
        for v in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0):
            G.fill(v, 0.0)
        G.pres_apply_boundary_values()
        G.copy(pk.VEC_P_OLD, pk.VEC_P)
        G.pres_assemble_residual(dt); G.pres_assemble_jacobian(dt)
        G.fill(pk.VEC_DP, 0.0)
        rc, info = G.pres_solve(rel_tol=1e-13, prec=prec, max_iter=2000)
        G.axpy(pk.VEC_P, 1.0, pk.VEC_DP)
        p = G.get(pk.VEC_P).reshape(7, 9)
        R = np.concatenate([[0.0], np.cumsum(h / layers)])
        err = abs(p - (R / R[-1])[:, None]).max()
        print(f"iterations {info.iterations} converged {info.converged} error {err:.2e}")
        assert rc == 0 and info.converged == 1
        assert err <= 1e-10
    finally:
        G.close(); P.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    P = box((3, 2, 2)); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        good = np.ones(P.desc.n_cells)
        for bad, word in ((np.ones(P.desc.n_cells + 1), "n_cells"), (np.r_[good[:-1], 0.0], "finite"), (np.r_[-1.0, good[1:]], "finite"), (np.r_[good[:-1], np.nan], "finite")):
            with pytest.raises(RuntimeError, match=word):
                G.set_cell_permeability(bad)
            assert G.get_cell_permeability() == (None, 0)
    finally:
        G.close(); P.close()
    # partitioned contexts: the test hook of the partitioned code path, and a 2-slab descriptor
    monkeypatch.setenv("PORO_FORCE_PARTITIONED_PATH", "1")
    P = box((3, 2, 2)); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    monkeypatch.delenv("PORO_FORCE_PARTITIONED_PATH")
    try:
        with pytest.raises(RuntimeError, match="one rank"):
            G.set_cell_permeability(np.ones(P.desc.n_cells))
    finally:
        G.close(); P.close()
    P = pk.Problem.box(3, [3, 2, 4], [3.0, 2.0, 4.0], 1, mat1(), rollers(3), (), 0, 2); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        with pytest.raises(RuntimeError, match="one rank"):
            G.set_cell_permeability(np.ones(P.desc.n_cells))
    finally:
        G.close(); P.close()
    # the two-level form of the pressure system on a refined box, and FDM on the Gmsh mesh
    for name, P in general_meshes():
        G = pk.Context(P, 0, pk.OP_CSR)
        try:
            had = G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)
            G.set_cell_permeability(centre_field(P))
            G.pres_assemble_jacobian(DT)
            assert not G.supports_preconditioner(1, pk.PREC_TWO_LEVEL) and not G.supports_preconditioner(1, pk.PREC_FDM)
            assert G.supports_preconditioner(1, pk.PREC_JACOBI)
            if name == "refined":
                assert had
                G.set(pk.VEC_RESIDUAL_P, np.ones(G.n_p))
                with pytest.raises(RuntimeError, match="per-cell permeability"):
                    G.pres_solve(prec=pk.PREC_TWO_LEVEL)
        finally:
            G.close(); P.close()


# ---- 7. time steps: a caprock over a reservoir ---------------------------------------------------------------------------------------------------------------
HEIGHT, SIGMA0 = 6.0, 1e5
KW = dict(fss_tol=1e-11, pressure_tol=1e-11, max_fss=200, max_it=50000)      # absolute residual norms, as test_terzaghi.py


def layered_column(dim, n, deg, mask=None):
    """a column held at the bottom and loaded at its drained top; the two top cell layers are a caprock of 1e-3 times the reservoir's k / mu"""
    last = dim - 1
    bc = [(2 * d, d, 0.0) for d in range(last)] + [(2 * d + 1, d, 0.0) for d in range(last)] + [(2 * last, last, 0.0)]
    m = material(flow_rate=0.0)
    size = [float(v) for v in n[:-1]] + [HEIGHT]
    if mask is None:
        P = pk.Problem.box(dim, list(n), size, deg, m, bc, [(2 * last + 1, last, -SIGMA0)])
    else:
        P = pk.Problem.refined_box_mask(dim, list(n), size, deg, m, bc, mask, [(2 * last + 1, last, -SIGMA0)])
    P.set_pressure_bc([(2 * last + 1, 0.0)])
    P.set_permeability_layers([(HEIGHT / 2 - 2 * HEIGHT / n[-1], m.k_over_mu), (HEIGHT / 2, 1e-3 * m.k_over_mu)])
    return P, m


def test_time_steps_on_a_layered_column():
    runs = {}
    for name, mode, kw in (("mf", pk.OP_MATRIX_FREE, dict(prec=-1)), ("csr", pk.OP_CSR, dict(jacobi_p=True))):
        P, m = layered_column(3, (4, 4, 6), 2)
        field = P.cell_permeability()
        assert field is not None and np.array_equal(field.reshape(6, 16), np.repeat([[1.0], [1.0], [1.0], [1.0], [1e-3], [1e-3]], 16, axis=1) * m.k_over_mu)
        R = pk.Runner(P, 0, mode, p_init=1e5, dt=60.0, coupled_fss=True, **KW, **kw)
        try:
            R.initialize()
            assert R.ctx.get_cell_permeability()[1] == 1
            counts = [len(R.step()[0]) for _ in range(3)]
            runs[name] = (counts, R.ctx.get(pk.VEC_P), R.ctx.get(pk.VEC_U), R.preconditioners())
        finally:
            R.close(); P.close()
    (c1, p1, u1, pr1), (c2, p2, u2, pr2) = runs["mf"], runs["csr"]
    ep, eu = abs(p1 - p2).max() / abs(p2).max(), abs(u1 - u2).max() / abs(u2).max()
    print(f"fixed-stress iterations {c1} / {c2}; p {ep:.2e} u {eu:.2e}; preconditioners {pr1} / {pr2}")
    assert pr1[1] == pk.PREC_FDM and pr2[1] == pk.PREC_JACOBI
    assert c1 == c2 and max(c1) < KW["max_fss"]
    assert ep <= 1e-6 and eu <= 1e-6


# ---- 8. adaptation -------------------------------------------------------------------------------------------------------------------------------------------
def test_adaptation_carries_the_field():
    P, m = layered_column(2, (4, 6), 1, mask=np.zeros(24, dtype=np.int32))
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=1e5, dt=60.0, coupled_fss=True, prec=-1, **KW)
    try:
        R.initialize()
        old = R.ctx.get_cell_permeability()[0]
        assert np.array_equal(old, P.cell_permeability())
        R.step()
        before, after = R.adapt()
        assert after > before
        coarse, child = R.problem.cell_parents()
        new, kind = R.ctx.get_cell_permeability()
        assert np.array_equal(new, old[coarse]) and (child >= 0).any()               # the first mesh is the coarse box itself: a child takes its parent's value, exactly
        assert np.array_equal(R.problem.cell_permeability(), new) and kind == 2       # (no lattice on a mesh with hanging nodes)
        assert R.preconditioners()[1] == pk.PREC_JACOBI
        rows = R.step()[0]
        print(f"cells {before} -> {after}; step after the adaptation: {len(rows)} fixed-stress iterations, error {rows[-1, 5]:.2e}")
        assert len(rows) < KW["max_fss"] and rows[-1, 5] <= KW["fss_tol"]
    finally:
        R.close(); P.close()

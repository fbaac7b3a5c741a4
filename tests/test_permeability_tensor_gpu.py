"""Per-cell diagonal permeability tensor diag(kx, ky[, kz]) / mu of the pressure system (Context.set_cell_permeability_tensor): assembled matrices, the tensor stencils
of matrix-free boxes, the tensor line solve of PREC_FDM (exact on layered boxes, per-component layer means otherwise), known answers, refusals and state, time steps
and adaptation.

The reference is written here in numpy / scipy and shares nothing with csrc/ or oracle/: Q1 element matrices under MappingQ1 with the tensorised Gauss(2) rule,
Ke = sum_q (G diag(kappa_c) G^T) JxW, assembled cell by cell.

Material of these tests: biot_M = 1, k_over_mu = 1, dt = 1 on cells of edge 1, so that J = M + K_kappa with the field's values taken literally.  The field is
kappa_d(c) = L_d[k] (1 + 0.5 sin(1.7 i + 2.3 j + 0.9 k + d)) with three different layer tables L_d over three decades; kz / kx is 1e-3 in layer 2.

Bounds: 1e-13 of the largest entry for CSR values, 1e-12 of max|y| for vectors, 1e-10 of max|dp| for the direct inverse, 1e-6 of the maximum where two iterative
solves stop at 1e-8 ||rhs|| - the project's bounds for these situations (test_permeability_gpu.py)."""
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


# the layer tables of the horizontal components and of the component along the slowest direction (the last one of a problem): layer 2 has L_H0 = 1, L_V = 1e-3
def L_H0(k): return 10.0 ** (-3 + 3 * ((7 * int(k)) % 5) / 4)
def L_H1(k): return 10.0 ** (-3 + 3 * ((3 * int(k) + 2) % 5) / 4)
def L_V(k): return 10.0 ** (-3 + 3 * ((2 * int(k) + 1) % 5) / 4)


def tables(dim):
    return [L_H0, L_V] if dim == 2 else [L_H0, L_H1, L_V]


def box_field(n, layered_only=False):
    """(n_cells, dim) in lattice cell order (x fastest); k = the index along the slowest direction (j in 2D)"""
    dim = len(n)
    out = np.empty((int(np.prod(n)), dim))
    for c, idx in enumerate(itertools.product(*[range(m) for m in n[::-1]])):
        ijk = list(idx[::-1]) + [0] * (3 - dim)
        for d, L in enumerate(tables(dim)):
            out[c, d] = L(ijk[dim - 1]) * (1.0 if layered_only else 1 + 0.5 * np.sin(1.7 * ijk[0] + 2.3 * ijk[1] + 0.9 * ijk[2] + d))
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
    out = np.empty((len(c), dim))
    for d, L in enumerate(tables(dim)):
        out[:, d] = np.array([L(np.floor(v)) for v in c[:, dim - 1]]) * (1 + 0.5 * np.sin(1.7 * c3[:, 0] + 2.3 * c3[:, 1] + 0.9 * c3[:, 2] + d))
    return out


def assemble(P, kappa):
    """(M, K_kappa) as scipy CSR: per-cell Q1 matrices, MappingQ1, Gauss(2); kappa (n_cells, dim) weights the gradient product per global axis"""
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
            Ke += (G @ np.diag(kappa[c]) @ G.T) * jxw
        rows.append(np.repeat(cd[c], nv)); cols.append(np.tile(cd[c], nv)); mv.append(Me.ravel()); kv.append(Ke.ravel())
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
        G.set_cell_permeability_tensor(kap)
        G.pres_assemble_jacobian(DT)
        M, K = assemble(P, kap)
        Kd = csr_to_scipy(*G.export_csr(pk.MAT_LAPLACE_P)); Jd = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
        eK, eJ = maxdiff(Kd, K) / abs(K).max(), maxdiff(Jd, M + K) / abs(M + K).max()
        print(f"{n}: K {eK:.2e} J {eJ:.2e}")
        assert eK <= 1e-13 and eJ <= 1e-13
        got, kind = G.get_cell_permeability_tensor()
        layers = kap.reshape(n[-1], -1, len(n))
        assert kind == (1 if np.all(layers == layers[:, :1]) else 2) and np.array_equal(got, kap)       # (a box of one cell per layer is layered)
        assert kind == (1 if int(np.prod(n[:-1])) == 1 else 2)
    finally:
        G.close(); P.close()


def test_exported_matrices_on_general_meshes():
    for name, P in general_meshes():
        G = pk.Context(P, 0, pk.OP_CSR)
        try:
            kap = centre_field(P)
            assert kap.min() > 0 and kap.max() > 1.5 * kap.min()
            G.set_cell_permeability_tensor(kap)
            G.pres_assemble_jacobian(DT)
            M, K = assemble(P, kap)
            Kd = csr_to_scipy(*G.export_csr(pk.MAT_LAPLACE_P)); Jd = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
            eK, eJ = maxdiff(Kd, K) / abs(K).max(), maxdiff(Jd, M + K) / abs(M + K).max()
            print(f"{name}: cells {P.desc.n_cells} K {eK:.2e} J {eJ:.2e}")
            assert eK <= 1e-13 and eJ <= 1e-13
            got, kind = G.get_cell_permeability_tensor()
            assert kind == 2 and np.array_equal(got, kap)
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
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n); rng = np.random.default_rng(7 + len(n) + n[0])
        M, K = assemble(P, kap)
        x = rng.standard_normal(G.n_p)
        G.set_cell_permeability_tensor(kap)
        G.pres_assemble_jacobian(DT)
        st = set_state(G, np.random.default_rng(99))
        y = G.pres_apply_jacobian(x)
        G.pres_assemble_residual(DT)
        res = G.get(pk.VEC_RESIDUAL_P)
        t = m.biot_alpha / DT * (st[pk.VEC_EPSV] - st[pk.VEC_EPSV0]) + 1.0 / m.biot_M / DT * (st[pk.VEC_P] - st[pk.VEC_P_OLD])
        y0 = (M + K) @ x; r0 = -(M @ t + K @ st[pk.VEC_P])
        ey, er = abs(y - y0).max() / abs(y0).max(), abs(res - r0).max() / abs(r0).max()
        print(f"{n}: operator {ey:.2e} residual {er:.2e}")
        assert ey <= 1e-12 and er <= 1e-12
        assert np.array_equal(G.pres_apply_jacobian(x), y)                         # bitwise from call to call
        G.pres_assemble_residual(DT)
        assert np.array_equal(G.get(pk.VEC_RESIDUAL_P), res)
    finally:
        G.close(); P.close()


# ---- 3. axis permutation -------------------------------------------------------------------------------------------------------------------------------------
def test_axis_permutation():
    """the box (4, 3, 5) with a general tensor field, and the same problem with the axes renamed (x', y', z') = (z, x, y) on the box (5, 4, 3): components, cells and
    nodes permuted alike; a kernel that weights the wrong direction gives another answer"""
    n = (4, 3, 5); n2 = (5, 4, 3)
    kap = box_field(n)
    kap2 = kap.reshape(n[2], n[1], n[0], 3).transpose(1, 2, 0, 3)[..., [2, 0, 1]].reshape(-1, 3)      # cell [k][j][i] -> [k' = j][j' = i][i' = k]; (kx', ky', kz') = (kz, kx, ky)
    nn = [v + 1 for v in n]
    x = np.random.default_rng(5).standard_normal(int(np.prod(nn)))
    x2 = x.reshape(nn[2], nn[1], nn[0]).transpose(1, 2, 0).ravel()
    out = []
    for shape, field, vec in ((n, kap, x), (n2, kap2, x2)):
        P = box(shape); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        try:
            G.set_cell_permeability_tensor(field)
            G.pres_assemble_jacobian(DT)
            set_state(G, np.random.default_rng(1))
            G.set(pk.VEC_P, vec)
            y = G.pres_apply_jacobian(vec)
            G.pres_assemble_residual(DT)
            out.append((y, G.get(pk.VEC_RESIDUAL_P)))
        finally:
            G.close(); P.close()
    y, y2 = out[0][0], out[1][0]
    e = abs(y.reshape(nn[2], nn[1], nn[0]).transpose(1, 2, 0).ravel() - y2).max() / abs(y).max()
    kap_wrong = kap[:, [1, 2, 0]]
    P = box(n)
    try:
        far = abs(jacobian(P, kap_wrong) @ x - y).max() / abs(y).max()
    finally:
        P.close()
    print(f"operator against its permuted twin {e:.2e}; against a field with rotated components {far:.2e}")
    assert e <= 1e-12 and far > 1e-3


# ---- 4. equal components reproduce the scalar field ----------------------------------------------------------------------------------------------------------
def solve(G, b, prec, rel_tol, max_iter=None):
    G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
    rc, info = G.pres_solve(rel_tol=rel_tol, prec=prec) if max_iter is None else G.pres_solve(rel_tol=rel_tol, prec=prec, max_iter=max_iter)
    return rc, info, G.get(pk.VEC_DP)


def test_equal_components_reproduce_the_scalar_field():
    n = (5, 4, 6); P = box(n)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE); F = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        for ctx in (G, F):
            set_state(ctx, np.random.default_rng(5))
            ctx.pres_assemble_jacobian(DT); ctx.pres_assemble_residual(DT)
        J0 = csr_to_scipy(*F.export_csr(pk.MAT_JACOBIAN_P)); R0 = F.get(pk.VEC_RESIDUAL_P)
        rng = np.random.default_rng(3)
        x = rng.standard_normal(G.n_p); b = rng.standard_normal(G.n_p)
        got = {}
        for layered in (True, False):
            kap = box_field(n, layered_only=layered)[:, 0]
            for name in ("scalar", "tensor"):
                if name == "scalar":
                    G.set_cell_permeability(kap)
                else:
                    G.set_cell_permeability_tensor(np.repeat(kap[:, None], 3, axis=1))
                G.pres_assemble_jacobian(DT)
                J = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P)); y = G.pres_apply_jacobian(x)
                dp = solve(G, b, pk.PREC_FDM, 1e-12) if layered else None
                got[name] = (J, y, dp)
            (Js, ys, ds), (Jt, yt, dt_) = got["scalar"], got["tensor"]
            eJ, ey = maxdiff(Js, Jt) / abs(Js).max(), abs(ys - yt).max() / abs(ys).max()
            print(f"layered {layered}: CSR {eJ:.2e} operator {ey:.2e}")
            assert eJ <= 1e-13 and ey <= 1e-12
            if layered:
                assert ds[0] == 0 and dt_[0] == 0 and ds[1].iterations == 0 and dt_[1].iterations == 0 and dt_[1].converged == 1
                ed = abs(ds[2] - dt_[2]).max() / abs(ds[2]).max()
                print(f"direct solve {ed:.2e}")
                assert ed <= 1e-10
        assert G.get_cell_permeability_tensor()[1] == 2
        G.set_cell_permeability_tensor(None)
        assert G.get_cell_permeability_tensor() == (None, 0) and G.get_cell_permeability() == (None, 0)
        G.pres_assemble_jacobian(DT); G.pres_assemble_residual(DT)
        J2 = csr_to_scipy(*G.export_csr(pk.MAT_JACOBIAN_P))
        assert np.array_equal(J2.data, J0.data) and np.array_equal(G.get(pk.VEC_RESIDUAL_P), R0)      # bitwise those of a fresh context
        assert np.array_equal(G.pres_apply_jacobian(x), F.pres_apply_jacobian(x))
    finally:
        G.close(); F.close(); P.close()


# ---- 5. layered direct solve ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(5, 4, 6), (9, 8, 7), (2, 1, 3), (1, 1, 1), (7, 5), (1, 1)], ids=str)
def test_layered_direct_solve(n):
    import scipy.sparse.linalg as spla
    P = box(n); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n, layered_only=True)
        G.set_cell_permeability_tensor(kap)
        assert G.get_cell_permeability_tensor()[1] == 1 and G.supports_preconditioner(1, pk.PREC_FDM)
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


@pytest.mark.parametrize("n", [(5, 4, 6), (9, 8, 7), (2, 1, 3), (1, 1, 1), (7, 5), (1, 1)], ids=str)
def test_layered_direct_solve_with_prescribed_faces(n):
    """the top face and the low-x face prescribed; then the whole field scaled by 1e12 (the removed modes: no inf, no nan)"""
    import scipy.sparse.linalg as spla
    dim = len(n)
    P = box(n, pbc=[(2 * dim - 1, 0.0), (0, 0.0)]); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n, layered_only=True)
        nd = P.desc.n_dirichlet_p; dofs = P.array("dirichlet_dof_p", (nd,), np.int32)
        free = np.setdiff1d(np.arange(G.n_p), dofs)
        b = np.random.default_rng(31).standard_normal(G.n_p)
        for scale in (1.0, 1e12):
            G.set_cell_permeability_tensor(scale * kap)
            assert G.supports_preconditioner(1, pk.PREC_FDM)
            G.pres_assemble_jacobian(DT)
            rc, info, x = solve(G, b, pk.PREC_FDM, 1e-12)
            assert np.all(np.isfinite(x)) and np.all(x[dofs] == 0.0)                # the removed modes return exactly 0, nothing of the size kappa h 1e300 is formed
            J = jacobian(P, scale * kap).tocsc()
            x0 = spla.spsolve(J[free][:, free], b[free])
            err = abs(x[free] - x0).max() / abs(x0).max()
            print(f"{n} scale {scale:g}: iterations {info.iterations} converged {info.converged} error {err:.2e}")
            if scale == 1.0:
                assert rc == 0 and info.iterations == 0 and info.converged == 1 and err <= 1e-10
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
            G.set_cell_permeability_tensor(kap)
            assert G.get_cell_permeability_tensor()[1] == 1
            G.pres_assemble_jacobian(DT)
            b = np.random.default_rng(21).standard_normal(G.n_p)
            rc, info, x = solve(G, b, pk.PREC_FDM, 1e-12)
            x0 = spla.spsolve(jacobian(P, kap).tocsc(), b)
            err = abs(x - x0).max() / abs(x0).max()
            print(f"{name}: iterations {info.iterations} error {err:.2e}")
            assert rc == 0 and info.converged == 1 and info.iterations == 1
            assert err <= 1e-10
        finally:
            G.close(); P.close()


# ---- 6. general field with the per-component layer-mean preconditioner ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(5, 4, 6), (9, 8, 7)], ids=str)
def test_general_field_with_the_layer_mean_preconditioner(n):
    import scipy.sparse.linalg as spla
    P = box(n); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        kap = box_field(n)
        G.set_cell_permeability_tensor(kap)
        assert G.get_cell_permeability_tensor()[1] == 2 and G.supports_preconditioner(1, pk.PREC_FDM)
        G.pres_assemble_jacobian(DT)
        b = np.random.default_rng(41).standard_normal(G.n_p)
        rc, info, x = solve(G, b, pk.PREC_FDM, 1e-8)
        rcj, infoj, _ = solve(G, b, pk.PREC_JACOBI, 1e-8, max_iter=5000)
        x0 = spla.spsolve(jacobian(P, kap).tocsc(), b)
        err = abs(x - x0).max() / abs(x0).max()
        print(f"{n}: FDM (layer means) {info.iterations} iterations, Jacobi {infoj.iterations}; error {err:.2e}")
        assert rc == 0 and info.converged == 1 and info.iterations > 0                # never a direct solve
        assert err <= 1e-6
        assert rcj == 0 and infoj.converged == 1 and info.iterations < infoj.iterations
    finally:
        G.close(); P.close()


# ---- 7. known answers ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec", [(pk.OP_MATRIX_FREE, pk.PREC_FDM), (pk.OP_CSR, pk.PREC_JACOBI)], ids=["mf-fdm", "csr-jacobi"])
@pytest.mark.parametrize("faces", ["z", "x"])
def test_known_answers(mode, prec, faces):
    """a column of 2 x 2 x 6 cells, steady state (dt = 1e21).  z: pressures prescribed on the two z faces - the series-resistance profile of kz ALONE.  x: on the two x
    faces - p is linear in x whatever kx(z), ky, kz are"""
    n, h = (2, 2, 6), 0.5
    pbc = [(4, 0.0), (5, 1.0)] if faces == "z" else [(0, 0.0), (1, 1.0)]
    P = box(n, pbc=pbc, size=[1.0, 1.0, 3.0]); G = pk.Context(P, 0, mode)
    try:
        kz = np.array([1.0, 1.0, 1.0, 100.0, 100.0, 100.0])
        kx = np.array([3.0, 0.5, 20.0, 0.1, 7.0, 2.0]); ky = np.array([0.2, 40.0, 1.0, 5.0, 0.3, 9.0])
        G.set_cell_permeability_tensor(np.repeat(np.stack([kx, ky, kz], axis=1), 4, axis=0))
        assert G.get_cell_permeability_tensor()[1] == 1
        dt = 1e21                                                                     # a h^2 / kappa_min = 2.5e-21
        for v in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0):
            G.fill(v, 0.0)
        G.pres_apply_boundary_values()
        G.copy(pk.VEC_P_OLD, pk.VEC_P)
        G.pres_assemble_residual(dt); G.pres_assemble_jacobian(dt)
        G.fill(pk.VEC_DP, 0.0)
        rc, info = G.pres_solve(rel_tol=1e-13, prec=prec, max_iter=2000)
        G.axpy(pk.VEC_P, 1.0, pk.VEC_DP)
        p = G.get(pk.VEC_P).reshape(7, 3, 3)
        if faces == "z":
            R = np.concatenate([[0.0], np.cumsum(h / kz)])
            err = abs(p - (R / R[-1])[:, None, None]).max()
        else:
            err = abs(p - np.array([0.0, 0.5, 1.0])[None, None, :]).max()
        print(f"{faces} faces: iterations {info.iterations} converged {info.converged} error {err:.2e}")
        assert rc == 0 and info.converged == 1
        assert err <= 1e-10
    finally:
        G.close(); P.close()


# ---- 8. refusals and state -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(monkeypatch):
    n = (3, 2, 2); P = box(n); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        nc = P.desc.n_cells
        good = box_field(n); x = np.random.default_rng(2).standard_normal(G.n_p)

        def bad_at(cell, comp, v):
            f = good.copy(); f[cell, comp] = v
            return f
        cases = ((np.ones((nc + 1, 3)), "n_cells"), (bad_at(nc - 1, 2, 0.0), f"component 2 of cell {nc - 1} is not finite"), (bad_at(0, 0, -1.0), "component 0 of cell 0 is not finite"),
                 (bad_at(5, 1, np.nan), "component 1 of cell 5 is not finite"), (bad_at(7, 2, np.inf), "component 2 of cell 7 is not finite"))
        for bad, word in cases:                                                       # no field yet: none afterwards
            with pytest.raises(RuntimeError, match=word):
                G.set_cell_permeability_tensor(bad)
            assert G.get_cell_permeability_tensor() == (None, 0) and G.get_cell_permeability() == (None, 0)
        G.set_cell_permeability_tensor(good)
        G.pres_assemble_jacobian(DT)
        y = G.pres_apply_jacobian(x)
        for bad, word in cases:                                                       # a refused call leaves the previous field and its results intact
            with pytest.raises(RuntimeError, match=word):
                G.set_cell_permeability_tensor(bad)
            got, kind = G.get_cell_permeability_tensor()
            assert kind == 2 and np.array_equal(got, good) and np.array_equal(G.pres_apply_jacobian(x), y)
        with pytest.raises(RuntimeError, match="n_cells"):
            G.set_cell_permeability(np.ones(nc + 1))
        assert np.array_equal(G.get_cell_permeability_tensor()[0], good) and np.array_equal(G.pres_apply_jacobian(x), y)
        # the scalar getter while a tensor is set: the tensor's kind; its `out` is refused with the other getter's name
        import ctypes as C
        kind = C.c_int32(-1)
        assert G.L.poro_ctx_get_cell_permeability(G.ptr, None, 0, C.byref(kind)) == 0 and kind.value == 2
        with pytest.raises(RuntimeError, match="poro_ctx_get_cell_permeability_tensor"):
            G.get_cell_permeability()
        # scalar and tensor replace each other, in either order
        s = good[:, 0].copy()
        G.set_cell_permeability(s)
        assert G.get_cell_permeability_tensor() == (None, 0)
        gs, ks = G.get_cell_permeability()
        assert ks == 2 and np.array_equal(gs, s)
        G.pres_assemble_jacobian(DT)
        ys = G.pres_apply_jacobian(x)
        assert abs(ys - (jacobian(P, np.repeat(s[:, None], 3, axis=1)) @ x)).max() <= 1e-12 * abs(ys).max()
        G.set_cell_permeability_tensor(good)
        G.pres_assemble_jacobian(DT)
        assert np.array_equal(G.get_cell_permeability_tensor()[0], good) and np.array_equal(G.pres_apply_jacobian(x), y)
        G.set_cell_permeability(None)                                                 # NULL to either setter drops whichever field is set
        assert G.get_cell_permeability_tensor() == (None, 0) and G.get_cell_permeability() == (None, 0)
    finally:
        G.close(); P.close()
    # partitioned contexts: the test hook of the partitioned code path, and a 2-slab descriptor
    monkeypatch.setenv("PORO_FORCE_PARTITIONED_PATH", "1")
    P = box((3, 2, 2)); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    monkeypatch.delenv("PORO_FORCE_PARTITIONED_PATH")
    try:
        with pytest.raises(RuntimeError, match="one rank"):
            G.set_cell_permeability_tensor(np.ones((P.desc.n_cells, 3)))
    finally:
        G.close(); P.close()
    P = pk.Problem.box(3, [3, 2, 4], [3.0, 2.0, 4.0], 1, mat1(), rollers(3), (), 0, 2); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        with pytest.raises(RuntimeError, match="one rank"):
            G.set_cell_permeability_tensor(np.ones((P.desc.n_cells, 3)))
    finally:
        G.close(); P.close()
    # the two-level form of the pressure system on a refined box, and FDM on the Gmsh mesh
    for name, P in general_meshes():
        G = pk.Context(P, 0, pk.OP_CSR)
        try:
            had = G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)
            G.set_cell_permeability_tensor(centre_field(P))
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


# ---- 9. time steps and adaptation ----------------------------------------------------------------------------------------------------------------------------
HEIGHT, SIGMA0 = 6.0, 1e5
KW = dict(fss_tol=1e-11, pressure_tol=1e-11, max_fss=200, max_it=50000)      # absolute residual norms, as test_terzaghi.py


def layered_column(dim, n, deg, mask=None):
    """a column held at the bottom and loaded at its drained top; kv = kh / 100 in the reservoir, and the two top cell layers are a caprock of 1e-3 times that"""
    last = dim - 1
    bc = [(2 * d, d, 0.0) for d in range(last)] + [(2 * d + 1, d, 0.0) for d in range(last)] + [(2 * last, last, 0.0)]
    m = material(flow_rate=0.0)
    size = [float(v) for v in n[:-1]] + [HEIGHT]
    if mask is None:
        P = pk.Problem.box(dim, list(n), size, deg, m, bc, [(2 * last + 1, last, -SIGMA0)])
    else:
        P = pk.Problem.refined_box_mask(dim, list(n), size, deg, m, bc, mask, [(2 * last + 1, last, -SIGMA0)])
    P.set_pressure_bc([(2 * last + 1, 0.0)])
    k = m.k_over_mu
    layers = [(HEIGHT / 2 - 2 * HEIGHT / n[-1],) + (k,) * last + (1e-2 * k,), (HEIGHT / 2,) + (1e-3 * k,) * last + (1e-5 * k,)]
    return P, m, layers


def test_time_steps_on_a_layered_column():
    runs = {}
    for name, mode, kw in (("mf", pk.OP_MATRIX_FREE, dict(prec=-1)), ("csr", pk.OP_CSR, dict(jacobi_p=True))):
        P, m, layers = layered_column(3, (4, 4, 6), 2)
        P.set_permeability_tensor_layers(layers)
        field = P.cell_permeability_tensor()
        P.set_cell_permeability_tensor(None)
        assert field.shape == (96, 3) and np.array_equal(field[:, 2].reshape(6, 16), np.repeat([[1e-2], [1e-2], [1e-2], [1e-2], [1e-5], [1e-5]], 16, axis=1) * m.k_over_mu)
        trace, G = pk.run_problem(P, 3, 1e5, 60.0, 0, mode, coupled_fss=True, permeability_tensor=field, **KW, **kw)
        try:
            got, kind = G.get_cell_permeability_tensor()
            assert kind == 1 and np.array_equal(got, field) and np.array_equal(P.cell_permeability_tensor(), field)
            rows = trace[1:]
            runs[name] = (rows, G.get(pk.VEC_P), G.get(pk.VEC_U))
        finally:
            G.close(); P.close()
    (r1, p1, u1), (r2, p2, u2) = runs["mf"], runs["csr"]
    ep, eu = abs(p1 - p2).max() / abs(p2).max(), abs(u1 - u2).max() / abs(u2).max()
    print(f"fixed-stress iterations {len(r1)} / {len(r2)}; pressure CG iterations {r1[:, 7].max():.0f} / {r2[:, 7].max():.0f}; p {ep:.2e} u {eu:.2e}")
    assert len(r1) == len(r2) and len(r1) < 3 * KW["max_fss"]
    assert r1[:, 7].max() == 0 and r2[:, 7].max() > 0                                 # the direct pressure solve: no CG iteration in any step of the matrix-free run
    assert ep <= 1e-6 and eu <= 1e-6


def test_adaptation_carries_the_tensor():
    P, m, layers = layered_column(2, (4, 6), 1, mask=np.zeros(24, dtype=np.int32))
    P.set_permeability_tensor_layers(layers)
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=1e5, dt=60.0, coupled_fss=True, prec=-1, **KW)
    try:
        R.initialize()
        old = R.ctx.get_cell_permeability_tensor()[0]
        assert old.shape == (24, 2) and np.array_equal(old, P.cell_permeability_tensor())
        R.step()
        before, after = R.adapt()
        assert after > before
        coarse, child = R.problem.cell_parents()
        new, kind = R.ctx.get_cell_permeability_tensor()
        assert np.array_equal(new, old[coarse]) and (child >= 0).any()               # the first mesh is the coarse box itself: a child takes its parent's components, exactly
        assert np.array_equal(R.problem.cell_permeability_tensor(), new) and kind == 2       # (no lattice on a mesh with hanging nodes)
        assert R.preconditioners()[1] == pk.PREC_JACOBI
        rows = R.step()[0]
        print(f"cells {before} -> {after}; field kind {kind}; step after the adaptation: {len(rows)} fixed-stress iterations, error {rows[-1, 5]:.2e}")
        assert len(rows) < KW["max_fss"] and rows[-1, 5] <= KW["fss_tol"]
    finally:
        R.close(); P.close()

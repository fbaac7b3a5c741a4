"""The general-mesh reference of tests/general_reference.py against the CPU oracle on skewed, non-affine and locally refined meshes (no GPU), and
convention-free checks of both: on meshes whose cells are all axis-aligned the MappingQ1 Jacobian is diagonal, so a transposed J^-1, a wrong cofactor
or a wrong face normal would pass every comparison of the product with the oracle (they are written the same way).  The checks below hold for any
correct FE code: rigid motions are in the kernel of the elasticity operator, Q1 / Q2 on MappingQ1 cells contain the linear fields (patch test), the
mass matrix sums to the measure of the domain, a uniform traction integrates to t n area, and the projected strain of a linear field is its
symmetric gradient."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
import oracle_py
from common import BC_2D, BC_3D, REF, csr_to_scipy, global_problem, material
from general_reference import (MAPS, GeneralReference, cell_vertices, distorted_msh, mapped, multilinear, multilinear_corners, q1_at, rule_1d,
                               shear)

SIZE = 10.0


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def source(dim, deg, bc=True, neumann=()):
    """a mildly graded box (cells of different sizes, no box tag)"""
    n = [4, 3, 3][:dim] if deg == 2 else [5, 4, 3][:dim]
    return pk.Problem.graded_box(dim, n, [SIZE] * dim, deg, material(), (BC_2D if dim == 2 else BC_3D) if bc else [], [0.4, -0.3, 0.2][:dim], neumann)


MAP_CASES = [(m, dim, deg) for m in MAPS for dim in (2, 3) for deg in (1, 2)]
MAP_IDS = [f"{m}-{d}d-q{k}" for m, d, k in MAP_CASES]


def compare(M, x_seed=3):
    O = oracle_py.Oracle(M, hoisted=True)
    try:
        O.fill(pk.VEC_P, 0.0); O.disp_assemble_system(True)
        R = GeneralReference(M)
        A = csr_to_scipy(*O.export_csr(pk.MAT_A_U))
        for x in (np.random.default_rng(x_seed).standard_normal(R.n_u), np.sin(0.37 * np.arange(R.n_u))):
            y = R.apply_A(x)
            assert (e := rel(y, O.apply(pk.MAT_A_U, x))) <= 1e-12, e
            assert (e := rel(y, A @ x)) <= 1e-12, e
        assert (e := rel(R.diag_A(), A.diagonal())) <= 1e-12, e
    finally:
        O.close()


# ---- the reference against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dim,deg", MAP_CASES, ids=MAP_IDS)
def test_reference_equals_the_oracle_on_mapped_boxes(name, dim, deg):
    P = source(dim, deg)
    M = mapped(P, MAPS[name](P))
    try:
        compare(M)
    finally:
        M.close()


@pytest.mark.parametrize("dim,deg", [(2, 1), (2, 2), (3, 1), (3, 2)], ids=str)
def test_reference_equals_the_oracle_on_a_mapped_refined_box(dim, deg):
    """hanging nodes: both return the unconstrained product (the condensation happens inside the solvers)"""
    P = global_problem("refined:" + ",".join(["4"] * dim), deg)
    assert P.desc.cons_u.n > 0
    M = mapped(P, multilinear(P))
    try:
        compare(M)
    finally:
        M.close()


@pytest.mark.parametrize("deg,refine", [(1, 0), (2, 0), (1, 1), (2, 1)], ids=str)
def test_reference_equals_the_oracle_on_the_distorted_gmsh_grid(tmp_path, deg, refine):
    P = pk.Problem.gmsh(distorted_msh(tmp_path), deg, material(), BC_2D, refine=refine)
    try:
        compare(P)
    finally:
        P.close()


# ---- convention-free checks ----------------------------------------------------------------------------------------------------------------------
def systems(M):
    """(oracle with its system assembled at p = 0, reference)"""
    O = oracle_py.Oracle(M, hoisted=True)
    O.fill(pk.VEC_P, 0.0); O.disp_assemble_system(True)
    return O, GeneralReference(M)


KAT_CASES = [(m, dim, deg) for m in ("shear", "multilinear", "jitter") for dim in (2, 3) for deg in (1, 2)]
KAT_IDS = [f"{m}-{d}d-q{k}" for m, d, k in KAT_CASES]


@pytest.mark.parametrize("name,dim,deg", KAT_CASES, ids=KAT_IDS)
def test_rigid_rotation_is_in_the_kernel(name, dim, deg):
    P = source(dim, deg, bc=False)
    M = mapped(P, MAPS[name](P))
    O, R = systems(M)
    try:
        W = np.array([[0.0, 0.7, -0.4], [-0.7, 0.0, 0.9], [0.4, -0.9, 0.0]])[:dim, :dim]
        u = R.linear_field(W) + 0.3                                   # rotation + translation
        scale = R.diag_A().max() * np.abs(u).max()
        for what, y in (("oracle", O.apply(pk.MAT_A_U, u)), ("reference", R.apply_A(u))):
            assert np.abs(y).max() <= 1e-12 * scale, (what, np.abs(y).max() / scale)
    finally:
        O.close(); M.close()


@pytest.mark.parametrize("name,dim,deg", KAT_CASES, ids=KAT_IDS)
def test_patch_test_linear_displacement_and_uniform_pressure(name, dim, deg):
    P = source(dim, deg, bc=False)
    M = mapped(P, MAPS[name](P))
    O, R = systems(M)
    try:
        B = np.array([[0.3, -0.5, 0.2], [0.7, 0.1, -0.4], [-0.6, 0.25, 0.45]])[:dim, :dim]
        u = R.linear_field(B)
        inner = ~R.boundary_dofs()
        assert inner.any()
        for what, y in (("oracle", O.apply(pk.MAT_A_U, u)), ("reference", R.apply_A(u))):
            assert np.abs(y[inner]).max() <= 1e-12 * np.abs(y).max(), (what, np.abs(y[inner]).max() / np.abs(y).max())
        # alpha int p div(phi_i) for uniform p = alpha p int_dK phi_i n: zero on the interior rows
        O.fill(pk.VEC_P, REF["p_init"]); O.disp_assemble_system(False)
        b = O.get(pk.VEC_RHS_U)
        assert np.abs(b[inner]).max() <= 1e-12 * np.abs(b).max(), np.abs(b[inner]).max() / np.abs(b).max()
    finally:
        O.close(); M.close()


def exact_measure(name, P, f):
    """the measure of the mapped box from the map alone"""
    dim = P.desc.dim
    if name == "shear":
        return np.linalg.det(f.matrix) * SIZE ** dim
    if name == "jitter":
        return SIZE ** dim
    t, w = rule_1d(4)                                                 # det of a multilinear map: degree <= dim - 1 per direction
    pts = np.array(list(np.ndindex(*([4] * dim))))[:, ::-1]
    _, dN = q1_at(dim, t[pts])
    J = np.einsum("va,qvb->qab", f.corners, dN)
    return float((np.linalg.det(J) * np.prod(w[pts], axis=1)).sum())


def p_boundary(desc):
    """pressure dofs on faces that belong to one cell only"""
    dim = desc.dim
    cv, cdp = cell_vertices(desc), np.ctypeslib.as_array(desc.cell_dofs_p, shape=(desc.n_cells, 1 << dim))
    count = {}
    for a in range(dim):
        for side in (0, 1):
            vs = [v for v in range(1 << dim) if ((v >> a) & 1) == side]
            for c, key in enumerate(map(tuple, np.sort(cv[:, vs], axis=1))):
                count.setdefault(key, []).append(cdp[c, vs])
    out = np.zeros(desc.n_dofs_p, bool)
    for key, owners in count.items():
        if len(owners) == 1:
            out[owners[0]] = True
    return out


def p_positions(desc, X):
    cv, cdp = cell_vertices(desc), np.ctypeslib.as_array(desc.cell_dofs_p, shape=(desc.n_cells, 1 << desc.dim))
    pos = np.zeros((desc.n_dofs_p, desc.dim)); pos[cdp.ravel()] = X[cv.ravel()]
    return pos


@pytest.mark.parametrize("name,dim", [(m, d) for m in ("shear", "multilinear", "jitter") for d in (2, 3)], ids=str)
def test_pressure_matrices_measure_and_linear_fields(name, dim):
    P = source(dim, 1, bc=False)
    f = MAPS[name](P)
    M = mapped(P, f)
    O = oracle_py.Oracle(M, hoisted=True)
    try:
        O.pres_assemble_jacobian(REF["dt"])
        Mp = csr_to_scipy(*O.export_csr(pk.MAT_MASS_P))
        vol = exact_measure(name, P, f)
        assert abs(Mp.sum() - vol) <= 1e-12 * vol, (Mp.sum(), vol)
        assert abs(GeneralReference(M).measure() - vol) <= 1e-12 * vol
        Kp = csr_to_scipy(*O.export_csr(pk.MAT_LAPLACE_P))
        q = p_positions(M.desc, M.coords) @ np.array([0.4, -1.3, 0.8])[:dim] + 2.0
        y = Kp @ q
        inner = ~p_boundary(M.desc)
        assert inner.any() and np.abs(y[inner]).max() <= 1e-12 * np.abs(y).max(), np.abs(y[inner]).max() / np.abs(y).max()
    finally:
        O.close(); M.close()


def test_pressure_mass_of_the_distorted_gmsh_grid_is_the_polygon_area(tmp_path):
    P = pk.Problem.gmsh(distorted_msh(tmp_path), 1, material(), BC_2D)
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        O.pres_assemble_jacobian(REF["dt"])
        c = multilinear_corners(2, np.array([-5.0, -5.0]), np.array([5.0, 5.0]))[[0, 1, 3, 2]]    # counter-clockwise
        area = 0.5 * abs(np.dot(c[:, 0], np.roll(c[:, 1], -1)) - np.dot(c[:, 1], np.roll(c[:, 0], -1)))
        s = csr_to_scipy(*O.export_csr(pk.MAT_MASS_P)).sum()
        assert abs(s - area) <= 1e-12 * area, (s, area)
    finally:
        O.close(); P.close()


@pytest.mark.parametrize("name,dim,deg", [(m, d, k) for m in ("shear", "jitter") for d in (2, 3) for k in (1, 2)], ids=str)
def test_uniform_neumann_traction_integrates_to_t_n_area(name, dim, deg):
    """label 0 = the face x = x_min: component-c loads sum to t n_c |face| (the value x normal-component convention of the reference)"""
    t = 2.5e6
    P = source(dim, deg, bc=False, neumann=[(0, c, t) for c in range(dim)])
    f = MAPS[name](P)
    M = mapped(P, f)
    O = oracle_py.Oracle(M, hoisted=True)
    try:
        O.fill(pk.VEC_P, 0.0); O.disp_assemble_system(True)
        b = O.get(pk.VEC_RHS_U)
        _, comp = GeneralReference(M).node_coords()
        N = -np.eye(dim)[0]
        if name == "shear":                                           # n dA = det(S) S^-T N dA_ref
            S = f.matrix
            want = t * np.linalg.det(S) * np.linalg.solve(S.T, N) * SIZE ** (dim - 1)
        else:
            want = t * N * SIZE ** (dim - 1)
        got = np.array([b[comp == c].sum() for c in range(dim)])
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (got, want)
    finally:
        O.close(); M.close()


@pytest.mark.parametrize("name,dim,deg", [(m, d, k) for m in ("shear", "multilinear", "jitter") for d in (2, 3) for k in (1, 2)], ids=str)
def test_projection_rhs_of_a_linear_field_sums_to_its_strain(name, dim, deg):
    P = source(dim, deg, bc=False)
    f = MAPS[name](P)
    M = mapped(P, f)
    O = oracle_py.Oracle(M, hoisted=True)
    try:
        B = np.array([[0.3, -0.5, 0.2], [0.7, 0.1, -0.4], [-0.6, 0.25, 0.45]])[:dim, :dim] * 1e-4
        O.set(pk.VEC_U, GeneralReference(M).linear_field(B))
        pairs = [(a, c) for a in range(dim) for c in range(a, dim)]
        O.proj_assemble_rhs([a * dim + c for a, c in pairs])
        vol = exact_measure(name, P, f)
        for a, c in pairs:
            e = a * dim + c - a * (a + 1) // 2
            want = 0.5 * (B[a, c] + B[c, a]) * vol
            assert abs(O.get(pk.VEC_PROJ_RHS0 + e).sum() - want) <= 1e-12 * np.abs(B).max() * vol, (a, c)
    finally:
        O.close(); M.close()


def test_shear_map_is_affine_and_the_one_vertex_map_is_not():
    """the maps do what their names say: parallelepipeds under shear, one moved vertex under one_vertex"""
    P = source(3, 2)
    try:
        X = np.ctypeslib.as_array(P.desc.vertex_coords, shape=(P.desc.n_vertices, 3)).copy()
        Y = shear(P)(X)
        cv = cell_vertices(P.desc)
        e = Y[cv]
        para = e[:, 0][:, None] + (e[:, [1]] - e[:, [0]]) * np.array([v & 1 for v in range(8)])[None, :, None] \
            + (e[:, [2]] - e[:, [0]]) * np.array([(v >> 1) & 1 for v in range(8)])[None, :, None] + (e[:, [4]] - e[:, [0]]) * np.array([v >> 2 for v in range(8)])[None, :, None]
        assert np.abs(para - e).max() <= 1e-12 * SIZE
        moved = np.abs(MAPS["one_vertex"](P)(X) - Y).max(axis=1)
        assert (moved > 0).sum() == 1
    finally:
        P.close()

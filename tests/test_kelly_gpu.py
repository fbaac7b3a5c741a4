"""The Kelly error indicator on the device (poro_pres_estimate_error; KellyErrorEstimator<dim>::estimate, PoroelasticityFSS.h:452-458) against an independent NumPy
model of the definition in include/poroel_hip.h.  The model finds neighbours and hanging subfaces by COORDINATES (not through the constraint list), takes the normal
from the face's tangents (not from cofactors) and finds the neighbour's reference point by Newton's method on its map: it shares no code with the library."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, BC_3D, DOMAIN_MSH, box_problem, material
from test_constraints_cpu import MESHES, cons_arrays

pytestmark = pytest.mark.gpu

G2 = (0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def q1(dim, xi):
    """values [nv] and reference gradients [nv][dim] of the Q1 basis (vertex v = bits of v, x fastest) at xi"""
    nv = 2 ** dim; N = np.ones(nv); dN = np.ones((nv, dim))
    for v in range(nv):
        for k in range(dim):
            b = (v >> k) & 1; f = xi[k] if b else 1.0 - xi[k]; df = 1.0 if b else -1.0
            N[v] *= f
            for g in range(dim):
                dN[v, g] *= df if g == k else f
    return N, dN


def grad_phys(dim, Xc, pc, xi):
    N, dN = q1(dim, xi)
    J = Xc.T @ dN                                  # J[r][b] = d x_r / d xi_b
    return np.linalg.solve(J.T, dN.T @ pc)


def invert_map(dim, Xc, x):
    xi = np.full(dim, 0.5)
    for _ in range(30):
        N, dN = q1(dim, xi)
        r = N @ Xc - x
        if np.abs(r).max() <= 1e-14 * max(1.0, np.abs(Xc).max()):
            break
        xi = xi - np.linalg.solve(Xc.T @ dN, r)
    assert np.abs(q1(dim, xi)[0] @ Xc - x).max() <= 1e-12 * max(1.0, np.abs(Xc).max())
    return xi


def face_vertices(dim, f):
    d, side = f // 2, f % 2
    return [v for v in range(2 ** dim) if ((v >> d) & 1) == side]


def face_integral(dim, Xa, pa, fa, Xb, pb):
    """J_F on face fa of cell A against cell B: Gauss(2) on A's face, its own surface element and normal"""
    fv = face_vertices(dim, fa); V = Xa[fv]; d, side = fa // 2, fa % 2; tang = [k for k in range(dim) if k != d]
    total = 0.0
    pts = [(s,) for s in G2] if dim == 2 else [(s, t) for t in G2 for s in G2]
    for st in pts:
        xi = np.zeros(dim); xi[d] = side
        for k, val in zip(tang, st):
            xi[k] = val
        if dim == 2:
            x = (1 - st[0]) * V[0] + st[0] * V[1]; t1 = V[1] - V[0]
            nrm = np.array([t1[1], -t1[0]])
        else:
            s, t = st
            x = (1 - s) * (1 - t) * V[0] + s * (1 - t) * V[1] + (1 - s) * t * V[2] + s * t * V[3]
            t1 = (1 - t) * (V[1] - V[0]) + t * (V[3] - V[2]); t2 = (1 - s) * (V[2] - V[0]) + s * (V[3] - V[1])
            nrm = np.cross(t1, t2)
        dS = np.linalg.norm(nrm); n = nrm / dS
        ga = grad_phys(dim, Xa, pa, xi)
        gb = grad_phys(dim, Xb, pb, invert_map(dim, Xb, x))
        total += (0.5 ** (dim - 1)) * (n @ (ga - gb)) ** 2 * dS
    return total


def cell_diameters(P):
    """the longest vertex diagonal of every cell"""
    d = P.desc; nv = 2 ** d.dim
    Xc = P.array("vertex_coords", (d.n_vertices, d.dim))[P.array("cell_vertices", (d.n_cells, nv), np.int32)]
    return np.array([max(np.linalg.norm(Xc[c, nv - 1 - v] - Xc[c, v]) for v in range(nv // 2)) for c in range(d.n_cells)])


def kelly_model(P, p):
    d = P.desc; dim = d.dim; nv = 2 ** dim; nc = d.n_cells
    X = P.array("vertex_coords", (d.n_vertices, dim)); cv = P.array("cell_vertices", (nc, nv), np.int32); cp = P.array("cell_dofs_p", (nc, nv), np.int32)
    Xc = X[cv]; pc = np.asarray(p)[cp]
    scale = np.abs(X).max()
    diam = cell_diameters(P)
    # faces by coordinates: key = the rounded, sorted vertex coordinates
    faces = {}
    for c in range(nc):
        for f in range(2 * dim):
            V = Xc[c, face_vertices(dim, f)]
            key = tuple(sorted(tuple(np.round(v / scale * 1e9).astype(np.int64)) for v in V))
            faces.setdefault(key, []).append((c, f))
    eta2 = np.zeros(nc); single = []
    n_regular = n_sub = 0
    for key, lst in faces.items():
        assert len(lst) <= 2
        if len(lst) == 2:
            (a, fa), (b, fb) = lst
            J = face_integral(dim, Xc[a], pc[a], fa, Xc[b], pc[b])
            eta2[a] += diam[a] / 24 * J; eta2[b] += diam[b] / 24 * J; n_regular += 1
        else:
            single.append(lst[0])
    # single faces: a face whose bounding box lies inside another single face's (larger) bounding box is a subface of that one; what is left is the boundary
    box = {(c, f): (Xc[c, face_vertices(dim, f)].min(axis=0), Xc[c, face_vertices(dim, f)].max(axis=0)) for c, f in single}
    tol = 1e-9 * scale
    for (a, fa) in single:
        lo, hi = box[(a, fa)]
        for (b, fb) in single:
            if b == a:
                continue
            Lo, Hi = box[(b, fb)]
            if np.all(lo >= Lo - tol) and np.all(hi <= Hi + tol) and np.any((hi - lo) < (Hi - Lo) - tol):
                J = face_integral(dim, Xc[a], pc[a], fa, Xc[b], pc[b])
                eta2[a] += diam[b] / 24 * J; eta2[b] += diam[b] / 24 * J; n_sub += 1      # the factor of BOTH sides from the coarse cell
                break
    return np.sqrt(eta2), dict(regular=n_regular, sub=n_sub)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------------------
def l_mask_3d(n):
    m = np.zeros(n[::-1], dtype=np.int32); m[:, :, 0] = 1; m[:, 0, :] = 1
    return m.reshape(-1)


def make(name):
    if name == "box2d":
        return box_problem(2, (5, 4), 2)
    if name == "box3d":
        return box_problem(3, (4, 3, 3), 1)
    if name.startswith("refined"):
        dim, n, deg, lo, hi = MESHES[int(name[-1])]
        return pk.Problem.refined_box(dim, n, [10.0] * dim, deg, material(), BC_2D if dim == 2 else BC_3D, lo, hi)
    if name == "lmask3d":
        return pk.Problem.refined_box_mask(3, (5, 4, 3), [10.0] * 3, 1, material(), BC_3D, l_mask_3d((5, 4, 3)))
    if name == "gmsh":
        return pk.Problem.gmsh(DOMAIN_MSH, 1, material(), BC_2D)
    raise KeyError(name)


ALL = ["box2d", "box3d", "refined0", "refined1", "refined2", "refined3", "lmask3d", "gmsh"]


def conforming(P, v):
    v = np.array(v, dtype=float)
    dof, ptr, m, w, _ = cons_arrays(P.desc.cons_p)
    for i in range(len(dof)):
        v[dof[i]] = w[ptr[i]:ptr[i + 1]] @ v[m[ptr[i]:ptr[i + 1]]]
    return v


def dof_coords(P):
    """coordinates of the pressure dofs (through the cells: dof numbering and vertex numbering need not coincide)"""
    d = P.desc; nv = 2 ** d.dim
    X = P.array("vertex_coords", (d.n_vertices, d.dim)); cv = P.array("cell_vertices", (d.n_cells, nv), np.int32); cp = P.array("cell_dofs_p", (d.n_cells, nv), np.int32)
    out = np.zeros((d.n_dofs_p, d.dim)); out[cp.reshape(-1)] = X[cv.reshape(-1)]
    return out


# ---- 5. a linear function has no jumps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_linear_pressure_gives_zero(name):
    P = make(name); G = pk.Context(P, 0, pk.OP_CSR)
    try:
        dim = P.desc.dim; g = np.array([1.5, -2.0, 0.75][:dim])
        G.set(pk.VEC_P, dof_coords(P) @ g)                  # linear: conforming on any mesh
        eta = G.pres_estimate_error()
        bound = 1e-12 * np.linalg.norm(g) * cell_diameters(P) ** ((dim + 1) / 2)
        print(name, "max eta / bound", (eta / bound).max())
        assert eta.shape == (P.desc.n_cells,) and np.all(eta >= 0) and np.all(eta <= bound)
    finally:
        G.close(); P.close()


# ---- 6. closed form -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("box2d", (5, 4)), ("box3d", (4, 3, 3))])
def test_closed_form_for_x_squared(name, n):
    """p = nodal interpolant of x^2 on a uniform box: the normal derivative jumps by 2 h_x across every interior x face and nowhere else, so
    eta^2 = (diam / 24) * 2 * (2 h_x)^2 * |F_x| in a cell with two interior x faces and half of that in a cell at an x boundary"""
    P = make(name); G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        dim = len(n); h = 10.0 / np.array(n); X = dof_coords(P)
        G.set(pk.VEC_P, X[:, 0] ** 2)
        eta = G.pres_estimate_error()
        area = np.prod(h[1:]); diam = np.linalg.norm(h)
        full = diam / 24 * 2 * (2 * h[0]) ** 2 * area
        ix = np.arange(P.desc.n_cells) % n[0]
        want = np.sqrt(np.where((ix == 0) | (ix == n[0] - 1), 0.5 * full, full))
        print(name, "max rel err", (np.abs(eta - want) / want).max())
        assert np.all(np.abs(eta - want) <= 1e-13 * want)
    finally:
        G.close(); P.close()


# ---- 7. random conforming functions against the model ---------------------------------------------------------------------------------------------------
_MODEL = {}


def model_case(name):
    """(p, model eta, model info) of a mesh: computed once, shared by the tests, never changed"""
    if name not in _MODEL:
        P = make(name)
        try:
            rng = np.random.default_rng(100 + ALL.index(name))
            p = conforming(P, rng.standard_normal(P.desc.n_dofs_p))
            eta, info = kelly_model(P, p)
            p.setflags(write=False); eta.setflags(write=False)
            _MODEL[name] = (p, eta, info)
        finally:
            P.close()
    return _MODEL[name]


@pytest.mark.parametrize("name", ALL)
def test_random_conforming_pressure_against_the_model(name):
    p, want, info = model_case(name)
    P = make(name)
    try:
        d = P.desc
        if name.startswith("refined") or name == "lmask3d":
            assert info["sub"] > 0 and d.cons_p.n > 0
        if name == "lmask3d":
            n_faces = info["regular"] + info["sub"]
            assert n_faces > 512 and n_faces % 256 != 0                              # several workgroups of the face kernel, a ragged last one
        results = []
        for mode in (pk.OP_CSR, pk.OP_MATRIX_FREE):
            G = pk.Context(P, 0, mode)
            try:
                G.set(pk.VEC_P, p)
                e1 = G.pres_estimate_error(); e2 = G.pres_estimate_error(pk.VEC_P)
                assert np.array_equal(e1, e2)                                          # no atomics: bitwise the same from call to call
                assert np.array_equal(G.get(pk.VEC_P), p)                              # the vector is only read
                G.set(pk.VEC_EPSV, 2.0 * p)                                            # any pressure-space vector
                assert np.allclose(G.pres_estimate_error(pk.VEC_EPSV), 2.0 * e1, rtol=1e-14, atol=0.0)
                s, launches = G.timer("kelly")
                assert launches == 0                                                   # (timing is off until asked for)
                G.timers_reset(); G.pres_estimate_error(); s, launches = G.timer("kelly")
                assert launches == 1 and s > 0
                results.append(e1)
            finally:
                G.close()
        err = np.abs(results[0] - want).max()
        print(name, "cells", d.n_cells, "faces", info["regular"], "+", info["sub"], "max |eta - model| / max eta", err / want.max())
        assert err <= 1e-12 * want.max()
        assert np.array_equal(results[0], results[1])                                  # the operator mode does not enter
    finally:
        P.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    P = make("box2d"); G = pk.Context(P, 0, pk.OP_CSR)
    try:
        for which in (12345, pk.VEC_U, pk.VEC_RHS_U, pk.VEC_DIAG_U):
            with pytest.raises(RuntimeError) as e:
                G.pres_estimate_error(which)
            assert "vector" in str(e.value)
        assert G.pres_estimate_error().shape == (P.desc.n_cells,)                       # the context is still usable
    finally:
        G.close(); P.close()
    # real pieces of a partition: a slab of a box, and a piece of a general partition
    S = box_problem(3, (2, 2, 4), 1, rank=0, n_ranks=2)
    W = make("refined1"); piece = W.partition(1, 2)
    try:
        for Q in (S, piece):
            G = pk.Context(Q, 0, pk.OP_CSR)
            try:
                with pytest.raises(RuntimeError) as e:
                    G.pres_estimate_error()
                assert "partitioned" in str(e.value)
            finally:
                G.close()
    finally:
        S.close(); piece.close(); W.close()

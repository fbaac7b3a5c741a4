"""Plain fp64 NumPy reference of the two gravity vectors on any MappingQ1 mesh, from the descriptor's geometry and dof lists alone (its own Gauss points and Lagrange
basis through tests/general_reference.py; poro_desc.fe is never read).  Helper module of the test-suite, not collected.

  body_force(P, g, rho)             b_i = sum_c rho_c int_c g . phi_i                         rho: one scalar, or one value per cell
  gravity_flux(P, g, rho_f, kappa)  f_i = -sum_c rho_f int_c (kappa_c g) . grad(phi_i)        kappa: one scalar, [n_cells], or [n_cells, dim] (diagonal tensor)
  laplace_apply(P, kappa, p)        (K_kappa p)_i = sum_c int_c grad(phi_i) . kappa_c grad(p_h)
  cell_volumes(P), vertex_of_dof_p(P)

The identities the tests use: for p_h = rho_f g . x + const, K_kappa p_h + f = 0 on every row; sum_i f_i = 0; sum_i b_i[component d] = g_d sum_c rho_c |c|."""
import numpy as np

from general_reference import cell_vertices, q1_at, rule_1d, tensor_shapes, vertices


def _arrays(P):
    d = P.desc
    dim = d.dim
    X = getattr(P, "coords", None)
    X = vertices(P) if X is None else np.asarray(X)
    cv = cell_vertices(d)
    cdu = np.ctypeslib.as_array(d.cell_dofs_u, shape=(d.n_cells, (d.degree_u + 1) ** dim * dim)).copy()
    cdp = np.ctypeslib.as_array(d.cell_dofs_p, shape=(d.n_cells, 1 << dim)).copy()
    return d, dim, X, cv, cdu, cdp


def _points(dim, n):
    t1, w1 = rule_1d(n)
    qi = np.array(list(np.ndindex(*([n] * dim))))[:, ::-1]
    return t1, t1[qi], np.prod(w1[qi], axis=1)


def _per_cell(values, n_cells, dim):
    """kappa as [n_cells, dim]"""
    k = np.asarray(values, dtype=np.float64)
    if k.ndim == 0:
        return np.full((n_cells, dim), float(k))
    if k.ndim == 1:
        return np.repeat(k[:, None], dim, axis=1)
    return k


def cell_volumes(P):
    d, dim, X, cv, _, _ = _arrays(P)
    _, xi, w = _points(dim, d.degree_u + 1)
    _, dN = q1_at(dim, xi)
    return (np.linalg.det(np.einsum("eva,qvb->eqab", X[cv], dN)) * w).sum(axis=1)


def body_force(P, g, rho):
    d, dim, X, cv, cdu, _ = _arrays(P)
    k = d.degree_u
    t1, xi, w = _points(dim, k + 1)
    phi, _ = tensor_shapes(dim, k, t1)                                  # [q][s]
    _, dN = q1_at(dim, xi)
    jxw = np.linalg.det(np.einsum("eva,qvb->eqab", X[cv], dN)) * w    # [e][q]
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (d.n_cells,))
    integ = np.einsum("eq,qs->es", jxw, phi) * rho[:, None]            # rho_c int_c phi_s
    b = np.zeros(d.n_dofs_u)
    for c in range(dim):
        np.add.at(b, cdu[:, c::dim].ravel(), (g[c] * integ).ravel())
    return b


def _p_geometry(P):
    d, dim, X, cv, _, cdp = _arrays(P)
    _, xi, w = _points(dim, 2)
    _, dN = q1_at(dim, xi)                                              # [q][v][b]
    J = np.einsum("eva,qvb->eqab", X[cv], dN)
    Gr = np.einsum("eqbd,qvb->eqvd", np.linalg.inv(J), dN)              # d phi_v / d x_d
    return d, dim, cdp, Gr, np.linalg.det(J) * w


def gravity_flux(P, g, rho_f, kappa):
    d, dim, cdp, Gr, jxw = _p_geometry(P)
    kg = _per_cell(kappa, d.n_cells, dim) * np.asarray(g, dtype=np.float64)[None, :]
    fe = -rho_f * np.einsum("eqvd,ed,eq->ev", Gr, kg, jxw)
    f = np.zeros(d.n_dofs_p)
    np.add.at(f, cdp.ravel(), fe.ravel())
    return f


def laplace_apply(P, kappa, p):
    d, dim, cdp, Gr, jxw = _p_geometry(P)
    kc = _per_cell(kappa, d.n_cells, dim)
    gp = np.einsum("eqvd,ev->eqd", Gr, np.asarray(p)[cdp])              # grad p_h at the points
    ye = np.einsum("eqvd,ed,eqd,eq->ev", Gr, kc, gp, jxw)
    y = np.zeros(d.n_dofs_p)
    np.add.at(y, cdp.ravel(), ye.ravel())
    return y


def laplace_abs_apply(P, kappa, p):
    """sum_j |K_ij| |p_j| with the entries of the cell matrices: the sum of the absolute values of the summands of a row of K_kappa p"""
    d, dim, cdp, Gr, jxw = _p_geometry(P)
    kc = _per_cell(kappa, d.n_cells, dim)
    Ke = np.einsum("eqvd,ed,eqwd,eq->evw", Gr, kc, Gr, jxw)
    ye = np.einsum("evw,ew->ev", np.abs(Ke), np.abs(np.asarray(p))[cdp])
    y = np.zeros(d.n_dofs_p)
    np.add.at(y, cdp.ravel(), ye.ravel())
    return y


def vertex_of_dof_p(P):
    """coordinates of every pressure dof (the vertices)"""
    d, dim, X, cv, _, cdp = _arrays(P)
    out = np.zeros((d.n_dofs_p, dim))
    out[cdp.ravel()] = X[cv.ravel()]
    return out

"""Plain fp64 NumPy reference of the flow post-processing (include/poroel_hip.h: Darcy velocity, boundary discharge, fluid mass balance) on any MappingQ1 mesh, from
the descriptor's geometry, dof lists and boundary-face list alone.  Its own Gauss(2) rule and its own MappingQ1 (the face normal comes from the cross product of the
face's tangents, oriented by the direction that leaves the cell - not from a cofactor column).  Helper module of the test-suite, not collected.

  cell_velocity(P, p, kappa, rho_f_g)       q_c = -kappa_c (grad p_h(x_c) - rho_f g) at the image of the reference centre              [n_cells, dim]
  face_discharge(P, p, kappa, rho_f_g)      Q_b = int_F q . n dS, Gauss(2) on the face, n outward                                        [n_bfaces]
  face_measures(P)                          |F_b| with the same rule (exact for the bilinear faces' normal integral only; used for scales)
  label_sums(P, Q, labels)                  sum of Q_b over the faces of each label
  balance_terms(...)                        the six sums and C^T(-r) from exported matrices and state vectors
kappa: one scalar, [n_cells], or [n_cells, dim] (diagonal tensor); rho_f_g: [dim] (zeros: no gravity flux)."""
import numpy as np

from general_reference import cell_vertices, vertices

GAUSS2 = np.array([0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0)])          # on [0, 1], both weights 1/2


def mesh(P):
    d = P.desc
    dim = d.dim
    X = getattr(P, "coords", None)
    X = vertices(P) if X is None else np.asarray(X)
    cv = cell_vertices(d)
    cdp = np.ctypeslib.as_array(d.cell_dofs_p, shape=(d.n_cells, 1 << dim)).copy()
    nb = d.n_bfaces
    bf = [np.ctypeslib.as_array(a, shape=(nb,)).copy() if nb else np.zeros(0, dtype=np.int32) for a in (d.bface_cell, d.bface_local, d.bface_id)]
    return d, dim, X, cv, cdp, bf


def q1_gradients(dim, xi):
    """d N_v / d xi_b of the Q1 basis at one reference point (vertices lexicographic, x fastest): [2^dim, dim]"""
    nv = 1 << dim
    dN = np.empty((nv, dim))
    for v in range(nv):
        for b in range(dim):
            t = 1.0 if (v >> b) & 1 else -1.0
            for a in range(dim):
                if a != b:
                    t *= xi[a] if (v >> a) & 1 else 1.0 - xi[a]
            dN[v, b] = t
    return dN


def per_cell(kappa, n_cells, dim):
    k = np.asarray(kappa, dtype=np.float64)
    if k.ndim == 0:
        return np.full((n_cells, dim), float(k))
    if k.ndim == 1:
        return np.repeat(k[:, None], dim, axis=1)
    return k


def _flux_at(Xc, pc, kc, rg, xi):
    """J [e][r][b] and q [e][r] of the cells (vertices Xc [e][v][r], nodal values pc [e][v], kappa kc [e][r]) at the reference point xi"""
    dN = q1_gradients(Xc.shape[2], xi)
    J = np.einsum("evr,vb->erb", Xc, dN)
    gh = np.einsum("ev,vb->eb", pc, dN)
    grad = np.linalg.solve(np.swapaxes(J, 1, 2), gh[:, :, None])[:, :, 0]            # J^T grad = grad_xi
    return J, -kc * (grad - np.asarray(rg)[None, :])


def cell_velocity(P, p, kappa, rho_f_g):
    d, dim, X, cv, cdp, _ = mesh(P)
    return _flux_at(X[cv], np.asarray(p)[cdp], per_cell(kappa, d.n_cells, dim), rho_f_g, np.full(dim, 0.5))[1]


def _face_points(dim, f):
    """reference points of local face f = 2 d + side and their weights"""
    dn, side = f >> 1, f & 1
    tang = [a for a in range(dim) if a != dn]
    pts = []
    for q in range(1 << (dim - 1)):
        xi = np.empty(dim)
        xi[dn] = float(side)
        for k, a in enumerate(tang):
            xi[a] = GAUSS2[(q >> k) & 1]
        pts.append(xi)
    return dn, side, tang, pts, 1.0 / (1 << (dim - 1))


def _normals(J, dn, side, tang):
    """n dS [e][r] from the face's own tangents T_a = J[:, :, a], oriented so that it leaves the cell (along +xi_dn on the high side, -xi_dn on the low side)"""
    if len(tang) == 1:
        T = J[:, :, tang[0]]
        N = np.stack([T[:, 1], -T[:, 0]], axis=1)
    else:
        N = np.cross(J[:, :, tang[0]], J[:, :, tang[1]])
    leave = J[:, :, dn] * (1.0 if side else -1.0)
    s = np.sign(np.einsum("er,er->e", N, leave))
    assert np.all(s != 0)
    return N * s[:, None]


def face_discharge(P, p, kappa, rho_f_g, with_measure=False):
    d, dim, X, cv, cdp, (bc, bl, _) = mesh(P)
    kc = per_cell(kappa, d.n_cells, dim)
    Q = np.zeros(d.n_bfaces); A = np.zeros(d.n_bfaces)
    p = np.asarray(p)
    for f in range(2 * dim):
        sel = np.nonzero(bl == f)[0]
        if not sel.size:
            continue
        cells = bc[sel]
        dn, side, tang, pts, w = _face_points(dim, f)
        for xi in pts:
            J, q = _flux_at(X[cv[cells]], p[cdp[cells]], kc[cells], rho_f_g, xi)
            N = _normals(J, dn, side, tang)
            Q[sel] += w * np.einsum("er,er->e", q, N)
            A[sel] += w * np.linalg.norm(N, axis=1)
    return (Q, A) if with_measure else Q


def face_measures(P):
    d = P.desc
    return face_discharge(P, np.zeros(d.n_dofs_p), 1.0, np.zeros(d.dim), with_measure=True)[1]


def label_sums(P, Q, labels):
    bid = mesh(P)[5][2]
    return np.array([Q[bid == l].sum() for l in labels])


def vertex_of_dof_p(P):
    d, dim, X, cv, cdp, _ = mesh(P)
    out = np.zeros((d.n_dofs_p, dim))
    out[cdp.ravel()] = X[cv.ravel()]
    return out


def constraints_p(P):
    """(dof, ptr, master, weight) of poro_desc.cons_p"""
    c = P.desc.cons_p
    n = c.n
    if not n:
        return np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)
    ptr = np.ctypeslib.as_array(c.ptr, shape=(n + 1,)).copy()
    return (np.ctypeslib.as_array(c.dof, shape=(n,)).copy(), ptr, np.ctypeslib.as_array(c.master, shape=(int(ptr[n]),)).copy(),
            np.ctypeslib.as_array(c.weight, shape=(int(ptr[n]),)).copy())


def prescribed_dofs_p(P):
    d = P.desc
    return np.ctypeslib.as_array(d.dirichlet_dof_p, shape=(d.n_dirichlet_p,)).copy() if d.n_dirichlet_p else np.zeros(0, np.int32)


def balance_terms(P, M, KK, src, p, p_old, ev, ev0, dt):
    """M: the pressure mass matrix, KK: kappa K (or K_kappa) - scipy matrices; src: the residual's source vector.  Returns a dict:
      terms      the six sums;  Rt = C^T(-r);  prescribed = the prescribed dofs in the descriptor's order
      scale      sum_i (|M t|_i + |kappa K p|_i + |src_i|): the sum of the absolute values behind the identity and behind every sum of rows of Rt
      scales     per term the sum of the absolute values of its own summands"""
    mat = P.desc.mat
    m = np.asarray(M.sum(axis=0)).ravel()
    a = mat.biot_alpha * (ev - ev0) / dt
    b = (p - p_old) / (mat.biot_M * dt)
    Mt, Kp = M @ (a + b), KK @ p
    Rt = -(Mt + Kp + src)
    dof, ptr, master, weight = constraints_p(P)
    add = np.zeros_like(Rt)
    for i, h in enumerate(dof):                                         # C^T: the hanging rows folded into their masters, then zero
        for k in range(ptr[i], ptr[i + 1]):
            add[master[k]] += weight[k] * Rt[h]
    Rt = Rt + add
    Rt[dof] = 0.0
    pd = prescribed_dofs_p(P)
    mask = np.zeros(len(Rt), dtype=bool); mask[pd] = True
    terms = dict(storage_rate_strain=float(m @ a), storage_rate_pressure=float(m @ b), source_sum=float(src.sum()), outflow_prescribed=float(Rt[mask].sum()),
                 free_row_sum=float(Rt[~mask].sum()), residual_l2=float(np.sqrt((Rt[~mask] ** 2).sum())))
    scale = float(np.abs(Mt).sum() + np.abs(Kp).sum() + np.abs(src).sum())
    scales = dict(storage_rate_strain=float(np.abs(m * a).sum()), storage_rate_pressure=float(np.abs(m * b).sum()), source_sum=float(np.abs(src).sum()),
                  outflow_prescribed=scale, free_row_sum=scale, residual_l2=scale)
    return dict(terms=terms, Rt=Rt, prescribed=pd, scale=scale, scales=scales)

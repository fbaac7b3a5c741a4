"""Plain fp64 NumPy reference of the mechanical post-processing (include/poroel_hip.h: cell stresses, failure measures, force balance) on any MappingQ1 mesh, from the
descriptor's geometry, dof lists, boundary-face list and constraint list alone; poro_desc.fe is never read.  Its own gradients at the cell centre (the full tensor
basis from its own Lagrange polynomials, every dof of the cell), its own stresses, principal values by numpy.linalg.eigvalsh, and for the force balance its own
A_full (Gauss(k+1), per-cell moduli), coupling, traction and body-force vectors, C^T and component table.  Helper module of the test-suite, not collected.

  cell_stress(P, u, p, lam, G, alpha)        (strain, effective, total), packed [n_cells][n_sym]; p None: total = effective
  full_tensor(packed, dim, zz=None)          [n][3][3]; 2D: the in-plane block plus zz (plane strain)
  measures(P, strain, eff, lam, c, phi)      [n_cells][6]: s1 >= s2 >= s3, mean, von Mises, f
  nodal_mean_stress(P, strain, lam, G)       the OLD rule on cell data: lambda, G replaced by the mean over the cells that share a vertex with the cell (for the interface check)
  force_balance(P, u, p, lam, G, alpha, g, rho)  dict: terms, Rt, deficit, scales, parts
lam, G, rho: one scalar or one value per cell."""
import numpy as np

from general_reference import cell_vertices, q1_at, rule_1d, vertices

PAIRS = {2: [(0, 0), (0, 1), (1, 1)], 3: [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]}


def arrays(P):
    d = P.desc
    dim, k = d.dim, d.degree_u
    X = getattr(P, "coords", None)
    X = vertices(P) if X is None else np.asarray(X)
    cv = cell_vertices(d)
    cdu = np.ctypeslib.as_array(d.cell_dofs_u, shape=(d.n_cells, (k + 1) ** dim * dim)).copy()
    cdp = np.ctypeslib.as_array(d.cell_dofs_p, shape=(d.n_cells, 1 << dim)).copy()
    return d, dim, k, X, cv, cdu, cdp


def per_cell(v, n):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy()


def physical_gradients(dim, k, Xc, xi):
    """d phi_s / d x_d [e][q][s][d] and det J [e][q] of the cells with vertices Xc [e][v][r] at the reference points xi [q][dim] (any points: no tensor structure is used)"""
    out = []
    for pt in np.atleast_2d(xi):
        val = np.ones(((k + 1) ** dim,)); grad = np.ones(((k + 1) ** dim, dim))
        nodes = np.arange(k + 1) / k
        si = np.array(list(np.ndindex(*([k + 1] * dim))))[:, ::-1]
        for a in range(dim):
            for s, idx in enumerate(si):
                i = idx[a]
                v = np.prod([(pt[a] - nodes[m]) / (nodes[i] - nodes[m]) for m in range(k + 1) if m != i])
                dv = sum(np.prod([(pt[a] - nodes[n]) / (nodes[i] - nodes[n]) for n in range(k + 1) if n not in (i, m)]) / (nodes[i] - nodes[m]) for m in range(k + 1) if m != i)
                val[s] *= v
                for b in range(dim):
                    grad[s, b] *= dv if a == b else v
        out.append((val, grad))
    phi = np.array([o[0] for o in out]); dphi = np.array([o[1] for o in out])             # [q][s], [q][s][b]
    N, dN = q1_at(dim, np.atleast_2d(xi))
    J = np.einsum("evr,qvb->eqrb", Xc, dN)
    Ji = np.linalg.inv(J)                                                                   # [b][d] = d xi_b / d x_d
    return phi, np.einsum("eqbd,qsb->eqsd", Ji, dphi), np.linalg.det(J), N


def pack(T, dim):
    return np.stack([T[:, a, b] for a, b in PAIRS[dim]], axis=1)


def cell_stress(P, u, p, lam, G, alpha):
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    nc = d.n_cells
    lam, G = per_cell(lam, nc), per_cell(G, nc)
    _, Gr, _, N = physical_gradients(dim, k, X[cv], np.full((1, dim), 0.5))
    ue = np.asarray(u)[cdu].reshape(nc, -1, dim)                                           # [e][s][c]
    g = np.einsum("esc,esd->ecd", ue, Gr[:, 0])                                            # d u_c / d x_d
    eps = 0.5 * (g + g.transpose(0, 2, 1))
    tr = np.trace(eps, axis1=1, axis2=2)
    I = np.eye(dim)[None]
    eff = lam[:, None, None] * tr[:, None, None] * I + 2.0 * G[:, None, None] * eps
    tot = eff.copy()
    if p is not None:
        pc = np.asarray(p)[cdp] @ N[0]
        tot = eff - alpha * pc[:, None, None] * I
    return pack(eps, dim), pack(eff, dim), pack(tot, dim)


def full_tensor(packed, dim, zz=None):
    n = len(packed)
    T = np.zeros((n, 3, 3))
    for i, (a, b) in enumerate(PAIRS[dim]):
        T[:, a, b] = packed[:, i]; T[:, b, a] = packed[:, i]
    if dim == 2:
        T[:, 2, 2] = zz
    return T


def measures_of(T, cohesion=None, phi=None):
    """[n][6] from full 3 x 3 tensors: eigvalsh descending, mean, von Mises from the deviator's norm, f"""
    ev = np.linalg.eigvalsh(T)[:, ::-1]
    mean = np.trace(T, axis1=1, axis2=2) / 3.0
    dev = T - mean[:, None, None] * np.eye(3)[None]
    vm = np.sqrt(1.5 * np.einsum("nab,nab->n", dev, dev))
    f = np.zeros(len(T)) if cohesion is None else 0.5 * (ev[:, 0] - ev[:, 2]) + 0.5 * (ev[:, 0] + ev[:, 2]) * np.sin(phi) - cohesion * np.cos(phi)
    return np.column_stack([ev, mean, vm, f])


def measures(P, strain, eff, lam, cohesion=None, phi=None):
    dim = P.desc.dim
    zz = per_cell(lam, P.desc.n_cells) * (strain[:, 0] + strain[:, 2]) if dim == 2 else None
    return measures_of(full_tensor(eff, dim, zz), cohesion, phi)


def nodal_mean_moduli(P, lam, G):
    """per cell the mean over its vertices of the nodal means (mean over the cells touching the vertex) of lambda and G: what a product of nodal constants sees"""
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    nc = d.n_cells
    lam, G = per_cell(lam, nc), per_cell(G, nc)
    cnt = np.zeros(d.n_dofs_p); sl = np.zeros(d.n_dofs_p); sg = np.zeros(d.n_dofs_p)
    np.add.at(cnt, cdp.ravel(), 1.0); np.add.at(sl, cdp.ravel(), np.repeat(lam, 1 << dim)); np.add.at(sg, cdp.ravel(), np.repeat(G, 1 << dim))
    return (sl / cnt)[cdp].mean(axis=1), (sg / cnt)[cdp].mean(axis=1)


def constraints_u(P):
    c = P.desc.cons_u
    n = c.n
    if not n:
        return np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)
    ptr = np.ctypeslib.as_array(c.ptr, shape=(n + 1,)).copy()
    nm = int(ptr[n])
    return (np.ctypeslib.as_array(c.dof, shape=(n,)).copy(), ptr, np.ctypeslib.as_array(c.master, shape=(nm,)).copy() if nm else np.zeros(0, np.int32),
            np.ctypeslib.as_array(c.weight, shape=(nm,)).copy() if nm else np.zeros(0))


def dirichlet_dofs(P):
    d = P.desc
    return np.ctypeslib.as_array(d.dirichlet_dof, shape=(d.n_dirichlet,)).copy() if d.n_dirichlet else np.zeros(0, np.int32)


def component_table(P):
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    comp = np.full(d.n_dofs_u, -1)
    for c in range(dim):
        comp[cdu[:, c::dim].ravel()] = c
    assert comp.min() >= 0
    return comp


def _volume_points(dim, k):
    t1, w1 = rule_1d(k + 1)
    qi = np.array(list(np.ndindex(*([k + 1] * dim))))[:, ::-1]
    return t1[qi], np.prod(w1[qi], axis=1)


def stiffness_apply(P, u, lam, G, absolute=False):
    """A_full u, A_full the unconstrained operator sum_c int_c (lambda_c tr eps(u) I + 2 G_c eps(u)) : grad phi_i with Gauss(k+1); absolute: sum_j |A_ij| |u_j|"""
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    nc = d.n_cells
    lam, G = per_cell(lam, nc), per_cell(G, nc)
    xi, w = _volume_points(dim, k)
    _, Gr, det, _ = physical_gradients(dim, k, X[cv], xi)
    jxw = det * w
    # element matrix K[(s,c),(t,e)] = int lam d_c phi_s d_e phi_t + G (delta_ce grad phi_s . grad phi_t + d_e phi_s d_c phi_t)
    K = (np.einsum("n,nqsc,nqte,nq->nscte", lam, Gr, Gr, jxw) + np.einsum("n,nqse,nqtc,nq->nscte", G, Gr, Gr, jxw)
         + np.einsum("n,nqsd,nqtd,nq,ce->nscte", G, Gr, Gr, jxw, np.eye(dim)))
    ns = Gr.shape[2]
    K = K.reshape(nc, ns * dim, ns * dim)
    ue = np.asarray(u)[cdu]
    ye = np.einsum("nij,nj->ni", np.abs(K), np.abs(ue)) if absolute else np.einsum("nij,nj->ni", K, ue)
    y = np.zeros(d.n_dofs_u)
    np.add.at(y, cdu.ravel(), ye.ravel())
    return y


def coupling_vector(P, p, alpha):
    """b_cpl,i = alpha int p_h div(phi_i), Gauss(k+1)"""
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    xi, w = _volume_points(dim, k)
    _, Gr, det, N = physical_gradients(dim, k, X[cv], xi)
    ph = np.einsum("nv,qv->nq", np.asarray(p)[cdp], N)
    be = alpha * np.einsum("nq,nqsc,nq->nsc", ph, Gr, det * w)
    b = np.zeros(d.n_dofs_u)
    np.add.at(b, cdu.ravel(), be.reshape(d.n_cells, -1).ravel())
    return b


def body_vector(P, g, rho):
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    xi, w = _volume_points(dim, k)
    phi, _, det, _ = physical_gradients(dim, k, X[cv], xi)
    integ = np.einsum("nq,qs->ns", det * w, phi) * per_cell(rho, d.n_cells)[:, None]
    be = integ[:, :, None] * np.asarray(g, dtype=np.float64)[None, None, :dim]
    b = np.zeros(d.n_dofs_u)
    np.add.at(b, cdu.ravel(), be.reshape(d.n_cells, -1).ravel())
    return b


def traction_vector(P):
    """b_neu: for every condition (label, component ci, value) and face of that label int_F phi_i value n_ci dS on component ci, Gauss(k+1) on the face, n the outward unit
    normal (from the cross product of the face's tangents, oriented by the direction that leaves the cell)"""
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    b = np.zeros(d.n_dofs_u)
    if not d.n_neumann or not d.n_bfaces:
        return b
    lab = np.ctypeslib.as_array(d.neumann_label, shape=(d.n_neumann,)); cmp_ = np.ctypeslib.as_array(d.neumann_component, shape=(d.n_neumann,))
    val = np.ctypeslib.as_array(d.neumann_value, shape=(d.n_neumann,))
    bc, bl, bid = (np.ctypeslib.as_array(a, shape=(d.n_bfaces,)) for a in (d.bface_cell, d.bface_local, d.bface_id))
    t1, w1 = rule_1d(k + 1)
    for f in range(2 * dim):
        dn, side = f >> 1, f & 1
        tang = [a for a in range(dim) if a != dn]
        for l in range(d.n_neumann):
            sel = np.nonzero((bl == f) & (bid == lab[l]))[0]
            if not sel.size:
                continue
            cells = bc[sel]
            for q in np.ndindex(*([k + 1] * (dim - 1))):
                xi = np.empty(dim); xi[dn] = float(side); wq = 1.0
                for a, i in zip(tang, q):
                    xi[a] = t1[i]; wq *= w1[i]
                phi, _, _, _ = physical_gradients(dim, k, X[cv[cells]], xi[None])
                _, dN = q1_at(dim, xi[None])
                J = np.einsum("evr,vb->erb", X[cv[cells]], dN[0])
                if dim == 2:
                    T = J[:, :, tang[0]]; Nn = np.stack([T[:, 1], -T[:, 0]], axis=1)
                else:
                    Nn = np.cross(J[:, :, tang[0]], J[:, :, tang[1]])
                s = np.sign(np.einsum("er,er->e", Nn, J[:, :, dn] * (1.0 if side else -1.0)))
                Nn = Nn * s[:, None]                                                       # n dS, outward
                add = val[l] * wq * Nn[:, cmp_[l]][:, None] * phi[0][None, :]             # [e][s]
                np.add.at(b, cdu[cells][:, cmp_[l]::dim].ravel(), add.ravel())
    return b


def condense(P, r):
    """(C^T r, deficit): hanging rows folded into their masters and zeroed; deficit[h] = (1 - sum of the row's weights) r_h, what the closed list no longer carries"""
    dof, ptr, master, weight = constraints_u(P)
    Rt = np.array(r, dtype=np.float64)
    deficit = np.zeros_like(Rt)
    add = np.zeros_like(Rt)
    for i, h in enumerate(dof):
        ws = 0.0
        for kk in range(ptr[i], ptr[i + 1]):
            add[master[kk]] += weight[kk] * r[h]; ws += weight[kk]
        deficit[h] = (1.0 - ws) * r[h]
    Rt += add
    Rt[dof] = 0.0
    return Rt, deficit


def force_balance(P, u, p, lam, G, alpha, g=None, rho=0.0):
    d = P.desc
    dim = d.dim
    comp = component_table(P)
    Au = stiffness_apply(P, u, lam, G)
    cpl, neu = coupling_vector(P, p, alpha), traction_vector(P)
    body = body_vector(P, g, rho) if g is not None and np.any(np.asarray(g)) else np.zeros(d.n_dofs_u)
    r = Au - (cpl + neu + body)
    Rt, deficit = condense(P, r)
    dd = dirichlet_dofs(P)
    mask = np.zeros(d.n_dofs_u, dtype=bool); mask[dd] = True
    absr = stiffness_apply(P, u, lam, G, absolute=True) + np.abs(cpl) + np.abs(neu) + np.abs(body)     # the summands behind every row of r
    terms, scales = {}, {}
    for name, vec_, sc in (("traction_sum", neu, np.abs(neu)), ("body_sum", body, np.abs(body)), ("coupling_sum", cpl, np.abs(cpl))):
        terms[name] = np.array([vec_[comp == c].sum() for c in range(dim)])
        scales[name] = np.array([sc[comp == c].sum() for c in range(dim)])
    terms["reaction_sum"] = np.array([Rt[mask & (comp == c)].sum() + deficit[comp == c].sum() for c in range(dim)])
    terms["free_row_sum"] = np.array([Rt[~mask & (comp == c)].sum() for c in range(dim)])
    terms["residual_l2"] = float(np.sqrt((Rt[~mask] ** 2).sum()))
    total = np.array([absr[comp == c].sum() for c in range(dim)])
    scales["reaction_sum"] = scales["free_row_sum"] = total
    scales["residual_l2"] = float(absr.sum())
    return dict(terms=terms, scales=scales, Rt=Rt, deficit=deficit, dirichlet=dd, comp=comp, total=total, parts=dict(Au=Au, cpl=cpl, neu=neu, body=body))

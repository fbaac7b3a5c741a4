"""Mesh adaptation, host layer (refine_mesh, PoroelasticityFSS.h:447-498), no GPU: mask-driven refined boxes, the fixed-fraction marking with the level
limits of one refinement level, and the rows that carry a pressure-space function from one refined box to the next."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, BC_3D, material
from test_constraints_cpu import MESHES, cons_arrays


def bc_of(dim):
    return BC_2D if dim == 2 else BC_3D


def masked(dim, n, deg, mask, bc=None):
    return pk.Problem.refined_box_mask(dim, n, [10.0] * dim, deg, material(), bc if bc is not None else bc_of(dim), mask)


def block_mask(n, lo, hi):
    n3, lo3, hi3 = list(n) + [1] * (3 - len(n)), list(lo) + [0] * (3 - len(lo)), list(hi) + [1] * (3 - len(hi))
    m = np.zeros(n3[::-1], dtype=np.int32)             # [z][y][x]
    m[lo3[2]:hi3[2], lo3[1]:hi3[1], lo3[0]:hi3[0]] = 1
    return m.reshape(-1)


def l_mask(n):
    """an L: the first column of coarse cells in x and the first row in y (all z)"""
    n3 = list(n) + [1] * (3 - len(n))
    m = np.zeros(n3[::-1], dtype=np.int32)
    m[:, :, 0] = 1; m[:, 0, :] = 1
    return m.reshape(-1)


def checker_mask(n):
    """refined where i + j + k is even: in 3D refined and unrefined cells also meet along edges only"""
    n3 = list(n) + [1] * (3 - len(n))
    k, j, i = np.meshgrid(np.arange(n3[2]), np.arange(n3[1]), np.arange(n3[0]), indexing="ij")
    return ((i + j + k) % 2 == 0).astype(np.int32).reshape(-1)


def desc_arrays(P):
    """every array of the descriptor a refined box fills, by name"""
    d = P.desc; dim = d.dim; nv = 2 ** dim; ns = (d.degree_u + 1) ** dim
    out = {"counts": np.array([d.n_cells, d.n_vertices, d.n_dofs_u, d.n_dofs_p, d.n_bfaces, d.n_dirichlet, d.box.enabled, d.coarse.enabled])}
    out["vertex_coords"] = P.array("vertex_coords", (d.n_vertices, dim))
    out["cell_vertices"] = P.array("cell_vertices", (d.n_cells, nv), np.int32)
    out["cell_dofs_u"] = P.array("cell_dofs_u", (d.n_cells, ns * dim), np.int32)
    out["cell_dofs_p"] = P.array("cell_dofs_p", (d.n_cells, nv), np.int32)
    for name in ("bface_cell", "bface_local", "bface_id"):
        out[name] = P.array(name, (d.n_bfaces,), np.int32)
    out["dirichlet_dof"] = P.array("dirichlet_dof", (d.n_dirichlet,), np.int32); out["dirichlet_value"] = P.array("dirichlet_value", (d.n_dirichlet,))
    for nm, c in (("cons_u", d.cons_u), ("cons_p", d.cons_p)):
        for k, a in zip(("dof", "ptr", "master", "weight", "inhom"), cons_arrays(c)):
            out[nm + "." + k] = a
    for suffix, rows in (("", d.n_dofs_u // dim), ("_p", d.n_dofs_p)):
        ptr = np.ctypeslib.as_array(getattr(d.coarse, "ptr" + suffix), shape=(rows + 1,)).copy(); nnz = int(ptr[-1])
        out["coarse.ptr" + suffix] = ptr
        out["coarse.node" + suffix] = np.ctypeslib.as_array(getattr(d.coarse, "node" + suffix), shape=(nnz,)).copy()
        out["coarse.weight" + suffix] = np.ctypeslib.as_array(getattr(d.coarse, "weight" + suffix), shape=(nnz,)).copy()
    return out


# ---- 1. mask = block ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,deg,lo,hi", MESHES, ids=str)
def test_block_mask_gives_the_block_form(dim, n, deg, lo, hi):
    A = pk.Problem.refined_box(dim, n, [10.0] * dim, deg, material(), bc_of(dim), lo, hi)
    B = masked(dim, n, deg, block_mask(n, lo, hi))
    try:
        a, b = desc_arrays(A), desc_arrays(B)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        assert np.array_equal(A.refine_mask(), block_mask(n, lo, hi)) and np.array_equal(B.refine_mask(), block_mask(n, lo, hi))
        for x, y in zip(A.cell_parents(), B.cell_parents()):
            assert np.array_equal(x, y)
    finally:
        A.close(); B.close()


# ---- 2. masks that are no block ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("dim,n", [(2, (4, 3)), (3, (3, 3, 2))], ids=str)
@pytest.mark.parametrize("shape", ["L", "checker"])
def test_hanging_nodes_of_general_masks(shape, dim, n, deg):
    mask = l_mask(n) if shape == "L" else checker_mask(n)
    P = masked(dim, n, deg, mask, bc=[])
    try:
        d = P.desc; nv = 2 ** dim
        assert d.n_cells == int((mask == 0).sum() + nv * (mask != 0).sum()) and d.box.enabled == 0 and d.coarse.enabled == 1
        coarse, child = P.cell_parents()
        assert np.array_equal(np.bincount(coarse, minlength=mask.size), np.where(mask != 0, nv, 1)) and np.all((child >= 0) == (mask[coarse] != 0))
        Xp = P.array("vertex_coords", (d.n_vertices, dim))
        # displacement nodes: the Q1 map of the lexicographic reference nodes of every cell
        k = deg; n1 = k + 1; ns = n1 ** dim
        cv = P.array("cell_vertices", (d.n_cells, nv), np.int32); cd = P.array("cell_dofs_u", (d.n_cells, ns * dim), np.int32)
        Xu = np.full((d.n_dofs_u // dim, dim), np.nan)
        for c in range(d.n_cells):
            x0, x1 = Xp[cv[c, 0]], Xp[cv[c, nv - 1]]
            for s in range(ns):
                Xu[cd[c, s * dim] // dim] = x0 + (x1 - x0) * np.array([s % n1, (s // n1) % n1, s // (n1 * n1)][:dim]) / k
        assert not np.isnan(Xu).any()
        lin = lambda X: 0.3 + X @ np.array([1.0, -2.0, 0.7][:dim])
        for c, X, ncomp in ((d.cons_p, Xp, 1), (d.cons_u, Xu, dim)):
            dof, ptr, m, w, inh = cons_arrays(c)
            assert c.n > 0 and len(set(dof)) == len(dof) and not set(dof) & set(m) and np.all(inh == 0)     # no master is itself constrained
            scale = np.abs(lin(X)).max()
            for i in range(c.n):
                ws, ms = w[ptr[i]:ptr[i + 1]], m[ptr[i]:ptr[i + 1]]
                assert abs(ws.sum() - 1) <= 1e-13
                assert abs(ws @ lin(X[ms // ncomp]) - lin(X[dof[i] // ncomp])) <= 1e-13 * scale
        # which vertices hang, independently: a vertex off the coarse lattice hangs exactly when one of the coarse cells whose closure contains it is unrefined - whatever the
        # contact (on the 3D checkerboard the four cells around a coarse edge alternate, and a refined cell meets its diagonal neighbour along that edge only)
        n3 = np.array(list(n) + [1] * (3 - dim)); m3 = mask.reshape(n3[::-1])
        lat = np.rint((Xp + 5.0) / (10.0 / np.array(n) / 2)).astype(int)
        want = set()
        for v, L in enumerate(lat):
            if np.all(L % 2 == 0):
                continue
            rng = [range(max(q // 2 - (1 if q % 2 == 0 else 0), 0), min(q // 2, n3[a] - 1) + 1) for a, q in enumerate(L)] + [range(1)] * (3 - dim)
            if any(m3[k, j, i] == 0 for i in rng[0] for j in rng[1] for k in rng[2]):
                want.add(v)
        assert want == set(cons_arrays(d.cons_p)[0].tolist())
    finally:
        P.close()


def test_edge_only_contact_3d():
    """3D: a refined and an unrefined cell that share ONLY an edge (the other two cells around it are refined).  The edge's midpoint hangs on the unrefined cell's edge
    with weights 1/2, 1/2."""
    n = (2, 2, 1)
    mask = np.array([1, 1, 1, 0], dtype=np.int32)     # cells (0,0), (1,0), (0,1) refined; (1,1) meets (0,0) along the z edge through the middle only
    P = masked(3, n, 1, mask, bc=[])
    try:
        d = P.desc
        X = P.array("vertex_coords", (d.n_vertices, 3))
        mid = np.nonzero(np.all(np.abs(X - np.array([0.0, 0.0, 0.0])) < 1e-12, axis=1))[0]      # midpoint of the central edge x = y = 0, z in [-5, 5]
        assert len(mid) == 1
        dof, ptr, m, w, _ = cons_arrays(d.cons_p)
        i = np.nonzero(dof == mid[0])[0]
        assert len(i) == 1
        ms, ws = m[ptr[i[0]]:ptr[i[0] + 1]], w[ptr[i[0]]:ptr[i[0] + 1]]
        assert np.allclose(ws, [0.5, 0.5]) and np.allclose(np.sort(X[ms][:, 2]), [-5.0, 5.0]) and np.allclose(X[ms][:, :2], 0.0)
    finally:
        P.close()


def test_all_zero_mask_is_the_uniform_box_as_a_general_mesh():
    P = masked(2, (3, 2), 2, np.zeros(6)); B = pk.Problem.box(2, (3, 2), [10.0, 10.0], 2, material(), BC_2D)
    try:
        d, b = P.desc, B.desc
        assert d.box.enabled == 0 and d.coarse.enabled == 1 and d.cons_u.n == 0 and d.cons_p.n == 0
        assert (d.n_cells, d.n_dofs_u, d.n_dofs_p) == (b.n_cells, b.n_dofs_u, b.n_dofs_p)
        assert np.array_equal(np.sort(P.array("vertex_coords", (d.n_vertices, 2)), axis=0), np.sort(B.array("vertex_coords", (b.n_vertices, 2)), axis=0))
        with pytest.raises(ValueError):
            masked(2, (3, 2), 2, np.zeros(5))
        with pytest.raises(RuntimeError):
            B.refine_mask()
    finally:
        P.close(); B.close()


# ---- 3. marking ---------------------------------------------------------------------------------------------------------------------------------
def mark_numpy(eta, old_mask, coarse, child, nchild, rf, cf):
    """The rule, restated.  Cells sorted by eta descending: the refine set is the shortest prefix whose running sum of eta reaches rf * sum(eta), plus every cell tied with
    its last member.  The coarsen set is the same from the ascending end with cf, minus the refine set.  All-zero eta (or a zero target) flags nothing.  One level: a refine
    flag on a child and a coarsen flag on a box cell are dropped; a refined coarse cell is coarsened only when all its children are flagged."""
    eta = np.asarray(eta, dtype=float); n = eta.size

    def cut(sorted_eta, frac):
        run = np.concatenate([[0.0], np.cumsum(sorted_eta)])        # running sums in the sorted order; run[m] = sum of the first m
        m = int(np.argmax(run >= frac * run[-1]))                    # the shortest prefix (m = 0: nothing)
        return None if m == 0 else sorted_eta[m - 1]
    t = cut(np.sort(eta)[::-1], rf)
    refine = np.zeros(n, bool) if t is None else eta >= t
    t = cut(np.sort(eta), cf)
    coarsen = np.zeros(n, bool) if t is None else (eta <= t) & ~refine
    new = np.array(old_mask, dtype=np.int32).copy()
    for c in range(new.size):
        cells = np.nonzero(coarse == c)[0]
        if old_mask[c]:
            assert len(cells) == nchild and np.all(child[cells] >= 0)
            if coarsen[cells].all():
                new[c] = 0
        else:
            assert len(cells) == 1 and child[cells[0]] == -1
            if refine[cells[0]]:
                new[c] = 1
    return new


def check_marking(P, eta, rf=0.6, cf=0.4):
    coarse, child = P.cell_parents()
    want = mark_numpy(eta, P.refine_mask(), coarse, child, 2 ** P.desc.dim, rf, cf)
    got = P.mark_fixed_fraction(eta, rf, cf)
    assert np.array_equal(got, want), (got, want)
    return got


@pytest.mark.parametrize("dim,n,lo,hi", [(2, (4, 4), (1, 1), (3, 3)), (3, (3, 3, 2), (0, 1, 0), (2, 3, 1))], ids=str)
def test_marking_random(dim, n, lo, hi):
    P = masked(dim, n, 1, block_mask(n, lo, hi))
    try:
        rng = np.random.default_rng(11 + dim)
        changed = 0
        for trial in range(20):
            eta = rng.random(P.desc.n_cells) ** 3
            if trial % 4 == 1:
                eta[rng.random(eta.size) < 0.3] = 0.0                 # many zeros at the ascending end
            if trial % 4 == 2:
                eta = np.round(eta * 4) / 4                           # many ties
            rf, cf = (0.6, 0.4) if trial % 2 == 0 else (float(rng.random()), float(rng.random()))
            changed += int(not np.array_equal(check_marking(P, eta, rf, cf), P.refine_mask()))
        assert changed > 10
        with pytest.raises(ValueError):
            P.mark_fixed_fraction(np.ones(3))
        with pytest.raises(RuntimeError):
            P.mark_fixed_fraction(-np.ones(P.desc.n_cells))
    finally:
        P.close()


def test_marking_hand_made_cases():
    n = (3, 2); old = np.array([0, 1, 0, 0, 0, 0], dtype=np.int32)     # coarse cell 1 refined: cells = [c0, c1.0, c1.1, c1.2, c1.3, c2, c3, c4, c5]
    P = masked(2, n, 1, old)
    try:
        coarse, child = P.cell_parents()
        assert list(coarse) == [0, 1, 1, 1, 1, 2, 3, 4, 5] and list(child) == [-1, 0, 1, 2, 3, -1, -1, -1, -1]
        z = np.zeros(9)
        # all-zero eta flags nothing
        assert np.array_equal(check_marking(P, z), old)
        # a tie at the refine threshold: 0.6 * 10 = 6 is reached after [4, 3] (sum 7); the second cell with eta = 3 is tied with the last member and refined too
        eta = z.copy(); eta[[0, 5, 6, 7]] = [4, 3, 3, 0]; eta[1:5] = 0
        got = check_marking(P, eta, 0.6, 0.0)
        assert list(got) == [1, 1, 1, 1, 0, 0]
        # a parent with 2^dim - 1 children flagged for coarsening stays refined ...
        eta = np.array([9.0, 0.1, 0.1, 0.1, 5.0, 9.0, 9.0, 9.0, 9.0])
        got = check_marking(P, eta, 0.0, 0.25 / eta.sum())                 # the running sum reaches 0.25 with the third 0.1: coarsen set = those three
        assert list(got) == list(old)
        # ... and is coarsened with all of them flagged
        eta[4] = 0.1
        got = check_marking(P, eta, 0.0, 0.35 / eta.sum())
        assert list(got) == [0, 0, 0, 0, 0, 0]
        # a refine flag on a child is dropped (maximum level), on box cells it refines; a coarsen flag on a box cell is dropped
        eta = np.array([1.0, 50.0, 0.2, 0.2, 0.2, 40.0, 0.05, 1.0, 1.0])
        got = check_marking(P, eta, 0.9, 0.001)
        assert list(got) == [0, 1, 1, 0, 0, 0]
    finally:
        P.close()


# ---- 4. transfer rows ---------------------------------------------------------------------------------------------------------------------------
def overlapping_masks(n):
    """A and B over the same box: one region newly refined in B, one kept, one coarsened"""
    n3 = list(n) + [1] * (3 - len(n))
    a = np.zeros(n3[::-1], dtype=np.int32); b = a.copy()
    a[:, :2, :2] = 1                       # A: the lower left 2 x 2 columns
    b[:, :2, 1:3] = 1                      # B: shifted by one in x: column 0 coarsened, column 1 kept, column 2 new
    return a.reshape(-1), b.reshape(-1)


def conforming(P, f):
    """nodal values of f at the vertices, hanging values from the constraints (so that the function is in the FE space)"""
    d = P.desc; X = P.array("vertex_coords", (d.n_vertices, d.dim))
    v = f(X)
    dof, ptr, m, w, _ = cons_arrays(d.cons_p)
    for i in range(len(dof)):
        v[dof[i]] = w[ptr[i]:ptr[i + 1]] @ v[m[ptr[i]:ptr[i + 1]]]
    return v


@pytest.mark.parametrize("dim,n", [(2, (4, 3)), (3, (3, 3, 2))], ids=str)
def test_transfer_rows(dim, n):
    ma, mb = overlapping_masks(n)
    zero = np.zeros_like(ma)
    f = (lambda X: 1.0 + 0.5 * X[:, 0] - 0.25 * X[:, 1] + 0.125 * X[:, 0] * X[:, 1]) if dim == 2 else \
        (lambda X: 1.0 + 0.5 * X[:, 0] - 0.25 * X[:, 1] + 0.3 * X[:, 2] + 0.125 * X[:, 0] * X[:, 1] * X[:, 2] - 0.2 * X[:, 1] * X[:, 2])
    box, A, B, Z = masked(dim, n, 1, zero), masked(dim, n, 1, ma), masked(dim, n, 1, mb), masked(dim, n, 1, zero)
    try:
        for old, new in ((box, A), (A, B), (B, Z)):
            ptr, node, w = old.transfer_rows_p(new)
            do, dn = old.desc, new.desc
            assert ptr[0] == 0 and len(ptr) == dn.n_dofs_p + 1 and np.all(np.diff(ptr) >= 1) and node.min() >= 0 and node.max() < do.n_dofs_p
            Xo, Xn = old.array("vertex_coords", (do.n_vertices, dim)), new.array("vertex_coords", (dn.n_vertices, dim))
            v_old = conforming(old, f)
            got = np.array([w[ptr[i]:ptr[i + 1]] @ v_old[node[ptr[i]:ptr[i + 1]]] for i in range(dn.n_dofs_p)])
            # f is multilinear in the coordinates, so it lies in the Q1 space of every mesh over the box: the old FE function IS f, at every point
            assert np.abs(got - f(Xn)).max() <= 1e-13 * np.abs(f(Xn)).max()
            for i in range(dn.n_dofs_p):
                ws, nd = w[ptr[i]:ptr[i + 1]], node[ptr[i]:ptr[i + 1]]
                assert abs(ws.sum() - 1) <= 1e-14 and np.all(np.diff(nd) > 0) and np.all(np.abs(ws) > 1e-13)
                same = np.nonzero(np.all(np.abs(Xo - Xn[i]) < 1e-9, axis=1))[0]
                if len(same):                                           # a vertex of both meshes: exactly one entry, weight 1
                    assert len(nd) == 1 and nd[0] == same[0] and ws[0] == 1.0
                else:
                    assert len(nd) in (2, 4, 8)[:dim]
        with pytest.raises(RuntimeError):
            P2 = masked(dim, [m + 1 for m in n], 1, np.zeros(int(np.prod([m + 1 for m in n]))))
            try:
                A.transfer_rows_p(P2)
            finally:
                P2.close()
        U = pk.Problem.box(dim, n, [10.0] * dim, 1, material(), bc_of(dim))
        try:
            with pytest.raises(RuntimeError):
                U.transfer_rows_p(A)
        finally:
            U.close()
    finally:
        for P in (box, A, B, Z):
            P.close()


# ---- the face tables of the Kelly indicator, without a GPU ----------------------------------------------------------------------------------------------
def eta_from_tables(P, p):
    """what the two kernels compute from the face tables (csrc/kernels_kelly.hip), in NumPy: cofactor normal, side B's points from the packed reference coordinates"""
    from test_kelly_gpu import G2, cell_diameters, grad_phys, q1
    d = P.desc; dim = d.dim; nv = 2 ** dim; nfv = nv // 2
    Xc = P.array("vertex_coords", (d.n_vertices, dim))[P.array("cell_vertices", (d.n_cells, nv), np.int32)]
    pc = np.asarray(p)[P.array("cell_dofs_p", (d.n_cells, nv), np.int32)]
    T = P.kelly_tables()
    assert np.all(np.diff(T["cell_a"]) >= 0)                                   # sorted by the first cell
    jump = np.zeros(len(T["cell_a"]))
    for i, (a, b, code) in enumerate(zip(T["cell_a"], T["cell_b"], T["code"])):
        fa = code & 7; da, side = fa >> 1, fa & 1; tang = [k for k in range(dim) if k != da]
        ref_b = np.array([[0.5 * ((code >> (3 + 2 * (3 * j + k))) & 3) for k in range(dim)] for j in range(nfv)])
        for q in range(nfv):
            st = [G2[q & 1], G2[q >> 1]]
            xa = np.zeros(dim); xa[da] = side
            for k, v in zip(tang, st):
                xa[k] = v
            nf = [((st[0] if j & 1 else 1 - st[0]) * ((st[1] if j >> 1 else 1 - st[1]) if dim == 3 else 1.0)) for j in range(nfv)]
            xb = np.array(nf) @ ref_b
            J = Xc[a].T @ q1(dim, xa)[1]
            N = (np.linalg.det(J) * np.linalg.inv(J).T)[:, da]
            jn = N @ (grad_phys(dim, Xc[a], pc[a], xa) - grad_phys(dim, Xc[b], pc[b], xb))
            jump[i] += jn * jn / np.linalg.norm(N) / nfv
    diam = cell_diameters(P); eta2 = np.zeros(d.n_cells)
    for c in range(d.n_cells):
        for e in range(T["ent_ptr"][c], T["ent_ptr"][c + 1]):
            eta2[c] += diam[T["ent_hcell"][e]] / 24 * jump[T["ent_face"][e]]
    return np.sqrt(eta2), T


@pytest.mark.parametrize("name", ["box2d", "box3d", "refined0", "refined1", "refined2", "refined3", "lmask3d", "gmsh"])
def test_kelly_face_tables_against_the_model(name):
    """the host half of poro_pres_estimate_error: the tables (regular faces by vertex tuple, hanging pairs through cons_p) give what the model finds by coordinates"""
    import test_kelly_gpu as tk
    p, want, info = tk.model_case(name)
    P = tk.make(name)
    try:
        got, T = eta_from_tables(P, p)
        assert len(T["cell_a"]) == info["regular"] + info["sub"] and len(T["ent_face"]) == 2 * len(T["cell_a"])
        assert np.abs(got - want).max() <= 1e-12 * want.max()
    finally:
        P.close()

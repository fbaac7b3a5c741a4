"""Plain fp64 NumPy reference of the displacement operator with PER-CELL Lame lambda and shear modulus G.  Helper module of the test-suite, not collected.

ModuliReference    general_reference.GeneralReference with one (lambda, G) per cell in the descriptor's cell order: apply_full / diag_full overridden, everything else
                   (its own quadrature, basis and MappingQ1; the conventions of apply_A) inherited.
assemble()         A_u as scipy CSR in the convention of apply_A and of PORO_MAT_A_U: free rows without the constrained columns, a constrained row keeps its
                   unconstrained diagonal alone.  Built from dense element matrices: for the small meshes of the tests.
layer_field()      per-cell values from per-layer values along the slowest direction, through the cells' centres.
"""
import numpy as np
import scipy.sparse as sp

from general_reference import GeneralReference


class ModuliReference(GeneralReference):
    def __init__(self, problem, lam, G, rule="gauss", threads=None):
        super().__init__(problem, rule, threads)
        self.lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
        self.G = np.ascontiguousarray(G, dtype=np.float64).reshape(-1)
        assert self.lam.shape == (self.n_cells,) and self.G.shape == (self.n_cells,)

    def apply_full(self, x):
        """the unconstrained operator: y_i = sum_K sum_q (lambda_K tr eps(u) I + 2 G_K eps(u)) : grad phi_i JxW"""
        x = np.asarray(x, dtype=np.float64)
        y = np.zeros(self.n_u)
        dim, nq, ns = self.dim, self.nq, self.ns

        def work(c0):
            c1 = min(c0 + self.chunk, self.n_cells)
            Gr, jxw = self._geometry(c0, c1)
            e = c1 - c0
            idx = self.cdu[c0:c1]
            lam, G = self.lam[c0:c1], self.G[c0:c1]
            u = x[idx].reshape(e, ns, dim)
            Gt = np.ascontiguousarray(Gr.transpose(0, 1, 3, 2)).reshape(e, nq * dim, ns)
            g = np.matmul(Gt, u).reshape(e, nq, dim, dim)                  # g[e, q, d, c] = d u_c / d x_d
            tr = np.trace(g, axis1=2, axis2=3)
            s = G[:, None, None, None] * (g + g.transpose(0, 1, 3, 2))
            for a in range(dim):
                s[:, :, a, a] += lam[:, None] * tr
            s *= jxw[:, :, None, None]
            ye = np.matmul(Gt.transpose(0, 2, 1), s.reshape(e, nq * dim, dim))
            self._scatter(y, idx, ye.reshape(e, ns * dim))
        self._run(work)
        return y

    def diag_full(self):
        y = np.zeros(self.n_u)
        dim = self.dim

        def work(c0):
            c1 = min(c0 + self.chunk, self.n_cells)
            Gr, jxw = self._geometry(c0, c1)
            lam, G = self.lam[c0:c1, None, None, None], self.G[c0:c1, None, None, None]
            n2 = (Gr * Gr).sum(axis=3)
            dd = (lam + G) * Gr * Gr + G * n2[:, :, :, None]
            de = np.einsum("eqsc,eq->esc", dd, jxw)
            self._scatter(y, self.cdu[c0:c1], de.reshape(c1 - c0, self.ns * dim))
        self._run(work)
        return y

    def element_matrices(self):
        """[cell][i][j], i = s * dim + c"""
        dim, ns = self.dim, self.ns
        Gr, jxw = self._geometry(0, self.n_cells)                          # [e][q][s][d], [e][q]
        H = np.einsum("eqsa,eqtb,eq->esatb", Gr, Gr, jxw, optimize=True)   # int d_a phi_s d_b phi_t
        lam, G = self.lam[:, None, None], self.G[:, None, None]
        Ke = np.zeros((self.n_cells, ns, dim, ns, dim))
        trH = np.einsum("esata->est", H)
        for ci in range(dim):
            for cj in range(dim):
                Ke[:, :, ci, :, cj] = lam * H[:, :, ci, :, cj] + G * H[:, :, cj, :, ci]
            Ke[:, :, ci, :, ci] += G * trH
        return Ke.reshape(self.n_cells, ns * dim, ns * dim)

    def assemble_full(self):
        Ke = self.element_matrices()
        rows = np.repeat(self.cdu[:, :, None], self.dpc, axis=2)
        cols = np.repeat(self.cdu[:, None, :], self.dpc, axis=1)
        A = sp.coo_matrix((Ke.ravel(), (rows.ravel(), cols.ravel())), shape=(self.n_u, self.n_u)).tocsr()
        A.sum_duplicates()
        return A

    def assemble(self):
        A = self.assemble_full().tolil()
        d = self.assemble_full().diagonal()
        fixed = np.where(self.mask)[0]
        A = A.tocsr()
        keep = sp.diags((~self.mask).astype(float))
        A = keep @ A @ keep + sp.diags(np.where(self.mask, d, 0.0))
        A = A.tocsr(); A.eliminate_zeros()
        assert len(fixed) == self.mask.sum()
        return A

    def block_diagonal(self):
        """assemble() without the coupling between displacement components (node-interleaved dofs)"""
        A = self.assemble().tocoo()
        same = (A.row % self.dim) == (A.col % self.dim)
        return sp.coo_matrix((A.data[same], (A.row[same], A.col[same])), shape=A.shape).tocsr()


def cell_centres(problem):
    d = problem.desc
    X = np.ctypeslib.as_array(d.vertex_coords, shape=(d.n_vertices, d.dim))
    cv = np.ctypeslib.as_array(d.cell_vertices, shape=(d.n_cells, 1 << d.dim))
    return X[cv].mean(axis=1)


def layer_field(problem, tops, values):
    """a cell takes the value of the first layer whose top is >= its centre along the slowest direction"""
    z = cell_centres(problem)[:, -1]
    idx = np.searchsorted(np.asarray(tops, dtype=float), z, side="left")
    assert idx.max() < len(values)
    return np.asarray(values, dtype=float)[idx]


# ---- NumPy model of the layered block inverse (PREC_FDM with a field layered along the slowest direction) -----------------------------------------------------
def fe1d_weighted(k, h, w):
    """dense FE_Q(k) mass and stiffness matrices of a line with cell sizes h and per-cell weights w"""
    M2 = np.array([[4, 2, -1], [2, 16, 2], [-1, 2, 4]]) / 30.0; K2 = np.array([[7, -8, 1], [-8, 16, -8], [1, -8, 7]]) / 3.0
    M1 = np.array([[2, 1], [1, 2]]) / 6.0; K1 = np.array([[1.0, -1], [-1, 1]])
    Me, Ke = (M2, K2) if k == 2 else (M1, K1)
    n = k * len(h) + 1
    M, K = np.zeros((n, n)), np.zeros((n, n))
    for e in range(len(h)):
        s = slice(k * e, k * e + k + 1)
        M[s, s] += w[e] * h[e] * Me; K[s, s] += w[e] / h[e] * Ke
    return M, K


def line_cells(problem):
    """cell sizes per direction of a box or tensor-product grid, from the vertex planes"""
    d = problem.desc
    X = np.ctypeslib.as_array(d.vertex_coords, shape=(d.n_vertices, d.dim))
    return [np.diff(np.unique(np.round(X[:, a], 12))) for a in range(d.dim)]


def fixed_faces(problem, bc):
    """fix[c][d][side] from the Dirichlet list [(label = 2 d + side, component, value)] of a colorized box"""
    dim = problem.desc.dim
    fix = np.zeros((dim, dim, 2), bool)
    for label, comp, _ in bc:
        fix[comp, label // 2, label % 2] = True
    return fix


def layered_block_inverse(problem, bc, layer_lam, layer_G, g):
    """z = blockdiag(A_cc)^-1 g on the free dofs (0 on the Dirichlet dofs) by the algorithm of the device: generalised eigenpairs of the leading directions per
    (component, direction), one banded solve per mode and component along the slowest direction.  Node-interleaved lexicographic dofs"""
    import scipy.linalg as sl
    d = problem.desc
    dim, k = d.dim, d.degree_u
    last = dim - 1
    h = line_cells(problem)
    nn = [k * len(h[a]) + 1 for a in range(dim)]
    fix = fixed_faces(problem, bc)
    layer_lam, layer_G = np.asarray(layer_lam, float), np.asarray(layer_G, float)
    l2g = layer_lam + 2 * layer_G
    gz = np.asarray(g, float).reshape(nn[::-1] + [dim])                      # [z][y][x][c] (2D: [y][x][c])
    z = np.zeros_like(gz)
    for c in range(dim):
        free = [np.arange(int(fix[c, a, 0]), nn[a] - int(fix[c, a, 1])) for a in range(dim)]
        S, lam = [], []
        for a in range(last):
            M, K = fe1d_weighted(k, h[a], np.ones(len(h[a])))
            f = free[a]
            w, V = sl.eigh(K[np.ix_(f, f)], M[np.ix_(f, f)])                  # V^T M V = I
            S.append(V); lam.append(w)
        f = free[last]
        Mw = [fe1d_weighted(k, h[last], l2g if a == c else layer_G)[0][np.ix_(f, f)] for a in range(last)]
        Kw = fe1d_weighted(k, h[last], l2g if last == c else layer_G)[1][np.ix_(f, f)]
        r = gz[..., c]
        if dim == 3:
            r = r[np.ix_(free[2], free[1], free[0])]
            t = np.einsum("zyx,xp,yq->zqp", r, S[0], S[1])
            out = np.empty_like(t)
            for q in range(t.shape[1]):
                for p in range(t.shape[2]):
                    out[:, q, p] = np.linalg.solve(lam[0][p] * Mw[0] + lam[1][q] * Mw[1] + Kw, t[:, q, p])
            zc = np.einsum("zqp,xp,yq->zyx", out, S[0], S[1])
            z[np.ix_(free[2], free[1], free[0], [c])] = zc[..., None]
        else:
            r = r[np.ix_(free[1], free[0])]
            t = np.einsum("yx,xp->yp", r, S[0])
            out = np.empty_like(t)
            for p in range(t.shape[1]):
                out[:, p] = np.linalg.solve(lam[0][p] * Mw[0] + Kw, t[:, p])
            zc = np.einsum("yp,xp->yx", out, S[0])
            z[np.ix_(free[1], free[0], [c])] = zc[..., None]
    return z.reshape(-1)


def layer_means(problem, values):
    """arithmetic mean of a per-cell array over every cell layer of the slowest direction"""
    zc = np.round(cell_centres(problem)[:, -1], 9)
    return np.array([np.asarray(values)[zc == v].mean() for v in np.unique(zc)])


# ---- the shapes of the block-inverse tests (tests/test_moduli_cpu.py: the model; tests/test_moduli_gpu.py: the device) -----------------------------------------
def _all(dim, faces):
    return [(f, c, 0.0) for f in faces for c in range(dim)]


BOTTOM3, BOTH3, XFACE3 = _all(3, [4]), _all(3, [4, 5]), _all(3, [0])
MIXED3 = [(0, 0, 0.0), (1, 0, 0.0), (4, 1, 0.0), (4, 2, 0.0), (5, 2, 0.0)]         # u_x: both x faces (z free at both ends), u_y: bottom only, u_z: both ends
MIXED2 = [(0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0)]
# name: (dim, cells, size, degree, Dirichlet list, grading or None)
FDM_CASES = {
    "q2-5x4x6-mixed": (3, [5, 4, 6], [5.0, 3.0, 4.0], 2, MIXED3, None),             # 11 x 9 columns: not a multiple of 64 lanes
    "q2-5x4x1-bottom": (3, [5, 4, 1], [5.0, 3.0, 0.7], 2, BOTTOM3, None),           # lines of 3 nodes
    "q2-5x4x2-both": (3, [5, 4, 2], [5.0, 3.0, 1.5], 2, BOTH3, None),
    "q2-3x2x6-xface": (3, [3, 2, 6], [3.0, 2.0, 4.0], 2, XFACE3, None),
    "q1-5x4x6-mixed": (3, [5, 4, 6], [5.0, 3.0, 4.0], 1, MIXED3, None),
    "q1-3x2x1-bottom": (3, [3, 2, 1], [3.0, 2.0, 0.7], 1, BOTTOM3, None),           # lines of 2 nodes
    "q2-graded-4x3x5-bottom": (3, [4, 3, 5], [10.0, 10.0, 10.0], 2, BOTTOM3, [1.0, 0.5, -0.7]),
    "2d-q2-5x4-mixed": (2, [5, 4], [5.0, 3.0], 2, MIXED2, None),
    "2d-q1-6x5-both": (2, [6, 5], [6.0, 4.0], 1, _all(2, [2, 3]), None),
    "2d-q2-7x1-bottom": (2, [7, 1], [7.0, 0.5], 2, _all(2, [2]), None),
}


def fdm_problem(name, material):
    import poroelasticity_dealii_amd as pk
    dim, n, size, deg, bc, grading = FDM_CASES[name]
    if grading is not None:
        return pk.Problem.graded_box(dim, n, size, deg, material, bc, grading), bc
    return pk.Problem.box(dim, n, size, deg, material, bc), bc


def layer_decades(material, n_layers, scale=1.0):
    """per-layer lambda and G over three decades (the stiffness of a layer), G / lambda varying by a factor of two from layer to layer (its Poisson ratio)"""
    dec = lambda k: 10.0 ** (-3 * ((7 * int(k)) % 5) / 4)                    # noqa: E731
    return (scale * material.lame_lambda * np.array([dec(k) for k in range(n_layers)]),
            scale * material.shear_G * np.array([dec(k) * (0.7, 1.0, 1.4)[k % 3] for k in range(n_layers)]))


def per_cell(problem, layer_values):
    """layer values -> cells, by the cell layer of the slowest direction"""
    zc = np.round(cell_centres(problem)[:, -1], 9)
    return np.asarray(layer_values)[np.searchsorted(np.unique(zc), zc)]

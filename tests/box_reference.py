"""Plain fp64 NumPy / SciPy reference of every operator on a tensor-product box (uniform or graded), independent of the product code.

On such a box each operator is a sum of Kronecker products of small 1D finite-element matrices (equidistant Lagrange bases of degree 1 / 2 on
the 1D grid of every direction, Gauss(k+1) quadrature, which integrates all of them exactly).  Operators are applied by contracting those 1D
matrices with the (nz, ny, nx) node array of a field - the 3D matrix is never assembled - and the exact inverses of the Kronecker sums come from
the 1D generalised eigendecompositions K V = M V diag(lam), V^T M V = I, restricted to the free nodes of each direction.

Numbering: displacement dof = node * dim + component, scalar dof = vertex, nodes lexicographic with x fastest (the box and graded-box builders
keep this numbering; the tests against the oracle check it).  Dirichlet rows follow the product's and the oracle's convention (checked against
export_csr(MAT_A_U)): a constrained row keeps only its unconstrained diagonal, free rows drop the constrained columns, and the right-hand side is
zero on the constrained dofs with the lifting -A g moved into the free rows."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp


def _lagrange(k, t):
    """values and derivatives of the equidistant Lagrange basis of degree k on [0, 1] at the points t: [len(t), k+1] each"""
    nodes = np.arange(k + 1) / k
    v, d = np.ones((len(t), k + 1)), np.zeros((len(t), k + 1))
    for i in range(k + 1):
        for m in range(k + 1):
            if m == i:
                continue
            f = (t - nodes[m]) / (nodes[i] - nodes[m])
            d[:, i] = d[:, i] * f + v[:, i] / (nodes[i] - nodes[m])
            v[:, i] *= f
    return v, d


def matrices_1d(grid, k_test, k_trial, what):
    """1D matrix on the vertex grid: rows = test basis of degree k_test, columns = trial basis of degree k_trial.  what: "mass" (phi psi),
    "stiff" (phi' psi'), "dtest" (phi' psi), "dtrial" (phi psi').  Gauss(max(k)+1) points: exact for all of them."""
    grid = np.asarray(grid, dtype=np.float64)
    ne = len(grid) - 1
    xq, wq = np.polynomial.legendre.leggauss(max(k_test, k_trial) + 1)
    xq, wq = (xq + 1) / 2, wq / 2
    vt, dt = _lagrange(k_test, xq)
    vs, ds = _lagrange(k_trial, xq)
    rows, cols, vals = [], [], []
    for e in range(ne):
        L = grid[e + 1] - grid[e]
        if what == "mass":
            loc = L * (vt * wq[:, None]).T @ vs
        elif what == "stiff":
            loc = (dt * wq[:, None]).T @ ds / L
        elif what == "dtest":
            loc = (dt * wq[:, None]).T @ vs
        elif what == "dtrial":
            loc = (vt * wq[:, None]).T @ ds
        else:
            raise ValueError(what)
        r, c = np.meshgrid(e * k_test + np.arange(k_test + 1), e * k_trial + np.arange(k_trial + 1), indexing="ij")
        rows.append(r.ravel()); cols.append(c.ravel()); vals.append(loc.ravel())
    shape = (ne * k_test + 1, ne * k_trial + 1)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=shape)


def along(B, X, d):
    """apply the 1D matrix B (dense or sparse) in direction d (0 = x, the last axis) of the node array X"""
    ax = X.ndim - 1 - d
    Y = np.moveaxis(X, ax, 0)
    sh = Y.shape
    Z = B @ Y.reshape(sh[0], -1)
    return np.moveaxis(np.asarray(Z).reshape((B.shape[0],) + sh[1:]), 0, ax)


def kron_apply(mats, X):
    """(mats[dim-1] x ... x mats[0]) X: mats[d] acts in direction d"""
    for d, B in enumerate(mats):
        X = along(B, X, d)
    return X


def _kron_diag(diags):
    """diagonal of the Kronecker product, as a node array"""
    out = np.ones(())
    for v in diags[::-1]:                       # slowest direction first
        out = np.multiply.outer(out, v)
    return out


class BoxReference:
    """every operator of the problem's tensor-product box, from its descriptor (material, 1D grids, Dirichlet list) alone"""

    def __init__(self, problem):
        d = problem.desc
        self.dim, self.k = d.dim, d.degree_u
        m = d.mat
        self.lam, self.G, self.alpha, self.M, self.kmu = m.lame_lambda, m.shear_G, m.biot_alpha, m.biot_M, m.k_over_mu
        if d.box.enabled:
            self.grid = [d.box.origin[a] + d.box.h[a] * np.arange(d.box.n[a] + 1) for a in range(self.dim)]
        elif d.tensor.enabled:
            self.grid = [np.ctypeslib.as_array(d.tensor.grid[a], shape=(d.tensor.n[a] + 1,)).copy() for a in range(self.dim)]
        else:
            raise ValueError("not a tensor-product box")
        if d.part.n_ranks > 1:
            raise ValueError("one rank only")
        self.n = [len(g) - 1 for g in self.grid]
        self.shape_u = tuple(self.k * n + 1 for n in self.n[::-1])        # (nz, ny, nx)
        self.shape_p = tuple(n + 1 for n in self.n[::-1])
        self.n_u, self.n_p = self.dim * int(np.prod(self.shape_u)), int(np.prod(self.shape_p))
        assert self.n_u == d.n_dofs_u and self.n_p == d.n_dofs_p, (self.n_u, d.n_dofs_u, self.n_p, d.n_dofs_p)
        k = self.k
        self.Mu = [matrices_1d(g, k, k, "mass") for g in self.grid]
        self.Ku = [matrices_1d(g, k, k, "stiff") for g in self.grid]
        self.Du = [matrices_1d(g, k, k, "dtest") for g in self.grid]          # phi_i' phi_j
        self.Mp = [matrices_1d(g, 1, 1, "mass") for g in self.grid]
        self.Kp = [matrices_1d(g, 1, 1, "stiff") for g in self.grid]
        self.Bup = [matrices_1d(g, k, 1, "dtest") for g in self.grid]         # (u test)' (p trial)
        self.Nup = [matrices_1d(g, k, 1, "mass") for g in self.grid]          # (u test) (p trial)
        nd = d.n_dirichlet
        self.dir_dof = np.ctypeslib.as_array(d.dirichlet_dof, shape=(nd,)).copy() if nd else np.zeros(0, np.int32)
        self.dir_val = np.ctypeslib.as_array(d.dirichlet_value, shape=(nd,)).copy() if nd else np.zeros(0)
        self.mask = np.zeros(self.n_u, bool); self.mask[self.dir_dof] = True
        self.g = np.zeros(self.n_u); self.g[self.dir_dof] = self.dir_val
        self._eig = {}

    # ---- layout ------------------------------------------------------------------------------------------------------------------------------
    def comps(self, x):
        return [np.asarray(x, dtype=np.float64)[c::self.dim].reshape(self.shape_u) for c in range(self.dim)]

    def pack(self, fields):
        out = np.empty(self.n_u)
        for c, f in enumerate(fields):
            out[c::self.dim] = f.ravel()
        return out

    # ---- displacement operator ---------------------------------------------------------------------------------------------------------------
    def apply_full(self, x):
        """the unconstrained elasticity operator: block (a, a) = (lam+2G) K_a + G sum_{b != a} K_b (each K tensored with M elsewhere); block (a, b), a != b:
        lam (D in a, D^T in b) + G (D^T in a, D in b), D = int phi_i' phi_j (test derivative)"""
        X = self.comps(x)
        Y = []
        for a in range(self.dim):
            y = np.zeros(self.shape_u)
            for d in range(self.dim):
                y += (self.lam + 2 * self.G if d == a else self.G) * kron_apply(self.Mu[:d] + [self.Ku[d]] + self.Mu[d + 1:], X[a])
            for b in range(self.dim):
                if b == a:
                    continue
                y += self.lam * kron_apply([self.Du[e] if e == a else self.Du[e].T if e == b else self.Mu[e] for e in range(self.dim)], X[b])
                y += self.G * kron_apply([self.Du[e].T if e == a else self.Du[e] if e == b else self.Mu[e] for e in range(self.dim)], X[b])
            Y.append(y)
        return self.pack(Y)

    def diag_full(self):
        dM = [B.diagonal() for B in self.Mu]
        dK = [B.diagonal() for B in self.Ku]
        out = []
        for a in range(self.dim):
            out.append(sum((self.lam + 2 * self.G if d == a else self.G) * _kron_diag(dM[:d] + [dK[d]] + dM[d + 1:]) for d in range(self.dim)))
        return self.pack(out)

    def apply_A(self, x):
        """A_u as the product and the oracle hold it: free rows without the constrained columns, constrained rows = their full diagonal"""
        x = np.asarray(x, dtype=np.float64)
        y = self.apply_full(np.where(self.mask, 0.0, x))
        y[self.mask] = self.diag_full()[self.mask] * x[self.mask]
        return y

    def diag_A(self):
        return self.diag_full()

    def rhs_u(self, p):
        """alpha int p div(phi_i) - (A_full g)_i on the free rows (g = the Dirichlet values), 0 on the constrained rows"""
        P = np.asarray(p, dtype=np.float64).reshape(self.shape_p)
        b = self.pack([self.alpha * kron_apply([self.Bup[e] if e == c else self.Nup[e] for e in range(self.dim)], P) for c in range(self.dim)])
        b -= self.apply_full(self.g)
        b[self.mask] = 0.0
        return b

    # ---- pressure and projection -------------------------------------------------------------------------------------------------------------
    def _scalar(self, x, c_mass, c_stiff):
        X = np.asarray(x, dtype=np.float64).reshape(self.shape_p)
        y = c_mass * kron_apply(self.Mp, X) if c_mass else np.zeros(self.shape_p)
        if c_stiff:
            for d in range(self.dim):
                y += c_stiff * kron_apply(self.Mp[:d] + [self.Kp[d]] + self.Mp[d + 1:], X)
        return y.ravel()

    def mass_p(self, x):
        return self._scalar(x, 1.0, 0.0)

    def laplace_p(self, x):
        return self._scalar(x, 0.0, 1.0)

    def jacobian_coefficients(self, dt):
        """J = M_p / (M dt) + (k / mu) K_p, as assemble_jacobian(dt) forms it"""
        return 1.0 / self.M / dt, self.kmu

    def jacobian_p(self, x, dt):
        return self._scalar(x, *self.jacobian_coefficients(dt))

    def proj_rhs(self, u, a, b):
        """int q eps_ab(u), eps = sym grad u, q the Q1 test functions"""
        U = self.comps(u)

        def grad(c, e):     # int q d_e u_c
            return kron_apply([self.Bup[f].T.tocsr() if f == e else self.Nup[f].T.tocsr() for f in range(self.dim)], U[c])
        return (0.5 * (grad(a, b) + grad(b, a))).ravel()

    # ---- exact inverses ----------------------------------------------------------------------------------------------------------------------
    def _eigh(self, key, K, M, keep):
        if key not in self._eig:
            Kd, Md = K.toarray()[np.ix_(keep, keep)], M.toarray()[np.ix_(keep, keep)]
            lam, V = sla.eigh(Kd, Md)
            self._eig[key] = (lam, V)
        return self._eig[key]

    def _kron_sum_solve(self, R, eigs, coef, c0):
        """(c0 M + sum_d coef[d] K_d)^-1 R with eigs[d] = (lam_d, V_d) of the pair (K_d, M_d) on the free nodes"""
        T = R
        for d, (lam, V) in enumerate(eigs):
            T = along(V.T, T, d)
        den = np.full(T.shape, c0)
        for d, (lam, V) in enumerate(eigs):
            sh = [1] * T.ndim; sh[T.ndim - 1 - d] = len(lam)
            den = den + coef[d] * lam.reshape(sh)
        T = T / den
        for d, (lam, V) in enumerate(eigs):
            T = along(V, T, d)
        return T

    def free_nodes(self, c):
        """per direction, the 1D nodes of component c that no Dirichlet face constrains; raises unless the constrained set is a union of whole faces"""
        M = self.mask[c::self.dim].reshape(self.shape_u)
        keep, want = [], np.zeros(self.shape_u, bool)
        for d in range(self.dim):
            ax = self.dim - 1 - d
            n1 = self.shape_u[ax]
            lo, hi = np.take(M, 0, axis=ax).all(), np.take(M, n1 - 1, axis=ax).all()
            keep.append(np.arange(int(lo), n1 - int(hi)))
            idx = [slice(None)] * self.dim
            if lo:
                idx[ax] = 0; want[tuple(idx)] = True
            if hi:
                idx[ax] = n1 - 1; want[tuple(idx)] = True
        if not np.array_equal(want, M):
            raise ValueError(f"component {c}: the Dirichlet dofs are not a union of whole faces")
        return keep

    def block_inverse_u(self, r):
        """blockdiag(A_cc)^-1 r on the free dofs of every component, zero on the constrained ones"""
        R = self.comps(r)
        out = []
        for c in range(self.dim):
            keep = self.free_nodes(c)
            eigs = [self._eigh(("u", d, tuple(keep[d][[0, -1]]), len(keep[d])), self.Ku[d], self.Mu[d], keep[d]) for d in range(self.dim)]
            sub = R[c][np.ix_(*keep[::-1])]
            z = np.zeros(self.shape_u)
            z[np.ix_(*keep[::-1])] = self._kron_sum_solve(sub, eigs, [self.lam + 2 * self.G if d == c else self.G for d in range(self.dim)], 0.0)
            out.append(z)
        return self.pack(out)

    def _eig_p(self):
        return [self._eigh(("p", d), self.Kp[d], self.Mp[d], np.arange(self.shape_p[self.dim - 1 - d])) for d in range(self.dim)]

    def jacobian_p_inverse(self, r, dt):
        a, b = self.jacobian_coefficients(dt)
        return self._kron_sum_solve(np.asarray(r, dtype=np.float64).reshape(self.shape_p), self._eig_p(), [b] * self.dim, a).ravel()

    def mass_p_inverse(self, r):
        return self._kron_sum_solve(np.asarray(r, dtype=np.float64).reshape(self.shape_p), self._eig_p(), [0.0] * self.dim, 1.0).ravel()


def reference_pcg(apply, precond, b, x0, abs_tol, rel_tol, max_iter, stop_rule=0, inert=None):
    """SolverCG as include/poroel_hip.h states it: recursive residual g, stop when ||g|| <= max(abs_tol, rel_tol * ||b||) (stop_rule 0, PORO_STOP_RHS)
    or rel_tol * ||g_0|| (1, PORO_STOP_REDUCTION).  inert: dofs whose initial residual is zeroed (the constrained rows, as the device recurrence does).
    Returns (x, iterations, [||g_0||, ||g_1||, ...], tolerance)."""
    x = np.array(x0, dtype=np.float64)
    g = apply(x) - b
    if inert is not None:
        g[inert] = 0.0
    res = np.sqrt(g @ g)
    tol = max(abs_tol, rel_tol * (res if stop_rule == 1 else np.sqrt(b @ b)))
    hist = [res]
    if res <= tol:
        return x, 0, hist, tol
    h = precond(g)
    dvec = -h
    gh = g @ h
    it = 0
    while True:
        it += 1
        h = apply(dvec)
        alpha = gh / (dvec @ h)
        g += alpha * h
        x += alpha * dvec
        res = np.sqrt(g @ g)
        hist.append(res)
        if res <= tol or it >= max_iter:
            return x, it, hist, tol
        h = precond(g)
        beta_old, gh = gh, g @ h
        dvec = (gh / beta_old) * dvec - h

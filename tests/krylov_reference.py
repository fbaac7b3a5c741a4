"""Long-double reference of the Krylov layer: the iterates x_1 .. x_K and the residual norms of SolverCG's recurrence (tests/box_reference.py::reference_pcg, without a
stopping test) and the preconditioners of include/poroel_hip.h as the formulas the header states.  Host only (NumPy / SciPy), independent of the product code.

Everything runs in two precisions from the same code: numpy.longdouble (the reference) and float64 (its twin).  An operator or preconditioner here is a function that
keeps the precision of its argument; `dual` makes one from a SciPy CSR matrix (CSR times vector keeps long double).  The twin measures how far plain fp64 rounding moves an
iterate: a (case, k) whose twin is further than 1e-14 from the long-double run is past the point where any fp64 implementation can be compared (`Iterates.drift`).

Conventions shared with the oracle (oracle/poro_oracle.cpp::cg) and restated here, not taken from the product:
  - the system lives on the rows that are not `inert` (Dirichlet rows, and the hanging rows on refined meshes): the initial residual is zeroed there, so every later
    vector of the recurrence is zero there too and x keeps its start value;
  - on a mesh with hanging nodes the operator is the condensed C^T A C (C: a hanging row holds its masters' weights), while the Jacobi diagonal D is that of the
    UNCONDENSED matrix A - the oracle scales by it as well, and it is what "D" means in every formula of the header on such a mesh.

Measured on the CPU, on (3,4,5) Q2, (5,7) Q1 and Q2, (9,5,2) Q1 (tests/test_krylov_reference_cpu.py prints the figures): the fp64 twin and the oracle's own capped Jacobi-CG
(another summation order) stay within 3.2e-15 of the long-double iterates for every k <= 12, relative to max|x_k|, residual norms within 7.2e-15 of theirs (Q1 systems: 1.1e-14); a 1 % error in lambda_max moves
the Chebyshev iterates by 2e-2 .. 3e-4 for k <= 4 (oct_q2, q1_2d)."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble


def csr_ld(A):
    """the same CSR matrix with long-double values"""
    A = sp.csr_matrix(A)
    return sp.csr_matrix((A.data.astype(LD), A.indices, A.indptr), shape=A.shape)


def dual(A):
    """v -> A v in the precision of v (float64 or long double)"""
    A64 = sp.csr_matrix(A, dtype=np.float64); Ald = csr_ld(A64)
    return lambda v: (Ald if v.dtype == LD else A64) @ v


def condensed(A, Cm):
    """v -> C^T A C v in the precision of v, never forming the product matrix"""
    a, c, ct = dual(A), dual(Cm), dual(sp.csr_matrix(Cm).T.tocsr())
    return lambda v: ct(a(c(v)))


class Operator:
    """the matrix of a system as the reference functions take it: A v in the precision of v (`__call__`), the Jacobi diagonal `diag`, and the fp64 matrix itself (`matrix`).
    Cm (refined meshes): the operator is the condensed C^T A C, applied factor by factor, while `diag` stays that of A (module docstring)"""

    def __init__(self, A, Cm=None):
        self.A = sp.csr_matrix(A, dtype=np.float64); self.Cm = Cm
        self.n = self.A.shape[0]
        self.diag = self.A.diagonal()
        self._apply = dual(self.A) if Cm is None else condensed(self.A, Cm)

    def __call__(self, v):
        return self._apply(v)

    def matrix(self):
        return self.A if self.Cm is None else (self.Cm.T @ self.A @ self.Cm).tocsr()


def constraint_matrix(n, dof, ptr, master, weight):
    """the square C of x = C x + x_inh: identity on the unconstrained dofs, a constrained row = the weights of its masters (the elimination of
    tests/test_constraints_cpu.py::test_condensed_solve_equals_direct_elimination, kept square so that vectors keep their numbering)"""
    free = np.setdiff1d(np.arange(n), dof)
    rows = list(free) + [dof[i] for i in range(len(dof)) for _ in range(ptr[i], ptr[i + 1])]
    cols = list(free) + list(master)
    vals = [1.0] * free.size + list(weight)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


class Iterates:
    """x[k - 1] = x_k (k = 1 .. K) and res[k] = ||g_k|| (k = 0 .. K) in long double; x64 / res64: the fp64 twin"""

    def __init__(self, x, res, x64, res64):
        self.x, self.res, self.x64, self.res64 = x, res, x64, res64

    def drift(self, k):
        """(iterate, residual): distance of the fp64 twin from the long-double run at iteration k, relative to max|x_k| and ||g_k||"""
        x, y = self.x[k - 1], self.x64[k - 1].astype(LD)
        return float(np.abs(x - y).max() / np.abs(x).max()), float(abs(self.res[k] - LD(self.res64[k])) / self.res[k])


def recurrence(apply, precond, b, x0, inert, K, dtype):
    x = np.array(x0, dtype=dtype); b = np.asarray(b).astype(dtype)
    g = apply(x) - b
    g[inert] = 0
    xs, res = [], [np.sqrt(g @ g)]
    h = precond(g)
    d = -h
    gh = g @ h
    for _ in range(K):
        h = apply(d)
        h[inert] = 0
        alpha = gh / (d @ h)
        g = g + alpha * h
        x = x + alpha * d
        xs.append(x.copy()); res.append(np.sqrt(g @ g))
        h = precond(g)
        gh_old, gh = gh, g @ h
        d = (gh / gh_old) * d - h
    assert all(v.dtype == dtype for v in xs)
    return xs, res


def pcg_iterates(apply, precond, b, x0, inert, K):
    """K iterations of SolverCG's recurrence from x0, no stopping test: g = A x - b (zeroed on `inert`), d = -P g, then alpha = g.Pg / d.Ad, g += alpha A d, x += alpha d,
    beta = g.Pg / (g.Pg)_old, d = beta d - P g.  apply / precond keep the precision of their argument"""
    inert = np.asarray(inert, dtype=bool)
    xs, res = recurrence(apply, precond, b, x0, inert, K, LD)
    x64, res64 = recurrence(apply, precond, b, x0, inert, K, np.float64)
    return Iterates(xs, res, x64, res64)


def _dinv(diag, inert, dtype):
    out = np.zeros(len(diag), dtype=dtype)
    keep = ~np.asarray(inert, dtype=bool)
    out[keep] = 1 / np.asarray(diag).astype(dtype)[keep]
    return out


def identity(inert):
    """PORO_PREC_NONE"""
    keep = ~np.asarray(inert, dtype=bool)
    return lambda g: np.where(keep, g, 0)


def jacobi(A, inert):
    """z = D^-1 g, zero on the inert rows (A: an Operator)"""
    inv = {t: _dinv(A.diag, inert, t) for t in (LD, np.float64)}
    return lambda g: inv[g.dtype.type] * g


def chebyshev_roots(lmax, ratio, m):
    """the m + 1 roots of T_{m+1} shifted to [lmax / ratio, lmax], largest first"""
    lmax, ratio = LD(lmax), LD(ratio)
    lmin = lmax / ratio
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    i = np.arange(m + 1).astype(LD)
    return np.sort(theta - delta * np.cos(LD(np.pi) * (2 * i + 1) / (2 * (m + 1))))[::-1]      # (np.pi in fp64 moves a root by 1e-16 relative: below everything compared here)


def chebyshev(A, inert, lmax, ratio, m):
    """z = q(D^-1 A) D^-1 g with 1 - lambda q(lambda) = prod_j (1 - lambda / r_j) over the roots r_j of T_{m+1} on [lmax / ratio, lmax]: z_1 = D^-1 g / r_0,
    z_{j+1} = z_j + D^-1 (g - A z_j) / r_j, j = 1 .. m.  Odd m is rounded up.  The polynomial does not depend on the order of the roots; they are taken largest first"""
    m = m + (m & 1)
    roots = chebyshev_roots(lmax, ratio, m)
    inv = {t: _dinv(A.diag, inert, t) for t in (LD, np.float64)}

    def precond(g):
        t = g.dtype.type
        r = roots.astype(t); di = inv[t]
        z = di * g / r[0]
        for j in range(1, m + 1):
            z = z + di * (g - A(z)) / r[j]
        return z
    return precond


def block_inverse(A, inert, dim):
    """z = blockdiag(A_cc)^-1 g on the rows that are not inert (c = dof % dim), zero elsewhere: sparse LU per component and one step of iterative refinement with the
    residual taken in the precision of g"""
    A = A.matrix(); keep = ~np.asarray(inert, dtype=bool)
    blocks = []
    for c in range(dim):
        idx = np.flatnonzero(keep[c::dim]) * dim + c
        B = A[idx][:, idx].tocsc()
        blocks.append((idx, spla.splu(B), dual(B.tocsr())))

    def precond(g):
        z = np.zeros_like(g)
        for idx, lu, B in blocks:
            r = g[idx]
            y = lu.solve(r.astype(np.float64)).astype(g.dtype)
            y = y + lu.solve((r - B(y)).astype(np.float64)).astype(g.dtype)
            z[idx] = y
        return z
    return precond


def interpolation(problem):
    """P of poro_desc.coarse as a CSR matrix on the dofs: one row of (node, weight) per displacement node, the same for every component"""
    d = problem.desc; dim = d.dim
    nf = d.n_dofs_u // dim
    box = C.cast(d.coarse.box_problem, C.POINTER(type(d))).contents
    nc = box.n_dofs_u // dim
    ptr = np.ctypeslib.as_array(d.coarse.ptr, shape=(nf + 1,)).copy(); nnz = int(ptr[-1])
    node = np.ctypeslib.as_array(d.coarse.node, shape=(nnz,)).copy(); w = np.ctypeslib.as_array(d.coarse.weight, shape=(nnz,)).copy()
    return sp.kron(sp.csr_matrix((w, node, ptr), shape=(nf, nc)), sp.identity(dim)).tocsr()


class CoarseProblem:
    """the uniform box under a refined mesh (poro_desc.coarse.box_problem) with the two members the oracle and BoxReference read"""

    def __init__(self, problem):
        d = problem.desc
        self.desc_ptr = C.cast(d.coarse.box_problem, C.POINTER(type(d)))
        self.desc = self.desc_ptr.contents


def refined_block_inverse(box_reference, A_H, dim):
    """coarse_block_inverse for two_level: BoxReference.block_inverse_u (fp64 fast diagonalisation) + one step of iterative refinement against the block diagonal of the
    coarse matrix A_H, the residual in the precision of the argument"""
    A_H = sp.coo_matrix(A_H)
    same = (A_H.row % dim) == (A_H.col % dim)
    blk = dual(sp.csr_matrix((A_H.data[same], (A_H.row[same], A_H.col[same])), shape=A_H.shape))
    mask = box_reference.mask

    def inverse(r):
        solve = lambda v: box_reference.block_inverse_u(np.asarray(v, dtype=np.float64)).astype(r.dtype)
        z = solve(r)
        res = r - blk(z)
        res[mask] = 0
        return z + solve(res)
    return inverse


def two_level(A, inert, P_interp, coarse_block_inverse, omega):
    """z = omega D^-1 g + P B_H^-1 P^T g, zero on the inert rows (g is zero there)"""
    p, pt = dual(P_interp), dual(sp.csr_matrix(P_interp).T.tocsr())
    inv = {t: _dinv(A.diag, inert, t) for t in (LD, np.float64)}
    keep = ~np.asarray(inert, dtype=bool)

    def precond(g):
        t = g.dtype.type
        g = np.where(keep, g, 0)
        z = t(omega) * inv[t] * g + p(coarse_block_inverse(pt(g)))
        return np.where(keep, z, 0)
    return precond


def chebyshev_default_ratio(problem):
    """the "mesh-size based default" of poro_solver_opts.poly_degree: min(400, max(10, c n^2)) with c = 0.2 (Q2) or 0.05 (Q1) and n the largest cell count of a
    direction on a uniform box, round(cells^(1/dim)) elsewhere (one rank)"""
    d = problem.desc
    n = max(d.box.n[:d.dim]) if d.box.enabled else round(d.n_cells ** (1.0 / d.dim))
    return min(400.0, max(10.0, (0.2 if d.degree_u == 2 else 0.05) * n * n))


# ---- the systems of a mesh, from the oracle -------------------------------------------------------------------------------------------------------------------------
def _cons_arrays(c):
    if c.n == 0:
        return np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0)
    ptr = np.ctypeslib.as_array(c.ptr, shape=(c.n + 1,)).copy(); nm = int(ptr[-1])
    return (np.ctypeslib.as_array(c.dof, shape=(c.n,)).copy(), ptr, np.ctypeslib.as_array(c.master, shape=(nm,)).copy(), np.ctypeslib.as_array(c.weight, shape=(nm,)).copy(),
            np.ctypeslib.as_array(c.inhomogeneity, shape=(c.n,)).copy())


class System:
    """one linear system of a mesh: the operator (condensed where `cons` lists hanging nodes), the right-hand side, the inert rows, and what a solve leaves on them"""

    def __init__(self, A, b, cons, dir_dof=(), dir_val=()):
        n = len(b)
        self.b = np.asarray(b, dtype=np.float64)
        self.dof, self.ptr, self.master, self.weight, self.inhom = cons
        self.dir_dof, self.dir_val = np.asarray(dir_dof, dtype=np.int64), np.asarray(dir_val, dtype=np.float64)
        self.inert = np.zeros(n, bool); self.inert[self.dir_dof] = True; self.inert[self.dof] = True
        self.free = ~self.inert
        self.A = Operator(A, constraint_matrix(n, self.dof, self.ptr, self.master, self.weight) if len(self.dof) else None)

    def distribute(self, x):
        """constraints.distribute on a copy of x: the Dirichlet values, then every hanging entry from its masters"""
        x = np.array(x)
        x[self.dir_dof] = self.dir_val
        for i, dof in enumerate(self.dof):
            k = slice(self.ptr[i], self.ptr[i + 1])
            x[dof] = self.inhom[i] + self.weight[k] @ x[self.master[k]]
        return x


def csr(rp, col, val):
    return sp.csr_matrix((val, col, rp), shape=(len(rp) - 1, len(rp) - 1))


def displacement_system(problem, oracle):
    """A_u, the oracle's right-hand side (assembled by the caller) and the constraint lists of the displacement space"""
    d = problem.desc; nd = d.n_dirichlet
    dof = np.ctypeslib.as_array(d.dirichlet_dof, shape=(nd,)).copy() if nd else np.zeros(0, np.int32)
    val = np.ctypeslib.as_array(d.dirichlet_value, shape=(nd,)).copy() if nd else np.zeros(0)
    return System(csr(*oracle.export_csr(0)), oracle.get(1), _cons_arrays(d.cons_u), dof, val)


def scalar_system(problem, oracle, which_matrix, which_rhs):
    """the pressure Jacobian (MAT_JACOBIAN_P, VEC_RESIDUAL_P) or the projection's mass matrix (MAT_MASS_P, VEC_PROJ_RHS0 + e) with the pressure space's hanging nodes"""
    return System(csr(*oracle.export_csr(which_matrix)), oracle.get(which_rhs), _cons_arrays(problem.desc.cons_p))

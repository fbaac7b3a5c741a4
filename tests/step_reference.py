"""Independent NumPy / SciPy model of the TIME STEP with every field on: per-cell moduli, scalar or diagonal-tensor permeability, gravity with per-cell density,
prescribed pressures, tractions and hanging nodes, on any MappingQ1 mesh.  Helper module of the test-suite, not collected.  It shares no code with the product or with
oracle/: a cell loop over the descriptor's mesh arrays (vertex_coords, cell_vertices, cell_dofs_u / _p, the boundary-face list, the Dirichlet / Neumann / prescribed-
pressure lists, the constraint lists) and the material constants, quadrature by einsum, COO scatter, sparse direct solves.

Reused from the suite: GeneralReference._geometry (gradients, JxW), ModuliReference.assemble_full (A_u), gravity_reference.body_force / gravity_flux,
darcy_reference.constraints_p / prescribed_dofs_p / _normals, krylov_reference.constraint_matrix.  New here:
  Du    [n_u, n_p]  int psi_j div(phi_i), Gauss(k + 1): what alpha p enters the displacement right-hand side through
  S     [n_u, n_p]  the same integral with the strain projection's Gauss(2) rule, sum_a S_aa.  Du == S on affine cells (Q2: the integrand has degree 3 per direction);
                    on non-affine Q2 cells the two rules differ and the step really solves with S in the pressure equation - the model keeps both
  Mp, K(kappa)      Gauss(2);  well source: Gauss(2) of the cylinder indicator x^2 + y^2 <= r^2 with the reference's pi = 3.1415926;  tractions: value * n_component on the
                    labelled boundary faces, Gauss(k + 1) on the face

Two drivers.
  monolithic_step(u_old, p_old)   the backward-Euler Biot system the coupled / incremental loop converges to,
        [ A_u                 -alpha Du              ] [u]   [ tractions + body force ]
        [ (alpha / dt) S^T    Mp / (M_b dt) + K      ] [p] = [ (alpha / dt) S^T u_old + Mp p_old / (M_b dt) - src_well - f_g ]
      on the free rows: u = C_u z + (Dirichlet values and inhomogeneities), p = C_p z + (prescribed values), rows folded with C^T.  One splu of the block matrix
      and one refinement step whose residual is formed in long double.  eps_v = the projection of div u: C_p (C_p^T Mp C_p)^-1 C_p^T S^T u.
  walk(...)                       the loop of host/problem.hpp time_step, both flavours, with the fixed-stress update eps_v += alpha / K_node dp (K_node: nodal means of
      lambda + 2 G / 3 over the cells that touch the pressure dof) and direct solves everywhere; returns the trace columns 1, 2, 4, 5, the state after every
      step and how far every stopping decision was from its threshold.
The ingredients the sensitivity runs perturb are plain attributes of the constructor: kappa, lam, G, rho_f, rho, alpha_u (displacement right-hand side), alpha_p (storage
term), traction (one value per Neumann entry) and p_bc (one value per prescribed dof)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import darcy_reference as dr
import gravity_reference as gr
from general_reference import cell_vertices, lagrange_1d, q1_at, rule_1d, tensor_shapes, vertices
from krylov_reference import constraint_matrix
from moduli_reference import ModuliReference

LD = np.longdouble
PI_WELL = 3.1415926


def _constraints(c):
    """(dof, ptr, master, weight, inhomogeneity) of one constraint list of the descriptor"""
    n = c.n
    if not n:
        return np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0)
    ptr = np.ctypeslib.as_array(c.ptr, shape=(n + 1,)).copy()
    inh = np.ctypeslib.as_array(c.inhomogeneity, shape=(n,)).copy() if c.inhomogeneity else np.zeros(n)
    return (np.ctypeslib.as_array(c.dof, shape=(n,)).copy(), ptr, np.ctypeslib.as_array(c.master, shape=(int(ptr[n]),)).copy(),
            np.ctypeslib.as_array(c.weight, shape=(int(ptr[n]),)).copy(), inh)


def _scatter(rows, cols, vals, shape):
    A = sp.coo_matrix((vals.ravel(), (rows.ravel(), cols.ravel())), shape=shape).tocsr()
    A.sum_duplicates()
    return A


def _shape_at(dim, k, xi):
    """values of the tensor-product Lagrange basis of degree k (x fastest) at one reference point"""
    m = k + 1
    si = np.array(list(np.ndindex(*([m] * dim))))[:, ::-1]
    out = np.ones(len(si))
    for a in range(dim):
        out *= lagrange_1d(k, np.array([xi[a]]))[0][0][si[:, a]]
    return out


def _ld_residual(A, x, b):
    """b - A x with the products and the sum in long double"""
    A = A.tocoo()
    r = np.asarray(b, dtype=LD).copy()
    np.subtract.at(r, A.row, A.data.astype(LD) * np.asarray(x, dtype=LD)[A.col])
    return r


class StepReference:
    def __init__(self, P, dt, p_init, lam=None, G=None, kappa=None, gravity=None, rho_f=0.0, rho=2700.0, hydrostatic=False,
                 alpha_u=None, alpha_p=None, traction=None, p_bc=None):
        d = P.desc
        m = d.mat
        self.P, self.dt, self.p_init, self.hydrostatic = P, float(dt), float(p_init), bool(hydrostatic)
        self.dim, self.k, self.nc, self.n_u, self.n_p = d.dim, d.degree_u, d.n_cells, d.n_dofs_u, d.n_dofs_p
        dim, k, nc = self.dim, self.k, self.nc
        self.alpha, self.M_b, self.K_dr = m.biot_alpha, m.biot_M, m.bulk_K
        self.alpha_u = self.alpha if alpha_u is None else float(alpha_u)
        self.alpha_p = self.alpha if alpha_p is None else float(alpha_p)
        self.has_moduli = lam is not None
        self.lam = np.full(nc, m.lame_lambda) if lam is None else np.asarray(lam, dtype=float).copy()
        self.G = np.full(nc, m.shear_G) if G is None else np.asarray(G, dtype=float).copy()
        self.kappa = gr._per_cell(m.k_over_mu if kappa is None else kappa, nc, dim).copy()
        self.g = None if gravity is None or not np.any(gravity) else np.asarray(gravity, dtype=float)
        self.rho_f = float(rho_f)
        self.rho = np.broadcast_to(np.asarray(rho, dtype=float), (nc,)).copy()
        self.X, self.cv = vertices(P), cell_vertices(d)
        self.cdu = np.ctypeslib.as_array(d.cell_dofs_u, shape=(nc, (k + 1) ** dim * dim)).copy()
        self.cdp = np.ctypeslib.as_array(d.cell_dofs_p, shape=(nc, 1 << dim)).copy()
        # boundary data
        nd = d.n_dirichlet
        self.dir_dof = np.ctypeslib.as_array(d.dirichlet_dof, shape=(nd,)).copy() if nd else np.zeros(0, np.int32)
        self.dir_val = np.ctypeslib.as_array(d.dirichlet_value, shape=(nd,)).copy() if nd else np.zeros(0)
        nn = d.n_neumann
        self.neu = [np.ctypeslib.as_array(a, shape=(nn,)).copy() if nn else np.zeros(0) for a in (d.neumann_label, d.neumann_component, d.neumann_value)]
        self.traction = self.neu[2].astype(float) if traction is None else np.asarray(traction, dtype=float)
        self.pd = dr.prescribed_dofs_p(P)
        self.p_bc = (np.ctypeslib.as_array(d.dirichlet_value_p, shape=(len(self.pd),)).copy() if len(self.pd) else np.zeros(0)) if p_bc is None else np.asarray(p_bc, dtype=float)
        self._assemble()

    # ---- operators --------------------------------------------------------------------------------------------------------------------------------
    def _u_geometry(self, n):
        """values [q][s], real gradients [e][q][s][d], JxW [e][q] of the displacement basis and Q1 values [q][v] at the Gauss(n) points"""
        dim, k = self.dim, self.k
        if n == k + 1:
            Gr, jxw = self.ref._geometry(0, self.nc)
            t1, _ = rule_1d(n)
            return tensor_shapes(dim, k, t1)[0], Gr, jxw, q1_at(dim, self.ref.xi)[0]
        t1, w1 = rule_1d(n)
        qi = np.array(list(np.ndindex(*([n] * dim))))[:, ::-1]
        phi, dphi = tensor_shapes(dim, k, t1)
        N, dN = q1_at(dim, t1[qi])
        J = np.einsum("eva,qvb->eqab", self.X[self.cv], dN)
        Gr = np.einsum("eqbd,qsb->eqsd", np.linalg.inv(J), dphi, optimize=True)
        return phi, Gr, np.linalg.det(J) * np.prod(w1[qi], axis=1), N

    def _divergence(self, n):
        _, Gr, jxw, N = self._u_geometry(n)
        ns, dim, nv = (self.k + 1) ** self.dim, self.dim, 1 << self.dim
        vals = np.einsum("eqsc,qv,eq->escv", Gr, N, jxw, optimize=True).reshape(self.nc, ns * dim, nv)
        rows = np.repeat(self.cdu[:, :, None], nv, axis=2)
        cols = np.repeat(self.cdp[:, None, :], ns * dim, axis=1)
        return _scatter(rows, cols, vals, (self.n_u, self.n_p))

    def _assemble(self):
        P, dim, nc, nv = self.P, self.dim, self.nc, 1 << self.dim
        self.ref = ModuliReference(P, self.lam, self.G, threads=1)
        self.A = self.ref.assemble_full()
        self.Du = self._divergence(self.k + 1)
        self.S = self.Du if self.k == 1 else self._divergence(2)
        # pressure space, Gauss(2)
        _, _, cdp, Grp, jxwp = gr._p_geometry(P)
        _, xi2, _ = gr._points(dim, 2)
        N2 = q1_at(dim, xi2)[0]
        rows, cols = np.repeat(cdp[:, :, None], nv, axis=2), np.repeat(cdp[:, None, :], nv, axis=1)
        self.Mp = _scatter(rows, cols, np.einsum("qv,qw,eq->evw", N2, N2, jxwp), (self.n_p, self.n_p))
        self.Kp = _scatter(rows, cols, np.einsum("eqvd,ed,eqwd,eq->evw", Grp, self.kappa, Grp, jxwp, optimize=True), (self.n_p, self.n_p))
        # well source
        m = P.desc.mat
        xq = np.einsum("qv,eva->eqa", N2, self.X[self.cv])
        inside = (xq[:, :, 0] ** 2 + xq[:, :, 1] ** 2) <= m.r_well ** 2
        s_val = -m.flow_rate / (PI_WELL * m.r_well ** 2)
        self.src_well = np.zeros(self.n_p)
        np.add.at(self.src_well, cdp.ravel(), np.einsum("qv,eq,eq->ev", N2, inside * s_val, jxwp).ravel())
        # gravity
        self.f_g = gr.gravity_flux(P, self.g, self.rho_f, self.kappa) if self.g is not None and self.rho_f != 0.0 else np.zeros(self.n_p)
        self.body = gr.body_force(P, self.g, self.rho) if self.g is not None else np.zeros(self.n_u)
        self.src = self.src_well + self.f_g
        self.f_ext = self._tractions() + self.body
        # constraints
        du, ptr, ma, we, inh = _constraints(P.desc.cons_u)
        self.Cu = constraint_matrix(self.n_u, du, ptr, ma, we)
        self.u_fix = np.zeros(self.n_u); self.u_fix[self.dir_dof] = self.dir_val
        self.u_fix = self.Cu @ self.u_fix
        self.u_fix[du] += inh
        fixed = np.zeros(self.n_u, bool); fixed[self.dir_dof] = True; fixed[du] = True
        self.free_u = np.where(~fixed)[0]
        self.hang_u = du
        dp_, ptr, ma, we = dr.constraints_p(P)
        self.Cp = constraint_matrix(self.n_p, dp_, ptr, ma, we)
        self.hang_p = dp_
        hang = np.zeros(self.n_p, bool); hang[dp_] = True
        pres = np.zeros(self.n_p, bool); pres[self.pd] = True
        self.pres_mask = pres
        z = np.zeros(self.n_p)
        z[self.pd] = self.p_bc
        z[hang] = 0.0
        self.p_fix = self.Cp @ z                                   # prescribed values (a hanging prescribed dof through its masters)
        self.free_p = np.where(~hang & ~pres)[0]
        self.nonhang_p = np.where(~hang)[0]
        # nodal fixed-stress coefficient alpha / K_node
        if self.has_moduli:
            Kc = self.lam + 2.0 * self.G / 3.0
            s, t = np.zeros(self.n_p), np.zeros(self.n_p)
            np.add.at(s, self.cdp.ravel(), np.repeat(Kc, nv)); np.add.at(t, self.cdp.ravel(), 1.0)
            self.fs_coef = self.alpha / (s / t)
        else:
            self.fs_coef = np.full(self.n_p, self.alpha / self.K_dr)
        # factorisations
        CuF, CpF = self.Cu[:, self.free_u], self.Cp[:, self.free_p]
        self.CuF, self.CpF = CuF, CpF
        self.Auu = (CuF.T @ self.A @ CuF).tocsc()
        self.lu_u = spla.splu(self.Auu)
        self.J = self.Mp / (self.M_b * self.dt) + self.Kp
        self.Jff = (CpF.T @ self.J @ CpF).tocsc()
        self.lu_J = spla.splu(self.Jff)
        Cn = self.Cp[:, self.nonhang_p]
        self.Cn = Cn
        self.lu_M = spla.splu((Cn.T @ self.Mp @ Cn).tocsc())
        self._block = None

    def _tractions(self):
        d, dim, k = self.P.desc, self.dim, self.k
        f = np.zeros(self.n_u)
        if not d.n_neumann or not d.n_bfaces:
            return f
        bc, bl, bid = (np.ctypeslib.as_array(a, shape=(d.n_bfaces,)).copy() for a in (d.bface_cell, d.bface_local, d.bface_id))
        t1, w1 = rule_1d(k + 1)
        for label, comp, value in zip(self.neu[0], self.neu[1], self.traction):
            comp = int(comp)
            for face in range(2 * dim):
                cells = bc[(bid == label) & (bl == face)]
                if not cells.size:
                    continue
                dn, side = face >> 1, face & 1
                tang = [a for a in range(dim) if a != dn]
                for q in np.ndindex(*([k + 1] * (dim - 1))):
                    xi = np.empty(dim); xi[dn] = float(side); w = 1.0
                    for a, i in zip(tang, q):
                        xi[a] = t1[i]; w *= w1[i]
                    J = np.einsum("evr,vb->erb", self.X[self.cv[cells]], dr.q1_gradients(dim, xi))
                    NdS = dr._normals(J, dn, side, tang)                                        # n dS, outward
                    phi = _shape_at(dim, k, xi)
                    np.add.at(f, self.cdu[cells][:, comp::dim].ravel(), (w * value * NdS[:, comp, None] * phi[None, :]).ravel())
        return f

    # ---- pieces of the loop -------------------------------------------------------------------------------------------------------------------------
    def initial_pressure(self):
        p = np.full(self.n_p, self.p_init)
        if self.hydrostatic and self.g is not None:
            gx = gr.vertex_of_dof_p(self.P) @ self.g
            p = self.p_init + self.rho_f * (gx - (self.X @ self.g).min())
        keep = np.ones(self.n_p, bool); keep[self.hang_p] = False
        z = np.where(keep, p, 0.0)
        z[self.pres_mask & keep] = self.p_fix[self.pres_mask & keep]
        return self.Cp @ z

    def solve_u(self, p):
        b = self.f_ext + self.alpha_u * (self.Du @ p)
        z = self.lu_u.solve(self.CuF.T @ (b - self.A @ self.u_fix))
        z += self.lu_u.solve((self.CuF.T @ (b - self.A @ self.u_fix) - self.Auu @ z))
        return self.CuF @ z + self.u_fix

    def project(self, u):
        r = self.Cn.T @ (self.S.T @ u)
        e = self.lu_M.solve(r)
        e += self.lu_M.solve(r - (self.Cn.T @ self.Mp @ self.Cn) @ e)
        return self.Cn @ e

    def residual(self, p, p_old, ev, ev0):
        t = self.alpha_p * (ev - ev0) / self.dt + (p - p_old) / (self.M_b * self.dt)
        R = self.Cp.T @ (-(self.Mp @ t + self.Kp @ p + self.src))
        R[self.pres_mask] = 0.0
        R[self.hang_p] = 0.0
        return R

    def solve_J(self, R):
        z = self.lu_J.solve(R[self.free_p])
        z += self.lu_J.solve(R[self.free_p] - self.Jff @ z)
        return self.CpF @ z

    def initial_state(self):
        """(u_0, p_0, eps_v0): p_0 = p_init (hydrostatic below the top where asked) with the prescribed values, u_0 = A^-1 f(p_0), eps_v0 its projected divergence"""
        p = self.initial_pressure()
        u = self.solve_u(p)
        return u, p, self.project(u)

    def first_residual(self):
        """l2 norm of the first pressure residual of step 1: the scale the loop's absolute tolerances are set against"""
        u, p, ev = self.initial_state()
        return float(np.linalg.norm(self.residual(p, p, ev, ev)))

    # ---- the monolithic system ----------------------------------------------------------------------------------------------------------------------
    def monolithic_step(self, u_old, p_old):
        dt, CuF, CpF = self.dt, self.CuF, self.CpF
        if self._block is None:
            B = sp.bmat([[self.Auu, -self.alpha_u * (CuF.T @ self.Du @ CpF)],
                         [(self.alpha_p / dt) * (CpF.T @ self.S.T @ CuF), self.Jff]]).tocsc()
            # rows and columns scaled to a unit diagonal: the two blocks differ by twenty orders of magnitude
            s = 1.0 / np.sqrt(np.abs(B.diagonal()))
            self._scale = s
            self._Bs = (sp.diags(s) @ B @ sp.diags(s)).tocsc()
            self._block = spla.splu(self._Bs)
        s = self._scale
        bu = CuF.T @ (self.f_ext - self.A @ self.u_fix + self.alpha_u * (self.Du @ self.p_fix))
        bp = CpF.T @ ((self.alpha_p / dt) * (self.S.T @ (u_old - self.u_fix)) + self.Mp @ p_old / (self.M_b * dt) - self.J @ self.p_fix - self.src)
        b = s * np.concatenate([bu, bp])
        y = self._block.solve(b)
        y = y + self._block.solve(np.asarray(_ld_residual(self._Bs, y, b), dtype=np.float64))
        z = s * y
        nu = len(self.free_u)
        u = CuF @ z[:nu] + self.u_fix
        p = CpF @ z[nu:] + self.p_fix
        return u, p, self.project(u)

    # ---- the loop ------------------------------------------------------------------------------------------------------------------------------------
    def walk(self, n_steps, fss_tol, pressure_tol, max_fss=50, max_pres=50, coupled=False, incremental=False):
        """dict: trace [(step, fss_iteration, pressure_iterations, |p|_inf, error after displacement)], states [(u, p, eps_v, eps_v0, p_old) after every step],
        margins [max(value / threshold, threshold / value) of every computed stopping decision]"""
        u, p, ev = self.initial_state()
        ev0 = ev.copy()
        trace, states, margins = [], [(u, p, ev, ev0, p)], []

        def decide(value, threshold):
            margins.append(max(value / threshold, threshold / value) if value > 0 else np.inf)

        for step in range(1, n_steps + 1):
            p_old = p.copy()
            if incremental and step > 1:
                ev0 = ev.copy()
            err, fss = 2 * pressure_tol, 0
            while fss < max_fss and err > fss_tol:
                fss += 1
                dp = np.zeros(self.n_p); pit = 0
                while pit < max_pres:
                    pit += 1
                    ev = ev + self.fs_coef * dp
                    R = self.residual(p, p_old, ev, ev0)
                    err = float(np.linalg.norm(R))
                    decide(err, pressure_tol)
                    if err < pressure_tol:
                        break
                    dp = self.solve_J(R)
                    p = p + dp
                pinf = float(np.abs(p).max())
                u = self.solve_u(p)
                e = self.project(u)
                if coupled:
                    ev = e
                err = float(np.linalg.norm(self.residual(p, p_old, ev, ev0)))
                decide(err, fss_tol)
                trace.append((step, fss, pit - 1, pinf, err))
            states.append((u, p, ev.copy(), ev0.copy(), p_old))
        return dict(trace=trace, states=states, margins=margins)


def distance(a, b):
    """max-norm relative distance of the (u, p, eps_v) triples a and b, per field"""
    return tuple(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a[:3], b[:3]))


# ---- the cases of tests/test_step_reference_cpu.py and tests/test_step_reference_gpu.py -------------------------------------------------------------------------------
DT, P_INIT, RHO_F, GRAV = 60.0, 1e5, 1000.0, 9.81
STIFF = 3.0      # modulus fields of the cases with a default-flavour run, in units of the material's: see the notes on the cases in tests/test_step_reference_cpu.py
MIXED_2D = [(0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0)]                                  # u_x on both x faces, u_y on the bottom
ROLLERS_3D = [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)]
REFINED_BC = [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (4, 2, 0.0)]                 # a non-zero value: lifting on a mesh with hanging nodes
# id: (mesh, degree, what is switched on).  In every 3D case gravity points along -z, in 2D along -y.
COUPLED_REL = 1e-10                     # fss_tol = pressure_tol = COUPLED_REL * (first residual of the case) in the coupled / incremental flavour
DEFAULT_REL = {"box3_q2": 7.5e-9, "refined3_q2": 3.2e-7, "box2_q1": 7.5e-9}      # the same for the reference's default flavour: every stopping decision >= a factor 3 from it
CASES = {
    "box3_q2": ("box3", 2), "box2_q1": ("box2", 1), "graded3_q2": ("graded3", 2), "refined3_q1": ("refined3", 1), "refined3_q2": ("refined3", 2),
    "refined3_q2_hybrid": ("refined3", 2), "jitter2_q2": ("jitter2", 2), "jitter3_q2": ("jitter3", 2),
}


def write_box_msh(path, n, size, f=None):
    """a uniform nx x ny grid on [-size / 2, size / 2]^2 as a Gmsh 2.2 file, its nodes moved by f; boundary lines carry the ids of a colorized box (2 d + side)"""
    nx, ny = n
    xs, ys = np.linspace(-size[0] / 2, size[0] / 2, nx + 1), np.linspace(-size[1] / 2, size[1] / 2, ny + 1)
    X = np.array([[x, y] for y in ys for x in xs])
    Y = X if f is None else f(X)
    node = lambda i, j: 1 + i + (nx + 1) * j                               # noqa: E731
    lines = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", str(len(Y))]
    lines += [f"{k + 1} {p[0]:.17g} {p[1]:.17g} 0" for k, p in enumerate(Y)]
    el = []
    for j in range(ny):
        el.append((1, 0, node(0, j), node(0, j + 1))); el.append((1, 1, node(nx, j), node(nx, j + 1)))
    for i in range(nx):
        el.append((1, 2, node(i, 0), node(i + 1, 0))); el.append((1, 3, node(i, ny), node(i + 1, ny)))
    for j in range(ny):
        for i in range(nx):
            el.append((3, 7, node(i, j), node(i + 1, j), node(i + 1, j + 1), node(i, j + 1)))
    lines += ["$EndNodes", "$Elements", str(len(el))]
    lines += [f"{k + 1} {e[0]} 2 {e[1]} {e[1] + 1} " + " ".join(str(v) for v in e[2:]) for k, e in enumerate(el)]
    lines += ["$EndElements", ""]
    with open(path, "w") as fh:
        fh.write("\n".join(lines))
    return path


def lower_half(P):
    """the cells whose centre lies in the lower half of the slowest direction: the 'layer' the sensitivity runs perturb"""
    from moduli_reference import cell_centres
    z = cell_centres(P)[:, -1]
    return z < 0.5 * (z.min() + z.max())


def lattice_transposition(P):
    """the permutation that reads a per-cell array as if the fastest and the slowest lattice direction of the cell order were swapped (cells ranked by centre, x fastest,
    against the same ranking with x and the last coordinate exchanged): layered fields change too; on a refined or unstructured mesh still a shuffle of most cells"""
    from moduli_reference import cell_centres
    c = np.round(cell_centres(P), 9)
    key = [c[:, a] for a in range(c.shape[1])][::-1]                             # x and the last coordinate exchanged
    natural = np.lexsort(tuple([c[:, a] for a in range(c.shape[1])]))            # rank of every cell with x fastest
    swapped = np.lexsort(tuple(key))
    perm = np.empty(len(c), dtype=np.int64)
    perm[natural] = swapped
    return perm


class Case:
    """one problem with its fields set (pk.Problem keeps them and hands them to every context), the keyword arguments of the StepReference of the same problem,
    and which of the seven perturbations the case switches on"""

    def __init__(self, name, tmp_path=None):
        import zlib
        import poroelasticity_dealii_amd as pk
        from common import BC_3D, material
        from general_reference import jitter
        from moduli_reference import per_cell
        self.name = name
        mesh, deg = CASES[name]
        m = material()
        rng = np.random.default_rng(zlib.crc32(mesh.encode()))
        self.p_label = self.p_value = None
        self.hydrostatic = False
        neumann = []
        if mesh == "box3":
            neumann = [(5, 2, -2e5)]                                                # the top carries a normal traction: its u_z condition is left out of BC_3D
            P = pk.Problem.box(3, [3, 2, 4], [10.0] * 3, deg, m, BC_3D[:-1], neumann)
            self.p_label, self.p_value, self.hydrostatic = 5, 0.1 * P_INIT, True
        elif mesh == "box2":
            P = pk.Problem.box(2, [4, 5], [10.0] * 2, deg, m, MIXED_2D)
        elif mesh == "graded3":
            P = pk.Problem.graded_box(3, [3, 3, 3], [10.0] * 3, deg, m, ROLLERS_3D, [1.0, 0.5, -0.7])
        elif mesh == "refined3":
            P = pk.Problem.refined_box(3, [3, 3, 2], [10.0] * 3, deg, m, REFINED_BC, [0, 0, 0], [2, 1, 2])
            self.p_label, self.p_value = 2, 0.2 * P_INIT                            # the face y = -5: two refined and one coarse cell per layer, hanging nodes on it
        elif mesh == "jitter2":
            B = pk.Problem.box(2, [4, 4], [10.0] * 2, deg, m, MIXED_2D)
            f = jitter(B); B.close()
            P = pk.Problem.gmsh(write_box_msh(str(tmp_path / "jitter2.msh"), [4, 4], [10.0, 10.0], f), deg, m, MIXED_2D)
        elif mesh == "jitter3":
            # the host layer builds no non-affine 3D mesh: a 3 x 3 x 3 box as a GENERAL mesh (all-zero refinement mask: no box tag), its vertices moved in place in the
            # arrays the descriptor points at - every context is created from the descriptor - and, below, its auxiliary coarse box switched off
            P = pk.Problem.refined_box_mask(3, [3, 3, 3], [10.0] * 3, deg, m, ROLLERS_3D, np.zeros(27, dtype=np.int32))
            assert not P.desc.box.enabled and not P.desc.cons_u.n
            X = np.ctypeslib.as_array(P.desc.vertex_coords, shape=(P.desc.n_vertices, 3))
            X[:] = jitter(P)(X.copy())
            self.p_label, self.p_value = 5, 0.2 * P_INIT                            # a drained top: without it the closed box hardly flows and kappa and the storage term move p by 6e-6 only
        else:
            raise KeyError(name)
        self.P = P
        d = P.desc
        dim, nc = d.dim, d.n_cells
        low = lower_half(P)
        self.gravity = np.array([0.0] * (dim - 1) + [-GRAV])
        self.lam = self.G = self.rho = None
        self.rho_scalar = 2700.0
        if mesh == "box3":                # moduli in two layers (contrast 10), a general tensor within a decade, per-cell density
            self.lam, self.G = np.where(low, 1.0, 10.0) * STIFF * m.lame_lambda, np.where(low, 1.0, 10.0) * STIFF * m.shear_G
            self.kappa = m.k_over_mu * 10.0 ** rng.random((nc, dim))
            self.rho = 2000.0 + 700.0 * rng.random(nc)
        elif mesh == "box2":              # k / mu in two layers, general moduli
            self.kappa = np.where(low, 1.0, 5.0) * m.k_over_mu
            self.lam, self.G = STIFF * m.lame_lambda * (1.0 + 2.0 * rng.random(nc)), STIFF * m.shear_G * (1.0 + 2.0 * rng.random(nc))
        elif mesh == "graded3":           # a tensor and moduli constant in every cell layer
            self.kappa = per_cell(P, m.k_over_mu * np.array([[1.0, 2.0, 0.5], [4.0, 1.0, 3.0], [0.7, 6.0, 2.0]]))
            self.lam, self.G = per_cell(P, STIFF * m.lame_lambda * np.array([1.0, 6.0, 2.0])), per_cell(P, STIFF * m.shear_G * np.array([1.0, 3.0, 5.0]))
        elif mesh == "refined3":
            self.kappa = m.k_over_mu * 10.0 ** rng.random((nc, dim))
            self.rho = 2000.0 + 700.0 * rng.random(nc)
            if "hybrid" not in name:
                self.lam, self.G = STIFF * m.lame_lambda * (1.0 + 2.0 * rng.random(nc)), STIFF * m.shear_G * (1.0 + 2.0 * rng.random(nc))
        else:                             # the jittered meshes: one k / mu per cell, general moduli
            self.kappa = m.k_over_mu * 10.0 ** rng.random(nc)
            self.lam, self.G = m.lame_lambda * (1.0 + 2.0 * rng.random(nc)), m.shear_G * (1.0 + 2.0 * rng.random(nc))      # (no default-flavour run: softer, stronger coupling)
        # hand the fields to the problem
        if self.lam is not None:
            P.set_cell_moduli(self.lam, self.G)
        if np.ndim(self.kappa) == 2:
            P.set_cell_permeability_tensor(self.kappa)
        else:
            P.set_cell_permeability(self.kappa)
        P.set_gravity(self.gravity, RHO_F, self.rho_scalar, hydrostatic_init=self.hydrostatic)
        if self.rho is not None:
            P.set_cell_density(self.rho)
        if self.p_label is not None:
            P.set_pressure_bc([(self.p_label, self.p_value)])
        self.has_traction = bool(neumann)
        if mesh == "jitter3":
            P.desc = P.desc_ptr.contents
            P.desc.coarse.enabled = 0
            P.desc.tensor.enabled = 0
            assert not P.desc.box.enabled

    def reference(self, **change):
        """the StepReference of the case; change: constructor arguments that replace the case's (the perturbed variants)"""
        kw = dict(lam=self.lam, G=self.G, kappa=self.kappa, gravity=self.gravity, rho_f=RHO_F, rho=self.rho_scalar if self.rho is None else self.rho, hydrostatic=self.hydrostatic)
        kw.update(change)
        return StepReference(self.P, DT, P_INIT, **kw)

    def perturbations(self, rel=1e-3):
        """name -> constructor arguments of the reference with ONE ingredient changed by the relative amount rel (what the case switches on only)"""
        low = lower_half(self.P)
        base = self.reference()
        out = {}
        k = base.kappa.copy()
        if np.ndim(self.kappa) == 2:
            k[low, 0] *= 1 + rel
        else:
            k[low] *= 1 + rel                                                       # one k / mu per cell: the scalar is the component
        out["kappa (x component of a tensor) of the lower layer"] = dict(kappa=k)
        if self.lam is not None:
            l = self.lam.copy(); l[low] *= 1 + rel
            out["lambda of the lower layer"] = dict(lam=l)
        out["rho_f"] = dict(rho_f=RHO_F * (1 + rel))
        r = base.rho.copy(); r[len(r) // 2] *= 1 + rel
        out["density of one cell"] = dict(rho=r)
        out["alpha in the displacement right-hand side"] = dict(alpha_u=base.alpha * (1 + rel))
        out["alpha in the storage term"] = dict(alpha_p=base.alpha * (1 + rel))
        if self.has_traction:
            out["one traction value"] = dict(traction=base.traction * (1 + rel))
        if self.p_label is not None:
            out["the prescribed pressure"] = dict(p_bc=base.p_bc * (1 + rel))
        perm = lattice_transposition(self.P)
        tr = dict(kappa=base.kappa[perm], rho=base.rho[perm])
        if self.lam is not None:
            tr.update(lam=self.lam[perm], G=self.G[perm])
        out["cell arrays transposed"] = tr
        return out

    def close(self):
        self.P.close()


# ---- the bounds of tests/test_step_reference_gpu.py: run -> (u and p, eps_v).  10 x the distance measured on one MI355X, rounded up to a power of ten and capped at 1e-6;
# its docstring has the figures -------------------------------------------------------------------------------------------------------------------------------------------
BOUNDS = {
    "box3_q2-mf": (1e-9, 1e-9), "box3_q2-csr": (1e-8, 1e-7), "box3_q2_struct-mf": (1e-9, 1e-9), "box2_q1-mf": (1e-8, 1e-8), "box2_q1-csr": (1e-8, 1e-7),
    "graded3_q2-mf": (1e-7, 1e-6), "refined3_q1-mf": (1e-7, 1e-6), "refined3_q1-mf-atomic": (1e-7, 1e-6), "refined3_q2-mf": (1e-7, 1e-6),
    "refined3_q2-mf-atomic": (1e-7, 1e-6), "refined3_q2_hybrid-mf": (1e-7, 1e-6), "jitter3_q2-mf": (1e-7, 1e-6), "jitter3_q2-csr": (1e-7, 1e-6),
    "jitter2_q2-mf": (1e-7, 1e-6), "jitter2_q2-csr": (1e-7, 1e-6),
}
DEFAULT_BOUNDS = {"box3_q2-mf": (1e-12, 1e-12), "refined3_q2-mf": (1e-12, 1e-6), "box2_q1-csr": (1e-13, 1e-13)}


def case_bound(name):
    """the largest bound on u and p any run of the case uses: what the sensitivities are held against"""
    return max([b[0] for run, b in BOUNDS.items() if run.split("-")[0] in (name, name + "_struct")] + [b[0] for run, b in DEFAULT_BOUNDS.items() if run.split("-")[0] == name])

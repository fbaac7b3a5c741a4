"""What the CG-iterate tests share (tests/test_krylov_iterates_gpu.py on one rank, tests/test_slab_iterates_gpu.py on rank threads): the bounds, the reference iterates of a
mesh with their Chebyshev slack, the comparison of one capped solve with them, and the capture of the library's PORO_CHEB_VERBOSE line.  A mesh is any object with the
members P (the single-rank problem), S (krylov_reference.System of the displacement system), refs (a dict), coarse and true_lmax (None until first use).  The docstring of
tests/test_krylov_iterates_gpu.py derives the bounds."""
import os
import sys
import tempfile

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import poroelasticity_dealii_amd as pk
import oracle_py
import krylov_reference as kr
from box_reference import BoxReference

KS = (1, 2, 3, 4, 5, 8, 12)
K_MAX = max(KS)
BOUND = 1e-12
TWIN = 1e-14
LAMBDA_LINE = r"lambda_max\(D\^-1 A_u\) ~ ([0-9.]+)"


def coarse_inverse(M):
    if M.coarse is None:
        H = kr.CoarseProblem(M.P)
        OH = oracle_py.Oracle(H, hoisted=True)
        try:
            OH.fill(pk.VEC_P, 0.0); OH.disp_assemble_system(True)
            A_H = kr.csr(*OH.export_csr(pk.MAT_A_U))
        finally:
            OH.close()
        M.coarse = (kr.interpolation(M.P), kr.refined_block_inverse(BoxReference(H), A_H, M.P.desc.dim))
    return M.coarse


def reference_preconditioner(M, spec):
    """spec: ("jacobi",) | ("none",) | ("chebyshev", m, ratio, lmax) | ("two_level", omega) | ("fdm",)"""
    S = M.S
    if spec[0] == "jacobi":
        return kr.jacobi(S.A, S.inert)
    if spec[0] == "none":
        return kr.identity(S.inert)
    if spec[0] == "chebyshev":
        return kr.chebyshev(S.A, S.inert, spec[3], spec[2], spec[1])
    if spec[0] == "two_level":
        return kr.two_level(S.A, S.inert, *coarse_inverse(M), spec[1])
    if spec[0] == "fdm":
        return kr.block_inverse(S.A, S.inert, M.P.desc.dim)
    raise ValueError(spec)


def reference(M, spec, x0=None, K=K_MAX):
    key = (spec, None if x0 is None else x0.tobytes(), K)
    if key not in M.refs:
        M.refs[key] = kr.pcg_iterates(M.S.A, reference_preconditioner(M, spec), M.S.b, np.zeros(M.S.A.n) if x0 is None else x0, M.S.inert, K)
    return M.refs[key]


def true_lambda_max(M):
    """lambda_max(D^-1 A) on the rows of the system, D as the preconditioners use it"""
    if M.true_lmax is None:
        S = M.S
        f = np.flatnonzero(S.free)
        s = sp.diags(1 / np.sqrt(S.A.diag[f]))
        B = (s @ S.A.matrix()[f][:, f] @ s).tocsr()
        M.true_lmax = float(spla.eigsh(B, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0])
    return M.true_lmax


class Bounds:
    """per k: (iterate bound, residual bound); Chebyshev adds what the six printed decimals of lambda_max leave open"""

    def __init__(self, M, spec, x0=None, K=K_MAX):
        self.ref = reference(M, spec, x0, K)
        self.slack_x, self.slack_r = np.zeros(K + 1), np.zeros(K + 1)
        if spec[0] == "chebyshev":
            for dl in (-5e-7, 5e-7):
                other = reference(M, spec[:3] + (spec[3] + dl,), x0, K)
                for k in range(1, K + 1):
                    self.slack_x[k] = max(self.slack_x[k], float(np.abs(other.x[k - 1] - self.ref.x[k - 1]).max() / np.abs(self.ref.x[k - 1]).max()))
                    self.slack_r[k] = max(self.slack_r[k], float(abs(other.res[k] - self.ref.res[k]) / self.ref.res[k]))

    def x(self, k):
        return 4 * self.slack_x[k] + BOUND

    def r(self, k):
        return 4 * self.slack_r[k] + BOUND


class Env:
    """environment switches of a case, for the duration of a block"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def capture_stderr(fn):
    """(result of fn, what the process wrote to file descriptor 2 meanwhile) - the library writes with stdio, not through sys.stderr"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as t:
        os.dup2(t.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2); os.close(saved)
        t.seek(0)
        return out, t.read().decode(errors="replace")


def capfd_capture(capfd):
    def capture(fn):
        capfd.readouterr()
        out = fn()
        return out, capfd.readouterr().err
    return capture


def deviation(S, x_ref, u):
    """(free dofs against the reference iterate, constrained dofs against their prescribed / distributed values), both relative to max|x_k|"""
    full = S.distribute(np.where(S.free, u, 0.0))       # what distribute makes of the device's own free values
    scale = float(np.abs(x_ref).max())
    return float(np.abs(u[S.free] - x_ref[S.free]).max() / scale), float(np.abs(u[S.inert] - full[S.inert]).max() / scale) if S.inert.any() else 0.0


def check_iterate(tag, S, B, k, rc, info, u, apps, worst=None, residual_slack=0.0):
    """residual_slack: added to the bound of the residual norm (section (b) at k = N - 1, beyond the iterations of (a): the reference's own error there)"""
    ref = B.ref
    dx, dr = ref.drift(k)
    ex, ec = deviation(S, ref.x[k - 1], u)
    er = float(abs(info.final_residual - ref.res[k]) / ref.res[k])
    e0 = float(abs(info.initial_residual - ref.res[0]) / ref.res[0])
    bound_r = B.r(k) + residual_slack
    print(f"{tag} k={k}: iterate {ex:.2e} (bound {B.x(k):.2e}) residual {er:.2e} (bound {bound_r:.2e}) initial {e0:.2e} constrained {ec:.2e}; reference twin {dx:.2e} {dr:.2e}", flush=True)
    if worst is not None:
        worst[0], worst[1] = max(worst[0], ex), max(worst[1], er, e0)
    assert dx <= TWIN, f"{tag} k={k}: the reference's fp64 twin is {dx:.2e} from its long-double run - this (case, k) cannot take part: change the mesh"
    assert (rc, info.iterations, info.converged) == (1, k, 0), (tag, k, rc, info.iterations, info.converged)
    assert info.operator_applications == apps, (tag, k, info.operator_applications, apps)
    assert e0 <= BOUND and er <= bound_r, (tag, k, e0, er)
    assert ex <= B.x(k) and ec <= BOUND, (tag, k, ex, ec)
    dirichlet_only = np.setdiff1d(S.dir_dof, S.dof)
    assert np.array_equal(u[dirichlet_only], S.distribute(np.zeros(len(u)))[dirichlet_only]), (tag, k)

"""The CG ITERATES of every solve path against the long-double reference of tests/krylov_reference.py: disp_solve(max_iter=k) from a zero start returns x_k and ||g_k||,
so alpha, beta, the preconditioner and the stopping test of every driver are observable one iteration at a time.  Converged solutions (tests/test_krylov_paths_gpu.py) and
bit equality between two forms of the product (tests/test_pcg_*_gpu.py) cannot see a defect that leaves a worse but valid Krylov method; these can.

(a) iterates and residual norms at k = 1, 2, 3, 4, 5, 8, 12; (b) the same capped solves on a context with a history (iteration-count hint, full work vectors) equal those of
a fresh context bit for bit: launches enqueued behind the finishing iteration change nothing; (c) the stopping test, with thresholds taken from the reference's residuals.

Bounds.  Jacobi / none / two-level / block FDM / Q1 systems: 1e-12, relative to max|x_k| (iterates) and ||g_k|| (residual norms) - about 300 x the 3.2e-15 by which two
independent fp64 implementations differ from long double on these meshes (tests/test_krylov_reference_cpu.py); the margin is for the device's block-wise sums and fma
contraction.  Chebyshev: lambda_max is read from the product's PORO_CHEB_VERBOSE line, six decimals, so the bound of an iterate is 4 x the reference's own change when
lambda_max moves by +-5e-7, plus 1e-12 (that change: <= 2.9e-7 at k = 1, falling with k).
A (case, k) takes part only while the ITERATE of the reference's fp64 twin is within 1e-14 (relative to max|x_k|) of its long-double run - a condition on the reference,
not a measurement; none may drop out, and none does (worst 4.8e-15, block FDM on nodal_full at k = 12; the twin's residual norm is 9.1e-14 there, the
largest outside Chebyshev, and its 1e-12 bound is asserted all the same).  The twin's residual NORM, relative to ||g_k||, is printed beside it
and is no condition: the recursive residual carries rounding of the size of eps ||g_0||, so once ||g_k|| has fallen by five orders (Chebyshev of degree 4, k >= 8) the twin's
norm is 1e-13 .. 5e-12 away while its iterate is still at 1e-15; the residual bound of those cases is the lambda_max term (1e-6), far above that.

Operator applications: k + 1 on the three-kernel recurrence (initial residual + one per iteration), k + 2 on the single-reduction recurrence of partitioned runs (one more:
it applies the operator to z before it knows that the residual has converged), (m + 1)(k + 1) with a Chebyshev polynomial of degree m on either.

Measured on one MI355X, worst over the k of a family, iterate (relative to max|x_k|) / residual norm (relative to ||g_k||); every line of a run with -s shows its figures:
  Jacobi, none (oct_q2 MF, q1_2d CSR, refined_2d MF)               6.2e-15 / 3.6e-15
  two-level (refined_2d, refined_3d; omega 1, 0.7)                  6.0e-15 / 9.5e-15
  block FDM (octant, planar, nodal, oct_q2 without octants)        8.3e-15 / 2.5e-14   (nodal_full, k = 12)
  block FDM, (26,26,26) Q2, against the fp64 Kronecker reference    9.6e-14 / 2.1e-14
  Q1 systems against the oracle (q1_3d; refined (5,4,3))            2.9e-15 / 7.9e-14   (pressure Jacobian, k = 12)
  single-reduction driver / three-kernel recurrence on that path   7.4e-15 / 6.3e-15   (Chebyshev as below)
  capped solve at k = N - 1 = 94 after a history (Jacobi)           6.6e-15 / 2.2e-12   (the twin's residual norm: 6.4e-13; bound 1e-12 + 4 x that, see section (b))
  the same for two-level (k = 36), FDM octant (21), FDM planar (18) 5.2e-15 / 1.9e-10, 6.0e-15 / 1.7e-14, 5.4e-15 / 3.9e-15   (twins 1.6e-10, 1.2e-14, 1.6e-14)
  Q1 systems on refined_3d, k <= 8                                  1.4e-15 / 2.4e-15
  Chebyshev: iterate <= 0.75 x the reference's own change under lambda_max +- 5e-7 (a quarter of the bound's term) everywhere (4.1e-7 at k = 1 on q1_2d, m = 2, ratio 30; 6.9e-8 on oct_q2, fused and unfused alike);
             residual norm <= 2.0e-5 (q1_2d, m = 4, ratio 10, k = 12, where ||g_12|| = 2e-13 ||g_0|| and the lambda_max term is 2.7e-5), 1.5e-6 on oct_q2.
             The device keeps all digits of lambda_max and the reference the six printed ones: these figures measure the rounding of that line, not the kernels.
  lambda_max printed / true: 1.0493 (oct_q2), 1.0492 (planar_split), 1.0500 (q1_2d, refined_2d): the Lanczos estimate + 5 %, nowhere capped by the element bound.
No defect found.  The tests bite: with two roots of chebyshev_plan made equal the 21 Chebyshev cases of (a) that were run fail (all but the odd-degree one, not run), and
with k_pcg_update_d_fused reading PcgScalars::gh2 at the other parity every case of (a) outside the octant / planar forms fails from k = 3 on, while
tests/test_krylov_paths_gpu.py passes with either (scratch builds, not committed)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tools"), HERE, os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import poroelasticity_dealii_amd as pk
import oracle_py
import krylov_reference as kr
import krylov_digest as kd
from box_reference import BoxReference
from krylov_checks import (BOUND, K_MAX, KS, LAMBDA_LINE, TWIN, Bounds, Env, capfd_capture, capture_stderr, check_iterate, deviation,   # noqa: F401 - shared with tests/test_slab_iterates_gpu.py
                           reference, true_lambda_max)

pytestmark = pytest.mark.gpu

MF, CSR = pk.OP_MATRIX_FREE, pk.OP_CSR
LD = kr.LD


# ---- reference side: one entry per mesh, built at first use and only read afterwards ------------------------------------------------------------------------------------
# The Q1 systems' mesh with hanging nodes.  On refined_3d of tools/krylov_digest.py the pressure space has 50 free dofs and Jacobi-CG on its mass matrix is close to an invariant
# subspace at k = 12: the oracle's own capped solve is 2.3e-11 (residual norm, projection entry 5) from the long-double recurrence there and the fp64 twin 1.3e-11 - the
# reference's own error is above the bound.  On this mesh (154 free pressure dofs) both stay below 2.2e-15 for every k <= 12
REFINED_Q1 = {"refined_3d_q1": ((5, 4, 3), 2, (1, 1, 0), (3, 3, 2))}


class Mesh:
    def __init__(self, name):
        if name in REFINED_Q1:
            n, deg, lo, hi = REFINED_Q1[name]
            self.P = pk.Problem.refined_box(len(n), list(n), [10.0] * len(n), deg, kd.bench.material(), kd.BC_3D, list(lo), list(hi))
        else:
            self.P = kd.problem(name)
        self.O = oracle_py.Oracle(self.P, hoisted=True)
        self.O.set(pk.VEC_P, kd.u_inputs(self.O.n_p)); self.O.disp_assemble_system(True)
        self.S = kr.displacement_system(self.P, self.O)
        self.refs, self.coarse, self.true_lmax = {}, None, None

    def close(self):
        self.O.close(); self.P.close()


_meshes = {}


def mesh(name):
    if name not in _meshes:
        _meshes[name] = Mesh(name)
    return _meshes[name]


def close_meshes():
    for M in _meshes.values():
        M.close()
    _meshes.clear()


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    close_meshes()


# ---- device side ----------------------------------------------------------------------------------------------------------------------------------------------------------
def context(M, mode, p=None):
    G = kd.context(M.P, mode)
    G.set(pk.VEC_P, kd.u_inputs(G.n_p) if p is None else p); G.disp_assemble_system(True)
    return G


def printed_lambda_max(G, solve_kw, capture=capture_stderr):
    """the first Chebyshev solve after assembly estimates lambda_max and, under PORO_CHEB_VERBOSE, prints it"""
    with Env({"PORO_CHEB_VERBOSE": "1"}):
        G.fill(pk.VEC_U, 0.0)
        _, err = capture(lambda: G.disp_solve(abs_tol=1e-300, rel_tol=0.0, max_iter=1, **solve_kw))
    found = re.findall(LAMBDA_LINE, err)
    assert len(found) == 1, err
    return float(found[0])


def capped(G, k, solve_kw, x0=None):
    if x0 is None:
        G.fill(pk.VEC_U, 0.0)
    else:
        G.set(pk.VEC_U, x0)
    rc, info = G.disp_solve(abs_tol=1e-300, rel_tol=0.0, max_iter=k, **solve_kw)
    return rc, info, G.get(pk.VEC_U)


def run_displacement_case(tag, mesh_name, mode, prec, spec, kw=None, env=None, apps=None, ks=KS, capture=capture_stderr):
    """section (a) for one displacement case.  spec: the reference preconditioner; ("chebyshev", m, ratio) gets lambda_max from the device's printed line.  apps(k): expected
    operator applications"""
    M = mesh(mesh_name); S = M.S
    solve_kw = dict(kw or {}, prec=prec)
    with Env(env or {}):
        G = context(M, mode)
        try:
            if spec[0] == "chebyshev":
                lmax = printed_lambda_max(G, solve_kw, capture)
                true = true_lambda_max(M)
                print(f"{tag}: lambda_max printed {lmax:.6f}, true {true:.6f} (ratio {lmax / true:.4f})")
                assert true * (1 - 1e-9) <= lmax <= 1.06 * true, (tag, lmax, true)
                spec = spec + (lmax,)
            runs = [(k,) + capped(G, k, solve_kw) for k in ks]
        finally:
            G.close()
    B = Bounds(M, spec)
    m = spec[1] + (spec[1] & 1) if spec[0] == "chebyshev" else 0
    apps = apps or ((lambda k: (m + 1) * (k + 1)) if m else (lambda k: k + 1))
    worst = [0.0, 0.0]
    for k, rc, info, u in runs:
        check_iterate(tag, S, B, k, rc, info, u, apps(k), worst)
    print(f"{tag}: worst iterate deviation {worst[0]:.2e}, worst residual deviation {worst[1]:.2e}", flush=True)
    return spec


# ---- (a) iterates -----------------------------------------------------------------------------------------------------------------------------------------------------------
JACOBI_CASES = {"jacobi_oct_q2_mf": ("oct_q2", MF, pk.PREC_JACOBI, ("jacobi",)), "jacobi_q1_2d_csr": ("q1_2d", CSR, pk.PREC_JACOBI, ("jacobi",)),
                "jacobi_refined_2d_mf": ("refined_2d", MF, pk.PREC_JACOBI, ("jacobi",)), "none_q1_2d_csr": ("q1_2d", CSR, pk.PREC_NONE, ("none",))}


@pytest.mark.parametrize("case", list(JACOBI_CASES))
def test_jacobi_iterates(case):
    run_displacement_case(case, *JACOBI_CASES[case])


CHEB_MESHES = {"oct_q2_fused": ("oct_q2", MF, {}), "oct_q2_unfused": ("oct_q2", MF, {"PORO_CHEB_UNFUSED": "1"}), "planar_split": ("planar_split", MF, {}), "q1_2d_csr": ("q1_2d", CSR, {}),
               "refined_2d": ("refined_2d", MF, {})}


@pytest.mark.parametrize("ratio", [10.0, 30.0])
@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("where", list(CHEB_MESHES))
def test_chebyshev_iterates(capfd, where, m, ratio):
    name, mode, env = CHEB_MESHES[where]
    run_displacement_case(f"chebyshev_{where}_m{m}_ratio{ratio:g}", name, mode, pk.PREC_CHEBYSHEV, ("chebyshev", m, ratio), {"poly_degree": m, "omega": ratio}, env, capture=capfd_capture(capfd))


def test_chebyshev_iterates_with_the_default_ratio_and_degree(capfd):
    """poly_degree 0 -> 6, omega 0 -> the mesh-size based default, restated in krylov_reference.chebyshev_default_ratio"""
    M = mesh("oct_q2")
    run_displacement_case("chebyshev_oct_q2_defaults", "oct_q2", MF, pk.PREC_CHEBYSHEV, ("chebyshev", 6, kr.chebyshev_default_ratio(M.P)), {"poly_degree": 0, "omega": 0.0}, capture=capfd_capture(capfd))


def test_chebyshev_rounds_an_odd_degree_up(capfd):
    run_displacement_case("chebyshev_oct_q2_m3", "oct_q2", MF, pk.PREC_CHEBYSHEV, ("chebyshev", 3, 30.0), {"poly_degree": 3, "omega": 30.0}, ks=(1, 2, 3), capture=capfd_capture(capfd))


@pytest.mark.parametrize("omega", [1.0, 0.7])
@pytest.mark.parametrize("name", ["refined_2d", "refined_3d"])
def test_two_level_iterates(name, omega):
    run_displacement_case(f"two_level_{name}_omega{omega:g}", name, MF, pk.PREC_TWO_LEVEL, ("two_level", omega), {"omega": omega})


FDM_CASES = {"fdm_oct_q2": ("oct_q2", {}), "fdm_planar_split": ("planar_split", {}), "fdm_nodal_full": ("nodal_full", {}), "fdm_oct_q2_no_oct": ("oct_q2", {"PORO_FDMU_NO_OCT": "1"})}


@pytest.mark.parametrize("case", list(FDM_CASES))
def test_block_fdm_iterates(case):
    name, env = FDM_CASES[case]
    run_displacement_case(case, name, MF, pk.PREC_FDM, ("fdm",), env=env)


def q1_setup(S, n_p, n_u, dim):
    """the inputs of tools/krylov_digest.py::run_q1 on an oracle or a context (same calls)"""
    vals, u = kd.q1_inputs(n_p, n_u)
    for k, v in vals.items():
        S.set(k, v)
    dt = kd.bench.INPUT["dt"]
    S.pres_assemble_residual(dt); S.pres_assemble_jacobian(dt)
    S.set(pk.VEC_U, u); S.proj_assemble_matrix(); S.proj_assemble_rhs([a * dim + a for a in range(dim)])


@pytest.mark.parametrize("name,ks", [("q1_3d", KS), ("refined_3d_q1", KS), ("refined_3d", KS[:-1])])
def test_q1_system_iterates_follow_the_oracles_capped_solve(name, ks):
    """pressure Jacobian and projection mass matrix with Jacobi: the device's capped solves against the oracle's (whole vectors: the hanging entries are distributed by both);
    the reference's twin condition, iterate and residual norm, is evaluated on the long-double recurrence of the same systems.  refined_3d itself takes part up to k = 8,
    where its twin holds (<= 2.4e-15); its k = 12 is what REFINED_Q1 replaces"""
    M = mesh(name); P, O = M.P, M.O
    dim = P.desc.dim
    q1_setup(O, O.n_p, O.n_u, dim)
    G = kd.context(P, MF)
    try:
        q1_setup(G, G.n_p, G.n_u, dim)
        systems = [("pressure", pk.MAT_JACOBIAN_P, pk.VEC_RESIDUAL_P, pk.VEC_DP, lambda S, **kw: S.pres_solve(**kw))]
        for e in kd.proj_entries(dim):
            systems.append((f"projection{e}", pk.MAT_MASS_P, pk.VEC_PROJ_RHS0 + e, pk.VEC_STRAIN0 + e, lambda S, e=e, **kw: S.proj_solve(e, **kw)))
        worst = [0.0, 0.0]
        for sysname, mat, rhs, vec, solve in systems:
            Sq = kr.scalar_system(P, O, mat, rhs)
            ref = kr.pcg_iterates(Sq.A, kr.jacobi(Sq.A, Sq.inert), Sq.b, np.zeros(O.n_p), Sq.inert, K_MAX)
            for k in ks:
                O.fill(vec, 0.0); G.fill(vec, 0.0)
                rc0, i0 = solve(O, abs_tol=1e-300, rel_tol=0.0, max_iter=k, prec=oracle_py.PREC_JACOBI)
                rc1, i1 = solve(G, abs_tol=1e-300, rel_tol=0.0, max_iter=k, prec=pk.PREC_JACOBI)
                x0, x1 = O.get(vec), G.get(vec)
                dx, dr = ref.drift(k)
                ex = float(np.abs(x1 - x0).max() / np.abs(x0).max())
                er, e0 = abs(i1.final_residual - i0.final_residual) / i0.final_residual, abs(i1.initial_residual - i0.initial_residual) / i0.initial_residual
                print(f"q1 {name} {sysname} k={k}: iterate {ex:.2e} residual {er:.2e} initial {e0:.2e}; reference twin {dx:.2e} {dr:.2e}", flush=True)
                worst[0], worst[1] = max(worst[0], ex), max(worst[1], er, e0)
                assert dx <= TWIN and dr <= TWIN, f"{name} {sysname} k={k}: the reference's fp64 twin is {dx:.2e} / {dr:.2e} from its long-double run"
                assert (rc0, i0.iterations, i0.converged) == (1, k, 0) and (rc1, i1.iterations, i1.converged) == (1, k, 0), (sysname, k)
                assert i1.operator_applications == k + 1, (sysname, k, i1.operator_applications)
                assert ex <= BOUND and er <= BOUND and e0 <= BOUND, (sysname, k, ex, er, e0)
        print(f"q1 {name}: worst iterate deviation {worst[0]:.2e}, worst residual deviation {worst[1]:.2e}")
    finally:
        G.close()


def test_block_fdm_iterates_above_the_polling_threshold():
    """(26,26,26) Q2 = 446 631 dofs, nodal form: above 400 000 dofs an ungated preconditioner is polled after every iteration.  Reference: the fp64 Kronecker operator and
    exact block inverse of tests/box_reference.py (no long-double twin at this size; three iterations)"""
    n = (26, 26, 26)
    P = pk.Problem.box(3, list(n), [10.0] * 3, 2, kd.bench.material(), kd.BC_3D)
    try:
        assert P.desc.n_dofs_u == 446631
        R = BoxReference(P)
        p = kd.u_inputs(R.n_p)
        xs, res = kr.recurrence(R.apply_A, R.block_inverse_u, R.rhs_u(p), np.zeros(R.n_u), R.mask, 3, np.float64)
        with Env({"PORO_FDMU_NO_OCT": "1"}):
            G = pk.Context(P, 0, MF)
            try:
                G.set(pk.VEC_P, p); G.disp_assemble_system(True)
                for k in (1, 2, 3):
                    rc, info, u = capped(G, k, dict(prec=pk.PREC_FDM))
                    free = ~R.mask
                    ex = float(np.abs(u[free] - xs[k - 1][free]).max() / np.abs(xs[k - 1]).max())
                    er, e0 = abs(info.final_residual - res[k]) / res[k], abs(info.initial_residual - res[0]) / res[0]
                    print(f"fdm_26x26x26_no_oct k={k}: iterate {ex:.2e} residual {er:.2e} initial {e0:.2e}", flush=True)
                    assert (rc, info.iterations, info.converged, info.operator_applications) == (1, k, 0, k + 1), (k, rc, info.iterations, info.converged, info.operator_applications)
                    assert ex <= BOUND and er <= BOUND and e0 <= BOUND, (k, ex, er, e0)
                    assert np.array_equal(u[R.mask], R.g[R.mask])
            finally:
                G.close()
    finally:
        P.close()


# ---- driver variants: one child process each (PORO_TWO_REDUCTION_CG is read once per process) -------------------------------------------------------------------------------
# case -> (mesh, preconditioner, reference spec, solve keywords, environment of the case); the last entry of VARIANT_APPS tells which recurrence counts the applications
VARIANT_CASES = {"jacobi": ("oct_q2", pk.PREC_JACOBI, ("jacobi",), {}, {}), "chebyshev": ("oct_q2", pk.PREC_CHEBYSHEV, ("chebyshev", 4, 30.0), {"poly_degree": 4, "omega": 30.0}, {}),
                 "fdm": ("oct_q2", pk.PREC_FDM, ("fdm",), {}, {}), "fdm_no_oct": ("oct_q2", pk.PREC_FDM, ("fdm",), {}, {"PORO_FDMU_NO_OCT": "1"})}
# the single-reduction driver runs Jacobi, Chebyshev and the nodal block FDM; the slab form of the octant kernels keeps the three-kernel recurrence
VARIANTS = {"partitioned": (dict(kd.ONE_RANK), {"jacobi": "single", "chebyshev": "polynomial", "fdm": "three", "fdm_no_oct": "single"}),
            "partitioned_two_reductions": (dict(kd.ONE_RANK, PORO_TWO_REDUCTION_CG="1"), {"jacobi": "three", "chebyshev": "polynomial", "fdm": "three", "fdm_no_oct": "three"})}


def run_variant(variant):
    """in the child: section (a) for the variant's cases, then section (c) for Jacobi on its driver"""
    for case, counting in VARIANTS[variant][1].items():
        name, prec, spec, kw, env = VARIANT_CASES[case]
        apps = {"single": lambda k: k + 2, "three": lambda k: k + 1, "polynomial": None}[counting]
        run_displacement_case(f"{variant}_{case}", name, MF, prec, spec, kw, env, apps)
    stopping_checks(f"{variant}_jacobi", "oct_q2", MF, pk.PREC_JACOBI, ("jacobi",), {})
    close_meshes()


def test_driver_variants_in_child_processes():
    """the single-reduction driver (the partitioned code path on one RCCL rank) and the three-kernel recurrence on the same path: one child per variant, each under its own
    time limit; nothing is started after a child that failed"""
    for variant, (env, _) in VARIANTS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", variant], env=dict(os.environ, **env), timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, flush=True)
        assert r.returncode == 0, f"variant {variant}: exit status {r.returncode}; nothing further was started\n{r.stdout[-3000:]}"


# ---- (b) history independence -----------------------------------------------------------------------------------------------------------------------------------------------
HISTORY_CASES = {"jacobi_mf": ("oct_q2", pk.PREC_JACOBI, ("jacobi",), {}), "chebyshev_fused": ("oct_q2", pk.PREC_CHEBYSHEV, ("chebyshev", 4, 30.0), {"poly_degree": 4, "omega": 30.0}),
                 "fdm_octant": ("oct_q2", pk.PREC_FDM, ("fdm",), {}), "fdm_planar": ("planar_split", pk.PREC_FDM, ("fdm",), {}), "two_level": ("refined_3d", pk.PREC_TWO_LEVEL, ("two_level", 1.0), {"omega": 1.0})}


@pytest.mark.parametrize("case", list(HISTORY_CASES))
def test_capped_solves_do_not_depend_on_the_contexts_history(capfd, case):
    """A context that has solved to rel_tol 1e-11 (N iterations) and then another right-hand side warm carries an iteration-count hint near N and full work vectors; a capped
    solve on it enqueues min(hint, 256) iterations, all but the first k behind the finishing one.  It must return the bits of the same capped solve on a fresh context, and
    meet the reference bound of (a) wherever the reference's twin condition holds"""
    name, prec, spec, kw = HISTORY_CASES[case]
    M = mesh(name); S = M.S
    solve_kw = dict(kw, prec=prec)
    p, p_other = kd.u_inputs(M.O.n_p), kd.u_inputs(M.O.n_p) * (1 + 0.1 * np.cos(0.21 * np.arange(M.O.n_p)))
    G = context(M, MF)
    try:
        if spec[0] == "chebyshev":
            spec = spec + (printed_lambda_max(G, solve_kw, capfd_capture(capfd)),)

        def with_history(k):
            G.fill(pk.VEC_U, 0.0)
            rc, first = G.disp_solve(abs_tol=1e-300, rel_tol=1e-11, max_iter=20000, **solve_kw)
            assert rc == 0
            G.set(pk.VEC_P, p_other); G.disp_assemble_system(False)
            assert G.disp_solve(abs_tol=1e-300, rel_tol=1e-11, max_iter=20000, **solve_kw)[0] == 0
            G.set(pk.VEC_P, p); G.disp_assemble_system(False)
            return (first.iterations,) + (capped(G, k, solve_kw) if k else ())
        N = with_history(0)[0]
        assert N >= 7, N
        ks = (1, 3, 4, 5, N - 1)
        B = Bounds(M, spec, K=max(K_MAX, N - 1))
        m = spec[1] if spec[0] == "chebyshev" else 0
        for k in ks:
            n_again, rc, info, u = with_history(k)
            assert n_again == N
            F = context(M, MF)
            try:
                rc_f, info_f, u_f = capped(F, k, solve_kw)
            finally:
                F.close()
            same = (rc, info.iterations, info.converged, info.operator_applications) == (rc_f, info_f.iterations, info_f.converged, info_f.operator_applications)
            print(f"history {case} k={k} (N={N}): iterations {info.iterations} / fresh {info_f.iterations}, residual equal {info.final_residual == info_f.final_residual}, u equal {np.array_equal(u, u_f)}", flush=True)
            assert same and info.final_residual == info_f.final_residual and info.initial_residual == info_f.initial_residual and np.array_equal(u, u_f), (case, k)
            dx, dr = B.ref.drift(k)
            # k = N - 1 lies beyond the iterations of (a), one iteration before ||g|| <= 1e-11 ||b||.  The iterate's twin still holds there (<= 1.6e-15 in the five cases)
            # and is asserted as everywhere; the twin's residual NORM has left 1e-14 in all five (rounding of the recursive residual, eps ||g_0||, against ||g_k|| =
            # 1e-11 ||g_0||): Jacobi (N = 95) 6.4e-13, Chebyshev (22) 1.5e-13, FDM octant (22) 1.2e-14, FDM planar (19) 1.6e-14, two-level (37) 1.6e-10; the device is
            # 2.2e-12, 1.1e-6 (the lambda_max term: 2e-6), 1.7e-14, 3.9e-15 and 1.9e-10 from the reference there.  The residual
            # bound there is that of (a) plus 4 x this drift - the reference's own error, the factor that of the Chebyshev term
            check_iterate(f"history {case}", S, B, k, rc, info, u, (m + 1) * (k + 1) if m else k + 1, residual_slack=0.0 if k <= K_MAX else 4 * dr)
    finally:
        G.close()


# ---- (c) stopping -------------------------------------------------------------------------------------------------------------------------------------------------------------
def threshold(res, k):
    """a tolerance that ||g_k|| meets and no earlier residual does: the geometric mean of ||g_{k-1}|| and ||g_k||"""
    thr = float(np.sqrt(res[k - 1] * res[k]))
    assert res[k] < thr < min(res[:k]), ("the reference's residuals do not single out iteration", k, [float(r) for r in res[:k + 1]])
    return thr


def warm_start(S, B):
    """half the zero start's last iterate, with a ripple: ||g_0|| = ||A x0 - b|| is about half of ||b||, so the two stop rules give different tolerances"""
    i = np.arange(S.A.n)
    return np.where(S.free, 0.5 * B.ref.x[-1].astype(np.float64) * (1 + 0.05 * np.sin(0.3 * i)), 0.0)


def stopping_checks(tag, mesh_name, mode, prec, spec, kw, capture=capture_stderr):
    M = mesh(mesh_name); S = M.S
    solve_kw = dict(kw, prec=prec)
    G = context(M, mode)
    try:
        if spec[0] == "chebyshev":
            spec = spec + (printed_lambda_max(G, solve_kw, capture),)
        B = Bounds(M, spec)
        res = B.ref.res
        x0 = warm_start(S, B)
        Bw = Bounds(M, spec, x0)
        norm_b = float(np.linalg.norm(S.b))
        assert abs(Bw.ref.res[0] / norm_b - 1) > 0.1, "the warm start's residual must differ from ||b||, or the two stop rules cannot be told apart"

        def stopped(what, k, bounds, x_start, **tol):
            if x_start is None:
                G.fill(pk.VEC_U, 0.0)
            else:
                G.set(pk.VEC_U, x_start)
            rc, info = G.disp_solve(**dict(dict(abs_tol=1e-300, rel_tol=0.0, max_iter=1000), **tol), **solve_kw)
            u = G.get(pk.VEC_U)
            ex, ec = deviation(S, bounds.ref.x[k - 1], u)
            er = float(abs(info.final_residual - bounds.ref.res[k]) / bounds.ref.res[k])
            print(f"stop {tag} {what} k={k}: rc {rc} iterations {info.iterations} converged {info.converged}; iterate {ex:.2e} (bound {bounds.x(k):.2e}) residual {er:.2e}", flush=True)
            assert (rc, info.iterations, info.converged) == (0, k, 1), (tag, what, k, rc, info.iterations, info.converged)
            assert ex <= bounds.x(k) and ec <= BOUND and er <= bounds.r(k), (tag, what, k, ex, ec, er)
        for k in (1, 2, 5):
            stopped("abs_tol", k, B, None, abs_tol=threshold(res, k))
            stopped("abs_tol + cap", k, B, None, abs_tol=threshold(res, k), max_iter=k)                  # the tolerance test comes before the cap
            stopped("rel_tol x ||g_0|| (warm)", k, Bw, x0, rel_tol=threshold(Bw.ref.res, k) / float(Bw.ref.res[0]), reduction=True)
            stopped("rel_tol x ||b|| (warm)", k, Bw, x0, rel_tol=threshold(Bw.ref.res, k) / norm_b)
        # a start that already meets the tolerance: no iteration, x untouched
        for what, tol in (("abs_tol", dict(abs_tol=2 * float(Bw.ref.res[0]))), ("rel_tol x ||g_0||", dict(rel_tol=1.0, reduction=True)), ("rel_tol x ||b||", dict(rel_tol=2 * float(Bw.ref.res[0]) / norm_b))):
            G.set(pk.VEC_U, x0)
            rc, info = G.disp_solve(**dict(dict(abs_tol=1e-300, rel_tol=0.0, max_iter=1000), **tol), **solve_kw)
            u = G.get(pk.VEC_U)
            print(f"stop {tag} no iterations, {what}: rc {rc} iterations {info.iterations} converged {info.converged}, x untouched {np.array_equal(u[S.free], x0[S.free])}", flush=True)
            assert (rc, info.iterations, info.converged) == (0, 0, 1) and np.array_equal(u[S.free], x0[S.free]), (tag, what)
            assert abs(info.initial_residual - float(Bw.ref.res[0])) <= BOUND * float(Bw.ref.res[0]) and info.final_residual == info.initial_residual
    finally:
        G.close()


STOP_CASES = {"jacobi": ("oct_q2", pk.PREC_JACOBI, ("jacobi",), {}), "chebyshev_fused": ("oct_q2", pk.PREC_CHEBYSHEV, ("chebyshev", 4, 30.0), {"poly_degree": 4, "omega": 30.0}),
              "fdm_octant": ("oct_q2", pk.PREC_FDM, ("fdm",), {})}


@pytest.mark.parametrize("case", list(STOP_CASES))
def test_stopping_at_thresholds_from_the_reference(capfd, case):
    """(Jacobi on the single-reduction driver: in the child of test_driver_variants_in_child_processes)"""
    name, prec, spec, kw = STOP_CASES[case]
    stopping_checks(case, name, MF, prec, spec, kw, capture=capfd_capture(capfd))


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--variant"
    run_variant(sys.argv[2])

"""The CG ITERATES of real multi-rank runs against the long-double reference of tests/krylov_reference.py: W rank threads (tests/slab_ranks.py), every rank with a context
of its slab, run the capped solves disp_solve(max_iter=k) from a zero start together, for k = 1, 2, 3, 5, 8; the stitched iterate x_k and the returned ||g_k|| are compared
with kr.pcg_iterates on the single-rank system of the same box.  tests/test_krylov_iterates_gpu.py does this for the partitioned code path on ONE rank; only here does a dot
product meet a plane that two ranks hold, an exchange a neighbour, and the distributed fast diagonalisation its all-to-alls.

Bounds and conditions: those of tests/test_krylov_iterates_gpu.py, unchanged (tests/krylov_checks.py): 1e-12 relative for iterate and residual norm; a (case, k) takes part only
while the reference's fp64 twin is within 1e-14 of its long-double run, and none may drop out; Chebyshev: lambda_max from the PORO_CHEB_VERBOSE line - every rank must print the
same line - and the bound is 4 x the reference's own change under +- 5e-7, plus 1e-12.  Every rank must return the same return code, iteration count, residual norms and
operator applications, and the two copies of every shared plane of x_k must agree to 1e-13 max|x_k|.

Operator applications (poro_solve_info.operator_applications of every rank): k + 1 on the three-kernel recurrence (the slab form of the block FDM), k + 2 on the single-reduction
driver (Jacobi, the nodal distributed block FDM), (m + 1)(k + 1) with Chebyshev.  The apply_u_matrix_free (+ apply_u_chebyshev_fused) timers count the launches that were
ENQUEUED, those behind the finishing iteration included (the drivers enqueue batches and poll; a gated launch behind the end is a no-op, an ungated one of the single-reduction
driver is real work that is discarded), so they are asserted to be at least the figure above and equal on all ranks, and printed.

Shapes: Jacobi and Chebyshev (m = 4, ratio 30) on (4,3,7) Q2 on 3 ranks (3D slabs: the Chebyshev recurrence runs fused in the operator kernel with the plane fix-up
k_cheb_fix_planes) and 2D (6,9) Q2 on 2 ranks; block FDM in slab form on (4,3,7) on 3 (1 tile), (3,3,16) on 5 (2 tiles, both-parity z pass, 12 chunks, 3 per rank: the last share empty) and (10,9,24) on 3 (2 tiles,
planes of 8 chunks); block FDM in the nodal distributed form on 2D (6,9) on 3 ranks.  (3,3,16) stands in for the thin (3,2,24) of tests/test_slab_fdm_gpu.py: on that box
(cells of 3.3 x 5 x 0.42) the reference's fp64 twin leaves 1e-14 at k = 5 and 8 (1.1e-14, iterate), so it cannot take part; on (3,3,16) - the same tile count, chunk count and
empty share, cells of 3.3 x 3.3 x 0.63 - the twin stays within 5.8e-15.  Twins of the other boxes, worst over k (iterate): (4,3,7) Jacobi 1.5e-15, Chebyshev 3.8e-15, FDM
1.9e-15; (6,9) 8.5e-16, 4.3e-15, 1.5e-15; (10,9,24) FDM 5.0e-15.

Measured on one MI355X, worst over k of a family, iterate (relative to max|x_k|) / residual norm (relative to ||g_k||); every line of a run with -s shows its figures:
  Jacobi, single-reduction driver ((4,3,7) on 3; 2D (6,9) on 2)          1.5e-14 / 3.0e-15
  block FDM, slab form, three-kernel recurrence ((4,3,7); (3,3,16); (10,9,24))   1.2e-14 / 8.0e-15; 5.8e-14 / 1.4e-13; 8.3e-14 / 8.0e-14
  block FDM, nodal distributed form, single-reduction driver (2D (6,9) on 3)     1.6e-14 / 6.1e-15
  Chebyshev m = 4, ratio 30: iterate = 0.5 x ((4,3,7): fused kernel + plane fix-up; 7.0e-8 at k = 1) and 0.81 x (2D (6,9); 2.0e-7) the reference's own change under
             lambda_max +- 5e-7, an eighth and a fifth of the bound; residual norm <= 1.5e-7 and 1.6e-6.  lambda_max printed / true: 1.0496 and 1.0486, the same line on every rank.
  The two copies of every shared plane of x_k: bitwise equal in every case.  Operator launches enqueued / applications at k = 1 and 8: Jacobi and nodal FDM 4 / 3 and 11 / 10,
  slab FDM 5 / 2 and 11 / 9, Chebyshev 41 / 10 and 51 / 45.
No defect found.  The tests bite (scratch builds, not committed): (i) with one eigenvalue of the global last-direction table scaled by 1 + 1e-6 (tests/test_slab_fdm_gpu.py) the
four block-FDM cases fail from k = 1 (iterate 8e-11 .. 1.2e-9, residual norm 4e-11 .. 1.4e-9) and the Jacobi / Chebyshev cases pass.  (ii) with the owned-row dots of both CG
drivers (and the owned planes of the slab form) running over all local rows all eight cases fail at k = 1 (iterate 2e-3 .. 1e-1).  The existing multi-rank tests do NOT pass
under (ii): a dot that counts the shared planes twice no longer gives a convergent CG - 11 of the 14 tests of tests/test_multirank_gpu.py fail and
tests/test_rank_threads_gpu.py does not finish within its time limit - so that defect was visible before; under (i) they pass (see tests/test_slab_fdm_gpu.py)."""
import os
import re
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
import slab_ranks as sr
from krylov_checks import LAMBDA_LINE, Bounds, Env, capfd_capture, check_iterate, true_lambda_max

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8)
K_MAX = max(KS)


def pressure(n_p):
    return sr.rank_threads.REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(n_p)))      # (the right-hand side of tools/krylov_digest.py::u_inputs)


# ---- reference side: one entry per box, built at first use and only read afterwards ------------------------------------------------------------------------------------
class Box:
    def __init__(self, dim, n, deg):
        self.P = sr.problem(dim, n, deg)
        self.O = oracle_py.Oracle(self.P, hoisted=True)
        self.p = pressure(self.O.n_p)
        self.O.set(pk.VEC_P, self.p); self.O.disp_assemble_system(True)
        self.S = kr.displacement_system(self.P, self.O)
        self.refs, self.coarse, self.true_lmax = {}, None, None

    def close(self):
        self.O.close(); self.P.close()


_boxes = {}


def box(dim, n, deg):
    key = (dim, tuple(n), deg)
    if key not in _boxes:
        _boxes[key] = Box(dim, n, deg)
    return _boxes[key]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for B in _boxes.values():
        B.close()
    _boxes.clear()


# ---- device side ----------------------------------------------------------------------------------------------------------------------------------------------------------
def run_case(tag, dim, n, deg, world, prec, spec, kw, apps, slab_form, capture):
    """spec: the reference preconditioner, ("chebyshev", m, ratio) gets lambda_max from the ranks' printed lines; apps(k): operator applications; slab_form: True / False for
    the block FDM (asserted through the fdm_u_slab_z_stage timer), None otherwise"""
    M = box(dim, n, deg); Sy = M.S
    S = sr.Slabs(dim, n, deg, world)
    solve_kw = dict(kw, prec=prec)
    try:
        def on_rank(r, P, comm):
            G = sr.context(P, r, comm)
            try:
                G.set(pk.VEC_P, S.window_p(M.p, r)); G.disp_assemble_system(True)
                runs = []
                for k in KS:
                    G.fill(pk.VEC_U, 0.0); G.timers_reset()
                    rc, info = G.disp_solve(abs_tol=1e-300, rel_tol=0.0, max_iter=k, **solve_kw)
                    launched = G.timer("apply_u_matrix_free")[1] + G.timer("apply_u_chebyshev_fused")[1]
                    runs.append((rc, info, G.get(pk.VEC_U), launched, G.timer("fdm_u_slab_z_stage")[1]))
                return runs
            finally:
                G.close()
        with Env({"PORO_CHEB_VERBOSE": "1"} if spec[0] == "chebyshev" else {}):
            out, err = capture(lambda: S.run(on_rank))
        if spec[0] == "chebyshev":
            found = re.findall(LAMBDA_LINE, err)
            assert len(found) == world and len(set(found)) == 1, err          # the estimate is made once per context: every rank prints the same line
            lmax, true = float(found[0]), true_lambda_max(M)
            print(f"{tag}: lambda_max printed {lmax:.6f} on all {world} ranks, true {true:.6f} (ratio {lmax / true:.4f})")
            assert true * (1 - 1e-9) <= lmax <= 1.06 * true, (tag, lmax, true)
            spec = spec + (lmax,)
        B = Bounds(M, spec, K=K_MAX)
        worst = [0.0, 0.0]
        for i, k in enumerate(KS):
            rc, info = out[0][i][0], out[0][i][1]
            for r in range(world):                                                # replicated recurrences: every rank returns the same numbers
                rc_r, info_r, _, launched_r, stages_r = out[r][i]
                same = (rc_r, info_r.iterations, info_r.converged, info_r.initial_residual, info_r.final_residual, info_r.operator_applications) == \
                       (rc, info.iterations, info.converged, info.initial_residual, info.final_residual, info.operator_applications)
                assert same, (tag, k, r, info_r.as_dict(), info.as_dict())
                assert launched_r == out[0][i][3] and launched_r >= apps(k), (tag, k, r, launched_r, apps(k))
                if slab_form is not None:
                    assert (stages_r >= 1) if slab_form else (stages_r == 0), (tag, k, r, stages_r)
            parts = [out[r][i][2] for r in range(world)]
            u = S.stitch_u(parts)
            shared = max(float(np.abs(a - b).max()) for a, b in sr.shared_copies(parts, S.plane_u)) / float(np.abs(u).max())
            print(f"{tag} k={k}: shared planes {shared:.2e}; operator launches enqueued {out[0][i][3]} (applications {apps(k)})", flush=True)
            assert shared <= 1e-13, (tag, k, shared)
            check_iterate(tag, Sy, B, k, rc, info, u, apps(k), worst)
        print(f"{tag}: worst iterate deviation {worst[0]:.2e}, worst residual deviation {worst[1]:.2e}", flush=True)
    finally:
        S.close()


single = lambda k: k + 2      # noqa: E731
three = lambda k: k + 1       # noqa: E731
M_CHEB = 4
poly = lambda k: (M_CHEB + 1) * (k + 1)   # noqa: E731

JACOBI_CHEB_SHAPES = {"4x3x7_w3": (3, (4, 3, 7), 2, 3), "2d_6x9_w2": (2, (6, 9), 2, 2)}


@pytest.mark.parametrize("shape", list(JACOBI_CHEB_SHAPES))
def test_jacobi_iterates_on_ranks(capfd, shape):
    run_case(f"slab jacobi {shape}", *JACOBI_CHEB_SHAPES[shape], pk.PREC_JACOBI, ("jacobi",), {}, single, None, capfd_capture(capfd))


@pytest.mark.parametrize("shape", list(JACOBI_CHEB_SHAPES))
def test_chebyshev_iterates_on_ranks(capfd, shape):
    run_case(f"slab chebyshev {shape}", *JACOBI_CHEB_SHAPES[shape], pk.PREC_CHEBYSHEV, ("chebyshev", M_CHEB, 30.0), {"poly_degree": M_CHEB, "omega": 30.0}, poly, None, capfd_capture(capfd))


FDM_SHAPES = {"slab_4x3x7_w3": (3, (4, 3, 7), 2, 3, True), "slab_3x3x16_w5": (3, (3, 3, 16), 2, 5, True), "slab_10x9x24_w3": (3, (10, 9, 24), 2, 3, True), "nodal_2d_6x9_w3": (2, (6, 9), 2, 3, False)}


@pytest.mark.parametrize("shape", list(FDM_SHAPES))
def test_block_fdm_iterates_on_ranks(capfd, shape):
    dim, n, deg, world, slab = FDM_SHAPES[shape]
    run_case(f"slab fdm {shape}", dim, n, deg, world, pk.PREC_FDM, ("fdm",), {}, three if slab else single, slab, capfd_capture(capfd))

"""The stopping test of the block-FDM preconditioned displacement CG (single rank, octant and planar form) runs in front of the preconditioner call: the first transform
kernel sums the g . g partials of the residual update, and in the finishing iteration (converged, or max_iter reached) the whole call is skipped - the direction update's
finishing branch does x += alpha d and never reads z.  PORO_PCG_FINAL_PREC=1 puts the test back behind the preconditioner, which is the reference here.  g . g is the same
sum of the same partials in the same order and x sees the same update, so everything a solve reports is compared for exact equality.  The timer family
"fdm_u_final_prec_skipped" counts the solves whose finishing iteration skipped the call."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import REF, box_problem

pytestmark = pytest.mark.gpu

HOOK, GZ_HOOK, BUF_HOOK = "PORO_PCG_FINAL_PREC", "PORO_FDMO_SEPARATE_GZ", "PORO_FDMO_SEPARATE_BUFFERS"
FAMILY = "fdm_u_final_prec_skipped"
TIGHT = dict(abs_tol=1e-14, rel_tol=1e-12, max_iter=200, prec=pk.PREC_FDM)      # (as tests/test_fdm_u_buffers_gpu.py)
# Q2 boxes: 4^3 (half line 5: one tile, 64-thread workgroups), 6 x 5 x 4 (odd and even node counts), 17 x 4 x 4 (half line 18: two tiles); one 2D box (planar form)
SHAPES = [(3, (4, 4, 4)), (3, (6, 5, 4)), (3, (17, 4, 4)), (2, (6, 5))]


def _pressure(G, k):
    return REF["p_init"] * (1 + 0.3 * np.sin((0.37 + 0.5 * k) * np.arange(G.n_p) + k))


def _report(G, rc, info):
    return (rc, info.iterations, info.operator_applications, info.converged, info.final_residual, G.get(pk.VEC_U).copy())


def _solves(dim, n, precision, plan):
    """the solves of `plan` on one context: per solve what it reports and by how much the counter rose"""
    P = box_problem(dim, n, 2)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        G.set_fdm_precision(precision)
        out = []
        for rhs, start, opts in plan(G):
            if rhs is not None:
                G.set(pk.VEC_P, _pressure(G, rhs)); G.disp_assemble_system(True)
            if start == "zero":
                G.fill(pk.VEC_U, 0.0)
            before = G.timer(FAMILY)[1]
            rc, info = G.disp_solve(**opts(out) if callable(opts) else opts)
            out.append(_report(G, rc, info) + (G.timer(FAMILY)[1] - before,))
        return out
    finally:
        G.close(); P.close()


def _ab(monkeypatch, dim, n, plan, precision=pk.FDM_FP64, env=()):
    for h in (GZ_HOOK, BUF_HOOK):
        monkeypatch.delenv(h, raising=False)
    for h in env:
        monkeypatch.setenv(h, "1")
    monkeypatch.setenv(HOOK, "1")
    ref = _solves(dim, n, precision, plan)
    monkeypatch.delenv(HOOK)
    new = _solves(dim, n, precision, plan)
    for k, (a, b) in enumerate(zip(new, ref)):
        print(f"{dim}D cells {n} solve {k}: rc {a[0]}, {a[1]} iterations, {a[2]} operator applications, converged {a[3]}, final residual {a[4]:.17e}, skipped {a[6]} "
              f"(test behind the preconditioner: {b[0]}, {b[1]}, {b[2]}, {b[3]}, {b[4]:.17e}, {b[6]}), max|du| = {np.abs(a[5] - b[5]).max():.3e}")
        assert a[:5] == b[:5], (a[:5], b[:5])
        assert np.array_equal(a[5], b[5])
        assert b[6] == 0                                        # with the hook no solve counts
        assert a[6] == (1 if a[1] >= 1 else 0), (a[1], a[6])    # without it every solve that ran an iteration does
    return new


def _zero_then_warm(G):
    """zero start, then another right-hand side warm-started from the first solution: two consecutive solves on one context (the stored decision is cleared in between)"""
    return [(0, "zero", TIGHT), (1, "warm", TIGHT)]


@pytest.mark.parametrize("dim,n", SHAPES, ids=str)
def test_solves_bit_for_bit_like_the_test_behind_the_preconditioner(monkeypatch, dim, n):
    new = _ab(monkeypatch, dim, n, _zero_then_warm)
    assert all(s[0] == 0 and s[3] == 1 and s[1] > 1 for s in new)
    assert not np.array_equal(new[0][5], new[1][5])


def test_the_same_with_fp32_transforms(monkeypatch):
    new = _ab(monkeypatch, 3, (6, 5, 4), _zero_then_warm, precision=pk.FDM_FP32)
    assert all(s[0] == 0 and s[1] > 1 for s in new)


@pytest.mark.parametrize("hook", [GZ_HOOK, BUF_HOOK])
def test_the_same_with_the_other_hooks(monkeypatch, hook):
    """g . z by its own dot kernel (gated like the passes: it would read a z that was not computed); separate h, z and scratch arrays"""
    new = _ab(monkeypatch, 3, (6, 5, 4), _zero_then_warm, env=(hook,))
    assert all(s[0] == 0 and s[1] > 1 for s in new)


def test_a_solve_that_stops_at_iteration_one(monkeypatch):
    """a first solve capped at one iteration gives the residual after iteration 1; a tolerance between it and the initial residual then stops a solve there, converged"""
    def plan(G):
        cap = dict(TIGHT, max_iter=1)
        loose = lambda out: dict(abs_tol=0.5 * (out[0][4] + out[1][4]), rel_tol=0.0, max_iter=200, prec=pk.PREC_FDM)
        # (solve 0 reports the residual after one iteration, solve 1 - whose tolerance any start meets - the initial one)
        return [(0, "zero", cap), (None, "zero", dict(TIGHT, abs_tol=1e300)), (None, "zero", loose)]
    new = _ab(monkeypatch, 3, (6, 5, 4), plan)
    after_one, initial = new[0][4], new[1][4]
    assert new[0][1] == 1 and new[0][3] == 0 and new[0][0] == 1           # the cap: one iteration, not converged
    assert new[1][1] == 0 and new[1][3] == 1 and new[1][6] == 0           # any start meets abs_tol = 1e300: no iteration, the counter stays
    assert after_one < initial, (after_one, initial)
    assert new[2][1] == 1 and new[2][3] == 1 and new[2][0] == 0, new[2][:5]
    assert new[2][4] == after_one and np.array_equal(new[2][5], new[0][5])


def test_a_start_that_meets_the_tolerance(monkeypatch):
    """the second solve starts from the first one's solution with a looser tolerance: 0 iterations, x untouched, the counter unchanged"""
    def plan(G):
        return [(0, "zero", TIGHT), (None, "warm", dict(TIGHT, abs_tol=1e-6, rel_tol=1e-6))]
    new = _ab(monkeypatch, 3, (4, 4, 4), plan)
    assert new[1][1] == 0 and new[1][3] == 1 and new[1][0] == 0 and new[1][6] == 0
    assert np.array_equal(new[0][5], new[1][5])


def test_max_iter_on_a_solve_that_needs_more(monkeypatch):
    """the fail path: three iterations, not converged, the last preconditioner call skipped all the same; the next solve on the context converges (the decision is cleared)"""
    def plan(G):
        return [(0, "zero", dict(TIGHT, max_iter=3)), (None, "warm", TIGHT)]
    new = _ab(monkeypatch, 3, (6, 5, 4), plan)
    assert new[0][0] == 1 and new[0][1] == 3 and new[0][3] == 0 and new[0][6] == 1
    assert new[1][0] == 0 and new[1][3] == 1 and new[1][1] > 1

"""The stopping test in the first transform pass of the block-FDM preconditioned displacement CG, shared out over the four waves of a workgroup (each wave adds a quarter
of the g . g partials, the wave sums meet in LDS at the staging barrier), and the direction update reading the sum that workgroup 0 of that pass stored instead of adding the
partials up again.  PORO_PCG_STOP_PER_WAVE=1 and PORO_PCG_GG_RESUM=1 (read once per solve) restore the forms before: every wave sums all the partials, the direction update
sums them once more.  The additions and their order are the same, so everything a solve reports is compared for exact equality, with both hooks set as the reference and
against each hook alone.  Q2 boxes, smallest per workgroup shape of the pass (half line = cells + 1 entries along x):
  64 x 2 x 2 - half line 65, five tiles on four waves (the heavy-wave instruction streams);   48 x 2 x 2 - four tiles, four waves;
  32 x 2 x 2 - three tiles, three waves (no sharing: the per-wave form stays);                   6 x 6 x 6 - one tile, one wave;
  6 x 5 (2D) - the planar form, whose first GEMM kernel carries the test and stores the sum for its direction update (fp64 only: it has no fp32 transforms).
One plan per box: a stop at iteration 1 by the cap and by the tolerance, a start that meets the tolerance, a solve that runs into max_iter, consecutive solves; repeated with
the test behind the preconditioner (PORO_PCG_FINAL_PREC), with g . z from its own dot kernel (PORO_FDMO_SEPARATE_GZ) and with fp32 transforms.  Method as
tests/test_pcg_final_prec_gpu.py."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import REF, box_problem

pytestmark = pytest.mark.gpu

WAVE_HOOK, SUM_HOOK = "PORO_PCG_STOP_PER_WAVE", "PORO_PCG_GG_RESUM"
OTHER = ("PORO_PCG_FINAL_PREC", "PORO_FDMO_SEPARATE_GZ", "PORO_FDMO_SEPARATE_BUFFERS")
TIGHT = dict(abs_tol=1e-14, rel_tol=1e-12, max_iter=200, prec=pk.PREC_FDM)
BOXES = [(64, 2, 2), (48, 2, 2), (32, 2, 2), (6, 6, 6), (6, 5)]
_CACHE = {}


def _pressure(G, k):
    return REF["p_init"] * (1 + 0.3 * np.sin((0.37 + 0.5 * k) * np.arange(G.n_p) + k))


def _plan(out):
    """(right-hand side or None = keep, start, options); options may depend on the reports so far"""
    cap = dict(TIGHT, max_iter=1)
    loose = lambda out: dict(abs_tol=0.5 * (out[0][4] + out[1][4]), rel_tol=0.0, max_iter=200, prec=pk.PREC_FDM)
    return [(0, "zero", cap),                                   # 0: one iteration, stopped by the cap
            (None, "zero", dict(TIGHT, abs_tol=1e300)),         # 1: the start meets the tolerance: reports the initial residual
            (None, "zero", loose),                              # 2: a tolerance between the two: converged at iteration 1
            (1, "zero", dict(TIGHT, max_iter=3)),               # 3: runs into max_iter
            (None, "warm", TIGHT),                              # 4: goes on from there and converges
            (0, "warm", TIGHT)]                                 # 5: another right-hand side right behind it


def _solves(n, precision):
    P = box_problem(len(n), n, 2)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        G.set_fdm_precision(precision)
        out = []
        for rhs, start, opts in _plan(out):
            if rhs is not None:
                G.set(pk.VEC_P, _pressure(G, rhs)); G.disp_assemble_system(True)
            if start == "zero":
                G.fill(pk.VEC_U, 0.0)
            rc, info = G.disp_solve(**opts(out) if callable(opts) else opts)
            out.append((rc, info.iterations, info.operator_applications, info.converged, info.final_residual, G.get(pk.VEC_U).copy()))
        return out
    finally:
        G.close(); P.close()


def _with(monkeypatch, n, precision, env, hooks):
    """the plan's reports under the hooks `hooks` (on top of `env`); the reference (both hooks) is computed once per (box, precision, env)"""
    key = (n, precision, tuple(env), tuple(hooks))
    if key not in _CACHE:
        for h in OTHER + (WAVE_HOOK, SUM_HOOK):
            monkeypatch.delenv(h, raising=False)
        for h in tuple(env) + tuple(hooks):
            monkeypatch.setenv(h, "1")
        _CACHE[key] = _solves(n, precision)
    return _CACHE[key]


def _same(n, what, new, ref):
    for k, (a, b) in enumerate(zip(new, ref)):
        print(f"cells {n} {what} solve {k}: rc {a[0]}, {a[1]} iterations, {a[2]} operator applications, converged {a[3]}, final residual {a[4]:.17e} "
              f"(forms before: {b[0]}, {b[1]}, {b[2]}, {b[3]}, {b[4]:.17e}), max|du| = {np.abs(a[5] - b[5]).max():.3e}")
        assert a[:5] == b[:5], (k, a[:5], b[:5])
        assert np.array_equal(a[5], b[5]), k


def _shape_of_the_plan(s):
    assert s[0][1] == 1 and s[0][3] == 0 and s[0][0] == 1, s[0][:5]                    # the cap: one iteration, not converged
    assert s[1][1] == 0 and s[1][3] == 1, s[1][:5]                                     # no iteration
    assert s[0][4] < s[1][4]
    assert s[2][1] == 1 and s[2][3] == 1 and s[2][0] == 0 and s[2][4] == s[0][4], s[2][:5]     # converged at iteration 1, on the same residual
    assert np.array_equal(s[2][5], s[0][5])
    assert s[3][1] == 3 and s[3][3] == 0 and s[3][0] == 1, s[3][:5]                    # max_iter
    assert all(t[0] == 0 and t[3] == 1 and t[1] > 1 for t in s[4:]), [t[:5] for t in s[4:]]
    assert not np.array_equal(s[4][5], s[5][5])


@pytest.mark.parametrize("n", BOXES, ids=str)
def test_solves_bit_for_bit_like_the_forms_before(monkeypatch, n):
    ref = _with(monkeypatch, n, pk.FDM_FP64, (), (WAVE_HOOK, SUM_HOOK))
    new = _with(monkeypatch, n, pk.FDM_FP64, (), ())
    _same(n, "both new forms", new, ref)
    _shape_of_the_plan(new)
    for hook in (WAVE_HOOK, SUM_HOOK):                           # each part alone
        _same(n, f"with {hook}", _with(monkeypatch, n, pk.FDM_FP64, (), (hook,)), ref)


@pytest.mark.parametrize("env", OTHER[:2])
@pytest.mark.parametrize("n", BOXES, ids=str)
def test_the_same_with_the_other_hooks(monkeypatch, n, env):
    """the test behind the preconditioner (nothing of this runs: the reports must not move); g . z by its own dot kernel"""
    ref = _with(monkeypatch, n, pk.FDM_FP64, (env,), (WAVE_HOOK, SUM_HOOK))
    new = _with(monkeypatch, n, pk.FDM_FP64, (env,), ())
    _same(n, f"under {env}", new, ref)
    _shape_of_the_plan(new)


@pytest.mark.parametrize("n", [n for n in BOXES if len(n) == 3], ids=str)
def test_the_same_with_fp32_transforms(monkeypatch, n):
    ref = _with(monkeypatch, n, pk.FDM_FP32, (), (WAVE_HOOK, SUM_HOOK))
    new = _with(monkeypatch, n, pk.FDM_FP32, (), ())
    _same(n, "fp32 transforms", new, ref)
    assert new[0][1] == 1 and new[3][1] == 3 and all(t[3] == 1 for t in new[4:])

"""g.z of the block-FDM preconditioned displacement CG from the transform pass (single-rank octant form): pass 2 of `k_fdmo_pass` leaves the partial sums
of g.z = sum ghat^2 / den, `k_fdmo_update_d` adds them up, and no dot kernel runs.  PORO_FDMO_SEPARATE_GZ=1 restores the separate dot of the two octant
arrays, which is the reference here: same iteration counts, same solution, and the new sums are bitwise reproducible."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import REF, box_problem

pytestmark = pytest.mark.gpu

HOOK = "PORO_FDMO_SEPARATE_GZ"
# (cells, degree, abs_tol, rel_tol, bound on |u_a - u_b| / |u_b|): half lines of 7, 13, 21, 41, 73 and 50 entries = 1, 1, 2, 3, 5 and 4 MFMA tiles, with (Q2) and
# without (Q1, 100 nodes) a centre node; one box with unequal directions.  Tolerances and bounds as tests/test_fdm_u_gpu.py uses for the same solves.
CASES = [(6, 2, 1e-14, 1e-12, 1e-9), (12, 2, 1e-14, 1e-12, 1e-9), (20, 2, 1e-14, 1e-12, 1e-9), (40, 2, 1e-14, 1e-12, 1e-9), ((20, 12, 6), 2, 1e-14, 1e-12, 1e-9),
         (72, 2, 1e-12, 1e-10, 1e-7), (99, 1, 1e-12, 1e-10, 1e-7)]


def _solve(G, abs_tol, rel_tol):
    G.fill(pk.VEC_U, 0.0)
    rc, info = G.disp_solve(abs_tol=abs_tol, rel_tol=rel_tol, max_iter=200, prec=pk.PREC_FDM)
    return rc, info.iterations, G.get(pk.VEC_U).copy()


@pytest.mark.parametrize("n,deg,abs_tol,rel_tol,bound", CASES, ids=lambda v: str(v))
def test_gz_from_the_transform_pass_solves_like_the_separate_dot(monkeypatch, n, deg, abs_tol, rel_tol, bound):
    P = box_problem(3, n, deg)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        p = REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(G.n_p)))
        G.set(pk.VEC_P, p); G.disp_assemble_system(True)
        monkeypatch.setenv(HOOK, "1")
        rc_b, it_b, u_b = _solve(G, abs_tol, rel_tol)
        monkeypatch.delenv(HOOK)
        rc_a, it_a, u_a = _solve(G, abs_tol, rel_tol)
        rc_c, it_c, u_c = _solve(G, abs_tol, rel_tol)
        err = np.linalg.norm(u_a - u_b) / np.linalg.norm(u_b)
        print(f"cells {n} Q{deg}: iterations {it_a} (pass) / {it_b} (separate dot), |u_a - u_b| / |u_b| = {err:.3e}")
        assert rc_a == 0 and rc_b == 0 and rc_c == 0
        assert it_a == it_b, (it_a, it_b)
        assert err <= bound, err
        assert it_c == it_a and np.array_equal(u_c, u_a)       # the partial sums are added up in a fixed order
    finally:
        G.close(); P.close()


def test_time_step_traces_do_not_depend_on_where_gz_comes_from(monkeypatch):
    """whole time steps on the 4^3 box: identical fixed-stress / pressure iteration counts (columns 0-2) and displacement CG iterations (column 6)"""
    P = box_problem(3, 4, 2)
    try:
        traces = []
        for separate in (True, False):
            if separate:
                monkeypatch.setenv(HOOK, "1")
            else:
                monkeypatch.delenv(HOOK, raising=False)
            t, G = pk.run_problem(P, 3, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, max_it=500, prec=pk.PREC_FDM)
            traces.append(np.array(t, copy=True)); G.close()
        assert np.array_equal(traces[0][:, :3], traces[1][:, :3])
        assert np.array_equal(traces[0][:, 6], traces[1][:, 6])
    finally:
        P.close()

"""Strip form of the scalar fast-diagonalisation passes (kernels_fdmo.hip: k_fdmo_strip) and the one-launch sum-and-publish (kernels_la.hip: k_reduce_post).

The strip form shares a block of the Q1 transform passes out over several workgroups; every accumulator still sees its k-steps in the order of k_fdmo_pass, so results
must be BIT-identical to the block-per-workgroup form, which PORO_FDMO_SCALAR_STRIPS=0 (read when a context builds its table set) keeps.  Two contexts of the same box
in one process, one built with the hook: `dp` and the reported residual of pres_solve(PREC_FDM) and the solutions of proj_solve_many with 1, 2 and 3 right-hand sides
are compared with np.array_equal.  Shapes are vertices per line.

Independently one pressure solve per shape is compared with numpy.linalg.solve of the dense Jacobian a M + kappa K, M and K exported from a CSR context of the same
problem.  Bounds: rel2 <= 1e-9 against that solution and final <= 1e-12 x initial residual - the figures of tests/test_pressure_bc_fdm_gpu.py
(test_exact_inverse_of_the_free_block), which has them from test_parity_gpu.py::test_fast_diagonalisation_preconditioner.

Which form ran is read from the count-only timer family "fdm_q1_strip_launches".  Lines of one 16-wide tile ((2, 2, 2), (9, 5, 2)) have nothing to share out: both
contexts run the block form there, and so they do above the selection threshold (kFdmoStripFill x the CUs of the device, common.hpp).

Sum-and-publish: pres_assemble_residual and vec_norm return the doubles recorded from the commit before k_reduce_post existed
(tests/golden/q1_strips/sum_publish.npy; recorded there by `python3 tests/test_fdm_q1_strips_gpu.py --record tests/golden/q1_strips/sum_publish.npy`)."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import poroelasticity_dealii_amd as pk
from common import GOLDEN, csr_to_scipy, material

pytestmark = pytest.mark.gpu
DT = 60.0
HOOK = "PORO_FDMO_SCALAR_STRIPS"
FAMILY = "fdm_q1_strip_launches"
STORED = os.path.join(GOLDEN, "q1_strips", "sum_publish.npy")


def rel2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def rollers(dim):
    return [(2 * d, d, 0.0) for d in range(dim)]


def problem(shape, pbc=None, graded=False):
    n = [v - 1 for v in shape]                     # cells of edge 1: a M and kappa K of comparable size
    if graded:
        P = pk.Problem.graded_box(3, n, [float(m) for m in n], 1, material(), rollers(3), [0.6, 0.0, 0.9])
    else:
        P = pk.Problem.box(3, n, [float(m) for m in n], 1, material(), rollers(3))
    return P.set_pressure_bc(pbc) if pbc else P


def rhs_for(n_p):
    return np.random.default_rng(4321 + n_p).standard_normal(n_p)


# id -> (vertices per line, prescribed faces, graded tensor grid)
CASES = {
    "2x2x2": ((2, 2, 2), None, False),                      # minimum size (one tile: block form in both contexts)
    "9x5x2": ((9, 5, 2), None, False),                      # the shape of tools/fdm_digest.py (one tile)
    "16x17x33": ((16, 17, 33), None, False),                # 1, 2 and 3 tiles in one box; 272 plane positions = 17 chunks of 16; 33 planes
    "73x9x9": ((73, 9, 9), None, False),                    # five tiles in x only: strips without valid outputs in pass 3, a partial last chunk (657 = 41 x 16 + 1)
    "9x9x73": ((9, 9, 73), None, False),                    # five tiles in z only: passes 1 / 3 have one strip of work per block
    "81x5x5": ((81, 5, 5), None, False),                    # six tiles: more than 64 KB of dynamic LDS in passes 1 / 3
    "16x17x33-top": ((16, 17, 33), [(5, 0.0)], False),      # removed modes (lam = inf): the second table set, one whole face
    "16x17x33-both-x": ((16, 17, 33), [(0, 0.0), (1, 0.0)], False),   # a pair of opposite faces
    "16x17x33-graded": ((16, 17, 33), None, True),          # tensor grid: CG preconditioned by the passes instead of the direct solve
}
ABOVE = (41, 41, 35)      # 3 x 35 planes = 105 and 3 x ceil(1681 / 48) = 108 workgroups per launch of the batched projection solve: not below 0.4 x 256 CUs = 102.4


def run(case, hook):
    """everything the comparisons need from one context; hook: PORO_FDMO_SCALAR_STRIPS=0 while the context lives"""
    shape, pbc, graded = CASES[case] if case in CASES else (case, None, False)
    big = case not in CASES
    old = os.environ.pop(HOOK, None)
    if hook:
        os.environ[HOOK] = "0"
    P = problem(shape, pbc, graded)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    out = {}
    try:
        G.timers_reset()
        if not big:
            G.set(pk.VEC_RESIDUAL_P, rhs_for(G.n_p)); G.fill(pk.VEC_DP, 0.0); G.pres_assemble_jacobian(DT)
            rc, info = G.pres_solve(rel_tol=1e-8, prec=pk.PREC_FDM)
            out["pres"] = (rc, info.iterations, info.converged, info.initial_residual, info.final_residual, G.get(pk.VEC_DP))
            out["strips_pres"] = G.timer(FAMILY)[1]
        G.set(pk.VEC_U, 1e-5 * np.sin(0.05 * np.arange(G.n_u)))
        G.proj_assemble_matrix(); G.proj_assemble_rhs([0, 4, 8])
        for entries in ([0, 3, 5],) if big else ([0], [0, 3], [0, 3, 5]):
            for e in entries:
                G.fill(pk.VEC_STRAIN0 + e, 0.0)
            rc, infos = G.proj_solve_many(entries, rel_tol=1e-8, prec=pk.PREC_FDM)
            out[len(entries)] = (rc, [(i.iterations, i.converged, i.initial_residual, i.final_residual) for i in infos], [G.get(pk.VEC_STRAIN0 + e) for e in entries])
        out["strips"] = G.timer(FAMILY)[1]
    finally:
        G.close(); P.close()
        os.environ.pop(HOOK, None)
        if old is not None:
            os.environ[HOOK] = old
    return out


_runs = {}


def both(case):
    if case not in _runs:
        _runs[case] = (run(case, hook=True), run(case, hook=False))
    return _runs[case]


def tiles(shape):
    return max((v + 15) // 16 for v in shape)


@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_pressure_solve_keeps_its_bits(case):
    block, strip = both(case)
    shape = CASES[case][0]
    print(f"{case}: strip launches {strip['strips_pres']} (block-form context: {block['strips_pres']}), iterations {strip['pres'][1]}, residual {strip['pres'][4]:.3e} / {strip['pres'][3]:.3e}")
    assert block["strips_pres"] == 0
    assert (strip["strips_pres"] > 0) == (tiles(shape) >= 2)           # one right-hand side: at most 73 workgroups in the block form, below the threshold
    if tiles(shape) >= 2 and not CASES[case][2]:
        assert strip["strips_pres"] == 3                                # one direct solve: all three passes
    assert strip["pres"][:5] == block["pres"][:5]                       # return code, iterations, converged, initial and final residual: the same doubles
    assert strip["pres"][0] == 0 and strip["pres"][2] == 1
    assert np.array_equal(strip["pres"][5], block["pres"][5])


@pytest.mark.parametrize("nrhs", [1, 2, 3])
@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_projection_solves_keep_their_bits(case, nrhs):
    block, strip = both(case)
    assert block["strips"] == 0
    assert strip[nrhs][0] == 0 and strip[nrhs][:2] == block[nrhs][:2]
    assert all(it == 0 and conv == 1 for it, conv, _, _ in strip[nrhs][1]) or CASES[case][2]      # (tensor grids have no direct path)
    for a, b in zip(strip[nrhs][2], block[nrhs][2]):
        assert np.any(a != 0.0) and np.array_equal(a, b)


_dense = {}


@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][1] is None and not CASES[c][2]], ids=str)
def test_pressure_solve_against_a_dense_solve(case):
    shape = CASES[case][0]
    if shape not in _dense:
        P = problem(shape)
        C = pk.Context(P, 0, pk.OP_CSR)
        try:
            M = csr_to_scipy(*C.export_csr(pk.MAT_MASS_P)); K = csr_to_scipy(*C.export_csr(pk.MAT_LAPLACE_P))
        finally:
            C.close(); P.close()
        m = material()
        x = np.linalg.solve((M / (m.biot_M * DT) + m.k_over_mu * K).toarray(), rhs_for(M.shape[0]))
        x.setflags(write=False)
        _dense[shape] = x
    _, strip = both(case)
    rc, its, conv, r0, r1, x = strip["pres"]
    print(f"{case}: rel2 {rel2(x, _dense[shape]):.3e}, residual {r1:.3e} / {r0:.3e}")
    assert rc == 0 and conv == 1 and its == 0
    assert r1 <= 1e-12 * r0
    assert rel2(x, _dense[shape]) <= 1e-9


def test_block_form_above_the_threshold():
    """a batched projection solve whose three block-form launches each start more workgroups than the threshold (kFdmoStripFill x CUs, MI355X: 256): no strip launch with or
    without the hook"""
    block, strip = both(ABOVE)
    assert block["strips"] == 0 and strip["strips"] == 0
    assert strip[3][0] == 0 and strip[3][:2] == block[3][:2] and all(it == 0 and conv == 1 for it, conv, _, _ in strip[3][1])
    for a, b in zip(strip[3][2], block[3][2]):
        assert np.any(a != 0.0) and np.array_equal(a, b)


# ---- sum and publish in one launch ---------------------------------------------------------------------------------------------------------------
SUM_SHAPES = ((9, 5, 2), (16, 17, 33))


def sum_publish_values():
    """per shape: the residual norm of pres_assemble_residual, then (l2, linf) of the residual, of p and of u"""
    vals = []
    for shape in SUM_SHAPES:
        P = problem(shape)
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        try:
            i = np.arange(G.n_p)
            p = 1e5 * (1 + 0.1 * np.sin(0.37 * i))
            G.set(pk.VEC_P_OLD, p); G.set(pk.VEC_P, 1.01 * p + 3.0 * np.cos(0.11 * i))
            G.set(pk.VEC_EPSV0, 1e-6 * np.sin(0.05 * i)); G.set(pk.VEC_EPSV, 1.1e-6 * np.sin(0.05 * i + 0.2))
            G.set(pk.VEC_U, 1e-5 * np.sin(0.05 * np.arange(G.n_u)))
            vals.append(G.pres_assemble_residual(DT))
            for which in (pk.VEC_RESIDUAL_P, pk.VEC_P, pk.VEC_U):
                vals.extend(G.norm(which))
        finally:
            G.close(); P.close()
    return np.array(vals)


def test_sum_and_publish_returns_the_recorded_doubles():
    got, want = sum_publish_values(), np.load(STORED)
    print(got)
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(got[::7] > 0.0)
    assert np.array_equal(got, want)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        v = sum_publish_values()
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        np.save(sys.argv[2], v)
        print(v)
    else:
        sys.exit("usage: test_fdm_q1_strips_gpu.py --record FILE.npy")

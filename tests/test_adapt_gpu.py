"""Mesh adaptation on the device and in the drivers (refine_mesh, PoroelasticityFSS.h:333-340, 447-498): the transfer of the pressure-space vectors between two
contexts, Runner.adapt / run_problem(refine_every=...) end to end, and poro_run --refine-every."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, BC_3D, INPUT_DATA, REF, material
from test_adapt_cpu import conforming, mark_numpy, masked, overlapping_masks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")


# ---- 9. transfer between two contexts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(2, (4, 3)), (3, (3, 3, 2))], ids=str)
def test_transfer_between_contexts(dim, n):
    ma, mb = overlapping_masks(n); zero = np.zeros_like(ma)
    rng = np.random.default_rng(5 + dim)
    n_sym = dim * (dim + 1) // 2
    for m_old, m_new in ((zero, ma), (ma, mb), (mb, zero)):
        Po, Pn = masked(dim, n, 1, m_old), masked(dim, n, 1, m_new)
        Go, Gn = pk.Context(Po, 0, pk.OP_CSR), pk.Context(Pn, 0, pk.OP_CSR)
        try:
            n_old, n_new = Po.desc.n_dofs_p, Pn.desc.n_dofs_p
            ids = (pk.VEC_P, pk.VEC_EPSV, pk.VEC_EPSV0)
            old = [conforming(Po, lambda X: rng.standard_normal(len(X)) * s) for s in (1e7, 1e-6, 3.0)]
            for which, v in zip(ids, old):
                Go.set(which, v)
            ptr, node, w = Po.transfer_rows_p(Pn)
            Gn.transfer_p_from(Go, (ptr, node, w))
            kept = np.diff(ptr) == 1
            assert kept.any() and (~kept).any() == bool(np.any((m_new != 0) & (m_old == 0)))     # new vertices appear exactly where something is newly refined
            for which, v in zip(ids, old):
                got = Gn.get(which)
                want = np.array([w[ptr[i]:ptr[i + 1]] @ v[node[ptr[i]:ptr[i + 1]]] for i in range(n_new)])
                assert np.abs(got - want).max() <= 1e-14 * np.abs(v).max()
                assert np.array_equal(got[kept], v[node[ptr[:-1][kept]]])                         # a kept vertex: the same bits
                assert np.array_equal(Go.get(which), v)                                           # `from` is only read
            zeros = [pk.VEC_U, pk.VEC_RHS_U, pk.VEC_DP, pk.VEC_P_OLD, pk.VEC_RESIDUAL_P] + [pk.VEC_STRAIN0 + e for e in range(n_sym)] + [pk.VEC_STRESS0 + e for e in range(n_sym)]
            for which in zeros:
                assert not Gn.get(which).any(), which
            # malformed rows: refused on the host, `to` stays as it is
            before = [Gn.get(which) for which in ids]
            bad_first = ptr.copy(); bad_first[0] = 1
            bad_order = ptr.copy(); bad_order[n_new // 2] = bad_order[n_new // 2 + 1] + 1
            bad_node = node.copy(); bad_node[len(node) // 2] = n_old
            neg_node = node.copy(); neg_node[0] = -1
            for rows in ((bad_first, node, w), (bad_order, node, w), (ptr, bad_node, w), (ptr, neg_node, w)):
                with pytest.raises(RuntimeError) as e:
                    Gn.transfer_p_from(Go, rows)
                assert "poro_state_transfer_p" in str(e.value)
                for which, b in zip(ids, before):
                    assert np.array_equal(Gn.get(which), b)
            with pytest.raises(RuntimeError):
                Gn.transfer_p_from(Gn, (ptr, node, w))
        finally:
            Go.close(); Gn.close(); Po.close(); Pn.close()


# ---- 10. end to end ---------------------------------------------------------------------------------------------------------------------------------
CASES = {"2d_q2": (2, (8, 8), 2), "3d_q1": (3, (4, 4, 4), 1)}
CONTROLS = dict(p_init=REF["p_init"], dt=REF["dt"], prec=-1)        # prec = -1: the strongest preconditioner the mesh supports (poro_run --fastest)


def start(case):
    dim, n, deg = CASES[case]
    return masked(dim, n, deg, np.zeros(int(np.prod(n)), dtype=np.int32))


def python_steps(G, first_step, n_steps, dt):
    """PoroElasticProblem::time_step through the C-ABI entry points, with the preconditioner choice of initialize(): what the runner does after an adapt, restated"""
    dim = G.dim
    prec_u = pk.PREC_FDM if G.supports_preconditioner(0, pk.PREC_FDM) else pk.PREC_TWO_LEVEL if G.supports_preconditioner(0, pk.PREC_TWO_LEVEL) else pk.PREC_CHEBYSHEV
    prec_proj = pk.PREC_FDM if G.supports_preconditioner(1, pk.PREC_FDM) else pk.PREC_JACOBI
    prec_p = pk.PREC_TWO_LEVEL if (prec_proj == pk.PREC_JACOBI and G.n_p >= 4096 and G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)) else prec_proj
    comps = [0, 3] if dim == 2 else [0, 4, 8]; entries = [0, 2] if dim == 2 else [0, 3, 5]
    G.disp_assemble_system(True); G.proj_assemble_matrix()             # PoroelasticityFSS.h:338-339
    rows = []
    for step in range(first_step, first_step + n_steps):
        G.copy(pk.VEC_P_OLD, pk.VEC_P)
        err, fss = 2e-8, 0
        while fss < 50 and err > 1e-8:
            fss += 1; it = 0; pcg = 0
            G.fill(pk.VEC_DP, 0.0)
            while it < 50:
                it += 1
                G.pres_update_volumetric_strain()
                err = inner = G.pres_assemble_residual(dt)
                if err < 1e-8:
                    break
                G.pres_assemble_jacobian(dt)
                rc, info = G.pres_solve(prec=prec_p); assert rc == 0
                pcg += info.iterations
                G.axpy(pk.VEC_P, 1.0, pk.VEC_DP)
            pinf = G.norm(pk.VEC_P)[1]
            G.disp_assemble_system(False)
            rc, info_u = G.disp_solve(prec=prec_u); assert rc == 0
            G.proj_assemble_rhs(comps)
            rc, _ = G.proj_solve_many(entries, prec=prec_proj); assert rc == 0
            err = G.pres_assemble_residual(dt)
            rows.append([step, fss, it - 1, inner, pinf, err, info_u.iterations, pcg])
    return np.array(rows), prec_u


@pytest.mark.parametrize("case", list(CASES))
def test_runner_adapt_end_to_end(case):
    P = start(case)
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, **CONTROLS)
    G2 = None
    try:
        R.initialize()
        for _ in range(4):
            R.step()
        # (a) the new mask is what the marking rule makes of the indicator the device returns
        eta = R.ctx.pres_estimate_error()
        coarse, child = R.problem.cell_parents()
        want = mark_numpy(eta, R.problem.refine_mask(), coarse, child, 2 ** P.desc.dim, 0.6, 0.4)
        before, after = R.adapt()
        assert R.problem.handle.value != P.handle.value and before == P.desc.n_cells and after == R.problem.desc.n_cells
        mask1 = R.problem.refine_mask()
        print(case, "cells", before, "->", after, "refined coarse cells", int(mask1.sum()), "eta max", eta.max())
        assert np.array_equal(mask1, want) and mask1.any() and after > before
        assert R.ctx.n_p == R.problem.desc.n_dofs_p and not R.ctx.get(pk.VEC_U).any()              # the displacement warm start is lost, as in the reference
        # (b) a fresh context on the new mesh, given the three transferred vectors, takes the same two steps: adapt() leaves no hidden state behind
        state = [R.ctx.get(w) for w in (pk.VEC_P, pk.VEC_EPSV, pk.VEC_EPSV0)]
        G2 = pk.Context(R.problem, 0, pk.OP_MATRIX_FREE)
        for w, v in zip((pk.VEC_P, pk.VEC_EPSV, pk.VEC_EPSV0), state):
            G2.set(w, v)
        t_runner = np.vstack([R.step()[0] for _ in range(2)])
        t_fresh, prec_u = python_steps(G2, 5, 2, REF["dt"])
        # (c) both steps converged (a step that does not raises), with the preconditioner --fastest picks on a mesh with hanging nodes
        assert prec_u == pk.PREC_TWO_LEVEL and np.isfinite(t_runner).all() and list(t_runner[:, 0]) == sorted(t_runner[:, 0]) and t_runner[-1, 0] == 6
        assert np.array_equal(t_runner, t_fresh), (t_runner, t_fresh)
        for w in (pk.VEC_U, pk.VEC_P):
            a, b = R.ctx.get(w), G2.get(w)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
        # (d) a second adapt: a refined -> refined transfer, and the runner still steps
        p_before = R.ctx.get(pk.VEC_P)
        R.adapt()
        mask2 = R.problem.refine_mask()
        print(case, "second adapt: refined coarse cells", int(mask2.sum()))
        assert np.isfinite(R.ctx.get(pk.VEC_P)).all() and abs(R.ctx.get(pk.VEC_P).mean() - p_before.mean()) <= 1e-3 * abs(p_before.mean())
        t7, _ = R.step()
        assert t7[-1, 0] == 7 and np.isfinite(t7).all()
    finally:
        if G2 is not None:
            G2.close()
        R.close(); P.close()


@pytest.mark.parametrize("case", list(CASES))
def test_run_problem_with_refine_every(case):
    """(e) run() with refine_every = 3 over 6 steps = the runner with adapts before steps 3 and 6; (f) refine_every = 0 = the run without adaptation, bit for bit"""
    P = start(case)
    try:
        kw = dict(operator_mode=pk.OP_MATRIX_FREE, prec=-1)
        R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, **CONTROLS)
        try:
            R.initialize()
            manual = []
            for step in range(1, 7):
                if step % 3 == 0:
                    R.adapt()
                manual.append(R.step()[0])
            manual = np.vstack(manual)
            final_mask = R.problem.refine_mask(); p_manual = R.ctx.get(pk.VEC_P)
        finally:
            R.close()
        trace, G = pk.run_problem(P, 6, REF["p_init"], REF["dt"], refine_every=3, **kw)
        try:
            assert G.problem is not P and np.array_equal(G.problem.refine_mask(), final_mask) and final_mask.any()
            assert np.array_equal(trace[1:], manual), (trace, manual)
            assert np.array_equal(G.get(pk.VEC_P), p_manual)
        finally:
            G.close(); G.problem.close()
        t0, G0 = pk.run_problem(P, 3, REF["p_init"], REF["dt"], refine_every=0, **kw)
        t1, G1 = pk.run_problem(P, 3, REF["p_init"], REF["dt"], **kw)                     # the unchanged poro_host_run
        try:
            assert G0.problem is P and np.array_equal(t0, t1) and np.array_equal(G0.get(pk.VEC_P), G1.get(pk.VEC_P)) and np.array_equal(G0.get(pk.VEC_U), G1.get(pk.VEC_U))
        finally:
            G0.close(); G1.close()
    finally:
        P.close()


def test_run_with_refine_every_needs_a_refined_box():
    B = pk.Problem.box(2, (4, 4), [10.0, 10.0], 1, material(), BC_2D)
    try:
        with pytest.raises(RuntimeError) as e:
            pk.run_problem(B, 2, REF["p_init"], REF["dt"], refine_every=2)
        assert "refined box" in str(e.value)
        R = pk.Runner(B, 0, pk.OP_CSR)
        try:
            R.initialize()
            with pytest.raises(RuntimeError):
                R.adapt()
            R.step()                                                                      # the runner is still whole
        finally:
            R.close()
    finally:
        B.close()


# ---- 11. the driver executable -------------------------------------------------------------------------------------------------------------------------
def test_poro_run_refine_every(tmp_path):
    out_dir = tmp_path / "solution"; out_dir.mkdir()
    r = subprocess.run([EXE, INPUT_DATA, "--matrix-free", "--fastest", "--refine-every", "2", "--steps", "3", "--output", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(re.findall(r"Time: ", r.stdout)) == 3
    cells = []
    for k in (1, 2, 3):
        m = re.search(r"^CELLS (\d+) ", (out_dir / f"solution-{k:04d}.vtk").read_text(), re.M)
        cells.append(int(m.group(1)))
    print("cells per step", cells)
    assert cells[1] != cells[0] and cells[2] == cells[1]                                  # the mesh changes at step 2 (and only there)
    r = subprocess.run([EXE, INPUT_DATA, "--refine-every", "2", "--mesh", os.path.join(ROOT, "tests", "golden", "domain.msh")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "boxes only" in r.stderr

"""The pressure Newton loop as gated batches (poro_pres_newton_loop) against the per-call loop, which the hook PORO_PRES_HOST_LOOP (read once per context) restores.
Everything is compared bit for bit: the batch enqueues the kernels of the per-call sequence in its order, a device-side test in place of every host decision.

Shapes: the smallest boxes at which the kernels can go wrong - 2 x 2 x 2 cells (every node on the boundary but one), 5 x 4 x 3 and 9 x 5 x 2 (non-cubic, odd and even
extents) and 6 x 5 cells in 2D (no batch there: the scalar passes have no gated form in 2D).  The benchmark's --dump-outputs comparison covers the benchmark size."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import REF, box_problem

pytestmark = pytest.mark.gpu
HOOK = "PORO_PRES_HOST_LOOP"
FAMILY = "pressure_newton_batched"
BOXES = [(3, (2, 2, 2)), (3, (5, 4, 3)), (3, (9, 5, 2)), (2, (6, 5))]
DT = REF["dt"]


def contexts(monkeypatch, P):
    """(default, hook) contexts of P"""
    monkeypatch.delenv(HOOK, raising=False)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    monkeypatch.setenv(HOOK, "1")
    H = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    monkeypatch.delenv(HOOK)
    return G, H


def seed_state(ctxs, seed):
    """a non-trivial p, p_old and strains, the same in every context"""
    rng = np.random.default_rng(seed)
    n = ctxs[0].get(pk.VEC_P).size
    p_old = REF["p_init"] * (1.0 + 0.05 * rng.standard_normal(n))
    p = p_old + 2.0e4 * rng.standard_normal(n)
    ev0 = 1.0e-5 * rng.standard_normal(n)
    ev = ev0 + 3.0e-6 * rng.standard_normal(n)
    for G in ctxs:
        for v, a in ((pk.VEC_P, p), (pk.VEC_P_OLD, p_old), (pk.VEC_EPSV, ev), (pk.VEC_EPSV0, ev0)):
            G.set(v, a)
        G.fill(pk.VEC_DP, 0.0)


@pytest.mark.parametrize("dim,n", BOXES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_gated_stencil_kernels_against_the_csr_operators(monkeypatch, dim, n):
    """The residual and Jacobian stencil kernels carry the batch's gate now (null outside a batch).  Against the assembled matrices of a PORO_OP_CSR context of the same
    box (other kernels, other order of additions): the residual, and J dp = R for the dp of the checked direct solve.
    Bounds: a row is 3^dim products of magnitude <= max |K p| ~ max |R| each, summed in fp64 in two different orders: a few 27 * 2^-53 ~ 3e-15 of max |R| per
    entry; 1e-12 max |R| leaves two orders for the cancellation inside a row.  J dp = R: the direct solve's own check holds it to 1e-8 |R| in the 2-norm (the reference's
    stopping rule), so the CSR product of the same dp is within 1e-8 |R|_2 + 1e-12 max |R| sqrt(n) of R"""
    P = box_problem(dim, n, 2)
    monkeypatch.delenv(HOOK, raising=False)
    G, A = pk.Context(P, 0, pk.OP_MATRIX_FREE), pk.Context(P, 0, pk.OP_CSR)
    try:
        seed_state((G, A), 11 + sum(n))
        l2 = [C.pres_assemble_residual(DT) for C in (G, A)]
        R = [C.get(pk.VEC_RESIDUAL_P) for C in (G, A)]
        scale = np.abs(R[1]).max()
        print("l2", l2, "max |R|", scale, "max difference", np.abs(R[0] - R[1]).max())
        assert scale > 0 and np.abs(R[0] - R[1]).max() <= 1e-12 * scale
        assert l2[0] == pytest.approx(np.linalg.norm(R[0]), rel=1e-12)
        assert G.supports_preconditioner(1, pk.PREC_FDM)
        G.pres_assemble_jacobian(DT); A.pres_assemble_jacobian(DT)
        rc, info = G.pres_solve(prec=pk.PREC_FDM)
        dp = G.get(pk.VEC_DP)
        assert rc == 0 and info.iterations == 0 and info.converged == 1 and np.abs(dp).max() > 0      # the direct solve, checked
        assert info.initial_residual == pytest.approx(np.linalg.norm(R[0]), rel=1e-12) and info.final_residual <= 1e-8 * info.initial_residual
        err = np.linalg.norm(A.pres_apply_jacobian(dp) - R[0])
        print("|J_csr dp - R|", err, "reported", info.final_residual)
        assert err <= 1e-8 * np.linalg.norm(R[0]) + 1e-12 * scale * np.sqrt(R[0].size)
    finally:
        G.close(); A.close(); P.close()


def run_steps(monkeypatch, P, hook, steps=4, restore=False, solver_rel_tol=None, **kw):
    if hook:
        monkeypatch.setenv(HOOK, "1")
    else:
        monkeypatch.delenv(HOOK, raising=False)
    probe = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    prec = pk.PREC_FDM if probe.supports_preconditioner(0, pk.PREC_FDM) else pk.PREC_JACOBI       # block FDM where the box supports it
    probe.close()
    R = pk.Runner(P, operator_mode=pk.OP_MATRIX_FREE, p_init=REF["p_init"], dt=DT, max_it=2000, prec=prec, **kw)
    try:
        if solver_rel_tol is not None:
            R.set_pressure_solver_tolerances(0.0, solver_rel_tol)
        R.initialize()
        if restore:
            R.save_state()
        traces = [np.array(R.step(restore=restore and s > 0)[0], copy=True) for s in range(steps)]
        return dict(traces=traces, vecs=[R.ctx.get(v).copy() for v in (pk.VEC_U, pk.VEC_P, pk.VEC_EPSV)], work=R.work(), batched=R.ctx.timer(FAMILY)[1],
                    prec_p=R.preconditioners()[1])
    finally:
        R.close()
        monkeypatch.delenv(HOOK, raising=False)


def same_run(a, b):
    assert len(a["traces"]) == len(b["traces"])
    for s, t in zip(a["traces"], b["traces"]):
        assert s.shape == t.shape and s.shape[0] > 0 and np.array_equal(s, t), (s, t)      # all eight columns
    for x, y in zip(a["vecs"], b["vecs"]):
        assert np.array_equal(x, y)
    wa, wb = dict(a["work"]), dict(b["work"])
    wa.pop("usec_solve_u"); wb.pop("usec_solve_u")      # a wall time
    assert wa == wb, (wa, wb)


@pytest.mark.parametrize("n", [(4, 4, 4), (5, 4, 3)], ids=lambda v: "x".join(map(str, v)))
def test_four_steps_equal_the_per_call_loop(monkeypatch, n):
    """fss_tol = 0 with three fixed-stress iterations per step: the first one takes its pressure iterations (more than one batch holds: the gate is still open behind the
    first), the second and third start from the residual the first one closed with, which is below the tolerance already - the gate closes at the first test and a
    prediction (hint slots 1 and 2, from the second step on) says so"""
    P = box_problem(3, n, 2)
    try:
        kw = dict(fss_tol=0.0, max_fss=3)
        a, b = run_steps(monkeypatch, P, False, **kw), run_steps(monkeypatch, P, True, **kw)
        print([t[:, 2].tolist() for t in a["traces"]], [t[:, 3].tolist() for t in a["traces"]])
        assert a["prec_p"] == pk.PREC_FDM
        assert a["batched"] == 4 and b["batched"] == 0
        its = np.concatenate([t[:, 2] for t in b["traces"]])
        assert its.max() >= 2 and its.min() == 0 and all(t.shape[0] == 3 for t in b["traces"])
        same_run(a, b)
    finally:
        P.close()


@pytest.mark.parametrize("case", ["max_pres_1", "max_pres_2", "restore", "per_cell_permeability"])
def test_caps_restore_and_ineligible_contexts(monkeypatch, case):
    P = box_problem(3, (4, 4, 4), 2)
    try:
        kw = dict(steps=2)
        if case.startswith("max_pres"):
            kw.update(max_pres=int(case[-1]), max_fss=6)      # the cap falls inside a batch
        if case == "restore":
            kw.update(steps=3, restore=True)                  # the same step three times: the restore clears the prediction every time
        if case == "per_cell_permeability":
            nc = 64
            kw.update(permeability=material_k() * (1.0 + 0.5 * np.sin(np.arange(nc))))
        a, b = run_steps(monkeypatch, P, False, **kw), run_steps(monkeypatch, P, True, **kw)
        assert b["batched"] == 0 and a["batched"] == (0 if case == "per_cell_permeability" else kw["steps"])
        same_run(a, b)
        if case == "restore":
            assert all(np.array_equal(a["traces"][0], t) for t in a["traces"][1:])
    finally:
        P.close()


@pytest.mark.parametrize("n", [(4, 4, 4), (5, 4, 3)], ids=lambda v: "x".join(map(str, v)))
def test_runs_whose_direct_checks_fail_go_on_to_cg_like_the_per_call_loop(monkeypatch, n):
    """A pressure solver tolerance of 1e-17 |R| is below what one fp64 stencil product can confirm (2^-53 ~ 1.1e-16 per rounding), so the check of every direct solve
    fails: the hook run goes on to CG in every pressure iteration (asserted: cg_p > 0), the batch closes its gate with the fallback code at its first solve and time_step
    takes the loop back at that solve - poro_pres_solve with CG, p += dp, the remaining iterations call by call.  Trace, vectors and counters as in the hook run"""
    P = box_problem(3, n, 2)
    try:
        kw = dict(steps=2, solver_rel_tol=1e-17, fss_tol=0.0, max_fss=2)
        a, b = run_steps(monkeypatch, P, False, **kw), run_steps(monkeypatch, P, True, **kw)
        print(b["work"], [t[:, [2, 7]].tolist() for t in b["traces"]])
        assert b["work"]["cg_p"] > 0 and all(t[0, 7] > 0 for t in b["traces"])      # the hook run itself takes CG
        assert a["batched"] == 2 and b["batched"] == 0
        same_run(a, b)
    finally:
        P.close()


def material_k():
    from common import material
    return material().k_over_mu


def per_call_loop(C, tol, max_it, from_solve=False, **solver):
    """PoroelasticityFSS.h:358-380 call by call; from_solve: the first iteration's residual has been taken already (a loop handed back at its solve)"""
    l2s, infos, it = [], [], 0
    while from_solve or it < max_it:
        if not from_solve:
            it += 1
            C.pres_update_volumetric_strain()
            l2s.append(C.pres_assemble_residual(DT))
            if l2s[-1] < tol:
                break
        from_solve = False
        C.pres_assemble_jacobian(DT)
        infos.append(C.pres_solve(prec=pk.PREC_FDM, **solver)[1].as_dict())
        C.axpy(pk.VEC_P, 1.0, pk.VEC_DP)
    return l2s, infos


def test_failed_check_hands_the_loop_back_at_its_solve(monkeypatch):
    """rel_tol = 1e-17 is below what a direct solve in fp64 can reach (its relative residual is a few 1e-16), so every check fails: the per-call loop of the hook context
    goes on to CG (asserted: iterations > 0), the batch closes its gate with the fallback code at iteration 1 with dp the direct result and p not updated, and the caller's
    poro_pres_solve from there gives the hook context's bits.  Then a loop whose checks hold, through the same entry, with the cap inside the batch"""
    P = box_problem(3, (5, 4, 3), 2)
    G, H = contexts(monkeypatch, P)
    try:
        seed_state((G, H), 5)
        solver = dict(rel_tol=1e-17, max_iter=3)
        assert G.supports_pres_newton_loop() and not H.supports_pres_newton_loop()
        l2_h, infos_h = per_call_loop(H, 0.0, 2, **solver)
        assert len(infos_h) == 2 and all(i["iterations"] > 0 for i in infos_h)          # the hook run itself takes CG
        p_before = G.get(pk.VEC_P)
        N = G.pres_newton_loop(DT, 0.0, 2, **solver)
        print(N)
        assert N["outcome"] == 2 and N["iterations"] == 1 and N["solves"] == 0 and N["l2"][0] == l2_h[0]
        assert N["res"][0] > 1e-17 * N["bn"][0] and N["bn"][0] == pytest.approx(l2_h[0], rel=1e-12)       # |R| is the residual norm and the check's |b| (two kernels' sums)
        assert np.array_equal(G.get(pk.VEC_P), p_before) and np.abs(G.get(pk.VEC_DP)).max() > 0
        l2_g, infos_g = per_call_loop(G, 0.0, 0, from_solve=True, **solver)             # iteration 1 from its solve ...
        l2_g2, infos_g2 = per_call_loop(G, 0.0, 1, **solver)                            # ... and iteration 2
        assert l2_g == [] and l2_g2 == l2_h[1:]
        for a, b in zip(infos_g + infos_g2, infos_h):
            assert all(a[k] == b[k] for k in ("iterations", "converged", "initial_residual", "final_residual", "operator_applications")), (a, b)
        for v in (pk.VEC_P, pk.VEC_DP, pk.VEC_EPSV, pk.VEC_RESIDUAL_P):
            assert np.array_equal(G.get(v), H.get(v)), v
        # checks that hold: 5 iterations under a cap of 5 need two batches (4 slots each); every number of the record against the per-call loop
        seed_state((G, H), 6)
        l2_h, infos_h = per_call_loop(H, 0.0, 5)
        N = G.pres_newton_loop(DT, 0.0, 5)
        print(N)
        assert N["outcome"] == 0 and N["iterations"] == 5 and N["solves"] == 5 and N["batches"] == 2
        assert N["l2"].tolist() == l2_h and N["res"].tolist() == [i["final_residual"] for i in infos_h] and N["bn"].tolist() == [i["initial_residual"] for i in infos_h]
        assert N["pinf"] == np.abs(H.get(pk.VEC_P)).max()
        for v in (pk.VEC_P, pk.VEC_DP, pk.VEC_EPSV, pk.VEC_RESIDUAL_P):
            assert np.array_equal(G.get(v), H.get(v)), v
    finally:
        G.close(); H.close(); P.close()

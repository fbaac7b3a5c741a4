"""Prescribed pressures beside hanging pressure nodes on the device: a drained face on a locally refined or adapted mesh (meshes and list counts: test_pressure_bc_hanging_cpu.py).

Reference: Oracle.run() is NOT one on these meshes - it only sets the listed dofs, so a hanging row with a prescribed master keeps the start value's share for ever (5.08 % /
6.16 % against Terzaghi's series on M2 / M3).  Its matrices, residual, solves and step-wise entry points are valid when the start pressure is conforming,
and that is what is used here, beside an independent elimination with scipy and the analytic series.

Bounds: 1e-14 max|p| on a constraint row is a few roundings of a sum of at most four terms; 1e-9 against the sparse direct solve and final <= 1e-12 initial are those of
test_pressure_bc_fdm_gpu.py; 1e-8 on p and u against the oracle are test_terzaghi.py::test_device_follows_the_oracle_with_prescribed_pressures'; 0.015 against the series is
test_terzaghi.py::test_oracle_consolidation_matches_terzaghi's bound for dt = 60 s (meshes without a prescribed master measure 1.02 - 1.19 %)."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import poroelasticity_dealii_amd as pk
import oracle_py
from common import BC_2D, DOMAIN_MSH, GOLDEN, INPUT_DATA, csr_to_scipy, material
from test_adapt_gpu import python_steps
from test_constraints_cpu import cons_arrays
from test_pressure_bc_hanging_cpu import H, column_bc, coarse_desc, drained_column, prescribed, violation
from test_terzaghi import KW, analytic, profile

pytestmark = pytest.mark.gpu
DT = 60.0
EXE = os.path.join(os.path.dirname(GOLDEN), os.pardir, "poroelasticity_dealii_amd", "lib", "poro_run")
EPS = np.finfo(float).eps


def block_touching_the_drained_side(deg):
    """2D, 4 x 3 coarse cells, the two middle cells of the two upper layers refined: the block meets the drained top from inside, so the hanging nodes on its vertical
    edges have the prescribed corner as a master while no dof is in both lists"""
    bc, neu = column_bc(2)
    P = pk.Problem.refined_box_mask(2, [4, 3], [10.0, H], deg, material(flow_rate=0.0), bc, [0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0], neu)
    return P.set_pressure_bc([(3, 0.0)])


def build(case, deg):
    return {"M2": lambda: drained_column(2, deg)[0], "M3": lambda: drained_column(3, deg)[0], "block": lambda: block_touching_the_drained_side(deg)}[case]()


def values_view(P):
    """the provider's own value array behind the descriptor: writes reach the next context.  Valid until the provider rebuilds its list (set_pressure_bc, tie_boundary);
    the tests below take the view afresh for every write and call neither in between"""
    return np.ctypeslib.as_array(P.desc.dirichlet_value_p, shape=(P.desc.n_dirichlet_p,))


def expansion(P, x):
    dof, ptr, m, w, inh = cons_arrays(P.desc.cons_p)
    return dof, np.array([w[ptr[i]:ptr[i + 1]] @ x[m[ptr[i]:ptr[i + 1]]] + inh[i] for i in range(len(dof))])


def conforming(P, p):
    """p with the prescribed values set and the constraints distributed (numpy)"""
    pd, pv = prescribed(P.desc)
    p = p.copy(); p[pd] = pv
    dof, e = expansion(P, p)
    p[dof] = e; p[pd] = pv
    return p


# ---- 1. conformity ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("case", ["M2", "M3", "block"])
def test_apply_boundary_values_gives_a_conforming_pressure(case, deg):
    P = build(case, deg)
    try:
        d = P.desc; dim = d.dim
        pd, _ = prescribed(d)
        dof, ptr, m, w, inh = cons_arrays(d.cons_p)
        is_pd = np.zeros(d.n_dofs_p, bool); is_pd[pd] = True
        assert len(dof) > 0 and any(is_pd[m[ptr[i]:ptr[i + 1]]].any() for i in range(len(dof)))       # a hanging row with a prescribed master: the case at stake
        X = np.ctypeslib.as_array(d.vertex_coords, shape=(d.n_vertices, dim))
        linear = 3.0e5 + 2.0e4 * X[pd, 0] + (1.5e4 * X[pd, 1] if dim == 3 else 0.0)                   # linear along the face: the midpoint rule of a dof in both lists holds
        for name, vals in (("constant", np.zeros(len(pd))), ("linear", linear)):
            values_view(P)[:] = vals
            G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
            try:
                G.fill(pk.VEC_P, 2.0e5)
                G.pres_apply_boundary_values()
                p = G.get(pk.VEC_P)
                v = violation(P, p)
                print(f"{case} Q{deg} {name}: max|p| {np.abs(p).max():.3e}, largest constraint violation {v:.3e}")
                assert np.array_equal(p[pd], vals)                                                   # exactly
                assert v <= 1e-14 * np.abs(p).max()
                free = np.setdiff1d(np.arange(d.n_dofs_p), np.union1d(pd, dof))
                assert np.all(p[free] == 2.0e5)                                                      # nothing else moved
                assert G.supports_preconditioner(1, pk.PREC_JACOBI) and G.supports_preconditioner(1, pk.PREC_NONE) and not G.supports_preconditioner(1, pk.PREC_FDM)
                assert G.supports_preconditioner(1, pk.PREC_TWO_LEVEL)                               # the coarse box carries the whole face
            finally:
                G.close()
        values_view(P)[:] = 0.0
        # lists that break the consistency rule are refused when the context is created, with the dof named
        # (a) a hanging dof added to the prescribed list although one of its masters is free
        i = next(i for i in range(len(dof)) if not is_pd[dof[i]] and not is_pd[m[ptr[i]:ptr[i + 1]]].all())
        more_dof = np.append(pd, dof[i]).astype(np.int32); more_val = np.zeros(len(more_dof))
        keep = (d.n_dirichlet_p, d.dirichlet_dof_p, d.dirichlet_value_p)
        try:
            d.n_dirichlet_p = len(more_dof); d.dirichlet_dof_p = more_dof.ctypes.data_as(C.POINTER(C.c_int32)); d.dirichlet_value_p = more_val.ctypes.data_as(C.POINTER(C.c_double))
            with pytest.raises(RuntimeError, match=rf"dof {dof[i]} is both hanging and prescribed"):
                pk.Context(P, 0, pk.OP_MATRIX_FREE)
        finally:
            d.n_dirichlet_p, d.dirichlet_dof_p, d.dirichlet_value_p = keep
        # (b) a dof in both lists whose value is not the one its masters give
        both = [h for h in dof if is_pd[h]]
        assert (len(both) > 0) == (case == "M3")
        if both:
            values_view(P)[list(pd).index(both[0])] = 1.0e-3                                         # the largest prescribed magnitude: 1e-12 x that is far below
            with pytest.raises(RuntimeError, match=rf"dof {both[0]} is both hanging and prescribed"):
                pk.Context(P, 0, pk.OP_MATRIX_FREE)
            values_view(P)[:] = 0.0
    finally:
        P.close()


# ---- 2. the pressure solve against an independent elimination -------------------------------------------------------------------------------------------------
_elimination = {}


def eliminated_solution(case, P):
    """C^T J C on the free rows (neither hanging nor prescribed; x = 0 on the prescribed ones, so their columns drop out of C), solved directly.  J from the oracle's raw
    mass and Laplace matrices.  Computed once per mesh"""
    if case not in _elimination:
        O = oracle_py.Oracle(P, hoisted=True)
        try:
            M = csr_to_scipy(*O.export_csr(pk.MAT_MASS_P)); K = csr_to_scipy(*O.export_csr(pk.MAT_LAPLACE_P))
        finally:
            O.close()
        mt = material(flow_rate=0.0); n = P.desc.n_dofs_p
        J = (M / (mt.biot_M * DT) + mt.k_over_mu * K).tocsr()
        pd, _ = prescribed(P.desc)
        dof, ptr, m, w, inh = cons_arrays(P.desc.cons_p)
        free = np.setdiff1d(np.arange(n), np.union1d(pd, dof))
        col_of = -np.ones(n, np.int64); col_of[free] = np.arange(free.size)
        rows, cols, vals = list(free), list(col_of[free]), [1.0] * free.size
        for i in range(len(dof)):
            for k in range(ptr[i], ptr[i + 1]):
                if col_of[m[k]] >= 0:
                    rows.append(dof[i]); cols.append(col_of[m[k]]); vals.append(w[k])
        Cm = sp.csr_matrix((vals, (rows, cols)), shape=(n, free.size))
        b = np.zeros(n); b[free] = np.random.default_rng(77 + n).standard_normal(free.size)
        x = Cm @ spla.spsolve((Cm.T @ J @ Cm).tocsc(), Cm.T @ b)
        for a in (b, x, free):
            a.setflags(write=False)
        _elimination[case] = (b, x, free)
    return _elimination[case]


@pytest.mark.parametrize("mode", [pk.OP_CSR, pk.OP_MATRIX_FREE], ids=["csr", "matrix-free"])
@pytest.mark.parametrize("case", ["M2", "M3"])
def test_pressure_solve_equals_an_independent_elimination(case, mode):
    P = build(case, 1)
    G = pk.Context(P, 0, mode)
    try:
        b, x0, free = eliminated_solution(case, P)
        pd, _ = prescribed(P.desc)
        G.pres_assemble_jacobian(DT)
        for name, prec in (("jacobi", pk.PREC_JACOBI), ("two-level", pk.PREC_TWO_LEVEL)):
            assert G.supports_preconditioner(1, prec)
            G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
            rc, info = G.pres_solve(rel_tol=1e-12, prec=prec)
            x = G.get(pk.VEC_DP)
            dof, e = expansion(P, x)
            err = np.linalg.norm(x[free] - x0[free]) / np.linalg.norm(x0[free])
            print(f"{case} {name}: iterations {info.iterations}, residual {info.final_residual:.3e} / {info.initial_residual:.3e}, free rows rel2 {err:.3e}, "
                  f"hanging rows off their expansion by {np.abs(x[dof] - e).max():.3e}")
            assert rc == 0 and info.converged == 1 and info.final_residual <= 1e-12 * info.initial_residual
            assert err <= 1e-9
            assert np.all(x[pd] == 0.0)                                                              # exactly, hanging-and-prescribed dofs included
            assert np.abs(x[dof] - e).max() <= 4 * EPS * np.abs(x).max()                            # a sum of at most four products, summed in any order
            assert np.linalg.norm(x - x0) <= 1e-9 * np.linalg.norm(x0)
    finally:
        G.close(); P.close()


# ---- 3. step parity with the oracle through the step-wise entry points ----------------------------------------------------------------------------------------
def oracle_steps(O, first_step, n_steps, dt):
    """the loop of test_adapt_gpu.python_steps on the oracle's entry points (Jacobi everywhere; vector arithmetic on the host)"""
    dim = O.dim
    comps = [0, 3] if dim == 2 else [0, 4, 8]; entries = [0, 2] if dim == 2 else [0, 3, 5]
    O.disp_assemble_system(True); O.proj_assemble_matrix()
    rows = []
    for step in range(first_step, first_step + n_steps):
        O.set(pk.VEC_P_OLD, O.get(pk.VEC_P))
        err, fss = 2e-8, 0
        while fss < 50 and err > 1e-8:
            fss += 1; it = 0
            O.fill(pk.VEC_DP, 0.0)
            while it < 50:
                it += 1
                O.pres_update_volumetric_strain()
                err = O.pres_assemble_residual(dt)
                if err < 1e-8:
                    break
                O.pres_assemble_jacobian(dt)
                rc, _ = O.pres_solve(prec=oracle_py.PREC_JACOBI); assert rc == 0
                O.set(pk.VEC_P, O.get(pk.VEC_P) + O.get(pk.VEC_DP))
            O.disp_assemble_system(False)
            rc, _ = O.disp_solve(prec=oracle_py.PREC_JACOBI, max_iter=50000); assert rc == 0
            O.proj_assemble_rhs(comps)
            for e in entries:
                rc, _ = O.proj_solve(e, prec=oracle_py.PREC_JACOBI); assert rc == 0
            err = O.pres_assemble_residual(dt)
            rows.append([step, fss, it - 1])
    return np.array(rows)


@pytest.mark.parametrize("case,deg", [("M2", 2), ("M3", 1)])
def test_steps_follow_the_oracle_from_a_conforming_start(case, deg):
    P = build(case, deg)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        p_start = conforming(P, 2.0e5 * (1 + 0.1 * np.sin(0.37 * np.arange(P.desc.n_dofs_p))))
        assert violation(P, p_start) <= 1e-14 * np.abs(p_start).max()
        for S in (G, O):
            S.set(pk.VEC_P, p_start)
        t_dev, _ = python_steps(G, 1, 3, DT)
        t_ora = oracle_steps(O, 1, 3, DT)
        p, p0, u, u0 = G.get(pk.VEC_P), O.get(pk.VEC_P), G.get(pk.VEC_U), O.get(pk.VEC_U)
        print(f"{case}: rows {len(t_dev)}, fixed-stress / pressure iterations {t_dev[:, 1:3].astype(int).tolist()}, |dp| {np.abs(p - p0).max() / np.abs(p0).max():.2e}, "
              f"|du| {np.linalg.norm(u - u0) / np.linalg.norm(u0):.2e}, violation {violation(P, p) / np.abs(p).max():.2e}")
        assert np.array_equal(t_dev[:, :3], t_ora)
        assert np.abs(p - p0).max() <= 1e-8 * np.abs(p0).max()
        assert np.linalg.norm(u - u0) <= 1e-8 * np.linalg.norm(u0)
    finally:
        O.close(); G.close(); P.close()


# ---- 4. Terzaghi's column on M2 and M3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 1)], ids=["M2", "M3"])
def test_terzaghi_on_a_mesh_with_prescribed_masters(dim, deg):
    """Measured on the MI355X: 1.10 % on M2 (Q2), 0.75 % on M3 (Q1), constraint violation of the final p 3e-16 / 1.4e-15 p0; the non-conforming bookkeeping gives 5.1 % / 6.2 %"""
    P, m = drained_column(dim, deg)
    try:
        _, p0, _ = analytic(m, np.zeros(1), 0.0)
        tr, G = pk.run_problem(P, 10, p0, DT, operator_mode=pk.OP_MATRIX_FREE, prec=pk.PREC_CHEBYSHEV, coupled_fss=True, incremental_strain=True, **KW)
        try:
            p = G.get(pk.VEC_P)
        finally:
            G.close()
        depth, pn = profile(P, p, dim)
        e = np.abs(pn - analytic(m, depth, 10 * DT)[0]).max() / p0
        v = violation(P, p)
        print(f"terzaghi M{dim} Q{deg}: error {e:.4e}, rows {len(tr)}, constraint violation {v / p0:.2e} p0")
        assert e < 0.015
        assert v <= 1e-12 * p0
    finally:
        P.close()


# ---- 5. adaptive Terzaghi ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 1)], ids=["2d_q2", "3d_q1"])
def test_adaptive_terzaghi(dim, deg):
    """all-zero mask, adapts before steps 3, 6 and 9.  Measured on the MI355X: 0.99 % (2D Q2, 15 of 20 coarse cells refined at the end), 0.41 % (3D Q1, 21 of 24)"""
    P, m = drained_column(dim, deg, "zero")
    try:
        _, p0, _ = analytic(m, np.zeros(1), 0.0)
        kw = dict(prec=-1, coupled_fss=True, incremental_strain=True, **KW)
        trace, G = pk.run_problem(P, 9, p0, DT, operator_mode=pk.OP_MATRIX_FREE, refine_every=3, **kw)
        try:
            assert G.problem is not P
            mask = G.problem.refine_mask(); p = G.get(pk.VEC_P)
            depth, pn = profile(G.problem, p, dim)
            e = np.abs(pn - analytic(m, depth, 9 * DT)[0]).max() / p0
            v = violation(G.problem, p)
            print(f"adaptive terzaghi {dim}d Q{deg}: error {e:.4e} at t = 540 s, refined coarse cells {int(mask.sum())} of {len(mask)}, cells {G.problem.desc.n_cells}, "
                  f"hanging {G.problem.desc.cons_p.n}, rows {len(trace)}, violation {v / p0:.2e} p0")
            assert mask.any() and trace[-1, 0] == 9
            assert e < 0.015
            assert v <= 1e-12 * p0
        finally:
            G.close(); G.problem.close()
        R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=p0, dt=DT, **kw)
        try:
            R.initialize()
            manual = []
            for step in range(1, 10):
                if step % 3 == 0:
                    R.adapt()
                manual.append(R.step()[0])
            assert np.array_equal(np.vstack(manual), trace[1:])                                    # bit for bit
            assert np.array_equal(R.problem.refine_mask(), mask) and np.array_equal(R.ctx.get(pk.VEC_P), p)
        finally:
            R.close()
    finally:
        P.close()


# ---- 6. iteration counts of the two-level form ---------------------------------------------------------------------------------------------------------------
def solve_counts(P, b, precs):
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    out = {}
    try:
        G.pres_assemble_jacobian(DT)
        for name, prec in precs:
            assert G.supports_preconditioner(1, prec), name
            G.set(pk.VEC_RESIDUAL_P, b); G.fill(pk.VEC_DP, 0.0)
            rc, info = G.pres_solve(rel_tol=1e-12, prec=prec, max_iter=20000)
            assert rc == 0 and info.converged == 1
            out[name] = (info.iterations, G.get(pk.VEC_DP))
    finally:
        G.close()
    return out


BOTH = (("jacobi", pk.PREC_JACOBI), ("two-level", pk.PREC_TWO_LEVEL))


def test_two_level_iteration_counts_with_a_drained_side(tmp_path):
    """2D refined boxes, a block of a quarter of the cells against the drained side.  (c): the drained system is a principal subsystem of the undrained one, so the
    two-level form should need about the undrained count; the margin ceil(1.2 x) + 1 covers the other right-hand side and the coarse space without its face nodes"""
    series = {"cells_per_side": [], "jacobi_drained": [], "two_level_drained": [], "two_level_undrained": []}
    for n in (8, 16, 32):
        mk = lambda: pk.Problem.refined_box(2, [n, n], [10.0, 10.0], 1, material(flow_rate=0.0), BC_2D, [n // 4, n // 2], [3 * n // 4, n])
        Pd, Pu = mk().set_pressure_bc([(3, 0.0)]), mk()
        try:
            b = np.random.default_rng(5 + n).standard_normal(Pd.desc.n_dofs_p)
            drained = solve_counts(Pd, b, BOTH)
            undrained = solve_counts(Pu, b, BOTH[1:])
            pd, _ = prescribed(Pd.desc)
            xj, xt = drained["jacobi"][1], drained["two-level"][1]
            assert np.all(xt[pd] == 0.0) and np.linalg.norm(xt - xj) <= 1e-9 * np.linalg.norm(xj)                                                  # (a)
            for key, v in (("cells_per_side", n), ("jacobi_drained", drained["jacobi"][0]), ("two_level_drained", drained["two-level"][0]), ("two_level_undrained", undrained["two-level"][0])):
                series[key].append(int(v))
        finally:
            Pd.close(); Pu.close()
    print("two-level counts:", json.dumps(series))
    # the record profiles/two_level_drained.json holds these series under "iteration_counts" (beside the step times of tools/drained_adaptive_step.py).  A test run must
    # not rewrite a committed file, so the series go into that file's layout in the directory PORO_PROFILE_DIR names (set it to profiles/ to refresh the record)
    out_dir = os.environ.get("PORO_PROFILE_DIR")
    if out_dir:
        path = os.path.join(out_dir, "two_level_drained.json")
        record = json.load(open(path)) if os.path.exists(path) else {}
        record.setdefault("iteration_counts", {}).update(series)
        with open(path, "w") as f:
            json.dump(record, f, indent=1)
    assert series["two_level_drained"][-1] < series["jacobi_drained"][-1]                                                                            # (b)
    for d, u in zip(series["two_level_drained"], series["two_level_undrained"]):                                                                      # (c)
        assert d <= math.ceil(1.2 * u) + 1, series


def test_two_level_on_the_gmsh_grid_with_a_drained_side():
    P = pk.Problem.gmsh(DOMAIN_MSH, 1, material(flow_rate=0.0), BC_2D, refine=1)
    try:
        label = int(max(np.ctypeslib.as_array(P.desc.bface_id, shape=(P.desc.n_bfaces,))))
        P.set_pressure_bc([(label, 0.0)])
        assert coarse_desc(P).n_dirichlet_p > 0
        b = np.random.default_rng(9).standard_normal(P.desc.n_dofs_p)
        out = solve_counts(P, b, BOTH)
        pd, _ = prescribed(P.desc)
        xj, xt = out["jacobi"][1], out["two-level"][1]
        print(f"gmsh grid, one refinement, {P.desc.n_dofs_p} pressure dofs, {len(pd)} prescribed: Jacobi {out['jacobi'][0]}, two-level {out['two-level'][0]} iterations")
        assert np.all(xt[pd] == 0.0) and np.linalg.norm(xt - xj) <= 1e-9 * np.linalg.norm(xj)
        assert out["two-level"][0] < out["jacobi"][0]
    finally:
        P.close()


# ---- 7. the driver executable --------------------------------------------------------------------------------------------------------------------------------
def test_poro_run_drained_and_adaptive():
    r = subprocess.run([EXE, INPUT_DATA, "--matrix-free", "--fastest", "--pressure-bc", "3=0", "--refine-every", "2", "--steps", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(re.findall(r"^Time: ", r.stdout, re.M)) == 3
    names = r"(Jacobi|two-level|FDM)"
    adapted = re.findall(rf"^adapted before step (\d+): (\d+) -> (\d+) cells; prescribed pressures: (\d+) dofs; pressure preconditioner: {names}, projection preconditioner: {names}$", r.stdout, re.M)
    print(adapted)
    assert [a[0] for a in adapted] == ["2"] and int(adapted[0][2]) > int(adapted[0][1]) and int(adapted[0][3]) >= 17
    assert re.search(rf"^prescribed pressures: (\d+) dofs; pressure preconditioner: {names}, projection preconditioner: {names}$", r.stdout, re.M)


# ---- 8. the traction load is the same in every context of a mesh ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 1), (3, 2)], ids=str)
def test_traction_load_is_bitwise_reproducible(dim, deg):
    """Up to four boundary faces meet in a displacement dof in 3D.  The load is assembled face group by face group in a fixed order (no atomics), so every context of a
    mesh holds the same bits - what an adaptive run on a laterally symmetric column needs, where equal indicators would let a last bit decide which cells are marked
    (every adapt builds a new context).  The value itself: the integral of the traction over the top face is -SIGMA0 x area."""
    P, _ = drained_column(dim, deg)
    try:
        loads = []
        for _ in range(4):
            G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
            try:
                G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
                loads.append(G.get(pk.VEC_RHS_U))
            finally:
                G.close()
        assert all(np.array_equal(loads[0], b) for b in loads[1:])
        total = loads[0][dim - 1::dim].sum()
        assert abs(total + 1.0e6 * 10.0 ** (dim - 1)) <= 1e-12 * 1.0e6 * 10.0 ** (dim - 1)
    finally:
        P.close()

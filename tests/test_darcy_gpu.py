"""Flow post-processing on the device (include/poroel_hip.h: Darcy velocity, boundary discharge, fluid mass balance) against the NumPy reference
(tests/darcy_reference.py) and closed forms: cell velocities and face discharges on boxes, a tensor-product grid, non-affine cells, a Gmsh mesh and hanging nodes;
deterministic label sums; the identities I1-I3; the balance terms against exported matrices; an exact steady flow; a consolidation run; the refusals.

Bounds (the project's own): 1e-12 of max|entry| for elementwise results (tests/test_parity_gpu.py); 1e-12 of the sum of the absolute values of the summands for sums and
identities (tests/test_gravity_gpu.py).  Every case runs in both operator modes, for the scalar, per-cell (random over a decade) and tensor permeability, and with gravity
off and with g = (1.7, -2.3, -9.81), rho_f = 1000."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, DOMAIN_MSH, ROLLERS3, box_problem, csr_to_scipy, layered_field_problems, material
from darcy_reference import balance_terms, cell_velocity, face_discharge, face_measures, label_sums, mesh, per_cell, vertex_of_dof_p
from general_reference import jitter, mapped
from gravity_reference import laplace_abs_apply
from test_terzaghi import KW as TERZAGHI_KW, analytic, column

pytestmark = pytest.mark.gpu
G3 = np.array([1.7, -2.3, -9.81])
RHO_F = 1000.0
ROLLERS2 = [(0, 0, 0.0), (2, 1, 0.0)]
MODES = [pk.OP_CSR, pk.OP_MATRIX_FREE]
SIZE = [3.1, 1.9, 2.6]


def permeabilities(rng, nc, dim, k0):
    return [("scalar", k0), ("cell", k0 * 10.0 ** rng.random(nc)), ("tensor", k0 * 10.0 ** rng.random((nc, dim)))]


def hand_permeability(C, form, value):
    if form == "scalar":
        C.set_cell_permeability(None)
    elif form == "cell":
        C.set_cell_permeability(value)
    else:
        C.set_cell_permeability_tensor(value)


def gravities(dim):
    return [("no_gravity", np.zeros(dim)), ("gravity", RHO_F * G3[:dim])]


def hand_gravity(C, dim, rg):
    if np.any(rg):
        C.set_gravity(G3[:dim], 2700.0, RHO_F)
    else:
        C.set_gravity(None, 2700.0, 0.0)


def problem(name):
    if name == "1x1_q1":
        return pk.Problem.box(2, [1, 1], SIZE[:2], 1, material(), ROLLERS2)
    if name == "1x1x1_q1":
        return pk.Problem.box(3, [1, 1, 1], SIZE, 1, material(), ROLLERS3)
    if name == "9x6x5_q1":            # 270 cells and 258 boundary faces: both lane-per-item kernels cross a 256-lane block
        return pk.Problem.box(3, [9, 6, 5], SIZE, 1, material(), ROLLERS3)
    if name == "33x9_q2":
        return pk.Problem.box(2, [33, 9], SIZE[:2], 2, material(), ROLLERS2)
    if name == "graded":
        return pk.Problem.graded_box(3, [3, 2, 4], [3.0, 2.0, 4.0], 2, material(), ROLLERS3, [0.6, 0.0, 0.9])
    if name == "jittered":
        B = pk.Problem.box(3, [3, 2, 4], [3.0, 2.0, 2.5], 2, material(), ROLLERS3)
        return mapped(B, jitter(B))
    if name == "gmsh":
        return pk.Problem.gmsh(DOMAIN_MSH, 2, material(), BC_2D)
    assert name == "refined"
    G, R = layered_field_problems()
    G.close()
    return R


MESHES = ["1x1_q1", "1x1x1_q1", "9x6x5_q1", "33x9_q2", "graded", "jittered", "gmsh", "refined"]


@pytest.mark.parametrize("mode", MODES, ids=["csr", "matrix_free"])
@pytest.mark.parametrize("name", MESHES, ids=str)
def test_velocity_and_discharge_against_the_reference(name, mode):
    """a random pressure vector: q_c and Q_b to 1e-12 of max|entry|; then I1 (linear p_h: q_c = -kappa_c (a - rho_f g)), I2 (p_h = rho_f g . x: q = 0 and Q_b = 0 to
    1e-12 max|kappa rho_f g| |F_b|) and I3 (scalar kappa, linear p_h: sum_b Q_b = 0 to 1e-12 sum |Q_b|) on the same context"""
    P = problem(name)
    C = pk.Context(P, 0, mode)
    try:
        desc = P.desc; dim, nc = desc.dim, desc.n_cells
        if name == "9x6x5_q1":
            assert nc == 270 and desc.n_bfaces == 258
        rng = np.random.default_rng(17)
        X = vertex_of_dof_p(P)
        h = np.ptp(X, axis=0).max()
        p_rand = 2.0e4 * h * rng.random(desc.n_dofs_p)                    # gradients of the size of rho_f |g|
        a = np.array([0.7e4, -1.3e4, 2.1e4])[:dim]
        p_lin = X @ a + 1.0e4
        A = face_measures(P)
        for form, kappa in permeabilities(rng, nc, dim, desc.mat.k_over_mu):
            hand_permeability(C, form, kappa)
            kc = per_cell(kappa, nc, dim)
            for gname, rg in gravities(dim):
                hand_gravity(C, dim, rg)
                C.set(pk.VEC_P, p_rand)
                q, (Q, _) = C.darcy_velocity(), C.boundary_discharge()
                q0, Q0 = cell_velocity(P, p_rand, kappa, rg), face_discharge(P, p_rand, kappa, rg)
                eq, eQ = np.abs(q - q0).max() / np.abs(q0).max(), np.abs(Q - Q0).max() / np.abs(Q0).max()
                print(f"{name} {form} {gname}: velocity {eq:.2e} discharge {eQ:.2e} of max|entry|")
                assert eq <= 1e-12 and eQ <= 1e-12, (form, gname, eq, eQ)
                # another vector of the space through which_vec: the same numbers, bit for bit
                C.set(pk.VEC_DP, p_rand)
                assert np.array_equal(C.darcy_velocity(pk.VEC_DP), q) and np.array_equal(C.boundary_discharge(which=pk.VEC_DP)[0], Q)
                # I1
                C.set(pk.VEC_P, p_lin)
                q = C.darcy_velocity()
                want = -kc * (a - rg)[None, :]
                e1 = np.abs(q - want).max() / np.abs(want).max()
                assert e1 <= 1e-12, (form, gname, "I1", e1)
                # I3
                if form == "scalar":
                    Q = C.boundary_discharge()[0]
                    assert abs(Q.sum()) <= 1e-12 * np.abs(Q).sum() and np.abs(Q).max() > 0, (gname, "I3", Q.sum(), np.abs(Q).sum())
            # I2 (gravity is on from the last pass of the loop)
            rg = RHO_F * G3[:dim]
            C.set(pk.VEC_P, X @ rg)
            q, (Q, _) = C.darcy_velocity(), C.boundary_discharge()
            scale = np.abs(kc * rg[None, :]).max()
            e2q, e2Q = np.abs(q).max() / scale, (np.abs(Q) / (scale * A)).max()
            print(f"{name} {form}: hydrostatic velocity {e2q:.2e} discharge {e2Q:.2e} of max|kappa rho_f g| (|F|)")
            assert e2q <= 1e-12 and e2Q <= 1e-12, (form, "I2", e2q, e2Q)
    finally:
        C.close(); P.close()


@pytest.mark.parametrize("name", ["17x16x1", "gmsh"], ids=str)
def test_label_sums_are_deterministic(name):
    """Q_label against numpy.sum of the per-face values (17 x 16 x 1: 272 faces on each z label, more than one workgroup's lanes), bitwise equal across two calls, and
    exactly 0 for a label no face carries"""
    P = pk.Problem.box(3, [17, 16, 1], SIZE, 1, material(), ROLLERS3) if name == "17x16x1" else problem("gmsh")
    C = pk.Context(P, 0, pk.OP_CSR)
    try:
        desc = P.desc; dim = desc.dim
        bid = mesh(P)[5][2]
        present = sorted(set(bid.tolist()))
        if name == "17x16x1":
            assert (bid == 4).sum() == 272 and (bid == 5).sum() == 272
        absent = max(present) + 71
        labels = present[::-1] + [absent] + present[:1]                 # any order, a label twice, one without faces
        rng = np.random.default_rng(23)
        C.set(pk.VEC_P, 1.0e5 * rng.random(desc.n_dofs_p))
        C.set_cell_permeability(desc.mat.k_over_mu * 10.0 ** rng.random(desc.n_cells))
        C.set_gravity(G3[:dim], 2700.0, RHO_F)
        Q, Ql = C.boundary_discharge(labels)
        Q2, Ql2 = C.boundary_discharge(labels)
        assert np.array_equal(Q, Q2) and np.array_equal(Ql, Ql2)
        want = label_sums(P, Q, labels)
        for l, got, w in zip(labels, Ql, want):
            assert abs(got - w) <= 1e-12 * np.abs(Q[bid == l]).sum(), (l, got, w)
        assert Ql[len(present)] == 0.0 and Ql[-1] == Ql[len(present) - 1]
        # per-face values without labels, labels without per-face values: the same numbers
        assert np.array_equal(C.boundary_discharge()[0], Q) and C.boundary_discharge()[1].size == 0
        out = np.empty(len(labels)); lab = np.asarray(labels, dtype=np.int32)
        import ctypes
        rc = C.L.poro_pres_boundary_discharge(C.ptr, pk.VEC_P, None, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(labels), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert rc == 0 and np.array_equal(out, Ql)
    finally:
        C.close(); P.close()


STATE_VECS = (pk.VEC_U, pk.VEC_RHS_U, pk.VEC_P, pk.VEC_P_OLD, pk.VEC_DP, pk.VEC_RESIDUAL_P, pk.VEC_EPSV, pk.VEC_EPSV0, pk.VEC_SOURCE_P)


def balance_problem(name):
    if name == "9x6x5":
        P = pk.Problem.box(3, [9, 6, 5], SIZE, 1, material(), ROLLERS3)
        P.set_pressure_bc([(5, 1.5e5)])                                   # drained top
        return P
    G, R = layered_field_problems()
    G.close()
    R.set_pressure_bc([(1, 0.5e5)])      # the face x = high of the refined box: cell 23 (the last one) is refined, so hanging nodes lie on the prescribed face and beside it
    return R


@pytest.mark.parametrize("name", ["9x6x5", "refined"], ids=str)
def test_balance_terms_against_exported_matrices(name):
    """random state vectors; r = M t + kappa K p + src from the CSR context's exported matrices, condensed in NumPy.  Every term of both contexts (CSR, matrix-free) to
    1e-12 of the sum of the absolute values of its summands, C^T(-r) on the prescribed dofs to 1e-12 of its maximum, the identity to 1e-12 of
    sum_i (|M t|_i + |kappa K p|_i + |src_i|); no vector of the context changes, bit for bit"""
    P = balance_problem(name)
    ctx = {mode: pk.Context(P, 0, mode) for mode in MODES}
    try:
        desc = P.desc; dim, nc, n = desc.dim, desc.n_cells, desc.n_dofs_p
        assert desc.n_dirichlet_p > 0 and (name != "refined" or desc.cons_p.n > 0)
        rng = np.random.default_rng(29)
        dt = 45.0
        p, p_old = 2.0e5 * rng.random(n), 2.0e5 * rng.random(n)
        ev, ev0 = 1e-4 * rng.standard_normal(n), 1e-4 * rng.standard_normal(n)
        for form, kappa in permeabilities(rng, nc, dim, desc.mat.k_over_mu):
            for gname, rg in gravities(dim):
                ref = None
                for mode in MODES:
                    C = ctx[mode]
                    hand_permeability(C, form, kappa)
                    hand_gravity(C, dim, rg)
                    for which, v in ((pk.VEC_P, p), (pk.VEC_P_OLD, p_old), (pk.VEC_EPSV, ev), (pk.VEC_EPSV0, ev0), (pk.VEC_RESIDUAL_P, rng.random(n)), (pk.VEC_DP, rng.random(n))):
                        C.set(which, v)
                    if ref is None:                                          # (the CSR context comes first)
                        M = csr_to_scipy(*C.export_csr(pk.MAT_MASS_P))
                        KK = csr_to_scipy(*C.export_csr(pk.MAT_LAPLACE_P)) * (desc.mat.k_over_mu if form == "scalar" else 1.0)
                        src = C.get(pk.VEC_SOURCE_P) + (C.gravity_vectors()[1] if np.any(rg) else 0.0)
                        ref = balance_terms(P, M, KK, src, p, p_old, ev, ev0, dt)
                    before = [C.get(w) for w in STATE_VECS]
                    t, per_dof = C.flow_balance(dt)
                    t2, per_dof2 = C.flow_balance(dt)
                    assert t == t2 and np.array_equal(per_dof, per_dof2)
                    for w, b in zip(STATE_VECS, before):
                        assert np.array_equal(C.get(w), b), (w, "changed by poro_pres_flow_balance")
                    for key, want in ref["terms"].items():
                        err = abs(t[key] - want) / ref["scales"][key]
                        print(f"{name} {form} {gname} mode {mode}: {key} = {t[key]:.6e}, off by {err:.2e} of its summands")
                        assert err <= 1e-12, (form, gname, mode, key, t[key], want)
                    Rt_pd = ref["Rt"][ref["prescribed"]]
                    assert np.abs(per_dof - Rt_pd).max() <= 1e-12 * np.abs(ref["Rt"]).max(), (form, gname, mode)
                    ident = t["outflow_prescribed"] + t["free_row_sum"] + t["storage_rate_strain"] + t["storage_rate_pressure"] + t["source_sum"]
                    assert abs(ident) <= 1e-12 * ref["scale"], (form, gname, mode, ident, ref["scale"])
                    # what poro_pres_assemble_residual returns is residual_l2 (same calls, same order of additions up to the masking)
                    assert abs(C.pres_assemble_residual(dt) - t["residual_l2"]) <= 1e-12 * ref["scale"]
    finally:
        for C in ctx.values():
            C.close()
        P.close()


@pytest.mark.parametrize("with_gravity", [False, True], ids=["no_gravity", "gravity"])
def test_exact_steady_flow_through_a_column(with_gravity):
    """2 x 2 x 6 column, top (label 5) and bottom (label 4) prescribed at different values, p = p_old linear between them (plus the hydrostatic part under gravity, which
    drops out of q), eps_v = eps_v0: both storage terms are 0 and at each face the conservative outflow and the face-integrated discharge equal +- kappa (dp / H) A"""
    m = material(flow_rate=0.0)
    Hc, side = 6.0, 2.0
    P = pk.Problem.box(3, [2, 2, 6], [side, side, Hc], 1, m, ROLLERS3)
    P.set_pressure_bc([(4, 3.0e5), (5, 1.0e5)])
    kw = dict(gravity=G3, fluid_density=RHO_F) if with_gravity else {}
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, dt=60.0, **kw)
    try:
        X = vertex_of_dof_p(P)
        z0 = X[:, 2].min()
        rg = RHO_F * G3 if with_gravity else np.zeros(3)
        p = 3.0e5 - 2.0e5 * (X[:, 2] - z0) / Hc + (X - X.mean(axis=0)) @ rg
        for w in (pk.VEC_P, pk.VEC_P_OLD):
            R.ctx.set(w, p)
        B = R.flow_balance()
        exact = m.k_over_mu * 2.0e5 / Hc * side * side                     # leaves through the top, enters through the bottom
        assert B["labels"] == [4, 5] and B["storage_rate_strain"] == 0.0 and B["storage_rate_pressure"] == 0.0
        # sums of absolute values: the rows of kappa |K| |p| (+ |f_g|) on the prescribed dofs; kappa (|grad p| + |rho_f g|) |F| on the faces
        rows = m.k_over_mu * laplace_abs_apply(P, 1.0, p) + (np.abs(R.ctx.gravity_vectors()[1]) if with_gravity else 0.0)
        labels = P.pressure_bc_labels(); pd = np.ctypeslib.as_array(P.desc.dirichlet_dof_p, shape=(P.desc.n_dirichlet_p,))
        face_scale = m.k_over_mu * (2.0e5 / Hc + np.abs(rg).sum()) * side * side
        for label, want in ((4, -exact), (5, exact)):
            out, dis = B["outflow_by_label"][label], B["discharge_by_label"][label]
            print(f"label {label}: outflow {out:.12e} discharge {dis:.12e} exact {want:.12e}")
            assert abs(out - want) <= 1e-12 * rows[pd[labels == label]].sum(), (label, out, want)
            assert abs(dis - want) <= 1e-12 * face_scale, (label, dis, want)
        assert abs(B["outflow_prescribed"]) <= 1e-12 * rows.sum() and abs(B["free_row_sum"]) <= 1e-12 * rows.sum()
        # the velocity itself: q = (0, 0, kappa dp / H) in every cell
        q = R.darcy_velocity()
        assert np.abs(q - np.array([0.0, 0.0, m.k_over_mu * 2.0e5 / Hc])).max() <= 1e-12 * face_scale / (side * side)
    finally:
        R.close(); P.close()


def test_a_consolidation_run_closes_its_balance():
    """the 3D Terzaghi column of tests/test_terzaghi.py, coupled_fss and incremental_strain, four steps through Runner.  After every step
    |storage + source + outflow| <= sqrt(n_dofs_p) residual_l2 + 1e-12 sum_i (|M t|_i + |kappa K p|_i + |src_i|); the outflow through the drained top is positive and
    falls from step 2 on; the cumulative drained volume equals minus the cumulative storage change within the summed per-step bounds.
    (Recorded, not asserted - no bound can be derived here: the drained volume against Terzaghi's series and the face-integrated against the conservative discharge.)"""
    P, m = column(3, 8, 1)
    _, p0, cv = analytic(m, np.zeros(1), 0.0)
    dt, steps = 30.0, 4
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=p0, dt=dt, prec=pk.PREC_CHEBYSHEV, coupled_fss=True, incremental_strain=True, **TERZAGHI_KW)
    try:
        n = P.desc.n_dofs_p
        R.track_flow_balance()
        R.initialize()
        assert R.flow_balance()["cumulative"]["steps"] == 0
        M = csr_to_scipy(*R.ctx.export_csr(pk.MAT_MASS_P)); K = csr_to_scipy(*R.ctx.export_csr(pk.MAT_LAPLACE_P)) * m.k_over_mu
        outflow, rounding = [], 0.0
        for s in range(steps):
            R.step()
            B = R.flow_balance()
            ref = balance_terms(P, M, K, R.ctx.get(pk.VEC_SOURCE_P), *(R.ctx.get(w) for w in (pk.VEC_P, pk.VEC_P_OLD, pk.VEC_EPSV, pk.VEC_EPSV0)), dt)
            lhs = B["storage_rate_strain"] + B["storage_rate_pressure"] + B["source_sum"] + B["outflow_prescribed"]
            bound = np.sqrt(n) * B["residual_l2"] + 1e-12 * ref["scale"]
            print(f"step {s + 1}: imbalance {lhs:.3e} bound {bound:.3e} (residual_l2 {B['residual_l2']:.3e}); outflow {B['outflow_by_label'][5]:.9e} face-integrated {B['discharge_by_label'][5]:.9e}")
            assert abs(lhs) <= bound, (s, lhs, bound)
            assert B["labels"] == [5] and B["outflow_by_label"][5] == pytest.approx(B["outflow_prescribed"], rel=1e-12)
            outflow.append(B["outflow_by_label"][5]); rounding += dt * 1e-12 * ref["scale"]
            assert B["cumulative"]["steps"] == s + 1
        assert all(v > 0 for v in outflow) and all(b < a for a, b in zip(outflow[1:], outflow[2:])), outflow
        cum = B["cumulative"]
        assert abs(cum["outflow"] - dt * sum(outflow)) <= 1e-12 * dt * sum(outflow) and cum["outflow_by_label"][5] == pytest.approx(cum["outflow"], rel=1e-12)
        gap = cum["outflow"] + cum["storage_strain"] + cum["storage_pressure"] + cum["source"]
        assert abs(gap) <= cum["bound"] + rounding, (gap, cum["bound"], rounding)
        # recorded: the drained volume per unit area against the series, int_0^t q dt = sum_k 8 p0 H (k/mu) / (pi^2 (2k+1)^2 cv) (1 - exp(-(2k+1)^2 pi^2 cv t / (4 H^2)))
        Hc = 10.0; t = steps * dt
        series = sum(8 * p0 * Hc * m.k_over_mu / (np.pi ** 2 * (2 * k + 1) ** 2 * cv) * (1 - np.exp(-(2 * k + 1) ** 2 * np.pi ** 2 * cv * t / (4 * Hc ** 2))) for k in range(2000))
        print(f"drained volume after {t:g} s: {cum['outflow']:.6e} (conservative) {cum['discharge_by_label'][5]:.6e} (face-integrated) against Terzaghi's series {series * 100.0:.6e}")
        # initialize() resets the accumulators
        R.initialize()
        assert R.flow_balance()["cumulative"]["steps"] == 0 and R.flow_balance()["cumulative"]["outflow"] == 0.0
    finally:
        R.close(); P.close()


def test_refusals():
    """a partitioned context, a displacement-space vector and dt = 0 are refused with a message; the context stays usable"""
    S = box_problem(3, (2, 2, 4), 1, rank=0, n_ranks=2)
    G = pk.Context(S, 0, pk.OP_CSR)
    try:
        for call in (G.darcy_velocity, G.boundary_discharge, lambda: G.flow_balance(60.0)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "partitioned" in str(e.value)
    finally:
        G.close(); S.close()
    P = pk.Problem.box(3, [2, 2, 2], SIZE, 2, material(), ROLLERS3)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        for call in (lambda: C.darcy_velocity(pk.VEC_U), lambda: C.boundary_discharge(which=pk.VEC_RHS_U)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "not a pressure-space vector" in str(e.value)
        for dt in (0.0, -1.0, float("nan")):
            with pytest.raises(RuntimeError) as e:
                C.flow_balance(dt)
            assert "time_step" in str(e.value)
        assert C.darcy_velocity().shape == (8, 3) and C.flow_balance(60.0)[1].size == 0
    finally:
        C.close(); P.close()

"""Mechanical post-processing on the device (include/poroel_hip.h: cell stresses, failure measures, force balance) against the NumPy reference
(tests/stress_reference.py) and closed forms: strain, effective and total stress on boxes, jittered and sheared cells and refined boxes, Q1 and Q2, with the scalar
moduli and a 3-layer field; the patch identities; the measures on random and degenerate states with the device-side summary; every term of the force balance, the
identity and the per-dof reactions; a loaded column; the refusals.

Bounds (the project's own, tests/test_parity_gpu.py and tests/test_darcy_gpu.py): 1e-12 of max|entry| for elementwise results; 1e-12 of the sum of the absolute values
of the summands for sums and identities.  Every case runs in both operator modes."""
import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import ROLLERS3, box_problem, material
from darcy_reference import vertex_of_dof_p
from general_reference import GeneralReference, cell_vertices, jitter, mapped, shear
from stress_reference import (arrays, cell_stress, component_table, force_balance, full_tensor, measures, measures_of, nodal_mean_moduli)
from test_terzaghi import KW as TERZAGHI_KW, SIGMA0, analytic, column

pytestmark = pytest.mark.gpu
MODES = [pk.OP_CSR, pk.OP_MATRIX_FREE]
MODE_IDS = ["csr", "matrix_free"]
SIZE = [3.1, 1.9, 2.6]
ROLLERS2 = [(0, 0, 0.0), (2, 1, 0.0)]
G3 = np.array([1.7, -2.3, -9.81])
STATE_VECS = (pk.VEC_U, pk.VEC_RHS_U, pk.VEC_P, pk.VEC_P_OLD, pk.VEC_DP, pk.VEC_RESIDUAL_P, pk.VEC_EPSV, pk.VEC_EPSV0)


def rollers(dim):
    return ROLLERS2 if dim == 2 else ROLLERS3


def top_load(dim):
    """a normal load on the high face of the last direction and a second condition on the high x face, other component (traction = value * n)"""
    return [(2 * dim - 1, dim - 1, -2.0e6), (1, 0, 0.7e6)]


def problem(name, k, neumann=()):
    dim = int(name[-1])
    n = [3, 2, 4][:dim]
    if name.startswith("box"):
        return pk.Problem.box(dim, n, SIZE[:dim], k, material(), rollers(dim), neumann)
    if name.startswith("jit"):                                       # jittered, then sheared: non-affine cells, no axis aligned with the grid
        B = pk.Problem.box(dim, n, SIZE[:dim], k, material(), rollers(dim), neumann)
        ji, sh = jitter(B), shear(B)
        return mapped(B, lambda X: sh(ji(X)))
    assert name.startswith("ref")                                    # a quarter of the 4^dim box refined: hanging nodes, some of them on the supported faces
    return pk.Problem.refined_box(dim, [4] * dim, [4.0, 3.0, 5.0][:dim], k, material(), rollers(dim), [0] * dim, [2, 2, 4][:dim], neumann)


SHAPES = ["box2", "box3", "jit2", "jit3", "ref2", "ref3"]


def layers(P, rng=None):
    """a 3-layer moduli field along the last direction (by cell centres): a stiff caprock over a soft reservoir over a base, every contrast a factor > 3"""
    d, dim, k, X, cv, cdu, cdp = arrays(P)
    z = X[cv].mean(axis=1)[:, dim - 1]
    lo, hi = X[:, dim - 1].min(), X[:, dim - 1].max()                # thirds of the mesh's extent: every centre lies strictly inside one
    layer = np.minimum(2, (3 * (z - lo) / (hi - lo)).astype(int))
    m = d.mat
    lam = m.lame_lambda * np.array([1.0, 0.2, 3.5])[layer]
    G = m.shear_G * np.array([1.0, 0.3, 4.0])[layer]
    return lam, G, layer


def random_state(P, rng):
    d = P.desc
    X = vertex_of_dof_p(P)
    h = np.ptp(X, axis=0).max()
    return 1e-4 * h * rng.standard_normal(d.n_dofs_u), 2.0e6 * rng.random(d.n_dofs_p)


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", [1, 2], ids=["q1", "q2"])
@pytest.mark.parametrize("name", SHAPES, ids=str)
def test_cell_stress_against_the_reference(name, k, mode):
    """random u and p: strain, effective and total stress to 1e-12 of max|entry| with the material's scalars and with the 3-layer field; which_p = None gives total =
    effective bit for bit; with the field, the cells that touch an interface show their OWN moduli: the result differs from the nodal-mean product by more than 1e-3
    relative there, so the old formula cannot pass"""
    P = problem(name, k)
    C = pk.Context(P, 0, mode)
    try:
        d = P.desc
        rng = np.random.default_rng(41)
        u, p = random_state(P, rng)
        C.set(pk.VEC_U, u); C.set(pk.VEC_P, p)
        before = [C.get(w) for w in STATE_VECS]
        lam_l, G_l, layer = layers(P)
        for field in ("scalar", "layered"):
            lam, G = (d.mat.lame_lambda, d.mat.shear_G) if field == "scalar" else (lam_l, G_l)
            C.set_cell_moduli(*((None, None) if field == "scalar" else (lam, G)))
            e, se, st = C.cell_stress()
            e0, se0, st0 = cell_stress(P, u, p, lam, G, d.mat.biot_alpha)
            errs = rel(e, e0), rel(se, se0), rel(st, st0)
            print(f"{name} q{k} mode {mode} {field}: strain {errs[0]:.2e} effective {errs[1]:.2e} total {errs[2]:.2e} of max|entry|")
            assert max(errs) <= 1e-12, (field, errs)
            e2, se2, st2 = C.cell_stress(which_p=None)
            assert np.array_equal(e2, e) and np.array_equal(se2, se) and np.array_equal(st2, se)
            if field == "layered":
                lam_n, G_n = nodal_mean_moduli(P, lam, G)
                at = np.nonzero((np.abs(lam_n - lam) > 1e-6 * lam))[0]                # the cells with a vertex on an interface
                assert at.size and len(set(layer[at].tolist())) >= 2      # cells on both sides of an interface
                old = cell_stress(P, u, p, lam_n, G_n, d.mat.biot_alpha)[1]
                gap = np.abs(se[at] - old[at]).max(axis=1) / np.abs(se[at]).max(axis=1)
                assert gap.min() > 1e-3, gap.min()
        C.set_cell_moduli(None, None)
        for w, b in zip(STATE_VECS, before):
            assert np.array_equal(C.get(w), b), (w, "changed by poro_disp_cell_stress")
    finally:
        C.close(); P.close()


@pytest.mark.parametrize("k", [1, 2], ids=["q1", "q2"])
@pytest.mark.parametrize("name", ["jit2", "jit3"], ids=str)
def test_patch_identities_on_jittered_meshes(name, k):
    """u = B x + c at the support points gives eps = sym B in every cell; p = a . x + p0 gives sigma = sigma' - alpha p(x_c) I; a rigid rotation plus translation gives
    eps = 0 to 1e-12 of |B|"""
    P = problem(name, k)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        d = P.desc; dim = d.dim
        rng = np.random.default_rng(43)
        R = GeneralReference(P)
        comp = component_table(P)
        B = 1e-4 * rng.standard_normal((dim, dim))
        a = np.array([0.7e4, -1.3e4, 2.1e4])[:dim]; p0 = 5.0e5
        C.set(pk.VEC_U, R.linear_field(B) + 1e-4 * rng.standard_normal(dim)[comp])   # (a translation of the size of B x: the entries of u round to eps max|u|)
        C.set(pk.VEC_P, vertex_of_dof_p(P) @ a + p0)
        e, se, st = C.cell_stress()
        symB = 0.5 * (B + B.T)
        E = full_tensor(e, dim, 0.0)[:, :dim, :dim]
        assert np.abs(E - symB[None]).max() <= 1e-12 * np.abs(B).max()
        m = d.mat
        want = m.lame_lambda * np.trace(symB) * np.eye(dim) + 2 * m.shear_G * symB
        S = full_tensor(se, dim, 0.0)[:, :dim, :dim]
        assert np.abs(S - want[None]).max() <= 1e-12 * np.abs(want).max()
        xc = P.coords[cell_vertices(d)].mean(axis=1)
        wantT = want[None] - m.biot_alpha * (xc @ a + p0)[:, None, None] * np.eye(dim)[None]
        T = full_tensor(st, dim, 0.0)[:, :dim, :dim]
        assert np.abs(T - wantT).max() <= 1e-12 * np.abs(wantT).max()
        W = rng.standard_normal((dim, dim)); W = 1e-4 * (W - W.T)
        C.set(pk.VEC_U, R.linear_field(W) + 3e-5)
        assert np.abs(C.cell_stress()[0]).max() <= 1e-12 * np.abs(W).max()
    finally:
        C.close(); P.close()


def rotation(dim, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    return Q


@pytest.mark.parametrize("dim", [2, 3], ids=str)
def test_measures_against_eigvalsh(dim):
    """u = B x on the sheared box gives the same strain in every cell; the states: B = a I (triple root), diag(0, .., a) (double root), the same rotated out of the axes,
    pure shear, a double root perturbed by 1e-9 relative, in 2D three states whose out-of-plane stress is the largest, the middle and the smallest principal value, and
    a random u.  Every column to 1e-12 of max|entry| against eigvalsh of the reference's stress; f against its formula; the summary against max / argmax / count of the
    returned column; two calls return the same bits"""
    B0 = pk.Problem.box(dim, [3, 2, 4][:dim], SIZE[:dim], 2, material(), rollers(dim))
    P = mapped(B0, shear(B0))
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        d = P.desc; m = d.mat
        rng = np.random.default_rng(47)
        R = GeneralReference(P)
        a = 2.0e-4
        I = np.eye(dim)
        last = np.zeros((dim, dim)); last[-1, -1] = a
        Q = rotation(dim, rng)
        ps = np.zeros((dim, dim)); ps[0, 1] = ps[1, 0] = a
        states = {"triple": a * I, "double": last, "double_rotated": Q @ last @ Q.T, "pure_shear": ps,
                  "double_perturbed": Q @ (last + 1e-9 * a * np.diag(np.arange(dim) == 0).astype(float)) @ Q.T}
        if dim == 2:
            states.update(zz_largest=np.diag([-a, -2 * a]), zz_middle=np.array([[a, 0.3 * a], [0.3 * a, -0.8 * a]]), zz_smallest=np.diag([a, 2 * a]))
        c, phi = 1.5e6, np.deg2rad(31.0)
        want_place = dict(zz_largest=0, zz_middle=1, zz_smallest=2)
        for name, Bm in states.items():
            u = R.linear_field(Bm)
            C.set(pk.VEC_U, u)
            M, summ = C.cell_measures(cohesion=c, friction_angle=phi)
            e0, se0, _ = cell_stress(P, u, None, m.lame_lambda, m.shear_G, m.biot_alpha)
            M0 = measures(P, e0, se0, m.lame_lambda, c, phi)
            scale = np.abs(M0[:, :5]).max()
            err = np.abs(M[:, :5] - M0[:, :5]).max() / scale
            print(f"{dim}D {name}: measures off by {err:.2e} of max|entry|; s = {M[0, :3]}")
            assert err <= 1e-12, (name, err)
            assert np.abs(M[:, 5] - M0[:, 5]).max() <= 1e-12 * (scale + c), name
            f = 0.5 * (M[:, 0] - M[:, 2]) + 0.5 * (M[:, 0] + M[:, 2]) * np.sin(phi) - c * np.cos(phi)
            assert np.abs(M[:, 5] - f).max() <= 1e-12 * (scale + c), name
            assert np.all(M[:, 0] >= M[:, 1]) and np.all(M[:, 1] >= M[:, 2])
            if name in want_place:                                     # plane strain: sigma'_zz = lambda tr(eps) sits where the state's name says
                zz = m.lame_lambda * np.trace(Bm)
                assert np.abs(M[:, want_place[name]] - zz).max() <= 1e-12 * scale
            assert summ["max_f"] == M[:, 5].max() and summ["argmax_cell"] == int(np.argmax(M[:, 5])) and summ["n_failing"] == int((M[:, 5] >= 0).sum())
        u, p = random_state(P, rng)
        C.set(pk.VEC_U, u); C.set(pk.VEC_P, p)
        M, summ = C.cell_measures(cohesion=c, friction_angle=phi)
        M2, summ2 = C.cell_measures(which_p=None, cohesion=c, friction_angle=phi)
        assert np.array_equal(M, M2) and summ == summ2                 # the same bits, and the pressure vector does not enter
        e0, se0, _ = cell_stress(P, u, p, m.lame_lambda, m.shear_G, m.biot_alpha)
        M0 = measures(P, e0, se0, m.lame_lambda, c, phi)
        assert np.abs(M - M0).max() <= 1e-12 * np.abs(M0).max()
        assert summ["max_f"] == M[:, 5].max() and summ["argmax_cell"] == int(np.argmax(M[:, 5])) and summ["n_failing"] == int((M[:, 5] >= 0).sum())
        assert 0 < summ["n_failing"] < d.n_cells or summ["n_failing"] in (0, d.n_cells)
        # no criterion: f = 0 and a summary of zeros, the other columns as before
        Mn, sn = C.cell_measures()
        assert np.array_equal(Mn[:, :5], M[:, :5]) and not Mn[:, 5].any() and sn == dict(max_f=0.0, argmax_cell=0, n_failing=0)
        # with the layered field the 2D out-of-plane stress takes the cell's own lambda
        lam_l, G_l, _ = layers(P)
        C.set_cell_moduli(lam_l, G_l)
        M = C.cell_measures(cohesion=c, friction_angle=phi)[0]
        e0, se0, _ = cell_stress(P, u, p, lam_l, G_l, m.biot_alpha)
        M0 = measures(P, e0, se0, lam_l, c, phi)
        assert np.abs(M - M0).max() <= 1e-12 * np.abs(M0).max()
    finally:
        C.close(); P.close()


def test_summary_tie_goes_to_the_lowest_cell():
    """3 x 2 unit cells with exactly representable vertices, Q1.  u = 0: every cell has the same state, the tie goes to cell 0 (cohesion 0: f = 0 >= 0 everywhere, all
    cells fail; cohesion > 0: none).  u_x = a on the vertices of the high x face: cells 2 and 5 carry the same bits and the largest f - the summary names cell 2.
    More cells than one block of the reduction takes (80 x 60, three blocks): the same tie across blocks"""
    P = pk.Problem.box(2, [3, 2], [3.0, 2.0], 1, material(), ROLLERS2)
    C = pk.Context(P, 0, pk.OP_CSR)
    try:
        phi = 0.5
        M, s = C.cell_measures(cohesion=0.0, friction_angle=phi)
        assert not M.any() and s == dict(max_f=0.0, argmax_cell=0, n_failing=6)
        M, s = C.cell_measures(cohesion=1.0e6, friction_angle=phi)
        assert s["argmax_cell"] == 0 and s["n_failing"] == 0 and s["max_f"] == M[0, 5] and abs(M[0, 5] + 1.0e6 * np.cos(phi)) <= 1e-9
        R = GeneralReference(P)
        X, comp = R.node_coords()
        u = np.where((comp == 0) & (X[:, 0] == X[:, 0].max()), 1e-4, 0.0)
        C.set(pk.VEC_U, u)
        M, s = C.cell_measures(cohesion=1.0e6, friction_angle=phi)
        assert np.array_equal(M[2], M[5]) and M[2, 5] > M[[0, 1, 3, 4], 5].max()
        assert s["argmax_cell"] == 2 and s["max_f"] == M[2, 5] and s["n_failing"] == int((M[:, 5] >= 0).sum())
    finally:
        C.close(); P.close()
    P = pk.Problem.box(2, [80, 60], [80.0, 60.0], 1, material(), ROLLERS2)
    C = pk.Context(P, 0, pk.OP_CSR)
    try:
        R = GeneralReference(P)
        X, comp = R.node_coords()
        C.set(pk.VEC_U, np.where((comp == 0) & (X[:, 0] == X[:, 0].max()), 1e-4, 0.0))
        M, s = C.cell_measures(cohesion=1.0e6, friction_angle=0.5)
        top = np.nonzero(M[:, 5] == M[:, 5].max())[0]
        assert top.size == 60 and top[0] == 79 and s["argmax_cell"] == 79 and s["max_f"] == M[79, 5]
    finally:
        C.close(); P.close()


def check_balance(C, P, ref, tag):
    """every term to 1e-12 of the sum of its absolute summands, the per-dof reactions to 1e-12 of max|Rt|, |coupling_sum| <= 1e-12 sum |b_cpl,i|, the identity"""
    before = [C.get(w) for w in STATE_VECS]
    t = C.force_balance()
    t2 = C.force_balance()
    for key in ("reaction_sum", "free_row_sum", "traction_sum", "body_sum", "coupling_sum", "reaction_dof"):
        assert np.array_equal(t[key], t2[key]), (tag, key)
    assert t["residual_l2"] == t2["residual_l2"]
    for w, b in zip(STATE_VECS, before):
        assert np.array_equal(C.get(w), b), (tag, w, "changed by poro_disp_force_balance")
    for key, want in ref["terms"].items():
        sc = ref["scales"][key]
        err = np.max(np.abs(t[key] - want) / np.where(np.asarray(sc) > 0, sc, 1.0))
        print(f"{tag}: {key} = {t[key]}, off by {err:.2e} of its summands")
        assert err <= 1e-12, (tag, key, t[key], want)
    assert np.abs(t["reaction_dof"] - ref["Rt"][ref["dirichlet"]]).max() <= 1e-12 * np.abs(ref["Rt"]).max(), tag
    assert np.all(np.abs(t["coupling_sum"]) <= 1e-12 * ref["scales"]["coupling_sum"]), (tag, t["coupling_sum"])
    ident = t["reaction_sum"] + t["free_row_sum"] + t["traction_sum"] + t["body_sum"] + t["coupling_sum"]
    assert np.all(np.abs(ident) <= 1e-12 * ref["total"]), (tag, ident, ref["total"])
    return t


@pytest.mark.parametrize("k", [1, 2], ids=["q1", "q2"])
@pytest.mark.parametrize("name", SHAPES, ids=str)
def test_force_balance_against_the_reference(name, k):
    """random u and p, two traction conditions; both operator modes; the material's scalars without gravity, then the 3-layer moduli with gravity and a per-cell density"""
    P = problem(name, k, top_load(int(name[-1])))
    ctx = {mode: pk.Context(P, 0, mode) for mode in MODES}
    try:
        d = P.desc; dim = d.dim
        rng = np.random.default_rng(53)
        u, p = random_state(P, rng)
        lam_l, G_l, _ = layers(P)
        rho = 2000.0 + 600.0 * rng.random(d.n_cells)
        if name.startswith("ref"):
            assert d.cons_u.n > 0
        refs = {}
        for case in ("plain", "layered_gravity"):
            lam, G = (d.mat.lame_lambda, d.mat.shear_G) if case == "plain" else (lam_l, G_l)
            refs[case] = force_balance(P, u, p, lam, G, d.mat.biot_alpha, g=None if case == "plain" else G3[:dim], rho=rho)
        if name == "ref3":                                           # hanging nodes on the supported faces: the closed list dropped their prescribed masters
            assert np.abs(refs["plain"]["deficit"]).max() > 0
        for mode, mid in zip(MODES, MODE_IDS):
            C = ctx[mode]
            C.set(pk.VEC_U, u); C.set(pk.VEC_P, p)
            for case in ("plain", "layered_gravity"):
                if case == "plain":
                    C.set_cell_moduli(None, None); C.set_gravity(None, 2700.0, 0.0); C.set_cell_density(None)
                else:
                    C.set_cell_moduli(lam_l, G_l); C.set_gravity(G3[:dim], 2700.0, 1000.0); C.set_cell_density(rho)
                C.disp_assemble_system(True)
                C.set(pk.VEC_U, u)
                t = check_balance(C, P, refs[case], f"{name} q{k} {mid} {case}")
                assert (np.abs(t["body_sum"]) > 0).all() == (case != "plain") and np.abs(t["traction_sum"][[0, dim - 1]]).min() > 0
                by = t["reaction_by_label"]
                lab = (P if hasattr(P, "displacement_bc_labels") else P.source).displacement_bc_labels()
                assert set(by) == {tuple(r) for r in lab.tolist()}
                for c in range(dim):
                    s = sum(v for (l, cc), v in by.items() if cc == c)
                    assert abs(s + refs[case]["deficit"][refs[case]["comp"] == c].sum() - t["reaction_sum"][c]) <= 1e-12 * refs[case]["total"][c]
    finally:
        for C in ctx.values():
            C.close()
        P.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_force_balance_before_any_assembly_and_with_a_rigid_plate(mode):
    """a fresh context (no matrix built yet) gives the same numbers; a rigid-plate tie (the top face's vertical displacement tied to one value) folds the tied rows'
    residual into the master row: terms, per-dof reactions and identity against the reference with the descriptor's own constraint list"""
    P = pk.Problem.box(3, [3, 2, 4], SIZE, 2, material(), ROLLERS3, [(5, 2, -2.0e6)])
    P.tie_boundary([(5, 2)])
    C = pk.Context(P, 0, mode)
    try:
        d = P.desc
        assert d.cons_u.n > 0
        rng = np.random.default_rng(59)
        u, p = random_state(P, rng)
        C.set(pk.VEC_U, u); C.set(pk.VEC_P, p)
        ref = force_balance(P, u, p, d.mat.lame_lambda, d.mat.shear_G, d.mat.biot_alpha)
        assert not ref["deficit"].any()
        t0 = check_balance(C, P, ref, f"tie fresh mode {mode}")
        C.disp_assemble_system(True)
        C.set(pk.VEC_U, u)
        t1 = check_balance(C, P, ref, f"tie assembled mode {mode}")
        for key in ("reaction_sum", "free_row_sum", "traction_sum", "coupling_sum"):
            assert np.array_equal(t0[key], t1[key])
    finally:
        C.close(); P.close()


def test_a_loaded_column_carries_its_load():
    """the Terzaghi column of tests/test_terzaghi.py, 2 x 2 x 6 cells, three steps.  After every step the vertical reaction of the bottom label equals the applied top
    traction times the area within sqrt(n_dofs_u) residual_l2 + 1e-12 of the summands; the horizontal reactions of opposite roller faces cancel within the same bound;
    reaction_by_label sums to reaction_sum"""
    P, m = column(3, 6, 1)
    _, p0, _ = analytic(m, np.zeros(1), 0.0)
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=p0, dt=30.0, prec=pk.PREC_CHEBYSHEV, coupled_fss=True, incremental_strain=True, **TERZAGHI_KW)
    try:
        d = P.desc
        area = 10.0 * 10.0
        R.initialize()
        for s in range(3):
            R.step()
            C = R.ctx
            t = C.force_balance()
            ref = force_balance(P, C.get(pk.VEC_U), C.get(pk.VEC_P), m.lame_lambda, m.shear_G, m.biot_alpha)
            bound = np.sqrt(d.n_dofs_u) * t["residual_l2"] + 1e-12 * ref["total"]
            by = t["reaction_by_label"]
            print(f"step {s + 1}: reactions {t['reaction_sum']} traction {t['traction_sum']} free rows {t['free_row_sum']} residual_l2 {t['residual_l2']:.3e} bound {bound}")
            assert abs(t["traction_sum"][2] + SIGMA0 * area) <= 1e-12 * ref["scales"]["traction_sum"][2]
            assert abs(by[(4, 2)] - SIGMA0 * area) <= bound[2], (by[(4, 2)], SIGMA0 * area, bound[2])
            assert abs(by[(0, 0)] + by[(1, 0)]) <= bound[0] and abs(by[(2, 1)] + by[(3, 1)]) <= bound[1]
            for c in range(3):
                assert abs(sum(v for (l, cc), v in by.items() if cc == c) - t["reaction_sum"][c]) <= 1e-12 * ref["total"][c]
                assert abs(t["free_row_sum"][c]) <= bound[c]
    finally:
        R.close(); P.close()


def test_refusals():
    """a partitioned context, vectors of the wrong space and bad Mohr-Coulomb parameters are refused with a message; the context stays usable"""
    S = box_problem(3, (2, 2, 4), 1, rank=0, n_ranks=2)
    Gc = pk.Context(S, 0, pk.OP_CSR)
    try:
        for call in (Gc.cell_stress, Gc.cell_measures, Gc.force_balance):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "partitioned" in str(e.value)
    finally:
        Gc.close(); S.close()
    P = pk.Problem.box(3, [2, 2, 2], SIZE, 2, material(), ROLLERS3)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        for call in (lambda: C.cell_stress(pk.VEC_P), lambda: C.cell_measures(pk.VEC_DP), lambda: C.cell_stress(pk.VEC_U, pk.VEC_STRAIN0 + 99)):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(RuntimeError) as e:
            C.cell_stress(pk.VEC_P)
        assert "not a displacement-space vector" in str(e.value)
        for call in (lambda: C.cell_stress(pk.VEC_U, pk.VEC_RHS_U), lambda: C.cell_measures(pk.VEC_U, pk.VEC_U)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "not a pressure-space vector" in str(e.value)
        for c, phi in ((-1.0, 0.5), (1.0, -0.1), (1.0, np.pi / 2), (1.0, float("nan")), (float("nan"), 0.5)):
            with pytest.raises(RuntimeError) as e:
                C.cell_measures(cohesion=c, friction_angle=phi)
            assert "cohesion" in str(e.value) or "friction angle" in str(e.value)
        e, se, st = C.cell_stress()
        M, s = C.cell_measures(cohesion=1.0, friction_angle=0.5)
        assert e.shape == (8, 6) and M.shape == (8, 6) and s["argmax_cell"] == 0 and C.force_balance()["reaction_dof"].size == P.desc.n_dirichlet
    finally:
        C.close(); P.close()

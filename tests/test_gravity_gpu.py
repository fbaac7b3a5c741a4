"""Gravity on the device: the two gravity vectors of every kernel against the NumPy reference (tests/gravity_reference.py), and the wiring - a hydrostatic column at
rest on every residual path, a column under its own weight against the closed form, the default bit for bit, the order of the setters, slab partitions, runs through
the host driver (steady state under gravity, hydrostatic start, an adaptive run) and the command-line driver.

Bounds: 1e-12 of max|entry| for assembled vectors (the project's bound, tests/test_parity_gpu.py); 1e-12 of the sum of the absolute values of the summands for the three
identities; 1e-12 max|f_g| for the hydrostatic residual; 1e-9 of max|u| for the solved columns (tests/test_moduli_gpu.py); 1e-13 of the maximum for the stitched vectors
of a partition; 1e-6 of the maximum for the steady state of a run."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import BC_2D, DOMAIN_MSH, INPUT_DATA, ROLLERS3, box_problem, material
from general_reference import GeneralReference, jitter, mapped
from gravity_reference import body_force, cell_volumes, gravity_flux, laplace_abs_apply, laplace_apply, vertex_of_dof_p
import slab_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G3 = np.array([1.7, -2.3, -9.81])          # every component non-zero
RHO_F = 1000.0
ROLLERS2 = [(0, 0, 0.0), (2, 1, 0.0)]


def rollers(dim):
    return ROLLERS2 if dim == 2 else ROLLERS3


def permeabilities(rng, nc, dim, k0):
    """the three forms a context can hold: the scalar of the material, one k / mu per cell, the diagonal tensor - the fields random over a decade"""
    return [("scalar", k0), ("cell", k0 * 10.0 ** rng.random(nc)), ("tensor", k0 * 10.0 ** rng.random((nc, dim)))]


def hand_permeability(C, form, value):
    if form == "scalar":
        C.set_cell_permeability(None)
    elif form == "cell":
        C.set_cell_permeability(value)
    else:
        C.set_cell_permeability_tensor(value)


def component_dofs(P, d):
    desc = P.desc
    cdu = np.ctypeslib.as_array(desc.cell_dofs_u, shape=(desc.n_cells, (desc.degree_u + 1) ** desc.dim * desc.dim))
    return np.unique(cdu[:, d::desc.dim])


def check_vectors(P, mode=pk.OP_MATRIX_FREE, seed=3):
    """body_u and flux_p of a context of P against the reference, and the three identities, for per-cell density and the three permeability forms"""
    desc = P.desc; dim, nc = desc.dim, desc.n_cells
    rng = np.random.default_rng(seed)
    g = G3[:dim]
    rho = 2000.0 * 10.0 ** rng.random(nc)
    X = vertex_of_dof_p(P)
    p_h = RHO_F * X @ g
    vol = cell_volumes(P)
    C = pk.Context(P, 0, mode)
    out = []
    try:
        C.set_cell_density(rho)
        for form, kappa in permeabilities(rng, nc, dim, desc.mat.k_over_mu):
            hand_permeability(C, form, kappa)
            C.set_gravity(g, 2700.0, RHO_F)
            b, f = C.gravity_vectors()
            b0, f0 = body_force(P, g, rho), gravity_flux(P, g, RHO_F, kappa)
            eb, ef = np.abs(b - b0).max() / np.abs(b0).max(), np.abs(f - f0).max() / np.abs(f0).max()
            out.append((form, eb, ef))
            assert eb <= 1e-12 and ef <= 1e-12, (form, eb, ef)
            assert abs(f.sum()) <= 1e-12 * np.abs(f).sum(), form
            for d in range(dim):
                dofs = component_dofs(P, d)
                assert abs(b[dofs].sum() - g[d] * (rho * vol).sum()) <= 1e-12 * np.abs(b[dofs]).sum(), (form, d)
            r = laplace_apply(P, kappa, p_h) + f
            assert np.all(np.abs(r) <= 1e-12 * (laplace_abs_apply(P, kappa, p_h) + np.abs(f)).max()), form
        # the scalar density: the same kernels without the field
        C.set_cell_density(None)
        b = C.gravity_vectors()[0]
        b0 = body_force(P, g, 2700.0)
        assert np.abs(b - b0).max() <= 1e-12 * np.abs(b0).max()
    finally:
        C.close()
    return out


# ---- 1. the vectors against the NumPy reference ------------------------------------------------------------------------------------------------------------------
BOX_CASES = {
    "1x1_q1": ([1, 1], 1), "1x1_q2": ([1, 1], 2), "1x1x1_q1": ([1, 1, 1], 1), "1x1x1_q2": ([1, 1, 1], 2),      # every node is a corner, edge or face node
    "2x1x3_q2": ([2, 1, 3], 2), "3x2x4_q1": ([3, 2, 4], 1),
    "17x3x2_q2": ([17, 3, 2], 2),      # 1225 nodes: several workgroups and a partial last one
    "40x5_q1": ([40, 5], 1),           # 246 nodes: one partial workgroup
    "33x9_q2": ([33, 9], 2),
}
SIZE = [3.1, 1.9, 2.6]                # different cell sides in every direction


@pytest.mark.parametrize("name", list(BOX_CASES), ids=str)
def test_box_kernels_against_the_reference(name):
    n, deg = BOX_CASES[name]
    dim = len(n)
    P = pk.Problem.box(dim, n, SIZE[:dim], deg, material(), rollers(dim))
    try:
        assert P.desc.box.enabled
        for form, eb, ef in check_vectors(P):
            print(f"{name} {form}: body {eb:.2e} flux {ef:.2e} of max|entry|")
    finally:
        P.close()


def general_problem(name):
    if name == "graded":
        return pk.Problem.graded_box(3, [3, 2, 4], [3.0, 2.0, 4.0], 2, material(), ROLLERS3, [0.6, 0.0, 0.9])
    if name == "jittered":
        B = pk.Problem.box(3, [3, 2, 2], [3.0, 2.0, 2.5], 2, material(), ROLLERS3)
        return mapped(B, jitter(B))
    if name == "gmsh":
        return pk.Problem.gmsh(DOMAIN_MSH, 2, material(), BC_2D)
    return pk.Problem.refined_box(3, [4, 4, 4], [4.0, 3.0, 5.0], 2 if name == "refined_q2" else 1, material(), ROLLERS3, [0, 0, 0], [2, 2, 2])      # one corner block refined: hanging nodes


@pytest.mark.parametrize("name", ["graded", "jittered", "gmsh", "refined_q1", "refined_q2"], ids=str)
def test_general_kernels_against_the_reference(name):
    P = general_problem(name)
    try:
        assert not P.desc.box.enabled
        for form, eb, ef in check_vectors(P):
            print(f"{name} {form}: body {eb:.2e} flux {ef:.2e} of max|entry|")
    finally:
        P.close()


# ---- 2. a hydrostatic column is at rest ---------------------------------------------------------------------------------------------------------------------------------
def rest_problem(name):
    m = material(flow_rate=0.0)
    if name == "refined":
        return pk.Problem.refined_box(3, [4, 4, 4], [4.0, 3.0, 5.0], 1, m, ROLLERS3, [0, 0, 0], [2, 2, 2])
    if name == "tensor_grid":
        return pk.Problem.graded_box(3, [3, 2, 4], [3.0, 2.0, 4.0], 2, m, ROLLERS3, [0.6, 0.0, 0.9])
    n = [5, 4, 6] if name.endswith("3d") else [7, 5]
    return pk.Problem.box(len(n), n, SIZE[:len(n)], 2, m, rollers(len(n)))


@pytest.mark.parametrize("name,mode", [("box_3d", pk.OP_MATRIX_FREE), ("box_2d", pk.OP_MATRIX_FREE), ("box_3d", pk.OP_CSR), ("tensor_grid", pk.OP_MATRIX_FREE),
                                       ("refined", pk.OP_MATRIX_FREE), ("refined", pk.OP_CSR)], ids=str)
def test_hydrostatic_pressure_is_at_rest(name, mode):
    """p = p_old = p_h = rho_f g . x, eps_v = eps_v0, no well: the residual vanishes on every row to 1e-12 max|f_g| - the matrix-free box (both stencil kernels), CSR, a
    tensor-product grid, hanging nodes, and the three permeability forms"""
    P = rest_problem(name)
    C = pk.Context(P, 0, mode)
    try:
        desc = P.desc; dim = desc.dim
        g = G3[:dim]
        p_h = RHO_F * vertex_of_dof_p(P) @ g
        rng = np.random.default_rng(5)
        for form, kappa in permeabilities(rng, desc.n_cells, dim, desc.mat.k_over_mu):
            hand_permeability(C, form, kappa)
            C.set_gravity(g, 2700.0, RHO_F)
            f = C.gravity_vectors()[1]
            C.set(pk.VEC_P, p_h); C.set(pk.VEC_P_OLD, p_h); C.fill(pk.VEC_EPSV, 0.0); C.fill(pk.VEC_EPSV0, 0.0)
            C.pres_assemble_residual(60.0)
            R = C.get(pk.VEC_RESIDUAL_P)
            e = np.abs(R).max() / np.abs(f).max()
            print(f"{name} {form}: max|R| = {e:.2e} max|f_g|")
            assert e <= 1e-12, (form, e)
            # without the flux term the same state is far from rest: the test sees the term
            C.set_gravity(g, 2700.0, 0.0)
            C.pres_assemble_residual(60.0)
            assert np.abs(C.get(pk.VEC_RESIDUAL_P)).max() >= 0.5 * np.abs(f).max()
    finally:
        C.close(); P.close()


# ---- 3. a column under its own weight ---------------------------------------------------------------------------------------------------------------------------------
def column_exact(z, tops, rho, kv, g):
    """u_z(z) of a column of layers (tops ascending from the bottom at 0, densities rho, lambda + 2G = kv) held at z = 0 with a free top under gravity g > 0:
    (lambda + 2G) u'' = rho g in every layer, u(0) = 0, sigma(H) = 0, u and sigma continuous - piecewise quadratic"""
    tops = np.asarray(tops, dtype=float); bottoms = np.r_[0.0, tops[:-1]]
    above = np.r_[np.cumsum((rho * g * (tops - bottoms))[::-1])[::-1][1:], 0.0]          # weight of the layers above layer l
    def piece(l, za, zb):                                                                # int_za^zb sigma / kv inside layer l
        return -((above[l] + rho[l] * g * tops[l]) * (zb - za) - rho[l] * g * (zb ** 2 - za ** 2) / 2) / kv[l]
    u_at_bottom = np.r_[0.0, np.cumsum([piece(l, bottoms[l], tops[l]) for l in range(len(tops))])]
    l = np.minimum(np.searchsorted(tops, z - 1e-12, side="left"), len(tops) - 1)
    return u_at_bottom[l] + np.array([piece(li, bottoms[li], zi) for li, zi in zip(l, z)])


@pytest.mark.parametrize("layered", [False, True], ids=["uniform", "layered"])
@pytest.mark.parametrize("n,deg", [([2, 6], 2), ([2, 2, 6], 2), ([2, 2, 8], 1)], ids=str)
def test_column_under_its_own_weight(n, deg, layered):
    """rollers on the sides, held at the bottom, free top, p = 0: u_z = rho_b g (z^2 / 2 - H z) / (lambda + 2G), the lateral components vanish; Q2 holds the quadratic,
    Q1 is nodally exact for this load.  Layered: three moduli layers and three density layers with interfaces on cell boundaries"""
    dim = len(n); last = dim - 1; H = float(n[-1])
    bc = [(2 * d, d, 0.0) for d in range(dim)] + [(2 * d + 1, d, 0.0) for d in range(last)]
    P = pk.Problem.box(dim, n, [float(v) for v in n], deg, material(), bc)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        m = P.desc.mat; grav = 9.81
        X = vertex_of_dof_p(P); cv = np.ctypeslib.as_array(P.desc.cell_dofs_p, shape=(P.desc.n_cells, 1 << dim))
        zc = X[cv][:, :, last].mean(axis=1) - X[:, last].min()                           # cell centres above the bottom
        if layered:
            third = n[-1] // 3
            tops = np.array([third, 2 * third, H], dtype=float)
            layer = np.searchsorted(tops, zc, side="left")
            lam_l, G_l, rho_l = m.lame_lambda * np.array([1.0, 0.05, 3.0]), m.shear_G * np.array([0.3, 1.0, 0.02]), np.array([2700.0, 1800.0, 2300.0])
            C.set_cell_moduli(lam_l[layer], G_l[layer]); C.set_cell_density(rho_l[layer])
            assert C.get_cell_density()[1] == 1                                          # constant within every cell layer of the slowest direction
            C.set_gravity([0.0] * last + [-grav], 1.0, 0.0)
        else:
            tops, rho_l, lam_l, G_l = np.array([H]), np.array([2700.0]), np.array([m.lame_lambda]), np.array([m.shear_G])
            C.set_gravity([0.0] * last + [-grav], 2700.0, 0.0)
        C.fill(pk.VEC_P, 0.0); C.disp_assemble_system(True)
        prec = pk.PREC_FDM if C.supports_preconditioner(0, pk.PREC_FDM) else pk.PREC_JACOBI
        rc, info = C.disp_solve(abs_tol=0.0, rel_tol=1e-12, max_iter=50000, prec=prec)
        assert rc == 0
        pos, comp = GeneralReference(P).node_coords()
        u = C.get(pk.VEC_U)
        z = pos[:, last] - pos[:, last].min()
        exact = np.where(comp == last, column_exact(z, tops, rho_l, lam_l + 2 * G_l, grav), 0.0)
        if not layered:
            assert np.allclose(exact[comp == last], 2700.0 * grav * (z[comp == last] ** 2 / 2 - H * z[comp == last]) / (m.lame_lambda + 2 * m.shear_G), rtol=1e-12, atol=0)
        e = np.abs(u - exact).max() / np.abs(exact).max()
        print(f"column {n} Q{deg} {'layered' if layered else 'uniform'}: {info.iterations} iterations ({'FDM' if prec == pk.PREC_FDM else 'Jacobi'}), error {e:.2e} of max|u|")
        assert e <= 1e-9
    finally:
        C.close(); P.close()


# ---- 4. the default, bit for bit ------------------------------------------------------------------------------------------------------------------------------------------
def rhs_and_residual(C, p):
    C.set(pk.VEC_P, p); C.set(pk.VEC_P_OLD, 0.9 * p); C.set(pk.VEC_EPSV, 1e-6 * np.cos(np.arange(C.n_p))); C.fill(pk.VEC_EPSV0, 0.0)
    C.disp_assemble_system(True)
    C.pres_assemble_residual(60.0)
    return C.get(pk.VEC_RHS_U).tobytes(), C.get(pk.VEC_RESIDUAL_P).tobytes()


@pytest.mark.parametrize("mesh,mode", [("box", pk.OP_MATRIX_FREE), ("box", pk.OP_CSR), ("refined", pk.OP_MATRIX_FREE)], ids=str)
def test_without_gravity_every_bit_is_what_it_was(mesh, mode):
    """PORO_VEC_RHS_U and the residual of a context that never had gravity, of one where it was set and cleared, and of one with g = 0: byte-equal"""
    def problem():
        if mesh == "box":
            return box_problem(3, [3, 2, 4], 2, neumann=[(5, 2, -1e6)])
        return pk.Problem.refined_box(3, [3, 3, 3], [10.0] * 3, 2, material(), [(0, 0, 0.0), (1, 0, -1e-5), (2, 1, 0.0), (4, 2, 0.0)], [0, 0, 0], [1, 1, 2], [(5, 2, -1e6)])
    P = problem()
    try:
        p = 1e7 * (1 + 0.1 * np.sin(0.7 * np.arange(P.desc.n_dofs_p)))
        A = pk.Context(P, 0, mode)
        never = rhs_and_residual(A, p); A.close()
        B = pk.Context(P, 0, mode)
        B.set_gravity(G3, 2700.0, RHO_F); B.set_cell_density(np.full(P.desc.n_cells, 2500.0))
        with_gravity = rhs_and_residual(B, p)
        assert with_gravity[0] != never[0] and with_gravity[1] != never[1]              # (gravity is seen by both vectors)
        B.set_gravity(None, 0.0, 0.0)
        assert B.get_gravity()[3] is False and not np.any(B.gravity_vectors()[0]) and not np.any(B.gravity_vectors()[1])
        assert rhs_and_residual(B, p) == never
        B.set_gravity(G3, 2700.0, RHO_F)
        assert rhs_and_residual(B, p) == with_gravity
        B.set_gravity([0.0, 0.0, 0.0], 2700.0, RHO_F)                                   # an all-zero g is "off"
        assert B.get_gravity()[3] is False and rhs_and_residual(B, p) == never
        B.close()
    finally:
        P.close()


def test_a_run_without_gravity_is_bitwise_the_run_it_was():
    """a two-step run_problem: a problem that never had gravity, one where it was set and cleared, and one run with g = 0 - the same trace and fields, byte for byte"""
    def run(prepare, **kw):
        P = box_problem(2, 4, 2)
        try:
            prepare(P)
            tr, G = pk.run_problem(P, 2, 10e6, 60.0, operator_mode=pk.OP_MATRIX_FREE, max_it=5000, **kw)
            out = (tr.tobytes(), G.get(pk.VEC_U).tobytes(), G.get(pk.VEC_P).tobytes())
            G.close()
            return out
        finally:
            P.close()

    def set_and_clear(P):
        P.set_gravity([0.0, -9.81], RHO_F, 2500.0, hydrostatic_init=True); P.set_density_layers([(9.0, 2000.0)])
        P.set_gravity(None); P.set_cell_density(None)
    never = run(lambda P: None)
    assert run(set_and_clear) == never
    assert run(lambda P: None, gravity=[0.0, 0.0], fluid_density=RHO_F, density=2500.0, hydrostatic_init=True) == never
    assert run(lambda P: None, gravity=[0.0, -9.81], fluid_density=RHO_F) != never      # (and gravity is seen by a run)


# ---- 5. the order of the setters ---------------------------------------------------------------------------------------------------------------------------------------
def test_setter_order_does_not_matter_and_the_matrix_is_not_rebuilt():
    P = box_problem(3, [3, 2, 4], 2, neumann=[(5, 2, -1e6)])
    try:
        nc = P.desc.n_cells
        rng = np.random.default_rng(9)
        p = 1e7 * (1 + 0.1 * np.sin(0.7 * np.arange(P.desc.n_dofs_p)))
        kappa, rho = P.desc.mat.k_over_mu * 10.0 ** rng.random(nc), 2000.0 * 10.0 ** rng.random(nc)

        def vectors(C):
            return tuple(v.tobytes() for v in C.gravity_vectors()) + rhs_and_residual_keep_matrix(C)

        def rhs_and_residual_keep_matrix(C):
            C.set(pk.VEC_P, p); C.set(pk.VEC_P_OLD, 0.9 * p); C.fill(pk.VEC_EPSV, 0.0); C.fill(pk.VEC_EPSV0, 0.0)
            C.disp_assemble_system(False)
            C.pres_assemble_residual(60.0)
            return C.get(pk.VEC_RHS_U).tobytes(), C.get(pk.VEC_RESIDUAL_P).tobytes()
        # gravity and density before the first assembly and before the permeability
        A = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        A.set_cell_density(rho); A.set_gravity(G3, 2700.0, RHO_F); A.set_cell_permeability(kappa)
        first = vectors(A); A.close()
        # ... after both
        B = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        B.timers_enable(1)
        B.set_cell_permeability(kappa)
        B.set(pk.VEC_P, p); B.disp_assemble_system(True)
        built = B.timer("assemble_u_matrix")[1]
        assert built == 1
        B.set_gravity(G3, 2700.0, RHO_F); B.set_cell_density(rho)
        assert vectors(B) == first
        # changing gravity and the density again: the load vector alone follows, the matrix block is not run again
        B.set_gravity(2 * G3, 2000.0, 900.0); B.set_cell_density(None)
        assert vectors(B) != first
        B.set_cell_density(rho); B.set_gravity(G3, 2700.0, RHO_F)
        assert vectors(B) == first
        # the permeability setters rebuild the flux while gravity is on
        B.set_cell_permeability(None)
        assert vectors(B)[1] != first[1]
        B.set_cell_permeability(kappa)
        assert vectors(B) == first
        assert B.timer("assemble_u_matrix")[1] == built and B.timer("assemble_u_rhs")[1] >= 5
        B.close()
    finally:
        P.close()


def test_refusals_leave_the_context_as_it_was():
    P = box_problem(2, [3, 4], 2)
    C = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        n = P.desc.n_cells
        rho = np.linspace(2000.0, 2600.0, n)
        C.set_cell_density(rho); C.set_gravity([0.0, -9.81], 2700.0, RHO_F)
        before = tuple(v.tobytes() for v in C.gravity_vectors())
        with pytest.raises(RuntimeError, match=f"n_cells is {n + 1}, the context has {n} cells"):
            C.set_cell_density(np.ones(n + 1))
        with pytest.raises(RuntimeError, match="value of cell 3 is not finite and > 0"):
            C.set_cell_density(np.r_[rho[:3], 0.0, rho[4:]])
        with pytest.raises(RuntimeError, match=f"value of cell {n - 1} is not finite"):
            C.set_cell_density(np.r_[rho[:-1], np.inf])
        with pytest.raises(RuntimeError, match="bulk_density"):
            C.set_gravity([0.0, -9.81], -1.0, RHO_F)
        with pytest.raises(RuntimeError, match="component 1 of g"):
            C.set_gravity([0.0, np.nan], 2700.0, RHO_F)
        got, kind = C.get_cell_density()
        assert np.array_equal(got, rho) and kind == 2 and tuple(v.tobytes() for v in C.gravity_vectors()) == before
        g, rho_b, rho_f, on = C.get_gravity()
        assert np.array_equal(g, [0.0, -9.81]) and (rho_b, rho_f, on) == (2700.0, RHO_F, True)
    finally:
        C.close(); P.close()


# ---- 6. slab partitions -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3], ids=str)
def test_scalar_gravity_on_slab_ranks(world):
    """2 x 2 x 6 Q2 on two and three slabs: the stitched right-hand side and residual equal the single rank's to 1e-13 of the maximum; a per-cell density is refused"""
    dim, n, deg = 3, (2, 2, 6), 2
    S1 = slab_ranks.Slabs(dim, n, deg, 1); S = slab_ranks.Slabs(dim, n, deg, world)
    try:
        p = 1e7 * (1 + 0.1 * np.sin(0.7 * np.arange(S1.N_p)))

        def work(slabs):
            def fn(r, P, comm):
                C = slab_ranks.context(P, r, comm)
                try:
                    if slabs.world > 1:
                        with pytest.raises(RuntimeError, match="partitioned contexts are not supported"):
                            C.set_cell_density(np.full(P.desc.n_cells, 2500.0))
                    C.set_gravity(G3, 2700.0, RHO_F)
                    pw = slabs.window_p(p, r)
                    C.set(pk.VEC_P, pw); C.set(pk.VEC_P_OLD, 0.9 * pw); C.fill(pk.VEC_EPSV, 0.0); C.fill(pk.VEC_EPSV0, 0.0)
                    C.disp_assemble_system(True)
                    C.pres_assemble_residual(60.0)
                    return C.get(pk.VEC_RHS_U), C.get(pk.VEC_RESIDUAL_P)
                finally:
                    C.close()
            parts = slabs.run(fn)
            return slabs.stitch_u([a for a, _ in parts]), slabs.stitch_p([b for _, b in parts])
        rhs1, res1 = work(S1)
        rhs, res = work(S)
        eu, ep = np.abs(rhs - rhs1).max() / np.abs(rhs1).max(), np.abs(res - res1).max() / np.abs(res1).max()
        print(f"{world} slabs: rhs_u {eu:.2e} residual {ep:.2e} of the maximum")
        assert eu <= 1e-13 and ep <= 1e-13
        # and the single rank's vectors hold the gravity terms of the reference
        P1 = S1.problems[0]
        C = pk.Context(P1, 0, pk.OP_MATRIX_FREE)
        try:
            C.set_gravity(G3, 2700.0, RHO_F)
            b, f = C.gravity_vectors()
            assert np.abs(b - body_force(P1, G3, 2700.0)).max() <= 1e-12 * np.abs(b).max()
            assert np.abs(f - gravity_flux(P1, G3, RHO_F, P1.desc.mat.k_over_mu)).max() <= 1e-12 * np.abs(f).max()
        finally:
            C.close()
    finally:
        S.close(); S1.close()


# ---- 7. runs through the host driver ----------------------------------------------------------------------------------------------------------------------------------------
H_COL = 10.0


def drained_column(rho_b, hydrostatic=False):
    """the drained 2D column of tests/test_terzaghi.py (Q2, 2 x 12) without the traction: rollers on the sides and the bottom, drained top, gravity along -y"""
    bc = [(0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0)]
    m = material(flow_rate=0.0)
    P = pk.Problem.box(2, [2, 12], [10.0, H_COL], 2, m, bc)
    P.set_pressure_bc([(3, 0.0)])
    P.set_gravity([0.0, -9.81], RHO_F, rho_b, hydrostatic_init=hydrostatic)
    return P, m


def column_fields(P, G):
    pos, comp = GeneralReference(P).node_coords()
    depth = H_COL / 2 - vertex_of_dof_p(P)[:, 1]
    z = pos[:, 1] + H_COL / 2
    return depth, z, comp, G.get(pk.VEC_P), G.get(pk.VEC_U)


def run_tolerances(m):
    """the fixed-stress loop stops on absolute residual norms: 1e-9 of the size of one entry of the gravity flux (k / mu rho_f |g| h_x)"""
    tol = 1e-9 * m.k_over_mu * RHO_F * 9.81 * 5.0
    return dict(fss_tol=tol, pressure_tol=tol, max_fss=200, max_it=50000)


def test_a_run_settles_into_the_steady_state_under_gravity():
    """backward Euler damps the slowest consolidation mode by 1 / (1 + lambda_1 dt) per step, lambda_1 = pi^2 c_v / (4 H^2), c_v = (k / mu) / (alpha^2 / (lambda + 2G) + 1 / M).
    For the material of input.data c_v = 0.045 m^2 / s and lambda_1 = 1.1e-3 / s; dt = 1e5 s gives 1 + lambda_1 dt = 112 and n = 4 steps 112^-4 = 6.3e-9 <= 1e-8.
    Then p = rho_f |g| depth and u_y = (rho_b - alpha rho_f) |g| (z^2 / 2 - H z) / (lambda + 2G), each to 1e-6 of its maximum"""
    rho_b = 2700.0
    P, m = drained_column(rho_b)
    try:
        kv = m.lame_lambda + 2 * m.shear_G
        cv = m.k_over_mu / (m.biot_alpha ** 2 / kv + 1.0 / m.biot_M)
        lam1 = math.pi ** 2 * cv / (4 * H_COL ** 2)
        dt, n = 1.0e5, 4
        assert (1 + lam1 * dt) ** -n <= 1e-8, (cv, lam1, (1 + lam1 * dt) ** -n)
        tr, G = pk.run_problem(P, n, 0.0, dt, operator_mode=pk.OP_MATRIX_FREE, prec=pk.PREC_CHEBYSHEV, coupled_fss=True, incremental_strain=True, **run_tolerances(m))
        depth, z, comp, p, u = column_fields(P, G)
        G.close()
        p_exact = RHO_F * 9.81 * depth
        u_exact = np.where(comp == 1, (rho_b - m.biot_alpha * RHO_F) * 9.81 * (z ** 2 / 2 - H_COL * z) / kv, 0.0)
        ep, eu = np.abs(p - p_exact).max() / np.abs(p_exact).max(), np.abs(u - u_exact).max() / np.abs(u_exact).max()
        print(f"steady state after {n} steps of {dt:g} s ({len(tr) - 1} fixed-stress iterations): p {ep:.2e} u {eu:.2e} of the maximum")
        assert ep <= 1e-6 and eu <= 1e-6
    finally:
        P.close()


def test_a_hydrostatic_start_with_neutral_weight_stays_at_rest():
    """hydrostatic_init and rho_b = alpha rho_f: the body force balances the pressure gradient, u = 0 and p = p_h from the first step on"""
    m0 = material(flow_rate=0.0)
    P, m = drained_column(m0.biot_alpha * RHO_F, hydrostatic=True)
    try:
        kv = m.lame_lambda + 2 * m.shear_G
        u_scale = (2700.0 - m.biot_alpha * RHO_F) * 9.81 * H_COL ** 2 / 2 / kv           # max|u| of the column above
        for steps in (1, 2):
            tr, G = pk.run_problem(P, steps, 0.0, 60.0, operator_mode=pk.OP_MATRIX_FREE, prec=pk.PREC_CHEBYSHEV, coupled_fss=True, incremental_strain=True, **run_tolerances(m))
            depth, z, comp, p, u = column_fields(P, G)
            G.close()
            p_h = RHO_F * 9.81 * depth
            ep, eu = np.abs(p - p_h).max() / p_h.max(), np.abs(u).max() / u_scale
            print(f"hydrostatic start, {steps} step(s): p {ep:.2e} of max p_h, u {eu:.2e} of the self-weight column's maximum")
            assert ep <= 1e-6 and eu <= 1e-6
    finally:
        P.close()


def test_an_adaptive_run_carries_gravity_and_density():
    """refine_every = 1, two steps, 3D Q1: the run ends on an adapted mesh with the density inherited from the coarse cells and the hydrostatic identity holding there"""
    n = [3, 3, 4]
    m = material()
    P = pk.Problem.refined_box_mask(3, n, [3.0, 3.0, 4.0], 1, m, [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)], np.zeros(int(np.prod(n)), dtype=np.int32))
    try:
        rho_c = 2000.0 + 100.0 * np.arange(P.desc.n_cells)
        g = np.array([0.0, 0.0, -9.81])
        tr, G = pk.run_problem(P, 2, 10e6, 60.0, operator_mode=pk.OP_MATRIX_FREE, max_it=5000, refine_every=1, gravity=g, fluid_density=RHO_F, density=rho_c, hydrostatic_init=True)
        try:
            Q = G.problem
            assert Q is not P and Q.desc.n_cells > P.desc.n_cells
            coarse, child = Q.cell_parents()
            assert (child >= 0).any() and np.array_equal(Q.cell_density(), rho_c[coarse])
            got, kind = G.get_cell_density()
            assert np.array_equal(got, rho_c[coarse]) and kind == 2
            gg, rho_b, rho_f, on = G.get_gravity()
            assert on and np.array_equal(gg, g) and rho_f == RHO_F
            b, f = G.gravity_vectors()
            assert np.abs(b - body_force(Q, g, rho_c[coarse])).max() <= 1e-12 * np.abs(b).max()
            # the hydrostatic identity on the last mesh (the well is part of src: take it out through PORO_VEC_SOURCE_P, which keeps meaning the well alone)
            p_h = RHO_F * vertex_of_dof_p(Q) @ g
            G.set(pk.VEC_P, p_h); G.set(pk.VEC_P_OLD, p_h); G.fill(pk.VEC_EPSV, 0.0); G.fill(pk.VEC_EPSV0, 0.0)
            G.pres_assemble_residual(60.0)
            R = G.get(pk.VEC_RESIDUAL_P) + condensed_source(Q, G)
            print(f"adapted mesh, {Q.desc.n_cells} cells: max|R + C^T src| = {np.abs(R).max() / np.abs(f).max():.2e} max|f_g|")
            assert np.abs(R).max() <= 1e-12 * np.abs(f).max()
        finally:
            G.close()
            if G.problem is not P:
                G.problem.close()
    finally:
        P.close()


def condensed_source(Q, G):
    """C^T src of the well source (hanging rows folded into their masters, as the residual is), from the descriptor's constraint list"""
    s = G.get(pk.VEC_SOURCE_P).copy()
    c = Q.desc.cons_p
    if c.n:
        dof = np.ctypeslib.as_array(c.dof, shape=(c.n,)); ptr = np.ctypeslib.as_array(c.ptr, shape=(c.n + 1,))
        master = np.ctypeslib.as_array(c.master, shape=(ptr[-1],)); w = np.ctypeslib.as_array(c.weight, shape=(ptr[-1],))
        for i, d in enumerate(dof):
            s[master[ptr[i]:ptr[i + 1]]] += w[ptr[i]:ptr[i + 1]] * s[d]
            s[d] = 0.0
    return s


# ---- 8. the command-line driver ---------------------------------------------------------------------------------------------------------------------------------------------
def test_driver_gravity_options():
    exe = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
    r = subprocess.run([exe, INPUT_DATA, "--matrix-free", "--gravity", "0,-9.81", "--fluid-density", "1000", "--hydrostatic-init"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "gravity: on, g = (0, -9.81), bulk density 2700, density layers: 0 (field kind 0), fluid density 1000, hydrostatic start: yes" in r.stdout
    r = subprocess.run([exe, INPUT_DATA, "--degree", "1", "--matrix-free", "--steps", "2", "--refine-every", "1", "--gravity", "0,-9.81", "--density-layers", "0=2000,5=2600"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"adapted before step \d+: gravity: on, g = \(0, -9.81\), bulk density 2700, density layers: 2 \(field kind 2\)", r.stdout)
    r = subprocess.run([exe, INPUT_DATA, "--gravity", "0,-9.81,1,2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "GX,GY[,GZ]" in r.stderr
    r = subprocess.run([exe, INPUT_DATA, "--gravity", "0,0,-9.81"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "2 components" in r.stderr

"""Gravity without a GPU: the closed forms of the box kernels (csrc/gravity_weights.hpp, through a small stand-alone program built with the address and
undefined-behaviour sanitizers), the NumPy reference of the two gravity vectors against its own identities on a jittered mesh, the host layer (layers by cell centres,
inheritance through a refine / coarsen pair, refusals, the hydrostatic start's arguments) and the exported symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import build_sanitized_check, centres, layered_field_problems, material, refine_and_coarsen_pair
from general_reference import jitter, mapped
from gravity_reference import body_force, cell_volumes, gravity_flux, laplace_apply, vertex_of_dof_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("poro_ctx_set_gravity", "poro_ctx_get_gravity", "poro_ctx_set_cell_density", "poro_ctx_get_cell_density", "poro_get_gravity_vectors")


def test_symbols_and_abi():
    hip = pk.load_hip()
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    assert re.search(r"#define PORO_ABI_VERSION 4\b", header) and hip.poro_abi_version() == 4
    for s in NEW_SYMBOLS:
        assert s in pk.HIP_SYMBOLS and getattr(hip, s) and re.search(r"\bint\s+" + s + r"\(", header)


def test_closed_forms_under_the_sanitizers(tmp_path):
    """gravity_weights.hpp through tests/gravity_check.cpp: the 1D weights sum to h, the +- pattern sums to 0 per cell, every value agrees with Gauss quadrature"""
    exe = build_sanitized_check(tmp_path, "gravity_check")
    for h in ((1.0, 1.0, 1.0), (0.7, 1.3, 2.9), (1e-3, 4.0, 250.0)):
        r = subprocess.run([exe] + [repr(v) for v in h], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
        # the printed weights themselves: h / 2, h / 2 and h / 6, 4 h / 6, h / 6
        got = {(int(m[0]), int(m[1]), float(m[2])): float(m[3]) for m in re.findall(r"weight k=(\d) s=(\d) h=(\S+): (\S+)", r.stdout)}
        for hd in h:
            assert [got[(1, s, hd)] for s in range(2)] == [hd / 2, hd / 2] and [got[(2, s, hd)] for s in range(3)] == [hd / 6, 4 * hd / 6, hd / 6]


@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 1), (3, 2)], ids=str)
def test_numpy_reference_satisfies_the_identities_on_a_jittered_mesh(dim, deg):
    """non-affine cells, every g component non-zero, density and permeability random over a decade per cell: K_kappa p_h + f_g = 0 for p_h = rho_f g . x + const,
    sum f_g = 0, sum b[component d] = g_d sum_c rho_c |c| - each to 1e-12 of the sum of the absolute values of its summands"""
    n = [3, 2, 2][:dim]
    B = pk.Problem.box(dim, n, [3.0, 2.0, 2.5][:dim], deg, material(), [(0, 0, 0.0)])
    P = mapped(B, jitter(B))
    try:
        rng = np.random.default_rng(11)
        nc = P.desc.n_cells
        g = np.array([1.7, -2.3, -9.81])[:dim]; rho_f = 1000.0
        rho = 2000.0 * 10.0 ** rng.random(nc)
        b = body_force(P, g, rho)
        vol = cell_volumes(P)
        assert vol.sum() == pytest.approx(np.prod([3.0, 2.0, 2.5][:dim]), rel=1e-13)
        cdu = np.ctypeslib.as_array(P.desc.cell_dofs_u, shape=(nc, (deg + 1) ** dim * dim))
        for d in range(dim):
            dofs = np.unique(cdu[:, d::dim])
            assert abs(b[dofs].sum() - g[d] * (rho * vol).sum()) <= 1e-12 * np.abs(b[dofs]).sum()
        X = vertex_of_dof_p(P)
        p_h = rho_f * X @ g + 3.0e4
        for kappa in (2.5e-12, 1e-12 * 10.0 ** rng.random(nc), 1e-12 * 10.0 ** rng.random((nc, dim))):
            f = gravity_flux(P, g, rho_f, kappa)
            assert abs(f.sum()) <= 1e-12 * np.abs(f).sum()
            r = laplace_apply(P, kappa, p_h) + f
            assert np.abs(r).max() <= 1e-12 * np.abs(f).max(), np.abs(r).max() / np.abs(f).max()
    finally:
        P.close()


# ---- host layer ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_density_layers_by_cell_centres_and_validation():
    layers = [(-1.0, 2700.0), (0.5, 1900.0), (2.0, 2300.0)]
    for P in layered_field_problems():
        try:
            assert P.cell_density() is None and P.gravity()[0] is None
            P.set_density_layers(layers)
            idx = np.searchsorted([l[0] for l in layers], centres(P)[:, -1], side="left")
            assert len(set(idx)) == 3 and np.array_equal(P.cell_density(), np.array([l[1] for l in layers])[idx])
            n = P.desc.n_cells
            with pytest.raises(RuntimeError, match="above every layer"):
                P.set_density_layers(layers[:2])
            with pytest.raises(RuntimeError, match="values for"):
                P.set_cell_density(np.ones(n + 1))
            with pytest.raises(RuntimeError, match=f"cell {n - 1} is not finite and > 0"):
                P.set_cell_density(np.r_[np.ones(n - 1), 0.0])
            with pytest.raises(RuntimeError, match="cell 2 is not finite and > 0"):
                P.set_cell_density(np.r_[1.0, 1.0, -3.0, np.ones(n - 3)])
            with pytest.raises(RuntimeError, match="cell 0 is not"):
                P.set_cell_density(np.r_[np.nan, np.ones(n - 1)])
            assert np.array_equal(P.cell_density(), np.array([l[1] for l in layers])[idx])      # a refused call leaves the field
            P.set_cell_density(None)
            assert P.cell_density() is None
            # the scalars: the bulk density defaults to the parameter file's declared default and is kept unless given
            assert P.gravity()[1:] == (0.0, pk.read_input().bulk_density, False)
            P.set_gravity([0.0, 0.0, -9.81], 1000.0, hydrostatic_init=True)
            g, rho_f, rho_b, hyd = P.gravity()
            assert np.array_equal(g, [0.0, 0.0, -9.81]) and (rho_f, rho_b, hyd) == (1000.0, pk.read_input().bulk_density, True)
            P.set_gravity([1.0, 0.0, 0.0], 0.0, bulk_density=2100.0)
            assert P.gravity()[1:] == (0.0, 2100.0, False)
            with pytest.raises(ValueError, match="3 components"):
                P.set_gravity([0.0, -9.81])
            with pytest.raises(RuntimeError, match="fluid density"):
                P.set_gravity([0.0, 0.0, -9.81], -1.0)
            P.set_gravity(None)
            assert P.gravity()[0] is None
        finally:
            P.close()


def test_density_inheritance_through_a_refine_and_a_coarsen():
    A, B, nc = refine_and_coarsen_pair()
    try:
        ca, _ = A.cell_parents(); cb, _ = B.cell_parents()
        rho_c = 2000.0 + 500.0 * np.random.default_rng(7).random(nc)
        A.set_cell_density(rho_c[ca]); A.set_gravity([0.0, 0.0, -9.81], 1000.0, 2500.0, hydrostatic_init=True)
        B.inherit_cell_density(A)
        assert np.array_equal(B.cell_density(), rho_c[cb])                                       # a child takes its parent's value, exactly
        g, rho_f, rho_b, hyd = B.gravity()
        assert np.array_equal(g, [0.0, 0.0, -9.81]) and (rho_f, rho_b, hyd) == (1000.0, 2500.0, True)      # the scalars go along
        ra = rho_c[ca].copy(); ra[np.flatnonzero(ca == 1)] = np.arange(1.0, 9.0)
        A.set_cell_density(ra); B.inherit_cell_density(A)
        rb = B.cell_density()
        assert rb[cb == 1] == pytest.approx(4.5, abs=0) and np.array_equal(rb[cb != 1], rho_c[cb][cb != 1])      # a coarsened parent: the mean of its children
        A.set_cell_density(None); B.inherit_cell_density(A)
        assert B.cell_density() is None
    finally:
        A.close(); B.close()

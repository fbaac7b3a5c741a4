"""Mechanical post-processing without a GPU: the exported symbols and prototypes, csrc/stress_measures.hpp through a small stand-alone program built with the address
and undefined-behaviour sanitizers (eigenvalues of degenerate states against NumPy), the NumPy reference (tests/stress_reference.py) against the patch identities
on a jittered mesh, and the (label, component) every Dirichlet dof gets."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import ROLLERS3, build_sanitized_check, material
from general_reference import GeneralReference, cell_vertices, jitter, mapped
from stress_reference import cell_stress, component_table, force_balance, full_tensor, measures_of
from darcy_reference import vertex_of_dof_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("poro_disp_cell_stress", "poro_disp_cell_measures", "poro_disp_force_balance")


def test_symbols_prototypes_and_abi():
    hip, host = pk.load_hip(), pk.load_host()
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    assert re.search(r"#define PORO_ABI_VERSION 4\b", header) and hip.poro_abi_version() == 4
    for s in NEW_SYMBOLS:
        assert s in pk.HIP_SYMBOLS and getattr(hip, s) and re.search(r"\bint\s+" + s + r"\(", header)
    for t in ("poro_mohr_coulomb", "poro_failure_summary", "poro_force_balance_terms"):
        assert re.search(r"typedef struct " + t + r" \{", header)
    assert getattr(host, "poro_host_displacement_bc_labels")
    for name in ("cell_stress", "cell_measures", "force_balance"):
        assert callable(getattr(pk.Context, name))
    assert callable(pk.Problem.displacement_bc_labels)
    # the structures member by member
    assert [f[0] for f in pk.ForceBalanceTerms._fields_] == ["reaction_sum", "free_row_sum", "traction_sum", "body_sum", "coupling_sum", "residual_l2"]
    assert C_sizeof(pk.ForceBalanceTerms) == 16 * 8 and C_sizeof(pk.FailureSummary) == 24 and C_sizeof(pk.MohrCoulomb) == 16


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_measures_header_under_the_sanitizers(tmp_path):
    """stress_measures.hpp through tests/stress_measures_check.cpp: for every printed state the three principal values against numpy.linalg.eigvalsh to 1e-14 of max|s|,
    mean and von Mises to the same bound, f against its formula (c = 2e6, phi = 0.5)"""
    exe = build_sanitized_check(tmp_path, "stress_measures_check")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("stress_measures_check ok"), r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"^(\w+): s (.*) -> (.*)$", r.stdout, flags=re.M)
    names = [n for n, _, _ in rows]
    for want in ("triple", "double_axis", "pure_shear", "double_rotated", "double_perturbed", "triple_perturbed", "plane_zz_largest", "plane_zz_middle", "plane_zz_smallest"):
        assert want in names
    for name, s, m in rows:
        s = np.array([float(x) for x in s.split()]); m = np.array([float(x) for x in m.split()])
        T = full_tensor(s[None, [0, 1, 2, 3, 4, 5]], 3)
        ref = measures_of(T, 2.0e6, 0.5)[0]
        scale = np.abs(s).max()
        err = np.abs(m[:5] - ref[:5]).max()
        print(f"{name}: principal values off by {np.abs(m[:3] - ref[:3]).max() / scale if scale else 0.0:.2e} of max|s|")
        assert err <= 1e-14 * scale, (name, m, ref)
        f = 0.5 * (m[0] - m[2]) + 0.5 * (m[0] + m[2]) * np.sin(0.5) - 2.0e6 * np.cos(0.5)
        assert abs(m[5] - f) <= 1e-14 * (scale + 2.0e6), (name, m[5], f)
    # the plane-strain states put zz where their name says
    for name, s, m in rows:
        if name.startswith("plane_zz_"):
            zz = float(s.split()[5]); m = [float(x) for x in m.split()]
            assert zz == m[{"largest": 0, "middle": 1, "smallest": 2}[name.split("_")[-1]]]


def jittered(dim, k):
    B = pk.Problem.box(dim, [3, 2, 4][:dim], [3.0, 2.0, 2.5][:dim], k, material(), [(0, 0, 0.0)])
    return mapped(B, jitter(B))


@pytest.mark.parametrize("k", [1, 2], ids=["q1", "q2"])
@pytest.mark.parametrize("dim", [2, 3], ids=str)
def test_numpy_reference_satisfies_the_patch_identities_on_a_jittered_mesh(dim, k):
    """non-affine cells.  u = B x + c at the support points gives eps = sym B in every cell; p = a . x + p0 gives sigma = sigma' - alpha p(x_c) I; a rigid rotation plus
    translation gives eps = 0 to 1e-12 of |B|; the rows of A_full of one component sum to zero and the coupling vector sums to zero per component"""
    P = jittered(dim, k)
    try:
        d = P.desc
        rng = np.random.default_rng(5)
        R = GeneralReference(P)
        B = rng.standard_normal((dim, dim)) * 1e-4
        u = R.linear_field(B) + 1e-4 * rng.standard_normal(dim)[component_table(P)]     # (a translation of the size of B x: the entries of u round to eps max|u|)
        Xp = vertex_of_dof_p(P)
        a = np.array([0.7e4, -1.3e4, 2.1e4])[:dim]
        p = Xp @ a + 5.0e5
        lam, G = 10.0 ** rng.uniform(9, 10, d.n_cells), 10.0 ** rng.uniform(9, 10, d.n_cells)
        alpha = 0.9
        e, se, st = cell_stress(P, u, p, lam, G, alpha)
        symB = 0.5 * (B + B.T)
        E = full_tensor(e, dim, 0.0)[:, :dim, :dim]
        assert np.abs(E - symB[None]).max() <= 1e-12 * np.abs(B).max()
        want = lam[:, None, None] * np.trace(symB) * np.eye(dim)[None] + 2 * G[:, None, None] * symB[None]
        S = full_tensor(se, dim, 0.0)[:, :dim, :dim]
        assert np.abs(S - want).max() <= 1e-12 * np.abs(want).max()
        # x_c, the image of the reference centre under MappingQ1, is the mean of the cell's vertices
        xc = P.coords[cell_vertices(d)].mean(axis=1)
        T = full_tensor(st, dim, 0.0)[:, :dim, :dim]
        wantT = want - alpha * (xc @ a + 5.0e5)[:, None, None] * np.eye(dim)[None]
        assert np.abs(T - wantT).max() <= 1e-12 * np.abs(wantT).max()
        W = rng.standard_normal((dim, dim)); W = 1e-4 * (W - W.T)
        e0 = cell_stress(P, R.linear_field(W) + 3e-5, None, lam, G, alpha)[0]
        assert np.abs(e0).max() <= 1e-12 * np.abs(W).max()
        # the identity behind the force balance, on a random state: sum of r over component k = -(sum of the loads)
        ref = force_balance(P, rng.standard_normal(d.n_dofs_u) * 1e-4, p, lam, G, alpha, g=np.array([1.7, -2.3, -9.81])[:dim], rho=2000.0 + 500 * rng.random(d.n_cells))
        t = ref["terms"]
        ident = t["reaction_sum"] + t["free_row_sum"] + t["traction_sum"] + t["body_sum"] + t["coupling_sum"]
        assert np.all(np.abs(ident) <= 1e-12 * ref["total"]), (ident, ref["total"])
        assert np.all(np.abs(t["coupling_sum"]) <= 1e-12 * ref["scales"]["coupling_sum"])
        assert np.all(np.abs(t["body_sum"]) > 0)
    finally:
        P.close()


def test_dirichlet_dofs_carry_label_and_component_of_the_first_condition():
    """3 x 2 x 2 box, Q2.  Conditions (label 0, comp 0), (label 4, comp 0), (label 4, comp 2): the component-0 dofs of the edge shared by the faces x = low and
    z = low go to whichever of the first two conditions is listed first, exactly as their values do; every dof's component is the component of its condition"""
    for order in ([(0, 0, 1.0), (4, 0, 2.0), (4, 2, 3.0)], [(4, 0, 2.0), (0, 0, 1.0), (4, 2, 3.0)]):
        P = pk.Problem.box(3, [3, 2, 2], [3.0, 2.0, 2.0], 2, material(), order)
        try:
            d = P.desc
            dofs = np.ctypeslib.as_array(d.dirichlet_dof, shape=(d.n_dirichlet,)).copy()
            vals = np.ctypeslib.as_array(d.dirichlet_value, shape=(d.n_dirichlet,)).copy()
            lab = P.displacement_bc_labels()
            assert lab.shape == (d.n_dirichlet, 2)
            comp = component_table(P)
            assert np.array_equal(lab[:, 1], comp[dofs])
            R = GeneralReference(P)
            X, _ = R.node_coords()
            on_x, on_z = np.abs(X[dofs, 0] - X[:, 0].min()) < 1e-12, np.abs(X[dofs, 2] - X[:, 2].min()) < 1e-12
            c0 = comp[dofs] == 0
            first = order[0][0]
            want = np.where(~c0, 4, np.where(on_x & on_z, first, np.where(on_x, 0, 4)))
            assert np.array_equal(lab[:, 0], want) and (c0 & on_x & on_z).sum() == 5
            assert np.array_equal(vals, np.where(~c0, 3.0, np.where(want == 0, 1.0, 2.0)))
        finally:
            P.close()
    P = pk.Problem.box(2, [2, 2], [1.0, 1.0], 1, material(), [])
    try:
        assert P.displacement_bc_labels().shape == (0, 2)
    finally:
        P.close()
    # the lists and values themselves are what they were: the rollers of a refined box, whose hanging dofs leave the list, keep labels in step
    mask = np.zeros(8, dtype=np.int32); mask[0] = 1
    Rf = pk.Problem.refined_box_mask(3, [2, 2, 2], [2.0, 2.0, 2.0], 1, material(), ROLLERS3, mask)
    try:
        d = Rf.desc
        lab = Rf.displacement_bc_labels()
        dofs = np.ctypeslib.as_array(d.dirichlet_dof, shape=(d.n_dirichlet,))
        assert lab.shape == (d.n_dirichlet, 2) and np.array_equal(lab[:, 1], component_table(Rf)[dofs]) and set(lab[:, 0].tolist()) == {0, 2, 4}
    finally:
        Rf.close()

"""Flow post-processing without a GPU: the face quadrature of the boundary discharge (csrc/darcy_faces.hpp, through a small stand-alone program built with the address
and undefined-behaviour sanitizers), the NumPy reference (tests/darcy_reference.py) against the identities I1-I3 on a jittered mesh, the label every prescribed
pressure dof gets, and the exported symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import ROLLERS3, build_sanitized_check, material
from darcy_reference import cell_velocity, face_discharge, face_measures, mesh, per_cell, vertex_of_dof_p
from general_reference import SHEAR, jitter, mapped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("poro_pres_darcy_velocity", "poro_pres_boundary_discharge", "poro_pres_flow_balance")
G3 = np.array([1.7, -2.3, -9.81])
RHO_F = 1000.0


def test_symbols_and_abi():
    hip, host = pk.load_hip(), pk.load_host()
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    assert re.search(r"#define PORO_ABI_VERSION 4\b", header) and hip.poro_abi_version() == 4
    for s in NEW_SYMBOLS:
        assert s in pk.HIP_SYMBOLS and getattr(hip, s) and re.search(r"\bint\s+" + s + r"\(", header)
    assert not re.search(r"poro_flow_balance_terms\s*\(", header)
    for s in ("poro_host_runner_flow_balance", "poro_host_runner_track_flow", "poro_host_runner_postprocess_darcy", "poro_host_pressure_bc_labels"):
        assert getattr(host, s)
    for name in ("darcy_velocity", "boundary_discharge", "flow_balance"):
        assert callable(getattr(pk.Context, name))
    for name in ("darcy_velocity", "flow_balance", "track_flow_balance"):
        assert callable(getattr(pk.Runner, name))


def test_face_tables_under_the_sanitizers(tmp_path):
    """darcy_faces.hpp through tests/darcy_faces_check.cpp: on a unit and a sheared cell, 2D and 3D, every local face has an outward n dS and its weights sum to the
    face measure; the printed measures against NumPy (unit cell: 1; sheared: the image edge / parallelogram)"""
    exe = build_sanitized_check(tmp_path, "darcy_faces_check")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("darcy_faces_check ok"), r.stdout[-2000:] + r.stderr[-2000:]
    got = {(m[0], int(m[1])): (float(m[2]), float(m[3])) for m in re.findall(r"(\w+) face (\d): sign (\S+) tangents \S+ \S+ measure (\S+)", r.stdout)}
    for dim in (2, 3):
        for f in range(2 * dim):
            d = f >> 1
            assert got[(f"unit{dim}", f)] == (1.0 if f & 1 else -1.0, 1.0)
            A = SHEAR[dim]
            tang = [a for a in range(dim) if a != d]
            want = np.linalg.norm(A[:, tang[0]]) if dim == 2 else np.linalg.norm(np.cross(A[:, tang[0]], A[:, tang[1]]))
            assert abs(got[(f"shear{dim}", f)][1] - want) <= 1e-14 * want
    assert len(got) == 2 * (4 + 6)


def jittered(dim):
    n = [3, 2, 4][:dim]
    B = pk.Problem.box(dim, n, [3.0, 2.0, 2.5][:dim], 1, material(), [(0, 0, 0.0)])
    return mapped(B, jitter(B))


@pytest.mark.parametrize("dim", [2, 3], ids=str)
def test_numpy_reference_satisfies_the_identities_on_a_jittered_mesh(dim):
    """non-affine cells, every g component non-zero, permeability random over a decade per cell and component.
    I1: p_h = a . x + b gives q_c = -kappa_c (a - rho_f g) in every cell; I2: p_h = rho_f g . x gives q = 0 and every Q_b = 0 to 1e-12 max|kappa rho_f g| |F|;
    I3: scalar kappa and linear p_h give sum_b Q_b = 0 over the closed boundary to 1e-12 sum |Q_b|"""
    P = jittered(dim)
    try:
        rng = np.random.default_rng(7)
        nc = P.desc.n_cells
        g = G3[:dim]; rg = RHO_F * g
        X = vertex_of_dof_p(P)
        a = np.array([0.7e4, -1.3e4, 2.1e4])[:dim]
        p_lin = X @ a + 5.0e5
        A = face_measures(P)
        for kappa in (3.0e-11, 1e-11 * 10.0 ** rng.random(nc), 1e-11 * 10.0 ** rng.random((nc, dim))):
            kc = per_cell(kappa, nc, dim)
            for grav in (np.zeros(dim), rg):
                q = cell_velocity(P, p_lin, kappa, grav)
                want = -kc * (a - grav)[None, :]
                assert np.abs(q - want).max() <= 1e-12 * np.abs(want).max()                   # I1
            q0 = cell_velocity(P, X @ rg, kappa, rg)
            Q0 = face_discharge(P, X @ rg, kappa, rg)
            scale = np.abs(kc * rg[None, :]).max()
            assert np.abs(q0).max() <= 1e-12 * scale and np.all(np.abs(Q0) <= 1e-12 * scale * A)   # I2
        for grav in (np.zeros(dim), rg):
            Q = face_discharge(P, p_lin, 3.0e-11, grav)
            assert abs(Q.sum()) <= 1e-12 * np.abs(Q).sum() and np.abs(Q).max() > 0                 # I3
        # the measures: a closed surface, sum of n dS = 0 is what I3 rests on; here the total area of the jittered box stays near the box's
        assert 0.8 < A.sum() / (2 * sum(np.prod([s for k, s in enumerate([3.0, 2.0, 2.5][:dim]) if k != d]) for d in range(dim))) < 1.2
    finally:
        P.close()


def test_face_discharge_sign_on_a_unit_box():
    """1 x 1 x 1 cell, p = x: q = -kappa e_x, so fluid leaves through the low-x face (Q = +kappa |F|) and enters through the high-x face"""
    P = pk.Problem.box(3, [1, 1, 1], [2.0, 3.0, 5.0], 1, material(), ROLLERS3)
    try:
        X = vertex_of_dof_p(P)
        Q = face_discharge(P, X[:, 0], 2.0, np.zeros(3))
        _, _, _, _, _, (bc, bl, bid) = mesh(P)
        by_face = dict(zip(bl.tolist(), Q.tolist()))
        assert abs(by_face[0] - 2.0 * 15.0) <= 1e-12 * 30 and abs(by_face[1] + 2.0 * 15.0) <= 1e-12 * 30
        assert all(abs(by_face[f]) <= 1e-12 * 30 for f in (2, 3, 4, 5))
    finally:
        P.close()


def test_prescribed_dofs_carry_the_label_of_the_first_condition():
    """3 x 2 x 2 box, the faces x = high (label 1) and z = high (label 5) drained: the dofs of the shared edge go to whichever condition is listed first"""
    for order in ([(1, 0.0), (5, 2.0)], [(5, 2.0), (1, 0.0)]):
        P = pk.Problem.box(3, [3, 2, 2], [3.0, 2.0, 2.0], 1, material(), ROLLERS3)
        try:
            P.set_pressure_bc(order)
            d = P.desc
            dofs = np.ctypeslib.as_array(d.dirichlet_dof_p, shape=(d.n_dirichlet_p,)).copy()
            vals = np.ctypeslib.as_array(d.dirichlet_value_p, shape=(d.n_dirichlet_p,)).copy()
            labels = P.pressure_bc_labels()
            assert labels.shape == dofs.shape and len(dofs) == 3 * 3 + 4 * 3 - 3
            X = vertex_of_dof_p(P)[dofs]
            on_x, on_z = np.abs(X[:, 0] - X[:, 0].max()) < 1e-12, np.abs(X[:, 2] - X[:, 2].max()) < 1e-12
            first = order[0][0]
            want = np.where(on_x & on_z, first, np.where(on_x, 1, 5))
            assert np.array_equal(labels, want) and (on_x & on_z).sum() == 3
            assert np.array_equal(vals, np.where(want == 5, 2.0, 0.0))          # the value follows the same rule
        finally:
            P.close()
    # no condition: no labels
    P = pk.Problem.box(2, [2, 2], [1.0, 1.0], 1, material(), [(0, 0, 0.0)])
    try:
        assert P.pressure_bc_labels().size == 0
    finally:
        P.close()

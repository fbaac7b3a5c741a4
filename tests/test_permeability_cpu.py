"""Host layer of the per-cell permeability (no GPU): layers by cell centres, inheritance through the coarse cells of refined boxes, the exported symbols, the ABI number,
and the 1D coefficient builder of the line solve (csrc/perm_line.hpp, through a small stand-alone program) against numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import build_sanitized_check, centres, layered_field_problems, material, refine_and_coarsen_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_layers(P, layers):
    z = centres(P)[:, -1]
    tops = np.array([l[0] for l in layers]); vals = np.array([l[1] for l in layers])
    return vals[np.searchsorted(tops, z, side="left")]


def test_layers_by_cell_centres_on_graded_and_refined_boxes():
    layers = [(-1.0, 3.0), (0.5, 1e-3), (2.0, 7.0)]
    for P in layered_field_problems():
        try:
            assert P.cell_permeability() is None
            P.set_permeability_layers(layers)
            f = P.cell_permeability()
            assert f.shape == (P.desc.n_cells,) and np.array_equal(f, expected_layers(P, layers)) and len(set(f)) == 3
            with pytest.raises(RuntimeError, match="above every layer"):
                P.set_permeability_layers(layers[:2])
            with pytest.raises(RuntimeError, match="values for"):
                P.set_cell_permeability(np.ones(P.desc.n_cells + 1))
            with pytest.raises(RuntimeError, match="finite"):
                P.set_cell_permeability(np.r_[np.ones(P.desc.n_cells - 1), -1.0])
            assert np.array_equal(P.cell_permeability(), f)
            P.set_cell_permeability(None)
            assert P.cell_permeability() is None
        finally:
            P.close()


def test_inheritance_through_cell_parents():
    A, B, nc = refine_and_coarsen_pair()
    try:
        ca, _ = A.cell_parents(); cb, _ = B.cell_parents()
        per_coarse = 1.0 + np.random.default_rng(3).random(nc)
        A.set_cell_permeability(per_coarse[ca])
        B.inherit_cell_permeability(A)
        assert np.array_equal(B.cell_permeability(), per_coarse[cb])          # exactly: children and parents take their coarse cell's value
        # children set apart by the caller: a coarsened parent takes their mean, the others keep exact values
        fa = per_coarse[ca].copy(); kids = np.flatnonzero(ca == 1); fa[kids] = np.arange(1.0, 9.0)
        A.set_cell_permeability(fa); B.inherit_cell_permeability(A)
        fb = B.cell_permeability()
        assert fb[cb == 1] == pytest.approx(4.5, abs=0) and np.array_equal(fb[cb != 1], per_coarse[cb][cb != 1])
        A.set_cell_permeability(None); B.inherit_cell_permeability(A)
        assert B.cell_permeability() is None
    finally:
        A.close(); B.close()


def test_symbols_and_abi():
    hip, host = pk.load_hip(), pk.load_host()
    for s in ("poro_ctx_set_cell_permeability", "poro_ctx_get_cell_permeability", "poro_pres_apply_jacobian"):
        assert s in pk.HIP_SYMBOLS and getattr(hip, s)
    for s in ("poro_host_set_cell_permeability", "poro_host_set_permeability_layers", "poro_host_inherit_cell_permeability", "poro_host_get_cell_permeability"):
        assert getattr(host, s)
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    assert re.search(r"#define PORO_ABI_VERSION 4\b", header) and hip.poro_abi_version() == 4
    for s in ("poro_ctx_set_cell_permeability", "poro_ctx_get_cell_permeability", "poro_pres_apply_jacobian"):
        assert re.search(r"\bint\s+" + s + r"\(", header)


def test_line_coefficients_against_numpy(tmp_path):
    """perm_line.hpp through tests/perm_line_check.cpp (host-only, built here with the address and undefined-behaviour sanitizers and run directly)"""
    exe = build_sanitized_check(tmp_path, "perm_line_check")
    rng = np.random.default_rng(17)
    for n, lo, hi in ((1, 0, 0), (1, 1, 0), (3, 0, 1), (6, 1, 1), (7, 0, 0)):
        h = 0.5 + rng.random(n); k = 10.0 ** rng.uniform(-3, 1, n)
        out = subprocess.run([exe, "1", str(lo), str(hi)] + [repr(float(v)) for v in np.r_[h, k, k]], check=True, capture_output=True, text=True).stdout.split()     # one weight line = the Laplace weights
        got = np.array([float(v) for v in out]).reshape(6, n + 1)
        nl = n + 1
        M = np.zeros((nl, nl)); W = np.zeros((nl, nl)); K = np.zeros((nl, nl))
        for e in range(n):
            M[e:e + 2, e:e + 2] += h[e] / 6 * np.array([[2, 1], [1, 2]]); W[e:e + 2, e:e + 2] += k[e] * h[e] / 6 * np.array([[2, 1], [1, 2]])
            K[e:e + 2, e:e + 2] += k[e] / h[e] * np.array([[1, -1], [-1, 1]])
        for f, at in ((lo, 0), (hi, n)):
            if f:
                for A, d in ((M, 0.0), (W, 0.0), (K, 1.0)):
                    A[at, :] = 0; A[:, at] = 0; A[at, at] = d
        for r, A in ((0, M), (2, W), (4, K)):
            assert np.allclose(got[r], np.diag(A), rtol=1e-15, atol=0) and np.allclose(got[r + 1][:n], np.diag(A, 1), rtol=1e-15, atol=0) and got[r + 1][n] == 0

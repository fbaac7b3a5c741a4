"""Per-cell elastic moduli without a GPU: the 1D mathematics of the line solve (csrc/moduli_line.hpp, through a small stand-alone program built with the address and
undefined-behaviour sanitizers) against numpy, the NumPy model of the layered block inverse against a sparse direct solve of the reference's block diagonal, and the
exported symbols."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import poroelasticity_dealii_amd as pk
from common import build_sanitized_check, centres, layered_field_problems, material, refine_and_coarsen_pair
from moduli_reference import FDM_CASES, ModuliReference, fdm_problem, fe1d_weighted, layer_decades, layered_block_inverse, per_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_abi():
    hip = pk.load_hip()
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    assert re.search(r"#define PORO_ABI_VERSION 4\b", header) and hip.poro_abi_version() == 4
    for s in ("poro_ctx_set_cell_moduli", "poro_ctx_get_cell_moduli"):
        assert s in pk.HIP_SYMBOLS and getattr(hip, s) and re.search(r"\bint\s+" + s + r"\(", header)


def test_line_mathematics_under_the_sanitizers(tmp_path):
    """moduli_line.hpp through tests/moduli_line_check.cpp: band arrays against dense numpy matrices, the banded L D L^T solve against numpy.linalg.solve, removed modes"""
    exe = build_sanitized_check(tmp_path, "moduli_line_check")
    rng = np.random.default_rng(23)
    for dim, k, comp, n, lo, hi, l0, l1 in ((3, 1, 2, 1, 0, 0, 0.7, 2.0), (3, 2, 0, 1, 1, 0, 3.0, 0.0), (3, 2, 2, 6, 1, 1, 1.5, 40.0), (3, 1, 1, 7, 0, 1, 0.0, 9.0), (2, 2, 1, 4, 1, 0, 5.0, 0.0),
                                            (2, 1, 0, 5, 0, 0, 0.3, 0.0), (3, 2, 1, 3, 1, 0, np.inf, 1.0), (3, 1, 0, 4, 0, 1, 2.0, np.inf)):
        nl = k * n + 1
        h = 0.5 + rng.random(n); lam = 10.0 ** rng.uniform(-3, 0, n); G = 10.0 ** rng.uniform(-3, 0, n); b = rng.standard_normal(nl)
        args = [str(v) for v in (dim, k, comp, lo, hi)] + [repr(float(l0)), repr(float(l1))] + [repr(float(v)) for v in np.r_[h, lam, G, b]]
        out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.split()
        got = np.array([float(v) for v in out]).reshape(3 * (k + 1) + (k + 1) + 1, nl)
        last = dim - 1
        w = lambda d: lam + 2 * G if d == comp else G                     # noqa: E731
        mats = [fe1d_weighted(k, h, w(d))[0] if d < last else np.zeros((nl, nl)) for d in range(2)] + [fe1d_weighted(k, h, w(last))[1]]
        for f, at in ((lo, 0), (hi, nl - 1)):
            if f:
                for m, A in enumerate(mats):
                    A[at, :] = 0; A[:, at] = 0; A[at, at] = 1.0 if m == 2 else 0.0
        for m, A in enumerate(mats):
            for band in range(k + 1):
                want = np.r_[np.diag(A, band), np.zeros(band)]
                assert np.allclose(got[m * (k + 1) + band], want, rtol=1e-14, atol=0), (dim, k, comp, m, band)
        x = got[-1]
        if not (np.isfinite(l0) and np.isfinite(l1)):
            assert np.all(got[3 * (k + 1):] == 0.0)                        # a removed mode: zero factors, zero solution, nothing non-finite
            continue
        T = l0 * mats[0] + l1 * mats[1] + mats[2]
        rhs = b.copy()
        if lo: rhs[0] = 0.0
        if hi: rhs[-1] = 0.0
        want = np.linalg.solve(T, rhs)
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max() * np.linalg.cond(T) ** 0.5, (dim, k, comp)
        assert np.all(got[3 * (k + 1)] > 0)                                # reciprocal pivots of an SPD matrix


@pytest.mark.parametrize("name", list(FDM_CASES), ids=str)
def test_numpy_model_of_the_layered_block_inverse(name):
    """the algorithm of the device (x / y generalised eigenpairs, one banded solve per mode and component) against spsolve of the block diagonal of the reference matrix:
    1e-11 of max|z| on the shapes of the GPU test"""
    m = material()
    P, bc = fdm_problem(name, m)
    try:
        n_layers = FDM_CASES[name][1][-1]
        ll, lG = layer_decades(m, n_layers)
        R = ModuliReference(P, per_cell(P, ll), per_cell(P, lG))
        B = R.block_diagonal()
        free = np.flatnonzero(~R.mask)
        g = np.sin(0.37 * np.arange(R.n_u) + 0.4)
        want = np.zeros(R.n_u)
        want[free] = spl.spsolve(B[free][:, free].tocsc(), g[free])
        got = layered_block_inverse(P, bc, ll, lG, g)
        e = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name}: model vs spsolve {e:.2e} of max|z|")
        assert np.all(got[R.mask] == 0.0) and e <= 1e-11
    finally:
        P.close()


# ---- host layer ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_moduli_layers_by_cell_centres_and_validation():
    layers = [(-1.0, 1.4e10, 0.3), (0.5, 2e7, 0.45), (2.0, 3e12, 0.0)]
    for P in layered_field_problems():
        try:
            assert P.cell_moduli() is None
            P.set_moduli_layers(layers)
            lam, G = P.cell_moduli()
            idx = np.searchsorted([l[0] for l in layers], centres(P)[:, -1], side="left")
            E, nu = np.array([l[1] for l in layers])[idx], np.array([l[2] for l in layers])[idx]
            assert lam.shape == (P.desc.n_cells,) and len(set(idx)) == 3
            assert np.allclose(lam, E * nu / ((1 + nu) * (1 - 2 * nu)), rtol=1e-15, atol=0) and np.allclose(G, 0.5 * E / (1 + nu), rtol=1e-15, atol=0)
            m = material()                                                   # the first layer is the parameter file's material: the same formula
            assert lam[idx == 0][0] == pytest.approx(m.lame_lambda, rel=1e-15) and G[idx == 0][0] == pytest.approx(m.shear_G, rel=1e-15)
            n = P.desc.n_cells
            with pytest.raises(RuntimeError, match="above every layer"):
                P.set_moduli_layers(layers[:2])
            with pytest.raises(RuntimeError, match="Poisson ratio"):
                P.set_moduli_layers([(9.0, 1e10, 0.5)])
            with pytest.raises(RuntimeError, match="values for"):
                P.set_cell_moduli(np.ones(n + 1), np.ones(n + 1))
            with pytest.raises(RuntimeError, match=f"cell {n - 1} are not finite with G > 0"):
                P.set_cell_moduli(np.ones(n), np.r_[np.ones(n - 1), 0.0])
            with pytest.raises(RuntimeError, match="cell 0 are not"):
                P.set_cell_moduli(np.r_[-1.0, np.ones(n - 1)], np.ones(n))
            with pytest.raises(RuntimeError, match="cell 2 are not"):
                P.set_cell_moduli(np.r_[1.0, 1.0, np.nan, np.ones(n - 3)], np.ones(n))
            assert np.array_equal(P.cell_moduli()[0], lam)
            P.set_cell_moduli(None, None)
            assert P.cell_moduli() is None
        finally:
            P.close()


def test_moduli_inheritance_through_a_refine_and_a_coarsen():
    A, B, nc = refine_and_coarsen_pair()
    try:
        ca, _ = A.cell_parents(); cb, _ = B.cell_parents()
        rng = np.random.default_rng(5)
        lam_c, G_c = 1.0 + rng.random(nc), 2.0 + rng.random(nc)
        A.set_cell_moduli(lam_c[ca], G_c[ca])
        B.inherit_cell_moduli(A)
        assert np.array_equal(B.cell_moduli()[0], lam_c[cb]) and np.array_equal(B.cell_moduli()[1], G_c[cb])      # exactly
        la = lam_c[ca].copy(); kids = np.flatnonzero(ca == 1); la[kids] = np.arange(1.0, 9.0)
        A.set_cell_moduli(la, G_c[ca]); B.inherit_cell_moduli(A)
        lb, gb = B.cell_moduli()
        assert lb[cb == 1] == pytest.approx(4.5, abs=0) and np.array_equal(lb[cb != 1], lam_c[cb][cb != 1]) and np.array_equal(gb, G_c[cb])
        A.set_cell_moduli(None, None); B.inherit_cell_moduli(A)
        assert B.cell_moduli() is None
    finally:
        A.close(); B.close()

"""Host layer of the per-cell permeability tensor diag(kx, ky[, kz]) / mu (no GPU): layers by cell centres, inheritance through the coarse cells of refined boxes, the
exported symbols, the ABI number, the command-line flag of poro_run, and the 1D coefficient builder of the tensor line solve (csrc/perm_line.hpp:
perm_line_coefficients, through a small stand-alone program) against a numpy 1D assembly."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import INPUT_DATA, ROLLERS3, build_sanitized_check, centres, layered_field_problems, material, refine_and_coarsen_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PORO_RUN = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")


def test_layers_by_cell_centres_on_graded_and_refined_boxes():
    layers = [(-1.0, 3.0, 5.0, 0.03), (0.5, 1e-3, 2e-3, 1e-6), (2.0, 7.0, 0.7, 0.07)]
    for P in layered_field_problems():
        try:
            assert P.cell_permeability_tensor() is None
            P.set_permeability_tensor_layers(layers)
            f = P.cell_permeability_tensor()
            z = centres(P)[:, -1]
            want = np.array([l[1:] for l in layers])[np.searchsorted([l[0] for l in layers], z, side="left")]
            assert f.shape == (P.desc.n_cells, 3) and np.array_equal(f, want) and len(set(f[:, 2])) == 3
            with pytest.raises(RuntimeError, match="above every layer"):
                P.set_permeability_tensor_layers(layers[:2])
            with pytest.raises(RuntimeError, match="values for"):
                P.set_cell_permeability_tensor(np.ones((P.desc.n_cells + 1, 3)))
            bad = np.ones((P.desc.n_cells, 3)); bad[4, 1] = -1.0
            with pytest.raises(RuntimeError, match="component 1 of cell 4 is not finite"):
                P.set_cell_permeability_tensor(bad)
            with pytest.raises(ValueError):
                P.set_permeability_tensor_layers([(2.0, 1.0, 1.0)])                # two values in 3D
            assert np.array_equal(P.cell_permeability_tensor(), f)                  # the refused calls left the field alone
            # the problem carries the scalar field or the tensor
            P.set_cell_permeability(np.full(P.desc.n_cells, 2.0))
            assert P.cell_permeability_tensor() is None and P.cell_permeability() is not None
            P.set_cell_permeability_tensor(f)
            assert P.cell_permeability() is None and np.array_equal(P.cell_permeability_tensor(), f)
            P.set_cell_permeability_tensor(None)
            assert P.cell_permeability_tensor() is None
        finally:
            P.close()


def test_inheritance_through_cell_parents():
    A, B, nc = refine_and_coarsen_pair()
    try:
        ca, _ = A.cell_parents(); cb, _ = B.cell_parents()
        per_coarse = 1.0 + np.random.default_rng(3).random((nc, 3)) * [1.0, 10.0, 100.0]
        A.set_cell_permeability_tensor(per_coarse[ca])
        B.inherit_cell_permeability_tensor(A)
        assert np.array_equal(B.cell_permeability_tensor(), per_coarse[cb])          # exactly: children and parents take their coarse cell's components
        # children set apart by the caller: a coarsened parent takes the per-component mean, the others keep exact values
        fa = per_coarse[ca].copy(); kids = np.flatnonzero(ca == 1)
        fa[kids] = np.arange(1.0, 9.0)[:, None] * [1.0, 2.0, 4.0]
        A.set_cell_permeability_tensor(fa); B.inherit_cell_permeability_tensor(A)
        fb = B.cell_permeability_tensor()
        assert np.array_equal(fb[cb == 1], [[4.5, 9.0, 18.0]]) and np.array_equal(fb[cb != 1], per_coarse[cb][cb != 1])
        A.set_cell_permeability_tensor(None); B.inherit_cell_permeability_tensor(A)
        assert B.cell_permeability_tensor() is None
    finally:
        A.close(); B.close()


def test_the_problem_carries_one_permeability_field():
    """the scalar after the tensor, and the tensor after the scalar, leave exactly one readable through the getters; None to one entry point leaves the other's field"""
    A, B, nc = refine_and_coarsen_pair()
    try:
        n = A.desc.n_cells
        scalar = 1.0 + np.arange(n); tensor = 1.0 + np.arange(3.0 * n).reshape(n, 3)
        A.set_cell_permeability_tensor(tensor); A.set_cell_permeability(scalar)
        assert A.cell_permeability_tensor() is None and np.array_equal(A.cell_permeability(), scalar)
        A.set_cell_permeability_tensor(None)                                         # (no tensor to drop: the scalar stays)
        assert A.cell_permeability_tensor() is None and np.array_equal(A.cell_permeability(), scalar)
        A.set_cell_permeability_tensor(tensor)
        assert A.cell_permeability() is None and np.array_equal(A.cell_permeability_tensor(), tensor)
        A.set_cell_permeability(None)                                                # (no scalar to drop: the tensor stays)
        assert A.cell_permeability() is None and np.array_equal(A.cell_permeability_tensor(), tensor)
        # inheritance likewise: each entry point carries the field of its own shape
        B.inherit_cell_permeability(A)
        assert B.cell_permeability() is None and B.cell_permeability_tensor() is None
        B.inherit_cell_permeability_tensor(A)
        assert B.cell_permeability() is None and B.cell_permeability_tensor().shape == (B.desc.n_cells, 3)
    finally:
        A.close(); B.close()


def test_layered_tensor_through_a_refine_and_coarsen_round_trip():
    """a tensor set by layers on the unrefined 2 x 2 x 2 box, carried to the box with three cells refined and back: the layer values, exactly, per component"""
    layers = [(0.0, 3.0, 5.0, 0.03), (2.0, 1e-3, 2e-3, 1e-6)]
    masks = [np.zeros(8, dtype=np.int32), np.array([1, 0, 0, 1, 0, 0, 1, 0], dtype=np.int32), np.zeros(8, dtype=np.int32)]
    A, B, C = [pk.Problem.refined_box_mask(3, [2, 2, 2], [4.0, 4.0, 4.0], 1, material(), ROLLERS3, m) for m in masks]
    try:
        def by_layers(P):
            return np.array([l[1:] for l in layers])[np.searchsorted([l[0] for l in layers], centres(P)[:, -1], side="left")]
        A.set_permeability_tensor_layers(layers)
        B.inherit_cell_permeability_tensor(A); C.inherit_cell_permeability_tensor(B)
        assert (A.desc.n_cells, B.desc.n_cells, C.desc.n_cells) == (8, 8 + 3 * 7, 8)
        for P in (A, B, C):
            f = P.cell_permeability_tensor()
            assert f.shape == (P.desc.n_cells, 3) and np.array_equal(f, by_layers(P))
        assert len(set(B.cell_permeability_tensor()[:, 2])) == 2 and np.array_equal(C.cell_permeability_tensor(), A.cell_permeability_tensor())
    finally:
        A.close(); B.close(); C.close()


def test_symbols_and_abi():
    hip, host = pk.load_hip(), pk.load_host()
    names = ("poro_ctx_set_cell_permeability_tensor", "poro_ctx_get_cell_permeability_tensor")
    for s in names:
        assert s in pk.HIP_SYMBOLS and getattr(hip, s)
    for s in ("poro_host_set_cell_permeability_tensor", "poro_host_set_permeability_tensor_layers", "poro_host_inherit_cell_permeability_tensor", "poro_host_get_cell_permeability_tensor"):
        assert getattr(host, s)
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    assert re.search(r"#define PORO_ABI_VERSION 4\b", header) and hip.poro_abi_version() == 4
    for s in names:
        assert re.search(r"\bint\s+" + s + r"\(", header)


def test_command_line_flag():
    """the flag parses before anything touches a device: a bad string and the clash with --permeability-layers leave with a message and a non-zero status"""
    def run(*args):
        return subprocess.run([PORO_RUN, INPUT_DATA, "--steps", "0", *args], capture_output=True, text=True)
    for bad in ("1=2", "1=2:3:4:5", "1=2:x", "2=1:1:1,1=1:1:1", "1=1:-1:1", "1=1:1,2=1:1:1", "=1:1"):
        r = run("--permeability-tensor-layers", bad)
        assert r.returncode != 0 and "--permeability-tensor-layers needs" in r.stderr, (bad, r.stderr)
    r = run("--permeability-tensor-layers", "5=1e-11:1e-11:1e-13", "--permeability-layers", "5=1e-11")
    assert r.returncode != 0 and "exclude each other" in r.stderr
    r = run("--permeability-tensor-layers")                     # the value is missing
    assert r.returncode != 0 and "unknown option" in r.stderr


def test_line_coefficients_against_numpy(tmp_path):
    """perm_line_coefficients with dim - 1 weight lines through tests/perm_line_check.cpp (host-only, built here with the address and undefined-behaviour sanitizers and run
    directly): [md mo | w0d w0o | (w1d w1o) | kd ko] against the 1D Q1 assembly, free, fixed-lo, fixed-hi and single-cell lines"""
    exe = build_sanitized_check(tmp_path, "perm_line_check")
    rng = np.random.default_rng(17)
    m1 = np.array([[2.0, 1.0], [1.0, 2.0]]); k1 = np.array([[1.0, -1.0], [-1.0, 1.0]])
    for dim in (2, 3):
        for n, lo, hi in ((1, 0, 0), (1, 1, 0), (1, 0, 1), (3, 0, 1), (4, 1, 0), (6, 1, 1), (7, 0, 0)):
            h = 0.5 + rng.random(n); k = 10.0 ** rng.uniform(-3, 1, (dim, n))
            out = subprocess.run([exe, str(dim - 1), str(lo), str(hi)] + [repr(float(v)) for v in np.r_[h, k.ravel()]], check=True, capture_output=True, text=True).stdout.split()
            got = np.array([float(v) for v in out]).reshape(2 * (dim + 1), n + 1)
            nl = n + 1
            mats = [np.zeros((nl, nl)) for _ in range(dim + 1)]       # M, M^k0 (, M^k1), K^k_last
            for e in range(n):
                mats[0][e:e + 2, e:e + 2] += h[e] / 6 * m1
                for d in range(dim - 1):
                    mats[1 + d][e:e + 2, e:e + 2] += k[d, e] * h[e] / 6 * m1
                mats[dim][e:e + 2, e:e + 2] += k[dim - 1, e] / h[e] * k1
            for f, at in ((lo, 0), (hi, n)):
                if f:
                    for i, A in enumerate(mats):
                        A[at, :] = 0; A[:, at] = 0; A[at, at] = 1.0 if i == dim else 0.0
            for i, A in enumerate(mats):
                assert np.allclose(got[2 * i], np.diag(A), rtol=1e-15, atol=0), (dim, n, lo, hi, i)
                assert np.allclose(got[2 * i + 1][:n], np.diag(A, 1), rtol=1e-15, atol=0) and got[2 * i + 1][n] == 0

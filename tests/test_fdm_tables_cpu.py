"""csrc/fdm_tables.hpp on the host: the 1D eigenpairs behind every fast-diagonalisation preconditioner, their even / odd classification and the MFMA fragment packers,
through the stand-alone program tests/fdm_tables_check.cpp (g++ -O2, no HIP, no GPU).

Bounds.  Orthonormality max |S^T M S - I| and residual max |S^T K S - Lambda| / lam_max on the free block: 1e-12 (measured with the same code before it moved into the
header: 2.8e-14 / 2.4e-14; this program: 3.9e-14 / 2.7e-14).  Eigenvalues against scipy.linalg.eigh(K_ff, M_ff) on the 1D matrices of box_reference.matrices_1d, relative
to lam_max: measured worst 3.2e-14 over these cases (the graded 97-point line; 2.8e-14 on the uniform one of the Jacobi branch, <= 2e-15 on the Householder branch), bound
100 x that rounded up to a power of ten = 1e-11.  The closed-form Q1 eigenvalues against the general solver: the same bound (both approximate the same pencil; measured
1.5e-15).  Parity and packers: exact."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from box_reference import matrices_1d

HERE = os.path.dirname(os.path.abspath(__file__))
EIG_TOL = 1e-11
UNIFORM_SAME_ENDS = [(1, 1, 0, 0), (2, 1, 1, 1), (2, 2, 0, 0), (2, 48, 0, 0), (2, 48, 1, 1), (2, 49, 1, 1), (1, 97, 0, 0), (2, 335, 0, 0), (2, 335, 1, 1)]
NOT_SPLIT = [(1, 2, 1, 0, 0.0), (2, 49, 1, 0, 0.0), (2, 48, 1, 1, 0.5), (2, 64, 1, 0, -0.7)]        # different ends, graded lines
PACKS = ([f"nodal_{form}_{nn}" for nn in (11, 145) for form in ("reg", "lds_f64", "lds_f32")] + [f"split_{w}_{nn}" for nn in (11, 145) for w in ("fwd", "bwd")] +
         [f"blocked_{w}_{nn}" for nn in (163, 671) for w in ("fwd", "bwd")] + [f"octant_{w}_nt{nt}" for nt in (1, 5, 8) for w in ("fwd", "bwd")])


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fdm_tables") / "fdm_tables_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "fdm_tables_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    recs = [json.loads(line) for line in out.splitlines()]
    lines = {(r["k"], r["cells"], r["fix_lo"], r["fix_hi"], round(r["grading"], 6)): r for r in recs if r["case"] == "line"}
    packs = {r["name"]: r for r in recs if r["case"] == "pack"}
    assert len(lines) == len(UNIFORM_SAME_ENDS) + len(NOT_SPLIT) and sorted(packs) == sorted(PACKS)
    return lines, packs


def test_eigenvectors_are_orthonormal_and_diagonalise(records):
    for key, r in records[0].items():
        print(key, "orth", r["orth"], "resid", r["resid"])
        assert r["orth"] <= 1e-12 and r["resid"] <= 1e-12, (key, r["orth"], r["resid"])


def test_full_length_storage(records):
    """zero rows at removed nodes, zero columns and lam = inf behind the free modes"""
    for key, r in records[0].items():
        k, cells, lo, hi, _ = key
        assert r["n"] == k * cells + 1 and r["n_free"] == r["n"] - lo - hi and len(r["lam"]) == r["n_free"], key
        assert r["rows_zero"] == 1 and r["cols_zero"] == 1 and r["lam_inf"] == 1, key


def test_uniform_lines_with_equal_ends_classify_completely(records):
    for key in UNIFORM_SAME_ENDS:
        r = records[0][key + (0.0,)]
        nf = r["n_free"]
        assert r["parity"] == 1 and (r["even"], r["odd"]) == ((nf + 1) // 2, nf // 2) == (r["modes_even"], r["modes_odd"]) and r["modes_neither"] == 0, (key, r["even"], r["odd"])
        assert r["mirror"] == 0.0, (key, r["mirror"])              # exact after the symmetrisation
    assert (records[0][(2, 335, 0, 0, 0.0)]["even"], records[0][(2, 335, 0, 0, 0.0)]["odd"]) == (336, 335)
    assert (records[0][(2, 335, 1, 1, 0.0)]["even"], records[0][(2, 335, 1, 1, 0.0)]["odd"]) == (335, 334)


def test_different_ends_and_graded_lines_are_not_split(records):
    for key in NOT_SPLIT:
        r = records[0][key]
        assert r["parity"] == 0 and r["even"] == 0 and r["odd"] == 0, key
        assert r["modes_neither"] == r["n_free"], (key, r["modes_even"], r["modes_odd"], r["modes_neither"])     # every mode is neither


def test_eigenvalues_equal_scipy_on_the_reference_matrices(records):
    for key, r in records[0].items():
        k, f0, f1 = r["k"], r["fix_lo"], r["n"] - r["fix_hi"]
        M, K = (matrices_1d(r["grid"], k, k, what).toarray()[f0:f1, f0:f1] for what in ("mass", "stiff"))
        w = sla.eigh(K, M, eigvals_only=True)
        dev = float(np.abs(np.sort(r["lam"]) - w).max() / w.max())
        print(key, "eigenvalues vs scipy", dev)
        assert dev <= EIG_TOL, (key, dev)


def test_closed_form_q1_eigenvalues_equal_the_general_solver(records):
    r = records[0][(1, 97, 0, 0, 0.0)]
    lam, q1 = np.sort(r["lam"]), np.sort(r["lam_q1"])
    dev = float(np.abs(lam - q1).max() / lam.max())
    print("q1_eig vs general", dev)
    assert len(q1) == 98 and dev <= EIG_TOL, dev


def test_packers_round_trip_exactly(records):
    for name, r in records[1].items():
        assert r["size"] == r["expected_size"] and r["mismatch"] == 0 and r["pad_nonzero"] == 0 and r["uncovered"] == 0, r

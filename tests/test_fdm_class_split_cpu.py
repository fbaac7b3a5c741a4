"""Class-split tables of csrc/fdm_tables.hpp (class_split_tables, class_fragments) on the host, through the stand-alone program tests/fdm_class_split_check.cpp
(g++ -O2, no HIP, no GPU): uniform Q2 lines of 1, 2, 5, 6, 8, 32, 33, 64, 72 and 96 cells with free and with removed ends, and the lines that must be turned down.

Bounds.  The program's own three checks (off-block entries of S^T K S and S^T M S, F^T M F = I and F^T K F = Lambda, spectrum of line_tables) hold to 1e-12 by
construction of `ok`.  Here the eigenvectors it prints are checked against the 1D matrices of box_reference.matrices_1d: orthonormality and residual (relative to the
largest eigenvalue) to 1e-12, the bound of tests/test_fdm_tables_cpu.py; eigenvalues against scipy.linalg.eigh relative to the largest, 1e-11 as there (both sides
approximate the same pencil in fp64).  Class sizes, fragments and fall-backs: exact."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from box_reference import matrices_1d

HERE = os.path.dirname(os.path.abspath(__file__))
CELLS = (1, 2, 5, 6, 8, 32, 33, 64, 72, 96)
SPLIT = [(2, n, f, f, 0.0) for n in CELLS for f in (0, 1)]
NOT_SPLIT = [(2, 48, 1, 1, 0.5), (2, 48, 0, 0, -0.7), (2, 49, 1, 0, 0.0), (2, 6, 0, 1, 0.0), (1, 48, 0, 0, 0.0), (1, 7, 1, 1, 0.0)]


def run_program(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, os.path.join(HERE, "fdm_class_split_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
    recs = [json.loads(line) for line in out.splitlines()]
    return {(r["k"], r["cells"], r["fix_lo"], r["fix_hi"], round(r["grading"], 6)): r for r in recs}


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    recs = run_program(tmp_path_factory.mktemp("fdm_class_split"), ["-O2"], "fdm_class_split_check")
    assert sorted(recs) == sorted(SPLIT + NOT_SPLIT)
    return recs


def test_uniform_lines_with_equal_ends_are_class_split(records):
    for key in SPLIT:
        r = records[key]
        print(key, "off_block", r["off_block"], "orth", r["orth"], "resid", r["resid"], "eig_dev", r["eig_dev"])
        assert r["ok"] == 1, (key, r["why"])
        assert max(r["off_block"], r["orth"], r["resid"], r["eig_dev"]) <= 1e-12, key


def test_eigenvectors_against_the_reference_matrices(records):
    for key in SPLIT:
        r = records[key]
        _, cells, fix, _, _ = key
        n = r["n"]
        M, K = (matrices_1d(r["grid"], 2, 2, what).toarray() for what in ("mass", "stiff"))
        lam = np.array(r["lam"])
        F = np.array(r["F"]).reshape(len(lam), n).T
        assert len(lam) == n - 2 * fix
        if fix:
            assert np.all(F[0] == 0.0) and np.all(F[-1] == 0.0)
        orth = float(np.abs(F.T @ M @ F - np.eye(len(lam))).max())
        resid = float(np.abs(F.T @ K @ F - np.diag(lam)).max() / lam.max())
        w = sla.eigh(K[fix:n - fix, fix:n - fix], M[fix:n - fix, fix:n - fix], eigvals_only=True)
        dev = float(np.abs(np.sort(lam) - w).max() / w.max())
        print(key, "orth", orth, "resid", resid, "eigenvalues vs scipy", dev)
        assert orth <= 1e-12 and resid <= 1e-12 and dev <= 1e-11, (key, orth, resid, dev)


def test_class_sizes_are_the_ones_the_kernels_assume(records):
    """positions: lower-half node 2 p -> vertex position p, 2 p + 1 -> midpoint position p.  Modes: free ends carry the cosines m = 0..N on the vertices and m = 0..N-1 on the
    midpoints, even m = even modes; removed ends the sines m = 1..N-1 and m = 1..N, odd m = even modes.  The frequencies of a group fill the slots of both classes from 0"""
    for key in SPLIT:
        _, N, fix, _, _ = key
        r = records[key]
        h = (2 * N + 1 + 1) // 2
        for p, g in enumerate(r["groups"]):
            fv = [m for m in (range(1, N) if fix else range(0, N + 1)) if (m + fix) % 2 == p]
            fm = [m for m in (range(1, N + 1) if fix else range(0, N)) if (m + fix) % 2 == p]
            assert (g["nv"], g["nm"]) == ((h + 1) // 2, h // 2), key
            assert (g["modes_v"], g["modes_m"]) == (len(fv), len(fm)), (key, p, g)
            assert g["slots"] == max(len(fv), len(fm)) and g["slots"] <= 8 * ((h + 15) // 16), (key, p, g)
    g72 = [(g["modes_v"], g["modes_m"]) for f in (0, 1) for g in records[(2, 72, f, f, 0.0)]["groups"]]
    assert g72 == [(37, 36), (36, 36), (36, 36), (35, 36)]


def test_fragments_round_trip_and_backward_is_the_transpose(records):
    for key in SPLIT:
        r = records[key]
        assert (r["frag_mismatch"], r["frag_pad_nonzero"], r["frag_not_transposed"]) == (0, 0, 0), key


def test_graded_lines_different_ends_and_q1_are_not_class_split(records):
    for key in NOT_SPLIT:
        r = records[key]
        print(key, r["why"], r["off_block"])
        assert r["ok"] == 0 and r["why"], key


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if shutil.which("g++") is None or subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtimes")
    recs = run_program(tmp_path, flags, "fdm_class_split_check_san")
    assert sorted(recs) == sorted(SPLIT + NOT_SPLIT) and all(recs[k]["ok"] == 1 for k in SPLIT)

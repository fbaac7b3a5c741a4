"""The form decision of the displacement system's block FDM on the host (csrc/fdm_tables.hpp: fdm_form_decide, whole_line_fragments) through the stand-alone program
tests/fdm_form_check.cpp (g++ -O2, no HIP, no GPU): which directions are split, the per-pass tile counts, the limit of 128 entries per transformed line, and the
whole-length fragments.  Everything here is exact.  Also: the public names of the per-direction form in the header, the Python module and the driver's usage line."""
import json
import os
import subprocess

import pytest

import poroelasticity_dealii_amd as pk
from common import BC_3D
from fdm_form_cases import BOXES, FORM_CASES, GRADED

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _arg(name, cells, deg, grading, bc):
    return f"{name}:{','.join(str(v) for v in cells)}:{deg}:{','.join(str(v) for v in grading)}:{','.join(f'{lab}.{comp}' for lab, comp, _ in bc)}"


def _box_args():
    args = []
    for cells, deg in BOXES:
        for name, (_, bc) in FORM_CASES.items():
            args.append(_arg(f"{name}_q{deg}", cells, deg, (0, 0, 0), bc))
        args.append(_arg(f"symmetric_q{deg}", cells, deg, (0, 0, 0), BC_3D))
    args.append(_arg("graded", GRADED[0], GRADED[1], GRADED[2], BC_3D))
    args.append(_arg("graded_in_y_equal_ends", (4, 3, 5), 2, (0.0, 0.5, 0.0), BC_3D))
    return args


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fdm_form") / "fdm_form_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "fdm_form_check.cpp")], check=True)
    out = subprocess.run([exe] + _box_args(), check=True, capture_output=True, text=True, timeout=120).stdout
    recs = [json.loads(line) for line in out.splitlines()]
    return {kind: {r["name"]: r for r in recs if r["case"] == kind} for kind in ("box", "tiles", "pack")}


def test_every_boundary_list_gets_its_mask(records):
    for cells, deg in BOXES:
        nn = [deg * m + 1 for m in cells]
        for name, (mask, _) in FORM_CASES.items():
            r = records["box"][f"{name}_q{deg}"]
            assert tuple(r["split"]) == mask and r["usable"] == 1 and r["all_split"] == 0, (name, deg, r)
            assert r["len"] == [(n + 1) // 2 if s else n for n, s in zip(nn, mask)] and r["parts"] == 2 ** sum(mask), (name, deg, r)
        r = records["box"][f"symmetric_q{deg}"]
        assert r["split"] == [1, 1, 1] and r["all_split"] == 1 and r["parts"] == 8, r        # today's octant form


def test_a_uniform_direction_with_equal_ends_is_split_a_graded_one_is_whole(records):
    r = records["box"]["graded"]
    assert tuple(r["split"]) == GRADED[3] and r["usable"] == 1, r
    assert records["box"]["graded_in_y_equal_ends"]["split"] == [1, 0, 1]


@pytest.mark.parametrize("length,tiles", [(16, 1), (17, 2), (80, 5), (81, 6), (128, 8)])
def test_tile_counts_per_pass(records, length, tiles):
    """passes 1 / 3 are sized by max(len_x, len_y), pass 2 by len_z; the other two directions have 3 entries (one tile)"""
    for kind in ("whole", "split"):
        for d in "xyz":
            r = records["tiles"][f"{kind}_{d}_{length}"]
            assert r["usable"] == 1 and r["len"]["xyz".index(d)] == length, r
            assert (r["nt_xy"], r["nt_z"]) == ((1, tiles) if d == "z" else (tiles, 1)), r
            assert r["split"]["xyz".index(d)] == (kind == "split"), r


def test_a_line_of_129_entries_is_not_usable(records):
    for kind in ("whole", "split"):
        for d in "xyz":
            assert records["tiles"][f"{kind}_{d}_129"]["usable"] == 0


def test_whole_length_fragments_unpack_to_the_eigenvector_matrix_and_its_transpose(records):
    assert sorted(records["pack"]) == ["q1_16_graded", "q2_17_lo", "q2_33_hi", "q2_73_lo"]
    for name, r in records["pack"].items():
        assert r["sizes_ok"] == 1 and r["mismatch"] == 0 and r["pad_nonzero"] == 0 and r["parity"] == 0, r


def test_public_names():
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    for name in ("PORO_FDM_FORM_DEFAULT", "PORO_FDM_FORM_PER_DIRECTION", "poro_ctx_set_fdm_form", "poro_ctx_get_fdm_form", "PORO_FDM_RUNS_NODAL", "PORO_FDM_RUNS_OCTANT",
                 "PORO_FDM_RUNS_PER_DIRECTION", "PORO_FDM_RUNS_SLAB", "PORO_FDM_RUNS_PLANAR", "PORO_FDMO_FORM", "fdm_u_per_direction_form"):
        assert name in header, name
    assert "#define PORO_ABI_VERSION 4 " in header
    assert (pk.FDM_FORM_DEFAULT, pk.FDM_FORM_PER_DIRECTION) == (0, 1)
    assert (pk.FDM_RUNS_NODAL, pk.FDM_RUNS_OCTANT, pk.FDM_RUNS_PER_DIRECTION, pk.FDM_RUNS_SLAB, pk.FDM_RUNS_PLANAR) == (0, 1, 2, 3, 4)
    assert callable(pk.Context.set_fdm_form) and callable(pk.Context.get_fdm_form)
    assert "poro_ctx_set_fdm_form" in pk.HIP_SYMBOLS and "poro_ctx_get_fdm_form" in pk.HIP_SYMBOLS
    hip = pk.load_hip()
    assert hip.poro_ctx_set_fdm_form and hip.poro_ctx_get_fdm_form
    import inspect
    assert "fdm_per_direction" in inspect.signature(pk.run_problem).parameters and "fdm_per_direction" in inspect.signature(pk.Runner.__init__).parameters


def test_poro_run_usage_names_the_option():
    exe = os.path.join(pk.LIB_DIR, "poro_run")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "specify the file name" in r.stderr and "--fdm-per-direction" in r.stderr and "--block-fdm" in r.stderr
    r = subprocess.run([exe, os.path.join(HERE, "golden", "input.data"), "--fdm-per-direction"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--fdm-per-direction needs --block-fdm or --fastest" in r.stderr

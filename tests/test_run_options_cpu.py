"""The run options across the C boundary (host/run_controls.hpp), without a GPU.  tests/run_options_check.cpp - a stand-alone program built with the address and
undefined-behaviour sanitizers and run directly; its exit code names the check that failed - holds poro_host_run_options -> RunControls member by member and prints the
layout of the C struct; the layout is held here against the ctypes mirror pk.RunOptions (size and every offset), which is the safety positional argument types gave."""
import ctypes as C
import subprocess

import pytest

import poroelasticity_dealii_amd as pk
from common import build_sanitized_check


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    run = subprocess.run([build_sanitized_check(tmp_path_factory.mktemp("run_options"), "run_options_check")], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    return run.stdout.splitlines()


def test_options_map_onto_run_controls_member_by_member(check_output):
    assert check_output[-1] == "run_options_check ok"


def test_the_ctypes_mirror_has_the_layout_of_the_c_struct(check_output):
    size = [int(l.split()[1]) for l in check_output if l.startswith("sizeof ")]
    offsets = [(l.split()[1], int(l.split()[2])) for l in check_output if l.startswith("offsetof ")]
    assert size == [C.sizeof(pk.RunOptions)]
    assert offsets == [(name, getattr(pk.RunOptions, name).offset) for name, _ in pk.RunOptions._fields_]      # the same members in the same order at the same places


def test_the_keyword_arguments_arrive_as_given():
    kw = dict(p_init=2e6, dt=30.0, n_steps=3, fss_tol=1e-6, pressure_tol=1e-7, max_fss=7, max_pres=9, abs_u=1e-11, rel_u=1e-9, max_it=123, prec=pk.PREC_CHEBYSHEV, coupled_fss=True,
              incremental_strain=False, reduction=True, cheb_degree=300, cheb_ratio=12.5, jacobi_p=False, two_level_p=False, atomic_scatter=True, fdm_fp32=False, hybrid_operator=True,
              fdm_per_direction=True, moduli_structured=True, refine_every=None)
    o = pk._run_options(kw)
    assert (o.chebyshev_degree, o.chebyshev_ratio) == (300, 12.5)                  # no clipping to 8 bits, no rounding to an integer of 15 bits
    assert (o.p_init, o.time_step, o.n_steps, o.fss_tol, o.pressure_tol, o.max_fss_iterations, o.max_pressure_iterations) == (2e6, 30.0, 3, 1e-6, 1e-7, 7, 9)
    assert (o.abs_tol_u, o.rel_tol_u, o.max_iter, o.preconditioner, o.stop_rule_u, o.preconditioner_p) == (1e-11, 1e-9, 123, pk.PREC_CHEBYSHEV, pk.STOP_REDUCTION, -1)
    assert (o.coupled_fss, o.incremental_strain, o.atomic_scatter, o.fdm_fp32, o.hybrid_operator, o.fdm_per_direction, o.moduli_structured) == (1, 0, 1, 0, 1, 1, 1)
    assert (o.refine_every, o.refine_fraction, o.coarsen_fraction) == (0, 0.6, 0.4)
    assert pk._run_options(dict(kw, jacobi_p=True)).preconditioner_p == pk.PREC_JACOBI
    assert pk._run_options(dict(kw, jacobi_p=True, two_level_p=True)).preconditioner_p == pk.PREC_TWO_LEVEL      # the two-level request wins, as it did
    assert pk._run_options(dict(kw, reduction=False)).stop_rule_u == pk.STOP_RHS

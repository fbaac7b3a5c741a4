"""csrc/newton_record.hpp without a GPU: the batches the pressure Newton loop plans and the per-call numbers the host rebuilds from their records, through the
stand-alone program tests/newton_record_check.cpp built with the address and undefined-behaviour sanitizers; and the new entry points' symbols."""
import os
import re
import subprocess

import poroelasticity_dealii_amd as pk
from common import build_sanitized_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_replay_under_the_sanitizers(tmp_path):
    """every (first converged iteration, failing solve, cap, prediction) of a small range: iterations, solves, outcome, residual list and checks equal the per-call loop;
    a right prediction costs one wait; records that contradict their batch are refused"""
    exe = build_sanitized_check(tmp_path, "newton_record_check")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("newton_record_check ok"), r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) cases, at most (\d+) batches per loop", r.stdout)
    assert m and int(m.group(1)) == 9 * 7 * 10 * 10 and int(m.group(2)) <= 5


def test_symbols():
    hip = pk.load_hip()
    header = open(os.path.join(ROOT, "include", "poroel_hip.h")).read()
    for s in ("poro_supports_pres_newton_loop", "poro_pres_newton_loop"):
        assert s in pk.HIP_SYMBOLS and getattr(hip, s) and re.search(r"\bint\s+" + s + r"\(", header)
    assert callable(pk.Context.pres_newton_loop) and callable(pk.Context.supports_pres_newton_loop)

"""poro_run --hybrid-operator: the hybrid operator form through the driver executable, on the adaptive path (a refined box), on the parameter file's own box
(box-tagged: accepted, no effect) and on a mesh that cannot take it (an error with a message)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
GOLDEN = os.path.join(ROOT, "tests", "golden")
INPUT = os.path.join(GOLDEN, "input.data")


def run(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def trace(out):
    return (re.findall(r"Coupling iteration: (\d+)", out), re.findall(r"pressure converged; iterations: (\d+)", out),
            [float(m) for m in re.findall(r"Solution limits: ([0-9.eE+-]+)", out)])


@pytest.mark.parametrize("adaptive", [("--refine-every", "1"), ()], ids=["refine-every-1", "box"])
def test_hybrid_operator_flag_gives_the_same_trace(adaptive):
    """--matrix-free --refine-every 1 builds the box as a refined box with an empty mask and adapts it before every step: the general kernels and, with the flag, the
    hybrid form on every mesh of the run.  Without --refine-every the context is box-tagged and the flag changes nothing.  The log prints |p|_inf with 6 digits"""
    args = (INPUT, "--matrix-free", "--steps", "3", *adaptive)
    a, b = trace(run(*args)), trace(run(*args, "--hybrid-operator"))
    assert a[0] == b[0] and a[1] == b[1] and len(a[1]) >= 3
    assert len(a[2]) == len(b[2]) and all(abs(x - y) <= 1e-9 * abs(y) for x, y in zip(b[2], a[2]))


def test_hybrid_operator_flag_on_a_mesh_that_cannot_take_it():
    """the Gmsh mesh carries an auxiliary box that is no coarsening of it; the assembled operator has no matrix-free form at all"""
    for extra, message in ((("--matrix-free", "--mesh", os.path.join(GOLDEN, "domain.msh")), "no injected image"), (("--refine-every", "1"), "PORO_OP_MATRIX_FREE")):
        r = subprocess.run([EXE, INPUT, "--steps", "1", "--hybrid-operator", *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and message in r.stderr, (extra, r.returncode, r.stderr[-2000:])

"""poro_run --atomic-scatter: the general matrix-free operator in its single-launch atomic mode gives the printed trace of the coloured mode."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def trace(out):
    return (re.findall(r"Coupling iteration: (\d+)", out), re.findall(r"pressure converged; iterations: (\d+)", out),
            [float(m) for m in re.findall(r"Solution limits: ([0-9.eE+-]+)", out)])


@pytest.mark.parametrize("mesh", [(), ("--mesh", os.path.join(GOLDEN, "domain.msh"))], ids=["box", "gmsh"])
def test_atomic_scatter_flag_gives_the_same_trace(mesh):
    """input.data --matrix-free with and without the flag.  On the parameter file's own box the context is box-tagged, so this case shows only that the flag is
    accepted and changes nothing; on the Gmsh mesh the general kernels run and the mode is in force.  --steps 2 keeps both runs short.  The log prints |p|_inf with
    6 digits, so the 1e-9 relative bound on it amounts to the two logs printing the same digits."""
    args = (os.path.join(GOLDEN, "input.data"), "--matrix-free", "--steps", "2", *mesh)
    a, b = trace(run(*args)), trace(run(*args, "--atomic-scatter"))
    assert a[0] == b[0] and a[1] == b[1] and len(a[1]) == 2
    assert len(a[2]) == len(b[2]) == 2 and all(abs(x - y) <= 1e-9 * abs(y) for x, y in zip(b[2], a[2]))


def test_unknown_flag_is_still_refused():
    r = subprocess.run([EXE, os.path.join(GOLDEN, "input.data"), "--atomic"], capture_output=True, text=True)
    assert r.returncode == 1 and "unknown option" in r.stderr

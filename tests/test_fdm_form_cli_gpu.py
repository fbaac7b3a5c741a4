"""poro_run --block-fdm --fdm-per-direction: the per-direction form of the block FDM through the driver executable, on a 3D 4^3 Q2 consolidation column (input.data
with three dimensions, refinement level 2 and the column's Dirichlet list: rollers on the x and y faces, held at the bottom): the run prints the form and the split
mask, and its steps equal the run with the nodal kernels (the same fixed-stress iterations, |p|_inf per step to 1e-9: the log prints 6 digits - the same digits).
The flag needs --block-fdm or --fastest."""
import os
import re
import subprocess

import pytest

from common import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")


def cli_trace(out):
    return (re.findall(r"Time: ([0-9.eE+-]+)", out), re.findall(r"Coupling iteration: (\d+)", out), [float(m) for m in re.findall(r"Solution limits: ([0-9.eE+-]+)", out)])


def test_poro_run_fdm_per_direction_flag(tmp_path):
    text = open(os.path.join(GOLDEN, "input.data"), encoding="latin1").read()
    text = text.replace("set Dimensions               = 2", "set Dimensions               = 3").replace("set Domain size              = 10, 10", "set Domain size              = 10, 10, 10")
    text = text.replace("set Initial refinement level = 4", "set Initial refinement level = 2")
    text = text.replace("= 0, 1, 2, 3\n", "= 0, 1, 2, 3, 4\n").replace("= 0, 0, 1, 1\n", "= 0, 0, 1, 1, 2\n").replace("= 0, -1e-5, 0, -1e-5\n", "= 0, -1e-5, 0, -1e-5, 0\n")
    assert "= 3\n" in text and "0, 1, 2, 3, 4\n" in text and "0, 0, 1, 1, 2\n" in text and "0, -1e-5, 0, -1e-5, 0\n" in text and "level = 2" in text
    inp = tmp_path / "column3d.data"; inp.write_text(text, encoding="latin1")

    def run(*args):
        r = subprocess.run([EXE, str(inp), "--matrix-free", "--steps", "2", *args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    a, b = run("--block-fdm"), run("--block-fdm", "--fdm-per-direction")
    assert "block FDM form" not in a                                          # the log changes only with the option
    assert "block FDM form: per-direction form, split directions (x y z): 1 1 0" in b
    ta, tb = cli_trace(a), cli_trace(b)
    assert len(ta[0]) == 2 and ta[0] == tb[0] and ta[1] == tb[1]
    assert len(ta[2]) == len(tb[2]) >= 2 and all(abs(x - y) <= 1e-9 * abs(y) for x, y in zip(tb[2], ta[2])), (ta[2], tb[2])
    r = subprocess.run([EXE, str(inp), "--matrix-free", "--fdm-per-direction"], capture_output=True, text=True)
    assert r.returncode == 1 and "--fdm-per-direction needs --block-fdm or --fastest" in r.stderr

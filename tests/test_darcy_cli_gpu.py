"""poro_run --flow-balance and --output DIR --darcy-output through the driver executable, on the 4 x 4 Q2 box of input.data (refinement level 2) with a drained face:
the per-step line and the totals, the darcy_velocity block of the VTK files against Runner.darcy_velocity() of the same run made from Python, and - the flags change
nothing else - the log and the files of the run with the flags, stripped of the new lines and the new block, byte for byte those of the run without."""
import os
import re
import subprocess

import numpy as np
import pytest

import poroelasticity_dealii_amd as pk
from common import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
STEPS = 2
NUM = r"([0-9.eE+-]+)"


def strip_block(text):
    """a VTK file without its CELL_DATA block (the last one of the file)"""
    at = text.find("CELL_DATA ")
    return text if at < 0 else text[:at]


def test_poro_run_flow_balance_and_darcy_output(tmp_path):
    text = open(os.path.join(GOLDEN, "input.data"), encoding="latin1").read().replace("set Initial refinement level = 4", "set Initial refinement level = 2")
    assert "level = 2" in text
    inp = tmp_path / "box.data"; inp.write_text(text, encoding="latin1")
    plain_dir, flow_dir = tmp_path / "plain", tmp_path / "flow"
    plain_dir.mkdir(); flow_dir.mkdir()

    def run(*args):
        r = subprocess.run([EXE, str(inp), "--matrix-free", "--steps", str(STEPS), "--pressure-bc", "3=0", *args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    plain = run("--output", str(plain_dir))
    flow = run("--output", str(flow_dir), "--flow-balance", "--darcy-output")

    # the per-step line and the totals
    lines = [l for l in flow.split("\n") if l.startswith("flow balance")]
    assert len(lines) == STEPS + 1 and "flow balance" not in plain
    step = re.compile(r"flow balance step (\d+): storage_strain " + NUM + " storage_pressure " + NUM + " source " + NUM + " outflow " + NUM + " free_rows " + NUM + " residual_l2 " + NUM +
                      "; label 3 outflow " + NUM + " discharge " + NUM + "; imbalance " + NUM + " bound " + NUM + "$")
    drained = 0.0
    for k, line in enumerate(lines[:STEPS]):
        m = step.match(line)
        assert m and int(m.group(1)) == k + 1, line
        s_strain, s_pres, src, out, free, l2, out3, dis3, imb, bound = (float(v) for v in m.groups()[1:])
        assert out3 == out and abs(imb - (s_strain + s_pres + src + out)) <= 1e-8 * (abs(s_strain) + abs(s_pres) + abs(src) + abs(out)) + 1e-3 * abs(imb)      # (what the line prints, to its digits)
        drained += out
    m = re.match(r"flow balance totals over (\d+) steps: storage_strain " + NUM + " storage_pressure " + NUM + " injected " + NUM + " drained " + NUM + "; label 3 drained " + NUM +
                 " face-integrated " + NUM + "; imbalance " + NUM + " bound " + NUM + "$", lines[-1])
    assert m and int(m.group(1)) == STEPS, lines[-1]
    dt = pk.read_input(str(inp)).time_step
    assert abs(float(m.group(5)) - dt * drained) <= 1e-8 * dt * abs(drained) and float(m.group(6)) == float(m.group(5))

    # without the flags: the same log and the same files
    assert "\n".join(l for l in flow.split("\n") if not l.startswith("flow balance")) == plain
    files = sorted(os.listdir(plain_dir))
    assert files == sorted(os.listdir(flow_dir)) == [f"solution-{k + 1:04d}.vtk" for k in range(STEPS)]
    for f in files:
        a, b = (plain_dir / f).read_bytes().decode(), (flow_dir / f).read_bytes().decode()
        assert "CELL_DATA" not in a and "darcy_velocity" not in a
        assert b.count("CELL_DATA ") == 1 and strip_block(b) == a

    # the block: n_cells rows that match Runner.darcy_velocity() of the same run
    I = pk.read_input(str(inp))
    dim, n = I.dim, [1 << I.initial_refinement_level] * I.dim
    bc = [(I.dirichlet_labels[i], I.dirichlet_components[i], I.dirichlet_values[i]) for i in range(I.n_dirichlet)]
    neu = [(I.neumann_labels[i], I.neumann_components[i], I.neumann_values[i]) for i in range(I.n_neumann)]
    P = pk.Problem.box(dim, n, list(I.domain_size)[:dim], 2, I.material, bc, neu)
    P.set_pressure_bc([(3, 0.0)])
    R = pk.Runner(P, 0, pk.OP_MATRIX_FREE, p_init=I.p_init, dt=I.time_step, fss_tol=I.fss_tol, pressure_tol=I.pressure_tol, max_fss=I.max_fss_iterations, max_pres=I.max_pressure_iterations)
    try:
        R.initialize()
        own_dir = tmp_path / "own"; own_dir.mkdir()
        for k in range(STEPS):
            R.step()
            R.postprocess(str(own_dir), darcy=True)
            q = R.darcy_velocity()
            block = (flow_dir / files[k]).read_text()
            block = block[block.index("CELL_DATA "):].split("\n")
            assert block[0] == f"CELL_DATA {P.desc.n_cells}" and block[1] == "VECTORS darcy_velocity double"
            rows = np.array([[float(v) for v in l.split()] for l in block[2:] if l.strip()])
            assert rows.shape == (P.desc.n_cells, 3) and np.all(rows[:, 2] == 0.0)
            assert np.abs(rows[:, :dim] - q).max() <= 1e-11 * np.abs(q).max() and np.abs(q).max() > 0       # the file prints 12 digits
            # Runner.postprocess(darcy=True) writes the same file, darcy=False the file without the block
            assert (own_dir / files[k]).read_text() == (flow_dir / files[k]).read_text()
        R.postprocess(str(own_dir))
        assert (own_dir / files[-1]).read_text() == (plain_dir / files[-1]).read_text()
    finally:
        R.close(); P.close()

"""The smallest shapes that reach every uploader of the 1D tables (csrc/fdm_tables.hpp) and every form decision of the displacement set-up (ctx_prec.hip: build_fdm_u):
z = apply_preconditioner_u(PREC_FDM, g) against the exact block inverse of the Kronecker reference at the suite's bound of 1e-10 (1e-5 under PORO_FDMU_SINGLE: fp32
transforms, see test_box_reference_gpu.py), exact zeros on the Dirichlet dofs.  The variants behind environment switches run in child processes (the switches are read
once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":          # a child process of test_nodal_variants: the repository root and the oracle on the path, as tests/conftest.py puts them
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]

import poroelasticity_dealii_amd as pk
from box_reference import BoxReference
from common import BC_2D, BC_3D, box_problem, material

pytestmark = pytest.mark.gpu

# name: (cells, degree, Dirichlet list (face label, component, value), grading)
CASES = {
    "octant Q2, lines of 7 / 9 / 11 points": ((3, 4, 5), 2, BC_3D, None),
    "octant Q1, lines of 4 / 5 / 6 points": ((3, 4, 5), 1, BC_3D, None),
    "nodal, full form in x, split form in y and z": ((3, 4, 5), 2, [(0, 0, 0.0)] + BC_3D[2:], None),
    "nodal, full form everywhere (low faces only)": ((3, 4, 5), 2, [(0, 0, 0.0), (2, 1, 0.0), (4, 2, 0.0)], None),
    "planar with the parity split": ((5, 7), 2, BC_2D, None),
    "planar without the split": ((5, 7), 2, [(2, 1, 0.0), (1, 0, -1e-5)], None),
    "graded, equal ends, not split: nodal full form": ((4, 3, 5), 2, BC_3D, (1.0, 0.5, -0.7)),
}
NO_OCT = {"PORO_FDMU_NO_OCT": "1"}
NODAL_VARIANTS = [NO_OCT, dict(NO_OCT, PORO_FDMU_LDS_FORM="1"), dict(NO_OCT, PORO_FDMU_NO_SPLIT="1"), dict(NO_OCT, PORO_FDMU_SINGLE="1")]
CHILD_CASES = {"split": ((3, 4, 5), 2, BC_3D, None), "blocked": ((81, 2), 2, BC_2D, None)}       # blocked: a 163-point line, above the 160 points of the split form


def check(n, deg, bc, grading, tol=1e-10):
    dim = len(n)
    P = box_problem(dim, n, deg, bc=bc) if grading is None else pk.Problem.graded_box(dim, list(n), [10.0] * dim, deg, material(), bc, list(grading))
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        R = BoxReference(P)
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        g = np.random.default_rng(7).standard_normal(G.n_u) * 1e3; g[R.mask] = 0.0
        z = G.apply_preconditioner_u(pk.PREC_FDM, g)
        z0 = R.block_inverse_u(g)
        assert np.abs(z[R.mask]).max() == 0.0
        err = float(np.abs(z - z0).max() / np.abs(z0).max())
        print(n, deg, f"{err:.3e}")
        assert err <= tol, (n, deg, err)
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_block_fdm_form(name):
    check(*CASES[name])


def run_child(env_over, case):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=dict(os.environ, **env_over), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (env_over, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    print(env_over, r.stdout.strip())


@pytest.mark.parametrize("env", NODAL_VARIANTS, ids=lambda v: ",".join(v))
def test_nodal_variants(env):
    """3 x 4 x 5 Q2 without the octant form: the nodal split form, the LDS form, the unsplit lines, the fp32 transforms"""
    run_child(env, "split")


def test_blocked_split_form_above_160_points():
    run_child(NO_OCT, "blocked")


if __name__ == "__main__":
    check(*CHILD_CASES[sys.argv[1]], tol=1e-5 if os.environ.get("PORO_FDMU_SINGLE") else 1e-10)
    print("child ok")

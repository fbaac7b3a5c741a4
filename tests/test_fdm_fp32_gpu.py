"""The opt-in fp32 transforms of the displacement system's block fast diagonalisation in its single-rank 3D octant form (Context.set_fdm_precision(FDM_FP32),
run_problem / Runner(fdm_fp32=True), poro_run --fdm-fp32, PORO_FDMO_PRECISION): the plumbing and the forms the mode must leave alone bit for bit; the fp32
preconditioner against the exact block inverse at every tile count and padding boundary; the fp64 PCG around it against the reference PCG with the exact fp64
preconditioner; whole time steps against the golden trace, the oracle and the driver executable's own fp64 run."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":          # a child process (the environment switches are read once per context / solve): the paths tests/conftest.py sets up
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]

import poroelasticity_dealii_amd as pk
from box_reference import BoxReference, reference_pcg
from common import BC_2D, BC_3D, REF, box_problem, material

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "poroelasticity_dealii_amd", "lib", "poro_run")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BENCH_TOL = dict(abs_tol=1e-12, rel_tol=1e-8, reduction=True)      # = tests/test_box_reference_gpu.py (bench.py defaults)
FP64, FP32 = pk.FDM_FP64, pk.FDM_FP32


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def assembled(P):
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
    return G


def random_rhs(G, R, seed=7):
    g = np.random.default_rng(seed).standard_normal(G.n_u) * 1e3
    g[R.mask] = 0.0
    return g


# ---- 1. plumbing ------------------------------------------------------------------------------------------------------------------------------------
def test_default_switch_and_unknown_value():
    P = box_problem(3, (8, 8, 8), 2)
    G, F = pk.Context(P, 0, pk.OP_MATRIX_FREE), None
    try:
        assert G.get_fdm_precision() == (FP64, FP64)
        G.fill(pk.VEC_P, 0.0); G.disp_assemble_system(True)
        R = BoxReference(P)
        g = random_rhs(G, R)
        G.set_fdm_precision(FP32)
        assert G.get_fdm_precision() == (FP32, FP32)
        with pytest.raises(RuntimeError):
            G.set_fdm_precision(7)
        assert G.get_fdm_precision() == (FP32, FP32)                    # a refused value changes nothing
        z32 = G.apply_preconditioner_u(pk.PREC_FDM, g)
        # switching back restores the fp64 path bit for bit: the z of a context that never left it
        F = assembled(P)
        z_fresh = F.apply_preconditioner_u(pk.PREC_FDM, g)
        assert not np.array_equal(z32, z_fresh)
        G.set_fdm_precision(FP64)
        assert G.get_fdm_precision() == (FP64, FP64)
        assert np.array_equal(G.apply_preconditioner_u(pk.PREC_FDM, g), z_fresh)
    finally:
        G.close()
        if F is not None:
            F.close()
        P.close()


ONE_SIDED = BC_2D + [(4, 2, 0.0)]           # u_z fixed on the lower z face only: the z lines are not mirror-symmetric, the octant form is off


@pytest.mark.parametrize("what", ["2d", "half line 129", "one-sided Dirichlet face"])
def test_forms_without_fp32_kernels_ignore_the_mode_bit_for_bit(what):
    P = {"2d": lambda: box_problem(2, (8, 8), 2), "half line 129": lambda: box_problem(3, (128, 3, 2), 2),
         "one-sided Dirichlet face": lambda: box_problem(3, (6, 6, 6), 2, bc=ONE_SIDED)}[what]()
    G = assembled(P)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        g = np.random.default_rng(7).standard_normal(G.n_u) * 1e3
        z0 = G.apply_preconditioner_u(pk.PREC_FDM, g)
        G.set_fdm_precision(FP32)
        assert G.get_fdm_precision() == (FP32, FP64)
        assert np.array_equal(G.apply_preconditioner_u(pk.PREC_FDM, g), z0)
    finally:
        G.close(); P.close()


def run_child(env_over, checks, timeout=900):
    env = dict(os.environ, **env_over)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), checks], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "child ok" in r.stdout, (env_over, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    print(env_over, f"{time.time() - t0:.1f} s:", r.stdout.strip())
    return r.stdout


def test_environment_variable_sets_the_initial_mode():
    run_child({"PORO_FDMO_PRECISION": "fp32"}, "env")


# ---- 2. the fp32 preconditioner against the exact block inverse --------------------------------------------------------------------------------------
# half lines h = n + 1 (Q2): tiles per half line NT = ceil(h / 16), the maximum over the directions selects the instantiation
FP32_CASES = [((15, 16, 17), 2),       # NT 1 / 2 / 2, odd and even x half lines
              ((31, 32, 33), 2),       # NT 2 / 3 / 3
              ((47, 63, 6), 2),        # NT 3 / 4
              ((72, 72, 4), 2),        # NT 5 in passes 1 and 3: shared tile row, corner tile
              ((8, 8, 72), 2),         # NT 5 in pass 2 with a short last chunk
              ((79, 80, 3), 2),        # NT 5 / 6
              ((111, 112, 6), 2),      # NT 7 / 8
              ((127, 3, 2), 2),        # h = 128, the largest
              ((16, 31, 5), 2),
              ((30, 33, 5), 1)]


def block_fdm_errors(P, effective=FP32):
    """check_block_fdm's procedure (tests/test_box_reference_gpu.py) with FDM_FP32 requested: g = 1e3 N(0, 1), zero on the mask, two applications; the two relative errors"""
    G = assembled(P)
    try:
        assert G.supports_preconditioner(0, pk.PREC_FDM)
        G.set_fdm_precision(FP32)
        assert G.get_fdm_precision() == (FP32, effective)
        R = BoxReference(P)
        rng = np.random.default_rng(7)
        errs = []
        for _ in range(2):
            g = rng.standard_normal(G.n_u) * 1e3; g[R.mask] = 0.0
            z = G.apply_preconditioner_u(pk.PREC_FDM, g)
            assert np.abs(z[R.mask]).max() == 0.0                       # removed modes and padding give exact zeros in fp32 too
            errs.append(rel(z, R.block_inverse_u(g)))
        return errs
    finally:
        G.close()


@pytest.mark.parametrize("n,deg", FP32_CASES, ids=str)
def test_fp32_block_fdm_against_the_exact_block_inverse(n, deg):
    """Bound asserted: 1e-5 relative to max|z| - the project's bound for its fp32 nodal transforms (test_single_precision_block_fdm_bound); the sums here are the
    same length or shorter (half lines of <= 128 entries).  The lower bound 1e-9 keeps the fp64 kernel from passing under the fp32 label.
    Measured on the MI355X (worst of the two applications), in the order of FP32_CASES: 2.2e-7, 3.1e-7, 3.6e-7, 5.0e-7, 2.2e-7, 4.4e-7, 5.8e-7, 4.4e-7, 2.1e-7, 2.2e-7."""
    P = box_problem(3, n, deg)
    try:
        worst = max(block_fdm_errors(P))
        print(f"fp32 block fdm {n} Q{deg}: {worst:.3e}")
        assert worst <= 1e-5, (n, deg, worst)
        assert worst >= 1e-9, (n, deg, worst)
    finally:
        P.close()


GRADED_MEASURED = 8.6e-14    # MI355X, worst of the two applications


def test_fp32_mode_on_a_graded_box():
    """Tensor-product grid with the exponential gradings (1.0, 0.5, -0.7): no grid line is mirror-symmetric, so the octant form - and with it the fp32 mode - does
    not run there (effective = FDM_FP64, the nodal fp64 kernels apply the preconditioner whatever was requested).  The project holds no bound for this grid: asserted
    is 10 x the measured worst of the two applications with FDM_FP32 requested, 8.6e-14 (the error moves by a small factor with the random right-hand side)."""
    P = pk.Problem.graded_box(3, [20, 17, 12], [10.0] * 3, 2, material(), BC_3D, [1.0, 0.5, -0.7])
    try:
        worst = max(block_fdm_errors(P, effective=FP64))
        print(f"fp32 requested, graded (20, 17, 12) Q2: {worst:.3e}")
        assert worst <= 10 * GRADED_MEASURED, worst
    finally:
        P.close()


# ---- 3. the fp64 PCG around the fp32 preconditioner ---------------------------------------------------------------------------------------------------
PCG_SHAPES = [(24, 24, 24), (72, 72, 4), (8, 8, 72)]


def assert_same_count(its, its_ref, hist, tol, what):
    """= tests/test_box_reference_gpu.py: identical counts; +-1 only where the reference's residual at the deciding iteration lies within 1e-6 (relative) of the tolerance"""
    if its == its_ref:
        return
    k = min(its, its_ref)
    near = abs(its - its_ref) == 1 and k < len(hist) and abs(hist[k] - tol) <= 1e-6 * tol
    assert near, f"{what}: device {its} iterations, reference {its_ref} (reference residual at iteration {k}: {hist[min(k, len(hist) - 1)]:.6e}, tolerance {tol:.6e})"


def check_pcg_fp32(n, fp64_too=True):
    """disp_solve(PREC_FDM) from zero and from a warm start (the reference's own converged iterate) against reference_pcg with the EXACT fp64 block inverse.
    fp32 mode: rc 0, the solution to 1e-9 (check_pcg's bound), the final residual below the tolerance, the iteration count within +-1 (the allowance the project
    gives its other non-bitwise mode).  fp64 mode on the same context: assert_same_count, as today."""
    P = box_problem(3, n, 2)
    G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
    out = []
    try:
        R = BoxReference(P)
        G.set(pk.VEC_P, REF["p_init"] * (1 + 0.3 * np.sin(0.37 * np.arange(G.n_p)))); G.disp_assemble_system(True)
        b = G.get(pk.VEC_RHS_U)
        x0 = np.zeros(G.n_u)
        for start in ("zero", "warm"):
            xr, its, hist, tol = reference_pcg(R.apply_A, R.block_inverse_u, b, x0, BENCH_TOL["abs_tol"], BENCH_TOL["rel_tol"], 200, 1, inert=R.mask)
            xr[R.dir_dof] = R.dir_val
            for mode in ((FP32, FP64) if fp64_too else (FP32,)):
                what = f"{n} Q2 from {start}, {'fp32' if mode == FP32 else 'fp64'} transforms"
                G.set_fdm_precision(mode)
                assert G.get_fdm_precision() == (mode, mode)
                G.set(pk.VEC_U, x0)
                rc, info = G.disp_solve(abs_tol=BENCH_TOL["abs_tol"], rel_tol=BENCH_TOL["rel_tol"], max_iter=200, prec=pk.PREC_FDM, reduction=BENCH_TOL["reduction"])
                e = rel(G.get(pk.VEC_U), xr)
                print(f"{what}: {info.iterations} iterations (reference {its}), final residual {info.final_residual:.3e} (tolerance {tol:.3e}), solution {e:.2e}")
                assert rc == 0, what
                if mode == FP32:
                    assert abs(info.iterations - its) <= 1, (what, info.iterations, its)
                else:
                    assert_same_count(info.iterations, its, hist, tol, what)
                assert info.final_residual <= tol, (what, info.final_residual, tol)
                assert e <= 1e-9, (what, e)
                out.append((start, mode, info.iterations, its))
            x0 = xr.copy()                  # warm start: the reference's converged iterate, the same vector for both modes
        return out
    finally:
        G.close(); P.close()


@pytest.mark.parametrize("n", PCG_SHAPES, ids=str)
def test_pcg_with_fp32_transforms_tracks_the_exact_preconditioner(n):
    check_pcg_fp32(n)


def test_pcg_with_fp32_transforms_and_the_separate_dot():
    """PORO_FDMO_SEPARATE_GZ=1: g . z by the separate fp64 dot kernel instead of pass 2's partial sums, same shapes, same rule"""
    run_child({"PORO_FDMO_SEPARATE_GZ": "1"}, "pcg")


# ---- 4. whole time steps -----------------------------------------------------------------------------------------------------------------------------
def test_time_steps_with_fp32_transforms_match_the_golden_trace_and_the_oracle():
    """3D Q2 4^3 box of tests/golden/box_traces.json, two steps through the host runner: the golden trace's fixed-stress and pressure iteration counts, and the
    tolerances of test_parity_gpu.py::test_transient_with_the_fast_solver_tracks_the_oracle against the oracle (|p|_inf rtol 1e-8, p 1e-9, u 1e-7 in the 2-norm)"""
    import oracle_py
    from common import host_material
    with open(os.path.join(GOLDEN, "box_traces.json")) as f:
        g = json.load(f)["3d_q2_4_reference"]
    P = box_problem(g["dim"], g["n"], g["degree"], mat=host_material())
    O = oracle_py.Oracle(P, hoisted=True)
    try:
        t0, _ = O.run(2, REF["p_init"], REF["dt"], max_it=5000)
        t1, G = pk.run_problem(P, 2, REF["p_init"], REF["dt"], operator_mode=pk.OP_MATRIX_FREE, max_it=5000, prec=pk.PREC_FDM, fdm_fp32=True)
        try:
            assert G.get_fdm_precision() == (FP32, FP32)
            rows = np.array(g["rows"])
            assert t1.shape[0] == rows.shape[0] and np.array_equal(t1[:, :3], rows[:, :3]), (t1[:, :3], rows[:, :3])
            assert np.allclose(t1[:, 4], t0[:, 4], rtol=1e-8)
            rel2 = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
            ep, eu = rel2(G.get(pk.VEC_P), O.get(pk.VEC_P)), rel2(G.get(pk.VEC_U), O.get(pk.VEC_U))
            print(f"fp32 transforms, 2 steps 4^3 Q2: |dp|/|p| = {ep:.2e}, |du|/|u| = {eu:.2e}, CG iterations per step {t1[1:, 6]}")
            assert ep <= 1e-9 and eu <= 1e-7, (ep, eu)
        finally:
            G.close()
    finally:
        O.close(); P.close()


def cli_trace(out):
    return (re.findall(r"Time: ([0-9.eE+-]+)", out), re.findall(r"Coupling iteration: (\d+)", out), [float(m) for m in re.findall(r"Solution limits: ([0-9.eE+-]+)", out)])


def test_poro_run_fdm_fp32_flag(tmp_path):
    """poro_run on a 3D 4^3 Q2 box (input.data with three dimensions and refinement level 2) --matrix-free --block-fdm, with and without --fdm-fp32: the same steps,
    the same fixed-stress iterations, |p|_inf per step to 1e-9 (the log prints 6 digits: the same digits).  The flag needs --block-fdm or --fastest."""
    text = open(os.path.join(GOLDEN, "input.data"), encoding="latin1").read()
    text = text.replace("set Dimensions               = 2", "set Dimensions               = 3").replace("set Domain size              = 10, 10", "set Domain size              = 10, 10, 10")
    text = text.replace("set Initial refinement level = 4", "set Initial refinement level = 2")
    text = text.replace("= 0, 1, 2, 3\n", "= 0, 1, 2, 3, 4, 5\n").replace("= 0, 0, 1, 1\n", "= 0, 0, 1, 1, 2, 2\n").replace("= 0, -1e-5, 0, -1e-5\n", "= 0, -1e-5, 0, -1e-5, 0, -1e-5\n")
    assert "= 3\n" in text and "0, 1, 2, 3, 4, 5" in text and "0, 0, 1, 1, 2, 2" in text and "level = 2" in text
    inp = tmp_path / "input3d.data"; inp.write_text(text, encoding="latin1")

    def run(*args):
        r = subprocess.run([EXE, str(inp), "--matrix-free", "--steps", "3", *args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return cli_trace(r.stdout)
    a, b = run("--block-fdm"), run("--block-fdm", "--fdm-fp32")
    assert len(a[0]) == 3 and a[0] == b[0] and a[1] == b[1]
    assert len(a[2]) == len(b[2]) >= 3 and all(abs(x - y) <= 1e-9 * abs(y) for x, y in zip(b[2], a[2])), (a[2], b[2])
    r = subprocess.run([EXE, str(inp), "--matrix-free", "--fdm-fp32"], capture_output=True, text=True)
    assert r.returncode == 1 and "--fdm-fp32 needs" in r.stderr


def _child(checks):
    if checks == "env":
        P = box_problem(3, (4, 4, 4), 2)
        G = pk.Context(P, 0, pk.OP_MATRIX_FREE)
        assert G.get_fdm_precision() == (FP32, FP32)                  # requested without any call; the octant form runs on this box
        G.close(); P.close()
    elif checks == "pcg":
        assert os.environ.get("PORO_FDMO_SEPARATE_GZ")
        for n in PCG_SHAPES:
            check_pcg_fp32(n, fp64_too=False)
    else:
        raise SystemExit(f"unknown check {checks}")
    print("child ok")


if __name__ == "__main__":
    _child(sys.argv[1])
